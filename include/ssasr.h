/* ssasr.h -- C ABI of libssasr_hip.so: the MI355X (gfx950) kernels behind the
 * ASR training hot path of cadia-lvl/ss_asr.
 *
 * The reference has no FFI layer: its "operator API" for this path is the
 * nn.Module surface of src/asr.py plus Solver.step() in src/trainer.py, and
 * all arithmetic is delegated to stock torch ops.  Each entry point below names
 * the reference lines whose arithmetic it replaces.  The Python host side
 * (ss_asr_amd/) binds these with ctypes; INTEGRATION.md shows the stub.
 *
 * Conventions (all entry points):
 *   - plain C symbols; every pointer is a DEVICE pointer unless it says host;
 *   - fp32 data, int32 lengths / character ids, int64_t sizes and strides
 *     (strides in ELEMENTS);
 *   - the caller owns every buffer, including workspaces and the events of
 *     ssasr_events_create; nothing is allocated, nothing synchronises, and no
 *     call leaves state behind for the next one: entry points are reentrant
 *     and may be called from several threads on different streams;
 *   - the only process-wide state is the table of diagnostic switches below
 *     (ssasr_set_option), read from the environment once and constant
 *     afterwards unless a tool changes it, plus a cache of occupancy-query
 *     results (a pure function of kernel and device);
 *   - work is enqueued on `stream` (a hipStream_t) by the calling thread;
 *   - return 0 on success, a negative value for an argument error, a positive
 *     hipError_t for a HIP failure.
 *
 * ABI history.  Added under 16 without changing anything older (the version number stays): ssasr_gemm_tile_choice; the encoder's
 * launch-form query -- ssasr_bilstm_forms; beam search --
 * ssasr_beam, ssasr_decode_beam_ws_bytes, ssasr_decode_beam; joint CTC / attention decoding -- ssasr_ctc_prefix,
 * ssasr_decode_beam_ctc_ws_bytes, ssasr_decode_beam_ctc; length bonus, coverage term and end detection in the beam
 * search -- ssasr_beam_terms, ssasr_decode_beam_ex_ws_bytes, ssasr_decode_beam_ex; a character graph in the beam search --
 * ssasr_decode_beam_graph_ws_bytes, ssasr_decode_beam_graph; SpecAugment in batch assembly and label smoothing in the
 * masked CE -- ssasr_specaug, ssasr_gather_batch_aug, ssasr_specaug_plan, ssasr_ce_loss_ls_fwd, ssasr_ce_loss_ls_bwd; CTC forced
 * alignment -- ssasr_ctc_align_ws_bytes, ssasr_ctc_align; CTC segmentation -- ssasr_ctc_segment_ws_bytes,
 * ssasr_ctc_segment_form, ssasr_ctc_segment, ssasr_ctc_segment_skip_ws_bytes, ssasr_ctc_segment_skip; CTC-only decoding -- ssasr_ctc_decode_ws_bytes, ssasr_ctc_decode; edit-distance scoring -- ssasr_edit_score; MWER training --
 * ssasr_mwer_ws_bytes, ssasr_mwer_loss_fwd, ssasr_mwer_loss_bwd, ssasr_mwer_pack, ssasr_rows_repeat_fwd, ssasr_rows_repeat_bwd; sampled
 * decoding -- ssasr_sample, ssasr_decode_sample_ws_bytes, ssasr_decode_sample, ssasr_mwer_loss_fwd_ex; minimum-Bayes-risk
 * selection -- ssasr_mbr_select.  16: CharLM training -- ssasr_charlm_train_ws_floats, ssasr_charlm_train_fwd, ssasr_charlm_train_bwd
 * (nothing older changed).  15: inference -- ssasr_charlm, ssasr_charlm_step, ssasr_infer, ssasr_decode_greedy (nothing
 * older changed).  14 and before: the training entry points below.
 *
 * Persistent launches.  Several entry points run a whole layer / decode loop as
 * ONE launch whose workgroups hand data to each other.  Such a grid is only
 * launched when an occupancy query says every workgroup of it can be resident
 * on the current device at once; otherwise the entry point takes its
 * one-launch-per-step form.  Hand-offs are bounded spins: a workgroup that
 * gives up sets the caller's status word (sync_ws[4] / ws_sync[5]) and the
 * launch drains (later waits of that launch return at once), so a caller must
 * check the status words before it trusts the results of that step.
 */
#ifndef SSASR_H
#define SSASR_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

int ssasr_abi_version(void);

/* Diagnostic switches (A/B measurements; every setting computes the same results).  Each is
 * initialised ONCE from the environment variable of the same name when the library is first
 * used -- entry points never read the environment -- and may be changed by tools between
 * calls.  Names: SSASR_NO_PERSISTENT, SSASR_NO_FUSED_INPUT, SSASR_BPTT_HALVES_OFF, SSASR_BPTT_RESERVE_KB,
 * SSASR_NO_PERSISTENT_DECODER, SSASR_NO_PERSISTENT_DECODER_BWD, SSASR_PERSIST_DELAY_FWD,
 * SSASR_PERSIST_DELAY_BWD, SSASR_GEMM_TILE (0 the launcher's cost model, 64 | 128 tile kernels, 256 the wide stream-K kernel,
 * 255 the wide kernel on whole tiles), SSASR_GEMM_WIDE (1; 0: the cost model never picks the wide kernel), SSASR_GEMM_X6, SSASR_GEMM_KCAT,
 * SSASR_GEMM_EPI (0; 1: the wide kernel's stores without their LDS staging, 2 | 3: direct | staged stores into the stream-K slabs instead of C),
 * SSASR_GEMM_TRACE_LO / _HI (set_option only: device address of a phase-stamp buffer, tools/gemm_trace.py), SSASR_WGRAD_FUSED, SSASR_BPTT_ONE_LAUNCH (1: a layer's BPTT ranges as one launch, the second stream released by in-kernel progress words), SSASR_NO_WINDOWS,
 * SSASR_LAST_SEG_PCT, SSASR_TAIL_INLINE, SSASR_NO_RESIDENCY_CHECK, SSASR_NO_TSAVE, SSASR_ATTN_RPH,
 * SSASR_TEST_DROP_TILE / SSASR_TEST_DROP_ATTN_SLICE / SSASR_TEST_DROP_DEC_SLICE (fault injection for the
 * time-out tests, one per kernel family, -1 = off).  Unknown name: -1.
 * The ONE switch that changes results: SSASR_GEMM_BF16 (0; 1 = the products of ssasr_gemm_f32 and of every GEMM the
 * library launches for the encoder -- input projections, input gradients, weight gradients -- take their operands
 * ROUNDED to bf16, one MFMA per block instead of six, fp32 accumulation, tile kernels only; tensors stay fp32, the
 * recurrences, the decode loop, the loss and the optimizer are untouched).  It is the bf16-storage variant of
 * BASELINE.json configs[1], not the reference's fp32 arithmetic (/root/reference/src/trainer.py:46-53 has no
 * autocast): 1.08-1.09 x the step rate, |d loss| < 4e-5 over 60 steps (bench.py "bf16_variant"). */
int ssasr_set_option(const char* name, int value);
int ssasr_get_option(const char* name, int* value);

/* A caller-owned set of events (and 64 progress words of device memory, allocated here) with which
 * ssasr_bilstm_bwd_overlapped orders its second stream behind the first.  One set serves all calls of its
 * owner (one thread at a time). */
int ssasr_events_create(void** handle);
int ssasr_events_destroy(void* handle);

/* C[b] = act(alpha * op(A[b]) . op(B[b]) + bias) + beta * C[b]; fp32 operands, fp32 accumulation on
 * the matrix cores (products as six bf16 MFMAs on the exact three-way operand split, or the fp32
 * MFMA instruction with SSASR_GEMM_X6=0: the same results to fp32 rounding).  Large products (>= 256 tiles of 256 x 128, 16-byte
 * aligned operands, K a multiple of 32) run as a stream-K grid whose cut tiles are finished through a workspace the LIBRARY allocates on
 * first use (4 x 64 MB, kept for the life of the process): the one buffer of this ABI that is not the caller's.  Each quarter belongs to the
 * first stream that launches such a product (launches of one stream follow each other; different streams never share a quarter); a fifth
 * stream's products take the tile kernels.  Same results either way.
 * ta = 0: A is [M][K] (ld = lda); ta = 1: A is [K][M].
 * tb = 0: B is [N][K] (torch Linear weight layout); tb = 1: B is [K][N].
 * act: 0 none, 1 tanh, 4 relu, 5 leaky relu (slope 0.01), 6 sigmoid.  splitk > 1 adds partial products atomically into a
 * caller-initialised C (beta is then ignored).
 * Replaces: torch.nn.Linear / torch.bmm call sites of src/asr.py:381,:385,:389
 * and the dense halves of nn.LSTM (src/asr.py:414,:262). */
int ssasr_gemm_f32(int ta, int tb, int64_t M, int64_t N, int64_t K, float alpha, const float* A,
                   int64_t lda, const float* B, int64_t ldb, float beta, float* C, int64_t ldc,
                   const float* bias, int act, int64_t batch, int64_t strideA, int64_t strideB,
                   int64_t strideC, int splitk, void* stream);

/* Which kernel family the launcher takes for a product of densely stored operands (lda = K or M, ldb = K or N, batch
 * strides M K and N K) under the current switches: 64 | 128 = the tile kernels with that block tile, 256 = the wide
 * kernel as a stream-K grid, 255 = the wide kernel on whole tiles (forced by SSASR_GEMM_TILE only); 0 for an empty
 * product, negative for an argument error.  kcat: K segments per product (0 | 1: none), aligned16: both operands start
 * on 16-byte boundaries.  A pure host function (no device needed): it labels a timing with the kernel that ran and
 * pins the decision table in a test.  A product chosen as 256 still takes the tile kernels on a fifth stream (above). */
int ssasr_gemm_tile_choice(int ta, int tb, int64_t M, int64_t N, int64_t K, int64_t batch, int splitk, int kcat,
                           int aligned16);

/* Bidirectional LSTM layer with packed-sequence semantics.
 * Logical input [S steps][N columns][I]: element (s, n, i) at
 * x[s * xs_s + n * xs_n + i].  A pBLSTM layer (batch-first [B, T, I]) passes
 * S = max(lens), N = B, xs_s = I, xs_n = T * I; blstm_4, which the reference
 * runs over the utterance axis (src/asr.py:237-238, :262), passes S = B,
 * N = T', lens = NULL.
 * lens: int32[N] or NULL; column n is live while s < lens[n]; dead positions
 * produce zeros in y (pad_packed_sequence, src/asr.py:417).
 * y element (s, n, d * H + u) at y[s * ys_s + n * ys_n + d * H + u].
 * Saved for backward: gates [2][S*N][4H], cs [2][S*N][H], hs [2][S*N][H].
 * Optional workspaces that enable the persistent recurrence (taken when H % 64 == 0: one launch per window of
 * 128 columns, i.e. a single launch up to N = 128): hx, ssasr_bilstm_fwd_hx_floats(S, N, H) floats of
 * exchange image (layout internal: [2][S][H/4][roundup(N,8)][4] floats), and sync_ws int32[8],
 * ZERO ON ENTRY (sync_ws[4] != 0
 * afterwards reports an exchange timeout); pass NULL for one launch per step.
 * armed != 0: hx already holds the fill pattern 0x7FC0DEAD in every word, written on the same
 * stream (a caller that arms the exchange workspaces of a whole pass with ONE fill: a dependent
 * launch costs ~6 us however small); 0: the call fills it itself.
 * tsave: optional, ssasr_bilstm_tsave_floats(S, N, H) floats (0: the shape has no use for it).
 * With it the activated gates and cell states that the backward pass streams back are saved
 * TILE-MAJOR there (5 KB contiguous per BPTT workgroup and step) instead of row-major in
 * gates / cs: `gates` then keeps the input projection (and receives the derivatives in backward),
 * cs is not touched and may be NULL.  The same pointer must be passed to the backward call.
 * Replaces: pBLSTM.forward / nn.LSTM, src/asr.py:406-427, :262. */
int64_t ssasr_bilstm_tsave_floats(int64_t S, int64_t N, int64_t H);
/* Which launch forms ssasr_bilstm_fwd and ssasr_bilstm_bwd take for column window `window` (0 .. ceil(N / 128) - 1) of
 * a layer under the current switches, given both sets of workspaces, contiguous 16-byte aligned buffers and all four
 * biases; answered by the decision functions the launches themselves call (occupancy answers are cached per kernel).
 * *fwd: 0 = one launch per step; 100 + c = the persistent recurrence, 200 + c = the persistent recurrence with the
 * fused input projection (I = 80, H = 256), c = 16 | 32 columns per workgroup in that window's launch.
 * *bwd, for a launch over the whole layer (iterations 0 .. S): 0 = one launch per step, 1 = the K-split persistent
 * BPTT, 2 = K-split with two workgroups per (unit tile, chunk) ("halves").  A forward that is persistent saves
 * tile-major exactly when ssasr_bilstm_tsave_floats is non-zero.  Returns 0, or negative for an argument error. */
int ssasr_bilstm_forms(int64_t S, int64_t N, int64_t I, int64_t H, int64_t window, int* fwd, int* bwd);
int64_t ssasr_bilstm_fwd_hx_floats(int64_t S, int64_t N, int64_t H);      /* 0: no persistent form for the shape */
int ssasr_bilstm_fwd(const float* x, int64_t xs_s, int64_t xs_n, int64_t S, int64_t N, int64_t I,
                     int64_t H, const int32_t* lens, const float* w_ih_f, const float* w_hh_f,
                     const float* b_ih_f, const float* b_hh_f, const float* w_ih_r,
                     const float* w_hh_r, const float* b_ih_r, const float* b_hh_r, float* y,
                     int64_t ys_s, int64_t ys_n, float* gates, float* cs, float* hs, float* hx,
                     int32_t* sync_ws, int armed, float* tsave, void* stream);

/* Backward of ssasr_bilstm_fwd.  `gates` is consumed (overwritten with the
 * gate pre-activation derivatives).  tsave: what the forward call was given (then cs may be NULL).  dx may be NULL.  db_* is the derivative
 * of b_ih and of b_hh alike.  Workspaces: ws_whhT [2][H][4H], ws_dc [2][2][N][H].
 * dw_ih_f == NULL defers every weight gradient to ssasr_bilstm_wgrad.
 * Optional, enabling the persistent BPTT (H in {64,128,256}; one launch per window of 128 columns): gx = ssasr_bilstm_bwd_gx_floats(S, N, H) floats of exchange
 * workspace (contents irrelevant on entry), sync_ws int32[8] zero on entry; NULL = one
 * launch per step. */
int64_t ssasr_bilstm_bwd_gx_floats(int64_t S, int64_t N, int64_t H);
/* Floats of the K-split BPTT's exchange ring alone (dirs = 1 or 2 directions), 0 when the
 * shape, the options or the device do not take that form.  A caller that arms several exchange
 * workspaces with one fill (`armed` below) reserves this instead of gx_floats.
 * armed != 0 (ssasr_bilstm_bwd, _overlapped): the first ssasr_bilstm_bwd_ring_floats(S, N, H, 2)
 * floats of gx already hold the fill pattern 0x7FC0DEAD, written on the same stream; only
 * meaningful when that query is non-zero. */
int64_t ssasr_bilstm_bwd_ring_floats(int64_t S, int64_t N, int64_t H, int64_t dirs);
int ssasr_bilstm_bwd(const float* dy, int64_t ys_s, int64_t ys_n, const float* x, int64_t xs_s,
                     int64_t xs_n, int64_t S, int64_t N, int64_t I, int64_t H, const int32_t* lens,
                     const float* w_ih_f, const float* w_hh_f, const float* w_ih_r,
                     const float* w_hh_r, float* gates, const float* cs, const float* hs, float* dx,
                     int64_t dxs_s, int64_t dxs_n, float* dw_ih_f, float* dw_hh_f, float* db_f,
                     float* dw_ih_r, float* dw_hh_r, float* db_r, float* ws_whhT, float* ws_dc,
                     float* gx, int32_t* sync_ws, int armed, const float* tsave, void* stream);

/* ssasr_bilstm_bwd with the weight gradients accumulated (+=) into dw_* / db* (db2_*: optional
 * second copy, b_ih and b_hh share theirs) on `side_stream`, overlapped with the recurrence:
 * for layers that take the persistent K-split BPTT, the recurrence is cut into `segments` (1..8)
 * consecutive step ranges and each range's weight-gradient products start on side_stream as soon
 * as the range is done -- the whole layer is ONE launch that counts its progress into words of the
 * events object, for which side_stream waits (hipStreamWaitValue32); where the device cannot do that,
 * or with SSASR_BPTT_ONE_LAUNCH=0, one launch per range with an event behind each.  The caller joins
 * side_stream before it reads the gradients.  events: from ssasr_events_create. */
int ssasr_bilstm_bwd_overlapped(const float* dy, int64_t ys_s, int64_t ys_n, const float* x, int64_t xs_s,
                                int64_t xs_n, int64_t S, int64_t N, int64_t I, int64_t H,
                                const int32_t* lens, const float* w_ih_f, const float* w_hh_f,
                                const float* w_ih_r, const float* w_hh_r, float* gates, const float* cs,
                                const float* hs, float* dx, int64_t dxs_s, int64_t dxs_n, float* dw_ih_f,
                                float* dw_hh_f, float* db_f, float* db2_f, float* dw_ih_r, float* dw_hh_r,
                                float* db_r, float* db2_r, float* ws_whhT, float* ws_dc, float* gx,
                                int32_t* sync_ws, int armed, const float* tsave, int segments, void* events,
                                void* stream, void* side_stream);

/* Weight gradients of a layer from the gate derivatives ssasr_bilstm_bwd left
 * in `gates`: dW_ih = dG^T X, dW_hh = sum_s dG[s]^T h[s_prev], db = column sums.
 * accumulate = 0 overwrites, 1 adds (e.g. straight into optimizer-zeroed
 * gradient buffers).  db2_* (optional) gets a second copy of the bias
 * gradient.  Not on the critical path of backward: may run on another stream.
 */
int ssasr_bilstm_wgrad(const float* dgates, const float* x, int64_t xs_s, int64_t xs_n,
                       const float* hs, int64_t S, int64_t N, int64_t I, int64_t H, float* dw_ih_f,
                       float* dw_hh_f, float* db_f, float* db2_f, float* dw_ih_r, float* dw_hh_r,
                       float* db_r, float* db2_r, int accumulate, void* stream);

/* One nn.LSTMCell step (src/asr.py:320-324); input given as column blocks
 * x1 | x2 (x2 may be NULL).  gates [N][4H] receives the activated i,f,g,o. */
int ssasr_lstm_cell_fwd(const float* x1, int64_t ldx1, int64_t k1, const float* x2, int64_t ldx2,
                        int64_t k2, const float* h_prev, const float* c_prev, const float* w_ih,
                        const float* w_hh, const float* b_ih, const float* b_hh, int64_t N,
                        int64_t H, float* gates, float* h_out, float* c_out, void* stream);

/* Gate derivatives of one cell step: dgates [N][4H], dc_prev [N][H]. */
int ssasr_lstm_cell_bwd(const float* dh, const float* dc, const float* gates, const float* c_prev,
                        const float* c, int64_t N, int64_t H, float* dgates, float* dc_prev,
                        void* stream);

/* comp = tanh(feat . W_psi^T + b_psi), the cached half of Attention.forward
 * (src/asr.py:381).  feat [rows][E], comp [rows][A]. */
int ssasr_attn_precompute_fwd(const float* feat, const float* w_psi, const float* b_psi,
                              int64_t rows, int64_t E, int64_t A, float* comp, void* stream);

/* Backward of the above.  dcomp is consumed (becomes the pre-tanh
 * derivative).  dfeat is ACCUMULATED into (beta = 1); dw_psi / db_psi are
 * overwritten. */
int ssasr_attn_precompute_bwd(float* dcomp, const float* comp, const float* feat,
                              const float* w_psi, int64_t rows, int64_t E, int64_t A, float* dfeat,
                              float* dw_psi, float* db_psi, void* stream);
/* The psi weight gradients alone, from the pre-activation derivative that
 * ssasr_attn_precompute_bwd left in dcomp: dW_psi (+)= dpre^T feat, db_psi (+)= column sums.
 * accumulate = 1 adds into the outputs (optimizer-owned gradient buffers, any stream). */
int ssasr_attn_precompute_wgrad(const float* dcomp, const float* feat, int64_t rows, int64_t E, int64_t A,
                                float* dw_psi, float* db_psi, int accumulate, void* stream);

/* One Attention.forward call after the cache exists (src/asr.py:383-390).
 * state [B][D], w_phi [A][D] (phi.weight), comp [B][T][A], feat [B][T][E],
 * enc_len int32[B] (NULL: every utterance has T frames; an entry above T acts as T).
 * Accepted: A % 4 == 0, E % 4 == 0, D % 4 == 0, T <= 16384, A <= 2048, E <= 8192, forward and
 * backward, every E among them included (the kernels' LDS limit is raised where a shape needs
 * more than 64 KB).  Two launches: q [B][A] = tanh(phi(state)) (small MFMA
 * kernel), then energies + masked softmax + context: att [B][T], ctx [B][E].
 * state == NULL skips the first launch and takes q as an input.
 * ws: optional workspace of ssasr_attn_step_ws_floats(B, T, A, E) floats that selects the
 * split-T form for long encoder outputs (T > 128 at A = 128, E = 512): frames of an utterance
 * spread over several workgroups (comp and feat are streamed exactly once, by >= 256 workgroups),
 * partial softmaxes exchanged through the workspace inside the launch.  The query returns 0 when
 * the shape, the options or the device (every workgroup of the grid must be resident at once) do
 * not take that form; then ws must be NULL.  With ws the split form is the only form: a NULL
 * ws_status, misaligned operands (16 bytes) or a shape whose query is 0 are argument errors, so
 * that what the caller believes about the workspace's phase is what was launched.
 * ws is two exchange buffers: a call uses buffer ws_phase & 1 and re-arms the other.
 * EVERY word of ws must hold the fill pattern 0x7FC0DEAD before the first call, and consecutive
 * calls on one workspace must alternate ws_phase (0, 1, 0, ...) and be ordered on one stream.
 * ws_status: int32[1], zero on entry (required with ws); non-zero after the stream has drained
 * means a hand-off of the launch timed out and att / ctx are not to be trusted (the word holds
 * 0x40000000 | 6 << 24 | workgroup << 12 | 0xfff). */
int64_t ssasr_attn_step_ws_floats(int64_t B, int64_t T, int64_t A, int64_t E);
int ssasr_attn_step_fwd(const float* state, const float* w_phi, const float* comp,
                        const float* feat, const int32_t* enc_len, int64_t B, int64_t T, int64_t A,
                        int64_t E, int64_t D, float* q, float* att, float* ctx, float* ws, int ws_phase,
                        int32_t* ws_status, void* stream);

/* Backward of one step given dctx [B][E] and datt [B][T] (may be NULL):
 * de [B][T] (derivative w.r.t. the masked energies) and dqpre [B][A]
 * (derivative w.r.t. phi's output before tanh). */
int ssasr_attn_step_bwd(const float* dctx, const float* datt, const float* att, const float* q,
                        const float* comp, const float* feat, const int32_t* enc_len, int64_t B,
                        int64_t T, int64_t A, int64_t E, float* de, float* dqpre, void* stream);

/* The fused decode loop of ASR.forward (src/asr.py:67-110): U steps of
 * attention -> Speller cell 1 -> cell 2 (-> char_trans + next-character choice
 * on steps that are not teacher forced), then char_trans for all steps. */
typedef struct ssasr_decoder {
  /* sizes */
  int64_t B, T, E, A, D, V, U;
  /* inputs */
  const float* feat;        /* [B][T][E] listener output                         */
  const float* comp;        /* [B][T][A] tanh(psi(feat))                         */
  const int32_t* enc_len;   /* [B]                                               */
  const int32_t* teacher;   /* [B][teacher_ld] character ids, or NULL            */
  int64_t teacher_ld;
  const int32_t* step_mode; /* HOST int32[U]: 0 teacher, 1 sample, 2 argmax      */
  const float* uniforms;    /* [U][B] uniforms for sampled steps, or NULL        */
  /* parameters (PyTorch layouts) */
  const float* w_phi;       /* [A][D]                                            */
  const float* w_ih1; const float* w_hh1; const float* b_ih1; const float* b_hh1; /* cell 1: I = D + E */
  const float* w_ih2; const float* w_hh2; const float* b_ih2; const float* b_hh2; /* cell 2: I = D     */
  const float* embed;       /* [V][D]                                            */
  const float* w_ct; const float* b_ct;   /* [V][D], [V]                         */
  /* outputs */
  float* logits;            /* [B][U][V]                                         */
  float* att;               /* [B][U][T]                                         */
  /* saved for backward / workspaces */
  float* w_phi_t;           /* [D][A]                                            */
  float* q;                 /* [U][B][A]                                         */
  float* ctx;               /* [U][B][E]                                         */
  float* emb_in;            /* [U+1][B][D] embedding fed to each step            */
  int32_t* chars;           /* [U+1][B]    character fed to each step            */
  float* gates1; float* c1; float* h1;   /* [U][B][4D], [U][B][D], [U][B][D]     */
  float* gates2; float* c2; float* h2;
  /* optional workspaces of the single-launch persistent loop (taken for
   * A = 128, E = 512, D = 256, B <= 32, T <= 128, V <= 64; all five non-NULL;
   * longer encoder outputs: see ws_part below) */
  float* ws_hx1; float* ws_hx2;          /* [U][D/4][32][4] each                 */
  float* ws_qx;                          /* [U][A/16][32][16]                    */
  int32_t* ws_modes;                     /* device int32[U]                      */
  int32_t* ws_sync;                      /* int32[8]; [5] != 0 reports a timeout */
  int32_t modes_ready;                   /* != 0: ws_modes already holds step_mode (the caller
                                          * uploaded it with its other per-step integers)   */
  int32_t ws_armed;                      /* != 0: ws_hx1, ws_hx2, ws_qx and ctx already hold the fill
                                          * pattern 0x7FC0DEAD (written on the same stream)  */
  float* ws_attn;                        /* optional: ssasr_attn_step_ws_floats(B, T, A, E) floats holding the fill
                                          * pattern 0x7FC0DEAD, for the per-step loop's attention (T > 128);
                                          * needs ws_sync (time-outs are reported in ws_sync[5])                */
  int32_t ws_attn_phase;                 /* phase of step 0 (step t uses ws_attn_phase + t): the buffer the
                                          * previous call on this workspace did NOT use last                */
  float* ws_part;                        /* optional: ssasr_decoder_fwd_part_floats(...) floats, every word the fill
                                          * pattern 0x7FC0DEAD on entry (covered by ws_armed like the images): with
                                          * ws_hx1, ws_hx2, ws_modes and ws_sync it enables the single-launch
                                          * persistent loop for LONG encoder outputs (128 < T <= 768, B * ceil(T / 64)
                                          * <= 192; ws_qx and ws_attn are not used by it)                      */
} ssasr_decoder;

/* Floats of the record ring of the long-encoder persistent decode loop for a shape; 0 when the
 * shape, the options or the device (all B * ceil(T / 64) + 64 workgroups of 512 threads resident at
 * once) do not take that form -- ssasr_decoder_fwd then runs one launch per stage and step. */
int64_t ssasr_decoder_fwd_part_floats(int64_t B, int64_t T, int64_t A, int64_t E, int64_t D, int64_t V);

int ssasr_decoder_fwd(const ssasr_decoder* d, void* stream);

typedef struct ssasr_decoder_grads {
  const float* dlogits;     /* [B][U][V]                                         */
  /* outputs (overwritten) */
  float* dfeat;             /* [B][T][E] through the context vectors             */
  float* dcomp;             /* [B][T][A]                                         */
  float* dw_phi;
  float* dw_ih1; float* dw_hh1; float* db1;   /* db = d b_ih = d b_hh            */
  float* dw_ih2; float* dw_hh2; float* db2;
  float* dembed; float* dw_ct; float* db_ct;
  /* workspaces */
  float* ws_t_ih1;          /* [D+E][4D] transposes of the cell weights          */
  float* ws_t_hh1;          /* [D][4D]                                           */
  float* ws_t_ih2;          /* [D][4D]                                           */
  float* ws_t_hh2;          /* [D][4D]                                           */
  float* ws_dh2;            /* [U][B][D]                                         */
  float* ws_dctx;           /* [U][B][E]                                         */
  float* ws_de;             /* [B][U][T]                                         */
  float* ws_dqpre;          /* [U][B][A]                                         */
  float* ws_dc;             /* [2][2][B][D]                                      */
  float* ws_demb;           /* [U][B][D]                                         */
  /* optional (both or neither): exchange ring + status words of the persistent
   * cell-2 BPTT, ssasr_bilstm_bwd_gx_floats(U, B, D) floats and int32[8]        */
  float* ws_gx;
  int32_t* ws_sync;
  /* optional (needs ws_gx / ws_sync too): ssasr_decoder_bwd_chain_floats(...) floats
   * for the persistent first-cell <-> attention backward chain                      */
  float* ws_chain;
  /* optional second copies of the bias gradients (b_ih and b_hh share theirs)        */
  float* db1_2; float* db2_2;
  /* != 0: ssasr_decoder_bwd leaves every parameter gradient (dw_*, db*, dembed) to
   * ssasr_decoder_wgrad, which may run later and on another stream                  */
  int32_t defer_wgrad;
  /* != 0: the ring at the head of ws_gx (ssasr_bilstm_bwd_ring_floats(U, B, D, 1) floats) and the
   * exchange part of ws_chain already hold the fill pattern 0x7FC0DEAD                       */
  int32_t ws_armed;
} ssasr_decoder_grads;

/* Workspace of the persistent decoder backward chain (0: shape has none). */
int64_t ssasr_decoder_bwd_chain_floats(int64_t U, int64_t B, int64_t T, int64_t A, int64_t E, int64_t D);

/* Backward of ssasr_decoder_fwd.  gates1 / gates2 of `d` are consumed. */
int ssasr_decoder_bwd(const ssasr_decoder* d, const ssasr_decoder_grads* g, void* stream);

/* Parameter gradients of the decode loop from what ssasr_decoder_bwd(defer_wgrad = 1)
 * left in d / g (gate derivatives, dqpre, dlogits): 11 products over all steps, off the
 * critical path of the backward pass.  accumulate = 0 overwrites the outputs, 1 adds. */
int ssasr_decoder_wgrad(const ssasr_decoder* d, const ssasr_decoder_grads* g, int accumulate,
                        void* stream);

/* Masked cross entropy of src/trainer.py:426-434 on the label matrix itself.
 * logits [B][U][V]; y int32 [B][y_cols] with row stride y_ld (0 = padding):
 * the label of step t is y[b][t + 1] (src/trainer.py:427, the <sos> column is
 * skipped) and a row's denominator is count(y[b][:] != 0) (src/trainer.py:431).
 * loss is one float; lse (B * U + 9 * B floats: log-sum-exp per step, then eight
 * partial sums per row, then the denominators) is saved for backward. */
int ssasr_ce_loss_fwd(const float* logits, const int32_t* y, int64_t y_ld, int64_t y_cols, int64_t B,
                      int64_t U, int64_t V, float* lse, float* loss, void* stream);
int ssasr_ce_loss_bwd(const float* logits, const int32_t* y, int64_t y_ld, const float* lse,
                      const float* dloss, int64_t B, int64_t U, int64_t V, float* dlogits, void* stream);

/* The same loss with label smoothing.  BUILD-DEFINED -- the reference's ASR loss has none (the BCE smoothing of
 * its ADVTrainer is the discriminator's and unrelated); the semantics are
 * torch.nn.functional.cross_entropy(..., label_smoothing=eps): the target is (1 - eps) on the label plus eps / V
 * on every one of the V classes, class 0 included, so a labelled step costs
 *   (1 - eps) (lse - z[lab]) + eps (lse - mean_v z[v]).
 * Labels, masking, denominators, the block-order mean and the layout of lse are ssasr_ce_loss_fwd's.  _bwd:
 * dlogits = (p - (1 - eps) [v == lab] - eps / V) dloss / (B denom[b]) on labelled steps, 0 elsewhere.
 * For eps > 0 the log-sum-exp and the gradient are formed in double and rounded once (lse holds the correctly
 * rounded value), so that a labelled step's dlogits sum to zero over V as closely as float storage allows.
 * 0 <= eps < 1, else an argument error; eps == 0 launches the kernels of the entries above (the same bits). */
int ssasr_ce_loss_ls_fwd(const float* logits, const int32_t* y, int64_t y_ld, int64_t y_cols, int64_t B,
                         int64_t U, int64_t V, float eps, float* lse, float* loss, void* stream);
int ssasr_ce_loss_ls_bwd(const float* logits, const int32_t* y, int64_t y_ld, const float* lse,
                         const float* dloss, int64_t B, int64_t U, int64_t V, float eps,
                         float* dlogits, void* stream);

/* CTC negative log likelihood over the Listener's frames: the auxiliary branch of
 * BASELINE.json configs[3] ("Joint CTC+attention loss").  BUILD-DEFINED -- the reference
 * has no CTC (its only loss is src/trainer.py:426-434), so this replaces no reference
 * interface; the semantics are torch.nn.functional.ctc_loss(log_softmax(logits), labels,
 * frame_lens, label_lens, blank, reduction='mean', zero_infinity=True).
 * logits [B][T][V] (log-softmax is taken inside); frame_lens / label_lens int32 [B];
 * label j of row b is y[b * y_ld + j] (pass y + 1 to skip the <sos> column of prepare_y's
 * matrix); Lmax >= every label length, 2 * Lmax + 1 <= 1024; blank is a class no label uses.
 * ws: ssasr_ctc_ws_floats(B, T, V, Lmax) floats, 8-byte aligned (alpha lattice and per-row
 * nll, held in double), written by _fwd and read by _bwd.  loss = mean_b(nll_b / max(label_len_b, 1)), rows with no
 * alignment counting 0.  frame_lens[b] > T is clamped to T; a row with label_lens[b] > Lmax or frame_lens[b] < 1
 * is treated as having no alignment (loss contribution 0, zero gradient), like one whose frames cannot hold its
 * labels.  _bwd writes dlogits [B][T][V] (zero past frame_lens) and, when
 * dbias is given, ADDS sum_{b,t} dlogits[b][t][:] to dbias [V]. */
int64_t ssasr_ctc_ws_floats(int64_t B, int64_t T, int64_t V, int64_t Lmax);
int ssasr_ctc_loss_fwd(const float* logits, const int32_t* frame_lens, const int32_t* y, int64_t y_ld,
                       const int32_t* label_lens, int64_t B, int64_t T, int64_t V, int64_t Lmax,
                       int blank, float* ws, float* loss, void* stream);
int ssasr_ctc_loss_bwd(const float* logits, const int32_t* frame_lens, const int32_t* y, int64_t y_ld,
                       const int32_t* label_lens, int64_t B, int64_t T, int64_t V, int64_t Lmax,
                       int blank, float* ws, const float* dloss, float* dlogits, float* dbias,
                       void* stream);

/* ---- CTC forced alignment (added under ABI 16) ------------------------------------------------------------------
 * BUILD-DEFINED: the reference has no CTC.  The most probable CTC path (Viterbi) of given labels through the frames
 * of the head that ssasr_ctc_loss_fwd trains: when each character was spoken, and how confident the head is of it.
 * logits [B][T][V] are the raw head outputs, as ssasr_ctc_loss_fwd takes them; frame_lens, y, y_ld, label_lens,
 * Lmax and blank are that entry's too.
 *   Lattice, per utterance: len = min(frame_lens[b], T), L = label_lens[b]; the extended sequence has S = 2 L + 1
 *   states, lab_s = blank at even s, label (s - 1) / 2 at odd s.  It is held in double and runs on the RAW logits,
 *   not on log-softmax values -- every path visits every frame exactly once, so the per-frame normaliser cannot
 *   change which path wins:
 *     d[0][s] = (double)logit[0][lab_s] for s < 2, -inf otherwise
 *     d[t][s] = best(d[t-1][s], d[t-1][s-1], d[t-1][s-2] if the skip is allowed) + (double)logit[t][lab_s]
 *   the skip being allowed as in the loss: s odd, s >= 3, lab_s != lab_{s-2}.
 *   Tie rule: the larger value wins; among equal values staying (s) wins over s - 1, which wins over s - 2; at the
 *   end s = S - 1 wins over S - 2 (S > 1).
 *   Exactness: each lattice value is ONE double add and comparisons, taken in frame order, so a float64 restatement
 *   that does the same operations gets the same bits, and the path is defined exactly -- tests compare it for
 *   equality, with no gap rule.  (A form of the kernel that reorders the sum or holds a float lattice is wrong.)
 *   Outputs: path[b][t] = the state 0 .. 2 L of frame t < len (character (s - 1) / 2 for odd s, blank for even s),
 *   -1 from len on; first[b][j] / last[b][j] = the first / last (inclusive) frame whose state is 2 j + 1, -1 for
 *   j >= L; char_logp[b][j] = sum over those frames of logit[t][y_j] - lse_t, 0 for j >= L; score[b] = d_end -
 *   sum_{t < len} lse_t, the log-probability of the path.  lse_t is the frame's log-sum-exp, (double)max +
 *   (double)logf(sum expf(x - max)) as the loss kernels' table computes it, accumulated in double.
 *   No alignment (len < 1, L < 0, L > Lmax, or len < L + the number of adjacent equal labels): score = -inf, the
 *   row's path, first and last are -1 and its char_logp 0.  Nothing is left unwritten.
 * Accepted: what ssasr_ctc_loss_fwd accepts (2 * Lmax + 1 <= 1024, V <= 1024, B <= 65535), 0 <= blank < V, ws
 * 8-byte aligned with ws_bytes >= ssasr_ctc_align_ws_bytes(...) (0: no kernel for the shape).  Lmax == 0 is legal:
 * first, last and char_logp may then be NULL.  Argument errors return before any HIP call.
 * One launch, one workgroup per utterance, one state per thread.  A step's back-pointers (two bits per state, packed
 * per 64 states) stay in LDS while T * ceil((2 * Lmax + 1) / 64) * 16 bytes <= 128 KB, i.e. for
 * T <= 8192 / ceil((2 * Lmax + 1) / 64) (integer division: 8192 frames up to Lmax 31, 819 at Lmax 300, 512 at Lmax
 * 511); from one frame more they go through the workspace.  Both forms give the same bits.  The workspace holds the
 * normalisers [B][T] (double), the back-pointers of the second form, and in its last 4 x B 64-bit words each
 * utterance's wall_clock64 at the start, before and after the traceback and at the end (tools/align_time.py). */
int64_t ssasr_ctc_align_ws_bytes(int64_t B, int64_t T, int64_t V, int64_t Lmax);
int ssasr_ctc_align(const float* logits, const int32_t* frame_lens, const int32_t* y, int64_t y_ld,
                    const int32_t* label_lens, int64_t B, int64_t T, int64_t V, int64_t Lmax, int blank,
                    void* ws, int64_t ws_bytes, int32_t* path, int32_t* first, int32_t* last,
                    float* char_logp, double* score, void* stream);

/* ---- CTC segmentation (added under ABI 16) -----------------------------------------------------------------------
 * BUILD-DEFINED: the reference has no CTC.  CTC segmentation (Kuerzinger et al. 2020) of a long recording with a
 * running transcript: where inside the recording the text was spoken, where each of its utterances starts and ends,
 * and how confident the head is of each.  It is ssasr_ctc_align's lattice with two differences: it runs on
 * NORMALISED values, and both of its ends are free.
 * logits [B][T][V], frame_lens, y, y_ld, label_lens, Lmax and blank are what ssasr_ctc_align takes; y holds the WHOLE
 * text of recording b, its utterances concatenated.  utt_ends int32 [B][utt_ld] holds, for utterance n < n_utts[b],
 * the exclusive end of its labels in y: strictly increasing, the first >= 1, the last == label_lens[b].
 *   Lattice, per recording: len = min(frame_lens[b], T), L = label_lens[b], S = 2 L + 1 states, lab_s and the skip
 *   rule as in ssasr_ctc_align.  It is held in double and runs on lp[t][v] = (double)logit[t][v] - lse_t, lse_t =
 *   (double)max + (double)logf(sum expf(x - max)) as ssasr_ctc_align forms it -- paths no longer visit the same
 *   frames, so the normaliser does change which path wins.  For every frame t < len and state s:
 *     d[t][s] = best(d[t-1][s], d[t-1][s-1], d[t-1][s-2] if the skip is allowed, 0 if s < 2) + lp[t][lab_s]
 *   with d[-1][.] = -inf.  The 0 is the free start: a path may begin at any frame, in state 0 or 1, and the frames
 *   before it are not scored.
 *   Tie rule: the larger value wins; among equal values staying (s) wins, then s - 1, then s - 2, then the start.
 *   Free end: score = max over t < len and s in {S - 1, S - 2} of d[t][s]; among equal values the earliest frame
 *   wins, then S - 1 over S - 2.  Frames after the end are not scored.
 *   Exactness: the lattice's operations are double adds and comparisons in frame order, as in ssasr_ctc_align, but
 *   lse_t is formed in float, and here it is not common to all paths: a float64 restatement on float64 log-softmax
 *   values agrees on the path only where its decisions are clear (tests compare the cases whose smallest margin on
 *   the returned path is >= 1e-3).
 *   Outputs: path[b][t] = the state of every scored frame, -1 for the frames before the start, after the end and
 *   from len on; first / last / char_logp [B][Lmax] as in ssasr_ctc_align (frames of the recording); score[b]
 *   (double) as above; utt_first[b][n] = first of utterance n's first label, utt_last[b][n] = last of its last
 *   label; utt_conf[b][n] (float) = Kuerzinger's min-mean: q_t = lp[t][lab(path[t])] over the frames utt_first ..
 *   utt_last, cut into consecutive blocks of `window` frames (the last may be shorter), each block's mean summed in
 *   double in frame order, the minimum over the blocks.  Slots n >= n_utts[b] get -1, -1 and 0.
 *   No segmentation (len < 1, L < 1, L > Lmax, n_utts[b] outside 1 .. Nmax, malformed utt_ends, or no finite end,
 *   i.e. len < L + the number of adjacent equal labels): score = -inf, every index -1, char_logp and utt_conf 0.
 *   Nothing is left unwritten.
 * Accepted: 1 <= Lmax, 2 * Lmax + 1 <= 16384, 1 <= T <= 32768, 2 <= V <= 1024, 1 <= B <= 65535, 1 <= Nmax <= Lmax,
 * window >= 1, 0 <= blank < V, y_ld >= Lmax, utt_ld >= Nmax, every pointer non-NULL, ws 8-byte aligned with ws_bytes
 * >= ssasr_ctc_segment_ws_bytes(...) (0: no kernel for the shape).  Argument errors return before any HIP call.
 * utt_ends lives on the device: the kernel checks it per recording and writes the no-segmentation outputs.
 * One launch, one workgroup per recording; a thread owns P consecutive states in registers.
 * ssasr_ctc_segment_form returns the launch form that serves (T, Lmax) -- 0 .. 6: 256 / 512 / 1024 threads x 1 state
 * up to 2 Lmax + 1 = 256 / 512 / 1024, 256 / 512 / 1024 threads x 8 states up to 2048 / 4096 / 8192, 1024 threads x 16
 * states up to 16384 -- and its threads and states per thread through the two pointers (either may be NULL); -1 when
 * no form does.  Every form gives the same bits.  The workspace holds the normalisers and the path's q_t [B][T]
 * (double each), the back-pointers (two bits per state and frame, 16 bytes per 64 states: 4 KB per frame and 128 MB
 * per recording at the limits), and in its last 4 x B 64-bit words each recording's wall_clock64 at the start, before
 * and after the traceback and at the end (tools/segment_time.py); four zeros for a recording without a segmentation. */
int64_t ssasr_ctc_segment_ws_bytes(int64_t B, int64_t T, int64_t V, int64_t Lmax, int64_t Nmax);
int ssasr_ctc_segment_form(int64_t T, int64_t Lmax, int* threads, int* states_per_thread);
int ssasr_ctc_segment(const float* logits, const int32_t* frame_lens, const int32_t* y, int64_t y_ld,
                      const int32_t* label_lens, const int32_t* utt_ends, int64_t utt_ld, const int32_t* n_utts,
                      int64_t B, int64_t T, int64_t V, int64_t Lmax, int64_t Nmax, int64_t window, int blank,
                      void* ws, int64_t ws_bytes, int32_t* path, int32_t* first, int32_t* last, float* char_logp,
                      double* score, int32_t* utt_first, int32_t* utt_last, float* utt_conf, void* stream);

/* ---- CTC segmentation with utterance skips and a filler (added under ABI 16) --------------------------------------
 * BUILD-DEFINED.  ssasr_ctc_segment for transcripts that are not verbatim: an utterance that was never spoken can be
 * passed over, and speech that nobody wrote down can be absorbed between two utterances.  Everything is
 * ssasr_ctc_segment's -- arguments, lattice, tie rule, free start (states 0 and 1), free end (S - 1 and S - 2),
 * outputs -- except what follows.  NOTE: skip_penalty and fill_penalty are the only HOST pointers among this entry's
 * device pointers.  They point to one double each in host memory, read before
 * the call returns (this ABI passes no double by value); each value is finite and <= 0, or -inf, which turns that
 * mechanism off; with both -inf every output that ssasr_ctc_segment writes is bit-equal to its.
 *   Junctions.  Recording b has N = n_utts[b] utterances; utterance n owns the labels [utt_ends[n-1], utt_ends[n])
 *   with utt_ends[-1] = 0.  The junction J_n is the blank state 2 * utt_ends[n-1]: J_0 = 0, J_N = S - 1, the others
 *   are the blanks between two utterances.
 *   Filler.  f_t = (double)(m + logf(sum_{v != blank} expf(x_v - m))) - lse_t, m the largest logit that is not the
 *   blank's and lse_t ssasr_ctc_segment's: the log-probability that frame t is some speech.  At a junction state,
 *   and only there, the frame's emission is max(lp[t][blank], f_t + fill_penalty); the blank wins a tie.
 *   Skip.  For n = 0 .. N - 1, J_{n+1} has one more predecessor: d[t-1][J_n] + skip_penalty -- the path passes over
 *   utterance n without visiting any of its labels.  The skip consumes the frame it lands on, scored with the
 *   junction's emission: m skipped utterances cost m frames and m penalties, there is no chain within a frame.  A
 *   blank state has no s - 2; the skip takes that place in the tie rule: stay, s - 1, skip, start.  The free ends
 *   stay where they are, so leading and trailing unspoken utterances are skipped through the chain and pay for it.
 *   An utterance is aligned whole or skipped whole.
 *   Outputs.  A skipped utterance has utt_first = utt_last = -1 and utt_conf = 0, its characters first = last = -1
 *   and char_logp = 0.  utt_skipped int32 [B][Nmax]: 1 skipped, 0 aligned, -1 for slots >= n_utts[b] and for a
 *   recording without a segmentation.  is_fill int32 [B][T]: 1 on a scored frame whose state is a junction and where
 *   the filler's value won (strictly), 0 on every other scored frame, -1 outside the span.  q_t of a junction frame
 *   is the junction's emission; no such frame lies inside an utterance's span.  No segmentation is: no finite end
 *   (with skips a recording may be shorter than its text), or ssasr_ctc_segment's other reasons.  Nothing is left
 *   unwritten.
 * Accepted: what ssasr_ctc_segment accepts, with Nmax <= 1024 (the junctions' values live in LDS: 2 x (Nmax + 3) doubles, J_0 .. J_Nmax and two spare slots),
 * both penalties <= 0 or -inf (a positive value, +inf or a NaN is an argument error), skip_penalty, fill_penalty,
 * utt_skipped and is_fill non-NULL, ws_bytes >= ssasr_ctc_segment_skip_ws_bytes(...): ssasr_ctc_segment's workspace and one more double per
 * frame, f_t, behind q_t.  Argument errors return before any HIP call.  The launch forms are ssasr_ctc_segment_form's. */
int64_t ssasr_ctc_segment_skip_ws_bytes(int64_t B, int64_t T, int64_t V, int64_t Lmax, int64_t Nmax);
int ssasr_ctc_segment_skip(const float* logits, const int32_t* frame_lens, const int32_t* y, int64_t y_ld,
                           const int32_t* label_lens, const int32_t* utt_ends, int64_t utt_ld, const int32_t* n_utts,
                           int64_t B, int64_t T, int64_t V, int64_t Lmax, int64_t Nmax, int64_t window, int blank,
                           const double* skip_penalty, const double* fill_penalty, void* ws, int64_t ws_bytes, int32_t* path,
                           int32_t* first, int32_t* last, float* char_logp, double* score, int32_t* utt_first,
                           int32_t* utt_last, float* utt_conf, int32_t* utt_skipped, int32_t* is_fill, void* stream);

/* ---- CTC-only decoding (added under ABI 16) ----------------------------------------------------------------------
 * BUILD-DEFINED: the reference has no CTC.  A transcript from the head's posteriors alone, with no Speller step: the
 * best path (K = 0) or a prefix beam search of width K (Graves 2012, 7.5.3; Hannun et al. 2014, alg. 1, without a
 * language model) over the frames of the head that ssasr_ctc_loss_fwd trains.  logits [B][T][V] are the raw head
 * outputs, frame_lens and blank as ssasr_ctc_align takes them.  Outputs, in the layout of ssasr_decode_beam's, with
 * Kr = max(K, 1): chars int32 [B][Kr][T], n_chars int32 [B][Kr], scores float [B][Kr], n_hyps int32 [B].  Every
 * element is written: slots from n_hyps on get length 0 and score -inf, characters from n_chars on are 0.
 *   len = min(frame_lens[b], T); lp[t][v] = (double)logit[t][v] - lse_t, lse_t = (double)max + (double)logf(sum
 *   expf(x - max)) as ssasr_ctc_align forms it.
 *   K = 0, best path: c_t = argmax_v logit[t][v], the lowest index among equal values; the text is c_0 .. c_{len-1}
 *   with repeats merged, then blanks removed; score = sum_t lp[t][c_t] accumulated in double; n_hyps = 1.  len < 1: the
 *   empty text, score 0.  Text and length are defined exactly (comparisons only): tests compare them for equality.
 *   K >= 1, prefix beam search, a search over TEXTS: a text occurs at most once in a beam however it was reached.
 *   Each member u of the beam B_t carries g_b(u) and g_n(u), the log-probabilities of the labellings of frames 0..t
 *   that collapse to u and end in a blank / a non-blank, restricted to labellings whose every earlier prefix was in
 *   its frame's beam.  B_{-1} = {empty: g_b = 0, g_n = -inf}.  Frame t: the candidates are every u in B_{t-1} and
 *   every u.c for non-blank c; with either(u) = logaddexp(g_b(u), g_n(u)), a candidate w with parent p (w minus its
 *   last character c) gets
 *     g_b'(w) = lp[t][blank] + either(w)                      if w in B_{t-1}, else -inf
 *     g_n'(w) = lp[t][c] + logaddexp(g_n(w) if w in B_{t-1},  (last(p) == c ? g_b(p) : either(p)) if p in B_{t-1})
 *   an absent term being -inf; the empty text has g_n' = -inf.  B_t is the min(K, number of finite candidates)
 *   candidates with the largest logaddexp(g_b', g_n') (among equal values: a kept text before an extension, then the
 *   lower slot, then the lower character).  After frame len - 1 the members are written best first, score = that
 *   value, n_hyps = their count (len < 1: the empty text alone, score 0).  g is held in double; exp and log run in
 *   float on differences from the larger operand.
 *   Identity of texts is established on the stored texts: each frame, a member's parent is looked up among the
 *   members by length and a 64-bit rolling hash as a filter, and then by comparing the characters.  An extension
 *   u.c that is itself a member is not a second candidate: its probability enters that member's g_n'.
 * Accepted: 1 <= B <= 65535, 1 <= T <= 4096 (the frame loop is serial and each member's text is copied once per frame:
 * the limit keeps a launch to tens of milliseconds), 0 <= K <= 32, 2 <= V <= 64 for K >= 1 (the lp[T][64] width of
 * ssasr_decode_beam_ctc) and V <= 1024 for K = 0, 0 <= blank < V, ws 8-byte aligned with ws_bytes >=
 * ssasr_ctc_decode_ws_bytes(...) (0: no kernel for the shape).  Argument errors return before any HIP call.
 * One launch of 256 threads per utterance, no exchange between workgroups, no spins; every loop is bounded by len, K,
 * V or T.  LDS holds the beam's scalars and ONE frame's candidates (K + K V totals, 17 KB at the limits); the texts
 * of the two beams B_{t-1} and B_t, [B][2][K][T] int32, live in the workspace (K = 0: the frame labels, [B][T]). */
int64_t ssasr_ctc_decode_ws_bytes(int64_t B, int64_t T, int64_t V, int64_t K);
int ssasr_ctc_decode(const float* logits, const int32_t* frame_lens, int64_t B, int64_t T, int64_t V, int64_t K,
                     int blank, void* ws, int64_t ws_bytes, int32_t* chars, int32_t* n_chars, float* scores,
                     int32_t* n_hyps, void* stream);

/* ---- Edit-distance scoring (added under ABI 16) -----------------------------------------------------------------
 * BUILD-DEFINED: the reference scores on the host (its calc_err).  Character and word error counts of P
 * (hypothesis, reference) pairs in ONE launch, one workgroup per pair: what CER, WER and an n-best list's oracle
 * error rate are sums of.
 *   Sequences: pair p reads hyp[p * hyp_ld + 0 .. min(hyp_lens[p], Hmax)) and, with r = ref_of[p] (p when ref_of is
 *   NULL, so that K hypotheses can share one row), ref[r * ref_ld + 0 .. min(ref_lens[r], Rmax)); negative lengths
 *   count as 0.  Every id < first_char is dropped first (with the Mapper first_char = 2: `<`, which is also the pad,
 *   and `>` go, `$` stays).  Words are the maximal runs of tokens != space (str.split(): no empty words, an empty
 *   sequence has none); two words are equal when their tokens are.
 *   Metric: an alignment of the hypothesis against the reference costs (S + D + I, S); the result is the
 *   lexicographic minimum over all alignments -- fewest edits, among those fewest substitutions:
 *     cell(i, j) = min(cell(i-1, j-1) + (ne, ne), cell(i-1, j) + (1, 0), cell(i, j-1) + (1, 0))
 *   with cell(i, 0) = (i, 0), cell(0, j) = (j, 0), i over the hypothesis, j over the reference.  With I - D = H - R
 *   and S + D + I = dist the counts are unique: no traceback, no dependence on a traversal order, so a host
 *   restatement (postprocess.edit_ops) is matched exactly.  Reference `ab` against hypothesis `ba` scores S = 0,
 *   D = 1, I = 1, not S = 2.
 *   out [P][8] = character S, D, I and the reference's character count, then word S, D, I and the reference's
 *   word count, all after dropping.
 * Accepted: 0 <= P <= INT32_MAX (P == 0 launches nothing), 0 <= Rmax <= 1023, 0 <= Hmax <= 8191 (both counted
 * before dropping), hyp_ld >= Hmax, ref_ld >= Rmax, non-NULL hyp_lens, ref_lens, out, hyp (unless Hmax == 0) and ref
 * (unless Rmax == 0).  Argument errors return before any HIP call.  ref_of's entries are not checked: the caller
 * keeps them inside ref's rows.
 * The block has 64 * ceil((Rmax + 1) / 64) threads, one per reference column; the dynamic LDS holds the kept
 * tokens, the word boundaries and the word ids (at most 63 KB). */
int ssasr_edit_score(const int32_t* hyp, int64_t hyp_ld, const int32_t* hyp_lens,
                     const int32_t* ref, int64_t ref_ld, const int32_t* ref_lens,
                     const int32_t* ref_of, int64_t P, int64_t Hmax, int64_t Rmax,
                     int32_t first_char, int32_t space, int32_t* out, void* stream);

/* ---- Minimum-Bayes-risk selection (added under ABI 16) -----------------------------------------------------------
 * BUILD-DEFINED: the reference has no n-best list to choose from.  Of the K hypotheses that a decode left for each of
 * N utterances (ssasr_decode_beam's or ssasr_decode_sample's chars, n_chars, n_hyps and hyp_scores), the one with the
 * lowest EXPECTED error count under the list's own posterior (Goel & Byrne 2000; Prabhavalkar et al. 2018, 3), in
 * ONE launch, one workgroup per utterance: the pairwise distances, the posterior, the risks and the choice.
 *   Sequences: hypothesis (n, k) is chars[(n * K + k) * hyp_ld + 0 .. clamp(n_chars[n][k], 0, Hmax)).  Its tokens and
 *   words are exactly ssasr_edit_score's: ids < first_char are dropped, words are the maximal runs of tokens !=
 *   space.  The set S_n is the rows k < clamp(n_hyps[n], 0, K).
 *   Distances: for j, k in S_n, pair[n][k][j][0] is the character S + D + I of hypothesis k against hypothesis j as
 *   the reference and pair[n][k][j][1] the same over words -- the first component of ssasr_edit_score's lexicographic
 *   minimum (S + D + I, S).  It is symmetric with a zero diagonal; each unordered pair's DP runs once and is written
 *   twice.  Entries with j or k outside S_n are -1.
 *   Posterior: posterior 1: p_j = 1 / |S_n|.  posterior 0: with x_j = (double)scale * (double)scores[n][j],
 *   p_j = exp(x_j - LSE_i x_i) over the finite x of the set, in double, LSE = m + log(sum_i exp(x_i - m)) with the
 *   maximum m subtracted first; a non-finite x_j gets p_j = 0; if no x of the set is finite the posterior is the
 *   uniform one.  scores may be NULL when posterior == 1.
 *   Risk and choice: risk[n][k] = sum_{j in S_n} p_j * pair[n][k][j][unit] (unit 0: characters, 1: words), products
 *   and sums in double, each rounded on its own (no fused multiply-add), in the order j = 0 .. K - 1, rounded once to
 *   float; rows outside S_n get +inf.  best[n] is the lowest k in S_n whose double risk is minimal, -1 for an empty
 *   set.  Every element of best, risk and pair is written; no atomics; nothing depends on scheduling.
 * Accepted: 0 <= N <= 65535 (N == 0 launches nothing), 1 <= K <= 32, 0 <= Hmax <= 1023 (both sides of a pair are DP
 * columns), K * Hmax <= 8192 (an utterance's kept tokens: 32 KB of LDS; its word tables stay under 25 KB), hyp_ld >=
 * Hmax, unit and posterior in {0, 1}, a finite scale >= 0, non-NULL n_chars, n_hyps, best, risk, pair, chars (unless
 * Hmax == 0) and scores (unless posterior == 1).  Argument errors return before any HIP call.
 * The block has 64 * max(ceil((Hmax + 1) / 64), min(K (K - 1) / 2, 16)) threads (at least 64): a wave per hypothesis
 * compacts it and finds its words once, a thread per word numbers it over all of the utterance's words, groups of
 * ceil((L + 1) / 64) waves (L: the utterance's longest kept sequence) take the pairs round-robin, and a lane per
 * candidate forms posterior, risk and argmin. */
int ssasr_mbr_select(const int32_t* chars, int64_t hyp_ld, const int32_t* n_chars, const int32_t* n_hyps,
                     const float* scores, int64_t N, int64_t K, int64_t Hmax, int32_t first_char, int32_t space,
                     int unit, int posterior, float scale, int32_t* best, float* risk, int32_t* pair,
                     void* stream);

/* ---- MWER training (added under ABI 16) ------------------------------------------------------------------------
 * BUILD-DEFINED: the reference trains on the masked CE alone.  Minimum word error rate training (Prabhavalkar et al.
 * 2018) minimises the expected number of errors over an n-best list, interpolated with CE.  The loss works on GROUPS
 * of teacher-forced rows: logits [R][U][V] with R = G * M, row r = g * M + k being candidate k of group (utterance) g.
 *   y int32 [R][y_cols], row stride y_ld: labels and masking are ssasr_ce_loss_fwd's -- the label of step t is
 *   y[r][t + 1], 0 is unlabelled, columns past y_cols read as 0.  An id outside 1 .. V - 1 counts as unlabelled too
 *   (nothing is read out of bounds).
 *   n_hyps int32 [G]: the set S_g is the rows k < clamp(n_hyps[g], 0, M).
 *   counts int32 [R][8]: ssasr_edit_score's out.  unit 0: characters, 1: words; risk_r = S + D + I of that unit.
 *   ce_w float [R] or NULL (all 0): the ABSOLUTE weight of the row's plain negative log-likelihood; the caller
 *   folds any 1 / (B denominator) into it.
 * Definition, every sequence-level quantity in double:
 *   logP_r  = sum over labelled t of (z[t][lab] - lse_t),  lse_t = (double)max + log(sum exp((double)z - max))
 *   p_k     = exp(logP_k - LSE_{j in S_g} logP_j) for k in S_g (the maximum is subtracted first: logP values 1e3
 *             apart give a one-hot p, never a NaN), 0 outside S_g
 *   Rbar_g  = sum_{k in S_g} p_k risk_k   (an empty S_g: 0)
 *   loss    = (1 / G) sum_g Rbar_g + sum_r ce_w[r] (-logP_r)   -- summed in a fixed order, no atomics
 *   _bwd:   dlogits[r][t][v] = dloss w_r (softmax(z[t])_v - [v == lab]) on labelled steps, 0 on unlabelled ones, with
 *           the row's sequence-level weight w_r = ce_w[r] - (1 / G) p_r (risk_r - Rbar_g); formed in double and
 *           rounded once.  Nothing is left unwritten.
 * ws: ssasr_mwer_ws_bytes(G, M, U) bytes, 8-byte aligned, written by _fwd and read by _bwd: doubles logP [R], p [R],
 * w [R], Rbar [G], then G + 8 R doubles of scratch and the log-sum-exp [R][U] in double (what _bwd normalises by, so
 * that a step's dlogits sum to zero as closely as float storage allows), then lse [R][U] as float (the correctly
 * rounded value).  _fwd also writes risk_out float [G] (= Rbar_g) and loss (one float).
 * Accepted: V > 0, U > 0, 1 <= M <= 33, G * M <= 65535, unit 0 | 1, y_cols >= U + 1, y_ld >= y_cols, ws as above
 * (ssasr_mwer_ws_bytes returns 0 for sizes outside these).  G == 0 launches nothing; _fwd then writes loss = 0 and
 * needs neither ws nor the inputs.  Argument errors return before any HIP call.
 * _fwd: grid (R, 8) x 256 threads, a wave per step, the step's logits held in registers (read once for V <= 256),
 * then ONE block of 256 threads, a wave per group and a lane per candidate.  _bwd: a wave per (r, t) step. */
int64_t ssasr_mwer_ws_bytes(int64_t G, int64_t M, int64_t U);
int ssasr_mwer_loss_fwd(const float* logits, const int32_t* y, int64_t y_ld, int64_t y_cols,
                        const int32_t* n_hyps, const int32_t* counts, int unit, const float* ce_w,
                        int64_t G, int64_t M, int64_t U, int64_t V, void* ws, int64_t ws_bytes,
                        float* risk_out, float* loss, void* stream);
int ssasr_mwer_loss_bwd(const float* logits, const int32_t* y, int64_t y_ld, int64_t y_cols, int64_t G,
                        int64_t M, int64_t U, int64_t V, const void* ws, int64_t ws_bytes,
                        const float* dloss, float* dlogits, void* stream);

/* ssasr_mwer_loss_fwd with a choice of posterior (added under ABI 16).  posterior 0: the definition above -- the same
 * kernels, the same bits.  posterior 1, the Monte-Carlo form for a set of SAMPLES drawn from the model's own
 * distribution (ssasr_decode_sample at temperature 1, no LM): p_k = 1 / |S_g| for k in S_g and 0 outside, whatever
 * logP is, so Rbar_g is the plain mean risk of the set and the row weight
 *   w_r = ce_w[r] - (1 / G) (1 / |S_g|) (risk_r - Rbar_g)
 * is the score-function (REINFORCE) estimator of the gradient of E[risk] with the set's mean risk as the baseline
 * (Shannon 2017; Prabhavalkar et al. 2018, 3.1).  The baseline INCLUDES the row itself: the estimate is the unbiased
 * leave-one-out one scaled by (|S| - 1) / |S|, and a set of ONE sample gets no risk gradient at all (its weight is
 * ce_w alone).  Duplicate samples are legitimate draws and stay in the set.  logP, the workspace layout, risk_out and
 * loss keep their meaning (loss = (1 / G) sum_g Rbar_g + the CE terms: its VALUE does not depend on logP through the
 * risk, the gradient is carried by w); ssasr_mwer_loss_bwd is unchanged, it reads w from the workspace.  Any other
 * posterior is an argument error. */
int ssasr_mwer_loss_fwd_ex(const float* logits, const int32_t* y, int64_t y_ld, int64_t y_cols,
                           const int32_t* n_hyps, const int32_t* counts, int unit, const float* ce_w,
                           int64_t G, int64_t M, int64_t U, int64_t V, void* ws, int64_t ws_bytes,
                           float* risk_out, float* loss, int posterior, void* stream);

/* The teacher / label matrix of an MWER step from device-resident results: ssasr_decode_beam's chars [N][K][steps],
 * n_chars [N][K] and n_hyps [N], and the batch's label matrix y_ref [N][ref_cols] (row stride ref_ld; <sos> column
 * first, 0-padded).  rows int32 [N * (K + 1)][L], every element written:
 *   row (n, k < K), k < clamp(n_hyps[n], 0, K):  0, chars[n][k][0 .. len), eos, 0 ...  with len = clamp(n_chars[n][k],
 *                                                 0, steps); eos is always appended, as references are formed
 *   row (n, k < K) from that clamp on:            all 0
 *   row (n, K):                                   y_ref[n][0 .. ref_cols), then 0
 * hyp_lens int32 [N * (K + 1)]: len for a hypothesis row (0 for an unused one); for a reference row the count of
 * non-zero ids minus one, the <eos>.  Column 1 onwards of `rows` with these lengths is what ssasr_edit_score takes
 * for hypotheses and references alike.
 * Accepted: N >= 0 (0 launches nothing), 1 <= K <= 32, steps >= 1, ref_ld >= ref_cols >= 0, L >= steps + 2 and
 * L >= ref_cols.  Argument errors return before any HIP call.  One block of 64 threads per row. */
int ssasr_mwer_pack(const int32_t* chars, const int32_t* n_chars, const int32_t* n_hyps, const int32_t* y_ref,
                    int64_t ref_ld, int64_t ref_cols, int64_t N, int64_t K, int64_t steps, int32_t eos, int64_t L,
                    int32_t* rows, int32_t* hyp_lens, void* stream);

/* Row repeat: one encoder output serves the M rows of its group.  _fwd: dst[g * M + k][0 .. n) = src[g][0 .. n), a
 * bit copy of 32-bit words (float or int32).  _bwd: dsrc[g][i] = sum_k ddst[g * M + k][i], added in float in the order
 * k = 0 .. M - 1 by the output's one owner thread: deterministic, no atomics.
 * Accepted: 0 <= G <= 65535 (0 launches nothing), 1 <= M <= 65535, n > 0, pointers 4-byte aligned.  Argument errors
 * return before any HIP call.  grid (ceil(n / 1024), G) x 256 threads, four words per thread (128-bit accesses when
 * n % 4 == 0 and both pointers are 16-byte aligned). */
int ssasr_rows_repeat_fwd(const void* src, int64_t G, int64_t M, int64_t n, void* dst, void* stream);
int ssasr_rows_repeat_bwd(const float* ddst, int64_t G, int64_t M, int64_t n, float* dsrc, void* stream);

/* ---- n-best rescoring (added under ABI 16) -----------------------------------------------------------------------
 * BUILD-DEFINED: the reference has no n-best list.  The second pass of two-pass decoding: the K texts that a first
 * pass left for each of G utterances (ssasr_ctc_decode's, ssasr_decode_beam's or ssasr_decode_sample's chars, n_chars,
 * n_hyps and scores) are teacher-forced through the Speller (and the CharLM) by the caller, and ONE launch, one
 * workgroup per utterance, scores every text under those logits, forms the weighted total, ranks the list and writes
 * it out in rank order.
 *   logits float [R][U][V], R = G * M, row r = g * M + k being candidate k of group g: ssasr_mwer_loss_fwd's layout
 *   (ssasr_mwer_pack with ref_cols = 0 gives M = K + 1, the group's last row idle).
 *   lm_logits float or NULL (no LM term): step t of row r starts at lm_logits + r * lm_row_stride + t *
 *   lm_step_stride, its V entries at unit stride ([U][R][V] as ssasr_charlm_train_fwd leaves them: strides V and R V).
 *   y int32 [R][y_cols], row stride y_ld: labels and masking are ssasr_mwer_loss_fwd's -- the label of step t is
 *   y[r][t + 1]; 0, an id outside 1 .. V - 1 and a column past y_cols are unlabelled; nothing is read out of bounds.
 *   n_hyps int32 [G]: the candidates of group g are the rows k < n_g = clamp(n_hyps[g], 0, K), K <= M.
 *   first float [G][K]: the first pass's scores.  chars int32 [G][K][steps], n_chars int32 [G][K]: the list.
 * Definition, every sequence-level quantity in double:
 *   att_k   = sum over labelled t of (z[t][lab] - lse_t): the logP_r of the MWER section above, formed by the same
 *             device function (csrc/seq_logp.h), the steps added in ascending t
 *   lm_k    = the same sum over lm_logits; 0 when lm_logits is NULL
 *   len_k   = clamp(n_chars[g][k], 0, steps)
 *   total_k = att_weight att_k + lm_weight lm_k + first_weight first_k + length_bonus len_k: each product rounded on
 *             its own (no fused multiply-add), added in this order, rounded ONCE to float.  A term whose weight is
 *             exactly 0 is left out, not multiplied: a -inf or NaN first-pass score does not poison the total when
 *             first_weight == 0.
 *   rank:     non-increasing float total, equal totals in input-slot order, a NaN total counting as -inf (it is
 *             written as it is): rank(k) = #{j < n_g: total_j > total_k or (total_j == total_k and j < k)}.
 * Outputs, every element written; none may overlap an input:
 *   order int32 [G][K]: the input slot at each rank.  total float [G][K] and parts float [G][K][3] = (att, lm, first),
 *   each rounded once, in rank order.  chars_out [G][K][steps], n_chars_out [G][K] (= len), n_hyps_out [G] (= n_g): the
 *   list in rank order, in the layout of the inputs; characters from a text's length on are 0.
 *   Ranks from n_g on: order -1, length 0, characters 0, parts 0 and total 0 -- what ssasr_decode_beam leaves in the
 *   slots it does not use (ssasr_ctc_decode leaves -inf there; readers go by n_hyps).
 * An utterance's results depend on its own rows alone: the same bits in any group, with or without the workspace.
 * Accepted: V > 0, U > 0, 1 <= K <= M <= 33, K <= 32, G * M <= 65535, y_cols >= U + 1, y_ld >= y_cols, steps >= 1,
 * lm strides >= V, finite weights, ws 8-byte aligned with ws_bytes >= ssasr_rescore_ws_bytes(G, K, U) when that is
 * > 0.  G == 0 launches nothing.  Argument errors return a negative code before any HIP call.
 * 256 threads per utterance: a wave per (k, t) step of the candidates, strided, the step's logits in registers as in
 * ssasr_mwer_loss_fwd (V <= 256 is read once; V <= 64 is one value per lane); the per-step terms (2 K U doubles) wait
 * in LDS when they fit 32 KB, else in the utterance's slice of ws; then a lane per candidate adds its terms, the first
 * wave ranks by counting, and all waves copy the texts.  No exchange between workgroups, no spins, no atomics; every
 * loop is bounded by K, U, V or steps. */
/* Bytes of `ws`: 0 when LDS holds the terms (2 K U <= 4096), else 16 G K U; -1 for sizes that are not accepted. */
int64_t ssasr_rescore_ws_bytes(int64_t G, int64_t K, int64_t U);
int ssasr_rescore(const float* logits, const float* lm_logits, int64_t lm_row_stride, int64_t lm_step_stride,
                  const int32_t* y, int64_t y_ld, int64_t y_cols, const int32_t* n_hyps, const float* first,
                  const int32_t* chars, const int32_t* n_chars, int64_t G, int64_t M, int64_t K, int64_t U, int64_t V,
                  int64_t steps, float att_weight, float lm_weight, float first_weight, float length_bonus,
                  void* ws, int64_t ws_bytes, int32_t* order, float* total, float* parts, int32_t* chars_out,
                  int32_t* n_chars_out, int32_t* n_hyps_out, void* stream);

/* Solver.step (src/trainer.py:131-148) with torch.optim.Adadelta
 * (src/trainer.py:401-403) on flat buffers of n floats: total L2 norm of
 * grad * grad_scale, NaN guard, clip to max_norm, Adadelta update.
 * stats: float[2] = {grad_norm, skipped (1 if the norm was NaN)}.
 * ws: float[1 + blocks] scratch, blocks = ssasr_clip_adadelta_ws(n) - 1.
 * zero_grad != 0 leaves grad zeroed (the next step's optimizer.zero_grad(),
 * src/trainer.py:419, without a pass of its own). */
int64_t ssasr_clip_adadelta_ws(int64_t n);
int ssasr_clip_adadelta(float* param, const float* grad, float* square_avg, float* acc_delta,
                        int64_t n, float grad_scale, float max_norm, float lr, float rho,
                        float eps, float* ws, float* stats, int zero_grad, void* stream);

/* Solver.step with torch.optim.Adam as TAETrainer uses them (src/trainer.py:633-641: ONE Adam over the text
 * autoencoder's parameters and the ASR model's embed / attention / decoder / char_trans; :676
 * `self.step(self.text_autoenc.parameters(), self.optim)`: the norm that is clipped and tested for NaN
 * is the text autoencoder's alone).  Parameters may therefore live in several flat buffers:
 *   ssasr_adam_prepare  once per step, over the CLIPPED gradient range grad_clip[0 .. n_clip): L2 norm of
 *     grad * grad_scale, NaN guard, clip coefficient; unless the step is skipped, advances the step count
 *     state[0] (float[1], persistent, zero before the first step) and forms Adam's bias corrections.
 *     ws: float[ssasr_adam_ws(n_clip)] scratch, read by the updates; stats: float[2] = {norm, skipped}.
 *   ssasr_adam_update   per flat buffer: the Adam update (amsgrad off, no weight decay) of n values;
 *     clipped != 0 multiplies the gradient by the clip coefficient * grad_scale (the clipped range),
 *     else by grad_scale alone.  A skipped step changes nothing (optim.step() is not called for it).
 *     zero_grad != 0 leaves grad zeroed, as for ssasr_clip_adadelta. */
int64_t ssasr_adam_ws(int64_t n_clip);
int ssasr_adam_prepare(const float* grad_clip, int64_t n_clip, float grad_scale, float max_norm, float lr,
                       float beta1, float beta2, float* state, float* ws, float* stats, void* stream);
int ssasr_adam_update(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                      const float* ws, int clipped, float grad_scale, float beta1, float beta2, float eps,
                      const float* stats, int zero_grad, void* stream);

/* ---- the Seed loop's other legs (BASELINE.json configs[4]): ADVTrainer, SAETrainer ------------------------
 * Dense layer with its activation, y = act(x . W^T + b): x [rows][K] (row stride ldx), W [N][K] (nn.Linear),
 * y [rows][N]; act as for ssasr_gemm_f32 (0, 1, 4, 5, 6).
 * Replaces: the nn.Sequential cores of src/discriminator.py:38-43 (+ :52 sigmoid) and
 * src/speech_autoencoder.py:183-188.
 * ssasr_linear_bwd: dy [rows][N] is the gradient of y and is OVERWRITTEN with dz = dy * act'(y) (y: the saved
 * output; unused for act 0); dx (optional) = dz . W, row stride lddx; dw (optional) += dz^T . x; db (optional)
 * += column sums of dz.  Partial products of dw are added atomically (K slices over the rows). */
int ssasr_linear_fwd(const float* x, int64_t ldx, const float* w, const float* b, float* y, int64_t rows,
                     int64_t K, int64_t N, int act, void* stream);
int ssasr_linear_bwd(float* dy, const float* y, const float* x, int64_t ldx, const float* w, float* dx,
                     int64_t lddx, float* dw, float* db, int64_t rows, int64_t K, int64_t N, int act,
                     void* stream);
/* dx[i] = dy[i] * act'(y[i]) through the saved OUTPUT y (dx may alias dy). */
int ssasr_act_bwd(int act, const float* dy, const float* y, float* dx, int64_t n, void* stream);

/* nn.BCELoss (mean) of n probabilities against ONE target value -- ADVTrainer's three losses
 * (src/trainer.py:981-984 real labels 1 - label_smoothing, :992-993 fake labels 0, :1012-1028 generator
 * labels 1), log terms clamped at -100 as torch does.  loss: float[1], written.
 * ssasr_bce_bwd: dp[i] = upstream * (p - t) / max((1 - p) p, 1e-12) / n; upstream: float[1] or NULL (= 1). */
int ssasr_bce_fwd(const float* p, int64_t n, float target, float* loss, void* stream);
int ssasr_bce_bwd(const float* p, int64_t n, float target, const float* upstream, float* dp, void* stream);

/* SAETrainer's SpeechAutoEncoder (src/speech_autoencoder.py; src/trainer.py:760-907).  Activations are
 * CHANNELS-LAST: [B][T][W][C] (time, mel, channel) -- the fbank batch [B][T][F] is the first layer's input as it
 * stands (W = F, C = 1), the global encoder's output [B][1][1][256] is [B][256].
 *
 * ssasr_conv2d_fwd: nn.Conv2d(C, F, [kh, kw], padding 0, bias False) (:118-147): x [B][T][W][C], w in torch's
 *   layout [F][C][kh][kw], y [B][T - kh + 1][W - kw + 1][F].  The product reads its overlapping input windows in
 *   place through the GEMM's row maps when a kernel row's kw * C values are a multiple of 32 or kh == 1;
 *   other shapes go through an im2col copy in ws.  ws: float[ssasr_conv2d_ws_floats(...)], scratch.
 * ssasr_conv2d_bwd: dw (optional, torch layout) += the weight gradient (needs x); dx (optional) [B][T][W][C] = the
 *   input gradient (needs w).  dy_bordered != 0: dy is stored inside a zero border of kh - 1 rows and kw - 1
 *   columns, [B][To + 2 (kh - 1)][Wo + 2 (kw - 1)][F] (what ssasr_bn_relu_pool_bwd writes with border_t = kh - 1,
 *   border_w = kw - 1) -- required for dx, whose full correlation reads the border in place; 0: dense
 *   [B][To][Wo][F]. */
int64_t ssasr_conv2d_ws_floats(int64_t B, int64_t T, int64_t W, int64_t C, int64_t F, int64_t kh, int64_t kw);
int ssasr_conv2d_fwd(const float* x, const float* w, float* y, int64_t B, int64_t T, int64_t W, int64_t C,
                     int64_t F, int64_t kh, int64_t kw, float* ws, void* stream);
int ssasr_conv2d_bwd(const float* dy, int dy_bordered, const float* x, const float* w, float* dx, float* dw,
                     int64_t B, int64_t T, int64_t W, int64_t C, int64_t F, int64_t kh, int64_t kw, float* ws,
                     void* stream);

/* nn.BatchNorm2d + nn.ReLU + nn.MaxPool2d([ph, pw]) of one encoder block (:123-125), channels-last.
 * ssasr_bn_stats: per-channel statistics of y [rows][C] (rows = B * T * W), two passes, sums in double.
 *   training != 0: batch mean / biased variance; running_mean / running_var are updated in place with
 *   `momentum` (the variance unbiased), as torch does.  0: the running statistics are used.
 *   save: float[4 * C] = mean, 1 / sqrt(var + eps), scale = gamma * invstd, shift = beta - mean * scale.
 *   ws: float[ssasr_bn_ws_floats(C)] scratch (shared with ssasr_bn_relu_pool_bwd).
 * ssasr_bn_relu_pool_fwd: p [B][T / ph][W / pw][C] = max over each window of relu(y * scale + shift) (floor
 *   mode: remainder rows / columns dropped); idx: offset i * pw + j of the FIRST maximum inside its window.
 *   ws: float[ssasr_pool_ws_floats(...)] scratch (0 floats, NULL allowed, for windows of fewer than 64 values;
 *   larger windows are reduced in chunks across the chip).
 * ssasr_bn_relu_pool_bwd (training-mode batch norm): from dp, the gradient of p, writes the gradient of the
 *   convolution output y, dy [B][T + 2 border_t][W + 2 border_w][C] (the border zeroed here), and adds
 *   dgamma / dbeta (optional).  Windows whose maximum is 0 pass nothing (ReLU). */
int64_t ssasr_bn_ws_floats(int64_t C);
int ssasr_bn_stats(const float* y, int64_t rows, int64_t C, const float* gamma, const float* beta,
                   float* running_mean, float* running_var, float momentum, float eps, int training, float* ws,
                   float* save, void* stream);
int64_t ssasr_pool_ws_floats(int64_t B, int64_t T, int64_t W, int64_t C, int64_t ph, int64_t pw);
int ssasr_bn_relu_pool_fwd(const float* y, const float* save, int64_t B, int64_t T, int64_t W, int64_t C,
                           int64_t ph, int64_t pw, float* p, int32_t* idx, float* ws, void* stream);
int ssasr_bn_relu_pool_bwd(const float* dp, const float* p, const int32_t* idx, const float* y, const float* save,
                           const float* gamma, int64_t B, int64_t T, int64_t W, int64_t C, int64_t ph, int64_t pw,
                           int64_t border_t, int64_t border_w, float* dy, float* dgamma, float* dbeta, float* ws,
                           void* stream);

/* The frame decoder's input (:62-75): din[(b, i)] = [listener[b][i][0 .. L) | enc[b][0 .. G)] for the Tq Listener
 * frames of every utterance, as ONE [B * Tq][L + G] matrix (the reference runs its decoder once per frame).
 * _bwd: dlistener [B][Tq][L] = the first L columns; denc [B][G] = the last G summed over an utterance's frames. */
int ssasr_sae_concat_fwd(const float* listener, const float* enc, int64_t B, int64_t Tq, int64_t L, int64_t G,
                         float* din, void* stream);
int ssasr_sae_concat_bwd(const float* ddin, int64_t B, int64_t Tq, int64_t L, int64_t G, float* dlistener, float* denc,
                         void* stream);

/* SAETrainer's loss (src/trainer.py:811-818): nn.SmoothL1Loss() (mean) between the prediction pred [B][R][F]
 * padded with zero rows up to bt frames and x[:, :bt] (x [B][Tx][F], Tx >= bt >= R).
 * ws: float[ssasr_smooth_l1_ws_floats()]; loss: float[1].  _bwd: dpred [B][R][F]; upstream float[1] or NULL. */
int64_t ssasr_smooth_l1_ws_floats(void);
int ssasr_smooth_l1_fwd(const float* pred, const float* x, int64_t B, int64_t bt, int64_t R, int64_t Tx, int64_t F,
                        float* ws, float* loss, void* stream);
int ssasr_smooth_l1_bwd(const float* pred, const float* x, int64_t B, int64_t bt, int64_t R, int64_t Tx, int64_t F,
                        const float* upstream, float* dpred, void* stream);

/* Frame lengths of zero-padded fbanks, prepare_x (src/ASRDataset.py:314):
 * lens[b] = number of frames whose feature sum is non-zero. */
int ssasr_frame_lengths(const float* x, int64_t B, int64_t T, int64_t F, int32_t* lens,
                        void* stream);

/* Batch assembly from a device-resident corpus: what ASRDataset.__getitem__ + the
 * DataLoader + prepare_x produce for one batch (src/ASRDataset.py:206-226, :297-315),
 * without host round trips.  frames [sum of lengths][F] holds the unpadded frames of every
 * utterance back to back; out[b][t][:] = frames[offsets[b] + t][:] for t < lens[b], zero
 * rows after (out is [B][T][F], T >= max lens). */
int ssasr_gather_batch(const float* frames, const int64_t* offsets, const int32_t* lens, int64_t B,
                       int64_t T, int64_t F, float* out, void* stream);

/* SpecAugment (Park et al. 2019: frequency and time masks on the log-mel input; no time warping) applied in the
 * pass that assembles the batch.  BUILD-DEFINED -- the reference trains on unaugmented filterbanks.
 * out[b][t][f] = frames[offsets[b] + t][f] for t < lens[b], EXCEPT that a cell whose t lies in one of the
 * utterance's time masks or whose f lies in one of its frequency masks holds `fill`; rows t >= lens[b] are zero,
 * not `fill`.  A mask (start, width) covers start <= i < start + width; masks may overlap, width 0 covers nothing.
 * utt_ids int32 [B]: every row's index in the CORPUS.  An utterance's masks depend on (seed, epoch, utt_id, len, F)
 * alone -- not on its batch, its slot, B or the rank -- and are drawn statelessly, in unsigned integer arithmetic
 * only (no floating point anywhere), all of it modulo 2^32 unless it says 64-bit:
 *   mix(x):  x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16
 *   h = mix((seed mod 2^32) ^ 0x9e3779b9); h = mix(h ^ (seed >> 32)); h = mix(h ^ (epoch mod 2^32));
 *   h = mix(h ^ (epoch >> 32)); hu = mix(h ^ utt_id)          (utt_id as its 32-bit two's complement pattern)
 *   draw(k, n) = (mix(hu ^ k) * n) >> 32                      (the product in 64 bits: uniform on 0 .. n - 1)
 * Masks are numbered j = 0 .. n_freq - 1 (frequency), then j = n_freq .. n_freq + n_time - 1 (time):
 *   frequency mask j:  width = draw(2 j, max_freq + 1),  start = draw(2 j + 1, F - width + 1)
 *   time mask j:       width = draw(2 j, cap + 1),       start = draw(2 j + 1, len - width + 1),
 *                      cap = min(max_time, len * time_permille / 1000)   (64-bit product, integer division).
 * Limits (argument error otherwise): n_freq, n_time in 0 .. 8, 0 <= max_freq <= F, max_time >= 0,
 * 0 <= time_permille <= 1000, and those of ssasr_gather_batch.  With n_freq = n_time = 0 the entry launches
 * ssasr_gather_batch's kernel.  epoch: the caller's draw counter (one value per pass over the corpus).
 * ssasr_specaug_plan is a HOST function (host pointers, no GPU work): the masks the kernel applies to one
 * utterance, from the same code, as masks[n_freq + n_time][2] = (start, width); len >= 0, F > 0. */
typedef struct ssasr_specaug {
  int32_t n_freq, max_freq;
  int32_t n_time, max_time;
  int32_t time_permille;
  float fill;
  uint64_t seed;
  uint64_t epoch;
} ssasr_specaug;
int ssasr_gather_batch_aug(const float* frames, const int64_t* offsets, const int32_t* lens,
                           const int32_t* utt_ids, int64_t B, int64_t T, int64_t F,
                           const ssasr_specaug* p, float* out, void* stream);
int ssasr_specaug_plan(const ssasr_specaug* p, int32_t utt_id, int32_t len, int32_t F, int32_t* masks);

/* Log-mel filterbank of one waveform: log_fbank, src/preprocess.py:187-208
 * (librosa 0.6.3 melspectrogram defaults: centred reflect-padded STFT with a
 * periodic Hann window of n_fft samples, power 2, Slaney mel filters, then
 * log(S + 2.22e-16)).  F = ssasr_logmel_frames(n_samples, n_fft, hop) = 1 + (n + 2 (n_fft / 2) - n_fft) / hop,
 * librosa's centred framing (1 + n / hop for an even window).
 * Constants (host-built, device-resident): window [n_fft]; dft_basis
 * [2*nb][Kp] with nb = n_fft/2+1, Kp = roundup(n_fft,4), rows 0..nb-1 =
 * cos(2 pi k n / n_fft), rows nb.. = sin; mel_basis [n_mels][nbp], nbp =
 * roundup(nb,4).  Workspaces: ws_frames [F][Kp], ws_spec [F][2*nb], ws_power
 * [F][nbp].  out [F][n_mels]. */
int64_t ssasr_logmel_frames(int64_t n_samples, int64_t n_fft, int64_t hop);
/* The same for a BATCH of utterances in three launches instead of four per utterance, without the
 * framed copy and without the complex spectrum in memory: (1) every waveform, reflect-extended, is laid
 * out hop-aligned in ws_wave -- utterance u at sample first_row_u * hop, occupying
 * ssasr_logmel_batch_rows(n_u, n_fft, hop) rows of `hop` samples, of which the first
 * ssasr_logmel_frames(n_u, n_fft, hop) are its frames (the rest straddle into the next utterance: ignore them);
 * (2) ONE DFT product over all rows, whose A operand is ws_wave read as overlapping rows of stride hop,
 * against dft_basis_w [2*nb][Kp]: the window folded into the basis and the cos / sin rows of a bin
 * interleaved (w cos_0, w sin_0, w cos_1, ...), so that the epilogue writes re^2 + im^2; (3) the mel
 * product with the log epilogue.
 * wav: all waveforms (any layout); utt: DEVICE int64 [n_utts][3] = {offset of the utterance in wav, its
 * sample count, its first row}; max_samples / total_rows: the longest utterance / the sum of all rows
 * (host values).  ws_wave: total_rows * hop + n_fft floats; ws_power: total_rows * nbp floats;
 * out [total_rows][n_mels] (rows of utterance u: first_row_u ... + frames_u). */
int64_t ssasr_logmel_batch_rows(int64_t n_samples, int64_t n_fft, int64_t hop);
int ssasr_logmel_batch(const float* wav, const int64_t* utt, int64_t n_utts, int64_t max_samples,
                       int64_t total_rows, int64_t n_fft, int64_t hop, int64_t n_mels,
                       const float* dft_basis_w, const float* mel_basis, float* ws_wave, float* ws_power,
                       float* out, void* stream);
int ssasr_logmel(const float* wav, int64_t n_samples, int64_t n_fft, int64_t hop, int64_t n_mels,
                 const float* window, const float* dft_basis, const float* mel_basis,
                 float* ws_frames, float* ws_spec, float* ws_power, float* out, void* stream);

/* ---- inference (ABI 15) -------------------------------------------------------------------------------------
 * Parameters of the character language model, CharLM (src/charlm.py:26-44), PyTorch layouts:
 * emb [V][H]; two nn.GRUCell (gate order r, z, n): w_ih*, w_hh* [3H][H], b_ih*, b_hh* [3H]; out: w_out [V][H],
 * b_out [V].  H % 4 == 0; every pointer 16-byte aligned. */
typedef struct ssasr_charlm {
  int64_t V, H;
  const float* emb;
  const float* w_ih1; const float* w_hh1; const float* b_ih1; const float* b_hh1;
  const float* w_ih2; const float* w_hh2; const float* b_ih2; const float* b_hh2;
  const float* w_out; const float* b_out;
} ssasr_charlm;

/* One CharLM.forward (src/charlm.py:46-57) for B rows: x int32 [B] character ids, h1 / h2 [B][H] ->
 * out [B][V] (the output layer, no softmax), h1_out / h2_out [B][H] (may alias h1 / h2).
 * GRUCell: r = s(W_ir x + b_ir + W_hr h + b_hr), z likewise, n = tanh(W_in x + b_in + r * (W_hn h + b_hn)),
 * h' = (1 - z) * n + z * h.  One workgroup per row. */
int ssasr_charlm_step(const ssasr_charlm* lm, const int32_t* x, const float* h1, const float* h2, int64_t B,
                      float* out, float* h1_out, float* h2_out, void* stream);

/* ---- CTC decoding with an LM: CharLM shallow fusion inside the prefix search (added under ABI 16) ---------------
 * BUILD-DEFINED.  ssasr_ctc_decode's prefix beam search (above: the same candidates, the same g_b' / g_n', the same
 * identity of texts) with the CharLM in the RANKING, as Hannun et al. 2014, alg. 1 places a language model.  The LM
 * score is a function of the TEXT alone, so g_b and g_n stay pure CTC masses and only the order changes.
 *   L(w) of a text w = c_1 .. c_n: sum_i log_softmax(lm_out(<SOS> = 0, c_1 .. c_{i-1}))[c_i]: the CharLM is fed class 0
 *   from zero states and then each character, as ssasr_decode_beam feeds it; the softmax runs over all V classes, blank
 *   included; a row's log-softmax is formed in float (y - max - logf(sum expf(y - max))), L is accumulated in double.
 *   Frame t: a candidate's key is logaddexp(g_b', g_n') + lm_weight L(w) + length_bonus |w| in double, the terms added
 *   in that order; B_t is the min(K, number of finite candidates) candidates with the largest keys, ties as in
 *   ssasr_ctc_decode (a kept text first, then the lower slot, then the lower character).  L(u.c) = L(u) +
 *   lmrow(u)[c], lmrow(u) being the LM's log-softmax row after u, computed ONCE, when u enters a beam: only a frame's
 *   winners that are new extensions take a CharLM step (at most K, run together, the weights streamed once per 8 of
 *   them); a kept member keeps its state and its row.
 *   After the last frame, with eos >= 0: final(w) = key(w) + lm_weight lmrow(w)[eos]; the members are ranked by
 *   counting as ssasr_rescore ranks (non-increasing total as rounded to float, equal totals in slot order).  With
 *   eos < 0 no end term is added and the order is the last frame's.
 *   A term whose weight is exactly 0 is left out of every sum.  At lm_weight == 0 no LM step runs and lm is unread
 *   (it may be NULL); at lm_weight == 0 && length_bonus == 0 the outputs are ssasr_ctc_decode's, bit for bit.
 * Outputs in ssasr_ctc_decode's layout (chars [B][K][T], n_chars [B][K], n_hyps [B]) and three score rows [B][K]:
 * scores the fused total, ctc_scores logaddexp(g_b, g_n), lm_scores L plus the end term.  Every element is written:
 * slots from n_hyps on get length 0, scores and ctc_scores -inf, lm_scores 0.
 * Accepted: B, T, V and blank as ssasr_ctc_decode takes them for K >= 1; 1 <= K <= 32 (the best path has no LM form);
 * lm a HOST pointer to a block ssasr_charlm_step accepts (H % 4 == 0, H <= 4096, 16-byte aligned pointers) with
 * lm->V == V, required when lm_weight != 0; finite lm_weight and length_bonus; eos < V; ws 16-byte aligned with
 * ws_bytes >= ssasr_ctc_decode_lm_ws_bytes(B, T, V, K, H), H = lm->H when lm_weight != 0 and 0 otherwise (0: no kernel
 * for the shape).  Argument errors return before any HIP call.
 * One launch of 512 threads per utterance, no exchange between workgroups, no spins, no atomics; every loop is bounded
 * by len, K, V, H or T.  LDS (32 KB, static) holds ssasr_ctc_decode's 20 KB, the K rows lmrow [K][64] and L; the
 * workspace holds, per utterance, the GRU states of K slots and of the frame's up to K new members ([2][K][2H]
 * floats), the embeddings, gate pre-activations and output rows of the 8 hypotheses in flight, the two beams' texts
 * [2][K][T] int32 and, in its last B words, the number of frames that ran an LM step (tools/ctc_lm_time.py). */
int64_t ssasr_ctc_decode_lm_ws_bytes(int64_t B, int64_t T, int64_t V, int64_t K, int64_t H);
int ssasr_ctc_decode_lm(const float* logits, const int32_t* frame_lens, int64_t B, int64_t T, int64_t V, int64_t K,
                        int blank, void* ws, int64_t ws_bytes, int32_t* chars, int32_t* n_chars, float* scores,
                        int32_t* n_hyps, const ssasr_charlm* lm, float lm_weight, float length_bonus, int eos,
                        float* ctc_scores, float* lm_scores, void* stream);

/* ---- CTC decoding with a character graph: n-gram LM and hotword biasing inside the prefix search (under ABI 16) ----
 * BUILD-DEFINED.  A character graph over V classes is a complete deterministic weighted automaton: S states, a start
 * state, next [S][V] int32 (the state after class c), arc [S][V] float (finite, or -inf: the extension is FORBIDDEN)
 * and fin [S] float (finite).  For a text w = c_1 .. c_n: s_0 = start, s_i = next[s_{i-1}][c_i],
 *   G(w) = sum_i arc[s_{i-1}][c_i],   state(w) = s_n.
 * A count-based n-gram LM (states: the seen histories, arcs: log P(c | history), fully backed off), a hotword list
 * (its Aho-Corasick automaton) and their product are such graphs; ss_asr_amd/char_graph.py builds them.  The blank's
 * column is never read.
 * The search is ssasr_ctc_decode's for K >= 1 (the same candidates, the same g_b' / g_n', the same identity of
 * texts) with G in the RANKING, as ssasr_ctc_decode_lm places the CharLM: G is a function of the text alone, so g_b and
 * g_n stay pure CTC masses.
 *   Frame t: a candidate's key is logaddexp(g_b', g_n') + graph_weight G(w) + length_bonus |w| in double, the terms
 *   added in that order; a candidate whose key is -inf (no CTC mass, or a forbidden arc) is no candidate; B_t is the
 *   min(K, number of finite candidates) candidates with the largest keys, ties as in ssasr_ctc_decode.  A kept text has
 *   a finite key, and the kept texts' blank extensions are always finite, so a beam never empties.
 *   G(u.c) = G(u) + arc[state(u)][c] in double, state(u.c) = next[state(u)][c], both taken when u.c enters a beam.
 *   After the last frame: total(w) = key(w) + graph_weight fin[state(w)]; the members are ranked by counting as
 *   ssasr_rescore ranks (non-increasing total as rounded to float, equal totals in slot order).
 *   A term whose weight is exactly 0 is left out of every sum.  At graph_weight == 0 the tables are unread (graph may
 *   be NULL); at graph_weight == 0 && length_bonus == 0 the outputs are ssasr_ctc_decode's, bit for bit.
 * Outputs in ssasr_ctc_decode's layout (chars [B][K][T], n_chars [B][K], n_hyps [B]) and three score rows [B][K]:
 * scores the fused total, ctc_scores logaddexp(g_b, g_n), graph_scores G + fin.  Every element is written: slots from
 * n_hyps on get length 0, scores and ctc_scores -inf, graph_scores 0.
 * Accepted: B, T, V and blank as ssasr_ctc_decode takes them for K >= 1; 1 <= K <= 32; graph a HOST pointer to a
 * struct of DEVICE tables with graph->V == V, 1 <= S <= 1,048,576 and 0 <= start < S, required when graph_weight != 0;
 * finite graph_weight >= 0 (a negative weight would turn a forbidden arc into +inf) and finite length_bonus; ws
 * 8-byte aligned with ws_bytes >= ssasr_ctc_decode_graph_ws_bytes(B, T, V, K) (0: no kernel for the shape).  Argument
 * errors return before any HIP call.  The tables' CONTENTS cannot be checked here: the kernel clamps every state it
 * reads to [0, S - 1], so a malformed table gives wrong scores and never a read outside the tables (char_graph.CharGraph
 * validates them before the upload).
 * One launch of 256 threads per utterance, no exchange between workgroups, no spins, no atomics; every loop is bounded
 * by len, K, V or T; an utterance's results depend on its own frames alone.  LDS (40 KB, static) holds
 * ssasr_ctc_decode's 20 KB, per member its state (int32) and G (double), and per member the two table rows of its
 * state, next and arc [K][64] each, addressed through a slot that a kept member keeps: the tables are read from memory
 * only for the members that newly enter a beam (at most K rows a frame), and the frame's candidates read LDS alone.
 * The workspace holds the two beams' texts [B][2][K][T] int32. */
typedef struct ssasr_char_graph {
  const int32_t* next;
  const float* arc;
  const float* fin;
  int32_t S, V, start;
} ssasr_char_graph;
int64_t ssasr_ctc_decode_graph_ws_bytes(int64_t B, int64_t T, int64_t V, int64_t K);
int ssasr_ctc_decode_graph(const float* logits, const int32_t* frame_lens, int64_t B, int64_t T, int64_t V, int64_t K,
                           int blank, void* ws, int64_t ws_bytes, int32_t* chars, int32_t* n_chars, float* scores,
                           int32_t* n_hyps, const ssasr_char_graph* graph, float graph_weight, float length_bonus,
                           float* ctc_scores, float* graph_scores, void* stream);

/* ---- CTC decoding over a lexicon with a word n-gram LM inside the prefix search (added under ABI 16) ---------------
 * BUILD-DEFINED.  A word graph over V classes with a space class sp (not the blank) has two parts.
 * The TRIE of the lexicon's spellings, N nodes, root 0: child [N][V] int32 (the node after class c; any value where the
 * arc is -inf), carc [N][V] float (finite, or -inf = FORBIDDEN; the columns sp and blank are never read), word [N]
 * int32 (the id of the word that ends at the node, -1: none; word[0] = -1) and pen [N] float (finite).
 * The WORD LM of H states over W words in back-off form: off [H + 1] int32 delimits the states' rows; wid [E] int32,
 * strictly ascending inside a row; wlp [E] float (finite); wnext [E] int32 (the state after the word); bow [H] float
 * (finite); bnext [H] int32 (the back-off state, -1 for state 0); eos [H] float (finite): log P(</s> | h), fully
 * resolved.  State 0 is the empty history and its row is DENSE: off[1] - off[0] == W and wid[e] == e there; it is
 * indexed directly, so a look-up always ends in it.
 *   lookup(h, w): acc = 0 in double; search w in h's row: found at e -> (acc + wlp[e], wnext[e]); else acc += bow[h],
 *   h = bnext[h], again.  At most SSASR_WORD_MAX_ORDER rounds; after them, or at bnext < 0, the result is -inf (a
 *   malformed table: word_graph.WordGraph never builds one).
 * A text's state is (n, h), the empty text's (0, 0).  For c != sp the arc is carc[n][c] and the state (child[n][c], h).
 * For c == sp with word[n] < 0 the arc is -inf (the root too: no leading or doubled space); otherwise, with
 * (lp, h') = lookup(h, word[n]), the arc is (float)((double)pen[n] + lp) and the state (0, h').
 *   G(text) = the sum of the arcs in double.  fin(n, h) = pen[n] + eos[h] where word[n] < 0 (the root after a trailing
 *   space, the empty text, or mid-word, where pen carries the builder's finite `unfinished` penalty);
 *   fin(n, h) = (that space arc) + eos[h'] where word[n] >= 0.
 * The search, the keys, the ties, the end ranking and the outputs are ssasr_ctc_decode_graph's word for word with this
 * G and fin: key = logaddexp(g_b', g_n') + graph_weight G + length_bonus |w|, total = key + graph_weight fin, both
 * state components taken when the extended text enters a beam; scores / ctc_scores / graph_scores (G + fin) [B][K].
 * A term whose weight is exactly 0 is left out; at graph_weight == 0 the tables are unread (graph may be NULL), and
 * at graph_weight == 0 && length_bonus == 0 the outputs are ssasr_ctc_decode's, bit for bit.
 * Accepted: ssasr_ctc_decode_graph's arguments, with graph a HOST pointer to a struct of DEVICE tables: no NULL table,
 * graph->V == V, 0 <= sp < V and sp != blank, N, H and W in 1 .. 1,048,576, E >= W; finite graph_weight >= 0 and finite
 * length_bonus.  Argument errors return before any HIP call.  The tables' CONTENTS cannot be checked here: the kernel
 * clamps every node, state, word id and row bound it reads into range, so a malformed table gives wrong scores and
 * never a read outside the tables (word_graph.WordGraph validates them before the upload).
 * One launch of 256 threads per utterance, no exchange between workgroups, no spins, no atomics, no barrier beyond
 * ssasr_ctc_decode_graph's; every loop is bounded by SSASR_WORD_MAX_ORDER, 32 search rounds, K, V or T.  LDS holds
 * ssasr_ctc_decode_graph's 40 KB with the pair (n, h) per member and h' per row: the tables are read only for the
 * members that newly enter a beam, one wave each -- two dense rows and, where a word ends at the node, one look-up by
 * the whole wave (64 cuts of the row per round) -- and once per member after the last frame for fin.
 * The workspace holds the two beams' texts [B][2][K][T] int32. */
#define SSASR_WORD_MAX_ORDER 8
typedef struct ssasr_word_graph {
  const int32_t* child;
  const float* carc;
  const int32_t* word;
  const float* pen;
  const int32_t* off;
  const int32_t* wid;
  const float* wlp;
  const int32_t* wnext;
  const float* bow;
  const int32_t* bnext;
  const float* eos;
  int32_t N, V, H, W, E, sp;
} ssasr_word_graph;
int64_t ssasr_ctc_decode_word_ws_bytes(int64_t B, int64_t T, int64_t V, int64_t K);
int ssasr_ctc_decode_word(const float* logits, const int32_t* frame_lens, int64_t B, int64_t T, int64_t V, int64_t K,
                          int blank, void* ws, int64_t ws_bytes, int32_t* chars, int32_t* n_chars, float* scores,
                          int32_t* n_hyps, const ssasr_word_graph* graph, float graph_weight, float length_bonus,
                          float* ctc_scores, float* graph_scores, void* stream);

/* The greedy decode loop of ASR.decode (src/asr.py:112-173, driven by ASRTester.exec, src/trainer.py:578-592)
 * for N encoded utterances as ONE launch: per utterance and step the attention (src/asr.py:383-390), both
 * Speller cells, char_trans and log_softmax (:149-153), one CharLM step fed with the previously emitted
 * character (<SOS> = 0 first; :154-155), final = asr + lm_weight * lm and its first maximum (:156-159), whose
 * embedding feeds the next step (:161-162), until <EOS> (:167-169) or max_steps (:128, :143).
 * One workgroup owns one utterance for the whole loop; workgroups exchange nothing (no status words, no
 * workspace to arm), every loop is bounded, and a finished utterance's workgroup exits.  An utterance's
 * results depend on its own frames and enc_len alone: the same bits in any batch, at any padded T.
 * Accepted: what ssasr_decoder_fwd accepts (A % 4 == 0, E % 4 == 0, D % 16 == 0, T <= 16384, A <= 2048,
 * E <= 8192) with V <= 64, as long as the utterance's state fits one CU's LDS
 * (9 D + E + A + T + 9 H + 2208 floats <= 160 KB); everything else is an argument error before any launch. */
typedef struct ssasr_infer {
  /* sizes */
  int64_t N, T, E, A, D, V, max_steps;
  /* inputs */
  const float* feat;        /* [N][T][E] listener outputs, each utterance encoded alone; frames >= enc_len unread */
  const int32_t* enc_len;   /* [N], clamped to 1 .. T                                                            */
  float* comp;              /* [N][T][A] workspace: tanh(psi(feat)), computed once by the launch itself          */
  /* parameters (PyTorch layouts), the fields of ssasr_decoder plus psi */
  const float* w_psi; const float* b_psi;   /* [A][E], [A]                       */
  const float* w_phi;       /* [A][D]                                            */
  const float* w_ih1; const float* w_hh1; const float* b_ih1; const float* b_hh1; /* cell 1: I = D + E */
  const float* w_ih2; const float* w_hh2; const float* b_ih2; const float* b_hh2; /* cell 2: I = D     */
  const float* embed;       /* [V][D]                                            */
  const float* w_ct; const float* b_ct;     /* [V][D], [V]                       */
  const ssasr_charlm* lm;   /* HOST pointer; NULL: no LM term, lm_weight ignored; lm->V must equal V */
  float lm_weight;
  int32_t eos;              /* the character that ends an utterance               */
  /* outputs, written completely by the launch; rows past an utterance's last executed step are zero */
  int32_t* chars;           /* [N][max_steps] the winner of every executed step (the <EOS> that ended it included) */
  int32_t* n_chars;         /* [N] characters emitted before <EOS>; max_steps when the cap ended the loop          */
  float* scores;            /* [N][max_steps][V] `final` of every executed step                                    */
  float* att;               /* [N][max_steps][T] attention weights, optional                                       */
} ssasr_infer;

int ssasr_decode_greedy(const ssasr_infer* d, void* stream);

/* ---- CharLM training (ABI 16) --------------------------------------------------------------------------------
 * One chunk of CHARLMTrainer.exec (src/trainer.py:229-251) as one forward and one backward launch.  A workgroup
 * owns 16 batch rows for the whole chunk; workgroups exchange nothing (no status words, nothing to arm), every
 * loop is bounded by U, B, H or V, and a row's results depend on that row's inputs alone: the same bits at
 * B = 1 as in any batch.  fp32 throughout (fp32 MFMA, expf, tanhf).
 * Accepted: V <= 64, H % 16 == 0 with 16 <= H <= 256, any B >= 1 and U >= 1 with U * B < 2^29; every pointer of
 * `lm` and `ws` 16-byte aligned.  Anything else: a negative code, and the size query returns 0.
 *
 * Workspace, ssasr_charlm_train_ws_floats(B, U, H, V) floats, consecutive blocks (R = U * B, row t * B + b):
 *   G1 [V][3H] rounded up to 16 floats: emb . W_ih1^T + b_ih1 | WT_hh1, WT_ih2, WT_hh2 [H][3H] | WT_out [H][64]
 *   (written by the forward's prologue kernel) | H1, H2 [U+1][B][H]: the state BEFORE step t in block t |
 *   S1, S2 [R][4H]: r, z, n, W_hn h + b_hn after the forward; d r_pre, d z_pre, d n_pre, r * d n_pre after the
 *   backward (d gi = columns [0, 3H), d gh = columns [0, 2H) and [3H, 4H)) | DL [R][64]: softmax after the forward,
 *   d logits after the backward (classes >= V zero) | OH [R][64]: one-hot of the character fed to the step.
 * The parameter gradients are products over these blocks (ssasr_gemm_f32, ta = 1, K = R), left to the caller. */
int64_t ssasr_charlm_train_ws_floats(int64_t B, int64_t U, int64_t H, int64_t V);

/* Forward (src/trainer.py:231-249; per step src/charlm.py:53-56, nn.CrossEntropyLoss(reduction='none'), and on
 * a sampled step Categorical(softmax).sample(), :245, as the first v with cumsum(exp(l - max))[v] > u * total).
 * y int32 [B][U] labels; feed int32 [B][U]: the character fed to step t + 1 when step t is teacher-forced
 * (training passes y); modes int32 [U] (0 teacher, 1 sample); uniforms [U][B] or NULL (every step is then
 * teacher-forced).  Ids are clamped to [0, V).
 * -> loss_rows [B]: sum over the steps of -log p[y]; fed int32 [U+1][B]: what each step was fed, row 0 = 0
 * (<SOS>, :231); logits [U][B][V], optional. */
int ssasr_charlm_train_fwd(const ssasr_charlm* lm, const int32_t* y, const int32_t* feed, const int32_t* modes,
                           const float* uniforms, int64_t B, int64_t U, float* loss_rows, int32_t* fed,
                           float* logits, float* ws, void* stream);

/* Backward through the chunk (loss.backward(), src/trainer.py:250) from the workspace the forward left, with
 * d loss_rows = dloss for every row (1 / B for the mean of :249).  No gradient flows through a sampled
 * character.  Rewrites S1, S2 and DL as described above. */
int ssasr_charlm_train_bwd(const ssasr_charlm* lm, const int32_t* y, int64_t B, int64_t U, float dloss, float* ws,
                           void* stream);

/* ---- beam search (added under ABI 16) ------------------------------------------------------------------------
 * The loop of ssasr_decode_greedy as a beam search over K hypotheses per utterance, ONE launch, one workgroup
 * per utterance for the whole loop; workgroups exchange nothing, nothing spins, every loop is bounded by
 * max_steps, enc_len, K or a dimension.  Every weight matrix is streamed once per step for all live hypotheses.
 * Per utterance (row_b = the score row ssasr_decode_greedy computes for hypothesis b):
 *   start: one live hypothesis, empty prefix, score 0, zero states, input <SOS> = 0;
 *   step:  width W = K - finished; candidates (b, v), live b, v < V, score_b + row_b[v]; the W best (all of them
 *          when fewer exist), by score descending, ties to the lower b * V + v.  A chosen candidate with v == eos
 *          finishes its parent's prefix (<EOS> is not part of the text, its log-probability is part of the
 *          score); the others are the new live set, in candidate order, each with a copy of its parent's state
 *          advanced by its own character;
 *   stop:  no live hypothesis left, or after max_steps steps: what is live then is emitted as it stands;
 *   output: hypotheses by score descending, ties to the earlier step, then to candidate order; unused slots zero.
 * This entry has no length term, no coverage term and no end detection; ssasr_decode_beam_ex (below) adds an
 * additive length bonus, a coverage term and a stop rule.  Still not built: normalising a score by its length, and
 * ESPnet's M-window end detector.  K == 1 follows greedy decoding (the
 * Python surface calls ssasr_decode_greedy for it).  An utterance's results depend on its own frames, enc_len,
 * K and max_steps alone: the same bits in any batch, at any padded T.
 * Accepted: the dimensions ssasr_decode_greedy accepts (its LDS bound does not apply: all per-hypothesis state is
 * in `ws`), 1 <= K <= 32, lm->H <= 4096; ws 16-byte aligned with ws_bytes >= ssasr_decode_beam_ws_bytes(...);
 * everything else is an argument error before any launch.  `ws` needs no initialisation and is private to the
 * launch while it runs; a slice per utterance holds, per hypothesis, the Speller and LM states twice
 * (re-parenting copies from one buffer to the other), the step's intermediates, and the (parent, char)
 * back-pointers of every step. */
typedef struct ssasr_beam {
  /* sizes */
  int64_t N, T, E, A, D, V, max_steps, K;
  /* inputs and parameters: the fields of ssasr_infer */
  const float* feat;
  const int32_t* enc_len;
  float* comp;
  const float* w_psi; const float* b_psi;
  const float* w_phi;
  const float* w_ih1; const float* w_hh1; const float* b_ih1; const float* b_hh1;
  const float* w_ih2; const float* w_hh2; const float* b_ih2; const float* b_hh2;
  const float* embed;
  const float* w_ct; const float* b_ct;
  const ssasr_charlm* lm;   /* HOST pointer; NULL: no LM term */
  float lm_weight;
  int32_t eos;
  /* workspace */
  float* ws;
  int64_t ws_bytes;         /* what the caller allocated at ws */
  /* outputs, written completely by the launch */
  int32_t* chars;           /* [N][K][max_steps] the hypotheses' characters, best first; zero past n_chars */
  int32_t* n_chars;         /* [N][K] characters of each hypothesis; max_steps for one the cap ended      */
  float* hyp_scores;        /* [N][K] summed scores, descending                                           */
  int32_t* n_hyps;          /* [N] hypotheses emitted, 1 .. K                                             */
} ssasr_beam;

/* Bytes of `ws` for these sizes (Hl = lm->H, 0 without an LM; S = max_steps); 0 when they are not accepted. */
int64_t ssasr_decode_beam_ws_bytes(int64_t N, int64_t K, int64_t T, int64_t E, int64_t A, int64_t D, int64_t V,
                                   int64_t Hl, int64_t S);
int ssasr_decode_beam(const ssasr_beam* d, void* stream);

/* ---- joint CTC / attention decoding (added under ABI 16) -----------------------------------------------------
 * BUILD-DEFINED: the reference has no CTC.  ssasr_decode_beam with the CTC prefix score of Watanabe et al. 2017 in
 * every candidate's score, from the head that joint training leaves on the encoder (ssasr_ctc_loss_fwd's logits:
 * W_ctc feat_t + b_ctc, blank = class 0 in training).  Per utterance, lp[t][v] = log_softmax(W_ctc feat_t + b_ctc)
 * for t < enc_len, computed once by the utterance's own workgroup.  For a prefix g, gamma_n^g[t] / gamma_b^g[t] are
 * the log-probabilities of g over frames 0..t ending in a non-blank / a blank, psi(g) its prefix score:
 *   empty prefix: gamma_n = -inf, gamma_b[t] = lp[0][blank] + ... + lp[t][blank], psi = 0;
 *   candidate (b, v), v != blank, v != eos, h = g . v:  psi(h) = logsumexp_t (phi_t + lp[t][v]) with phi_0 = 0 for
 *     the empty g and -inf otherwise, phi_t = logaddexp(gamma_b^g[t-1], gamma_n^g[t-1]), or gamma_b^g[t-1] alone when
 *     v equals g's last character (psi(h) needs the parent's gamma only);
 *   v == eos: psi = logaddexp(gamma_n^g[len-1], gamma_b^g[len-1]);   v == blank: psi = -inf;
 *   candidate score: score_b + (1 - ctc_weight) * log_softmax(speller)[v] + ctc_weight * (psi(h) - psi(g))
 *     + lm_weight * log_softmax(lm)[v];
 *   a candidate whose score is -inf (the blank character, a prefix that no longer fits the utterance's frames) is
 *     never chosen: the width is min(K - finished, finite candidates).  A live hypothesis with a finite score always
 *     keeps a finite <EOS> candidate, so the loop still ends;
 *   a chosen non-eos candidate gets gamma^h from its parent's gamma by the standard recursion
 *     gamma_n^h[t] = logaddexp(gamma_n^h[t-1], phi_t) + lp[t][v],
 *     gamma_b^h[t] = logaddexp(gamma_b^h[t-1], gamma_n^h[t-1]) + lp[t][blank]   (gamma^h[-1] = -inf),
 *     written into the other state buffer beside the copy of the Speller and LM state.
 * Everything else -- ties, the <EOS> rule, the cap (a live hypothesis is emitted as it stands), the output order,
 * the unused slots, an utterance's independence of N and the padded T -- is ssasr_decode_beam's.  gamma and psi are
 * doubles, exp / log run in float on differences from the running maximum (as ssasr_ctc_loss_fwd's lattice).
 * Accepted: what ssasr_decode_beam accepts, with 0 <= ctc_weight <= 1, 0 <= blank < V, blank != eos, and for
 * ctc_weight > 0 w_ctc (16-byte aligned) and b_ctc; ws_bytes >= ssasr_decode_beam_ctc_ws_bytes(...), which is never
 * less than ssasr_decode_beam_ws_bytes(...): the slice also holds lp [T][64] floats, gamma 2 x K x 2 x T doubles and
 * psi 2 x K doubles.  ctc_weight == 0 launches ssasr_decode_beam's own kernel (the same bits; the head is unread).
 * Everything else is an argument error before any launch, and the size query returns 0. */
typedef struct ssasr_ctc_prefix {
  const float* w_ctc;       /* [V][E] ctc_head.weight */
  const float* b_ctc;       /* [V]    ctc_head.bias   */
  float ctc_weight;         /* lambda                 */
  int32_t blank;
} ssasr_ctc_prefix;

int64_t ssasr_decode_beam_ctc_ws_bytes(int64_t N, int64_t K, int64_t T, int64_t E, int64_t A, int64_t D, int64_t V,
                                       int64_t Hl, int64_t S);
int ssasr_decode_beam_ctc(const ssasr_beam* d, const ssasr_ctc_prefix* c, void* stream);

/* ---- length bonus, coverage term, end detection (added under ABI 16) -------------------------------------------
 * BUILD-DEFINED: the reference has no beam search.  ssasr_decode_beam (c NULL or ctc_weight 0) / ssasr_decode_beam_ctc
 * with three terms inside the same one-launch kernel.  Per utterance, on top of those entries' semantics; everything
 * else -- ties, the <EOS> rule, the cap, the output order, the unused slots, an utterance's independence of N and
 * the padded T -- is unchanged.
 *   Length bonus: candidate score = that entry's candidate score + length_bonus (beta) when v != eos, so a
 *     hypothesis of n characters carries n * beta.  beta is any finite float.  This is the ADDITIVE reward, not a
 *     division by the length: a normalised score is not a sum over steps, it could only re-order the final list and
 *     could not change which prefixes survive.  Score normalisation by length is not built.
 *   Coverage (Chorowski & Jaitly 2016): every live hypothesis g keeps cum_g[t], the sum of its attention weights
 *     over its executed steps (float, zero at the start), and cov_g, the number of frames with cum_g[t] >
 *     coverage_threshold (tau).  At a step, after the softmax over the frames, for every live b:
 *     cum'_b[t] = cum_b[t] + att_b[t] for t < enc_len, cov'_b = the number of t < enc_len with cum'_b[t] > tau; every
 *     candidate (b, v), <EOS> included, gets + coverage_weight (eta) * (cov'_b - cov_b); a chosen non-eos candidate's
 *     new slot takes cum', cov' of its parent.  The counts are integers, so the term telescopes to
 *     eta * cov(final prefix).  eta == 0: no coverage state exists and tau is not read.
 *   End detection, after the selection of step s (the finished list and the new live set are known): the loop ends
 *     when at least one hypothesis is finished, at least one is live, and
 *     max(live scores) < max(finished scores) - end_margin (delta).  The live hypotheses are then DISCARDED, not
 *     emitted (they are abandoned prefixes, unlike the cap's): n_hyps = finished.  With beta == 0, eta == 0 and
 *     lm_weight >= 0 every step's increment is <= 0 (with the CTC term as well: a prefix probability never grows), so
 *     with delta == 0 the best hypothesis and its score are exactly those of the search without the rule; only the
 *     tail of the N-best list is lost.  Otherwise the rule is a heuristic.  ESPnet's M-window end detector is not
 *     built.
 *   n_steps[n]: the loop iterations the utterance executed, for any combination of terms.
 * Accepted: what the underlying entry accepts (c non-NULL: ssasr_decode_beam_ctc's checks), with beta and eta
 * finite, tau finite and > 0 when eta != 0, delta not NaN (delta < 0: no end detection), and
 * ws_bytes >= ssasr_decode_beam_ex_ws_bytes(..., ctc = (c != NULL), coverage = (eta != 0)).  That figure is
 * ssasr_decode_beam_ws_bytes / ssasr_decode_beam_ctc_ws_bytes for coverage == 0 and larger by the coverage block
 * otherwise: cum, 2 buffers x K x up4(T) floats per utterance, behind everything else in the slice (a new slot's row
 * is a copy of its parent's into the other buffer, beside the Speller state).  Everything else, t == NULL included,
 * is an argument error before any launch, and the size query returns 0.
 * All terms off (beta == 0, eta == 0, delta < 0): the call launches exactly the kernel ssasr_decode_beam /
 * ssasr_decode_beam_ctc launch and gives the same bits. */
typedef struct ssasr_beam_terms {
  float length_bonus;        /* beta: added to every candidate (b, v) with v != eos                      */
  float coverage_weight;     /* eta; 0: coverage off, no coverage state, threshold ignored               */
  float coverage_threshold;  /* tau > 0                                                                  */
  float end_margin;          /* delta >= 0: end detection on; < 0: off                                   */
  int32_t* n_steps;          /* [N] optional: steps the utterance's loop executed                        */
} ssasr_beam_terms;

int64_t ssasr_decode_beam_ex_ws_bytes(int64_t N, int64_t K, int64_t T, int64_t E, int64_t A, int64_t D,
                                      int64_t V, int64_t Hl, int64_t S, int32_t ctc, int32_t coverage);
int ssasr_decode_beam_ex(const ssasr_beam* d, const ssasr_ctc_prefix* c /* NULL or weight 0: no CTC */,
                         const ssasr_beam_terms* t, void* stream);

/* ---- a character graph in the attention beam search: n-gram LM and hotword biasing (added under ABI 16) ----------
 * BUILD-DEFINED.  ssasr_decode_beam_ex's search (c and t both optional) with the ssasr_char_graph of
 * ssasr_ctc_decode_graph (above: next [S][V], arc [S][V] finite or -inf = FORBIDDEN, fin [S] finite, start) inside the
 * same one-launch kernel.  Per utterance, on top of that entry's semantics:
 *   every live hypothesis g carries state(g) (int32) and G(g) (double, the sum of the arcs taken); the empty prefix has
 *     state = start, G = 0;
 *   candidate (b, v), v != eos: that entry's candidate score + graph_weight * arc[state_b][v];
 *   candidate (b, eos): that entry's candidate score + graph_weight * fin[state_b]; the column arc[.][eos] is never read;
 *   the graph term is ONE float product, added LAST: after the CTC term, the LM term, the parent's score, beta and the
 *     coverage increment;
 *   a candidate at -inf (a forbidden arc, or the CTC form's own rule) is never chosen: in every graph form the width is
 *     min(K - finished, finite candidates).  fin is finite, so a live hypothesis with a finite score keeps a finite
 *     <EOS> candidate and the loop still ends; a beam may hold fewer than K members;
 *   a chosen non-eos candidate's new slot takes state = next[state_b][v], clamped to [0, S - 1], and
 *     G = G_b + arc[state_b][v] (double).  The tables' CONTENTS cannot be checked here: with the clamp (and start checked
 *     below) a malformed table gives wrong scores and never a read outside the tables;
 *   the cap is unchanged: a hypothesis still live after max_steps is emitted as it stands, with NO fin term, exactly as
 *     it carries no <EOS> term.  Consequence: a capped text in the middle of a partial hotword match keeps the advance
 *     that fin would have retracted;
 *   ties, the <EOS> rule, end detection (which compares the fused scores), the output order, the unused slots and an
 *     utterance's independence of N and the padded T are unchanged.
 * graph_scores [N][K], in output order beside hyp_scores (the fused total): G of a capped hypothesis, G + fin of one
 * ended by <EOS>, each rounded once from double; unused slots 0.
 * graph_weight == 0: the term is left out and the tables are unread (graph may be NULL); the call launches exactly the
 * kernel ssasr_decode_beam_ex would launch (t == NULL: the one ssasr_decode_beam / ssasr_decode_beam_ctc launch), gives
 * the same bits, and graph_scores is all zeros.
 * Accepted: what the underlying entry accepts (c NULL or ssasr_decode_beam_ctc's checks; t NULL -- every term off -- or
 * ssasr_decode_beam_ex's checks); graph_weight finite and >= 0 (a negative weight would turn a forbidden arc into
 * +inf); graph a HOST pointer to a struct of DEVICE tables, required with its three tables when graph_weight != 0, and
 * whenever it is passed graph->V == d->V, 1 <= S <= 1,048,576 and 0 <= start < S; graph_scores non-NULL;
 * ws_bytes >= ssasr_decode_beam_graph_ws_bytes(...), which takes ssasr_decode_beam_ex_ws_bytes' arguments and returns
 * its figure: the graph state (K states, K doubles, twice, and the finished entries' parts) is in LDS.  Everything else
 * is an argument error before any HIP call, and the size query returns 0.
 * One workgroup per utterance, no exchange between workgroups, no spins, no atomics; every loop is bounded by
 * max_steps, enc_len, K or a dimension.  Table reads per step: one row of arc (4 V bytes) per live hypothesis, then
 * next / arc of the <= K chosen candidates and fin of the step's finished ones.
 * Not built: a graph term in ssasr_rescore or ssasr_decode_sample, per-phrase bonuses, word-level n-grams. */
int64_t ssasr_decode_beam_graph_ws_bytes(int64_t N, int64_t K, int64_t T, int64_t E, int64_t A, int64_t D,
                                         int64_t V, int64_t Hl, int64_t S, int32_t ctc, int32_t coverage);
int ssasr_decode_beam_graph(const ssasr_beam* d, const ssasr_ctc_prefix* c /* NULL or weight 0: no CTC */,
                            const ssasr_beam_terms* t /* NULL: every term off */,
                            const ssasr_char_graph* graph, float graph_weight,
                            float* graph_scores, void* stream);

/* ---- sampled decoding (added under ABI 16) ---------------------------------------------------------------------
 * BUILD-DEFINED: the reference draws characters only inside its training loop (scheduled sampling).  The loop of
 * ssasr_decode_greedy for K independent SAMPLES per utterance drawn from the model's own distribution, ONE launch,
 * one workgroup per utterance for the whole loop; workgroups exchange nothing, nothing spins, every loop is bounded
 * by max_steps, enc_len, K or a dimension.  comp and every weight matrix are streamed once per step for all of the
 * utterance's samples.  d: a ssasr_beam whose K is the number of samples per utterance; sizes, pointers, parameters,
 * lm, lm_weight and eos mean what they mean to ssasr_decode_beam.
 * Per sample (n, k): zero states, input <SOS> = 0.  At step s, with row = the score row ssasr_decode_greedy computes
 * for that state (log_softmax(speller) + lm_weight * log_softmax(lm); the first term alone when lm is NULL) and
 * u = uniforms[n][k][s]:
 *   z_v = row_v / tau,  m = max_v z_v,  e_v = expf(z_v - m),  total = sum_v e_v (index order);
 *   the drawn character is the first v, in index order, whose running sum e_0 + .. + e_v exceeds u * total, and
 *   V - 1 when none does (the rule of the training loop's sampled steps);
 *   a drawn eos ends the sample: it is not part of the text, its terms are part of the two sums below; otherwise the
 *   character's embedding feeds the next step;
 *   after max_steps steps a live sample is emitted as it stands, n_chars = max_steps.
 * Outputs, all written completely: chars [N][K][max_steps] in SLOT order (unsorted), zero past n_chars; n_chars [N][K];
 * hyp_scores [N][K] = the sum of row[drawn] over the executed steps (ssasr_decode_beam's score of that text, so the
 * two are comparable); n_hyps[n] = K; logq[n][k] = the sum of (z_drawn - m - logf(total)), the log-probability of the
 * draws under the distribution that was sampled (equal to hyp_scores at tau = 1 without an LM, up to rounding).
 * Sample (n, k) depends on its utterance's frames, enc_len, tau and its own row of uniforms alone: the same bits for
 * any N, any padded T.  A finished sample keeps its slot: the step's products run over the slots up to the highest
 * live one and what a finished slot computes is discarded; a workgroup exits once none of its samples is live.  A
 * slot's state is kept once (no selection, no re-parenting).
 * Accepted: what ssasr_decode_beam accepts, with 1 <= K <= 32, uniforms non-NULL and 4-byte aligned, tau finite and
 * > 0, ws_bytes >= ssasr_decode_sample_ws_bytes(...) (0 for sizes that are not accepted).  Everything else, s == NULL
 * included, is an argument error before any HIP call.  Not built: top-k / nucleus truncation, a generator inside the
 * kernel, a CTC term. */
typedef struct ssasr_sample {
  const float* uniforms;  /* [N][K][max_steps], each in [0, 1); step s of sample (n, k) reads [n][k][s]          */
  float temperature;      /* tau > 0, finite                                                                       */
  float* logq;            /* [N][K] optional: the summed log-probability of the drawn characters under the      */
                          /* distribution that was sampled (the ending <EOS>'s included)                         */
} ssasr_sample;

int64_t ssasr_decode_sample_ws_bytes(int64_t N, int64_t K, int64_t T, int64_t E, int64_t A, int64_t D, int64_t V,
                                     int64_t Hl, int64_t S);
int ssasr_decode_sample(const ssasr_beam* d, const ssasr_sample* s, void* stream);

#ifdef __cplusplus
}
#endif
#endif
