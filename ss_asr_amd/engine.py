"""One ASR train step (the body of ASRTrainer.exec, src/trainer.py:415-438) as a
reusable object: forward, masked CE, backward, gradient all-reduce across
ranks, clip + NaN guard + Adadelta.  ASRTrainer.exec, bench.py, smoke() and the
tests all run THIS object, so that what is timed and checked is what trains."""
import os

import torch

from . import dist as sdist
from . import ops
from .optim import FlatParameters, FusedAdadelta, FusedAdam


_settled = False


def settle_collector(again=False):
    """Once per process, after its FIRST train step (any step object): collect, then move everything
    alive to the collector's permanent generation (gc.freeze).  A process holding the model, the
    optimizer and the library bindings tracks ~270 k long-lived objects; a full (generation-2)
    collection walks all of them -- 74 ms on the benchmark host, once per ~300 train steps, which a
    5.6 ms step cannot hide (tools/hiccup.py: one block of 20 steps at 7.47 instead of 5.60 ms/step;
    with the freeze none, and the young collections fall from 0.8 to 0.4 ms).  The collection this
    function itself runs costs the same ~80 ms, once, in the first step's shadow.  `again`: a caller
    that has built more long-lived state since (bench.py after its warm-up) repeats it.
    SSASR_GC_FREEZE=0 leaves the collector alone."""
    global _settled
    if (_settled and not again) or os.environ.get('SSASR_GC_FREEZE', '1') == '0':
        return
    _settled = True
    import gc
    gc.collect()
    gc.freeze()


class TrainStep:
    """What every step object does around its loss, once.  A step is

        self._open()                                   the previous step's verdict, the listener, clean gradients
        with ops.shared_status_row(<optimizer>.status_row):
            <loss>.backward(self._one)                 every persistent launch reports into that optimizer's row
        scale = <all-reduce>
        self._update(scale)                            clip + NaN guard + update, buffers clean again

    and the subclass writes that out with its own loss and all-reduce in the middle.  Its __init__ calls
    `_models_on_gpu`, builds its optimizers and calls `_set_up`."""

    # the process-wide weight-gradient listener (ops.set_wgrad_listener) at the opening of a step: True claims it for
    # `self._listener` -- None keeps another step object's reducer from seeing this pass's gradients; False leaves it
    # alone (the CharLM's step enqueues no weight gradient on the side stream)
    claims_listener = True
    _listener = None

    def _models_on_gpu(self, what, *models):
        for m in models:
            if not next(m.parameters()).is_cuda:
                raise RuntimeError('%s needs %s on the GPU (no CPU path)' % (type(self).__name__, what))

    def _set_up(self, flats, verdicts, grad_clip):
        """flats: the FlatParameters the step zeroes at its opening and its last update leaves clean.  verdicts:
        ((attribute, optimizer), ...) in polling order; the last one's optimizer is the one `_update` steps, and its
        attribute must be 'last_done'."""
        self._flats, self._verdicts, self.grad_clip = tuple(flats), tuple(verdicts), grad_clip
        self._one = torch.ones((), device=self._flats[0].data.device)
        for name, _ in self._verdicts:
            setattr(self, name, None)  # (grad_norm, skipped) of that optimizer's last step whose words have arrived
        self.skipped_steps = 0         # updates (of any of the optimizers) skipped because the gradient norm was NaN

    def _note(self, wait=False):
        """Picks up the verdict of the previous step (gradient norm, NaN skip, and whether one of its persistent
        launches timed out) from each optimizer whose words have reached the host; a time-out raises."""
        for name, optim in self._verdicts:
            done = optim.poll(wait)
            if done is not None:
                setattr(self, name, done)
                self.skipped_steps += int(done[1])

    def finish(self):
        """Waits for the last step's words of every optimizer: returns the last one's (grad_norm, skipped); raises on
        a time-out.  Whoever writes a checkpoint calls this first."""
        self._note(wait=True)
        return self.last_done

    def _open(self):
        self._note()                  # no synchronisation
        if self.claims_listener:
            # (several step objects may alternate in one process: the ASR and joint steps, the trainers of the Seed loop)
            ops.set_wgrad_listener(self._listener)
        for flat in self._flats:
            if not flat.clean:        # (True right after a step whose update kernel zeroed the gradients)
                flat.zero_grad()
            flat.clean = False

    def _update(self, scale):
        """The step's last update.  Its kernel zeroes the gradients it read (zero_grad=True), and the pass touched no
        other gradient of `_flats`: only here are they marked clean."""
        self._verdicts[-1][1].clip_and_step(self.grad_clip, grad_scale=scale, zero_grad=True)
        for flat in self._flats:
            flat.clean = True
        settle_collector()


class ASRTrainStep(TrainStep):
    def __init__(self, model, lr=1.0, eps=1e-8, rho=0.9, grad_clip=5.0, label_smoothing=0.0):
        """label_smoothing in [0, 1) (build-defined): the smoothed CE of ops.masked_ce_loss; 0 is the reference's loss."""
        if not 0.0 <= float(label_smoothing) < 1.0:
            raise ValueError('label_smoothing must lie in [0, 1), got %r' % (label_smoothing,))
        self.label_smoothing = float(label_smoothing)
        self._set_up_asr(model, lr, eps, rho, grad_clip)

    def _set_up_asr(self, model, lr, eps, rho, grad_clip):
        """Adadelta over the whole model and the two-bucket reducer: what every step of the ASR family trains with."""
        self._models_on_gpu('the model', model)
        self.model = model
        self.flat = FlatParameters.of(model)       # (a TAETrainStep over the same model may have made it already)
        sdist.broadcast_flat(self.flat.data)
        self.optim = FusedAdadelta(self.flat, lr=lr, rho=rho, eps=eps)
        # gradient all-reduce in two buckets, the large one overlapped with the last layer's BPTT
        self.reducer = sdist.GradReducer(self.flat, list(model.encoder.blstm_1.parameters()))
        self._listener = self.reducer.wgrad_enqueued
        ops.set_wgrad_listener(self._listener)
        self._set_up([self.flat], [('last_done', self.optim)], grad_clip)
        self.last_logits = None        # [B, U, V] of the most recent step (for the trainer's logging)

    def forward_loss(self, x, y, x_lens, ans_len):
        _, logits, att = self.model(x, ans_len, teacher=y, state_len=x_lens)
        return ops.masked_ce_loss(logits, y, ans_len, self.label_smoothing), logits, att

    def __call__(self, x, y, x_lens, ans_len):
        """x [B,T,F] float32, y [B,L] int64 (both on the GPU), x_lens host list
        (descending), ans_len = max label length - 1 (handed on to forward_loss, whose first two results are the
        loss and the logits).  Returns the loss tensor (on the device; reading it synchronises)."""
        self._open()
        self.reducer.begin()
        # the attention map is only looked at by valid(): no device-to-host copy per train step
        keep, self.model.att_on_host = getattr(self.model, 'att_on_host', True), False
        try:
            with ops.shared_status_row(self.optim.status_row):
                out = self.forward_loss(x, y, x_lens, ans_len)
                loss, self.last_logits = out[0], out[1]
                loss.backward(self._one)
        finally:
            self.model.att_on_host = keep
        self._update(self.reducer.finish())
        return loss


class MWERTrainStep(ASRTrainStep):
    """BUILD-DEFINED (the reference trains on the masked CE alone): one step of minimum word error rate training
    (Prabhavalkar et al. 2018), the second stage of an attention model -- the expected number of word (or
    character) errors over an n-best list, plus ce_weight times the masked CE of the reference transcript.
    Optimizer, gradient reduction, status row, the step around the loss and NaN-skip accounting are ASRTrainStep's,
    inherited (its att_on_host switch too: only ASR.forward reads it, which this loss does not call).

    forward_loss: the Listener runs ONCE on the batch (blstm_4 recurs over the utterance axis, so a batch of
    repeated utterances would be encoded differently); a beam search without grad on those very features gives K
    hypotheses per utterance; ssasr_mwer_pack lays them and the reference out as M = K + 1 teacher / label rows per
    utterance, ssasr_edit_score counts every row's errors against its reference; the features are repeated M
    times (ops.rows_repeat) and the decode loop runs teacher-forced over all B * M rows (every step in mode 0,
    whatever model.tf_rate is); ops.mwer_loss weighs the rows.  The reference row is teacher-forced for the CE term
    only: it is not a member of the hypothesis set.  Nothing of the n-best list goes to the host but one integer, the
    longest row's length.

    B * (K + 1) > 32 rows are outside the persistent decode loop's shapes (include/ssasr.h: B <= 32) and take one
    launch per stage and step: slower per row, the same results.  A ctc.JointCTCASR model may be trained, but its
    CTC branch takes no part in this step (the head gets no gradient)."""

    UNITS = {'char': 0, 'word': 1}

    def __init__(self, model, beam_size, ce_weight=0.01, unit='word', lm=None, lm_weight=0.0, max_decoding_steps=200,
                 lr=1.0, eps=1e-8, rho=0.9, grad_clip=5.0, eos=None, space=None, sampling=False, seed=None):
        """beam_size 1 .. 32 (K); ce_weight >= 0; unit 'word' | 'char': whose errors are the risk; lm, lm_weight: a
        charlm.CharLM fused into the SEARCH only (the loss is the model's own likelihood); max_decoding_steps: the
        search's step limit.  eos / space: the Mapper's ids of `>` and ` ` (its fixed alphabet's by default).
        sampling: search() DRAWS the K hypotheses from the model's own distribution (ops.decode_sample at temperature
        1, no LM) instead of searching for them, and the loss weighs them uniformly (ops.mwer_loss, posterior
        'uniform': the score-function estimate of the expected risk's gradient, the set's mean risk as the
        baseline).  The uniforms come from a generator the step owns, seeded with `seed` (None: from torch's global
        generator's seed): the same seed and the same weights give the same samples.  An LM weight is a ValueError
        then: the samples would no longer come from the distribution the loss differentiates, and an
        importance-weighted form is not built."""
        from .asr import EOS_INDEX
        from .preprocess import ALL_CHARS, TOKENS, UNK_TKN
        beam_size = int(beam_size)
        if not 1 <= beam_size <= ops.MAX_BEAM:
            raise ValueError('beam_size must be in 1..%d, got %d' % (ops.MAX_BEAM, beam_size))
        if unit not in self.UNITS:
            raise ValueError("unit must be 'word' or 'char', got %r" % (unit,))
        if not float(ce_weight) >= 0.0:
            raise ValueError('ce_weight must be >= 0, got %r' % (ce_weight,))
        if int(max_decoding_steps) < 1:
            raise ValueError('max_decoding_steps must be >= 1, got %r' % (max_decoding_steps,))
        if sampling and float(lm_weight) != 0.0:
            raise ValueError('sampling draws from the model alone: lm_weight must be 0 with it, got %r' % (lm_weight,))
        if seed is not None and (isinstance(seed, bool) or int(seed) != seed or seed < 0):
            raise ValueError('seed must be None or an integer >= 0, got %r' % (seed,))
        self._set_up_asr(model, lr, eps, rho, grad_clip)
        self.beam_size, self.ce_weight, self.unit = beam_size, float(ce_weight), unit
        self.lm, self.lm_weight, self.max_decoding_steps = lm, float(lm_weight), int(max_decoding_steps)
        self.eos = EOS_INDEX if eos is None else int(eos)
        self.space = (TOKENS + ALL_CHARS).index(' ') if space is None else int(space)
        self.first_char = TOKENS.index(UNK_TKN)             # `<` (the pad) and `>` are dropped before scoring
        self._ref_of = {}
        self.sampling = bool(sampling)
        self.generator = None          # sampling: the source of search()'s uniforms
        if self.sampling:
            self.generator = torch.Generator(device=self.flat.data.device)
            self.generator.manual_seed(torch.initial_seed() if seed is None else int(seed))
        # last_logits: [B * (K + 1), U, V] of the most recent step
        self.last_rows = None          # int32 [B * (K + 1), L]: its teacher / label rows
        self.last_hyps = None          # (chars [B, K, steps], n_chars [B, K], n_hyps [B]) it was given or searched
        self.last_counts = None        # int32 [B * (K + 1), 8]: every row's edit counts against its reference
        self.last_risk = None          # float [B]: the expected risk per utterance, on the device
        self.last_info = None          # ops.MWERInfo of its loss (p_hat, logp, weight, lse)

    def search(self, feat, enc_len_dev):
        """The n-best list of this batch's own features (sampling: K draws per utterance), without grad:
        (chars, n_chars, n_hyps) on the device."""
        with torch.no_grad():
            if self.sampling:
                args = self.model._decode_args(feat.detach(), enc_len_dev, None, 0.0, self.eos, self.max_decoding_steps)
                uniforms = torch.rand(feat.shape[0], self.beam_size, self.max_decoding_steps, device=feat.device,
                                      dtype=torch.float32, generator=self.generator)
                chars, n_chars, _, n_hyps, _ = ops.decode_sample(*args, self.beam_size, uniforms)
            else:
                args = self.model._decode_args(feat.detach(), enc_len_dev, self.lm, self.lm_weight, self.eos,
                                               self.max_decoding_steps)
                chars, n_chars, _, n_hyps = ops.decode_beam(*args, self.beam_size)
        return chars, n_chars, n_hyps

    def _reference_rows(self, B, M, dev):
        """ref_of of the scoring launch: every row of utterance b is scored against row b * M + K."""
        key = (B, M, str(dev))
        if key not in self._ref_of:
            self._ref_of[key] = ((torch.arange(B * M, dtype=torch.int32) // M) * M + (M - 1)).to(dev)
        return self._ref_of[key]

    def forward_loss(self, x, y, x_lens, hyps=None):
        """x [B, T, F], y [B, L] label rows (<sos> column first, 0-padded), x_lens host list (descending).
        hyps: (chars [B, K, steps], n_chars [B, K], n_hyps [B]) int32 device tensors used instead of the search
        (tests, reproducible runs).  Returns (loss, logits [B * (K + 1), U, V])."""
        m = self.model
        feat, _, enc_len_dev, _, _ = m.encode(x, x_lens)                       # 1. encode once, with grad
        if hyps is None:
            hyps = self.search(feat, enc_len_dev)                              # 2. search on these features
        chars, n_chars, n_hyps = [t.to(torch.int32).contiguous() for t in hyps]
        B, K = chars.shape[0], chars.shape[1]
        if B != x.shape[0] or K > ops.MAX_BEAM:
            raise ValueError('MWERTrainStep: hypotheses [%d, %d, ...] for a batch of %d (at most %d per utterance)'
                             % (B, K, x.shape[0], ops.MAX_BEAM))
        M = K + 1
        y32 = ops.as_i32(y)
        rows, hyp_lens = ops.mwer_pack(chars, n_chars, n_hyps, y32, self.eos)  # 3. pack and score
        counts = ops.edit_score(rows[:, 1:], hyp_lens, rows[:, 1:max(y32.shape[1], 2)], hyp_lens,
                                self._reference_rows(B, M, rows.device), first_char=self.first_char,
                                space=self.space, check_ref_of=False)
        # 4. the teacher-forced pass over B * M rows; its length is the one integer the host reads
        U = int(hyp_lens.max()) + 1
        logits, _, _ = ops.decoder_loop(ops.rows_repeat(feat, M), None, ops.rows_repeat(enc_len_dev, M), rows,
                                        [0] * U, None, m._decoder_params(),
                                        psi=(m.attention.psi.weight, m.attention.psi.bias))
        # 5. the reference rows carry the CE: ce_weight / (B denom_b), denom_b = count(y[b] != 0) as in the masked CE
        ce_w = torch.zeros(B, M, device=rows.device, dtype=torch.float32)
        ce_w[:, K] = self.ce_weight / (B * (hyp_lens.view(B, M)[:, K] + 1).clamp(min=1).to(torch.float32))
        loss, info = ops.mwer_loss(logits, rows, n_hyps, counts, self.UNITS[self.unit], ce_w.view(B * M),
                                   posterior='uniform' if self.sampling else 'renorm')
        self.last_rows, self.last_hyps, self.last_counts = rows, (chars, n_chars, n_hyps), counts
        self.last_risk, self.last_info, self.last_logits = info.risk, info, logits
        return loss, logits

    def __call__(self, x, y, x_lens, hyps=None):
        """One train step (ASRTrainStep's, around this loss); returns the loss tensor (on the device)."""
        return super().__call__(x, y, x_lens, hyps)


class TAETrainStep(TrainStep):
    """One TAETrainer step (the body of TAETrainer.exec, src/trainer.py:652-677) as a reusable object: the
    text autoencoder's forward through the shared attend-and-spell loop (text_autoencoder.py), the loss of
    :662-672, backward, gradient all-reduce across ranks, then Solver.step as the reference calls it --
    norm, NaN guard and clip over the TEXT AUTOENCODER's parameters only (:676), Adam (:633-641,
    conf/default.yaml:43-45) over the text autoencoder AND the ASR model's embed / attention / decoder /
    char_trans.  Those shared parameters stay where the ASR model's flat buffer has them (everything behind
    the Listener is one run of it), so an ASRTrainStep and a TAETrainStep over the same ASR object train
    the same storage, in turn: the two legs of the Seed loop (src/trainer.py:1126-1177) this build has."""

    def __init__(self, asr_model, tae_model, lr=1e-4, eps=1e-8, grad_clip=5.0):
        self._models_on_gpu('both models', tae_model, asr_model)
        self.asr, self.tae = asr_model, tae_model
        self.asr_flat = FlatParameters.of(asr_model)
        self.tae_flat = FlatParameters.of(tae_model)
        shared = (list(asr_model.attention.parameters()) + list(asr_model.decoder.parameters()) +
                  list(asr_model.embed.parameters()) + list(asr_model.char_trans.parameters()))
        self.lo, self.hi = self.asr_flat.range_of(shared)
        sdist.broadcast_flat(self.tae_flat.data)
        sdist.broadcast_flat(self.asr_flat.data)
        self.optim = FusedAdam([(self.tae_flat.data, self.tae_flat.grad, True),
                                (self.asr_flat.data[self.lo:self.hi], self.asr_flat.grad[self.lo:self.hi], False)],
                               lr=lr, eps=eps)
        self._set_up([self.tae_flat, self.asr_flat], [('last_done', self.optim)], grad_clip)
        self.last_logits = None

    def forward_loss(self, y, y_noise, decode_step, noise_lens):
        from .text_autoencoder import tae_loss
        _, logits = self.tae(self.asr, y, y_noise, decode_step, noise_lens=noise_lens)
        return tae_loss(logits, y), logits

    def __call__(self, y, y_noise, y_lens, noise_lens):
        """y [B, L] clean label rows, y_noise [B, <= L] noised rows (int64, on the GPU), their prepare_y
        lengths.  Returns the loss tensor."""
        self._open()
        with ops.shared_status_row(self.optim.status_row):
            loss, self.last_logits = self.forward_loss(y, y_noise, max(y_lens), noise_lens)
            loss.backward(self._one)
        scale = sdist.allreduce_grad(self.tae_flat.grad)
        sdist.allreduce_grad(self.asr_flat.grad[self.lo:self.hi])
        # (the Listener's gradients were never touched by this pass: the whole ASR buffer is clean again)
        self._update(scale)
        return loss


class CharLMTrainStep(TrainStep):
    """One CHARLMTrainer step (src/trainer.py:229-251) as a reusable object: the chunk loop as ONE forward
    launch (ops.charlm_chunk; teacher forcing flipped per step on the host as the reference's random.random()
    does, :241, the sampled steps drawn in the kernel from device uniforms), ONE backward launch, the parameter
    gradients as deferred products, then Solver.step -- norm, NaN guard, clip at 5 -- fused with
    torch.optim.Adam(lr, eps=1e-8) (:215-218) over the model's one flat buffer."""

    claims_listener = False            # nothing in its two launches notifies the listener

    def __init__(self, lm, tf_rate, lr=1e-4, eps=1e-8, grad_clip=5.0, opt_type='Adam'):
        if opt_type != 'Adam':
            raise NotImplementedError("char_lm.opt.type '%s': the fused CharLM step has Adam only" % opt_type)
        self._models_on_gpu('the model', lm)
        self.lm, self.tf_rate = lm, float(tf_rate)
        self.flat = FlatParameters.of(lm)
        self.optim = FusedAdam([(self.flat.data, self.flat.grad, True)], lr=lr, eps=eps)
        self._set_up([self.flat], [('last_done', self.optim)], grad_clip)
        self._ws = None
        self.last_chunk = None

    def draw_modes(self, U):
        """0 teacher / 1 sample per step, the reference's coin (src/trainer.py:241)."""
        import random
        return [0 if random.random() <= self.tf_rate else 1 for _ in range(U)]

    def __call__(self, y, modes=None, uniforms=None, feed=None):
        """y [B, U] labels on the GPU.  Returns the loss tensor (mean over the batch of the per-row sums, :249)."""
        self._open()
        B, U = y.shape
        dev = y.device
        if modes is None:
            modes = self.draw_modes(U)
        if not torch.is_tensor(modes):
            sampled = any(modes)
            modes = torch.tensor(modes, dtype=torch.int32).to(dev, non_blocking=True)
            if sampled and uniforms is None:
                uniforms = torch.rand(U, B, device=dev)
        chunk = ops.charlm_chunk(self.lm, y, feed=feed, modes=modes, uniforms=uniforms, ws=self._ws)
        self._ws = chunk.ws
        ops.charlm_chunk_backward(self.lm, chunk, dloss=1.0 / B)
        self.last_chunk = chunk
        self._update(sdist.allreduce_grad(self.flat.grad))
        return chunk.loss_rows.mean()


def label_geometry(y_cpu):
    """prepare_y's lengths on the host (src/ASRDataset.py:338): returns
    (y_lens, ans_len)."""
    y_lens = [int(v) + 1 for v in (y_cpu != 0).sum(-1)]
    return y_lens, max(y_lens) - 1


def _fused_optimizer(kind, flat, span, lr, eps=1e-8):
    """The fused form of torch.optim.<kind>(params, lr=lr, eps=eps) over one run of a flat buffer, with
    Solver.step's clip over that same run; None for a kind this build has no kernel for."""
    lo, hi = span if span is not None else (0, flat.numel)
    if kind == 'Adadelta':
        return FusedAdadelta(flat, lr=lr, eps=eps, span=(lo, hi))
    if kind == 'Adam':
        return FusedAdam([(flat.data[lo:hi], flat.grad[lo:hi], True)], lr=lr, eps=eps)
    return None


class ADVTrainStep(TrainStep):
    """One ADVTrainer iteration (src/trainer.py:968-1032) as a reusable object: the discriminator is trained to
    score the text encoder's frames high (labels 1 - label_smoothing) and the Listener's low (labels 0), then
    the Listener -- the generator -- to be scored high (labels 1) by the UPDATED discriminator; Solver.step
    over the discriminator's parameters with D_opt, then over the Listener's with G_opt.  The reference leaves
    `self.loss_metric` undefined (:984): it is nn.BCELoss here, what
    src/discriminator.py:17-19 describes.

    The Listener runs ONCE per iteration (as in the reference, which reuses `fake_data`'s graph for the
    generator pass); gradients the reference computes and never uses -- the text encoder's from the real
    pass, the discriminator's from the generator pass (zeroed at :975 before anything reads them) -- are not
    computed.  The Listener's parameters stay where the ASR model's flat buffer has them: the other legs of
    the Seed loop train the same storage."""

    def __init__(self, asr_model, tae_model, discriminator, g_opt=('Adadelta', 1.0), d_opt=('Adadelta', 1.0),
                 label_smoothing=0.1, grad_clip=5.0):
        self._models_on_gpu('every model', asr_model, tae_model, discriminator)
        self.asr, self.tae, self.disc = asr_model, tae_model, discriminator
        self.asr_flat = FlatParameters.of(asr_model)
        self.d_flat = FlatParameters.of(discriminator)
        self.span = self.asr_flat.range_of(list(asr_model.encoder.parameters()))
        sdist.broadcast_flat(self.asr_flat.data)
        sdist.broadcast_flat(self.d_flat.data)
        # the text autoencoder is only READ here (its encoder's frames are the discriminator's real data): every
        # rank must read the same one; buffers (none today) ride along
        sdist.broadcast_module(tae_model)
        sdist.broadcast_buffers(asr_model, discriminator)
        self.G_optim = _fused_optimizer(g_opt[0], self.asr_flat, self.span, g_opt[1])
        self.D_optim = _fused_optimizer(d_opt[0], self.d_flat, None, d_opt[1])
        if self.G_optim is None or self.D_optim is None:
            raise NotImplementedError('ADVTrainStep: optimizer types %r / %r (Adadelta and Adam have kernels)'
                                      % (g_opt[0], d_opt[0]))
        self.label_smoothing = float(label_smoothing)
        # D's verdict is polled first; last_done is the generator's (grad norm, skipped) of the last finished iteration
        self._set_up([self.d_flat, self.asr_flat], [('last_done_d', self.D_optim), ('last_done', self.G_optim)], grad_clip)

    def frames(self, x, x_lens, y):
        """The two encoders' frames: (real [B, seq, 512] from the text encoder, no graph; fake [B, T', 512] from
        the Listener, with its graph)."""
        with torch.no_grad():
            real = self.tae.encoder(y)                               # the data distribution, [B, seq, 512]
        fake, _ = self.asr.encoder(x, x_lens)
        return real, fake

    def __call__(self, x, x_lens, y):
        """x [B, T, F] padded fbanks, x_lens host list (descending), y [B, L] label rows (int64), all on
        the GPU.  Returns (D_realloss, D_fakeloss, G_loss) device tensors."""
        from .seed_ops import bce_loss
        self._open()
        lo, hi = self.span
        with ops.shared_status_row(self.G_optim.status_row):
            # --- discriminator: maximise log D(real) + log(1 - D(G(x)))
            real, fake = self.frames(x, x_lens, y)
            d_real = bce_loss(self.disc(real), 1.0 - self.label_smoothing)
            d_real.backward(self._one)
            d_fake = bce_loss(self.disc(fake.detach()), 0.0)
            d_fake.backward(self._one)
            scale = sdist.allreduce_grad(self.d_flat.grad)
            self.D_optim.clip_and_step(self.grad_clip, grad_scale=scale, zero_grad=True)
            self.d_flat.clean = True
            # --- generator: maximise log D(G(x)), through the discriminator just updated
            g_loss = bce_loss(self.disc(fake, frozen=True), 1.0)
            g_loss.backward(self._one)
        # G_optim's update; nothing behind the Listener was touched by this pass, and the frozen discriminator of the
        # generator pass took no gradient: both buffers are clean
        self._update(sdist.allreduce_grad(self.asr_flat.grad[lo:hi]))
        return d_real, d_fake, g_loss


class SAETrainStep(TrainStep):
    """One SAETrainer iteration (src/trainer.py:803-820) as a reusable object: the shared Listener, the speech
    autoencoder over its output and the raw frames, smooth-L1 against the input frames (:811-818), backward,
    gradient all-reduce, then Solver.step as the reference calls it -- norm, NaN guard and clip over the SPEECH
    AUTOENCODER's parameters only (:820), Adam (:789-794, conf/default.yaml:24-26) over them AND the Listener.
    The Listener's parameters stay where the ASR model's flat buffer has them (its first run): the other legs of
    the Seed loop train the same storage.  Batch-norm running statistics are per rank (the reference is
    single-device; they do not enter the training arithmetic)."""

    def __init__(self, asr_model, sae_model, opt=('Adam', 1e-4), grad_clip=5.0):
        self._models_on_gpu('both models', sae_model, asr_model)
        if opt[0] != 'Adam':
            raise NotImplementedError('SAETrainStep: optimizer type %r (Adam has the kernel whose clipped range may '
                                      'differ from its update range)' % (opt[0],))
        self.asr, self.sae = asr_model, sae_model
        self.asr_flat = FlatParameters.of(asr_model)
        self.sae_flat = FlatParameters.of(sae_model)
        self.lo, self.hi = self.asr_flat.range_of(list(asr_model.encoder.parameters()))
        sdist.broadcast_flat(self.sae_flat.data)
        sdist.broadcast_flat(self.asr_flat.data)
        sdist.broadcast_buffers(sae_model)     # batch-norm running statistics start from rank 0's (then evolve per rank)
        self.optim = FusedAdam([(self.sae_flat.data, self.sae_flat.grad, True),
                                (self.asr_flat.data[self.lo:self.hi], self.asr_flat.grad[self.lo:self.hi], False)],
                               lr=opt[1], eps=1e-8)
        self._set_up([self.sae_flat, self.asr_flat], [('last_done', self.optim)], grad_clip)
        # SSASR_SAE_OVERLAP: 0 the speech encoder behind the Listener on one stream, 1 / 2 see forward_loss (same results)
        self.overlap = int(os.environ.get('SSASR_SAE_OVERLAP', '1'))
        self.last_pred = None          # [B, 8 T', F] of the most recent step (for the trainer's figures)

    def forward_loss(self, x, x_lens):
        """Listener and global speech encoder both read the fbanks and nothing of each other.  With `overlap` the speech
        encoder runs on the second stream -- 1: its forward still AFTER the Listener's, its backward (autograd runs a
        node on its forward's stream; created after the Listener's nodes it comes first in autograd's order) beside the
        Listener's BPTT; 2: its forward beside the Listener's too (measured: the first layer's recurrence then takes
        2.42 instead of 1.44 ms -- a loss).  The frame decoder waits for both.  A caller that runs forward_loss + backward by
        itself with overlap on must call ops.join_side_stream() before it reads sae_flat.grad (__call__ does)."""
        from .seed_ops import sae_loss
        if not (self.overlap and x.is_cuda):
            listener_out, _ = self.asr.encoder(x, x_lens)
            pred = self.sae(x, listener_out)
            return sae_loss(pred, x, max(x_lens)), pred
        cur, side = torch.cuda.current_stream(), ops.side_stream()
        ready = torch.cuda.Event()
        ready.record(cur)                                  # x (and the zeroed gradient buffers) are final here
        listener_out, _ = self.asr.encoder(x, x_lens)
        if self.overlap == 2:
            side.wait_event(ready)
        else:
            side.wait_stream(cur)
        with torch.cuda.stream(side):
            enc = self.sae.encoder(x)
        cur.wait_stream(side)
        enc.record_stream(cur)
        pred = self.sae.decode_frames(enc, listener_out)
        return sae_loss(pred, x, max(x_lens)), pred

    def __call__(self, x, x_lens):
        """x [B, T, F] padded fbanks on the GPU (T: the corpus' padding, >= max(x_lens)), x_lens host list
        (descending).  Returns the loss tensor."""
        self._open()
        with ops.shared_status_row(self.optim.status_row):
            loss, self.last_pred = self.forward_loss(x, x_lens)
            loss.backward(self._one)
        # the speech encoder's backward ran on the second stream and wrote its parameter gradients through sinks
        # (autograd's end-of-backward stream sync does not cover them): joined HERE, not left to the next reader
        ops.join_side_stream()
        scale = sdist.allreduce_grad(self.sae_flat.grad)
        sdist.allreduce_grad(self.asr_flat.grad[self.lo:self.hi])
        self._update(scale)            # (nothing behind the Listener was touched: the whole ASR buffer is clean again)
        return loss
