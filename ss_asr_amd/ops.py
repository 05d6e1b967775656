"""torch.autograd bindings of the HIP kernels (C ABI: include/ssasr.h).

Every function here runs on a CUDA(=HIP) device tensor through
libssasr_hip.so.  There is no CPU implementation: calling these with CPU
tensors, or without the shared object, raises.
"""
import ctypes as C
import math
import os
import weakref

import torch

from . import _lib
from ._lib import check


_persist_status = []     # int32[8] workspaces of persistent launches not yet checked
TIMEOUT_MESSAGE = 'ss_asr_amd: a persistent recurrence / decode loop timed out'
_KERNELS = {1: 'encoder forward recurrence', 2: 'encoder BPTT',
            4: 'decode loop forward', 5: 'decoder backward chain', 6: 'split-T attention step'}


def describe_status(words):
    """Message for non-zero status words of persistent launches (csrc/rnn_kernels.h, persist_code):
    which kernel, workgroup and step gave up waiting first."""
    parts = []
    for v in words:
        v = int(v) & 0xffffffff
        if v == 0:
            continue
        if v & 0x40000000:
            step = v & 0xfff
            parts.append('%s, workgroup %d, %s' % (_KERNELS.get((v >> 24) & 0x3f, 'kernel %d' % ((v >> 24) & 0x3f)),
                                                    (v >> 12) & 0xfff, 'step %d' % step if step != 0xfff else 'step unknown'))
        else:
            parts.append('status %d' % v)
    return TIMEOUT_MESSAGE + (' (' + '; '.join(parts) + ')' if parts else '')


def check_persistent_status():
    """Raises if any persistent kernel launched since the last call timed out
    waiting for its peers (synchronises the device).  For callers that drive the ops
    themselves; a train step (engine.ASRTrainStep) gets the same verdict without a
    synchronisation from the status row that travels with its optimizer statistics."""
    global _persist_status
    pending, _persist_status = _persist_status, []
    if pending:
        words = torch.stack([t[i] for t, i in pending]).cpu().tolist()
        if any(words):
            raise RuntimeError(describe_status(words))


_status_pools = {}
_shared_status = None    # one int32[8] row for every persistent launch of the step in progress


class shared_status_row:
    """Context manager: every persistent launch inside it reports into `row` (int32[8] on the
    device, zero on entry) instead of a row of its own.  The launches only ever write a time-out
    code into words 4 / 5 (first failure wins), so the launches of a whole train step can share one
    row, which the caller then reads back with its other per-step statistics (no extra copy, no
    synchronisation)."""

    def __init__(self, row):
        self.row = row

    def __enter__(self):
        global _shared_status
        self.prev = _shared_status
        _shared_status = self.row
        return self

    def __exit__(self, *exc):
        global _shared_status
        _shared_status = self.prev
        return False


def _status_words(device):
    """int32[8] status / counter words for one persistent launch, zero on entry as the C ABI
    asks.  Rows of one zero-initialised pool are handed out in turn, so that no fill kernel
    runs per launch; a row is reused after 4096 launches and still holds zeros unless a
    launch timed out (check_persistent_status() reports that, and it is fatal anyway)."""
    if _shared_status is not None:
        return _shared_status
    key = str(device)
    pool = _status_pools.get(key)
    if pool is None:
        pool = _status_pools[key] = [torch.zeros(4096, 8, device=device, dtype=torch.int32), 0]
    row = pool[0][pool[1]]
    pool[1] = (pool[1] + 1) % 4096
    return row


def _track_status(sync, index):
    """Remembers a status word for check_persistent_status(); checks by itself
    before the list grows without bound (a caller that never checks)."""
    if sync is _shared_status:
        return                      # its owner reads it back
    _persist_status.append((sync, index))
    if len(_persist_status) > 4096:
        check_persistent_status()


_events = None
# step ranges per BiLSTM layer whose weight gradients overlap the recurrence (1..8)
bptt_segments = int(os.environ.get('SSASR_BPTT_SEGMENTS', '4'))


def _overlap_events():
    """The caller-owned event set of ssasr_bilstm_bwd_overlapped (one per process: autograd's
    backward runs the layers one after another on one thread)."""
    global _events
    if _events is None:
        h = C.c_void_p()
        check(_lib.load().ssasr_events_create(C.byref(h)), 'ssasr_events_create')
        _events = h
    return _events


# ---- weight-gradient overlap ------------------------------------------------
# Weight gradients are off the critical path of backward.  For parameters whose
# .grad lives in an optimizer-owned flat buffer (optim.FlatParameters marks
# them), the BiLSTM backward enqueues its weight-gradient GEMMs on a second
# stream and accumulates straight into .grad, while the main stream goes on
# with the next layer's recurrence.  join_side_stream() must run before
# anything reads the gradients (FusedAdadelta.clip_and_step does).
_side = None


def side_stream():
    global _side
    if _side is None:
        _side = torch.cuda.Stream()
    return _side


def join_side_stream():
    if _side is not None:
        torch.cuda.current_stream().wait_stream(_side)


_SENTINEL_I32 = 0x7FC0DEAD        # PERSIST_SENTINEL (csrc/rnn_kernels.h): the exchange fill pattern


class ExchangeArena:
    """Exchange workspaces of one pass over the model (all forward images, or all BPTT rings),
    laid out back to back and armed with ONE fill: every slot is reserved before the first one
    is taken; the calls that receive a slot are told so with their `armed` argument."""

    def __init__(self, device):
        self.device, self.sizes, self.offsets, self.buf = device, [], None, None

    def reserve(self, floats):
        assert self.buf is None, 'reserve every slot before taking the first'
        self.sizes.append((int(floats) + 63) & ~63)
        return len(self.sizes) - 1

    def take(self, slot):
        if self.buf is None:
            self.offsets = [0]
            for n in self.sizes:
                self.offsets.append(self.offsets[-1] + n)
            self.buf = torch.empty(self.offsets[-1], device=self.device, dtype=torch.float32)
            self.buf.view(torch.int32).fill_(_SENTINEL_I32)
            self.taken = set()
        view = self.buf[self.offsets[slot]:self.offsets[slot] + self.sizes[slot]]
        if slot in self.taken:          # a second pass over the same graph (retain_graph): arm it again
            view.view(torch.int32).fill_(_SENTINEL_I32)
        self.taken.add(slot)
        return view


def bilstm_exchange_floats(S, N, H):
    """(forward image floats, BPTT ring floats) of a BiLSTM layer; 0 where the layer has no
    persistent form that an ExchangeArena can serve."""
    lib = _lib.load()
    return int(lib.ssasr_bilstm_fwd_hx_floats(S, N, H)), int(lib.ssasr_bilstm_bwd_ring_floats(S, N, H, 2))


def upload_i32(device, *seqs):
    """Host integer sequences -> int32 device tensors, all through ONE pinned staging buffer
    and one asynchronous copy (a copy from pageable memory waits for the stream to drain;
    one copy per sequence costs a dispatch each).  Returns one tensor per sequence."""
    flat = [int(v) for s in seqs for v in s]
    t = torch.tensor(flat, dtype=torch.int32)
    if torch.device(device).type == 'cuda':
        t = t.pin_memory().to(device, non_blocking=True)
    else:
        t = t.to(device)
    out, o = [], 0
    for s in seqs:
        out.append(t[o:o + len(s)])
        o += len(s)
    return out


_wgrad_listener = None


def set_wgrad_listener(fn):
    """fn(list of gradient tensors) is called whenever deferred weight gradients have
    been enqueued on the side stream (dist.GradReducer overlaps its all-reduce with the
    rest of the backward pass from that)."""
    global _wgrad_listener
    _wgrad_listener = fn


def _notify_wgrad(sinks):
    if _wgrad_listener is not None:
        _wgrad_listener(sinks)


def _grad_sinks(params):
    """The .grad tensors to accumulate into, or None if any parameter is not
    managed by a flat gradient buffer."""
    sinks = []
    for p in params:
        if not getattr(p, '_ssasr_flat_grad', False) or p.grad is None:
            return None
        sinks.append(p.grad)
    return sinks


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _need_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError('ss_asr_amd ops need tensors on the GPU (no CPU path); got %s'
                               % t.device)


def _f32c(t):
    if t.dtype != torch.float32:
        raise TypeError('expected float32, got %s' % t.dtype)
    return t if t.is_contiguous() else t.contiguous()


# ---------------------------------------------------------------------------
# plain GEMM (no autograd): C = act(alpha * op(A) op(B) + bias) + beta * C
# ---------------------------------------------------------------------------
def gemm(a, b, ta=False, tb=False, out=None, bias=None, act=0, alpha=1.0, beta=0.0, splitk=1):
    """2-D or batched 3-D fp32 GEMM on the MFMA kernel.  ``tb=False`` means b is
    stored [N, K] (the torch Linear weight layout)."""
    lib = _lib.load()
    _need_gpu(a, b)
    a, b = _f32c(a), _f32c(b)
    batched = a.dim() == 3
    am, bm = (a[0], b[0]) if batched else (a, b)
    M, K = (am.shape[1], am.shape[0]) if ta else (am.shape[0], am.shape[1])
    N = bm.shape[1] if tb else bm.shape[0]
    kb = bm.shape[0] if tb else bm.shape[1]
    if kb != K:
        raise ValueError('gemm: inner dimensions differ (%d vs %d)' % (K, kb))
    batch = a.shape[0] if batched else 1
    if out is None:
        shape = (batch, M, N) if batched else (M, N)
        out = (torch.zeros if splitk > 1 else torch.empty)(shape, device=a.device,
                                                           dtype=torch.float32)
    check(lib.ssasr_gemm_f32(int(ta), int(tb), M, N, K, alpha, _p(a), am.stride(0), _p(b),
                             bm.stride(0), beta, _p(out), out.stride(-2), _p(bias), act, batch,
                             a.stride(0) if batched else 0, b.stride(0) if batched else 0,
                             out.stride(0) if batched else 0, splitk, _stream()), 'ssasr_gemm_f32')
    return out


# ---------------------------------------------------------------------------
# bidirectional LSTM layer (packed semantics)
# ---------------------------------------------------------------------------
class _BiLSTM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, lens, steps, batch_first, sinks, slots, *w):
        lib = _lib.load()
        _need_gpu(x, *w)
        ctx.sinks = sinks
        ctx.slots = slots
        # an input may come with its own strides (pBLSTM.downsample's view of an
        # odd-length layer output: rows of 2F floats, utterances T * F apart): the kernels take strides, no copy
        strided = (x.dtype == torch.float32 and x.dim() == 3 and x.stride(2) == 1 and
                   x.stride(1) % 4 == 0 and x.stride(0) % 4 == 0 and x.stride(1) >= x.shape[2] and
                   x.stride(0) >= x.shape[1] * x.stride(1) and x.data_ptr() % 16 == 0)
        if not strided:
            x = _f32c(x)
        w = [_f32c(t) for t in w]
        H = w[1].shape[1]
        I = x.shape[2]
        if batch_first:
            N, S = x.shape[0], int(steps)
            xs_s, xs_n = x.stride(1), x.stride(0)
            y = torch.empty(N, S, 2 * H, device=x.device, dtype=torch.float32)
            ys_s, ys_n = 2 * H, S * 2 * H
        else:
            S, N = x.shape[0], x.shape[1]
            xs_s, xs_n = x.stride(0), x.stride(1)
            y = torch.empty(S, N, 2 * H, device=x.device, dtype=torch.float32)
            ys_s, ys_n = N * 2 * H, 2 * H
        gates = torch.empty(2, S * N, 4 * H, device=x.device, dtype=torch.float32)
        hs = torch.empty(2, S * N, H, device=x.device, dtype=torch.float32)
        # what the BPTT streams back (activated gates, cell states): tile-major when the layer takes
        # both persistent forms (include/ssasr.h, tsave), else row-major in gates / cs
        ts_floats = int(lib.ssasr_bilstm_tsave_floats(S, N, H))
        tsave = torch.empty(ts_floats, device=x.device, dtype=torch.float32) if ts_floats else None
        cs = None if ts_floats else torch.empty(2, S * N, H, device=x.device, dtype=torch.float32)
        # workspaces of the persistent recurrence (exchange image + counters)
        hx_floats = int(lib.ssasr_bilstm_fwd_hx_floats(S, N, H))
        armed = 0
        if slots is not None and slots[1] is not None and hx_floats:
            hx = slots[0].take(slots[1])              # armed with the arena's one fill
            assert hx.numel() >= hx_floats
            armed = 1
        else:
            hx = torch.empty(hx_floats, device=x.device, dtype=torch.float32) if hx_floats else None
        sync = _status_words(x.device) if hx is not None else None
        check(lib.ssasr_bilstm_fwd(_p(x), xs_s, xs_n, S, N, I, H, _p(lens), *[_p(t) for t in w],
                                   _p(y), ys_s, ys_n, _p(gates), _p(cs), _p(hs), _p(hx), _p(sync),
                                   armed, _p(tsave), _stream()), 'ssasr_bilstm_fwd')
        if sync is not None:
            _track_status(sync, 4)
        ctx.save_for_backward(x, lens, gates, cs, hs, tsave, *w)
        ctx.geom = (S, N, I, H, xs_s, xs_n, ys_s, ys_n, bool(batch_first))
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        if getattr(ctx, 'consumed', False):
            raise RuntimeError('bilstm: the saved gates were overwritten with their derivatives by the first '
                               'backward pass; a second pass over the same graph (retain_graph) is not supported')
        ctx.consumed = True
        x, lens, gates, cs, hs, tsave, *w = ctx.saved_tensors
        S, N, I, H, xs_s, xs_n, ys_s, ys_n, batch_first = ctx.geom
        dy = _f32c(dy)
        dev = x.device
        need_dx = ctx.needs_input_grad[0]
        dx = None
        if need_dx:
            # frames past `steps` of a batch-first input get no gradient
            full = (not batch_first) or x.shape[1] == S
            dx = (torch.empty if full else torch.zeros)(x.shape, device=dev, dtype=torch.float32)     # (contiguous whatever x's strides)
        dxs_s, dxs_n = (I, x.shape[1] * I) if batch_first else (N * I, I)
        sinks = ctx.sinks
        if sinks is None:
            dw = [torch.empty_like(w[0]), torch.empty_like(w[1]), torch.empty(4 * H, device=dev),
                  torch.empty_like(w[4]), torch.empty_like(w[5]), torch.empty(4 * H, device=dev)]
        else:
            dw = [None] * 6          # deferred: ssasr_bilstm_wgrad on the side stream
        ws_t = torch.empty(2, H, 4 * H, device=dev)
        ws_dc = torch.empty(2, 2, N, H, device=dev)
        # workspaces of the persistent BPTT (exchange image + counters)
        slots = ctx.slots
        armed = slots is not None and slots[3] is not None and int(lib.ssasr_bilstm_bwd_ring_floats(S, N, H, 2)) > 0
        if armed:
            gx = slots[2].take(slots[3])              # the K-split ring, armed with the arena's one fill
        else:
            gx_floats = int(lib.ssasr_bilstm_bwd_gx_floats(S, N, H))
            gx = torch.empty(gx_floats, device=dev, dtype=torch.float32) if gx_floats else None
        sync = _status_words(dev) if gx is not None else None
        if sync is not None:
            _track_status(sync, 4)
        if sinks is not None:
            # Weight gradients go to the side stream, accumulated into the flat gradient
            # buffer.  The BPTT is cut into 4 segments whose weight-gradient GEMMs start
            # while the next segment recurs: the first layer is the last of the backward
            # pass and nothing else would run beside its GEMMs (measured +2 % with 4
            # segments on every layer, against +0.7 % on the first only).
            segments = bptt_segments
            side = side_stream()
            check(lib.ssasr_bilstm_bwd_overlapped(
                _p(dy), ys_s, ys_n, _p(x), xs_s, xs_n, S, N, I, H, _p(lens), _p(w[0]), _p(w[1]), _p(w[4]),
                _p(w[5]), _p(gates), _p(cs), _p(hs), _p(dx), dxs_s, dxs_n, *[_p(t) for t in sinks], _p(ws_t),
                _p(ws_dc), _p(gx), _p(sync), int(armed), _p(tsave), segments, _overlap_events(), _stream(),
                C.c_void_p(side.cuda_stream)), 'ssasr_bilstm_bwd_overlapped')
            for t in (gates, x, hs):
                t.record_stream(side)
            _notify_wgrad(sinks)
            return (dx,) + (None,) * 13
        check(lib.ssasr_bilstm_bwd(_p(dy), ys_s, ys_n, _p(x), xs_s, xs_n, S, N, I, H, _p(lens),
                                   _p(w[0]), _p(w[1]), _p(w[4]), _p(w[5]), _p(gates), _p(cs),
                                   _p(hs), _p(dx), dxs_s, dxs_n, *[_p(t) for t in dw], _p(ws_t),
                                   _p(ws_dc), _p(gx), _p(sync), int(armed), _p(tsave), _stream()), 'ssasr_bilstm_bwd')
        # inputs: x, lens, steps, batch_first, sinks, slots, then w_ih,w_hh,b_ih,b_hh per direction
        return (dx, None, None, None, None, None, dw[0], dw[1], dw[2], dw[2].clone(),
                dw[3], dw[4], dw[5], dw[5].clone())


def bilstm(x, lens, steps, batch_first, weights, slots=None):
    """weights = (w_ih, w_hh, b_ih, b_hh) forward then the same four reverse.
    batch_first: x [N, T, I], the first ``steps`` frames are processed and the
    result is [N, steps, 2H]; otherwise x is [S, N, I] -> [S, N, 2H].
    lens: int32 device tensor [N] or None.
    slots: (forward ExchangeArena, slot, backward ExchangeArena, slot) reserved with the sizes of
    bilstm_exchange_floats, or None (the layer allocates and arms its own workspaces).
    """
    return _BiLSTM.apply(x, lens, steps, batch_first, _grad_sinks(weights), slots, *weights)


# ---------------------------------------------------------------------------
# attention: cached projection, single step
# ---------------------------------------------------------------------------
class _AttnPrecompute(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, w_psi, b_psi):
        lib = _lib.load()
        _need_gpu(feat, w_psi, b_psi)
        feat, w_psi, b_psi = _f32c(feat), _f32c(w_psi), _f32c(b_psi)
        B, T, E = feat.shape
        A = w_psi.shape[0]
        comp = torch.empty(B, T, A, device=feat.device, dtype=torch.float32)
        check(lib.ssasr_attn_precompute_fwd(_p(feat), _p(w_psi), _p(b_psi), B * T, E, A, _p(comp),
                                            _stream()), 'ssasr_attn_precompute_fwd')
        ctx.save_for_backward(feat, w_psi, comp)
        return comp

    @staticmethod
    def backward(ctx, dcomp):
        lib = _lib.load()
        feat, w_psi, comp = ctx.saved_tensors
        B, T, E = feat.shape
        A = w_psi.shape[0]
        dpre = dcomp.contiguous().clone()
        dfeat = torch.zeros_like(feat)
        dw = torch.empty_like(w_psi)
        db = torch.empty(A, device=feat.device, dtype=torch.float32)
        check(lib.ssasr_attn_precompute_bwd(_p(dpre), _p(comp), _p(feat), _p(w_psi), B * T, E, A,
                                            _p(dfeat), _p(dw), _p(db), _stream()),
              'ssasr_attn_precompute_bwd')
        return dfeat, dw, db


def attn_precompute(feat, w_psi, b_psi):
    """tanh(psi(feat)), src/asr.py:381."""
    return _AttnPrecompute.apply(feat, w_psi, b_psi)


class _AttnStep(torch.autograd.Function):
    @staticmethod
    def forward(ctx, state, w_phi, comp, feat, enc_len):
        lib = _lib.load()
        _need_gpu(state, w_phi, comp, feat, enc_len)
        state, w_phi, comp, feat = _f32c(state), _f32c(w_phi), _f32c(comp), _f32c(feat)
        B, T, E = feat.shape
        A, D = w_phi.shape
        q = torch.empty(B, A, device=feat.device)
        att = torch.empty(B, T, device=feat.device)
        cx = torch.empty(B, E, device=feat.device)
        ws, phase = attn_workspace(B, T, A, E, feat.device)
        sync = _status_words(feat.device) if ws is not None else None
        check(lib.ssasr_attn_step_fwd(_p(state), _p(w_phi), _p(comp), _p(feat), _p(enc_len), B, T,
                                      A, E, D, _p(q), _p(att), _p(cx), _p(ws), phase,
                                      None if sync is None else C.c_void_p(sync.data_ptr() + 20), _stream()),
              'ssasr_attn_step_fwd')
        if ws is not None:
            attn_workspace_advance(B, T, A, E, feat.device, 1)     # only a launch that happened moves the phase
            _track_status(sync, 5)
        ctx.save_for_backward(state, w_phi, comp, feat, enc_len, q, att)
        return att, cx

    @staticmethod
    def backward(ctx, datt, dctx):
        lib = _lib.load()
        state, w_phi, comp, feat, enc_len, q, att = ctx.saved_tensors
        B, T, E = feat.shape
        A, D = w_phi.shape
        dctx = _f32c(dctx) if dctx is not None else torch.zeros(B, E, device=feat.device)
        datt = _f32c(datt) if datt is not None else None
        de = torch.empty(B, T, device=feat.device)
        dqpre = torch.empty(B, A, device=feat.device)
        check(lib.ssasr_attn_step_bwd(_p(dctx), _p(datt), _p(att), _p(q), _p(comp), _p(feat),
                                      _p(enc_len), B, T, A, E, _p(de), _p(dqpre), _stream()),
              'ssasr_attn_step_bwd')
        dstate = gemm(dqpre, w_phi, tb=True)                       # [B,A] . [A,D]
        dw_phi = gemm(dqpre, state, ta=True, tb=True)              # [A,B] . [B,D]
        # outer products per utterance: K = 1 batched GEMMs
        dcomp = gemm(de.unsqueeze(1), q.unsqueeze(1), ta=True, tb=True)        # [B,T,A]
        dfeat = gemm(att.unsqueeze(1), dctx.unsqueeze(1), ta=True, tb=True)    # [B,T,E]
        return dstate, dw_phi, dcomp, dfeat, None


_attn_ws = {}


def _attn_ws_key(B, T, A, E, device):
    return (str(device), torch.cuda.current_stream(device).cuda_stream, B, T, A, E)


def attn_workspace(B, T, A, E, device):
    """(workspace, phase of the next call) of the split-T attention kernel for a shape on the
    current stream, or (None, 0) when the library does not take that form (shape, options,
    residency: ssasr_attn_step_ws_floats).  The workspace is two exchange buffers armed with the
    fill pattern once and then reused by every call of that (stream, shape): a call exchanges
    through buffer `phase` and re-arms the other (include/ssasr.h), so consecutive calls alternate.
    The phase only moves through attn_workspace_advance(), which callers invoke AFTER the library
    accepted their launches; with a workspace the library launches the split form or fails."""
    n = int(_lib.load().ssasr_attn_step_ws_floats(B, T, A, E))
    if n == 0:
        return None, 0
    key = _attn_ws_key(B, T, A, E, device)
    ent = _attn_ws.get(key)
    if ent is None or ent[0].numel() != n:          # (a changed SSASR_ATTN_RPH changes the record count)
        ws = torch.empty(n, device=device, dtype=torch.float32)
        ws.view(torch.int32).fill_(_SENTINEL_I32)
        ent = _attn_ws[key] = [ws, 0]
    return ent[0], ent[1]


def attn_workspace_advance(B, T, A, E, device, calls):
    """Records that `calls` consecutive split-T launches (phase, phase + 1, ...) were enqueued on
    the current stream's workspace of this shape."""
    ent = _attn_ws[_attn_ws_key(B, T, A, E, device)]
    ent[1] = (ent[1] + calls) & 1


def attn_step(state, w_phi, comp, feat, enc_len):
    """One Attention.forward after the cache exists (src/asr.py:383-390)."""
    return _AttnStep.apply(state, w_phi, comp, feat, enc_len)


# ---------------------------------------------------------------------------
# single LSTM cell step
# ---------------------------------------------------------------------------
class _LSTMCell(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, h, c, w_ih, w_hh, b_ih, b_hh):
        lib = _lib.load()
        _need_gpu(x, h, c, w_ih, w_hh, b_ih, b_hh)
        x, h, c = _f32c(x), _f32c(h), _f32c(c)
        w_ih, w_hh, b_ih, b_hh = _f32c(w_ih), _f32c(w_hh), _f32c(b_ih), _f32c(b_hh)
        N, I = x.shape
        H = w_hh.shape[1]
        gates = torch.empty(N, 4 * H, device=x.device)
        h1 = torch.empty(N, H, device=x.device)
        c1 = torch.empty(N, H, device=x.device)
        check(lib.ssasr_lstm_cell_fwd(_p(x), I, I, None, 0, 0, _p(h), _p(c), _p(w_ih), _p(w_hh),
                                      _p(b_ih), _p(b_hh), N, H, _p(gates), _p(h1), _p(c1),
                                      _stream()), 'ssasr_lstm_cell_fwd')
        ctx.save_for_backward(x, h, c, w_ih, w_hh, gates, c1)
        return h1, c1

    @staticmethod
    def backward(ctx, dh1, dc1):
        lib = _lib.load()
        x, h, c, w_ih, w_hh, gates, c1 = ctx.saved_tensors
        N, H = h.shape
        dh1 = _f32c(dh1) if dh1 is not None else torch.zeros_like(h)
        dc1 = _f32c(dc1) if dc1 is not None else None
        dg = torch.empty_like(gates)
        dc = torch.empty_like(c)
        check(lib.ssasr_lstm_cell_bwd(_p(dh1), _p(dc1), _p(gates), _p(c), _p(c1), N, H, _p(dg),
                                      _p(dc), _stream()), 'ssasr_lstm_cell_bwd')
        dx = gemm(dg, w_ih, tb=True)
        dh = gemm(dg, w_hh, tb=True)
        dw_ih = gemm(dg, x, ta=True, tb=True)
        dw_hh = gemm(dg, h, ta=True, tb=True)
        db = dg.sum(0)
        return dx, dh, dc, dw_ih, dw_hh, db, db.clone()


def lstm_cell(x, h, c, w_ih, w_hh, b_ih, b_hh):
    """nn.LSTMCell step (src/asr.py:320-324) -> (h', c')."""
    return _LSTMCell.apply(x, h, c, w_ih, w_hh, b_ih, b_hh)


# ---------------------------------------------------------------------------
# fused decode loop
# ---------------------------------------------------------------------------
_DEC_PARAMS = ('w_phi', 'w_ih1', 'w_hh1', 'b_ih1', 'b_hh1', 'w_ih2', 'w_hh2', 'b_ih2', 'b_hh2',
               'embed', 'w_ct', 'b_ct')


class _DecoderLoop(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, comp, enc_len, teacher, step_mode, uniforms, sinks, modes_dev, slots, *params):
        lib = _lib.load()
        ctx.sinks = sinks
        ctx.set_materialize_grads(False)      # no zero tensors for the att / chars outputs
        _need_gpu(feat, enc_len, *params)
        feat = _f32c(feat)
        params = [_f32c(t) for t in params]
        pw = dict(zip(_DEC_PARAMS, params))
        dev = feat.device
        B, T, E = feat.shape
        A, D = pw['w_phi'].shape
        ctx.psi = len(params) == len(_DEC_PARAMS) + 2
        if ctx.psi:
            # comp = tanh(psi(feat)) (src/asr.py:381) belongs to this node: its backward then
            # adds into the decoder's dfeat and into the flat gradients instead of going
            # through three autograd accumulations
            w_psi, b_psi = params[-2:]
            comp = torch.empty(B, T, A, device=dev, dtype=torch.float32)
            check(lib.ssasr_attn_precompute_fwd(_p(feat), _p(w_psi), _p(b_psi), B * T, E, A, _p(comp),
                                                _stream()), 'ssasr_attn_precompute_fwd')
        else:
            _need_gpu(comp)
            comp = _f32c(comp)
        V = pw['w_ct'].shape[0]
        U = len(step_mode)
        f = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)
        bufs = dict(logits=f(B, U, V), att=f(B, U, T), w_phi_t=f(D, A), q=f(U, B, A),
                    emb_in=f(U + 1, B, D),
                    chars=torch.empty(U + 1, B, device=dev, dtype=torch.int32),
                    gates1=f(U, B, 4 * D), c1=f(U, B, D), h1=f(U, B, D),
                    gates2=f(U, B, 4 * D), c2=f(U, B, D), h2=f(U, B, D))
        geom = _decoder_fwd_ws(B, T, U, A, E, D, V)
        if geom is not None:
            # workspaces of the persistent decode loop: the exchange images back to back, the context
            # rows behind them, then (long encoder outputs) the record ring -- all start as the fill
            # pattern, one fill instead of four
            nh, nq, npart = geom
            nimg, nctx = 2 * nh + nq, U * B * E
            if slots is not None and slots.get('fwd') is not None:
                img = slots['fwd_arena'].take(slots['fwd'])[:nimg + nctx + npart]     # armed by the arena
                assert img.numel() == nimg + nctx + npart
                ctx_armed = True
            else:
                img = f(nimg + nctx + npart)
                ctx_armed = False
            bufs.update(ws_hx1=img[:nh], ws_hx2=img[nh:2 * nh], ctx=img[nimg:nimg + nctx].view(U, B, E),
                        ws_modes=modes_dev if modes_dev is not None else
                        torch.empty(U, device=dev, dtype=torch.int32),
                        ws_sync=_status_words(dev))
            if nq:
                bufs['ws_qx'] = img[2 * nh:nimg]
            if npart:
                bufs['ws_part'] = img[nimg + nctx:]
            _track_status(bufs['ws_sync'], 5)
        if 'ctx' not in bufs:
            bufs['ctx'] = f(U, B, E)
            ws_attn, attn_phase = attn_workspace(B, T, A, E, dev)     # per-step loop, long encoder outputs
            if ws_attn is not None:
                bufs['ws_attn'] = ws_attn
                bufs['ws_sync'] = _status_words(dev)
                _track_status(bufs['ws_sync'], 5)
        modes = (C.c_int32 * U)(*[int(m) for m in step_mode])
        d = _lib.Decoder()
        d.B, d.T, d.E, d.A, d.D, d.V, d.U = B, T, E, A, D, V, U
        d.feat, d.comp, d.enc_len = feat.data_ptr(), comp.data_ptr(), enc_len.data_ptr()
        if teacher is not None:
            teacher = teacher.contiguous()
            d.teacher, d.teacher_ld = teacher.data_ptr(), teacher.stride(0)
        d.step_mode = C.cast(modes, C.c_void_p)
        d.modes_ready = 1 if modes_dev is not None else 0
        if uniforms is not None:
            d.uniforms = uniforms.data_ptr()
        for k, t in pw.items():
            setattr(d, k, t.data_ptr())
        for k, t in bufs.items():
            setattr(d, k, t.data_ptr())
        d.ws_armed = 1 if ('ws_hx1' in bufs and ctx_armed) else 0
        d.ws_attn_phase = attn_phase if 'ws_attn' in bufs else 0
        check(lib.ssasr_decoder_fwd(C.byref(d), _stream()), 'ssasr_decoder_fwd')
        if 'ws_attn' in bufs:
            attn_workspace_advance(B, T, A, E, dev, U)
        ctx.dec = d
        ctx.slots = slots
        ctx.keep = (feat, comp, enc_len, teacher, modes, uniforms, params, bufs)
        ctx.mark_non_differentiable(bufs['att'])
        return bufs['logits'], bufs['att'], bufs['chars']

    @staticmethod
    def backward(ctx, dlogits, _datt, _dchars):
        lib = _lib.load()
        if dlogits is None:
            raise RuntimeError('decoder_loop: no gradient reached the logits')
        if getattr(ctx, 'consumed', False):
            raise RuntimeError('decoder_loop: the saved gates were overwritten with their derivatives by the '
                               'first backward pass; a second pass over the same graph is not supported')
        ctx.consumed = True
        d = ctx.dec
        feat, comp, enc_len, teacher, modes, uniforms, params, bufs = ctx.keep
        pw = dict(zip(_DEC_PARAMS, params))
        dev = feat.device
        B, T, E, A, D, V, U = d.B, d.T, d.E, d.A, d.D, d.V, d.U
        dlogits = _f32c(dlogits)
        f = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)
        # Parameter gradients: with optimizer-owned flat gradients they are deferred to
        # the side stream and accumulated in place (as for the BiLSTM layers).
        sinks = ctx.sinks
        if sinks is None:
            out = dict(dfeat=f(B, T, E), dcomp=f(B, T, A), dw_phi=f(A, D), dw_ih1=f(4 * D, D + E),
                       dw_hh1=f(4 * D, D), db1=f(4 * D), dw_ih2=f(4 * D, D), dw_hh2=f(4 * D, D),
                       db2=f(4 * D), dembed=f(V, D), dw_ct=f(V, D), db_ct=f(V))
        else:
            sk = dict(zip(_DEC_PARAMS, sinks))
            out = dict(dfeat=f(B, T, E), dcomp=f(B, T, A), dw_phi=sk['w_phi'], dw_ih1=sk['w_ih1'],
                       dw_hh1=sk['w_hh1'], db1=sk['b_ih1'], dw_ih2=sk['w_ih2'], dw_hh2=sk['w_hh2'],
                       db2=sk['b_ih2'], dembed=sk['embed'], dw_ct=sk['w_ct'], db_ct=sk['b_ct'])
        ws = dict(ws_t_ih1=f(D + E, 4 * D), ws_t_hh1=f(D, 4 * D), ws_t_ih2=f(D, 4 * D),
                  ws_t_hh2=f(D, 4 * D), ws_dh2=f(U, B, D), ws_dctx=f(U, B, E),
                  ws_de=f(B, U, T), ws_dqpre=f(U, B, A), ws_dc=f(2, 2, B, D),
                  ws_demb=f(U, B, D))
        gx_floats = int(lib.ssasr_bilstm_bwd_gx_floats(U, B, D))
        armed = False
        if gx_floats:                     # persistent BPTT of the second cell
            chain_floats = int(lib.ssasr_decoder_bwd_chain_floats(U, B, T, A, E, D))
            slots = ctx.slots
            armed = (slots is not None and slots.get('ring') is not None and chain_floats > 0 and
                     int(lib.ssasr_bilstm_bwd_ring_floats(U, B, D, 1)) > 0)
            if armed:                     # ring and chain workspace from the backward arena, armed by its one fill
                ws['ws_gx'] = slots['bwd_arena'].take(slots['ring'])
                ws['ws_chain'] = slots['bwd_arena'].take(slots['chain'])
            else:
                ws['ws_gx'] = f(gx_floats)
                if chain_floats:          # persistent first-cell <-> attention chain
                    ws['ws_chain'] = f(chain_floats)
            ws['ws_sync'] = _status_words(dev)
            _track_status(ws['ws_sync'], 4)
            _track_status(ws['ws_sync'], 5)
        g = _lib.DecoderGrads()
        g.dlogits = dlogits.data_ptr()
        for k, t in list(out.items()) + list(ws.items()):
            setattr(g, k, t.data_ptr())
        if sinks is not None:
            g.db1_2, g.db2_2 = sk['b_hh1'].data_ptr(), sk['b_hh2'].data_ptr()
            g.defer_wgrad = 1
        g.ws_armed = 1 if armed else 0
        check(lib.ssasr_decoder_bwd(C.byref(d), C.byref(g), _stream()), 'ssasr_decoder_bwd')
        dpsi = ()
        if ctx.psi:
            # dcomp -> d(pre-activation) in place, dfeat += dpre . W_psi; the psi weight gradients
            # are left to the weight-gradient pass below
            w_psi = params[-2]
            check(lib.ssasr_attn_precompute_bwd(_p(out['dcomp']), _p(comp), _p(feat), _p(w_psi), B * T, E, A,
                                                _p(out['dfeat']), None, None, _stream()),
                  'ssasr_attn_precompute_bwd')
            if sinks is None:
                dpsi = (f(A, E), f(A))
                check(lib.ssasr_attn_precompute_wgrad(_p(out['dcomp']), _p(feat), B * T, E, A, _p(dpsi[0]),
                                                      _p(dpsi[1]), 0, _stream()), 'ssasr_attn_precompute_wgrad')
        if sinks is not None:
            main = torch.cuda.current_stream()
            side = side_stream()
            side.wait_stream(main)
            with torch.cuda.stream(side):
                check(lib.ssasr_decoder_wgrad(C.byref(d), C.byref(g), 1, C.c_void_p(side.cuda_stream)),
                      'ssasr_decoder_wgrad')
                if ctx.psi:
                    check(lib.ssasr_attn_precompute_wgrad(_p(out['dcomp']), _p(feat), B * T, E, A, _p(sinks[-2]),
                                                          _p(sinks[-1]), 1, C.c_void_p(side.cuda_stream)),
                          'ssasr_attn_precompute_wgrad')
            for t in list(bufs.values()) + list(ws.values()) + [dlogits, out['dcomp'], feat]:
                t.record_stream(side)
            _notify_wgrad(sinks)
            return (out['dfeat'], None if ctx.psi else out['dcomp']) + (None,) * (7 + len(params))
        o = out
        return (o['dfeat'], None if ctx.psi else o['dcomp'], None, None, None, None, None, None, None,
                o['dw_phi'], o['dw_ih1'], o['dw_hh1'], o['db1'], o['db1'].clone(),
                o['dw_ih2'], o['dw_hh2'], o['db2'], o['db2'].clone(),
                o['dembed'], o['dw_ct'], o['db_ct']) + dpsi


def decoder_loop(feat, comp, enc_len, teacher, step_mode, uniforms, params, modes_dev=None, psi=None,
                 slots=None):
    """The decode loop of ASR.forward (src/asr.py:67-110).

    step_mode: host sequence of U ints (0 teacher forced, 1 sample, 2 argmax);
    modes_dev: the same values as an int32 device tensor when the caller has already
    uploaded them (with its other per-step integers), else None.
    psi: (weight, bias) of Attention.psi with comp=None: the projection comp = tanh(psi(feat))
    (src/asr.py:381) is then computed and differentiated inside this node.
    slots: what decoder_reserve returned for this call's sizes, or None.
    teacher: int32 [B, L] device tensor of character ids or None.
    params: dict with the keys of ``_DEC_PARAMS``.
    Returns (logits [B,U,V], att [B,U,T] (no grad), chars [U+1,B] int32)."""
    plist = [params[k] for k in _DEC_PARAMS]
    if psi is not None:
        assert comp is None
        plist += list(psi)
    return _DecoderLoop.apply(feat, comp, enc_len, teacher, list(step_mode), uniforms, _grad_sinks(plist),
                              modes_dev, slots, *plist)


def _decoder_fwd_ws(B, T, U, A, E, D, V):
    """(floats of one h image over all steps, of the q image, of the record ring) for the decode
    loop's persistent forward forms, or None when the shape takes one launch per stage and step:
    T <= 128 -> the short form (csrc/decoder_persistent.h); longer encoder outputs -> the form of
    csrc/decoder_long.h when the library says it is taken (ssasr_decoder_fwd_part_floats)."""
    if not (A == 128 and E == 512 and D == 256 and B <= 32 and V <= 64 and U > 0):
        return None
    nh = U * (D // 4) * 32 * 4
    if T <= 128:
        return nh, U * (A // 16) * 32 * 16, 0
    npart = int(_lib.load().ssasr_decoder_fwd_part_floats(B, T, A, E, D, V))
    return (nh, 0, npart) if npart else None


def decoder_reserve(fwd_arena, bwd_arena, B, T, U, A=128, E=512, D=256, V=64):
    """Reserves the decode loop's exchange workspaces in the two arenas of a pass (forward
    images + context rows (+ record ring); cell-2 ring + chain workspace).  Returns the `slots`
    argument of decoder_loop, or None when the sizes have no persistent form."""
    lib = _lib.load()
    geom = _decoder_fwd_ws(B, T, U, A, E, D, V)
    if geom is None:
        return None
    slots = dict(fwd_arena=fwd_arena, bwd_arena=bwd_arena, fwd=None, ring=None, chain=None)
    slots['fwd'] = fwd_arena.reserve(2 * geom[0] + geom[1] + U * B * E + geom[2])
    ring = int(lib.ssasr_bilstm_bwd_ring_floats(U, B, D, 1))
    chain = int(lib.ssasr_decoder_bwd_chain_floats(U, B, T, A, E, D))
    if ring and chain:
        slots['ring'] = bwd_arena.reserve(ring)
        slots['chain'] = bwd_arena.reserve(chain)
    return slots


# ---------------------------------------------------------------------------
# masked cross entropy
# ---------------------------------------------------------------------------
class _CELoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, y32):
        lib = _lib.load()
        _need_gpu(logits, y32)
        logits = _f32c(logits)
        B, U, V = logits.shape
        lse = torch.empty(B * U + 9 * B, device=logits.device, dtype=torch.float32)
        loss = torch.empty((), device=logits.device, dtype=torch.float32)
        check(lib.ssasr_ce_loss_fwd(_p(logits), _p(y32), y32.stride(0), y32.shape[1], B, U, V, _p(lse),
                                    _p(loss), _stream()), 'ssasr_ce_loss_fwd')
        ctx.save_for_backward(logits, y32, lse)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        lib = _lib.load()
        logits, y32, lse = ctx.saved_tensors
        B, U, V = logits.shape
        dloss = dloss.to(torch.float32).contiguous()
        dlogits = torch.empty_like(logits)
        check(lib.ssasr_ce_loss_bwd(_p(logits), _p(y32), y32.stride(0), _p(lse), _p(dloss), B, U, V,
                                    _p(dlogits), _stream()), 'ssasr_ce_loss_bwd')
        return dlogits, None


class _CELossLS(torch.autograd.Function):
    """_CELoss with label smoothing eps in (0, 1): ssasr_ce_loss_ls_fwd / _bwd."""

    @staticmethod
    def forward(ctx, logits, y32, eps):
        lib = _lib.load()
        _need_gpu(logits, y32)
        logits = _f32c(logits)
        B, U, V = logits.shape
        lse = torch.empty(B * U + 9 * B, device=logits.device, dtype=torch.float32)
        loss = torch.empty((), device=logits.device, dtype=torch.float32)
        check(lib.ssasr_ce_loss_ls_fwd(_p(logits), _p(y32), y32.stride(0), y32.shape[1], B, U, V, eps, _p(lse),
                                       _p(loss), _stream()), 'ssasr_ce_loss_ls_fwd')
        ctx.save_for_backward(logits, y32, lse)
        ctx.eps = eps
        return loss

    @staticmethod
    def backward(ctx, dloss):
        lib = _lib.load()
        logits, y32, lse = ctx.saved_tensors
        B, U, V = logits.shape
        dloss = dloss.to(torch.float32).contiguous()
        dlogits = torch.empty_like(logits)
        check(lib.ssasr_ce_loss_ls_bwd(_p(logits), _p(y32), y32.stride(0), _p(lse), _p(dloss), B, U, V, ctx.eps,
                                       _p(dlogits), _stream()), 'ssasr_ce_loss_ls_bwd')
        return dlogits, None, None


_i32_cache = (None, None, None)      # (weak reference to the source tensor, its version, the int32 copy)


def as_i32(t):
    """int32 copy of an integer device tensor, remembered for the tensor OBJECT it was made from
    (weak reference + version counter, never an address: the next batch's labels may well be
    allocated where the last batch's were): the label matrix of a step is needed twice, for
    teacher forcing and for the loss."""
    global _i32_cache
    if t.dtype == torch.int32 and t.stride(-1) == 1:
        return t
    ref, version, copy = _i32_cache
    if ref is not None and ref() is t and version == t._version:
        return copy
    copy = t.to(torch.int32).contiguous()
    _i32_cache = (weakref.ref(t), t._version, copy)
    return copy


def masked_ce_loss(logits, y, ans_len, label_smoothing=0.0):
    """src/trainer.py:426-434.  logits [B,U,V] (U >= ans_len), y [B,L] int, L > ans_len: the
    labels are y[:, 1:ans_len + 1], read in place; rows are normalised by count(y != 0).
    label_smoothing in [0, 1) (build-defined, the reference has none): the token loss of
    torch's cross_entropy(label_smoothing=...), uniform over all V classes; 0 is the reference's loss."""
    label_smoothing = float(label_smoothing)
    if not 0.0 <= label_smoothing < 1.0:
        raise ValueError('label_smoothing must lie in [0, 1), got %r' % label_smoothing)
    if logits.shape[1] != ans_len:
        logits = logits[:, :ans_len].contiguous()
    if label_smoothing == 0.0:
        return _CELoss.apply(logits, as_i32(y))
    return _CELossLS.apply(logits, as_i32(y), label_smoothing)


# ---------------------------------------------------------------------------
# CTC branch (build-defined: the reference has no CTC; checker = torch's ctc_loss)
# ---------------------------------------------------------------------------
def _ctc_label_matrix(name, y32, lmax):
    """The label matrix every CTC kernel reads: int32 with unit column stride, at least lmax columns."""
    if y32.dtype != torch.int32 or y32.stride(-1) != 1:
        raise TypeError('%s: labels must be int32 with unit column stride' % name)
    if lmax > y32.shape[1]:
        raise ValueError('%s: Lmax exceeds the label matrix' % name)


def _ctc_head_logits(feat, weight, bias):
    """The CTC head's product feat @ weight.T + bias, issued one way by the training node and by every decoder,
    aligner and segmenter.  -> (logits [B, T, V], and the contiguous float32 feat and weight the product read)."""
    _need_gpu(feat, weight, bias)
    feat, w, b = _f32c(feat), _f32c(weight), _f32c(bias)
    B, T, E = feat.shape
    return gemm(feat.view(B * T, E), w, bias=b).view(B, T, w.shape[0]), feat, w


def _ctc_geometry(logits, y32, lmax):
    B, T, V = logits.shape
    _ctc_label_matrix('ctc', y32, lmax)
    n = _lib.load().ssasr_ctc_ws_floats(B, T, V, lmax)
    if n <= 0:
        raise ValueError('ctc: shape B=%d T=%d V=%d Lmax=%d has no kernel' % (B, T, V, lmax))
    return B, T, V, n


def _ctc_fwd(logits, frame_lens, y32, label_lens, lmax, blank):
    lib = _lib.load()
    B, T, V, n = _ctc_geometry(logits, y32, lmax)
    ws = torch.empty(n, device=logits.device, dtype=torch.float32)
    loss = torch.empty((), device=logits.device, dtype=torch.float32)
    check(lib.ssasr_ctc_loss_fwd(_p(logits), _p(frame_lens), _p(y32), y32.stride(0), _p(label_lens), B, T, V,
                                 lmax, blank, _p(ws), _p(loss), _stream()), 'ssasr_ctc_loss_fwd')
    return loss, ws


def _ctc_bwd(logits, frame_lens, y32, label_lens, lmax, blank, ws, dloss, dbias=None):
    lib = _lib.load()
    B, T, V = logits.shape
    dlogits = torch.empty_like(logits)
    dloss = dloss.to(torch.float32).contiguous()
    check(lib.ssasr_ctc_loss_bwd(_p(logits), _p(frame_lens), _p(y32), y32.stride(0), _p(label_lens), B, T, V,
                                 lmax, blank, _p(ws), _p(dloss), _p(dlogits), _p(dbias), _stream()),
          'ssasr_ctc_loss_bwd')
    return dlogits


class _CTCLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, frame_lens, y32, label_lens, lmax, blank):
        _need_gpu(logits, frame_lens, y32, label_lens)
        logits = _f32c(logits)
        loss, ws = _ctc_fwd(logits, frame_lens, y32, label_lens, lmax, blank)
        ctx.save_for_backward(logits, frame_lens, y32, label_lens, ws)
        ctx.geom = (lmax, blank)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        logits, frame_lens, y32, label_lens, ws = ctx.saved_tensors
        return (_ctc_bwd(logits, frame_lens, y32, label_lens, *ctx.geom, ws, dloss),) + (None,) * 5


class _CTCHead(torch.autograd.Function):
    """Linear(E -> V) on the Listener's output + CTC in one node: the bias gradient comes out of
    the CTC backward kernel, the two other products are GEMMs."""

    @staticmethod
    def forward(ctx, feat, w, b, frame_lens, y32, label_lens, lmax, blank):
        _need_gpu(frame_lens, y32, label_lens)
        logits, feat, w = _ctc_head_logits(feat, w, b)
        loss, ws = _ctc_fwd(logits, frame_lens, y32, label_lens, lmax, blank)
        ctx.save_for_backward(feat, w, logits, frame_lens, y32, label_lens, ws)
        ctx.geom = (lmax, blank)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        feat, w, logits, frame_lens, y32, label_lens, ws = ctx.saved_tensors
        B, T, E = feat.shape
        V = w.shape[0]
        db = torch.zeros(V, device=feat.device, dtype=torch.float32)
        dlogits = _ctc_bwd(logits, frame_lens, y32, label_lens, *ctx.geom, ws, dloss, dbias=db).view(B * T, V)
        dfeat = gemm(dlogits, w, tb=True).view(B, T, E)
        dw = gemm(dlogits, feat.view(B * T, E), ta=True, tb=True)
        return (dfeat, dw, db) + (None,) * 5


def ctc_loss(logits, frame_lens, y, label_lens, lmax, blank=0):
    """mean_b(nll_b / max(label_len_b, 1)) of torch's ctc_loss(reduction='mean', zero_infinity=True)
    on log_softmax(logits).  logits [B,T,V] float32; frame_lens, label_lens int32 [B] on the device;
    y int32 [B, >= lmax]: row b's labels are y[b, :label_lens[b]]."""
    return _CTCLoss.apply(logits, frame_lens, y, label_lens, int(lmax), int(blank))


def ctc_head_loss(feat, weight, bias, frame_lens, y, label_lens, lmax, blank=0):
    """ctc_loss(feat @ weight.T + bias, ...) as one autograd node."""
    return _CTCHead.apply(feat, weight, bias, frame_lens, y, label_lens, int(lmax), int(blank))


def ctc_align(logits, frame_lens, y32, label_lens, lmax, blank=0):
    """ssasr_ctc_align: the most probable CTC path (Viterbi) of each row's labels through its frames, on the raw
    logits [B, T, V] (include/ssasr.h).  Arguments as ctc_loss.  -> (path [B, T] int32: the lattice state per
    frame, -1 past the row's frames; first, last [B, lmax] int32: each character's first / last (inclusive) frame,
    -1 past the row's labels; char_logp [B, lmax] float32; score [B] float64, -inf: no alignment fits) on the
    device.  No autograd."""
    lib = _lib.load()
    lmax, blank = int(lmax), int(blank)
    _need_gpu(logits, frame_lens, y32, label_lens)
    logits = _f32c(logits.detach())
    B, T, V = logits.shape
    _ctc_label_matrix('ctc_align', y32, lmax)
    need = int(lib.ssasr_ctc_align_ws_bytes(B, T, V, lmax))
    if need <= 0:
        raise ValueError('ctc_align: shape B=%d T=%d V=%d Lmax=%d has no kernel' % (B, T, V, lmax))
    dev = logits.device
    ws = torch.empty(need // 8, device=dev, dtype=torch.float64)
    path = torch.empty(B, T, device=dev, dtype=torch.int32)
    first = torch.empty(B, lmax, device=dev, dtype=torch.int32)
    last = torch.empty(B, lmax, device=dev, dtype=torch.int32)
    char_logp = torch.empty(B, lmax, device=dev, dtype=torch.float32)
    score = torch.empty(B, device=dev, dtype=torch.float64)
    check(lib.ssasr_ctc_align(_p(logits), _p(frame_lens), _p(y32), y32.stride(0), _p(label_lens), B, T, V, lmax, blank,
                              _p(ws), need, _p(path), _p(first) if lmax else None, _p(last) if lmax else None,
                              _p(char_logp) if lmax else None, _p(score), _stream()), 'ssasr_ctc_align')
    return path, first, last, char_logp, score


def ctc_head_align(feat, weight, bias, frame_lens, y32, label_lens, lmax, blank=0):
    """ctc_align on the head's logits, the product issued exactly as the training node issues it (_CTCHead.forward).
    -> ctc_align's five tensors and the logits [B, T, V] they were aligned on.  No autograd."""
    logits = _ctc_head_logits(feat.detach(), weight.detach(), bias.detach())[0]
    return ctc_align(logits, frame_lens, y32, label_lens, lmax, blank) + (logits,)


CTC_SEGMENT_MAX_LABELS = 8191   # ssasr_ctc_segment's limits (include/ssasr.h): 2 * Lmax + 1 <= 16384
CTC_SEGMENT_MAX_FRAMES = 32768


def ctc_segment_form(T, lmax):
    """ssasr_ctc_segment_form: (form, threads, states per thread) of the launch that serves T frames and lmax labels;
    None when no form does."""
    threads, per_thread = C.c_int(0), C.c_int(0)
    form = int(_lib.load().ssasr_ctc_segment_form(int(T), int(lmax), C.byref(threads), C.byref(per_thread)))
    return None if form < 0 else (form, threads.value, per_thread.value)


CTC_SEGMENT_SKIP_MAX_UTTS = 1024   # ssasr_ctc_segment_skip's: the junctions' values live in LDS


def _segment_penalty(name, value):
    """None (off) -> -inf; else a finite number <= 0."""
    if value is None:
        return -math.inf
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not math.isfinite(value) or value > 0:
        raise ValueError('ctc_segment: %s must be None or a finite number <= 0, got %r' % (name, value))
    return float(value)


def ctc_segment(logits, frame_lens, y32, label_lens, utt_ends, n_utts, lmax, nmax, window, blank=0, *,
                skip_penalty=None, fill_penalty=None):
    """ssasr_ctc_segment: CTC segmentation of each row's WHOLE text (its utterances concatenated in y32) inside its
    frames, on the raw logits [B, T, V]: ctc_align's lattice on normalised values with a free start and a free end
    (include/ssasr.h).  utt_ends int32 [B, >= nmax]: the exclusive end of each utterance's labels; n_utts int32 [B].
    -> (path [B, T] int32, -1 outside the span; first, last [B, lmax] int32; char_logp [B, lmax] float32; score [B]
    float64, -inf: nothing fits; utt_first, utt_last [B, nmax] int32; utt_conf [B, nmax] float32: the min-mean of the
    path's log-probabilities over blocks of `window` frames) on the device.  No autograd.
    skip_penalty / fill_penalty (None: off; else finite and <= 0): with either given, ssasr_ctc_segment_skip runs
    instead -- an utterance may be passed over at skip_penalty, and a frame at an utterance boundary may be taken as
    unwritten speech at fill_penalty (include/ssasr.h) -- and two more tensors follow the eight: utt_skipped [B, nmax]
    int32 (1 skipped, 0 aligned, -1 no such utterance) and is_fill [B, T] int32 (1 a filler frame, 0 another scored
    frame, -1 outside the span).  With both None the call and its result are what they were."""
    lib = _lib.load()
    lmax, nmax, window, blank = int(lmax), int(nmax), int(window), int(blank)
    skip_pen, fill_pen = _segment_penalty('skip_penalty', skip_penalty), _segment_penalty('fill_penalty', fill_penalty)
    with_skip = skip_penalty is not None or fill_penalty is not None
    _need_gpu(logits, frame_lens, y32, label_lens, utt_ends, n_utts)
    logits = _f32c(logits.detach())
    B, T, V = logits.shape
    for name, t in (('labels', y32), ('utt_ends', utt_ends)):
        if t.dtype != torch.int32 or t.dim() != 2 or t.stride(-1) != 1:
            raise TypeError('ctc_segment: %s must be an int32 matrix with unit column stride' % name)
    if lmax > y32.shape[1] or nmax > utt_ends.shape[1]:
        raise ValueError('ctc_segment: Lmax / Nmax exceed the label / utterance matrix')
    if window < 1:
        raise ValueError('ctc_segment: window must be >= 1, got %d' % window)
    if with_skip and nmax > CTC_SEGMENT_SKIP_MAX_UTTS:
        raise ValueError('ctc_segment: %d utterances; with skip_penalty / fill_penalty at most %d'
                         % (nmax, CTC_SEGMENT_SKIP_MAX_UTTS))
    need = int((lib.ssasr_ctc_segment_skip_ws_bytes if with_skip else lib.ssasr_ctc_segment_ws_bytes)(B, T, V, lmax, nmax))
    if need <= 0:
        raise ValueError('ctc_segment: shape B=%d T=%d V=%d Lmax=%d Nmax=%d has no kernel (at most %d frames and %d '
                         'labels)' % (B, T, V, lmax, nmax, CTC_SEGMENT_MAX_FRAMES, CTC_SEGMENT_MAX_LABELS))
    dev = logits.device
    ws = torch.empty(need // 8, device=dev, dtype=torch.float64)
    path = torch.empty(B, T, device=dev, dtype=torch.int32)
    first = torch.empty(B, lmax, device=dev, dtype=torch.int32)
    last = torch.empty(B, lmax, device=dev, dtype=torch.int32)
    char_logp = torch.empty(B, lmax, device=dev, dtype=torch.float32)
    score = torch.empty(B, device=dev, dtype=torch.float64)
    utt_first = torch.empty(B, nmax, device=dev, dtype=torch.int32)
    utt_last = torch.empty(B, nmax, device=dev, dtype=torch.int32)
    utt_conf = torch.empty(B, nmax, device=dev, dtype=torch.float32)
    if with_skip:
        utt_skipped = torch.empty(B, nmax, device=dev, dtype=torch.int32)
        is_fill = torch.empty(B, T, device=dev, dtype=torch.int32)
        pens = (C.c_double * 2)(skip_pen, fill_pen)            # host memory, read before the call returns
        check(lib.ssasr_ctc_segment_skip(
            _p(logits), _p(frame_lens), _p(y32), y32.stride(0), _p(label_lens), _p(utt_ends), utt_ends.stride(0),
            _p(n_utts), B, T, V, lmax, nmax, window, blank, C.addressof(pens), C.addressof(pens) + 8, _p(ws), need,
            _p(path), _p(first), _p(last), _p(char_logp), _p(score), _p(utt_first), _p(utt_last), _p(utt_conf),
            _p(utt_skipped), _p(is_fill), _stream()), 'ssasr_ctc_segment_skip')
        return path, first, last, char_logp, score, utt_first, utt_last, utt_conf, utt_skipped, is_fill
    check(lib.ssasr_ctc_segment(_p(logits), _p(frame_lens), _p(y32), y32.stride(0), _p(label_lens), _p(utt_ends),
                                utt_ends.stride(0), _p(n_utts), B, T, V, lmax, nmax, window, blank, _p(ws), need,
                                _p(path), _p(first), _p(last), _p(char_logp), _p(score), _p(utt_first), _p(utt_last),
                                _p(utt_conf), _stream()), 'ssasr_ctc_segment')
    return path, first, last, char_logp, score, utt_first, utt_last, utt_conf


def ctc_head_segment(feat, weight, bias, frame_lens, y32, label_lens, utt_ends, n_utts, lmax, nmax, window, blank=0, *,
                     skip_penalty=None, fill_penalty=None):
    """ctc_segment on the head's logits, the product issued exactly as the training node issues it (_CTCHead.forward).
    -> ctc_segment's eight (with a penalty: ten) tensors and the logits [B, T, V] they were computed on.  No
    autograd."""
    logits = _ctc_head_logits(feat.detach(), weight.detach(), bias.detach())[0]
    return ctc_segment(logits, frame_lens, y32, label_lens, utt_ends, n_utts, lmax, nmax, window, blank,
                       skip_penalty=skip_penalty, fill_penalty=fill_penalty) + (logits,)


CTC_DECODE_MAX_BEAM = 32       # ssasr_ctc_decode's limits (include/ssasr.h)
CTC_DECODE_MAX_FRAMES = 4096


def _prefix_search_entry(name, logits, frame_lens, beam_size, blank, score_names, term=None, classes=None):
    """What ctc_decode, ctc_decode_lm and ctc_decode_graph (`name`) do before their launch: the checks of beam_size
    (from 0 without a `term`, from 1 and an int with one: 'LM' or 'graph', the word the message uses), of logits,
    frame_lens and blank, then classes(V) (the caller's own checks against the number of classes), then the tensors'
    device.  -> (logits float32 contiguous, (B, T, V), the outputs: chars [B, Kr, T], n_chars [B, Kr], n_hyps [B]
    int32 and a float32 [B, Kr] per name in score_names, Kr = max(beam_size, 1))."""
    if isinstance(beam_size, bool) or not isinstance(beam_size, int) or \
            not (0 if term is None else 1) <= beam_size <= CTC_DECODE_MAX_BEAM:
        if term is None:
            raise ValueError('%s: beam_size must be in 0..%d, got %d' % (name, CTC_DECODE_MAX_BEAM, beam_size))
        raise ValueError('%s: beam_size must be an int in 1..%d (the best path has no %s form), got %r'
                         % (name, CTC_DECODE_MAX_BEAM, term, beam_size))
    if logits.dim() != 3:
        raise ValueError('%s: logits must be [B, T, V], got %r' % (name, tuple(logits.shape)))
    if frame_lens.dtype != torch.int32 or frame_lens.numel() != logits.shape[0]:
        raise TypeError('%s: frame_lens must be int32 [B]' % name)
    B, T, V = logits.shape
    if not 0 <= blank < V:
        raise ValueError('%s: blank %d is no class of V=%d' % (name, blank, V))
    if classes is not None:
        classes(V)
    _need_gpu(logits, frame_lens)
    logits = _f32c(logits.detach())
    dev, kr = logits.device, max(beam_size, 1)
    out = {'chars': torch.empty(B, kr, T, device=dev, dtype=torch.int32),
           'n_chars': torch.empty(B, kr, device=dev, dtype=torch.int32),
           'n_hyps': torch.empty(B, device=dev, dtype=torch.int32)}
    for score in score_names:
        out[score] = torch.empty(B, kr, device=dev, dtype=torch.float32)
    return logits, (B, T, V), out


def ctc_decode(logits, frame_lens, beam_size, blank=0):
    """ssasr_ctc_decode: a transcript per row from the CTC posteriors alone, in one launch (include/ssasr.h).  logits
    [B, T, V] raw head outputs, frame_lens int32 [B] on the device.  beam_size 0: the best path (V <= 1024); 1 .. 32:
    prefix beam search of that width (V <= 64).  -> (chars [B, Kr, T] int32, n_chars [B, Kr] int32, scores [B, Kr]
    float32, n_hyps [B] int32) on the device, Kr = max(beam_size, 1), best first; slots from n_hyps on have length 0
    and score -inf.  No autograd."""
    lib = _lib.load()
    beam_size, blank = int(beam_size), int(blank)
    logits, (B, T, V), out = _prefix_search_entry('ctc_decode', logits, frame_lens, beam_size, blank, ('scores',))
    need = int(lib.ssasr_ctc_decode_ws_bytes(B, T, V, beam_size))
    if need <= 0:
        raise ValueError('ctc_decode: shape B=%d T=%d V=%d beam_size=%d has no kernel' % (B, T, V, beam_size))
    ws = torch.empty((need + 7) // 8, device=logits.device, dtype=torch.int64)
    check(lib.ssasr_ctc_decode(_p(logits), _p(frame_lens.contiguous()), B, T, V, beam_size, blank, _p(ws), ws.numel() * 8,
                               _p(out['chars']), _p(out['n_chars']), _p(out['scores']), _p(out['n_hyps']), _stream()),
          'ssasr_ctc_decode')
    return out['chars'], out['n_chars'], out['scores'], out['n_hyps']


def ctc_head_decode(feat, weight, bias, frame_lens, beam_size, blank=0):
    """ctc_decode on the head's logits, the product issued exactly as the training node issues it (_CTCHead.forward).
    -> ctc_decode's four tensors and the logits [B, T, V] they were decoded from.  No autograd."""
    logits = _ctc_head_logits(feat.detach(), weight.detach(), bias.detach())[0]
    return ctc_decode(logits, frame_lens, beam_size, blank) + (logits,)


def ctc_decode_lm(logits, frame_lens, beam_size, lm, lm_weight=0.0, length_bonus=0.0, eos=1, blank=0):
    """ssasr_ctc_decode_lm: ctc_decode's prefix beam search with the CharLM in the ranking, in one launch
    (include/ssasr.h).  logits [B, T, V], frame_lens int32 [B] on the device; beam_size 1 .. 32; lm a charlm.CharLM
    with input_size == V (None is allowed at lm_weight 0); eos < 0: no end term.  -> a dict: chars [B, K, T] int32,
    n_chars [B, K] int32, scores / ctc_scores / lm_scores [B, K] float32 (the fused total, the CTC part, the LM part
    with the end term), n_hyps [B] int32, lm_frames [B] int32 (frames that ran an LM step), best first.  At zero
    weights the first four are ctc_decode's bits.  No autograd."""
    lib = _lib.load()
    blank, eos, lm_weight, length_bonus = int(blank), int(eos), float(lm_weight), float(length_bonus)
    if not (math.isfinite(lm_weight) and math.isfinite(length_bonus)):
        raise ValueError('ctc_decode_lm: lm_weight and length_bonus must be finite, got %r, %r'
                         % (lm_weight, length_bonus))
    if lm is None and lm_weight != 0.0:
        raise ValueError('ctc_decode_lm: lm_weight %g needs a language model' % lm_weight)

    def classes(V):
        if eos >= V:
            raise ValueError('ctc_decode_lm: eos %d is no class of V=%d' % (eos, V))
        if lm is not None and lm.input_size != V:
            raise ValueError('ctc_decode_lm: the language model has %d classes, the logits %d' % (lm.input_size, V))
    logits, (B, T, V), out = _prefix_search_entry('ctc_decode_lm', logits, frame_lens, beam_size, blank,
                                                  ('scores', 'ctc_scores', 'lm_scores'), term='LM', classes=classes)
    s, keep = _charlm_struct(lm) if lm is not None else (None, None)
    H = lm.hidden_size if lm_weight != 0.0 else 0
    need = int(lib.ssasr_ctc_decode_lm_ws_bytes(B, T, V, beam_size, H))
    if need <= 0:
        raise ValueError('ctc_decode_lm: shape B=%d T=%d V=%d beam_size=%d H=%d has no kernel' % (B, T, V, beam_size, H))
    ws = torch.empty((need + 15) // 16 * 2, device=logits.device, dtype=torch.int64)
    check(lib.ssasr_ctc_decode_lm(_p(logits), _p(frame_lens.contiguous()), B, T, V, beam_size, blank, _p(ws),
                                  ws.numel() * 8, _p(out['chars']), _p(out['n_chars']), _p(out['scores']),
                                  _p(out['n_hyps']), C.byref(s) if s is not None else None, lm_weight, length_bonus,
                                  eos, _p(out['ctc_scores']), _p(out['lm_scores']), _stream()), 'ssasr_ctc_decode_lm')
    out['lm_frames'] = ws.view(torch.int32)[need // 4 - B:need // 4]
    return out


def ctc_head_decode_lm(feat, weight, bias, frame_lens, beam_size, lm, lm_weight=0.0, length_bonus=0.0, eos=1, blank=0):
    """ctc_decode_lm on the head's logits, the product issued as ctc_head_decode issues it.  -> ctc_decode_lm's dict
    with the logits [B, T, V] they were decoded from under 'logits'.  No autograd."""
    logits = _ctc_head_logits(feat.detach(), weight.detach(), bias.detach())[0]
    out = ctc_decode_lm(logits, frame_lens, beam_size, lm, lm_weight, length_bonus, eos, blank)
    out['logits'] = logits
    return out


def ctc_decode_graph(logits, frame_lens, beam_size, graph, graph_weight=0.0, length_bonus=0.0, blank=0):
    """ssasr_ctc_decode_graph: ctc_decode's prefix beam search with a character graph (char_graph.CharGraph: an n-gram
    LM, hotwords, their product) in the ranking, in one launch (include/ssasr.h).  logits [B, T, V], frame_lens int32
    [B] on the device; beam_size 1 .. 32; graph with n_classes == V (None is allowed at graph_weight 0), uploaded to
    the logits' device on first use and held there; graph_weight finite and >= 0.  -> a dict: chars [B, K, T] int32,
    n_chars [B, K] int32, scores / ctc_scores / graph_scores [B, K] float32 (the fused total, the CTC part, G + fin),
    n_hyps [B] int32, best first.  At zero weights the first four are ctc_decode's bits.  No autograd."""
    from .char_graph import CharGraph
    return _prefix_search_graph('ctc_decode_graph', CharGraph, 'char_graph.CharGraph', logits, frame_lens, beam_size,
                                graph, graph_weight, length_bonus, blank)


def _prefix_search_graph(name, cls, cls_name, logits, frame_lens, beam_size, graph, graph_weight, length_bonus, blank):
    """ctc_decode_graph and ctc_decode_word (`name`: also the C entry's, behind 'ssasr_'): the checks of the weights and
    of the graph (an instance of `cls`, None allowed at weight 0), the upload, the workspace and the launch."""
    lib = _lib.load()
    blank, graph_weight, length_bonus = int(blank), float(graph_weight), float(length_bonus)
    if not (math.isfinite(graph_weight) and graph_weight >= 0.0 and math.isfinite(length_bonus)):
        raise ValueError('%s: graph_weight must be finite and >= 0 and length_bonus finite, got %r, %r'
                         % (name, graph_weight, length_bonus))
    if graph is None and graph_weight != 0.0:
        raise ValueError('%s: graph_weight %g needs a graph' % (name, graph_weight))
    if graph is not None and not isinstance(graph, cls):
        raise TypeError('%s: graph must be a %s, got %s' % (name, cls_name, type(graph).__name__))

    def classes(V):
        if graph is not None and graph.n_classes != V:
            raise ValueError('%s: the graph has %d classes, the logits %d' % (name, graph.n_classes, V))
        if graph is not None and getattr(graph, 'space', None) == blank:
            raise ValueError('%s: the graph\'s space class %d is the blank' % (name, blank))
    logits, (B, T, V), out = _prefix_search_entry(name, logits, frame_lens, beam_size, blank,
                                                  ('scores', 'ctc_scores', 'graph_scores'), term='graph',
                                                  classes=classes)
    s, keep = graph.to(logits.device) if graph is not None else (None, None)
    need = int(getattr(lib, 'ssasr_%s_ws_bytes' % name)(B, T, V, beam_size))
    if need <= 0:
        raise ValueError('%s: shape B=%d T=%d V=%d beam_size=%d has no kernel' % (name, B, T, V, beam_size))
    ws = torch.empty((need + 7) // 8, device=logits.device, dtype=torch.int64)
    check(getattr(lib, 'ssasr_' + name)(_p(logits), _p(frame_lens.contiguous()), B, T, V, beam_size, blank, _p(ws),
                                        ws.numel() * 8, _p(out['chars']), _p(out['n_chars']), _p(out['scores']),
                                        _p(out['n_hyps']), C.byref(s) if s is not None else None, graph_weight,
                                        length_bonus, _p(out['ctc_scores']), _p(out['graph_scores']), _stream()),
          'ssasr_' + name)
    return out


def ctc_decode_word(logits, frame_lens, beam_size, graph, graph_weight=0.0, length_bonus=0.0, blank=0):
    """ssasr_ctc_decode_word: ctc_decode's prefix beam search over a lexicon with a word n-gram LM
    (word_graph.WordGraph) in the ranking, in one launch (include/ssasr.h).  The arguments and the dict returned are
    ctc_decode_graph's, graph_scores holding G + fin of the word graph.  No autograd."""
    from .word_graph import WordGraph
    return _prefix_search_graph('ctc_decode_word', WordGraph, 'word_graph.WordGraph', logits, frame_lens, beam_size,
                                graph, graph_weight, length_bonus, blank)


def ctc_head_decode_word(feat, weight, bias, frame_lens, beam_size, graph, graph_weight=0.0, length_bonus=0.0, blank=0):
    """ctc_decode_word on the head's logits, the product issued as ctc_head_decode issues it.  -> ctc_decode_word's
    dict with the logits [B, T, V] they were decoded from under 'logits'.  No autograd."""
    logits = _ctc_head_logits(feat.detach(), weight.detach(), bias.detach())[0]
    out = ctc_decode_word(logits, frame_lens, beam_size, graph, graph_weight, length_bonus, blank)
    out['logits'] = logits
    return out


def ctc_head_decode_graph(feat, weight, bias, frame_lens, beam_size, graph, graph_weight=0.0, length_bonus=0.0, blank=0):
    """ctc_decode_graph on the head's logits, the product issued as ctc_head_decode issues it.  -> ctc_decode_graph's
    dict with the logits [B, T, V] they were decoded from under 'logits'.  No autograd."""
    logits = _ctc_head_logits(feat.detach(), weight.detach(), bias.detach())[0]
    out = ctc_decode_graph(logits, frame_lens, beam_size, graph, graph_weight, length_bonus, blank)
    out['logits'] = logits
    return out


EDIT_SCORE_MAX_HYP = 8191     # ssasr_edit_score's limits on a row's tokens, counted before dropping
EDIT_SCORE_MAX_REF = 1023


def edit_score(hyp, hyp_lens, ref, ref_lens, ref_of=None, *, first_char=2, space, check_ref_of=True):
    """ssasr_edit_score: character and word edit counts of P (hypothesis, reference) pairs in one launch
    (include/ssasr.h).  hyp [P, Hmax] and ref [rows, Rmax] int32 with unit column stride (rows may be padded: the
    row stride is passed), hyp_lens [P] and ref_lens [rows] int32; ref_of [P] int32: the ref row of pair p, None:
    row p.  Ids < first_char are dropped, words split at `space`.  -> int32 [P, 8] on the device: character S, D,
    I, N, then word S, D, I, N.  Shapes past the kernel's limits raise ValueError (postprocess.edit_counts is the
    host form).  check_ref_of False: ref_of's entries are the caller's own arithmetic and are not read back to be
    range-checked (that check synchronises the device; a train step cannot afford it)."""
    lib = _lib.load()
    _need_gpu(hyp, hyp_lens, ref, ref_lens, ref_of)
    for name, t in (('hyp', hyp), ('ref', ref)):
        if (t.dtype != torch.int32 or t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1) or
                (t.shape[0] > 1 and t.stride(0) < t.shape[1])):
            raise TypeError('edit_score: %s must be a 2-D int32 matrix with unit column stride and disjoint rows' % name)
    for name, t in (('hyp_lens', hyp_lens), ('ref_lens', ref_lens), ('ref_of', ref_of)):
        if t is not None and (t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous()):
            raise TypeError('edit_score: %s must be a contiguous int32 vector' % name)
    P, hmax = hyp.shape
    rows, rmax = ref.shape
    if hmax > EDIT_SCORE_MAX_HYP or rmax > EDIT_SCORE_MAX_REF:
        raise ValueError('edit_score: %d hypothesis / %d reference columns exceed the kernel\'s %d / %d'
                         % (hmax, rmax, EDIT_SCORE_MAX_HYP, EDIT_SCORE_MAX_REF))
    if hyp_lens.shape[0] != P or ref_lens.shape[0] != rows:
        raise ValueError('edit_score: one length per row')
    if ref_of is None:
        if rows != P:
            raise ValueError('edit_score: %d hypotheses against %d references need ref_of' % (P, rows))
    elif ref_of.shape[0] != P or (P and check_ref_of and bool(((ref_of < 0) | (ref_of >= rows)).any())):
        raise ValueError('edit_score: ref_of must name one of the %d reference rows per pair' % rows)
    out = torch.empty(P, 8, device=hyp.device, dtype=torch.int32)
    hyp_ld = hyp.stride(0) if P > 1 else max(hmax, 1)
    ref_ld = ref.stride(0) if rows > 1 else max(rmax, 1)
    check(lib.ssasr_edit_score(_p(hyp), max(hyp_ld, hmax), _p(hyp_lens), _p(ref), max(ref_ld, rmax), _p(ref_lens),
                               _p(ref_of), P, hmax, rmax, int(first_char), int(space), _p(out), _stream()),
          'ssasr_edit_score')
    return out


MBR_MAX_HYPS = 32              # ssasr_mbr_select's limits: hypotheses per utterance, tokens per row before dropping,
MBR_MAX_LEN = 1023             # and the two multiplied
MBR_MAX_TOKENS = 8192
MBR_UNITS = {'char': 0, 'word': 1}
MBR_POSTERIORS = {'softmax': 0, 'uniform': 1}


def mbr_fits(K, hmax):
    """Whether ssasr_mbr_select takes K hypotheses per utterance of at most hmax tokens each."""
    return 1 <= K <= MBR_MAX_HYPS and 0 <= hmax <= MBR_MAX_LEN and K * hmax <= MBR_MAX_TOKENS


def mbr_select(chars, n_chars, n_hyps, scores, *, first_char=2, space, unit='word', posterior='softmax', scale=1.0):
    """ssasr_mbr_select: minimum-Bayes-risk selection over each utterance's hypotheses in one launch
    (include/ssasr.h; postprocess.mbr_reference is its float64 restatement).  chars [N, K, Hmax] int32 with unit
    column stride and rows in (n, k) order (the row stride is passed), n_chars [N, K] and n_hyps [N] int32, scores
    [N, K] float32 (None with posterior 'uniform'); unit 'char' | 'word' (or 0 | 1), posterior 'softmax' | 'uniform'
    (or 0 | 1), scale finite and >= 0.  -> (best int32 [N], risk float32 [N, K], pair int32 [N, K, K, 2]) on the
    device.  Shapes past the kernel's limits (mbr_fits) raise ValueError."""
    lib = _lib.load()
    _need_gpu(chars, n_chars, n_hyps, scores)
    unit = MBR_UNITS.get(unit, unit)
    if unit not in (0, 1):
        raise ValueError("mbr_select: unit must be 'char' or 'word', got %r" % (unit,))
    posterior = MBR_POSTERIORS.get(posterior, posterior)
    if posterior not in (0, 1):
        raise ValueError("mbr_select: posterior must be 'softmax' or 'uniform', got %r" % (posterior,))
    scale = float(scale)
    if not (math.isfinite(scale) and scale >= 0.0):
        raise ValueError('mbr_select: scale must be finite and >= 0, got %r' % (scale,))
    if chars.dtype != torch.int32 or chars.dim() != 3:
        raise TypeError('mbr_select: chars must be an int32 tensor [N, K, Hmax]')
    N, K, hmax = chars.shape
    hyp_ld = chars.stride(1) if N * K > 1 else max(hmax, 1)
    if ((hmax > 1 and chars.stride(2) != 1) or (N * K > 1 and hyp_ld < hmax) or
            (N > 1 and K > 0 and chars.stride(0) != K * hyp_ld)):
        raise TypeError('mbr_select: chars must have unit column stride and equally spaced, disjoint rows')
    for name, t, shape in (('n_chars', n_chars, (N, K)), ('n_hyps', n_hyps, (N,))):
        if t.dtype != torch.int32 or not t.is_contiguous():
            raise TypeError('mbr_select: %s must be a contiguous int32 tensor' % name)
        if tuple(t.shape) != shape:
            raise ValueError('mbr_select: %s must be %r, got %r' % (name, shape, tuple(t.shape)))
    if posterior == 0:
        if scores is None:
            raise ValueError("mbr_select: posterior 'softmax' needs the scores")
        if scores.dtype != torch.float32 or not scores.is_contiguous():
            raise TypeError('mbr_select: scores must be a contiguous float32 tensor')
        if tuple(scores.shape) != (N, K):
            raise ValueError('mbr_select: scores must be %r, got %r' % ((N, K), tuple(scores.shape)))
    else:
        scores = None
    if N > 65535 or not mbr_fits(K, hmax):
        raise ValueError('mbr_select: %d utterances of %d hypotheses of %d columns exceed the kernel\'s 65535, %d, %d '
                         '(and %d tokens per utterance)' % (N, K, hmax, MBR_MAX_HYPS, MBR_MAX_LEN, MBR_MAX_TOKENS))
    dev = chars.device
    best = torch.empty(N, device=dev, dtype=torch.int32)
    risk = torch.empty(N, K, device=dev, dtype=torch.float32)
    pair = torch.empty(N, K, K, 2, device=dev, dtype=torch.int32)
    check(lib.ssasr_mbr_select(_p(chars), max(hyp_ld, hmax), _p(n_chars), _p(n_hyps), _p(scores), N, K, hmax,
                               int(first_char), int(space), unit, posterior, scale, _p(best), _p(risk), _p(pair),
                               _stream()), 'ssasr_mbr_select')
    return best, risk, pair


# ---------------------------------------------------------------------------
# MWER training (build-defined; include/ssasr.h, "MWER training")
# ---------------------------------------------------------------------------
MWER_MAX_ROWS = 33             # ssasr_mwer_loss_fwd's limit on the rows of a group


class MWERInfo:
    """What ssasr_mwer_loss_fwd left on the device beside the loss: risk [G] float (the expected risk per group),
    p_hat [R], logp [R] and weight [R] double (views of the workspace: the set's posterior, the rows'
    log-probabilities and their sequence-level weights), lse [R, U] float."""
    __slots__ = ('risk', 'p_hat', 'logp', 'weight', 'lse', 'ws')


class _MWERLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, rows, n_hyps, counts, unit, ce_w, info, posterior=0):
        lib = _lib.load()
        R, U, V = logits.shape
        G = n_hyps.shape[0]
        M = R // G if G else 1
        dev = logits.device
        need = int(lib.ssasr_mwer_ws_bytes(G, M, U))
        if G and need <= 0:
            raise ValueError('mwer_loss: no kernel for %d groups of %d rows, %d steps (1 <= rows <= %d, '
                             'groups * rows <= 65535)' % (G, M, U, MWER_MAX_ROWS))
        ws = torch.empty(max(need // 8, 1), device=dev, dtype=torch.float64)
        risk = torch.empty(G, device=dev, dtype=torch.float32)
        loss = torch.empty((), device=dev, dtype=torch.float32)
        if posterior:
            check(lib.ssasr_mwer_loss_fwd_ex(_p(logits), _p(rows), rows.stride(0), rows.shape[1], _p(n_hyps),
                                             _p(counts), unit, _p(ce_w), G, M, U, V, _p(ws), need, _p(risk), _p(loss),
                                             posterior, _stream()), 'ssasr_mwer_loss_fwd_ex')
        else:
            check(lib.ssasr_mwer_loss_fwd(_p(logits), _p(rows), rows.stride(0), rows.shape[1], _p(n_hyps), _p(counts),
                                          unit, _p(ce_w), G, M, U, V, _p(ws), need, _p(risk), _p(loss), _stream()),
                  'ssasr_mwer_loss_fwd')
        info.ws, info.risk = ws, risk
        info.logp, info.p_hat, info.weight = ws[:R], ws[R:2 * R], ws[2 * R:3 * R]
        info.lse = ws[3 * R + 2 * G + 8 * R + R * U:].view(torch.float32)[:R * U].view(R, U)
        ctx.save_for_backward(logits, rows, ws)
        ctx.geom = (G, M, need)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        lib = _lib.load()
        logits, rows, ws = ctx.saved_tensors
        G, M, need = ctx.geom
        R, U, V = logits.shape
        dloss = dloss.to(torch.float32).contiguous()
        dlogits = torch.empty_like(logits)
        check(lib.ssasr_mwer_loss_bwd(_p(logits), _p(rows), rows.stride(0), rows.shape[1], G, M, U, V, _p(ws), need,
                                      _p(dloss), _p(dlogits), _stream()), 'ssasr_mwer_loss_bwd')
        return dlogits, None, None, None, None, None, None, None


MWER_POSTERIORS = {'renorm': 0, 'uniform': 1}


def mwer_loss(logits, rows, n_hyps, counts, unit, ce_w=None, posterior='renorm'):
    """The MWER loss of include/ssasr.h (ssasr_mwer_loss_fwd / _bwd; postprocess.mwer_reference is its float64
    restatement).  logits [R, U, V] float32 of R = G * M teacher-forced rows, row g * M + k being candidate k of
    group g; rows int32 [R, >= U + 1], the rows' label matrix (the label of step t is rows[r, t + 1], 0 unlabelled);
    n_hyps int32 [G]: the first clamp(n_hyps[g], 0, M) rows of a group are its hypothesis set; counts int32 [R, 8]:
    edit_score's result; unit 'char' | 'word' (or 0 | 1); ce_w float32 [R] or None: absolute weights of the rows'
    negative log-likelihoods.  posterior 'renorm': the set's posterior is the softmax of the rows' log-probabilities
    (an n-best list); 'uniform': every member weighs 1 / |set| (samples drawn from the model, ssasr_mwer_loss_fwd_ex's
    Monte-Carlo form: the loss VALUE is the mean risk plus the CE terms, the gradient is the score-function estimate).
    -> (loss, MWERInfo): the loss tensor carries the graph, the info is for logging."""
    _need_gpu(logits, rows, n_hyps, counts, ce_w)
    if posterior not in MWER_POSTERIORS:
        raise ValueError("mwer_loss: posterior must be 'renorm' or 'uniform', got %r" % (posterior,))
    unit = {'char': 0, 'word': 1}.get(unit, unit)
    if unit not in (0, 1):
        raise ValueError("mwer_loss: unit must be 'char' or 'word', got %r" % (unit,))
    logits = _f32c(logits)
    if logits.dim() != 3:
        raise ValueError('mwer_loss: logits must be [rows, steps, classes]')
    R, U, V = logits.shape
    if rows.dtype != torch.int32 or rows.dim() != 2 or rows.stride(1) != 1 or rows.shape[0] != R or rows.shape[1] < U + 1:
        raise TypeError('mwer_loss: rows must be int32 [%d, >= %d] with unit column stride' % (R, U + 1))
    for name, t, shape in (('n_hyps', n_hyps, None), ('counts', counts, (R, 8))):
        if t.dtype != torch.int32 or not t.is_contiguous() or (shape is not None and tuple(t.shape) != shape):
            raise TypeError('mwer_loss: %s must be a contiguous int32 tensor%s' % (name, '' if shape is None else ' of shape %r' % (shape,)))
    G = n_hyps.shape[0]
    if n_hyps.dim() != 1 or (G == 0) != (R == 0) or (G and R % G):
        raise ValueError('mwer_loss: %d rows do not form %d equal groups' % (R, G))
    if ce_w is not None:
        ce_w = _f32c(ce_w)
        if tuple(ce_w.shape) != (R,):
            raise ValueError('mwer_loss: ce_w must hold one weight per row')
    info = MWERInfo()
    return _MWERLoss.apply(logits, rows, n_hyps, counts, unit, ce_w, info, MWER_POSTERIORS[posterior]), info


def mwer_pack(chars, n_chars, n_hyps, y_ref, eos, L=None):
    """ssasr_mwer_pack: an n-best list (decode_beam's chars [N, K, steps], n_chars [N, K], n_hyps [N], int32) and the
    batch's label matrix y_ref [N, ref_cols] (int32, <sos> column first, 0-padded) -> (rows int32 [N * (K + 1), L],
    hyp_lens int32 [N * (K + 1)]): per utterance its K hypothesis rows `0, chars, eos, 0 ...` (all 0 from n_hyps on)
    and then its reference row; hyp_lens is what edit_score needs for rows[:, 1:] (include/ssasr.h).
    L: the row length, by default max(steps + 2, ref_cols), its minimum."""
    lib = _lib.load()
    _need_gpu(chars, n_chars, n_hyps, y_ref)
    for name, t in (('chars', chars), ('n_chars', n_chars), ('n_hyps', n_hyps)):
        if t.dtype != torch.int32 or not t.is_contiguous():
            raise TypeError('mwer_pack: %s must be a contiguous int32 tensor' % name)
    if y_ref.dtype != torch.int32 or y_ref.dim() != 2 or (y_ref.shape[1] > 1 and y_ref.stride(1) != 1):
        raise TypeError('mwer_pack: y_ref must be an int32 matrix with unit column stride')
    N, K, steps = chars.shape
    if tuple(n_chars.shape) != (N, K) or tuple(n_hyps.shape) != (N,) or y_ref.shape[0] != N:
        raise ValueError('mwer_pack: chars [N, K, steps], n_chars [N, K], n_hyps [N] and y_ref [N, cols] disagree')
    ref_cols = y_ref.shape[1]
    if L is None:
        L = max(steps + 2, ref_cols)
    rows = torch.empty(N * (K + 1), L, device=chars.device, dtype=torch.int32)
    hyp_lens = torch.empty(N * (K + 1), device=chars.device, dtype=torch.int32)
    ref_ld = y_ref.stride(0) if N > 1 else max(ref_cols, 1)
    check(lib.ssasr_mwer_pack(_p(chars), _p(n_chars), _p(n_hyps), _p(y_ref), max(ref_ld, ref_cols), ref_cols, N, K,
                              steps, int(eos), L, _p(rows), _p(hyp_lens), _stream()), 'ssasr_mwer_pack')
    return rows, hyp_lens


class _RowsRepeat(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, M):
        lib = _lib.load()
        G = t.shape[0]
        n = t[0].numel() if G else 1
        out = torch.empty((G * M,) + tuple(t.shape[1:]), device=t.device, dtype=t.dtype)
        check(lib.ssasr_rows_repeat_fwd(_p(t), G, M, n, _p(out), _stream()), 'ssasr_rows_repeat_fwd')
        ctx.geom = (G, M, n)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        G, M, n = ctx.geom
        dout = _f32c(dout)
        dt = torch.empty((G,) + tuple(dout.shape[1:]), device=dout.device, dtype=torch.float32)
        check(lib.ssasr_rows_repeat_bwd(_p(dout), G, M, n, _p(dt), _stream()), 'ssasr_rows_repeat_bwd')
        return dt, None


def rows_repeat(t, M):
    """torch.repeat_interleave(t, M, dim=0) for a float32 or int32 tensor [G, ...] (ssasr_rows_repeat_fwd: a bit
    copy); the backward of a float32 tensor adds each group's M rows in row order (ssasr_rows_repeat_bwd:
    deterministic, no atomics)."""
    _need_gpu(t)
    if t.dtype not in (torch.float32, torch.int32) or t.dim() < 1:
        raise TypeError('rows_repeat: a float32 or int32 tensor with a row axis, got %s' % t.dtype)
    M = int(M)
    if M < 1:
        raise ValueError('rows_repeat: M must be >= 1, got %d' % M)
    t = t if t.is_contiguous() else t.contiguous()
    if t.dtype == torch.int32:
        return _RowsRepeat.apply(t.detach(), M)
    return _RowsRepeat.apply(t, M)


# ---------------------------------------------------------------------------
# n-best rescoring (build-defined; include/ssasr.h, "n-best rescoring")
# ---------------------------------------------------------------------------
RESCORE_MAX_ROWS = 33          # ssasr_rescore's limit on the rows of a group
RESCORE_LOOP_ROWS = 32         # rows of one teacher-forced decoder_loop call: the persistent loop's limit (B <= 32)
RESCORE_MAX_CALLS = 5          # more persistent calls than this are slower than one call over all rows


def rescore_launch(logits, lm_logits, rows, n_hyps, first, chars, n_chars, *, att_weight=1.0, lm_weight=0.0,
                   first_weight=0.0, length_bonus=0.0):
    """ssasr_rescore: scores, ranks and reorders each utterance's list in one launch (include/ssasr.h;
    postprocess.rescore_reference is its float64 restatement).  logits [R, U, V] float32 of R = G * M teacher-forced
    rows (row g * M + k: candidate k of group g); lm_logits None or a float32 tensor indexed [R, U, V] with unit
    stride over V and any row / step strides (charlm_chunk's [U, R, V] as .permute(1, 0, 2)); rows int32 [R, >= U + 1],
    the rows' label matrix; n_hyps int32 [G]; first float32 [G, K]; chars int32 [G, K, steps]; n_chars int32 [G, K];
    K <= M.  -> (order int32 [G, K], total [G, K], parts [G, K, 3] = (att, lm, first), chars [G, K, steps],
    n_chars [G, K], n_hyps [G]) on the device, the list in rank order.  No autograd."""
    lib = _lib.load()
    _need_gpu(logits, lm_logits, rows, n_hyps, first, chars, n_chars)
    weights = [float(w) for w in (att_weight, lm_weight, first_weight, length_bonus)]
    if not all(math.isfinite(w) for w in weights):
        raise ValueError('rescore: the weights must be finite, got %r' % (weights,))
    logits = _f32c(logits.detach())
    if logits.dim() != 3:
        raise ValueError('rescore: logits must be [rows, steps, classes]')
    R, U, V = logits.shape
    if rows.dtype != torch.int32 or rows.dim() != 2 or rows.stride(1) != 1 or rows.shape[0] != R or rows.shape[1] < U + 1:
        raise TypeError('rescore: rows must be int32 [%d, >= %d] with unit column stride' % (R, U + 1))
    if chars.dtype != torch.int32 or chars.dim() != 3 or not chars.is_contiguous():
        raise TypeError('rescore: chars must be a contiguous int32 tensor [G, K, steps]')
    G, K, steps = chars.shape
    for name, t, shape in (('n_chars', n_chars, (G, K)), ('n_hyps', n_hyps, (G,))):
        if t.dtype != torch.int32 or not t.is_contiguous() or tuple(t.shape) != shape:
            raise TypeError('rescore: %s must be a contiguous int32 tensor of shape %r' % (name, shape))
    first = _f32c(first.detach())
    if tuple(first.shape) != (G, K):
        raise ValueError('rescore: first must be %r, got %r' % ((G, K), tuple(first.shape)))
    if (G == 0) != (R == 0) or (G and R % G):
        raise ValueError('rescore: %d rows do not form %d equal groups' % (R, G))
    M = R // G if G else K
    need = int(lib.ssasr_rescore_ws_bytes(G, K, U))
    if need < 0 or not K <= M <= RESCORE_MAX_ROWS or steps < 1:
        raise ValueError('rescore: no kernel for %d groups of %d rows, %d candidates, %d steps (1 <= candidates <= %d, '
                         'candidates <= rows <= %d)' % (G, M, K, U, MAX_BEAM, RESCORE_MAX_ROWS))
    lm_row = lm_step = 0
    if lm_logits is not None:
        if lm_logits.dtype != torch.float32 or tuple(lm_logits.shape) != (R, U, V) or (V > 1 and lm_logits.stride(2) != 1):
            raise TypeError('rescore: lm_logits must be float32, indexed %r with unit stride over the classes'
                            % ((R, U, V),))
        lm_logits = lm_logits.detach()
        lm_row, lm_step = max(lm_logits.stride(0), V), max(lm_logits.stride(1), V)
    dev = logits.device
    ws = torch.empty(need // 8, device=dev, dtype=torch.float64) if need else None
    order = torch.empty(G, K, device=dev, dtype=torch.int32)
    total = torch.empty(G, K, device=dev, dtype=torch.float32)
    parts = torch.empty(G, K, 3, device=dev, dtype=torch.float32)
    chars_out, n_chars_out, n_hyps_out = torch.empty_like(chars), torch.empty_like(n_chars), torch.empty_like(n_hyps)
    check(lib.ssasr_rescore(_p(logits), _p(lm_logits), lm_row, lm_step, _p(rows), rows.stride(0), rows.shape[1],
                            _p(n_hyps), _p(first), _p(chars), _p(n_chars), G, M, K, U, V, steps, *weights, _p(ws), need,
                            _p(order), _p(total), _p(parts), _p(chars_out), _p(n_chars_out), _p(n_hyps_out), _stream()),
          'ssasr_rescore')
    return order, total, parts, chars_out, n_chars_out, n_hyps_out


def rescore_loop_rows(T):
    """Rows per teacher-forced call that keep the decode loop in its single-launch persistent form: 32 up to 128
    encoder frames, beyond that what the long form's B * ceil(T' / 64) <= 192 leaves."""
    return RESCORE_LOOP_ROWS if T <= 128 else max(1, min(RESCORE_LOOP_ROWS, 192 // ((T + 63) // 64)))


def rescore_logits(feat, enc_len, params, psi, rows, M, U, *, loop_rows=None):
    """The teacher-forced pass of rescore(): feat [N, T', E] and enc_len int32 [N] repeated M times, the decode loop
    over the N * M rows of `rows` for U steps, every step in mode 0, without grad.  loop_rows: rows per decoder_loop
    call; 0: ONE call over all rows (past 32 rows one launch per stage and step); None: the faster of the two as
    measured -- calls of rescore_loop_rows(T') rows, each the single-launch persistent loop, up to
    RESCORE_MAX_CALLS of them (0.55 ms each at 68 steps: 2.8 ms for 160 rows beside 3.0 ms), one call beyond (3.3 ms
    for 256 rows beside 4.2 ms).
    -> logits [N * M, U, V]."""
    with torch.no_grad():
        comp = attn_precompute(_f32c(feat.detach()), psi[0].detach(), psi[1].detach())
        feat_r, comp_r, len_r = rows_repeat(feat.detach(), M), rows_repeat(comp, M), rows_repeat(enc_len, M)
        R = rows.shape[0]
        step = R if loop_rows == 0 else int(loop_rows or rescore_loop_rows(feat.shape[1]))
        if loop_rows is None and (R + step - 1) // step > RESCORE_MAX_CALLS:
            step = R
        modes = [0] * U
        modes_dev = torch.zeros(U, device=feat.device, dtype=torch.int32)
        out = [decoder_loop(feat_r[lo:lo + step], comp_r[lo:lo + step], len_r[lo:lo + step], rows[lo:lo + step], modes,
                            None, params, modes_dev=modes_dev)[0] for lo in range(0, R, step)]
        return out[0] if len(out) == 1 else torch.cat(out, 0)


def rescore(feat, enc_len, params, psi, chars, n_chars, n_hyps, first, eos, lm=None, *, att_weight=1.0, lm_weight=0.0,
            first_weight=0.0, length_bonus=0.0, loop_rows=None, drop_idle=True):
    """Attention rescoring of an n-best list (include/ssasr.h, "n-best rescoring"): the K texts per utterance in
    chars [N, K, steps] / n_chars [N, K] / n_hyps [N] (int32, as the decoders leave them) with their first-pass scores
    first [N, K] are packed into teacher rows (mwer_pack with an empty reference), teacher-forced through the Speller
    on the encoder output feat [N, T', E] (rescore_logits) and, with lm and lm_weight != 0, through the CharLM
    (charlm_chunk), then scored, ranked and reordered by one rescore_launch.  The one integer the host reads is the
    longest text's length.  drop_idle: the empty reference row of each packed group is left out of the loop (M = K
    rows per utterance instead of K + 1).  -> rescore_launch's six tensors."""
    _need_gpu(feat, enc_len, chars, n_chars, n_hyps, first)
    chars, n_chars, n_hyps = [t.to(torch.int32).contiguous() for t in (chars, n_chars, n_hyps)]
    N, K, steps = chars.shape
    with torch.no_grad():
        rows, hyp_lens = mwer_pack(chars, n_chars, n_hyps, torch.empty(N, 0, device=chars.device, dtype=torch.int32), eos)
        U = int(hyp_lens.max()) + 1
        M = K + 1
        if drop_idle:
            rows, M = rows.view(N, K + 1, -1)[:, :K].reshape(N * K, -1), K
        logits = rescore_logits(feat, enc_len, params, psi, rows, M, U, loop_rows=loop_rows)
        lm_logits = None
        if lm is not None and float(lm_weight) != 0.0:
            lm_logits = charlm_chunk(lm, rows[:, 1:U + 1].contiguous(), want_logits=True).logits.permute(1, 0, 2)
        return rescore_launch(logits, lm_logits, rows, n_hyps, first, chars, n_chars, att_weight=att_weight,
                              lm_weight=lm_weight, first_weight=first_weight, length_bonus=length_bonus)


# ---------------------------------------------------------------------------
# misc
# ---------------------------------------------------------------------------
def frame_lengths(x):
    """prepare_x length recovery on the device (src/ASRDataset.py:314) -> int32 [B]."""
    lib = _lib.load()
    _need_gpu(x)
    x = _f32c(x)
    B, T, F = x.shape
    lens = torch.empty(B, device=x.device, dtype=torch.int32)
    check(lib.ssasr_frame_lengths(_p(x), B, T, F, _p(lens), _stream()), 'ssasr_frame_lengths')
    return lens


def gather_batch(frames, offsets, lens, T):
    """[B, T, F] zero-padded batch from a device-resident corpus (see include/ssasr.h).
    frames [rows, F] float32, offsets int64 [B], lens int32 [B], all on the GPU."""
    lib = _lib.load()
    _need_gpu(frames, offsets, lens)
    B, F = offsets.shape[0], frames.shape[1]
    out = torch.empty(B, T, F, device=frames.device, dtype=torch.float32)
    check(lib.ssasr_gather_batch(_p(frames), _p(offsets), _p(lens), B, T, F, _p(out), _stream()),
          'ssasr_gather_batch')
    return out


def specaug_params(spec, epoch=0):
    """struct ssasr_specaug from a dict of its fields (n_freq, max_freq, n_time, max_time, fill, seed, and the
    time cap as `time_ratio` in [0, 1] -> time_permille = round(1000 * ratio), or `time_permille` itself)."""
    spec = dict(spec)
    if 'time_ratio' in spec:
        spec['time_permille'] = int(round(1000 * spec.pop('time_ratio')))
    unknown = set(spec) - {f[0] for f in _lib.SpecAug._fields_}
    if unknown:
        raise ValueError('spec_augment: unknown keys %s' % sorted(unknown))
    return _lib.SpecAug(int(spec.get('n_freq', 0)), int(spec.get('max_freq', 0)), int(spec.get('n_time', 0)),
                        int(spec.get('max_time', 0)), int(spec.get('time_permille', 1000)),
                        float(spec.get('fill', 0.0)), int(spec.get('seed', 0)), int(spec.get('epoch', epoch)))


def specaug_plan(spec, utt_id, length, F):
    """The (start, width) rows of one utterance's masks, frequency masks first (ssasr_specaug_plan: host only)."""
    import ctypes
    lib = _lib.load()
    n = spec.n_freq + spec.n_time
    masks = (ctypes.c_int32 * (2 * max(n, 1)))()
    check(lib.ssasr_specaug_plan(ctypes.byref(spec), utt_id, length, F, masks), 'ssasr_specaug_plan')
    return [(masks[2 * j], masks[2 * j + 1]) for j in range(n)]


def gather_batch_aug(frames, offsets, lens, utt_ids, T, spec, out=None):
    """gather_batch with the utterances' SpecAugment masks applied in the same pass (see include/ssasr.h).
    utt_ids int32 [B] on the GPU: corpus indices; spec: a _lib.SpecAug (specaug_params); out: the [B, T, F]
    float32 tensor to fill, allocated when None."""
    import ctypes
    lib = _lib.load()
    _need_gpu(frames, offsets, lens, utt_ids)
    B, F = offsets.shape[0], frames.shape[1]
    if out is None:
        out = torch.empty(B, T, F, device=frames.device, dtype=torch.float32)
    elif out.shape != (B, T, F) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != frames.device:
        raise ValueError('gather_batch_aug: out must be a contiguous float32 [B, T, F] tensor on the frames\' device')
    if utt_ids.dtype != torch.int32 or utt_ids.shape != (B,) or not utt_ids.is_contiguous():
        raise TypeError('gather_batch_aug: utt_ids must be a contiguous int32 [B] tensor')
    check(lib.ssasr_gather_batch_aug(_p(frames), _p(offsets), _p(lens), _p(utt_ids), B, T, F, ctypes.byref(spec),
                                     _p(out), _stream()), 'ssasr_gather_batch_aug')
    return out


def clip_adadelta_(param, grad, square_avg, acc_delta, ws, stats, grad_scale=1.0, max_norm=5.0,
                   lr=1.0, rho=0.9, eps=1e-8, zero_grad=False):
    """Solver.step on flat buffers (src/trainer.py:131-148).  stats <- [norm, skipped]."""
    lib = _lib.load()
    _need_gpu(param, grad, square_avg, acc_delta, ws, stats)
    check(lib.ssasr_clip_adadelta(_p(param), _p(grad), _p(square_avg), _p(acc_delta), param.numel(),
                                  grad_scale, float(max_norm), lr, rho, eps, _p(ws), _p(stats),
                                  1 if zero_grad else 0, _stream()), 'ssasr_clip_adadelta')


def adam_prepare(clip_grad, state_step, ws, stats, grad_scale=1.0, max_norm=5.0, lr=1e-4, betas=(0.9, 0.999)):
    """First half of Solver.step + torch.optim.Adam on flat buffers (include/ssasr.h, ssasr_adam_prepare):
    norm / NaN guard / clip coefficient over `clip_grad`, step count and bias corrections."""
    lib = _lib.load()
    _need_gpu(clip_grad, state_step, ws, stats)
    check(lib.ssasr_adam_prepare(_p(clip_grad), clip_grad.numel(), grad_scale, float(max_norm), lr, betas[0], betas[1],
                                 _p(state_step), _p(ws), _p(stats), _stream()), 'ssasr_adam_prepare')


def adam_update_(param, grad, exp_avg, exp_avg_sq, ws, stats, clipped, grad_scale=1.0, betas=(0.9, 0.999), eps=1e-8,
                 zero_grad=False):
    """The Adam update of one flat buffer (ssasr_adam_update); `clipped`: this buffer is the range whose norm
    adam_prepare clipped."""
    lib = _lib.load()
    _need_gpu(param, grad, exp_avg, exp_avg_sq, ws, stats)
    check(lib.ssasr_adam_update(_p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), param.numel(), _p(ws),
                                1 if clipped else 0, grad_scale, betas[0], betas[1], eps, _p(stats),
                                1 if zero_grad else 0, _stream()), 'ssasr_adam_update')


def clip_adadelta_ws(n, device):
    lib = _lib.load()
    return torch.empty(int(lib.ssasr_clip_adadelta_ws(n)), device=device, dtype=torch.float32)


# ---------------------------------------------------------------------------
# inference: CharLM step, single-launch greedy and beam-search decode (csrc/infer.hip)
# ---------------------------------------------------------------------------
_CHARLM_NAMES = ('emb.weight', 'layer_1.weight_ih', 'layer_1.weight_hh', 'layer_1.bias_ih', 'layer_1.bias_hh',
                 'layer_2.weight_ih', 'layer_2.weight_hh', 'layer_2.bias_ih', 'layer_2.bias_hh', 'out.weight', 'out.bias')


def _charlm_struct(lm):
    """(struct ssasr_charlm, the tensors it points into) of a charlm.CharLM."""
    params = dict(lm.named_parameters())
    keep = [_f32c(params[n].detach()) for n in _CHARLM_NAMES]
    _need_gpu(*keep)
    s = _lib.CharLM(lm.input_size, lm.hidden_size, *[t.data_ptr() for t in keep])
    return s, keep


def charlm_step(lm, x, h_1, h_2):
    """CharLM.forward (src/charlm.py:46-57): x [B] character ids, h_1 / h_2 [B, H] -> (out [B, V], h_1', h_2')."""
    lib = _lib.load()
    _need_gpu(x, h_1, h_2)
    s, keep = _charlm_struct(lm)
    B = x.shape[0]
    x32, h_1, h_2 = as_i32(x.reshape(B)), _f32c(h_1), _f32c(h_2)
    out = torch.empty(B, lm.input_size, device=x.device, dtype=torch.float32)
    n1, n2 = torch.empty_like(h_1), torch.empty_like(h_2)
    check(lib.ssasr_charlm_step(C.byref(s), _p(x32), _p(h_1), _p(h_2), B, _p(out), _p(n1), _p(n2), _stream()),
          'ssasr_charlm_step')
    return out, n1, n2


def _decode_struct(cls, feat, enc_len, params, psi, lm, lm_weight, eos, max_steps):
    """What decode_greedy and beam_struct share: a _lib.Infer / _lib.Beam (cls) with the sizes, the inputs, comp,
    the parameters, the language model and eos filled in -> (struct, the tensors and structs it points into)."""
    feat = _f32c(feat)
    _need_gpu(feat, enc_len)
    N, T, E = feat.shape
    A, D = params['w_phi'].shape
    keep = {k: _f32c(v.detach()) for k, v in params.items()}
    w_psi, b_psi = _f32c(psi[0].detach()), _f32c(psi[1].detach())
    comp = torch.empty(N, T, A, device=feat.device, dtype=torch.float32)
    d = cls()
    d.N, d.T, d.E, d.A, d.D, d.V, d.max_steps = N, T, E, A, D, params['w_ct'].shape[0], int(max_steps)
    d.feat, d.enc_len, d.comp = feat.data_ptr(), enc_len.data_ptr(), comp.data_ptr()
    d.w_psi, d.b_psi = w_psi.data_ptr(), b_psi.data_ptr()
    for k, v in keep.items():
        setattr(d, k, v.data_ptr())
    lm_keep = None
    if lm is not None:
        lm_keep = _charlm_struct(lm)
        d.lm = C.pointer(lm_keep[0])
        d.lm_weight = float(lm_weight)
    d.eos = int(eos)
    return d, (feat, enc_len, keep, w_psi, b_psi, comp, lm_keep)


def decode_greedy(feat, enc_len, params, psi, lm, lm_weight, eos, max_steps, want_att=True):
    """ssasr_decode_greedy over feat [N, T, E] (each utterance encoded alone) and enc_len int32 [N]:
    -> (chars [N, max_steps] int32, n_chars [N] int32, scores [N, max_steps, V], att [N, max_steps, T] or None).
    params: ASR._decoder_params(); psi: (weight, bias); lm: a charlm.CharLM or None."""
    lib = _lib.load()
    d, keep = _decode_struct(_lib.Infer, feat, enc_len, params, psi, lm, lm_weight, eos, max_steps)
    dev = keep[0].device
    chars = torch.empty(d.N, d.max_steps, device=dev, dtype=torch.int32)
    n_chars = torch.empty(d.N, device=dev, dtype=torch.int32)
    scores = torch.empty(d.N, d.max_steps, d.V, device=dev, dtype=torch.float32)
    att = torch.empty(d.N, d.max_steps, d.T, device=dev, dtype=torch.float32) if want_att else None
    d.chars, d.n_chars, d.scores = chars.data_ptr(), n_chars.data_ptr(), scores.data_ptr()
    d.att = att.data_ptr() if want_att else None
    check(lib.ssasr_decode_greedy(C.byref(d), _stream()), 'ssasr_decode_greedy')
    return chars, n_chars, scores, att


MAX_BEAM = 32


def beam_struct(feat, enc_len, params, psi, lm, lm_weight, eos, max_steps, beam_size, ws=None, ctc=False,
                coverage=False, size_query=None):
    """(struct ssasr_beam, its outputs (chars, n_chars, hyp_scores, n_hyps), the tensors it points into) for
    decode_beam's arguments; the outputs are allocated, not yet written.  The workspace is sized by
    ssasr_decode_beam_ex_ws_bytes for the CTC form (ctc) and the coverage block (coverage), or by size_query, another
    entry's query over the same nine sizes (ssasr_decode_sample_ws_bytes).  Sizes no entry takes are refused before
    anything else is looked at."""
    lib = _lib.load()
    (N, T, E), (A, D), V = feat.shape, params['w_phi'].shape, params['w_ct'].shape[0]
    K, S, hl = int(beam_size), int(max_steps), lm.hidden_size if lm is not None else 0
    sizes = (N, K, T, E, A, D, V, hl, S)
    if size_query is None:
        entry, need = 'ssasr_decode_beam', lib.ssasr_decode_beam_ex_ws_bytes(*sizes, int(bool(ctc)), int(bool(coverage)))
    else:
        entry, need = size_query.__name__[:-len('_ws_bytes')], size_query(*sizes)
    if need <= 0:
        raise RuntimeError('%s: invalid argument (beam size %d, sizes N %d T %d E %d A %d D %d V %d H %d steps %d)'
                           % (entry, K, N, T, E, A, D, V, hl, S))
    d, keep = _decode_struct(_lib.Beam, feat, enc_len, params, psi, lm, lm_weight, eos, S)
    dev = keep[0].device
    if ws is None:
        ws = torch.empty(need // 4, device=dev, dtype=torch.float32)
    _need_gpu(ws)
    chars = torch.empty(N, K, S, device=dev, dtype=torch.int32)
    n_chars = torch.empty(N, K, device=dev, dtype=torch.int32)
    hyp_scores = torch.empty(N, K, device=dev, dtype=torch.float32)
    n_hyps = torch.empty(N, device=dev, dtype=torch.int32)
    d.K, d.ws, d.ws_bytes = K, ws.data_ptr(), ws.numel() * ws.element_size()
    d.chars, d.n_chars, d.hyp_scores, d.n_hyps = (chars.data_ptr(), n_chars.data_ptr(), hyp_scores.data_ptr(),
                                                  n_hyps.data_ptr())
    return d, (chars, n_chars, hyp_scores, n_hyps), keep + (ws,)


def decode_beam(feat, enc_len, params, psi, lm, lm_weight, eos, max_steps, beam_size, ws=None):
    """ssasr_decode_beam over feat [N, T, E] (each utterance encoded alone) and enc_len int32 [N] with
    1 <= beam_size <= 32 hypotheses per utterance:
    -> (chars [N, K, max_steps] int32, n_chars [N, K] int32, hyp_scores [N, K], n_hyps [N] int32), hypotheses
    best first, unused slots zero.  params, psi, lm: as for decode_greedy.  ws: a float32 workspace of at least
    ssasr_decode_beam_ws_bytes bytes, or None to allocate one."""
    d, outs, keep = beam_struct(feat, enc_len, params, psi, lm, lm_weight, eos, max_steps, beam_size, ws)
    check(_lib.load().ssasr_decode_beam(C.byref(d), _stream()), 'ssasr_decode_beam')
    return outs


def decode_sample(feat, enc_len, params, psi, lm, lm_weight, eos, max_steps, n_samples, uniforms, temperature=1.0):
    """ssasr_decode_sample over feat [N, T, E] (each utterance encoded alone) and enc_len int32 [N]: 1 <= n_samples
    <= 32 samples per utterance drawn from softmax(score row / temperature), sample (n, k) taking step s's uniform
    from uniforms[n, k, s] (float32 [N, n_samples, max_steps] in [0, 1), on the device).
    -> (chars [N, K, max_steps] int32 in slot order, n_chars [N, K] int32, hyp_scores [N, K] (the beam search's score
    of that text), n_hyps [N] int32 (= K), logq [N, K]: the draws' log-probability under the sampled distribution).
    params, psi, lm: as for decode_greedy."""
    lib = _lib.load()
    d, outs, keep = beam_struct(feat, enc_len, params, psi, lm, lm_weight, eos, max_steps, n_samples,
                                size_query=lib.ssasr_decode_sample_ws_bytes)
    _need_gpu(uniforms)
    if uniforms.dtype != torch.float32 or tuple(uniforms.shape) != tuple(outs[0].shape):
        raise ValueError('decode_sample: uniforms must be float32 %r, got %s %r'
                         % (list(outs[0].shape), uniforms.dtype, tuple(uniforms.shape)))
    uniforms = uniforms.contiguous()
    logq = torch.empty_like(outs[2])
    s = _lib.Sample(uniforms.data_ptr(), float(temperature), logq.data_ptr())
    check(lib.ssasr_decode_sample(C.byref(d), C.byref(s), _stream()), 'ssasr_decode_sample')
    return outs + (logq,)


CTC_BLANK = 0      # class 0, as in training (ctc.BLANK)


def ctc_prefix_struct(ctc, blank=CTC_BLANK):
    """(struct ssasr_ctc_prefix, the tensors it points into) of ctc = (ctc_head weight [V, E], bias [V], ctc_weight)."""
    w, b = _f32c(ctc[0].detach()), _f32c(ctc[1].detach())
    _need_gpu(w, b)
    return _lib.CtcPrefix(w.data_ptr(), b.data_ptr(), float(ctc[2]), int(blank)), (w, b)


def decode_beam_ctc(feat, enc_len, params, psi, lm, lm_weight, eos, max_steps, beam_size, ctc, ws=None,
                    blank=CTC_BLANK):
    """ssasr_decode_beam_ctc: decode_beam with the CTC prefix score of ctc = (ctc_head weight [V, E], bias [V],
    ctc_weight in [0, 1]) in every candidate's score (include/ssasr.h), for 1 <= beam_size <= 32.  Same results as
    decode_beam; ws: at least ssasr_decode_beam_ctc_ws_bytes bytes, or None to allocate one."""
    d, outs, keep = beam_struct(feat, enc_len, params, psi, lm, lm_weight, eos, max_steps, beam_size, ws, ctc=True)
    c, c_keep = ctc_prefix_struct(ctc, blank)
    check(_lib.load().ssasr_decode_beam_ctc(C.byref(d), C.byref(c), _stream()), 'ssasr_decode_beam_ctc')
    return outs


def decode_beam_ex(feat, enc_len, params, psi, lm, lm_weight, eos, max_steps, beam_size, ctc=None, *, length_bonus=0.0,
                   coverage_weight=0.0, coverage_threshold=0.5, end_margin=None, ws=None, blank=CTC_BLANK):
    """ssasr_decode_beam_ex: decode_beam (ctc None) / decode_beam_ctc (ctc = (ctc_head weight, bias, ctc_weight)) with
    the length bonus added to every non-<EOS> candidate, coverage_weight * (the increase of the parent's count of
    frames whose summed attention exceeds coverage_threshold) added to every candidate, and, for end_margin >= 0
    (None: off), the loop ended once the best live score is below the best finished one by more than end_margin
    (include/ssasr.h).  -> decode_beam's four results and n_steps [N] int32, the loop iterations each utterance
    executed.  ws: at least ssasr_decode_beam_ex_ws_bytes bytes, or None to allocate one."""
    d, outs, keep = beam_struct(feat, enc_len, params, psi, lm, lm_weight, eos, max_steps, beam_size, ws,
                                ctc=ctc is not None, coverage=float(coverage_weight) != 0.0)
    n_steps = torch.empty(d.N, device=outs[0].device, dtype=torch.int32)
    t = _lib.BeamTerms(float(length_bonus), float(coverage_weight), float(coverage_threshold),
                       -1.0 if end_margin is None else float(end_margin), n_steps.data_ptr())
    c, c_keep = ctc_prefix_struct(ctc, blank) if ctc is not None else (None, None)
    check(_lib.load().ssasr_decode_beam_ex(C.byref(d), C.byref(c) if c is not None else None, C.byref(t), _stream()),
          'ssasr_decode_beam_ex')
    return outs + (n_steps,)


def decode_beam_graph(feat, enc_len, params, psi, lm, lm_weight, eos, max_steps, beam_size, ctc=None, *, graph,
                      graph_weight, length_bonus=0.0, coverage_weight=0.0, coverage_threshold=0.5, end_margin=None,
                      ws=None, blank=CTC_BLANK):
    """ssasr_decode_beam_graph: decode_beam_ex's search (ctc and every term optional) with a character graph
    (char_graph.CharGraph: an n-gram LM, hotwords, their product) in every candidate's score: graph_weight *
    arc[state][v], graph_weight * fin[state] for <EOS>, a forbidden arc never chosen (include/ssasr.h).  graph with
    n_classes == V (None is allowed at graph_weight 0), uploaded to feat's device on first use and held there;
    graph_weight finite and >= 0.  -> decode_beam_ex's five results and graph_scores [N, K] float32, each hypothesis'
    G (+ fin when <EOS> ended it).  ws: at least ssasr_decode_beam_graph_ws_bytes bytes, or None to allocate one."""
    from .char_graph import CharGraph
    graph_weight = float(graph_weight)
    if not (math.isfinite(graph_weight) and graph_weight >= 0.0):
        raise ValueError('decode_beam_graph: graph_weight must be finite and >= 0, got %r' % (graph_weight,))
    if graph is None and graph_weight != 0.0:
        raise ValueError('decode_beam_graph: graph_weight %g needs a graph' % graph_weight)
    if graph is not None and not isinstance(graph, CharGraph):
        raise TypeError('decode_beam_graph: graph must be a char_graph.CharGraph, got %s' % type(graph).__name__)
    V = params['w_ct'].shape[0]
    if graph is not None and graph.n_classes != V:
        raise ValueError('decode_beam_graph: the graph has %d classes, the model %d' % (graph.n_classes, V))
    d, outs, keep = beam_struct(feat, enc_len, params, psi, lm, lm_weight, eos, max_steps, beam_size, ws,
                                ctc=ctc is not None, coverage=float(coverage_weight) != 0.0)
    dev = outs[0].device
    n_steps = torch.empty(d.N, device=dev, dtype=torch.int32)
    graph_scores = torch.empty(d.N, d.K, device=dev, dtype=torch.float32)
    t = _lib.BeamTerms(float(length_bonus), float(coverage_weight), float(coverage_threshold),
                       -1.0 if end_margin is None else float(end_margin), n_steps.data_ptr())
    c, c_keep = ctc_prefix_struct(ctc, blank) if ctc is not None else (None, None)
    g, g_keep = graph.to(dev) if graph is not None else (None, None)
    check(_lib.load().ssasr_decode_beam_graph(C.byref(d), C.byref(c) if c is not None else None, C.byref(t),
                                              C.byref(g) if g is not None else None, graph_weight,
                                              _p(graph_scores), _stream()), 'ssasr_decode_beam_graph')
    return outs + (n_steps, graph_scores)


# ---------------------------------------------------------------------------
# CharLM training: one chunk forward / backward (csrc/charlm_train.hip)
# ---------------------------------------------------------------------------
def charlm_ws_layout(B, U, H, V):
    """{block: (offset, floats)} of the training workspace (include/ssasr.h, ssasr_charlm_train_ws_floats)."""
    R, out, o = U * B, {}, 0
    for name, n in (('g1', (V * 3 * H + 15) // 16 * 16), ('wt_hh1', 3 * H * H), ('wt_ih2', 3 * H * H),
                    ('wt_hh2', 3 * H * H), ('wt_out', 64 * H), ('h1', (U + 1) * B * H), ('h2', (U + 1) * B * H),
                    ('s1', R * 4 * H), ('s2', R * 4 * H), ('dl', R * 64), ('oh', R * 64)):
        out[name] = (o, n)
        o += n
    out['total'] = o
    return out


class CharLMChunk:
    """What charlm_chunk returns: loss_rows [B], fed int32 [U+1, B], logits [U, B, V] or None, and what
    charlm_chunk_backward needs (the workspace, y)."""
    __slots__ = ('loss_rows', 'fed', 'logits', 'ws', 'y', 'B', 'U')


def charlm_chunk(lm, y, feed=None, modes=None, uniforms=None, want_logits=False, ws=None):
    """The chunk loop of CHARLMTrainer.exec (src/trainer.py:231-249) as one launch: y [B, U] labels, feed [B, U]
    (default y), modes int32 [U] on the device (default all teacher-forced), uniforms [U, B] for the sampled
    steps.  ws: a float32 buffer of at least ssasr_charlm_train_ws_floats floats to reuse."""
    lib = _lib.load()
    _need_gpu(y, feed, modes, uniforms, ws)
    s, keep = _charlm_struct(lm)
    B, U = y.shape
    H, V = lm.hidden_size, lm.input_size
    need = int(lib.ssasr_charlm_train_ws_floats(B, U, H, V))
    if need <= 0:
        raise RuntimeError('ssasr_charlm_train_fwd: unsupported shape B %d U %d H %d V %d (V <= 64, H %% 16 == 0, '
                           '16 <= H <= 256)' % (B, U, H, V))
    assert need == charlm_ws_layout(B, U, H, V)['total']
    dev = y.device
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, device=dev, dtype=torch.float32)
    y32 = as_i32(y).contiguous()
    feed32 = y32 if feed is None else as_i32(feed).contiguous()
    if modes is None:
        modes = torch.zeros(U, device=dev, dtype=torch.int32)
    out = CharLMChunk()
    out.loss_rows = torch.empty(B, device=dev, dtype=torch.float32)
    out.fed = torch.empty(U + 1, B, device=dev, dtype=torch.int32)
    out.logits = torch.empty(U, B, V, device=dev, dtype=torch.float32) if want_logits else None
    out.ws, out.y, out.B, out.U = ws, y32, B, U
    check(lib.ssasr_charlm_train_fwd(C.byref(s), _p(y32), _p(feed32), _p(as_i32(modes)),
                                     _p(None if uniforms is None else _f32c(uniforms)), B, U, _p(out.loss_rows),
                                     _p(out.fed), _p(out.logits), _p(ws), _stream()), 'ssasr_charlm_train_fwd')
    return out


def charlm_chunk_backward(lm, chunk, dloss=None):
    """loss.backward() of src/trainer.py:250 for loss = mean(loss_rows) (dloss = 1 / B): the BPTT launch, then
    every parameter gradient as products over the workspace, ACCUMULATED into the parameters' .grad."""
    lib = _lib.load()
    s, keep = _charlm_struct(lm)
    B, U, H, V = chunk.B, chunk.U, lm.hidden_size, lm.input_size
    check(lib.ssasr_charlm_train_bwd(C.byref(s), _p(chunk.y), B, U, 1.0 / B if dloss is None else float(dloss),
                                     _p(chunk.ws), _stream()), 'ssasr_charlm_train_bwd')
    lay, R = charlm_ws_layout(B, U, H, V), U * B
    blk = lambda n: chunk.ws[lay[n][0]:lay[n][0] + lay[n][1]]
    params = dict(lm.named_parameters())
    for n in _CHARLM_NAMES:
        if params[n].grad is None:
            params[n].grad = torch.zeros_like(params[n])
    g = {n: params[n].grad for n in _CHARLM_NAMES}
    h1, h2 = blk('h1').view(U + 1, B, H), blk('h2').view(U + 1, B, H)
    h1_prev, h1_new = h1[:U].reshape(R, H), h1[1:].reshape(R, H)
    h2_prev, h2_new = h2[:U].reshape(R, H), h2[1:].reshape(R, H)
    s1, s2 = blk('s1').view(R, 4 * H), blk('s2').view(R, 4 * H)
    dl, oh = blk('dl').view(R, 64), blk('oh').view(R, 64)
    ones = torch.ones(R, 1, device=chunk.ws.device, dtype=torch.float32)

    def acc_cols(out, m, lo, hi, b):          # out += m[:, lo:hi]^T . b over the R rows (K = R), rows keep m's stride
        a = m[:, lo:hi]
        check(lib.ssasr_gemm_f32(1, 1, hi - lo, b.shape[1], R, 1.0, _p(a), m.stride(0), _p(b), b.stride(0), 1.0,
                                 _p(out), out.stride(0) if out.dim() == 2 else 1, None, 0, 1, 0, 0, 0, 1, _stream()),
              'ssasr_gemm_f32')

    col = lambda v: v.view(-1, 1)
    acc_cols(g['out.weight'], dl, 0, V, h2_new)
    acc_cols(col(g['out.bias']), dl, 0, V, ones)
    for cell, sv, x_in, h_prev in (('layer_2', s2, h1_new, h2_prev), ('layer_1', s1, None, h1_prev)):
        w_hh, b_hh = g[cell + '.weight_hh'], g[cell + '.bias_hh']
        acc_cols(w_hh[:2 * H], sv, 0, 2 * H, h_prev)
        acc_cols(w_hh[2 * H:], sv, 3 * H, 4 * H, h_prev)
        acc_cols(col(b_hh[:2 * H]), sv, 0, 2 * H, ones)
        acc_cols(col(b_hh[2 * H:]), sv, 3 * H, 4 * H, ones)
        if x_in is not None:
            acc_cols(g[cell + '.weight_ih'], sv, 0, 3 * H, x_in)
            acc_cols(col(g[cell + '.bias_ih']), sv, 0, 3 * H, ones)
    # layer 1's input side: d gi1 summed per fed character, dG [V, 3H] = onehot^T . d gi1, then through the table
    dG = torch.empty(V, 3 * H, device=chunk.ws.device, dtype=torch.float32)
    check(lib.ssasr_gemm_f32(1, 1, V, 3 * H, R, 1.0, _p(oh), 64, _p(s1), 4 * H, 0.0, _p(dG), 3 * H, None, 0, 1, 0, 0, 0,
                             1, _stream()), 'ssasr_gemm_f32')
    emb_w, w_ih1 = params['emb.weight'].detach(), params['layer_1.weight_ih'].detach()
    gemm(dG, emb_w, ta=True, tb=True, out=g['layer_1.weight_ih'], beta=1.0)           # dW_ih1 = dG^T . emb
    gemm(dG, w_ih1, ta=False, tb=True, out=g['emb.weight'], beta=1.0)                 # d emb = dG . W_ih1
    gemm(dG, torch.ones(V, 1, device=dG.device), ta=True, tb=True, out=col(g['layer_1.bias_ih']), beta=1.0)
