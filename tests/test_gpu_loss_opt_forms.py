"""Every kernel of csrc/loss_opt.hip that predates label smoothing and SpecAugment, at the sizes that pick its
branches, against float64: the plain masked CE (las_oracle.masked_ce_loss), the fused clip + Adadelta step
(las_oracle.clip_adadelta_explicit), the fused clip + Adam step (torch.optim.Adam under las_oracle.solver_step),
the frame-length recovery (las_oracle.frame_lengths) and the batch gather (a numpy gather).  Inputs are seeded
float64 draws rounded to float32 once; the float64 references see the rounded values.  Which branch a group enters:

    ce_fwd_kernel     one wave per step, lanes stride the vocabulary by 64, CE_G = 8 blocks per utterance, each
                      wave steps t by 32.  (1, 1, 2): two lanes, blocks 1..7 idle.  (3, 9, 31): V < 64, block 0
                      has a step for two of its waves.  (2, 70, 64): U > 32, a wave's second and third step, U % 8 != 0.
                      (2, 5, 130): three vocabulary passes with a tail of 2, blocks 5..7 publish a zero tail.
                      (2, 3, 257): five passes, tail of 1.  (300, 2, 7): ce_mean_kernel's serial loop over rows.
                      Every label row starts with a non-zero token (it counts in the denominator).  On top: an
                      upstream gradient of 3, y as a column view of a wider int32 tensor (y_ld > y_cols, garbage
                      on both sides), logits longer than ans_len (the wrapper's slice), logits of scale 10 and the
                      same plus 80 (the max subtraction).
    ce_bwd_kernel     one thread per logit over the same cases: 1 thread's worth of work up to several blocks.
    sumsq_kernel      float4 path (16-byte aligned gradient, whole 4096-float blocks), scalar path (the partial
                      last block; every block of a gradient that starts 4 bytes past a 16-byte boundary).
    adadelta_kernel   n = 4096 * 256 + 4096 * 5 + 3: the grid is clamped to 4096 blocks of 256 threads, 20,483
                      threads take a second grid-stride trip, the others do not.  Step and NaN-skip branch, each
                      with and without the folded zero_grad.
    adam_prepare_kernel / adam_kernel
                      clipped range of 4096 * 256 + 1237 floats (second trip, partial sumsq block, unaligned run
                      of a flat tensor) and an unclipped buffer of 777 (one trip, 4 blocks, multiplier grad_scale
                      alone); a clipped, a clipped and an unclipped step; gradients of 1e-9 (eps decides the
                      update) and exact zeros; the skipped step (state, bias corrections, zero_grad).
    frame_len_kernel  4 waves stride the frames, lanes stride F by 64: (1, 1, 1), (3, 7, 5), (2, 9, 130) with a
                      lane tail, (5, 50, 80).
    gather_batch_kernel
                      scalar path (F = 1, 3, 130, or F = 4 with frames 4 bytes past a 16-byte boundary) and
                      float4 path (F = 4: one lane; F = 80: 20 of 64 lanes busy).

Tolerances: close() of the suite (absolute for O(1) data, relative above) with the project's LOSS_TOL = 1e-6 and
GRAD_TOL = 1e-7 for the CE and the bounds of test_clip_adadelta_matches_oracle (param 2e-6, states 1e-7, norm 1e-5
relative) for both optimizers; acc_delta and Adam's moments take the bound of square_avg.  No case needed another
bound; what was measured is in DESIGN.md 4.5.  Needs an MI355X."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import las_oracle as lo

pytestmark = pytest.mark.gpu

LOSS_TOL, GRAD_TOL = 1e-6, 1e-7              # test_masked_ce_loss_forward_backward's
PARAM_TOL, STATE_TOL, NORM_RTOL = 2e-6, 1e-7, 1e-5      # test_clip_adadelta_matches_oracle's


def dev():
    return torch.device('cuda:0')


def rnd(*shape, seed=0, scale=1.0):
    """Seeded float64 normal draws, rounded to float32 once: what the device gets, as float64."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale).float().double()


def close(got, want, atol, what=''):
    got = got.detach().double().cpu()
    want = want.detach().double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = (got - want).abs().max().item()
    tol = atol * max(1.0, want.abs().max().item())     # absolute for O(1) data, relative above
    print('%-40s max abs err %.3e (allowed %.1e)' % (what, err, tol))
    assert err <= tol, '%s: max abs err %.3e > %.1e' % (what, err, tol)


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _p(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------- 1. masked CE ----
# (B, U, V) and the label count of every row: ragged, no row without a label
CE_SHAPES = [((1, 1, 2), [1]), ((3, 9, 31), [9, 5, 1]), ((2, 70, 64), [70, 33]), ((2, 5, 130), [5, 2]),
             ((2, 3, 257), [3, 1]), ((300, 2, 7), [2 - b % 2 for b in range(300)])]
CE_IDS = ['%dx%dx%d' % s for s, _ in CE_SHAPES]


def ce_labels(B, U, V, counts, seed, extra=2):
    """y [B, U + extra]: a non-zero start token in column 0 (counted by the denominator), counts[b] labels."""
    g = torch.Generator().manual_seed(seed)
    y = torch.zeros(B, U + extra, dtype=torch.long)
    y[:, 0] = 1
    for b, n in enumerate(counts):
        y[b, 1:1 + n] = torch.randint(1, V, (n,), generator=g)
    return y


def ce_reference(logits, y, U, upstream=1.0):
    """float64 loss and dlogits of the oracle (the gradient of upstream * loss)."""
    lr = logits.clone().requires_grad_(True)
    want = lo.masked_ce_loss(lr[:, :U], y, U)
    (upstream * want).backward()
    return want.detach(), lr.grad


@functools.lru_cache(maxsize=None)
def ce_case(k):
    (B, U, V), counts = CE_SHAPES[k]
    logits = rnd(B, U, V, seed=800 + k)                  # unit scale: the premise of the absolute tolerances
    y = ce_labels(B, U, V, counts, 850 + k)
    return (logits, y, U) + ce_reference(logits, y, U)


def ce_device(logits, yd, U, upstream=1.0):
    """Loss and dlogits of ops.masked_ce_loss for float64 `logits` (rounded already) and device labels `yd`."""
    from ss_asr_amd import ops
    ld = logits.float().to(dev()).requires_grad_(True)
    got = ops.masked_ce_loss(ld, yd, U)
    if upstream == 1.0:
        got.backward()                                     # the train steps' form: the cached unit gradient
    else:
        (upstream * got).backward()
    return got.detach(), ld.grad


def check_ce_steps(grad, y, U, what):
    """An unlabelled step has no gradient at all; on a labelled step the probabilities minus the one-hot sum to
    zero over V up to rounding: recorded, not asserted (the bound on dlogits is the assertion)."""
    grad = grad[:, :U].cpu()
    labelled = y[:, 1:U + 1] != 0
    assert bool((grad[~labelled] == 0).all()), '%s: gradient on an unlabelled step' % what
    sums = grad.double().sum(-1)[labelled].abs()
    print('%-40s max |sum over V of dlogits| on a labelled step %.3e' % (what, sums.max().item()))


@pytest.mark.parametrize('k', range(len(CE_SHAPES)), ids=CE_IDS)
def test_plain_ce_loss_and_gradient_against_float64(k):
    """ce_fwd_kernel, ce_mean_kernel and ce_bwd_kernel at every shape of the module docstring."""
    logits, y, U, want, dwant = ce_case(k)
    got, dgot = ce_device(logits, y.to(dev()), U)
    close(got, want, LOSS_TOL, 'loss %s' % CE_IDS[k])
    close(dgot, dwant, GRAD_TOL, 'dlogits %s' % CE_IDS[k])
    check_ce_steps(dgot, y, U, CE_IDS[k])
    assert (y[:, 1:U + 1] == 0).any() or k == 0           # the ragged rows are there


def test_plain_ce_upstream_gradient():
    """(3.0 * loss).backward(): dloss reaches ce_bwd_kernel as a device scalar other than the cached 1."""
    logits, y, U, want, _ = ce_case(1)
    _, dwant = ce_reference(logits, y, U, upstream=3.0)
    got, dgot = ce_device(logits, y.to(dev()), U, upstream=3.0)
    close(got, want, LOSS_TOL, 'loss')
    close(dgot, dwant, GRAD_TOL, 'dlogits, upstream 3')
    check_ce_steps(dgot, y, U, 'upstream 3')


def test_plain_ce_start_token_counts_in_the_denominator():
    """count(y != 0) runs over the whole label row, column 0 included: with the start token zeroed the loss of the
    same logits is another number (both against float64), so the cases above do pin the count."""
    logits, y, U, want, _ = ce_case(1)
    y0 = y.clone()
    y0[:, 0] = 0
    want0, dwant0 = ce_reference(logits, y0, U)
    got0, dgot0 = ce_device(logits, y0.to(dev()), U)
    close(got0, want0, LOSS_TOL, 'loss, y[:, 0] == 0')
    close(dgot0, dwant0, GRAD_TOL, 'dlogits, y[:, 0] == 0')
    assert abs(float(want0) - float(want)) > 0.05 * float(want)


def test_plain_ce_labels_as_a_column_view():
    """y is columns 2 .. 2 + L of a wider int32 tensor: y_ld = L + 5 > y_cols = L, the columns on both sides hold
    non-zero garbage that is neither a label nor counted."""
    logits, y, U, want, dwant = ce_case(1)
    B, L = y.shape
    wide = torch.full((B, L + 5), 7, dtype=torch.int32)
    wide[:, 2:2 + L] = y.to(torch.int32)
    view = wide.to(dev())[:, 2:2 + L]
    assert view.stride(0) == L + 5 and not view.is_contiguous()
    got, dgot = ce_device(logits, view, U)
    close(got, want, LOSS_TOL, 'loss, column view')
    close(dgot, dwant, GRAD_TOL, 'dlogits, column view')


def test_plain_ce_logits_longer_than_ans_len():
    """logits [B, U + 3, V] with ans_len = U: ops.masked_ce_loss slices, the steps past U get no gradient."""
    (B, U, V), counts = CE_SHAPES[1]
    logits = rnd(B, U + 3, V, seed=870)
    y = ce_labels(B, U, V, counts, 871)
    want, dwant = ce_reference(logits, y, U)
    got, dgot = ce_device(logits, y.to(dev()), U)
    close(got, want, LOSS_TOL, 'loss, long logits')
    close(dgot, dwant, GRAD_TOL, 'dlogits, long logits')
    assert dgot.shape == (B, U + 3, V) and bool((dgot[:, U:] == 0).all())


@functools.lru_cache(maxsize=None)
def ce_shift_case():
    """Logits of scale 10 on a grid of 2^-10 (so that adding 80 is exact in float32 and both problems are the same
    problem in real arithmetic), three vocabulary passes with a tail, (B, U, V) = (16, 5, 130) with 5 or 4 labels
    a row.  Why B = 16: the saved log-sum-exp is ONE float per step (include/ssasr.h), so the probabilities of a
    step carry its rounding as a common relative error, up to ulp(lse) / 2 = 3.8e-6 for lse in [64, 128), and
    dlogits = (p - onehot) / (B * denom) an absolute error of up to 3.8e-6 / (B * denom).  GRAD_TOL = 1e-7 can be
    asked of logits this large only where B * denom >= 38; here B * denom >= 16 * 5 = 80."""
    B, U, V = 16, 5, 130
    base = torch.round(rnd(B, U, V, seed=880, scale=10.0) * 1024.0) / 1024.0
    shifted = base + 80.0
    assert torch.equal(shifted.float().double(), shifted) and torch.equal(base.float().double(), base)
    assert shifted.max().item() + np.log(V) < 128.0                       # the premise above: lse < 128
    y = ce_labels(B, U, V, [5 - b % 2 for b in range(B)], 881)
    return base, shifted, y, U


def test_plain_ce_shift_invariance():
    """Logits of scale 10 and the same plus 80.0: exp(z) of the shifted row overflows float32 unless the row's
    maximum is subtracted first.  Each loss against its own float64 reference, and the two device losses against
    each other, at LOSS_TOL."""
    base, shifted, y, U = ce_shift_case()
    yd = y.to(dev())
    losses = []
    for name, z in (('scale 10', base), ('scale 10 + 80', shifted)):
        want, dwant = ce_reference(z, y, U)
        got, dgot = ce_device(z, yd, U)
        close(got, want, LOSS_TOL, 'loss, %s' % name)
        close(dgot, dwant, GRAD_TOL, 'dlogits, %s' % name)
        check_ce_steps(dgot, y, U, name)
        losses.append(got)
    close(losses[1], losses[0], LOSS_TOL, 'shifted loss against unshifted')


# -------------------------------------------------------------------------------------------- 2. Adadelta ----
N_ADADELTA = 4096 * 256 + 4096 * 5 + 3
ADADELTA_SCALES = (0.001, 3.0)                 # gradient norm 1.0 (below max_norm = 5), then 3,100 (above)


@functools.lru_cache(maxsize=None)
def adadelta_case():
    """Parameters, the two gradients, and the float64 oracle's norm, param, square_avg and acc_delta after each
    step."""
    n = N_ADADELTA
    p = rnd(n, seed=901, scale=0.1)
    grads = [rnd(n, seed=902 + k, scale=s) for k, s in enumerate(ADADELTA_SCALES)]
    pr, sq, ad = [p.clone()], [torch.zeros(n, dtype=torch.float64)], [torch.zeros(n, dtype=torch.float64)]
    steps = []
    for g in grads:
        norm, ok = lo.clip_adadelta_explicit(pr, [g.clone()], sq, ad)
        assert ok
        steps.append((norm, pr[0].clone(), sq[0].clone(), ad[0].clone()))
    assert steps[0][0] < 5.0 < steps[1][0]
    return p, grads, steps


def run_adadelta(off):
    """Both steps on the device with grad, param and both states as buf[off:off + n] views; every step against the
    oracle.  Returns the two norms."""
    from ss_asr_amd import ops
    n = N_ADADELTA
    p, grads, steps = adadelta_case()
    view = lambda: torch.zeros(n + 8, device=dev())[off:off + n]           # noqa: E731
    pd, gd, sqd, add = view(), view(), view(), view()
    for t in (pd, gd, sqd, add):
        assert t.data_ptr() % 16 == 4 * off
    pd.copy_(p)
    ws, stats = ops.clip_adadelta_ws(n, dev()), torch.zeros(2, device=dev())
    norms = []
    for k, (g, (norm, pw, sqw, adw)) in enumerate(zip(grads, steps)):
        gd.copy_(g)
        ops.clip_adadelta_(pd, gd, sqd, add, ws, stats)
        s = stats.cpu()
        print('step %d norm %.9g (oracle %.9g)' % (k, float(s[0]), norm))
        assert s[1] == 0, 'step %d skipped' % k
        assert abs(float(s[0]) - norm) <= NORM_RTOL * max(1.0, norm), \
            'gradient norm, step %d, buffers %d bytes past alignment: %.9g, oracle %.9g' % (k, 4 * off, float(s[0]), norm)
        close(pd, pw, PARAM_TOL, 'param, step %d' % k)
        close(sqd, sqw, STATE_TOL, 'square_avg, step %d' % k)
        close(add, adw, STATE_TOL, 'acc_delta, step %d' % k)
        assert bits_equal(gd.cpu(), g.float())                             # zero_grad off: the gradient stays
        norms.append(float(s[0]))
    return norms


def test_adadelta_second_grid_stride_trip_aligned_and_unaligned():
    """n = 4096 * 256 + 4096 * 5 + 3: adadelta_kernel's second grid-stride trip (for 20,483 threads only) and a
    partial last sumsq block; a step below the clip norm, then one above.  Run with 16-byte aligned buffers (the
    float4 sumsq path for the 260 whole blocks) and again with every buffer 4 bytes past a 16-byte boundary (the
    scalar path throughout): both against the oracle, and the norms of the two runs within 1e-6 relative."""
    aligned = run_adadelta(0)
    unaligned = run_adadelta(1)
    for a, u in zip(aligned, unaligned):
        print('norm aligned %.9g unaligned %.9g' % (a, u))
        assert abs(a - u) <= 1e-6 * max(1.0, abs(a)), 'gradient norm: float4 path %.9g, scalar path %.9g' % (a, u)


def test_adadelta_zero_grad_on_a_good_and_on_a_skipped_step():
    """zero_grad = 1 at the same n: after a good step the gradient is all zero (second trip included) and the step
    is the oracle's; after a NaN step (the NaN in the partial last sumsq block) the gradient is all zero too,
    stats[1] == 1, and param and both states are bit for bit what the good step left."""
    from ss_asr_amd import ops
    n = N_ADADELTA
    p, grads, steps = adadelta_case()
    pd, gd = p.float().to(dev()), grads[0].float().to(dev())
    sqd, add = torch.zeros(n, device=dev()), torch.zeros(n, device=dev())
    ws, stats = ops.clip_adadelta_ws(n, dev()), torch.zeros(2, device=dev())
    ops.clip_adadelta_(pd, gd, sqd, add, ws, stats, zero_grad=True)
    assert stats[1].item() == 0, 'good step skipped'
    assert int(torch.count_nonzero(gd)) == 0, 'gradient not zeroed on a good step'
    _, pw, sqw, adw = steps[0]
    close(pd, pw, PARAM_TOL, 'param')
    close(sqd, sqw, STATE_TOL, 'square_avg')
    close(add, adw, STATE_TOL, 'acc_delta')
    before = [t.clone() for t in (pd, sqd, add)]
    gd.copy_(grads[1])
    gd[n - 2] = float('nan')
    ops.clip_adadelta_(pd, gd, sqd, add, ws, stats, zero_grad=True)
    assert stats[1].item() == 1, 'NaN step not flagged'
    assert int(torch.count_nonzero(gd)) == 0 and not bool(torch.isnan(gd).any()), 'gradient not zeroed on a skipped step'
    for name, a, b in zip(('param', 'square_avg', 'acc_delta'), (pd, sqd, add), before):
        assert bits_equal(a, b), name


# ------------------------------------------------------------------------------------------------ 3. Adam ----
N_CLIP, N_FREE = 4096 * 256 + 1237, 777
ADAM = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8)
MAX_NORM, GRAD_SCALE = 5.0, 0.25
# 0.25 * s * sqrt(N_CLIP) = 25.6, 12.8, 2.56: steps 1 and 2 are clipped at 5, step 3 is not
ADAM_SCALES = (0.1, 0.05, 0.01)
# gradients of +-1e-9 (|g| << eps = 1e-8: eps decides the update) and exact zeros; in the clipped range one block of
# each lies in the first grid-stride trip and one in the second (from 4096 * 256 on)
TINY_CLIP, ZERO_CLIP = [(1000, 1200), (N_CLIP - 600, N_CLIP - 400)], [(5000, 5300), (N_CLIP - 300, N_CLIP - 100)]
TINY_FREE, ZERO_FREE = [(100, 150)], [(200, 250)]


def adam_gradient(n, seed, scale, tiny, zero):
    g = rnd(n, seed=seed, scale=scale)
    for a, b in tiny:
        g[a:b] = torch.tensor(1e-9).float().double() * (1 - 2 * (torch.arange(b - a) % 2))
    for a, b in zero:
        g[a:b] = 0.0
    return g


@functools.lru_cache(maxsize=None)
def adam_case():
    """Parameters and the three gradients of both buffers; torch.optim.Adam on float64 under lo.solver_step (clip
    over the clipped parameter alone), fed grad_scale * g: its norm and (param, exp_avg, exp_avg_sq) of both
    buffers after each step."""
    pc, pf = rnd(N_CLIP, seed=931, scale=0.1), rnd(N_FREE, seed=932, scale=0.1)
    gcs = [adam_gradient(N_CLIP, 940 + k, s, TINY_CLIP, ZERO_CLIP) for k, s in enumerate(ADAM_SCALES)]
    gfs = [adam_gradient(N_FREE, 950 + k, 1.0, TINY_FREE, ZERO_FREE) for k in range(len(ADAM_SCALES))]
    rc, rf = pc.clone().requires_grad_(True), pf.clone().requires_grad_(True)
    opt = torch.optim.Adam([rc, rf], amsgrad=False, weight_decay=0, **ADAM)
    steps = []
    for gc, gf in zip(gcs, gfs):
        rc.grad, rf.grad = GRAD_SCALE * gc, GRAD_SCALE * gf
        norm, stepped = lo.solver_step([rc], opt, MAX_NORM)
        assert stepped
        steps.append((norm, [(r.detach().clone(), opt.state[r]['exp_avg'].clone(), opt.state[r]['exp_avg_sq'].clone())
                             for r in (rc, rf)]))
    assert steps[0][0] > MAX_NORM and steps[1][0] > MAX_NORM and steps[2][0] < MAX_NORM
    return pc, pf, gcs, gfs, steps


class AdamBuffers:
    """Device buffers laid out as FusedAdam's segments: the clipped range an unaligned run (4 bytes past a 16-byte
    boundary) of a larger flat tensor, data and gradient alike; the unclipped buffer a tensor of its own."""

    def __init__(self, pc, pf):
        self.pc = torch.zeros(N_CLIP + 8, device=dev())[1:1 + N_CLIP]
        self.gc = torch.zeros(N_CLIP + 8, device=dev())[1:1 + N_CLIP]
        assert self.pc.data_ptr() % 16 == 4 and self.gc.data_ptr() % 16 == 4
        self.pc.copy_(pc)
        self.pf = pf.float().to(dev())
        self.gf = torch.zeros(N_FREE, device=dev())

    def segments(self):
        return [(self.pc, self.gc, True), (self.pf, self.gf, False)]


class DirectAdam:
    """ops.adam_prepare + ops.adam_update_ per segment: FusedAdam.clip_and_step spelled out."""

    def __init__(self, buf):
        from ss_asr_amd import _lib
        self.buf = buf
        self.m = [torch.zeros_like(d) for d, _, _ in buf.segments()]
        self.v = [torch.zeros_like(d) for d, _, _ in buf.segments()]
        self.state = torch.zeros(1, device=dev())
        self.ws = torch.empty(int(_lib.load().ssasr_adam_ws(N_CLIP)), device=dev())
        self.stats = torch.zeros(2, device=dev())

    def step(self, zero_grad=False):
        from ss_asr_amd import ops
        ops.adam_prepare(self.buf.gc, self.state, self.ws, self.stats, grad_scale=GRAD_SCALE, max_norm=MAX_NORM,
                         lr=ADAM['lr'], betas=ADAM['betas'])
        for (d, g, c), m, v in zip(self.buf.segments(), self.m, self.v):
            ops.adam_update_(d, g, m, v, self.ws, self.stats, clipped=c, grad_scale=GRAD_SCALE, betas=ADAM['betas'],
                             eps=ADAM['eps'], zero_grad=zero_grad)

    def tensors(self):
        """(param, exp_avg, exp_avg_sq) of the clipped, then of the unclipped buffer."""
        return [(d, m, v) for (d, _, _), m, v in zip(self.buf.segments(), self.m, self.v)]


def check_adam_against(opt, want, what):
    for name, got3, want3 in zip(('clipped', 'unclipped'), opt.tensors(), want):
        close(got3[0], want3[0], PARAM_TOL, '%s param, %s' % (name, what))
        close(got3[1], want3[1], STATE_TOL, '%s exp_avg, %s' % (name, what))
        close(got3[2], want3[2], STATE_TOL, '%s exp_avg_sq, %s' % (name, what))


def test_adam_three_steps_against_float64():
    """ops.adam_prepare / ops.adam_update_ over both buffers for three steps at grad_scale = 0.25.  After every step:
    the step count in `state`, stats[0] against the reference's norm, stats[1] == 0, and (beyond what is asked,
    at the same bounds) param and both moments of both buffers; the unclipped buffer's moments are those of
    0.25 g, whatever the clip coefficient was."""
    pc, pf, gcs, gfs, steps = adam_case()
    buf = AdamBuffers(pc, pf)
    opt = DirectAdam(buf)
    for k, (gc, gf, (norm, want)) in enumerate(zip(gcs, gfs, steps)):
        buf.gc.copy_(gc)
        buf.gf.copy_(gf)
        opt.step()
        s = opt.stats.cpu()
        print('step %d norm %.9g (reference %.9g)' % (k + 1, float(s[0]), norm))
        assert opt.state.item() == k + 1, 'step count %g after step %d' % (opt.state.item(), k + 1)
        assert abs(float(s[0]) - norm) <= NORM_RTOL * max(1.0, norm), \
            'gradient norm, step %d: %.9g, reference %.9g' % (k + 1, float(s[0]), norm)
        assert s[1] == 0, 'step %d skipped' % (k + 1)
        check_adam_against(opt, want, 'step %d' % (k + 1))
    # and the reference did see 0.25 g there: after step 1 (clip coefficient 0.195) the unclipped buffer's first
    # moment is (1 - beta1) * 0.25 * g; under the clip coefficient it would be five times smaller
    m1 = steps[0][1][1][1]
    assert torch.allclose(m1, 0.1 * GRAD_SCALE * gfs[0], rtol=1e-12, atol=0)


def test_adam_skipped_step_does_not_count():
    """A NaN in the clipped gradient at step 1 (zero_grad on): params and moments of BOTH buffers stay bit for bit,
    `state` stays 0, stats[1] is 1 and both gradient buffers are zeroed.  The good step after it is then the
    first step of a fresh optimizer, bit for bit, and the float64 reference's first step: the bias corrections
    are those of t = 1."""
    pc, pf, gcs, gfs, steps = adam_case()
    buf = AdamBuffers(pc, pf)
    opt = DirectAdam(buf)
    before = [[t.clone() for t in three] for three in opt.tensors()]
    buf.gc.copy_(gcs[1])
    buf.gc[N_CLIP - 5] = float('nan')
    buf.gf.copy_(gfs[1])
    opt.step(zero_grad=True)
    assert opt.stats[1].item() == 1, 'NaN step not flagged'
    assert opt.state.item() == 0, 'the skipped step was counted: state = %g' % opt.state.item()
    for name, g in (('clipped', buf.gc), ('unclipped', buf.gf)):
        assert int(torch.count_nonzero(g)) == 0 and not bool(torch.isnan(g).any()), \
            '%s gradient not zeroed on the skipped step' % name
    for got3, want3 in zip(opt.tensors(), before):
        for name, got, want in zip(('param', 'exp_avg', 'exp_avg_sq'), got3, want3):
            assert bits_equal(got, want), '%s changed on the skipped step' % name
    buf.gc.copy_(gcs[0])
    buf.gf.copy_(gfs[0])
    opt.step()
    assert opt.stats[1].item() == 0, 'good step skipped'
    assert opt.state.item() == 1, 'step count after one good step: %g' % opt.state.item()
    check_adam_against(opt, steps[0][1], 'first good step')
    fresh_buf = AdamBuffers(pc, pf)
    fresh = DirectAdam(fresh_buf)
    fresh_buf.gc.copy_(gcs[0])
    fresh_buf.gf.copy_(gfs[0])
    fresh.step()
    for got3, want3 in zip(opt.tensors(), fresh.tensors()):
        for name, got, want in zip(('param', 'exp_avg', 'exp_avg_sq'), got3, want3):
            assert bits_equal(got, want), '%s differs from a fresh optimizer\'s first step' % name


def test_fused_adam_is_the_direct_calls():
    """One optim.FusedAdam.clip_and_step over the same two segments: bit for bit the direct ops calls."""
    from ss_asr_amd import optim
    pc, pf, gcs, gfs, steps = adam_case()
    a, b = AdamBuffers(pc, pf), AdamBuffers(pc, pf)
    for buf in (a, b):
        buf.gc.copy_(gcs[0])
        buf.gf.copy_(gfs[0])
    direct = DirectAdam(a)
    direct.step()
    fused = optim.FusedAdam(b.segments(), **ADAM)
    fused.clip_and_step(max_norm=MAX_NORM, grad_scale=GRAD_SCALE)
    norm, skipped = fused.poll(wait=True)
    assert not skipped and norm == direct.stats[0].item() and fused.state_step.item() == 1
    for (d, m, v), (fd, _, _), fm, fv in zip(direct.tensors(), b.segments(), fused.exp_avg, fused.exp_avg_sq):
        assert bits_equal(d, fd) and bits_equal(m, fm) and bits_equal(v, fv)
    check_adam_against(direct, steps[0][1], 'step 1')


# --------------------------------------------------------------------------------------- 4. frame lengths ----
def frames_case(B, T, F, seed):
    """Small integers as floats (every row sum is exact in any order).  Utterance b is a prefix of ragged length
    with every frame's sum non-zero; then, where the shape has room: the last utterance all zero, an all-zero
    frame inside utterance 0, and a frame [+3, -3, 0, ...] inside utterance 0."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-4, 5, (B, T, F), generator=g).double()
    x[..., 0] += (x.sum(-1) == 0).double()                   # no accidental zero-sum frame
    for b in range(B):
        x[b, max(1, T - 2 * b):] = 0
    if B > 1:
        x[B - 1] = 0
    if T >= 3:
        x[0, 1] = 0
    if T >= 5 and F >= 2:
        x[0, 3] = 0
        x[0, 3, 0], x[0, 3, 1] = 3.0, -3.0
    return x


@pytest.mark.parametrize('B,T,F', [(1, 1, 1), (3, 7, 5), (2, 9, 130), (5, 50, 80)])
def test_frame_lengths_count_non_zero_sum_frames(B, T, F):
    """frame_len_kernel against lo.frame_lengths, exactly: the count of frames whose sum is non-zero, not a prefix
    length -- an all-zero frame and a frame that is [+3, -3, 0, ...] inside an utterance do not count, an all-zero
    utterance has length 0."""
    from ss_asr_amd import ops
    x = frames_case(B, T, F, 1000 + T)
    want = lo.frame_lengths(x)
    if B > 1:
        assert want[-1] == 0
    if T >= 5 and F >= 2:
        assert want[0] == T - 2 and x[0, 3].abs().sum() == 6 and x[0, T - 1].sum() != 0
    assert ops.frame_lengths(x.float().to(dev())).cpu().tolist() == want


# ------------------------------------------------------------------------------------------ 5. batch gather ----
ROWS, GATHER_B, GATHER_T = 3000, 3, 6
GATHER_OFFSETS = [ROWS - 6, ROWS - 7, ROWS - 6]          # the end of the corpus, out of order, overlapping


def corpus(F, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(ROWS, F, generator=g, dtype=torch.float32)


def gather_reference(frames, lens):
    want = np.zeros((GATHER_B, GATHER_T, frames.shape[1]), dtype=np.float32)
    for b, (o, l) in enumerate(zip(GATHER_OFFSETS, lens)):
        want[b, :l] = frames[o:o + l]
    return want


def gather_direct(frames_ptr, F, lens):
    """ssasr_gather_batch through the C ABI into a NaN-filled buffer."""
    from ss_asr_amd import _lib
    out = torch.full((GATHER_B, GATHER_T, F), float('nan'), device=dev())
    offs = torch.tensor(GATHER_OFFSETS, dtype=torch.int64, device=dev())
    ld = torch.tensor(lens, dtype=torch.int32, device=dev())
    _lib.check(_lib.load().ssasr_gather_batch(C.c_void_p(frames_ptr), _p(offs), _p(ld), GATHER_B, GATHER_T, F, _p(out),
                                              _stream()), 'ssasr_gather_batch')
    return out.cpu().numpy()


@pytest.mark.parametrize('lens', [[6, 2, 0], [5, 2, 0]], ids=['T_is_max_len', 'T_above_max_len'])
@pytest.mark.parametrize('F', [1, 3, 4, 80, 130])
def test_gather_batch_scalar_and_float4_paths(F, lens):
    """gather_batch_kernel against a numpy gather, exactly, every element (the output starts as NaN): F = 1, 3, 130
    take the scalar path (130: a second lane trip), F = 4 and 80 the float4 path.  A row of pure padding, padding
    after a short row, offsets at the end of a 3000-row corpus (offsets[b] * F is not small)."""
    from ss_asr_amd import ops
    frames = corpus(F, 1100 + F)
    want = gather_reference(frames.numpy(), lens)
    fd = frames.to(dev())
    assert fd.data_ptr() % 16 == 0
    got = gather_direct(fd.data_ptr(), F, lens)
    assert np.array_equal(got, want)
    got = ops.gather_batch(fd, torch.tensor(GATHER_OFFSETS, dtype=torch.int64, device=dev()),
                           torch.tensor(lens, dtype=torch.int32, device=dev()), GATHER_T)
    assert np.array_equal(got.cpu().numpy(), want)


def test_gather_batch_misaligned_frames_take_the_scalar_path():
    """F = 4 with `frames` 4 bytes past a 16-byte boundary: a float4 load there would be misaligned, the kernel's
    alignment test sends it down the scalar path, and the result is still exact."""
    frames = corpus(4, 1199)
    flat = torch.zeros(ROWS * 4 + 8, device=dev())
    flat[1:1 + ROWS * 4].copy_(frames.reshape(-1))
    ptr = flat.data_ptr() + 4
    assert ptr % 16 == 4
    got = gather_direct(ptr, 4, [6, 2, 0])
    assert np.array_equal(got, gather_reference(frames.numpy(), [6, 2, 0]))
