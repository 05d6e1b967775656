"""Label smoothing in the masked CE (ssasr_ce_loss_ls_fwd / _bwd) on the GPU: loss and dlogits against float64
torch.nn.functional.cross_entropy(label_smoothing=eps) with the masking and normalisation of src/trainer.py:426-434
restated on the CPU, at the tolerance tests/test_gpu_kernels.py applies to the unsmoothed kernels (1e-6 on the
loss, 1e-7 on dlogits, relative above 1); eps = 0 is today's kernels bit for bit; the gradient sums to zero over
the classes; the fused train steps take the argument.

The logits are unit-scale normal draws, as in the test the tolerances are taken from: those tolerances are
absolute, and what float32 can hold scales with the logits.  The saved log-sum-exp is one float, so every
probability of a step carries its rounding as a common relative error, and the sum over V of dlogits is off by
that much over B * denom[b] before anything else rounds; at (1, 1, 5), B * denom = 1, nothing scales it down.
The smoothed kernels therefore form the log-sum-exp and the gradient in double and round once (the correctly
rounded lse of that case is off by 4.1e-8), which is what holds the sums inside 1e-7."""
import ctypes
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

LOSS_TOL, GRAD_TOL = 1e-6, 1e-7              # test_masked_ce_loss_forward_backward's


def dev():
    return torch.device('cuda:0')


def close(got, want, atol, what=''):
    got = got.detach().double().cpu()
    want = want.detach().double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = (got - want).abs().max().item()
    tol = atol * max(1.0, want.abs().max().item())     # absolute for O(1) data, relative above
    print('%s: max abs err %.3e (tolerance %.1e)' % (what, err, tol))
    assert err <= tol, '%s: max abs err %.3e > %.1e' % (what, err, tol)


def smoothed_loss(logits, y, ans_len, eps):
    """float64: mean_b( sum_t CE_eps(logits[b, t], y[b, t + 1]) [y[b, t + 1] != 0] / count(y[b] != 0) )."""
    logits = logits.double()
    B, U, V = logits.shape
    label = y[:, 1:ans_len + 1].contiguous()
    tok = F.cross_entropy(logits.reshape(B * U, V), label.reshape(-1), ignore_index=0, reduction='none',
                          label_smoothing=eps).view(B, U)
    return (tok.sum(-1) / (y != 0).sum(-1).double()).mean()


# (B, U, V) and the label count of every row (rows with fewer labels than U; none without labels)
SHAPES = [((1, 1, 5), [1]), ((3, 9, 31), [9, 5, 1]), ((2, 70, 64), [70, 33]), ((2, 5, 130), [5, 2])]
_cases = {}


def case(k):
    if k not in _cases:
        (B, U, V), counts = SHAPES[k]
        g = torch.Generator().manual_seed(700 + k)
        logits = torch.randn(B, U, V, generator=g, dtype=torch.float64)       # unit scale: see the module docstring
        y = torch.zeros(B, U + 2, dtype=torch.long)
        for b, n in enumerate(counts):
            y[b, 1:1 + n] = torch.randint(1, V, (n,), generator=g)
        _cases[k] = (logits, y, U)
    return _cases[k]


@pytest.mark.parametrize('eps', [0.1, 0.5])
@pytest.mark.parametrize('k', range(len(SHAPES)))
def test_smoothed_loss_and_gradient_against_float64(k, eps):
    from ss_asr_amd import ops
    logits, y, U = case(k)
    lr = logits.clone().requires_grad_(True)
    want = smoothed_loss(lr, y, U, eps)
    want.backward()
    ld = logits.float().to(dev()).requires_grad_(True)
    got = ops.masked_ce_loss(ld, y.to(dev()), U, label_smoothing=eps)
    close(got, want, LOSS_TOL, 'loss %s eps %g' % (SHAPES[k][0], eps))
    got.backward()
    close(ld.grad, lr.grad, GRAD_TOL, 'dlogits %s eps %g' % (SHAPES[k][0], eps))
    assert float(want.detach()) != float(smoothed_loss(logits, y, U, 0.0))


@pytest.mark.parametrize('eps', [0.1, 0.5])
@pytest.mark.parametrize('k', range(len(SHAPES)))
def test_gradient_sums_to_zero_over_the_classes(k, eps):
    """The smoothed target sums to one, so dlogits sums to zero over V on a labelled step, within the dlogits
    tolerance; an unlabelled step has no gradient at all.

    With the log-sum-exp and the gradient formed in float, as the plain kernels form them, (1, 1, 5) measured
    1.75e-7 (eps 0.1) and 1.34e-7 (eps 0.5) on an MI355X; the figures of the double form are in DESIGN.md 4.5."""
    from ss_asr_amd import ops
    logits, y, U = case(k)
    ld = logits.float().to(dev()).requires_grad_(True)
    ops.masked_ce_loss(ld, y.to(dev()), U, label_smoothing=eps).backward()
    labelled = (y[:, 1:U + 1] != 0)
    assert bool((ld.grad.cpu()[~labelled] == 0).all())
    sums = ld.grad.double().sum(-1).cpu()
    close(sums[labelled], torch.zeros_like(sums[labelled]), GRAD_TOL, 'sum over V of dlogits %s eps %g' % (SHAPES[k][0], eps))


def _raw(logits, y32, eps, entries):
    """loss, dlogits and the saved block through the C entries themselves; eps None: the unsmoothed entries."""
    from ss_asr_amd import _lib
    lib = _lib.load()
    B, U, V = logits.shape
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lse = torch.zeros(B * U + 9 * B, device=dev())
    loss = torch.zeros((), device=dev())
    dl = torch.zeros_like(logits)
    one = torch.ones((), device=dev())
    if entries == 'plain':
        assert lib.ssasr_ce_loss_fwd(p(logits), p(y32), y32.stride(0), y32.shape[1], B, U, V, p(lse), p(loss), st) == 0
        assert lib.ssasr_ce_loss_bwd(p(logits), p(y32), y32.stride(0), p(lse), p(one), B, U, V, p(dl), st) == 0
    else:
        assert lib.ssasr_ce_loss_ls_fwd(p(logits), p(y32), y32.stride(0), y32.shape[1], B, U, V, eps, p(lse), p(loss),
                                        st) == 0
        assert lib.ssasr_ce_loss_ls_bwd(p(logits), p(y32), y32.stride(0), p(lse), p(one), B, U, V, eps, p(dl), st) == 0
    torch.cuda.synchronize()
    return loss, dl, lse


@pytest.mark.parametrize('k', range(len(SHAPES)))
def test_eps_zero_is_the_existing_kernels_bit_for_bit(k):
    from ss_asr_amd import ops
    logits, y, U = case(k)
    ld, yd = logits.float().to(dev()), y.to(dev())
    y32 = yd.to(torch.int32)
    loss0, dl0, lse0 = _raw(ld, y32, None, 'plain')
    loss1, dl1, lse1 = _raw(ld, y32, 0.0, 'ls')
    bits = lambda t: t.view(torch.int32)
    assert torch.equal(bits(loss0), bits(loss1)) and torch.equal(bits(dl0), bits(dl1)) and torch.equal(bits(lse0), bits(lse1))
    a = ld.clone().requires_grad_(True)
    b = ld.clone().requires_grad_(True)
    la, lb = ops.masked_ce_loss(a, yd, U), ops.masked_ce_loss(b, yd, U, label_smoothing=0.0)
    la.backward()
    lb.backward()
    assert torch.equal(bits(la.detach()), bits(lb.detach())) and torch.equal(bits(la.detach()), bits(loss0))
    assert torch.equal(bits(a.grad), bits(b.grad)) and torch.equal(bits(a.grad), bits(dl0))
    # and the smoothed entries at eps > 0 save the same block: the log-sum-exp of every step (correctly rounded
    # there, so within an ulp or two of the plain kernel's) and the same denominators
    _, _, lse2 = _raw(ld, y32, 0.1, 'ls')
    B, U_, V = ld.shape
    close(lse2[:B * U_], lse0[:B * U_], LOSS_TOL, 'saved log-sum-exp')
    assert torch.equal(lse2[B * U_ + 8 * B:], lse0[B * U_ + 8 * B:])


def _two_steps(step_cls, model_fn, eps):
    from ss_asr_amd.engine import label_geometry
    from ss_asr_amd.synthetic import make_batch
    x, y, lens = make_batch(np.array([96, 80, 64, 40]), np.array([6, 5, 4, 3]), 80, seed=3)
    _, ans_len = label_geometry(y)
    torch.manual_seed(0)
    model = model_fn().to(dev())
    step = step_cls(model, label_smoothing=eps)
    random.seed(0)
    losses = []
    for _ in range(2):
        loss = step(x.to(dev()), y.to(dev()), lens, ans_len)
        norm, skipped = step.finish()
        assert not skipped and np.isfinite(norm)
        losses.append((float(loss), step.last_logits.detach().clone()))
    return losses, y, ans_len, step


def test_fused_train_steps_take_the_smoothing():
    from ss_asr_amd.asr import ASR
    from ss_asr_amd.ctc import JointCTCASR, JointCTCTrainStep
    from ss_asr_amd.engine import ASRTrainStep
    make = lambda: ASR(50, 64, 64, 32, 80, 1.0)
    smooth, y, ans_len, step = _two_steps(ASRTrainStep, make, 0.1)
    plain, _, _, _ = _two_steps(ASRTrainStep, make, 0.0)
    assert step.label_smoothing == pytest.approx(0.1)
    for (ls, logits), (lp, plogits) in zip(smooth, plain):
        assert np.isfinite(ls) and ls != lp
        close(torch.tensor(ls), smoothed_loss(logits.cpu(), y, ans_len, 0.1), LOSS_TOL, 'step loss')
        close(torch.tensor(lp), smoothed_loss(plogits.cpu(), y, ans_len, 0.0), LOSS_TOL, 'plain step loss')
    close(smooth[0][1], plain[0][1], 1e-5, 'first forward')                  # same seed: the first forward is shared
    # the joint step smooths its attention branch only
    joint, y, ans_len, jstep = _two_steps(JointCTCTrainStep, lambda: JointCTCASR(50, 64, 64, 32, 80, 1.0, ctc_weight=0.3),
                                          0.1)
    assert jstep.label_smoothing == pytest.approx(0.1) and all(np.isfinite(l) for l, _ in joint)
    close(jstep.last_att_loss, smoothed_loss(joint[1][1].cpu(), y, ans_len, 0.1), LOSS_TOL, 'joint attention loss')
    with pytest.raises(ValueError, match='label_smoothing'):
        ASRTrainStep(make().to(dev()), label_smoothing=1.0)
