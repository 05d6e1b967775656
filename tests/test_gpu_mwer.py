"""MWER training on the GPU: the loss kernels (ops.mwer_loss) against postprocess.mwer_reference in float64 with
autograd for the gradient, ssasr_mwer_pack against a Python loop, ssasr_rows_repeat against torch, and
engine.MWERTrainStep against OracleASR in float64 driven the same way (encode the batch once, repeat the features,
teacher-force every row, mwer_reference).  Shapes are the smallest at which each mechanism can fail: one hypothesis,
partial and empty sets, the widest group (33 rows), more steps than one pass of a block's waves (U = 70 > 32),
V over one, two and three lanes' passes."""
import os
import random
import types

import numpy as np
import pytest
import torch

import las_oracle as lo
from test_host_cpu import make_corpus

from ss_asr_amd.postprocess import edit_counts, mwer_reference
from ss_asr_amd.preprocess import ALL_CHARS, TOKENS

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
# the CE loss tests' own bounds and rule (tests/test_gpu_kernels.py, test_masked_ce_loss_forward_backward)
LOSS_TOL, GRAD_TOL = 1e-6, 1e-7
# the per-tensor bound that tests/test_gpu_trainer.py holds parameter gradients to against the float64 oracle
# (test_sae_gradients_match_the_oracle_tensor_by_tensor): norm of the difference relative to the tensor's norm
PARAM_GRAD_TOL = 2e-5
SPACE, EOS = (TOKENS + ALL_CHARS).index(' '), 1


def close(got, want, atol, what=''):
    got = got.detach().double().cpu()
    want = want.detach().double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = (got - want).abs().max().item()
    tol = atol * max(1.0, want.abs().max().item())     # absolute for O(1) data, relative above
    print('%s: max abs err %.3e (bound %.1e)' % (what, err, tol))
    assert err <= tol, '%s: max abs err %.3e > %.1e' % (what, err, tol)


def make_case(G, M, U, V, seed, extra_cols=1):
    """(logits float32, rows int32 [R, U + 1 + extra_cols], counts int32 [R, 8]) on the CPU: some rows with interior
    zeros, some shorter than U; the slack columns hold a label that the loss must not read."""
    gen = torch.Generator().manual_seed(seed)
    R = G * M
    logits = 2.0 * torch.randn(R, U, V, generator=gen)
    rows = torch.randint(1, V, (R, U + 1 + extra_cols), generator=gen, dtype=torch.int32)
    rows[:, 0] = 0
    for r in range(R):
        if r % 3 == 1 and U > 2:
            rows[r, 1 + int(torch.randint(0, U, (1,), generator=gen))] = 0
        if r % 4 == 2:
            rows[r, 1 + int(torch.randint(0, U, (1,), generator=gen)):U + 1] = 0
    counts = torch.randint(0, 10, (R, 8), generator=gen, dtype=torch.int32)
    return logits, rows, counts


SHAPES = [((1, 1, 1, 5), [1]), ((3, 4, 9, 31), [4, 2, 0]), ((2, 33, 70, 64), None), ((2, 3, 5, 130), None)]


@pytest.mark.parametrize('with_ce', [False, True])
@pytest.mark.parametrize('unit', [0, 1])
@pytest.mark.parametrize('shape,n_hyps', SHAPES)
def test_loss_and_gradient_against_the_float64_reference(shape, n_hyps, unit, with_ce):
    from ss_asr_amd import ops
    G, M, U, V = shape
    R = G * M
    logits, rows, counts = make_case(G, M, U, V, seed=sum(shape) + unit)
    n_hyps = torch.tensor(n_hyps if n_hyps is not None else [M] * G, dtype=torch.int32)
    ce_w = (0.2 * torch.rand(R, generator=torch.Generator().manual_seed(5))) if with_ce else None
    ref_logits = logits.double().requires_grad_()
    want, want_risk, want_p = mwer_reference(ref_logits, rows, n_hyps, counts, unit, ce_w)
    (want_grad,) = torch.autograd.grad(want, ref_logits)

    got_logits = logits.to(DEV).requires_grad_()
    got, info = ops.mwer_loss(got_logits, rows.to(DEV), n_hyps.to(DEV), counts.to(DEV), unit,
                              None if ce_w is None else ce_w.to(DEV))
    got.backward()
    torch.cuda.synchronize()
    close(got, want, LOSS_TOL, 'loss')
    close(info.risk, want_risk, LOSS_TOL, 'risk')
    close(info.p_hat, want_p, GRAD_TOL, 'p_hat')
    close(got_logits.grad, want_grad, GRAD_TOL, 'dlogits')

    # properties of what the kernel wrote, by themselves
    grad = got_logits.grad.double().cpu()
    risk = counts.double()[:, 4 * unit:4 * unit + 3].sum(1)
    bound = GRAD_TOL * max(1.0, float(risk.max()))
    n = n_hyps.clamp(0, M)
    inside = (torch.arange(M).unsqueeze(0) < n.long().unsqueeze(1)).reshape(R)
    seq_w = info.weight.cpu() - (ce_w.double() if with_ce else 0.0)      # the MWER part of each row's weight
    assert float((seq_w * inside).view(G, M).sum(1).abs().max()) <= bound
    assert float(seq_w[~inside].abs().max() if (~inside).any() else 0.0) == 0.0
    lab = rows[:, 1:U + 1].long()
    labelled = lab != 0
    assert float(grad.sum(-1)[labelled].abs().max() if labelled.any() else 0.0) <= bound
    assert float(grad[~labelled].abs().max() if (~labelled).any() else 0.0) == 0.0
    if not with_ce and (~inside).any():
        assert float(grad[~inside].abs().max()) == 0.0
    if shape == (1, 1, 1, 5):
        # a single hypothesis: the loss is its risk (plus the CE term) and the MWER gradient is 0
        assert float(info.p_hat[0]) == 1.0 and float(seq_w.abs().max()) == 0.0
        if not with_ce:
            assert float(got.detach()) == float(risk[0]) and float(grad.abs().max()) == 0.0
    # the float lse kept for logging is the correctly rounded double one
    lse = torch.logsumexp(logits.double(), -1)
    assert torch.equal(info.lse.cpu(), lse.float()) or float((info.lse.cpu().double() - lse).abs().max()) < 5e-7


def test_logp_values_far_apart_clamped_sets_and_equal_risks():
    from ss_asr_amd import ops
    # two one-step rows whose log-probabilities are 1e3 apart: a finite loss, a one-hot posterior
    logits = torch.zeros(2, 1, 4)
    logits[1, 0, 1] = -1000.0
    rows = torch.tensor([[0, 1], [0, 1]], dtype=torch.int32)
    counts = torch.tensor([[0] * 4 + [3, 0, 0, 3], [0] * 4 + [0, 1, 0, 3]], dtype=torch.int32)
    loss, info = ops.mwer_loss(logits.to(DEV).requires_grad_(), rows.to(DEV), torch.tensor([2], dtype=torch.int32).to(DEV),
                               counts.to(DEV), 'word')
    loss = float(loss.detach())
    assert np.isfinite(loss) and info.p_hat.cpu().tolist() == [1.0, 0.0] and loss == 3.0
    # n_hyps above M and below 0 clamp
    logits, rows, counts = make_case(3, 4, 6, 11, seed=2)
    outs = []
    for n_hyps in ([9, -3, 2], [4, 0, 2]):
        loss, info = ops.mwer_loss(logits.to(DEV), rows.to(DEV), torch.tensor(n_hyps, dtype=torch.int32).to(DEV),
                                   counts.to(DEV), 0)
        outs.append((float(loss), info.p_hat.cpu(), info.risk.cpu()))
    assert outs[0][0] == outs[1][0] and torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][2], outs[1][2])
    assert float(outs[0][2][1]) == 0.0 and float(outs[0][1][4:8].abs().max()) == 0.0
    # equal risks: the MWER part of every row's gradient is 0 within the bound, and two runs give the same bits
    counts[:] = torch.tensor([2, 1, 0, 5, 1, 1, 1, 4], dtype=torch.int32)
    grads = []
    for _ in range(2):
        z = logits.to(DEV).requires_grad_()
        loss, info = ops.mwer_loss(z, rows.to(DEV), torch.tensor([4, 4, 4], dtype=torch.int32).to(DEV), counts.to(DEV), 1)
        loss.backward()
        grads.append((float(loss), z.grad.cpu()))
    assert float(grads[0][1].abs().max()) <= GRAD_TOL * 3.0 and abs(grads[0][0] - 3.0) <= LOSS_TOL * 3.0
    assert grads[0][0] == grads[1][0] and torch.equal(grads[0][1], grads[1][1])


def pack_loop(chars, n_chars, n_hyps, y_ref, eos, L):
    N, K, steps = chars.shape
    rows = np.zeros((N * (K + 1), L), dtype=np.int32)
    lens = np.zeros(N * (K + 1), dtype=np.int32)
    for n in range(N):
        for k in range(min(max(int(n_hyps[n]), 0), K)):
            ln = min(max(int(n_chars[n, k]), 0), steps)
            r = n * (K + 1) + k
            rows[r, 1:1 + ln] = chars[n, k, :ln]
            rows[r, 1 + ln] = eos
            lens[r] = ln
        r = n * (K + 1) + K
        rows[r, :y_ref.shape[1]] = y_ref[n]
        lens[r] = max(int((y_ref[n] != 0).sum()) - 1, 0)
    return rows, lens


@pytest.mark.parametrize('N,K,steps,ref_cols,L', [(5, 3, 6, 7, None), (2, 1, 4, 3, None), (3, 32, 9, 14, 20), (70, 2, 65, 70, None)])
def test_pack_equals_a_python_loop(N, K, steps, ref_cols, L):
    from ss_asr_amd import ops
    rng = np.random.default_rng(N + K)
    chars = rng.integers(2, 50, size=(N, K, steps)).astype(np.int32)
    n_chars = rng.integers(0, steps + 1, size=(N, K)).astype(np.int32)
    n_hyps = rng.integers(1, K + 1, size=N).astype(np.int32)
    n_hyps[0] = 0                          # no hypothesis at all
    n_chars[1 % N, 0] = steps              # the search left no room: eos is still appended
    n_chars[-1, 0] = -2                    # a negative count is an empty hypothesis
    n_chars[-1, K - 1] = steps + 5         # a count past the steps is clamped
    n_hyps[-1] = K + 4                     # as is a hypothesis count past K
    padded = np.zeros((N, ref_cols + 2), dtype=np.int32)      # a label matrix with slack that must not be read
    padded[:, ref_cols:] = 9
    for n in range(N):
        ln = int(rng.integers(0, ref_cols - 1))
        padded[n, 1:1 + ln] = rng.integers(2, 50, size=ln)
        padded[n, 1 + ln] = EOS
    y_ref = torch.from_numpy(padded).to(DEV)[:, :ref_cols]
    rows, lens = ops.mwer_pack(torch.from_numpy(chars).to(DEV), torch.from_numpy(n_chars).to(DEV),
                               torch.from_numpy(n_hyps).to(DEV), y_ref, EOS, L)
    want_rows, want_lens = pack_loop(chars, n_chars, n_hyps, padded[:, :ref_cols], EOS, L or max(steps + 2, ref_cols))
    assert rows.dtype == torch.int32 and np.array_equal(rows.cpu().numpy(), want_rows)
    assert np.array_equal(lens.cpu().numpy(), want_lens)
    # the packed rows are scored in place: column 1 onwards, every row against its utterance's reference row
    M = K + 1
    ref_of = ((torch.arange(N * M, dtype=torch.int32) // M) * M + K).to(DEV)
    counts = ops.edit_score(rows[:, 1:], lens, rows[:, 1:max(ref_cols, 2)], lens, ref_of, space=SPACE).cpu().tolist()
    for r in (0, K, N * M - 1, N * M - M):
        ref = want_rows[(r // M) * M + K]
        assert counts[r] == edit_counts(want_rows[r], ref, SPACE), r


@pytest.mark.parametrize('G,M,shape', [(3, 4, (5, 8)), (2, 33, (7,)), (5, 2, (1030,)), (1, 1, (3,)), (4, 3, ())])
def test_rows_repeat_forward_bits_and_backward_order(G, M, shape):
    from ss_asr_amd import ops
    gen = torch.Generator().manual_seed(G * M)
    t = torch.randn((G,) + shape, generator=gen)
    src = t.to(DEV).requires_grad_()
    out = ops.rows_repeat(src, M)
    assert torch.equal(out.detach().cpu(), t.repeat_interleave(M, 0))
    ddst = torch.randn((G * M,) + shape, generator=gen) * torch.logspace(-3, 3, G * M).view((G * M,) + (1,) * len(shape))
    grads = []
    for _ in range(2):
        (g,) = torch.autograd.grad(ops.rows_repeat(src, M), src, ddst.to(DEV))
        grads.append(g.cpu())
    assert torch.equal(grads[0], grads[1])
    want = ddst.double().view((G, M) + shape).sum(1)
    bound = (M - 1) * 2.0 ** -24 * ddst.double().abs().view((G, M) + shape).sum(1)
    assert bool(((grads[0].double() - want).abs() <= bound).all())
    # the order k = 0 .. M - 1, in float: the same bits as a float loop
    loop = ddst.view((G, M) + shape)[:, 0].clone()
    for k in range(1, M):
        loop += ddst.view((G, M) + shape)[:, k]
    assert torch.equal(grads[0], loop)
    ints = torch.randint(-5, 500, (G,) + shape, generator=gen, dtype=torch.int32)
    assert torch.equal(ops.rows_repeat(ints.to(DEV), M).cpu(), ints.repeat_interleave(M, 0))


# ------------------------------------------------------------------------------------------------ the step ----
TINY = (50, 64, 64, 32, 80)            # V, encoder, decoder, mlp, features (the sizes of smoke())
FULL = (50, 256, 256, 128, 80)          # the real widths: E = 512, D = 256, A = 128 (the persistent decode-loop forms)
_cases = {}


def step_case(name):
    """A seeded model pair (GPU float32 / oracle float64), a batch and fixed hypotheses, with the oracle's loss and
    gradients for them, computed once and shared."""
    if name in _cases:
        return _cases[name]
    from ss_asr_amd.asr import ASR
    from ss_asr_amd.synthetic import make_batch
    dims = TINY if name == 'tiny' else FULL
    B, K = 4, 3
    frames = np.array([64, 57, 49, 40])
    n_lab = np.array([9, 7, 6, 4])
    x, y, lens = make_batch(frames, n_lab, dims[4], seed=7)
    rng = np.random.default_rng(11)
    steps = 10                                                     # U <= 12: the longest row has 10 + 1 labels
    chars = rng.integers(3, dims[0], size=(B, K, steps)).astype(np.int32)
    n_chars = rng.integers(1, steps + 1, size=(B, K)).astype(np.int32)
    n_hyps = np.array([3, 3, 2, 1], dtype=np.int32)
    for b in range(B):                                             # near-misses of the reference: small, unequal risks
        ref = y[b, 1:1 + n_lab[b]].numpy()
        chars[b, 0, :n_lab[b]] = ref
        n_chars[b, 0] = n_lab[b]
        chars[b, 1, :n_lab[b]] = ref
        chars[b, 1, 1] = SPACE
        n_chars[b, 1] = n_lab[b] - 1
    chars[:, :, 2] = np.where(chars[:, :, 2] == SPACE, 5, chars[:, :, 2])
    model = ASR(*dims, 0.3)                                        # tf_rate < 1: the step must ignore it
    lo.seeded_weights(model, 5)
    ref = lo.OracleASR(*dims, 1.0)
    lo.seeded_weights(ref, 5)
    ref = ref.double()
    case = dict(dims=dims, B=B, K=K, x=x, y=y, lens=lens, model=model.to(DEV), ref=ref,
                hyps=(torch.from_numpy(chars), torch.from_numpy(n_chars), torch.from_numpy(n_hyps)))
    _cases[name] = case
    return case


def oracle_forward(case, hyps, ce_weight, unit):
    """OracleASR in float64 driven as the step is: -> (loss, risk, rows, counts, logits) with the graph."""
    chars, n_chars, n_hyps = [t.numpy() for t in hyps]
    B, K = chars.shape[0], chars.shape[1]
    M = K + 1
    y = case['y']
    rows, lens = pack_loop(chars, n_chars, n_hyps, y.numpy().astype(np.int32), EOS, max(chars.shape[2] + 2, y.shape[1]))
    counts = np.array([edit_counts(rows[r, 1:1 + lens[r]], rows[(r // M) * M + K, 1:1 + lens[(r // M) * M + K]], SPACE)
                       for r in range(B * M)], dtype=np.int32)
    ref = case['ref']
    feat, enc_len = ref.encoder(case['x'].double(), case['lens'])                     # the batch, encoded ONCE
    U = int(lens.max()) + 1
    rows_t = torch.from_numpy(rows)
    logits, _, _, _ = lo.decoder_replay(ref, feat.repeat_interleave(M, 0), np.repeat(np.array(enc_len), M),
                                        rows_t.long(), [0] * U)
    ce_w = torch.zeros(B, M, dtype=torch.float64)
    ce_w[:, K] = ce_weight / (B * (y != 0).sum(1).double())
    loss, risk, _ = mwer_reference(logits, rows_t, torch.from_numpy(n_hyps), torch.from_numpy(counts), unit,
                                   ce_w.view(-1))
    return loss, risk, rows, counts, logits


def compare_parameter_gradients(got, want, what):
    """got / want: {name: gradient}.  Every tensor is held to PARAM_GRAD_TOL by the norm of the difference relative to
    the tensor's norm.  A tensor that is zero up to rounding has no meaningful relative error: by the rule
    tests/test_gpu_model.py already has for it (largest element below 1e-4 of the largest gradient element of the
    model: the psi bias, whose float64 gradient is ~1e-9 beside elements of ~1e-2) it may instead meet PARAM_GRAD_TOL
    times that largest element, element by element.
    Measured on an MI355X: worst relative error 4.6e-6 (blstm_4.weight_hh, small model), 3.2e-6 (real widths), 2.7e-7
    (K = 1 against the CE step); the psi bias 8e-4 relative, 2e-11 of the largest element."""
    top = max(float(w.abs().max()) for w in want.values())
    worst, floor = [], []
    for k, w in want.items():
        g = got[k].double()
        rel = float((g - w).norm()) / max(float(w.norm()), 1e-300)
        if rel >= PARAM_GRAD_TOL and float(w.abs().max()) < 1e-4 * top:
            floor.append((float((g - w).abs().max()) / top, k, float(w.abs().max())))
        else:
            worst.append((rel, k, float(w.norm())))
    worst.sort(reverse=True)
    for err, k, nrm in worst[:6]:
        print('%s %-40s rel err %.3g (norm %.3g)' % (what, k, err, nrm))
    for err, k, big in floor:
        print('%s %-40s zero up to rounding (largest element %.3g of %.3g): abs err / top %.3g' % (what, k, big, top, err))
    assert worst[0][0] < PARAM_GRAD_TOL, worst[:3]
    assert all(err < PARAM_GRAD_TOL for err, _, _ in floor), floor


@pytest.mark.parametrize('name', ['tiny', 'full'])
def test_step_gradients_match_the_oracle_driven_the_same_way(name):
    """(a) and (c): fixed hypotheses; every parameter's gradient against OracleASR in float64; the recorded risk
    against the expected risk recomputed on the host from last_logits, last_rows and last_counts."""
    from ss_asr_amd.engine import MWERTrainStep
    case = step_case(name)
    model, ref = case['model'], case['ref']
    from ss_asr_amd import ops
    step = MWERTrainStep(model, case['K'], ce_weight=0.1, unit='char', space=SPACE)
    ops.set_wgrad_listener(None)                   # forward_loss + backward by hand: no reducer is listening
    step.optim.zero_grad()
    ref.zero_grad()
    hyps = tuple(t.to(DEV) for t in case['hyps'])
    loss, logits = step.forward_loss(case['x'].to(DEV), case['y'].to(DEV), case['lens'], hyps=hyps)
    loss.backward()
    ops.join_side_stream()
    torch.cuda.synchronize()
    ops.check_persistent_status()
    want, want_risk, rows, counts, ref_logits = oracle_forward(case, case['hyps'], 0.1, 0)
    want.backward()
    assert np.array_equal(step.last_rows.cpu().numpy(), rows)
    assert np.array_equal(step.last_counts.cpu().numpy(), counts)
    assert logits.shape == ref_logits.shape and logits.shape[0] == case['B'] * (case['K'] + 1) and logits.shape[1] <= 12
    print('loss %.9f (oracle %.9f)' % (float(loss), float(want)))
    assert abs(float(loss) - float(want)) < 1e-4 * max(1.0, abs(float(want)))       # (the first-step bound of the trainer tests)
    compare_parameter_gradients({k: p.grad.detach().cpu() for k, p in model.named_parameters()},
                                {k: p.grad.detach() for k, p in ref.named_parameters()}, name)
    # (c) the recorded risk, recomputed on the host from what the step left
    _, host_risk, _ = mwer_reference(step.last_logits.detach().cpu(), step.last_rows.cpu(), step.last_hyps[2].cpu(),
                                     step.last_counts.cpu(), 0)
    close(step.last_risk, host_risk, LOSS_TOL, 'last_risk')
    assert step.last_risk.is_cuda and float(host_risk.max()) > 0


def test_with_one_hypothesis_and_ce_weight_one_the_step_is_the_ce_step():
    """(b): K = 1, ce_weight = 1: the single hypothesis' sequence-level weight is 0, so the loss is the masked CE plus
    the (constant) risk and the gradients are ASRTrainStep.forward_loss's with tf_rate 1."""
    from ss_asr_amd import ops
    from ss_asr_amd.engine import ASRTrainStep, MWERTrainStep, label_geometry
    case = step_case('tiny')
    model = case['model']
    x, y = case['x'].to(DEV), case['y'].to(DEV)
    chars, n_chars, _ = case['hyps']
    hyps = (chars[:, 2:3].contiguous().to(DEV), n_chars[:, 2:3].contiguous().to(DEV),
            torch.ones(case['B'], dtype=torch.int32, device=DEV))
    step = MWERTrainStep(model, 1, ce_weight=1.0, unit='word', space=SPACE)
    ops.set_wgrad_listener(None)
    step.optim.zero_grad()
    loss, logits = step.forward_loss(x, y, case['lens'], hyps=hyps)
    loss.backward()
    ops.join_side_stream()
    torch.cuda.synchronize()
    got = {k: p.grad.detach().cpu().double().clone() for k, p in model.named_parameters()}
    assert float(step.last_info.weight.view(case['B'], 2)[:, 0].abs().max()) <= GRAD_TOL
    _, ans_len = label_geometry(case['y'])
    ce = ops.masked_ce_loss(logits[1::2, :ans_len].contiguous(), y, ans_len)
    ce_part = loss.detach().double() - step.last_risk.double().mean()
    close(ce_part, ce, LOSS_TOL, 'loss - risk against the masked CE')
    keep, model.tf_rate = model.tf_rate, 1.0
    try:
        ce_step = ASRTrainStep(model)
        ops.set_wgrad_listener(None)
        ce_step.optim.zero_grad()
        ce_loss, _, _ = ce_step.forward_loss(x, y, case['lens'], ans_len)
        ce_loss.backward()
        ops.join_side_stream()
        torch.cuda.synchronize()
    finally:
        model.tf_rate = keep
    close(ce_part, ce_loss, LOSS_TOL, 'loss - risk against the CE step')
    compare_parameter_gradients(got, {k: p.grad.detach().cpu().double() for k, p in model.named_parameters()}, 'K = 1')
    ops.check_persistent_status()


def test_the_search_runs_on_the_batch_mode_features():
    """(d): with hyps=None the hypotheses are ops.decode_beam's on the batch-mode encoder output of this very batch,
    not decode_nbest's, which encodes every utterance alone."""
    from ss_asr_amd import ops
    from ss_asr_amd.engine import MWERTrainStep
    case = step_case('tiny')
    model = case['model']
    x, y = case['x'].to(DEV), case['y'].to(DEV)
    step = MWERTrainStep(model, 3, max_decoding_steps=12, space=SPACE)
    ops.set_wgrad_listener(None)
    step.optim.zero_grad()
    loss, _ = step.forward_loss(x, y, case['lens'])
    with torch.no_grad():
        feat, _, enc_len_dev, _, _ = model.encode(x, case['lens'])
        chars, n_chars, _, n_hyps = ops.decode_beam(feat, enc_len_dev, model._decoder_params(),
                                                    (model.attention.psi.weight, model.attention.psi.bias), None, 0.0,
                                                    EOS, 12, 3)
    torch.cuda.synchronize()
    assert np.isfinite(float(loss))
    for got, want in zip(step.last_hyps, (chars, n_chars, n_hyps)):
        assert torch.equal(got, want)
    # decode_nbest encodes each utterance alone: blstm_4 recurs over the utterance axis, so its features differ
    alone, _ = model.encoder(x[1:2, :case['lens'][1]], [case['lens'][1]])
    assert float((alone[0] - feat[1, :alone.shape[1]]).abs().max()) > 1e-4
    ops.check_persistent_status()


def trainer_config(index, mwer):
    conf = {'asr': {'opt': {'type': 'Adadelta', 'learning_rate': 1.0},
                    'mdl': {'encoder_state_size': 256, 'mlp_out_size': 128, 'decoder_state_size': 256, 'tf_rate': 1.0,
                            'feature_dim': 80},
                    'train_index': index, 'valid_index': index, 'wer_step': 1, 'train_batch_size': 8,
                    'valid_batch_size': 8, 'n_epochs': 2, 'logging_step': 1, 'save_step': 100, 'valid_step': 100,
                    'loader_jobs': 0, 'gpu_resident_loader': False}}
    if mwer:
        conf['asr']['mwer'] = {'beam_size': 2, 'ce_weight': 0.05, 'unit': 'word', 'max_decoding_steps': 12}
    return conf


def run_trainer(root, name, mwer, seed=1):
    import json
    from ss_asr_amd.trainer import ASRTrainer
    index = os.path.join(root, 'index.tsv')
    paras = types.SimpleNamespace(name=name, logdir=os.path.join(root, 'runs'), ckpdir=os.path.join(root, 'result'),
                                  verbose=False, seed=seed)
    random.seed(seed); np.random.seed(seed); torch.manual_seed(seed)
    tr = ASRTrainer(trainer_config(index, mwer), paras)
    tr.load_data()
    tr.set_model()
    start = {k: v.detach().cpu().clone() for k, v in tr.asr_model.state_dict().items()}
    tr.exec()
    tr.close()
    torch.cuda.synchronize()
    events = [json.loads(l) for l in open(os.path.join(root, 'runs', name, 'asr', 'events.jsonl'))]
    return tr, start, events


def test_trainer_with_and_without_the_mwer_mapping(tmp_path):
    """(e): with asr.mwer the trainer drives MWERTrainStep for two iterations and logs mwer_risk; without it the
    first step's loss has the bits of ASRTrainStep called directly on the same weights and batch."""
    from ss_asr_amd.ASRDataset import load_asr_dataset, prepare_x, prepare_y
    from ss_asr_amd.asr import ASR
    from ss_asr_amd.engine import ASRTrainStep, MWERTrainStep
    root = str(tmp_path)
    index, _ = make_corpus(root, n=8, t_max=64, feat=80, seed=3)
    tr, _, events = run_trainer(root, 'mwer', True)
    assert isinstance(tr.train_step, MWERTrainStep) and tr.train_step.beam_size == 2
    risks = [e['value'] for e in events if e['key'] == 'asr_mwer_risk']
    losses = [e['value'] for e in events if e['key'] == 'asr_train_loss']
    assert len(risks) == 2 and len(losses) == 2 and all(np.isfinite(risks + losses)) and min(risks) >= 0
    assert tr.train_step.finish()[1] == 0                 # no skipped step

    tr, start, events = run_trainer(root, 'plain', False)
    assert type(tr.train_step) is ASRTrainStep
    assert not any(e['key'] == 'asr_mwer_risk' for e in events)
    losses = [e['value'] for e in events if e['key'] == 'asr_train_loss']
    _, _, loader = load_asr_dataset(index, batch_size=8, n_jobs=0)
    x, y = next(iter(loader))
    x, x_lens = prepare_x(x, device=DEV)
    y, y_lens = prepare_y(y, device=DEV)
    model = ASR(tr.mapper.get_dim(), 256, 256, 128, 80, 1.0)
    model.load_state_dict(start)
    direct = ASRTrainStep(model.to(DEV), lr=1.0, eps=1e-8, grad_clip=5.0)
    want = direct(x, y, x_lens, max(y_lens) - 1)
    direct.finish()
    assert losses[0] == float(want), (losses[0], float(want))
