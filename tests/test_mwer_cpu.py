"""MWER training without a GPU: postprocess.mwer_reference (the float64 restatement that the loss kernels are defined
against) on a hand-worked case and against a brute-force computation, the argument checks of the new entries, which
return before any HIP call, and ASRTrainer's validation of the asr.mwer mapping."""
import ctypes
import math

import pytest
import torch

from ss_asr_amd.postprocess import mwer_reference


def brute_force(logits, rows, n_hyps, counts, unit, ce_w):
    """The definition of include/ssasr.h written out with Python floats (float64) and loops."""
    R, U, V = logits.shape
    G = len(n_hyps)
    M = R // G
    z = logits.double().tolist()
    logp = []
    for r in range(R):
        total = 0.0
        for t in range(U):
            lab = int(rows[r][t + 1]) if t + 1 < rows.shape[1] else 0
            if lab == 0:
                continue
            mx = max(z[r][t])
            total += z[r][t][lab] - (mx + math.log(sum(math.exp(v - mx) for v in z[r][t])))
        logp.append(total)
    risk, p_hat = [], [0.0] * R
    for g in range(G):
        n = min(max(int(n_hyps[g]), 0), M)
        members = [g * M + k for k in range(n)]
        rbar = 0.0
        if members:
            mx = max(logp[r] for r in members)
            den = sum(math.exp(logp[r] - mx) for r in members)
            for r in members:
                p_hat[r] = math.exp(logp[r] - mx) / den
                rbar += p_hat[r] * sum(int(c) for c in counts[r][4 * unit:4 * unit + 3])
        risk.append(rbar)
    loss = sum(risk) / G
    if ce_w is not None:
        loss += sum(float(ce_w[r]) * -logp[r] for r in range(R))
    return loss, risk, p_hat


def test_a_hand_worked_two_hypothesis_case():
    """One group, two one-step hypotheses over two classes with uniform logits: each row's logP is log(1/2), the
    posterior is (1/2, 1/2), word risks 2 and 0 give an expected risk of 1; character risks 1 and 3 give 2; a CE weight
    of 0.5 on row 0 adds 0.5 log 2."""
    logits = torch.zeros(2, 1, 2)
    rows = torch.tensor([[0, 1], [0, 1]], dtype=torch.int32)
    counts = torch.tensor([[1, 0, 0, 3, 1, 1, 0, 2], [0, 2, 1, 3, 0, 0, 0, 2]], dtype=torch.int32)
    n_hyps = torch.tensor([2], dtype=torch.int32)
    loss, risk, p_hat = mwer_reference(logits, rows, n_hyps, counts, 'word')
    assert loss.dtype == torch.float64
    assert abs(float(loss) - 1.0) < 1e-15 and abs(float(risk[0]) - 1.0) < 1e-15
    assert p_hat.tolist() == [0.5, 0.5]
    loss, _, _ = mwer_reference(logits, rows, n_hyps, counts, 'char', torch.tensor([0.5, 0.0]))
    assert abs(float(loss) - (2.0 + 0.5 * math.log(2.0))) < 1e-15
    # a lower logit on the costly hypothesis' label moves the posterior away from it: 1/3 against 2/3
    logits = torch.tensor([[[0.0, -math.log(2.0)]], [[0.0, 0.0]]], dtype=torch.float64)
    lp0, lp1 = math.log(1 / 3), math.log(1 / 2)
    p0 = math.exp(lp0) / (math.exp(lp0) + math.exp(lp1))
    loss, _, p_hat = mwer_reference(logits, rows, n_hyps, counts, 1)
    assert abs(float(p_hat[0]) - p0) < 1e-15 and abs(float(loss) - 2.0 * p0) < 1e-15
    with pytest.raises(ValueError):
        mwer_reference(logits, rows, n_hyps, counts, 2)


@pytest.mark.parametrize('unit', [0, 1])
@pytest.mark.parametrize('with_ce', [False, True])
def test_the_reference_equals_a_brute_force_computation_and_differentiates(unit, with_ce):
    gen = torch.Generator().manual_seed(11 + unit)
    G, M, U, V = 3, 4, 6, 7
    R = G * M
    logits = (2.0 * torch.randn(R, U, V, generator=gen)).requires_grad_()
    rows = torch.randint(1, V, (R, U + 2), generator=gen, dtype=torch.int32)
    rows[:, 0] = 0
    rows[1, 3] = 0                       # an interior zero
    rows[2, 4:] = 0                      # a short row
    rows[:, U + 1] = 5                   # a column the loss never reads as a label
    counts = torch.randint(0, 6, (R, 8), generator=gen, dtype=torch.int32)
    n_hyps = torch.tensor([4, 2, 0], dtype=torch.int32)
    ce_w = torch.rand(R, generator=gen) * 0.1 if with_ce else None
    loss, risk, p_hat = mwer_reference(logits, rows, n_hyps, counts, unit, ce_w)
    want_loss, want_risk, want_p = brute_force(logits.detach(), rows, n_hyps.tolist(), counts.tolist(), unit, ce_w)
    assert abs(float(loss.detach()) - want_loss) < 1e-12
    assert max(abs(a - b) for a, b in zip(risk.tolist(), want_risk)) < 1e-12
    assert max(abs(a - b) for a, b in zip(p_hat.tolist(), want_p)) < 1e-12
    assert risk[2] == 0 and p_hat[2 * M:].abs().max() == 0 and p_hat[M + 2:2 * M].abs().max() == 0
    (grad,) = torch.autograd.grad(loss, logits)
    assert torch.isfinite(grad).all()
    # the derivative restated: dloss / dz = w_r (softmax - onehot) on labelled steps
    lab = rows[:, 1:U + 1].long()
    err = counts.double()[:, 4 * unit:4 * unit + 3].sum(1)
    w = -p_hat.detach() * (err - risk.detach().repeat_interleave(M)) / G
    if with_ce:
        w = w + ce_w.double()
    want = w.view(R, 1, 1) * (torch.softmax(logits.detach().double(), -1) - torch.nn.functional.one_hot(lab, V))
    want = want * (lab != 0).unsqueeze(2)
    assert (grad.double() - want).abs().max() < 1e-6      # (autograd ran in the float32 of `logits`' leaf)


def test_logp_values_a_thousand_apart_give_a_one_hot_posterior():
    logits = torch.zeros(2, 1, 2)
    logits[1, 0, 1] = -1000.0
    rows = torch.tensor([[0, 1], [0, 1]], dtype=torch.int32)
    counts = torch.tensor([[0] * 4 + [3, 0, 0, 3], [0] * 4 + [0, 0, 0, 3]], dtype=torch.int32)
    loss, risk, p_hat = mwer_reference(logits, rows, torch.tensor([2], dtype=torch.int32), counts, 1)
    assert math.isfinite(float(loss)) and p_hat.tolist() == [1.0, 0.0] and float(risk[0]) == 3.0


def _lib():
    from ss_asr_amd import _lib
    return _lib, _lib.load()


def test_the_new_entries_are_bound_and_the_abi_version_stays():
    _lib_mod, lib = _lib()
    for name in ('ssasr_mwer_ws_bytes', 'ssasr_mwer_loss_fwd', 'ssasr_mwer_loss_bwd', 'ssasr_mwer_pack',
                 'ssasr_rows_repeat_fwd', 'ssasr_rows_repeat_bwd'):
        assert name in _lib_mod.SIGNATURES and hasattr(lib, name)
    assert lib.ssasr_abi_version() == 16
    # the workspace: 3 R + 2 G + 8 R + R U doubles, then R U floats rounded up to whole doubles
    assert lib.ssasr_mwer_ws_bytes(3, 4, 9) == 8 * (36 + 6 + 96 + 108) + 8 * ((12 * 9 + 1) // 2)
    assert lib.ssasr_mwer_ws_bytes(1, 0, 4) == 0 and lib.ssasr_mwer_ws_bytes(1, 34, 4) == 0
    assert lib.ssasr_mwer_ws_bytes(2000, 33, 4) == 0 and lib.ssasr_mwer_ws_bytes(1, 1, 0) == 0


def test_the_loss_entries_reject_bad_arguments_before_any_hip_call():
    _, lib = _lib()
    buf = (ctypes.c_double * 4096)()
    base = ctypes.addressof(buf)
    p = ctypes.c_void_p(base)
    G, M, U, V = 2, 3, 4, 5
    need = lib.ssasr_mwer_ws_bytes(G, M, U)
    assert 0 < need <= ctypes.sizeof(buf)

    def fwd(logits=p, y=p, y_ld=U + 1, y_cols=U + 1, n_hyps=p, counts=p, unit=1, ce_w=None, G=G, M=M, U=U, V=V, ws=p,
            ws_bytes=need, risk=p, loss=p):
        return lib.ssasr_mwer_loss_fwd(logits, y, y_ld, y_cols, n_hyps, counts, unit, ce_w, G, M, U, V, ws, ws_bytes,
                                       risk, loss, None)

    def bwd(logits=p, y=p, y_ld=U + 1, y_cols=U + 1, G=G, M=M, U=U, V=V, ws=p, ws_bytes=need, dloss=p, dlogits=p):
        return lib.ssasr_mwer_loss_bwd(logits, y, y_ld, y_cols, G, M, U, V, ws, ws_bytes, dloss, dlogits, None)

    for call in (fwd, bwd):
        assert call(M=0) < 0 and call(M=34) < 0
        assert call(ws=ctypes.c_void_p(base + 4)) < 0, 'a misaligned workspace'
        assert call(ws_bytes=need - 1) < 0 and call(ws=None) < 0
        assert call(G=2000, M=33) < 0                       # G * M > 65535
        assert call(U=0) < 0 and call(V=0) < 0 and call(G=-1) < 0
        assert call(y_cols=U) < 0 and call(y_ld=U) < 0
        assert call(logits=None) < 0 and call(y=None) < 0
    assert fwd(unit=2) < 0 and fwd(unit=-1) < 0
    assert fwd(n_hyps=None) < 0 and fwd(counts=None) < 0 and fwd(risk=None) < 0 and fwd(loss=None) < 0
    assert bwd(dloss=None) < 0 and bwd(dlogits=None) < 0
    assert bwd(G=0, ws=None, ws_bytes=0) == 0               # legal, launches nothing


def test_pack_and_rows_repeat_reject_bad_arguments_before_any_hip_call():
    _, lib = _lib()
    buf = (ctypes.c_int32 * 1024)()
    base = ctypes.addressof(buf)
    p = ctypes.c_void_p(base)

    def pack(chars=p, n_chars=p, n_hyps=p, y_ref=p, ref_ld=6, ref_cols=6, N=2, K=3, steps=5, L=7, rows=p, lens=p):
        return lib.ssasr_mwer_pack(chars, n_chars, n_hyps, y_ref, ref_ld, ref_cols, N, K, steps, 1, L, rows, lens, None)

    assert pack(L=6) < 0, 'L < steps + 2'
    assert pack(ref_cols=8, ref_ld=8) < 0, 'L < ref_cols'
    assert pack(K=0) < 0 and pack(K=33) < 0 and pack(steps=0) < 0 and pack(N=-1) < 0 and pack(ref_ld=5) < 0
    for name in ('chars', 'n_chars', 'n_hyps', 'y_ref', 'rows', 'lens'):
        assert pack(**{name: None}) < 0, name
    assert pack(N=0, chars=None, rows=None) == 0            # legal, launches nothing

    def rep(fn, src=p, G=2, M=3, n=8, dst=p):
        return fn(src, G, M, n, dst, None)

    for fn in (lib.ssasr_rows_repeat_fwd, lib.ssasr_rows_repeat_bwd):
        assert rep(fn, M=0) < 0 and rep(fn, n=0) < 0 and rep(fn, G=-1) < 0 and rep(fn, G=65536) < 0
        assert rep(fn, src=None) < 0 and rep(fn, dst=None) < 0
        assert rep(fn, G=0, src=None, dst=None) == 0
    assert rep(lib.ssasr_rows_repeat_fwd, src=ctypes.c_void_p(base + 2)) < 0


def test_ops_refuse_cpu_tensors_and_malformed_arguments():
    from ss_asr_amd import ops
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
    with pytest.raises(RuntimeError, match='GPU'):
        ops.mwer_loss(torch.zeros(2, 3, 4), i32(2, 4), i32(1), i32(2, 8), 'word')
    with pytest.raises(RuntimeError, match='GPU'):
        ops.mwer_pack(i32(1, 2, 3), i32(1, 2), i32(1), i32(1, 4), 1)
    with pytest.raises(RuntimeError, match='GPU'):
        ops.rows_repeat(torch.zeros(2, 3), 2)


GOOD = dict(beam_size=4, ce_weight=0.05, unit='char', max_decoding_steps=60)


def test_trainer_validates_the_mwer_mapping():
    from ss_asr_amd.trainer import ASRTrainer
    assert ASRTrainer.mwer_options({}) is None and ASRTrainer.mwer_options({'mwer': None}) is None
    assert ASRTrainer.mwer_options({'mwer': dict(GOOD)}) == GOOD
    assert ASRTrainer.mwer_options({'mwer': {'beam_size': 2}}) == dict(beam_size=2, ce_weight=0.01, unit='word',
                                                                     max_decoding_steps=200)
    assert ASRTrainer.mwer_options({'mwer': dict(GOOD, ce_weight=0)})['ce_weight'] == 0.0
    bad = [('beam_size', 1), ('beam_size', 33), ('beam_size', 4.0), ('beam_size', True), ('beam_size', '4'),
           ('ce_weight', -0.1), ('ce_weight', float('nan')), ('ce_weight', float('inf')), ('ce_weight', 'x'),
           ('ce_weight', True), ('unit', 'phone'), ('unit', 1), ('max_decoding_steps', 0),
           ('max_decoding_steps', 2.5), ('max_decoding_steps', 10 ** 6)]
    for key, value in bad:
        with pytest.raises(ValueError, match='asr.mwer.' + key):
            ASRTrainer.mwer_options({'mwer': dict(GOOD, **{key: value})})
    with pytest.raises(ValueError, match='beam_size'):
        ASRTrainer.mwer_options({'mwer': {'unit': 'word'}})
    with pytest.raises(ValueError, match='beam_width'):
        ASRTrainer.mwer_options({'mwer': dict(GOOD, beam_width=3)})
    with pytest.raises(ValueError, match='mapping'):
        ASRTrainer.mwer_options({'mwer': 4})
    with pytest.raises(ValueError, match='label_smoothing'):
        ASRTrainer.mwer_options({'mwer': dict(GOOD), 'label_smoothing': 0.1})
    assert ASRTrainer.mwer_options({'mwer': dict(GOOD), 'label_smoothing': 0.0}) == GOOD
    # the regularisers are untouched by the new key
    assert ASRTrainer.regularisers({'mwer': dict(GOOD)}) == (0.0, None)


def test_the_step_needs_a_gpu_and_sane_arguments():
    from ss_asr_amd.asr import ASR
    from ss_asr_amd.engine import MWERTrainStep
    model = ASR(12, 8, 8, 8, 8, 1.0)
    for kw in (dict(beam_size=0), dict(beam_size=33), dict(beam_size=2, unit='phone'), dict(beam_size=2, ce_weight=-1),
               dict(beam_size=2, max_decoding_steps=0)):
        with pytest.raises(ValueError):
            MWERTrainStep(model, **kw)
    with pytest.raises(RuntimeError, match='GPU'):
        MWERTrainStep(model, 2)
