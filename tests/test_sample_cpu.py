"""Sampled decoding without a GPU: the bindings and argument checks of ssasr_decode_sample and ssasr_mwer_loss_fwd_ex
(which return before any HIP call), postprocess.mwer_reference(posterior='uniform') on a hand-worked case and against
float64 autograd of the score-function surrogate, ASRTrainer / MWERTrainStep's validation of the sampling keys, and
sample_walk, a float64 checker of an utterance's samples written here from the words of include/ssasr.h alone (it shares nothing
with the library's host code; tests/test_gpu_sample.py holds the kernel to it)."""
import ctypes
import math

import pytest
import torch

from ss_asr_amd.postprocess import mwer_reference


# ------------------------------------------------------------------------------------------ the checker ----
def sample_walk(step_fn, state, choose_u, tau, eos, max_steps, K=1):
    """The K samples of one utterance of include/ssasr.h's ssasr_decode_sample in Python floats (float64), step by
    step (the samples are independent; they share the walk so that a batched model serves a step of all of them).
    step_fn(state, last) -> (rows: the step's score row of every slot as lists of floats, new state), `last` being
    the K characters fed (<SOS> = 0 first; a finished slot is still fed its last one and its row is dropped).
    choose_u(k, step, bounds) -> the step's uniform of slot k, given bounds[v] = (e_0 + .. + e_v) / total.
    -> per slot dict(chars, n_chars, score, logq, ended: the step whose draw was <EOS>, None for a sample the cap
    ended, picks: every drawn character, the ending <EOS> included, uniforms: what choose_u gave, 0 afterwards)."""
    out = [dict(chars=[], n_chars=max_steps, score=0.0, logq=0.0, ended=None, picks=[], uniforms=[0.0] * max_steps)
           for _ in range(K)]
    last, live = [0] * K, list(range(K))
    for step in range(max_steps):
        if not live:
            break
        rows, state = step_fn(state, list(last))
        for k in list(live):
            row, o = rows[k], out[k]
            z = [r / tau for r in row]
            m = max(z)
            e = [math.exp(v - m) for v in z]
            total = 0.0
            for v in e:
                total += v
            bounds, run = [], 0.0
            for v in e:
                run += v
                bounds.append(run / total)
            u = choose_u(k, step, bounds)
            o['uniforms'][step] = u
            run, pick = 0.0, len(row) - 1
            for v, ev in enumerate(e):
                run += ev
                if run > u * total:
                    pick = v
                    break
            o['picks'].append(pick)
            o['score'] += row[pick]
            o['logq'] += z[pick] - m - math.log(total)
            if pick == eos:
                o['ended'], o['n_chars'] = step, len(o['chars'])
                live.remove(k)
            else:
                o['chars'].append(pick)
                last[k] = pick
    return out


def hand_rows(state, last):
    """Three classes, <EOS> = 1: after <SOS> / class 0 the probabilities are (1/2, 1/4, 1/4), after class 2 they are
    (1/4, 1/4, 1/2).  The state counts the steps."""
    rows = [[math.log(v) for v in ((0.25, 0.25, 0.5) if c == 2 else (0.5, 0.25, 0.25))] for c in last]
    return rows, state + 1


def test_the_checker_on_a_hand_worked_three_class_two_step_case():
    fixed = lambda *us: (lambda k, step, bounds: us[k][step])
    # slot 0: u = 0.6 lies in class 1's interval (1/2, 3/4]: <EOS> at step 0, no characters, both sums log(1/4).
    # slot 1: u = 0.1 draws class 0; after it u = 0.9 lies in class 2's interval (3/4, 1]; the cap ends the sample at
    # two characters, and no <EOS> term is added
    a, b = sample_walk(hand_rows, 0, fixed([0.6, 0.0], [0.1, 0.9]), 1.0, 1, 2, K=2)
    assert a['chars'] == [] and a['n_chars'] == 0 and a['ended'] == 0 and a['picks'] == [1]
    assert abs(a['score'] - math.log(0.25)) < 1e-15 and abs(a['logq'] - math.log(0.25)) < 1e-15
    assert a['uniforms'] == [0.6, 0.0] and b['uniforms'] == [0.1, 0.9]
    assert b['chars'] == [0, 2] and b['n_chars'] == 2 and b['ended'] is None
    assert abs(b['score'] - math.log(0.5 * 0.25)) < 1e-15 and abs(b['logq'] - b['score']) < 1e-15
    # class 2 is fed back: after it class 2 owns (1/2, 1]; then <EOS> at step 2 of a longer run
    (c,) = sample_walk(hand_rows, 0, fixed([0.8, 0.7, 0.3]), 1.0, 1, 3)
    assert c['picks'] == [2, 2, 1] and c['chars'] == [2, 2] and c['n_chars'] == 2 and c['ended'] == 2
    assert abs(c['score'] - math.log(0.25 * 0.5 * 0.25)) < 1e-15
    # tau = 2 flattens: e is proportional to sqrt(p) = (0.7071, 0.5, 0.5), the boundaries 0.4142, 0.7071, 1; the score
    # stays the sum of the UNTEMPERED rows, logq is the tempered distribution's
    (d,) = sample_walk(hand_rows, 0, fixed([0.45, 0.0]), 2.0, 1, 2)
    norm = math.sqrt(0.5) + 1.0
    assert d['picks'] == [1] and abs(d['score'] - math.log(0.25)) < 1e-15
    assert abs(d['logq'] - math.log(0.5 / norm)) < 1e-15
    assert sample_walk(hand_rows, 0, fixed([0.45, 0.0]), 1.0, 1, 2)[0]['picks'][0] == 0
    # a boundary itself is not exceeded: u = 1/2 draws class 1; no running sum exceeds u = 1: class V - 1
    assert sample_walk(hand_rows, 0, fixed([0.5]), 1.0, 1, 1)[0]['picks'] == [1]
    assert sample_walk(hand_rows, 0, fixed([1.0]), 1.0, 1, 1)[0]['picks'] == [2]
    seen = []
    sample_walk(hand_rows, 0, lambda k, s, bounds: seen.append(bounds) or 0.0, 1.0, 1, 1)
    assert max(abs(x - y) for x, y in zip(seen[0], (0.5, 0.75, 1.0))) < 1e-15


# ------------------------------------------------------------------------------- bindings and arguments ----
def _lib():
    from ss_asr_amd import _lib
    return _lib, _lib.load()


def test_the_new_entries_are_bound_and_the_abi_version_stays():
    _lib_mod, lib = _lib()
    for name in ('ssasr_decode_sample_ws_bytes', 'ssasr_decode_sample', 'ssasr_mwer_loss_fwd_ex'):
        assert name in _lib_mod.SIGNATURES and hasattr(lib, name)
    assert lib.ssasr_abi_version() == 16 == _lib_mod.ABI_VERSION


GOOD_SIZES = dict(N=2, K=3, T=20, E=64, A=32, D=64, V=50, Hl=16, S=24)


def test_the_workspace_query_rejects_what_the_beam_query_rejects():
    _, lib = _lib()
    order = ('N', 'K', 'T', 'E', 'A', 'D', 'V', 'Hl', 'S')
    sizes = lambda **kw: [dict(GOOD_SIZES, **kw)[k] for k in order]
    good = lib.ssasr_decode_sample_ws_bytes(*sizes())
    assert 0 < good < lib.ssasr_decode_beam_ws_bytes(*sizes()) and good % 16 == 0      # the state is kept once
    assert lib.ssasr_decode_sample_ws_bytes(*sizes(N=4)) == 2 * good
    bad = [dict(N=0), dict(N=2 ** 31), dict(K=0), dict(K=33), dict(K=-1), dict(T=0), dict(T=16385), dict(E=0), dict(E=66),
           dict(E=8196), dict(A=0), dict(A=30), dict(A=2052), dict(D=0), dict(D=72), dict(D=4112), dict(V=0), dict(V=65),
           dict(Hl=-4), dict(Hl=18), dict(Hl=4100), dict(S=0), dict(S=(1 << 20) + 1)]
    for kw in bad:
        assert lib.ssasr_decode_beam_ws_bytes(*sizes(**kw)) == 0, kw
        assert lib.ssasr_decode_sample_ws_bytes(*sizes(**kw)) == 0, kw
    for K in (1, 32):
        assert lib.ssasr_decode_sample_ws_bytes(*sizes(K=K)) > 0


def test_decode_sample_rejects_bad_arguments_before_any_hip_call():
    _lib_mod, lib = _lib()
    buf = (ctypes.c_float * (1 << 16))()
    base = (ctypes.addressof(buf) + 15) & ~15
    N, K, T, E, A, D, V, S = 1, 2, 4, 8, 4, 16, 5, 3
    need = lib.ssasr_decode_sample_ws_bytes(N, K, T, E, A, D, V, 0, S)
    assert 0 < need <= 4 * (1 << 16) - 16

    def beam(**kw):
        d = _lib_mod.Beam()
        d.N, d.T, d.E, d.A, d.D, d.V, d.max_steps, d.K = N, T, E, A, D, V, S, K
        for name, ctype in _lib_mod.Beam._fields_:
            if ctype is _lib_mod.P:
                setattr(d, name, base)
        d.eos, d.ws_bytes = 1, need
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def call(d=None, uniforms=base, tau=1.0, logq=None, null_s=False):
        d = d if d is not None else beam()
        s = _lib_mod.Sample(uniforms, tau, logq)
        return lib.ssasr_decode_sample(ctypes.byref(d), None if null_s else ctypes.byref(s), None)

    assert call(null_s=True) < 0
    assert lib.ssasr_decode_sample(None, ctypes.byref(_lib_mod.Sample(base, 1.0, None)), None) < 0
    assert call(uniforms=None) < 0
    assert call(uniforms=base + 2) < 0 and call(uniforms=base + 1) < 0, 'misaligned uniforms'
    for tau in (0.0, -1.0, float('nan'), float('inf'), -float('inf')):
        assert call(tau=tau) < 0, tau
    assert call(beam(ws_bytes=need - 1)) < 0 and call(beam(ws=None)) < 0 and call(beam(ws=base + 4)) < 0
    assert call(beam(K=0)) < 0 and call(beam(K=33)) < 0
    # what ssasr_decode_beam refuses is refused here
    assert call(beam(eos=V)) < 0 and call(beam(eos=-1)) < 0 and call(beam(V=65)) < 0 and call(beam(D=20)) < 0
    for name in ('feat', 'enc_len', 'comp', 'w_psi', 'embed', 'w_ct', 'chars', 'n_chars', 'hyp_scores', 'n_hyps'):
        assert call(beam(**{name: None})) < 0, name
    assert call(beam(feat=base + 4)) < 0


def test_the_loss_entry_rejects_an_unknown_posterior_before_any_hip_call():
    _, lib = _lib()
    buf = (ctypes.c_double * 4096)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    G, M, U, V = 2, 3, 4, 5
    need = lib.ssasr_mwer_ws_bytes(G, M, U)

    def fwd(posterior, ws_bytes=need, unit=1, loss=p):
        return lib.ssasr_mwer_loss_fwd_ex(p, p, U + 1, U + 1, p, p, unit, None, G, M, U, V, p, ws_bytes, p, loss,
                                          posterior, None)

    assert fwd(2) < 0 and fwd(-1) < 0
    # and for either posterior, what ssasr_mwer_loss_fwd refuses
    for posterior in (0, 1):
        assert fwd(posterior, ws_bytes=need - 1) < 0 and fwd(posterior, unit=2) < 0 and fwd(posterior, loss=None) < 0


def test_ops_validate_their_arguments_without_a_gpu():
    from ss_asr_amd import ops
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
    with pytest.raises(RuntimeError, match='GPU'):
        ops.mwer_loss(torch.zeros(2, 3, 4), i32(2, 4), i32(1), i32(2, 8), 'word', posterior='uniform')
    params = dict(w_phi=torch.zeros(32, 64), w_ct=torch.zeros(50, 64))
    for K in (0, 33):
        with pytest.raises(RuntimeError, match='invalid argument'):
            ops.decode_sample(torch.zeros(1, 5, 64), i32(1), params, None, None, 0.0, 1, 8, K, torch.zeros(1, K, 8))
    with pytest.raises(RuntimeError, match='GPU'):
        ops.decode_sample(torch.zeros(1, 5, 64), i32(1), params, None, None, 0.0, 1, 8, 2, torch.zeros(1, 2, 8))


# ------------------------------------------------------------------------------------ the reference loss ----
def test_the_uniform_posterior_on_a_hand_worked_case():
    """One group of three one-step rows over two classes, uniform logits (every logP is log 1/2), word risks 3, 0, 0:
    p = 1/3 each, the mean risk is 1, and the row weights -(1/G)(1/3)(risk - 1) are -2/3, 1/3, 1/3.  A step's
    gradient is w (softmax - onehot): row 0, label 1 -> -2/3 * (1/2, -1/2)."""
    logits = torch.zeros(3, 1, 2, dtype=torch.float64, requires_grad=True)
    rows = torch.tensor([[0, 1], [0, 1], [0, 1]], dtype=torch.int32)
    counts = torch.tensor([[0] * 4 + [3, 0, 0, 3], [0] * 4 + [0, 0, 0, 3], [0] * 4 + [0, 0, 0, 3]], dtype=torch.int32)
    n_hyps = torch.tensor([3], dtype=torch.int32)
    loss, risk, p_hat = mwer_reference(logits, rows, n_hyps, counts, 'word', posterior='uniform')
    assert loss.dtype == torch.float64 and abs(float(loss.detach()) - 1.0) < 1e-15 and abs(float(risk[0]) - 1.0) < 1e-15
    assert max(abs(v - 1 / 3) for v in p_hat.tolist()) < 1e-15
    (grad,) = torch.autograd.grad(loss, logits)
    want = torch.tensor([[[-1 / 3, 1 / 3]], [[1 / 6, -1 / 6]], [[1 / 6, -1 / 6]]], dtype=torch.float64)
    assert float((grad - want).abs().max()) < 1e-15
    # the posterior does not follow logP: a much less probable costly row still weighs 1/3
    skew = torch.tensor([[[0.0, -5.0]], [[0.0, 0.0]], [[0.0, 0.0]]], dtype=torch.float64)
    loss, risk, p_hat = mwer_reference(skew, rows, n_hyps, counts, 1, posterior='uniform')
    assert abs(float(loss) - 1.0) < 1e-15 and max(abs(v - 1 / 3) for v in p_hat.tolist()) < 1e-15
    assert float(mwer_reference(skew, rows, n_hyps, counts, 1)[0]) < 0.05          # 'renorm' follows it
    # a set of two of the three rows: the third is outside, the mean is 3/2
    loss, risk, p_hat = mwer_reference(skew, rows, torch.tensor([2], dtype=torch.int32), counts, 1, posterior='uniform')
    assert p_hat.tolist() == [0.5, 0.5, 0.0] and float(risk[0]) == 1.5
    with pytest.raises(ValueError, match='posterior'):
        mwer_reference(skew, rows, n_hyps, counts, 1, posterior='mc')


def random_case(unit, with_ce, seed=23):
    gen = torch.Generator().manual_seed(seed + unit)
    G, M, U, V = 4, 4, 6, 7
    R = G * M
    logits = (2.0 * torch.randn(R, U, V, generator=gen, dtype=torch.float64)).requires_grad_()
    rows = torch.randint(1, V, (R, U + 2), generator=gen, dtype=torch.int32)
    rows[:, 0] = 0
    rows[1, 3] = 0
    rows[2, 4:] = 0
    rows[5] = rows[4]                    # duplicate samples are legitimate draws and stay in the set
    counts = torch.randint(0, 6, (R, 8), generator=gen, dtype=torch.int32)
    counts[5] = counts[4]
    n_hyps = torch.tensor([4, 2, 0, 1], dtype=torch.int32)
    ce_w = torch.rand(R, generator=gen, dtype=torch.float64) * 0.1 if with_ce else None
    return G, M, U, V, logits, rows, counts, n_hyps, ce_w


@pytest.mark.parametrize('unit', [0, 1])
@pytest.mark.parametrize('with_ce', [False, True])
def test_the_uniform_posterior_is_the_score_function_surrogate(unit, with_ce):
    G, M, U, V, logits, rows, counts, n_hyps, ce_w = random_case(unit, with_ce)
    R = G * M
    loss, risk, p_hat = mwer_reference(logits, rows, n_hyps, counts, unit, ce_w, posterior='uniform')
    (grad,) = torch.autograd.grad(loss, logits)
    # the definition, with loops: p = 1 / |S|, the mean risk, the detached coefficients c_r
    err = counts.double()[:, 4 * unit:4 * unit + 3].sum(1)
    c = torch.zeros(R, dtype=torch.float64)
    mean_risk = []
    for g in range(G):
        n = min(max(int(n_hyps[g]), 0), M)
        members = [g * M + k for k in range(n)]
        rbar = sum(float(err[r]) for r in members) / n if n else 0.0
        mean_risk.append(rbar)
        for r in range(g * M, (g + 1) * M):
            want_p = 1.0 / n if r in members else 0.0
            assert abs(float(p_hat[r]) - want_p) < 1e-15
            if r in members:
                c[r] = (1.0 / G) * (1.0 / n) * (float(err[r]) - rbar)
        assert abs(sum(float(c[r]) for r in members)) < 1e-14, 'the weights of a set sum to zero'
    assert max(abs(a - b) for a, b in zip(risk.tolist(), mean_risk)) < 1e-13
    assert float(c[3 * M]) == 0.0, 'a set of one sample gets no risk gradient'
    lab = rows[:, 1:U + 1].long()
    logp = (torch.log_softmax(logits, -1).gather(2, lab.unsqueeze(2)).squeeze(2) * (lab != 0)).sum(1)
    value = sum(mean_risk) / G - (float((ce_w * logp).sum()) if with_ce else 0.0)
    assert abs(float(loss) - value) < 1e-12
    surrogate = (c * logp).sum()
    if with_ce:
        surrogate = surrogate - (ce_w * logp).sum()
    (want,) = torch.autograd.grad(surrogate, logits)
    assert float((grad - want).abs().max()) < 1e-14
    # the same thing as row weights: dloss / dz = w_r (softmax - onehot), w_r = ce_w[r] - c_r
    w = (ce_w if with_ce else 0.0) - c
    direct = w.view(R, 1, 1) * (torch.softmax(logits.detach(), -1) - torch.nn.functional.one_hot(lab, V))
    direct = direct * (lab != 0).unsqueeze(2)
    assert float((grad - direct).abs().max()) < 1e-14
    # with |S| = 1 (group 3) only ce_w remains, outside the sets as well
    only_ce = grad[3 * M:].abs().max()
    assert (float(only_ce) > 0) == with_ce
    if not with_ce:
        assert float(grad[M + 2:2 * M].abs().max()) == 0.0 and float(grad[2 * M:3 * M].abs().max()) == 0.0


@pytest.mark.parametrize('unit', [0, 1])
@pytest.mark.parametrize('with_ce', [False, True])
def test_renorm_reproduces_the_existing_outputs_bit_for_bit(unit, with_ce):
    from test_mwer_cpu import brute_force
    G, M, U, V, logits, rows, counts, n_hyps, ce_w = random_case(unit, with_ce, seed=31)
    old = mwer_reference(logits, rows, n_hyps, counts, unit, ce_w)
    new = mwer_reference(logits, rows, n_hyps, counts, unit, ce_w, posterior='renorm')
    for a, b in zip(old, new):
        assert torch.equal(a.detach(), b.detach())
    (ga,) = torch.autograd.grad(old[0], logits)
    (gb,) = torch.autograd.grad(new[0], logits)
    assert torch.equal(ga, gb)
    want_loss, want_risk, want_p = brute_force(logits.detach(), rows, n_hyps.tolist(), counts.tolist(), unit, ce_w)
    assert abs(float(new[0]) - want_loss) < 1e-12
    assert max(abs(a - b) for a, b in zip(new[2].tolist(), want_p)) < 1e-12


# ------------------------------------------------------------------------------------- the host layers ----
GOOD = dict(beam_size=4, ce_weight=0.05, unit='char', max_decoding_steps=60)


def test_trainer_validates_the_sampling_keys():
    from ss_asr_amd.trainer import ASRTrainer
    # neither key: the mapping it returned before the keys existed
    assert ASRTrainer.mwer_options({'mwer': dict(GOOD)}) == GOOD
    assert ASRTrainer.mwer_options({'mwer': {'beam_size': 2}}) == dict(beam_size=2, ce_weight=0.01, unit='word',
                                                                     max_decoding_steps=200)
    assert ASRTrainer.mwer_options({'mwer': dict(GOOD, sampling=True)}) == dict(GOOD, sampling=True)
    assert ASRTrainer.mwer_options({'mwer': dict(GOOD, sampling=False, seed=0)}) == dict(GOOD, sampling=False, seed=0)
    assert ASRTrainer.mwer_options({'mwer': dict(GOOD, seed=7)}) == dict(GOOD, seed=7)
    for key, value in [('sampling', 1), ('sampling', 'yes'), ('sampling', None), ('seed', -1), ('seed', 1.5),
                       ('seed', True), ('seed', '3'), ('seed', None)]:
        with pytest.raises(ValueError, match='asr.mwer.' + key):
            ASRTrainer.mwer_options({'mwer': dict(GOOD, **{key: value})})
    with pytest.raises(ValueError, match='samples'):
        ASRTrainer.mwer_options({'mwer': dict(GOOD, samples=3)})


def test_the_step_rejects_sampling_with_an_lm_weight():
    from ss_asr_amd.asr import ASR
    from ss_asr_amd.engine import MWERTrainStep
    model = ASR(12, 8, 8, 8, 8, 1.0)
    with pytest.raises(ValueError, match='lm_weight'):
        MWERTrainStep(model, 2, sampling=True, lm_weight=0.3)
    for seed in (-1, 1.5, True):
        with pytest.raises(ValueError, match='seed'):
            MWERTrainStep(model, 2, sampling=True, seed=seed)
    with pytest.raises(RuntimeError, match='GPU'):
        MWERTrainStep(model, 2, sampling=True, seed=3)


def test_asr_sample_validates_before_it_encodes():
    from ss_asr_amd.asr import ASR
    model = ASR(12, 8, 8, 8, 8, 1.0)
    for n in (0, 33):
        with pytest.raises(ValueError, match='n_samples'):
            model.sample([], [], None, n)
    for tau in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='temperature'):
            model.sample([], [], None, 2, temperature=tau)
