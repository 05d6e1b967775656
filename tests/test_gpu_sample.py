"""Sampled decoding on the GPU: ssasr_decode_sample (ops.decode_sample, ASR.sample) against test_sample_cpu's float64
checker walking the float64 model of tests/decode_checker.py, K rows a step (it shares nothing with the library's host
code), ssasr_mwer_loss_fwd_ex against postprocess.mwer_reference, and
engine.MWERTrainStep(sampling=True) against OracleASR in float64 driven the same way.

Tolerances.  A step's score row is held to SCORE_ATOL = 5e-5 (test_gpu_decode); a sample's score is a sum of at most
`steps` such entries, hence SCORE_ATOL * steps, and logq is that sum of entries divided by tau, hence times
max(1, 1 / tau).  The uniforms are CONSTRUCTED through the checker: a seeded draw whose u lies within MIN_GAP = 1e-3 of
a running-sum boundary (normalised by the total), or in an interval narrower than 2 * MIN_GAP, is redrawn from the same
seeded stream, so an error inside the bound (1e-3 = 20 * SCORE_ATOL per row entry bounds the error of a normalised
running sum) cannot move a draw and the characters must be EQUAL.  No sample is left out."""
import json
import os
import random
import types

import numpy as np
import pytest
import torch

import decode_checker as dc
import las_oracle as lo
import test_gpu_beam as tgb
import test_gpu_decode as tgd
import test_gpu_mwer as tgm
from test_host_cpu import make_corpus
from test_sample_cpu import sample_walk

from ss_asr_amd.postprocess import mwer_reference

pytestmark = pytest.mark.gpu

SCORE_ATOL = tgd.SCORE_ATOL
MIN_GAP = tgb.MIN_GAP
DEV = tgd.DEV
Mapper = tgd.Mapper
EOS = tgb.EOS
STEPS = tgb.STEPS
KS = (1, 3, 32)
TAUS = (0.5, 1.0, 2.0)
# test_gpu_beam's fixtures and frame counts (T' = 5, 3 and 20) and the 9-frame T' = 1 case of test_gpu_ctc_decode
SHAPES = sorted({(n, f) for n, f, _ in tgb.PAIR_CASES}) + [(n, 9) for n in tgb.SMALL]


model64 = dc.model


def walk(m64, lm_weight, K, tau, choose_u):
    """The K samples of one utterance in float64: sample_walk over one batched model step per step index."""
    return sample_walk(m64.step_fn(lm_weight), m64.start(K), choose_u, tau, EOS, STEPS, K)


def gapped(rng, forced=None, never_eos=()):
    """choose_u of the constructed uniforms.  forced {slot: step}: that slot draws <EOS> at that step (the middle of
    its interval) and not before; never_eos: slots that never draw it.  Every other draw comes from rng and is redrawn
    while it lies within MIN_GAP of a boundary or in an interval narrower than 2 * MIN_GAP."""
    forced = forced or {}

    def choose(k, step, bounds):
        edges = [0.0] + list(bounds)
        if forced.get(k) == step:
            assert edges[EOS + 1] - edges[EOS] >= 2 * MIN_GAP, 'the <EOS> interval is too narrow to be forced'
            return float(np.float32(0.5 * (edges[EOS] + edges[EOS + 1])))
        for _ in range(1000):
            u = float(np.float32(rng.random()))
            v = next((i for i, b in enumerate(bounds) if b > u), len(bounds) - 1)
            if v == EOS and (k in never_eos or k in forced):
                continue
            if edges[v + 1] - edges[v] < 2 * MIN_GAP or u - edges[v] < MIN_GAP or edges[v + 1] - u < MIN_GAP or u >= 1.0:
                continue
            return u
        raise AssertionError('no uniform keeps the gap')
    return choose


def encoded(asr, xs):
    with torch.no_grad():
        return asr._encode_packed(xs, [[x.shape[1]] for x in xs])


def launch(asr, lm, lm_weight, feat, enc_lens, uniforms, tau):
    from ss_asr_amd import ops
    u = torch.tensor(uniforms, dtype=torch.float32).to(DEV) if not torch.is_tensor(uniforms) else uniforms
    out = ops.decode_sample(feat, enc_lens, asr._decoder_params(), (asr.attention.psi.weight, asr.attention.psi.bias),
                            lm, 0.0 if lm is None else lm_weight, EOS, STEPS, u.shape[1], u, tau)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def compare(got, want, tau, what):
    """One utterance's kernel results (index 0 of the launch) against the checker's: -> the worst score and logq errors
    per executed step."""
    chars, n_chars, scores, n_hyps, logq = got
    K = len(want)
    assert chars.shape == (1, K, STEPS) and int(n_hyps[0]) == K
    worst = [0.0, 0.0]
    for k, w in enumerate(want):
        steps = len(w['picks'])
        assert int(n_chars[0, k]) == w['n_chars'], (what, k, int(n_chars[0, k]), w['n_chars'])
        assert np.array_equal(chars[0, k, :w['n_chars']], w['chars']), (what, k)
        assert not chars[0, k, w['n_chars']:].any(), (what, k)
        es, eq = abs(float(scores[0, k]) - w['score']), abs(float(logq[0, k]) - w['logq'])
        assert es <= SCORE_ATOL * steps, (what, k, es)
        assert eq <= SCORE_ATOL * steps * max(1.0, 1.0 / tau), (what, k, eq)
        worst = [max(worst[0], es / steps), max(worst[1], eq / steps * min(1.0, tau))]
    return worst


@pytest.mark.parametrize('name,frames', SHAPES)
def test_the_kernel_draws_what_the_float64_checker_draws(golden, name, frames):
    fx = golden(name)
    asr, lm = tgd.models(fx)
    m64 = model64(golden, name, frames)
    x = torch.from_numpy(fx['x'][:, :frames]).to(DEV)
    feat, enc_lens = encoded(asr, [x])
    assert feat.shape[1] == max(frames // 8, 1)
    weight = float(max(fx['lm_weights']))
    assert weight > 0
    worst, ended, capped = [0.0, 0.0], 0, 0
    for w in (None, weight):
        for K in KS:
            for tau in TAUS:
                rng = np.random.default_rng(1000 * K + int(10 * tau) + (w is not None))
                want = walk(m64, w, K, tau, gapped(rng))
                got = launch(asr, None if w is None else lm, w, feat, enc_lens, [[s['uniforms'] for s in want]], tau)
                err = compare(got, want, tau, (name, frames, w, K, tau))
                worst = [max(a, b) for a, b in zip(worst, err)]
                ended += sum(s['ended'] is not None for s in want)
                capped += sum(s['ended'] is None for s in want)
    print('%s frames %d: %d samples ended by <EOS>, %d by the cap; worst |score error| per step %.2e, worst |logq error| '
          'per step (times min(1, tau)) %.2e (bound %.1e)' % (name, frames, ended, capped, worst[0], worst[1], SCORE_ATOL))
    assert ended + capped == 2 * len(TAUS) * sum(KS) and capped >= 1


@pytest.mark.parametrize('with_lm', [False, True])
def test_finished_slots_leave_the_others_alone(golden, with_lm):
    """Constructed rows: slot 0 draws <EOS> at step 0, slot 1 never draws it (the cap), the rest end at different
    steps, the highest slot early and a middle slot last -- whatever the kernel does with finished slots, every slot
    must match."""
    name, frames = tgb.SMALL[0], 40
    fx = golden(name)
    asr, lm = tgd.models(fx)
    m64 = model64(golden, name, frames)
    feat, enc_lens = encoded(asr, [torch.from_numpy(fx['x'][:, :frames]).to(DEV)])
    w = float(max(fx['lm_weights'])) if with_lm else None
    K = 11                                         # more than one pass of eight vectors
    forced = {0: 0, 2: 7, 3: 1, 4: 19, 5: 2, 6: 12, 7: 3, 8: 23, 9: 5, 10: 1}
    want = walk(m64, w, K, 1.0, gapped(np.random.default_rng(5), forced, never_eos=(1,)))
    assert [s['ended'] for s in want] == [forced.get(k) for k in range(K)]
    assert want[0]['n_chars'] == 0 and want[1]['n_chars'] == STEPS and want[8]['n_chars'] == 23
    got = launch(asr, lm if with_lm else None, w, feat, enc_lens, [[s['uniforms'] for s in want]], 1.0)
    err = compare(got, want, 1.0, 'constructed')
    print('constructed rows, lm %s: n_chars %s, worst |score error| per step %.2e, |logq error| %.2e'
          % (with_lm, got[1][0].tolist(), err[0], err[1]))
    if not with_lm:
        # tau = 1 without an LM: the two sums are the same quantity
        assert np.abs(got[2] - got[4]).max() <= SCORE_ATOL * STEPS


def test_a_group_samples_every_utterance_as_it_samples_alone(golden):
    from ss_asr_amd import ops
    fx = golden(tgb.SMALL[0])
    asr, lm = tgd.models(fx)
    x = torch.from_numpy(fx['x']).to(DEV)
    other = torch.from_numpy(golden(tgb.SMALL[1])['x']).to(DEV)
    both = torch.cat([x, other, x, other], 1)
    xs = [both[:, :f] for f in (160, 40, 9)]                         # T' = 20, 5, 1
    K = 5
    uniforms = torch.rand(3, K, STEPS, generator=torch.Generator().manual_seed(4)).to(DEV)
    feat, enc_lens = encoded(asr, xs)
    assert feat.shape[:2] == (3, 20)
    group = launch(asr, lm, 0.5, feat, enc_lens, uniforms, 1.3)
    assert group[0].shape == (3, K, STEPS) and group[3].tolist() == [K] * 3
    for i, t in enumerate(xs):
        f1, l1 = encoded(asr, [t])
        alone = launch(asr, lm, 0.5, f1, l1, uniforms[i:i + 1].contiguous(), 1.3)
        padded = torch.zeros(1, f1.shape[1] + 3, f1.shape[2], device=DEV)
        padded[:, :f1.shape[1]] = f1
        wide = launch(asr, lm, 0.5, padded, l1, uniforms[i:i + 1].contiguous(), 1.3)
        for g, a, w in zip(group, alone, wide):
            assert np.array_equal(a[0], g[i]) and np.array_equal(w[0], g[i]), i
        for k in range(K):
            assert not group[0][i, k, int(group[1][i, k]):].any()
    # slot k's result does not change when the other slots' uniforms change
    f1, l1 = encoded(asr, [xs[1]])
    changed = uniforms[1:2].clone()
    changed[0, :2] = torch.rand(2, STEPS, generator=torch.Generator().manual_seed(9)).to(DEV)
    changed[0, 3:] = 0.999                                            # the last class at every step: they run into the cap
    again = launch(asr, lm, 0.5, f1, l1, changed, 1.3)
    assert not np.array_equal(again[0][0, 0], group[0][1, 0]) and int(again[1][0, 4]) == STEPS
    steps = min(int(group[1][1, 2]) + 1, STEPS)
    assert int(again[1][0, 2]) == int(group[1][1, 2]) and np.array_equal(again[0][0, 2], group[0][1, 2])
    assert abs(float(again[2][0, 2]) - float(group[2][1, 2])) <= SCORE_ATOL * steps
    assert abs(float(again[4][0, 2]) - float(group[4][1, 2])) <= SCORE_ATOL * steps
    print('slot 2 beside other draws: score %.7f / %.7f, logq %.7f / %.7f' % (
        float(again[2][0, 2]), float(group[2][1, 2]), float(again[4][0, 2]), float(group[4][1, 2])))
    # K = 0 and K = 33 are argument errors before any launch
    for bad in (0, 33):
        with pytest.raises(RuntimeError, match='invalid argument'):
            ops.decode_sample(f1, l1, asr._decoder_params(), (asr.attention.psi.weight, asr.attention.psi.bias), None, 0.0,
                              EOS, STEPS, bad, torch.zeros(1, bad, STEPS, device=DEV))


def test_asr_sample(golden):
    fx = golden(tgb.SMALL[0])
    asr, lm = tgd.models(fx)
    x = torch.from_numpy(fx['x']).to(DEV)
    xs, lens = [x, x[:, :24]], [[40], [24]]
    runs = []
    for _ in range(2):
        gen = torch.Generator(device=DEV).manual_seed(3)
        out = asr.sample(xs, lens, Mapper(), 4, temperature=0.8, rnn_lm=lm, lm_weight=0.5, max_decoding_steps=STEPS,
                         generator=gen)
        runs.append((out, [t.cpu().numpy() for t in asr.last_samples]))
    assert runs[0][0] == runs[1][0] and all(np.array_equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))
    out, (chars, n_chars, scores, n_hyps, logq) = runs[0]
    assert len(out) == 2 and all(len(o) == 4 for o in out) and chars.shape == (2, 4, STEPS) and logq.shape == (2, 4)
    for i in range(2):
        for k in range(4):
            assert out[i][k][0] == tgb.text_of(chars[i, k, :n_chars[i, k]]) and out[i][k][1] == float(scores[i, k])
    assert np.isfinite(scores).all() and np.isfinite(logq).all() and (logq <= 0).all()
    other = asr.sample(xs, lens, Mapper(), 4, temperature=0.8, rnn_lm=lm, lm_weight=0.5, max_decoding_steps=STEPS,
                       generator=torch.Generator(device=DEV).manual_seed(4))
    assert other != out
    # uniforms passed in: the draw of the launch itself
    u = torch.rand(2, 4, STEPS, generator=torch.Generator().manual_seed(1))
    given = asr.sample(xs, lens, Mapper(), 4, max_decoding_steps=STEPS, uniforms=u)
    assert given == asr.sample(xs, lens, Mapper(), 4, max_decoding_steps=STEPS, uniforms=u.to(DEV))
    # score() scores the samples: slot 0 first, the oracle entry is the best of the draws
    refs = [given[0][2][0], 'a b']
    got = asr.score(refs, Mapper())
    assert len(got) == 2 and got[0].oracle[0] in range(4) and sum(got[0].oracle[2][:3]) == 0
    from ss_asr_amd.postprocess import edit_counts
    space = Mapper().char_to_ind(' ')
    ids = [Mapper().char_to_ind(c) for c in refs[1]]
    host = [edit_counts(asr.last_hyps[0][1, k, :int(asr.last_hyps[1][1, k])].cpu().tolist(), ids, space) for k in range(4)]
    assert tuple(host[0][:4]) == got[1].chars and sum(got[1].oracle[2][:3]) == min(sum(h[4:7]) for h in host)
    for bad in (0, 33):
        with pytest.raises(ValueError, match='n_samples'):
            asr.sample(xs, lens, Mapper(), bad)
    with pytest.raises(ValueError, match='uniforms'):
        asr.sample(xs, lens, Mapper(), 4, max_decoding_steps=STEPS, uniforms=u[:, :3])


# ------------------------------------------------------------------------------------------------ the loss ----
LOSS_SHAPES = [((1, 1, 1, 5), [1]), ((3, 4, 9, 31), [4, 2, 0]), ((2, 33, 70, 64), None)]


@pytest.mark.parametrize('with_ce', [False, True])
@pytest.mark.parametrize('unit', [0, 1])
@pytest.mark.parametrize('shape,n_hyps', LOSS_SHAPES)
def test_the_uniform_posterior_against_the_float64_reference(shape, n_hyps, unit, with_ce):
    from ss_asr_amd import ops
    G, M, U, V = shape
    R = G * M
    logits, rows, counts = tgm.make_case(G, M, U, V, seed=sum(shape) + unit)
    n_hyps = torch.tensor(n_hyps if n_hyps is not None else [M] * G, dtype=torch.int32)
    ce_w = (0.2 * torch.rand(R, generator=torch.Generator().manual_seed(5))) if with_ce else None
    ref_logits = logits.double().requires_grad_()
    want, want_risk, want_p = mwer_reference(ref_logits, rows, n_hyps, counts, unit, ce_w, posterior='uniform')
    (want_grad,) = torch.autograd.grad(want, ref_logits, allow_unused=True)
    want_grad = torch.zeros_like(ref_logits) if want_grad is None else want_grad
    got_logits = logits.to(DEV).requires_grad_()
    got, info = ops.mwer_loss(got_logits, rows.to(DEV), n_hyps.to(DEV), counts.to(DEV), unit,
                              None if ce_w is None else ce_w.to(DEV), posterior='uniform')
    got.backward()
    torch.cuda.synchronize()
    tgm.close(got, want, tgm.LOSS_TOL, 'loss')
    tgm.close(info.risk, want_risk, tgm.LOSS_TOL, 'risk')
    tgm.close(info.p_hat, want_p, tgm.GRAD_TOL, 'p_hat')
    tgm.close(got_logits.grad, want_grad, tgm.GRAD_TOL, 'dlogits')
    # the MWER part of a set's weights sums to zero; a set of one and the rows outside a set carry ce_w alone
    n = n_hyps.clamp(0, M)
    inside = (torch.arange(M).unsqueeze(0) < n.long().unsqueeze(1)).reshape(R)
    seq_w = info.weight.cpu() - (ce_w.double() if with_ce else 0.0)
    risk = counts.double()[:, 4 * unit:4 * unit + 3].sum(1)
    assert float((seq_w * inside).view(G, M).sum(1).abs().max()) <= tgm.GRAD_TOL * max(1.0, float(risk.max()))
    assert float(seq_w[~inside].abs().max() if (~inside).any() else 0.0) == 0.0
    if shape == (1, 1, 1, 5):
        assert float(info.p_hat[0]) == 1.0 and float(seq_w.abs().max()) == 0.0
    # logP is what the other posterior leaves
    _, other = ops.mwer_loss(logits.to(DEV), rows.to(DEV), n_hyps.to(DEV), counts.to(DEV), unit,
                             None if ce_w is None else ce_w.to(DEV))
    assert torch.equal(other.logp, info.logp) and torch.equal(other.lse, info.lse)


@pytest.mark.parametrize('shape,n_hyps', LOSS_SHAPES)
def test_posterior_zero_through_the_new_entry_has_the_old_entry_s_bits(shape, n_hyps):
    from ss_asr_amd import _lib, ops
    lib = _lib.load()
    G, M, U, V = shape
    R = G * M
    logits, rows, counts = tgm.make_case(G, M, U, V, seed=sum(shape))
    n_hyps = torch.tensor(n_hyps if n_hyps is not None else [M] * G, dtype=torch.int32).to(DEV)
    logits, rows, counts = logits.to(DEV), rows.to(DEV), counts.to(DEV)
    ce_w = (0.2 * torch.rand(R, generator=torch.Generator().manual_seed(5))).to(DEV)
    need = int(lib.ssasr_mwer_ws_bytes(G, M, U))
    outs = []
    for entry in ('old', 'new'):
        ws = torch.zeros(need // 8, device=DEV, dtype=torch.float64)
        risk = torch.zeros(G, device=DEV)
        loss = torch.zeros((), device=DEV)
        args = (ops._p(logits), ops._p(rows), rows.stride(0), rows.shape[1], ops._p(n_hyps), ops._p(counts), 1,
                ops._p(ce_w), G, M, U, V, ops._p(ws), need, ops._p(risk), ops._p(loss))
        if entry == 'old':
            rc = lib.ssasr_mwer_loss_fwd(*args, ops._stream())
        else:
            rc = lib.ssasr_mwer_loss_fwd_ex(*args, 0, ops._stream())
        torch.cuda.synchronize()
        assert rc == 0
        outs.append((ws.cpu(), risk.cpu(), loss.cpu()))
    for a, b in zip(*outs):
        assert torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a.view(torch.int32),
                           b.view(torch.int64) if b.dtype == torch.float64 else b.view(torch.int32))


# ------------------------------------------------------------------------------------------------ the step ----
def oracle_forward_uniform(case, hyps, ce_weight, unit):
    """test_gpu_mwer.oracle_forward with the uniform posterior: OracleASR in float64 driven as the step is."""
    chars, n_chars, n_hyps = [t.numpy() for t in hyps]
    B, K = chars.shape[0], chars.shape[1]
    M = K + 1
    y = case['y']
    rows, lens = tgm.pack_loop(chars, n_chars, n_hyps, y.numpy().astype(np.int32), EOS, max(chars.shape[2] + 2, y.shape[1]))
    counts = np.array([tgm.edit_counts(rows[r, 1:1 + lens[r]], rows[(r // M) * M + K, 1:1 + lens[(r // M) * M + K]],
                                       tgm.SPACE) for r in range(B * M)], dtype=np.int32)
    ref = case['ref']
    feat, enc_len = ref.encoder(case['x'].double(), case['lens'])
    U = int(lens.max()) + 1
    rows_t = torch.from_numpy(rows)
    logits, _, _, _ = lo.decoder_replay(ref, feat.repeat_interleave(M, 0), np.repeat(np.array(enc_len), M),
                                        rows_t.long(), [0] * U)
    ce_w = torch.zeros(B, M, dtype=torch.float64)
    ce_w[:, K] = ce_weight / (B * (y != 0).sum(1).double())
    loss, risk, _ = mwer_reference(logits, rows_t, torch.from_numpy(n_hyps), torch.from_numpy(counts), unit,
                                   ce_w.view(-1), posterior='uniform')
    return loss, risk, rows, counts, logits


@pytest.mark.parametrize('name', ['tiny', 'full'])
def test_sampled_step_gradients_match_the_oracle_driven_the_same_way(name):
    from ss_asr_amd import ops
    from ss_asr_amd.engine import MWERTrainStep
    case = tgm.step_case(name)
    model, ref = case['model'], case['ref']
    step = MWERTrainStep(model, case['K'], ce_weight=0.1, unit='char', space=tgm.SPACE, sampling=True, seed=0)
    ops.set_wgrad_listener(None)
    step.optim.zero_grad()
    ref.zero_grad()
    hyps = tuple(t.to(DEV) for t in case['hyps'])
    loss, logits = step.forward_loss(case['x'].to(DEV), case['y'].to(DEV), case['lens'], hyps=hyps)
    loss.backward()
    ops.join_side_stream()
    torch.cuda.synchronize()
    ops.check_persistent_status()
    want, want_risk, rows, counts, ref_logits = oracle_forward_uniform(case, case['hyps'], 0.1, 0)
    want.backward()
    assert np.array_equal(step.last_rows.cpu().numpy(), rows) and np.array_equal(step.last_counts.cpu().numpy(), counts)
    print('loss %.9f (oracle %.9f)' % (float(loss), float(want)))
    assert abs(float(loss) - float(want)) < 1e-4 * max(1.0, abs(float(want)))
    tgm.close(step.last_risk, want_risk, 1e-4, 'last_risk')
    # the sets of two and three members have unequal risks: the risk gradient is there
    assert float(step.last_info.weight.view(case['B'], -1)[:, :case['K']].abs().max()) > 1e-3
    tgm.compare_parameter_gradients({k: p.grad.detach().cpu() for k, p in model.named_parameters()},
                                    {k: p.grad.detach() for k, p in ref.named_parameters()}, name + ' sampled')


def test_two_sampled_steps_from_one_seed_repeat(golden):
    from ss_asr_amd.asr import ASR
    from ss_asr_amd.engine import MWERTrainStep
    case = tgm.step_case('tiny')
    x, y = case['x'].to(DEV), case['y'].to(DEV)
    runs = []
    for seed in (5, 5, 6):
        model = ASR(*case['dims'], 1.0)
        lo.seeded_weights(model, 5)
        step = MWERTrainStep(model.to(DEV), 3, max_decoding_steps=12, space=tgm.SPACE, sampling=True, seed=seed)
        seen = []
        for _ in range(2):
            loss = step(x, y, case['lens'])
            seen.append((loss.detach().cpu(),) + tuple(t.cpu() for t in step.last_hyps))
        assert step.finish()[1] == 0
        assert all(int(n) == 3 for n in step.last_hyps[2].cpu())
        runs.append(seen)
    for a, b in zip(runs[0], runs[1]):
        assert all(torch.equal(s, t) for s, t in zip(a, b))
    assert not torch.equal(runs[0][0][1], runs[0][1][1]), 'the second step draws new uniforms'
    assert not torch.equal(runs[0][0][1], runs[2][0][1]), 'another seed draws other samples'
    # lm_weight with sampling is refused on the GPU as well
    with pytest.raises(ValueError, match='lm_weight'):
        MWERTrainStep(case['model'], 3, sampling=True, lm_weight=0.2)


def test_trainer_with_sampled_mwer(tmp_path):
    from ss_asr_amd.engine import MWERTrainStep
    from ss_asr_amd.trainer import ASRTrainer
    root = str(tmp_path)
    index, _ = make_corpus(root, n=8, t_max=64, feat=80, seed=3)
    conf = tgm.trainer_config(os.path.join(root, 'index.tsv'), False)
    conf['asr']['mwer'] = {'beam_size': 3, 'sampling': True, 'seed': 0, 'max_decoding_steps': 12}
    paras = types.SimpleNamespace(name='sampled', logdir=os.path.join(root, 'runs'), ckpdir=os.path.join(root, 'result'),
                                  verbose=False, seed=1)
    random.seed(1); np.random.seed(1); torch.manual_seed(1)
    tr = ASRTrainer(conf, paras)
    tr.load_data()
    tr.set_model()
    tr.exec()
    tr.close()
    torch.cuda.synchronize()
    assert isinstance(tr.train_step, MWERTrainStep) and tr.train_step.sampling and tr.train_step.beam_size == 3
    events = [json.loads(l) for l in open(os.path.join(root, 'runs', 'sampled', 'asr', 'events.jsonl'))]
    risks = [e['value'] for e in events if e['key'] == 'asr_mwer_risk']
    losses = [e['value'] for e in events if e['key'] == 'asr_train_loss']
    assert len(risks) == 2 and len(losses) == 2 and all(np.isfinite(risks + losses)) and min(risks) >= 0
    assert tr.train_step.finish()[1] == 0
