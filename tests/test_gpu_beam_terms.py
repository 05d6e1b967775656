"""The beam search's length bonus, coverage term and end detection on the GPU (ssasr_decode_beam_ex; ASR.decode /
decode_many / decode_nbest with length_bonus, coverage_weight, coverage_threshold, end_margin; ASRTester with the
asr.decode_* keys) against the float64 CPU beam search of tests/decode_checker.py with its three terms (and, at
lambda > 0, its CTC term) on.  It shares nothing with the library's host code.

Gaps.  A (case, K, lambda, terms) tuple is compared only when the checker's smallest gap is >= MIN_GAP = 1e-3: kept /
dropped, kept / kept, emitted / emitted, and the stop rule's |max live - (best finished - delta)| at every step it is
evaluated; and, with the coverage term on, only when no |cum'_b[t] - tau| < TAU_MARGIN = 1e-4 for any live b, t and
step (attention rows carry about 1e-6 of float error: the margin keeps that from flipping a count).  The N-best
lists and n_steps must then be EQUAL.

Scores hold the bound of tests/test_gpu_beam.py / test_gpu_ctc_decode.py, 5e-5 * steps + lambda * c: the beta and
eta terms are exact up to the rounding of a handful of float adds.  The worst measured error is printed by every
test and recorded in DESIGN 4.13."""
import math
import os
import shutil
import types

import numpy as np
import pytest
import torch

import decode_checker as dc
import test_gpu_beam as tgb
import test_gpu_ctc_decode as tgc
import test_gpu_decode as tgd
from conftest import GOLDEN
from test_host_cpu import make_corpus

pytestmark = pytest.mark.gpu

SCORE_ATOL = tgd.SCORE_ATOL
MIN_GAP = tgb.MIN_GAP
TAU_MARGIN = 1e-4
DEV = tgd.DEV
Mapper = tgd.Mapper
EOS, STEPS = 1, 24
BEAMS = (2, 3, 5)
LAMBDAS = (0.0, 0.3)
LONG_CASE = 'decode_long_s6'
# (beta, eta, tau, delta), delta None: no end detection: the length bonus alone, the coverage term alone, and all
# three.  Found by sweeping the checker on the CPU.  With these seeded weights the attention is near-uniform (1 / T'
# per frame and step, within 3 %), so a hypothesis' frames cross tau almost together: tau = 0.36 is crossed at the
# second step at T' = 5 and 3 and at the eighth at T' = 20, clear of every level n / T' by more than the margin, and
# eta = 1.5 is what it takes for T' frames' worth of coverage to lift a longer hypothesis over the shorter ones that
# ended before the crossing.  In float64 78 of the 180 tuples keep the gaps: 22 + 29 + 27 per grid entry, 15 at full
# dimensions, 40 with CTC; the list differs from beta = 0 in 24, from eta = 0 in 4; the stop rule ends the loop early in 4.
GRID = ((0.6, 0.0, 0.5, None), (0.0, 1.5, 0.36, None), (0.1, 1.5, 0.36, 0.0))


forced, ref_of, bound = dc.forced, dc.model, tgc.bound
_refs, _beams = {}, {}


def reference(golden, name, frames, k, K, lam, terms, S=STEPS):
    key = (name, frames, k, K, lam, terms, S)
    if key not in _beams:
        w = float(golden(name)['lm_weights'][k])
        _beams[key] = dc.beam_search(ref_of(golden, name, frames), K, S, w, lam, *terms)
    return _beams[key]


def kwargs_of(terms, lam=0.0):
    beta, eta, tau, delta = terms
    return dict(ctc_weight=lam, length_bonus=beta, coverage_weight=eta, coverage_threshold=tau, end_margin=delta)


def arrays(asr):
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in asr.last_beam] + [asr.last_beam_steps.cpu().numpy()]


def lists_of(r):
    return [(h[0], h[2], h[3]) for h in r['hyps']]


def check_against(r, out, nbest, lam, S=STEPS, where=''):
    """The launch's results for one utterance equal the checker's; -> the worst |score error|."""
    chars, n_chars, scores, n_hyps, n_steps = out
    hyps = r['hyps']
    assert int(n_hyps[0]) == len(hyps) == len(nbest) <= chars.shape[1], where
    assert int(n_steps[0]) == r['n_steps'], where
    worst = 0.0
    for i, (ref_chars, ref_score, ended, was_capped, _) in enumerate(hyps):
        n = int(n_chars[0, i])
        assert n == len(ref_chars) and np.array_equal(chars[0, i, :n], ref_chars), (where, i)
        assert not chars[0, i, n:].any()
        assert nbest[i][0] == tgb.text_of(ref_chars) and nbest[i][1] == float(scores[0, i])
        err = abs(float(scores[0, i]) - ref_score)
        worst = max(worst, err)
        assert err <= bound(min(ended + 1, S), lam), (where, i, err)
    rest = slice(len(hyps), None)
    assert not chars[0, rest].any() and not n_chars[0, rest].any() and not scores[0, rest].any()
    return worst


def test_beam_search_with_terms_matches_the_float64_checker(golden):
    compared = full = with_ctc = beta_differs = eta_differs = early = 0
    worst = 0.0
    for name, frames, k in tgb.PAIR_CASES:
        fx = golden(name)
        asr, lm = tgc.models(fx)
        w = float(fx['lm_weights'][k])
        x = torch.from_numpy(fx['x'][:, :frames]).to(DEV)
        for K in BEAMS:
            for lam in LAMBDAS:
                for terms in GRID:
                    r = reference(golden, name, frames, k, K, lam, terms)
                    tag = '%s frames %d lm_weight %.1f K %d lambda %.1f terms %s' % (name, frames, w, K, lam, terms)
                    if r['gap'] < MIN_GAP or (terms[1] != 0 and r['tau_gap'] < TAU_MARGIN):
                        print('%s: smallest gap %.2e, distance from tau %.2e, not compared' % (tag, r['gap'], r['tau_gap']))
                        continue
                    nbest = asr.decode_nbest([x], [[frames]], lm, Mapper(), w, K, max_decoding_steps=STEPS,
                                             **kwargs_of(terms, lam))[0]
                    out = arrays(asr)
                    assert asr.decode(x, [frames], lm, Mapper(), w, max_decoding_steps=STEPS, beam_size=K,
                                      **kwargs_of(terms, lam)) == nbest[0][0]
                    err = check_against(r, out, nbest, lam, where=tag)
                    worst = max(worst, err)
                    print('%s: smallest gap %.2e, %d hypotheses, %d steps, stop rule fired %s, max |score error| %.2e'
                          % (tag, r['gap'], len(r['hyps']), r['n_steps'], r['fired'], err))
                    compared += 1
                    full += name == tgb.FULL_CASE
                    with_ctc += lam > 0
                    early += r['early']
                    beta, eta, tau, delta = terms
                    if beta != 0:
                        off = reference(golden, name, frames, k, K, lam, (0.0, eta, tau, delta))
                        beta_differs += lists_of(off) != lists_of(r)
                    if eta != 0:
                        off = reference(golden, name, frames, k, K, lam, (beta, 0.0, tau, delta))
                        eta_differs += lists_of(off) != lists_of(r)
    print('%d tuples compared: %d at full dimensions, %d with CTC, the list differs from beta = 0 in %d, from eta = 0 '
          'in %d, the stop rule ended the loop early in %d; worst |score error| %.3e'
          % (compared, full, with_ctc, beta_differs, eta_differs, early, worst))
    assert compared >= 12 and full >= 2 and with_ctc >= 3 and beta_differs >= 1 and eta_differs >= 1 and early >= 1


@pytest.mark.parametrize('K', [1, 3])
def test_all_terms_off_is_todays_kernel_bit_for_bit(golden, K):
    from ss_asr_amd import ops
    for name in tgb.SMALL:
        fx = golden(name)
        asr, lm = tgc.models(fx)
        args = tgc.entry_args(asr, lm, torch.from_numpy(fx['x']).to(DEV), 0.5)
        head = tgc.head_of(asr, 0.3)
        for ctc, plain in ((None, ops.decode_beam(*args, K)), (head, ops.decode_beam_ctc(*args, K, head))):
            plain = [t.cpu().numpy() for t in plain]
            # eta = 0: a NaN threshold is ignored; delta < 0 in any form is off
            for tau, delta in ((math.nan, None), (0.5, -0.0001), (math.nan, -math.inf)):
                got = [t.cpu().numpy() for t in ops.decode_beam_ex(*args, K, ctc, length_bonus=0.0, coverage_weight=0.0,
                                                                   coverage_threshold=tau, end_margin=delta)]
                for a, b in zip(plain, got[:4]):
                    assert a.dtype == b.dtype and np.array_equal(a, b)
                longest = int(plain[1][0, :int(plain[3][0])].max())
                assert got[4].dtype == np.int32 and got[4].shape == (1,) and longest <= int(got[4][0]) <= STEPS


def test_a_zero_margin_keeps_the_best_hypothesis(golden):
    """beta = eta = 0, lm_weight >= 0: no step adds to a score, so delta = 0 cannot lose the best hypothesis.  The
    cases are those whose checker run with the rule keeps every gap (the stop rule's comparisons included)."""
    from ss_asr_amd import ops
    terms = (0.0, 0.0, 0.5, 0.0)
    cases = fired = shorter = 0
    for name, frames, k in tgb.PAIR_CASES:
        fx = golden(name)
        asr, lm = tgc.models(fx)
        w = float(fx['lm_weights'][k])
        args = tgc.entry_args(asr, lm, torch.from_numpy(fx['x'][:, :frames]).to(DEV), w)
        for K in (3, 5):
            for lam in LAMBDAS:
                r = reference(golden, name, frames, k, K, lam, terms)
                if r['gap'] < MIN_GAP:
                    continue
                ctc = tgc.head_of(asr, lam) if lam > 0 else None
                free = [t.cpu().numpy() for t in ops.decode_beam_ex(*args, K, ctc)]
                got = [t.cpu().numpy() for t in ops.decode_beam_ex(*args, K, ctc, end_margin=0.0)]
                assert np.array_equal(got[0][0, 0], free[0][0, 0]) and got[1][0, 0] == free[1][0, 0]
                assert got[2][0, 0].tobytes() == free[2][0, 0].tobytes()

                def emitted(o, finished_only):
                    return [(tuple(o[0][0, i, :o[1][0, i]]), o[2][0, i].tobytes()) for i in range(int(o[3][0]))
                            if not finished_only or o[1][0, i] < STEPS]
                assert 1 <= int(got[3][0]) <= int(free[3][0])
                if r['fired']:                      # what was live is dropped: finished hypotheses alone are left
                    assert all(h in emitted(free, True) for h in emitted(got, False))
                else:                               # the rule never held: the search without it, the cap's list included
                    assert all(np.array_equal(a, b) for a, b in zip(got, free))
                assert int(got[4][0]) == r['n_steps'] <= int(free[4][0])
                print('%s frames %d lm_weight %.1f K %d lambda %.1f: %d of %d hypotheses, %d of %d steps'
                      % (name, frames, w, K, lam, int(got[3][0]), int(free[3][0]), int(got[4][0]), int(free[4][0])))
                cases += 1
                fired += r['fired']
                shorter += int(got[4][0]) < int(free[4][0])
    print('%d cases, the rule fired in %d and shortened the loop in %d' % (cases, fired, shorter))
    assert cases >= 8 and fired >= 4 and shorter >= 4


def long_small_input(golden):
    """1100 frames (T' = 137: more than one wave of frames, no multiple of 4) for the small-dimension models."""
    a, b = (golden(n)['x'] for n in tgb.SMALL)
    x = np.concatenate([a, b] * 14, 1)[:, :1100]
    return x * np.linspace(0.5, 1.5, 1100, dtype=np.float32)[None, :, None]


@pytest.mark.parametrize('K', [8, 32])
def test_the_coverage_term_of_every_emitted_hypothesis_is_eta_times_its_count(golden, K):
    """No gap is needed: whatever the kernel chose, an emitted score minus the score of the same prefix teacher-forced
    without the term must be eta * cov(prefix), as long as no sum of that prefix lies within TAU_MARGIN of tau."""
    eta, S = 0.5, 12
    if K == 8:
        name = LONG_CASE
        fx = golden(name)
        xs = fx['x']
    else:
        name = tgb.SMALL[0]
        fx = golden(name)
        xs = long_small_input(golden)
    asr, lm = tgc.models(fx)
    key = (name, 'long', K)
    if key not in _refs:
        _refs[key] = dc.Model(dict(fx, x=xs) if K == 32 else fx, 1100)
    ref = _refs[key]
    assert ref.T == 137
    tau = 2.5 / 137                                   # near-uniform attention: crossed at about the third step
    w = float(fx['lm_weights'][1])
    x = torch.from_numpy(xs).to(DEV)
    nbest = asr.decode_nbest([x], [[1100]], lm, Mapper(), w, K, max_decoding_steps=S, coverage_weight=eta,
                             coverage_threshold=tau)[0]
    chars, n_chars, scores, n_hyps, n_steps = arrays(asr)
    nh = int(n_hyps[0])
    assert 1 <= nh <= K and len(nbest) == nh and 1 <= int(n_steps[0]) <= S
    checked = counted = 0
    for i in range(nh):
        n = int(n_chars[0, i])
        text, ended = [int(c) for c in chars[0, i, :n]], n < S
        base, cov, tau_gap = forced(ref, text, ended, 0.0, w, tau)
        err = abs(float(scores[0, i]) - base - eta * cov)
        print('K %d hypothesis %d: %d characters, %s, score %.6f, without the term %.6f, cov %d, distance from tau '
              '%.2e, error %.2e' % (K, i, n, 'ended' if ended else 'capped', float(scores[0, i]), base, cov, tau_gap, err))
        if tau_gap < TAU_MARGIN:
            continue
        assert err <= bound(n + ended, 0.0)
        checked += 1
        counted += cov > 0
    assert checked >= 1 and counted >= 1


def test_a_large_length_bonus_runs_every_hypothesis_to_the_cap(golden):
    for name in tgb.SMALL:
        fx = golden(name)
        asr, lm = tgc.models(fx)
        # above the largest |score row entry| of the fixture: a parent's 49 characters all beat its <EOS>
        beta = math.ceil(max(float(np.abs(fx['w%d_scores' % k]).max()) for k in (0, 1))) + 1.0
        ref = ref_of(golden, name, 40)
        x = torch.from_numpy(fx['x']).to(DEV)
        for K in (3, 5):
            w = float(fx['lm_weights'][1])
            nbest = asr.decode_nbest([x], [[40]], lm, Mapper(), w, K, max_decoding_steps=STEPS, length_bonus=beta)[0]
            chars, n_chars, scores, n_hyps, n_steps = arrays(asr)
            assert int(n_hyps[0]) == K == len(nbest) and int(n_steps[0]) == STEPS
            assert (n_chars[0] == STEPS).all() and not (chars[0] == EOS).any()
            for i in range(K):
                base, _, _ = forced(ref, [int(c) for c in chars[0, i]], False, 0.0, w, 1.0)
                err = abs(float(scores[0, i]) - (base + STEPS * beta))
                print('%s K %d hypothesis %d: score %.5f, beta = 0 score of the prefix %.5f + %d x %.1f, error %.2e'
                      % (name, K, i, float(scores[0, i]), base, STEPS, beta, err))
                assert err <= bound(STEPS, 0.0)


@pytest.mark.parametrize('lam', [0.0, 0.3])
def test_a_group_decodes_every_utterance_as_it_decodes_alone(golden, lam):
    fx = golden(tgb.SMALL[0])
    asr, lm = tgc.models(fx)
    x = torch.from_numpy(fx['x']).to(DEV)
    other = torch.from_numpy(golden(tgb.SMALL[1])['x']).to(DEV)
    both = torch.cat([x, other, x, other], 1)
    xs = [both[:, :f] for f in (160, 40, 25, 9)]                    # T' = 20, 5, 3, 1
    lens = [[t.shape[1]] for t in xs]
    kw = kwargs_of((0.3, 0.25, 0.35, 0.5), lam)
    texts = asr.decode_many(xs, lens, lm, Mapper(), 0.5, max_decoding_steps=STEPS, beam_size=3, **kw)
    group = arrays(asr)
    assert group[0].shape == (4, 3, STEPS) and group[3].shape == (4,) and group[4].shape == (4,)
    for i, (t, l) in enumerate(zip(xs, lens)):
        assert asr.decode(t, l, lm, Mapper(), 0.5, max_decoding_steps=STEPS, beam_size=3, **kw) == texts[i]
        alone = arrays(asr)
        for a, b in zip(alone, group):
            assert np.array_equal(a[0], b[i]), i
        nh = int(group[3][i])
        assert 1 <= nh <= 3 and 1 <= int(group[4][i]) <= STEPS
        assert not group[0][i, nh:].any() and not group[1][i, nh:].any() and not group[2][i, nh:].any()


def test_width_one_with_a_term_on_is_the_beam_kernel(golden):
    name, frames = tgb.SMALL[0], 40
    fx = golden(name)
    asr, lm = tgc.models(fx)
    x = torch.from_numpy(fx['x']).to(DEV)
    w = float(fx['lm_weights'][1])
    compared = 0
    for lam in LAMBDAS:
        for terms in GRID:
            r = reference(golden, name, frames, 1, 1, lam, terms)
            if r['gap'] < MIN_GAP or (terms[1] != 0 and r['tau_gap'] < TAU_MARGIN):
                continue
            asr.last_beam = asr.last_beam_steps = None
            nbest = asr.decode_nbest([x], [[frames]], lm, Mapper(), w, 1, max_decoding_steps=STEPS,
                                     **kwargs_of(terms, lam))[0]
            out = arrays(asr)
            assert out[0].shape == (1, 1, STEPS)
            check_against(r, out, nbest, lam, where='K 1 lambda %.1f terms %s' % (lam, terms))
            compared += 1
    assert compared >= 2
    # every term off: beam_size 1 is the greedy kernel, last_beam stays what it was
    marker, steps = asr.last_beam, asr.last_beam_steps
    asr.last_decode = None
    nbest = asr.decode_nbest([x], [[frames]], lm, Mapper(), w, 1, max_decoding_steps=STEPS)
    assert asr.last_decode is not None and asr.last_beam is marker and asr.last_beam_steps is steps
    assert nbest[0][0][0] == asr.decode(x, [frames], lm, Mapper(), w, max_decoding_steps=STEPS)


def test_asr_tester_with_the_new_keys(tmp_path):
    from ss_asr_amd.ASRDataset import prepare_x
    from ss_asr_amd.trainer import ASRTester
    fx = np.load(os.path.join(GOLDEN, 'dataset_ref.npz'), allow_pickle=False)
    dims = [int(v) for v in fx['cpt_dims']]
    root = str(tmp_path)
    index, lens = make_corpus(root, n=5, t_max=40, feat=dims[4], seed=5)
    os.makedirs(os.path.join(root, 'result', 'dec'))
    shutil.copy(os.path.join(GOLDEN, 'ref_small_asr.cpt'), os.path.join(root, 'result', 'dec', 'asr.cpt'))

    def tester(**decode_keys):
        config = {'asr': dict({'mdl': {'encoder_state_size': dims[1], 'decoder_state_size': dims[2],
                                       'mlp_out_size': dims[3], 'feature_dim': dims[4], 'tf_rate': 1.0},
                               'test_index': index, 'decode_lm_weight': 0.5, 'decode_beam_size': 3, 'decode_jobs': 1,
                               'max_decode_step_ratio': 0.25, 'loader_jobs': 0}, **decode_keys),
                  'char_lm': {'mdl': {'hidden_size': 16}}}
        paras = types.SimpleNamespace(name='dec', logdir=os.path.join(root, 'runs'), ckpdir=os.path.join(root, 'result'),
                                      verbose=False, seed=1)
        torch.manual_seed(3)
        t = ASRTester(config, paras)
        t.load_data()
        t.set_model()
        t.decode_group = 2                                          # three launches: 2 + 2 + 1
        return t
    t = tester(decode_length_bonus=0.5, decode_coverage_weight=0.2, decode_coverage_threshold=0.4, decode_end_margin=1.0)
    assert t.decode_file == 'decode_beam_3_len_0.25_lm0.5_lb0.5_cov0.2_end1.0'
    said = []
    t.verbose = said.append
    got = t.exec()
    assert 'beam search, beam size 3' in said[0] and 'length bonus 0.5' in said[0]
    xs, x_lens = [], []
    for x, _ in t.test_set:
        x, l = prepare_x(x, t.device)
        xs.append(x[:, :l[0]])
        x_lens.append(l)
    nbest = t.asr_model.decode_nbest(xs, x_lens, t.lm, t.mapper, 0.5, 3, length_bonus=0.5, coverage_weight=0.2,
                                     coverage_threshold=0.4, end_margin=1.0)
    assert got == [n[0][0] for n in nbest] and len(got) == 5 and all(isinstance(s, str) for s in got)
    assert t.asr_model.last_beam_steps.shape == (5,)
    # no new key: today's name and today's transcripts
    t0 = tester()
    assert t0.decode_file == 'decode_beam_3_len_0.25_lm0.5' and t0.decode_term_args == {}
    t0.lm = t.lm
    t0.verbose = said.append
    plain = t0.exec()
    assert 'length bonus' not in said[-2]
    assert plain == t0.asr_model.decode_many(xs, x_lens, t0.lm, t0.mapper, 0.5, beam_size=3) and len(plain) == 5
