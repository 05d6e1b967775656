"""Beam-search decoding on the GPU: ASR.decode / decode_many / decode_nbest with beam_size (ssasr_decode_beam) and
trainer.ASRTester with asr.decode_beam_size, against the float64 CPU beam search of tests/decode_checker.py, written
from the semantics of include/ssasr.h (it shares nothing with the library's host code).

Tolerances.  A step's score row is held to SCORE_ATOL = 5e-5 (test_gpu_decode); a hypothesis' score is a sum of at
most `steps` such entries, hence 5e-5 * steps.  The checker records, per step, the gap between the last kept and
the first dropped candidate and the smallest gap between adjacent kept candidates, and at the end the smallest
gap between adjacent emitted hypotheses; a (K, case) pair is compared only when the smallest of all of them is
>= MIN_GAP = 1e-3 (the rule of the greedy fixtures), so an error inside the bound cannot reorder anything and
the N-best lists must be EQUAL.  Pairs below the gap are not in the list; the test asserts how many are."""
import os
import shutil
import types

import numpy as np
import pytest
import torch

import decode_checker as dc
import test_gpu_decode as tgd
from conftest import GOLDEN
from test_host_cpu import make_corpus

pytestmark = pytest.mark.gpu

SCORE_ATOL = tgd.SCORE_ATOL
MIN_GAP = 1e-3
DEV = tgd.DEV
Mapper = tgd.Mapper
EOS = 1
STEPS = 24
BEAMS = (2, 3, 5)
SMALL = sorted(n for n in tgd.CASES if 'small' in n)
FULL = sorted(n for n in tgd.CASES if 'full' in n)
FULL_CASE = 'decode_full_s6'
# (fixture, frames of its x that are decoded, index of the LM weight): the small fixtures whole (40 frames) and
# truncated, one full-dims fixture whole (160 frames).  In float64 15 of these 30 (K, case) pairs keep the gap.
PAIR_CASES = [(n, f, k) for n in SMALL for f in (40, 24) for k in (0, 1)] + [(FULL_CASE, 160, 0), (FULL_CASE, 160, 1)]


def beam_reference(m, lm_weight, K, S):
    """The plain beam search over the float64 model m.  -> (hyps, min_gap): hyps = [(chars, score, step it ended at,
    capped)] in output order."""
    r = dc.beam_search(m, K, S, lm_weight)
    return [h[:4] for h in r['hyps']], r['gap']


_refs = {}


def reference(golden, name, frames, k, K):
    key = (name, frames, k, K)
    if key not in _refs:
        _refs[key] = beam_reference(dc.model(golden, name, frames), float(golden(name)['lm_weights'][k]), K, STEPS)
    return _refs[key]


def beam_arrays(asr):
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in asr.last_beam]


def text_of(chars):
    return ''.join(Mapper.chars[c] for c in chars)


@pytest.mark.parametrize('k', [0, 1])
@pytest.mark.parametrize('name', SMALL + FULL)
def test_beam_size_one_is_greedy_decoding(golden, name, k):
    fx = golden(name)
    asr, lm = tgd.models(fx)
    x = torch.from_numpy(fx['x']).to(DEV)
    w = float(fx['lm_weights'][k])
    plain_text = asr.decode(x, [x.shape[1]], lm, Mapper(), w)
    plain = tgd.decoded(asr)
    asr.last_decode = None
    assert asr.decode(x, [x.shape[1]], lm, Mapper(), w, beam_size=1) == plain_text
    again = tgd.decoded(asr)
    for a, b in zip(plain, again):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    nbest = asr.decode_nbest([x], [[x.shape[1]]], lm, Mapper(), w, 1)
    assert len(nbest) == 1 and len(nbest[0]) == 1 and nbest[0][0][0] == plain_text
    chars, n_chars, scores, _ = plain
    steps = min(int(n_chars[0]) + 1, scores.shape[1])
    want = float(sum(np.float64(scores[0, s, chars[0, s]]) for s in range(steps)))
    print('%s lm_weight %.1f: %d steps, score %.6f, sum of the chosen entries %.6f' % (name, w, steps, nbest[0][0][1], want))
    assert abs(nbest[0][0][1] - want) <= SCORE_ATOL * steps


@pytest.mark.parametrize('k', [0, 1, None])
@pytest.mark.parametrize('name', SMALL)
def test_the_beam_kernel_at_width_one_is_the_greedy_kernel(golden, name, k):
    """ssasr_decode_beam itself at K = 1 (ASR.decode(beam_size=1) never reaches it) against ssasr_decode_greedy on
    the same encoded input, with each LM weight of the fixture and without an LM.  Every greedy decision of these
    fixtures has a gap >= MIN_GAP, so the two kernels' different softmax summation orders cannot flip a character."""
    from ss_asr_amd import ops
    fx = golden(name)
    asr, lm = tgd.models(fx)
    x = torch.from_numpy(fx['x']).to(DEV)
    with torch.no_grad():
        feat, enc_lens = asr._encode_packed([x], [[x.shape[1]]])
    assert feat.shape[1] == 5
    args = (feat, enc_lens, asr._decoder_params(), (asr.attention.psi.weight, asr.attention.psi.bias),
            None if k is None else lm, 0.5 if k is None else float(fx['lm_weights'][k]), EOS, STEPS)
    g_chars, g_n, g_scores, _ = [None if t is None else t.cpu().numpy() for t in ops.decode_greedy(*args)]
    chars, n_chars, hyp_scores, n_hyps = [t.cpu().numpy() for t in ops.decode_beam(*args, 1)]
    n = int(g_n[0])
    steps = min(n + 1, STEPS)
    want = float(sum(np.float64(g_scores[0, s, g_chars[0, s]]) for s in range(steps)))
    print('%s lm %s: %d characters, %d steps, beam score %.6f, sum of greedy\'s chosen entries %.6f' % (
        name, k, n, steps, float(hyp_scores[0, 0]), want))
    assert chars.shape == (1, 1, STEPS) and int(n_hyps[0]) == 1
    assert int(n_chars[0, 0]) == n
    assert np.array_equal(chars[0, 0, :n], g_chars[0, :n]) and not chars[0, 0, n:].any()
    assert abs(float(hyp_scores[0, 0]) - want) <= SCORE_ATOL * steps


def test_beam_search_matches_the_float64_checker(golden):
    pairs = differs = capped = staggered = full = 0
    for name, frames, k in PAIR_CASES:
        fx = golden(name)
        asr, lm = tgd.models(fx)
        w = float(fx['lm_weights'][k])
        x = torch.from_numpy(fx['x'][:, :frames]).to(DEV)
        greedy = asr.decode(x, [frames], lm, Mapper(), w, max_decoding_steps=STEPS)
        for K in BEAMS:
            hyps, gap = reference(golden, name, frames, k, K)
            if gap < MIN_GAP:
                print('%s frames %d lm_weight %.1f K %d: smallest gap %.2e, not compared' % (name, frames, w, K, gap))
                continue
            nbest = asr.decode_nbest([x], [[frames]], lm, Mapper(), w, K, max_decoding_steps=STEPS)[0]
            chars, n_chars, scores, n_hyps = beam_arrays(asr)
            assert asr.decode(x, [frames], lm, Mapper(), w, max_decoding_steps=STEPS, beam_size=K) == nbest[0][0]
            err = max(abs(float(scores[0, i]) - h[1]) / (min(h[2] + 1, STEPS)) for i, h in enumerate(hyps[:int(n_hyps[0])]))
            print('%s frames %d lm_weight %.1f K %d: smallest gap %.2e, %d hypotheses, ended at %s, max |score error| '
                  'per step %.2e' % (name, frames, w, K, gap, len(hyps), [h[2] for h in hyps], err))
            assert int(n_hyps[0]) == len(hyps) == len(nbest) <= K
            for i, (ref_chars, ref_score, ended, was_capped) in enumerate(hyps):
                n = int(n_chars[0, i])
                assert n == len(ref_chars) and np.array_equal(chars[0, i, :n], ref_chars), (name, frames, k, K, i)
                assert not chars[0, i, n:].any()
                assert nbest[i][0] == text_of(ref_chars) and nbest[i][1] == float(scores[0, i])
                assert abs(float(scores[0, i]) - ref_score) <= SCORE_ATOL * min(ended + 1, STEPS)
            rest = slice(len(hyps), None)
            assert not chars[0, rest].any() and not n_chars[0, rest].any() and not scores[0, rest].any()
            pairs += 1
            full += name == FULL_CASE
            differs += nbest[0][0] != greedy
            capped += any(h[3] for h in hyps)
            staggered += len({h[2] for h in hyps if not h[3]}) > 1
    print('%d pairs compared: best differs from greedy in %d, a capped hypothesis in %d, <EOS> at different steps in %d'
          % (pairs, differs, capped, staggered))
    assert pairs >= 6 and differs >= 1 and capped >= 1 and staggered >= 1 and full >= 1


def test_a_group_decodes_every_utterance_as_it_decodes_alone(golden):
    fx = golden(SMALL[0])
    asr, lm = tgd.models(fx)
    x = torch.from_numpy(fx['x']).to(DEV)
    other = torch.from_numpy(golden(SMALL[1])['x']).to(DEV)
    both = torch.cat([x, other, x, other], 1)
    xs = [both[:, :f] for f in (160, 72, 40, 25, 9)]                # T' = 20, 9, 5, 3, 1
    lens = [[t.shape[1]] for t in xs]
    assert [l[0] // 8 for l in lens] == [20, 9, 5, 3, 1]
    texts = asr.decode_many(xs, lens, lm, Mapper(), 0.5, max_decoding_steps=STEPS, beam_size=3)
    group = beam_arrays(asr)
    assert group[0].shape == (5, 3, STEPS) and group[3].shape == (5,)
    for i, (t, l) in enumerate(zip(xs, lens)):
        assert asr.decode(t, l, lm, Mapper(), 0.5, max_decoding_steps=STEPS, beam_size=3) == texts[i]
        alone = beam_arrays(asr)
        for a, b in zip(alone, group):
            assert np.array_equal(a[0], b[i]), i
        nh = int(group[3][i])
        assert 1 <= nh <= 3
        assert not group[0][i, nh:].any() and not group[1][i, nh:].any() and not group[2][i, nh:].any()
        for j in range(nh):
            assert not group[0][i, j, int(group[1][i, j]):].any()


def test_beam_limits(golden):
    from ss_asr_amd import _lib, ops
    fx = golden(SMALL[0])
    asr, lm = tgd.models(fx)
    x = torch.from_numpy(fx['x']).to(DEV)
    for K in (20, 32):
        nbest = asr.decode_nbest([x], [[x.shape[1]]], lm, Mapper(), 0.5, K, max_decoding_steps=STEPS)[0]
        chars, n_chars, scores, n_hyps = beam_arrays(asr)
        nh = int(n_hyps[0])
        assert 1 <= nh <= K and len(nbest) == nh and chars.shape == (1, K, STEPS)
        assert np.all(np.diff(scores[0, :nh]) <= 0) and np.isfinite(scores[0, :nh]).all()
        assert (n_chars[0, :nh] >= 0).all() and (n_chars[0, :nh] <= STEPS).all()
        assert not scores[0, nh:].any() and not chars[0, nh:].any()
        assert len({tuple(chars[0, i, :n_chars[0, i]]) + (int(n_chars[0, i]) == STEPS,) for i in range(nh)}) == nh
    # outside 1 .. 32: an argument error before any launch
    with torch.no_grad():
        feat, enc_lens = asr._encode_packed([x], [[x.shape[1]]])
    args = (feat, enc_lens, asr._decoder_params(), (asr.attention.psi.weight, asr.attention.psi.bias), lm, 0.5, EOS, STEPS)
    lib = _lib.load()
    N, T, E = feat.shape
    A, D = asr.attention.phi.weight.shape
    sizes = (T, E, A, D, 50, lm.hidden_size, STEPS)
    for K in (0, 33):
        assert lib.ssasr_decode_beam_ws_bytes(N, K, *sizes) == 0
        with pytest.raises(RuntimeError, match='invalid argument'):
            ops.decode_beam(*args, K)
        with pytest.raises(ValueError, match='beam_size'):
            asr.decode_nbest([x], [[x.shape[1]]], lm, Mapper(), 0.5, K)
    # the entry itself refuses K = 33 and K = 0 in a struct that is valid for K = 3, and writes nothing
    import ctypes
    d, outs, keep = ops.beam_struct(*args, 3)
    for t in outs:
        t.fill_(7)
    for K in (33, 0):
        d.K = K
        assert lib.ssasr_decode_beam(ctypes.byref(d), ops._stream()) == -1            # SSASR_EARG
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in outs)
    # a workspace one float short of ssasr_decode_beam_ws_bytes is refused, that size is taken
    need = int(lib.ssasr_decode_beam_ws_bytes(N, 3, *sizes))
    assert need > 0 and need % 16 == 0 and d.ws_bytes == need
    with pytest.raises(RuntimeError, match='invalid argument'):
        ops.decode_beam(*args, 3, ws=torch.empty(need // 4 - 1, device=DEV))
    chars = ops.decode_beam(*args, 3, ws=torch.empty(need // 4, device=DEV))[0]
    torch.cuda.synchronize()
    assert chars.shape == (1, 3, STEPS)


def test_asr_tester_with_a_beam(tmp_path):
    from ss_asr_amd.ASRDataset import prepare_x
    from ss_asr_amd.trainer import ASRTester
    fx = np.load(os.path.join(GOLDEN, 'dataset_ref.npz'), allow_pickle=False)
    dims = [int(v) for v in fx['cpt_dims']]
    root = str(tmp_path)
    index, lens = make_corpus(root, n=5, t_max=40, feat=dims[4], seed=5)
    os.makedirs(os.path.join(root, 'result', 'dec'))
    shutil.copy(os.path.join(GOLDEN, 'ref_small_asr.cpt'), os.path.join(root, 'result', 'dec', 'asr.cpt'))

    def tester(beam):
        config = {'asr': {'mdl': {'encoder_state_size': dims[1], 'decoder_state_size': dims[2], 'mlp_out_size': dims[3],
                                  'feature_dim': dims[4], 'tf_rate': 1.0},
                          'test_index': index, 'decode_lm_weight': 0.5, 'decode_beam_size': beam, 'decode_jobs': 1,
                          'max_decode_step_ratio': 0.25, 'loader_jobs': 0},
                  'char_lm': {'mdl': {'hidden_size': 16}}}
        paras = types.SimpleNamespace(name='dec', logdir=os.path.join(root, 'runs'), ckpdir=os.path.join(root, 'result'),
                                      verbose=False, seed=1)
        torch.manual_seed(3)
        t = ASRTester(config, paras)
        t.load_data()
        t.set_model()
        t.decode_group = 2                                          # three launches: 2 + 2 + 1
        return t
    t3 = tester(3)
    assert t3.decode_file == 'decode_beam_3_len_0.25_lm0.5'
    said = []
    t3.verbose = said.append
    got = t3.exec()
    assert said[0].startswith('Start decoding') and 'beam search, beam size 3' in said[0]
    xs, x_lens = [], []
    for x, _ in t3.test_set:
        x, l = prepare_x(x, t3.device)
        xs.append(x[:, :l[0]])
        x_lens.append(l)
    assert [l[0] for l in x_lens] == lens
    assert got == t3.asr_model.decode_many(xs, x_lens, t3.lm, t3.mapper, 0.5, beam_size=3) and len(got) == 5
    assert all(isinstance(s, str) for s in got)
    # beam size 1: what the tester gave before it read the key
    t1 = tester(1)
    t1.lm = t3.lm                                                   # the same freshly initialised LM
    t1.verbose = said.append
    plain = t1.exec()
    assert said[-2].startswith('Start decoding') and 'beam search' not in said[-2]
    assert plain == t1.asr_model.decode_many(xs, x_lens, t1.lm, t1.mapper, 0.5)
    t1.decode_beam_size = 33
    with pytest.raises(ValueError, match='decode_beam_size'):
        t1.exec()
