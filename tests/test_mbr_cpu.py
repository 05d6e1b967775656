"""Minimum-Bayes-risk selection without a GPU: postprocess.mbr_reference (the float64 restatement that
ssasr_mbr_select is defined against) on a hand-worked set and on its edge cases, and the argument checks of the new
entry, which return before any HIP call."""
import ctypes
import math

import numpy as np
import pytest

from ss_asr_amd.postprocess import edit_ops, mbr_reference, score_sequences

SPACE = 9
A, B, C, D = 3, 4, 5, 6


def words(*ws):
    """token ids of the words joined by single spaces"""
    out = []
    for i, w in enumerate(ws):
        out += ([SPACE] if i else []) + list(w)
    return out


def test_a_hand_worked_set_where_map_and_mbr_differ():
    # three entries: the MAP entry `a b` stands alone, the two others agree with each other on more words
    hyps = [[words([A], [B]), words([A], [C], [D]), words([A], [C], [C])]]
    scores = [[math.log(0.4), math.log(0.3), math.log(0.3)]]
    best, risk, pair = mbr_reference(hyps, [3], scores, SPACE, unit='word')
    # word distances: (0, 1) = 2 (b -> c, + d), (0, 2) = 2, (1, 2) = 1; characters: 3, 3, 1
    assert pair[0] == [[[0, 0], [3, 2], [3, 2]], [[3, 2], [0, 0], [1, 1]], [[3, 2], [1, 1], [0, 0]]]
    want = [0.3 * 2 + 0.3 * 2, 0.4 * 2 + 0.3 * 1, 0.4 * 2 + 0.3 * 1]
    assert risk[0] == pytest.approx(want, rel=1e-7)          # the scores are taken as floats
    assert best == [1]                                       # the tie of entries 1 and 2 goes to the lower slot
    assert max(range(3), key=lambda k: scores[0][k]) == 0    # which the MAP choice is not
    # characters: the same shape of answer from the other column of pair
    best_c, risk_c, _ = mbr_reference(hyps, [3], scores, SPACE, unit='char')
    assert risk_c[0] == pytest.approx([0.3 * 3 + 0.3 * 3, 0.4 * 3 + 0.3, 0.4 * 3 + 0.3], rel=1e-7) and best_c == [1]
    # a sharper posterior gives the MAP entry back
    assert mbr_reference(hyps, [3], scores, SPACE, scale=1e4)[0] == [0]
    # the float32 rounding of scale and scores that the entry applies is part of the definition
    x = [float(np.float64(np.float32(0.3)) * np.float64(np.float32(s))) for s in scores[0]]
    lse = max(x) + math.log(sum(math.exp(v - max(x)) for v in x))
    p = [math.exp(v - lse) for v in x]
    assert mbr_reference(hyps, [3], scores, SPACE, scale=0.3)[1][0][0] == 0.0 + p[0] * 0.0 + p[1] * 2.0 + p[2] * 2.0


def random_set(rng, K, longest=12):
    return [[int(v) for v in rng.choice([0, 1, A, B, C, SPACE], size=int(rng.integers(0, longest + 1)))]
            for _ in range(K)]


def test_pair_is_symmetric_with_a_zero_diagonal_and_is_the_scorer_s_distance():
    rng = np.random.default_rng(0)
    hyps = [random_set(rng, K) for K in (1, 2, 5, 8)]
    padded = [rows + [[]] * (8 - len(rows)) for rows in hyps]
    n_hyps = [1, 2, 5, 8]
    scores = rng.normal(size=(4, 8)).tolist()
    best, risk, pair = mbr_reference(padded, n_hyps, scores, SPACE)
    for n, nh in enumerate(n_hyps):
        for k in range(8):
            for j in range(8):
                if k < nh and j < nh:
                    assert pair[n][k][j] == pair[n][j][k] and (k != j or pair[n][k][j] == [0, 0])
                    sk, sj = score_sequences(padded[n][k], SPACE), score_sequences(padded[n][j], SPACE)
                    assert pair[n][k][j] == [sum(edit_ops(sk[0], sj[0])), sum(edit_ops(sk[1], sj[1]))]
                else:
                    assert pair[n][k][j] == [-1, -1]
            assert (risk[n][k] == math.inf) == (k >= nh)
        assert 0 <= best[n] < nh and risk[n][best[n]] == min(risk[n])


def test_a_large_scale_returns_slot_zero_of_a_sorted_list():
    rng = np.random.default_rng(1)
    hyps = [random_set(rng, 6) for _ in range(8)]
    scores = [sorted(rng.normal(size=6).tolist(), reverse=True) for _ in range(8)]
    assert mbr_reference(hyps, [6] * 8, scores, SPACE, scale=1e4)[0] == [0] * 8


def test_the_uniform_posterior_ignores_the_scores():
    rng = np.random.default_rng(2)
    hyps = [random_set(rng, 5) for _ in range(6)]
    a = mbr_reference(hyps, [5] * 6, rng.normal(size=(6, 5)).tolist(), SPACE, posterior='uniform')
    b = mbr_reference(hyps, [5] * 6, None, SPACE, posterior='uniform')
    assert a == b
    for n in range(6):
        for k in range(5):
            assert a[1][n][k] == pytest.approx(sum(a[2][n][k][j][1] for j in range(5)) / 5, rel=1e-12)
    # scale 0 makes the softmax uniform too
    c = mbr_reference(hyps, [5] * 6, rng.normal(size=(6, 5)).tolist(), SPACE, scale=0.0)
    assert c[0] == a[0] and c[1] == a[1]


def test_identical_rows_outside_rows_and_the_empty_set():
    row = words([A, B], [C])
    best, risk, pair = mbr_reference([[row] * 4, [row, [A], [B], [C]], [row] * 4], [4, 2, 0], [[0.0] * 4] * 3, SPACE)
    assert best == [0, 0, -1]
    assert risk[0] == [0.0] * 4 and all(p == [0, 0] for r in pair[0] for p in r)
    assert risk[1][2:] == [math.inf] * 2 and risk[2] == [math.inf] * 4
    assert all(pair[1][k][j] == [-1, -1] for k in range(4) for j in range(4) if k >= 2 or j >= 2)
    assert all(p == [-1, -1] for r in pair[2] for p in r)
    # n_hyps past K is clamped, a negative one is an empty set
    assert mbr_reference([[row] * 2, [row] * 2], [5, -3], [[0.0] * 2] * 2, SPACE)[0] == [0, -1]


def test_non_finite_scores_follow_the_definition():
    hyps = [[words([A]), words([B]), words([B])]]
    # entry 0 has no weight: the risks are over entries 1 and 2 alone, and the two equal entries win
    best, risk, _ = mbr_reference(hyps, [3], [[-math.inf, -1.0, -1.0]], SPACE)
    assert best == [1] and risk[0] == [1.0, 0.0, 0.0]
    best, risk, _ = mbr_reference(hyps, [3], [[math.nan, -1.0, math.inf]], SPACE)
    assert best == [1] and risk[0] == [1.0, 0.0, 0.0]          # only entry 1 is finite
    # nothing finite: the uniform posterior
    best, risk, _ = mbr_reference(hyps, [3], [[-math.inf, math.nan, math.inf]], SPACE)
    assert best == [1] and risk[0] == pytest.approx([2 / 3, 1 / 3, 1 / 3], rel=1e-12)
    with pytest.raises(ValueError):
        mbr_reference(hyps, [3], [[0.0] * 3], SPACE, unit='phone')
    with pytest.raises(ValueError):
        mbr_reference(hyps, [3], [[0.0] * 3], SPACE, posterior='flat')
    for bad in (-1.0, math.nan, math.inf):
        with pytest.raises(ValueError):
            mbr_reference(hyps, [3], [[0.0] * 3], SPACE, scale=bad)


def test_mbr_select_argument_errors_are_negative_and_need_no_gpu():
    from ss_asr_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(chars=p, hyp_ld=8, n_chars=p, n_hyps=p, scores=p, N=1, K=2, Hmax=8, unit=1, posterior=0, scale=1.0,
             best=p, risk=p, pair=p):
        return lib.ssasr_mbr_select(chars, hyp_ld, n_chars, n_hyps, scores, N, K, Hmax, 2, SPACE, unit, posterior,
                                    scale, best, risk, pair, None)

    assert call(K=0) < 0 and call(K=33) < 0
    assert call(Hmax=1024, hyp_ld=1024, K=1) < 0 and call(Hmax=-1) < 0
    assert call(K=9, Hmax=911, hyp_ld=911) < 0                     # 9 * 911 = 8199
    assert call(K=1, Hmax=8193, hyp_ld=8193) < 0
    assert call(K=17, Hmax=482, hyp_ld=482) < 0                    # 8194, each factor inside its own limit
    assert call(hyp_ld=7) < 0
    assert call(unit=2) < 0 and call(unit=-1) < 0 and call(posterior=2) < 0 and call(posterior=-1) < 0
    assert call(scale=-1.0) < 0 and call(scale=math.nan) < 0 and call(scale=math.inf) < 0
    assert call(scores=None) < 0                                   # the softmax posterior needs them
    for name in ('chars', 'n_chars', 'n_hyps', 'best', 'risk', 'pair'):
        assert call(**{name: None}) < 0, name
    assert call(N=-1) < 0 and call(N=65536) < 0
    assert call(N=0) == 0                                          # legal, launches nothing


def test_the_limit_on_tokens_per_utterance_is_8192():
    from ss_asr_amd import _lib, ops
    lib = _lib.load()
    buf = (ctypes.c_int32 * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    # K * Hmax = 8193 is refused whatever else holds; no factorisation of 8193 = 3 * 2731 fits K <= 32 with
    # Hmax <= 1023, so the product check is reached through the nearest products above the limit
    for K, hmax in ((32, 257), (16, 513), (9, 911), (8, 1025)):
        assert K * hmax > 8192
        assert lib.ssasr_mbr_select(p, hmax, p, p, p, 1, K, hmax, 2, SPACE, 1, 0, 1.0, p, p, p, None) < 0
        assert not ops.mbr_fits(K, hmax)
    assert ops.mbr_fits(32, 256) and ops.mbr_fits(8, 1023) and ops.mbr_fits(1, 0) and not ops.mbr_fits(0, 4)
    assert not ops.mbr_fits(33, 1) and not ops.mbr_fits(1, 1024)


def test_the_new_entry_is_bound_and_the_abi_version_stays():
    from ss_asr_amd import _lib
    lib = _lib.load()
    assert 'ssasr_mbr_select' in _lib.SIGNATURES and lib.ssasr_mbr_select.restype is ctypes.c_int32
    assert lib.ssasr_abi_version() == 16 == _lib.ABI_VERSION
    header = open(_lib_header()).read()
    assert 'int ssasr_mbr_select(' in header and 'ssasr_mbr_select.  16:' in header.replace('\n * ', ' ')


def _lib_header():
    import os
    return os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'ssasr.h')


def test_asr_tester_validates_decode_mbr():
    from ss_asr_amd.trainer import ASRTester
    assert ASRTester.mbr_args({'decode_beam_size': 1}) is None
    assert ASRTester.mbr_args({'decode_beam_size': 4, 'decode_mbr': {}}) == {'unit': 'word', 'scale': 1.0}
    assert ASRTester.mbr_args({'decode_beam_size': 2, 'decode_mbr': {'unit': 'char', 'scale': 2}}) == \
        {'unit': 'char', 'scale': 2.0}
    for bad in ({'unit': 'phone'}, {'scale': -1}, {'scale': math.nan}, {'scale': True}, {'units': 'word'}, 'word'):
        with pytest.raises(ValueError):
            ASRTester.mbr_args({'decode_beam_size': 4, 'decode_mbr': bad})
    with pytest.raises(ValueError, match='decode_beam_size'):
        ASRTester.mbr_args({'decode_beam_size': 1, 'decode_mbr': {'unit': 'word'}})
