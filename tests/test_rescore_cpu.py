"""N-best rescoring without a GPU: postprocess.rescore_reference (the float64 restatement that ssasr_rescore is defined
against) against a float64 teacher-forced pass of the oracle model (tests/decode_checker.py's Model, OracleASR and the
float64 GRU), the identity that ties it to the decoders (att_weight 1 with lm_weight w reproduces the beam checker's
score of every text it returns), hand-built cases, the argument checks of the new entries, which return before any HIP
call, and ASRTester's validation of asr.decode_rescore.  synthetic_case builds the seeded inputs that
tests/test_gpu_rescore.py runs the kernel on; `python tests/test_rescore_cpu.py` prints their float32 NOISE."""
import ctypes
import math

import numpy as np
import pytest
import torch

import decode_checker as dc
from ss_asr_amd.postprocess import rescore_reference

EOS = dc.EOS
SMALL = 'decode_small_s4'
MIN_GAP = 1e-3
MAX_DRAWS = 8
# (G, K, U, V, n_hyps): one step of two classes; an odd shape with a short and an empty list; the widest list, whose
# 2 K U terms go to the workspace; more utterances than rows per utterance
SHAPES = [(1, 1, 1, 2, None), (3, 4, 9, 31, [4, 2, 0]), (2, 32, 70, 64, None), (33, 2, 5, 50, None)]
WEIGHTS = dict(att_weight=0.7, lm_weight=0.3, first_weight=0.5, length_bonus=0.1)


def small_name():
    import test_gpu_decode as tgd
    names = [n for n in tgd.CASES if 'small' in n]
    return SMALL if SMALL in names else names[0]


def teacher_forced(m, texts, ended):
    """The float64 model's teacher-forced pass over `texts` (lists of ids; ended[i]: <EOS> follows text i) ->
    (speller rows [R, U, V], lm rows [R, U, V], label rows [R, U + 1]): log_softmax rows serve as logits."""
    U = max(len(t) + int(e) for t, e in zip(texts, ended))
    R = len(texts)
    z, zl = np.zeros((R, max(U, 1), m.V)), np.zeros((R, max(U, 1), m.V))
    rows = np.zeros((R, max(U, 1) + 1), dtype=np.int64)
    for r, (text, e) in enumerate(zip(texts, ended)):
        labels = list(text) + ([EOS] if e else [])
        st, last = m.start(), 0
        for t, lab in enumerate(labels):
            row, lm_row, _, st = m.step(st, [last])
            z[r, t], zl[r, t], rows[r, t + 1], last = row[0], lm_row[0], lab, lab
    return z, zl, rows


@pytest.mark.parametrize('with_lm', [False, True])
@pytest.mark.parametrize('frames', [8, 24, 40])
def test_the_restatement_equals_the_oracle_models_teacher_forced_pass(golden, frames, with_lm):
    m = dc.model(golden, small_name(), frames)
    assert m.T == frames // 8
    rng = np.random.default_rng(frames)
    texts = [rng.integers(2, m.V, size=n).tolist() for n in (4, 0, 7)]
    z, zl, rows = teacher_forced(m, texts, [True] * 3)
    w = float(np.float32(0.4))               # the entry takes its weights as floats
    order, total, parts = rescore_reference(z, zl if with_lm else None, rows, [3], [[0.0] * 3], [[len(t) for t in texts]],
                                            16, att_weight=1.0, lm_weight=w if with_lm else 0.0)
    for rank, k in enumerate(order[0]):
        att = dc.forced(m, texts[k], True, 0.0, None)[0]
        assert abs(parts[0][rank][0] - att) < 1e-12
        if with_lm:
            both = dc.forced(m, texts[k], True, 0.0, w)[0]
            assert abs(parts[0][rank][1] - (both - att) / w) < 1e-12 and abs(total[0][rank] - both) < 1e-12
        else:
            assert parts[0][rank][1] == 0.0 and abs(total[0][rank] - att) < 1e-12
    assert [float(np.float32(t)) for t in total[0]] == sorted((float(np.float32(t)) for t in total[0]), reverse=True)


@pytest.mark.parametrize('k', [0, 1])
def test_att_weight_one_with_the_lm_weight_gives_the_beam_checkers_score(golden, k):
    """Every text the float64 beam search returns: its rescoring total at att_weight 1, lm_weight w is the search's own
    score of it, <EOS>'s term included exactly when <EOS> ended the hypothesis (a capped one gets no <EOS> label)."""
    name = small_name()
    m = dc.model(golden, name, 40)
    w = float(np.float32(golden(name)['lm_weights'][k]))      # the entry takes its weights as floats
    seen = set()
    for K, S in ((3, 24), (5, 6), (4, 2)):
        hyps = dc.beam_search(m, K, S, w)['hyps']
        texts, ended = [h[0] for h in hyps], [not h[3] for h in hyps]
        seen |= set(ended)
        z, zl, rows = teacher_forced(m, texts, ended)
        order, total, _ = rescore_reference(z, zl, rows, [len(texts)], [[0.0] * len(texts)],
                                            [[len(t) for t in texts]], S, att_weight=1.0, lm_weight=w)
        for rank, slot in enumerate(order[0]):
            assert abs(total[0][rank] - hyps[slot][1]) < 1e-12, (K, S, slot)
        # the search emits best first: where its scores differ the rescoring keeps its order
        assert all(order[0][i] < order[0][i + 1] or total[0][i] > total[0][i + 1] for i in range(len(texts) - 1))
    assert seen == {True, False}, 'both an ended and a capped hypothesis are covered'


def hand(first, n_hyps, labels, n_chars=None, **weights):
    """One group over uniform two-class logits: every labelled step contributes log(1/2)."""
    K, U = len(labels), max(len(l) for l in labels)
    rows = np.zeros((K, U + 1), dtype=np.int64)
    for k, l in enumerate(labels):
        rows[k, 1:1 + len(l)] = l
    n_chars = n_chars or [[max(len(l) - 1, 0) for l in labels]]
    return rescore_reference(np.zeros((K, U, 2)), None, rows, [n_hyps], [first], n_chars, U, **weights)


def test_hand_built_cases():
    half = math.log(0.5)
    # two identical rows keep slot order, the shorter row ranks first
    order, total, parts = hand([0.0, 0.0, 0.0], 3, [[1, 1], [1, 1], [1]])
    assert order == [[2, 0, 1]] and total == [[half, 2 * half, 2 * half]] and parts[0][1] == [2 * half, 0.0, 0.0]
    # n_hyps 0: nothing ranked; n_hyps > K is clamped
    assert hand([1.0, 2.0], 0, [[1], [1]]) == ([[-1, -1]], [[0.0, 0.0]], [[[0.0] * 3] * 2])
    assert hand([1.0, 2.0], 7, [[1], [1]])[0] == [[0, 1]]
    assert hand([1.0, 2.0], 1, [[1], [1]])[0] == [[0, -1]]
    # a length-0 text: only <EOS>'s term remains, and the length bonus adds nothing
    order, total, _ = hand([0.0], 1, [[1]], length_bonus=2.0)
    assert order == [[0]] and total == [[half]]
    order, total, _ = hand([0.0], 1, [[1, 1, 1]], length_bonus=2.0)
    assert total == [[3 * half + 4.0]]
    # first = -inf: ignored at first_weight 0, last at first_weight > 0
    order, total, parts = hand([-math.inf, 0.0], 2, [[1], [1, 1]])
    assert order == [[0, 1]] and total == [[half, 2 * half]] and parts[0][0][2] == -math.inf
    order, total, _ = hand([-math.inf, 0.0], 2, [[1], [1, 1]], first_weight=0.5)
    assert order == [[1, 0]] and total == [[2 * half, -math.inf]]
    # a NaN first score: ignored at weight 0; at a positive weight the NaN total ranks as -inf, in slot order
    assert hand([math.nan, 0.0], 2, [[1], [1, 1]])[0] == [[0, 1]]
    order, total, _ = hand([math.nan, 0.0, -math.inf], 3, [[1], [1, 1], [1]], first_weight=1.0)
    assert order == [[1, 0, 2]] and total[0][0] == 2 * half and math.isnan(total[0][1]) and total[0][2] == -math.inf
    # att_weight 0 leaves the attention term out of the total, not out of parts
    order, total, parts = hand([3.0, 4.0], 2, [[1], [1]], att_weight=0.0, first_weight=1.0)
    assert order == [[1, 0]] and total == [[4.0, 3.0]] and parts[0][0] == [half, 0.0, 4.0]
    # an id that names no class and a column past the row are unlabelled
    assert hand([0.0], 1, [[1, 2, -1]])[1] == [[half]]


def synthetic_case(G, K, U, V, n_hyps=None, lm=False, seed=0):
    """Seeded inputs of one kernel case, redrawn until the smallest gap between adjacent float64 totals of a list is
    >= MIN_GAP (an error inside the bound then cannot reorder anything) -> (dict of numpy arrays, the float64
    reference's (order, total, parts), draws taken)."""
    M = min(K + 1, 33)
    R = G * M
    for draw in range(MAX_DRAWS):
        rng = np.random.default_rng([seed, G, K, U, V, draw])
        c = dict(G=G, K=K, U=U, V=V, M=M, steps=U)
        c['logits'] = (4.0 * rng.standard_normal((R, U, V))).astype(np.float32)
        c['lm_logits'] = (4.0 * rng.standard_normal((R, U, V))).astype(np.float32) if lm else None
        rows = np.zeros((R, U + 2), dtype=np.int32)
        lens = rng.integers(0, U, size=(G, K))
        for g in range(G):
            for k in range(K):
                n = int(lens[g, k])
                rows[g * M + k, 1:1 + n] = rng.integers(1, V, size=n)
                rows[g * M + k, 1 + n] = EOS
        c['rows'], c['n_chars'] = rows, lens.astype(np.int32)
        c['chars'] = rng.integers(1, V, size=(G, K, U)).astype(np.int32)
        c['first'] = (5.0 * rng.standard_normal((G, K))).astype(np.float32)
        c['n_hyps'] = np.asarray([K] * G if n_hyps is None else n_hyps, dtype=np.int32)
        weights = dict(WEIGHTS, lm_weight=WEIGHTS['lm_weight'] if lm else 0.0)
        ref = rescore_reference(c['logits'], c['lm_logits'], rows, c['n_hyps'], c['first'], c['n_chars'], U, **weights)
        gaps = [a - b for g in range(G) for a, b in zip(ref[1][g], ref[1][g][1:min(max(int(c['n_hyps'][g]), 0), K)])]
        if not gaps or min(gaps) >= MIN_GAP:
            return c, ref, draw + 1
    raise AssertionError('no draw of %r kept the gap' % ((G, K, U, V),))


def noise_of(c, ref, lm):
    """max |float32 checker - float64 checker| over the totals and parts of a case."""
    weights = dict(WEIGHTS, lm_weight=WEIGHTS['lm_weight'] if lm else 0.0)
    o32, t32, p32 = rescore_reference(c['logits'], c['lm_logits'], c['rows'], c['n_hyps'], c['first'], c['n_chars'],
                                      c['steps'], dtype=np.float32, **weights)
    worst = 0.0
    for g in range(c['G']):
        for rank, k in enumerate(ref[0][g]):
            if k < 0:
                continue
            j = o32[g].index(k)
            worst = max([worst, abs(t32[g][j] - ref[1][g][rank])] + [abs(a - b) for a, b in zip(p32[g][j], ref[2][g][rank])])
    return worst


@pytest.mark.parametrize('lm', [False, True])
def test_the_synthetic_cases_keep_the_gap_within_a_few_draws(lm):
    for G, K, U, V, n_hyps in SHAPES:
        c, ref, draws = synthetic_case(G, K, U, V, n_hyps, lm)
        assert draws <= 4, (G, K, U, V, draws)
        assert c['logits'].shape == (G * c['M'], U, V) and len(ref[0]) == G and len(ref[0][0]) == K


def _lib():
    from ss_asr_amd import _lib
    return _lib, _lib.load()


def test_the_new_entries_are_bound_and_the_abi_version_stays():
    from test_host_cpu import header_prototypes
    _lib_mod, lib = _lib()
    protos, _ = header_prototypes()
    for name in ('ssasr_rescore', 'ssasr_rescore_ws_bytes'):
        assert name in protos and name in _lib_mod.SIGNATURES and hasattr(lib, name)
    assert lib.ssasr_abi_version() == 16 == _lib_mod.ABI_VERSION
    # LDS holds 2 K U <= 4096 terms; past that a slice of 2 K U doubles per utterance
    assert lib.ssasr_rescore_ws_bytes(5, 32, 64) == 0 and lib.ssasr_rescore_ws_bytes(5, 32, 65) == 5 * 2 * 32 * 65 * 8
    assert lib.ssasr_rescore_ws_bytes(1, 8, 101) == 0
    for G, K, U in ((1, 0, 4), (1, 33, 4), (1, 4, 0), (-1, 4, 4)):
        assert lib.ssasr_rescore_ws_bytes(G, K, U) < 0


def test_the_entry_rejects_bad_arguments_before_any_hip_call():
    _, lib = _lib()
    buf = (ctypes.c_double * 16384)()
    base = ctypes.addressof(buf)
    p = ctypes.c_void_p(base)
    nan, inf = float('nan'), float('inf')

    def call(logits=p, lm=None, lm_row=5, lm_step=5, y=p, y_ld=5, y_cols=5, n_hyps=p, first=p, chars=p, n_chars=p, G=2,
             M=4, K=3, U=4, V=5, steps=6, aw=1.0, lw=0.0, fw=0.0, lb=0.0, ws=None, ws_bytes=0, order=p, total=p, parts=p,
             chars_out=p, n_chars_out=p, n_hyps_out=p):
        return lib.ssasr_rescore(logits, lm, lm_row, lm_step, y, y_ld, y_cols, n_hyps, first, chars, n_chars, G, M, K, U,
                                 V, steps, aw, lw, fw, lb, ws, ws_bytes, order, total, parts, chars_out, n_chars_out,
                                 n_hyps_out, None)

    assert call(K=0) < 0 and call(K=33, M=33) < 0 and call(M=2) < 0 and call(M=34, K=32) < 0
    assert call(G=-1) < 0 and call(G=20000) < 0                  # G * M > 65535
    assert call(U=0) < 0 and call(V=0) < 0 and call(steps=0) < 0
    assert call(y_cols=4) < 0 and call(y_ld=4) < 0
    assert call(lm=p, lm_row=4) < 0 and call(lm=p, lm_step=4) < 0
    for name in ('aw', 'lw', 'fw', 'lb'):
        assert call(**{name: nan}) < 0 and call(**{name: inf}) < 0, name
    for name in ('logits', 'y', 'n_hyps', 'first', 'chars', 'n_chars', 'order', 'total', 'parts', 'chars_out',
                 'n_chars_out', 'n_hyps_out'):
        assert call(**{name: None}) < 0, name
    # the workspace is needed from 2 K U > 4096 on: missing, misaligned, short
    big = dict(K=32, M=33, U=70, y_ld=71, y_cols=71)
    need = lib.ssasr_rescore_ws_bytes(2, 32, 70)
    assert 0 < need <= ctypes.sizeof(buf)
    assert call(**big) < 0 and call(ws=ctypes.c_void_p(base + 4), ws_bytes=need, **big) < 0
    assert call(ws=p, ws_bytes=need - 1, **big) < 0
    assert call(G=0, logits=None, order=None) == 0             # legal, launches nothing


def test_ops_refuse_cpu_tensors():
    from ss_asr_amd import ops
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
    with pytest.raises(RuntimeError, match='GPU'):
        ops.rescore_launch(torch.zeros(2, 3, 4), None, i32(2, 4), i32(1), torch.zeros(1, 2), i32(1, 2, 3), i32(1, 2))
    with pytest.raises(RuntimeError, match='GPU'):
        ops.rescore(torch.zeros(1, 2, 4), i32(1), {}, (None, None), i32(1, 2, 3), i32(1, 2), i32(1), torch.zeros(1, 2), 1)
    assert ops.rescore_loop_rows(100) == 32 and ops.rescore_loop_rows(128) == 32
    assert ops.rescore_loop_rows(129) == 32 and ops.rescore_loop_rows(500) == 24 and ops.rescore_loop_rows(10 ** 5) == 1


def test_rescore_raises_on_a_missing_list_and_bad_weights():
    from ss_asr_amd.asr import ASR
    model = ASR(12, 8, 8, 8, 8, 1.0)
    with pytest.raises(ValueError, match='nothing decoded'):
        model.rescore(None)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
    model._keep_hyps(i32(1, 2, 3), i32(1, 2), i32(1), torch.zeros(1, 2), sampled=False)
    with pytest.raises(ValueError, match='nothing decoded'):          # no encoder output kept
        model.rescore(None)
    model.last_encoded_packed = (torch.zeros(1, 2, 16), i32(1))
    for kw in (dict(att_weight=float('nan')), dict(lm_weight=float('inf')), dict(first_weight=-float('inf')),
               dict(length_bonus=float('nan'))):
        with pytest.raises(ValueError, match='finite'):
            model.rescore(None, **kw)
    with pytest.raises(ValueError, match='all zero'):
        model.rescore(None, att_weight=0.0)
    assert model.last_rescore is None
    for kw in (dict(ctc_weight=1.5), dict(ctc_weight=-0.1), dict(ctc_weight='x'), dict(ctc_weight=True),
               dict(beam_size=0), dict(beam_size=33), dict(beam_size=2.0)):
        with pytest.raises(ValueError, match='ctc_weight|beam_size'):
            model.decode_two_pass([], [], None, None, 0.0, **kw)


def test_the_tester_validates_the_rescore_mapping():
    from ss_asr_amd.trainer import ASRTester
    ctc = {'decode_ctc_only': {'beam_size': 4}}
    assert ASRTester.rescore_args({}) is None and ASRTester.rescore_args({'decode_rescore': None}) is None
    assert ASRTester.rescore_args(dict(ctc, decode_rescore={})) == {'ctc_weight': 0.3, 'length_bonus': 0.0}
    assert ASRTester.rescore_args(dict(ctc, decode_rescore=True)) == {'ctc_weight': 0.3, 'length_bonus': 0.0}
    assert ASRTester.rescore_args(dict(ctc, decode_rescore={'ctc_weight': 0, 'length_bonus': 1})) == {
        'ctc_weight': 0, 'length_bonus': 1.0}
    with pytest.raises(ValueError, match='mapping'):
        ASRTester.rescore_args(dict(ctc, decode_rescore=4))
    with pytest.raises(ValueError, match='mapping'):
        ASRTester.rescore_args(dict(ctc, decode_rescore={'ctc_weight': 0.3, 'lm_weight': 0.1}))
    for bad in (1.5, -0.1, float('nan'), '0.3', True):
        with pytest.raises(ValueError, match='asr.decode_rescore.ctc_weight'):
            ASRTester.rescore_args(dict(ctc, decode_rescore={'ctc_weight': bad}))
    for bad in (float('inf'), 'x', False):
        with pytest.raises(ValueError, match='asr.decode_rescore.length_bonus'):
            ASRTester.rescore_args(dict(ctc, decode_rescore={'length_bonus': bad}))
    with pytest.raises(ValueError, match='decode_ctc_only'):
        ASRTester.rescore_args({'decode_rescore': {'ctc_weight': 0.3}})
    with pytest.raises(ValueError, match='beam_size >= 1'):
        ASRTester.rescore_args({'decode_ctc_only': {'beam_size': 0}, 'decode_rescore': {}})
    # the neighbouring keys are untouched by the new one
    assert ASRTester.ctc_only_beam(dict(ctc, decode_rescore={})) == 4 and ASRTester.mbr_args(dict(ctc, decode_rescore={})) is None


if __name__ == '__main__':
    for lm in (False, True):
        for G, K, U, V, n_hyps in SHAPES:
            c, ref, draws = synthetic_case(G, K, U, V, n_hyps, lm)
            print('G=%d K=%d U=%d V=%d lm=%s: %d draw(s), NOISE %.4g' % (G, K, U, V, lm, draws, noise_of(c, ref, lm)))
