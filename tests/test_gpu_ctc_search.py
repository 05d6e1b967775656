"""CTC-only decoding on the GPU (ssasr_ctc_decode; ops.ctc_decode; ASR.decode_ctc; ASRTester with
asr.decode_ctc_only) against postprocess.ctc_prefix_beam_reference, the float64 restatement of include/ssasr.h.

Best path (K = 0): the text is comparisons only, so it must be EQUAL in every case, with no gap rule.
Prefix search (K >= 1): a case is compared when the checker's smallest kept / dropped gap over its frames is >=
MIN_GAP = 1e-3 (the project's rule); the kernel's list must then hold the checker's SET of texts, in non-increasing
order of the kernel's own scores, each score within BOUND of the checker's score of that text.  At most a quarter of
the enumerated cases may be skipped and no (T, V, K) cell entirely.
BOUND = 8 * NOISE, NOISE = max |score32 - score64| of the checker run in float32 (log-softmax included) against
float64 over the compared hypotheses -- the rule of test_gpu_ctc_decode.py.  Measured on the CPU by `python
tests/test_gpu_ctc_search.py` (measure_noise below): 5.09e-5 over the cells (at T = 160, K = 3), 2.12e-4 for the 4,096-frame row (its own
constant: a float32 sum of 4,096 terms).  BOUND = 4.08e-4; the worst kernel error measured on the MI355X is 6.55e-6
over the 519 of 544 compared cases (7.24e-6 for the best path, 5.74e-6 for the 4,096-frame row)."""
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
MIN_GAP = 1e-3
SEEDS = range(16)
CELLS = ([(T, 8, K) for T in (1, 3, 5) for K in (1, 2, 3, 5, 8, 16, 32)] +
         [(20, V, K) for V in (8, 40) for K in (1, 2, 3, 5, 8)] +
         [(160, 40, K) for K in (1, 2, 3)])
BEST_PATH_SHAPES = sorted({(T, V) for T, V, _ in CELLS}) + [(3, 2), (5, 65), (7, 1000)]
NOISE = 5.1e-5
BOUND = 8 * NOISE
T_LIMIT = 4096
NOISE_LIMIT = 2.2e-4
BOUND_LIMIT = 8 * NOISE_LIMIT
CANARY_I, CANARY_F = -77, 12345.0
PAD = 64                                                         # canary elements behind every output


def logits_of(T, V, seed):
    return (4.0 * np.random.default_rng([T, V, seed]).standard_normal((T, V))).astype(np.float32)


def limit_logits():
    """4,096 frames of a peaked head (one class 12 above the noise): the search at K = 1 has a clear winner per frame."""
    rng = np.random.default_rng(4096)
    z = rng.standard_normal((T_LIMIT, 8))
    z[np.arange(T_LIMIT), rng.integers(0, 8, T_LIMIT)] += 12.0
    return z.astype(np.float32)


def log_softmax(z, dtype=np.float64):
    z = z.astype(dtype)
    m = z.max(-1, keepdims=True)
    return z - (m + np.log(np.exp(z - m).sum(-1, keepdims=True, dtype=dtype)))


_refs = {}


def reference(key, z, K, blank=0):
    """(hyps, gap) of the checker on float64 log_softmax(z), computed once per key."""
    from ss_asr_amd.postprocess import ctc_prefix_beam_reference
    if (key, K, blank) not in _refs:
        _refs[(key, K, blank)] = ctc_prefix_beam_reference(log_softmax(z), K, blank)
    return _refs[(key, K, blank)]


def noise_of(z, K, blank=0):
    """max |score32 - score64| over the texts both runs of the checker hold (None: the case is not compared)."""
    from ss_asr_amd.postprocess import ctc_prefix_beam_reference
    hyps, gap = ctc_prefix_beam_reference(log_softmax(z), K, blank)
    if gap < MIN_GAP:
        return None
    lp32 = log_softmax(z, np.float32)
    assert lp32.dtype == np.float32
    hyps32 = dict(ctc_prefix_beam_reference(lp32, K, blank, dtype=np.float32)[0])
    return max(abs(hyps32[text] - score) for text, score in hyps if text in hyps32)


def measure_noise():
    worst = 0.0
    for T, V, K in [(T, V, 0) for T, V in BEST_PATH_SHAPES] + CELLS:
        cell = [n for n in (noise_of(logits_of(T, V, s), K) for s in SEEDS) if n is not None]
        worst = max([worst] + cell)
        print('T=%d V=%d K=%d: %d of %d compared, noise %.3g' % (T, V, K, len(cell), len(SEEDS), max(cell)), flush=True)
    print('NOISE over the cells: %.4g' % worst)
    print('NOISE of the %d-frame row: %.4g' % (T_LIMIT, noise_of(limit_logits(), 1)))


def run(z, frame_lens, K, blank=0):
    """ssasr_ctc_decode on z [B, T, V] through the C entry, every output followed by PAD canaries and pre-filled, so
    that an element the kernel leaves unwritten or writes past its end shows.  -> per row the list of (text, score)
    and the raw arrays."""
    from ss_asr_amd import _lib, ops
    lib = _lib.load()
    B, T, V = z.shape
    kr = max(K, 1)
    need = int(lib.ssasr_ctc_decode_ws_bytes(B, T, V, K))
    assert need > 0
    logits = torch.from_numpy(np.ascontiguousarray(z)).to(DEV)
    lens = torch.tensor(list(frame_lens), dtype=torch.int32, device=DEV)
    ws = torch.full((need // 4 + PAD,), CANARY_I, dtype=torch.int32, device=DEV)
    chars = torch.full((B * kr * T + PAD,), CANARY_I, dtype=torch.int32, device=DEV)
    n_chars = torch.full((B * kr + PAD,), CANARY_I, dtype=torch.int32, device=DEV)
    scores = torch.full((B * kr + PAD,), CANARY_F, dtype=torch.float32, device=DEV)
    n_hyps = torch.full((B + PAD,), CANARY_I, dtype=torch.int32, device=DEV)
    ops.check(lib.ssasr_ctc_decode(ops._p(logits), ops._p(lens), B, T, V, K, blank, ops._p(ws), need, ops._p(chars),
                                   ops._p(n_chars), ops._p(scores), ops._p(n_hyps), ops._stream()), 'ssasr_ctc_decode')
    torch.cuda.synchronize()
    ws, chars, n_chars, scores, n_hyps = [t.cpu().numpy() for t in (ws, chars, n_chars, scores, n_hyps)]
    for name, arr, n, canary in (('ws', ws, need // 4, CANARY_I), ('chars', chars, B * kr * T, CANARY_I),
                                 ('n_chars', n_chars, B * kr, CANARY_I), ('scores', scores, B * kr, CANARY_F),
                                 ('n_hyps', n_hyps, B, CANARY_I)):
        assert (arr[n:] == canary).all(), name + ': written past its end'
        if name != 'ws':
            assert not (arr[:n] == canary).any(), name + ': an element was left unwritten'
    chars, n_chars = chars[:B * kr * T].reshape(B, kr, T), n_chars[:B * kr].reshape(B, kr)
    scores, n_hyps = scores[:B * kr].reshape(B, kr), n_hyps[:B]
    out = []
    for b in range(B):
        assert 0 <= n_hyps[b] <= kr
        for k in range(kr):
            n = n_chars[b, k]
            assert 0 <= n <= T and (chars[b, k, n:] == 0).all()
            if k >= n_hyps[b]:
                assert n == 0 and scores[b, k] == -math.inf
        out.append([(tuple(int(c) for c in chars[b, k, :n_chars[b, k]]), float(scores[b, k])) for k in range(n_hyps[b])])
    return out, (chars, n_chars, scores, n_hyps)


def check_row(got, want, bound):
    """The kernel's list against the checker's: the same set of texts, the kernel's own order, each score within
    bound.  -> the worst score error."""
    assert len(got) == len(want) and {t for t, _ in got} == {t for t, _ in want} and len({t for t, _ in got}) == len(got)
    scores = [s for _, s in got]
    assert scores == sorted(scores, reverse=True)
    ref = dict(want)
    worst = max(abs(s - ref[t]) for t, s in got)
    assert worst <= bound, (worst, bound)
    return worst


def test_best_path_equals_the_checker_in_every_case():
    worst = 0.0
    for T, V in BEST_PATH_SHAPES:
        z = np.stack([logits_of(T, V, s) for s in SEEDS])
        if (T, V) == (3, 2):
            z = np.round(z)                                      # two classes, rounded: ties, decided for the lower index
        got, _ = run(z, [T] * len(SEEDS), 0)
        for s in SEEDS:
            want, _ = reference((T, V, s, (T, V) == (3, 2)), z[s], 0)
            path = z[s].argmax(1)                                # on the raw logits, as the kernel takes it
            keep = (path != 0) & np.r_[True, path[1:] != path[:-1]]
            assert len(got[s]) == 1 and got[s][0][0] == want[0][0] == tuple(int(c) for c in path[keep]), (T, V, s)
            worst = max(worst, abs(got[s][0][1] - want[0][1]))
    print('best path: worst |score - float64| %.3g (bound %.3g)' % (worst, BOUND))
    assert worst <= BOUND


def test_prefix_search_matches_the_checker_on_every_compared_case():
    compared, worst = {}, 0.0
    for T, V in sorted({(T, V) for T, V, _ in CELLS}):
        z = np.stack([logits_of(T, V, s) for s in SEEDS])
        for K in [k for t, v, k in CELLS if (t, v) == (T, V)]:
            got, _ = run(z, [T] * len(SEEDS), K)
            compared[(T, V, K)] = 0
            for s in SEEDS:
                want, gap = reference((T, V, s, False), z[s], K)
                if gap < MIN_GAP:
                    continue
                compared[(T, V, K)] += 1
                worst = max(worst, check_row(got[s], want, BOUND))
            if T == 1:
                assert all(len(g) == min(K, 8) for g in got)     # 7 extensions and the empty text: fewer than 16 or 32
    total = len(CELLS) * len(SEEDS)
    done = sum(compared.values())
    print('compared per cell (of %d): %s' % (len(SEEDS), compared))
    print('prefix search: %d of %d cases compared, worst |score - float64| %.3g (NOISE %.3g, bound %.3g)'
          % (done, total, worst, NOISE, BOUND))
    assert set(compared) == set(CELLS) and all(n > 0 for n in compared.values())
    assert total - done <= total // 4


def edge_rows():
    """[(name, logits [T', V], frame_len, blank)] at T' = 20, V = 8."""
    T, V = 20, 8
    rows = [('no frames', logits_of(T, V, 100), 0, 0), ('one frame', logits_of(T, V, 101), 1, 0),
            ('length past the rows', logits_of(T, V, 102), 25, 0), ('blank 3', logits_of(T, V, 103), 20, 3)]
    silent = logits_of(T, V, 104)
    silent[:, 0] = silent.max(1) + 6.0                          # every frame's argmax is the blank
    rows.append(('all blank', silent, 20, 0))
    for name, path in (('repeat with a blank between', [1, 1, 0, 1, 2]), ('repeat without', [1, 1, 1, 2, 2])):
        z = logits_of(T, V, 105)
        z[np.arange(5), path] = z[:5].max(1) + 9.0 + np.array([0.0, 0.31, 0.73, 1.2, 1.9], dtype=np.float32)   # unequal: no ties
        rows.append((name, z, 5, 0))
    return rows


@pytest.mark.parametrize('K', [0, 1, 3, 8])
def test_edges(K):
    rows = edge_rows()
    for blank in (0, 3):
        group = [r for r in rows if r[3] == blank]
        got, _ = run(np.stack([r[1] for r in group]), [r[2] for r in group], K, blank)
        for (name, z, n, _), mine in zip(group, got):
            want, gap = reference(name, z[:min(n, 20)], K, blank)
            assert K == 0 or gap >= MIN_GAP, (name, K, gap)      # chosen to be compared: none of them is skipped
            if K == 0:
                assert [t for t, _ in mine] == [t for t, _ in want] and abs(mine[0][1] - want[0][1]) <= BOUND, name
            else:
                check_row(mine, want, BOUND)
            if name == 'no frames':
                assert mine == [((), 0.0)]
            if name == 'all blank':
                assert mine[0][0] == ()
            if name == 'repeat with a blank between':
                assert mine[0][0] == (1, 1, 2)
            if name == 'repeat without':
                assert mine[0][0] == (1, 2)


@pytest.mark.parametrize('K', [0, 2, 8])
def test_an_utterance_decodes_in_a_group_as_it_decodes_alone(K):
    lens = [20, 9, 5, 3, 1]
    z = np.stack([logits_of(20, 8, 200 + i) for i in range(len(lens))])
    _, (chars, n_chars, scores, n_hyps) = run(z, lens, K)
    for i, n in enumerate(lens):
        _, (c1, n1, s1, h1) = run(z[i:i + 1, :n], [n], K)
        assert h1[0] == n_hyps[i] and np.array_equal(n1[0], n_chars[i])
        assert np.array_equal(s1[0].view(np.int32), scores[i].view(np.int32))       # bit-equal
        assert np.array_equal(c1[0], chars[i, :, :n]) and (chars[i, :, n:] == 0).all()


def test_the_frame_limit():
    from ss_asr_amd import ops
    z = limit_logits()
    want, gap = reference('limit', z, 1)
    assert gap >= MIN_GAP
    got, _ = run(z[None], [T_LIMIT], 1)
    err = check_row(got[0], want, BOUND_LIMIT)
    best, _ = run(z[None], [T_LIMIT], 0)
    assert best[0][0][0] == reference('limit', z, 0)[0][0][0]
    print('%d frames, K = 1: %d characters, |score - float64| %.3g (noise %.3g, bound %.3g)'
          % (T_LIMIT, len(got[0][0][0]), err, NOISE_LIMIT, BOUND_LIMIT))
    lens = torch.tensor([8], dtype=torch.int32, device=DEV)
    for shape, K in (((1, T_LIMIT + 1, 8), 1), ((1, T_LIMIT + 1, 8), 0), ((1, 8, 65), 1), ((1, 8, 1025), 0)):
        with pytest.raises(ValueError, match='no kernel'):
            ops.ctc_decode(torch.zeros(shape, device=DEV), lens, K)
    with pytest.raises(ValueError, match='beam_size'):
        ops.ctc_decode(torch.zeros(1, 8, 8, device=DEV), lens, 33)
    with pytest.raises(ValueError, match='blank'):
        ops.ctc_decode(torch.zeros(1, 8, 8, device=DEV), lens, 2, blank=8)
    # ops.ctc_decode is the entry: the same bits as the direct call
    zs = np.stack([logits_of(20, 8, s) for s in range(3)])
    out = ops.ctc_decode(torch.from_numpy(zs).to(DEV), torch.tensor([20, 7, 0], dtype=torch.int32, device=DEV), 5)
    _, raw = run(zs, [20, 7, 0], 5)
    for a, b in zip(out, raw):
        assert np.array_equal(a.cpu().numpy().view(np.int32), b.view(np.int32))


def test_decode_ctc_and_the_tester_key(tmp_path):
    import las_oracle as lo
    import test_gpu_ctc_decode as tcd
    from conftest import GOLDEN
    from test_host_cpu import make_corpus
    from ss_asr_amd.ASRDataset import prepare_x
    from ss_asr_amd.ctc import JointCTCASR
    from ss_asr_amd.trainer import ASRTester
    fx = np.load(os.path.join(GOLDEN, 'dataset_ref.npz'), allow_pickle=False)
    dims = [int(v) for v in fx['cpt_dims']]
    root = str(tmp_path)
    index, _ = make_corpus(root, n=5, t_max=40, feat=dims[4], seed=5)
    os.makedirs(os.path.join(root, 'result', 'dec'))
    torch.manual_seed(11)
    trained = JointCTCASR(*dims[:5], 1.0, ctc_weight=0.3)
    trained.load_state_dict(torch.load(os.path.join(GOLDEN, 'ref_small_asr.cpt'), map_location='cpu'))
    lo.seeded_generic_weights(trained.ctc_head, tcd.HEAD_SEED)
    torch.save(trained.state_dict(), os.path.join(root, 'result', 'dec', 'asr.cpt'))

    def tester(**decode_keys):
        config = {'asr': dict({'mdl': {'encoder_state_size': dims[1], 'decoder_state_size': dims[2],
                                       'mlp_out_size': dims[3], 'feature_dim': dims[4], 'tf_rate': 1.0, 'ctc_weight': 0.3},
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
    t = tester(decode_ctc_only={'beam_size': 4})
    assert t.decode_file == 'decode_beam_3_len_0.25_lm0.5_ctconly4' and isinstance(t.asr_model, JointCTCASR)
    said = []
    t.verbose = said.append
    got = t.exec()
    assert 'CTC only, prefix beam search, beam size 4' in said[0]
    xs, x_lens = [], []
    for x, _ in t.test_set:
        x, l = prepare_x(x, t.device)
        xs.append(x[:, :l[0]])
        x_lens.append(l)
    asr, mapper = t.asr_model, t.mapper
    # the model's entry: the checker on the GPU's own logits
    nbest = asr.decode_ctc(xs, x_lens, mapper, beam_size=4)
    assert got == [n[0][0] for n in nbest] and len(got) == 5 and all(isinstance(s, str) for s in got)
    chars, n_chars, scores, n_hyps, logits = [v.cpu().numpy() for v in asr.last_ctc_decode]
    assert chars.shape == (5, 4, logits.shape[1]) and logits.shape[2] == dims[0]
    assert asr.last_hyps[0] is asr.last_ctc_decode[0] and asr.last_hyp_scores is asr.last_ctc_decode[2]
    assert not asr.last_hyps_sampled
    frames = asr.last_encoded_packed[1].cpu().tolist()
    compared = 0
    for i in range(5):
        want, gap = reference(('model', i), logits[i, :frames[i]], 4)
        mine = [(tuple(int(c) for c in chars[i, k, :n_chars[i, k]]), float(scores[i, k])) for k in range(n_hyps[i])]
        assert [''.join(mapper.ind_to_char(c) for c in text) for text, _ in mine] == [text for text, _ in nbest[i]]
        assert [s for _, s in mine] == [s for _, s in nbest[i]]
        if gap >= MIN_GAP:
            compared += 1
            check_row(mine, want, BOUND)
    assert compared >= 3
    # what follows a decode follows this one: score, mbr, align
    sc = asr.score(got, mapper)
    assert len(sc) == 5 and all(s.chars[:3] == (0, 0, 0) for s in sc)
    picks = asr.mbr(mapper, unit='char')
    assert len(picks) == 5 and all(0 <= m.k < 4 and math.isfinite(m.risk) for m in picks)
    al = asr.align(xs, x_lens, got, mapper, encoded=asr.last_encoded_packed)
    assert all(math.isfinite(a.score) for a in al)
    # best path through the same surface, alone as in the group
    best = asr.decode_ctc(xs, x_lens, mapper, beam_size=0)
    assert all(len(h) == 1 for h in best) and asr.last_ctc_decode[0].shape[1] == 1
    assert asr.decode_ctc(xs[2:3], x_lens[2:3], mapper, beam_size=0)[0] == best[2]
    t0 = tester(decode_ctc_only={'beam_size': 0})
    assert t0.decode_file.endswith('_ctconly0') and t0.exec() == [h[0][0] for h in best]
    # the key composes with score, mbr and align
    tc = tester(decode_ctc_only={'beam_size': 4}, decode_score=True, decode_mbr={'unit': 'char'}, decode_align=True)
    assert tc.decode_file == 'decode_beam_3_len_0.25_lm0.5_ctconly4_align_mbrchar'
    composed = tc.exec()
    assert len(composed) == 5 and len(tc.last_scores) == 5 and len(tc.last_alignments) == 5
    assert tc.last_mbr_choices == [m.k for m in picks] and composed == [m.text for m in picks]
    assert all(math.isfinite(a.score) for a in tc.last_alignments) and 0.0 <= tc.last_error_rates['cer']
    # without the key: the attention search, under the old name
    plain = tester()
    assert plain.decode_file == 'decode_beam_3_len_0.25_lm0.5' and plain.decode_ctc_only is None
    plain.lm = t.lm
    assert plain.exec() == plain.asr_model.decode_many(xs, x_lens, plain.lm, plain.mapper, 0.5, beam_size=3)
    assert plain.asr_model.last_ctc_decode is None


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    measure_noise()
