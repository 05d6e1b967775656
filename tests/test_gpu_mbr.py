"""Minimum-Bayes-risk selection on the GPU (ssasr_mbr_select through ops.mbr_select; ASR.mbr, ASR.decode_mbr;
ASRTester with asr.decode_mbr) against postprocess.mbr_reference, the float64 restatement that tests/test_mbr_cpu.py
pins.  Distances are integers and are compared exactly.  A risk is a double rounded once to float (2^-24 relative),
so it is held to 1e-6 * max(1, reference).  Under the uniform posterior kernel and restatement perform the same IEEE
operations in the same order, so the choice is compared exactly, constructed ties included; under the softmax
posterior exp and log may differ in the last place, so the choice must be equal wherever the restatement's runner-up
is further away than the risk tolerance, and the seeds are chosen (and checked here, on the host) so that this holds
for at least 90 % of the utterances.  An entry at distance 0 from the chosen one is no runner-up: it is the same
sequence, its row of distances is the chosen entry's row, so its risk has the same bits on either side and the
lower slot wins on both.
The shapes are the smallest at which each mechanism can fail: one wave per pair and several (kept lengths 63 / 64 /
65 in one utterance), sixteen waves and the LDS limit (K = 8, Hmax = 1023), the K * Hmax limit with waves that belong
to no group (K = 32, Hmax = 256), sets of 0, 1, K - 1, K and more than K rows."""
import math
import os
import shutil
import types

import numpy as np
import pytest
import torch

import test_gpu_beam as tgb
import test_gpu_decode as tgd
from conftest import GOLDEN
from test_host_cpu import make_corpus

from ss_asr_amd.postprocess import ErrorStats, edit_counts, mbr_reference

pytestmark = pytest.mark.gpu

DEV = tgd.DEV
Mapper = tgd.Mapper
SPACE = Mapper().char_to_ind(' ')
POISON = 7                      # a kept character: a kernel that reads slack or past a row's length counts it
ALPHABET = [0, 1, 3, 4, 5, SPACE, SPACE]       # ids below first_char inside the rows, runs of spaces
RTOL = 1e-6
UNITS = ('char', 'word')
POSTERIORS = ('softmax', 'uniform')


class Group:
    """N utterances of K rows: rows[n][k] the raw ids, n_chars[n][k] what the kernel is told (may be negative or
    past Hmax), n_hyps[n], scores[n][k]; the restatement sees each row cut to clamp(n_chars, 0, Hmax)."""

    def __init__(self, rows, n_chars, n_hyps, scores, hmax):
        self.rows, self.n_chars, self.n_hyps, self.scores, self.hmax = rows, n_chars, n_hyps, scores, hmax
        self.N, self.K = len(rows), len(rows[0])
        self._want = {}

    def cut(self):
        return [[self.rows[n][k][:min(max(self.n_chars[n][k], 0), self.hmax)] for k in range(self.K)]
                for n in range(self.N)]

    def want(self, unit, posterior, scale=1.0):
        key = (unit, posterior, scale)
        if key not in self._want:
            self._want[key] = mbr_reference(self.cut(), self.n_hyps, self.scores, SPACE, 2, unit, posterior, scale)
        return self._want[key]

    def only(self, n):
        return Group([self.rows[n]], [self.n_chars[n]], [self.n_hyps[n]], [self.scores[n]], self.hmax)

    def launch(self, unit, posterior, scale=1.0, pad=3):
        """The entry itself on outputs pre-filled with sentinels, the rows in a matrix `pad` columns wider than Hmax
        whose slack holds POISON.  -> (best, risk, pair) as numpy arrays."""
        from ss_asr_amd import _lib, ops
        N, K, hmax = self.N, self.K, self.hmax
        m = np.full((N, K, hmax + pad), POISON, dtype=np.int32)
        for n in range(N):
            for k in range(K):
                row = self.rows[n][k][:hmax + pad]
                m[n, k, :len(row)] = row
        chars = torch.from_numpy(m).to(DEV)
        n_chars = torch.tensor(self.n_chars, dtype=torch.int32, device=DEV)
        n_hyps = torch.tensor(self.n_hyps, dtype=torch.int32, device=DEV)
        scores = torch.tensor(self.scores, dtype=torch.float32, device=DEV)
        best = torch.full((N,), -7, dtype=torch.int32, device=DEV)
        risk = torch.full((N, K), math.nan, dtype=torch.float32, device=DEV)
        pair = torch.full((N, K, K, 2), -7, dtype=torch.int32, device=DEV)
        rc = _lib.load().ssasr_mbr_select(ops._p(chars), hmax + pad, ops._p(n_chars), ops._p(n_hyps), ops._p(scores),
                                          N, K, hmax, 2, SPACE, UNITS.index(unit), POSTERIORS.index(posterior), scale,
                                          ops._p(best), ops._p(risk), ops._p(pair), ops._stream())
        assert rc == 0
        # the wrapper on a strided view of the same matrix gives the same three tensors
        got = ops.mbr_select(chars[:, :, :hmax], n_chars, n_hyps, scores if posterior == 'softmax' else None,
                             space=SPACE, unit=unit, posterior=posterior, scale=scale)
        assert got[0].dtype == torch.int32 and got[1].dtype == torch.float32 and got[2].dtype == torch.int32
        assert got[0].shape == (N,) and got[1].shape == (N, K) and got[2].shape == (N, K, K, 2)
        assert torch.equal(got[0], best) and torch.equal(got[1], risk) and torch.equal(got[2], pair)
        return best.cpu().numpy(), risk.cpu().numpy(), pair.cpu().numpy()


def draw_row(rng, longest):
    n = int(rng.integers(0, longest + 1))
    row = [int(v) for v in rng.choice(ALPHABET, size=n)]
    style = int(rng.integers(0, 6))
    if style == 0:
        row = [SPACE, SPACE] + row + [SPACE]            # leading and trailing spaces
    elif style == 1:
        row = []                                        # an empty row
    elif style == 2:
        row = [0, 1, 0][:max(n, 1)]                     # empty only after dropping
    return row


def random_group(seed, K, hmax, longest, duplicates=True):
    """N = 5 with n_hyps = 0, 1, K - 1, K, K + 3; row lengths up to `longest` (past hmax: clamped), some n_chars
    negative, some rows duplicated (ties), scores random with a -inf and a NaN among them."""
    rng = np.random.default_rng(seed)
    rows, n_chars, scores = [], [], []
    for n in range(5):
        rs = [draw_row(rng, longest) for _ in range(K)]
        if duplicates and K >= 3:
            rs[K - 1] = list(rs[0])
            rs[K // 2] = list(rs[1])
        ls = [len(r) for r in rs]
        if K >= 2:                                      # a negative length: an empty row, not one of the duplicates
            ls[1 if K <= 3 else int(rng.choice([k for k in range(2, K - 1) if k != K // 2]))] = -2
        rows.append(rs)
        n_chars.append(ls)
        sc = (-np.abs(rng.normal(size=K)) * 3).astype(np.float32).tolist()
        if K >= 8:
            sc[3], sc[5] = -math.inf, math.nan
        scores.append(sc)
    return Group(rows, n_chars, [0, 1, K - 1, K, K + 3], scores, hmax)


_groups = {}


def group(name):
    """The groups of this file and their restatements, built once."""
    if name not in _groups:
        if name.startswith('random'):
            K = int(name[6:])
            _groups[name] = random_group(10 + K, K, 20, 26)
        elif name == 'waves':
            # utterance 0: every pair in one wave (longest kept length 63); utterance 1: kept lengths 63, 64 and 65
            # (two waves per pair, pairs that would fit one wave among them); utterance 2: short rows
            rng = np.random.default_rng(5)
            kept = lambda n: [int(v) for v in rng.choice([3, 4, 5, SPACE], size=n)]
            with_dropped = lambda row: [0] + row[:30] + [1, 0] + row[30:]
            u0 = [kept(63), with_dropped(kept(63)), kept(10), [], kept(62), kept(1)]
            u1 = [kept(63), kept(64), with_dropped(kept(65)), kept(65), kept(5), with_dropped(kept(64))]
            u1[3] = list(u1[2][1:31] + u1[2][33:])       # the same kept tokens as row 2: a tie
            u2 = [kept(n) for n in (3, 0, 7, 7, 2, 1)]
            rows = [u0, u1, u2]
            sc = (-np.abs(rng.normal(size=(3, 6))) * 2).astype(np.float32).tolist()
            _groups[name] = Group(rows, [[len(r) for r in u] for u in rows], [6, 6, 5], sc, 80)
        elif name == 'sixteen':
            # K = 8, Hmax = 1023: rows of 1023 and of 1000 kept tokens (sixteen waves per pair), the others short
            rng = np.random.default_rng(6)
            long_a = [int(v) for v in rng.choice([3, 4, 5, 6, 8, SPACE], size=1023)]
            long_b = list(long_a)
            for n, i in enumerate(rng.choice(1023, size=43, replace=False)):
                long_b[int(i)] = 0 if n < 23 else 4     # 23 dropped, 20 replaced
            rows = [[long_a, [3, SPACE, 4], long_b, [], [SPACE], [4, 4, SPACE, 3], [0, 1], [5]]]
            sc = [(-np.arange(8, dtype=np.float32) * 0.25).tolist()]
            _groups[name] = Group(rows, [[len(r) for r in rows[0]]], [8], sc, 1023)
        elif name == 'limit':
            # K = 32, Hmax = 256: K * Hmax = 8192; five waves per pair, so one of the sixteen belongs to no group
            g = random_group(7, 32, 256, 14)
            rng = np.random.default_rng(8)
            for n, (k, length) in enumerate(((0, 256), (31, 256), (4, 200), (9, 300), (2, 129))):
                g.rows[n][k] = [int(v) for v in rng.choice([3, 4, 5, SPACE], size=length)]
                g.n_chars[n][k] = length
            _groups[name] = g
    return _groups[name]


def check(g, unit, posterior, scale=1.0):
    best, risk, pair = g.launch(unit, posterior, scale)
    w_best, w_risk, w_pair = g.want(unit, posterior, scale)
    assert np.array_equal(pair, np.asarray(w_pair, dtype=np.int32).reshape(pair.shape))
    assert not np.isnan(risk).any() and (best != -7).all()                  # nothing is left unwritten
    w_risk = np.asarray(w_risk, dtype=np.float64).reshape(risk.shape)
    inside = np.isfinite(w_risk)
    assert np.array_equal(np.isposinf(risk), ~inside)
    err = np.abs(risk.astype(np.float64)[inside] - w_risk[inside])
    print('%s %s: largest risk error %.3g of %.3g allowed' % (unit, posterior, err.max(initial=0.0), RTOL))
    assert (err <= RTOL * np.maximum(1.0, w_risk[inside])).all()
    if posterior == 'uniform':
        assert best.tolist() == w_best
        return
    clear = 0
    for n in range(g.N):
        nh = min(max(g.n_hyps[n], 0), g.K)
        if nh == 0:
            assert best[n] == -1 == w_best[n]
            clear += 1
            continue
        tol = RTOL * max(1.0, w_risk[n, w_best[n]])
        assert 0 <= best[n] < nh and w_risk[n, best[n]] <= w_risk[n, w_best[n]] + tol
        u = UNITS.index(unit)
        others = [w_risk[n, k] for k in range(nh) if w_pair[n][k][w_best[n]][u] != 0]
        if not others or min(others) > w_risk[n, w_best[n]] + tol:
            assert best[n] == w_best[n]
            clear += 1
    assert clear >= 0.9 * g.N, 'the seeds of this file must leave a clear runner-up on 90 %% of the utterances'


@pytest.mark.parametrize('K', (1, 2, 3, 8, 32))
def test_random_groups_against_the_restatement(K):
    g = group('random%d' % K)
    assert max(len(r) for u in g.rows for r in u) > g.hmax or K < 3        # a length past Hmax is clamped
    for unit in UNITS:
        for posterior in POSTERIORS:
            check(g, unit, posterior)
    if K >= 3:      # the duplicated rows tie under the uniform posterior; the lower slot wins
        best, risk, pair = g.launch('word', 'uniform')
        for n in (3, 4):
            assert risk[n, 0] == risk[n, K - 1] and pair[n, 0, K - 1].tolist() == [0, 0]
            assert best[n] != K - 1


def test_unit_and_scale_change_what_they_should():
    g = group('random8')
    by_char, by_word = g.launch('char', 'softmax'), g.launch('word', 'softmax')
    assert np.array_equal(by_char[2], by_word[2])                          # the distances are the unit's business
    fin = np.isfinite(by_char[1])
    assert (by_char[1][fin] != by_word[1][fin]).any()
    check(g, 'word', 'softmax', 0.25)
    check(g, 'char', 'softmax', 1e4)
    # a sharp posterior puts all the weight on the highest score: the risks are the distances to that entry
    best, risk, pair = g.launch('char', 'softmax', 1e6)
    top = int(np.nanargmax(np.where(np.isfinite(g.scores[3]), g.scores[3], -np.inf)))
    assert best[3] == min(k for k in range(8) if pair[3, k, top, 0] == 0)
    assert risk[3].tolist() == pair[3, :, top, 0].astype(np.float32).tolist()


def test_one_wave_and_two_wave_pairs_in_one_launch():
    g = group('waves')
    kept = [[sum(c >= 2 for c in r) for r in u] for u in g.rows]
    assert max(kept[0]) == 63 and {63, 64, 65} <= set(kept[1]) and max(kept[1]) == 65
    for unit in UNITS:
        check(g, unit, 'uniform')
    check(g, 'word', 'softmax')
    best, risk, pair = g.launch('char', 'uniform')
    assert pair[1, 2, 3].tolist() == [0, 0] and best[1] != 3


def test_an_utterance_alone_gives_what_it_gives_in_a_group():
    for name, n in (('waves', 1), ('random8', 3), ('random32', 4)):
        g = group(name)
        for posterior in POSTERIORS:
            together = g.launch('word', posterior)
            alone = g.only(n).launch('word', posterior)
            for a, t in zip(alone, together):
                assert np.array_equal(a[0], t[n], equal_nan=True)


def test_sixteen_waves_and_the_lds_limit():
    g = group('sixteen')
    kept = [sum(c >= 2 for c in r) for r in g.rows[0]]
    assert kept[0] == 1023 and kept[2] == 1000
    check(g, 'word', 'softmax')         # one restatement: the long pair is a million cells on the host


def test_the_limit_on_an_utterance_s_tokens():
    g = group('limit')
    assert g.K * g.hmax == 8192
    check(g, 'word', 'softmax')
    check(g, 'char', 'uniform')


def test_what_the_wrapper_refuses():
    from ss_asr_amd import ops
    chars = torch.zeros(1, 2, 4, dtype=torch.int32, device=DEV)
    n_chars = torch.ones(1, 2, dtype=torch.int32, device=DEV)
    n_hyps = torch.full((1,), 2, dtype=torch.int32, device=DEV)
    scores = torch.zeros(1, 2, device=DEV)
    best, risk, pair = ops.mbr_select(chars, n_chars, n_hyps, scores, space=SPACE)
    assert best.tolist() == [0] and risk.tolist() == [[0.0, 0.0]] and pair.tolist() == [[[[0, 0]] * 2] * 2]
    with pytest.raises(ValueError):
        ops.mbr_select(torch.zeros(1, 33, 4, dtype=torch.int32, device=DEV), torch.ones(1, 33, dtype=torch.int32, device=DEV),
                       n_hyps, torch.zeros(1, 33, device=DEV), space=SPACE)
    with pytest.raises(ValueError):
        ops.mbr_select(torch.zeros(1, 2, 1024, dtype=torch.int32, device=DEV), n_chars, n_hyps, scores, space=SPACE)
    with pytest.raises(ValueError):
        ops.mbr_select(chars, n_chars, n_hyps, None, space=SPACE)
    with pytest.raises(ValueError):
        ops.mbr_select(chars, n_chars, n_hyps, scores, space=SPACE, unit='phone')
    with pytest.raises(ValueError):
        ops.mbr_select(chars, n_chars, n_hyps, scores, space=SPACE, scale=-1.0)
    with pytest.raises(TypeError):
        ops.mbr_select(chars.long(), n_chars, n_hyps, scores, space=SPACE)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.mbr_select(chars.cpu(), n_chars, n_hyps, scores, space=SPACE)
    empty = ops.mbr_select(chars[:0], n_chars[:0], n_hyps[:0], scores[:0], space=SPACE)
    assert empty[0].shape == (0,) and empty[2].shape == (0, 2, 2, 2)


# ------------------------------------------------------------------------------------------- the model level ----
def ids_of(texts):
    m = Mapper()
    return [[m.char_to_ind(c) for c in t] for t in texts]


def want_from_texts(lists, unit, posterior, scale=1.0):
    """mbr_reference on the returned (text, score) lists, padded to the longest list"""
    K = max(len(entry) for entry in lists)
    hyps = [ids_of([t for t, _ in entry]) + [[]] * (K - len(entry)) for entry in lists]
    scores = [[s for _, s in entry] + [0.0] * (K - len(entry)) for entry in lists]
    return mbr_reference(hyps, [len(entry) for entry in lists], scores, SPACE, 2, unit, posterior, scale)


def same_choice(got, lists, want):
    best, risk, _ = want
    for m, entry, b, r in zip(got, lists, best, risk):
        assert len(m.risks) == len(entry)
        assert np.allclose(m.risks, r[:len(entry)], rtol=RTOL, atol=RTOL)
        gap = sorted(r[:len(entry)])
        if len(gap) < 2 or gap[1] - gap[0] > RTOL * max(1.0, gap[0]):
            assert m.k == b
        assert m.text == entry[m.k][0] and m.risk == m.risks[m.k]


def test_asr_mbr_and_decode_mbr(golden, monkeypatch):
    from ss_asr_amd import ops
    from ss_asr_amd.asr import ASR, MBR
    fx = golden(tgb.SMALL[0])
    asr, lm = tgd.models(fx)
    m = Mapper()
    with pytest.raises(ValueError):
        ASR(*[int(v) for v in fx['dims']], 1.0).mbr(m)                      # nothing decoded yet
    x = torch.from_numpy(fx['x']).to(DEV)
    xs, lens = [x[:, :40], x[:, :24]], [[40], [24]]
    nbest = asr.decode_nbest(xs, lens, lm, m, 0.3, 4, max_decoding_steps=tgb.STEPS)
    assert torch.equal(asr.last_hyp_scores, asr.last_beam[2])
    for unit in UNITS:
        got = asr.mbr(m, unit=unit, scale=0.5)
        assert all(isinstance(g, MBR) for g in got)
        same_choice(got, nbest, want_from_texts(nbest, unit, 'softmax', 0.5))
    assert asr.last_mbr[0].tolist() == [g.k for g in got] and asr.last_mbr[2].shape == (2, 4, 4, 2)
    uniform = asr.mbr(m, posterior='uniform')
    same_choice(uniform, nbest, want_from_texts(nbest, 'word', 'uniform'))
    # decode_mbr: the texts of the chosen slots; score() afterwards still scores slot 0
    chosen = asr.decode_mbr(xs, lens, lm, m, 0.3, 4, max_decoding_steps=tgb.STEPS, unit='word', scale=0.5)
    assert chosen == [g.text for g in got] == [nbest[i][int(k)][0] for i, k in enumerate(asr.last_mbr[0].tolist())]
    sc = asr.score([nbest[0][0][0], nbest[1][0][0]], m)
    assert all(sum(s.chars[:3]) == 0 for s in sc) and len(asr.last_score_rows[0]) == 4
    # samples: the uniform posterior by default
    gen = torch.Generator(device=DEV).manual_seed(3)
    draws = asr.sample(xs, lens, m, 8, temperature=0.8, rnn_lm=lm, lm_weight=0.5, max_decoding_steps=tgb.STEPS,
                       generator=gen)
    assert torch.equal(asr.last_hyp_scores, asr.last_samples[2])
    got = asr.mbr(m)
    want = want_from_texts(draws, 'word', 'uniform')
    same_choice(got, draws, want)
    assert [g.k for g in got] == want[0]                                    # exact under the uniform posterior
    same_choice(asr.mbr(m, posterior='softmax'), draws, want_from_texts(draws, 'word', 'softmax'))
    # greedy decoding leaves a list of one
    greedy = asr.decode_many(xs, lens, lm, m, 0.3, max_decoding_steps=tgb.STEPS)
    assert asr.last_hyp_scores.shape == (2, 1)
    assert [(g.k, g.text, g.risk, g.risks) for g in asr.mbr(m)] == [(0, t, 0.0, (0.0,)) for t in greedy]
    # a group past the kernel's limits is selected on the host: the same type of result, no launch
    # (this model ends every hypothesis within some 70 characters, so no decode of it holds 8,192 tokens; ASR.mbr
    # takes the limits from ops, and with the token limit lowered there the same group is past them)
    steps = 260
    wide = asr.decode_nbest(xs[1:], lens[1:], lm, m, 0.3, 32, max_decoding_steps=steps)
    longest = int(asr.last_hyps[1].max())
    assert ops.mbr_fits(32, min(steps, longest))
    monkeypatch.setattr(ops, 'MBR_MAX_TOKENS', 32 * min(steps, longest) - 1)
    assert not ops.mbr_fits(32, min(steps, longest))

    def refuse(*a, **k):
        raise AssertionError('the kernel was launched for a group past its limits')
    monkeypatch.setattr(ops, 'mbr_select', refuse)
    got = asr.mbr(m, unit='char')
    same_choice(got, wide, want_from_texts(wide, 'char', 'softmax'))
    assert isinstance(got[0], MBR) and asr.last_mbr[0].is_cuda and asr.last_mbr[2].shape == (1, 32, 32, 2)
    with pytest.raises(ValueError):
        ASR(*[int(v) for v in fx['dims']], 1.0).mbr(m)


def test_asr_tester_with_decode_mbr(tmp_path):
    from ss_asr_amd.ASRDataset import prepare_x, prepare_y
    from ss_asr_amd.trainer import ASRTester
    fx = np.load(os.path.join(GOLDEN, 'dataset_ref.npz'), allow_pickle=False)
    dims = [int(v) for v in fx['cpt_dims']]
    root = str(tmp_path)
    index, _ = make_corpus(root, n=5, t_max=40, feat=dims[4], seed=5)
    os.makedirs(os.path.join(root, 'result', 'dec'))
    shutil.copy(os.path.join(GOLDEN, 'ref_small_asr.cpt'), os.path.join(root, 'result', 'dec', 'asr.cpt'))

    def tester(beam, **decode_keys):
        config = {'asr': dict({'mdl': {'encoder_state_size': dims[1], 'decoder_state_size': dims[2],
                                       'mlp_out_size': dims[3], 'feature_dim': dims[4], 'tf_rate': 1.0},
                               'test_index': index, 'decode_lm_weight': 0.5, 'decode_beam_size': beam, 'decode_jobs': 1,
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

    t0 = tester(3, decode_score=True)
    plain = t0.exec()
    assert not hasattr(t0, 'last_mbr_choices') and 'mbr_wer' not in t0.last_error_rates
    t = tester(3, decode_score=True, decode_mbr={'unit': 'char', 'scale': 0.5})
    assert t.decode_file == t0.decode_file + '_mbrchar' == 'decode_beam_3_len_0.25_lm0.5_mbrchar'
    t.lm = t0.lm
    got = t.exec()
    assert len(got) == 5 == len(t.last_mbr_choices) and all(0 <= k < 3 for k in t.last_mbr_choices)
    # the n-best lists, decoded again one utterance at a time, and the restatement's choice among them
    nbest = []
    for x, _ in t.test_set:
        x, l = prepare_x(x, t.device)
        nbest.append(t.asr_model.decode_nbest([x[:, :l[0]]], [l], t.lm, t.mapper, 0.5, 3)[0])
    assert [n[0][0] for n in nbest] == plain
    want = want_from_texts(nbest, 'char', 'softmax', 0.5)
    for i, (k, text) in enumerate(zip(t.last_mbr_choices, got)):
        assert text == nbest[i][k][0]
        gap = sorted(want[1][i][:len(nbest[i])])
        if len(gap) < 2 or gap[1] - gap[0] > RTOL * max(1.0, gap[0]):
            assert k == want[0][i]
    # the unchanged keys are the plain run's, the new ones are postprocess on the written strings
    assert {k: v for k, v in t.last_error_rates.items() if not k.startswith('mbr_')} == t0.last_error_rates
    assert t.last_scores == t0.last_scores
    ref_ids = [prepare_y(y)[0][0].tolist() for _, y in t.test_set]
    stats = ErrorStats()
    for text, ref in zip(got, ref_ids):
        row = edit_counts(ids_of([text])[0], ref, SPACE)
        stats.add(row[:4], row[4:])
    assert t.last_error_rates['mbr_cer'] == stats.cer and t.last_error_rates['mbr_wer'] == stats.wer
    # without decode_score: the choices and the name, no rates
    t2 = tester(3, decode_mbr={'unit': 'word'})
    t2.lm = t0.lm
    assert t2.decode_file.endswith('_mbrword') and len(t2.exec()) == 5 and not hasattr(t2, 'last_error_rates')
    with pytest.raises(ValueError, match='decode_beam_size'):
        tester(1, decode_mbr={'unit': 'word', 'scale': 1.0})
