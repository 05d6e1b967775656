"""ssasr_ctc_decode_graph on the GPU (ctc_prefix_beam_graph_kernel, csrc/ctc.hip): the CTC prefix beam search with a
character graph in the ranking, held to postprocess.ctc_prefix_beam_graph_reference, the float64 restatement that
tests/test_ctc_graph_cpu.py pins.

Cases.  Logits 4 N(0, 1) from default_rng([T, V, seed]), seeds 0..15, graph_weight 0.5, length_bonus 0.3, over CELLS;
every cell runs with three graphs over its V classes: random ones of S = 7 and S = 300 states (random next, arcs
N(0, 1) with one in ten -inf, start = S - 1 so that the last row is read) and the hotword graph of three phrases drawn
from the classes at bonus 1; the V = 40 cells also with the order-3 n-gram graph of the golden text, its 48 characters
folded onto the classes 2..39.  The 16 seeds of a cell and graph are one launch.
A case is compared when the checker's gap (on the fused keys and between adjacent final totals) is >= MIN_GAP = 1e-3,
the project's rule; at least 85 % of all cases must be compared and no (cell, graph) below half.  The checker alone
(this file's __main__, on the CPU) meets both with arcs of scale 1: 1075 of 1120 cases (96 %), the worst cell 12 of
16.
A compared case must hold the checker's SET of texts, in the kernel's own non-increasing order, with the fused score and
each part within BOUND = 8 * NOISE.  NOISE = max |float32 - float64| of the checker run in float32 over the compared
hypotheses' totals and parts, measured by __main__ on the CPU: 9.5e-5 (the n-gram graph at T' = 80; 2.1e-5 without
it).  The kernel's worst error on the MI355X is recorded beside it (KERNEL_WORST): 1.4e-5.
Zero weights are bit-equal to ssasr_ctc_decode on every cell, with a graph and with NULL; an utterance alone is bit-equal
to itself in a group."""
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
CELLS = ([(T, 8, K) for T in (1, 3, 5) for K in (1, 2, 3, 8, 32)] +
         [(20, V, K) for V in (8, 40) for K in (1, 3, 8)] +
         [(80, 40, 2)])
GW, BETA = 0.5, 0.3
ARC_SCALE = 1.0
COMPARED_CPU = (1075, 1120)                                      # measure(), on the CPU
WORST_CELL_CPU = 12
NOISE = 9.5e-5                                                   # measure(), on the CPU
BOUND = 8 * NOISE
KERNEL_WORST = 1.4e-5                                            # worst |kernel - float64| seen on the MI355X
CANARY_I, CANARY_F = -77, 12345.0
PAD = 64                                                         # canary elements behind every output


def logits_of(T, V, seed):
    return (4.0 * np.random.default_rng([T, V, seed]).standard_normal((T, V))).astype(np.float32)


def log_softmax(z, dtype=np.float64):
    z = z.astype(dtype)
    m = z.max(-1, keepdims=True)
    return z - (m + np.log(np.exp(z - m).sum(-1, keepdims=True, dtype=dtype)))


_graphs = {}


def graph_of(kind, V):
    """The test's graphs over V classes, built once."""
    from test_ctc_graph_cpu import EOS, golden_sequences, random_graph
    from ss_asr_amd.char_graph import CharGraph
    if (kind, V) not in _graphs:
        if kind == 'rand7':
            g = random_graph(7, V, 0, ARC_SCALE)
        elif kind == 'rand300':
            g = random_graph(300, V, 1, ARC_SCALE)
        elif kind == 'hot':
            rng = np.random.default_rng([V, 5])
            g = CharGraph.hotwords([rng.integers(1, V, n).tolist() for n in (2, 3, 2)], 1.0, V)
        else:
            seqs, _ = golden_sequences()
            g = CharGraph.ngram([[2 + (c - 2) % (V - 2) for c in s] for s in seqs], 3, V, EOS)
        _graphs[(kind, V)] = g
    return _graphs[(kind, V)]


def kinds_of(V):
    return ('rand7', 'rand300', 'hot') + (('ngram3',) if V == 40 else ())


_refs = {}


def reference(key, z, K, graph, gw=GW, beta=BETA, blank=0):
    """(hyps, gap, parts) of the checker on float64 log_softmax(z), computed once per key."""
    from ss_asr_amd.postprocess import ctc_prefix_beam_graph_reference
    full = (key, K, gw, beta, blank)
    if full not in _refs:
        parts = []
        hyps, gap = ctc_prefix_beam_graph_reference(log_softmax(z), K, graph, gw, beta, blank, parts=parts)
        _refs[full] = (hyps, gap, parts)
    return _refs[full]


def noise_of(z, K, graph):
    """max |float32 - float64| of the totals and parts over the texts both runs of the checker hold (None: the case is
    not compared)."""
    from ss_asr_amd.postprocess import ctc_prefix_beam_graph_reference
    parts = []
    hyps, gap = ctc_prefix_beam_graph_reference(log_softmax(z), K, graph, GW, BETA, parts=parts)
    if gap < MIN_GAP:
        return None
    parts32 = []
    hyps32, _ = ctc_prefix_beam_graph_reference(log_softmax(z, np.float32), K, graph, GW, BETA, dtype=np.float32,
                                                parts=parts32)
    low = {t: (s,) + p for (t, s), p in zip(hyps32, parts32)}
    return max([0.0] + [abs(a - b) for (t, s), p in zip(hyps, parts) if t in low for a, b in zip((s,) + p, low[t])])


def measure():
    worst, done, total, least = 0.0, 0, 0, len(SEEDS)
    for T, V, K in CELLS:
        for kind in kinds_of(V):
            cell = [n for n in (noise_of(logits_of(T, V, s), K, graph_of(kind, V)) for s in SEEDS) if n is not None]
            worst, done, total, least = max([worst] + cell), done + len(cell), total + len(SEEDS), min(least, len(cell))
            print('T=%d V=%d K=%d %s: %d of %d compared, noise %.3g' % (T, V, K, kind, len(cell), len(SEEDS),
                                                                      max([0.0] + cell)), flush=True)
    print('%d of %d compared (%.1f %%), the worst cell %d of %d' % (done, total, 100.0 * done / total, least, len(SEEDS)))
    print('NOISE: %.4g' % worst)


def run(z, frame_lens, K, graph, gw=GW, beta=BETA, blank=0):
    """ssasr_ctc_decode_graph on z [B, T, V] through the C entry, every output and the workspace followed by PAD canaries
    and pre-filled, so that an element the kernel leaves unwritten or writes past its end shows.  -> per row the list
    of (text, total, ctc, graph part) and the raw arrays."""
    import ctypes
    from ss_asr_amd import _lib, ops
    lib = _lib.load()
    B, T, V = z.shape
    need = int(lib.ssasr_ctc_decode_graph_ws_bytes(B, T, V, K))
    assert need > 0 and need % 4 == 0
    s, keep = graph.to(DEV) if graph is not None else (None, None)
    logits = torch.from_numpy(np.ascontiguousarray(z)).to(DEV)
    lens = torch.tensor(list(frame_lens), dtype=torch.int32, device=DEV)
    ws = torch.full((need // 4 + PAD,), CANARY_I, dtype=torch.int32, device=DEV)
    ints = {'chars': B * K * T, 'n_chars': B * K, 'n_hyps': B}
    flts = {'scores': B * K, 'ctc_scores': B * K, 'graph_scores': B * K}
    buf = {n: torch.full((c + PAD,), CANARY_I, dtype=torch.int32, device=DEV) for n, c in ints.items()}
    buf.update({n: torch.full((c + PAD,), CANARY_F, dtype=torch.float32, device=DEV) for n, c in flts.items()})
    ops.check(lib.ssasr_ctc_decode_graph(ops._p(logits), ops._p(lens), B, T, V, K, blank, ops._p(ws), need,
                                         ops._p(buf['chars']), ops._p(buf['n_chars']), ops._p(buf['scores']),
                                         ops._p(buf['n_hyps']), ctypes.byref(s) if s is not None else None, gw, beta,
                                         ops._p(buf['ctc_scores']), ops._p(buf['graph_scores']), ops._stream()),
              'ssasr_ctc_decode_graph')
    torch.cuda.synchronize()
    assert (ws.cpu().numpy()[need // 4:] == CANARY_I).all(), 'ws: written past its end'
    raw = {}
    for name, count in list(ints.items()) + list(flts.items()):
        arr = buf[name].cpu().numpy()
        canary = CANARY_I if name in ints else CANARY_F
        assert (arr[count:] == canary).all(), name + ': written past its end'
        assert not (arr[:count] == canary).any(), name + ': an element was left unwritten'
        raw[name] = arr[:count].reshape((B, K, T) if name == 'chars' else (B,) if name == 'n_hyps' else (B, K))
    out = []
    for b in range(B):
        n_h = raw['n_hyps'][b]
        assert 1 <= n_h <= K                                     # a beam never empties
        for k in range(K):
            n = raw['n_chars'][b, k]
            assert 0 <= n <= T and (raw['chars'][b, k, n:] == 0).all()
            if k >= n_h:
                assert n == 0 and raw['scores'][b, k] == -math.inf and raw['ctc_scores'][b, k] == -math.inf
                assert raw['graph_scores'][b, k] == 0.0
            else:
                assert math.isfinite(raw['scores'][b, k]) and math.isfinite(raw['graph_scores'][b, k])
        out.append([(tuple(int(c) for c in raw['chars'][b, k, :raw['n_chars'][b, k]]), float(raw['scores'][b, k]),
                     float(raw['ctc_scores'][b, k]), float(raw['graph_scores'][b, k])) for k in range(n_h)])
    return out, raw


def check_row(got, want, parts, bound):
    """The kernel's list against the checker's: the same set of texts, the kernel's own order, the fused score and each
    part within bound.  -> the worst error."""
    texts = [g[0] for g in got]
    assert len(got) == len(want) and set(texts) == {t for t, _ in want} and len(set(texts)) == len(got)
    totals = [g[1] for g in got]
    assert totals == sorted(totals, reverse=True)
    ref = {t: (s,) + tuple(p) for (t, s), p in zip(want, parts)}
    worst = max(abs(a - b) for g in got for a, b in zip(g[1:], ref[g[0]]))
    assert worst <= bound, (worst, bound)
    return worst


def plain(z, frame_lens, K, blank=0):
    """ssasr_ctc_decode's four arrays."""
    from ss_asr_amd import ops
    out = ops.ctc_decode(torch.from_numpy(np.ascontiguousarray(z)).to(DEV),
                         torch.tensor(list(frame_lens), dtype=torch.int32, device=DEV), K, blank)
    return [t.cpu().numpy() for t in out]


def bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def test_the_kernel_matches_the_checker_on_every_compared_case():
    compared, worst, total = {}, 0.0, 0
    for T, V, K in CELLS:
        z = np.stack([logits_of(T, V, s) for s in SEEDS])
        for kind in kinds_of(V):
            graph = graph_of(kind, V)
            got, _ = run(z, [T] * len(SEEDS), K, graph)
            compared[(T, V, K, kind)] = 0
            for s in SEEDS:
                total += 1
                want, gap, parts = reference((T, V, s, kind), z[s], K, graph)
                if gap < MIN_GAP:
                    continue
                compared[(T, V, K, kind)] += 1
                worst = max(worst, check_row(got[s], want, parts, BOUND))
    done = sum(compared.values())
    print('compared per cell (of %d): %s' % (len(SEEDS), compared))
    print('%d of %d cases compared, worst |kernel - float64| %.3g (NOISE %.3g, bound %.3g)'
          % (done, total, worst, NOISE, BOUND))
    assert total == COMPARED_CPU[1]
    assert done >= 0.85 * total
    assert all(2 * n >= len(SEEDS) for n in compared.values())


def test_zero_weights_are_ssasr_ctc_decode_bit_for_bit_on_every_cell():
    for T, V, K in CELLS:
        z = np.stack([logits_of(T, V, s) for s in SEEDS])
        chars, n_chars, scores, n_hyps = plain(z, [T] * len(SEEDS), K)
        for graph in (None, graph_of('rand300', V)):             # with a graph at weight 0: unread
            _, raw = run(z, [T] * len(SEEDS), K, graph, gw=0.0, beta=0.0)
            assert np.array_equal(raw['chars'], chars) and np.array_equal(raw['n_chars'], n_chars), (T, V, K)
            assert np.array_equal(raw['n_hyps'], n_hyps)
            assert np.array_equal(bits(raw['scores']), bits(scores)) and np.array_equal(bits(raw['ctc_scores']), bits(scores))
            assert (raw['graph_scores'] == 0.0).all()


@pytest.mark.parametrize('K', [2, 8])
def test_an_utterance_decodes_in_a_group_as_it_decodes_alone(K):
    lens = [20, 5, 1]
    graph = graph_of('rand300', 8)
    z = np.stack([logits_of(20, 8, 200 + i) for i in range(len(lens))])
    _, group = run(z, lens, K, graph)
    for i, n in enumerate(lens):
        _, alone = run(z[i:i + 1, :n], [n], K, graph)
        for name in ('n_chars', 'n_hyps', 'scores', 'ctc_scores', 'graph_scores'):
            assert np.array_equal(bits(alone[name][0]), bits(group[name][i])), name
        assert np.array_equal(alone['chars'][0], group['chars'][i, :, :n]) and (group['chars'][i, :, n:] == 0).all()


@pytest.mark.parametrize('K', [1, 3, 8])
def test_edges(K):
    """Lengths 0, 1 and past T', blank 3, a length bonus alone, and a start state with one open arc."""
    from test_ctc_graph_cpu import random_graph
    from ss_asr_amd.char_graph import CharGraph
    T, V = 20, 8
    rows = [('no frames', logits_of(T, V, 100), 0), ('one frame', logits_of(T, V, 101), 1),
            ('length past the rows', logits_of(T, V, 102), 25), ('whole', logits_of(T, V, 103), 20)]
    base = graph_of('rand7', V)
    arc = base.arc.astype(np.float64)                            # every non-blank arc out of the start but one is -inf
    arc[base.start, 1:] = -np.inf
    arc[base.start, 5] = 0.25
    gate = CharGraph(base.next, arc, base.fin, base.start)
    for tag, blank, gw, beta, graph in (('base', 0, GW, BETA, base), ('blank 3', 3, GW, BETA, random_graph(7, V, 2, blank=3)),
                                        ('bonus alone', 0, 0.0, BETA, base), ('gate', 0, GW, 0.0, gate)):
        got, raw = run(np.stack([r[1] for r in rows]), [r[2] for r in rows], K, graph, gw, beta, blank)
        for (name, z, n), mine in zip(rows, got):
            want, gap, parts = reference((name, tag), z[:min(n, T)], K, graph, gw, beta, blank)
            if gap >= MIN_GAP:
                check_row(mine, want, parts, BOUND)
            if name == 'no frames':                              # the empty text alone: fin[start] is its whole score
                assert len(mine) == 1 and mine[0][0] == () and mine[0][2] == 0.0
                assert abs(mine[0][1] - want[0][1]) <= BOUND
            if tag == 'gate':
                assert all(g[0] == () or g[0][0] == 5 for g in mine)
        if gw == 0.0:
            assert (raw['graph_scores'] == 0.0).all()


def test_ops_is_the_entry_and_rejects_what_the_entry_rejects():
    from ss_asr_amd import ops
    V = 8
    graph = graph_of('hot', V)
    zs = np.stack([logits_of(20, V, s) for s in range(3)])
    lens = torch.tensor([20, 7, 0], dtype=torch.int32, device=DEV)
    out = ops.ctc_decode_graph(torch.from_numpy(zs).to(DEV), lens, 5, graph, GW, BETA)
    _, raw = run(zs, [20, 7, 0], 5, graph)
    for name, arr in raw.items():
        assert np.array_equal(bits(out[name].cpu().numpy()), bits(arr)), name
    with pytest.raises(ValueError, match='no kernel'):
        ops.ctc_decode_graph(torch.zeros(1, 4097, V, device=DEV), lens[:1], 2, graph, 0.5)
    with pytest.raises(ValueError, match='classes'):
        ops.ctc_decode_graph(torch.zeros(1, 8, 9, device=DEV), lens[:1], 2, graph, 0.5)


def test_decode_ctc_with_a_graph_and_the_tester_keys(golden, tmp_path):
    import las_oracle as lo
    import test_gpu_ctc_decode as tcd
    import test_gpu_rescore as tgr
    from conftest import GOLDEN
    from test_ctc_graph_cpu import random_graph
    from test_host_cpu import make_corpus
    from ss_asr_amd.ASRDataset import Mapper, prepare_x
    from ss_asr_amd.char_graph import CharGraph
    from ss_asr_amd.ctc import JointCTCASR
    from ss_asr_amd.trainer import ASRTester
    fx = golden(tgr.SMALL)
    asr, lm = tcd.models(fx)
    mapper = Mapper()
    V = mapper.get_dim()
    xs, x_lens = tgr.ctc_groups(fx, (40, 24, 8), 3)
    graph = random_graph(40, V, 3, ARC_SCALE)
    nbest = asr.decode_ctc(xs, x_lens, mapper, beam_size=3, graph=graph, graph_weight=GW, length_bonus=BETA)
    assert len(asr.last_ctc_decode) == 7 and asr.last_hyp_scores is asr.last_ctc_decode[2]
    chars, n_chars, scores, n_hyps, logits, ctc_s, gr_s = [t.cpu().numpy() for t in asr.last_ctc_decode]
    frames = asr.last_encoded_packed[1].cpu().tolist()
    compared = 0
    for i in range(3):
        n = int(n_hyps[i])
        assert [s for _, s in nbest[i]] == scores[i, :n].tolist()
        want, gap, parts = reference(('model', i), logits[i, :frames[i]], 3, graph)
        if gap >= MIN_GAP:
            compared += 1
            mine = [(tuple(int(c) for c in chars[i, k, :n_chars[i, k]]), float(scores[i, k]), float(ctc_s[i, k]),
                     float(gr_s[i, k])) for k in range(n)]
            check_row(mine, want, parts, BOUND)
    assert compared >= 2
    # the plain search's second text as the one hotword, at a bonus that must make it win
    asr.decode_ctc(xs, x_lens, mapper, beam_size=4)
    p_chars, p_n, p_scores, p_hyps = [t.cpu().numpy() for t in asr.last_ctc_decode[:4]]
    def inside(short, long):
        return any(long[j:j + len(short)] == short for j in range(len(long) - len(short) + 1))
    texts = [[[int(c) for c in p_chars[i, k, :p_n[i, k]]] for k in range(int(p_hyps[i]))] for i in range(3)]
    # A text without the phrase is paid nothing at the end, so the phrase passes the plain search's first text once
    # bonus * len exceeds that text's lead: half a nat more than the lead.  A text that CONTAINS the phrase is paid the
    # same, and the biased search keeps more of such a text's labellings than the plain one did, so whether the phrase
    # itself ends first is the checker's to say: the first utterance where it does (on the head's own logits) is used.
    chosen = None
    for i in range(3):
        if len(texts[i]) < 2 or not texts[i][1] or inside(texts[i][1], texts[i][0]):
            continue
        second = texts[i][1]
        bonus = (float(p_scores[i, 0] - p_scores[i, 1]) + 0.5) / len(second)
        hot = CharGraph.hotwords([second], bonus, V)
        want, gap, parts = reference(('hotword', i), logits[i, :frames[i]], 4, hot, 1.0, 0.0)
        print('utterance %d: hotword %r, plain scores %s, bonus %.4g, the checker\'s first %r, gap %.3g'
              % (i, second, p_scores[i].tolist(), bonus, want[0][0], gap))
        if list(want[0][0]) == second and gap >= MIN_GAP and chosen is None:
            chosen = (i, second, bonus, hot, want, parts)
    assert chosen is not None
    i, second, bonus, hot, want, parts = chosen
    asr.decode_ctc(xs[i:i + 1], x_lens[i:i + 1], mapper, beam_size=4, graph=hot, graph_weight=1.0)
    b_chars, b_n, b_scores, b_hyps, _, b_ctc, b_gr = [t.cpu().numpy() for t in asr.last_ctc_decode]
    assert [int(c) for c in b_chars[0, 0, :b_n[0, 0]]] == second
    assert abs(float(b_gr[0, 0]) - bonus * len(second)) <= 1e-5 * bonus * len(second)
    check_row([(tuple(int(c) for c in b_chars[0, k, :b_n[0, k]]), float(b_scores[0, k]), float(b_ctc[0, k]),
                float(b_gr[0, k])) for k in range(int(b_hyps[0]))], want, parts, BOUND)
    # score, mbr and align follow it
    nbest = asr.decode_ctc(xs, x_lens, mapper, beam_size=3, graph=graph, graph_weight=GW)
    tops = [h[0][0] for h in nbest]
    assert len(asr.score(tops, mapper)) == 3
    assert all(0 <= m.k < 3 for m in asr.mbr(mapper, unit='char'))
    assert len(asr.align(xs, x_lens, tops, mapper, encoded=asr.last_encoded_packed)) == 3
    # the default keywords, and a graph at weight 0, take the old entry
    asr.decode_ctc(xs, x_lens, mapper, beam_size=3, graph=graph)
    assert len(asr.last_ctc_decode) == 5

    # ASRTester with and without the new keys
    fxd = np.load(os.path.join(GOLDEN, 'dataset_ref.npz'), allow_pickle=False)
    dims = [int(v) for v in fxd['cpt_dims']]
    root = str(tmp_path)
    index, _ = make_corpus(root, n=5, t_max=40, feat=dims[4], seed=5)
    os.makedirs(os.path.join(root, 'result', 'dec'))
    torch.manual_seed(11)
    trained = JointCTCASR(*dims[:5], 1.0, ctc_weight=0.3)
    trained.load_state_dict(torch.load(os.path.join(GOLDEN, 'ref_small_asr.cpt'), map_location='cpu'))
    lo.seeded_generic_weights(trained.ctc_head, tcd.HEAD_SEED)
    torch.save(trained.state_dict(), os.path.join(root, 'result', 'dec', 'asr.cpt'))
    lm_path = os.path.join(root, 'ngram.npz')
    ngram = CharGraph.ngram([[mapper.char_to_ind(c) for c in w] for w in ('hello', 'halló', 'hold')], 3, V, 1)
    ngram.save(lm_path)

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
        t.decode_group = 2
        return t
    old = tester(decode_ctc_only={'beam_size': 4})
    assert old.decode_file == 'decode_beam_3_len_0.25_lm0.5_ctconly4' and old.decode_ctc_graph is None
    base = old.exec()
    assert len(old.asr_model.last_ctc_decode) == 5
    t = tester(decode_ctc_only={'beam_size': 4, 'hotwords': ['hold', 'hal'], 'hotword_bonus': 1.5, 'ngram_lm': lm_path,
                                'ngram_weight': 0.25, 'length_bonus': 0.25}, decode_score=True)
    assert t.decode_file == 'decode_beam_3_len_0.25_lm0.5_ctconly4_hw2x1.5_ng0.25_clb0.25'
    got = t.exec()
    assert len(got) == 5 and len(t.last_scores) == 5 and len(t.asr_model.last_ctc_decode) == 7
    hot = CharGraph.hotwords([[mapper.char_to_ind(c) for c in w] for w in ('hold', 'hal')], 1.5, V)
    both = CharGraph.product(ngram.scaled(0.25), hot)
    direct = []
    for x, _ in t.test_set:
        x, l = prepare_x(x, t.device)
        direct.append(t.asr_model.decode_ctc([x[:, :l[0]]], [l], t.mapper, beam_size=4, length_bonus=0.25, graph=both,
                                             graph_weight=1.0)[0][0][0])
    assert got == direct
    one = tester(decode_ctc_only={'beam_size': 4, 'ngram_lm': lm_path})
    assert one.decode_file == 'decode_beam_3_len_0.25_lm0.5_ctconly4_ng0.5' and one.decode_ctc_graph[1] == 0.5
    assert len(one.exec()) == 5 and len(one.asr_model.last_ctc_decode) == 7
    assert base == tester(decode_ctc_only={'beam_size': 4}).exec()


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    measure()
