"""CTC decoding with a character graph in the search, without a GPU: char_graph.CharGraph and its builders (a
Witten-Bell character n-gram LM, the hotwords' Aho-Corasick automaton, the product) checked against brute force and
against the recursion evaluated directly from the counts; postprocess.ctc_prefix_beam_graph_reference, the float64
restatement of ssasr_ctc_decode_graph (include/ssasr.h) that test_gpu_ctc_graph.py holds the kernel to, checked against
the sum over every frame labelling and hand-built tables; and the argument errors of the C entries, ops,
ASR.decode_ctc and ASRTester's asr.decode_ctc_only keys."""
import ctypes
import itertools
import math
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_ctc_search_cpu import brute_force, log_softmax64
from test_host_cpu import header_prototypes

NEG = -math.inf
TEXT = os.path.join(GOLDEN, 'charlm_dataset.txt')
EOS = 1


def random_graph(S, V, seed, scale=1.0, forbid=0.1, blank=0):
    """Random next, arcs scale N(0, 1) with a share `forbid` of them -inf, start = S - 1 (the last row is read)."""
    from ss_asr_amd.char_graph import CharGraph
    rng = np.random.default_rng([S, V, seed, 11])
    nxt = rng.integers(0, S, (S, V))
    arc = scale * rng.standard_normal((S, V))
    arc[rng.random((S, V)) < forbid] = NEG
    nxt[:, blank], arc[:, blank] = np.arange(S), 0.0
    return CharGraph(nxt, arc, scale * rng.standard_normal(S), S - 1)


def golden_sequences():
    """(the golden text's words as label sequences, the number of classes)"""
    from ss_asr_amd.LMDataset import LMDataset
    ds = LMDataset(TEXT, 8)
    return [[ds.char2idx[ch] for ch in word] for word in ds.file.split(' ') if word], ds.get_num_chars()


_ngrams = {}


def golden_ngram(order):
    from ss_asr_amd.char_graph import CharGraph
    if order not in _ngrams:
        seqs, V = golden_sequences()
        _ngrams[order] = CharGraph.ngram(seqs, order, V, EOS)
    return _ngrams[order]


def walk(graph, text):
    """G and the state by a walk that shares nothing with CharGraph.score."""
    s, total = graph.start, 0.0
    for c in text:
        total, s = total + float(graph.arc[s][c]), int(graph.next[s][c])
    return total, s


def texts_up_to(classes, n):
    return [t for k in range(n + 1) for t in itertools.product(classes, repeat=k)]


# ------------------------------------------------------------------ the checker ----
def test_zero_weights_are_the_plain_checker_exactly():
    from ss_asr_amd.postprocess import ctc_prefix_beam_graph_reference, ctc_prefix_beam_reference
    for T, V, K, seed in ((1, 8, 3, 0), (5, 8, 2, 1), (20, 8, 8, 2), (20, 40, 3, 3)):
        lp = log_softmax64(4.0 * np.random.default_rng([T, V, seed]).standard_normal((T, V)))
        for graph in (None, random_graph(7, V, seed)):
            tr_a, tr_b, parts = [], [], []
            got, gap = ctc_prefix_beam_graph_reference(lp, K, graph, 0.0, 0.0, trace=tr_a, parts=parts)
            want, plain_gap = ctc_prefix_beam_reference(lp, K, trace=tr_b)
            assert got == want and tr_a == tr_b
            assert [p[0] for p in parts] == [s for _, s in want] and all(p[1] == 0.0 for p in parts)
            final = min([math.inf] + [a[1] - b[1] for a, b in zip(want, want[1:])])
            assert gap == min(plain_gap, final)
        lp32 = lp.astype(np.float32)
        assert ctc_prefix_beam_graph_reference(lp32, K, None, dtype=np.float32)[0] == \
            ctc_prefix_beam_reference(lp32, K, dtype=np.float32)[0]


@pytest.mark.parametrize('T', [1, 2, 3, 4])
@pytest.mark.parametrize('blank', [0, 1])
def test_a_beam_that_drops_nothing_scores_every_text_as_the_enumeration_plus_the_graph(T, blank):
    from ss_asr_amd.postprocess import ctc_prefix_beam_graph_reference
    V, gw, beta = 3, 0.5, 0.3
    lp = log_softmax64(np.random.default_rng([T, blank, 9]).standard_normal((T, V)) * 2.0)
    graph = random_graph(5, V, T, forbid=0.0, blank=blank)
    every = brute_force(lp, blank)
    parts = []
    got, gap = ctc_prefix_beam_graph_reference(lp, 32, graph, gw, beta, blank, parts=parts)
    assert len(every) <= 32 and {t for t, _ in got} == set(every)
    g32, b32 = float(np.float32(gw)), float(np.float32(beta))
    for (text, total), (ctc, part) in zip(got, parts):
        G, s = walk(graph, text)
        assert abs(ctc - every[text]) <= 1e-12
        assert abs(part - (G + float(graph.fin[s]))) <= 1e-12
        assert abs(total - (every[text] + g32 * (G + float(graph.fin[s])) + b32 * len(text))) <= 1e-12
    assert [s for _, s in got] == sorted((s for _, s in got), reverse=True)
    assert gap == min(a[1] - b[1] for a, b in zip(got, got[1:])) if len(got) > 1 else gap == math.inf


def test_the_graph_flips_the_winner_of_a_hand_built_table():
    from ss_asr_amd.char_graph import CharGraph
    from ss_asr_amd.postprocess import ctc_prefix_beam_graph_reference
    # one frame, classes (blank, 1, 2): the head prefers 1 by log(0.5 / 0.4); the graph pays 1 nat for class 2
    lp = np.log(np.array([[0.1, 0.5, 0.4]]))
    graph = CharGraph([[0, 0, 1], [1, 1, 1]], [[0.0, 0.0, 1.0], [0.0, 0.0, 0.0]], [0.0, 0.25])
    assert ctc_prefix_beam_graph_reference(lp, 3, None)[0][0][0] == (1,)
    parts = []
    got, gap = ctc_prefix_beam_graph_reference(lp, 3, graph, 1.0, parts=parts)
    assert [t for t, _ in got] == [(2,), (1,), ()]
    assert abs(got[0][1] - (math.log(0.4) + 1.25)) <= 1e-12 and parts[0] == (math.log(0.4), 1.25)
    assert abs(got[1][1] - math.log(0.5)) <= 1e-12 and abs(got[2][1] - math.log(0.1)) <= 1e-12
    assert abs(gap - min(got[0][1] - got[1][1], got[1][1] - got[2][1])) <= 1e-12
    # a tenth of the weight does not pay for the head's preference (0.125 < log 1.25)
    assert ctc_prefix_beam_graph_reference(lp, 3, graph, 0.1)[0][0][0] == (1,)
    # K = 1: the graph keeps a text the plain search drops for good
    two = np.log(np.array([[0.1, 0.5, 0.4], [0.98, 0.01, 0.01]]))
    trace = []
    assert ctc_prefix_beam_graph_reference(two, 1, graph, 1.0, trace=trace)[0][0][0] == (2,)
    assert trace[0] == frozenset({(2,)})
    with pytest.raises(ValueError, match='>= 0'):
        ctc_prefix_beam_graph_reference(lp, 3, graph, -1.0)
    for bad in (dict(K=0), dict(graph=None), dict(graph_weight=math.inf), dict(length_bonus=math.nan)):
        args = dict(K=2, graph=graph, graph_weight=0.5, length_bonus=0.0)
        args.update(bad)
        with pytest.raises(ValueError):
            ctc_prefix_beam_graph_reference(lp, args['K'], args['graph'], args['graph_weight'], args['length_bonus'])
    with pytest.raises(ValueError, match='classes'):
        ctc_prefix_beam_graph_reference(np.log(np.full((1, 4), 0.25)), 2, graph, 0.5)


def test_a_forbidden_arc_removes_the_text_the_plain_search_ranks_first():
    from ss_asr_amd.char_graph import CharGraph
    from ss_asr_amd.postprocess import ctc_prefix_beam_graph_reference, ctc_prefix_beam_reference
    lp = log_softmax64(np.array([[0.0, 3.0, 1.0], [0.0, 1.0, 3.5], [2.0, 0.0, 0.0]]))
    best = ctc_prefix_beam_reference(lp, 4)[0][0][0]
    assert best == (1, 2)
    # a lexicon-like table: after a 1 no 2 may follow (state 1 = 'the text ends in 1')
    graph = CharGraph([[0, 1, 0], [1, 1, 0]], [[0.0, 0.0, 0.0], [0.0, 0.0, NEG]], [0.0, 0.0])
    trace, parts = [], []
    got, _ = ctc_prefix_beam_graph_reference(lp, 4, graph, 1.0, trace=trace, parts=parts)
    assert got and all(not any(a == 1 and b == 2 for a, b in zip(t, t[1:])) for beam in trace for t in beam)
    assert best not in {t for t, _ in got}
    plain = dict(ctc_prefix_beam_reference(lp, 32)[0])
    for (text, total), (ctc, part) in zip(got, parts):          # the survivors keep their pure CTC mass
        assert part == 0.0 and total == ctc and math.isfinite(total)
    assert abs(dict(got)[(1,)] - plain[(1,)]) <= 1e-12
    # every non-blank arc out of the start state forbidden: the empty text alone survives, the beam never empties
    wall = CharGraph([[0, 0, 0]], [[0.0, NEG, NEG]], [0.5])
    got, gap = ctc_prefix_beam_graph_reference(lp, 4, wall, 2.0)
    assert [t for t, _ in got] == [()] and abs(got[0][1] - (lp[:, 0].sum() + 1.0)) <= 1e-12 and gap == math.inf


def test_one_state_is_a_per_class_bias():
    from ss_asr_amd.char_graph import CharGraph
    from ss_asr_amd.postprocess import ctc_prefix_beam_graph_reference
    V, T = 4, 2
    bias = np.array([0.0, 0.75, -0.5, 0.25])                     # exact in float32
    graph = CharGraph(np.zeros((1, V), dtype=np.int64), bias[None], [0.0])
    lp = log_softmax64(np.random.default_rng(3).standard_normal((T, V)) * 2.0)
    every = brute_force(lp, 0)
    got, _ = ctc_prefix_beam_graph_reference(lp, 32, graph, 0.5)
    want = {t: every[t] + 0.5 * sum(bias[c] for c in t) for t in every}
    assert len(every) == 10 and {t for t, _ in got} == set(every)
    assert [t for t, _ in got] == sorted(want, key=lambda t: -want[t])
    assert all(abs(total - want[text]) <= 1e-12 for text, total in got)
    assert [t for t, _ in got] != [t for t, _ in ctc_prefix_beam_graph_reference(lp, 32, None)[0]]


# -------------------------------------------------------------------- builders ----
PHRASES = [(1, 2), (1, 2, 3), (2, 3), (2,), (3, 1, 2)]           # ab, abc, bc, b, cab over (blank, a, b, c)


def substring_lengths(text, phrases):
    return sum(len(p) for p in phrases for i in range(len(text) - len(p) + 1) if tuple(text[i:i + len(p)]) == p)


def test_hotwords_score_the_summed_length_of_every_occurrence():
    from ss_asr_amd.char_graph import CharGraph
    bonus = 0.75
    graph = CharGraph.hotwords(PHRASES, bonus, 4)
    assert graph.n_states == 1 + 8 and graph.start == 0          # the trie of the five phrases: a ab abc b bc c ca cab
    for text in texts_up_to((1, 2, 3), 6):
        G, s = graph.score(text)
        assert (G, s) == walk(graph, text)
        pend = -float(graph.fin[s]) / bonus
        assert pend >= 0.0
        assert abs(G + float(graph.fin[s]) - bonus * substring_lengths(text, PHRASES)) <= 1e-12
        # pend: the length of the longest suffix of the text that is a proper prefix of a phrase, minus the longest
        # phrase that is a suffix of THAT; checked directly
        depth = max(k for k in range(len(text) + 1)
                    if any(p[:k] == tuple(text[len(text) - k:]) for p in PHRASES))
        tail = tuple(text[len(text) - depth:])
        longest = max([len(p) for p in PHRASES if len(p) <= len(tail) and tail[len(tail) - len(p):] == p] + [0])
        assert abs(pend - (depth - longest)) <= 1e-12
        for c in (1, 2, 3):
            assert abs(graph.score(text + (c,))[0] - G - float(graph.arc[s][c])) <= 1e-12
    assert (graph.next[:, 0] == np.arange(graph.n_states)).all() and (graph.arc[:, 0] == 0).all()
    assert np.isfinite(graph.arc).all()
    twice = CharGraph.hotwords(PHRASES + [(1, 2)], bonus, 4)     # a phrase given twice counts once
    assert np.array_equal(twice.arc, graph.arc) and np.array_equal(twice.next, graph.next)
    for bad in ([], [()], [(0, 1)], [(4,)], [(1, -1)]):
        with pytest.raises(ValueError, match='hotwords'):
            CharGraph.hotwords(bad, 1.0, 4)
    with pytest.raises(ValueError, match='bonus'):
        CharGraph.hotwords(PHRASES, math.inf, 4)
    with pytest.raises(ValueError, match='blank'):
        CharGraph.hotwords(PHRASES, 1.0, 4, blank=4)


def ngram_counts(seqs, order, eos):
    """{history: {class: count}} straight from the definition."""
    follow = {}
    for seq in seqs:
        seq = tuple(seq) + (eos,)
        for i in range(len(seq)):
            for n in range(order):
                if i - n >= 0:
                    follow.setdefault(seq[i - n:i], {}).setdefault(seq[i], 0)
                    follow[seq[i - n:i]][seq[i]] += 1
    return follow


def witten_bell(follow, h, c, V, blank=0):
    """P(c | h) by the recursion, in float64, an unseen history backing off."""
    lower = witten_bell(follow, h[1:], c, V, blank) if h else (0.0 if c == blank else 1.0 / (V - 1))
    row = follow.get(h)
    if not row:
        return lower
    return (row.get(c, 0) + len(row) * lower) / (sum(row.values()) + len(row))


@pytest.mark.parametrize('order', [1, 2, 3, 4])
def test_the_ngram_graph_is_the_witten_bell_recursion_on_the_golden_text(order):
    seqs, V = golden_sequences()
    assert V == 50 and len(seqs) == 3
    graph = golden_ngram(order)
    follow = ngram_counts(seqs, order, EOS)
    states = sorted(follow, key=lambda h: (len(h), h))
    assert graph.n_states == len(states) and graph.start == 0 and states[0] == ()
    assert graph.n_states > 1 if order > 1 else graph.n_states == 1
    # 1e-6: a float32 log-probability of magnitude < 16 is within 2^-21 = 4.8e-7 of its float64 value, and a sum of
    # probabilities carries that as a relative error
    worst = 0.0
    for i, h in enumerate(states):
        assert abs(np.exp(graph.arc[i, 1:].astype(np.float64)).sum() - 1.0) <= 1e-6
        for c in range(1, V):
            p = witten_bell(follow, h, c, V)
            assert p > 0 and abs(math.log(p)) < 16
            worst = max(worst, abs(float(graph.arc[i, c]) - math.log(p)))
            hc = (h + (c,))[-(order - 1):] if order > 1 else ()
            while hc not in follow:
                hc = hc[1:]
            assert states[graph.next[i, c]] == hc                # the longest seen suffix
        assert graph.next[i, 0] == i and graph.arc[i, 0] == 0.0
        assert graph.fin[i] == graph.arc[i, EOS]
    assert worst <= 1e-6
    # held-out strings, unseen histories among them: score() is the recursion on the last order - 1 labels
    rng = np.random.default_rng(order)
    held = [tuple(int(c) for c in rng.integers(2, V, n)) for n in (1, 2, 5, 9)] + [tuple(seqs[0][3:9]), tuple(seqs[1][:4])]
    unseen = 0
    for text in held:
        want = 0.0
        for i, c in enumerate(text):
            h = text[max(0, i - (order - 1)):i]
            unseen += h not in follow
            want += math.log(witten_bell(follow, h, c, V))
        G, s = graph.score(text)
        assert abs(G - want) <= 1e-6 * max(len(text), 1)
        tail = text[len(text) - (order - 1):] if order > 1 else ()
        while tail not in follow:
            tail = tail[1:]
        assert states[s] == tail
    assert unseen > 0 or order <= 2                             # every class occurs in the text: none unseen at order 2


def test_ngram_rejects_bad_arguments():
    from ss_asr_amd.char_graph import CharGraph
    for bad in (dict(order=0), dict(eos=0), dict(eos=50), dict(blank=50), dict(n_classes=65), dict(n_classes=1),
                dict(sequences=[[2, 50]]), dict(sequences=[[2, 0]]), dict(sequences=[[2, 1]])):
        args = dict(sequences=[[2, 3]], order=2, n_classes=50, eos=1, blank=0)
        args.update(bad)
        with pytest.raises(ValueError, match='ngram'):
            CharGraph.ngram(**args)
    empty = CharGraph.ngram([], 3, 4, 1)                        # no data: the uniform distribution
    assert empty.n_states == 1 and np.allclose(np.exp(empty.arc[0, 1:]), 1 / 3)


def test_the_product_adds_the_scores_on_every_text():
    from ss_asr_amd.char_graph import CharGraph
    V = 4
    a = random_graph(5, V, 1, forbid=0.15)
    b = CharGraph.hotwords(PHRASES, 0.5, V)
    prod = CharGraph.product(a.scaled(0.5), b)
    assert prod.n_states <= a.n_states * b.n_states and prod.start == 0
    finite = 0
    for text in texts_up_to((1, 2, 3), 5):
        (ga, sa), (gb, sb), (gp, sp) = walk(a, text), walk(b, text), walk(prod, text)
        want = 0.5 * ga + gb if ga > NEG else NEG
        if want == NEG:
            assert gp == NEG
            continue
        finite += 1
        assert abs(gp - want) <= 1e-5                            # the factors' and the product's tables are float32
        assert abs(float(prod.fin[sp]) - (0.5 * float(a.fin[sa]) + float(b.fin[sb]))) <= 1e-6
    assert finite > 50
    assert (prod.next[:, 0] == np.arange(prod.n_states)).all() and (prod.arc[:, 0] == 0).all()
    with pytest.raises(ValueError, match='max_states'):
        CharGraph.product(a, b, max_states=3)
    with pytest.raises(ValueError, match='classes'):
        CharGraph.product(a, random_graph(3, 5, 0))
    for bad in (-1.0, math.inf, math.nan):
        with pytest.raises(ValueError, match='scaled'):
            a.scaled(bad)
    assert np.array_equal(np.isneginf(a.scaled(0.0).arc), np.isneginf(a.arc))


def test_chargraph_validates_and_round_trips(tmp_path):
    from ss_asr_amd.char_graph import CharGraph
    g = random_graph(7, 8, 0)
    path = os.path.join(str(tmp_path), 'g.npz')
    g.save(path)
    back = CharGraph.load(path)
    assert back.start == g.start == 6 and back.next.dtype == np.int32 and back.arc.dtype == np.float32
    for name in ('next', 'arc', 'fin'):
        assert np.array_equal(getattr(back, name), getattr(g, name))
    assert back.score((1, 2, 3)) == g.score((1, 2, 3)) == walk(g, (1, 2, 3))
    np.savez(os.path.join(str(tmp_path), 'short.npz'), next=g.next, arc=g.arc)
    with pytest.raises(ValueError, match='lacks'):
        CharGraph.load(os.path.join(str(tmp_path), 'short.npz'))
    with pytest.raises(ValueError, match='no class'):
        g.score((8,))
    nxt, arc, fin = np.zeros((2, 3), dtype=np.int64), np.zeros((2, 3)), np.zeros(2)

    def changed(a, index, value):
        a = a.copy()
        a[index] = value
        return a
    for bad in ((nxt[0], arc, fin), (nxt, arc[:, :2], fin), (nxt, arc, fin[:1]), (nxt[:, :1], arc[:, :1], fin),
                (np.zeros((2, 65), dtype=np.int64), np.zeros((2, 65)), fin), (nxt.astype(np.float64), arc, fin),
                (changed(nxt, (0, 1), 2), arc, fin), (changed(nxt, (1, 0), -1), arc, fin),
                (nxt, changed(arc, (0, 1), math.nan), fin), (nxt, changed(arc, (0, 1), math.inf), fin),
                (nxt, arc.astype(np.int64), fin), (nxt, arc, changed(fin, 0, NEG)), (nxt, arc, changed(fin, 1, math.nan))):
        with pytest.raises(ValueError, match='CharGraph'):
            CharGraph(*bad)
    for start in (-1, 2, 1.0, True):
        with pytest.raises(ValueError, match='start'):
            CharGraph(nxt, arc, fin, start)
    assert CharGraph(nxt, changed(arc, (0, 1), NEG), fin, 1).start == 1     # -inf is an arc


# ---------------------------------------------------------------- C entries ----
def _entry_args(**over):
    from ss_asr_amd import _lib
    lib = _lib.load()
    a = dict(B=2, T=6, V=5, K=3, blank=0, graph_weight=0.5, length_bonus=0.25)
    a.update({k: v for k, v in over.items() if k in a})
    need = int(lib.ssasr_ctc_decode_graph_ws_bytes(2, 6, 5, 3))
    names = ('logits', 'frame_lens', 'chars', 'n_chars', 'scores', 'n_hyps', 'ctc_scores', 'graph_scores', 'next', 'arc',
             'fin')
    bufs = {n: ctypes.create_string_buffer(4096) for n in names}
    ws = ctypes.create_string_buffer(need + 32)
    ptr = {n: ctypes.addressof(b) for n, b in bufs.items()}
    ptr['ws'] = (ctypes.addressof(ws) + 15) & ~15
    for k, v in over.items():
        if k in ptr:
            ptr[k] = v(ptr[k]) if callable(v) else v
    graph = _lib.CharGraph(ptr['next'], ptr['arc'], ptr['fin'], over.get('g_S', 4), over.get('g_V', 5),
                           over.get('g_start', 3))
    g_arg = None if over.get('graph', 1) is None else ctypes.byref(graph)
    keep = (bufs, ws, graph)
    return lib, keep, (ptr['logits'], ptr['frame_lens'], a['B'], a['T'], a['V'], a['K'], a['blank'], ptr['ws'],
                       over.get('ws_bytes', need), ptr['chars'], ptr['n_chars'], ptr['scores'], ptr['n_hyps'], g_arg,
                       a['graph_weight'], a['length_bonus'], ptr['ctc_scores'], ptr['graph_scores'], None)


def test_the_entries_reject_bad_arguments_before_any_hip_call():
    from ss_asr_amd import _lib
    lib = _lib.load()
    assert lib.ssasr_abi_version() == 16 == _lib.ABI_VERSION
    protos, header = header_prototypes()
    assert {'ssasr_ctc_decode_graph', 'ssasr_ctc_decode_graph_ws_bytes'} <= set(protos) & set(_lib.SIGNATURES)
    assert 'typedef struct ssasr_char_graph {' in header
    assert [f[0] for f in _lib.CharGraph._fields_] == ['next', 'arc', 'fin', 'S', 'V', 'start']
    assert ctypes.sizeof(_lib.CharGraph) == 3 * 8 + 3 * 4 + 4
    ws = lib.ssasr_ctc_decode_graph_ws_bytes
    assert ws(2, 6, 5, 3) == 2 * 2 * 3 * 6 * 4 == lib.ssasr_ctc_decode_ws_bytes(2, 6, 5, 3)
    assert ws(1, 4096, 64, 32) > 0 and ws(65535, 1, 2, 1) > 0
    for shape in ((0, 6, 5, 3), (65536, 6, 5, 3), (2, 0, 5, 3), (2, 4097, 5, 3), (2, 6, 1, 3), (2, 6, 65, 3), (2, 6, 5, 0),
                  (2, 6, 5, 33), (2, 6, 5, -1)):
        assert ws(*shape) == 0, shape
    for name in ('logits', 'frame_lens', 'ws', 'chars', 'n_chars', 'scores', 'n_hyps', 'ctc_scores', 'graph_scores',
                 'graph', 'next', 'arc', 'fin'):
        _, keep, args = _entry_args(**{name: None})
        assert lib.ssasr_ctc_decode_graph(*args) == -1, name
    for bad in (dict(B=0), dict(B=65536), dict(T=0), dict(T=4097), dict(V=1), dict(V=65), dict(K=0), dict(K=33), dict(K=-1),
                dict(blank=5), dict(blank=-1), dict(graph_weight=math.inf), dict(graph_weight=math.nan),
                dict(graph_weight=-0.5), dict(length_bonus=-math.inf), dict(length_bonus=math.nan),
                dict(ws=lambda p: p + 4), dict(ws_bytes=ws(2, 6, 5, 3) - 1), dict(g_V=6), dict(g_S=0),
                dict(g_S=(1 << 20) + 1), dict(g_start=4), dict(g_start=-1), dict(graph_weight=0.0, g_V=6)):
        _, keep, args = _entry_args(**bad)
        assert lib.ssasr_ctc_decode_graph(*args) == -1, bad


# ------------------------------------------------------------ Python surface ----
def test_ops_and_decode_ctc_reject_bad_arguments():
    from ss_asr_amd import ops
    from ss_asr_amd.ASRDataset import Mapper
    from ss_asr_amd.charlm import CharLM
    from ss_asr_amd.ctc import JointCTCASR
    z, lens = torch.zeros(1, 4, 5), torch.tensor([4], dtype=torch.int32)
    g = random_graph(3, 5, 0)
    for bad in (0, 33, 2.0, True, None):
        with pytest.raises(ValueError, match='beam_size'):
            ops.ctc_decode_graph(z, lens, bad, g, 0.5)
    for gw, lb in ((math.nan, 0.0), (-0.5, 0.0), (0.5, math.inf)):
        with pytest.raises(ValueError, match='finite'):
            ops.ctc_decode_graph(z, lens, 2, g, gw, lb)
    with pytest.raises(ValueError, match='needs a graph'):
        ops.ctc_decode_graph(z, lens, 2, None, 0.5)
    with pytest.raises(TypeError, match='CharGraph'):
        ops.ctc_decode_graph(z, lens, 2, (g.next, g.arc, g.fin), 0.5)
    with pytest.raises(ValueError, match=r'\[B, T, V\]'):
        ops.ctc_decode_graph(z[0], lens, 2, g, 0.5)
    with pytest.raises(TypeError, match='frame_lens'):
        ops.ctc_decode_graph(z, lens.long(), 2, g, 0.5)
    with pytest.raises(ValueError, match='blank'):
        ops.ctc_decode_graph(z, lens, 2, g, 0.5, blank=5)
    with pytest.raises(ValueError, match='classes'):
        ops.ctc_decode_graph(z, lens, 2, random_graph(3, 6, 0), 0.5)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.ctc_decode_graph(z, lens, 2, g, 0.5)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.ctc_head_decode_graph(torch.zeros(1, 4, 8), torch.zeros(5, 8), torch.zeros(5), lens, 2, g, 0.5)
    joint = JointCTCASR(50, 32, 32, 16, 12, 1.0)
    g50 = random_graph(3, 50, 0)
    one = ([torch.zeros(1, 16, 12)], [[16]], Mapper())
    for bad in (math.nan, math.inf, -0.5, '1', None, True):
        with pytest.raises(ValueError, match='graph_weight'):
            joint.decode_ctc(*one, graph=g50, graph_weight=bad)
    with pytest.raises(ValueError, match='needs graph'):
        joint.decode_ctc(*one, graph_weight=0.5)
    with pytest.raises(ValueError, match='CharGraph'):
        joint.decode_ctc(*one, graph=(1, 2), graph_weight=0.5)
    with pytest.raises(ValueError, match='best path'):
        joint.decode_ctc(*one, beam_size=0, graph=g50, graph_weight=0.5)
    with pytest.raises(ValueError, match='not built'):
        joint.decode_ctc(*one, graph=g50, graph_weight=0.5, rnn_lm=CharLM(50, 8), lm_weight=0.5)
    with pytest.raises(ValueError, match='classes'):
        joint.decode_ctc(*one, graph=g, graph_weight=0.5)
    with pytest.raises(RuntimeError, match='no CPU path|GPU'):
        joint.decode_ctc(*one, graph=g50, graph_weight=0.5, length_bonus=0.1)
    assert joint.last_ctc_decode is None and joint.last_hyps is None


def test_tester_validates_the_graph_keys_of_decode_ctc_only(tmp_path):
    from test_ctc_search_cpu import _tester
    from ss_asr_amd.ASRDataset import Mapper
    from ss_asr_amd.char_graph import CharGraph
    from ss_asr_amd.trainer import ASRTester
    beam, keys = ASRTester.ctc_only_beam, ASRTester.ctc_only_graph
    assert keys({}) is None and keys({'decode_ctc_only': True}) is None
    assert keys({'decode_ctc_only': {'beam_size': 4, 'lm_weight': 0.5}}) is None
    conf = {'decode_ctc_only': {'beam_size': 4, 'hotwords': ['ab', 'c d'], 'length_bonus': 0.25}}
    assert beam(conf) == 4
    assert keys(conf) == {'hotwords': ['ab', 'c d'], 'hotword_bonus': 1.0, 'ngram_lm': None, 'ngram_weight': 0.5}
    both = {'decode_ctc_only': {'hotwords': ['ab'], 'hotword_bonus': 2, 'ngram_lm': 'lm.npz', 'ngram_weight': 0.25}}
    assert keys(both) == {'hotwords': ['ab'], 'hotword_bonus': 2.0, 'ngram_lm': 'lm.npz', 'ngram_weight': 0.25}
    for bad in ({'hotwords': []}, {'hotwords': 'ab'}, {'hotwords': ['ab', '']}, {'hotwords': [1]}, {'ngram_lm': 3},
                {'ngram_lm': ''}, {'hotword_bonus': 1.0}, {'ngram_weight': 0.5}, {'hotwords': ['a'], 'ngram_weight': 0.5},
                {'ngram_lm': 'x.npz', 'hotword_bonus': 1.0}):
        with pytest.raises(ValueError, match='decode_ctc_only'):
            keys({'decode_ctc_only': bad})
    for key, need in (('hotword_bonus', {'hotwords': ['a']}), ('ngram_weight', {'ngram_lm': 'x.npz'})):
        for bad in (math.nan, math.inf, -1, '1', None, True, [1]):
            with pytest.raises(ValueError, match=r'decode_ctc_only\.' + key):
                keys({'decode_ctc_only': dict(need, **{key: bad})})
    with pytest.raises(ValueError, match='best path'):
        keys({'decode_ctc_only': {'beam_size': 0, 'hotwords': ['a']}})
    with pytest.raises(ValueError, match='decode_rescore'):
        keys({'decode_ctc_only': {'hotwords': ['a']}, 'decode_rescore': True})
    with pytest.raises(ValueError, match='not built'):
        keys({'decode_ctc_only': {'hotwords': ['a'], 'lm_weight': 0.5}})
    with pytest.raises(ValueError, match='decode_ctc_only'):
        beam({'decode_ctc_only': {'beam_size': 4, 'hotword': ['a']}})
    # set_model validates everything, the files and the characters included
    root = str(tmp_path)
    mapper = Mapper()
    V = mapper.get_dim()

    def model_error(match, **ctc_only):
        t = _tester(root, {'ctc_weight': 0.3}, decode_ctc_only=dict({'beam_size': 4}, **ctc_only))
        t.mapper = mapper
        with pytest.raises(ValueError, match=match):
            t.set_model()
    model_error(r'hotwords.*no character', hotwords=['a#'])
    model_error(r'ngram_lm: no file', ngram_lm=os.path.join(root, 'none.npz'))
    small = os.path.join(root, 'small.npz')
    random_graph(3, 8, 0).save(small)
    model_error(r'ngram_lm: the graph has 8 classes', ngram_lm=small)
    t = _tester(root, {}, decode_ctc_only={'beam_size': 4, 'hotwords': ['ab']})
    t.mapper = mapper
    with pytest.raises(ValueError, match=r'asr\.decode_ctc_only.*ctc_weight'):
        t.set_model()
    # what set_model builds: the hotwords at weight 1, the n-gram at its weight, both as the product at weight 1
    good = os.path.join(root, 'lm.npz')
    lm = CharGraph.ngram([[mapper.char_to_ind(c) for c in 'abcab']], 2, V, mapper.char_to_ind('>'))
    lm.save(good)
    t = _tester(root, {'ctc_weight': 0.3})
    t.mapper = mapper
    ab = [mapper.char_to_ind(c) for c in 'ab']
    hot, w = t.build_ctc_graph(keys({'decode_ctc_only': {'hotwords': ['ab'], 'hotword_bonus': 2}}))
    assert w == 1.0 and hot.n_states == 3 and abs(hot.score(ab)[0] - 4.0) <= 1e-6
    only, w = t.build_ctc_graph(keys({'decode_ctc_only': {'ngram_lm': good, 'ngram_weight': 0.25}}))
    assert w == 0.25 and np.array_equal(only.arc, lm.arc)
    prod, w = t.build_ctc_graph(keys({'decode_ctc_only': {'hotwords': ['ab'], 'hotword_bonus': 2, 'ngram_lm': good,
                                                          'ngram_weight': 0.25}}))
    assert w == 1.0 and abs(prod.score(ab)[0] - (0.25 * lm.score(ab)[0] + 4.0)) <= 1e-5
