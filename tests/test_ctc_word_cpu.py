"""CTC decoding over a lexicon with a word n-gram LM in the search, without a GPU: word_graph.WordGraph (the trie with
its lookahead, the Witten-Bell word LM in back-off form, the expansion into a dense CharGraph) checked against the
recursion evaluated directly from the counts and against walks that share nothing with it;
postprocess.ctc_prefix_beam_word_reference, the float64 restatement of ssasr_ctc_decode_word (include/ssasr.h) that
test_gpu_ctc_word.py holds the kernel to, checked against the sum over every frame labelling, the expanded graph in
ctc_prefix_beam_graph_reference and hand-built tables; and the argument errors of the C entries, ops, ASR.decode_ctc
and ASRTester's asr.decode_ctc_only keys."""
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
A, B, SP = 1, 2, 3                                               # V = 4: blank, a, b, space
SPELL = {'a': [A], 'ab': [A, B], 'b': [B]}
SENTENCES = [['a', 'b'], ['ab', 'a', 'a'], ['b'], ['a', 'ab'], ['a', 'b', 'a']]


def tiny(order=2, **kw):
    from ss_asr_amd.word_graph import WordGraph
    return WordGraph.build(SENTENCES, order, SPELL.__getitem__, 4, SP, **kw)


def random_corpus(n_words, n_sentences, seed):
    """Words w0 .. over the letters 1 .. 6 (distinct spellings of 1-4 letters), random sentences of 1-6 words drawn
    with a skew, so that some n-grams repeat and some words are never seen."""
    rng = np.random.default_rng([n_words, n_sentences, seed])
    spell = {}
    while len(spell) < n_words:
        s = tuple(rng.integers(1, 7, rng.integers(1, 5)).tolist())
        spell.setdefault(s, 'w%d' % len(spell))
    spell = {w: list(s) for s, w in spell.items()}
    words = sorted(spell)
    p = 1.0 / np.arange(1, n_words + 1)
    sents = [[words[i] for i in rng.choice(n_words, rng.integers(1, 7), p=p / p.sum())] for _ in range(n_sentences)]
    return words, spell, sents


def golden_words():
    """(the golden text's words, a spelling over V = 64 classes with the space 2 and the letters 3 ..)"""
    text = open(TEXT, encoding='utf-8').read().strip('\n')
    letters = sorted(set(text) - {' '})
    code = {ch: 3 + i for i, ch in enumerate(letters)}
    return [w for w in text.split(' ') if w], lambda w: [code[ch] for ch in w]


def direct_wb(sentences, words, order):
    """P(w | h) by the Witten-Bell recursion straight from the counts, float64; `None` stands for </s>."""
    count = {}
    for s in sentences:
        seq = tuple(s) + (None,)
        for i in range(len(seq)):
            for n in range(min(i, order - 1) + 1):
                count.setdefault(seq[i - n:i], {}).setdefault(seq[i], 0)
                count[seq[i - n:i]][seq[i]] += 1

    def p(w, h):
        h = tuple(h)[-(order - 1):] if order > 1 else ()
        while h and h not in count:                             # an unseen history is no state: its suffix is used
            h = h[1:]
        row = count.get(h, {})
        total, distinct = sum(row.values()), len(row)
        lower = p(w, h[1:]) if h else 1.0 / (len(words) + 1)
        return (row.get(w, 0) + distinct * lower) / (total + distinct) if total else lower
    return p


def own_walk(g, text):
    """(G, (n, h), fin) by a walk over the tables with a linear scan of the rows: shares nothing with WordGraph."""
    def look(h, w):
        acc = 0.0
        while True:
            for e in range(g.off[h], g.off[h + 1]):
                if g.wid[e] == w:
                    return acc + float(g.wlp[e]), int(g.wnext[e])
            acc, h = acc + float(g.bow[h]), int(g.bnext[h])

    def space(n, h):
        lp, h2 = look(h, int(g.word[n]))
        return float(np.float32(float(g.pen[n]) + lp)), h2
    n, h, total = 0, 0, 0.0
    for c in text:
        if c == g.space:
            if g.word[n] < 0:
                return NEG, None, None
            arc, h = space(n, h)
            total, n = total + arc, 0
        else:
            if g.carc[n, c] == NEG:
                return NEG, None, None
            total, n = total + float(g.carc[n, c]), int(g.child[n, c])
    if g.word[n] < 0:
        return total, (n, h), float(g.pen[n]) + float(g.eos[h])
    arc, h2 = space(n, h)
    return total, (n, h), arc + float(g.eos[h2])


def texts_up_to(classes, n):
    return [t for k in range(n + 1) for t in itertools.product(classes, repeat=k)]


# ------------------------------------------------------------------ the checker ----
def test_zero_weights_are_the_plain_checker_exactly():
    from ss_asr_amd.postprocess import ctc_prefix_beam_reference, ctc_prefix_beam_word_reference
    for T, V, K, seed in ((1, 4, 3, 0), (5, 4, 2, 1), (20, 4, 8, 2), (20, 40, 3, 3)):
        lp = log_softmax64(4.0 * np.random.default_rng([T, V, seed]).standard_normal((T, V)))
        for graph in (None, tiny()):
            tr_a, tr_b, parts = [], [], []
            got, gap = ctc_prefix_beam_word_reference(lp, K, graph, 0.0, 0.0, trace=tr_a, parts=parts)
            want, plain_gap = ctc_prefix_beam_reference(lp, K, trace=tr_b)
            assert got == want and tr_a == tr_b
            assert [p[0] for p in parts] == [s for _, s in want] and all(p[1] == 0.0 for p in parts)
            final = min([math.inf] + [a[1] - b[1] for a, b in zip(want, want[1:])])
            assert gap == min(plain_gap, final)
        lp32 = lp.astype(np.float32)
        assert ctc_prefix_beam_word_reference(lp32, K, None, dtype=np.float32)[0] == \
            ctc_prefix_beam_reference(lp32, K, dtype=np.float32)[0]


@pytest.mark.parametrize('T', [1, 2, 3, 4])
@pytest.mark.parametrize('order', [1, 2, 3])
def test_a_beam_that_drops_nothing_scores_every_text_as_the_enumeration_plus_the_graph(T, order):
    from ss_asr_amd.postprocess import ctc_prefix_beam_word_reference
    gw, beta = 0.5, 0.3
    lp = log_softmax64(np.random.default_rng([T, order, 9]).standard_normal((T, 4)) * 2.0)
    g = tiny(order)
    every = {t: s for t, s in brute_force(lp, 0).items() if own_walk(g, t)[0] > NEG}     # the lexicon's texts
    parts = []
    got, gap = ctc_prefix_beam_word_reference(lp, 32, g, gw, beta, parts=parts)
    assert len(every) <= 32 and {t for t, _ in got} == set(every)
    g32, b32 = float(np.float32(gw)), float(np.float32(beta))
    for (text, total), (ctc, part) in zip(got, parts):
        G, _, fin = own_walk(g, text)
        assert abs(ctc - every[text]) <= 1e-12
        assert abs(part - (G + fin)) <= 1e-12
        assert abs(total - (every[text] + g32 * (G + fin) + b32 * len(text))) <= 1e-12
    assert [s for _, s in got] == sorted((s for _, s in got), reverse=True)


def test_the_word_lm_flips_the_winner_and_the_lexicon_removes_the_plain_winner():
    from ss_asr_amd.postprocess import ctc_prefix_beam_reference, ctc_prefix_beam_word_reference
    from ss_asr_amd.word_graph import WordGraph
    # two words 'a' and 'b'; 'a' is 9 times as frequent.  One frame where the head prefers b by log(0.5 / 0.4).
    g = WordGraph.build([['a']] * 9 + [['b']], 1, SPELL.__getitem__, 4, SP, lexicon=['a', 'b'], lookahead=False)
    lp = np.log(np.array([[0.05, 0.4, 0.5, 0.05]]))
    assert ctc_prefix_beam_reference(lp, 4)[0][0][0] == (B,)
    parts = []
    got, _ = ctc_prefix_beam_word_reference(lp, 4, g, 1.0, parts=parts)
    assert got[0][0] == (A,) and {t for t, _ in got} == {(), (A,), (B,)}          # a lone space is no text
    # unigram Witten-Bell: c = 9, 1, </s> 10; N1+ = 3; uniform 1/3
    p_a, p_b, p_end = (9 + 1) / 23, (1 + 1) / 23, (10 + 1) / 23
    want = {(A,): math.log(0.4) + math.log(p_a) + math.log(p_end), (B,): math.log(0.5) + math.log(p_b) + math.log(p_end),
            (): math.log(0.05) + math.log(p_end)}
    for text, total in got:
        assert abs(total - want[text]) <= 1e-6
    assert ctc_prefix_beam_word_reference(lp, 4, g, 0.1)[0][0][0] == (B,)         # a tenth of the weight does not pay
    # the lexicon {a, ab}: the plain search's first text 'ba' is no text of it
    lex = WordGraph.build([['a', 'ab']], 2, SPELL.__getitem__, 4, SP, lexicon=['a', 'ab'])
    lp = log_softmax64(np.array([[0.0, 1.0, 3.0, 0.0], [0.0, 3.5, 1.0, 0.0], [2.0, 0.0, 0.0, 0.0]]))
    assert ctc_prefix_beam_reference(lp, 4)[0][0][0] == (B, A)
    trace = []
    got, _ = ctc_prefix_beam_word_reference(lp, 4, lex, 1.0, trace=trace)
    assert got and all(t[:1] != (B,) for beam in trace for t in beam) and (B, A) not in {t for t, _ in got}
    with pytest.raises(ValueError, match='>= 0'):
        ctc_prefix_beam_word_reference(lp, 3, lex, -1.0)
    for bad in (dict(K=0), dict(graph=None), dict(graph_weight=math.inf), dict(length_bonus=math.nan)):
        args = dict(K=2, graph=lex, graph_weight=0.5, length_bonus=0.0)
        args.update(bad)
        with pytest.raises(ValueError):
            ctc_prefix_beam_word_reference(lp, args['K'], args['graph'], args['graph_weight'], args['length_bonus'])
    with pytest.raises(ValueError, match='classes'):
        ctc_prefix_beam_word_reference(np.log(np.full((1, 5), 0.2)), 2, lex, 0.5)
    with pytest.raises(ValueError, match='blank'):
        ctc_prefix_beam_word_reference(lp, 2, lex, 0.5, blank=SP)


@pytest.mark.parametrize('order', [1, 2, 3])
def test_the_expanded_graph_has_the_walks_g_and_fin_and_gives_the_same_search(order):
    from ss_asr_amd.postprocess import ctc_prefix_beam_graph_reference, ctc_prefix_beam_word_reference
    g = tiny(order)
    dense = g.to_char_graph()
    for text in texts_up_to((A, B, SP), 6):
        G, state, fin = own_walk(g, text)
        mine, at = g.score(text)
        assert mine == G
        if G == NEG:
            assert dense.score(text)[0] == NEG
            continue
        assert at == state and g.fin(*at) == fin
        dG, ds = dense.score(text)
        assert abs(dG - G) <= 1e-12 and float(dense.fin[ds]) == float(np.float32(fin))
    with pytest.raises(ValueError, match='max_states'):
        g.to_char_graph(max_states=2)
    compared = 0
    for seed in range(12):
        T, K = (3, 5, 12)[seed % 3], (1, 3, 8)[seed // 4]
        lp = log_softmax64(3.0 * np.random.default_rng([order, seed, 4]).standard_normal((T, 4)))
        pw, pd = [], []
        want, gap = ctc_prefix_beam_word_reference(lp, K, g, 0.5, 0.3, parts=pw)
        got, _ = ctc_prefix_beam_graph_reference(lp, K, dense, 0.5, 0.3, parts=pd)
        if gap < 1e-5:                                           # fin is rounded to float32 in the dense table
            continue
        compared += 1
        assert [t for t, _ in got] == [t for t, _ in want]
        assert all(abs(a[1] - b[1]) <= 2e-6 for a, b in zip(got, want))
        assert all(x[0] == y[0] and abs(x[1] - y[1]) <= 4e-6 for x, y in zip(pd, pw))
    assert compared >= 10


# -------------------------------------------------------------------- the builder ----
def corpora():
    words, spell, sents = random_corpus(12, 40, 0)
    yield 'random', words + ['extra'], dict(spell, extra=[6, 6, 6, 6, 6]).__getitem__, sents, 8, 7
    gw, enc = golden_words()
    yield 'golden', sorted(set(gw)), enc, [gw], 64, 2


@pytest.mark.parametrize('order', [1, 2, 3])
def test_witten_bell_and_the_normalisation_in_every_state(order):
    from ss_asr_amd.word_graph import WordGraph
    for name, words, encode, sents, V, space in corpora():
        g = WordGraph.build(sents, order, encode, V, space, lexicon=words)
        p = direct_wb(sents, words, order)
        W = len(words)
        assert g.n_words == W and g.off[1] == W
        hist = {0: ()}                                           # state -> its history, found through wnext
        frontier = [0]
        while frontier:
            h = frontier.pop()
            for e in range(g.off[h], g.off[h + 1]):
                to = int(g.wnext[e])
                if to not in hist:                              # the suffix as long as the state's back-off chain
                    hist[to] = (hist[h] + (words[g.wid[e]],))[len(hist[h]) + 1 - _depth(g, to):]
                    frontier.append(to)
        assert len(hist) == g.n_states                           # every state is reached
        for h, past in hist.items():
            total = math.exp(float(g.eos[h]))
            assert abs(total - p(None, past)) <= 1e-6
            for w in range(W):
                lp, _ = g.lookup(h, w)
                assert abs(math.exp(lp) - p(words[w], past)) <= 1e-6, (name, past, words[w])
                total += math.exp(lp)
            assert abs(total - 1.0) <= 1e-6
            for e in range(g.off[h], g.off[h + 1]):              # the stored entries: the full interpolated value
                assert abs(math.exp(float(g.wlp[e])) - p(words[g.wid[e]], past)) <= 1e-6
            if h:
                assert hist[int(g.bnext[h])] == past[1:]


def _depth(g, h):
    n = 0
    while h:
        h, n = int(g.bnext[h]), n + 1
    return n


@pytest.mark.parametrize('lookahead', [True, False])
def test_whole_words_score_the_direct_formula_and_the_rest_is_forbidden_or_unfinished(lookahead):
    from ss_asr_amd.word_graph import WordGraph
    words, spell, sents = random_corpus(12, 40, 1)
    rng = np.random.default_rng(5)
    for order in (1, 2, 3):
        g = WordGraph.build(sents, order, spell.__getitem__, 8, 7, lookahead=lookahead, unfinished=-20.0)
        p = direct_wb(sents, words, order)
        assert (g.pen[0], g.word[0]) == (0.0, -1)
        if not lookahead:
            assert set(np.unique(g.carc)) == {NEG, 0.0}
        for _ in range(30):
            sent = [words[i] for i in rng.integers(0, len(words), rng.integers(1, 5))]
            want = sum(math.log(p(w, sent[:i])) for i, w in enumerate(sent)) + math.log(p(None, sent))
            open_text = [c for i, w in enumerate(sent) for c in ([7] if i else []) + spell[w]]
            # float32 tables: an arc of magnitude <= 32 carries <= 2e-6 of rounding, a text here <= 24 arcs
            for text in (open_text, open_text + [7]):            # the last word open, or closed by a space
                G, state = g.score(text)
                assert abs(G + g.fin(*state) - want) <= 1e-4, (order, sent)
            assert g.score(open_text + [7])[1][0] == 0
            # a text that stops inside a word: `unfinished` beside the history's </s>
            cut = open_text[:-1]
            G, (n, h) = g.score(cut)
            if n and g.word[n] < 0:                              # not the root: a one-letter word cut leaves a space
                done = sent[:-1]
                base = sum(math.log(p(w, done[:i])) for i, w in enumerate(done)) + math.log(p(None, done))
                assert abs(G + g.fin(n, h) - (base - 20.0)) <= 1e-4
        # forbidden: a space at the root, a doubled space, a space inside a word, a letter outside the lexicon
        first = spell[words[0]]
        assert g.score([7])[0] == NEG and g.score(first + [7, 7])[0] == NEG
        inner = next(spell[w][:k] for w in words for k in range(1, len(spell[w]))
                     if tuple(spell[w][:k]) not in {tuple(s) for s in spell.values()})
        assert g.score(inner + [7])[0] == NEG
        assert g.score(first + [7] + [6, 6, 6, 6, 6])[0] == NEG


def test_save_load_and_every_validation_error(tmp_path):
    from ss_asr_amd.word_graph import TABLES, WordGraph
    g = tiny(3)
    path = os.path.join(str(tmp_path), 'wg.npz')
    g.save(path)
    back = WordGraph.load(path)
    for k in TABLES:
        assert np.array_equal(getattr(back, k), getattr(g, k)) and getattr(back, k).dtype == getattr(g, k).dtype
    assert (back.space, back.blank, back.n_classes, back.n_words) == (SP, 0, 4, 3)
    np.savez(path, child=g.child)
    with pytest.raises(ValueError, match='lacks'):
        WordGraph.load(path)
    good = {k: getattr(g, k).copy() for k in TABLES}

    def bad(match, space=SP, blank=0, **change):
        t = dict(good)
        for k, v in change.items():
            t[k] = v(t[k].copy()) if callable(v) else v
        with pytest.raises(ValueError, match=match):
            WordGraph(*[t[k] for k in TABLES], space, blank)

    def put(index, value):
        def f(a):
            a[index] = value
            return a
        return f
    word_end = int(np.nonzero(g.word >= 0)[0][0])
    bad('integers', child=good['child'].astype(np.float32))
    bad('floats', carc=np.zeros(good['carc'].shape, dtype=np.int32))
    bad(r'\[N, V\]', carc=good['carc'][:, :3])
    bad(r'\[N, V\]', pen=good['pen'][:-1])
    bad('2 <= V', child=np.zeros((2, 65), dtype=np.int32), carc=np.zeros((2, 65), dtype=np.float32),
        word=np.full(2, -1), pen=np.zeros(2, dtype=np.float32))
    bad('space', space=4)
    bad('space', space=True)
    bad('blank', blank=-1)
    bad('is the blank', space=0)
    bad(r'\[H \+ 1\]', bow=good['bow'][:-1])
    bad(r'\[E\]', wlp=good['wlp'][:-1])
    bad('rise from 0', off=put(0, 1))
    bad('rise from 0', off=put(-1, g.n_entries - 1))
    bad('rise from 0', off=put(2, 0))
    bad('dense', wid=put(1, 2))
    bad(r'wid must lie', wid=put(g.n_entries - 1, 3))
    bad('ascending', wid=put(slice(int(g.off[1]), int(g.off[2])), 0)) if g.off[2] - g.off[1] > 1 else None
    bad('wnext', wnext=put(0, g.n_states))
    bad('wnext', wnext=put(0, -1))
    for k in ('pen', 'wlp', 'bow', 'eos'):
        bad(k + ' must be finite', **{k: put(0, math.nan)})
        bad(k + ' must be finite', **{k: put(0, NEG)})
    bad('NaN or', carc=put((0, A), math.nan))
    bad('NaN or', carc=put((0, A), math.inf))
    bad('child must lie', child=put((0, A), g.n_nodes))
    bad('child must lie', child=put((0, A), -1))
    bad(r'word\[0\]', word=put(0, 0))
    bad(r'word must lie', word=put(word_end, 3))
    bad(r'word must lie', word=put(word_end, -2))
    bad('bnext', bnext=put(0, 0))
    bad('bnext', bnext=put(1, -1))
    bad('bnext', bnext=put(1, g.n_states))
    bad('does not reach', bnext=put(1, 1))
    # the unread columns may hold anything
    WordGraph(*[put((0, SP), 99)(good[k].copy()) if k == 'child' else good[k] for k in TABLES], SP, 0)
    # the builder's own errors
    for kw, match in ((dict(order=0), 'order'), (dict(order=9), 'order'), (dict(space=0), 'two classes'),
                      (dict(space=4), 'two classes'), (dict(n_classes=65), 'two classes'), (dict(unfinished=NEG), 'unfinished'),
                      (dict(lexicon=[]), 'lexicon'), (dict(lexicon=['a', 'a', 'b', 'ab']), 'lexicon'),
                      (dict(lexicon=['a', 'b']), 'not in the lexicon'),
                      (dict(encode={'a': [A], 'ab': [A], 'b': [B]}.__getitem__), 'share a spelling'),
                      (dict(encode={'a': [A], 'ab': [], 'b': [B]}.__getitem__), 'spelled'),
                      (dict(encode={'a': [A], 'ab': [A, SP], 'b': [B]}.__getitem__), 'spelled'),
                      (dict(encode={'a': [A], 'ab': [A, 0], 'b': [B]}.__getitem__), 'spelled')):
        args = dict(sentences=SENTENCES, order=2, encode=SPELL.__getitem__, n_classes=4, space=SP)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            WordGraph.build(**args)
    with pytest.raises(ValueError, match='no non-blank class'):
        g.score([0])


# ---------------------------------------------------------------- C entries ----
def _entry_args(**over):
    from ss_asr_amd import _lib
    lib = _lib.load()
    a = dict(B=2, T=6, V=5, K=3, blank=0, graph_weight=0.5, length_bonus=0.25)
    a.update({k: v for k, v in over.items() if k in a})
    need = int(lib.ssasr_ctc_decode_word_ws_bytes(2, 6, 5, 3))
    names = ('logits', 'frame_lens', 'chars', 'n_chars', 'scores', 'n_hyps', 'ctc_scores', 'graph_scores') + \
        _lib.WORD_GRAPH_TABLES
    bufs = {n: ctypes.create_string_buffer(4096) for n in names}
    ws = ctypes.create_string_buffer(need + 32)
    ptr = {n: ctypes.addressof(b) for n, b in bufs.items()}
    ptr['ws'] = (ctypes.addressof(ws) + 15) & ~15
    for k, v in over.items():
        if k in ptr:
            ptr[k] = v(ptr[k]) if callable(v) else v
    dims = dict(N=4, V=5, H=3, W=2, E=4, sp=4)
    dims.update({k[2:]: v for k, v in over.items() if k.startswith('g_')})
    graph = _lib.WordGraph(*[ptr[n] for n in _lib.WORD_GRAPH_TABLES], *[dims[n] for n in ('N', 'V', 'H', 'W', 'E', 'sp')])
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
    assert {'ssasr_ctc_decode_word', 'ssasr_ctc_decode_word_ws_bytes'} <= set(protos) & set(_lib.SIGNATURES)
    assert protos['ssasr_ctc_decode_word'][1][:13] == protos['ssasr_ctc_decode_graph'][1][:13]
    assert protos['ssasr_ctc_decode_word'][1][14:] == protos['ssasr_ctc_decode_graph'][1][14:]
    assert 'typedef struct ssasr_word_graph {' in header and '#define SSASR_WORD_MAX_ORDER 8' in header
    assert [f[0] for f in _lib.WordGraph._fields_] == list(_lib.WORD_GRAPH_TABLES) + ['N', 'V', 'H', 'W', 'E', 'sp']
    assert ctypes.sizeof(_lib.WordGraph) == 11 * 8 + 6 * 4
    from ss_asr_amd.word_graph import TABLES
    assert TABLES == _lib.WORD_GRAPH_TABLES                      # WordGraph.to fills the struct in this order
    ws = lib.ssasr_ctc_decode_word_ws_bytes
    assert ws(2, 6, 5, 3) == 2 * 2 * 3 * 6 * 4 == lib.ssasr_ctc_decode_ws_bytes(2, 6, 5, 3)
    assert ws(1, 4096, 64, 32) > 0 and ws(65535, 1, 2, 1) > 0
    for shape in ((0, 6, 5, 3), (65536, 6, 5, 3), (2, 0, 5, 3), (2, 4097, 5, 3), (2, 6, 1, 3), (2, 6, 65, 3), (2, 6, 5, 0),
                  (2, 6, 5, 33), (2, 6, 5, -1)):
        assert ws(*shape) == 0, shape
    for name in ('logits', 'frame_lens', 'ws', 'chars', 'n_chars', 'scores', 'n_hyps', 'ctc_scores', 'graph_scores',
                 'graph') + _lib.WORD_GRAPH_TABLES:
        _, keep, args = _entry_args(**{name: None})
        assert lib.ssasr_ctc_decode_word(*args) == -1, name
    big = (1 << 20) + 1
    for bad in (dict(B=0), dict(B=65536), dict(T=0), dict(T=4097), dict(V=1), dict(V=65), dict(K=0), dict(K=33), dict(K=-1),
                dict(blank=5), dict(blank=-1), dict(graph_weight=math.inf), dict(graph_weight=math.nan),
                dict(graph_weight=-0.5), dict(length_bonus=-math.inf), dict(length_bonus=math.nan),
                dict(ws=lambda p: p + 4), dict(ws_bytes=ws(2, 6, 5, 3) - 1), dict(g_V=6), dict(g_sp=5), dict(g_sp=-1),
                dict(g_sp=0), dict(blank=4), dict(g_N=0), dict(g_N=big), dict(g_H=0), dict(g_H=big), dict(g_W=0),
                dict(g_W=big), dict(g_E=1), dict(g_E=-1), dict(graph_weight=0.0, g_V=6)):
        _, keep, args = _entry_args(**bad)
        assert lib.ssasr_ctc_decode_word(*args) == -1, bad


# ------------------------------------------------------------ Python surface ----
def test_ops_and_decode_ctc_reject_bad_arguments():
    from test_ctc_graph_cpu import random_graph
    from ss_asr_amd import ops
    from ss_asr_amd.ASRDataset import Mapper
    from ss_asr_amd.charlm import CharLM
    from ss_asr_amd.ctc import JointCTCASR
    from ss_asr_amd.word_graph import WordGraph
    z, lens = torch.zeros(1, 4, 4), torch.tensor([4], dtype=torch.int32)
    g = tiny()
    for bad in (0, 33, 2.0, True, None):
        with pytest.raises(ValueError, match='beam_size'):
            ops.ctc_decode_word(z, lens, bad, g, 0.5)
    for gw, lb in ((math.nan, 0.0), (-0.5, 0.0), (0.5, math.inf)):
        with pytest.raises(ValueError, match='finite'):
            ops.ctc_decode_word(z, lens, 2, g, gw, lb)
    with pytest.raises(ValueError, match='needs a graph'):
        ops.ctc_decode_word(z, lens, 2, None, 0.5)
    with pytest.raises(TypeError, match='WordGraph'):
        ops.ctc_decode_word(z, lens, 2, random_graph(3, 4, 0), 0.5)
    with pytest.raises(TypeError, match='CharGraph'):
        ops.ctc_decode_graph(z, lens, 2, g, 0.5)
    with pytest.raises(ValueError, match=r'\[B, T, V\]'):
        ops.ctc_decode_word(z[0], lens, 2, g, 0.5)
    with pytest.raises(TypeError, match='frame_lens'):
        ops.ctc_decode_word(z, lens.long(), 2, g, 0.5)
    with pytest.raises(ValueError, match='blank'):
        ops.ctc_decode_word(z, lens, 2, g, 0.5, blank=4)
    with pytest.raises(ValueError, match='is the blank'):
        ops.ctc_decode_word(z, lens, 2, g, 0.5, blank=SP)
    with pytest.raises(ValueError, match='classes'):
        ops.ctc_decode_word(torch.zeros(1, 4, 5), lens, 2, g, 0.5)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.ctc_decode_word(z, lens, 2, g, 0.5)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.ctc_head_decode_word(torch.zeros(1, 4, 8), torch.zeros(4, 8), torch.zeros(4), lens, 2, g, 0.5)
    mapper = Mapper()
    V, space = mapper.get_dim(), mapper.char_to_ind(' ')
    joint = JointCTCASR(V, 32, 32, 16, 12, 1.0)
    wg = WordGraph.build([['ab', 'ba']], 2, lambda w: [mapper.char_to_ind(c) for c in w], V, space)
    one = ([torch.zeros(1, 16, 12)], [[16]], mapper)
    for bad in (math.nan, math.inf, -0.5, '1', None, True):
        with pytest.raises(ValueError, match='graph_weight'):
            joint.decode_ctc(*one, word_graph=wg, graph_weight=bad)
    with pytest.raises(ValueError, match='WordGraph'):
        joint.decode_ctc(*one, word_graph=random_graph(3, V, 0), graph_weight=0.5)
    with pytest.raises(ValueError, match='give one of them'):
        joint.decode_ctc(*one, word_graph=wg, graph=random_graph(3, V, 0), graph_weight=0.5)
    with pytest.raises(ValueError, match='best path'):
        joint.decode_ctc(*one, beam_size=0, word_graph=wg, graph_weight=0.5)
    with pytest.raises(ValueError, match='not built'):
        joint.decode_ctc(*one, word_graph=wg, graph_weight=0.5, rnn_lm=CharLM(V, 8), lm_weight=0.5)
    with pytest.raises(ValueError, match='classes'):
        joint.decode_ctc(*one, word_graph=g, graph_weight=0.5)
    with pytest.raises(RuntimeError, match='no CPU path|GPU'):
        joint.decode_ctc(*one, word_graph=wg, graph_weight=0.5, length_bonus=0.1)
    assert joint.last_ctc_decode is None and joint.last_hyps is None


def test_tester_validates_the_word_keys_of_decode_ctc_only(tmp_path):
    from test_ctc_search_cpu import _tester
    from ss_asr_amd.ASRDataset import Mapper
    from ss_asr_amd.trainer import ASRTester
    from ss_asr_amd.word_graph import WordGraph
    beam, keys = ASRTester.ctc_only_beam, ASRTester.ctc_only_word
    assert keys({}) is None and keys({'decode_ctc_only': True}) is None
    assert keys({'decode_ctc_only': {'beam_size': 4, 'lm_weight': 0.5}}) is None
    conf = {'decode_ctc_only': {'beam_size': 8, 'word_lm': 'file.npz', 'word_lm_weight': 0.5}}
    assert beam(conf) == 8 and keys(conf) == {'word_lm': 'file.npz', 'word_lm_weight': 0.5}
    assert keys({'decode_ctc_only': {'word_lm': 'f.npz', 'length_bonus': 1}}) == {'word_lm': 'f.npz', 'word_lm_weight': 0.5}
    for bad in ({'word_lm_weight': 0.5}, {'word_lm': 3}, {'word_lm': ''}):
        with pytest.raises(ValueError, match=r'decode_ctc_only\.word_lm'):
            keys({'decode_ctc_only': bad})
    for bad in (math.nan, math.inf, -1, '1', None, True, [1]):
        with pytest.raises(ValueError, match=r'decode_ctc_only\.word_lm_weight'):
            keys({'decode_ctc_only': {'word_lm': 'f.npz', 'word_lm_weight': bad}})
    with pytest.raises(ValueError, match='best path'):
        keys({'decode_ctc_only': {'beam_size': 0, 'word_lm': 'f.npz'}})
    for clash in ({'hotwords': ['a']}, {'ngram_lm': 'x.npz'}, {'lm_weight': 0.5}):
        with pytest.raises(ValueError, match='not built'):
            keys({'decode_ctc_only': dict({'word_lm': 'f.npz'}, **clash)})
    with pytest.raises(ValueError, match='decode_rescore'):
        keys({'decode_ctc_only': {'word_lm': 'f.npz'}, 'decode_rescore': True})
    with pytest.raises(ValueError, match='decode_ctc_only'):
        beam({'decode_ctc_only': {'beam_size': 4, 'word_lms': 'f.npz'}})
    root = str(tmp_path)
    mapper = Mapper()
    V, space = mapper.get_dim(), mapper.char_to_ind(' ')

    def model_error(match, **ctc_only):
        t = _tester(root, {'ctc_weight': 0.3}, decode_ctc_only=dict({'beam_size': 4}, **ctc_only))
        t.mapper = mapper
        with pytest.raises(ValueError, match=match):
            t.set_model()
    model_error(r'word_lm: no file', word_lm=os.path.join(root, 'none.npz'))
    small = os.path.join(root, 'small.npz')
    tiny().save(small)
    model_error(r'word_lm: the graph has 4 classes', word_lm=small)
    good = os.path.join(root, 'wg.npz')
    WordGraph.build([['ab', 'ba']], 2, lambda w: [mapper.char_to_ind(c) for c in w], V, space).save(good)
    t = _tester(root, {'ctc_weight': 0.3})
    t.mapper = mapper
    wg, w = t.load_word_graph(keys({'decode_ctc_only': {'word_lm': good, 'word_lm_weight': 0.25}}))
    assert w == 0.25 and wg.n_words == 2 and wg.space == space
