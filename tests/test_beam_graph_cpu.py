"""The attention beam search with a character graph, without a GPU: the float64 checker of tests/graph_beam_checker.py
(what test_gpu_beam_graph.py holds the kernel to) against decode_checker's plain search, its teacher-forced scores, an
independent walk of the graph and enumeration; hand-built graphs; and the surface: ABI 16, the two prototypes, every
argument error of both C entries before any HIP call, the errors of ops.decode_beam_graph, ASR.decode / decode_nbest /
decode_mbr and ASRTester's asr.decode_hotwords / decode_hotword_bonus / decode_ngram_lm / decode_ngram_weight keys."""
import ctypes
import itertools
import math
import os

import numpy as np
import pytest
import torch

import decode_checker as dc
import graph_beam_checker as gbc
from test_ctc_graph_cpu import random_graph
from test_host_cpu import header_prototypes

NEG = -math.inf
EOS = 1
SMALL, FRAMES = 'decode_small_s4', 24


# ------------------------------------------------------------------ the checker ----
def test_weight_zero_is_the_plain_checker_exactly(golden):
    m = dc.model(golden, SMALL, FRAMES)
    w = float(golden(SMALL)['lm_weights'][0])
    for lam, terms in ((0.0, ()), (0.3, (0.1, 1.5, 0.36, 0.0))):
        want = dc.beam_search(m, 3, 12, w, lam, *terms)
        for graph in (None, random_graph(7, m.V, 0)):
            got = gbc.beam_search(gbc.with_graph(m, graph, 0.0), 3, 12, w, lam, *terms)
            assert got.pop('parts') == [0.0] * len(want['hyps']) and got.pop('forbidden') == 0
            assert got == want


@pytest.mark.parametrize('kind', ['random', 'hotwords'])
def test_every_score_is_the_forced_score_plus_the_length_bonus_plus_the_walk(golden, kind):
    from ss_asr_amd.char_graph import CharGraph
    m = dc.model(golden, SMALL, FRAMES)
    w = float(golden(SMALL)['lm_weights'][0])
    gw, beta, S = 0.5, 0.1, 8
    graph = random_graph(7, m.V, 0) if kind == 'random' else CharGraph.hotwords([[5, 6], [5, 6, 7], [30]], 0.75, m.V)
    for lam in (0.0, 0.3):
        r = gbc.beam_search(gbc.with_graph(m, graph, gw), 5, S, w, lam, beta)
        assert len(r['hyps']) >= 3 and len({(tuple(h[0]), h[3]) for h in r['hyps']}) == len(r['hyps'])
        for (text, score, ended, capped, _), part in zip(r['hyps'], r['parts']):
            G, s = graph.score(text)                                 # CharGraph's own walk, not the checker's
            walk = G + (0.0 if capped else float(graph.fin[s]))
            assert abs(part - walk) <= 1e-9
            total = dc.forced(m, text, not capped, lam, w)[0]
            assert abs(score - (total + beta * len(text) + gw * walk)) <= 1e-9, (text, capped)
        assert [h[1] for h in r['hyps']] == sorted((h[1] for h in r['hyps']), reverse=True)


def test_a_beam_that_drops_nothing_is_the_enumerated_arg_sort():
    V, S, gw = 3, 2, 0.5
    texts = [t for n in range(S + 1) for t in itertools.product((0, 2), repeat=n)]
    assert len(texts) == 7
    seen_forbidden = 0
    for seed in range(6):
        graph = random_graph(4, V, seed, forbid=0.25)
        m = gbc.RowModel(V, seed, graph, gw)
        every = []
        for t in texts:                                              # length < S: ended by <EOS>; length S: capped
            s, G, score = graph.start, 0.0, 0.0
            for i, c in enumerate(t):
                score += m.row(t[:i])[c]
                G += float(graph.arc[s, c])
                s = int(graph.next[s, c])
            capped = len(t) == S
            if not capped:
                score += m.row(t)[EOS]
                G += float(graph.fin[s])
            if G > NEG:
                every.append((list(t), score + gw * G, G, capped))
        seen_forbidden += len(every) < len(texts)
        every.sort(key=lambda e: -e[1])
        for K in (7, 32):
            r = gbc.beam_search(m, K, S, None)
            assert [h[0] for h in r['hyps']] == [e[0] for e in every] and [h[3] for h in r['hyps']] == [e[3] for e in every]
            assert all(abs(h[1] - e[1]) <= 1e-12 for h, e in zip(r['hyps'], every))
            assert all(abs(p - e[2]) <= 1e-12 for p, e in zip(r['parts'], every))
    assert seen_forbidden >= 2


# ------------------------------------------------------------ hand-built graphs ----
TABLE = [0.5, 0.1, 0.4]                                              # after every prefix: class 0, <EOS>, class 2


def toy(graph=None, gw=0.0):
    return gbc.RowModel(3, 0, graph, gw, table=TABLE)


def texts_of(r):
    return [(h[0], h[3]) for h in r['hyps']]


def test_a_hotword_makes_the_second_text_come_first():
    from ss_asr_amd.char_graph import CharGraph
    plain = gbc.beam_search(toy(), 3, 1, None)
    assert texts_of(plain) == [([0], True), ([2], True), ([], False)]
    hot = CharGraph.hotwords([[2]], 1.0, 3)
    r = gbc.beam_search(toy(hot, 1.0), 3, 1, None)
    assert texts_of(r) == [([2], True), ([0], True), ([], False)]
    assert abs(r['hyps'][0][1] - (math.log(0.4) + 1.0)) <= 1e-12 and r['parts'] == [1.0, 0.0, 0.0]
    # a tenth of the weight does not pay for the model's preference (0.1 < log 1.25)
    assert texts_of(gbc.beam_search(toy(hot, 0.1), 3, 1, None)) == texts_of(plain)
    # two steps: 'ab'-like partial matches are paid in advance and a capped text keeps the advance
    two = CharGraph.hotwords([[2, 3]], 1.0, 4)
    r = gbc.beam_search(gbc.RowModel(4, 0, two, 1.0, table=[0.1, 0.1, 0.4, 0.4]), 13, 2, None)
    parts = {(tuple(h[0]), h[3]): p for h, p in zip(r['hyps'], r['parts'])}
    assert len(parts) == 13
    assert parts[((2, 3), True)] == 2.0 and parts[((2,), False)] == 0.0 and parts[((2, 2), True)] == 1.0
    assert parts[((3, 2), True)] == 1.0 and parts[((3,), False)] == 0.0


def test_a_forbidden_arc_removes_the_first_text_and_a_closed_start_leaves_the_empty_text():
    from ss_asr_amd.char_graph import CharGraph
    no_zero = CharGraph([[0, 0, 0]], [[NEG, 0.0, 0.0]], [0.0])
    r = gbc.beam_search(toy(no_zero, 1.0), 3, 1, None)
    assert texts_of(r) == [([2], True), ([], False)] and r['forbidden'] == 1          # fewer than K members
    assert abs(r['hyps'][0][1] - math.log(0.4)) <= 1e-12 and r['parts'] == [0.0, 0.0]
    # every arc out of the start state forbidden (the <EOS> column too: it is never read, fin is): the empty text alone
    wall = CharGraph([[0, 0, 0]], [[NEG, NEG, NEG]], [0.5])
    for K, S in ((1, 1), (3, 4)):
        r = gbc.beam_search(toy(wall, 2.0), K, S, None)
        assert texts_of(r) == [([], False)] and r['n_steps'] == 1 and r['gap'] == math.inf
        assert abs(r['hyps'][0][1] - (math.log(0.1) + 1.0)) <= 1e-12 and r['parts'] == [0.5]


def test_one_state_is_a_per_class_bias():
    from ss_asr_amd.char_graph import CharGraph
    bias, b_eos, gw, S = np.array([0.75, 123.0, -0.5]), 0.25, 0.5, 2    # exact in float32; arc[0][<EOS>] is unread
    graph = CharGraph(np.zeros((1, 3), dtype=np.int64), bias[None], [b_eos])
    m = gbc.RowModel(3, 4, graph, gw)
    r = gbc.beam_search(m, 7, S, None)
    want = {}
    for n in range(S + 1):
        for t in itertools.product((0, 2), repeat=n):
            score = sum(m.row(t[:i])[c] + gw * bias[c] for i, c in enumerate(t))
            want[t] = score + (m.row(t)[EOS] + gw * b_eos if n < S else 0.0)
    assert [tuple(h[0]) for h in r['hyps']] == sorted(want, key=lambda t: -want[t])
    assert all(abs(h[1] - want[tuple(h[0])]) <= 1e-12 for h in r['hyps'])
    assert [tuple(h[0]) for h in r['hyps']] != [tuple(h[0]) for h in gbc.beam_search(gbc.RowModel(3, 4), 7, S, None)['hyps']]


# ---------------------------------------------------------------- C entries ----
SIZES = (1, 3, 5, 64, 16, 32, 50, 0, 24)                             # N K T E A D V Hl S


def _call(beam=None, ctc=None, terms=None, graph=1, weight=0.5, scores=1, **g):
    """ssasr_decode_beam_graph on a description whose pointers are not NULL (never dereferenced: the checks come
    first) with the named fields changed -> its code."""
    from ss_asr_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 4096)()
    at = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    d = _lib.Beam()
    d.N, d.K, d.T, d.E, d.A, d.D, d.V, _, d.max_steps = SIZES
    for name, _ in _lib.Beam._fields_:
        if name not in ('N', 'T', 'E', 'A', 'D', 'V', 'max_steps', 'K', 'lm', 'lm_weight', 'eos', 'ws_bytes'):
            setattr(d, name, at)
    d.eos, d.ws_bytes = 1, 1 << 40
    for k, v in (beam or {}).items():
        setattr(d, k, v)
    gs = _lib.CharGraph(at, at, at, g.get('S', 4), g.get('V', 50), g.get('start', 3))
    for k in ('next', 'arc', 'fin'):
        if k in g:
            setattr(gs, k, g[k])
    c = None if ctc is None else ctypes.byref(_lib.CtcPrefix(at, at, *ctc))
    t = None if terms is None else ctypes.byref(_lib.BeamTerms(*terms, None))
    return lib.ssasr_decode_beam_graph(ctypes.byref(d), c, t, ctypes.byref(gs) if graph else None, weight,
                                       at if scores else None, None)


def test_the_entries_are_exported_and_bound_under_abi_16():
    from ss_asr_amd import _lib
    lib = _lib.load()
    assert lib.ssasr_abi_version() == 16 == _lib.ABI_VERSION
    protos, header = header_prototypes()
    for name in ('ssasr_decode_beam_graph', 'ssasr_decode_beam_graph_ws_bytes'):
        assert name in protos and name in _lib.SIGNATURES and hasattr(lib, name)
    assert protos['ssasr_decode_beam_graph'] == ('i32', ['ptr', 'ptr', 'ptr', 'ptr', 'f32', 'ptr', 'ptr'])
    assert protos['ssasr_decode_beam_graph_ws_bytes'] == protos['ssasr_decode_beam_ex_ws_bytes'] == \
        ('i64', ['i64'] * 9 + ['i32', 'i32'])
    res, args = _lib.SIGNATURES['ssasr_decode_beam_graph']
    assert res is ctypes.c_int and args[3] is ctypes.POINTER(_lib.CharGraph) and args[4] is ctypes.c_float
    assert 'typedef struct ssasr_char_graph {' in header             # the structure of the CTC search, reused


def test_the_entry_rejects_bad_arguments_before_any_hip_call():
    from ss_asr_amd import _lib
    lib = _lib.load()
    d = _lib.Beam()
    at = ctypes.addressof((ctypes.c_float * 8)())
    assert lib.ssasr_decode_beam_graph(None, None, None, None, 0.0, at, None) == -1
    assert lib.ssasr_decode_beam_graph(ctypes.byref(d), None, None, None, 0.0, at, None) == -1     # all sizes zero
    # the graph arguments, everything else being acceptable
    for bad in (dict(graph=None), dict(V=49), dict(V=51), dict(S=0), dict(S=-1), dict(S=(1 << 20) + 1), dict(start=4),
                dict(start=-1), dict(weight=-0.5), dict(weight=math.nan), dict(weight=math.inf), dict(weight=-math.inf),
                dict(scores=None), dict(next=None), dict(arc=None), dict(fin=None),
                dict(weight=0.0, V=49), dict(weight=0.0, S=0), dict(weight=0.0, start=4), dict(weight=0.0, scores=None),
                dict(graph=None, weight=0.0, scores=None)):
        assert _call(**bad) == -1, bad
    # the underlying entry's own errors, with a good graph
    for bad in (dict(beam=dict(K=0)), dict(beam=dict(K=33)), dict(beam=dict(N=0)), dict(beam=dict(T=16385)),
                dict(beam=dict(V=65)), dict(beam=dict(E=62)), dict(beam=dict(eos=50)), dict(beam=dict(eos=-1)),
                dict(beam=dict(ws=None)), dict(beam=dict(hyp_scores=None)), dict(beam=dict(n_hyps=None)),
                dict(beam=dict(feat=None)), dict(beam=dict(chars=None)),
                dict(beam=dict(ws_bytes=lib.ssasr_decode_beam_graph_ws_bytes(*SIZES, 0, 0) - 1)),
                dict(beam=dict(ws_bytes=lib.ssasr_decode_beam_graph_ws_bytes(*SIZES, 0, 0)), terms=(0.0, 0.3, 0.5, -1.0)),
                dict(beam=dict(ws_bytes=lib.ssasr_decode_beam_graph_ws_bytes(*SIZES, 0, 0)), ctc=(0.3, 0)),
                dict(terms=(math.nan, 0.0, 0.5, -1.0)), dict(terms=(0.0, math.inf, 0.5, -1.0)),
                dict(terms=(0.0, 0.3, 0.0, -1.0)), dict(terms=(0.0, 0.0, 0.5, math.nan)),
                dict(ctc=(1.5, 0)), dict(ctc=(-0.1, 0)), dict(ctc=(0.3, 50)), dict(ctc=(0.3, -1)), dict(ctc=(0.3, 1))):
        assert _call(**bad) == -1, bad
        assert _call(weight=0.0, **bad) == -1, bad
        assert _call(weight=0.0, graph=None, **bad) == -1, bad


def test_the_size_query_is_the_search_s_own_and_zero_for_rejected_sizes():
    from ss_asr_amd import _lib
    lib = _lib.load()
    big = (32, 8, 100, 512, 128, 256, 50, 128, 200)
    for sizes in (SIZES, big, (3, 32, 137, 512, 128, 256, 50, 128, 200)):
        for ctc in (0, 1):
            for cov in (0, 1):
                got = lib.ssasr_decode_beam_graph_ws_bytes(*sizes, ctc, cov)
                assert got == lib.ssasr_decode_beam_ex_ws_bytes(*sizes, ctc, cov) > 0       # the graph state is in LDS
    for ctc in (0, 1):
        for cov in (0, 1):
            for i, v in ((0, 0), (1, 0), (1, 33), (2, 16385), (6, 65), (3, 510), (5, 250), (8, 0)):
                sizes = list(big)
                sizes[i] = v
                assert lib.ssasr_decode_beam_graph_ws_bytes(*sizes, ctc, cov) == 0, (i, v)


# ------------------------------------------------------------ Python surface ----
class _Mapper:
    def char_to_ind(self, c):
        return 1

    def ind_to_char(self, i):
        return '?'


def test_ops_rejects_bad_arguments_and_has_no_cpu_path():
    from ss_asr_amd import ops
    from ss_asr_amd.asr import ASR
    model = ASR(50, 32, 32, 16, 12, 1.0)
    params = model._decoder_params()
    E = params['w_ih1'].shape[1] - params['w_phi'].shape[1]
    args = model._decode_args(torch.zeros(1, 4, E), torch.tensor([4], dtype=torch.int32), None, 0.0, 1, 24)
    g = random_graph(3, 50, 0)
    for bad in (math.nan, math.inf, -0.5):
        with pytest.raises(ValueError, match='finite'):
            ops.decode_beam_graph(*args, 3, None, graph=g, graph_weight=bad)
    with pytest.raises(ValueError, match='needs a graph'):
        ops.decode_beam_graph(*args, 3, None, graph=None, graph_weight=0.5)
    with pytest.raises(TypeError, match='CharGraph'):
        ops.decode_beam_graph(*args, 3, None, graph=(g.next, g.arc, g.fin), graph_weight=0.5)
    with pytest.raises(ValueError, match='classes'):
        ops.decode_beam_graph(*args, 3, None, graph=random_graph(3, 49, 0), graph_weight=0.5)
    with pytest.raises(TypeError):                                   # keyword-only, and both required
        ops.decode_beam_graph(*args, 3, None, g, 0.5)
    with pytest.raises(TypeError):
        ops.decode_beam_graph(*args, 3, None, graph=g)
    for K in (0, 33):
        with pytest.raises(RuntimeError, match='invalid argument'):
            ops.decode_beam_graph(*args, K, None, graph=g, graph_weight=0.5)
    for kw in (dict(graph=g, graph_weight=0.5), dict(graph=None, graph_weight=0.0), dict(graph=g, graph_weight=0.0),
               dict(graph=g, graph_weight=0.5, length_bonus=0.5, coverage_weight=0.2, end_margin=1.0)):
        with pytest.raises(RuntimeError, match='no CPU path'):
            ops.decode_beam_graph(*args, 3, None, **kw)


def test_the_decode_methods_check_the_graph_keywords_before_anything_runs():
    from ss_asr_amd.asr import ASR
    model = ASR(50, 32, 32, 16, 12, 1.0)
    x = torch.zeros(1, 16, 12)
    g = random_graph(3, 50, 0)
    calls = (lambda **kw: model.decode(x, [16], None, _Mapper(), 0.0, beam_size=3, **kw),
             lambda **kw: model.decode_many([x], [[16]], None, _Mapper(), 0.0, beam_size=1, **kw),
             lambda **kw: model.decode_nbest([x], [[16]], None, _Mapper(), 0.0, 3, **kw),
             lambda **kw: model.decode_mbr([x], [[16]], None, _Mapper(), 0.0, 3, **kw))
    for call in calls:
        for bad in (math.nan, math.inf, -0.5, '1', None, True):
            with pytest.raises(ValueError, match='graph_weight'):
                call(graph=g, graph_weight=bad)
        with pytest.raises(ValueError, match='needs graph'):
            call(graph_weight=0.5)
        with pytest.raises(ValueError, match='CharGraph'):
            call(graph=(1, 2), graph_weight=0.5)
        with pytest.raises(ValueError, match='CharGraph'):
            call(graph=(1, 2))                                       # looked at even at weight 0
        with pytest.raises(ValueError, match='classes'):
            call(graph=random_graph(3, 49, 0), graph_weight=0.5)
        for kw in (dict(graph=g, graph_weight=0.5), dict(graph=g), dict(graph=g, graph_weight=0.5, length_bonus=0.3)):
            with pytest.raises(RuntimeError, match='no CPU path'):
                call(**kw)
    with pytest.raises(TypeError):                                   # keyword-only
        model.decode_nbest([x], [[16]], None, _Mapper(), 0.0, 3, 200, 0.0, 0.0, 0.0, 0.5, None, g, 0.5)
    assert model.last_beam is None and model.last_beam_steps is None and model.last_beam_graph is None


def test_tester_validates_the_graph_keys_of_the_attention_search(tmp_path):
    from test_ctc_search_cpu import _tester
    from ss_asr_amd.ASRDataset import Mapper
    from ss_asr_amd.char_graph import CharGraph
    from ss_asr_amd.trainer import ASRTester
    keys = ASRTester.beam_graph
    assert keys({}) is None and keys({'decode_beam_size': 3, 'decode_lm_weight': 0.5}) is None
    assert keys({'decode_ctc_only': {'beam_size': 4, 'hotwords': ['ab']}}) is None       # that mapping's own keys
    assert keys({'decode_hotwords': ['ab', 'c d']}) == \
        {'hotwords': ['ab', 'c d'], 'hotword_bonus': 1.0, 'ngram_lm': None, 'ngram_weight': 0.5}
    assert keys({'decode_hotwords': ['ab'], 'decode_hotword_bonus': 2, 'decode_ngram_lm': 'lm.npz',
                 'decode_ngram_weight': 0.25}) == \
        {'hotwords': ['ab'], 'hotword_bonus': 2.0, 'ngram_lm': 'lm.npz', 'ngram_weight': 0.25}
    for bad in ({'decode_hotwords': []}, {'decode_hotwords': 'ab'}, {'decode_hotwords': ['ab', '']},
                {'decode_hotwords': [1]}, {'decode_ngram_lm': 3}, {'decode_ngram_lm': ''},
                {'decode_hotword_bonus': 1.0}, {'decode_ngram_weight': 0.5},                # a bonus without words, ...
                {'decode_hotwords': ['a'], 'decode_ngram_weight': 0.5},                     # a weight without a file
                {'decode_ngram_lm': 'x.npz', 'decode_hotword_bonus': 1.0}):
        with pytest.raises(ValueError, match=r'asr\.decode_(hotword|ngram)'):
            keys(bad)
    for key, need in (('decode_hotword_bonus', {'decode_hotwords': ['a']}), ('decode_ngram_weight', {'decode_ngram_lm': 'x.npz'})):
        for bad in (math.nan, math.inf, -1, '1', None, True, [1]):
            with pytest.raises(ValueError, match=r'asr\.' + key):
                keys(dict(need, **{key: bad}))
    for other in (True, {'beam_size': 4}, {'beam_size': 4, 'hotwords': ['a']}):
        with pytest.raises(ValueError, match='decode_ctc_only'):
            keys({'decode_hotwords': ['a'], 'decode_ctc_only': other})
    # every rejection that decode_ctc_only makes stays as it is
    with pytest.raises(ValueError, match='decode_rescore'):
        ASRTester.ctc_only_graph({'decode_ctc_only': {'hotwords': ['a']}, 'decode_rescore': True})
    with pytest.raises(ValueError, match='not built'):
        ASRTester.ctc_only_graph({'decode_ctc_only': {'hotwords': ['a'], 'lm_weight': 0.5}})
    # set_model validates everything, the files and the characters included
    root = str(tmp_path)
    mapper = Mapper()
    V = mapper.get_dim()

    def model_error(match, mdl=None, **asr_keys):
        t = _tester(root, mdl or {}, **asr_keys)
        t.mapper = mapper
        with pytest.raises(ValueError, match=match):
            t.set_model()
    model_error(r'asr\.decode_hotwords.*no character', decode_hotwords=['a#'])
    model_error(r'asr\.decode_ngram_lm: no file', decode_ngram_lm=os.path.join(root, 'none.npz'))
    small = os.path.join(root, 'small.npz')
    random_graph(3, 8, 0).save(small)
    model_error(r'asr\.decode_ngram_lm: the graph has 8 classes', decode_ngram_lm=small)
    model_error('decode_ctc_only', {'ctc_weight': 0.3}, decode_hotwords=['ab'], decode_ctc_only={'beam_size': 4})
    model_error(r'asr\.decode_hotword_bonus', decode_hotwords=['ab'], decode_hotword_bonus=-1)
    # what set_model builds: the hotwords at weight 1, the n-gram at its weight, both as the product at weight 1
    good = os.path.join(root, 'lm.npz')
    lm = CharGraph.ngram([[mapper.char_to_ind(c) for c in 'abcab']], 2, V, mapper.char_to_ind('>'))
    lm.save(good)
    t = _tester(root, {})
    t.mapper = mapper
    ab = [mapper.char_to_ind(c) for c in 'ab']
    name = 'asr.decode_{}'.format
    hot, w = t.build_ctc_graph(keys({'decode_hotwords': ['ab'], 'decode_hotword_bonus': 2}), name)
    assert w == 1.0 and hot.n_states == 3 and abs(hot.score(ab)[0] - 4.0) <= 1e-6
    only, w = t.build_ctc_graph(keys({'decode_ngram_lm': good, 'decode_ngram_weight': 0.25}), name)
    assert w == 0.25 and np.array_equal(only.arc, lm.arc)
    prod, w = t.build_ctc_graph(keys({'decode_hotwords': ['ab'], 'decode_hotword_bonus': 2, 'decode_ngram_lm': good,
                                      'decode_ngram_weight': 0.25}), name)
    assert w == 1.0 and abs(prod.score(ab)[0] - (0.25 * lm.score(ab)[0] + 4.0)) <= 1e-5


def test_without_the_keys_the_tester_names_the_file_as_before(tmp_path):
    import types
    from test_ctc_search_cpu import _tester
    from ss_asr_amd.ASRDataset import Mapper
    root, mapper = str(tmp_path), Mapper()

    def built(**asr_keys):
        """set_model with freshly initialised modules in place of the checkpoint's (no decode is run)."""
        t = _tester(root, {}, **asr_keys)
        t.mapper, t.ds = mapper, types.SimpleNamespace(get_char_dim=mapper.get_dim)
        t.setup_module = lambda cls, path, *a, **kw: cls(*a, **kw)
        t.set_model()
        return t
    plain = built()
    assert plain.decode_file == 'decode_beam_1_len_0.25_lm0.5' and plain.decode_beam_graph is None
    assert built(decode_length_bonus=0.5).decode_file == 'decode_beam_1_len_0.25_lm0.5_lb0.5'
    t = built(decode_hotwords=['ab', 'c'], decode_length_bonus=0.5)
    assert t.decode_file == 'decode_beam_1_len_0.25_lm0.5_hw2x1.0_lb0.5'
    assert t.decode_beam_graph[1] == 1.0 and t.decode_beam_graph[0].n_states == 4 and t.decode_ctc_graph is None
