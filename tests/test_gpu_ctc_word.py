"""ssasr_ctc_decode_word on the GPU (ctc_prefix_beam_word_kernel, csrc/ctc.hip): the CTC prefix beam search over a
lexicon with a word n-gram LM in the ranking, held to postprocess.ctc_prefix_beam_word_reference, the float64
restatement that tests/test_ctc_word_cpu.py pins.

Cases.  test_gpu_ctc_graph.py's CELLS, logits (4 N(0, 1) from default_rng([T, V, seed]), seeds 0..15 in one launch),
graph_weight 0.5 and length_bonus 0.3; the letters of a cell are the classes 1 .. V - 2, the space is V - 1.  Every
cell runs with four word graphs: 'lex2' / 'lex3', a random lexicon of 12 words of 1-4 letters with a Witten-Bell LM of
order 2 / 3 from 40 random sentences; 'single', every letter a one-letter word (every node below the root ends a
word, so the look-up runs for almost every new member), order 2; 'chain', 450 words with a hand-built LM of 8 states in
one back-off chain: every word leads to state 7, whose row and those of states 6..4 are empty, state 3 holds 300 words
(two rounds of the 64-way search), states 2 and 1 are empty again, so a word outside state 3's row walks all 8 rounds.
The V = 40 cells also run 'golden', the golden text's words at order 3.
A case is compared when the checker's gap is >= MIN_GAP = 1e-3, the project's rule; at least 90 % of all cases must be
compared and no (cell, graph) below 8 of 16.  The checker alone (this file's __main__, on the CPU) meets both: 1441
of 1472 cases (97.9 %), the worst cell 12 of 16.
A compared case must hold the checker's SET of texts, in the kernel's own non-increasing order, with the fused score and
each part within BOUND = 8 * NOISE.  NOISE = max |float32 - float64| of the checker run in float32 over the compared
hypotheses' totals and parts, measured by __main__ on the CPU: 1.82e-4 (the golden text's graph at T' = 80; 1.24e-4
the chain graph there).  The kernel's worst error on the MI355X is recorded beside it (KERNEL_WORST): 1.7e-5.
The same launches are held to ssasr_ctc_decode_graph on the EXPANDED graph (WordGraph.to_char_graph) of the small
lexicons: an independent yardstick through an existing kernel.  Zero weights are bit-equal to ssasr_ctc_decode on every
cell, with a graph and with NULL; an utterance alone is bit-equal to itself in a group."""
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_ctc_graph import (BETA, CANARY_F, CANARY_I, CELLS, DEV, GW, MIN_GAP, PAD, SEEDS, bits, check_row,
                                log_softmax, logits_of, plain)

COMPARED_CPU = (1441, 1472)                                      # measure(), on the CPU
WORST_CELL_CPU = 12
NOISE = 1.82e-4                                                  # measure(), on the CPU
BOUND = 8 * NOISE
KERNEL_WORST = 1.7e-5                                            # worst |kernel - float64| seen on the MI355X
SMALL = ('lex2', 'lex3', 'single')                               # the kinds whose expansion is small


def lexicon_of(V, n_words, seed):
    """n_words distinct spellings of 1-4 letters over 1 .. V - 2, 40 sentences of 1-5 words drawn with a skew."""
    rng = np.random.default_rng([V, n_words, seed])
    spell = {}
    while len(spell) < n_words:
        spell.setdefault(tuple(rng.integers(1, V - 1, rng.integers(1, 5)).tolist()), len(spell))
    words = sorted(spell)
    p = 1.0 / np.arange(1, n_words + 1)
    return words, [[words[i] for i in rng.choice(n_words, rng.integers(1, 6), p=p / p.sum())] for _ in range(40)]


def chain_graph(V):
    """The hand-built LM of the header over the 450 shortest spellings."""
    from ss_asr_amd.word_graph import WordGraph
    letters = range(1, V - 1)
    words = [(a,) for a in letters] + [(a, b) for a in letters for b in letters] + \
        [(a, b, c) for a in letters for b in letters for c in letters]
    words = words[:450]
    trie = WordGraph.build([], 1, list, V, V - 1, lexicon=words, lookahead=False)
    rng = np.random.default_rng([V, 77])
    W, H = len(words), 8
    row3 = np.array([w for w in range(W) if w % 3])
    off = np.array([0, W, W, W, W + len(row3)] + [W + len(row3)] * 4)
    wid = np.concatenate([np.arange(W), row3])
    wlp = -np.abs(rng.standard_normal(len(wid))) - 0.1
    wnext = np.full(len(wid), 7)
    bow = -0.125 * np.arange(H)
    bnext = np.arange(H) - 1
    eos = -np.abs(rng.standard_normal(H)) - 0.1
    return WordGraph(trie.child, trie.carc, trie.word, trie.pen, off, wid, wlp, wnext, bow, bnext, eos, V - 1)


_graphs = {}


def graph_of(kind, V):
    """The test's word graphs over V classes, built once."""
    from ss_asr_amd.word_graph import WordGraph
    if (kind, V) not in _graphs:
        if kind in ('lex2', 'lex3'):
            words, sents = lexicon_of(V, 12, 0)
            g = WordGraph.build(sents, int(kind[3]), list, V, V - 1, lexicon=words)
        elif kind == 'single':
            words, sents = lexicon_of(V, 12, 1)
            letters = [(c,) for c in range(1, V - 1)]
            g = WordGraph.build([[(w[0],) for w in s] for s in sents], 2, list, V, V - 1, lexicon=letters)
        elif kind == 'one':                                      # a one-word lexicon
            g = WordGraph.build([[(3, 1)], [(3, 1), (3, 1)]], 2, list, V, V - 1)
        elif kind == 'chain':
            g = chain_graph(V)
        else:
            from test_ctc_word_cpu import golden_words
            gw, _ = golden_words()
            code = {ch: 1 + i % (V - 2) for i, ch in enumerate(sorted(set(''.join(gw))))}
            g = WordGraph.build([gw], 3, lambda w: [code[ch] for ch in w], V, V - 1)
        _graphs[(kind, V)] = g
    return _graphs[(kind, V)]


def kinds_of(V):
    return ('lex2', 'lex3', 'single', 'chain') + (('golden',) if V == 40 else ())


_refs = {}


def reference(key, z, K, graph, gw=GW, beta=BETA, blank=0):
    """(hyps, gap, parts) of the checker on float64 log_softmax(z), computed once per key."""
    from ss_asr_amd.postprocess import ctc_prefix_beam_word_reference
    full = (key, K, gw, beta, blank)
    if full not in _refs:
        parts = []
        hyps, gap = ctc_prefix_beam_word_reference(log_softmax(z), K, graph, gw, beta, blank, parts=parts)
        _refs[full] = (hyps, gap, parts)
    return _refs[full]


def noise_of(z, K, graph):
    """max |float32 - float64| of the totals and parts over the texts both runs of the checker hold (None: the case is
    not compared)."""
    from ss_asr_amd.postprocess import ctc_prefix_beam_word_reference
    parts = []
    hyps, gap = ctc_prefix_beam_word_reference(log_softmax(z), K, graph, GW, BETA, parts=parts)
    if gap < MIN_GAP:
        return None
    parts32 = []
    hyps32, _ = ctc_prefix_beam_word_reference(log_softmax(z, np.float32), K, graph, GW, BETA, dtype=np.float32,
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
    """ssasr_ctc_decode_word on z [B, T, V] through the C entry, every output and the workspace followed by PAD canaries
    and pre-filled, so that an element the kernel leaves unwritten or writes past its end shows.  -> per row the list
    of (text, total, ctc, graph part) and the raw arrays."""
    import ctypes
    from ss_asr_amd import _lib, ops
    lib = _lib.load()
    B, T, V = z.shape
    need = int(lib.ssasr_ctc_decode_word_ws_bytes(B, T, V, K))
    assert need > 0 and need % 4 == 0
    s, keep = graph.to(DEV) if graph is not None else (None, None)
    logits = torch.from_numpy(np.ascontiguousarray(z)).to(DEV)
    lens = torch.tensor(list(frame_lens), dtype=torch.int32, device=DEV)
    ws = torch.full((need // 4 + PAD,), CANARY_I, dtype=torch.int32, device=DEV)
    ints = {'chars': B * K * T, 'n_chars': B * K, 'n_hyps': B}
    flts = {'scores': B * K, 'ctc_scores': B * K, 'graph_scores': B * K}
    buf = {n: torch.full((c + PAD,), CANARY_I, dtype=torch.int32, device=DEV) for n, c in ints.items()}
    buf.update({n: torch.full((c + PAD,), CANARY_F, dtype=torch.float32, device=DEV) for n, c in flts.items()})
    ops.check(lib.ssasr_ctc_decode_word(ops._p(logits), ops._p(lens), B, T, V, K, blank, ops._p(ws), need,
                                        ops._p(buf['chars']), ops._p(buf['n_chars']), ops._p(buf['scores']),
                                        ops._p(buf['n_hyps']), ctypes.byref(s) if s is not None else None, gw, beta,
                                        ops._p(buf['ctc_scores']), ops._p(buf['graph_scores']), ops._stream()),
              'ssasr_ctc_decode_word')
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


_runs, _dense = {}, {}


def cell_run(T, V, K, kind):
    """The kernel's lists for the 16 seeds of a cell and graph: one launch, shared by the tests that read it."""
    if (T, V, K, kind) not in _runs:
        z = np.stack([logits_of(T, V, s) for s in SEEDS])
        _runs[(T, V, K, kind)] = (z, run(z, [T] * len(SEEDS), K, graph_of(kind, V))[0])
    return _runs[(T, V, K, kind)]


def test_the_kernel_matches_the_checker_on_every_compared_case():
    compared, worst, total = {}, 0.0, 0
    for T, V, K in CELLS:
        for kind in kinds_of(V):
            z, got = cell_run(T, V, K, kind)
            compared[(T, V, K, kind)] = 0
            for s in SEEDS:
                total += 1
                want, gap, parts = reference((T, V, s, kind), z[s], K, graph_of(kind, V))
                if gap < MIN_GAP:
                    continue
                compared[(T, V, K, kind)] += 1
                worst = max(worst, check_row(got[s], want, parts, BOUND))
    done = sum(compared.values())
    print('compared per cell (of %d): %s' % (len(SEEDS), compared))
    print('%d of %d cases compared, worst |kernel - float64| %.3g (NOISE %.3g, bound %.3g)'
          % (done, total, worst, NOISE, BOUND))
    assert total == COMPARED_CPU[1]
    assert done >= 0.9 * total
    assert all(2 * n >= len(SEEDS) for n in compared.values())


def test_the_graph_kernel_on_the_expanded_graph_gives_the_same_lists():
    import test_gpu_ctc_graph as tgg
    compared = 0
    for T, V, K in CELLS:
        for kind in SMALL:
            graph = graph_of(kind, V)
            z, got = cell_run(T, V, K, kind)
            if (kind, V) not in _dense:
                _dense[(kind, V)] = graph.to_char_graph()
            dense, _ = tgg.run(z, [T] * len(SEEDS), K, _dense[(kind, V)])
            for s in SEEDS:
                if reference((T, V, s, kind), z[s], K, graph)[1] < MIN_GAP:
                    continue
                compared += 1
                assert [g[0] for g in got[s]] == [d[0] for d in dense[s]], (T, V, K, kind, s)
                assert max(abs(a - b) for g, d in zip(got[s], dense[s]) for a, b in zip(g[1:], d[1:])) <= BOUND
    assert compared >= 0.9 * len(CELLS) * len(SMALL) * len(SEEDS)


def test_zero_weights_are_ssasr_ctc_decode_bit_for_bit_on_every_cell():
    for T, V, K in CELLS:
        z = np.stack([logits_of(T, V, s) for s in SEEDS])
        chars, n_chars, scores, n_hyps = plain(z, [T] * len(SEEDS), K)
        for graph in (None, graph_of('lex3', V)):                # with a graph at weight 0: unread
            _, raw = run(z, [T] * len(SEEDS), K, graph, gw=0.0, beta=0.0)
            assert np.array_equal(raw['chars'], chars) and np.array_equal(raw['n_chars'], n_chars), (T, V, K)
            assert np.array_equal(raw['n_hyps'], n_hyps)
            assert np.array_equal(bits(raw['scores']), bits(scores)) and np.array_equal(bits(raw['ctc_scores']), bits(scores))
            assert (raw['graph_scores'] == 0.0).all()


@pytest.mark.parametrize('K', [2, 8])
def test_an_utterance_decodes_in_a_group_as_it_decodes_alone(K):
    lens = [20, 5, 1]
    graph = graph_of('single', 8)
    z = np.stack([logits_of(20, 8, 200 + i) for i in range(len(lens))])
    _, group = run(z, lens, K, graph)
    for i, n in enumerate(lens):
        _, alone = run(z[i:i + 1, :n], [n], K, graph)
        for name in ('n_chars', 'n_hyps', 'scores', 'ctc_scores', 'graph_scores'):
            assert np.array_equal(bits(alone[name][0]), bits(group[name][i])), name
        assert np.array_equal(alone['chars'][0], group['chars'][i, :, :n]) and (group['chars'][i, :, n:] == 0).all()


@pytest.mark.parametrize('K', [1, 3, 8])
def test_edges(K):
    """Lengths 0, 1 and past T', blank 3 (the space stays V - 1), a length bonus alone, and a one-word lexicon."""
    from ss_asr_amd.word_graph import WordGraph
    T, V = 20, 8
    rows = [('no frames', logits_of(T, V, 100), 0), ('one frame', logits_of(T, V, 101), 1),
            ('length past the rows', logits_of(T, V, 102), 25), ('whole', logits_of(T, V, 103), 20)]
    base = graph_of('lex3', V)
    words, sents = lexicon_of(V, 12, 0)
    moved = WordGraph.build(sents, 3, lambda w: [c - 1 if c <= 3 else c for c in w], V, V - 1, lexicon=words,
                            blank=3)                             # the letters 0, 1, 2, 4, 5, 6 around the blank 3
    for tag, blank, gw, beta, graph in (('base', 0, GW, BETA, base), ('blank 3', 3, GW, BETA, moved),
                                        ('bonus alone', 0, 0.0, BETA, base), ('one word', 0, GW, 0.0, graph_of('one', V))):
        got, raw = run(np.stack([r[1] for r in rows]), [r[2] for r in rows], K, graph, gw, beta, blank)
        for (name, z, n), mine in zip(rows, got):
            want, gap, parts = reference((name, tag), z[:min(n, T)], K, graph, gw, beta, blank)
            if gap >= MIN_GAP:
                check_row(mine, want, parts, BOUND)
            if name == 'no frames':                              # the empty text alone: fin(0, 0) is its whole score
                assert len(mine) == 1 and mine[0][0] == () and mine[0][2] == 0.0
                assert abs(mine[0][1] - want[0][1]) <= BOUND
            if tag == 'one word':                                # (3, 1) and spaces between, nothing else
                for g in mine:
                    assert all(c == (3, 1, V - 1)[i % 3] for i, c in enumerate(g[0]))
        if gw == 0.0:
            assert (raw['graph_scores'] == 0.0).all()


def test_ops_is_the_entry_and_rejects_what_the_entry_rejects():
    from ss_asr_amd import ops
    V = 8
    graph = graph_of('lex2', V)
    zs = np.stack([logits_of(20, V, s) for s in range(3)])
    lens = torch.tensor([20, 7, 0], dtype=torch.int32, device=DEV)
    out = ops.ctc_decode_word(torch.from_numpy(zs).to(DEV), lens, 5, graph, GW, BETA)
    _, raw = run(zs, [20, 7, 0], 5, graph)
    for name, arr in raw.items():
        assert np.array_equal(bits(out[name].cpu().numpy()), bits(arr)), name
    with pytest.raises(ValueError, match='no kernel'):
        ops.ctc_decode_word(torch.zeros(1, 4097, V, device=DEV), lens[:1], 2, graph, 0.5)
    with pytest.raises(ValueError, match='classes'):
        ops.ctc_decode_word(torch.zeros(1, 8, 9, device=DEV), lens[:1], 2, graph, 0.5)


def test_decode_ctc_with_a_word_graph_and_the_tester_keys(golden, tmp_path):
    import las_oracle as lo
    import test_gpu_ctc_decode as tcd
    import test_gpu_rescore as tgr
    from conftest import GOLDEN
    from test_host_cpu import make_corpus
    from ss_asr_amd.ASRDataset import Mapper, prepare_x
    from ss_asr_amd.ctc import JointCTCASR
    from ss_asr_amd.trainer import ASRTester
    from ss_asr_amd.word_graph import WordGraph
    fx = golden(tgr.SMALL)
    asr, lm = tcd.models(fx)
    mapper = Mapper()
    V, space = mapper.get_dim(), mapper.char_to_ind(' ')
    xs, x_lens = tgr.ctc_groups(fx, (40, 24, 8), 3)
    # a lexicon from what the head itself says: the words of the plain search's lists, and a few more
    plain_lists = asr.decode_ctc(xs, x_lens, mapper, beam_size=4)
    assert len(asr.last_ctc_decode) == 5
    seen = sorted({w for hyps in plain_lists for text, _ in hyps for w in text.split(' ') if w})
    lexicon = sorted(set(seen) | {'hello', 'halló', 'hold'})
    sents = [text.split() for hyps in plain_lists for text, _ in hyps if text.split()] + [['hello', 'hold']]
    wg = WordGraph.build(sents, 3, lambda w: [mapper.char_to_ind(c) for c in w], V, space, lexicon=lexicon)
    nbest = asr.decode_ctc(xs, x_lens, mapper, beam_size=3, word_graph=wg, graph_weight=GW, length_bonus=BETA)
    assert len(asr.last_ctc_decode) == 7 and asr.last_hyp_scores is asr.last_ctc_decode[2]
    chars, n_chars, scores, n_hyps, logits, ctc_s, gr_s = [t.cpu().numpy() for t in asr.last_ctc_decode]
    frames = asr.last_encoded_packed[1].cpu().tolist()
    compared = 0
    for i in range(3):
        n = int(n_hyps[i])
        assert [s for _, s in nbest[i]] == scores[i, :n].tolist()
        for text, _ in nbest[i]:                                 # every complete word is a lexicon word
            parts = text.split(' ')
            assert all(w in lexicon for w in parts[:-1]) and (text.endswith(' ') or any(
                w.startswith(parts[-1]) for w in lexicon))
        want, gap, parts = reference(('model', i), logits[i, :frames[i]], 3, wg)
        if gap >= MIN_GAP:
            compared += 1
            mine = [(tuple(int(c) for c in chars[i, k, :n_chars[i, k]]), float(scores[i, k]), float(ctc_s[i, k]),
                     float(gr_s[i, k])) for k in range(n)]
            check_row(mine, want, parts, BOUND)
    assert compared >= 2
    # score, mbr and align follow it
    tops = [h[0][0] for h in nbest]
    assert len(asr.score(tops, mapper)) == 3
    assert all(0 <= m.k < 3 for m in asr.mbr(mapper, unit='char'))
    assert len(asr.align(xs, x_lens, tops, mapper, encoded=asr.last_encoded_packed)) == 3
    # a word graph at weight 0 takes the old entry
    asr.decode_ctc(xs, x_lens, mapper, beam_size=3, word_graph=wg)
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
    wg_path = os.path.join(root, 'words.npz')
    wg.save(wg_path)

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
    assert old.decode_file == 'decode_beam_3_len_0.25_lm0.5_ctconly4' and old.decode_ctc_word is None
    base = old.exec()
    assert len(old.asr_model.last_ctc_decode) == 5
    t = tester(decode_ctc_only={'beam_size': 4, 'word_lm': wg_path, 'word_lm_weight': 0.25, 'length_bonus': 0.25},
               decode_score=True)
    assert t.decode_file == 'decode_beam_3_len_0.25_lm0.5_ctconly4_wlm0.25_clb0.25'
    got = t.exec()
    assert len(got) == 5 and len(t.last_scores) == 5 and len(t.asr_model.last_ctc_decode) == 7
    direct = []
    for x, _ in t.test_set:
        x, l = prepare_x(x, t.device)
        direct.append(t.asr_model.decode_ctc([x[:, :l[0]]], [l], t.mapper, beam_size=4, length_bonus=0.25,
                                             word_graph=wg, graph_weight=0.25)[0][0][0])
    assert got == direct
    one = tester(decode_ctc_only={'beam_size': 4, 'word_lm': wg_path})
    assert one.decode_file == 'decode_beam_3_len_0.25_lm0.5_ctconly4_wlm0.5' and one.decode_ctc_word[1] == 0.5
    assert len(one.exec()) == 5 and len(one.asr_model.last_ctc_decode) == 7
    assert base == tester(decode_ctc_only={'beam_size': 4}).exec()


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    measure()
