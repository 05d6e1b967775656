"""The attention beam search with a character graph on the GPU (ssasr_decode_beam_graph; ops.decode_beam_graph; ASR.decode
/ decode_many / decode_nbest / decode_mbr with graph, graph_weight; ASRTester with asr.decode_hotwords / decode_ngram_lm)
against the float64 CPU checker of tests/graph_beam_checker.py: decode_checker.beam_search run unchanged on a model
whose root / entries / child carry the graph state.  It shares nothing with the library's host code.

Grid: test_gpu_beam.PAIR_CASES (the small fixtures at T' = 5 and 3, one full-dimension fixture at T' = 20), 24 steps,
K in {1, 2, 3, 5} (K = 32 once), lambda in {0, 0.3}, terms off and GRID[2] of test_gpu_beam_terms (length bonus, coverage
and end detection together), graph_weight 0.5, four graphs: random ones of S = 7 and S = 300 (random next, arcs N(0, 1),
one in ten -inf, start = S - 1), a hotword graph of three phrases taken from the plain search's own lower-ranked texts,
and the order-3 n-gram graph of the golden text folded onto the fixture's classes.

A tuple is compared when the checker's smallest gap is >= MIN_GAP = 1e-3 (and, with coverage on, no |cum' - tau| is
below TAU_MARGIN); the lists, n_chars, n_hyps and n_steps must then be EQUAL.  A hypothesis' score is held to
test_gpu_ctc_decode.bound(steps, lambda) + 2^-22 * steps * max(1, |reference score|): the added term is one float
product and one float add per step, each within 2^-24 relative to the running score, with a factor 4 of margin.
graph_scores is held to 2^-22 * steps * max(1, |G|) (the kernel sums in double and rounds once).

The float64 checker alone over the grid, on the CPU before any GPU run (`PYTHONPATH=.:oracle python
tests/test_gpu_beam_graph.py`):
COUNTS_CPU below.  Worst errors measured on the MI355X: DESIGN 4.23."""
import ctypes
import math
import os
import shutil
import types

import numpy as np
import pytest
import torch

import decode_checker as dc
import graph_beam_checker as gbc
import test_gpu_beam as tgb
import test_gpu_beam_terms as tgt
import test_gpu_ctc_decode as tgc
import test_gpu_decode as tgd
from conftest import GOLDEN
from test_host_cpu import make_corpus

pytestmark = pytest.mark.gpu

DEV = tgd.DEV
Mapper = tgd.Mapper
MIN_GAP, TAU_MARGIN = tgb.MIN_GAP, tgt.TAU_MARGIN
EOS, STEPS, GW = 1, 24, 0.5
BEAMS = (1, 2, 3, 5)
LAMBDAS = (0.0, 0.3)
OFF = (0.0, 0.0, 0.5, None)
TERMS = (OFF, tgt.GRID[2])
KINDS = ('rand7', 'rand300', 'hot', 'ngram3')
WIDE = (tgb.SMALL[0], 24, 0, 32, 0.0, OFF, 'rand7')                 # K = 32, once
EPS = 2.0 ** -22
NEG = -math.inf
PAD = 64
# the float64 checker alone over the grid (the CPU, before any GPU run): tuples, compared, and of those: at full
# dimensions, with CTC, with a plain-search text that a -inf arc removes, with a list that differs from graph_weight = 0
COUNTS_CPU = (641, 415, 76, 238, 86, 412)                           # measure(); no seed or scale had to be changed


_graphs, _refs = {}, {}


def plain(golden, name, frames, k, K, lam=0.0, terms=OFF):
    """The search without a graph (graph_weight = 0), from test_gpu_beam_terms' cache."""
    return tgt.reference(golden, name, frames, k, K, lam, terms)


def graph_of(golden, kind, name, frames, k):
    """The grid's graphs over the fixture's classes, built once; the hotword graph is per (fixture, frames, LM weight):
    three phrases from the plain K = 5 search's texts below the first."""
    from test_ctc_graph_cpu import golden_sequences, random_graph
    from ss_asr_amd.char_graph import CharGraph
    V = int(golden(name)['dims'][0])
    key = (kind, V) if kind != 'hot' else (kind, name, frames, k)
    if key not in _graphs:
        if kind == 'rand7':
            g = random_graph(7, V, 0)
        elif kind == 'rand300':
            g = random_graph(300, V, 1)
        elif kind == 'hot':
            texts = [tuple(h[0]) for h in plain(golden, name, frames, k, 5)['hyps'][1:]]
            phrases = [list(t) for t in dict.fromkeys(texts) if t and 0 not in t][:3] or [[2, 3]]
            g = CharGraph.hotwords(phrases, 1.0, V)
        else:
            seqs, _ = golden_sequences()
            g = CharGraph.ngram([[2 + (c - 2) % (V - 2) for c in s] for s in seqs], 3, V, EOS)
        _graphs[key] = g
    return _graphs[key]


def reference(golden, name, frames, k, K, lam, terms, graph, gw=GW, S=STEPS):
    key = (name, frames, k, K, lam, terms, id(graph), gw, S)
    if key not in _refs:
        m = gbc.with_graph(dc.model(golden, name, frames), graph, gw)
        _refs[key] = gbc.beam_search(m, K, S, float(golden(name)['lm_weights'][k]), lam, *terms)
    return _refs[key]


def tuples():
    for name, frames, k in tgb.PAIR_CASES:
        for K in BEAMS:
            for lam in LAMBDAS:
                for terms in TERMS:
                    for kind in KINDS:
                        yield name, frames, k, K, lam, terms, kind
    yield WIDE


def walk_is_forbidden(graph, text):
    s = graph.start
    for c in text:
        if graph.arc[s, c] == NEG:
            return True
        s = int(graph.next[s, c])
    return False


def judge(golden, t):
    """(the checker's result, compared?, a -inf arc removes a text of the plain search's list, the list differs from
    graph_weight = 0) of one tuple."""
    name, frames, k, K, lam, terms, kind = t
    graph = graph_of(golden, kind, name, frames, k)
    r = reference(golden, name, frames, k, K, lam, terms, graph)
    off = plain(golden, name, frames, k, K, lam, terms)
    compared = r['gap'] >= MIN_GAP and not (terms[1] != 0 and r['tau_gap'] < TAU_MARGIN)
    removed = any(walk_is_forbidden(graph, h[0]) for h in off['hyps'])
    return r, compared, removed, tgt.lists_of(off) != tgt.lists_of(r)


def measure(golden):
    """The checker-only counts over the grid (no GPU)."""
    n = compared = full = with_ctc = removed = differs = 0
    for t in tuples():
        r, ok, rem, dif = judge(golden, t)
        n += 1
        compared += ok
        full += ok and t[0] == tgb.FULL_CASE
        with_ctc += ok and t[4] > 0
        removed += ok and rem
        differs += ok and dif
    return n, compared, full, with_ctc, removed, differs


def kwargs_of(terms, lam, graph, gw=GW):
    return dict(tgt.kwargs_of(terms, lam), graph=graph, graph_weight=gw)


def arrays(asr):
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in asr.last_beam] + [asr.last_beam_steps.cpu().numpy(), asr.last_beam_graph.cpu().numpy()]


def check_against(r, out, nbest, lam, S=STEPS, where=''):
    """One utterance's results equal the checker's -> (worst |score error|, worst |graph part error|)."""
    chars, n_chars, scores, n_hyps, n_steps, parts = out
    hyps = r['hyps']
    assert int(n_hyps[0]) == len(hyps) == len(nbest) <= chars.shape[1], where
    assert int(n_steps[0]) == r['n_steps'], where
    worst = worst_part = 0.0
    for i, (ref_chars, ref_score, ended, was_capped, _) in enumerate(hyps):
        n, steps = int(n_chars[0, i]), min(ended + 1, S)
        assert n == len(ref_chars) and np.array_equal(chars[0, i, :n], ref_chars), (where, i)
        assert not chars[0, i, n:].any()
        assert nbest[i][0] == tgb.text_of(ref_chars) and nbest[i][1] == float(scores[0, i])
        err, perr = abs(float(scores[0, i]) - ref_score), abs(float(parts[0, i]) - r['parts'][i])
        print('    %d: %d steps, score %.6f (error %.2e), graph part %.6f (error %.2e)'
              % (i, steps, ref_score, err, r['parts'][i], perr))
        worst, worst_part = max(worst, err), max(worst_part, perr)
        assert err <= tgc.bound(steps, lam) + EPS * steps * max(1.0, abs(ref_score)), (where, i, err)
        assert perr <= EPS * steps * max(1.0, abs(r['parts'][i])), (where, i, perr)
    rest = slice(len(hyps), None)
    assert not chars[0, rest].any() and not n_chars[0, rest].any() and not scores[0, rest].any()
    assert not parts[0, rest].any()
    return worst, worst_part


def test_the_kernel_matches_the_float64_checker_over_the_grid(golden):
    n = compared = full = with_ctc = removed = differs = 0
    worst = worst_part = 0.0
    for t in tuples():
        name, frames, k, K, lam, terms, kind = t
        r, ok, rem, dif = judge(golden, t)
        n += 1
        tag = '%s frames %d lm %d K %d lambda %.1f terms %s graph %s' % t
        if not ok:
            print('%s: smallest gap %.2e, distance from tau %.2e, not compared' % (tag, r['gap'], r['tau_gap']))
            continue
        fx = golden(name)
        asr, lm = tgc.models(fx)
        w = float(fx['lm_weights'][k])
        x = torch.from_numpy(fx['x'][:, :frames]).to(DEV)
        graph = graph_of(golden, kind, name, frames, k)
        nbest = asr.decode_nbest([x], [[frames]], lm, Mapper(), w, K, max_decoding_steps=STEPS,
                                 **kwargs_of(terms, lam, graph))[0]
        out = arrays(asr)
        print('%s: smallest gap %.2e, %d hypotheses, %d steps' % (tag, r['gap'], len(r['hyps']), r['n_steps']))
        err, perr = check_against(r, out, nbest, lam, where=tag)
        worst, worst_part = max(worst, err), max(worst_part, perr)
        compared += 1
        full += name == tgb.FULL_CASE
        with_ctc += lam > 0
        removed += rem
        differs += dif
    print('%d of %d tuples compared: %d at full dimensions, %d with CTC, a -inf arc removes a text of the plain list in '
          '%d, the list differs from graph_weight = 0 in %d; worst |score error| %.3e, worst |graph part error| %.3e'
          % (compared, n, full, with_ctc, removed, differs, worst, worst_part))
    assert 2 * compared >= n and full >= 2 and with_ctc >= 3 and removed >= 3 and differs >= 3


def entry_args(golden, name, frames=40, lm_weight=0.5, steps=STEPS):
    fx = golden(name)
    asr, lm = tgc.models(fx)
    x = torch.from_numpy(fx['x'][:, :frames]).to(DEV)
    with torch.no_grad():
        feat, enc_lens = asr._encode_packed([x], [[frames]])
    return asr, (feat, enc_lens, asr._decoder_params(), (asr.attention.psi.weight, asr.attention.psi.bias), lm,
                 lm_weight, EOS, steps)


@pytest.mark.parametrize('K', [1, 3])
def test_weight_zero_is_the_kernel_without_a_graph_bit_for_bit(golden, K):
    from ss_asr_amd import ops
    for name in tgb.SMALL:
        asr, args = entry_args(golden, name)
        head = tgc.head_of(asr, 0.3)
        terms = tgt.kwargs_of(tgt.GRID[2])
        del terms['ctc_weight']
        graph = graph_of(golden, 'rand300', name, 40, 0)
        for ctc, kw, want in ((None, {}, ops.decode_beam(*args, K)), (head, {}, ops.decode_beam_ctc(*args, K, head)),
                              (None, terms, ops.decode_beam_ex(*args, K, None, **terms)),
                              (head, terms, ops.decode_beam_ex(*args, K, head, **terms))):
            want = [t.cpu().numpy() for t in want]
            for g in (graph, None):
                got = [t.cpu().numpy() for t in ops.decode_beam_graph(*args, K, ctc, graph=g, graph_weight=0.0, **kw)]
                assert len(got) == 6
                for a, b in zip(want, got):                          # the four results, and n_steps beside _ex's
                    assert a.dtype == b.dtype and np.array_equal(a, b)
                assert got[5].dtype == np.float32 and got[5].shape == (1, K) and not got[5].any()


def test_an_utterance_decodes_in_a_group_as_it_decodes_alone(golden):
    fx = golden(tgb.SMALL[0])
    asr, lm = tgc.models(fx)
    x = torch.from_numpy(fx['x']).to(DEV)
    other = torch.from_numpy(golden(tgb.SMALL[1])['x']).to(DEV)
    both = torch.cat([x, other, x, other], 1)
    xs = [both[:, :f] for f in (160, 40, 9)]                         # T' = 20, 5, 1
    lens = [[t.shape[1]] for t in xs]
    graph = graph_of(golden, 'rand300', tgb.SMALL[0], 40, 0)
    for lam in LAMBDAS:
        kw = kwargs_of(tgt.GRID[2], lam, graph)
        texts = asr.decode_many(xs, lens, lm, Mapper(), 0.5, max_decoding_steps=STEPS, beam_size=3, **kw)
        group = arrays(asr)
        assert group[0].shape == (3, 3, STEPS) and group[5].shape == (3, 3)
        assert asr.last_encoded_packed[1].cpu().tolist() == [20, 5, 1]
        for i, (t, l) in enumerate(zip(xs, lens)):
            assert asr.decode(t, l, lm, Mapper(), 0.5, max_decoding_steps=STEPS, beam_size=3, **kw) == texts[i]
            alone = arrays(asr)
            for a, b in zip(alone, group):
                assert np.array_equal(a[0], b[i]), (lam, i)
            nh = int(group[3][i])
            assert 1 <= nh <= 3 and np.isfinite(group[2][i, :nh]).all() and np.isfinite(group[5][i, :nh]).all()
            assert not group[0][i, nh:].any() and not group[2][i, nh:].any() and not group[5][i, nh:].any()


def test_a_cap_of_one_step_emits_the_arc_and_no_fin(golden):
    from ss_asr_amd import ops
    asr, args = entry_args(golden, tgb.SMALL[0], steps=1)
    graph = graph_of(golden, 'rand7', tgb.SMALL[0], 40, 0)
    s0 = graph.start
    chars, n_chars, scores, n_hyps, n_steps, parts = [
        t.cpu().numpy() for t in ops.decode_beam_graph(*args, 5, None, graph=graph, graph_weight=GW)]
    nh = int(n_hyps[0])
    assert nh == 5 and int(n_steps[0]) == 1 and chars.shape == (1, 5, 1)
    capped = 0
    for i in range(nh):
        if n_chars[0, i] == 0:                                       # <EOS> at the first step: the empty text, fin[start]
            assert parts[0, i] == graph.fin[s0]
        else:                                                        # capped: the arc alone, whatever fin[next] is
            c = int(chars[0, i, 0])
            assert np.isfinite(graph.arc[s0, c]) and parts[0, i] == graph.arc[s0, c]
            assert graph.fin[graph.next[s0, c]] != 0
            capped += 1
    assert capped >= 3 and np.all(np.diff(scores[0, :nh]) <= 0)


def test_canaries_and_every_output_element(golden):
    from ss_asr_amd import _lib, ops
    lib = _lib.load()
    asr, args = entry_args(golden, tgb.SMALL[0], frames=24)
    head = tgc.head_of(asr, 0.3)
    K, N = 5, 1
    graph = graph_of(golden, 'rand7', tgb.SMALL[0], 24, 0)
    feat = args[0]
    sizes = (N, K, feat.shape[1], feat.shape[2], *asr.attention.phi.weight.shape, graph.n_classes, args[4].hidden_size, STEPS)
    need = int(lib.ssasr_decode_beam_graph_ws_bytes(*sizes, 1, 1))
    assert need == int(lib.ssasr_decode_beam_ex_ws_bytes(*sizes, 1, 1)) > 0
    ws = torch.full((need // 4 + PAD,), 123.0, device=DEV)
    d, outs, keep = ops.beam_struct(*args, K, ws, ctc=True, coverage=True)
    d.ws_bytes = need
    shapes = dict(chars=(N * K * STEPS, torch.int32), n_chars=(N * K, torch.int32), hyp_scores=(N * K, torch.float32),
                  n_hyps=(N, torch.int32), n_steps=(N, torch.int32), graph_scores=(N * K, torch.float32))
    bufs = {k: torch.full((n + PAD,), -7, dtype=dt, device=DEV) for k, (n, dt) in shapes.items()}
    d.chars, d.n_chars, d.hyp_scores, d.n_hyps = (bufs[k].data_ptr() for k in ('chars', 'n_chars', 'hyp_scores', 'n_hyps'))
    terms = tgt.GRID[2]
    t = _lib.BeamTerms(terms[0], terms[1], terms[2], terms[3], bufs['n_steps'].data_ptr())
    c, c_keep = ops.ctc_prefix_struct(head)
    g, g_keep = graph.to(DEV)
    # a narrow beam whose list is short: K = 5 at T' = 3 leaves unused slots with the forbidden arcs of this graph or not;
    # either way every element of every output must have been written
    rc = lib.ssasr_decode_beam_graph(ctypes.byref(d), ctypes.byref(c), ctypes.byref(t), ctypes.byref(g), GW,
                                     bufs['graph_scores'].data_ptr(), ops._stream())
    assert rc == 0
    torch.cuda.synchronize()
    for k, (n, _) in shapes.items():
        host = bufs[k].cpu().numpy()
        assert (host[n:] == -7).all(), k                             # the canary behind the output
        assert not (host[:n] == -7).any(), k                         # every element written
    assert bool((ws[need // 4:] == 123.0).all())
    nh = int(bufs['n_hyps'][0])
    assert 1 <= nh <= K
    for k in ('n_chars', 'hyp_scores', 'graph_scores'):
        assert not bufs[k].cpu().numpy()[nh:N * K].any(), k
    assert not bufs['chars'].cpu().numpy()[nh * STEPS:N * K * STEPS].any()


def test_decode_nbest_with_a_hotword_and_what_follows_the_call(golden):
    from ss_asr_amd.char_graph import CharGraph
    mapper = Mapper()
    chosen = None
    for name, frames, k in tgb.PAIR_CASES:
        if name == tgb.FULL_CASE or chosen is not None:
            continue
        hyps = plain(golden, name, frames, k, 4)['hyps']
        if len(hyps) < 2 or not hyps[1][0] or 0 in hyps[1][0]:
            continue
        first, second = list(hyps[0][0]), list(hyps[1][0])
        if any(first[j:j + len(second)] == second for j in range(len(first) - len(second) + 1)):
            continue
        # a text without the phrase is paid nothing at the end, so the phrase passes the first text once bonus * len
        # exceeds its lead; texts that CONTAIN the phrase are paid the same, so the checker says whether it ends first
        bonus = (hyps[0][1] - hyps[1][1] + 0.5) / len(second)
        hot = CharGraph.hotwords([second], bonus, int(golden(name)['dims'][0]))
        r = reference(golden, name, frames, k, 4, 0.0, OFF, hot, 1.0)
        print('%s frames %d lm %d: hotword %r at bonus %.4g, the checker\'s first %r, gap %.3g'
              % (name, frames, k, second, bonus, r['hyps'][0][0], r['gap']))
        # (a capped text that IS the phrase has pend = 0: its part is bonus * len with or without fin)
        if list(r['hyps'][0][0]) == second and r['gap'] >= MIN_GAP:
            chosen = (name, frames, k, second, bonus, hot, r)
    assert chosen is not None
    name, frames, k, second, bonus, hot, r = chosen
    fx = golden(name)
    asr, lm = tgc.models(fx)
    w = float(fx['lm_weights'][k])
    x = torch.from_numpy(fx['x'][:, :frames]).to(DEV)
    nbest = asr.decode_nbest([x], [[frames]], lm, mapper, w, 4, max_decoding_steps=STEPS, graph=hot, graph_weight=1.0)[0]
    out = arrays(asr)
    check_against(r, out, nbest, 0.0, where='hotword')
    assert nbest[0][0] == tgb.text_of(second)
    assert abs(float(out[5][0, 0]) - bonus * len(second)) <= 1e-5 * bonus * len(second)
    assert asr.last_hyp_scores is asr.last_beam[2] and asr.last_beam_graph.shape == (1, 4)
    # score, mbr and rescore follow the call
    assert len(asr.score([nbest[0][0]], mapper)) == 1
    assert all(0 <= m.k < 4 for m in asr.mbr(mapper, unit='char'))
    again = asr.rescore(mapper, rnn_lm=lm, lm_weight=w)
    assert len(again) == 1 and {t for t, _ in again[0]} == {t for t, _ in nbest}
    # decode_mbr passes the keywords through; a call without a graph forgets the parts and takes today's path
    assert len(asr.decode_mbr([x], [[frames]], lm, mapper, w, 4, max_decoding_steps=STEPS, graph=hot, graph_weight=1.0)) == 1
    assert asr.last_beam_graph is not None
    base = asr.decode_nbest([x], [[frames]], lm, mapper, w, 4, max_decoding_steps=STEPS)
    kept = [t.cpu().numpy() for t in asr.last_beam]
    assert asr.last_beam_graph is None
    assert base == asr.decode_nbest([x], [[frames]], lm, mapper, w, 4, max_decoding_steps=STEPS, graph=hot)
    assert asr.last_beam_graph is None
    for a, b in zip(kept, asr.last_beam):
        assert np.array_equal(a, b.cpu().numpy())
    assert asr.decode(x, [frames], lm, mapper, w, max_decoding_steps=STEPS, graph=hot, graph_weight=1.0, beam_size=1) \
        == asr.decode_nbest([x], [[frames]], lm, mapper, w, 1, max_decoding_steps=STEPS, graph=hot, graph_weight=1.0)[0][0][0]
    assert asr.last_beam[0].shape[1] == 1 and asr.last_beam_graph.shape == (1, 1)      # width 1: the beam kernel at K = 1


def test_asr_tester_with_the_graph_keys(tmp_path):
    from ss_asr_amd.ASRDataset import prepare_x
    from ss_asr_amd.char_graph import CharGraph
    from ss_asr_amd.trainer import ASRTester
    fx = np.load(os.path.join(GOLDEN, 'dataset_ref.npz'), allow_pickle=False)
    dims = [int(v) for v in fx['cpt_dims']]
    root = str(tmp_path)
    index, lens = make_corpus(root, n=5, t_max=40, feat=dims[4], seed=5)
    os.makedirs(os.path.join(root, 'result', 'dec'))
    shutil.copy(os.path.join(GOLDEN, 'ref_small_asr.cpt'), os.path.join(root, 'result', 'dec', 'asr.cpt'))

    def tester(**keys):
        config = {'asr': dict({'mdl': {'encoder_state_size': dims[1], 'decoder_state_size': dims[2],
                                       'mlp_out_size': dims[3], 'feature_dim': dims[4], 'tf_rate': 1.0},
                               'test_index': index, 'decode_lm_weight': 0.5, 'decode_beam_size': 3, 'decode_jobs': 1,
                               'max_decode_step_ratio': 0.25, 'loader_jobs': 0}, **keys),
                  'char_lm': {'mdl': {'hidden_size': 16}}}
        paras = types.SimpleNamespace(name='dec', logdir=os.path.join(root, 'runs'), ckpdir=os.path.join(root, 'result'),
                                      verbose=False, seed=1)
        torch.manual_seed(3)
        t = ASRTester(config, paras)
        t.load_data()
        t.set_model()
        t.decode_group = 2
        return t
    old = tester()
    assert old.decode_file == 'decode_beam_3_len_0.25_lm0.5' and old.decode_beam_graph is None
    base = old.exec()
    assert old.asr_model.last_beam_graph is None
    xs, x_lens = [], []
    for x, _ in old.test_set:
        x, l = prepare_x(x, old.device)
        xs.append(x[:, :l[0]])
        x_lens.append(l)
    assert base == old.asr_model.decode_many(xs, x_lens, old.lm, old.mapper, 0.5, beam_size=3)
    mapper = old.mapper
    V = mapper.get_dim()
    lm_path = os.path.join(root, 'ngram.npz')
    ngram = CharGraph.ngram([[mapper.char_to_ind(c) for c in w] for w in ('hello', 'halló', 'hold')], 3, V, 1)
    ngram.save(lm_path)
    t = tester(decode_hotwords=['hold', 'hal'], decode_hotword_bonus=1.5, decode_ngram_lm=lm_path,
               decode_ngram_weight=0.25, decode_length_bonus=0.5)
    assert t.decode_file == 'decode_beam_3_len_0.25_lm0.5_hw2x1.5_ng0.25_lb0.5'
    t.lm = old.lm                                                    # the same freshly initialised LM
    said = []
    t.verbose = said.append
    got = t.exec()
    assert 'character graph' in said[0] and len(got) == 5 and t.asr_model.last_beam_graph is not None
    hot = CharGraph.hotwords([[mapper.char_to_ind(c) for c in w] for w in ('hold', 'hal')], 1.5, V)
    both = CharGraph.product(ngram.scaled(0.25), hot)
    assert got == t.asr_model.decode_many(xs, x_lens, t.lm, mapper, 0.5, beam_size=3, length_bonus=0.5, graph=both,
                                          graph_weight=1.0)
    one = tester(decode_ngram_lm=lm_path)
    assert one.decode_file == 'decode_beam_3_len_0.25_lm0.5_ng0.5' and one.decode_beam_graph[1] == 0.5
    one.lm = old.lm
    assert one.exec() == one.asr_model.decode_many(xs, x_lens, one.lm, mapper, 0.5, beam_size=3, graph=ngram,
                                                   graph_weight=0.5)
    again = tester()
    again.lm = old.lm
    assert again.decode_file == old.decode_file and again.exec() == base


if __name__ == '__main__':
    def load(name):
        return np.load(os.path.join(GOLDEN, name + '.npz'), allow_pickle=False)
    print('tuples %d: compared %d, at full dimensions %d, with CTC %d, a -inf arc removes a plain text %d, the list '
          'differs %d' % measure(load))
