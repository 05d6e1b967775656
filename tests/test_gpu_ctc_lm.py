"""ssasr_ctc_decode_lm on the GPU (ctc_prefix_beam_lm_kernel, csrc/infer.hip): the CTC prefix beam search with the
CharLM in the ranking, held to postprocess.ctc_prefix_beam_lm_reference, the float64 restatement that
tests/test_ctc_lm_cpu.py pins.

Cases.  Logits 4 N(0, 1) from default_rng([T, V, seed]), LM weights scale N(0, 1) from default_rng([V, H, seed, 7]) drawn
in struct ssasr_charlm's field order, seeds 0..15, lm_weight 0.5, length_bonus 0.3, eos = V - 1, over CELLS at (H, scale) =
(8, 0.5) and (40, 0.3), plus (T' 5, V 8, K 3, H 260, scale 0.1): matmat's k-loop then takes its second 256-column pass.
K = 32 at T' = 5 puts up to 32 new members, four helper passes, into one frame.
A case is compared when the checker's gap (on the fused keys and between adjacent final totals) is >= MIN_GAP = 1e-3,
the project's rule; at most a quarter of the cases may be skipped and no cell entirely.  The checker alone (this file's
__main__, on the CPU): 673 of 704 compared, worst cell 11 of 16; the H = 260 cell 16 of 16.
A compared case must hold the checker's SET of texts, in the kernel's own non-increasing order, with the fused score and
each part within BOUND = 8 * NOISE.  NOISE = max |float32 - float64| of the checker run in float32, LM included, over
the compared hypotheses' totals and parts, measured by __main__: 8.9e-5 (the T' = 80 cell at H = 8).  The kernel's worst error on the MI355X is
recorded beside it (KERNEL_WORST): 1.9e-5.
Zero weights are bit-equal to ssasr_ctc_decode on every cell; an utterance alone is bit-equal to itself in a group."""
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
LMS = [(8, 0.5), (40, 0.3)]
WIDE = (5, 8, 3, 260, 0.1)                                       # T', V, K, H, scale
ALPHA, BETA = 0.5, 0.3
NOISE = 8.9e-5                                                   # measure_noise(), on the CPU
BOUND = 8 * NOISE
KERNEL_WORST = 1.9e-5                                            # worst |kernel - float64| seen on the MI355X
CANARY_I, CANARY_F = -77, 12345.0
PAD = 64                                                         # canary elements behind every output
SCORE_ATOL = 5e-5                                                # per step: test_gpu_rescore's bound


def logits_of(T, V, seed):
    return (4.0 * np.random.default_rng([T, V, seed]).standard_normal((T, V))).astype(np.float32)


def lm_of(V, H, seed, scale):
    """The CharLM's eleven arrays in the struct's field order, float32."""
    rng = np.random.default_rng([V, H, seed, 7])
    shapes = [(V, H), (3 * H, H), (3 * H, H), (3 * H,), (3 * H,), (3 * H, H), (3 * H, H), (3 * H,), (3 * H,), (V, H), (V,)]
    return [(scale * rng.standard_normal(s)).astype(np.float32) for s in shapes]


def log_softmax(z, dtype=np.float64):
    z = z.astype(dtype)
    m = z.max(-1, keepdims=True)
    return z - (m + np.log(np.exp(z - m).sum(-1, keepdims=True, dtype=dtype)))


_refs = {}


def reference(key, z, K, lm, alpha=ALPHA, beta=BETA, eos=None, blank=0):
    """(hyps, gap, parts) of the checker on float64 log_softmax(z), computed once per key."""
    from ss_asr_amd.postprocess import ctc_prefix_beam_lm_reference
    eos = z.shape[1] - 1 if eos is None else eos
    full = (key, K, alpha, beta, eos, blank)
    if full not in _refs:
        parts = []
        hyps, gap = ctc_prefix_beam_lm_reference(log_softmax(z), K, lm, alpha, beta, eos, blank, parts=parts)
        _refs[full] = (hyps, gap, parts)
    return _refs[full]


def noise_of(z, K, lm):
    """max |float32 - float64| of the totals and parts over the texts both runs of the checker hold (None: the case is
    not compared)."""
    from ss_asr_amd.postprocess import ctc_prefix_beam_lm_reference
    eos = z.shape[1] - 1
    parts = []
    hyps, gap = ctc_prefix_beam_lm_reference(log_softmax(z), K, lm, ALPHA, BETA, eos, parts=parts)
    if gap < MIN_GAP:
        return None
    parts32 = []
    hyps32, _ = ctc_prefix_beam_lm_reference(log_softmax(z, np.float32), K, lm, ALPHA, BETA, eos, dtype=np.float32,
                                             parts=parts32)
    low = {t: (s,) + p for (t, s), p in zip(hyps32, parts32)}
    return max([0.0] + [abs(a - b) for (t, s), p in zip(hyps, parts) if t in low for a, b in zip((s,) + p, low[t])])


def measure_noise():
    worst, done = 0.0, 0
    for H, scale in LMS:
        for T, V, K in CELLS:
            cell = [n for n in (noise_of(logits_of(T, V, s), K, lm_of(V, H, s, scale)) for s in SEEDS) if n is not None]
            worst, done = max([worst] + cell), done + len(cell)
            print('H=%d T=%d V=%d K=%d: %d of %d compared, noise %.3g' % (H, T, V, K, len(cell), len(SEEDS), max(cell)),
                  flush=True)
    print('%d of %d compared' % (done, len(LMS) * len(CELLS) * len(SEEDS)))
    T, V, K, H, scale = WIDE
    cell = [n for n in (noise_of(logits_of(T, V, s), K, lm_of(V, H, s, scale)) for s in SEEDS) if n is not None]
    print('H=%d T=%d V=%d K=%d: %d of %d compared, noise %.3g' % (H, T, V, K, len(cell), len(SEEDS), max(cell)))
    print('NOISE: %.4g' % max([worst] + cell))


def lm_struct(lm):
    """(_lib.CharLM on the device, the tensors it points into) of lm_of's arrays."""
    from ss_asr_amd import _lib
    keep = [torch.from_numpy(a).to(DEV) for a in lm]
    return _lib.CharLM(lm[0].shape[0], lm[0].shape[1], *[t.data_ptr() for t in keep]), keep


def run(z, frame_lens, K, lm, alpha=ALPHA, beta=BETA, eos=None, blank=0):
    """ssasr_ctc_decode_lm on z [B, T, V] through the C entry, every output and the workspace followed by PAD canaries
    and pre-filled, so that an element the kernel leaves unwritten or writes past its end shows.  -> per row the list
    of (text, total, ctc, lm) and the raw arrays."""
    import ctypes
    from ss_asr_amd import _lib, ops
    lib = _lib.load()
    B, T, V = z.shape
    eos = V - 1 if eos is None else eos
    H = lm[0].shape[1] if (lm is not None and alpha != 0) else 0
    need = int(lib.ssasr_ctc_decode_lm_ws_bytes(B, T, V, K, H))
    assert need > 0 and need % 4 == 0
    s, keep = lm_struct(lm) if lm is not None else (None, None)
    logits = torch.from_numpy(np.ascontiguousarray(z)).to(DEV)
    lens = torch.tensor(list(frame_lens), dtype=torch.int32, device=DEV)
    ws = torch.full((need // 4 + PAD,), CANARY_I, dtype=torch.int32, device=DEV)
    ints = {'chars': B * K * T, 'n_chars': B * K, 'n_hyps': B}
    flts = {'scores': B * K, 'ctc_scores': B * K, 'lm_scores': B * K}
    buf = {n: torch.full((c + PAD,), CANARY_I, dtype=torch.int32, device=DEV) for n, c in ints.items()}
    buf.update({n: torch.full((c + PAD,), CANARY_F, dtype=torch.float32, device=DEV) for n, c in flts.items()})
    ops.check(lib.ssasr_ctc_decode_lm(ops._p(logits), ops._p(lens), B, T, V, K, blank, ops._p(ws), need, ops._p(buf['chars']),
                                      ops._p(buf['n_chars']), ops._p(buf['scores']), ops._p(buf['n_hyps']),
                                      ctypes.byref(s) if s is not None else None, alpha, beta, eos,
                                      ops._p(buf['ctc_scores']), ops._p(buf['lm_scores']), ops._stream()),
              'ssasr_ctc_decode_lm')
    torch.cuda.synchronize()
    assert (ws.cpu().numpy()[need // 4:] == CANARY_I).all(), 'ws: written past its end'
    raw = {}
    for name, count in list(ints.items()) + list(flts.items()):
        arr = buf[name].cpu().numpy()
        canary = CANARY_I if name in ints else CANARY_F
        assert (arr[count:] == canary).all(), name + ': written past its end'
        assert not (arr[:count] == canary).any(), name + ': an element was left unwritten'
        raw[name] = arr[:count].reshape((B, K, T) if name == 'chars' else (B,) if name == 'n_hyps' else (B, K))
    raw['lm_frames'] = ws.cpu().numpy()[need // 4 - B:need // 4]
    out = []
    for b in range(B):
        n_h = raw['n_hyps'][b]
        assert 0 <= n_h <= K
        for k in range(K):
            n = raw['n_chars'][b, k]
            assert 0 <= n <= T and (raw['chars'][b, k, n:] == 0).all()
            if k >= n_h:
                assert n == 0 and raw['scores'][b, k] == -math.inf and raw['ctc_scores'][b, k] == -math.inf
                assert raw['lm_scores'][b, k] == 0.0
        out.append([(tuple(int(c) for c in raw['chars'][b, k, :raw['n_chars'][b, k]]), float(raw['scores'][b, k]),
                     float(raw['ctc_scores'][b, k]), float(raw['lm_scores'][b, k])) for k in range(n_h)])
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


def run_cells(cells, H, scale):
    compared, worst = {}, 0.0
    for T, V, K in cells:
        compared[(T, V, K, H)] = 0
        for s in SEEDS:
            z, lm = logits_of(T, V, s), lm_of(V, H, s, scale)
            want, gap, parts = reference((T, V, s, H), z, K, lm)
            got, raw = run(z[None], [T], K, lm)
            assert 0 <= raw['lm_frames'][0] <= T
            if gap < MIN_GAP:
                continue
            compared[(T, V, K, H)] += 1
            worst = max(worst, check_row(got[0], want, parts, BOUND))
    return compared, worst


@pytest.mark.parametrize('H,scale', LMS)
def test_the_kernel_matches_the_checker_on_every_compared_case(H, scale):
    compared, worst = run_cells(CELLS, H, scale)
    total, done = len(CELLS) * len(SEEDS), sum(compared.values())
    print('compared per cell (of %d): %s' % (len(SEEDS), compared))
    print('H = %d: %d of %d cases compared, worst |kernel - float64| %.3g (NOISE %.3g, bound %.3g)'
          % (H, done, total, worst, NOISE, BOUND))
    assert all(n > 0 for n in compared.values())
    assert total - done <= total // 4


def test_a_hidden_size_past_one_pass_of_the_k_loop():
    T, V, K, H, scale = WIDE
    compared, worst = run_cells([(T, V, K)], H, scale)
    print('H = %d: %d of %d compared, worst |kernel - float64| %.3g (bound %.3g)'
          % (H, compared[(T, V, K, H)], len(SEEDS), worst, BOUND))
    assert compared[(T, V, K, H)] >= 12


def test_zero_weights_are_ssasr_ctc_decode_bit_for_bit_on_every_cell():
    for T, V, K in CELLS:
        z = np.stack([logits_of(T, V, s) for s in SEEDS])
        chars, n_chars, scores, n_hyps = plain(z, [T] * len(SEEDS), K)
        for lm in (None, lm_of(V, 8, 0, 0.5)):                   # with a model at weight 0: unread, no LM step
            _, raw = run(z, [T] * len(SEEDS), K, lm, alpha=0.0, beta=0.0)
            assert np.array_equal(raw['chars'], chars) and np.array_equal(raw['n_chars'], n_chars), (T, V, K)
            assert np.array_equal(raw['n_hyps'], n_hyps)
            assert np.array_equal(bits(raw['scores']), bits(scores)) and np.array_equal(bits(raw['ctc_scores']), bits(scores))
            assert (raw['lm_scores'] == 0.0).all() and (raw['lm_frames'] == 0).all()


@pytest.mark.parametrize('K', [2, 8])
def test_an_utterance_decodes_in_a_group_as_it_decodes_alone(K):
    lens = [20, 5, 1]
    lm = lm_of(8, 40, 3, 0.3)
    z = np.stack([logits_of(20, 8, 200 + i) for i in range(len(lens))])
    _, group = run(z, lens, K, lm)
    for i, n in enumerate(lens):
        _, alone = run(z[i:i + 1, :n], [n], K, lm)
        for name in ('n_chars', 'n_hyps', 'scores', 'ctc_scores', 'lm_scores', 'lm_frames'):
            assert np.array_equal(bits(alone[name][0]), bits(group[name][i])), name
        assert np.array_equal(alone['chars'][0], group['chars'][i, :, :n]) and (group['chars'][i, :, n:] == 0).all()


@pytest.mark.parametrize('K', [1, 3, 8])
def test_edges(K):
    """Lengths 0, 1 and past T', blank 3, eos < 0 (no end term) and a length bonus alone (no LM step)."""
    T, V = 20, 8
    lm = lm_of(V, 8, 5, 0.5)
    rows = [('no frames', logits_of(T, V, 100), 0), ('one frame', logits_of(T, V, 101), 1),
            ('length past the rows', logits_of(T, V, 102), 25), ('whole', logits_of(T, V, 103), 20)]
    for blank, eos, alpha, beta in ((0, V - 1, ALPHA, BETA), (3, V - 1, ALPHA, BETA), (0, -1, ALPHA, BETA),
                                    (0, V - 1, 0.0, BETA), (0, V - 1, -0.25, 0.0)):
        got, raw = run(np.stack([r[1] for r in rows]), [r[2] for r in rows], K, lm, alpha, beta, eos, blank)
        for (name, z, n), mine in zip(rows, got):
            want, gap, parts = reference(name, z[:min(n, T)], K, lm, alpha, beta, eos, blank)
            if gap >= MIN_GAP:
                check_row(mine, want, parts, BOUND)
            if name == 'no frames':                              # the empty text alone: the end term is its whole score
                assert len(mine) == 1 and mine[0][0] == () and mine[0][2] == 0.0
                assert abs(mine[0][1] - want[0][1]) <= BOUND
        if alpha == 0.0:
            assert (raw['lm_frames'] == 0).all() and (raw['lm_scores'] == 0.0).all()
        else:
            assert raw['lm_frames'][0] == 0 and raw['lm_frames'][3] >= 1


def test_ops_is_the_entry_and_rejects_what_the_entry_rejects():
    from ss_asr_amd import ops
    from ss_asr_amd.charlm import CharLM
    V, H = 8, 8
    arrays = lm_of(V, H, 1, 0.5)
    lm = CharLM(V, H).to(DEV)
    with torch.no_grad():
        for name, a in zip(ops._CHARLM_NAMES, arrays):
            dict(lm.named_parameters())[name].copy_(torch.from_numpy(a))
    zs = np.stack([logits_of(20, V, s) for s in range(3)])
    lens = torch.tensor([20, 7, 0], dtype=torch.int32, device=DEV)
    out = ops.ctc_decode_lm(torch.from_numpy(zs).to(DEV), lens, 5, lm, ALPHA, BETA, V - 1)
    _, raw = run(zs, [20, 7, 0], 5, arrays)
    for name, arr in raw.items():
        assert np.array_equal(bits(out[name].cpu().numpy()), bits(arr)), name
    with pytest.raises(ValueError, match='no kernel'):
        ops.ctc_decode_lm(torch.zeros(1, 4097, V, device=DEV), lens[:1], 2, lm, 0.5)
    with pytest.raises(ValueError, match='classes'):
        ops.ctc_decode_lm(torch.zeros(1, 8, 9, device=DEV), lens[:1], 2, lm, 0.5)


def test_decode_ctc_with_the_lm_two_pass_and_the_tester_keys(golden, tmp_path):
    import las_oracle as lo
    import test_gpu_ctc_decode as tcd
    import test_gpu_rescore as tgr
    from conftest import GOLDEN
    from test_host_cpu import make_corpus
    from ss_asr_amd import ops
    from ss_asr_amd.ASRDataset import Mapper
    from ss_asr_amd.ctc import JointCTCASR
    from ss_asr_amd.trainer import ASRTester
    fx = golden(tgr.SMALL)
    asr, lm = tcd.models(fx)
    mapper, w = Mapper(), 0.5
    eos = int(mapper.char_to_ind('>'))
    xs, x_lens = tgr.ctc_groups(fx, (40, 24, 8), 3)
    nbest = asr.decode_ctc(xs, x_lens, mapper, beam_size=3, rnn_lm=lm, lm_weight=w)
    assert len(asr.last_ctc_decode) == 7 and asr.last_hyp_scores is asr.last_ctc_decode[2]
    chars, n_chars, scores, n_hyps, logits, ctc_s, lm_s = [t.cpu().numpy() for t in asr.last_ctc_decode]
    frames = asr.last_encoded_packed[1].cpu().tolist()
    arrays = [dict(lm.named_parameters())[n].detach().cpu().numpy() for n in ops._CHARLM_NAMES]
    compared = 0
    for i in range(3):
        n = int(n_hyps[i])
        assert [s for _, s in nbest[i]] == scores[i, :n].tolist()
        want, gap, parts = reference(('model', i), logits[i, :frames[i]], 3, arrays, w, 0.0, eos)
        if gap >= MIN_GAP:                                       # the CTC part is the LM checker's CTC part
            compared += 1
            mine = [(tuple(int(c) for c in chars[i, k, :n_chars[i, k]]), float(scores[i, k]), float(ctc_s[i, k]),
                     float(lm_s[i, k])) for k in range(n)]
            check_row(mine, want, parts, BOUND)
    assert compared >= 2
    # the LM part is what ASR.rescore reports for the same texts
    first_total = asr.last_ctc_decode[2].clone()
    asr.rescore(mapper, rnn_lm=lm, lm_weight=w, att_weight=0.0, first_weight=0.0)
    order, total, parts_r = [t.cpu().numpy() for t in asr.last_rescore]
    for i in range(3):
        for rank in range(int(n_hyps[i])):
            k = int(order[i, rank])
            assert abs(float(parts_r[i, rank, 1]) - float(lm_s[i, k])) <= SCORE_ATOL * (int(n_chars[i, k]) + 1)
    # two passes with the LM in the first: decode_ctc with the LM, then rescore on the CTC part
    two = asr.decode_two_pass(xs, x_lens, lm, mapper, w, beam_size=3, ctc_weight=0.3, first_lm_weight=w)
    kept = [t.clone() for t in asr.last_rescore + asr.last_hyps]
    asr.decode_ctc(xs, x_lens, mapper, beam_size=3, rnn_lm=lm, lm_weight=w)
    assert np.array_equal(asr.last_ctc_decode[2].cpu().numpy().view(np.int32), first_total.cpu().numpy().view(np.int32))
    asr.last_hyp_scores = asr.last_ctc_decode[5]
    again = asr.rescore(mapper, rnn_lm=lm, lm_weight=w, att_weight=1.0 - 0.3, first_weight=0.3)
    assert two == again
    for a, b in zip(kept, asr.last_rescore + asr.last_hyps):
        assert a.dtype == b.dtype and np.array_equal(a.cpu().numpy().view(np.int32), b.cpu().numpy().view(np.int32))
    order2, parts2 = asr.last_rescore[0].cpu().numpy(), asr.last_rescore[2].cpu().numpy()
    for i in range(3):                                           # rescore's `first` part is the pure CTC score
        for rank in range(int(n_hyps[i])):
            assert parts2[i, rank, 2] == ctc_s[i, order2[i, rank]]
    # score, mbr and align follow it
    tops = [h[0][0] for h in two]
    assert len(asr.score(tops, mapper)) == 3
    assert all(0 <= m.k < 3 for m in asr.mbr(mapper, unit='char'))
    assert len(asr.align(xs, x_lens, tops, mapper, encoded=asr.last_encoded_packed)) == 3
    # the default keywords take the old entry
    asr.decode_ctc(xs, x_lens, mapper, beam_size=3)
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
    from ss_asr_amd.ASRDataset import prepare_x
    old = tester(decode_ctc_only={'beam_size': 4})
    assert old.decode_file == 'decode_beam_3_len_0.25_lm0.5_ctconly4'
    base = old.exec()
    assert len(old.asr_model.last_ctc_decode) == 5
    zero = tester(decode_ctc_only={'beam_size': 4, 'lm_weight': 0.0})
    assert zero.decode_file == old.decode_file and zero.exec() == base
    t = tester(decode_ctc_only={'beam_size': 4, 'lm_weight': 0.5, 'length_bonus': 0.25}, decode_score=True)
    assert t.decode_file == 'decode_beam_3_len_0.25_lm0.5_ctconly4_clm0.5_clb0.25'
    got = t.exec()
    assert len(got) == 5 and len(t.last_scores) == 5 and len(t.asr_model.last_ctc_decode) == 7
    direct = []
    for x, _ in t.test_set:
        x, l = prepare_x(x, t.device)
        direct.append(t.asr_model.decode_ctc([x[:, :l[0]]], [l], t.mapper, beam_size=4, rnn_lm=t.lm, lm_weight=0.5,
                                             length_bonus=0.25)[0][0][0])
    assert got == direct
    tr = tester(decode_ctc_only={'beam_size': 4, 'lm_weight': 0.5}, decode_rescore={'ctc_weight': 0.3})
    assert tr.decode_file == 'decode_beam_3_len_0.25_lm0.5_ctconly4_clm0.5_rescore0.3'
    assert len(tr.exec()) == 5 and len(tr.asr_model.last_ctc_decode) == 7


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    measure_noise()
