"""N-best rescoring on the GPU: ssasr_rescore against postprocess.rescore_reference (float64) on the seeded synthetic
cases of tests/test_rescore_cpu.py, and ASR.rescore / decode_two_pass / ASRTester's asr.decode_rescore end to end on
the small model and on the real widths against the float64 oracle model of tests/decode_checker.py.

Kernel bound.  The rule of test_gpu_ctc_search.py: NOISE[shape] = max |checker in float32 - checker in float64| over
the totals and parts of the shape's cases, measured on the CPU by `python tests/test_rescore_cpu.py` (the smaller of
the figures with and without the LM term); the bound is 8 * NOISE.  Every case is compared: synthetic_case redraws a
seed whose smallest gap between adjacent totals is under 1e-3 (none of these shapes needs a second draw), so `order`
must be EQUAL everywhere.
End to end.  A step's score row is held to SCORE_ATOL = 5e-5 (test_gpu_decode), a teacher-forced sum over s steps to
5e-5 * s."""
import math
import os
import types

import numpy as np
import pytest
import torch

import decode_checker as dc
import test_gpu_ctc_decode as tcd
import test_gpu_decode as tgd
import test_rescore_cpu as trc
from ss_asr_amd.postprocess import rescore_reference

pytestmark = pytest.mark.gpu

DEV = tgd.DEV
Mapper = tgd.Mapper
SCORE_ATOL = tgd.SCORE_ATOL
EOS = dc.EOS
STEPS = 24
NOISE = {(1, 1, 1, 2): 1.15e-7, (3, 4, 9, 31): 4.3e-6, (2, 32, 70, 64): 1.9e-4, (33, 2, 5, 50): 4.8e-6}
CANARY_I, CANARY_F = -77, 12345.0
PAD = 64
SMALL = trc.small_name()
FULL = 'decode_full_s6'


def launch(c, lm_mode, weights):
    """ssasr_rescore on a synthetic case through the C entry, every output and the workspace followed by PAD canaries
    and pre-filled.  lm_mode None | 'step' ([U][R][V], charlm_chunk's layout) | 'row' ([R][U][V] with padded steps)."""
    from ss_asr_amd import _lib, ops
    lib = _lib.load()
    G, K, U, V, M, steps = (c[n] for n in ('G', 'K', 'U', 'V', 'M', 'steps'))
    R = G * M
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    logits, rows, n_hyps, first, chars, n_chars = (dev(c[n]) for n in ('logits', 'rows', 'n_hyps', 'first', 'chars', 'n_chars'))
    lm, lm_row, lm_step = None, 0, 0
    if lm_mode == 'step':
        lm, lm_row, lm_step = dev(c['lm_logits'].transpose(1, 0, 2)), V, R * V
    elif lm_mode == 'row':
        lm = torch.full((R, U, V + 3), CANARY_F, device=DEV)
        lm[:, :, :V] = dev(c['lm_logits'])
        lm_row, lm_step = U * (V + 3), V + 3
    need = int(lib.ssasr_rescore_ws_bytes(G, K, U))
    assert need >= 0 and (need > 0) == (2 * K * U > 4096)
    full = lambda n, v, t: torch.full((n + PAD,), v, dtype=t, device=DEV)
    ws = full(need // 8, CANARY_F, torch.float64)
    outs = dict(order=full(G * K, CANARY_I, torch.int32), total=full(G * K, CANARY_F, torch.float32),
                parts=full(G * K * 3, CANARY_F, torch.float32), chars_out=full(G * K * steps, CANARY_I, torch.int32),
                n_chars_out=full(G * K, CANARY_I, torch.int32), n_hyps_out=full(G, CANARY_I, torch.int32))
    ops.check(lib.ssasr_rescore(ops._p(logits), ops._p(lm), lm_row, lm_step, ops._p(rows), rows.stride(0), rows.shape[1],
                                ops._p(n_hyps), ops._p(first), ops._p(chars), ops._p(n_chars), G, M, K, U, V, steps,
                                weights['att_weight'], weights['lm_weight'], weights['first_weight'],
                                weights['length_bonus'], ops._p(ws) if need else None, need, *[ops._p(t) for t in outs.values()],
                                ops._stream()), 'ssasr_rescore')
    torch.cuda.synchronize()
    assert (ws.cpu().numpy()[need // 8:] == CANARY_F).all(), 'ws: written past its end'
    res = {}
    for name, t in outs.items():
        arr, n = t.cpu().numpy(), t.numel() - PAD
        assert (arr[n:] == (CANARY_I if arr.dtype == np.int32 else CANARY_F)).all(), name + ': written past its end'
        assert not (arr[:n] == (CANARY_I if arr.dtype == np.int32 else CANARY_F)).any(), name + ': an element was left unwritten'
        res[name] = arr[:n]
    return (res['order'].reshape(G, K), res['total'].reshape(G, K), res['parts'].reshape(G, K, 3),
            res['chars_out'].reshape(G, K, steps), res['n_chars_out'].reshape(G, K), res['n_hyps_out'])


def check_case(c, ref, got, bound):
    """Order, list and figures of one case against the float64 reference -> the worst |error|."""
    order, total, parts, chars, n_chars, n_hyps = got
    G, K = c['G'], c['K']
    worst = 0.0
    assert order.tolist() == ref[0]
    for g in range(G):
        n = min(max(int(c['n_hyps'][g]), 0), K)
        assert n_hyps[g] == n
        for rank in range(K):
            k = order[g, rank]
            if rank >= n:
                assert k == -1 and total[g, rank] == 0 and not parts[g, rank].any() and n_chars[g, rank] == 0
                assert not chars[g, rank].any()
                continue
            length = int(c['n_chars'][g, k])
            assert n_chars[g, rank] == length and np.array_equal(chars[g, rank, :length], c['chars'][g, k, :length])
            assert not chars[g, rank, length:].any()
            assert parts[g, rank, 2] == c['first'][g, k]
            err = max([abs(float(total[g, rank]) - ref[1][g][rank])] +
                      [abs(float(a) - b) for a, b in zip(parts[g, rank], ref[2][g][rank])])
            worst = max(worst, err)
        assert all(total[g, i] >= total[g, i + 1] for i in range(n - 1))
    assert worst <= bound, (worst, bound)
    return worst


@pytest.mark.parametrize('lm_mode', [None, 'step', 'row'])
@pytest.mark.parametrize('shape', trc.SHAPES, ids=lambda s: '%dx%dx%dx%d' % s[:4])
def test_the_kernel_matches_the_float64_restatement(shape, lm_mode):
    G, K, U, V, n_hyps = shape
    c, ref, draws = trc.synthetic_case(G, K, U, V, n_hyps, lm_mode is not None)
    weights = dict(trc.WEIGHTS, lm_weight=trc.WEIGHTS['lm_weight'] if lm_mode else 0.0)
    bound = 8 * NOISE[shape[:4]]
    worst = check_case(c, ref, launch(c, lm_mode, weights), bound)
    print('G=%d K=%d U=%d V=%d lm %s: %d draw(s), worst |kernel - float64| %.3g (NOISE %.3g, bound %.3g)'
          % (G, K, U, V, lm_mode, draws, worst, NOISE[shape[:4]], bound))


@pytest.mark.parametrize('shape', [trc.SHAPES[1], trc.SHAPES[2]], ids=['lds', 'workspace'])
def test_an_utterance_alone_is_bit_equal_to_itself_in_a_group(shape):
    G, K, U, V, _ = shape
    G = 3
    c, _, _ = trc.synthetic_case(G, K, U, V, None, True)
    weights = dict(trc.WEIGHTS)
    group = launch(c, 'step', weights)
    M = c['M']
    for g in range(G):
        one = dict(c, G=1, logits=c['logits'][g * M:(g + 1) * M], lm_logits=c['lm_logits'][g * M:(g + 1) * M],
                   rows=c['rows'][g * M:(g + 1) * M], n_hyps=c['n_hyps'][g:g + 1], first=c['first'][g:g + 1],
                   chars=c['chars'][g:g + 1], n_chars=c['n_chars'][g:g + 1])
        alone = launch(one, 'step', weights)
        for a, b in zip(alone, group):
            assert np.array_equal(a[0].view(np.int32), b[g].view(np.int32))


def test_duplicated_rows_get_bit_equal_totals_in_slot_order():
    from ss_asr_amd import ops
    c, _, _ = trc.synthetic_case(2, 6, 9, 31, None, True)
    M = c['M']
    for g in range(2):
        for src, dst in ((1, 4), (1, 5), (0, 2)):
            for name in ('logits', 'lm_logits', 'rows'):
                c[name][g * M + dst] = c[name][g * M + src]
            for name in ('first', 'n_chars'):
                c[name][g, dst] = c[name][g, src]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    order, total, parts, _, _, _ = [t.cpu().numpy() for t in ops.rescore_launch(
        dev(c['logits']), dev(c['lm_logits']), dev(c['rows']), dev(c['n_hyps']), dev(c['first']), dev(c['chars']),
        dev(c['n_chars']), **trc.WEIGHTS)]
    ref = rescore_reference(c['logits'], c['lm_logits'], c['rows'], c['n_hyps'], c['first'], c['n_chars'], c['steps'],
                            **trc.WEIGHTS)
    assert order.tolist() == ref[0]
    for g in range(2):
        rank = {int(k): r for r, k in enumerate(order[g])}
        assert rank[1] + 1 == rank[4] and rank[4] + 1 == rank[5] and rank[0] + 1 == rank[2]
        bits = total[g].view(np.int32)
        assert bits[rank[1]] == bits[rank[4]] == bits[rank[5]] and bits[rank[0]] == bits[rank[2]]
        assert np.array_equal(parts[g, rank[1]].view(np.int32), parts[g, rank[5]].view(np.int32))


def oracle_list(m, texts, first, lm_weight, **weights):
    """rescore_reference over the float64 model's teacher-forced pass of one utterance's texts (<EOS> appended)."""
    z, zl, rows = trc.teacher_forced(m, texts, [True] * len(texts))
    return rescore_reference(z, zl if lm_weight else None, rows, [len(texts)], [first], [[len(t) for t in texts]],
                             10 ** 6, lm_weight=lm_weight, **weights)


@pytest.mark.parametrize('name,frames', [(SMALL, 40), (FULL, 160)], ids=['small', 'full'])
def test_rescoring_a_beam_list_reproduces_the_beams_scores(golden, name, frames):
    """decode_nbest with the CharLM at weight w, then rescore(lm_weight = w): the total of every entry is the beam's own
    score of it (a hypothesis that the step cap ended has no <EOS> term in the beam's score: the float64 model's is
    added), and the order is unchanged wherever the beam's adjacent scores differ by more than twice the bound."""
    fx = golden(name)
    asr, lm = tcd.models(fx)
    w = float(fx['lm_weights'][1])
    assert w != 0.0
    x = torch.from_numpy(fx['x'][:, :frames]).to(DEV)
    nbest = asr.decode_nbest([x], [[frames]], lm, Mapper(), w, 4, max_decoding_steps=STEPS)[0]
    chars, n_chars, scores, n_hyps = [t.cpu().numpy() for t in asr.last_beam]
    assert chars.shape[2] == STEPS and asr.last_encoded_packed[0].shape[1] == frames // 8
    again = asr.rescore(Mapper(), rnn_lm=lm, lm_weight=w)[0]
    order, total, parts = [t.cpu().numpy() for t in asr.last_rescore]
    n = int(n_hyps[0])
    assert len(again) == n == len(nbest) and sorted(order[0, :n].tolist()) == list(range(n))
    worst = 0.0
    for rank in range(n):
        k = int(order[0, rank])
        length = int(n_chars[0, k])
        want, steps = float(scores[0, k]), length + 1
        if length == STEPS:                                  # capped: the beam never scored an <EOS>
            m = dc.model(golden, name, frames)
            text = chars[0, k, :length].tolist()
            want += dc.forced(m, text, True, 0.0, w)[0] - dc.forced(m, text, False, 0.0, w)[0]
        err = abs(float(total[0, rank]) - want) / steps
        worst = max(worst, err)
        assert err <= SCORE_ATOL, (rank, k, float(total[0, rank]), want)
        assert again[rank][0] == nbest[k][0] and again[rank][1] == float(total[0, rank])
    print('%s: %d entries, order %s, worst |total - beam score| per step %.3g' % (name, n, order[0, :n].tolist(), worst))
    uncapped = [k for k in range(n) if n_chars[0, k] < STEPS]
    for a, b in zip(uncapped, uncapped[1:]):
        if scores[0, a] - scores[0, b] > 2 * SCORE_ATOL * (max(n_chars[0, a], n_chars[0, b]) + 1):
            assert order[0].tolist().index(a) < order[0].tolist().index(b)
    # the re-kept list is what score() and mbr() read
    assert np.array_equal(asr.last_hyps[0].cpu().numpy()[0, 0], chars[0, order[0, 0]])
    assert asr.last_hyp_scores is asr.last_rescore[1] and not asr.last_hyps_sampled


def ctc_groups(fx, frames_cycle, n):
    xs = [torch.from_numpy(fx['x'][:, :frames_cycle[i % len(frames_cycle)]]).to(DEV) for i in range(n)]
    return xs, [[x.shape[1]] for x in xs]


@pytest.mark.parametrize('name,cycle,sizes', [(SMALL, (8, 24, 40), ((3, True),)),
                                              (FULL, (160, 24), ((1, True), (8, False), (11, True), (10, False)))],
                         ids=['small', 'full'])
def test_rescoring_a_ctc_list_matches_the_float64_oracle(golden, name, cycle, sizes):
    """decode_ctc(beam_size = 3), then the second pass at ctc_weight 0.3 with the CharLM: totals and parts against the
    float64 model's teacher-forced pass plus the kept CTC scores.  The groups give 3 rows (one persistent launch), 32,
    33 (the chunk boundary) and 40 rows, in chunks that keep the persistent form, on the real widths, over T' = 20 and 3; the small model covers T' = 1, 3, 5."""
    from ss_asr_amd import ops
    fx = golden(name)
    asr, lm = tcd.models(fx)
    w, lam = float(np.float32(fx['lm_weights'][1])), float(np.float32(0.3))
    weights = dict(att_weight=1.0 - lam, first_weight=lam)
    refs, worst, rows_seen = {}, 0.0, []
    for n_utts, drop_idle in sizes:
        xs, x_lens = ctc_groups(fx, cycle, n_utts)
        asr.decode_ctc(xs, x_lens, Mapper(), beam_size=3)
        chars, n_chars, scores, n_hyps, _ = [t.cpu().numpy() for t in asr.last_ctc_decode]
        packed, enc_lens = asr.last_encoded_packed
        got = ops.rescore(packed, enc_lens, asr._decoder_params(), (asr.attention.psi.weight, asr.attention.psi.bias),
                          *asr.last_hyps, asr.last_hyp_scores, EOS, lm, lm_weight=w, drop_idle=drop_idle,
                          loop_rows=ops.rescore_loop_rows(packed.shape[1]), **weights)
        order, total, parts, chars_out, n_chars_out, n_hyps_out = [t.cpu().numpy() for t in got]
        rows_seen.append(n_utts * (3 if drop_idle else 4))
        assert np.array_equal(n_hyps_out, n_hyps)
        for i in range(n_utts):
            frames, n = x_lens[i][0], int(n_hyps[i])
            texts = [chars[i, k, :n_chars[i, k]].tolist() for k in range(n)]
            key = (frames, str(texts))
            if key not in refs:
                refs[key] = oracle_list(dc.model(golden, name, frames), texts, scores[i, :n].tolist(), w, **weights)
            want = refs[key]
            for rank in range(n):
                k = int(order[i, rank])
                j = want[0][0].index(k)
                tol = SCORE_ATOL * (len(texts[k]) + 1)
                errs = [abs(float(parts[i, rank, 0]) - want[2][0][j][0]), abs(float(parts[i, rank, 1]) - want[2][0][j][1]),
                        abs(float(total[i, rank]) - want[1][0][j]) / (1.0 - lam + w)]
                worst = max(worst, max(errs) / (len(texts[k]) + 1))
                assert max(errs) <= tol, (n_utts, i, rank, errs, tol)
                assert parts[i, rank, 2] == scores[i, k]
                assert chars_out[i, rank, :n_chars_out[i, rank]].tolist() == texts[k]
            gaps = [a - b for a, b in zip(want[1][0], want[1][0][1:])]
            if all(g > 2 * (1.0 - lam + w) * SCORE_ATOL * (chars.shape[2] + 1) for g in gaps):
                assert order[i, :n].tolist() == want[0][0]
            assert (order[i, n:] == -1).all()
    ops.check_persistent_status()
    print('%s: rows per pass %s, worst |error| per step %.3g (bound %.3g)' % (name, rows_seen, worst, SCORE_ATOL))
    # one call over all 40 rows (one launch per stage and step past 32 rows): the same texts within the bound
    one = ops.rescore(packed, enc_lens, asr._decoder_params(), (asr.attention.psi.weight, asr.attention.psi.bias),
                      *asr.last_hyps, asr.last_hyp_scores, EOS, lm, lm_weight=w, loop_rows=0, drop_idle=drop_idle, **weights)
    assert (np.abs(one[1].cpu().numpy() - total) <= 2 * SCORE_ATOL * (chars.shape[2] + 1)).all()


def test_two_pass_is_decode_ctc_then_rescore_and_the_list_is_followed(golden):
    fx = golden(SMALL)
    asr, lm = tcd.models(fx)
    mapper, w = Mapper(), float(fx['lm_weights'][1])
    xs, x_lens = ctc_groups(fx, (40, 24, 8), 3)
    two = asr.decode_two_pass(xs, x_lens, lm, mapper, w, beam_size=3, ctc_weight=0.3, length_bonus=0.25)
    kept = [t.clone() for t in asr.last_rescore + asr.last_hyps]
    first = asr.decode_ctc(xs, x_lens, mapper, beam_size=3)
    ctc_chars, ctc_n = asr.last_ctc_decode[0].cpu().numpy(), asr.last_ctc_decode[1].cpu().numpy()
    again = asr.rescore(mapper, rnn_lm=lm, lm_weight=w, att_weight=1.0 - 0.3, first_weight=0.3, length_bonus=0.25)
    assert two == again and [len(h) for h in two] == [len(h) for h in first]
    for a, b in zip(kept, asr.last_rescore + asr.last_hyps):
        assert a.dtype == b.dtype and np.array_equal(a.cpu().numpy().view(np.int32), b.cpu().numpy().view(np.int32))
    order = asr.last_rescore[0].cpu().numpy()
    chars, n_chars, n_hyps = [t.cpu().numpy() for t in asr.last_hyps]
    for i in range(3):
        assert sorted(t for t, _ in two[i]) == sorted(t for t, _ in first[i])
        for rank in range(n_hyps[i]):
            k = order[i, rank]
            assert np.array_equal(chars[i, rank, :n_chars[i, rank]], ctc_chars[i, k, :ctc_n[i, k]])
    # score, mbr and align see the re-ranked list
    tops = [h[0][0] for h in two]
    sc = asr.score(tops, mapper)
    assert len(sc) == 3 and all(s.chars[:3] == (0, 0, 0) for s in sc)
    picks = asr.mbr(mapper, unit='char')
    assert all(0 <= m.k < 3 and m.text == two[i][m.k][0] for i, m in enumerate(picks))
    al = asr.align(xs, x_lens, tops, mapper, encoded=asr.last_encoded_packed)
    assert len(al) == 3
    # a second rescore works from the re-kept list: first_weight 1 alone keeps it as it is
    same = asr.rescore(mapper, att_weight=0.0, first_weight=1.0)
    assert [[t for t, _ in h] for h in same] == [[t for t, _ in h] for h in two]
    assert asr.last_rescore[0].cpu().numpy()[:, 0].tolist() == [0, 0, 0]


def test_the_tester_key(tmp_path):
    import las_oracle as lo
    from conftest import GOLDEN
    from test_host_cpu import make_corpus
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
    t = tester(decode_ctc_only={'beam_size': 4}, decode_rescore={'ctc_weight': 0.3}, decode_score=True)
    assert t.decode_file == 'decode_beam_3_len_0.25_lm0.5_ctconly4_rescore0.3'
    got = t.exec()
    assert len(got) == 5 and all(isinstance(s, str) for s in got) and len(t.last_scores) == 5
    assert 0.0 <= t.last_error_rates['cer'] and 0.0 <= t.last_error_rates['wer']
    assert t.asr_model.last_rescore is not None
    # the tester's result is decode_two_pass's with its own language model
    from ss_asr_amd.ASRDataset import prepare_x
    xs, x_lens = [], []
    for x, _ in t.test_set:
        x, l = prepare_x(x, t.device)
        xs.append(x[:, :l[0]])
        x_lens.append(l)
    direct = []
    for lo_ in range(0, 5, 2):
        direct += [h[0][0] for h in t.asr_model.decode_two_pass(xs[lo_:lo_ + 2], x_lens[lo_:lo_ + 2], t.lm, t.mapper, 0.5,
                                                               beam_size=4, ctc_weight=0.3)]
    assert got == direct
    # with the key removed: the CTC-only run, under its own name
    plain = tester(decode_ctc_only={'beam_size': 4}, decode_score=True)
    assert plain.decode_file == 'decode_beam_3_len_0.25_lm0.5_ctconly4' and plain.decode_rescore is None
    want = plain.exec()
    assert plain.asr_model.last_rescore is None
    assert want == [h[0][0] for i in range(5) for h in plain.asr_model.decode_ctc(xs[i:i + 1], x_lens[i:i + 1], plain.mapper,
                                                                                 beam_size=4)]
    with pytest.raises(ValueError, match='decode_ctc_only'):
        tester(decode_rescore={'ctc_weight': 0.3})
    with pytest.raises(ValueError, match='beam_size >= 1'):
        tester(decode_ctc_only={'beam_size': 0}, decode_rescore={})
