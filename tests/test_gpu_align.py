"""CTC forced alignment on the GPU (ssasr_ctc_align through ops.ctc_align; ASR.align; ASRTester with
asr.decode_align) against test_align_cpu.viterbi_reference, the float64 restatement of include/ssasr.h.

The lattice runs on the raw logits: one double add and comparisons per value, in frame order, which the checker does
too -- so path, first, last and the set of rows without an alignment must be EQUAL, for every case, with no gap rule
and no excluded case.  score and char_logp carry the frames' normalisers, which the kernel takes in float: they must
lie within 8 * NOISE of the checker's float64 values, NOISE = the largest |float32 - float64| of the checker's
normaliser sum (sum_t lse_t, each lse_t and the sum evaluated in float32) over the compared rows -- the rule of
test_gpu_charlm_train.py and test_gpu_ctc_decode.py.  NOISE below was measured with the checker on the CPU
(2.005e-4, at the 820-frame rows); the test recomputes and prints it with the worst GPU error."""
import ctypes
import math
import os
import types

import numpy as np
import pytest
import torch

import las_oracle as lo
import test_gpu_ctc_decode as tcd
import test_gpu_beam as tgb
import test_gpu_decode as tgd
from conftest import GOLDEN
from test_align_cpu import viterbi_reference
from test_host_cpu import make_corpus

pytestmark = pytest.mark.gpu

DEV = tgd.DEV
Mapper = tgd.Mapper
NOISE = 2.01e-4
BOUND = 8 * NOISE


def labels_of(rng, L, V, blank, repeats=True):
    classes = [c for c in range(V) if c != blank]
    out = []
    for _ in range(L):
        c = int(rng.choice(classes))
        while not repeats and out and c == out[-1]:
            c = int(rng.choice(classes))
        out.append(c)
    return out


def min_frames(labels):
    return len(labels) + sum(a == b for a, b in zip(labels, labels[1:]))


def make_case(name, V, T, rows, lmax, blank=0, seed=0, logits=None):
    """rows: [(frame_len, labels)].  y_ld > lmax, the label matrix padded with a class that must not be read."""
    rng = np.random.default_rng(seed)
    B = len(rows)
    if logits is None:
        logits = (2.0 * rng.standard_normal((B, T, V))).astype(np.float32)
    y = np.full((B, lmax + 3), V - 1, dtype=np.int32)
    for b, (_, labels) in enumerate(rows):
        y[b, :len(labels)] = labels
    return types.SimpleNamespace(name=name, V=V, T=T, B=B, lmax=lmax, blank=blank, logits=logits, y=y,
                                 frame_lens=np.array([r[0] for r in rows], dtype=np.int32),
                                 label_lens=np.array([len(r[1]) for r in rows], dtype=np.int32), rows=rows)


def build_cases():
    rng = np.random.default_rng(2024)
    cases = []
    rep = [5, 5, 7, 7, 7, 9]                                    # three adjacent repeats: 9 frames at the least
    assert min_frames(rep) == 9
    cases.append(make_case('mixed', 50, 20, [(20, []), (1, [6]), (7, labels_of(rng, 7, 50, 0, repeats=False)),
                                             (9, rep), (8, rep), (15, labels_of(rng, 6, 50, 0))], 7, seed=1))
    cases.append(make_case('one frame', 50, 1, [(1, [4]), (1, []), (1, [3, 8])], 2, seed=2))
    cases.append(make_case('frames == labels', 50, 12, [(12, labels_of(rng, 12, 50, 0, repeats=False)),
                                                        (30, labels_of(rng, 12, 50, 0, repeats=False))], 12, seed=3))
    cases.append(make_case('two classes', 2, 9, [(9, [1, 1, 1]), (5, [1, 1, 1]), (4, [1, 1, 1]), (9, [1])], 3, seed=4))
    cases.append(make_case('blank 3', 50, 12, [(12, labels_of(rng, 5, 50, 3)), (10, [0, 0, 2])], 5, blank=3, seed=5))
    for lmax in (127, 128, 255, 256, 511):                      # Sp 255, 257, 511, 513, 1023: 256 / 512 / 1024 threads
        T = lmax + 5
        cases.append(make_case('lmax %d' % lmax, 50, T, [(T, labels_of(rng, lmax, 50, 0, repeats=False)),
                                                         (T - 3, labels_of(rng, lmax // 2, 50, 0))], lmax, seed=lmax))
    cases.append(make_case('375 frames', 50, 375, [(375, labels_of(rng, 300, 50, 0)), (350, labels_of(rng, 280, 50, 0))],
                           300, seed=6))
    # the back-pointers' two homes: at Lmax 300 (ten 64-state groups) LDS holds 8192 // 10 = 819 frames
    for T in (819, 820):
        cases.append(make_case('%d frames' % T, 50, T, [(T, labels_of(rng, 300, 50, 0)), (T - 101, labels_of(rng, 150, 50, 0))],
                               300, seed=T))
    return cases


_cases, _refs = [], {}


def cases():
    if not _cases:
        _cases.extend(build_cases())
    return _cases


def reference(case):
    if case.name not in _refs:
        _refs[case.name] = [viterbi_reference(case.logits[b], case.frame_lens[b], list(case.rows[b][1]), case.blank)
                            if len(case.rows[b][1]) <= case.lmax else None for b in range(case.B)]
    return _refs[case.name]


def noise_of(case, refs):
    """max |float32 - float64| of the rows' normaliser sums."""
    worst = 0.0
    for b, ref in enumerate(refs):
        if ref is None:
            continue
        x = case.logits[b, :len(ref.path)]
        m = x.max(1)
        lse32 = m + np.log(np.exp(x - m[:, None]).sum(1, dtype=np.float32))
        assert lse32.dtype == np.float32
        worst = max(worst, abs(float(lse32.sum(dtype=np.float32)) - float(ref.lse.sum())))
    return worst


def run(case):
    from ss_asr_amd import ops
    out = ops.ctc_align(torch.from_numpy(case.logits).to(DEV), torch.from_numpy(case.frame_lens).to(DEV),
                        torch.from_numpy(case.y).to(DEV), torch.from_numpy(case.label_lens).to(DEV), case.lmax, case.blank)
    return [t.cpu().numpy() for t in out]


def compare(case, got, refs):
    """Exact part asserted; -> the worst |score| / |char_logp| error."""
    path, first, last, logp, score = got
    assert path.shape == (case.B, case.T) and first.shape == last.shape == logp.shape == (case.B, case.lmax)
    assert path.dtype == first.dtype == np.int32 and score.dtype == np.float64 and logp.dtype == np.float32
    worst = 0.0
    for b, ref in enumerate(refs):
        tag = (case.name, b)
        if ref is None:
            assert score[b] == -math.inf, tag
            assert (path[b] == -1).all() and (first[b] == -1).all() and (last[b] == -1).all() and not logp[b].any(), tag
            continue
        n, L = len(ref.path), len(ref.first)
        assert np.array_equal(path[b, :n], ref.path), tag
        assert (path[b, n:] == -1).all(), tag
        assert np.array_equal(first[b, :L], ref.first) and np.array_equal(last[b, :L], ref.last), tag
        assert (first[b, L:] == -1).all() and (last[b, L:] == -1).all() and not logp[b, L:].any(), tag
        worst = max(worst, abs(float(score[b]) - ref.score), float(np.abs(logp[b, :L] - ref.char_logp).max()) if L else 0.0)
    return worst


def test_paths_spans_and_scores_match_the_float64_checker():
    noise = worst = 0.0
    none = 0
    for case in cases():
        refs = reference(case)
        err = compare(case, run(case), refs)
        n = noise_of(case, refs)
        none += sum(r is None for r in refs)
        print('%-18s B %d T %4d Lmax %3d: rows without an alignment %d, normaliser noise %.3e, worst |error| %.3e'
              % (case.name, case.B, case.T, case.lmax, sum(r is None for r in refs), n, err))
        noise, worst = max(noise, n), max(worst, err)
        assert err <= BOUND, case.name
    print('NOISE %.3e (constant %.3e), worst GPU |score| / |char_logp| error %.3e' % (noise, NOISE, worst))
    assert noise <= NOISE and none == 3
    by_name = {c.name: reference(c) for c in cases()}
    assert by_name['mixed'][3] is not None and by_name['mixed'][4] is None       # the minimum, and one frame fewer
    assert by_name['two classes'][1] is not None and by_name['two classes'][2] is None
    assert by_name['one frame'][2] is None


@pytest.mark.parametrize('value', [0.0, 0.37])
def test_all_equal_logits_are_decided_by_the_tie_rule(value):
    logits = np.full((2, 9, 50), value, dtype=np.float32)
    case = make_case('ties %g' % value, 50, 9, [(9, [4, 4, 9]), (7, [4, 4, 9])], 3, logits=logits)
    refs = [viterbi_reference(case.logits[b], case.frame_lens[b], [4, 4, 9], 0) for b in range(2)]
    assert list(refs[0].path) == [1, 2, 3, 5, 6, 6, 6, 6, 6]
    assert compare(case, run(case), refs) <= BOUND


def test_canaries_behind_every_output_stay_intact():
    from ss_asr_amd import _lib, ops
    lib = _lib.load()
    for case in (cases()[0], cases()[9]):
        B, T, V, lmax = case.B, case.T, case.V, case.lmax
        need = int(lib.ssasr_ctc_align_ws_bytes(B, T, V, lmax))
        ws = torch.empty(need // 8, device=DEV, dtype=torch.float64)
        dev = [torch.from_numpy(a).to(DEV) for a in (case.logits, case.frame_lens, case.y, case.label_lens)]
        pad = 64
        path = torch.full((B * T + pad,), 77, device=DEV, dtype=torch.int32)
        first = torch.full((B * lmax + pad,), 77, device=DEV, dtype=torch.int32)
        last = torch.full((B * lmax + pad,), 77, device=DEV, dtype=torch.int32)
        logp = torch.full((B * lmax + pad,), 77.0, device=DEV, dtype=torch.float32)
        score = torch.full((B + pad,), 77.0, device=DEV, dtype=torch.float64)
        rc = lib.ssasr_ctc_align(ops._p(dev[0]), ops._p(dev[1]), ops._p(dev[2]), case.y.shape[1], ops._p(dev[3]), B, T, V,
                                 lmax, case.blank, ops._p(ws), need, ops._p(path), ops._p(first), ops._p(last),
                                 ops._p(logp), ops._p(score), ops._stream())
        assert rc == 0
        torch.cuda.synchronize()
        for t, n in ((path, B * T), (first, B * lmax), (last, B * lmax), (logp, B * lmax), (score, B)):
            assert bool((t[n:] == 77).all()), case.name
        got = [path[:B * T].view(B, T), first[:B * lmax].view(B, lmax), last[:B * lmax].view(B, lmax),
               logp[:B * lmax].view(B, lmax), score[:B]]
        assert compare(case, [t.cpu().numpy() for t in got], reference(case)) <= BOUND
        for b in range(B):
            assert bool((got[0][b, int(case.frame_lens[b]):] == -1).all())


def test_the_best_path_is_at_most_the_loss_kernels_total():
    from ss_asr_amd import ops
    for case in (cases()[0], cases()[5], cases()[10]):
        dev = [torch.from_numpy(a).to(DEV) for a in (case.logits, case.frame_lens, case.y, case.label_lens)]
        score = ops.ctc_align(*dev, case.lmax, case.blank)[4].cpu().numpy()
        _, ws = ops._ctc_fwd(dev[0], dev[1], dev[2], dev[3], case.lmax, case.blank)
        sp = 2 * case.lmax + 1
        nll = ws.view(torch.float64)[case.B * case.T * sp:case.B * case.T * sp + case.B].cpu().numpy()
        for b, ref in enumerate(reference(case)):
            print('%s row %d: score %.6f, -nll %.6f' % (case.name, b, score[b], -nll[b]))
            if ref is None:
                assert nll[b] == math.inf and score[b] == -math.inf
            else:
                assert score[b] <= -nll[b] + BOUND and math.isfinite(nll[b])


def test_model_level_alignment_is_the_checker_on_the_gpus_own_logits(golden):
    from ss_asr_amd.asr import Alignment, input_span
    fx = golden(tgb.SMALL[0])
    asr, _ = tcd.models(fx)
    x = torch.from_numpy(fx['x']).to(DEV)
    xs, lens = [x[:, :40], x[:, :24]], [[40], [24]]
    texts = ['<hey>', 'no']
    got = asr.align(xs, lens, texts, Mapper())
    path, first, last, logp, score, logits = [t.cpu().numpy() for t in asr.last_align]
    assert logits.shape == (2, 5, 50) and path.shape == (2, 5) and first.shape == (2, 3)
    assert len(got) == 2 and all(isinstance(a, Alignment) for a in got)
    for i, (text, frames) in enumerate(zip(('hey', 'no'), (5, 3))):
        labels = [Mapper().char_to_ind(c) for c in text]
        ref = viterbi_reference(logits[i], frames, labels, 0)
        assert np.array_equal(path[i, :frames], ref.path) and (path[i, frames:] == -1).all()
        assert np.array_equal(first[i, :len(text)], ref.first) and np.array_equal(last[i, :len(text)], ref.last)
        assert abs(got[i].score - ref.score) <= BOUND and got[i].score == float(score[i])
        assert len(got[i].chars) == len(text)
        for j, (c, lo_, hi_, lp) in enumerate(got[i].chars):
            assert c == text[j] and (lo_, hi_) == input_span(int(ref.first[j]), int(ref.last[j]), lens[i][0])
            assert (lo_, hi_) == (8 * int(ref.first[j]), 8 * int(ref.last[j]) + 8)
            assert abs(lp - ref.char_logp[j]) <= BOUND and lp == float(logp[i, j])
    # seconds, and a text the frames cannot hold
    secs = asr.align(xs, lens, texts, Mapper(), frame_shift=0.01)
    assert [(c, round(a * 100), round(b * 100)) for c, a, b, _ in secs[0].chars] == [t[:3] for t in got[0].chars]
    long = asr.align(xs, lens, ['hey', 'hello'], Mapper())
    assert long[0].chars == got[0].chars and long[1].chars is None and long[1].score == -math.inf
    # each utterance aligns in a group as it aligns alone
    alone = asr.align(xs[1:], lens[1:], ['no'], Mapper())
    assert alone[0] == got[1]


def test_asr_tester_with_decode_align(tmp_path):
    from ss_asr_amd.ASRDataset import prepare_x
    from ss_asr_amd.ctc import JointCTCASR
    from ss_asr_amd.trainer import ASRTester
    fx = np.load(os.path.join(GOLDEN, 'dataset_ref.npz'), allow_pickle=False)
    dims = [int(v) for v in fx['cpt_dims']]
    root = str(tmp_path)
    index, lens = make_corpus(root, n=5, t_max=40, feat=dims[4], seed=5)
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
    # with the CTC prefix score in the search no hypothesis outgrows its frames, so the hypotheses align
    t0 = tester(decode_ctc_weight=0.3)
    assert t0.decode_file == 'decode_beam_3_len_0.25_lm0.5_ctc0.3'
    plain = t0.exec()
    assert not hasattr(t0, 'last_alignments')
    t = tester(decode_ctc_weight=0.3, decode_align=True)
    assert t.decode_file == 'decode_beam_3_len_0.25_lm0.5_ctc0.3_align'
    t.lm = t0.lm
    encodes = []
    inner = t.asr_model._encode_packed
    t.asr_model._encode_packed = lambda *a: encodes.append(len(a[0])) or inner(*a)
    got = t.exec()
    assert got == plain and len(got) == 5 and all(isinstance(s, str) for s in got)
    assert encodes == [2, 2, 1]                                     # the alignment re-used each group's encoder outputs
    assert len(t.last_alignments) == 5
    xs, x_lens = [], []
    for x, _ in t.test_set:
        x, l = prepare_x(x, t.device)
        xs.append(x[:, :l[0]])
        x_lens.append(l)
    for i, text in enumerate(got):
        assert t.last_alignments[i] == t.asr_model.align(xs[i:i + 1], x_lens[i:i + 1], [text], t.mapper)[0], i
    feasible = [a for a in t.last_alignments if a.chars is not None]
    print('%d of 5 hypotheses align; %s' % (len(feasible), [(s, a.score) for s, a in zip(got, t.last_alignments)]))
    assert len(feasible) >= 3
    for a in feasible:
        assert all(0 <= lo_ < hi_ <= 40 for _, lo_, hi_, _ in a.chars)
    # the plain search's hypotheses outgrow these short utterances: the key still works, chars is None there
    t1 = tester(decode_align=True)
    assert t1.decode_file == 'decode_beam_3_len_0.25_lm0.5_align'
    t1.lm = t0.lm
    assert t1.exec() == tester().exec() and len(t1.last_alignments) == 5
