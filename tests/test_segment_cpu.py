"""CTC segmentation without a GPU: postprocess.ctc_segment_reference, the float64 restatement of ssasr_ctc_segment
(include/ssasr.h), pinned by brute force over every span and frame labelling, against the forced-alignment checker
and on planted recordings; the C entries' argument checks, which return before any HIP call; segment.write_segments;
and ASR.segment's argument errors."""
import ctypes
import itertools
import math
import os

import numpy as np
import pytest
import torch

from test_align_cpu import collapse, viterbi_reference

NEG = -math.inf


def seg(lp, y, ends=None, window=3, blank=0, dtype=np.float64):
    from ss_asr_amd.postprocess import ctc_segment_reference
    return ctc_segment_reference(lp, y, [len(y)] if ends is None else ends, window, blank, dtype)


def log_softmax(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max(-1, keepdims=True)
    return x - (m + np.log(np.exp(x - m).sum(-1, keepdims=True)))


def states_of(frames, blank):
    """The lattice states of a frame labelling, by walking it: a blank after label j is state 2 (j + 1), a new or
    changed non-blank class moves to the next label.  No use of the skip rule."""
    out, j, prev = [], -1, None
    for c in frames:
        if c == blank:
            out.append(2 * (j + 1))
        else:
            if c != prev:
                j += 1
            out.append(2 * j + 1)
        prev = c
    return out


BRUTE = [(T, labels) for T in range(1, 7) for labels in
         ([1], [2], [1, 2], [1, 1], [2, 2], [1, 2, 1], [1, 1, 2], [2, 2, 2], [2, 1, 1], [1, 2, 2])]


def test_the_checker_is_the_best_of_all_spans_and_frame_labellings():
    """V = 3, blank 0, values that are multiples of 1 / 2 in [-2, 0] (sums are exact, ties are real, and a 0 makes the
    start tie with staying): every start frame, every end frame and every labelling of the frames between that
    collapses to the text.  Among the best sums the stated rule chooses: the earliest end frame, then S - 1 over
    S - 2, then, frame by frame from the end, stay before s - 1 before s - 2 before the start.  Score and path must
    be equal; the cases without a labelling are the checker's None."""
    rng = np.random.default_rng(5)
    compared = none = tied = 0
    for T, labels in BRUTE:
        for rep in range(3):
            lp = -rng.integers(0, 5, (T, 3)).astype(np.float64) / 2.0
            S = 2 * len(labels) + 1
            found = []
            for a in range(T):
                for e in range(a, T):
                    for frames in itertools.product(range(3), repeat=e - a + 1):
                        if collapse(frames, 0) != labels:
                            continue
                        total = np.float64(0.0)
                        for t, c in zip(range(a, e + 1), frames):
                            total = total + lp[t, c]
                        st = states_of(frames, 0)
                        codes = [st[i] - st[i - 1] if i else 3 for i in range(len(st))]
                        key = (-total, e, 0 if st[-1] == S - 1 else 1, tuple(reversed(codes)))
                        found.append((key, a, e, st))
            got = seg(lp, labels)
            if not found:
                assert got is None and T < len(labels) + sum(x == y for x, y in zip(labels, labels[1:]))
                none += 1
                continue
            found.sort(key=lambda f: f[0])
            key, a, e, st = found[0]
            tied += len(found) > 1 and found[1][0][0] == key[0]
            assert got.score == -key[0], (T, labels, rep)
            assert got.span == (a, e), (T, labels, rep)
            assert list(got.path[a:e + 1]) == st and (got.path[:a] == -1).all() and (got.path[e + 1:] == -1).all()
            if len(found) > 1 and found[1][0][0] == key[0]:
                assert got.gap == 0.0
            for j in range(len(labels)):
                run = [t for t in range(T) if got.path[t] == 2 * j + 1]
                assert run == list(range(got.first[j], got.last[j] + 1)) and run
            compared += 1
    assert compared >= 120 and none >= 15 and tied >= 20


def test_against_the_alignment_checker():
    """The free ends can only add paths: on the same log-softmax values the segment score is >= the alignment's.
    When the text fills the frames (len = L + the adjacent repeats) the one set of paths is the same, and so are the
    path and the score."""
    rng = np.random.default_rng(11)
    for T, V, labels in ((12, 6, [1, 2, 2, 5]), (30, 50, [int(c) for c in rng.integers(1, 50, 11)]), (9, 5, [4, 1, 4])):
        logits = (2.0 * rng.standard_normal((T, V))).astype(np.float32)
        got = seg(log_softmax(logits), labels)
        assert got.score >= viterbi_reference(logits, T, labels, 0).score - 1e-9
    for labels in ([3, 3, 1, 2, 2, 2, 4], [1, 2, 3], [2]):
        T = len(labels) + sum(a == b for a, b in zip(labels, labels[1:]))
        logits = (2.0 * rng.standard_normal((T, 6))).astype(np.float32)
        got, ref = seg(log_softmax(logits), labels), viterbi_reference(logits, T, labels, 0)
        assert np.array_equal(got.path, ref.path) and got.span == (0, T - 1)
        assert abs(got.score - ref.score) < 1e-9 and np.abs(got.char_logp - ref.char_logp).max() < 1e-9
        assert np.array_equal(got.first, ref.first) and np.array_equal(got.last, ref.last)
        assert seg(log_softmax(logits[:T - 1]), labels) is None


def peaked(frames, V, peak=12.0, seed=0):
    """Logits whose frame t is `peak` above unit noise at class frames[t]."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((len(frames), V))
    x[np.arange(len(frames)), frames] += peak
    return x.astype(np.float32)


def test_a_planted_utterance_is_found_inside_other_speech():
    """The utterance's frames inside frames peaked on labels the text does not have.  Every scored frame costs
    something (lp <= 0), so the free ends keep ONE frame of the first and of the last label's run: those two are
    planted with one frame, the inner labels with two."""
    text = [3, 4, 3, 5]
    before, after = [6, 7, 6, 0, 7], [7, 7, 6, 0, 6, 7, 6]
    frames = before + [3, 4, 4, 3, 3, 5] + after
    got = seg(log_softmax(peaked(frames, 8)), text)
    a = len(before)
    assert got.span == (a, a + 5) and got.gap > 1.0
    assert list(got.first) == [a, a + 1, a + 3, a + 5] and list(got.last) == [a, a + 2, a + 4, a + 5]
    assert list(got.path[a:a + 6]) == [1, 3, 3, 5, 5, 7] and (got.path[:a] == -1).all() and (got.path[a + 6:] == -1).all()
    assert list(got.utt_first) == [a] and list(got.utt_last) == [a + 5]
    # with two frames for the outer labels the span keeps the inner one of each
    got = seg(log_softmax(peaked(before + [3, 3, 4, 5, 5] + after, 8)), [3, 4, 5])
    assert got.span == (a + 1, a + 3)


def test_three_planted_utterances_and_their_confidences():
    utts = [[3, 4, 5], [5, 6], [2, 3, 4, 2]]
    frames, bounds = [0] * 4, []
    for n, u in enumerate(utts):
        lo = len(frames)
        for j, c in enumerate(u):                                # the text's outer labels get one frame (see above)
            frames += [c] * (1 if (n, j) in ((0, 0), (2, 3)) else 3)
        bounds.append((lo, len(frames) - 1))
        frames += [0] * 5
    y = [c for u in utts for c in u]
    ends = list(np.cumsum([len(u) for u in utts]))
    lp = log_softmax(peaked(frames, 8, seed=3))
    for window in (3, 4, 100):          # divides the 6-frame span / divides none / longer than any
        got = seg(lp, y, ends, window=window)
        assert [(int(a), int(b)) for a, b in zip(got.utt_first, got.utt_last)] == bounds
        assert got.span == (bounds[0][0], bounds[-1][1])
        for n, (lo, hi) in enumerate(bounds):
            q = [lp[t, 0 if got.path[t] % 2 == 0 else y[got.path[t] // 2]] for t in range(lo, hi + 1)]
            blocks = [q[i:i + window] for i in range(0, len(q), window)]
            assert abs(got.utt_conf[n] - min(sum(b) / len(b) for b in blocks)) < 1e-12
            assert len(blocks) == -(-(hi - lo + 1) // window)
    # a damaged utterance has the lowest confidence
    bad = peaked(frames, 8, seed=3)
    lo, hi = bounds[1]
    bad[lo:lo + 3] = 0.0
    got = seg(log_softmax(bad), y, ends, window=3)
    assert int(np.argmin(got.utt_conf)) == 1 and got.utt_conf[1] < -1.0 < got.utt_conf[0]


def test_no_segmentation():
    lp = log_softmax(np.random.default_rng(1).standard_normal((4, 5)))
    assert seg(lp, [1, 1, 2, 3]) is None                       # five frames at the least
    assert seg(lp, [1, 2, 3, 4], [2, 4]) is not None
    for ends in ([], [2, 3], [2, 2, 4], [3, 2, 4], [0, 4], [2, 5]):
        assert seg(lp, [1, 2, 3, 4], ends) is None, ends
    assert seg(lp, [], []) is None and seg(lp[:0], [1]) is None
    with pytest.raises(ValueError, match='window'):
        seg(lp, [1], window=0)


def test_the_float32_run_is_the_same_function():
    lp = log_softmax(peaked([0, 0, 1, 1, 0, 2, 2, 0, 0], 4))
    a, b = seg(lp, [1, 2]), seg(lp.astype(np.float32), [1, 2], dtype=np.float32)
    assert np.array_equal(a.path, b.path) and 0 < abs(a.score - b.score) < 1e-5 and b.utt_conf.dtype == np.float32


# ---------------------------------------------------------------- C entries ----
def _entry_args(**over):
    from ss_asr_amd import _lib
    lib = _lib.load()
    a = dict(B=2, T=6, V=5, Lmax=3, Nmax=2, window=2, blank=0, y_ld=4, utt_ld=2)
    a.update({k: v for k, v in over.items() if k in a})
    need = int(lib.ssasr_ctc_segment_ws_bytes(2, 6, 5, 3, 2))
    names = ('logits', 'frame_lens', 'y', 'label_lens', 'utt_ends', 'n_utts', 'path', 'first', 'last', 'char_logp',
             'score', 'utt_first', 'utt_last', 'utt_conf')
    bufs = {n: ctypes.create_string_buffer(4096) for n in names}
    ws = ctypes.create_string_buffer(need + 16)
    ptr = {n: ctypes.addressof(b) for n, b in bufs.items()}
    ptr['ws'] = (ctypes.addressof(ws) + 7) & ~7
    for k, v in over.items():
        if k in ptr:
            ptr[k] = v(ptr[k]) if callable(v) else v
    return lib, (bufs, ws), (ptr['logits'], ptr['frame_lens'], ptr['y'], a['y_ld'], ptr['label_lens'], ptr['utt_ends'],
                             a['utt_ld'], ptr['n_utts'], a['B'], a['T'], a['V'], a['Lmax'], a['Nmax'], a['window'],
                             a['blank'], ptr['ws'], over.get('ws_bytes', need), ptr['path'], ptr['first'], ptr['last'],
                             ptr['char_logp'], ptr['score'], ptr['utt_first'], ptr['utt_last'], ptr['utt_conf'], None)


def test_the_entries_reject_bad_arguments_before_any_hip_call():
    from ss_asr_amd import _lib
    lib = _lib.load()
    assert lib.ssasr_abi_version() == 16 == _lib.ABI_VERSION
    for name in ('ssasr_ctc_segment', 'ssasr_ctc_segment_ws_bytes', 'ssasr_ctc_segment_form'):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    # lse and q per frame, 16 bytes per 64 states and frame, four stamps per recording
    assert lib.ssasr_ctc_segment_ws_bytes(2, 6, 5, 3, 2) == 2 * (6 * 16 + 6 * 16 + 32)
    assert lib.ssasr_ctc_segment_ws_bytes(1, 32768, 1024, 8191, 8191) == 32768 * 16 + 32768 * 256 * 16 + 32
    for shape in ((1, 32769, 5, 3, 2), (1, 6, 5, 8192, 2), (1, 6, 1025, 3, 2), (1, 6, 1, 3, 2), (0, 6, 5, 3, 2),
                  (65536, 6, 5, 3, 2), (1, 0, 5, 3, 2), (1, 6, 5, 0, 1), (1, 6, 5, 3, 0), (1, 6, 5, 3, 4)):
        assert lib.ssasr_ctc_segment_ws_bytes(*shape) == 0, shape
    th, per = ctypes.c_int(0), ctypes.c_int(0)
    forms = []
    for lmax in (1, 127, 128, 255, 256, 511, 512, 1023, 1024, 2047, 2048, 4095, 4096, 8191):
        f = lib.ssasr_ctc_segment_form(100, lmax, ctypes.byref(th), ctypes.byref(per))
        assert f >= 0 and th.value * per.value >= 2 * lmax + 1 and th.value in (256, 512, 1024) and 1 <= per.value <= 16
        forms.append(f)
    assert forms == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6]
    for T, lmax in ((32769, 3), (0, 3), (6, 8192), (6, 0)):
        assert lib.ssasr_ctc_segment_form(T, lmax, None, None) == -1
    assert lib.ssasr_ctc_segment_form(32768, 8191, None, None) == 6
    lib_, keep, args = _entry_args()
    for name in ('logits', 'frame_lens', 'y', 'label_lens', 'utt_ends', 'n_utts', 'ws', 'path', 'first', 'last',
                 'char_logp', 'score', 'utt_first', 'utt_last', 'utt_conf'):
        _, keep, args = _entry_args(**{name: None})
        assert lib.ssasr_ctc_segment(*args) == -1, name
    for bad in (dict(Lmax=8192), dict(T=32769), dict(V=1), dict(V=1025), dict(blank=5), dict(blank=-1), dict(window=0),
                dict(Nmax=0), dict(Nmax=4), dict(ws=lambda p: p + 4), dict(ws_bytes=100), dict(B=0), dict(T=0),
                dict(Lmax=0), dict(y_ld=2), dict(utt_ld=1)):
        _, keep, args = _entry_args(**bad)
        assert lib.ssasr_ctc_segment(*args) == -1, bad


# ---------------------------------------------------------- write_segments ----
def test_write_segments_rows_load_back_and_equal_the_source(tmp_path):
    from ss_asr_amd.asr import Segment, Segmentation
    from ss_asr_amd.ASRDataset import ASRDataset, load_index
    from ss_asr_amd.segment import write_segments
    rng = np.random.default_rng(2)
    fbank = rng.standard_normal((200, 12)).astype(np.float32)
    utts = [Segment('halló heimur', 8, 56, -0.2), Segment('a "b"\tc', 64, 80, -3.5), Segment('já, 7.', 96, 160, -0.9),
            Segment('x', 168, 200, -1.0)]
    sg = Segmentation(-40.0, (8, 200), utts, None)
    index = str(tmp_path / 'index.tsv')
    kept, dropped = write_segments(sg, fbank, str(tmp_path / 'seg'), index, min_confidence=-1.0, name='rec7')
    assert [w.segment for w in kept] == [utts[0], utts[2], utts[3]] and [w.segment for w in dropped] == [utts[1]]
    assert dropped[0].row is None
    rows = load_index(index)
    assert rows == [w.row for w in kept] and len(rows) == 3
    for row, u, k in zip(rows, (utts[0], utts[2], utts[3]), (0, 2, 3)):
        assert row['normalized_text'] == '<' + u.text + '>' and row['s_len'] == len(u.text) + 2
        assert row['unpadded_num_frames'] == u.end - u.start and row['wav_fname'] == 'rec7_%04d.wav' % k
        fb = np.load(row['path_to_fbank'])
        assert fb.shape == (64, 12) and fb.dtype == np.float64
        assert np.array_equal(fb[:u.end - u.start], fbank[u.start:u.end]) and not fb[u.end - u.start:].any()
    # a second recording is appended; quoting survives the round trip; the data set batches the rows
    kept2, _ = write_segments(Segmentation(-9.0, (64, 80), [utts[1]], None), fbank, str(tmp_path / 'seg'), index,
                              min_confidence=-math.inf, name='rec8', pad_to=64)
    rows = load_index(index)
    assert len(rows) == 4 and rows[3]['normalized_text'] == '<a "b"\tc>' and rows[3] == kept2[0].row
    ds = ASRDataset(index, batch_size=2)
    assert len(ds) == 2 and ds.get_feature_dim() == 12
    assert ds.get_batched_fbanks(2).shape == (2, 64, 12) and ds.get_batched_framelengths(2) == [32, 16]
    assert ds.get_text(1) == '<já, 7.>'
    # nothing fits: nothing written; spans in seconds and outside the recording are errors
    assert write_segments(Segmentation(NEG, None, None, None), fbank, str(tmp_path / 'seg'), index,
                          min_confidence=-1.0, name='rec9') == ([], [])
    assert len(load_index(index)) == 4
    with pytest.raises(ValueError, match='input frames'):
        write_segments(Segmentation(-1.0, (0.0, 0.5), [Segment('a', 0.0, 0.5, -0.1)], None), fbank, str(tmp_path), index,
                       min_confidence=-1.0, name='r')
    with pytest.raises(ValueError, match='outside'):
        write_segments(Segmentation(-1.0, (0, 208), [Segment('a', 0, 208, -0.1)], None), fbank, str(tmp_path), index,
                       min_confidence=-1.0, name='r')
    with pytest.raises(ValueError, match='pad_to'):
        write_segments(sg, fbank, str(tmp_path), index, min_confidence=-1.0, name='r', pad_to=10)


# ------------------------------------------------------------ Python surface ----
def test_segment_argument_errors_that_need_no_gpu():
    from ss_asr_amd import ops
    from ss_asr_amd.asr import ASR, Segmentation
    from ss_asr_amd.ASRDataset import Mapper
    from ss_asr_amd.ctc import JointCTCASR
    x, lens = [torch.zeros(1, 16, 12)], [[16]]
    model = ASR(50, 32, 32, 16, 12, 1.0)
    with pytest.raises(ValueError, match=r'needs a model with a ctc_head \(ctc.JointCTCASR\); ASR has none') as mine:
        model.segment(x, lens, [['ab']], Mapper())
    with pytest.raises(ValueError) as plain:
        model._ctc_head(0.3)
    assert str(plain.value) == str(mine.value)
    joint = JointCTCASR(50, 32, 32, 16, 12, 1.0)
    with pytest.raises(ValueError, match='does not know'):
        joint.segment(x, lens, [['ab', 'a中b']], Mapper())
    with pytest.raises(ValueError, match='empty'):
        joint.segment(x, lens, [['ab', '<>']], Mapper())
    with pytest.raises(ValueError, match='list of its utterances'):
        joint.segment(x, lens, ['ab'], Mapper())
    with pytest.raises(ValueError, match='list of its utterances'):
        joint.segment(x, lens, [[]], Mapper())
    with pytest.raises(ValueError, match='1 recordings, 1 lengths, 2 texts'):
        joint.segment(x, lens, [['a'], ['b']], Mapper())
    with pytest.raises(ValueError, match='window'):
        joint.segment(x, lens, [['a']], Mapper(), window=0)
    with pytest.raises(ValueError, match='at most %d' % ops.CTC_SEGMENT_MAX_LABELS):
        joint.segment(x, lens, [['a' * 5000, 'b' * 3192]], Mapper())
    with pytest.raises(ValueError, match='at most %d encoder frames' % ops.CTC_SEGMENT_MAX_FRAMES):
        joint.segment(x, [[8 * 32768 + 1]], [['a']], Mapper())
    assert joint.last_segment is None and Segmentation(NEG, None, None, None).utterances is None
    assert ops.CTC_SEGMENT_MAX_LABELS == 8191 and ops.CTC_SEGMENT_MAX_FRAMES == 32768
    assert ops.ctc_segment_form(100, 300) == (2, 1024, 1) and ops.ctc_segment_form(100, 8192) is None
