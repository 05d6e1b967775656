"""CTC segmentation with utterance skips and a filler, the parts that need no GPU: the float64 restatement
(postprocess.ctc_segment_skip_reference) against ctc_segment_reference and against brute force, planted recordings, the
C entries' argument checks, the host interfaces and write_segments."""
import ctypes
import itertools
import math

import numpy as np
import pytest
import torch

from test_segment_cpu import log_softmax, peaked

NEG = -math.inf


def seg(lp, y, ends, skip=NEG, fill=NEG, window=3, blank=0, dtype=np.float64):
    from ss_asr_amd.postprocess import ctc_segment_skip_reference
    return ctc_segment_skip_reference(lp, y, ends, window, skip, fill, blank, dtype)


def test_with_both_penalties_off_it_is_the_plain_checker():
    from ss_asr_amd.postprocess import ctc_segment_reference
    rng = np.random.default_rng(0)
    some = none = 0
    for _ in range(150):
        T, V, L = int(rng.integers(1, 30)), int(rng.integers(2, 9)), int(rng.integers(1, 8))
        y = [int(c) for c in rng.integers(0, V, L)]
        blank = int(rng.integers(0, V))
        y = [c if c != blank else (c + 1) % V for c in y]
        n = int(rng.integers(1, min(L, 3) + 1))
        ends = sorted(rng.choice(np.arange(1, L), n - 1, replace=False).tolist()) + [L] if n > 1 else [L]
        lp = log_softmax(4 * rng.standard_normal((T, V)))
        a, b = ctc_segment_reference(lp, y, ends, 3, blank), seg(lp, y, ends, blank=blank)
        assert (a is None) == (b is None)
        if a is None:
            none += 1
            continue
        for k, v in vars(a).items():                            # score, span, path, gap and every output
            assert np.array_equal(np.asarray(v), np.asarray(getattr(b, k))), k
        assert not b.utt_skipped.any() and set(b.is_fill[b.path >= 0]) == {0} and (b.is_fill[b.path < 0] == -1).all()
        some += 1
    assert some >= 100 and none >= 5
    for ends in ([], [2, 3], [2, 2, 4], [0, 4], [2, 5]):
        assert seg(log_softmax(rng.standard_normal((4, 5))), [1, 2, 3, 4], ends, -1.0, -1.0) is None
    for bad in (dict(skip=0.5), dict(fill=1e-9), dict(skip=math.nan), dict(fill=math.inf)):
        with pytest.raises(ValueError, match='penalty'):
            seg(log_softmax(rng.standard_normal((4, 5))), [1, 2], [2], **bad)


# ------------------------------------------------------------- brute force ----
def all_paths(T, labels, ends, blank=0):
    """Every (start frame, states, codes) of the lattice: a path starts in state 0 or 1, moves by stay / s - 1 / an
    allowed s - 2 / a skip from J_n to J_{n+1}, and ends in S - 1 or S - 2."""
    S = 2 * len(labels) + 1
    junc = [0] + [2 * e for e in ends]
    out = []

    def walk(a, st, codes):
        s = st[-1]
        if s in (S - 1, S - 2):
            out.append((a, list(st), list(codes)))
        if a + len(st) == T:
            return
        moves = [(s, 0)]
        if s + 1 < S:
            moves.append((s + 1, 1))
        if s % 2 and s + 2 < S and labels[(s + 2) // 2] != labels[s // 2]:
            moves.append((s + 2, 2))
        if s % 2 == 0 and s in junc[:-1]:
            moves.append((junc[junc.index(s) + 1], 2))
        for s2, code in moves:
            walk(a, st + [s2], codes + [code])
    for a in range(T):
        for s0 in (0, 1):
            walk(a, [s0], [3])
    return out, junc


def brute(lp, labels, ends, skip, fill):
    """The best path by the stated rule, over every path and every filler choice: the largest sum (in frame order),
    then the earliest end frame, S - 1 over S - 2, from the end backwards stay < s - 1 < s - 2 / skip < start, and the
    blank over the filler."""
    T = lp.shape[0]
    S = 2 * len(labels) + 1
    paths, junc = all_paths(T, labels, ends)
    others = [v for v in range(lp.shape[1]) if v != 0]
    fv = []
    for t in range(T):
        m = lp[t, others].max()
        fv.append(np.float64(m + np.log(np.exp(lp[t, others] - m).sum())) + np.float64(fill))
    best = None
    for a, st, codes in paths:
        spots = [i for i, s in enumerate(st) if s in junc]
        for choice in itertools.product((0, 1), repeat=len(spots)) if fill > NEG else [(0,) * len(spots)]:
            pick = dict(zip(spots, choice))
            total = np.float64(0.0)
            for i, s in enumerate(st):
                t = a + i
                if pick.get(i):
                    e = fv[t]
                else:
                    e = lp[t, labels[s // 2] if s % 2 else 0]
                if i and codes[i] == 2 and s % 2 == 0:
                    total = total + np.float64(skip)
                total = total + e if i else e + np.float64(0.0)
            if not total > NEG:
                continue
            e = a + len(st) - 1
            fills = tuple(pick.get(i, 0) for i in range(len(st)))
            key = (-total, e, 0 if st[-1] == S - 1 else 1, tuple(reversed(codes)), fills)
            if best is None or key < best[0]:
                best = (key, a, e, st, fills)
    return best


CASES = [(T, labels, ends) for T in range(1, 7) for labels, ends in
         (([1], [1]), ([1, 2], [1, 2]), ([1, 1], [1, 2]), ([1, 2], [2]), ([1, 2, 1], [1, 3]), ([2, 2, 1], [2, 3]),
          ([1, 1, 2], [1, 3]), ([2, 1, 2], [3]), ([1, 2, 2], [2, 3]))]


@pytest.mark.parametrize('mode', ['skip', 'skip and filler'])
def test_the_checker_is_the_best_of_all_paths_skips_and_filler_choices(mode):
    """V = 3, blank 0, T <= 6, L <= 3, N <= 2, every start, end, labelling, subset of skipped utterances and filler
    choice.  'skip': every value a multiple of 1 / 2 in [-2, 0] and skip_penalty -1 / 2 or -1, so sums are exact and
    ties are real.  'skip and filler': one of the two label classes is -inf in every frame, so that f_t is the other's
    value exactly and the sums stay exact with fill_penalty -1 / 2; ties between the blank and the filler occur."""
    rng = np.random.default_rng(7 if mode == 'skip' else 8)
    compared = none = tied = skips = fills = 0
    for T, labels, ends in CASES:
        for rep in range(3):
            lp = -rng.integers(0, 5, (T, 3)).astype(np.float64) / 2.0
            skip, fill = -float(rng.integers(1, 3)) / 2.0, NEG
            if mode != 'skip':
                fill = -0.5
                lp[np.arange(T), rng.integers(1, 3, T)] = NEG
            want = brute(lp, labels, ends, skip, fill)
            got = seg(lp, labels, ends, skip, fill)
            if want is None:
                assert got is None
                none += 1
                continue
            key, a, e, st, fl = want
            tag = (T, labels, ends, rep)
            assert got is not None and got.score == -key[0], tag
            assert got.span == (a, e) and list(got.path[a:e + 1]) == st, tag
            assert (got.path[:a] == -1).all() and (got.path[e + 1:] == -1).all(), tag
            assert list(got.is_fill[a:e + 1]) == list(fl) and (got.is_fill[:a] == -1).all(), tag
            seen = {s // 2 for s in st if s % 2}
            want_skipped = [int(not any(j in seen for j in range(lo, hi))) for lo, hi in zip([0] + ends, ends)]
            assert list(got.utt_skipped) == want_skipped, tag
            for n, (lo, hi) in enumerate(zip([0] + ends, ends)):    # whole or not at all
                assert all((j in seen) != bool(want_skipped[n]) for j in range(lo, hi)), tag
                if want_skipped[n]:
                    assert got.utt_first[n] == got.utt_last[n] == -1 and got.utt_conf[n] == 0
                    assert (got.first[lo:hi] == -1).all() and (got.last[lo:hi] == -1).all() and not got.char_logp[lo:hi].any()
            skips += sum(want_skipped) > 0
            fills += any(fl)
            tied += got.gap == 0.0
            compared += 1
    assert compared >= 100 and skips >= 20 and tied >= 10
    if mode != 'skip':
        assert fills >= 10


# ---------------------------------------------------------------- planted ----
def planted_frames(V, utts, absent=(), foreign_after=None, foreign_len=3, lead=3, tail=3):
    """The frame classes of a recording whose best path is forced: the present utterances' labels (two frames each,
    one for the first and the last label of the recording, which the free ends would otherwise cut; a blank frame
    before a repeat), exactly m + 1 blank frames where m adjacent utterances are absent (the junction's frame and one
    landing frame per skip), none between two present neighbours, `foreign_len` frames of class V - 2 after utterance
    `foreign_after`, and frames of class V - 1 before and after.  Neither class is in the text.
    -> (frames, {n: (first, last)} of the present utterances, the foreign frames)."""
    present = [n for n in range(len(utts)) if n not in absent]
    frames, spans, foreign = [V - 1] * lead, {}, []
    pending = 0
    prev = None
    for n, u in enumerate(utts):
        if n in absent:
            pending += 1
            continue
        if pending:
            frames += [0] * (pending + 1)
            prev = None
        pending = 0
        lo = len(frames)
        for j, c in enumerate(u):
            if c == prev:
                frames.append(0)
                if j == 0:
                    lo += 1
            outer = (n == present[0] and j == 0) or (n == present[-1] and j == len(u) - 1)
            frames += [c] * (1 if outer else 2)
            prev = c
        spans[n] = (lo, len(frames) - 1)
        if n == foreign_after:
            foreign = list(range(len(frames), len(frames) + foreign_len))
            frames += [V - 2] * foreign_len
            prev = None
    if pending:
        frames += [0] * (pending + 1)
    return frames + [V - 1] * tail, spans, foreign


def text_of(utts):
    return [c for u in utts for c in u], [int(e) for e in np.cumsum([len(u) for u in utts])]


def test_a_middle_utterance_that_was_never_spoken():
    utts = [[3, 4, 5], [2, 5, 3, 2], [4, 3]]
    y, ends = text_of(utts)
    frames, spans, _ = planted_frames(8, utts, absent=(1,))
    lp = log_softmax(peaked(frames, 8, seed=1))
    got = seg(lp, y, ends, -3.0)
    assert list(got.utt_skipped) == [0, 1, 0] and got.gap >= 1e-3
    assert (int(got.utt_first[0]), int(got.utt_last[0])) == spans[0] and (int(got.utt_first[2]), int(got.utt_last[2])) == spans[2]
    assert got.utt_first[1] == got.utt_last[1] == -1 and got.utt_conf[1] == 0 and got.span == (spans[0][0], spans[2][1])
    assert (got.first[3:7] == -1).all() and (got.last[3:7] == -1).all() and not got.char_logp[3:7].any()
    assert min(got.utt_conf[0], got.utt_conf[2]) > -0.1
    # off: the plain result, which forces the four characters onto the others' frames
    from ss_asr_amd.postprocess import ctc_segment_reference
    off, plain = seg(lp, y, ends), ctc_segment_reference(lp, y, ends, 3)
    assert np.array_equal(off.path, plain.path) and off.score == plain.score and not off.utt_skipped.any()
    assert plain.score < got.score - 10 and min(plain.utt_conf) < -3


def test_frames_of_a_foreign_label_between_two_utterances():
    utts = [[3, 4, 5], [2, 5, 3]]
    y, ends = text_of(utts)
    frames, spans, foreign = planted_frames(8, utts, foreign_after=0)
    x = peaked(frames, 8, seed=2)
    got = seg(log_softmax(x), y, ends, NEG, -1.0)
    assert [t for t in range(len(frames)) if got.is_fill[t] == 1] == foreign and got.gap >= 1e-3
    assert not got.utt_skipped.any() and (int(got.utt_first[1]), int(got.utt_last[1])) == spans[1]
    assert all(got.path[t] == 2 * ends[0] for t in foreign)
    without = seg(log_softmax(np.delete(x, foreign, axis=0)), y, ends, NEG, -1.0)
    assert (without.is_fill <= 0).all()
    assert (got.utt_conf >= without.utt_conf - 1e-12).all()     # no junction frame lies inside an utterance's span
    off = seg(log_softmax(x), y, ends)
    assert (off.is_fill <= 0).all() and off.score < got.score - 10


def test_leading_and_trailing_unspoken_utterances_and_a_chain():
    utts = [[2, 3], [3, 4, 5], [5, 2], [4], [2, 3, 4], [5, 5]]
    y, ends = text_of(utts)
    frames, spans, foreign = planted_frames(8, utts, absent=(0, 2, 3, 5), foreign_after=None)
    got = seg(log_softmax(peaked(frames, 8, seed=3)), y, ends, -3.0, -1.0)
    assert list(got.utt_skipped) == [1, 0, 1, 1, 0, 1] and got.gap >= 1e-3
    assert (int(got.utt_first[1]), int(got.utt_last[1])) == spans[1] and (int(got.utt_first[4]), int(got.utt_last[4])) == spans[4]
    a, e = got.span
    assert got.path[a] == 0 and got.path[a + 1] == 2 * ends[0] and got.path[e] == 2 * len(y)   # the ends pay for their skips
    assert (a, e) == (spans[1][0] - 2, spans[4][1] + 2)
    assert abs(got.score - (-12.0)) < 0.5                        # four penalties


def test_a_single_utterance_that_is_skipped():
    lp = log_softmax(peaked([0, 0, 0, 0], 6, seed=4))
    got = seg(lp, [3, 4], [2], -2.0)
    assert list(got.utt_skipped) == [1] and list(got.path[got.span[0]:got.span[1] + 1]) == [0, 4]
    assert got.span[1] == got.span[0] + 1 and abs(got.score + 2.0) < 1e-3
    assert (got.first == -1).all() and got.utt_first[0] == -1 and got.utt_conf[0] == 0
    assert seg(lp[:1], [3, 4], [2], -2.0) is None               # the start and the landing frame: two at the least
    assert seg(lp[:3], [1, 1, 2, 3], [4], -2.0) is not None and seg(lp[:3], [1, 1, 2, 3], [4]) is None


def test_the_float32_run_is_the_same_function():
    utts = [[3, 4, 5], [2, 5, 3, 2], [4, 3]]
    y, ends = text_of(utts)
    frames, _, _ = planted_frames(8, utts, absent=(1,), foreign_after=0)
    lp = log_softmax(peaked(frames, 8, seed=5))
    a, b = seg(lp, y, ends, -3.0, -1.0), seg(lp.astype(np.float32), y, ends, -3.0, -1.0, dtype=np.float32)
    assert np.array_equal(a.path, b.path) and np.array_equal(a.is_fill, b.is_fill) and (a.is_fill == 1).sum() == 3
    assert 0 < abs(a.score - b.score) < 1e-4 and b.utt_conf.dtype == np.float32


# ---------------------------------------------------------------- C entries ----
def _entry_args(entry='skip', **over):
    from ss_asr_amd import _lib
    lib = _lib.load()
    a = dict(B=2, T=6, V=5, Lmax=3, Nmax=2, window=2, blank=0, y_ld=4, utt_ld=2)
    a.update({k: v for k, v in over.items() if k in a})
    need = int(lib.ssasr_ctc_segment_skip_ws_bytes(2, 6, 5, 3, 2))
    names = ('logits', 'frame_lens', 'y', 'label_lens', 'utt_ends', 'n_utts', 'path', 'first', 'last', 'char_logp',
             'score', 'utt_first', 'utt_last', 'utt_conf', 'utt_skipped', 'is_fill')
    bufs = {n: ctypes.create_string_buffer(4096) for n in names}
    ws = ctypes.create_string_buffer(need + 16)
    pens = (ctypes.c_double * 2)(over.get('skip_value', -3.0), over.get('fill_value', -1.0))
    ptr = {n: ctypes.addressof(b) for n, b in bufs.items()}
    ptr['ws'] = (ctypes.addressof(ws) + 7) & ~7
    ptr['skip_penalty'], ptr['fill_penalty'] = ctypes.addressof(pens), ctypes.addressof(pens) + 8
    for k, v in over.items():
        if k in ptr:
            ptr[k] = v(ptr[k]) if callable(v) else v
    return lib, (bufs, ws, pens), (
        ptr['logits'], ptr['frame_lens'], ptr['y'], a['y_ld'], ptr['label_lens'], ptr['utt_ends'], a['utt_ld'],
        ptr['n_utts'], a['B'], a['T'], a['V'], a['Lmax'], a['Nmax'], a['window'], a['blank'], ptr['skip_penalty'],
        ptr['fill_penalty'], ptr['ws'], over.get('ws_bytes', need), ptr['path'], ptr['first'], ptr['last'],
        ptr['char_logp'], ptr['score'], ptr['utt_first'], ptr['utt_last'], ptr['utt_conf'], ptr['utt_skipped'],
        ptr['is_fill'], None)


def test_the_entries_reject_bad_arguments_before_any_hip_call():
    from ss_asr_amd import _lib
    lib = _lib.load()
    assert lib.ssasr_abi_version() == 16 == _lib.ABI_VERSION
    for name in ('ssasr_ctc_segment_skip', 'ssasr_ctc_segment_skip_ws_bytes'):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    # the plain workspace and one more double per frame
    assert lib.ssasr_ctc_segment_skip_ws_bytes(2, 6, 5, 3, 2) == lib.ssasr_ctc_segment_ws_bytes(2, 6, 5, 3, 2) + 2 * 6 * 8
    assert lib.ssasr_ctc_segment_skip_ws_bytes(1, 32768, 1024, 8191, 1024) == 32768 * 24 + 32768 * 256 * 16 + 32
    for shape in ((1, 32769, 5, 3, 2), (1, 6, 5, 8192, 2), (1, 6, 1025, 3, 2), (1, 6, 1, 3, 2), (0, 6, 5, 3, 2),
                  (65536, 6, 5, 3, 2), (1, 0, 5, 3, 2), (1, 6, 5, 0, 1), (1, 6, 5, 3, 0), (1, 6, 5, 3, 4),
                  (1, 6, 5, 2000, 1025)):
        assert lib.ssasr_ctc_segment_skip_ws_bytes(*shape) == 0, shape
    assert lib.ssasr_ctc_segment_skip_ws_bytes(1, 6, 5, 2000, 1024) > 0
    assert lib.ssasr_ctc_segment_ws_bytes(1, 6, 5, 2000, 1025) > 0            # the plain entry's limit is where it was
    for name in ('logits', 'frame_lens', 'y', 'label_lens', 'utt_ends', 'n_utts', 'ws', 'path', 'first', 'last',
                 'char_logp', 'score', 'utt_first', 'utt_last', 'utt_conf', 'utt_skipped', 'is_fill', 'skip_penalty',
                 'fill_penalty'):
        _, keep, args = _entry_args(**{name: None})
        assert lib.ssasr_ctc_segment_skip(*args) == -1, name
    for bad in (dict(Lmax=8192), dict(T=32769), dict(V=1), dict(V=1025), dict(blank=5), dict(blank=-1), dict(window=0),
                dict(Nmax=0), dict(Nmax=4), dict(ws=lambda p: p + 4), dict(ws_bytes=100), dict(B=0), dict(T=0),
                dict(Lmax=0), dict(y_ld=2), dict(utt_ld=1), dict(Lmax=2000, Nmax=1025, y_ld=2000, utt_ld=1025),
                dict(skip_value=0.5), dict(fill_value=1e-300), dict(skip_value=math.nan), dict(fill_value=math.nan),
                dict(skip_value=math.inf), dict(fill_value=math.inf),
                dict(ws_bytes=int(lib.ssasr_ctc_segment_ws_bytes(2, 6, 5, 3, 2)))):   # the plain size is too small
        _, keep, args = _entry_args(**bad)
        assert lib.ssasr_ctc_segment_skip(*args) == -1, bad


# --------------------------------------------------------------------- host ----
def test_ops_and_segment_argument_errors_that_need_no_gpu():
    from ss_asr_amd import ops
    from ss_asr_amd.asr import Segment, Segmentation
    z = torch.zeros(1, 4, 5)
    i32 = lambda *shape: torch.zeros(*shape, dtype=torch.int32)
    for bad in (0.5, math.nan, -math.inf, math.inf, '1', True):
        for name in ('skip_penalty', 'fill_penalty'):
            with pytest.raises(ValueError, match=name):
                ops.ctc_segment(z, i32(1), i32(1, 2), i32(1), i32(1, 1), i32(1), 2, 1, 3, **{name: bad})
    assert Segment('a', 0, 8, -0.5) == Segment('a', 0, 8, -0.5, False) and Segment('a', 0, 8, -0.5).skipped is False
    assert Segmentation(-1.0, (0, 8), [], None).fillers is None


def test_asr_segment_rejects_bad_penalties():
    from ss_asr_amd import ops
    from ss_asr_amd.ASRDataset import Mapper
    from ss_asr_amd.ctc import JointCTCASR
    x, lens = [torch.zeros(1, 16, 12)], [[16]]
    joint = JointCTCASR(50, 32, 32, 16, 12, 1.0)
    for bad in (0.5, math.nan, -math.inf, 'x', True):
        for name in ('skip_penalty', 'fill_penalty'):
            with pytest.raises(ValueError, match='segment: %s' % name):
                joint.segment(x, lens, [['a']], Mapper(), **{name: bad})
    with pytest.raises(ValueError, match='at most %d' % ops.CTC_SEGMENT_SKIP_MAX_UTTS):
        joint.segment(x, lens, [['a'] * 1025], Mapper(), skip_penalty=-1.0)
    assert joint.last_segment is None and ops.CTC_SEGMENT_SKIP_MAX_UTTS == 1024


def test_write_segments_leaves_skipped_utterances_out(tmp_path):
    from ss_asr_amd.asr import Segment, Segmentation
    from ss_asr_amd.segment import write_segments
    fbank = np.random.default_rng(0).standard_normal((208, 4))
    utts = [Segment('halló', 8, 56, -0.2), Segment('never read', None, None, 0.0, True), Segment('low', 64, 80, -3.5),
            Segment('já', 96, 160, -0.9), Segment('nor this', None, None, 0.0, True)]
    sg = Segmentation(-40.0, (8, 160), utts, None, [(56, 64)])
    index = str(tmp_path / 'index.tsv')
    out = write_segments(sg, fbank, str(tmp_path / 'seg'), index, min_confidence=-1.0, name='rec')
    kept, dropped = out
    assert [w.segment.text for w in kept] == ['halló', 'já'] and out.skipped == 2
    assert [w.segment.text for w in dropped] == ['never read', 'low', 'nor this'] and all(w.row is None for w in dropped)
    assert [w.row['wav_fname'] for w in kept] == ['rec_0000.wav', 'rec_0003.wav']   # k: the place in the transcript
    assert len(open(index, encoding='utf-8').read().splitlines()) == 2
    # a confidence of 0 passes any threshold: it is `skipped` that keeps the utterance out
    out = write_segments(sg, fbank, str(tmp_path / 'seg2'), index, min_confidence=-100.0, name='rec')
    assert len(out[0]) == 3 and out.skipped == 2
    plain = write_segments(Segmentation(-1.0, (8, 56), utts[:1], None), fbank, str(tmp_path / 'seg3'), index,
                           min_confidence=-1.0, name='r')
    assert plain.skipped == 0 and len(plain[0]) == 1
