"""CTC forced alignment without a GPU: the float64 checker of ssasr_ctc_align (viterbi_reference, written from the
semantics in include/ssasr.h alone; it shares nothing with the library's host code and test_gpu_align.py imports
it), pinned by brute force over every frame labelling and against torch's ctc_loss; the C entries' argument checks,
which return before any HIP call; and the Python surface's errors and frame conversion."""
import ctypes
import itertools
import math
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

NEG = -math.inf


def viterbi_reference(logits, length, labels, blank):
    """The most probable CTC path of `labels` through the first min(length, T) rows of logits [T, V], in float64 on
    the RAW logits, in the header's order: one add per lattice value, the larger value wins, among equals staying
    wins over s - 1 over s - 2, at the end S - 1 wins over S - 2.  -> None when no alignment fits, else a namespace
    of path [len], first / last [L], char_logp [L], score, d_end and lse [len] (all float64)."""
    logits = np.asarray(logits)
    T, V = logits.shape
    n, L = min(int(length), T), len(labels)
    if n < 1:
        return None
    S = 2 * L + 1
    lab = np.full(S, blank, dtype=np.int64)
    lab[1::2] = labels
    skip = np.zeros(S, dtype=bool)
    for s in range(3, S, 2):
        skip[s] = lab[s] != lab[s - 2]
    x = logits[:n].astype(np.float64)
    d = np.full(S, NEG)
    d[:2] = x[0, lab[:2]]
    back = np.zeros((n, S), dtype=np.int64)
    for t in range(1, n):
        one = np.concatenate(([NEG], d[:-1]))
        two = np.concatenate(([NEG, NEG], d[:-2]))[:S]
        two[~skip] = NEG
        best = d.copy()
        m = one > best
        best[m], back[t, m] = one[m], 1
        m = two > best
        best[m], back[t, m] = two[m], 2
        d = best + x[t, lab]
    s = S - 1
    if S > 1 and d[S - 2] > d[S - 1]:
        s = S - 2
    d_end = d[s]
    if d_end == NEG:
        return None
    path = np.zeros(n, dtype=np.int64)
    for t in range(n - 1, -1, -1):
        path[t] = s
        s -= back[t, s]
    m = x.max(1)
    lse = m + np.log(np.exp(x - m[:, None]).sum(1))
    first, last, logp = np.zeros(L, dtype=np.int64), np.zeros(L, dtype=np.int64), np.zeros(L)
    for j in range(L):
        frames = np.nonzero(path == 2 * j + 1)[0]
        first[j], last[j] = frames[0], frames[-1]
        logp[j] = (x[frames, labels[j]] - lse[frames]).sum()
    return types.SimpleNamespace(path=path, first=first, last=last, char_logp=logp, score=d_end - lse.sum(),
                                 d_end=d_end, lse=lse, states=lab)


def collapse(frames, blank):
    out, prev = [], None
    for c in frames:
        if c != prev and c != blank:
            out.append(c)
        prev = c
    return out


BRUTE = [(T, labels) for T in range(1, 7) for labels in
         ([], [1], [2], [1, 2], [1, 1], [2, 2], [1, 2, 1], [1, 1, 2], [2, 2, 2], [2, 1, 1], [1, 2, 2])]


def test_the_checker_is_the_best_of_all_frame_labellings():
    """V = 3, blank 0: every one of the 3^T labellings that collapses to the labels, its logits summed in frame
    order.  The best sum is the checker's d_end to the bit and its labelling the checker's path; the cases without a
    labelling are the checker's None.  No case is left out: best and second best differ everywhere."""
    rng = np.random.default_rng(7)
    compared = none = 0
    for T, labels in BRUTE:
        logits = rng.standard_normal((T, 3)).astype(np.float32)
        sums = []
        for frames in itertools.product(range(3), repeat=T):
            if collapse(frames, 0) == labels:
                total = np.float64(logits[0, frames[0]])
                for t in range(1, T):
                    total = total + np.float64(logits[t, frames[t]])
                sums.append((total, frames))
        got = viterbi_reference(logits, T, labels, 0)
        if not sums:
            assert got is None and T < len(labels) + sum(a == b for a, b in zip(labels, labels[1:]))
            none += 1
            continue
        sums.sort(key=lambda p: -p[0])
        assert len(sums) == 1 or sums[0][0] > sums[1][0], (T, labels)
        assert got.d_end == sums[0][0], (T, labels)
        assert [int(got.states[s]) for s in got.path] == list(sums[0][1]), (T, labels)
        for j, c in enumerate(labels):
            run = [t for t in range(T) if got.path[t] == 2 * j + 1]
            assert run == list(range(got.first[j], got.last[j] + 1)) and run
        compared += 1
    assert compared >= 40 and none >= 10


def torch_total(logits, labels, blank):
    lp = torch.log_softmax(torch.from_numpy(np.asarray(logits, dtype=np.float64)), -1).unsqueeze(1)
    return -float(F.ctc_loss(lp, torch.tensor([labels], dtype=torch.long), torch.tensor([lp.shape[0]]),
                             torch.tensor([len(labels)]), blank=blank, reduction='sum'))


def test_the_score_is_at_most_the_total_probability_and_equal_for_a_single_path():
    rng = np.random.default_rng(11)
    for T, V, labels, blank in ((12, 6, [1, 2, 2, 5], 0), (30, 50, list(rng.integers(1, 50, 11)), 0),
                                (9, 5, [0, 1, 0], 3), (5, 4, [], 0)):
        logits = rng.standard_normal((T, V)).astype(np.float32)
        got = viterbi_reference(logits, T, [int(c) for c in labels], blank)
        total = torch_total(logits, [int(c) for c in labels], blank)
        assert got.score <= total + 1e-9
        assert abs(got.char_logp.sum() + sum(float((logits[t].astype(np.float64) - got.lse[t])[blank])
                                             for t in range(T) if got.path[t] % 2 == 0) - got.score) < 1e-9
    # T == L without repeats: exactly one path, so the best path is the total
    for T, V in ((1, 4), (4, 7), (9, 50)):
        logits = rng.standard_normal((T, V)).astype(np.float32)
        labels = [1 + (3 * j) % (V - 1) for j in range(T)]
        assert all(a != b for a, b in zip(labels, labels[1:]))
        got = viterbi_reference(logits, T, labels, 0)
        assert list(got.path) == [2 * j + 1 for j in range(T)]
        assert abs(got.score - torch_total(logits, labels, 0)) < 1e-9


def test_a_repeated_label_needs_a_blank_between():
    rng = np.random.default_rng(3)
    logits = rng.standard_normal((3, 4)).astype(np.float32)
    assert viterbi_reference(logits, 2, [2, 2], 0) is None
    assert viterbi_reference(logits[:2], 5, [2, 2], 0) is None        # length is clipped to the rows
    got = viterbi_reference(logits, 3, [2, 2], 0)
    assert list(got.path) == [1, 2, 3] and [int(got.states[s]) for s in got.path] == [2, 0, 2]
    assert list(got.first) == [0, 2] and list(got.last) == [0, 2]
    assert viterbi_reference(logits, 0, [], 0) is None


def test_all_equal_logits_are_decided_by_the_tie_rule():
    """S - 1 wins the end, and staying wins every step on the way back: the path sits in the final blank for as long
    as that state is reachable, i.e. it runs through the labels as early as it can (with the blank that the repeat
    needs, and the skip where the labels differ)."""
    for value in (0.0, 0.37):
        got = viterbi_reference(np.full((9, 5), value, dtype=np.float32), 9, [4, 4, 2], 0)
        assert list(got.path) == [1, 2, 3, 5, 6, 6, 6, 6, 6]


# ---------------------------------------------------------------- C entries ----
def _entry_args(**over):
    B, T, V, Lmax = 2, 6, 5, 3
    a = dict(B=B, T=T, V=V, Lmax=Lmax, blank=0, y_ld=4)
    a.update({k: v for k, v in over.items() if k in a})
    from ss_asr_amd import _lib
    lib = _lib.load()
    need = int(lib.ssasr_ctc_align_ws_bytes(B, T, V, Lmax))
    bufs = {n: ctypes.create_string_buffer(4096) for n in
            ('logits', 'frame_lens', 'y', 'label_lens', 'path', 'first', 'last', 'char_logp', 'score')}
    ws = ctypes.create_string_buffer(need + 16)
    base = (ctypes.addressof(ws) + 7) & ~7
    ptr = {n: ctypes.addressof(b) for n, b in bufs.items()}
    ptr['ws'] = base
    for k, v in over.items():
        if k in ptr or k == 'ws':
            ptr[k] = v(ptr[k]) if callable(v) else v
    ws_bytes = over.get('ws_bytes', need)
    keep = (bufs, ws)
    return lib, need, keep, (ptr['logits'], ptr['frame_lens'], ptr['y'], a['y_ld'], ptr['label_lens'], a['B'], a['T'],
                             a['V'], a['Lmax'], a['blank'], ptr['ws'], ws_bytes, ptr['path'], ptr['first'], ptr['last'],
                             ptr['char_logp'], ptr['score'], None)


def test_the_entries_reject_bad_arguments_before_any_hip_call():
    from ss_asr_amd import _lib
    lib = _lib.load()
    assert lib.ssasr_abi_version() == 16 == _lib.ABI_VERSION
    assert 'ssasr_ctc_align' in _lib.SIGNATURES and 'ssasr_ctc_align_ws_bytes' in _lib.SIGNATURES
    assert lib.ssasr_ctc_align_ws_bytes(2, 6, 5, 3) >= 2 * 6 * 8
    for shape in ((2, 6, 5, 512), (2, 6, 1, 3), (2, 6, 1025, 3), (0, 6, 5, 3), (2, 0, 5, 3), (65536, 6, 5, 3), (2, 6, 5, -1)):
        assert lib.ssasr_ctc_align_ws_bytes(*shape) == 0, shape
    # the LDS form needs the normalisers only; one frame past the boundary the back-pointers are added
    # (every form: a normaliser per frame and four phase stamps per utterance)
    assert lib.ssasr_ctc_align_ws_bytes(1, 819, 50, 300) == 819 * 8 + 32
    assert lib.ssasr_ctc_align_ws_bytes(1, 820, 50, 300) == 820 * 8 + 820 * 10 * 16 + 32
    assert lib.ssasr_ctc_align_ws_bytes(3, 8192, 50, 31) == 3 * (8192 * 8 + 32)
    assert lib.ssasr_ctc_align_ws_bytes(3, 8193, 50, 31) == 3 * (8193 * (8 + 16) + 32)
    for name in ('logits', 'frame_lens', 'y', 'label_lens', 'ws', 'path', 'first', 'last', 'char_logp', 'score'):
        _, _, keep, args = _entry_args(**{name: None})
        assert lib.ssasr_ctc_align(*args) == -1, name
    for bad in (dict(Lmax=512), dict(V=1), dict(blank=5), dict(blank=-1), dict(ws=lambda p: p + 4),
                dict(ws_bytes=2 * 6 * 8 - 1), dict(B=0), dict(T=0)):
        _, _, keep, args = _entry_args(**bad)
        assert lib.ssasr_ctc_align(*args) == -1, bad


# ------------------------------------------------------------ Python surface ----
def test_align_needs_a_ctc_head_and_known_characters():
    from ss_asr_amd.asr import ASR, Alignment
    from ss_asr_amd.ctc import JointCTCASR
    from ss_asr_amd.ASRDataset import Mapper
    model = ASR(50, 32, 32, 16, 12, 1.0)
    with pytest.raises(ValueError, match=r'needs a model with a ctc_head \(ctc.JointCTCASR\); ASR has none'):
        model.align([torch.zeros(1, 16, 12)], [[16]], ['ab'], Mapper())
    with pytest.raises(ValueError, match='ctc_head') as plain:
        model._ctc_head(0.3)
    with pytest.raises(ValueError) as mine:
        model.align([], [], [], Mapper())
    assert str(plain.value) == str(mine.value)
    joint = JointCTCASR(50, 32, 32, 16, 12, 1.0)
    with pytest.raises(ValueError, match='does not know'):
        joint.align([torch.zeros(1, 16, 12)], [[16]], ['a中b'], Mapper())
    assert joint.last_align is None and Alignment(1.0, None).chars is None


def test_encoder_frames_to_input_frames():
    from ss_asr_amd.asr import ENCODER_STRIDE, input_span
    assert ENCODER_STRIDE == 8
    n = 43                                   # five encoder frames, three input frames left over
    assert input_span(0, 0, n) == (0, 8) and input_span(1, 3, n) == (8, 32) and input_span(4, 4, n) == (32, 40)
    assert input_span(4, 5, n) == (32, 43) and input_span(5, 5, n) == (40, 43) and input_span(6, 7, n) == (43, 43)
    lo, hi = input_span(1, 3, n, frame_shift=0.01)
    assert abs(lo - 0.08) < 1e-12 and abs(hi - 0.32) < 1e-12
    assert input_span(5, 5, n, frame_shift=0.5) == (20.0, 21.5)


def test_tester_with_decode_align_needs_a_ctc_head(tmp_path):
    from ss_asr_amd.trainer import ASRTester
    root = str(tmp_path)
    config = {'asr': {'mdl': {'encoder_state_size': 32, 'decoder_state_size': 32, 'mlp_out_size': 16, 'feature_dim': 12,
                              'tf_rate': 1.0},
                      'test_index': os.path.join(root, 'none.tsv'), 'decode_lm_weight': 0.5, 'decode_beam_size': 1,
                      'decode_jobs': 1, 'max_decode_step_ratio': 0.25, 'loader_jobs': 0, 'decode_align': True},
              'char_lm': {'mdl': {'hidden_size': 16}}}
    paras = types.SimpleNamespace(name='dec', logdir=os.path.join(root, 'runs'), ckpdir=os.path.join(root, 'result'),
                                  verbose=False, seed=1)
    t = ASRTester(config, paras)
    with pytest.raises(ValueError, match=r'asr\.decode_align.*ctc_weight'):
        t.set_model()
    assert not hasattr(t, 'last_alignments') and not t.decode_file.endswith('_align')
