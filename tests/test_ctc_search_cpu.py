"""CTC-only decoding without a GPU: postprocess.ctc_prefix_beam_reference, the float64 restatement of ssasr_ctc_decode
(include/ssasr.h) that test_gpu_ctc_search.py holds the kernel to, checked here against things that do not share its
recursion -- the sum over every frame labelling, torch's ctc_loss, a hand-built table -- and the argument errors of
the C entries, ops, ASR.decode_ctc and ASRTester's asr.decode_ctc_only."""
import ctypes
import itertools
import math
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_host_cpu import header_prototypes

NEG = -math.inf


def log_softmax64(z):
    z = np.asarray(z, dtype=np.float64)
    m = z.max(-1, keepdims=True)
    return z - (m + np.log(np.exp(z - m).sum(-1, keepdims=True)))


def collapse(path, blank):
    return tuple(int(c) for t, c in enumerate(path) if c != blank and (t == 0 or c != path[t - 1]))


def brute_force(lp, blank):
    """{text: log of the summed probability of every frame labelling that collapses to it}."""
    T, V = lp.shape
    acc = {}
    for path in itertools.product(range(V), repeat=T):
        acc.setdefault(collapse(path, blank), []).append(sum(lp[t, c] for t, c in enumerate(path)))
    return {text: float(np.logaddexp.reduce(np.array(v))) for text, v in acc.items()}


@pytest.mark.parametrize('T', [1, 2, 3, 4])
@pytest.mark.parametrize('blank', [0, 2])
def test_a_beam_that_drops_nothing_sums_every_labelling(T, blank):
    from ss_asr_amd.postprocess import ctc_prefix_beam_reference
    worst = 0.0
    for seed in range(4):
        lp = log_softmax64(4.0 * np.random.default_rng(100 * T + seed).standard_normal((T, 3)))
        exact = brute_force(lp, blank)
        K = len(exact)                                          # every distinct text has a slot: nothing is dropped
        got, gap = ctc_prefix_beam_reference(lp, K, blank)
        assert {text for text, _ in got} == set(exact) and len(got) == K
        assert [s for _, s in got] == sorted((s for _, s in got), reverse=True)
        for text, score in got:
            worst = max(worst, abs(score - exact[text]))
        # 2 non-blank classes: at most 2 candidates more than K per frame, all finite from frame 1 on -- gap is finite
        # only where a frame had more finite candidates than slots
        assert gap == math.inf or gap >= 0.0
    print('T=%d blank=%d: max |score - sum over labellings| = %.3g' % (T, blank, worst))
    assert worst <= 1e-14


def test_the_best_entry_scores_as_torch_ctc_loss_scores_its_text():
    from ss_asr_amd.postprocess import ctc_prefix_beam_reference
    """K = 32, T = 6, V = 5.  32 slots do not hold every text of six frames (85 texts of up to three characters
    alone), and the contract sums only the labellings whose every prefix was in its frame's beam: an entry's score is
    exactly the log-sum of THOSE labellings (checked by enumeration against the traced beams), never above
    -ctc_loss, and equal to -ctc_loss when no labelling of the text ran through a dropped prefix.  At z = 4 N(0, 1),
    seed 0, the best text (2, 1, 4, 1, 4) loses 9.3e-6 to a dropped prefix; the seeds whose best text lost nothing
    must match ctc_loss to 1e-12 (float64 sums of a few hundred terms), and there must be such seeds."""
    T, V = 6, 5
    unrestricted = 0
    for seed in range(8):
        scale = 4.0 if seed < 4 else 8.0
        lp = log_softmax64(scale * np.random.default_rng(seed).standard_normal((T, V)))
        beams = []
        got, _ = ctc_prefix_beam_reference(lp, 32, 0, trace=beams)
        assert len(beams) == T and all(len(b) <= 32 for b in beams)
        text, score = got[0]
        kept, lost = [], []
        for path in itertools.product(range(V), repeat=T):
            if collapse(path, 0) == text:
                inside = all(collapse(path[:t + 1], 0) in beams[t] for t in range(T))
                (kept if inside else lost).append(sum(lp[t, c] for t, c in enumerate(path)))
        assert abs(score - float(np.logaddexp.reduce(np.array(kept)))) <= 1e-12
        nll = float(F.ctc_loss(torch.from_numpy(lp).unsqueeze(1), torch.tensor(list(text), dtype=torch.long).reshape(1, -1),
                               torch.tensor([T]), torch.tensor([len(text)]), blank=0, reduction='sum'))
        assert score <= -nll + 1e-12
        print('seed %d: best %r score %.12f, -ctc_loss %.12f, %d labellings lost' % (seed, text, score, -nll, len(lost)))
        if not lost:
            unrestricted += 1
            assert abs(score + nll) <= 1e-12, (seed, text, score, nll)
    assert unrestricted >= 2


def test_a_text_reached_by_extension_and_by_staying_is_one_member_with_both_routes():
    from ss_asr_amd.postprocess import ctc_prefix_beam_reference
    # classes: 0 blank, 1 'a', 2 'b'.  After frame 0 the beam {a, empty}; at frame 1 the text (1,) is reached by
    # staying (a a, a blank) and by extending the empty text (blank a)
    p = np.array([[0.3, 0.6, 0.1], [0.5, 0.4, 0.1]])
    lp = np.log(p)
    got, gap = ctc_prefix_beam_reference(lp, 2, 0)
    texts = [t for t, _ in got]
    assert len(texts) == len(set(texts)) == 2 and texts[0] == (1,)
    want = 0.6 * 0.4 + 0.6 * 0.5 + 0.3 * 0.4                   # a a, a blank, blank a
    assert abs(math.exp(got[0][1]) - want) <= 1e-15
    assert texts[1] == () and abs(math.exp(got[1][1]) - 0.3 * 0.5) <= 1e-15
    assert gap > 0
    # a repeat needs a blank between: (1, 1) only through a blank a
    p3 = np.array([[0.1, 0.9, 0.0], [0.8, 0.2, 0.0], [0.1, 0.9, 0.0]])
    with np.errstate(divide='ignore'):
        got3, _ = ctc_prefix_beam_reference(np.log(p3), 8, 0)
    d = dict(got3)
    assert abs(math.exp(d[(1, 1)]) - 0.9 * 0.8 * 0.9) <= 1e-15
    # a: aaa, aa_, a__, _aa, _a_, __a, a_a is (1,1): not counted
    assert abs(math.exp(d[(1,)]) - (0.9 * 0.2 * 0.9 + 0.9 * 0.2 * 0.1 + 0.9 * 0.8 * 0.1 + 0.1 * 0.2 * 0.9 + 0.1 * 0.2 * 0.1 +
                                    0.1 * 0.8 * 0.9)) <= 1e-15
    assert all(2 not in t for t in d)                           # a class of probability 0 is no finite candidate
    # a dropped text that comes back: K = 1 keeps one text per frame, yet the result is a text with its full history
    got1, gap1 = ctc_prefix_beam_reference(lp, 1, 0)
    assert got1[0][0] == (1,) and abs(math.exp(got1[0][1]) - (0.6 * 0.4 + 0.6 * 0.5)) <= 1e-15 and gap1 < math.inf


def test_fewer_finite_candidates_than_slots_and_no_frames():
    from ss_asr_amd.postprocess import ctc_prefix_beam_reference
    lp = log_softmax64(np.random.default_rng(0).standard_normal((1, 8)))
    got, gap = ctc_prefix_beam_reference(lp, 32, 0)
    assert len(got) == 8 and gap == math.inf and got[0][0] == collapse([int(lp[0].argmax())], 0)
    assert ctc_prefix_beam_reference(np.zeros((0, 8)), 4, 0) == ([((), 0.0)], math.inf)
    assert ctc_prefix_beam_reference(np.zeros((0, 8)), 0, 0) == ([((), 0.0)], math.inf)
    with pytest.raises(ValueError):
        ctc_prefix_beam_reference(np.zeros(8), 4, 0)
    with pytest.raises(ValueError):
        ctc_prefix_beam_reference(lp, -1, 0)


def test_the_best_path_is_argmax_merge_drop_with_the_lowest_index_on_ties():
    from ss_asr_amd.postprocess import ctc_prefix_beam_reference
    rng = np.random.default_rng(5)
    for T, V, blank in ((1, 2, 0), (7, 5, 0), (40, 50, 3), (12, 4, 3)):
        z = np.round(2.0 * rng.standard_normal((T, V)))         # rounded: many ties
        lp = log_softmax64(z)
        path = lp.argmax(1)
        keep = (path != blank) & np.r_[True, path[1:] != path[:-1]]
        want = tuple(int(c) for c in path[keep])
        got, gap = ctc_prefix_beam_reference(lp, 0, blank)
        assert len(got) == 1 and gap == math.inf and got[0][0] == want
        assert abs(got[0][1] - lp[np.arange(T), path].sum()) <= 1e-12
    tie = np.log(np.full((3, 4), 0.25))
    assert ctc_prefix_beam_reference(tie, 0, 0)[0][0][0] == () and ctc_prefix_beam_reference(tie, 0, 1)[0][0][0] == (0,)
    # repeats with and without a blank between
    onehot = np.full((5, 3), -30.0)
    for t, c in enumerate([1, 1, 0, 1, 2]):
        onehot[t, c] = 0.0
    assert ctc_prefix_beam_reference(onehot, 0, 0)[0][0][0] == (1, 1, 2)
    assert ctc_prefix_beam_reference(onehot, 4, 0)[0][0][0] == (1, 1, 2)


# ---------------------------------------------------------------- C entries ----
def _entry_args(**over):
    a = dict(B=2, T=6, V=5, K=3, blank=0)
    a.update({k: v for k, v in over.items() if k in a})
    from ss_asr_amd import _lib
    lib = _lib.load()
    need = int(lib.ssasr_ctc_decode_ws_bytes(2, 6, 5, 3))
    bufs = {n: ctypes.create_string_buffer(4096) for n in ('logits', 'frame_lens', 'chars', 'n_chars', 'scores', 'n_hyps')}
    ws = ctypes.create_string_buffer(need + 16)
    ptr = {n: ctypes.addressof(b) for n, b in bufs.items()}
    ptr['ws'] = (ctypes.addressof(ws) + 7) & ~7
    for k, v in over.items():
        if k in ptr:
            ptr[k] = v(ptr[k]) if callable(v) else v
    keep = (bufs, ws)
    return lib, keep, (ptr['logits'], ptr['frame_lens'], a['B'], a['T'], a['V'], a['K'], a['blank'], ptr['ws'],
                       over.get('ws_bytes', need), ptr['chars'], ptr['n_chars'], ptr['scores'], ptr['n_hyps'], None)


def test_the_entries_reject_bad_arguments_before_any_hip_call():
    from ss_asr_amd import _lib
    lib = _lib.load()
    assert lib.ssasr_abi_version() == 16 == _lib.ABI_VERSION
    protos, _ = header_prototypes()
    assert {'ssasr_ctc_decode', 'ssasr_ctc_decode_ws_bytes'} <= set(protos) & set(_lib.SIGNATURES)
    ws = lib.ssasr_ctc_decode_ws_bytes
    assert ws(2, 6, 5, 3) == 2 * 2 * 3 * 6 * 4 and ws(2, 6, 5, 0) == 2 * 6 * 4
    assert ws(1, 4096, 64, 32) == 2 * 32 * 4096 * 4 and ws(65535, 1, 2, 1) > 0 and ws(1, 4096, 1024, 0) == 4096 * 4
    for shape in ((0, 6, 5, 3), (65536, 6, 5, 3), (2, 0, 5, 3), (2, 4097, 5, 3), (2, 4097, 5, 0), (2, 6, 1, 3), (2, 6, 65, 1),
                  (2, 6, 65, 32), (2, 6, 1025, 0), (2, 6, 5, 33), (2, 6, 5, -1)):
        assert ws(*shape) == 0, shape
    assert ws(2, 6, 65, 0) > 0 and ws(2, 6, 1024, 0) > 0         # the best path takes the loss's class count
    for name in ('logits', 'frame_lens', 'ws', 'chars', 'n_chars', 'scores', 'n_hyps'):
        _, keep, args = _entry_args(**{name: None})
        assert lib.ssasr_ctc_decode(*args) == -1, name
    for bad in (dict(B=0), dict(B=65536), dict(T=0), dict(T=4097), dict(V=1), dict(V=65), dict(K=33), dict(K=-1),
                dict(blank=5), dict(blank=-1), dict(ws=lambda p: p + 4), dict(ws_bytes=2 * 2 * 3 * 6 * 4 - 1),
                dict(V=1025, K=0)):
        _, keep, args = _entry_args(**bad)
        assert lib.ssasr_ctc_decode(*args) == -1, bad


# ------------------------------------------------------------ Python surface ----
def test_ops_and_decode_ctc_reject_bad_arguments():
    from ss_asr_amd import ops
    from ss_asr_amd.asr import ASR
    from ss_asr_amd.ctc import JointCTCASR
    from ss_asr_amd.ASRDataset import Mapper
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.ctc_decode(torch.zeros(1, 4, 5), torch.tensor([4], dtype=torch.int32), 2)
    model = ASR(50, 32, 32, 16, 12, 1.0)
    with pytest.raises(ValueError, match=r'needs a model with a ctc_head \(ctc.JointCTCASR\); ASR has none') as mine:
        model.decode_ctc([torch.zeros(1, 16, 12)], [[16]], Mapper())
    with pytest.raises(ValueError) as plain:
        model._ctc_head(0.3)
    assert str(plain.value) == str(mine.value)
    joint = JointCTCASR(50, 32, 32, 16, 12, 1.0)
    for bad in (-1, 33, 2.0, True, None, '8'):
        with pytest.raises(ValueError, match='beam_size'):
            joint.decode_ctc([torch.zeros(1, 16, 12)], [[16]], Mapper(), beam_size=bad)
    with pytest.raises(ValueError, match='utterances'):
        joint.decode_ctc([torch.zeros(1, 16, 12)], [], Mapper())
    with pytest.raises(ValueError, match='utterances'):
        joint.decode_ctc([], [], Mapper())
    with pytest.raises(RuntimeError, match='no CPU path|GPU'):
        joint.decode_ctc([torch.zeros(1, 16, 12)], [[16]], Mapper())
    assert joint.last_ctc_decode is None and joint.last_hyps is None


def _tester(root, mdl_extra, **keys):
    from ss_asr_amd.trainer import ASRTester
    config = {'asr': dict({'mdl': dict({'encoder_state_size': 32, 'decoder_state_size': 32, 'mlp_out_size': 16,
                                        'feature_dim': 12, 'tf_rate': 1.0}, **mdl_extra),
                           'test_index': os.path.join(root, 'none.tsv'), 'decode_lm_weight': 0.5, 'decode_beam_size': 1,
                           'decode_jobs': 1, 'max_decode_step_ratio': 0.25, 'loader_jobs': 0}, **keys),
              'char_lm': {'mdl': {'hidden_size': 16}}}
    paras = types.SimpleNamespace(name='dec', logdir=os.path.join(root, 'runs'), ckpdir=os.path.join(root, 'result'),
                                  verbose=False, seed=1)
    return ASRTester(config, paras)


def test_tester_validates_decode_ctc_only(tmp_path):
    from ss_asr_amd.trainer import ASRTester
    beam = ASRTester.ctc_only_beam
    assert beam({}) is None and beam({'decode_ctc_only': False}) is None and beam({'decode_ctc_only': None}) is None
    assert beam({'decode_ctc_only': True}) == 8 and beam({'decode_ctc_only': {}}) == 8
    assert beam({'decode_ctc_only': {'beam_size': 0}}) == 0 and beam({'decode_ctc_only': {'beam_size': 32}}) == 32
    for bad in (3, 'x', [8], {'beam': 3}, {'beam_size': -1}, {'beam_size': 33}, {'beam_size': 2.0}, {'beam_size': True}):
        with pytest.raises(ValueError, match='decode_ctc_only'):
            beam({'decode_ctc_only': bad})
    # MBR chooses among THIS search's list
    assert ASRTester.mbr_args({'decode_mbr': True, 'decode_beam_size': 1, 'decode_ctc_only': {'beam_size': 4}}) == \
        {'unit': 'word', 'scale': 1.0}
    with pytest.raises(ValueError, match=r'decode_ctc_only\.beam_size must be >= 2'):
        ASRTester.mbr_args({'decode_mbr': True, 'decode_beam_size': 5, 'decode_ctc_only': {'beam_size': 1}})
    with pytest.raises(ValueError, match=r'decode_beam_size must be >= 2'):
        ASRTester.mbr_args({'decode_mbr': True, 'decode_beam_size': 1})
    root = str(tmp_path)
    t = _tester(root, {}, decode_ctc_only={'beam_size': 4})
    with pytest.raises(ValueError, match=r'asr\.decode_ctc_only.*ctc_weight'):
        t.set_model()
    assert '_ctconly' not in t.decode_file
    for clash in (dict(decode_ctc_weight=0.3), dict(decode_length_bonus=0.5), dict(decode_coverage_weight=0.2),
                  dict(decode_end_margin=1.0)):
        t = _tester(root, {'ctc_weight': 0.3}, decode_ctc_only={'beam_size': 4}, **clash)
        with pytest.raises(ValueError, match=r'decode_ctc_only.*asr\.%s' % list(clash)[0]):
            t.set_model()
