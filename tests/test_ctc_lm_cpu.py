"""CTC decoding with the CharLM in the search, without a GPU: postprocess.ctc_prefix_beam_lm_reference, the float64
restatement of ssasr_ctc_decode_lm (include/ssasr.h) that test_gpu_ctc_lm.py holds the kernel to, checked here against
things that do not share its recursion -- the sum over every frame labelling plus an LM evaluated through
torch.nn.GRUCell, hand-built tables -- and the argument errors of the C entries, ops, ASR.decode_ctc /
decode_two_pass and ASRTester's asr.decode_ctc_only keys."""
import ctypes
import math

import numpy as np
import pytest
import torch

from test_ctc_search_cpu import brute_force, log_softmax64
from test_host_cpu import header_prototypes

NEG = -math.inf


def lm_arrays(V, H, seed, scale=0.5):
    rng = np.random.default_rng([V, H, seed, 7])
    shapes = [(V, H), (3 * H, H), (3 * H, H), (3 * H,), (3 * H,), (3 * H, H), (3 * H, H), (3 * H,), (3 * H,), (V, H), (V,)]
    return [scale * rng.standard_normal(s) for s in shapes]


def lm_logps(lm, text, eos):
    """(log P_lm(text), log P_lm(eos | text); 0 with eos < 0) through torch.nn.GRUCell in float64: <SOS> = 0 is fed
    first, then the characters one by one."""
    emb, w_ih1, w_hh1, b_ih1, b_hh1, w_ih2, w_hh2, b_ih2, b_hh2, w_out, b_out = [torch.from_numpy(a) for a in lm]
    H = emb.shape[1]
    c1, c2 = torch.nn.GRUCell(H, H).double(), torch.nn.GRUCell(H, H).double()
    with torch.no_grad():
        for cell, (w_ih, w_hh, b_ih, b_hh) in ((c1, (w_ih1, w_hh1, b_ih1, b_hh1)), (c2, (w_ih2, w_hh2, b_ih2, b_hh2))):
            cell.weight_ih.copy_(w_ih)
            cell.weight_hh.copy_(w_hh)
            cell.bias_ih.copy_(b_ih)
            cell.bias_hh.copy_(b_hh)
        h1 = h2 = torch.zeros(1, H, dtype=torch.float64)
        total = 0.0
        fed = (0,) + tuple(text)
        for i, c in enumerate(fed):
            h1 = c1(emb[c][None], h1)
            h2 = c2(h1, h2)
            row = torch.log_softmax(h2 @ w_out.T + b_out, -1)[0]
            if i < len(text):
                total += float(row[text[i]])
        return total, (float(row[eos]) if eos >= 0 else 0.0)


def test_zero_weights_are_the_plain_checker_exactly():
    from ss_asr_amd.postprocess import ctc_prefix_beam_lm_reference, ctc_prefix_beam_reference
    for T, V, K, seed in ((1, 8, 3, 0), (5, 8, 2, 1), (20, 8, 8, 2), (20, 40, 3, 3)):
        lp = log_softmax64(4.0 * np.random.default_rng([T, V, seed]).standard_normal((T, V)))
        for lm in (None, lm_arrays(V, 8, seed)):
            tr_a, tr_b, parts = [], [], []
            got, gap = ctc_prefix_beam_lm_reference(lp, K, lm, 0.0, 0.0, V - 1, trace=tr_a, parts=parts)
            want, plain_gap = ctc_prefix_beam_reference(lp, K, trace=tr_b)
            assert got == want and tr_a == tr_b
            assert [p[0] for p in parts] == [s for _, s in want] and all(p[1] == 0.0 for p in parts)
            final = min([math.inf] + [a[1] - b[1] for a, b in zip(want, want[1:])])
            assert gap == min(plain_gap, final)
        lp32 = lp.astype(np.float32)
        assert ctc_prefix_beam_lm_reference(lp32, K, None, dtype=np.float32)[0] == \
            ctc_prefix_beam_reference(lp32, K, dtype=np.float32)[0]


@pytest.mark.parametrize('T', [1, 2, 3, 4])
@pytest.mark.parametrize('blank,eos', [(0, 2), (1, 0), (0, -1)])
def test_a_beam_that_drops_nothing_scores_every_text_as_the_enumeration_plus_the_lm(T, blank, eos):
    from ss_asr_amd.postprocess import ctc_prefix_beam_lm_reference
    V, alpha, beta = 3, 0.5, 0.3
    lp = log_softmax64(np.random.default_rng([T, blank, 9]).standard_normal((T, V)) * 2.0)
    lm = lm_arrays(V, 4, T)
    every = brute_force(lp, blank)
    parts = []
    got, gap = ctc_prefix_beam_lm_reference(lp, 32, lm, alpha, beta, eos, blank, parts=parts)
    assert len(every) <= 32 and {t for t, _ in got} == set(every)
    a32, b32 = float(np.float32(alpha)), float(np.float32(beta))
    for (text, total), (ctc, lmv) in zip(got, parts):
        body, end = lm_logps(lm, text, eos)
        assert abs(ctc - every[text]) <= 1e-12
        assert abs(lmv - (body + end)) <= 1e-12
        assert abs(total - (every[text] + a32 * (body + end) + b32 * len(text))) <= 1e-12
    assert [s for _, s in got] == sorted((s for _, s in got), reverse=True)
    assert gap == min(a[1] - b[1] for a, b in zip(got, got[1:])) if len(got) > 1 else gap == math.inf


def peaked_lm(V, H, favourite, strength):
    """A CharLM whose output bias alone speaks: every row is log_softmax(b_out), b_out[favourite] = strength."""
    lm = [np.zeros(s) for s in [(V, H), (3 * H, H), (3 * H, H), (3 * H,), (3 * H,), (3 * H, H), (3 * H, H), (3 * H,),
                                (3 * H,), (V, H), (V,)]]
    lm[10][favourite] = strength
    return lm


def test_the_lm_flips_the_winner_of_a_hand_built_table():
    from ss_asr_amd.postprocess import ctc_prefix_beam_lm_reference
    # one frame, classes (blank, 1, 2): the head prefers 1 by log(0.5 / 0.4); the LM prefers 2 by 4 nats
    lp = np.log(np.array([[0.1, 0.5, 0.4]]))
    lm = peaked_lm(3, 4, 2, 4.0)
    row = log_softmax64(lm[10])
    assert ctc_prefix_beam_lm_reference(lp, 3, None)[0][0][0] == (1,)
    parts = []
    got, gap = ctc_prefix_beam_lm_reference(lp, 3, lm, 1.0, 0.0, -1, parts=parts)
    assert [t for t, _ in got] == [(2,), (), (1,)]              # the empty text has no LM term without an end term
    assert abs(got[0][1] - (math.log(0.4) + row[2])) <= 1e-12 and abs(got[2][1] - (math.log(0.5) + row[1])) <= 1e-12
    assert abs(got[1][1] - math.log(0.1)) <= 1e-12 and parts[1] == (math.log(0.1), 0.0)
    assert abs(gap - min(got[0][1] - got[1][1], got[1][1] - got[2][1])) <= 1e-12     # nothing was dropped: the final gaps
    # a negative weight turns the LM's preference round; a length bonus alone lifts the longer texts
    assert ctc_prefix_beam_lm_reference(lp, 3, lm, -1.0)[0][0][0] == (1,)
    assert ctc_prefix_beam_lm_reference(np.log(np.array([[0.5, 0.3, 0.2]])), 3, None, 0.0, 1.0)[0][0][0] == (1,)


def test_the_lm_keeps_a_text_that_the_plain_search_drops():
    from ss_asr_amd.postprocess import ctc_prefix_beam_lm_reference, ctc_prefix_beam_reference
    # K = 1.  Frame 0: the head ranks 1 above 2, so the plain search keeps (1,) and (2,) is gone for good; frame 1
    # is all blank.  The LM wants 2: with it the search keeps (2,), which no rescoring of the plain list could return.
    lp = np.log(np.array([[0.1, 0.5, 0.4], [0.98, 0.01, 0.01]]))
    lm = peaked_lm(3, 4, 2, 4.0)
    tr_plain, tr_lm = [], []
    plain, _ = ctc_prefix_beam_reference(lp, 1, trace=tr_plain)
    fused, _ = ctc_prefix_beam_lm_reference(lp, 1, lm, 1.0, 0.0, -1, trace=tr_lm)
    assert plain[0][0] == (1,) and all((2,) not in beam for beam in tr_plain)
    assert fused[0][0] == (2,) and tr_lm[0] == frozenset({(2,)})
    row = log_softmax64(lm[10])
    # its CTC part is the mass of the labellings (2, blank) and (2, 2): g stays a pure CTC quantity
    parts = []
    ctc_prefix_beam_lm_reference(lp, 1, lm, 1.0, 0.0, -1, parts=parts)
    assert abs(parts[0][0] - math.log(0.4 * 0.98 + 0.4 * 0.01)) <= 1e-12 and abs(parts[0][1] - row[2]) <= 1e-12


def test_the_end_term_reranks_the_final_list_and_eos_below_zero_adds_none():
    from ss_asr_amd.postprocess import ctc_prefix_beam_lm_reference
    lp = log_softmax64(np.random.default_rng(5).standard_normal((4, 4)) * 2.0)
    lm = lm_arrays(4, 4, 5, 1.0)
    p_no, p_eos = [], []
    no, _ = ctc_prefix_beam_lm_reference(lp, 4, lm, 0.7, 0.0, -1, parts=p_no)
    with_eos, _ = ctc_prefix_beam_lm_reference(lp, 4, lm, 0.7, 0.0, 3, parts=p_eos)
    assert {t for t, _ in no} == {t for t, _ in with_eos}        # the end term enters after the last frame only
    a32 = float(np.float32(0.7))
    by_text = {t: (s, p) for (t, s), p in zip(no, p_no)}
    for (text, total), (ctc, lmv) in zip(with_eos, p_eos):
        end = lm_logps(lm, text, 3)[1]
        assert abs(total - (by_text[text][0] + a32 * end)) <= 1e-12 and abs(lmv - (by_text[text][1][1] + end)) <= 1e-12
        assert ctc == by_text[text][1][0]
    assert [s for _, s in with_eos] == sorted((s for _, s in with_eos), reverse=True)
    for bad in (dict(K=0), dict(eos=4), dict(lm_weight=math.inf), dict(lm=None)):
        args = dict(K=2, lm=lm, lm_weight=0.5, eos=3)
        args.update(bad)
        with pytest.raises(ValueError):
            ctc_prefix_beam_lm_reference(lp, args['K'], args['lm'], args['lm_weight'], 0.0, args['eos'])


# ---------------------------------------------------------------- C entries ----
def _entry_args(**over):
    from ss_asr_amd import _lib
    lib = _lib.load()
    a = dict(B=2, T=6, V=5, K=3, blank=0, lm_weight=0.5, length_bonus=0.25, eos=1)
    a.update({k: v for k, v in over.items() if k in a})
    H = 8
    need = int(lib.ssasr_ctc_decode_lm_ws_bytes(2, 6, 5, 3, H))
    names = ('logits', 'frame_lens', 'chars', 'n_chars', 'scores', 'n_hyps', 'ctc_scores', 'lm_scores')
    bufs = {n: ctypes.create_string_buffer(4096) for n in names}
    ws = ctypes.create_string_buffer(need + 32)
    weights = ctypes.create_string_buffer(16 * 4096 + 16)
    w0 = (ctypes.addressof(weights) + 15) & ~15
    ptr = {n: ctypes.addressof(b) for n, b in bufs.items()}
    ptr['ws'] = (ctypes.addressof(ws) + 15) & ~15
    for k, v in over.items():
        if k in ptr:
            ptr[k] = v(ptr[k]) if callable(v) else v
    lm = _lib.CharLM(over.get('lm_V', 5), over.get('lm_H', H), *[w0 + 4096 * i + over.get('lm_shift', 0) for i in range(11)])
    lm_arg = None if over.get('lm', 1) is None else ctypes.byref(lm)
    keep = (bufs, ws, weights, lm)
    return lib, keep, (ptr['logits'], ptr['frame_lens'], a['B'], a['T'], a['V'], a['K'], a['blank'], ptr['ws'],
                       over.get('ws_bytes', need), ptr['chars'], ptr['n_chars'], ptr['scores'], ptr['n_hyps'], lm_arg,
                       a['lm_weight'], a['length_bonus'], a['eos'], ptr['ctc_scores'], ptr['lm_scores'], None)


def test_the_entries_reject_bad_arguments_before_any_hip_call():
    from ss_asr_amd import _lib
    lib = _lib.load()
    assert lib.ssasr_abi_version() == 16 == _lib.ABI_VERSION
    protos, _ = header_prototypes()
    assert {'ssasr_ctc_decode_lm', 'ssasr_ctc_decode_lm_ws_bytes'} <= set(protos) & set(_lib.SIGNATURES)
    ws = lib.ssasr_ctc_decode_lm_ws_bytes
    texts = (2 * 2 * 3 * 6 * 4 + 15) // 16 * 16
    assert ws(2, 6, 5, 3, 0) == texts + 2 * 4
    # per utterance: 2 x K x 2H states, and 3 of the 8-in-flight blocks: H + 3H + 3H floats and a 64-float row each
    assert ws(2, 6, 5, 3, 8) == 2 * 4 * (2 * 3 * 16 + 3 * (7 * 8 + 64)) + texts + 2 * 4
    assert ws(1, 8, 8, 32, 512) == 4 * (2 * 32 * 1024 + 8 * (7 * 512 + 64)) + 2 * 32 * 8 * 4 + 4
    assert ws(1, 4096, 64, 32, 4096) > 0 and ws(65535, 1, 2, 1, 4) > 0
    for shape in ((0, 6, 5, 3, 8), (65536, 6, 5, 3, 8), (2, 0, 5, 3, 8), (2, 4097, 5, 3, 8), (2, 6, 1, 3, 8), (2, 6, 65, 3, 8),
                  (2, 6, 5, 0, 8), (2, 6, 5, 33, 8), (2, 6, 5, -1, 8), (2, 6, 5, 3, 6), (2, 6, 5, 3, -4), (2, 6, 5, 3, 4100)):
        assert ws(*shape) == 0, shape
    for name in ('logits', 'frame_lens', 'ws', 'chars', 'n_chars', 'scores', 'n_hyps', 'ctc_scores', 'lm_scores', 'lm'):
        _, keep, args = _entry_args(**{name: None})
        assert lib.ssasr_ctc_decode_lm(*args) == -1, name
    for bad in (dict(B=0), dict(B=65536), dict(T=0), dict(T=4097), dict(V=1), dict(V=65), dict(K=0), dict(K=33), dict(K=-1),
                dict(blank=5), dict(blank=-1), dict(eos=5), dict(lm_weight=math.inf), dict(lm_weight=math.nan),
                dict(length_bonus=-math.inf), dict(ws=lambda p: p + 8), dict(ws_bytes=ws(2, 6, 5, 3, 8) - 1),
                dict(lm_V=6), dict(lm_H=6), dict(lm_H=0), dict(lm_H=4100), dict(lm_shift=4),
                dict(lm_weight=0.0, lm_V=6)):
        _, keep, args = _entry_args(**bad)
        assert lib.ssasr_ctc_decode_lm(*args) == -1, bad


# ------------------------------------------------------------ Python surface ----
def test_ops_decode_ctc_and_two_pass_reject_bad_arguments():
    from ss_asr_amd import ops
    from ss_asr_amd.ASRDataset import Mapper
    from ss_asr_amd.charlm import CharLM
    from ss_asr_amd.ctc import JointCTCASR
    z, lens = torch.zeros(1, 4, 5), torch.tensor([4], dtype=torch.int32)
    lm = CharLM(5, 8)
    for bad in (0, 33, 2.0, True, None):
        with pytest.raises(ValueError, match='beam_size'):
            ops.ctc_decode_lm(z, lens, bad, lm, 0.5)
    with pytest.raises(ValueError, match='finite'):
        ops.ctc_decode_lm(z, lens, 2, lm, math.nan)
    with pytest.raises(ValueError, match='finite'):
        ops.ctc_decode_lm(z, lens, 2, lm, 0.5, math.inf)
    with pytest.raises(ValueError, match='needs a language model'):
        ops.ctc_decode_lm(z, lens, 2, None, 0.5)
    with pytest.raises(ValueError, match=r'\[B, T, V\]'):
        ops.ctc_decode_lm(z[0], lens, 2, lm, 0.5)
    with pytest.raises(TypeError, match='frame_lens'):
        ops.ctc_decode_lm(z, lens.long(), 2, lm, 0.5)
    with pytest.raises(ValueError, match='blank'):
        ops.ctc_decode_lm(z, lens, 2, lm, 0.5, blank=5)
    with pytest.raises(ValueError, match='eos'):
        ops.ctc_decode_lm(z, lens, 2, lm, 0.5, eos=5)
    with pytest.raises(ValueError, match='classes'):
        ops.ctc_decode_lm(z, lens, 2, CharLM(6, 8), 0.5)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.ctc_decode_lm(z, lens, 2, lm, 0.5)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.ctc_head_decode_lm(torch.zeros(1, 4, 8), torch.zeros(5, 8), torch.zeros(5), lens, 2, lm, 0.5)
    joint = JointCTCASR(50, 32, 32, 16, 12, 1.0)
    lm50 = CharLM(50, 8)
    one = ([torch.zeros(1, 16, 12)], [[16]], Mapper())
    for key in ('lm_weight', 'length_bonus'):
        for bad in (math.nan, math.inf, '1', None, True):
            with pytest.raises(ValueError, match=key):
                joint.decode_ctc(*one, rnn_lm=lm50, **{key: bad})
    with pytest.raises(ValueError, match='needs rnn_lm'):
        joint.decode_ctc(*one, lm_weight=0.5)
    with pytest.raises(ValueError, match='best path'):
        joint.decode_ctc(*one, beam_size=0, rnn_lm=lm50, lm_weight=0.5)
    with pytest.raises(ValueError, match='best path'):
        joint.decode_ctc(*one, beam_size=0, length_bonus=0.5)
    with pytest.raises(RuntimeError, match='no CPU path|GPU'):
        joint.decode_ctc(*one, rnn_lm=lm50, lm_weight=0.5)
    for bad in (-0.5, math.nan, math.inf, '1', None, True):
        with pytest.raises(ValueError, match='first_lm_weight'):
            joint.decode_two_pass(one[0], one[1], lm50, one[2], 0.5, first_lm_weight=bad)
    with pytest.raises(ValueError, match='first_lm_weight 0.5 needs rnn_lm'):
        joint.decode_two_pass(one[0], one[1], None, one[2], 0.0, first_lm_weight=0.5)
    assert joint.last_ctc_decode is None and joint.last_hyps is None


def test_tester_validates_the_lm_keys_of_decode_ctc_only(tmp_path):
    from test_ctc_search_cpu import _tester
    from ss_asr_amd.trainer import ASRTester
    beam, terms = ASRTester.ctc_only_beam, ASRTester.ctc_only_lm
    off = {'lm_weight': 0.0, 'length_bonus': 0.0}
    assert terms({}) == off and terms({'decode_ctc_only': True}) == off and terms({'decode_ctc_only': {'beam_size': 0}}) == off
    conf = {'decode_ctc_only': {'beam_size': 4, 'lm_weight': 0.5, 'length_bonus': -1}}
    assert beam(conf) == 4 and terms(conf) == {'lm_weight': 0.5, 'length_bonus': -1.0}      # an int stays the return type
    for key in ('lm_weight', 'length_bonus'):
        for bad in (math.nan, math.inf, '1', None, True, [1]):
            with pytest.raises(ValueError, match=r'decode_ctc_only\.' + key):
                terms({'decode_ctc_only': {key: bad}})
        with pytest.raises(ValueError, match='best path'):
            terms({'decode_ctc_only': {'beam_size': 0, key: 0.5}})
    with pytest.raises(ValueError, match='decode_ctc_only'):
        beam({'decode_ctc_only': {'beam_size': 4, 'lm': 0.5}})
    for bad in ({'lm_weight': -0.5}, {'lm_weight': 0.5, 'length_bonus': 0.1}):
        with pytest.raises(ValueError, match='first pass'):
            terms({'decode_ctc_only': dict({'beam_size': 4}, **bad), 'decode_rescore': {'ctc_weight': 0.3}})
    assert terms({'decode_ctc_only': {'lm_weight': 0.5}, 'decode_rescore': True})['lm_weight'] == 0.5
    root = str(tmp_path)
    t = _tester(root, {}, decode_ctc_only={'beam_size': 4, 'lm_weight': 0.5})
    with pytest.raises(ValueError, match=r'asr\.decode_ctc_only.*ctc_weight'):
        t.set_model()
    t = _tester(root, {'ctc_weight': 0.3}, decode_ctc_only={'beam_size': 4, 'lm_weight': '0.5'})
    with pytest.raises(ValueError, match=r'decode_ctc_only\.lm_weight'):
        t.set_model()
