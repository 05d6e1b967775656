"""Joint CTC / attention decoding without a GPU: the CTC prefix scorer that tests/test_gpu_ctc_decode.py checks the
kernel with, pinned here by brute force and by torch's ctc_loss; the new C entries' argument checks; the Python
surface's argument checks.

The scorer (PrefixState, empty_prefix, candidate_psi, extend) is a restatement of include/ssasr.h's semantics in
numpy, float64 unless a dtype is given (float32 measures the noise the GPU test's tolerance comes from).  It shares
nothing with the library's host code."""
import ctypes
import itertools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

NEG = -math.inf
BLANK = 0


class PrefixState:
    """A prefix g: gn[t] / gb[t] = log-probability of g over frames 0..t ending in a non-blank / a blank, psi(g),
    g's last character (None: the empty prefix)."""

    def __init__(self, gn, gb, psi, last):
        self.gn, self.gb, self.psi, self.last = gn, gb, psi, last


def _lae(a, b):
    return np.logaddexp(a, b)            # -inf for two -inf


def empty_prefix(lp, blank=BLANK):
    T = lp.shape[0]
    return PrefixState(np.full(T, NEG, dtype=lp.dtype), np.cumsum(lp[:, blank], dtype=lp.dtype), lp.dtype.type(0.0), None)


def _phi(lp, st, v, either=None):
    """phi_t for t = 0 .. T-1 of st's prefix extended by v (either: logaddexp(gb, gn)[:-1] when the caller has it)."""
    T = lp.shape[0]
    phi = np.full(T, NEG, dtype=lp.dtype)
    if st.last is None:
        phi[0] = 0.0
    if v == st.last:
        phi[1:] = st.gb[:-1]
    else:
        phi[1:] = _lae(st.gb[:-1], st.gn[:-1]) if either is None else either
    return phi


def candidate_psi(lp, st, eos, blank=BLANK):
    """psi(g . v) for every v [V]: -inf for the blank, the probability of g itself for eos."""
    T, V = lp.shape
    out = np.full(V, NEG, dtype=lp.dtype)
    either = _lae(st.gb[:-1], st.gn[:-1])
    for v in range(V):
        if v == blank:
            continue
        if v == eos:
            out[v] = _lae(st.gn[T - 1], st.gb[T - 1])
            continue
        x = _phi(lp, st, v, either) + lp[:, v]
        m = x.max()
        out[v] = NEG if m == NEG else m + np.log(np.exp(x - m).sum(dtype=lp.dtype))
    return out


def extend(lp, st, v, psi, blank=BLANK):
    """The state of st's prefix extended by v (psi: its candidate_psi entry)."""
    T = lp.shape[0]
    phi = _phi(lp, st, v)
    gn, gb = np.full(T, NEG, dtype=lp.dtype), np.full(T, NEG, dtype=lp.dtype)
    n_prev = b_prev = lp.dtype.type(NEG)
    for t in range(T):
        gn[t] = _lae(n_prev, phi[t]) + lp[t, v]
        gb[t] = _lae(b_prev, n_prev) + lp[t, blank]
        n_prev, b_prev = gn[t], gb[t]
    return PrefixState(gn, gb, psi, v)


def prefix_chain(lp, text, eos=-1):
    """The states of text's prefixes, from the empty one on."""
    states = [empty_prefix(lp)]
    for v in text:
        states.append(extend(lp, states[-1], v, candidate_psi(lp, states[-1], eos)[v]))
    return states


def random_lp(T, V, seed):
    rng = np.random.default_rng(seed)
    z = 2.0 * rng.standard_normal((T, V))
    return z - np.log(np.exp(z).sum(1, keepdims=True))


def collapse(path):
    out, prev = [], None
    for c in path:
        if c != prev and c != BLANK:
            out.append(c)
        prev = c
    return tuple(out)


@pytest.mark.parametrize('T', [1, 2, 3, 4])
def test_prefix_scores_equal_the_sum_over_all_frame_labellings(T):
    V = 3
    lp = random_lp(T, V, 10 + T)
    starts, exact = {}, {}
    for path in itertools.product(range(V), repeat=T):
        pr = math.exp(sum(lp[t, c] for t, c in enumerate(path)))
        text = collapse(path)
        exact[text] = exact.get(text, 0.0) + pr
        for n in range(len(text) + 1):
            starts[text[:n]] = starts.get(text[:n], 0.0) + pr
    # every prefix of up to T + 1 characters: repeated characters ((1, 1), (2, 2, 1), ...) and ones longer than T
    checked = impossible = 0
    for n in range(1, T + 2):
        for h in itertools.product((1, 2), repeat=n):
            st = prefix_chain(lp, h[:-1])[-1]
            if st.psi == NEG:
                assert h[:-1] not in starts
                continue
            psi = candidate_psi(lp, st, eos=-1)
            assert psi[BLANK] == NEG
            if h in starts:
                assert abs(psi[h[-1]] - math.log(starts[h])) <= 1e-12, (T, h)
                checked += 1
            else:
                assert psi[h[-1]] == NEG, (T, h)
                impossible += 1
            # with v as the end marker: the probability of the prefix itself
            end = candidate_psi(lp, st, eos=h[-1])[h[-1]]
            g = h[:-1]
            assert abs(end - math.log(exact[g])) <= 1e-12 if g in exact else end == NEG
    assert abs(sum(exact.values()) - 1.0) <= 1e-12 and starts[()] == pytest.approx(1.0, abs=1e-12)
    assert checked >= 2 and impossible >= 1
    assert (1, 1) not in starts or T >= 3                    # a repeat needs a blank between: three frames


def test_the_lattice_ends_at_torch_ctc_loss():
    T, V = 6, 5
    lp = random_lp(T, V, 3)
    for text in ((1,), (2, 2), (1, 2, 3), (4, 4, 4), (3, 1, 1, 2), ()):
        st = prefix_chain(lp, text)[-1]
        mine = float(_lae(st.gn[T - 1], st.gb[T - 1]))
        want = -float(F.ctc_loss(torch.from_numpy(lp).unsqueeze(1), torch.tensor([list(text)], dtype=torch.long),
                                 torch.tensor([T]), torch.tensor([len(text)]), blank=BLANK, reduction='sum',
                                 zero_infinity=False))
        assert abs(mine - want) <= 1e-12, (text, mine, want)
    # (2, 2, 2, 2) needs seven frames
    st = prefix_chain(lp, (2, 2, 2, 2))[-1]
    assert st.psi == NEG and _lae(st.gn[T - 1], st.gb[T - 1]) == NEG


def test_float32_scorer_follows_the_float64_one():
    lp = random_lp(20, 50, 5)
    a, b = prefix_chain(lp, (3, 3, 7, 9))[-1], prefix_chain(lp.astype(np.float32), (3, 3, 7, 9))[-1]
    assert b.gn.dtype == np.float32 and abs(float(a.psi) - float(b.psi)) <= 1e-4 * abs(float(a.psi))


def test_the_new_entries_are_bound_and_refuse_bad_arguments_without_a_gpu():
    from ss_asr_amd import _lib
    lib = _lib.load()
    assert {'ssasr_decode_beam_ctc', 'ssasr_decode_beam_ctc_ws_bytes'} <= set(_lib.SIGNATURES)
    assert [f[0] for f in _lib.CtcPrefix._fields_] == ['w_ctc', 'b_ctc', 'ctc_weight', 'blank']
    assert ctypes.sizeof(_lib.CtcPrefix) == 24
    assert lib.ssasr_decode_beam_ctc(None, None, None) < 0
    d, c = _lib.Beam(), _lib.CtcPrefix()
    assert lib.ssasr_decode_beam_ctc(ctypes.byref(d), None, None) < 0
    assert lib.ssasr_decode_beam_ctc(None, ctypes.byref(c), None) < 0
    assert lib.ssasr_decode_beam_ctc(ctypes.byref(d), ctypes.byref(c), None) < 0          # all sizes zero
    sizes = (100, 512, 128, 256, 50, 128, 200)                                              # T E A D V Hl S
    for N, K in ((32, 8), (1, 1), (3, 32)):
        plain, ctc = lib.ssasr_decode_beam_ws_bytes(N, K, *sizes), lib.ssasr_decode_beam_ctc_ws_bytes(N, K, *sizes)
        # behind the plain slice: lp [T][64] floats, gamma 2 x K x 2 x T doubles, psi 2 x K doubles
        assert plain > 0 and ctc == plain + N * (4 * 64 * 100 + 8 * 4 * K * 100 + 8 * 2 * K) and ctc % 16 == 0
    for N, K in ((0, 8), (32, 0), (32, 33)):
        assert lib.ssasr_decode_beam_ctc_ws_bytes(N, K, *sizes) == 0
    assert lib.ssasr_decode_beam_ctc_ws_bytes(1, 8, 16385, 512, 128, 256, 50, 128, 200) == 0
    assert lib.ssasr_decode_beam_ctc_ws_bytes(1, 8, 100, 512, 128, 256, 65, 128, 200) == 0
    assert lib.ssasr_decode_beam_ctc_ws_bytes(1, 32, 16384, 512, 128, 256, 50, 128, 200) > 2 ** 24


class _Mapper:
    def char_to_ind(self, c):
        return 1

    def ind_to_char(self, i):
        return '?'


def test_the_python_surface_checks_ctc_weight_before_anything_runs():
    from ss_asr_amd.asr import ASR
    from ss_asr_amd.ctc import JointCTCASR
    x = torch.zeros(1, 16, 12)
    plain, joint = ASR(50, 32, 32, 16, 12, 1.0), JointCTCASR(50, 32, 32, 16, 12, 1.0)
    for model in (plain, joint):
        for w in (-0.1, 1.5, float('nan')):
            with pytest.raises(ValueError, match='ctc_weight'):
                model.decode(x, [16], None, _Mapper(), 0.0, ctc_weight=w)
            with pytest.raises(ValueError, match='ctc_weight'):
                model.decode_many([x], [[16]], None, _Mapper(), 0.0, beam_size=3, ctc_weight=w)
            with pytest.raises(ValueError, match='ctc_weight'):
                model.decode_nbest([x], [[16]], None, _Mapper(), 0.0, 3, ctc_weight=w)
    for w in (0.3, 1.0):
        with pytest.raises(ValueError, match='ctc_head'):
            plain.decode(x, [16], None, _Mapper(), 0.0, ctc_weight=w)
        with pytest.raises(ValueError, match='ctc_head'):
            plain.decode_nbest([x], [[16]], None, _Mapper(), 0.0, 3, ctc_weight=w)
    # a weight inside the range on a model with a head gets as far as the device check
    with pytest.raises(RuntimeError, match='no CPU path'):
        joint.decode(x, [16], None, _Mapper(), 0.0, ctc_weight=0.3)
