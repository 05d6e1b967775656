"""The encoder BiLSTM's launch forms that the default switches never pick on a healthy MI355X at the shapes the rest of
the suite uses (csrc/rnn.hip; DESIGN.md 4.2 has the table): the per-step kernels at the persistent widths, the row-major
save path of the persistent forward and the K-split BPTT, the K-split BPTT without halves at H >= 128, sequences of one
to four steps, and H = 512.  Every case runs forward and backward through ops.bilstm, asserts through
ssasr_bilstm_forms -- answered by the launches' own decision functions -- that the form it is about is the one that
runs, and compares y, dx and the eight parameter gradients with oracle/las_oracle.py in float64.  Only switches that
select a more conservative form are set.  Needs an MI355X."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import las_oracle as lo

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
TOL_Y, TOL_DX, TOL_DW, TOL_DW_FLAT = 2e-5, 5e-5, 2e-4, 3e-4      # the suite's BiLSTM bounds (test_gpu_kernels.py)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale)


def close(got, want, atol, what=''):
    got = got.detach().double().cpu()
    want = want.detach().double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = (got - want).abs().max().item()
    tol = atol * max(1.0, want.abs().max().item())     # absolute for O(1) data, relative above
    print('%s: max abs err %.3e (bound %.1e)' % (what, err, tol))
    assert err <= tol, '%s: max abs err %.3e > %.1e' % (what, err, tol)


def lstm_weights(I, H, seed):
    w = []
    for d in range(2):
        w += [rnd(4 * H, I, seed=seed + 10 * d, scale=I ** -0.5),
              rnd(4 * H, H, seed=seed + 10 * d + 1, scale=H ** -0.5),
              rnd(4 * H, seed=seed + 10 * d + 2, scale=0.1),           # biases are not zero
              rnd(4 * H, seed=seed + 10 * d + 3, scale=0.1)]
    return w


def ragged(N, S):
    """N lengths from S down to 1."""
    return [S] if N == 1 else [S - (k * (S - 1)) // (N - 1) for k in range(N)]


NAMES = ['w_ih', 'w_hh', 'b_ih', 'b_hh'] * 2


@functools.lru_cache(maxsize=None)
def oracle_case(N, S, I, H, pad, packed=True):
    """Seeded inputs and the float64 results of one layer, computed once per shape and never modified.  packed: x is
    batch-first [N, S + pad, I] (pad > 0: an input longer than max(lens), whose frames past S are NOT zero) with lengths
    S .. 1; else sequence-major [S, N, I] without lengths."""
    lens = ragged(N, S) if packed else None
    x = rnd(N, S + pad, I, seed=11) if packed else rnd(S, N, I, seed=13)
    w = lstm_weights(I, H, 20)
    xr = x.clone().requires_grad_(True)
    wr = [t.clone().requires_grad_(True) for t in w]
    if packed:
        yr = lo.bilstm_explicit(xr[:, :S].transpose(0, 1), lens, wr).transpose(0, 1)
        gy = rnd(N, S, 2 * H, seed=12)
    else:
        yr = lo.bilstm_explicit(xr, None, wr)
        gy = rnd(S, N, 2 * H, seed=14)
    (yr * gy).sum().backward()
    return dict(S=S, packed=packed, lens=lens, x=x, w=w, gy=gy, y=yr.detach(), dx=xr.grad, dw=[t.grad for t in wr])


def run_layer(case):
    """Forward and backward of the case through ops.bilstm: (y, dx, [dw]) after a synchronize and a status check."""
    from ss_asr_amd import ops
    xd = case['x'].float().to(DEV).requires_grad_(True)
    wd = [t.float().to(DEV).requires_grad_(True) for t in case['w']]
    ld = torch.tensor(case['lens'], dtype=torch.int32, device=DEV) if case['lens'] is not None else None
    yd = ops.bilstm(xd, ld, case['S'], case['packed'], wd)
    (yd * case['gy'].float().to(DEV)).sum().backward()
    torch.cuda.synchronize()
    ops.check_persistent_status()
    return yd, xd.grad, [t.grad for t in wd]


def compare(case, got, what, tol=(TOL_Y, TOL_DX, TOL_DW)):
    y, dx, dw = got
    close(y, case['y'], tol[0], what + ' y')
    close(dx, case['dx'], tol[1], what + ' dx')
    for name, a, b in zip(NAMES, dw, case['dw']):
        close(a, b, tol[2], what + ' d' + name)


def forms(S, N, I, H, window=0):
    """(fwd, bwd) of ssasr_bilstm_forms (include/ssasr.h): fwd 0 | 100 + c | 200 + c, bwd 0 | 1 | 2."""
    from ss_asr_amd import _lib
    fwd, bwd = ctypes.c_int(-1), ctypes.c_int(-1)
    assert _lib.load().ssasr_bilstm_forms(S, N, I, H, window, ctypes.byref(fwd), ctypes.byref(bwd)) == 0
    return fwd.value, bwd.value


def tsave_floats(S, N, H):
    from ss_asr_amd import _lib
    return int(_lib.load().ssasr_bilstm_tsave_floats(S, N, H))


def ring_floats(S, N, H):
    from ss_asr_amd import _lib
    return int(_lib.load().ssasr_bilstm_bwd_ring_floats(S, N, H, 2))


class switches:
    """Sets library switches for a block and puts the old values back."""

    def __init__(self, **values):
        self.values = values

    def __enter__(self):
        from ss_asr_amd import _lib
        self.old = []
        try:
            for name, v in self.values.items():
                self.old.append((name, _lib.set_option(name, v)))
        except BaseException:
            self.__exit__()
            raise
        return self

    def __exit__(self, *exc):
        from ss_asr_amd import _lib
        for name, v in reversed(self.old):
            _lib.set_option(name, v)
        return False


@functools.lru_cache(maxsize=None)
def segmented_oracle(N, S, I, H):
    """Inputs and float64 results of the train-step case of test_gpu_kernels.py (_segmented_bptt_case)."""
    lens = sorted(np.random.default_rng(3).integers(S // 3, S + 1, size=N).tolist(), reverse=True)
    lens[0] = S
    x = rnd(N, S, I, seed=51)
    for i, l in enumerate(lens):
        x[i, l:] = 0
    w = lstm_weights(I, H, 60)
    xr = x.clone().requires_grad_(True)
    wr = [t.clone().requires_grad_(True) for t in w]
    yr = lo.bilstm_explicit(xr.transpose(0, 1), lens, wr).transpose(0, 1)
    gy = rnd(N, S, 2 * H, seed=52)
    (yr * gy).sum().backward()
    return dict(S=S, packed=True, lens=lens, x=x, w=w, gy=gy, y=yr.detach(), dx=xr.grad, dw=[t.grad for t in wr])


def segmented_bptt_case(N, S, I, H, segments, monkeypatch):
    """The path the train step takes: gradients in an optimizer-owned flat buffer, so the BPTT runs in `segments` step
    ranges and the weight gradients are ACCUMULATED into the buffer from a second stream, range by range."""
    from ss_asr_amd import ops
    from ss_asr_amd.optim import FlatParameters
    monkeypatch.setattr(ops, 'bptt_segments', segments)
    case = segmented_oracle(N, S, I, H)

    class Holder(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.ps = torch.nn.ParameterList([torch.nn.Parameter(t.float().to(DEV)) for t in case['w']])
    holder = Holder()
    flat = FlatParameters(holder)
    flat.grad.fill_(0.25)                                   # gradients are ACCUMULATED into the buffer
    xd = case['x'].float().to(DEV).requires_grad_(True)
    ld = torch.tensor(case['lens'], dtype=torch.int32, device=DEV)
    yd = ops.bilstm(xd, ld, S, True, list(holder.ps))
    (yd * case['gy'].float().to(DEV)).sum().backward()
    ops.join_side_stream()
    torch.cuda.synchronize()
    ops.check_persistent_status()
    close(yd, case['y'], TOL_Y, 'y')
    close(xd.grad, case['dx'], TOL_DX, 'dx')
    for name, a, b in zip(NAMES, holder.ps, case['dw']):
        close(a.grad - 0.25, b, TOL_DW_FLAT, 'd' + name)


# ------------------------------------------------------------------------------------------------------------------
# A. the per-step kernels (lstm_enc_fwd_kernel / lstm_enc_bwd_kernel) at the widths the persistent kernels take
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,S,I,H,pad,packed', [
    (17, 9, 24, 64, 2, True),            # an input longer than max(lens)
    (33, 7, 48, 128, 0, True),           # a third 16-column BPTT chunk / second 32-column forward chunk with one live column
    (13, 6, 80, 256, 0, True),           # fused input projection by default: here the GEMM feeds the per-step kernel
    (35, 5, 32, 256, 0, False),          # sequence-major, no lengths
])
def test_per_step_kernels_at_persistent_widths(N, S, I, H, pad, packed):
    """SSASR_NO_PERSISTENT=1: what runs when a residency check says no."""
    assert forms(S, N, I, H)[0] >= 100                      # by default the shape is a persistent one
    case = oracle_case(N, S, I, H, pad, packed)
    with switches(SSASR_NO_PERSISTENT=1):
        assert forms(S, N, I, H) == (0, 0)
        assert tsave_floats(S, N, H) == 0 and ring_floats(S, N, H) == 0
        got = run_layer(case)
    compare(case, got, 'per-step N=%d H=%d' % (N, H))


# ------------------------------------------------------------------------------------------------------------------
# B. no column windows: the per-step kernels over more than 128 columns at a persistent width
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('packed', [False, True])
def test_per_step_kernels_over_more_than_one_window(packed):
    N, S, I, H = 130, 6, 16, 64
    narrow = forms(S, 128, I, H)
    assert narrow[0] >= 100 and narrow[1] >= 1
    assert forms(S, N, I, H, 1)[0] >= 100                   # by default: two windows, both persistent
    case = oracle_case(N, S, I, H, 1 if packed else 0, packed)      # packed: an input longer than max(lens)
    with switches(SSASR_NO_WINDOWS=1):
        assert forms(S, N, I, H, 0) == (0, 0) and forms(S, N, I, H, 1) == (0, 0)
        assert forms(S, 128, I, H) == narrow                # one window's worth of columns is not affected
        assert tsave_floats(S, N, H) == 0 and ring_floats(S, N, H) == 0
        got = run_layer(case)
    compare(case, got, 'no windows, %s' % ('packed' if packed else 'sequence-major'))


# ------------------------------------------------------------------------------------------------------------------
# C. row-major saves: the persistent forward writes gates / cs in place, the K-split BPTT reads them (tsave null)
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,S,I,H,pad,fwd', [
    (17, 9, 24, 64, 2, 116),             # an input longer than max(lens)
    (20, 8, 16, 128, 0, 116),
    (33, 7, 24, 256, 0, 132),            # 32-column workgroups, last chunk with one live column
    (130, 6, 16, 64, 0, 116),            # two windows, with lengths
    (13, 6, 80, 256, 0, 216),            # fused input
])
def test_row_major_saves(N, S, I, H, pad, fwd):
    """SSASR_NO_TSAVE=1: what a C-ABI caller that passes no tsave gets."""
    assert tsave_floats(S, N, H) > 0                        # by default the shape saves tile-major
    case = oracle_case(N, S, I, H, pad)
    with switches(SSASR_NO_TSAVE=1):
        assert tsave_floats(S, N, H) == 0
        for w in range((N + 127) // 128):
            got_fwd, got_bwd = forms(S, N, I, H, w)
            assert got_fwd // 100 == fwd // 100 and got_bwd >= 1, (w, got_fwd, got_bwd)
        assert forms(S, N, I, H)[0] == fwd
        got = run_layer(case)
    compare(case, got, 'row-major saves N=%d H=%d' % (N, H))


@pytest.mark.parametrize('one_launch', [1, 0])
def test_row_major_saves_segmented(one_launch, monkeypatch):
    """The train-step path on row-major saves: the layer's step ranges in one launch (progress words), and as one launch
    per range (SSASR_BPTT_ONE_LAUNCH=0), which carries dc_state and the ring across launches.  That switch is the
    conservative side too: per-range launches are what a device without stream-wait-value, or a layer of several column
    windows, takes by itself, and test_gpu_kernels.py::test_bilstm_segmented_bptt_launch_forms already runs them at this
    shape on tile-major saves; it touches neither residency nor pacing."""
    N, S, I, H = 17, 64, 24, 64
    with switches(SSASR_NO_TSAVE=1, SSASR_BPTT_ONE_LAUNCH=one_launch):
        assert tsave_floats(S, N, H) == 0
        assert forms(S, N, I, H) == (116, 1)
        segmented_bptt_case(N, S, I, H, 2, monkeypatch)


# ------------------------------------------------------------------------------------------------------------------
# D. the K-split BPTT without halves at H >= 128 (lstm_enc_bwd_rs_kernel<2, 1> / <4, 1>) for launches of >= 3 steps
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('halves_off', [1, 0])
@pytest.mark.parametrize('N,S,I,H', [(9, 8, 16, 128), (16, 4, 16, 128), (20, 6, 24, 256)])     # 16 columns at H = 128: live columns 12 .. 15 of a chunk
def test_ksplit_bptt_without_halves(N, S, I, H, halves_off):
    case = oracle_case(N, S, I, H, 1 if N == 9 else 0)              # N = 9: an input longer than max(lens)
    with switches(SSASR_BPTT_HALVES_OFF=halves_off):
        assert forms(S, N, I, H) == (116, 1 if halves_off else 2)
        assert tsave_floats(S, N, H) > 0
        got = run_layer(case)
    compare(case, got, 'K-split %s halves N=%d H=%d' % ('without' if halves_off else 'with', N, H))


@pytest.mark.parametrize('halves_off', [1, 0])
def test_ksplit_bptt_without_halves_segmented(halves_off, monkeypatch):
    N, S, I, H = 17, 64, 24, 128
    with switches(SSASR_BPTT_HALVES_OFF=halves_off):
        assert forms(S, N, I, H) == (116, 1 if halves_off else 2)
        segmented_bptt_case(N, S, I, H, 2, monkeypatch)


# ------------------------------------------------------------------------------------------------------------------
# E. one to four steps through the default forms: S = 1 has no recurrent weight-gradient product, S <= 2 no halves
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S', [1, 2, 3, 4])
@pytest.mark.parametrize('N,H', [(17, 128), (20, 256)])
def test_short_sequences_default_forms(N, H, S):
    I = 24
    fwd, bwd = forms(S, N, I, H)
    assert fwd == 116 and bwd == (2 if S >= 3 else 1), (fwd, bwd)      # a launch of fewer than three steps has no halves
    assert tsave_floats(S, N, H) > 0
    case = oracle_case(N, S, I, H, 1 if S == 2 else 0)
    got = run_layer(case)
    compare(case, got, 'S=%d N=%d H=%d' % (S, N, H))
    if S == 1:
        for k in (1, 5):                                     # no step has a predecessor: dw_hh is exactly zero
            assert not case['dw'][k].any() and not got[2][k].any()


# ------------------------------------------------------------------------------------------------------------------
# F. H = 512: lstm_enc_fwd_persistent_kernel<8, 1> / <8, 2> writing row-major saves for the per-step BPTT
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,packed,fwd', [
    (1, True, 116), (16, True, 116),     # <8, 1>, 256 workgroups
    (17, True, 132), (32, True, 132),    # <8, 2>, 256 workgroups
    (32, False, 132),                    # sequence-major, no lengths
    (40, True, None),                    # <8, 2>, 512 workgroups: persistent if they are all resident, else per-step
    (70, True, 0),                       # three chunks = 768 workgroups: per-step
])
def test_h512(N, packed, fwd):
    S, I, H = 6, 32, 512
    got_fwd, got_bwd = forms(S, N, I, H)
    print('H = 512, N = %d: forward form %d, BPTT form %d' % (N, got_fwd, got_bwd))
    if fwd is None:
        assert got_fwd in (0, 132)
    else:
        assert got_fwd == fwd
    assert got_bwd == 0 and tsave_floats(S, N, H) == 0 and ring_floats(S, N, H) == 0
    case = oracle_case(N, S, I, H, 2 if N == 17 else 0, packed)
    got = run_layer(case)
    compare(case, got, 'H=512 N=%d' % N)


# ------------------------------------------------------------------------------------------------------------------
def test_forms_query_agrees_with_the_workspace_queries_at_default_switches():
    """At the shapes of test_gpu_kernels.py::test_bilstm_packed_forward_backward (N, S = max(lens), I, H): the K-split
    ring exists exactly where the query says K-split, tile-major saves exactly where it says both persistent forms."""
    shapes = [(4, 12, 12, 32), (5, 7, 20, 16), (33, 6, 8, 16), (3, 10, 80, 256), (48, 40, 64, 256), (64, 24, 64, 256),
              (32, 37, 64, 256), (29, 21, 48, 256), (13, 26, 80, 256), (150, 40, 80, 256), (130, 36, 48, 64)]
    for N, S, I, H in shapes:
        for w in range((N + 127) // 128):
            fwd, bwd = forms(S, N, I, H, w)
            assert (ring_floats(S, N, H) > 0) == (bwd >= 1), (N, S, I, H, w)
            assert (tsave_floats(S, N, H) > 0) == (fwd >= 100 and bwd >= 1), (N, S, I, H, w)
            assert (fwd >= 200) == (I == 80 and H == 256), (N, S, I, H, w)
    assert forms(10, 3, 80, 256) == (216, 2) and forms(12, 4, 12, 32) == (0, 0)
    # three and four 16-column chunks at H = 256: 16 x 2 x 3 x 2 = 192 and 16 x 2 x 4 x 2 = 256 workgroups, both with halves
    assert forms(40, 48, 64, 256) == (132, 2) and forms(24, 64, 64, 256) == (132, 2)
    assert forms(40, 150, 80, 256, 0) == (232, 1) and forms(40, 150, 80, 256, 1) == (216, 2)
    fwd, bwd = ctypes.c_int(), ctypes.c_int()
    from ss_asr_amd import _lib
    assert _lib.load().ssasr_bilstm_forms(40, 150, 80, 256, 2, ctypes.byref(fwd), ctypes.byref(bwd)) < 0      # no such window
