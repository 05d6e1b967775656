"""Every GEMM kernel family (csrc/gemm.hip) against float64 at small shapes with edge tiles in every axis: the fp32
tile kernels, the split-bf16 tile kernels (64 x 64 and 128 x 128 each) and the wide 256 x 128 kernel, with a bias and
each activation, alpha / beta, the pair power (act 3), split-K parts added atomically, an unaligned C with an odd row
stride, and a C whose rows take 16-byte stores.  The four-columns-per-lane store exists twice (epi_store_quad and the
wide kernel's staged epilogue): a fix to one has to show up, or be missed, here for each family.  Needs an MI355X."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'

# family -> switches.  'wide-direct' is the wide kernel's store-mode epilogue without its LDS staging (SSASR_GEMM_EPI=1):
# the only way into the four-columns-per-lane loop of gemm_epilogue32.
FAMILIES = {
    'fp32-64': {'SSASR_GEMM_X6': 0, 'SSASR_GEMM_TILE': 64},
    'fp32-128': {'SSASR_GEMM_X6': 0, 'SSASR_GEMM_TILE': 128},
    'x6-64': {'SSASR_GEMM_X6': 1, 'SSASR_GEMM_TILE': 64},
    'x6-128': {'SSASR_GEMM_X6': 1, 'SSASR_GEMM_TILE': 128},
    'wide': {'SSASR_GEMM_X6': 1, 'SSASR_GEMM_TILE': 256},
    'wide-direct': {'SSASR_GEMM_X6': 1, 'SSASR_GEMM_TILE': 256, 'SSASR_GEMM_EPI': 1},
}
# Tile kernels: edge tiles in both axes, a last column quad with two valid columns, a partial K step.
TILE_SHAPES = [(ta, tb, 150, 138, 72) for ta in (0, 1) for tb in (0, 1)]
# Wide kernel (16-byte loads and whole K steps only): interior wave tiles (straight-line stores when C's rows allow
# 16-byte stores), edge tiles for the general loop, a scalar tail; with both operands MN-contiguous M and N must be multiples of 4.
WIDE_SHAPES = [(0, 0, 300, 138, 96), (1, 1, 300, 140, 96)]
CASES = [(f,) + s for f in FAMILIES for s in (WIDE_SHAPES if f.startswith('wide') else TILE_SHAPES)]
# A freshly allocated C has rows of N floats: with N = 138 they do not start on 16-byte boundaries, so those modes take
# the one-float stores everywhere.  The two 'vec_out' modes write into a view whose rows are a multiple of four floats
# apart: 16-byte stores (plain: the wide kernel's straight-line path on interior wave tiles; act_beta: with the
# activation and the read of C), and the scalar tail only in the last, partial column quad.
MODES = ['act0', 'act1', 'act2', 'act4', 'act5', 'act6', 'alpha_beta', 'pair_power', 'splitk2', 'unaligned_out',
         'vec_out_plain', 'vec_out_act_beta']


def close(got, want, atol, what=''):
    got = got.detach().double().cpu()
    want = want.detach().double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = (got - want).abs().max().item()
    tol = atol * max(1.0, want.abs().max().item())     # absolute for O(1) data, relative above
    assert err <= tol, '%s: max abs err %.3e > %.1e' % (what, err, tol)


def rnd(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64).float()


@functools.lru_cache(maxsize=None)
def operands(ta, tb, M, N, K, nonneg):
    """Seeded fp32 operands on the device and their float64 product (computed once per shape, never modified)."""
    a = rnd(*((K, M) if ta else (M, K)), seed=101)
    b = rnd(*((K, N) if tb else (N, K)), seed=102)
    if nonneg:
        a, b = a.abs(), b.abs()
    prod = (a.double().t() if ta else a.double()) @ (b.double() if tb else b.double().t())
    return a.to(DEV), b.to(DEV), prod


def reference_act(code, v):
    return {0: lambda x: x, 1: torch.tanh, 2: lambda x: torch.log(x.clamp(min=0) + 2.220446049250313e-16),
            4: torch.relu, 5: lambda x: torch.where(x > 0, x, 0.01 * x), 6: torch.sigmoid}[code](v)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('family,ta,tb,M,N,K', CASES)
def test_gemm_family_epilogue_against_float64(family, ta, tb, M, N, K, mode):
    from ss_asr_amd import _lib, ops
    lib = _lib.load()
    tol = 2e-4 * max(1.0, K ** 0.5 / 4)
    what = '%s %d%d %dx%dx%d %s' % (family, ta, tb, M, N, K, mode)
    switches = dict({'SSASR_GEMM_WIDE': 1, 'SSASR_GEMM_BF16': 0, 'SSASR_GEMM_EPI': 0}, **FAMILIES[family])
    old = {k: _lib.set_option(k, v) for k, v in switches.items()}
    try:
        # the launcher really takes this family for this shape (a wide case that is not eligible would run the tile kernels)
        splitk = 2 if mode == 'splitk2' else 1
        assert lib.ssasr_gemm_tile_choice(ta, tb, M, N, K, 1, splitk, 1, 1) == switches['SSASR_GEMM_TILE'], what
        a, b, prod = operands(ta, tb, M, N, K, mode == 'act2')
        kw = dict(ta=bool(ta), tb=bool(tb))
        if mode.startswith('act'):
            code = int(mode[3:])
            # act 2 is log(x + eps): non-negative operands and a bias of 1 keep every pre-activation >= 1, where the
            # logarithm does not amplify the product's error
            bias = torch.ones(N) if code == 2 else rnd(N, seed=103)
            got = ops.gemm(a, b, bias=bias.to(DEV), act=code, **kw)
            close(got, reference_act(code, prod + bias.double()), tol, what)
        elif mode == 'alpha_beta':
            c0 = rnd(M, N, seed=104)
            got = ops.gemm(a, b, out=c0.to(DEV), alpha=0.5, beta=2.0, **kw)
            close(got, 0.5 * prod + 2.0 * c0.double(), tol, what)
        elif mode == 'pair_power':
            got = ops.gemm(a, b, act=3, **kw)
            close(got[:, :N // 2], prod[:, 0::2] ** 2 + prod[:, 1::2] ** 2, tol, what)
        elif mode == 'splitk2':
            got = ops.gemm(a, b, out=torch.zeros(M, N, device=DEV), splitk=2, **kw)
            close(got, prod, tol, what)
        elif mode.startswith('vec_out'):
            ld = N + ((-N) % 4 or 4)
            c0 = rnd(M, ld, seed=105)
            buf = c0.to(DEV)
            bias = rnd(N, seed=103)
            if mode == 'vec_out_plain':
                ops.gemm(a, b, out=buf[:, :N], bias=bias.to(DEV), **kw)
                want = prod + bias.double()
            else:
                ops.gemm(a, b, out=buf[:, :N], bias=bias.to(DEV), act=1, alpha=0.5, beta=2.0, **kw)
                want = torch.tanh(0.5 * prod + bias.double()) + 2.0 * c0[:, :N].double()
            close(buf[:, :N], want, tol, what)
            assert torch.equal(buf[:, N:].cpu(), c0[:, N:]), what
        else:
            # C starts 4 bytes past a 16-byte boundary and its rows are an odd number of floats apart: no 16-byte stores
            buf = torch.full((M, N + 3), 7.0, device=DEV)
            ops.gemm(a, b, out=buf[:, 1:1 + N], **kw)
            close(buf[:, 1:1 + N], prod, tol, what)
            assert bool((buf[:, 0] == 7.0).all()) and bool((buf[:, 1 + N:] == 7.0).all()), what
    finally:
        for k, v in old.items():
            _lib.set_option(k, v)
