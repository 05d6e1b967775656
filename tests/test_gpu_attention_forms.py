"""Every launch form of the attention step (csrc/decoder.hip, launch_attn_fwd / launch_attn_bwd) at its shape
limits against the float64 oracle (oracle/las_oracle.py, attention_step_explicit, itself pinned in
tests/test_oracle.py).  One ssasr_attn_step_fwd call ends in one of eight kernels:

    fast<1>            A = 128, E = 128 nch, T <= 128, no workspace
    fast<2>            the same, 128 < T <= 256
    long               the same, T > 256
    split<2|3|4|6>     A = 128, E = 512, 128 < T <= 1024 with the workspace (rows per half-wave: attn_split_rph)
    general            any other A or E
and attn_step_bwd_kernel does every backward pass.  A case can never quietly test another form: a case routed
through ops.attn_step asserts what ssasr_attn_step_ws_floats says for its shape (0 for the forms without a
workspace, the record count of the forced slice size for the split forms), and the forms that ops would route to
the split kernel (E = 512, T > 128) are called through the C ABI with ws = NULL.

Every case checks alpha, ctx and the gradients of feat, state, w_phi, w_psi and b_psi with the tolerances of
test_attention_step_forward_backward (test_gpu_kernels.py).  Needs an MI355X."""
import ctypes as C
import functools

import pytest
import torch

import las_oracle as lo

pytestmark = pytest.mark.gpu

D = 64
TOL_ALPHA, TOL_CTX, TOL_GRAD = 2e-6, 1e-5, 1e-4
ATTN_PART = 512 + 32          # floats per split-T record (csrc/attn_kernels.h)
NAMES = ['feat', 'state', 'w_phi', 'w_psi', 'b_psi']


def dev():
    return torch.device('cuda:0')


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale)


def close(got, want, atol, what=''):
    got = got.detach().double().cpu()
    want = want.detach().double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = (got - want).abs().max().item()
    tol = atol * max(1.0, want.abs().max().item())     # absolute for O(1) data, relative above
    print('%-24s max abs err %.3e (allowed %.1e)' % (what, err, tol))
    assert err <= tol, '%s: max abs err %.3e > %.1e' % (what, err, tol)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ws_floats(B, T, A, E):
    from ss_asr_amd import _lib
    return int(_lib.load().ssasr_attn_step_ws_floats(B, T, A, E))


def edge_lens(T, edge):
    """A full-length utterance, T - 1, a length exactly on a row-group / slice boundary and 1 (duplicates of
    tiny T dropped, but at least three utterances)."""
    out = []
    for l in (T, T - 1, edge, 1):
        if 1 <= l <= T and l not in out:
            out.append(l)
    while len(out) < 3:
        out.append(out[-1])
    return out


@functools.lru_cache(maxsize=3)
def reference(B, T, A, E, lens, use_datt=True, use_dctx=True):
    """Seeded float64 inputs and the oracle's alpha, ctx and gradients for them (shared by the cases of one
    shape: the four split sizes, both calls on one workspace).  `lens` None or a tuple, entries above T allowed.
    W_phi is scaled so that |e| ~ 10 at every A (e = comp . q sums A terms): the premise of the alpha tolerance."""
    feat, state = rnd(B, T, E, seed=21), rnd(B, D, seed=22)
    w_phi = rnd(A, D, seed=23, scale=D ** -0.5 * min(1.0, (128.0 / A) ** 0.5))
    w_psi, b_psi = rnd(A, E, seed=24, scale=E ** -0.5), rnd(A, seed=25, scale=0.1)
    ga, gc = rnd(B, T, seed=26), rnd(B, E, seed=27)
    inputs = (feat, state, w_phi, w_psi, b_psi)
    leaves = [t.clone().requires_grad_(True) for t in inputs]
    f, s, wp, ws, bs = leaves
    comp = torch.tanh(f @ ws.t() + bs)
    clamped = None if lens is None else [min(l, T) for l in lens]       # the kernels clamp enc_len to T
    alpha, ctx = lo.attention_step_explicit(s, f, comp, clamped, wp)
    loss = 0.0
    if use_datt:
        loss = loss + (alpha * ga).sum()
    if use_dctx:
        loss = loss + (ctx * gc).sum()
    loss.backward()
    return inputs, ga, gc, alpha.detach(), ctx.detach(), [t.grad for t in leaves]


class _DirectStep(torch.autograd.Function):
    """ssasr_attn_step_fwd / _bwd through the C ABI with ws = NULL (ops.attn_step always passes the workspace when
    the library offers one): the form then follows from the shape alone.  q comes from the same call (`state`
    given).  A missing output gradient reaches the library as it is: datt = NULL is the kernel's own path,
    dctx is mandatory in the C ABI and becomes zeros, as in ops."""

    @staticmethod
    def forward(ctx, state, w_phi, comp, feat, enc_len):
        from ss_asr_amd import _lib
        lib = _lib.load()
        B, T, E = feat.shape
        A, Dd = w_phi.shape
        q = torch.empty(B, A, device=feat.device)
        att = torch.empty(B, T, device=feat.device)
        cx = torch.empty(B, E, device=feat.device)
        _lib.check(lib.ssasr_attn_step_fwd(_p(state), _p(w_phi), _p(comp), _p(feat), _p(enc_len), B, T, A, E, Dd,
                                           _p(q), _p(att), _p(cx), None, 0, None, _stream()), 'ssasr_attn_step_fwd')
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(state, w_phi, comp, feat, enc_len, q, att)
        return att, cx

    @staticmethod
    def backward(ctx, datt, dctx):
        from ss_asr_amd import _lib, ops
        lib = _lib.load()
        state, w_phi, comp, feat, enc_len, q, att = ctx.saved_tensors
        B, T, E = feat.shape
        A = w_phi.shape[0]
        dctx = dctx.contiguous() if dctx is not None else torch.zeros(B, E, device=feat.device)
        datt = datt.contiguous() if datt is not None else None
        de = torch.empty(B, T, device=feat.device)
        dqpre = torch.empty(B, A, device=feat.device)
        _lib.check(lib.ssasr_attn_step_bwd(_p(dctx), _p(datt), _p(att), _p(q), _p(comp), _p(feat), _p(enc_len),
                                           B, T, A, E, _p(de), _p(dqpre), _stream()), 'ssasr_attn_step_bwd')
        dstate = ops.gemm(dqpre, w_phi, tb=True)
        dw_phi = ops.gemm(dqpre, state, ta=True, tb=True)
        dcomp = ops.gemm(de.unsqueeze(1), q.unsqueeze(1), ta=True, tb=True)
        dfeat = ops.gemm(att.unsqueeze(1), dctx.unsqueeze(1), ta=True, tb=True)
        return dstate, dw_phi, dcomp, dfeat, None


def run_case(B, T, A, E, lens, direct=False, calls=1, use_datt=True, use_dctx=True):
    """Forward (`calls` times, each against the reference) and backward of one shape on the device."""
    from ss_asr_amd import ops
    lens = None if lens is None else tuple(lens)
    assert B == (len(lens) if lens is not None else B)
    inputs, ga, gc, alpha, ctx, grads = reference(B, T, A, E, lens, use_datt, use_dctx)
    dl = [t.float().to(dev()).requires_grad_(True) for t in inputs]
    fd, sd, wpd, wsd, bsd = dl
    compd = ops.attn_precompute(fd, wsd, bsd)
    ld = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=dev())
    for k in range(calls):
        ad, cd = _DirectStep.apply(sd, wpd, compd, fd, ld) if direct else ops.attn_step(sd, wpd, compd, fd, ld)
        close(ad, alpha, TOL_ALPHA, 'alpha (call %d)' % k)
        close(cd, ctx, TOL_CTX, 'ctx (call %d)' % k)
    loss = 0.0
    if use_datt:
        loss = loss + (ad * ga.float().to(dev())).sum()
    if use_dctx:
        loss = loss + (cd * gc.float().to(dev())).sum()
    loss.backward()
    for name, a, g in zip(NAMES, dl, grads):
        close(a.grad, g, TOL_GRAD, 'd' + name)


def lens_for(mode, T, edge):
    if mode == 'none':
        return None
    lens = edge_lens(T, edge)
    if mode == 'above':
        lens[0] = T + 5          # stands for the full-length utterance: the kernels clamp
    return lens


def _B(lens, default=4):
    return default if lens is None else len(lens)


# ------------------------------------------------------------------------------------------------ fast<1> ----
@pytest.mark.parametrize('T,E,mode', [(1, 512, 'edges'), (8, 512, 'edges'), (127, 512, 'edges'), (128, 512, 'edges'),
                                      (128, 128, 'edges'), (128, 256, 'edges'), (128, 1024, 'edges'),
                                      (127, 512, 'none'), (128, 256, 'above')])
def test_fast1_kernel(T, E, mode):
    """attn_step_fwd_fast_kernel<1>: A = 128, E = 128 nch, T <= 128 (no shape with T <= 128 has a workspace, so
    ops.attn_step lands here).  T = 1 and 8: one row, one row per half-wave; 127 / 128: the last of the 16 rows
    per half-wave missing / present; E = 128 is nch = 1, E = 1024 is 8 column chunks.  Lengths on a row-group
    edge (a multiple of 8), NULL and above T."""
    lens = lens_for(mode, T, 8 * ((T - 1) // 8))
    assert ws_floats(_B(lens), T, 128, E) == 0
    run_case(_B(lens), T, 128, E, lens)


# ------------------------------------------------------------------------------------------------ fast<2> ----
@pytest.mark.parametrize('T,E,direct,mode', [(129, 256, False, 'edges'), (255, 256, False, 'edges'),
                                             (256, 256, False, 'edges'), (129, 512, True, 'edges'),
                                             (256, 512, True, 'edges'), (255, 256, False, 'none'),
                                             (256, 512, True, 'above')])
def test_fast2_kernel(T, E, direct, mode):
    """attn_step_fwd_fast_kernel<2>: A = 128, E = 128 nch, 128 < T <= 256 and no workspace.  At E = 256 the library
    offers no workspace (asserted) and ops.attn_step lands here; at E = 512 ops would take the split form, so the
    C ABI is called with ws = NULL: the path of a device on which the split grid is not resident.  T = 129 is one
    row in the second pass, 256 fills it; a length of 128 ends exactly on the first pass."""
    lens = lens_for(mode, T, 128)
    if not direct:
        assert ws_floats(_B(lens), T, 128, E) == 0
    run_case(_B(lens), T, 128, E, lens, direct=direct)


# --------------------------------------------------------------------------------------------------- long ----
@pytest.mark.parametrize('T,E,direct,mode', [(257, 256, False, 'edges'), (384, 256, False, 'edges'),
                                             (385, 256, False, 'edges'), (300, 512, True, 'edges'),
                                             (1025, 512, False, 'edges'), (385, 256, False, 'none'),
                                             (300, 512, True, 'above')])
def test_long_kernel(T, E, direct, mode):
    """attn_step_fwd_long_kernel: A = 128, E = 128 nch, T > 256 and no workspace.  E = 256 has no workspace
    (asserted); E = 512 at T = 300 is the C ABI with ws = NULL; E = 512 at T = 1025 is past the split form's
    T <= 1024 (workspace asserted 0), the only default-size shape that reaches this kernel through ops.  T = 257 is
    one row in the third pass of 128 rows, 384 three exact passes, 385 one row past them; a length of 256 ends on
    a pass."""
    lens = lens_for(mode, T, 256)
    if not direct:
        assert ws_floats(_B(lens), T, 128, E) == 0
    run_case(_B(lens), T, 128, E, lens, direct=direct)


# -------------------------------------------------------------------------------------------------- split ----
def split_rph_model(B, T):
    """attn_split_rph (csrc/attn_kernels.h) as published: the largest of 6, 4, 3, 2 rows per half-wave that still
    gives 256 workgroups, else 2."""
    for rph in (6, 4, 3, 2):
        if B * ((T + 8 * rph - 1) // (8 * rph)) >= 256:
            return rph
    return 2


def run_split(B, T, lens, rph, forced):
    from ss_asr_amd import _lib, ops
    old = _lib.set_option('SSASR_ATTN_RPH', rph if forced else 0)
    try:
        ns = (T + 8 * rph - 1) // (8 * rph)
        n = ws_floats(B, T, 128, 512)
        assert n > 0, 'the split grid is not resident on this device'
        assert n == 2 * B * ns * ATTN_PART, (n, ns)           # the record count of THIS slice size
        run_case(B, T, 128, 512, lens, calls=2)               # both exchange buffers of the workspace
        ops.check_persistent_status()
    finally:
        _lib.set_option('SSASR_ATTN_RPH', old)


@pytest.mark.parametrize('T,rph', [(T, rph) for T in (129, 192, 193, 1024) for rph in (2, 3, 4, 6)])
def test_split_kernel_forced_size(T, rph):
    """attn_step_fwd_split_kernel<rph> forced with SSASR_ATTN_RPH (slices of R = 8 rph = 16 / 24 / 32 / 48 rows): the
    workspace size asserted first is the one of exactly this slice size.  T = 129 is the smallest split shape,
    192 a whole number of slices for every R, 193 one row past it, 1024 the largest (NS = 64 at rph = 2: every
    pair lane and all of sPm / sPs).  Lengths: T, T - 1, the largest whole number of slices below T (the last slice
    empty) and 1 (every slice but the first empty).  Two calls on one workspace, both checked: the two exchange
    buffers, as the decode loop alternates them."""
    R = 8 * rph
    lens = edge_lens(T, R * ((T - 1) // R))
    run_split(len(lens), T, lens, rph, True)


@pytest.mark.parametrize('mode', ['none', 'above'])
def test_split_kernel_lengths_null_and_above_T(mode):
    """The split form with enc_len = NULL and with an entry above T (clamped), at T = 193 and 3 rows per half-wave."""
    lens = lens_for(mode, 193, 192)
    run_split(_B(lens), 193, lens, 3, True)


def test_split_kernel_size_the_model_picks():
    """Option 0 at B = 32, T = 300: 6 rows per half-wave give 32 x 7 = 224 workgroups, 4 give 32 x 10 = 320 >= 256,
    so the published rule picks split<4> (asserted through the workspace size)."""
    B, T = 32, 300
    assert split_rph_model(B, T) == 4
    run_split(B, T, [T - 7 * k for k in range(B)], 4, False)


# ------------------------------------------------------------------------------ general forward, backward ----
GENERAL = [(4, 4, 1), (12, 132, 9), (132, 512, 130), (128, 516, 300), (16, 1028, 9), (16, 2056, 9), (2048, 8, 7)]


@pytest.mark.parametrize('A,E,T,mode', [s + ('edges',) for s in GENERAL] +
                         [(12, 132, 9, 'none'), (132, 512, 130, 'above')])
def test_general_kernel_and_backward(A, E, T, mode):
    """attn_step_fwd_kernel (any A other than 128, or an E whose column chunks are not 128 wide) and
    attn_step_bwd_kernel, the one backward form, over the same shapes.  (4, 4, 1) is the smallest legal shape;
    (132, 512, 130) misses the fast forms by A, (128, 516, 300) by E (nch = 3, chunks of 172); A = 2048 is the
    declared limit.  E = 1028 = 4 x 257 has no quad-aligned divisor, so attn_pick_nch gives ONE chunk of 257 quads,
    more than the block's 256 threads, and E = 2056 two such chunks: before the strided context loop these two
    cases returned ctx = 0 (with a correct alpha)."""
    lens = lens_for(mode, T, 8 * ((T - 1) // 8))
    assert ws_floats(_B(lens), T, A, E) == 0
    run_case(_B(lens), T, A, E, lens)


@pytest.mark.parametrize('T', [5, 6, 7])
@pytest.mark.parametrize('use_datt,use_dctx', [(True, True), (False, True), (True, False)])
def test_backward_kernel_missing_gradients_and_lds_offsets(T, use_datt, use_dctx):
    """attn_step_bwd_kernel at T = 5, 6, 7 (its LDS regions start at (T + 3) & ~3 floats) with datt = NULL (only
    ctx carries gradient: the kernel's own branch, reached through the C ABI) and without dctx (only alpha)."""
    lens = [T, T - 1, 1]
    run_case(3, T, 12, 132, lens, direct=True, use_datt=use_datt, use_dctx=use_dctx)


# ----------------------------------------------------------------------------------------- declared corners ----
def corner_reference(q, comp, feat, ga, gc):
    """float64 alpha, ctx, de (derivative by the energies) and dqpre (by the argument of q's tanh) of the oracle,
    from the float32 inputs the kernels get.  q enters the oracle as tanh(atanh(q) . I); de is recovered from
    dcomp = de (x) q."""
    q64 = q.double()
    qpre = torch.atanh(q64).requires_grad_(True)
    c = comp.double().requires_grad_(True)
    alpha, ctx = lo.attention_step_explicit(qpre, feat.double(), c, None, torch.eye(q.shape[1], dtype=torch.float64))
    ((alpha * ga.double()).sum() + (ctx * gc.double()).sum()).backward()
    de = (c.grad * q64.unsqueeze(1)).sum(-1) / (q64 * q64).sum(-1, keepdim=True)
    return alpha.detach(), ctx.detach(), de, qpre.grad


def run_corner(A, E, T, forward):
    """One utterance at a declared limit of ssasr_attn_step_fwd / _bwd, through the C ABI on float32 inputs: the
    kernels' own outputs (alpha, ctx, de, dqpre) against the oracle on the same numbers.  Without `forward` the
    backward pass gets the oracle's alpha (rounded to float32) as its att."""
    from ss_asr_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(A + E + T)
    r32 = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)      # noqa: E731
    q = torch.tanh(r32(1, A)) * min(1.0, (128.0 / A) ** 0.5)                # |e| ~ 10, as in reference()
    comp, feat = torch.tanh(r32(1, T, A)), r32(1, T, E)
    ga, gc = r32(1, T), r32(1, E)
    alpha, ctx, de, dqpre = corner_reference(q, comp, feat, ga, gc)
    qd, compd, featd, gad, gcd = (t.to(dev()) for t in (q, comp, feat, ga, gc))
    if forward:
        att, cx = torch.empty(1, T, device=dev()), torch.empty(1, E, device=dev())
        # state = NULL: q is an input, w_phi (mandatory, unused) any device pointer, D = 0
        _lib.check(lib.ssasr_attn_step_fwd(None, _p(qd), _p(compd), _p(featd), None, 1, T, A, E, 0, _p(qd), _p(att),
                                           _p(cx), None, 0, None, _stream()), 'ssasr_attn_step_fwd')
        close(att, alpha, TOL_ALPHA, 'alpha')
        close(cx, ctx, TOL_CTX, 'ctx')
    else:
        att = alpha.float().to(dev())
    ded, dqd = torch.empty(1, T, device=dev()), torch.empty(1, A, device=dev())
    _lib.check(lib.ssasr_attn_step_bwd(_p(gcd), _p(gad), _p(att), _p(qd), _p(compd), _p(featd), None, 1, T, A, E,
                                       _p(ded), _p(dqd), _stream()), 'ssasr_attn_step_bwd')
    close(ded, de, TOL_GRAD, 'de')
    close(dqd, dqpre, TOL_GRAD, 'dqpre')


CORNERS = [(128, 512, 16384, True), (2048, 4, 16384, True), (4, 8192, 16384, False)]


@pytest.mark.parametrize('A,E,T,forward', CORNERS)
def test_declared_corner(A, E, T, forward):
    """The limits ssasr.h declares (T <= 16384, A <= 2048, E <= 8192), where the dynamic LDS of the long, general
    and backward kernels passes 64 KB and the launch first has to raise the kernel's limit: (128, 512, 16384) is
    the long kernel (69,696 bytes) and the backward kernel (75,840); (2048, 4, 16384) the general kernel (77,888);
    (4, 8192, 16384) the backward kernel's largest request (106,560), backward only, at a given alpha."""
    run_corner(A, E, T, forward)
