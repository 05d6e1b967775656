"""The CTC loss kernels (ssasr_ctc_loss_fwd / _bwd of csrc/ctc.hip, through ops.ctc_loss, ops._ctc_fwd / _ctc_bwd and
the C entries themselves) at every launch form and edge, against float64 on the CPU.

Checker: torch.nn.functional.ctc_loss(reduction='none') in float64, called PER ROW on log_softmax(logits[b, :n]),
n = min(frame_len, T); the test composes loss = (1 / B) sum_b nll_b / max(L_b, 1) over the rows that have an
alignment itself and takes autograd of that.  A row has none when n < 1, L > Lmax or n < L + adjacent repeats: it
adds 0 and its gradient must be EXACTLY zero, as must every frame at or past n.  (The batched torch call cannot say
"no frames" or "more frames than T".)  References are built once per module (_refs).

The launcher picks ctc_threads(Sp, V) = 256 | 512 | 1024 by max(Sp = 2 Lmax + 1, V), and the log-softmax table's home
by T * V * 4 <= 128 KB (LDS) or more (workspace).  Which case runs which instantiation <LDS_TABLE, NT> -- the same
pair for ctc_alpha_kernel and ctc_beta_kernel, since both entries decide alike:

    <true,  256>   lmax 127 (Sp 255), V 2 / 64 / 65 (Sp 9), 655 frames, blank 49 / 3, the edges, wide y
    <false, 256>   656 frames (V 50, Sp 121: 131,200 bytes of table)
    <true,  512>   lmax 128 (Sp 257), lmax 255 (Sp 511), V 257 (chosen by V), one of four (Sp 281)
    <false, 512>   V 300 ws (Sp 401, T 110: 132,000 bytes)
    <true, 1024>   lmax 256 (Sp 513), V 513 and V 1024 (chosen by V), largest LDS (Sp 1023, V 1024), scale 8 (Sp 561)
    <false,1024>   V 1024 ws (Sp 33, T 33: 135,168 bytes; threads chosen by V)

V 65 / 257 / 300 / 513 / 1024 take ctc_table's lane loop (v += 64) more than once, V 65 with a tail of one lane.
Every case passes its labels as the [:, 1:] view of a wider int32 matrix (non-zero storage offset, y_ld > Lmax) whose
unused columns hold a non-blank class, so a read past label_lens[b] changes the result.

Bounds.  Logits are 2.0 * randn rounded to float32 once (the checker sees the rounded values); loss and gradient
take test_gpu_ctc.py's own bounds, scaled by dloss: |loss - want| <= 2e-6 max(1, |want|), max |dlogits - want| <=
5e-7 dloss.  The scale-8 case follows the NOISE rule of test_gpu_align.py: NOISE = |checker in float32 on the CPU -
checker in float64|, for the loss and for max |gradient| apart; the kernel must lie within 8 * NOISE.  The constants
below were measured with the checker on the CPU; the test recomputes them and prints them with the GPU's worst
errors.  Needs an MI355X."""
import math
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_align import labels_of, min_frames

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
LOSS_TOL, GRAD_TOL = 2e-6, 5e-7             # test_gpu_ctc.py's
# float32 checker against float64 checker on the CPU at the scale-8 case (V 50, T 600, L 280 / 120; loss 39.497, nll
# 6070 and 6878, max |gradient| 4.2e-3): measured 9.03e-6 (loss) and 2.14e-5 (max |gradient|); the constants leave a
# tenth for another host's float32 exp / log
NOISE_LOSS, NOISE_GRAD = 1.0e-5, 2.4e-5
PAD = 64


def repeating(rng, L, V, blank):
    """L labels from at most three classes, the second equal to the first: adjacent repeats for certain."""
    classes = [c for c in range(V) if c != blank][:3]
    out = [int(rng.choice(classes)) for _ in range(L)]
    if L > 1:
        out[1] = out[0]
    return out


def distinct(rng, L, V, blank):
    """L labels without adjacent repeats; with one label class (V == 2) every neighbour is a repeat."""
    if V == 2:
        return [1 - blank] * L
    return labels_of(rng, L, V, blank, repeats=False)


def make_case(name, V, T, rows, lmax, blank=0, seed=0, scale=2.0, y_ld=None, offset=1, none=0, logits=None):
    """rows: [(frame_len, labels)].  y is wide[:, offset:]; columns that hold no label hold a non-blank class.
    none: how many rows the checker must find without an alignment."""
    B = len(rows)
    if logits is None:
        g = torch.Generator().manual_seed(seed)
        logits = (torch.randn(B, T, V, generator=g, dtype=torch.float64) * scale).float()
    y_ld = lmax + 3 if y_ld is None else y_ld
    fill = (blank + 1) % V
    wide = torch.full((B, offset + y_ld), fill, dtype=torch.int32)
    for b, (_, labels) in enumerate(rows):
        assert len(labels) <= y_ld and all(0 <= c < V and c != blank for c in labels)
        wide[b, offset:offset + len(labels)] = torch.tensor(labels, dtype=torch.int32)
    return types.SimpleNamespace(name=name, V=V, T=T, B=B, lmax=lmax, blank=blank, logits=logits, wide=wide, offset=offset,
                                 frame_lens=torch.tensor([r[0] for r in rows], dtype=torch.int32),
                                 label_lens=torch.tensor([len(r[1]) for r in rows], dtype=torch.int32), rows=rows,
                                 none=none)


REP = [5, 5, 7, 7, 7, 9]                                        # three adjacent repeats: 9 frames at the least
BY_SP = ['lmax %d' % n for n in (127, 128, 255, 256)]
BY_V = ['V %d' % v for v in (2, 64, 65, 257, 513, 1024)]
TABLES = ['655 frames', '656 frames', 'V 300 ws', 'V 1024 ws']
OTHERS = ['largest LDS', 'blank 49', 'blank 3', 'frame edges', 'repeat edges', 'wide y']
NAMES = BY_SP + BY_V + TABLES + OTHERS


def build_cases():
    rng = np.random.default_rng(2025)
    cases = []
    for lmax in (127, 128, 255, 256):                           # 1. Sp 255 | 257, 511 | 513: 256 | 512 | 512 | 1024 threads
        T = lmax + 5
        rows = [(T, labels_of(rng, lmax, 50, 0, repeats=False)), (T - 3, repeating(rng, lmax // 2, 50, 0)),
                (T, labels_of(rng, 3, 50, 0))]                  # S = 7 << Sp: the lattice stride is not the live width
        assert min_frames(rows[1][1]) > lmax // 2
        cases.append(make_case('lmax %d' % lmax, 50, T, rows, lmax, seed=lmax))
    for V in (2, 64, 65, 257, 513, 1024):                       # 2. threads by V: 256, 256, 256, 512, 1024, 1024
        rows = [(9, repeating(rng, 3, V, 0)), (4, distinct(rng, 4, V, 0)), (9, [])]
        cases.append(make_case('V %d' % V, V, 9, rows, 4, seed=V, none=int(V == 2)))    # V 2: four 1s need 7 frames
    for name, V, lmax, T in (('655 frames', 50, 60, 655), ('656 frames', 50, 60, 656),  # 3. the table's two homes
                             ('V 300 ws', 300, 200, 110), ('V 1024 ws', 1024, 16, 33)):
        n = min(lmax, T - 10)
        rows = [(T, labels_of(rng, n, V, 0, repeats=False)), (T - 7, repeating(rng, n // 2, V, 0)),
                (T, labels_of(rng, 3, V, 0))]
        cases.append(make_case(name, V, T, rows, lmax, seed=T))
    rows = [(32, repeating(rng, 16, 1024, 0)), (32, labels_of(rng, 32, 1024, 0, repeats=False)), (32, [])]
    assert 16 < min_frames(rows[0][1]) <= 32
    cases.append(make_case('largest LDS', 1024, 32, rows, 511, seed=40))                # 4. 159,756 bytes in _bwd
    for blank in (49, 3):                                       # 5. class 0 is a label
        rows = [(12, [0, 0, 2, 7, 0]), (10, labels_of(rng, 5, 50, blank) + [0]), (12, [])]
        cases.append(make_case('blank %d' % blank, 50, 12, rows, 6, blank=blank, seed=50 + blank))
    cases.append(frame_edges(21))                               # 6. T + 9 frames, none, L > Lmax
    cases.append(make_case('repeat edges', 50, 10, [(10, REP), (9, REP), (8, REP)], 6, seed=61, none=1))
    rows = [(20, labels_of(rng, 7, 50, 0)), (15, labels_of(rng, 2, 50, 0)), (20, []), (18, repeating(rng, 5, 50, 0))]
    cases.append(make_case('wide y', 50, 20, rows, 7, seed=70, y_ld=7 + 300))           # 7. y_ld >> Lmax
    assert [c.name for c in cases] == NAMES
    return cases


def frame_edges(first_len, name='frame edges'):
    rng = np.random.default_rng(60)
    rows = [(first_len, labels_of(rng, 5, 50, 0)), (0, labels_of(rng, 3, 50, 0)), (12, labels_of(rng, 4, 50, 0)),
            (12, labels_of(rng, 6, 50, 0, repeats=False))]      # label_lens[3] = Lmax + 1
    return make_case(name, 50, 12, rows, 5, seed=60, none=2)


def batch_of_four():
    """10. one row (T - 3 frames, 70 labels with repeats, Sp 281: five waves of 512 threads) inside four."""
    rng = np.random.default_rng(100)
    T, lmax = 200, 140
    rows = [(T, labels_of(rng, 140, 50, 0, repeats=False)), (150, labels_of(rng, 20, 50, 0)),
            (T - 3, repeating(rng, 70, 50, 0)), (T, [])]
    return make_case('one of four', 50, T, rows, lmax, seed=100)


def scale_8():
    """11. V 50, T 600, (600 frames, 280 labels) and (590 frames, 120 labels), logits 8.0 * randn: Sp 561."""
    rng = np.random.default_rng(110)
    rows = [(600, labels_of(rng, 280, 50, 0)), (590, labels_of(rng, 120, 50, 0))]
    return make_case('scale 8', 50, 600, rows, 280, seed=110, scale=8.0)


_cases, _refs = {}, {}


def case_of(name):
    if not _cases:
        for c in build_cases() + [batch_of_four(), scale_8()]:
            _cases[c.name] = c
    return _cases[name]


def frames_of(case, b):
    return min(int(case.frame_lens[b]), case.T)


def has_alignment(case, b):
    labels = case.rows[b][1]
    return frames_of(case, b) >= 1 and len(labels) <= case.lmax and frames_of(case, b) >= min_frames(labels)


def checker(case, dtype=torch.float64):
    """-> loss (float), dlogits [B, T, V] for dloss = 1, nll per row (inf: no alignment)."""
    x = case.logits.to(dtype).clone().requires_grad_(True)
    total, nll = None, []
    for b, (_, labels) in enumerate(case.rows):
        if not has_alignment(case, b):
            nll.append(math.inf)
            continue
        n, L = frames_of(case, b), len(labels)
        lp = F.log_softmax(x[b, :n], dim=-1).unsqueeze(1)
        v = F.ctc_loss(lp, torch.tensor([labels], dtype=torch.long).view(1, L), torch.tensor([n]), torch.tensor([L]),
                       blank=case.blank, reduction='none', zero_infinity=False)[0]
        nll.append(float(v.detach()))
        assert math.isfinite(nll[-1]), (case.name, b)
        total = v / max(L, 1) if total is None else total + v / max(L, 1)
    assert total is not None, case.name
    loss = total / case.B
    loss.backward()
    return types.SimpleNamespace(loss=float(loss.detach()), grad=x.grad, nll=nll)


def reference(case):
    if case.name not in _refs:
        ref = checker(case)
        assert sum(v == math.inf for v in ref.nll) == case.none, case.name
        _refs[case.name] = ref
    return _refs[case.name]


def device_inputs(case):
    return (case.logits.to(DEV), case.frame_lens.to(DEV), case.wide.to(DEV)[:, case.offset:], case.label_lens.to(DEV))


def run(case, dloss=1.0):
    """Loss and dlogits of ops.ctc_loss through autograd, the gradient of dloss * loss."""
    from ss_asr_amd import ops
    logits, frame_lens, y, label_lens = device_inputs(case)
    logits.requires_grad_(True)
    got = ops.ctc_loss(logits, frame_lens, y, label_lens, case.lmax, case.blank)
    (dloss * got).backward()
    return got.detach().cpu(), logits.grad.cpu()


def exact_zeros(case, grad):
    for b in range(case.B):
        live = frames_of(case, b) if has_alignment(case, b) else 0
        assert int(torch.count_nonzero(grad[b, live:])) == 0, (case.name, b)


def compare(case, loss, grad, ref, dloss=1.0):
    """Asserts the bounds of the module's docstring; -> (loss error, gradient error)."""
    assert loss.dtype == grad.dtype == torch.float32 and grad.shape == ref.grad.shape
    e_loss = abs(float(loss) - ref.loss)
    e_grad = (grad.double() - dloss * ref.grad).abs().max().item()
    print('%-13s B %d T %3d V %4d Lmax %3d dloss %g: loss %.9g (want %.9g, error %.3e), gradient error %.3e'
          % (case.name, case.B, case.T, case.V, case.lmax, dloss, float(loss), ref.loss, e_loss, e_grad))
    assert e_loss <= LOSS_TOL * max(1.0, abs(ref.loss)), (case.name, e_loss)
    assert e_grad <= GRAD_TOL * dloss, (case.name, e_grad)
    exact_zeros(case, grad)
    return e_loss, e_grad


def lattice(case, ws):
    """alpha [B, T, Sp] and nll [B] doubles of the workspace that ssasr_ctc_loss_fwd left."""
    sp = 2 * case.lmax + 1
    n = case.B * case.T * sp
    d = ws[:2 * (n + case.B)].view(torch.float64)
    return d[:n].view(case.B, case.T, sp).cpu(), d[n:].cpu()


@pytest.mark.parametrize('name', NAMES)
def test_loss_and_gradient_match_the_per_row_float64_checker(name):
    """Cases 1 - 7.  'largest LDS' asks _bwd for 159,756 bytes of dynamic LDS: ops raises unless both launches
    return SSASR_OK."""
    case = case_of(name)
    compare(case, *run(case), reference(case))


def test_the_checker_counts_the_rows_without_an_alignment():
    none = {n: sum(v == math.inf for v in reference(case_of(n)).nll) for n in NAMES}
    assert {n: k for n, k in none.items() if k} == {'V 2': 1, 'frame edges': 2, 'repeat edges': 1}
    assert [has_alignment(case_of('frame edges'), b) for b in range(4)] == [True, False, True, False]
    assert [has_alignment(case_of('repeat edges'), b) for b in range(3)] == [True, True, False]
    assert [has_alignment(case_of('V 2'), b) for b in range(3)] == [True, False, True]
    # nine frames hold REP in exactly one way: 5 _ 5 7 _ 7 _ 7 9
    case = case_of('repeat edges')
    lp = F.log_softmax(case.logits[1, :9].double(), dim=-1)
    one = -sum(float(lp[t, c]) for t, c in enumerate([5, 0, 5, 7, 0, 7, 0, 7, 9]))
    assert abs(reference(case).nll[1] - one) <= 1e-12 * one


def test_the_table_leaves_lds_above_128_kb():
    """ssasr_ctc_ws_floats holds the lattice and nll in doubles, and the table only from T * V * 4 > 128 KB on."""
    from ss_asr_amd import _lib
    lib = _lib.load()
    in_ws = {'655 frames': False, '656 frames': True, 'V 300 ws': True, 'V 1024 ws': True, 'largest LDS': False}
    for name in NAMES:
        c = case_of(name)
        table = in_ws.get(name, False)
        assert table == (c.T * c.V * 4 > 128 * 1024), name
        want = 2 * (c.B * c.T * (2 * c.lmax + 1) + c.B) + (c.B * c.T * c.V if table else 0)
        assert int(lib.ssasr_ctc_ws_floats(c.B, c.T, c.V, c.lmax)) == want, name


def test_frames_beyond_t_are_clamped():
    """frame_lens[0] = T + 9 against the same batch with frame_lens[0] = T: no atomics feed nll or the loss."""
    from ss_asr_amd import ops
    case, twin = case_of('frame edges'), frame_edges(12, 'frame edges at T')
    assert int(case.frame_lens[0]) == case.T + 9 and torch.equal(case.logits, twin.logits)
    loss, grad = run(case)
    loss_t, grad_t = run(twin)
    compare(twin, loss_t, grad_t, reference(case))
    assert torch.equal(loss, loss_t)
    assert (grad - grad_t).abs().max().item() <= GRAD_TOL
    nll = [lattice(c, ops._ctc_fwd(*device_inputs(c), c.lmax, c.blank)[1])[1] for c in (case, twin)]
    assert torch.equal(nll[0], nll[1])
    assert [math.isfinite(float(v)) for v in nll[0]] == [True, False, True, False]


def test_label_matrix_layout_does_not_matter():
    """y_ld = Lmax + 300 behind a one-column offset against a [B, Lmax] matrix of its own, padded with the blank."""
    case = case_of('wide y')
    tight = make_case('tight y', case.V, case.T, case.rows, case.lmax, y_ld=case.lmax, offset=0, logits=case.logits)
    tight.wide[tight.wide == 1] = 0
    for b, (_, labels) in enumerate(case.rows):
        tight.wide[b, :len(labels)] = torch.tensor(labels, dtype=torch.int32)
    assert case.wide.shape == (4, 308) and tight.wide.shape == (4, 7)
    assert int((case.wide[:, 1:8] != tight.wide).sum()) > 0          # the padding differs where no label is
    loss, grad = run(case)
    loss_t, grad_t = run(tight)
    compare(tight, loss_t, grad_t, reference(case))
    assert torch.equal(loss, loss_t)
    assert (grad - grad_t).abs().max().item() <= GRAD_TOL


@pytest.mark.parametrize('name', ['lmax 128', 'V 65', 'V 300 ws'])
def test_dloss_scales_the_gradient_and_dbias_is_added_to(name):
    from ss_asr_amd import ops
    case, ref = case_of(name), reference(case_of(name))
    compare(case, *run(case, dloss=3.0), ref, dloss=3.0)
    inputs = device_inputs(case)
    loss, ws = ops._ctc_fwd(*inputs, case.lmax, case.blank)
    dbias = torch.full((case.V,), 0.25, device=DEV)
    dlogits = ops._ctc_bwd(*inputs, case.lmax, case.blank, ws, torch.tensor(3.0, device=DEV), dbias=dbias).cpu()
    compare(case, loss.cpu(), dlogits, ref, dloss=3.0)
    dbias_identity(case, dbias.cpu(), dlogits)


def dbias_identity(case, dbias, dlogits):
    added = dbias.double() - 0.25
    want = dlogits.double().sum((0, 1))
    tol = 1e-6 * dlogits.double().abs().sum((0, 1)).clamp(min=1.0)
    print('%-13s dbias - 0.25 against the sum of dlogits: worst %.3e' % (case.name, (added - want).abs().max().item()))
    assert bool(((added - want).abs() <= tol).all()), case.name
    assert float(want.abs().max()) > 1e-3                           # the identity is not 0 == 0


@pytest.mark.parametrize('name', ['655 frames', '656 frames'])
def test_canaries_behind_every_output_stay_intact(name):
    """ws of exactly ssasr_ctc_ws_floats floats, dlogits, loss and dbias, each with 64 sentinels behind it: one
    case with the table in LDS, one with it in the workspace.  Every dlogits element is written."""
    from ss_asr_amd import _lib, ops
    lib = _lib.load()
    case = case_of(name)
    B, T, V, lmax = case.B, case.T, case.V, case.lmax
    n = int(lib.ssasr_ctc_ws_floats(B, T, V, lmax))
    logits, frame_lens, y, label_lens = device_inputs(case)
    assert y.storage_offset() == 1 and y.stride(0) == lmax + 4
    ws = torch.full((n + PAD,), 77.0, device=DEV)
    loss = torch.full((1 + PAD,), 77.0, device=DEV)
    dlogits = torch.full((B * T * V + PAD,), math.nan, device=DEV)
    dlogits[B * T * V:] = 77.0
    dbias = torch.full((V + PAD,), 77.0, device=DEV)
    dbias[:V] = 0.25
    dloss = torch.ones((), device=DEV)
    head = (ops._p(logits), ops._p(frame_lens), ops._p(y), y.stride(0), ops._p(label_lens), B, T, V, lmax, case.blank)
    assert lib.ssasr_ctc_loss_fwd(*head, ops._p(ws), ops._p(loss), ops._stream()) == 0
    assert lib.ssasr_ctc_loss_bwd(*head, ops._p(ws), ops._p(dloss), ops._p(dlogits), ops._p(dbias), ops._stream()) == 0
    torch.cuda.synchronize()
    for t, k in ((ws, n), (loss, 1), (dlogits, B * T * V), (dbias, V)):
        assert bool((t[k:] == 77.0).all()), name
    assert not bool(torch.isnan(dlogits).any())
    grad = dlogits[:B * T * V].view(B, T, V).cpu()
    compare(case, loss[0].cpu(), grad, reference(case))
    assert bool(torch.isfinite(dbias[:V]).all()) and bool((dbias[:V] != 0.25).any())


def test_a_row_does_not_see_its_batch():
    """The row alone (B = 1, dloss 0.25) and as row 2 of four (dloss 1.0): the same scale dloss / B.  nll and the
    alpha lattice have no atomics behind them and must be bit-equal; the class sums are LDS float atomics in no
    fixed order, so the gradients agree within the gradient bound only."""
    from ss_asr_amd import ops
    four = case_of('one of four')
    alone = make_case('alone', four.V, four.T, four.rows[2:3], four.lmax, logits=four.logits[2:3].clone())
    n, S = frames_of(four, 2), 2 * len(four.rows[2][1]) + 1
    got = []
    for case, b, dloss in ((four, 2, 1.0), (alone, 0, 0.25)):
        inputs = device_inputs(case)
        loss, ws = ops._ctc_fwd(*inputs, case.lmax, case.blank)
        alpha, nll = lattice(case, ws)
        grad = ops._ctc_bwd(*inputs, case.lmax, case.blank, ws, torch.tensor(dloss, device=DEV)).cpu()
        compare(case, loss.cpu(), grad, reference(case), dloss=dloss)
        got.append((alpha[b, :n, :S].clone(), nll[b].clone(), grad[b]))
    assert math.isfinite(float(got[0][1])) and got[0][0].shape == (n, S) and n == four.T - 3 and S == 141
    assert torch.equal(got[0][1], got[1][1])
    assert torch.equal(got[0][0], got[1][0])
    assert (got[0][2] - got[1][2]).abs().max().item() <= GRAD_TOL
    assert abs(reference(four).nll[2] - float(got[0][1])) <= LOSS_TOL * reference(four).nll[2]


def test_the_double_lattice_holds_at_logit_scale_8():
    """Case 11: the kernel within 8 * NOISE of float64, NOISE = the float32 checker's own error."""
    case = case_of('scale 8')
    ref, ref32 = reference(case), checker(case, torch.float32)
    noise_loss = abs(ref32.loss - ref.loss)
    noise_grad = (ref32.grad.double() - ref.grad).abs().max().item()
    loss, grad = run(case)
    e_loss = abs(float(loss) - ref.loss)
    e_grad = (grad.double() - ref.grad).abs().max().item()
    print('scale 8: loss %.9g, nll %s; NOISE loss %.3e (constant %.3e) gradient %.3e (constant %.3e); '
          'GPU error loss %.3e gradient %.3e' % (ref.loss, ref.nll, noise_loss, NOISE_LOSS, noise_grad, NOISE_GRAD,
                                                 e_loss, e_grad))
    assert noise_loss <= NOISE_LOSS and noise_grad <= NOISE_GRAD
    assert e_loss <= 8 * NOISE_LOSS and e_grad <= 8 * NOISE_GRAD
    exact_zeros(case, grad)
