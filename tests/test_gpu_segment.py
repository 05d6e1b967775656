"""CTC segmentation on the GPU (ssasr_ctc_segment through ops.ctc_segment / ops.ctc_head_segment; ASR.segment) against
postprocess.ctc_segment_reference on float64 log_softmax values, the float64 restatement of include/ssasr.h.

The rule.  The kernel forms each frame's normaliser in float, and with free ends the paths no longer share their
frames, so a decision whose margin is below the float arithmetic can fall either way.  A case is COMPARED when the
checker's gap (the smallest margin over the decisions on the returned path and the end choice) is >= MIN_GAP = 1e-3,
the project's rule (test_gpu_ctc_search.py); rows that the checker cannot segment are always compared.  path, first,
last, utt_first, utt_last and the set of rows without a segmentation must then be EQUAL; score, char_logp and
utt_conf must lie within BOUND = 8 * NOISE of the checker's.  NOISE is the largest |float32 run - float64 run| of the
checker over the compared cases, log-softmax included, measured on the CPU by running this file as a script
(`python tests/test_gpu_segment.py`, with oracle/ on the path): 7.35e-4 over the issue's cells, the form boundaries and
the batches (worst: a score of the (600,40,200) cell; the boundary cases reach 4.5e-4 at 8,839 frames); the two limit
rows have NOISE_LONG = 5.8e-4 of their own (5.72e-4 at the 32,768-frame row, 3.93e-4 at the 8,200-frame row), as the
4,096-frame row of test_gpu_ctc_search.py has, and so has each wide cell (WIDE_NOISE: 2.70e-3, 3.74e-3, 7.49e-2).  At
most a quarter of the enumerated cell cases may be skipped, and no cell entirely.  With the committed restatement and
this file's seeds every one of the issue's cells compares 16 of 16: 176 compared, 0 skipped (the issue's throw-away
run, with other seeds, skipped 2 of 176); the wide cells compare 8 of 8, 4 of 4 and 3 of 4.

Shapes.  The issue expected its cells to cross 'one state per thread, the first P > 1 form, blocks that are not full,
and S not a multiple of 64'.  With the form table that was built (one state per thread up to 1,024 states) they cross
only the first and the last: all have L <= 200.  Several states per thread and blocks that are not full are covered
by other cases instead: WIDE_CELLS, cells of the same make (random logits, a repeated pair in every second seed,
the same gap rule and cap) in the 256 x 8, 512 x 8 and 1024 x 16 forms, none with S a multiple of 8 or 16; the
all-equal-logits cases at 8 and 16 states per thread; and the boundary cases, which sit on each side of every
boundary that ssasr_ctc_segment_form reports (asked, not hard-coded), cross every (threads, states per thread) form
and are planted with two frames per label and adjacent repeats, so that their paths hold stay, s - 1 and s - 2 steps,
blank states and disallowed skips.  (The T = 8,200 / L = 8,191 limit row has no room for any of that: every step of
its path is s - 2.)  A thread's block of 8 or 16 states never straddles a 64-state back-pointer group (both divide
64): the group boundaries are always at block edges, and every boundary case with more than 64 states has them."""
import math
import types

import numpy as np
import pytest
import torch

import test_gpu_beam as tgb
import test_gpu_ctc_decode as tcd
import test_gpu_decode as tgd

pytestmark = pytest.mark.gpu

DEV = tgd.DEV
Mapper = tgd.Mapper
MIN_GAP = 1e-3
NOISE = 7.4e-4
NOISE_LONG = 5.8e-4
BOUND = 8 * NOISE
BOUND_LONG = 8 * NOISE_LONG
CELLS = [(1, 8, 1), (3, 8, 1), (3, 8, 2), (5, 8, 2), (5, 8, 3), (20, 8, 4), (20, 40, 10), (20, 40, 14), (160, 40, 30),
         (160, 40, 100), (600, 40, 200)]
SEEDS = 16
# cells of the same make in the forms with several states per thread: (T, V, L, seeds) -- 256 x 8, 512 x 8, 1024 x 16
# (the 1024 x 8 form has the boundary cases); fewer seeds, since a row's checker costs T x L.  Each has a NOISE of its
# own, for the reason the limit rows have: a float32 lattice of 1,500 .. 4,400 frames of 4 * standard_normal logits
# (scores of -10^4) is far noisier than the 600-frame cell, and one constant would loosen every smaller case.
WIDE_CELLS = [(1500, 40, 600, 8), (1300, 40, 1100, 4), (4400, 40, 4100, 4)]
WIDE_NOISE = {600: 2.8e-3, 1100: 3.8e-3, 4100: 7.5e-2}


def log_softmax(x, dtype=np.float64):
    x = np.asarray(x).astype(dtype)
    m = x.max(-1, keepdims=True)
    return x - (m + np.log(np.exp(x - m).sum(-1, keepdims=True, dtype=dtype)))


def split(rng, L):
    """Random utterance ends of an L-label text."""
    n = int(rng.integers(1, min(L, 4) + 1))
    cuts = sorted(rng.choice(np.arange(1, L), size=n - 1, replace=False).tolist()) if n > 1 else []
    return cuts + [L]


def make_case(name, V, T, rows, blank=0, window=3, logits=None, seed=0, long=False):
    """rows: [(frame_len, labels, utt_ends)].  The label and end matrices are one column wider than Lmax / Nmax and
    padded with values that must not be read."""
    B = len(rows)
    lmax, nmax = max(max(len(r[1]) for r in rows), 1), max(max(len(r[2]) for r in rows), 1)
    if logits is None:
        logits = (4.0 * np.random.default_rng(seed).standard_normal((B, T, V))).astype(np.float32)
    y = np.full((B, lmax + 1), V - 1, dtype=np.int32)
    ue = np.full((B, nmax + 1), -7, dtype=np.int32)
    for b, (_, labels, ends) in enumerate(rows):
        y[b, :len(labels)] = labels
        ue[b, :len(ends)] = ends
    return types.SimpleNamespace(name=name, V=V, T=T, B=B, lmax=lmax, nmax=nmax, blank=blank, window=window,
                                 logits=logits, y=y, utt_ends=ue, rows=rows, long=long,
                                 frame_lens=np.array([r[0] for r in rows], dtype=np.int32),
                                 label_lens=np.array([len(r[1]) for r in rows], dtype=np.int32),
                                 n_utts=np.array([len(r[2]) for r in rows], dtype=np.int32))


def cell_case(T, V, L, seeds=SEEDS):
    """The issue's cell: logits 4 * standard_normal, random labels in [1, V), a repeated first pair in every second
    seed; one row per seed."""
    rows = []
    for seed in range(seeds):
        rng = np.random.default_rng(1000 * T + 10 * L + seed)
        labels = [int(c) for c in rng.integers(1, V, L)]
        if seed % 2 and L >= 2:
            labels[1] = labels[0]
        rows.append((T, labels, split(rng, L)))
    return make_case('cell %s' % ((T, V, L),), V, T, rows, window=1 + T // 7, seed=T * V + L)


def planted(name, T, V, labels, ends, start, runs=1, window=30, long=False, seed=0):
    """One row whose path is planted 12 above unit noise: frames peaked on class V - 1, which the text does not have,
    around the labels' frames; the text's outer labels get one frame (each scored frame costs something, so free ends
    keep one frame of an outer run and the choice among a longer run's frames would be a near-tie), the inner ones
    `runs`, and a repeat gets a blank frame before it."""
    frames = []
    for j, c in enumerate(labels):
        if j and labels[j - 1] == c:
            frames.append(0)
        frames += [c] * (1 if j in (0, len(labels) - 1) else runs)
    assert V - 1 not in labels and start + len(frames) <= T
    frames = [V - 1] * start + frames + [V - 1] * (T - start - len(frames))
    x = np.random.default_rng(seed).standard_normal((T, V)).astype(np.float32)
    x[np.arange(T), frames] += 12.0
    return make_case(name, V, T, [(T, labels, ends)], window=window, logits=x[None], long=long)


def form_boundaries():
    """The largest Lmax of every launch form but the last, asked of the library."""
    from ss_asr_amd import ops
    out, prev = [], ops.ctc_segment_form(8, 1)
    for lmax in range(2, 8192):
        cur = ops.ctc_segment_form(8, lmax)
        if cur != prev:
            out.append(lmax - 1)
        prev = cur
    return out


def boundary_case(lmax):
    """A planted path with every kind of step: two frames per inner label (stay, then s - 2 or, through the blank
    frame that a repeat gets, s - 1 twice) and random labels of six classes, about a sixth of them adjacent repeats."""
    rng = np.random.default_rng(lmax)
    labels = [int(c) for c in rng.integers(1, 7, lmax)]
    repeats = sum(a == b for a, b in zip(labels, labels[1:]))
    assert lmax < 12 or repeats > lmax // 12
    return planted('boundary lmax %d' % lmax, 2 * lmax + repeats + 5, 8, labels, [max(lmax // 3, 1), max(lmax // 2, 2), lmax],
                   2, runs=2, seed=lmax)


def batch_cases():
    rng = np.random.default_rng(77)
    lab = lambda L, V, lo=1: [int(c) for c in rng.integers(lo, V, L)]
    rep = [5, 5, 7, 7, 7, 9]                                    # three adjacent repeats: nine frames at the least
    mixed = make_case('mixed', 12, 20, [(20, lab(4, 12), [1, 4]), (1, [6], [1]), (7, [1, 2, 3, 4, 5, 6, 7], [7]), (9, rep, [2, 6]),
                                        (8, rep, [2, 6]), (15, lab(6, 12), [1, 2, 3, 6]), (20, lab(5, 12), [2, 2, 5]),
                                        (0, [3], [1]), (6, [], [])], seed=1)
    blank3 = make_case('blank 3', 12, 14, [(14, [0, 0, 2, 5], [2, 4]), (10, [1, 2], [2])], blank=3, seed=2)
    return [mixed, blank3]


_refs = {}


def reference(case, dtype=np.float64):
    from ss_asr_amd.postprocess import ctc_segment_reference
    key = (case.name, np.dtype(dtype).name)
    if key not in _refs:
        out = []
        for b, (n, labels, ends) in enumerate(case.rows):
            n = min(n, case.T)
            out.append(ctc_segment_reference(log_softmax(case.logits[b, :n], dtype), labels, ends, case.window, case.blank,
                                             dtype) if n >= 1 else None)
        _refs[key] = out
    return _refs[key]


def run(case):
    from ss_asr_amd import ops
    dev = [torch.from_numpy(a).to(DEV) for a in (case.logits, case.frame_lens, case.y, case.label_lens, case.utt_ends,
                                                 case.n_utts)]
    return [t.cpu().numpy() for t in ops.ctc_segment(*dev, case.lmax, case.nmax, case.window, case.blank)]


def compare(case, got, refs, bound, min_gap=MIN_GAP):
    """The exact part asserted for every compared row; -> (rows compared, rows skipped, worst float error)."""
    path, first, last, logp, score, uf, ul, uc = got
    assert path.shape == (case.B, case.T) and first.shape == last.shape == logp.shape == (case.B, case.lmax)
    assert uf.shape == ul.shape == uc.shape == (case.B, case.nmax) and score.shape == (case.B,)
    assert path.dtype == first.dtype == uf.dtype == np.int32 and score.dtype == np.float64
    assert logp.dtype == uc.dtype == np.float32
    compared = skipped = 0
    worst = 0.0
    for b, ref in enumerate(refs):
        tag = (case.name, b)
        if ref is None:
            assert score[b] == -math.inf, tag
            assert (path[b] == -1).all() and (first[b] == -1).all() and (last[b] == -1).all() and not logp[b].any(), tag
            assert (uf[b] == -1).all() and (ul[b] == -1).all() and not uc[b].any(), tag
            compared += 1
            continue
        assert math.isfinite(score[b]), tag                     # the set of rows without a segmentation is exact
        if ref.gap < min_gap:
            skipped += 1
            continue
        n, L, N = len(ref.path), len(ref.first), len(ref.utt_first)
        assert np.array_equal(path[b, :n], ref.path) and (path[b, n:] == -1).all(), tag
        assert np.array_equal(first[b, :L], ref.first) and np.array_equal(last[b, :L], ref.last), tag
        assert (first[b, L:] == -1).all() and (last[b, L:] == -1).all() and not logp[b, L:].any(), tag
        assert np.array_equal(uf[b, :N], ref.utt_first) and np.array_equal(ul[b, :N], ref.utt_last), tag
        assert (uf[b, N:] == -1).all() and (ul[b, N:] == -1).all() and not uc[b, N:].any(), tag
        err = max(abs(float(score[b]) - ref.score), float(np.abs(logp[b, :L] - ref.char_logp).max()),
                  float(np.abs(uc[b, :N] - ref.utt_conf).max()))
        assert err <= bound, (tag, err, bound)
        worst = max(worst, err)
        compared += 1
    return compared, skipped, worst


def noise_of(case):
    """max |float32 run - float64 run| of the checker over the case's compared rows (paths that the float32 run
    moves are reported, not counted)."""
    worst = 0.0
    for b, (r64, r32) in enumerate(zip(reference(case), reference(case, np.float32))):
        if r64 is None or r64.gap < MIN_GAP:
            continue
        if r32 is None or not np.array_equal(r32.path, r64.path):
            print('%s row %d: the float32 run takes another path (gap %.3e)' % (case.name, b, r64.gap))
            continue
        worst = max(worst, abs(r32.score - r64.score), float(np.abs(r32.char_logp - r64.char_logp).max()),
                    float(np.abs(r32.utt_conf - r64.utt_conf).max()))
    return worst


def limit_cases():
    rng = np.random.default_rng(9)
    few = [int(c) for c in rng.integers(1, 7, 40)]
    many = [int(c) for c in rng.integers(1, 7, 8191)]
    for j in range(1, 8191):
        if many[j] == many[j - 1]:
            many[j] = 1 + many[j] % 6
    return [planted('long traceback', 32768, 8, few, [7, 19, 40], 20011, runs=300, window=30, long=True, seed=3),
            planted('largest lattice', 8200, 8, many, [100, 4000, 8191], 4, window=30, long=True, seed=4)]


# ------------------------------------------------------------------- tests ----
@pytest.mark.parametrize('cell', CELLS + WIDE_CELLS, ids=lambda c: 'T%d-V%d-L%d' % c[:3])
def test_cells_match_the_float64_checker(cell):
    from ss_asr_amd import ops
    case = cell_case(*cell)
    seeds = case.B
    if len(cell) == 4:
        assert ops.ctc_segment_form(case.T, case.lmax)[2] > 1                # several states per thread
    bound = 8 * WIDE_NOISE[cell[2]] if len(cell) == 4 else BOUND
    compared, skipped, worst = compare(case, run(case), reference(case), bound)
    print('%s: %d compared, %d skipped, worst |error| %.3e (bound %.3e)' % (case.name, compared, skipped, worst, bound))
    assert compared + skipped == seeds and compared >= 1 and 4 * skipped <= seeds


def test_the_cap_on_skipped_cases_holds_over_all_cells():
    skipped = total = 0
    for cell in CELLS + WIDE_CELLS:
        refs = reference(cell_case(*cell))
        here = sum(r is not None and r.gap < MIN_GAP for r in refs)
        assert here < len(refs), cell
        skipped += here
        total += len(refs)
    assert 4 * skipped <= total


def test_the_boundaries_separate_every_form():
    from ss_asr_amd import ops
    bounds = form_boundaries()
    forms = {ops.ctc_segment_form(8, lmax) for edge in bounds for lmax in (edge, edge + 1)}
    assert len(bounds) >= 3 and len(forms) == len(bounds) + 1
    assert {f[2] for f in forms} >= {1, 8, 16}
    for edge in bounds:
        f = ops.ctc_segment_form(8, edge + 1)
        assert f[1] * f[2] >= 2 * (edge + 1) + 1 > ops.ctc_segment_form(8, edge)[1] * ops.ctc_segment_form(8, edge)[2]


@pytest.mark.parametrize('part', [0, 1, 2])
def test_each_side_of_every_form_boundary(part):
    """Every third boundary per case of this test, so that each case's checker stays within a few seconds."""
    from ss_asr_amd import ops
    bounds = form_boundaries()
    for edge in bounds[part::3]:
        for lmax in (edge, edge + 1):
            case = boundary_case(lmax)
            refs = reference(case)
            assert refs[0] is not None and refs[0].gap >= MIN_GAP, (lmax, refs[0].gap)
            compared, skipped, worst = compare(case, run(case), refs, BOUND)
            print('%s (form %s): worst |error| %.3e' % (case.name, ops.ctc_segment_form(case.T, lmax), worst))
            assert (compared, skipped) == (1, 0)
            steps = np.diff(refs[0].path[refs[0].span[0]:refs[0].span[1] + 1])
            assert min((steps == 0).sum(), (steps == 1).sum(), (steps == 2).sum()) > lmax // 8      # every kind of step


@pytest.mark.parametrize('which', [0, 1], ids=['T32768-L40', 'T8200-L8191'])
def test_limit_rows(which):
    case = limit_cases()[which]
    refs = reference(case)
    assert refs[0] is not None and refs[0].gap >= MIN_GAP, refs[0].gap       # compared, not skipped
    got = run(case)
    compared, skipped, worst = compare(case, got, refs, BOUND_LONG)
    print('%s: span %s, gap %.3e, worst |error| %.3e (bound %.3e)' % (case.name, refs[0].span, refs[0].gap, worst, BOUND_LONG))
    assert (compared, skipped) == (1, 0)
    if which == 0:
        assert refs[0].span[0] == 20011 and refs[0].span[1] > 20011 + 38 * 300


def test_one_past_a_limit_is_an_argument_error():
    from ss_asr_amd import _lib, ops
    lib = _lib.load()
    assert lib.ssasr_ctc_segment_ws_bytes(1, 32769, 8, 40, 1) == 0 and lib.ssasr_ctc_segment_ws_bytes(1, 8, 8, 8192, 1) == 0
    assert lib.ssasr_ctc_segment_ws_bytes(1, 32768, 8, 8191, 1) > 0
    z = lambda *shape: torch.zeros(*shape, dtype=torch.int32, device=DEV)
    for T, lmax in ((32769, 40), (8, 8192)):
        with pytest.raises(ValueError, match='has no kernel'):
            ops.ctc_segment(torch.zeros(1, T, 8, device=DEV), z(1), z(1, lmax), z(1), z(1, 1), z(1), lmax, 1, 3)
        ws = torch.zeros(64, device=DEV, dtype=torch.float64)
        out = [torch.zeros(64, device=DEV, dtype=torch.float64) for _ in range(8)]
        args = [ops._p(ws)] * 3 + [lmax, ops._p(ws), ops._p(ws), 1, ops._p(ws), 1, T, 8, lmax, 1, 3, 0, ops._p(ws), 512]
        assert lib.ssasr_ctc_segment(*args, *[ops._p(t) for t in out], ops._stream()) == -1


def test_batches_whose_rows_differ():
    mixed, blank3 = batch_cases()
    refs = reference(mixed)
    assert [r is None for r in refs] == [False, False, False, False, True, False, True, True, True]
    total = 0
    for case in (mixed, blank3):
        compared, skipped, worst = compare(case, run(case), reference(case), BOUND)
        print('%s: %d compared, %d skipped, worst |error| %.3e' % (case.name, compared, skipped, worst))
        total += compared
        assert skipped <= 1
    assert total >= 10


@pytest.mark.parametrize('value', [0.0, 0.37])
def test_all_equal_logits_are_decided_by_the_tie_rule(value):
    """Every lp is the same negative number: the shortest path wins, among those the earliest end, and stay before
    s - 1 before s - 2 on the way back.  Rounded logits have exact ties, so the rows are compared for equality
    whatever the gap says."""
    logits = np.full((3, 9, 8), value, dtype=np.float32)
    case = make_case('ties %g' % value, 8, 9, [(9, [4, 4, 2], [1, 3]), (7, [1, 2, 3], [3]), (4, [5], [1])], logits=logits)
    refs = reference(case)
    assert refs[0].gap == 0.0 and list(refs[0].path) == [1, 2, 3, 5, -1, -1, -1, -1, -1]
    assert list(refs[1].path) == [1, 3, 5, -1, -1, -1, -1] and list(refs[2].path) == [1, -1, -1, -1]
    assert compare(case, run(case), refs, BOUND, min_gap=0.0)[:2] == (3, 0)


@pytest.mark.parametrize('L', [600, 4100], ids=['256x8', '1024x16'])
def test_all_equal_logits_with_several_states_per_thread(L):
    """The tie rule alone decides every step of a block of 8 / 16 states: four classes, so a third of the pairs are
    repeats (blank steps, disallowed skips), seven frames more than the text needs."""
    from ss_asr_amd import ops
    rng = np.random.default_rng(L)
    labels = [int(c) for c in rng.integers(1, 5, L)]
    T = L + sum(a == b for a, b in zip(labels, labels[1:])) + 7
    case = make_case('ties L %d' % L, 5, T, [(T, labels, [L // 2, L])], logits=np.full((1, T, 5), 0.25, dtype=np.float32))
    assert ops.ctc_segment_form(T, L)[2] == (8 if L == 600 else 16)
    refs = reference(case)
    assert refs[0].gap == 0.0 and refs[0].span == (0, T - 8)
    steps = np.diff(refs[0].path[:T - 7])
    assert (steps == 1).sum() > L // 4 and (steps == 2).sum() > L // 2 and (steps == 0).sum() == 0
    assert compare(case, run(case), refs, BOUND, min_gap=0.0)[:2] == (1, 0)


def test_canaries_behind_every_output_stay_intact():
    from ss_asr_amd import _lib, ops
    lib = _lib.load()
    for case in (batch_cases()[0], boundary_case(form_boundaries()[2] + 1)):            # the first x 8 form
        B, T, V, lmax, nmax = case.B, case.T, case.V, case.lmax, case.nmax
        need = int(lib.ssasr_ctc_segment_ws_bytes(B, T, V, lmax, nmax))
        ws = torch.empty(need // 8, device=DEV, dtype=torch.float64)
        dev = [torch.from_numpy(a).to(DEV) for a in (case.logits, case.frame_lens, case.y, case.label_lens,
                                                     case.utt_ends, case.n_utts)]
        pad = 64
        sizes = [B * T, B * lmax, B * lmax, B * lmax, B, B * nmax, B * nmax, B * nmax]
        kinds = [torch.int32, torch.int32, torch.int32, torch.float32, torch.float64, torch.int32, torch.int32, torch.float32]
        outs = [torch.full((n + pad,), 77, device=DEV, dtype=k) for n, k in zip(sizes, kinds)]
        rc = lib.ssasr_ctc_segment(ops._p(dev[0]), ops._p(dev[1]), ops._p(dev[2]), case.y.shape[1], ops._p(dev[3]),
                                   ops._p(dev[4]), case.utt_ends.shape[1], ops._p(dev[5]), B, T, V, lmax, nmax,
                                   case.window, case.blank, ops._p(ws), need, *[ops._p(t) for t in outs], ops._stream())
        assert rc == 0
        torch.cuda.synchronize()
        for t, n in zip(outs, sizes):
            assert bool((t[n:] == 77).all()), case.name
        shapes = [(B, T), (B, lmax), (B, lmax), (B, lmax), (B,), (B, nmax), (B, nmax), (B, nmax)]
        got = [t[:n].view(*s).cpu().numpy() for t, n, s in zip(outs, sizes, shapes)]
        compared, skipped, _ = compare(case, got, reference(case), BOUND)
        assert compared >= 1


def test_the_head_form_equals_the_plain_form_on_the_heads_logits():
    from ss_asr_amd import ops
    g = torch.Generator().manual_seed(5)
    feat = torch.randn(2, 12, 16, generator=g).to(DEV)
    weight, bias = torch.randn(10, 16, generator=g).to(DEV), torch.randn(10, generator=g).to(DEV)
    i32 = lambda rows: torch.tensor(rows, dtype=torch.int32, device=DEV)
    args = (i32([12, 9]), i32([[3, 4, 4, 7], [2, 9, 0, 0]]), i32([4, 2]), i32([[2, 4], [2, 0]]), i32([2, 1]), 4, 2, 3)
    head = ops.ctc_head_segment(feat, weight, bias, *args)
    assert len(head) == 9 and head[8].shape == (2, 12, 10)
    plain = ops.ctc_segment(head[8], *args)
    for a, b in zip(head[:8], plain):
        assert torch.equal(a, b)
    assert bool(torch.isfinite(head[4]).all())
    ref = (feat.double() @ weight.double().T + bias.double()).float()
    assert float((head[8] - ref).abs().max()) < 1e-4


def test_model_level_segmentation(golden):
    from ss_asr_amd.asr import Segment, Segmentation, input_span
    fx = golden(tgb.SMALL[0])
    asr, _ = tcd.models(fx)
    x = torch.from_numpy(fx['x']).to(DEV)
    xs, lens = [x[:, :40], x[:, :24]], [[40], [24]]
    texts = [['<he', 'y>'], ['no']]
    calls = []
    inner = asr._encode_packed
    asr._encode_packed = lambda *a: calls.append(1) or inner(*a)
    got = asr.segment(xs, lens, texts, Mapper(), window=2)
    assert calls == [1]
    path, first, last, logp, score, uf, ul, uc, logits = [t.cpu().numpy() for t in asr.last_segment]
    assert logits.shape == (2, 5, 50) and path.shape == (2, 5) and first.shape == (2, 3) and uf.shape == (2, 2)
    assert len(got) == 2 and all(isinstance(s, Segmentation) for s in got)
    for i, (utts, frames) in enumerate(((['he', 'y'], 5), (['no'], 3))):
        assert math.isfinite(got[i].score) and got[i].score == float(score[i])
        scored = np.nonzero(path[i] >= 0)[0]
        assert got[i].span == input_span(int(scored[0]), int(scored[-1]), lens[i][0]) and scored[-1] < frames
        assert [u.text for u in got[i].utterances] == utts and all(isinstance(u, Segment) for u in got[i].utterances)
        for k, u in enumerate(got[i].utterances):
            assert (u.start, u.end) == input_span(int(uf[i, k]), int(ul[i, k]), lens[i][0])
            assert (u.start, u.end) == (8 * int(uf[i, k]), 8 * int(ul[i, k]) + 8) and u.confidence == float(uc[i, k])
        text = ''.join(utts)
        assert [c[0] for c in got[i].chars] == list(text)
        for j, (c, lo_, hi_, lp) in enumerate(got[i].chars):
            assert (lo_, hi_) == input_span(int(first[i, j]), int(last[i, j]), lens[i][0]) and lp == float(logp[i, j])
        assert got[i].utterances[0].start == got[i].chars[0][1] and got[i].utterances[-1].end == got[i].chars[-1][2]
    # seconds
    secs = asr.segment(xs, lens, texts, Mapper(), window=2, frame_shift=0.01)
    assert [(u.text, round(u.start * 100), round(u.end * 100)) for u in secs[0].utterances] == \
        [(u.text, u.start, u.end) for u in got[0].utterances]
    assert round(secs[0].span[0] * 100) == got[0].span[0] and round(secs[0].span[1] * 100) == got[0].span[1]
    # encoded=: the same result without a second encode
    del calls[:]
    enc = asr._encode_packed(xs, lens)
    again = asr.segment(xs, lens, texts, Mapper(), window=2, encoded=enc)
    assert calls == [1] and again == got
    # a text the frames cannot hold
    long = asr.segment(xs, lens, [['he', 'y'], ['hello']], Mapper(), window=2)
    assert long[0] == got[0] and long[1] == Segmentation(-math.inf, None, None, None)
    # one utterance that fills its frames: the path is ASR.align's
    one = asr.segment(xs[:1], lens[:1], [['heyno']], Mapper())[0]
    ali = asr.align(xs[:1], lens[:1], ['heyno'], Mapper())[0]
    assert [c[:3] for c in one.chars] == [c[:3] for c in ali.chars] and one.span == (0, 40)
    assert abs(one.score - ali.score) < 1e-9 and all(abs(a[3] - b[3]) < 1e-6 for a, b in zip(one.chars, ali.chars))
    assert (one.utterances[0].start, one.utterances[0].end) == (0, 40)


if __name__ == '__main__':                                      # the NOISE constants and the cells' counts, on the CPU
    worst = 0.0
    for cell in CELLS:
        case = cell_case(*cell)
        refs = reference(case)
        n = noise_of(case)
        worst = max(worst, n)
        print('%-22s compared %2d skipped %2d noise %.3e' % (case.name, sum(r is None or r.gap >= MIN_GAP for r in refs),
                                                            sum(r is not None and r.gap < MIN_GAP for r in refs), n))
    for case in batch_cases() + [boundary_case(l) for l in (127, 128, 255, 256, 511, 512, 1023, 1024, 2047, 2048, 4095, 4096)]:
        n = noise_of(case)
        worst = max(worst, n)
        print('%-22s gaps %s noise %.3e' % (case.name, ['%.2e' % r.gap for r in reference(case) if r is not None], n))
    for cell in WIDE_CELLS:
        case = cell_case(*cell)
        refs = reference(case)
        n = noise_of(case)
        worst = max(worst, n)
        print('%-22s compared %2d skipped %2d noise %.3e' % (case.name, sum(r is None or r.gap >= MIN_GAP for r in refs),
                                                            sum(r is not None and r.gap < MIN_GAP for r in refs), n))
    print('NOISE %.3e (constant %.3e)' % (worst, NOISE))
    long = 0.0
    for case in limit_cases():
        n = noise_of(case)
        long = max(long, n)
        print('%-22s gap %.3e noise %.3e' % (case.name, reference(case)[0].gap, n))
    print('NOISE_LONG %.3e (constant %.3e)' % (long, NOISE_LONG))
