"""CTC segmentation with utterance skips and a filler on the GPU (ssasr_ctc_segment_skip through ops.ctc_segment /
ASR.segment) against postprocess.ctc_segment_skip_reference on float64 log_softmax values.

The rule is test_gpu_segment.py's.  A case is COMPARED when the checker's gap (the smallest margin over the decisions on
the returned path, the end choice and the filler-versus-blank choice on every junction frame of the path) is >= 1e-3;
path, spans, utt_skipped, is_fill and the set of rows without a segmentation must then be EQUAL, and score, char_logp
and utt_conf lie within 8 * NOISE of the checker's.  NOISE is the largest |float32 run - float64 run| of the checker
over a cell's compared rows, log-softmax included, per cell, measured on the CPU by running this file as a script
(`python tests/test_gpu_segment_skip.py`), which prints the figures in NOISE and the counts below.  At most a quarter
of a cell's random rows may be left out, and no cell entirely.

Cells (T, V, L, N), logits 4 * standard_normal, random utterance boundaries, skip_penalty -3, fill_penalty -1: the
issue's six, and -- as the plain kernel's test does it -- one planted recording on each side of every boundary that
ssasr_ctc_segment_form reports.  Compared of the random rows, with this file's seeds: (1,2,1,1) 16 of 16, (12,8,3,2) 16
of 16, (40,8,6,3) 16 of 16, (200,40,100,10) 15 of 16, (1500,40,600,20) 4 of 4, (4400,40,4100,40) 3 of 4; every planted
row and every boundary case is compared (gaps 0.99).

Planted rows.  On random logits a skip is rare in the wide cells and a chain rarer, so each cell's launch also holds
planted rows made as test_segment_skip_cpu.planted_frames makes them: a leading and a trailing unspoken utterance, a
chain of two, and a run of foreign frames between two utterances.  The small cells' shapes cannot hold that (one frame,
one label); their planted rows have 12 labels in 7 utterances of 8 classes, which is the same launch form.  The test
asserts that the checker's path does take a leading skip, a chain of two skips and a filler run, so that the jumping
traceback runs in every form."""
import math

import numpy as np
import pytest
import torch

import test_gpu_beam as tgb
import test_gpu_ctc_decode as tcd
import test_gpu_segment as tgs
from test_segment_skip_cpu import planted_frames, text_of

pytestmark = pytest.mark.gpu

DEV = tgs.DEV
MIN_GAP = tgs.MIN_GAP
SKIP, FILL = -3.0, -1.0
NEG = -math.inf
CELLS = [(1, 2, 1, 1, 16), (12, 8, 3, 2, 16), (40, 8, 6, 3, 16), (200, 40, 100, 10, 16), (1500, 40, 600, 20, 4),
         (4400, 40, 4100, 40, 4)]
# max |float32 run - float64 run| of the checker per cell (its random and its planted rows) and over the boundary cases
# (measured: 8.28e-7, 2.01e-6, 1.52e-6, 5.41e-6, 3.05e-5, 8.86e-5; boundaries 2.46e-4 at 4,096 labels).  They are far below
# the plain kernel's: with skips at -3 the best path of random logits passes over most of the text and scores little.
# 'junction': the row of 1,019 skips in a row, whose float32 score of -3,057 carries 1.33e-2.
NOISE = {1: 8.3e-7, 3: 2.1e-6, 6: 1.6e-6, 100: 5.5e-6, 600: 3.1e-5, 4100: 8.9e-5, 'boundary': 2.5e-4, 'junction': 1.4e-2}


def split_n(rng, L, N):
    cuts = sorted(rng.choice(np.arange(1, L), size=N - 1, replace=False).tolist()) if N > 1 else []
    return [int(c) for c in cuts] + [L]


def planted_row(V, L, N, seed):
    """(T, logits [T, V], labels, ends, absent) of a planted recording with L labels in N >= 7 utterances: utterances
    0, 2, 3 and N - 1 are absent, three foreign frames follow utterance 4."""
    rng = np.random.default_rng(seed)
    labels = [int(c) for c in rng.integers(1, V - 2, L)]
    ends = split_n(rng, L, N)
    utts = [labels[a:b] for a, b in zip([0] + ends, ends)]
    absent = (0, 2, 3, N - 1)
    frames, _, _ = planted_frames(V, utts, absent=absent, foreign_after=4)
    x = rng.standard_normal((len(frames), V)).astype(np.float32)
    x[np.arange(len(frames)), frames] += 12.0
    return len(frames), x, labels, ends, absent


def build(name, V, rows, logits, window=30, blank=0):
    """rows: [(frame_len, labels, ends)], logits: one [T_b, V] per row; padded to the longest with noise."""
    T = max(x.shape[0] for x in logits)
    full = (4.0 * np.random.default_rng(len(name)).standard_normal((len(rows), T, V))).astype(np.float32)
    for b, x in enumerate(logits):
        full[b, :x.shape[0]] = x
    return tgs.make_case(name, V, T, rows, blank=blank, window=window, logits=full)


_cases = {}
# With skips on, random logits leave many near-ties (about four rows in ten of the wide cells have a gap below 1e-3), and
# the 600-label cell's first seeds left two of four out; its seeds start 500 further on, where the float64 checker alone
# compares four of four.
SEED_OFFSET = {600: 500}


def cell_case(T, V, L, N, seeds):
    """The cell's random rows: a repeated first pair in every second seed."""
    key = (T, V, L, N)
    if key not in _cases:
        rows, logits = [], []
        for seed in range(seeds):
            rng = np.random.default_rng(7000 * T + 10 * L + SEED_OFFSET.get(L, 0) + seed)
            labels = [int(c) for c in rng.integers(1, V, L)]
            if seed % 2 and L >= 2:
                labels[1] = labels[0]
            rows.append((T, labels, split_n(rng, L, N)))
            logits.append((4.0 * rng.standard_normal((T, V))).astype(np.float32))
        _cases[key] = build('skip cell %s' % (key,), V, rows, logits, window=1 + T // 7)
    return _cases[key]


def planted_case(T, V, L, N, seeds):
    """The cell's two planted rows, in the cell's launch form."""
    key = ('planted', T, V, L, N)
    if key not in _cases:
        made = [planted_row(max(V, 8), max(L, 12), max(N, 7), 31 * L + seed) for seed in (0, 2)]
        _cases[key] = build('skip planted %s' % ((T, V, L, N),), max(V, 8), [(m[0], m[2], m[3]) for m in made],
                            [m[1] for m in made], window=1 + T // 7)
    return _cases[key]


def boundary_case(lmax):
    pt, x, labels, ends, _ = planted_row(8, lmax, 9, lmax)
    case = build('skip boundary %d' % lmax, 8, [(pt, labels, ends)], [x])
    return case


_refs = {}


def reference(case, dtype=np.float64, skip=SKIP, fill=FILL):
    from ss_asr_amd.postprocess import ctc_segment_skip_reference
    key = (case.name, np.dtype(dtype).name, skip, fill)
    if key not in _refs:
        out = []
        for b, (n, labels, ends) in enumerate(case.rows):
            n = min(n, case.T)
            out.append(ctc_segment_skip_reference(tgs.log_softmax(case.logits[b, :n], dtype), labels, ends, case.window,
                                                  skip, fill, case.blank, dtype) if n >= 1 else None)
        _refs[key] = out
    return _refs[key]


def run(case, skip=SKIP, fill=FILL, plain=False):
    from ss_asr_amd import ops
    dev = [torch.from_numpy(a).to(DEV) for a in (case.logits, case.frame_lens, case.y, case.label_lens, case.utt_ends,
                                                 case.n_utts)]
    if plain:
        return [t.cpu().numpy() for t in ops.ctc_segment(*dev, case.lmax, case.nmax, case.window, case.blank)]
    return [t.cpu().numpy() for t in ops.ctc_segment(*dev, case.lmax, case.nmax, case.window, case.blank,
                                                     skip_penalty=skip, fill_penalty=fill)]


def compare(case, got, refs, bound, min_gap=MIN_GAP):
    """test_gpu_segment.compare on the eight shared outputs, then utt_skipped and is_fill."""
    counts = tgs.compare(case, got[:8], refs, bound, min_gap)
    us, fl = got[8], got[9]
    assert us.shape == (case.B, case.nmax) and fl.shape == (case.B, case.T) and us.dtype == fl.dtype == np.int32
    for b, ref in enumerate(refs):
        tag = (case.name, b)
        if ref is None:
            assert (us[b] == -1).all() and (fl[b] == -1).all(), tag
        elif ref.gap >= min_gap:
            n, N = len(ref.path), len(ref.utt_skipped)
            assert np.array_equal(us[b, :N], ref.utt_skipped) and (us[b, N:] == -1).all(), tag
            assert np.array_equal(fl[b, :n], ref.is_fill) and (fl[b, n:] == -1).all(), tag
    return counts


def takes_everything(ref, ends, absent):
    """The planted path: the absent utterances skipped (a leading one, a chain of two, a trailing one), and a filler
    run of three frames."""
    a, e = ref.span
    steps = list(zip(ref.path[a:e], ref.path[a + 1:e + 1]))
    junc = [0] + [2 * x for x in ends]
    jumps = [junc.index(q) for p, q in steps if p in junc and q in junc and junc.index(q) == junc.index(p) + 1
             and q - p >= 2]
    fill = np.nonzero(ref.is_fill == 1)[0]
    return (sorted(jumps) == [x + 1 for x in sorted(absent)] and ref.path[a] == 0 and ref.path[a + 1] == junc[1]
            and list(ref.utt_skipped) == [int(n in absent) for n in range(len(ends))]
            and len(fill) == 3 and fill[2] - fill[0] == 2)


def noise_of(case):
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


# ------------------------------------------------------------------- tests ----
@pytest.mark.parametrize('cell', CELLS, ids=lambda c: 'T%d-V%d-L%d-N%d' % c[:4])
def test_cells_match_the_float64_checker(cell):
    from ss_asr_amd import ops
    case, plant = cell_case(*cell), planted_case(*cell)
    assert ops.ctc_segment_form(case.T, case.lmax)[1:] == ops.ctc_segment_form(plant.T, plant.lmax)[1:]   # one form
    refs, prefs = reference(case), reference(plant)
    seeds = case.B
    left_out = sum(r is not None and r.gap < MIN_GAP for r in refs)
    assert 4 * left_out <= seeds and left_out < seeds            # the cap, on the float64 checker alone
    for b, r in enumerate(prefs):                                # the planted rows are compared and take every move
        assert r is not None and r.gap >= MIN_GAP, (b, r.gap)
        assert takes_everything(r, plant.rows[b][2], (0, 2, 3, len(plant.rows[b][2]) - 1)), b
    bound = 8 * NOISE[cell[2]]
    compared, skipped, worst = compare(case, run(case), refs, bound)
    pc, ps, pw = compare(plant, run(plant), prefs, bound)
    print('%s: %d compared, %d left out, %d rows with a skip, worst |error| %.3e, planted %.3e (bound %.3e)'
          % (case.name, compared, skipped, sum(r is not None and r.utt_skipped.any() for r in refs), worst, pw, bound))
    assert compared + skipped == seeds and skipped == left_out and (pc, ps) == (2, 0)


@pytest.mark.parametrize('part', [0, 1, 2])
def test_each_side_of_every_form_boundary(part):
    from ss_asr_amd import ops
    bounds = tgs.form_boundaries()
    assert len(bounds) == 6
    for edge in bounds[part::3]:
        for lmax in (edge, edge + 1):
            case = boundary_case(lmax)
            refs = reference(case)
            assert refs[0] is not None and refs[0].gap >= MIN_GAP, (lmax, refs[0].gap)
            assert takes_everything(refs[0], case.rows[0][2], (0, 2, 3, 8))
            compared, skipped, worst = compare(case, run(case), refs, 8 * NOISE['boundary'])
            print('%s (form %s): worst |error| %.3e' % (case.name, ops.ctc_segment_form(case.T, lmax), worst))
            assert (compared, skipped) == (1, 0)


@pytest.mark.parametrize('cell', CELLS, ids=lambda c: 'T%d-V%d-L%d-N%d' % c[:4])
def test_with_both_penalties_off_every_output_is_the_plain_kernels(cell):
    """ssasr_ctc_segment_skip with -inf, -inf (straight through the C entry: ops takes None for off and then calls the
    plain entry) against ssasr_ctc_segment, bit for bit."""
    from ss_asr_amd import _lib, ops
    lib = _lib.load()
    case = cell_case(*cell)
    plain = run(case, plain=True)
    got = call_entry(lib, ops, case, NEG, NEG)[0]
    for a, b in zip(plain, got[:8]):
        assert a.tobytes() == b.tobytes()
    seg = np.isfinite(got[4])
    assert seg.any()
    for b in range(case.B):
        N = int(case.n_utts[b])
        if seg[b]:
            assert (got[8][b, :N] == 0).all() and (got[8][b, N:] == -1).all()
            assert ((got[9][b] == 0) == (got[0][b] >= 0)).all() and ((got[9][b] == -1) == (got[0][b] < 0)).all()
        else:
            assert (got[8][b] == -1).all() and (got[9][b] == -1).all()


def call_entry(lib, ops, case, skip, fill, pad=64, fillv=77):
    """The C entry with canaries behind every output and the workspace -> (outputs cut to size, canaries intact)."""
    import ctypes
    B, T, V, lmax, nmax = case.B, case.T, case.V, case.lmax, case.nmax
    need = int(lib.ssasr_ctc_segment_skip_ws_bytes(B, T, V, lmax, nmax))
    ws = torch.full((need // 8 + pad,), 77.0, device=DEV, dtype=torch.float64)
    dev = [torch.from_numpy(a).to(DEV) for a in (case.logits, case.frame_lens, case.y, case.label_lens, case.utt_ends,
                                                 case.n_utts)]
    sizes = [B * T, B * lmax, B * lmax, B * lmax, B, B * nmax, B * nmax, B * nmax, B * nmax, B * T]
    kinds = [torch.int32, torch.int32, torch.int32, torch.float32, torch.float64, torch.int32, torch.int32, torch.float32,
             torch.int32, torch.int32]
    outs = [torch.full((n + pad,), fillv, device=DEV, dtype=k) for n, k in zip(sizes, kinds)]
    pens = (ctypes.c_double * 2)(skip, fill)
    rc = lib.ssasr_ctc_segment_skip(ops._p(dev[0]), ops._p(dev[1]), ops._p(dev[2]), case.y.shape[1], ops._p(dev[3]),
                                    ops._p(dev[4]), case.utt_ends.shape[1], ops._p(dev[5]), B, T, V, lmax, nmax,
                                    case.window, case.blank, ctypes.addressof(pens), ctypes.addressof(pens) + 8,
                                    ops._p(ws), need, *[ops._p(t) for t in outs], ops._stream())
    assert rc == 0
    torch.cuda.synchronize()
    intact = all(bool((t[n:] == fillv).all()) for t, n in zip(outs, sizes)) and bool((ws[need // 8:] == 77.0).all())
    shapes = [(B, T), (B, lmax), (B, lmax), (B, lmax), (B,), (B, nmax), (B, nmax), (B, nmax), (B, nmax), (B, T)]
    return [t[:n].view(*s).cpu().numpy() for t, n, s in zip(outs, sizes, shapes)], intact


def edge_batch(blank=0):
    """Unequal rows: a planted row, rows with frame_lens 0 and past T, malformed utt_ends, an empty text, a text that
    the frames can hold only with a skip.  blank != 0: the same batch with classes 0 and `blank` exchanged."""
    pt, x, labels, ends, _ = planted_row(8, 14, 7, 6)
    rng = np.random.default_rng(3)
    lab = lambda L: [int(c) for c in rng.integers(1, 6, L)]
    rows = [(pt, labels, ends), (0, lab(3), [1, 3]), (pt + 50, lab(5), [2, 5]), (20, lab(4), [2, 2, 4]), (20, lab(4), [3, 2, 4]),
            (20, lab(4), [2, 3]), (20, [], []), (3, [1, 1, 2, 3], [1, 4]), (1, [2], [1]), (9, lab(6), [1, 2, 3, 4, 5, 6])]
    logits = [x] + [(4.0 * rng.standard_normal((max(min(r[0], pt), 1), 8))).astype(np.float32) for r in rows[1:]]
    if blank:
        rows = [(n, [0 if c == blank else c for c in l], e) for n, l, e in rows]
        for a in logits:
            a[:, [0, blank]] = a[:, [blank, 0]]
    return build('skip edges blank %d' % blank, 8, rows, logits, window=4, blank=blank)


@pytest.mark.parametrize('blank', [0, 3])
def test_edges_canaries_and_every_element_written(blank):
    from ss_asr_amd import _lib, ops
    lib = _lib.load()
    case = edge_batch(blank)
    refs = reference(case)
    assert [r is None for r in refs] == [False, True, False, True, True, True, True, False, False, False]
    assert refs[7].utt_skipped.any()                             # three frames hold [1 1 2 3] only with a skip
    got, intact = call_entry(lib, ops, case, SKIP, FILL)
    assert intact
    again, _ = call_entry(lib, ops, case, SKIP, FILL, fillv=-9)  # every element written: no canary value shows through
    for a, b in zip(got, again):
        assert a.tobytes() == b.tobytes()
    assert refs[0].gap >= MIN_GAP and takes_everything(refs[0], case.rows[0][2], (0, 2, 3, 6))   # the planted row counts
    left_out = sum(r is not None and r.gap < MIN_GAP for r in refs)
    compared, skipped, worst = compare(case, got, refs, 8 * NOISE['boundary'])
    assert (compared, skipped) == (case.B - left_out, left_out) and left_out <= 1
    # a recording alone is bit-equal to itself in the group
    for b in (0, 7, 9):
        n, labels, ends = case.rows[b]
        alone = build('alone %d %d' % (blank, b), 8, [case.rows[b]], [case.logits[b, :min(n, case.T)]], window=4, blank=blank)
        one = run(alone)
        L, N, T1 = len(labels), len(ends), alone.T
        assert one[0][0].tobytes() == got[0][b, :T1].tobytes() and one[9][0].tobytes() == got[9][b, :T1].tobytes()
        for k in (1, 2, 3):
            assert one[k][0, :L].tobytes() == got[k][b, :L].tobytes()
        for k in (5, 6, 7, 8):
            assert one[k][0, :N].tobytes() == got[k][b, :N].tobytes()
        assert one[4][0] == got[4][b]


def test_the_largest_utterance_count_at_a_small_t():
    """Nmax = 1,024 at T = 40, one label per utterance: a text of 1,024 utterances cannot be passed in 40 frames (a
    skip costs a frame), one of 30 can, and has to skip."""
    rng = np.random.default_rng(11)
    labels = [int(c) for c in rng.integers(1, 8, 1024)]
    x = (4.0 * rng.standard_normal((2, 40, 8))).astype(np.float32)
    case = build('skip nmax 1024', 8, [(40, labels, list(range(1, 1025))), (40, labels[:30], list(range(1, 31)))],
                 list(x), window=5)
    assert case.nmax == 1024 and case.lmax == 1024
    refs = reference(case, skip=-0.25)
    assert refs[0] is None and refs[1] is not None and refs[1].utt_skipped.sum() >= 3 and refs[1].gap >= MIN_GAP
    got = run(case, skip=-0.25)
    compared, skipped, worst = compare(case, got, refs, 8 * NOISE['boundary'])
    assert (compared, skipped) == (2, 0) and (got[8][0] == -1).all() and (got[8][1, 30:] == -1).all()


def junction_case():
    rng = np.random.default_rng(12)
    labels = [1 + (j % 5) for j in range(1024)]                 # no adjacent repeats
    frames, spans, _ = planted_frames(8, [[c] for c in labels], absent=tuple(range(1019)))
    x = rng.standard_normal((len(frames), 8)).astype(np.float32)
    x[np.arange(len(frames)), frames] += 12.0
    case = build('skip junction 1024', 8, [(len(frames), labels, list(range(1, 1025)))], [x], window=5)
    case.spans = spans
    return case


def test_the_last_slots_of_the_junction_table_on_a_real_path():
    """1,024 utterances of one label, the first 1,019 never spoken: the path starts in J_0, takes 1,019 skips in a row
    (1,020 blank frames) and aligns the last five, so every slot of the LDS table up to J_1024 carries a value that
    the path depends on."""
    case = junction_case()
    assert case.nmax == 1024
    spans = case.spans
    refs = reference(case)
    assert refs[0].gap >= MIN_GAP and refs[0].utt_skipped.sum() == 1019 and list(refs[0].utt_skipped[1019:]) == [0] * 5
    assert (int(refs[0].utt_first[1023]), int(refs[0].utt_last[1023])) == spans[1023]
    compared, skipped, worst = compare(case, run(case), refs, 8 * NOISE['junction'])
    print('%s: worst |error| %.3e' % (case.name, worst))
    assert (compared, skipped) == (1, 0)


def test_model_level_segmentation_with_an_invented_utterance(golden):
    """The small joint model's OWN transcript of the recording -- its CTC best path, collapsed; cut in two utterances
    when it has two characters or more -- with one invented utterance inserted behind the first: two characters that
    the path does not contain, the two least likely of the head.  Nothing here is conditional: the float64 checker on
    the logits the kernel saw must skip the invented utterance and only it, with a clear gap, and ASR.segment must say
    the same, keep the others within a frame of the plain call on the true transcript, and report the checker's
    filler runs.  (The seeded model's best path is one character, 'r', in frame 0 of 5; the invented utterance then
    trails it, the path is r, junction, landing frame, and the two junction frames are filler: checker gap 4.4e-3.)"""
    from ss_asr_amd import ops
    from ss_asr_amd.asr import Segment, input_span
    from ss_asr_amd.postprocess import ctc_segment_skip_reference
    mapper = tgs.Mapper()
    fx = golden(tgb.SMALL[0])
    asr, _ = tcd.models(fx)
    x = torch.from_numpy(fx['x']).to(DEV)
    xs, lens = [x[:, :40]], [[40]]
    asr.segment(xs, lens, [['a']], mapper, window=2)            # any text: the head's logits
    lp = tgs.log_softmax(asr.last_segment[8][0].cpu().numpy())
    best = lp.argmax(1)
    own = [int(c) for t, c in enumerate(best) if c != ops.CTC_BLANK and (t == 0 or best[t - 1] != c)]
    assert own and all(c >= 2 for c in own)
    ids = [own] if len(own) < 2 else [own[:len(own) // 2], own[len(own) // 2:]]
    invented = [int(c) for c in np.argsort(lp.sum(0)) if c >= 2 and c not in own][:2]
    truth = [''.join(mapper.ind_to_char(c) for c in u) for u in ids]
    texts = truth[:1] + [''.join(mapper.ind_to_char(c) for c in invented)] + truth[1:]
    want = [0, 1] + [0] * (len(ids) - 1)
    plain = asr.segment(xs, lens, [truth], mapper, window=2)[0]
    got = asr.segment(xs, lens, [texts], mapper, window=2, skip_penalty=SKIP, fill_penalty=FILL)[0]
    assert len(asr.last_segment) == 11 and asr.last_segment[8].shape == (1, len(texts)) and asr.last_segment[9].shape == (1, 5)
    y, ends = text_of(ids[:1] + [invented] + ids[1:])
    ref = ctc_segment_skip_reference(tgs.log_softmax(asr.last_segment[10][0].cpu().numpy()), y, ends, 2, SKIP, FILL,
                                     ops.CTC_BLANK)
    print('own %r, texts %r, gap %.3e, path %s, is_fill %s' % (truth, texts, ref.gap, list(ref.path), list(ref.is_fill)))
    assert ref is not None and list(ref.utt_skipped) == want and ref.gap >= MIN_GAP
    assert all(isinstance(u, Segment) for u in got.utterances) and [u.text for u in got.utterances] == texts
    assert [u.skipped for u in got.utterances] == [bool(k) for k in want]
    assert (got.utterances[1].start, got.utterances[1].end, got.utterances[1].confidence) == (None, None, 0.0)
    assert all(c[1:] == (None, None, 0.0) for c in got.chars[len(ids[0]):len(ids[0]) + 2])
    kept = [u for u in got.utterances if not u.skipped]
    assert len(kept) == len(plain.utterances)
    for k, (u, p) in enumerate(zip(kept, plain.utterances)):     # within one encoder frame of the plain call
        assert u.text == p.text and abs(u.start - p.start) <= 8 and abs(u.end - p.end) <= 8
        n = [0] + [m for m in range(2, len(texts))]
        assert (u.start, u.end) == input_span(int(ref.utt_first[n[k]]), int(ref.utt_last[n[k]]), 40)
    # the filler runs are the checker's is_fill runs, as input spans
    fill = [int(t) for t in np.nonzero(ref.is_fill == 1)[0]]
    runs = [(t, u) for t, u in zip([t for t in fill if t - 1 not in fill], [t for t in fill if t + 1 not in fill])]
    assert fill and got.fillers == [input_span(lo, hi, 40) for lo, hi in runs]
    assert np.array_equal(asr.last_segment[9][0].cpu().numpy(), ref.is_fill)
    secs = asr.segment(xs, lens, [texts], mapper, window=2, skip_penalty=SKIP, fill_penalty=FILL, frame_shift=0.01)[0]
    assert [u.skipped for u in secs.utterances] == [u.skipped for u in got.utterances]
    assert [(round(a * 100), round(b * 100)) for a, b in secs.fillers] == got.fillers
    # both None: the plain call, field for field
    assert asr.segment(xs, lens, [truth], mapper, window=2, skip_penalty=None, fill_penalty=None)[0] == plain
    assert plain.fillers is None and not any(u.skipped for u in plain.utterances)


if __name__ == '__main__':                                      # the NOISE constants and the cells' counts, on the CPU
    import sys
    for cell in CELLS if len(sys.argv) < 2 else [c for c in CELLS if c[2] <= int(sys.argv[1])]:
        case, plant = cell_case(*cell), planted_case(*cell)
        refs, prefs = reference(case), reference(plant)
        print('%-36s compared %2d of %2d random rows, rows with a skip %2d, planted gaps %s (all moves: %s), noise %.3e '
              'planted %.3e (constant %.3e)'
              % (case.name, sum(r is None or r.gap >= MIN_GAP for r in refs), case.B,
                 sum(r is not None and bool(r.utt_skipped.any()) for r in refs), ['%.2e' % r.gap for r in prefs],
                 [takes_everything(r, plant.rows[b][2], (0, 2, 3, len(plant.rows[b][2]) - 1)) for b, r in enumerate(prefs)],
                 noise_of(case), noise_of(plant), NOISE[cell[2]]), flush=True)
    worst = 0.0
    for lmax in (127, 128, 255, 256, 511, 512, 1023, 1024, 2047, 2048, 4095, 4096):
        if len(sys.argv) >= 2 and lmax > int(sys.argv[1]):
            continue
        case = boundary_case(lmax)
        n = noise_of(case)
        worst = max(worst, n)
        print('%-36s gap %.3e noise %.3e' % (case.name, reference(case)[0].gap, n), flush=True)
    print('boundary NOISE %.3e (constant %.3e)' % (worst, NOISE['boundary']))
    print('junction NOISE %.3e (constant %.3e)' % (noise_of(junction_case()), NOISE['junction']))
