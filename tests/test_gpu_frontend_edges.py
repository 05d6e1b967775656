"""The log-mel frontend (csrc/frontend.hip: ssasr_logmel per utterance, ssasr_logmel_batch for a list) at its signal,
rate and batch edges against the float64 oracle (oracle/frontend_oracle.py::log_fbank, fed the same float32-rounded
waveform), with bounds MEASURED on the CPU: oracle/frontend_oracle.py::log_fbank_f32 restates the kernels' arithmetic
in float32 (float32 constants, sums accumulated sequentially over k); its largest error against the oracle over
every case of this file, times four, is the bound (the factor covers fused against separately rounded products and
the order of the sums inside a tile).

Metric, per frame f with P = exp(feature):  err_f = max_m |P_got - P_ref| / max_m P_ref[f, :]  -- the frame's OWN
peak (at least eps, never zero), so a quiet frame next to a loud one, or a reflect-padded edge frame, is held to its
own scale; on bands with P_ref >= 1e-3 of the frame's peak also |got - want| in the log domain.

The CPU tests of this file pin the preconditions (the oracle's reflection is the kernels' fold rule, the host-side
frame / row counts, the restatement inside a quarter of the bounds) and show that the cases have teeth: three
one-line faults in the RESTATEMENT (never in a kernel) fail many cases by orders of magnitude."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import frontend_oracle as fo

# Measured on the CPU (measure_cpu() below, every case of this file: CASES of all eight settings and every utterance
# of BATCH_LISTS at its three rates, both forms of the restatement) against the float64 oracle:
#   largest err_f                       2.907e-06   (44100 Hz / 80 mels, single form, list 'many_300', utterance 32)
#   largest log-domain error (strong)   8.516e-06   (44100 Hz / 80 mels, batch form, case 'ramp_long')
# (per setting the largest err_f lies between 1.95e-06 and 2.91e-06: mostly the float32 rounding of the log itself --
# half an ulp of a log near -36 is 1.9e-06, and P = exp(log) carries it -- on top of the float32 sums; the log-domain
# figure is the sums' error on bands a thousand times below the frame's peak.)  The bounds are four times the maxima,
# rounded up in the third digit: 1.164e-05 and 3.408e-05; tests/test_frontend.py allows 2e-3 in both.
CPU_MAX_POW, CPU_MAX_LOG = 2.91e-06, 8.52e-06
BOUND_POW, BOUND_LOG = 4 * CPU_MAX_POW, 4 * CPU_MAX_LOG

RATES = [(8000, 40), (11025, 40), (16000, 80), (22050, 80), (44100, 80), (48000, 40), (22050, 13), (44100, 23)]
BATCH_RATES = [(16000, 80), (22050, 80), (44100, 80)]
EPS = np.finfo(float).eps
EARG = -1                                      # SSASR_EARG (csrc/common.h)


def geometry(sr):
    return int(sr * 0.025), int(sr * 0.010)    # n_fft, hop


def lengths(sr):
    n_fft, hop = geometry(sr)
    return [1, 2, 3, hop - 1, hop, hop + 1, n_fft // 2 - 1, n_fft // 2, n_fft // 2 + 1, n_fft - 1, n_fft, n_fft + 1,
            5 * hop - 1, 5 * hop, 5 * hop + 1, 5 * hop + 2]


def noise(n, *seed):
    return np.random.default_rng([int(s) for s in seed] + [n]).standard_normal(n)


@functools.lru_cache(maxsize=None)
def cases(sr):
    """{name: float32 waveform}: every per-rate case of the issue (at most 0.25 s each)."""
    n_fft, hop = geometry(sr)
    out = {}
    for n in lengths(sr):
        out['len%d' % n] = 0.3 * noise(n, sr, 1)
    # edge-sensitive content, once shorter than the pad (folds more than once) and once a few frames long
    for tag, n in (('short', hop + 1), ('long', n_fft + hop + 1)):
        for pos in (0, 1, n - 2, n - 1):
            y = np.zeros(n)
            y[pos] = 1.0
            out['imp%d_%s' % (pos if pos < 2 else pos - n, tag)] = y
        out['ramp_' + tag] = np.linspace(-0.7, 0.9, n)
        out['partsine_' + tag] = 0.8 * np.sin(2 * np.pi * 0.8 * np.arange(n) / n + 0.3)     # 0.8 of a period
    t = np.arange(8 * hop)
    out['zeros_tone_zeros'] = np.concatenate([np.zeros(5 * hop), 0.9 * np.sin(2 * np.pi * t / 10.0), np.zeros(5 * hop)])
    base = noise(3 * hop + 7, sr, 2)
    for amp in (1e-9, 1e-4, 1.0, 32767.0):
        out['amp%g' % amp] = amp * base
    out['dc'] = np.full(4 * hop + 1, 0.5)
    out = {k: v.astype(np.float32) for k, v in out.items()}
    assert max(len(v) for v in out.values()) <= 0.25 * sr
    return out


@functools.lru_cache(maxsize=None)
def batch_lists(sr):
    """{name: [float32 waveforms]}: the batch-layout lists of the issue."""
    n_fft, hop = geometry(sr)
    body = [0.3 * noise(3 * hop + 5, sr, 3), 0.3 * noise(n_fft + 3, sr, 4)]
    loud = 32767.0 * noise(2 * hop + 3, sr, 8)
    out = {
        'last_1': body + [0.3 * noise(1, sr, 5)],
        'last_2': body + [0.3 * noise(2, sr, 5)],
        'last_hop': body + [0.3 * noise(hop, sr, 5)],
        'longest_last': [0.3 * noise(hop + 1, sr, 6), 0.3 * noise(2, sr, 6), 0.3 * noise(5 * hop + 1, sr, 6),
                         0.3 * noise(int(0.25 * sr), sr, 6)],
        'longest_middle': [0.3 * noise(hop, sr, 7), 0.3 * noise(int(0.2 * sr), sr, 7), 0.3 * noise(3, sr, 7)],
        'one_sample_alone': [0.3 * noise(1, sr, 5)],
        'many_300': [0.3 * noise(hop + (1 if i % 3 else -1), sr, 100 + i) for i in range(300)],
        'loud_quiet_loud': [loud, 1e-6 * noise(2 * hop + 3, sr, 9), loud[::-1].copy()],
        'long_3s_then_3': [0.3 * noise(3 * sr, sr, 10), 0.3 * noise(3, sr, 10)],
    }
    return {k: [w.astype(np.float32) for w in v] for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def oracle(sr, n_mels, name, idx=None):
    """The float64 reference of one case, computed once and shared (read-only)."""
    y = cases(sr)[name] if idx is None else batch_lists(sr)[name][idx]
    want = fo.log_fbank(y.astype(np.float64), sr, n_mels)
    want.setflags(write=False)
    return want


def frame_metric(got, want):
    """(err_f [frames], largest log-domain error on the strong bands of each frame [frames])."""
    got = np.asarray(got, dtype=np.float64)
    p_got, p_ref = np.exp(got), np.exp(want)
    peak = p_ref.max(axis=1)
    assert (peak >= EPS * (1 - 1e-12)).all()
    err = np.abs(p_got - p_ref).max(axis=1) / peak
    strong = p_ref >= 1e-3 * peak[:, None]
    return err, np.where(strong, np.abs(got - want), 0.0).max(axis=1)


def zero_frames(y, sr):
    """Frames of y whose whole (reflect-padded) window holds exact zeros."""
    n_fft, hop = geometry(sr)
    padded = np.pad(np.abs(y.astype(np.float64)), n_fft // 2, mode='reflect')
    return [f for f in range(fo.n_frames(len(y), sr)) if padded[f * hop:f * hop + n_fft].max() == 0.0]


class Worst:
    """Largest figures a test saw, printed as one line (profiles/frontend_edges.txt is made of these lines)."""

    def __init__(self, label):
        self.label, self.pow, self.log, self.pow_at, self.log_at = label, 0.0, 0.0, '', ''

    def check(self, got, want, where):
        assert got.shape == want.shape, (where, got.shape, want.shape)      # the oracle's frame count
        assert got.dtype == np.float32 and np.isfinite(got).all(), where
        err, lerr = frame_metric(got, want)
        if err.max() > self.pow:
            self.pow, self.pow_at = float(err.max()), '%s frame %d' % (where, int(err.argmax()))
        if lerr.max() > self.log:
            self.log, self.log_at = float(lerr.max()), '%s frame %d' % (where, int(lerr.argmax()))
        return err, lerr

    def report(self):
        print('frontend_edges %s: worst err_f %.3e (%s), worst log %.3e (%s); bounds %.3e / %.3e'
              % (self.label, self.pow, self.pow_at, self.log, self.log_at, BOUND_POW, BOUND_LOG))


def assert_case(worst, got, want, where, y=None, sr=None):
    err, lerr = worst.check(got, want, where)
    # the first and the last frame are the reflect-padded ones: a repeated or dropped edge sample, or a fold shifted by
    # one, shows there first -- named separately so that a failure says which edge it was
    assert err[0] <= BOUND_POW and lerr[0] <= BOUND_LOG, (where, 'first frame', err[0], lerr[0])
    assert err[-1] <= BOUND_POW and lerr[-1] <= BOUND_LOG, (where, 'last frame', err[-1], lerr[-1])
    assert err.max() <= BOUND_POW, (where, 'frame %d' % err.argmax(), err.max())
    assert lerr.max() <= BOUND_LOG, (where, 'frame %d' % lerr.argmax(), lerr.max())
    if y is not None:
        # digital silence: log(eps) in every band, as float32 holds it (the spacing of float32 at 36 is 3.8e-6, so
        # "to 1e-6" of the float32 value is that very float32)
        zf = zero_frames(y, sr)
        assert len(zf) >= 3, where
        assert np.abs(got[zf].astype(np.float64) - float(np.float32(np.log(EPS)))).max() <= 1e-6, where


# ------------------------------------------------------------------------------------------------ CPU: preconditions
def test_oracle_reflection_is_the_kernels_fold_rule():
    """numpy.pad(..., 'reflect') -- what the oracle pads with -- equals the fold rule both kernels state (period
    2 (n - 1), negative wrap, i >= n -> period - i, n == 1 -> sample 0), also where the pad is many periods long."""
    for n in (1, 2, 3, 5, 79, 100, 275, 276):
        for pad in (7, 275, 600):
            y = np.arange(1.0, n + 1)
            assert np.array_equal(np.pad(y, pad, mode='reflect'), y[fo.fold(np.arange(-pad, n + pad), n)]), (n, pad)


@pytest.mark.parametrize('sr,n_mels', RATES[:6])
def test_host_frame_and_row_counts_match_the_oracles_framing(sr, n_mels):
    """ssasr_logmel_frames / ssasr_logmel_batch_rows (host code: the library loads without a device) against the
    oracle's framing (numpy's padded length cut into hops) for n = 1 .. 3 hop + n_fft: the count changes at k hop for
    an even window and at k hop + 1 for an odd one; an utterance's rows hold every sample its frames read."""
    from ss_asr_amd import _lib
    lib = _lib.load()
    n_fft, hop = geometry(sr)
    changes = []
    for n in range(1, 3 * hop + n_fft + 1):
        want = 1 + (len(np.pad(np.zeros(n), n_fft // 2, mode='reflect')) - n_fft) // hop
        frames, rows = lib.ssasr_logmel_frames(n, n_fft, hop), lib.ssasr_logmel_batch_rows(n, n_fft, hop)
        assert frames == want == fo.n_frames(n, sr), (n, frames, want)
        assert rows >= frames and rows * hop >= (frames - 1) * hop + n_fft, (n, rows, frames)
        if n > 1 and frames != lib.ssasr_logmel_frames(n - 1, n_fft, hop):
            changes.append(n)
    assert changes[:3] == [k * hop + n_fft % 2 for k in (1, 2, 3)], changes[:3]
    assert lib.ssasr_logmel_frames(0, n_fft, hop) == 0 and lib.ssasr_logmel_frames(5, 1, hop) == 0
    assert lib.ssasr_logmel_batch_rows(5, n_fft, 0) == 0


def restatement_worst(sr, n_mels, form, fault=None, only=None):
    """{case: (largest err_f, largest strong-band log error)} of the float32 restatement against the oracle."""
    out = {}
    for name, y in cases(sr).items():
        if only is None or name in only:
            err, lerr = frame_metric(fo.log_fbank_f32(y, sr, n_mels, form, fault), oracle(sr, n_mels, name))
            out[name] = (float(err.max()), float(lerr.max()))
    return out


def measure_cpu(rates=RATES, batch_rates=BATCH_RATES):
    """The measurement behind CPU_MAX_POW / CPU_MAX_LOG: every case of this file through both forms of the float32
    restatement.  Returns (largest err_f, where, largest log error, where).  Minutes on one core; not a test."""
    best = [0.0, '', 0.0, '']

    def see(e, l, where):
        if e > best[0]:
            best[0:2] = [e, where]
        if l > best[2]:
            best[2:4] = [l, where]
    for sr, n_mels in rates:
        for form in ('single', 'batch'):
            for name, (e, l) in restatement_worst(sr, n_mels, form).items():
                see(e, l, '%d/%d %s %s' % (sr, n_mels, form, name))
    for sr, n_mels in batch_rates:
        for lname, waves in batch_lists(sr).items():
            for i, y in enumerate(waves):
                for form in ('single', 'batch'):
                    err, lerr = frame_metric(fo.log_fbank_f32(y, sr, n_mels, form), oracle(sr, n_mels, lname, i))
                    see(float(err.max()), float(lerr.max()), '%d/%d %s %s[%d]' % (sr, n_mels, form, lname, i))
    return tuple(best)


@pytest.mark.parametrize('sr,n_mels', RATES)
def test_restatement_stays_inside_a_quarter_of_the_bounds(sr, n_mels):
    """The bounds are four times what the float32 restatement shows (measure_cpu() adds the batch lists; here every
    per-rate case, both forms): nothing it produces may exceed the recorded maxima."""
    for form in ('single', 'batch'):
        for name, (e, l) in restatement_worst(sr, n_mels, form).items():
            assert e <= CPU_MAX_POW and l <= CPU_MAX_LOG, (form, name, e, l)
    assert BOUND_POW <= 2e-3 and BOUND_LOG <= 2e-3            # never looser than tests/test_frontend.py


@pytest.mark.parametrize('fault', ['edge', 'window', 'frame'])
def test_cases_have_teeth_against_one_line_faults(fault):
    """A repeated edge sample in the fold, a Hann window shifted by one sample, frame f read at f hop + 1: each, put
    into the RESTATEMENT, fails at least ten cases of one rate by more than 100 times the bound (most by far more;
    profiles/frontend_edges.txt has the figures for every rate)."""
    sr, n_mels = 11025, 40
    factors = sorted((max(e / BOUND_POW, l / BOUND_LOG) for e, l in restatement_worst(sr, n_mels, 'batch', fault).values()),
                     reverse=True)
    print('frontend_edges fault %s at %d Hz: %d of %d cases fail, 10th largest factor %.3g, largest %.3g'
          % (fault, sr, sum(f > 1 for f in factors), len(factors), factors[9], factors[0]))
    assert factors[9] > 100.0, factors[:12]
    # the edge frames of the edge-sensitive content are where a wrong fold shows
    if fault == 'edge':
        for name in ('imp1_long', 'imp-2_long', 'ramp_short', 'ramp_long', 'partsine_long'):
            got, want = fo.log_fbank_f32(cases(sr)[name], sr, n_mels, 'batch', fault), oracle(sr, n_mels, name)
            err, _ = frame_metric(got, want)
            assert max(err[0], err[-1]) > 100 * BOUND_POW, (name, err[0], err[-1])


# ------------------------------------------------------------------------------------------------ GPU: both forms
@pytest.mark.gpu
@pytest.mark.parametrize('sr,n_mels', RATES)
def test_per_utterance_form_matches_the_oracle_at_every_length_and_content(sr, n_mels):
    """ssasr_logmel (log_fbank) on every case of the rate: 16 lengths from 1 sample (the n == 1 branch, folds over
    hundreds of periods) to 5 hop + 2 around every frame-count change, impulses at both edges, a ramp, an incomplete
    sine, silence around a tone, four amplitudes of one noise from 1e-9 to int16 scale, DC."""
    from ss_asr_amd.frontend import log_fbank
    worst = Worst('log_fbank %d Hz / %d mels' % (sr, n_mels))
    try:
        for name, y in cases(sr).items():
            got = log_fbank(y, sr, n_mels).cpu().numpy()
            assert_case(worst, got, oracle(sr, n_mels, name), name, *((y, sr) if name == 'zeros_tone_zeros' else ()))
    finally:
        worst.report()


@pytest.mark.gpu
@pytest.mark.parametrize('sr,n_mels', RATES)
def test_batched_form_matches_the_oracle_at_every_length_and_content(sr, n_mels):
    """ssasr_logmel_batch (log_fbank_batch) on the same cases as ONE list: hops of 441 (odd: unaligned overlapping
    rows, guarded loads), 110 (2 mod 4, odd window, Kp != n_fft), 80, 160, 220 and 480; 13 and 23 mel bands (output
    rows that are no multiple of four floats)."""
    from ss_asr_amd.frontend import log_fbank_batch
    worst = Worst('log_fbank_batch %d Hz / %d mels' % (sr, n_mels))
    names = list(cases(sr))
    waves = [cases(sr)[k] for k in names]
    feats, first, frames = log_fbank_batch(waves, sr, n_mels)
    assert feats.dtype == torch.float32 and feats.shape[1] == n_mels
    feats = feats.cpu().numpy()
    try:
        for name, y, r0, nf in zip(names, waves, first, frames):
            assert_case(worst, feats[r0:r0 + nf], oracle(sr, n_mels, name), name,
                        *((y, sr) if name == 'zeros_tone_zeros' else ()))
    finally:
        worst.report()


# ------------------------------------------------------------------------------------------------ GPU: batch layout
@pytest.mark.gpu
@pytest.mark.parametrize('lname', ['last_1', 'last_2', 'last_hop', 'longest_last', 'longest_middle', 'one_sample_alone',
                                   'many_300', 'loud_quiet_loud', 'long_3s_then_3'])
@pytest.mark.parametrize('sr,n_mels', BATCH_RATES)
def test_batch_layout_edges(sr, n_mels, lname):
    """A list through log_fbank_batch: every utterance against the oracle at its OWN per-frame scale (a 1e-6 utterance
    between two of int16 scale included), first / frames tile the rows without overlap, EVERY utterance -- the first,
    and the last, which owns the n_fft extension even when it has one sample -- bit-identical to the same utterance
    run alone, and a list of device tensors gives the bits of the list of host arrays."""
    from ss_asr_amd import _lib
    from ss_asr_amd.frontend import log_fbank_batch
    lib = _lib.load()
    n_fft, hop = geometry(sr)
    waves = batch_lists(sr)[lname]
    feats, first, frames = log_fbank_batch(waves, sr, n_mels)
    torch.cuda.synchronize()
    rows = [int(lib.ssasr_logmel_batch_rows(len(w), n_fft, hop)) for w in waves]
    assert first[0] == 0 and feats.shape == (sum(rows), n_mels)
    for i in range(len(waves)):
        assert 1 <= frames[i] <= rows[i]
        assert first[i] == (first[i - 1] + rows[i - 1] if i else 0)         # tiles: no overlap, no gap but the spare rows
    assert torch.isfinite(feats).all()                                       # the rows between utterances too
    on_dev, f2, n2 = log_fbank_batch([torch.from_numpy(w).cuda() for w in waves], sr, n_mels)
    assert (f2, n2) == (first, frames) and torch.equal(on_dev, feats)
    host = feats.cpu().numpy()
    worst = Worst('batch list %s %d Hz / %d mels' % (lname, sr, n_mels))
    try:
        for i, y in enumerate(waves):
            assert_case(worst, host[first[i]:first[i] + frames[i]], oracle(sr, n_mels, lname, i), '%s[%d]' % (lname, i))
    finally:
        worst.report()
    for i, y in enumerate(waves):
        alone, f0, n0 = log_fbank_batch([y], sr, n_mels)
        assert n0[0] == frames[i]
        assert torch.equal(alone[f0[0]:f0[0] + n0[0]], feats[first[i]:first[i] + frames[i]]), (lname, i)


# ------------------------------------------------------------------------------------------------ GPU: workspaces
CANARY, TAIL = 12345.0, 64


def guarded(n, dev):
    """n floats of NaN followed by a canary tail; returns (whole buffer, the n floats)."""
    buf = torch.full((n + TAIL,), float('nan'), device=dev, dtype=torch.float32)
    buf[n:] = CANARY
    return buf, buf[:n]


def canary_intact(buf):
    return bool((buf[-TAIL:] == CANARY).all())


@pytest.mark.gpu
@pytest.mark.parametrize('sr,n_mels', [(22050, 80), (44100, 80), (16000, 80)])
def test_workspace_contract_of_both_entry_points(sr, n_mels):
    """ssasr_logmel_batch and ssasr_logmel called directly with every workspace and the output at EXACTLY the
    documented size (ws_wave total_rows hop + n_fft, ws_power total_rows nbp, out total_rows n_mels; ws_frames F Kp,
    ws_spec F 2 nb, ws_power F nbp), NaN-filled, each followed by a canary tail: every output row is finite (the rows
    between utterances as well), no canary changes, and the utterances' rows are the wrapper's bits.  The list ends in
    a one-sample utterance, whose reflection fills the n_fft extension."""
    from ss_asr_amd import _lib
    from ss_asr_amd.frontend import frontend_constants, log_fbank, log_fbank_batch
    lib = _lib.load()
    dev = torch.device('cuda')
    n_fft, hop, window, basis, mel, basis_w = frontend_constants(sr, n_mels, dev)
    assert (n_fft, hop) == geometry(sr)
    nb = n_fft // 2 + 1
    kp, nbp = (n_fft + 3) // 4 * 4, (nb + 3) // 4 * 4
    assert basis.shape == (2 * nb, kp) and basis_w.shape == (2 * nb, kp) and mel.shape == (n_mels, nbp)
    waves = batch_lists(sr)['last_1']
    lens = [len(w) for w in waves]
    rows = [int(lib.ssasr_logmel_batch_rows(n, n_fft, hop)) for n in lens]
    frames = [int(lib.ssasr_logmel_frames(n, n_fft, hop)) for n in lens]
    first = [sum(rows[:i]) for i in range(len(rows))]
    offs = [sum(lens[:i]) for i in range(len(lens))]
    total = sum(rows)
    wav = torch.from_numpy(np.concatenate(waves)).to(dev)
    utt = torch.tensor([[o, n, r] for o, n, r in zip(offs, lens, first)], dtype=torch.int64, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    (b_wave, ws_wave), (b_pow, ws_pow), (b_out, out) = (guarded(total * hop + n_fft, dev), guarded(total * nbp, dev),
                                                        guarded(total * n_mels, dev))
    rc = lib.ssasr_logmel_batch(p(wav), p(utt), len(lens), max(lens), total, n_fft, hop, n_mels, p(basis_w), p(mel),
                                p(ws_wave), p(ws_pow), p(out), stream)
    torch.cuda.synchronize()
    assert rc == 0
    assert canary_intact(b_wave) and canary_intact(b_pow) and canary_intact(b_out)
    assert torch.isfinite(ws_wave).all()                       # the layout fills its whole buffer, extension included
    assert torch.isfinite(ws_pow.view(total, nbp)[:, :nb]).all()
    out = out.view(total, n_mels)
    assert torch.isfinite(out).all()
    feats, f1, n1 = log_fbank_batch(waves, sr, n_mels)
    assert (f1, n1) == (first, frames)
    for i in range(len(waves)):
        assert torch.equal(out[first[i]:first[i] + frames[i]], feats[first[i]:first[i] + frames[i]]), i

    for i, y in enumerate(waves):
        n, nf = lens[i], frames[i]
        (b_fr, ws_fr), (b_sp, ws_sp), (b_pw, ws_pw), (b_o, o) = (guarded(nf * kp, dev), guarded(nf * 2 * nb, dev),
                                                                 guarded(nf * nbp, dev), guarded(nf * n_mels, dev))
        one = torch.from_numpy(y).to(dev)
        rc = lib.ssasr_logmel(p(one), n, n_fft, hop, n_mels, p(window), p(basis), p(mel), p(ws_fr), p(ws_sp), p(ws_pw),
                              p(o), stream)
        torch.cuda.synchronize()
        assert rc == 0
        assert canary_intact(b_fr) and canary_intact(b_sp) and canary_intact(b_pw) and canary_intact(b_o), i
        assert all(bool(torch.isfinite(t).all()) for t in (ws_fr, ws_sp, ws_pw, o)), i
        assert torch.equal(o.view(nf, n_mels), log_fbank(y, sr, n_mels)), i


# ------------------------------------------------------------------------------------------------ GPU: arguments
@pytest.mark.gpu
def test_bad_arguments_are_refused_before_any_launch():
    """Each bad argument alone gives SSASR_EARG; every pointer handed over is a live device buffer of the size a
    valid call would need (the utterance table has 65,536 rows)."""
    from ss_asr_amd import _lib
    from ss_asr_amd.frontend import frontend_constants, log_fbank_batch
    lib = _lib.load()
    dev = torch.device('cuda')
    sr, n_mels = 16000, 80
    n_fft, hop, window, basis, mel, basis_w = frontend_constants(sr, n_mels, dev)
    nb = n_fft // 2 + 1
    n = 3 * hop
    rows, frames = int(lib.ssasr_logmel_batch_rows(n, n_fft, hop)), int(lib.ssasr_logmel_frames(n, n_fft, hop))
    wav = torch.zeros(n, device=dev)
    utt = torch.zeros(65536, 3, dtype=torch.int64, device=dev)
    utt[:, 1] = n
    f = lambda *s: torch.zeros(*s, device=dev, dtype=torch.float32)
    ws_wave, ws_pow, out = f(rows * hop + n_fft), f(rows, mel.shape[1]), f(rows, n_mels)
    ws_fr, ws_sp = f(frames, basis.shape[1]), f(frames, 2 * nb)
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def batch(n_utts=1, max_samples=n, total_rows=rows, n_fft_=n_fft, hop_=hop, n_mels_=n_mels, ws=p(ws_wave)):
        return lib.ssasr_logmel_batch(p(wav), p(utt), n_utts, max_samples, total_rows, n_fft_, hop_, n_mels_,
                                      p(basis_w), p(mel), ws, p(ws_pow), p(out), stream)

    def single(n_samples=n, n_fft_=n_fft, hop_=hop, n_mels_=n_mels, ws=p(ws_fr)):
        return lib.ssasr_logmel(p(wav), n_samples, n_fft_, hop_, n_mels_, p(window), p(basis), p(mel), ws, p(ws_sp),
                                p(ws_pow), p(out), stream)
    before = out.clone()
    assert batch(n_utts=0) == EARG and batch(n_utts=65536) == EARG
    assert batch(hop_=0) == EARG and batch(n_fft_=1) == EARG and batch(n_mels_=0) == EARG
    assert batch(max_samples=0) == EARG and batch(ws=None) == EARG
    assert single(n_samples=0) == EARG and single(hop_=0) == EARG and single(n_fft_=1) == EARG
    assert single(n_mels_=0) == EARG and single(ws=None) == EARG
    torch.cuda.synchronize()
    assert torch.equal(out, before)                            # nothing ran
    assert batch() == 0 and single() == 0                      # the same buffers make a valid call
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        log_fbank_batch([], sr, n_mels)
    with pytest.raises(ValueError):
        log_fbank_batch([np.ones(5, dtype=np.float32), np.zeros(0, dtype=np.float32)], sr, n_mels)
