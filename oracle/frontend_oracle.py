"""CPU oracle for the log-mel frontend  --  TEST INFRASTRUCTURE ONLY.

PARITY UNPINNED: the reference's log_fbank (src/preprocess.py:187-208) calls
librosa 0.6.3, which is neither vendored in the reference nor installed in
this image, and the reference holds no sample fbanks.  This file restates
librosa's published algorithm for melspectrogram with the arguments the
reference passes (n_fft = int(0.025 sr), hop = int(0.010 sr), defaults
otherwise: center=True, pad_mode='reflect', periodic Hann, power 2, Slaney mel,
norm=1, fmin=0, fmax=sr/2) in float64 numpy, written independently of
ss_asr_amd/frontend.py (FFT-based, loop-built filters)."""
import functools

import numpy as np


def hz_to_mel(f):
    f_sp = 200.0 / 3
    if f >= 1000.0:
        return 1000.0 / f_sp + np.log(f / 1000.0) / (np.log(6.4) / 27.0)
    return f / f_sp


def mel_to_hz(m):
    f_sp = 200.0 / 3
    min_log_mel = 1000.0 / f_sp
    if m >= min_log_mel:
        return 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - min_log_mel))
    return f_sp * m


@functools.lru_cache(maxsize=None)
def mel_basis(sr, n_fft, n_mels):
    """[n_mels, n_fft // 2 + 1] float64 (cached: callers must not write to it)."""
    nb = n_fft // 2 + 1
    freqs = [i * (sr / 2.0) / (nb - 1) for i in range(nb)]
    lo, hi = hz_to_mel(0.0), hz_to_mel(sr / 2.0)
    pts = [mel_to_hz(lo + (hi - lo) * i / (n_mels + 1)) for i in range(n_mels + 2)]
    w = np.zeros((n_mels, nb))
    for m in range(n_mels):
        left, centre, right = pts[m], pts[m + 1], pts[m + 2]
        for k, f in enumerate(freqs):
            up = (f - left) / (centre - left)
            down = (right - f) / (right - centre)
            w[m, k] = max(0.0, min(up, down)) * 2.0 / (right - left)
    w.setflags(write=False)
    return w


def n_frames(n, sr):
    """Frames of log_fbank for n samples: numpy's padded length, cut as librosa's util.frame cuts it."""
    n_fft, hop = int(sr * 0.025), int(sr * 0.010)
    return 1 + (n + 2 * (n_fft // 2) - n_fft) // hop


def fold(i, n, fault=None):
    """Index into y of sample i of numpy's 'reflect' extension of y (i may be negative or past the end; signals
    shorter than the pad fold as often as needed).  fault 'edge': the edge sample repeated (numpy's 'symmetric')."""
    i = np.asarray(i, dtype=np.int64)
    if n == 1:
        return np.zeros_like(i)
    if fault == 'edge':
        i = i % (2 * n)
        return np.where(i >= n, 2 * n - 1 - i, i)
    period = 2 * (n - 1)
    i = i % period                                # numpy's %: result in [0, period)
    return np.where(i >= n, period - i, i)


_f32_constants = {}


def log_fbank_f32(y, sr, n_mels, form='batch', fault=None):
    """float32 [frames, n_mels]: the ARITHMETIC of the GPU frontend restated on the CPU, for error bounds only.
    float32 window / DFT basis / mel filters (float64 values rounded once; form 'batch': the window folded into
    the basis in float64 and rounded once, form 'single': the frame windowed in float32 first), the DFT and mel
    sums accumulated sequentially over k in float32, power and log(S + eps) in float32.
    fault (to show that a test has teeth, never a property of the product): 'edge' repeats the edge sample in the
    reflection, 'window' uses the Hann window shifted by one sample, 'frame' reads frame f at f * hop + 1."""
    y = np.asarray(y, dtype=np.float32).reshape(-1)
    n_fft, hop = int(sr * 0.025), int(sr * 0.010)
    nb = n_fft // 2 + 1
    key = (sr, n_mels, form, fault == 'window')
    if key not in _f32_constants:
        k = np.arange(n_fft, dtype=np.float64)
        window = 0.5 - 0.5 * np.cos(2 * np.pi * (k + (fault == 'window')) / n_fft)
        ang = 2 * np.pi * np.outer(k, np.arange(nb, dtype=np.float64)) / n_fft          # [k][bin]
        if form == 'batch':
            cos, sin, w = np.cos(ang) * window[:, None], np.sin(ang) * window[:, None], None
        else:
            cos, sin, w = np.cos(ang), np.sin(ang), window.astype(np.float32)
        _f32_constants[key] = (w, np.concatenate([cos, sin], axis=1).astype(np.float32),
                               np.ascontiguousarray(mel_basis(sr, n_fft, n_mels).T).astype(np.float32))
    window, basis, mel = _f32_constants[key]
    frames = n_frames(len(y), sr)
    at = (np.arange(frames)[:, None] * hop + (fault == 'frame')) + np.arange(n_fft)[None, :] - n_fft // 2
    x = y[fold(at, len(y), fault)]
    if window is not None:
        x = x * window[None, :]
    spec = np.zeros((frames, 2 * nb), dtype=np.float32)
    for k in range(n_fft):
        spec += x[:, k:k + 1] * basis[k][None, :]
    re, im = spec[:, :nb], spec[:, nb:]
    power = re * re + im * im
    out = np.zeros((frames, n_mels), dtype=np.float32)
    for k in range(nb):
        out += power[:, k:k + 1] * mel[k][None, :]
    return np.log(out + np.float32(np.finfo(float).eps))


def log_fbank(y, sr, n_mels):
    """float64 [frames, n_mels]; src/preprocess.py:194-206."""
    y = np.asarray(y, dtype=np.float64)
    n_fft, hop = int(sr * 0.025), int(sr * 0.010)
    padded = np.pad(y, n_fft // 2, mode='reflect')
    frames = 1 + (len(padded) - n_fft) // hop
    n = np.arange(n_fft)
    window = 0.5 - 0.5 * np.cos(2 * np.pi * n / n_fft)
    spec = np.empty((frames, n_fft // 2 + 1))
    for f in range(frames):
        seg = padded[f * hop:f * hop + n_fft] * window
        spec[f] = np.abs(np.fft.rfft(seg)) ** 2
    mel = spec @ mel_basis(sr, n_fft, n_mels).T
    return np.log(mel + np.finfo(float).eps)
