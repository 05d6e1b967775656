"""Times the segmentation kernel with utterance skips and a filler (ssasr_ctc_segment_skip, skip_penalty -3,
fill_penalty -1) beside the plain kernel (ssasr_ctc_segment) on the same inputs, alternating in one process, at
tools/segment_time.py's four shapes.  Prints microseconds per launch and per frame for both, their ratio, and each
kernel's phase shares from its own stamps (the workspace's last 4 x B words: wall_clock64 at the start, before and
after the traceback, at the end), and writes the same lines to profiles/segment_skip_time.txt."""
import ctypes
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ss_asr_amd import _lib, ops  # noqa: E402

d = torch.device('cuda:0')
lib = _lib.load()
lines = []
for B, T, V, lmax in ((32, 375, 50, 300), (1, 375, 50, 300), (1, 32768, 50, 40), (1, 8200, 50, 8191)):
    g = torch.Generator().manual_seed(0)
    logits = torch.randn(B, T, V, generator=g).to(d)
    frame_lens = torch.full((B,), T, dtype=torch.int32, device=d)
    label_lens = torch.full((B,), lmax, dtype=torch.int32, device=d)
    y = torch.randint(2, V, (B, lmax), generator=g)
    for j in range(1, lmax):                                # no adjacent repeats: the frames hold the text
        same = y[:, j] == y[:, j - 1]
        y[same, j] = 2 + (y[same, j] - 1) % (V - 2)
    y = y.to(d, torch.int32)
    utt_ends = torch.tensor([[lmax // 2, lmax]] * B, dtype=torch.int32, device=d)
    n_utts = torch.full((B,), 2, dtype=torch.int32, device=d)
    need = [int(lib.ssasr_ctc_segment_ws_bytes(B, T, V, lmax, 2)), int(lib.ssasr_ctc_segment_skip_ws_bytes(B, T, V, lmax, 2))]
    ws = [torch.zeros(n // 8, device=d, dtype=torch.int64) for n in need]
    path, fill = torch.empty(B, T, device=d, dtype=torch.int32), torch.empty(B, T, device=d, dtype=torch.int32)
    first, last = torch.empty(B, lmax, device=d, dtype=torch.int32), torch.empty(B, lmax, device=d, dtype=torch.int32)
    logp = torch.empty(B, lmax, device=d)
    score = [torch.empty(B, device=d, dtype=torch.float64) for _ in range(2)]
    uf, ul, us = [torch.empty(B, 2, device=d, dtype=torch.int32) for _ in range(3)]
    uc = torch.empty(B, 2, device=d)
    pens = (ctypes.c_double * 2)(-3.0, -1.0)

    def plain():
        ops.check(lib.ssasr_ctc_segment(ops._p(logits), ops._p(frame_lens), ops._p(y), lmax, ops._p(label_lens),
                                        ops._p(utt_ends), 2, ops._p(n_utts), B, T, V, lmax, 2, 30, 0, ops._p(ws[0]), need[0],
                                        ops._p(path), ops._p(first), ops._p(last), ops._p(logp), ops._p(score[0]), ops._p(uf),
                                        ops._p(ul), ops._p(uc), ops._stream()), 'ssasr_ctc_segment')

    def skip():
        ops.check(lib.ssasr_ctc_segment_skip(
            ops._p(logits), ops._p(frame_lens), ops._p(y), lmax, ops._p(label_lens), ops._p(utt_ends), 2, ops._p(n_utts),
            B, T, V, lmax, 2, 30, 0, ctypes.addressof(pens), ctypes.addressof(pens) + 8, ops._p(ws[1]), need[1],
            ops._p(path), ops._p(first), ops._p(last), ops._p(logp), ops._p(score[1]), ops._p(uf), ops._p(ul), ops._p(uc),
            ops._p(us), ops._p(fill), ops._stream()), 'ssasr_ctc_segment_skip')

    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    total = [0.0, 0.0]
    phases = [[], []]                                       # (normalisers and frame loop, traceback, derived outputs)
    n = 20 if T <= 1000 else 5
    for it in range(n + 2):
        ev[0].record()
        plain()
        ev[1].record()
        skip()
        ev[2].record()
        torch.cuda.synchronize()
        if it >= 2:
            total[0] += ev[0].elapsed_time(ev[1])
            total[1] += ev[1].elapsed_time(ev[2])
            for k in range(2):
                st = ws[k][-4 * B:].view(B, 4).cpu().double()
                st = st[st[:, 3] > st[:, 0]]                # rows without a segmentation report no phases
                if len(st):
                    whole = st[:, 3] - st[:, 0]
                    phases[k].append([float(((st[:, i + 1] - st[:, i]) / whole).mean()) for i in range(3)])
    tp, tk = [t * 1e3 / n for t in total]
    form = ops.ctc_segment_form(T, lmax)
    line = ('B=%d T=%d Lmax=%d (form %d: %d threads x %d states): plain %.1f us (%.3f us / frame), skip %.1f us '
            '(%.3f us / frame), ratio %.2f' % (B, T, lmax, form[0], form[1], form[2], tp, tp / T, tk, tk / T, tk / tp))
    for name, ph in zip(('plain', 'skip'), phases):
        if ph:
            mean = [100.0 * sum(p[i] for p in ph) / len(ph) for i in range(3)]
            line += '; %s phases: lattice %.1f %%, traceback %.1f %%, outputs %.1f %%' % (name, *mean)
    line += '; rows segmented %d / %d, skipped utterances %d' % (
        int(torch.isfinite(score[0]).sum()), int(torch.isfinite(score[1]).sum()), int((us == 1).sum()))
    print(line, flush=True)
    lines.append(line)
with open(os.path.join(ROOT, 'profiles', 'segment_skip_time.txt'), 'w') as f:
    f.write('\n'.join(lines) + '\n')
