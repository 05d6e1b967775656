"""Times the CTC segmentation kernel (ssasr_ctc_segment).  First beside the forced-alignment kernel (ssasr_ctc_align)
on the same inputs, alternating in one process, at the encoder geometry of BASELINE.json configs[3] (T' = 375, 300
characters), where both apply; then alone at two long shapes, one with many frames and few states (T = 32768, 40
characters: the 256 x 1 form) and one with many states (T = 8200, 8191 characters: the 1024 x 16 form).  Prints
microseconds per launch and per frame, and the traceback's share of the segment launch from the kernel's own phase
stamps (the workspace's last 4 x B words: wall_clock64 at the start, before and after the traceback, at the end)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ss_asr_amd import _lib, ops  # noqa: E402

d = torch.device('cuda:0')
lib = _lib.load()
for B, T, V, lmax, with_align in ((32, 375, 50, 300, True), (1, 375, 50, 300, True), (1, 32768, 50, 40, False),
                                  (1, 8200, 50, 8191, False)):
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
    need = int(lib.ssasr_ctc_segment_ws_bytes(B, T, V, lmax, 2))
    ws = torch.zeros(need // 8, device=d, dtype=torch.int64)
    path = torch.empty(B, T, device=d, dtype=torch.int32)
    first, last = torch.empty(B, lmax, device=d, dtype=torch.int32), torch.empty(B, lmax, device=d, dtype=torch.int32)
    logp, score = torch.empty(B, lmax, device=d), torch.empty(B, device=d, dtype=torch.float64)
    uf, ul = torch.empty(B, 2, device=d, dtype=torch.int32), torch.empty(B, 2, device=d, dtype=torch.int32)
    uc = torch.empty(B, 2, device=d)
    a_score = torch.empty(B, device=d, dtype=torch.float64)
    if with_align:
        a_need = int(lib.ssasr_ctc_align_ws_bytes(B, T, V, lmax))
        a_ws = torch.zeros(a_need // 8, device=d, dtype=torch.int64)

    def segment():
        ops.check(lib.ssasr_ctc_segment(ops._p(logits), ops._p(frame_lens), ops._p(y), lmax, ops._p(label_lens),
                                        ops._p(utt_ends), 2, ops._p(n_utts), B, T, V, lmax, 2, 30, 0, ops._p(ws), need,
                                        ops._p(path), ops._p(first), ops._p(last), ops._p(logp), ops._p(score), ops._p(uf),
                                        ops._p(ul), ops._p(uc), ops._stream()), 'ssasr_ctc_segment')

    def align():
        ops.check(lib.ssasr_ctc_align(ops._p(logits), ops._p(frame_lens), ops._p(y), lmax, ops._p(label_lens), B, T, V,
                                      lmax, 0, ops._p(a_ws), a_need, ops._p(path), ops._p(first), ops._p(last),
                                      ops._p(logp), ops._p(a_score), ops._stream()), 'ssasr_ctc_align')

    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    ts = ta = 0.0
    share = []
    n = 20 if T <= 1000 else 5
    for it in range(n + 2):
        ev[0].record()
        segment()
        ev[1].record()
        if with_align:
            align()
        ev[2].record()
        torch.cuda.synchronize()
        if it >= 2:
            ts += ev[0].elapsed_time(ev[1])
            ta += ev[1].elapsed_time(ev[2])
            st = ws[-4 * B:].view(B, 4).cpu().double()
            st = st[st[:, 3] > st[:, 0]]                    # rows without a segmentation report no phases
            if len(st):
                share.append(float(((st[:, 2] - st[:, 1]) / (st[:, 3] - st[:, 0])).mean()))
    ts, ta = ts * 1e3 / n, ta * 1e3 / n
    form = ops.ctc_segment_form(T, lmax)
    line = 'B=%d T=%d Lmax=%d (form %d: %d threads x %d states; %d rows segment): segment %.1f us (%.3f us / frame)' % (
        B, T, lmax, form[0], form[1], form[2], int(torch.isfinite(score).sum()), ts, ts / T)
    if with_align:
        line += ', align %.1f us (%.3f us / frame), ratio %.2f' % (ta, ta / T, ts / ta)
    print(line + (', traceback %.1f %% of the segment kernel' % (100.0 * sum(share) / len(share)) if share else ''))
