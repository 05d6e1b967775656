"""Times the CTC forced-alignment kernel (ssasr_ctc_align) beside the loss's forward kernel (ssasr_ctc_loss_fwd:
ctc_alpha_kernel and its one-thread mean) on the same inputs, alternating in one process, at the encoder geometries
of BASELINE.json configs[1] (T' = 100, 40 characters) and configs[3] (T' = 375, 300 characters).  Prints microseconds
per launch and per frame, and the traceback's share of the align launch from the kernel's own phase stamps (the
workspace's last 4 x B words: wall_clock64 at the start, before and after the traceback, at the end)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ss_asr_amd import _lib, ops  # noqa: E402

d = torch.device('cuda:0')
lib = _lib.load()
for B, T, V, lmax in ((32, 100, 50, 40), (32, 375, 50, 300)):
    g = torch.Generator().manual_seed(0)
    logits = torch.randn(B, T, V, generator=g).to(d)
    frame_lens = torch.full((B,), T, dtype=torch.int32, device=d)
    label_lens = torch.full((B,), lmax, dtype=torch.int32, device=d)
    y = torch.randint(2, V, (B, lmax), generator=g).to(d, torch.int32)
    need = int(lib.ssasr_ctc_align_ws_bytes(B, T, V, lmax))
    ws = torch.zeros(need // 8, device=d, dtype=torch.int64)
    path = torch.empty(B, T, device=d, dtype=torch.int32)
    first, last = torch.empty(B, lmax, device=d, dtype=torch.int32), torch.empty(B, lmax, device=d, dtype=torch.int32)
    logp, score = torch.empty(B, lmax, device=d), torch.empty(B, device=d, dtype=torch.float64)
    loss_ws = torch.empty(int(lib.ssasr_ctc_ws_floats(B, T, V, lmax)), device=d)
    loss = torch.empty((), device=d)

    def align():
        ops.check(lib.ssasr_ctc_align(ops._p(logits), ops._p(frame_lens), ops._p(y), lmax, ops._p(label_lens), B, T, V,
                                      lmax, 0, ops._p(ws), need, ops._p(path), ops._p(first), ops._p(last), ops._p(logp),
                                      ops._p(score), ops._stream()), 'ssasr_ctc_align')

    def alpha():
        ops.check(lib.ssasr_ctc_loss_fwd(ops._p(logits), ops._p(frame_lens), ops._p(y), lmax, ops._p(label_lens), B, T, V,
                                         lmax, 0, ops._p(loss_ws), ops._p(loss), ops._stream()), 'ssasr_ctc_loss_fwd')

    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    ta = tl = 0.0
    share = []
    n = 20
    for it in range(n + 4):
        ev[0].record()
        align()
        ev[1].record()
        alpha()
        ev[2].record()
        torch.cuda.synchronize()
        if it >= 4:
            ta += ev[0].elapsed_time(ev[1])
            tl += ev[1].elapsed_time(ev[2])
            st = ws[-4 * B:].view(B, 4).cpu().double()
            share.append(float(((st[:, 2] - st[:, 1]) / (st[:, 3] - st[:, 0])).mean()))
    ta, tl = ta * 1e3 / n, tl * 1e3 / n
    feasible = int(torch.isfinite(score).sum())
    print('B=%d T=%d Lmax=%d (%d rows align): align %.1f us (%.3f us / frame), loss forward %.1f us (%.3f us / frame), '
          'traceback %.1f %% of the align kernel' % (B, T, lmax, feasible, ta, ta / T, tl, tl / T,
                                                     100.0 * sum(share) / len(share)))
