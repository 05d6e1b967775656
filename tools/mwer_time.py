"""Times the MWER loss launches (ssasr_mwer_loss_fwd / _bwd) beside the masked CE's (ssasr_ce_loss_fwd / _bwd) on the
same [R, U, V] logits, and one engine.MWERTrainStep beside one engine.ASRTrainStep on the same batch for K = 4 and
K = 8.  The MWER step decodes a beam and then teacher-forces K + 1 rows per utterance where the CE step
teacher-forces one: the two step times are printed for what they are, not as a like-for-like comparison.
Device events around the launches, warm-up, many repetitions, medians; the step times are wall-clock over
synchronised blocks of steps.  --batch B --frames T --chars C choose the synthetic batch (default 4 x 400 x 40)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ss_asr_amd import _lib, ops  # noqa: E402
from ss_asr_amd.asr import ASR  # noqa: E402
from ss_asr_amd.engine import ASRTrainStep, MWERTrainStep, label_geometry  # noqa: E402
from ss_asr_amd.synthetic import make_batch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=50)
ap.add_argument('--steps', type=int, default=20)
ap.add_argument('--batch', type=int, default=4)
ap.add_argument('--frames', type=int, default=400)
ap.add_argument('--chars', type=int, default=40)
args = ap.parse_args()

d = torch.device('cuda:0')
lib = _lib.load()


def median_us(run):
    for _ in range(5):
        run()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.reps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        run()
        ev[1].record()
        torch.cuda.synchronize()
        times.append(ev[0].elapsed_time(ev[1]) * 1e3)
    times.sort()
    return times[len(times) // 2], times[0], times[-1]


def loss_times(G, M, U, V):
    R = G * M
    gen = torch.Generator().manual_seed(0)
    logits = torch.randn(R, U, V, generator=gen).to(d)
    rows = torch.randint(1, V, (R, U + 1), generator=gen, dtype=torch.int32)
    rows[:, 0] = 0
    rows = rows.to(d)
    counts = torch.randint(0, 10, (R, 8), generator=gen, dtype=torch.int32).to(d)
    n_hyps = torch.full((G,), M - 1, dtype=torch.int32, device=d)
    ce_w = torch.full((R,), 1e-3, device=d)
    need = int(lib.ssasr_mwer_ws_bytes(G, M, U))
    ws = torch.empty(need // 8, dtype=torch.float64, device=d)
    risk = torch.empty(G, device=d)
    loss = torch.empty((), device=d)
    one = torch.ones((), device=d)
    dlogits = torch.empty_like(logits)
    lse = torch.empty(R * U + 9 * R, device=d)
    p, st = ops._p, ops._stream
    runs = {
        'mwer fwd': lambda: ops.check(lib.ssasr_mwer_loss_fwd(p(logits), p(rows), U + 1, U + 1, p(n_hyps), p(counts), 1,
                                                              p(ce_w), G, M, U, V, p(ws), need, p(risk), p(loss), st()), 'fwd'),
        'mwer bwd': lambda: ops.check(lib.ssasr_mwer_loss_bwd(p(logits), p(rows), U + 1, U + 1, G, M, U, V, p(ws), need,
                                                              p(one), p(dlogits), st()), 'bwd'),
        'ce fwd': lambda: ops.check(lib.ssasr_ce_loss_fwd(p(logits), p(rows), U + 1, U + 1, R, U, V, p(lse), p(loss), st()), 'ce'),
        'ce bwd': lambda: ops.check(lib.ssasr_ce_loss_bwd(p(logits), p(rows), U + 1, p(lse), p(one), R, U, V, p(dlogits), st()),
                                    'ce'),
    }
    mb = R * U * V * 4 / 1e6
    print('[R, U, V] = [%d x %d, %d, %d] (%.2f MB of logits):' % (G, M, U, V, mb))
    for name, run in runs.items():
        med, lo, hi = median_us(run)
        print('  %-9s %8.1f us (min %.1f, max %.1f, %d reps)' % (name, med, lo, hi, args.reps))


def step_time(step, call):
    for _ in range(3):
        call()
    step.finish()
    torch.cuda.synchronize()
    blocks = []
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(args.steps):
            call()
        step.finish()
        torch.cuda.synchronize()
        blocks.append((time.perf_counter() - t0) * 1e3 / args.steps)
    blocks.sort()
    return blocks[1], blocks[0], blocks[2]


for K in (4, 8):
    loss_times(args.batch, K + 1, args.chars + 1, 50)

frames = np.linspace(args.frames, args.frames * 0.6, args.batch).astype(int)
chars = np.linspace(args.chars, args.chars * 0.6, args.batch).astype(int)
x, y, lens = make_batch(frames, chars, 80, seed=1)
x, y = x.to(d), y.to(d)
_, ans_len = label_geometry(y.cpu())
torch.manual_seed(0)
model = ASR(50, 256, 256, 128, 80, 1.0).to(d)
ce = ASRTrainStep(model)
med, lo, hi = step_time(ce, lambda: ce(x, y, lens, ans_len))
print('batch %d x %d frames x %d characters:' % (args.batch, args.frames, args.chars))
print('  ASRTrainStep            %8.2f ms / step (blocks of %d: min %.2f, max %.2f)' % (med, args.steps, lo, hi))
for K in (4, 8):
    step = MWERTrainStep(model, K, max_decoding_steps=args.chars + 10)
    med, lo, hi = step_time(step, lambda: step(x, y, lens))
    print('  MWERTrainStep K = %d     %8.2f ms / step (min %.2f, max %.2f), %d rows of %d steps, mean risk %.2f'
          % (K, med, lo, hi, step.last_logits.shape[0], step.last_logits.shape[1], float(step.last_risk.mean())))
