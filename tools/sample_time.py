"""Times the sampling launch (ssasr_decode_sample) beside the beam search (ssasr_decode_beam) at the same K = 4 and 8
on the batch-mode features of tools/mwer_time.py's batch, and one sampled engine.MWERTrainStep beside the beam-searched
one on that batch.  An untrained model rarely draws or chooses <EOS>, so both launches run close to their step limit:
the launch times compare the cost of a step, not the length of the transcripts.  Device events around the launches,
5 warm-up launches, --reps repetitions, medians; the step times are wall-clock over synchronised blocks of steps.
--batch B --frames T --chars C choose the synthetic batch (default 4 x 400 x 40)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ss_asr_amd import ops  # noqa: E402
from ss_asr_amd.asr import ASR  # noqa: E402
from ss_asr_amd.engine import MWERTrainStep  # noqa: E402
from ss_asr_amd.synthetic import make_batch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=50)
ap.add_argument('--steps', type=int, default=20)
ap.add_argument('--batch', type=int, default=4)
ap.add_argument('--frames', type=int, default=400)
ap.add_argument('--chars', type=int, default=40)
args = ap.parse_args()

d = torch.device('cuda:0')
EOS = 1


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


frames = np.linspace(args.frames, args.frames * 0.6, args.batch).astype(int)
chars = np.linspace(args.chars, args.chars * 0.6, args.batch).astype(int)
x, y, lens = make_batch(frames, chars, 80, seed=1)
x, y = x.to(d), y.to(d)
torch.manual_seed(0)
model = ASR(50, 256, 256, 128, 80, 1.0).to(d)
S = args.chars + 10
with torch.no_grad():
    feat, _, enc_len_dev, _, _ = model.encode(x, lens)
    feat = feat.detach().contiguous()
common = (feat, enc_len_dev, model._decoder_params(), (model.attention.psi.weight, model.attention.psi.bias), None, 0.0,
          EOS, S)
print('batch %d x %d frames (T\' = %d), %d decoding steps:' % (args.batch, args.frames, feat.shape[1], S))
for K in (4, 8):
    uniforms = torch.rand(args.batch, K, S, device=d, generator=torch.Generator(device=d).manual_seed(K))
    with torch.no_grad():
        n_s = ops.decode_sample(*common, K, uniforms)[1].float().mean().item()
        n_b = ops.decode_beam(*common, K)[1].float().mean().item()
        med, lo, hi = median_us(lambda: ops.decode_sample(*common, K, uniforms))
        print('  decode_sample K = %d  %9.1f us (min %.1f, max %.1f, %d reps), mean length %.1f' % (K, med, lo, hi, args.reps, n_s))
        med, lo, hi = median_us(lambda: ops.decode_beam(*common, K))
        print('  decode_beam   K = %d  %9.1f us (min %.1f, max %.1f, %d reps), mean length %.1f' % (K, med, lo, hi, args.reps, n_b))
for K in (4, 8):
    for sampling in (False, True):
        torch.manual_seed(0)
        fresh = ASR(50, 256, 256, 128, 80, 1.0).to(d)
        step = MWERTrainStep(fresh, K, max_decoding_steps=S, sampling=sampling, seed=0 if sampling else None)
        med, lo, hi = step_time(step, lambda: step(x, y, lens))
        print('  MWERTrainStep K = %d %-8s %8.2f ms / step (min %.2f, max %.2f), %d rows of %d steps, mean risk %.2f'
              % (K, 'sampled' if sampling else 'beam', med, lo, hi, step.last_logits.shape[0], step.last_logits.shape[1],
                 float(step.last_risk.mean())))
