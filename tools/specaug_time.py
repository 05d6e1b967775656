"""What SpecAugment in batch assembly and label smoothing in the CE cost, measured in one sitting.

  python tools/specaug_time.py [--out FILE]                batch assembly at 32 x 800 x 80: ssasr_gather_batch_aug
                                                           with 2 + 2 masks against ssasr_gather_batch, warm, in
                                                           alternating blocks of 100 launches, median of 5 blocks
  python tools/specaug_time.py --train-step [frames]       the fixed train step of tools/ab_option.py (batch
                                                           assembly + engine.ASRTrainStep) with both features on
                                                           against both off, alternating blocks of 10 steps

Every line printed is one JSON object; --out appends them to FILE as well."""
import json
import os
import random
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from ss_asr_amd import ops

SPEC = dict(n_freq=2, max_freq=27, n_time=2, max_time=40, time_ratio=0.2, fill=0.0, seed=2019)
dev = torch.device('cuda', 0)
out_file = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None


def emit(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    if out_file:
        with open(out_file, 'a') as f:
            f.write(line + '\n')


def assembly(B=32, T=800, F=80, launches=100, blocks=5):
    rng = np.random.default_rng(0)
    lens = np.sort(rng.integers(T // 2, T + 1, size=B))[::-1].astype(np.int32)
    lens[0] = T
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    frames = torch.randn(int(lens.sum()), F, device=dev)
    offs_d, lens_d = torch.from_numpy(offs).to(dev), torch.from_numpy(lens.copy()).to(dev)
    ids = torch.arange(B, dtype=torch.int32, device=dev)
    spec = ops.specaug_params(SPEC)
    run = {'gather_batch': lambda: ops.gather_batch(frames, offs_d, lens_d, T),
           'gather_batch_aug': lambda: ops.gather_batch_aug(frames, offs_d, lens_d, ids, T, spec)}
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    res = {k: [] for k in run}
    for k in run:
        for _ in range(20):
            run[k]()
    torch.cuda.synchronize()
    for r in range(blocks):
        for k in (sorted(run) if r % 2 == 0 else sorted(run, reverse=True)):
            run[k]()
            start.record()
            for _ in range(launches):
                run[k]()
            stop.record()
            torch.cuda.synchronize()
            res[k].append(start.elapsed_time(stop) / launches * 1e3)
    bytes_moved = 4 * F * (int(lens.sum()) + B * T)
    for k in sorted(run):
        emit(what='batch assembly', entry=k, shape=[B, T, F], masks=[2, 2] if k.endswith('aug') else [0, 0],
             us_per_launch_blocks=[round(v, 3) for v in res[k]], us_per_launch_median=round(float(np.median(res[k])), 3),
             us_per_launch_spread=round(max(res[k]) - min(res[k]), 3), bytes_read_and_written=bytes_moved,
             note='device events around the block: the output allocation and the enqueue are part of both')


def train_step(frames_wanted=470, n=10, rounds=5):
    import bench
    from ss_asr_amd.asr import ASR
    from ss_asr_amd.engine import ASRTrainStep, label_geometry
    from ss_asr_amd.gpu_loader import GpuResidentLoader
    from ss_asr_amd.synthetic import config2_batches
    random.seed(1); np.random.seed(1); torch.manual_seed(1)
    model = ASR(**bench.DIMS).to(dev)
    model.train()
    stepper = ASRTrainStep(model, lr=1.0, eps=1e-8, grad_clip=5.0)
    best = None
    for x, y, lens in config2_batches(40, batch_size=32, feat_dim=80, seed=1, rank=0, hi=800):
        if best is None or abs(max(lens) - frames_wanted) < abs(max(best[2]) - frames_wanted):
            best = (x, y, lens)
    x, y, lens = best
    _, ans_len = label_geometry(y)
    utts = [x[b, :lens[b]].numpy() for b in range(len(lens))]
    labels = [y[b, :int((y[b] != 0).sum()) + 1].tolist() for b in range(len(lens))]       # '<' chars '>'
    loaders = {'off': GpuResidentLoader.from_arrays(utts, labels, 32, dev),
               'on': GpuResidentLoader.from_arrays(utts, labels, 32, dev, spec_augment=SPEC)}
    smoothing = {'off': 0.0, 'on': 0.1}

    def step(v):
        stepper.label_smoothing = smoothing[v]
        xb, xl, yb, yl = loaders[v].batch(0)
        return stepper(xb, yb, xl, max(yl) - 1)
    for v in ('off', 'on'):
        for _ in range(4):
            step(v)
    torch.cuda.synchronize()
    res, last = {'off': [], 'on': []}, {}
    for r in range(rounds):
        for v in (('off', 'on') if r % 2 == 0 else ('on', 'off')):
            step(v)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                last[v] = step(v)
            torch.cuda.synchronize()
            res[v].append((time.perf_counter() - t0) / n * 1e3)
    stepper.finish()
    for v in ('off', 'on'):
        emit(what='train step (batch assembly + fused step)', features=v, frames=int(max(lens)),
             spec_augment=SPEC if v == 'on' else None, label_smoothing=smoothing[v],
             ms_per_step_blocks=[round(t, 3) for t in res[v]], ms_per_step_median=round(float(np.median(res[v])), 3),
             ms_per_step_spread=round(max(res[v]) - min(res[v]), 3), last_loss=round(float(last[v]), 4))


if __name__ == '__main__':
    if '--train-step' in sys.argv:
        i = sys.argv.index('--train-step')
        train_step(int(sys.argv[i + 1]) if len(sys.argv) > i + 1 and sys.argv[i + 1].isdigit() else 470)
    else:
        assembly()
