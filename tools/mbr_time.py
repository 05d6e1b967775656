"""Times the minimum-Bayes-risk launch (ssasr_mbr_select) for one group -- 32 utterances x K in {8, 32} hypotheses of
about 100 characters (80 .. 120, one in six a space), random tokens from a fixed seed -- beside the N * K * K pair
launch of ssasr_edit_score through ref_of on the same rows, which is how the K x K distances of an utterance could be
had before: every ordered pair a workgroup that compacts both rows and numbers their words again.  The two must give
the same distances; that is asserted first.  Device events around the launch, warm-up, many repetitions; prints
microseconds per launch.  The pair launch's figure leaves out the posterior, the risks and the argmin, which it would
leave to the host."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ss_asr_amd import _lib, ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=50)
args = ap.parse_args()

d = torch.device('cuda:0')
lib = _lib.load()
N, V, SPACE, COLS = 32, 50, 46, 120
rng = np.random.default_rng(0)


def median_time(run):
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


for K in (8, 32):
    lens = rng.integers(80, COLS + 1, size=(N, K)).astype(np.int32)
    rows = np.zeros((N, K, COLS), dtype=np.int32)
    for n in range(N):
        for k in range(K):
            t = rng.integers(3, V, size=lens[n, k])
            t[rng.random(lens[n, k]) < 1.0 / 6.0] = SPACE
            rows[n, k, :lens[n, k]] = t
    chars = torch.from_numpy(rows).to(d)
    n_chars = torch.from_numpy(lens).to(d)
    n_hyps = torch.full((N,), K, dtype=torch.int32, device=d)
    scores = torch.from_numpy(-np.abs(rng.normal(size=(N, K))).astype(np.float32)).to(d)
    best = torch.empty(N, dtype=torch.int32, device=d)
    risk = torch.empty(N, K, dtype=torch.float32, device=d)
    pair = torch.empty(N, K, K, 2, dtype=torch.int32, device=d)

    def mbr():
        ops.check(lib.ssasr_mbr_select(ops._p(chars), COLS, ops._p(n_chars), ops._p(n_hyps), ops._p(scores), N, K, COLS,
                                       2, SPACE, 1, 0, 1.0, ops._p(best), ops._p(risk), ops._p(pair), ops._stream()),
                  'ssasr_mbr_select')

    # pair p = (n, k, j): hypothesis row n * K + k against reference row n * K + j
    flat, flat_lens = chars.view(N * K, COLS), n_chars.view(N * K)
    hyp = flat.repeat_interleave(K, dim=0).contiguous()
    hyp_lens = flat_lens.repeat_interleave(K).contiguous()
    idx = torch.arange(N * K * K, device=d)
    ref_of = ((idx // (K * K)) * K + idx % K).to(torch.int32)
    out = torch.empty(N * K * K, 8, dtype=torch.int32, device=d)

    def pairs():
        ops.check(lib.ssasr_edit_score(ops._p(hyp), COLS, ops._p(hyp_lens), ops._p(flat), COLS, ops._p(flat_lens),
                                       ops._p(ref_of), N * K * K, COLS, COLS, 2, SPACE, ops._p(out), ops._stream()),
                  'ssasr_edit_score')

    mbr()
    pairs()
    torch.cuda.synchronize()
    o = out.view(N, K, K, 8)
    assert torch.equal(pair[..., 0], o[..., 0:3].sum(-1)) and torch.equal(pair[..., 1], o[..., 4:7].sum(-1)), \
        'the two launches disagree on the distances'
    a, b = median_time(mbr), median_time(pairs)
    print('K = %2d: ssasr_mbr_select, %d workgroups, %d pair sweeps: %.1f us (min %.1f, max %.1f); ssasr_edit_score over '
          '%d pairs through ref_of: %.1f us (min %.1f, max %.1f); %d reps; distances equal'
          % (K, N, N * K * (K - 1) // 2, a[0], a[1], a[2], N * K * K, b[0], b[1], b[2], args.reps))
