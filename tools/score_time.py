"""Times the edit-distance scoring launch (ssasr_edit_score) for one n-best group -- 32 utterances x 32 hypotheses =
1,024 pairs, 200 decode steps, references of about 100 characters, random tokens from a fixed seed -- beside
postprocess.edit_counts over the same pairs on the host, and the same 1,024 pairs at full-length rows of 63 (one
wave per pair: no barrier in the sweep), 64 (two waves: one barrier per step) and 1,023 tokens (16 waves), to show
what the per-step barrier costs.  Device events around the launch, warm-up, many repetitions; prints microseconds
per launch and nanoseconds per sweep step (the launch over the H + R steps of the character sweep, the longer of the
two sweeps; the word sweep, compaction and word ids are inside the figure).  --host-pairs N times the host on the
first N pairs only (default: all)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ss_asr_amd import _lib, ops  # noqa: E402
from ss_asr_amd.postprocess import edit_counts  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--host-pairs', type=int, default=None)
ap.add_argument('--reps', type=int, default=50)
args = ap.parse_args()

d = torch.device('cuda:0')
lib = _lib.load()
N, K, V, SPACE = 32, 32, 50, 46
rng = np.random.default_rng(0)


def tokens(n):
    """n random characters, one in six a space"""
    t = rng.integers(3, V, size=n)
    t[rng.random(n) < 1.0 / 6.0] = SPACE
    return t.astype(np.int32)


def group(hyp_lens, ref_lens, cols, ref_cols):
    hyp = np.zeros((N * K, cols), dtype=np.int32)
    ref = np.zeros((N, ref_cols), dtype=np.int32)
    for i, n in enumerate(ref_lens):
        ref[i, :n] = tokens(n)
    for p, n in enumerate(hyp_lens):
        hyp[p, :n] = tokens(n)
    ref_of = np.repeat(np.arange(N, dtype=np.int32), K)
    return hyp, np.asarray(hyp_lens, dtype=np.int32), ref, np.asarray(ref_lens, dtype=np.int32), ref_of


def launch_time(g):
    hyp, hyp_lens, ref, ref_lens, ref_of = [torch.from_numpy(a).to(d) for a in g]
    assert torch.equal(ops.edit_score(hyp, hyp_lens, ref, ref_lens, ref_of, space=SPACE),
                       ops.edit_score(hyp, hyp_lens, ref[ref_of.long()].contiguous(), ref_lens[ref_of.long()], space=SPACE))
    out = torch.empty(hyp.shape[0], 8, dtype=torch.int32, device=d)

    def run():          # the entry itself: ops.edit_score's check of ref_of reads a flag back, which is not the launch
        ops.check(lib.ssasr_edit_score(ops._p(hyp), hyp.shape[1], ops._p(hyp_lens), ops._p(ref), ref.shape[1],
                                       ops._p(ref_lens), ops._p(ref_of), hyp.shape[0], hyp.shape[1], ref.shape[1], 2,
                                       SPACE, ops._p(out), ops._stream()), 'ssasr_edit_score')

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
    return out.cpu().numpy(), times[len(times) // 2], times[0], times[-1]


# the n-best group of a 200-step decode
g = group(rng.integers(60, 201, size=N * K).tolist(), rng.integers(80, 121, size=N).tolist(), 200, 120)
out, med, lo, hi = launch_time(g)
steps = int(g[1].max() + g[3].max())
print('n-best group, %d pairs, hypotheses 60..200 of 200 columns, references 80..120: launch %.1f us (min %.1f, max %.1f, '
      '%d reps), %.0f ns per sweep step (%d steps)' % (N * K, med, lo, hi, args.reps, med * 1e3 / steps, steps))
n_host = N * K if args.host_pairs is None else min(args.host_pairs, N * K)
t0 = time.perf_counter()
want = [edit_counts(g[0][p, :g[1][p]], g[2][g[4][p], :g[3][g[4][p]]], SPACE) for p in range(n_host)]
host = time.perf_counter() - t0
assert np.array_equal(out[:n_host], np.asarray(want, dtype=np.int32)), 'the launch and the host routine disagree'
print('host edit_counts over %d of the pairs: %.2f s (%.1f ms per pair; %.1f s for the group at that rate), results equal'
      % (n_host, host, host * 1e3 / n_host, host / n_host * N * K))

# what the barrier costs: the same 1,024 pairs at full-length rows
for L in (63, 64, 1023):
    g = group([L] * (N * K), [L] * N, L, L)
    _, med, lo, hi = launch_time(g)
    print('rows of %4d tokens (%2d waves per pair): launch %.1f us (min %.1f, max %.1f), %.0f ns per sweep step (%d steps)'
          % (L, (L + 64) // 64, med, lo, hi, med * 1e3 / (2 * L), 2 * L))
