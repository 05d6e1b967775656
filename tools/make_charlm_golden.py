"""Generates tests/golden/charlm_*.npz by RUNNING THE REAL REFERENCE's CharLM (src/charlm.py) and LMDataset
(src/LMDataset.py) on CPU, imported through oracle/ref_harness.py, through the statements of
CHARLMTrainer.exec (src/trainer.py:229-251) with nn.CrossEntropyLoss(reduction='none'),
torch.optim.Adam(eps=1e-8) and clip_grad_norm_(..., 5).  Build-container tool: no test imports it, and it needs the
reference sources (SSASR_REFERENCE_SRC).

    python tools/make_charlm_golden.py

A fixture holds data only: the SEED of the weights (las_oracle.seeded_generic_weights; never the initial weights),
and for 3 consecutive steps at tf_rate 0.9 the labels y, the characters actually fed, the per-row losses, the
loss, the gradient norm, the gradients and the post-step weights.  The same trajectory (the same fed characters)
is run in float64, and every recorded quantity comes with noise = max |fp32 - fp64|: what a correct fp32
implementation may differ by, up to summation order (stored per step; for the two per-step scalars, loss and gradient
norm, the test takes the max over the steps: one number's distance from its twin can be far below fp32's resolution
by chance).  `charlm_full` stores gradients and weights as per-parameter
norms plus a fixed-seed sample of 2,048 entries per tensor (smaller tensors whole).
The dataset fixture is a short text with what the reference's LMDataset returns for it."""
import copy
import os
import random
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.distributions.categorical import Categorical

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
from ref_harness import import_reference  # noqa: E402
import las_oracle as lo  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden')
V, STEPS, TF_RATE, LR, SAMPLE = 50, 3, 0.9, 1e-4, 2048
# name, hidden, batch, chunk, weights seed, sampled (gradients / weights as norms + sample)
CASES = [('charlm_small', 16, 3, 5, 11, False), ('charlm_tile', 16, 17, 4, 12, False),
         ('charlm_full', 128, 20, 12, 13, True)]


def sample_index(seed, k, numel):
    """The fixed-seed entries of tensor k that a sampled fixture keeps (the test restates this)."""
    if numel <= SAMPLE:
        return np.arange(numel)
    return np.sort(np.random.default_rng(seed * 1000 + k).choice(numel, SAMPLE, replace=False))


def run_steps(lm, ys, fed_in, dtype):
    """src/trainer.py:229-251 for each y of ys.  fed_in None: flip and sample as the reference does and record what
    was fed; otherwise feed the recorded characters (the float64 twin follows the float32 trajectory)."""
    loss_metric = nn.CrossEntropyLoss(reduction='none')
    optim = torch.optim.Adam(lm.parameters(), lr=LR, eps=1e-8)
    rec = dict(fed=[], loss_rows=[], loss=[], grad_norm=[], grads=[], weights=[])
    for s, y in enumerate(ys):
        B, U = y.shape
        lm.zero_grad()
        loss = 0
        last_char = torch.zeros((B))
        (h_1, h_2) = lm.init_hidden(B, torch.device('cpu'))
        h_1, h_2 = h_1.to(dtype), h_2.to(dtype)
        fed = [last_char.long().numpy().copy()]
        for i in range(U):
            out, (h_1, h_2) = lm(last_char, h_1, h_2)
            label = y[:, i]
            loss += loss_metric(out, label.long())
            if fed_in is not None:
                last_char = torch.from_numpy(fed_in[s][i + 1]).to(torch.float32)
            elif random.random() <= TF_RATE:
                last_char = label
            else:
                last_char = Categorical(F.softmax(out, dim=-1)).sample()
            fed.append(last_char.long().numpy().copy())
        rows = loss.detach().clone()
        loss = torch.mean(loss)
        loss.backward()
        grad_norm = nn.utils.clip_grad_norm_(lm.parameters(), 5)       # Solver.step, :144-148
        grads = [p.grad.detach().clone() for p in lm.parameters()]     # after the clip, as the optimizer sees them
        assert not np.isnan(grad_norm.item())
        optim.step()
        rec['fed'].append(np.stack(fed).astype(np.int32))
        rec['loss_rows'].append(rows.numpy().astype(np.float64))
        rec['loss'].append(loss.item())
        rec['grad_norm'].append(grad_norm.item())
        rec['grads'].append([g.numpy().astype(np.float64).reshape(-1) for g in grads])
        rec['weights'].append([p.detach().numpy().astype(np.float64).reshape(-1).copy() for p in lm.parameters()])
    return rec


def make_case(charlm_mod, name, H, B, U, seed, sampled):
    """-> whether the case was kept: at least one of its steps must have fed a sampled character."""
    random.seed(seed)
    torch.manual_seed(seed)
    rng = np.random.default_rng(seed + 500)
    ys = [torch.from_numpy(rng.integers(0, V, (B, U))).to(torch.float32) for _ in range(STEPS)]
    lm32 = lo.seeded_generic_weights(charlm_mod.CharLM(V, H), seed)
    lm64 = copy.deepcopy(lm32).double()
    r32 = run_steps(lm32, ys, None, torch.float32)
    r64 = run_steps(lm64, [y.double() for y in ys], r32['fed'], torch.float64)
    n_sampled = sum(int((f[1:U] != y.numpy().astype(np.int32).T[:U - 1]).any()) for f, y in zip(r32['fed'], ys))
    names = [n for n, _ in lm32.named_parameters()]
    out = dict(V=np.int64(V), H=np.int64(H), B=np.int64(B), U=np.int64(U), weights_seed=np.int64(seed),
               tf_rate=np.float64(TF_RATE), lr=np.float64(LR), eps=np.float64(1e-8), max_norm=np.float64(5),
               sampled=np.int64(sampled), sample_size=np.int64(SAMPLE), names=np.array(names),
               y=np.stack([y.numpy() for y in ys]).astype(np.int32), fed=np.stack(r32['fed']),
               loss_rows=np.stack(r32['loss_rows']).astype(np.float32), loss=np.array(r32['loss'], np.float32),
               grad_norm=np.array(r32['grad_norm'], np.float32))
    diff = lambda a, b: float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))
    out['noise_loss_rows'] = np.array([diff(a, b) for a, b in zip(r32['loss_rows'], r64['loss_rows'])])
    out['noise_loss'] = np.array([diff(a, b) for a, b in zip(r32['loss'], r64['loss'])])
    out['noise_grad_norm'] = np.array([diff(a, b) for a, b in zip(r32['grad_norm'], r64['grad_norm'])])
    for kind in ('grads', 'weights'):
        out['noise_' + kind] = np.array([max(diff(a, b) for a, b in zip(s32, s64))
                                         for s32, s64 in zip(r32[kind], r64[kind])])
        for s in range(STEPS):
            for k, t in enumerate(r32[kind][s]):
                keep = sample_index(seed, k, t.size) if sampled else np.arange(t.size)
                out['%s_s%d_%d' % (kind, s, k)] = t[keep].astype(np.float32)
            out['%s_norms_s%d' % (kind, s)] = np.array([np.sqrt((t ** 2).sum()) for t in r32[kind][s]])
    if n_sampled < 1:
        print('%-13s seed %d: no sampled character in %d steps, next seed' % (name, seed, STEPS))
        return False
    path = os.path.join(OUT, name + '.npz')
    np.savez_compressed(path, **out)
    print('%-13s steps with a sampled character: %d / %d  loss %s  |g| %s  noise loss %.1e rows %.1e |g| %.1e g %.1e w %.1e'
          '  -> %.0f KB' % (name, n_sampled, STEPS, np.round(out['loss'], 4), np.round(out['grad_norm'], 4),
                            out['noise_loss'].max(), out['noise_loss_rows'].max(), out['noise_grad_norm'].max(),
                            out['noise_grads'].max(), out['noise_weights'].max(), os.path.getsize(path) / 1024))
    assert os.path.getsize(path) < 400 * 1024
    return True


def make_dataset(lmds_mod):
    chars = lo.TOKENS + lo.ALL_CHARS
    rng = np.random.default_rng(7)
    text = ''.join(chars[i] for i in rng.integers(3, len(chars), 203))
    path = os.path.join(OUT, 'charlm_dataset.txt')
    with open(path, 'w') as f:
        f.write(text)
    chunk = 8
    ds = lmds_mod.LMDataset(path, chunk)
    ds.device = torch.device('cpu')
    first, last = ds[0], ds[len(ds) - 1]
    out = dict(text=np.array(text), chunk_size=np.int64(chunk), length=np.int64(len(ds)),
               num_chars=np.int64(ds.get_num_chars()), chars=np.array(ds.chars))
    for tag, ((sx, sy), (x, y)) in (('first', first), ('last', last)):
        out[tag + '_sx'], out[tag + '_sy'] = np.array(sx), np.array(sy)
        out[tag + '_x'], out[tag + '_y'] = x.numpy(), y.numpy()
    probe = text[5:16]
    out['probe'] = np.array(probe)
    out['probe_s2l'] = ds.s2l(probe).numpy()
    out['probe_s2oh'] = ds.s2oh(probe).numpy()
    _, dl = lmds_mod.load_lm_dataset(path, chunk, 4, shuffle=False)
    out['batches_drop_last'] = np.int64(len(dl))
    out['all_y'] = np.stack([ds.s2l(ds.file[i + 1: i + chunk + 1]).numpy() for i in range(len(ds))]).astype(np.int32)
    np.savez_compressed(os.path.join(OUT, 'charlm_dataset.npz'), **out)
    print('dataset: %d chars, chunk %d, len %d, %d batches of 4' % (len(text), chunk, len(ds), len(dl)))


def main():
    import_reference()
    import charlm as charlm_mod                  # the reference's, from the same REF_SRC
    import LMDataset as lmds_mod
    ref = os.path.abspath(os.environ.get('SSASR_REFERENCE_SRC', '/root/reference/src'))
    assert os.path.abspath(charlm_mod.__file__).startswith(ref) and os.path.abspath(lmds_mod.__file__).startswith(ref)
    make_dataset(lmds_mod)
    for name, H, B, U, seed, sampled in CASES:
        while not make_case(charlm_mod, name, H, B, U, seed, sampled):     # the seed is recorded in the fixture
            seed += 100


if __name__ == '__main__':
    main()
