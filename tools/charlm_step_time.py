"""ms per CharLM train step at conf/default.yaml's shape (B 128, U 200, H 128, V 50): the fused path
(engine.CharLMTrainStep: one forward launch, one backward launch, the gradient products, fused clip + Adam) and the
same step written as the reference writes it (nn.GRUCell loop, autograd, clip_grad_norm_, torch.optim.Adam;
src/trainer.py:229-251) on torch-ROCm on the same GPU.  Warm, median over --steps steps, each step timed with
events around it and one synchronisation per step; the forward / backward / products split of the fused path is
timed the same way on its own launches.

    python tools/charlm_step_time.py [--steps 20] [--warmup 3] [--no-torch]
"""
import argparse
import json
import os
import random
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--chunk', type=int, default=200)
    ap.add_argument('--hidden', type=int, default=128)
    ap.add_argument('--no-torch', action='store_true')
    args = ap.parse_args()
    from ss_asr_amd import ops
    from ss_asr_amd.charlm import CharLM
    from ss_asr_amd.engine import CharLMTrainStep
    dev, V, B, U, H = 'cuda:0', 50, args.batch, args.chunk, args.hidden
    torch.manual_seed(0)
    random.seed(0)
    y = torch.randint(0, V, (B, U), device=dev)
    lm = CharLM(V, H).to(dev)
    step = CharLMTrainStep(lm, 0.9, lr=1e-4)
    res = {'shape': dict(B=B, U=U, H=H, V=V), 'steps': args.steps,
           'workspace_mb': ops.charlm_ws_layout(B, U, H, V)['total'] * 4 / 2 ** 20}
    res['fused_step_ms'] = timed(lambda: step(y), args.steps, args.warmup)
    step.finish()
    modes = torch.tensor(step.draw_modes(U), dtype=torch.int32, device=dev)
    uni = torch.rand(U, B, device=dev)
    held = {}

    def fwd():
        held['c'] = ops.charlm_chunk(lm, y, modes=modes, uniforms=uni, ws=step._ws)
    res['fused_fwd_ms'] = timed(fwd, args.steps, args.warmup)

    def fwd_bwd():
        fwd()
        ops.charlm_chunk_backward(lm, held['c'])
    res['fused_fwd_bwd_products_ms'] = timed(fwd_bwd, args.steps, args.warmup)
    lib = ops._lib.load()
    import ctypes as C
    s, keep = ops._charlm_struct(lm)

    def fwd_bwd_kernel():
        fwd()
        ops.check(lib.ssasr_charlm_train_bwd(C.byref(s), ops._p(held['c'].y), B, U, 1.0 / B, ops._p(held['c'].ws),
                                             ops._stream()), 'ssasr_charlm_train_bwd')
    res['fused_fwd_bwd_kernel_ms'] = timed(fwd_bwd_kernel, args.steps, args.warmup)

    if not args.no_torch:
        ref = nn.ModuleDict(dict(emb=nn.Embedding(V, H), l1=nn.GRUCell(H, H), l2=nn.GRUCell(H, H), out=nn.Linear(H, V))).to(dev)
        optim = torch.optim.Adam(ref.parameters(), lr=1e-4, eps=1e-8)
        ce = nn.CrossEntropyLoss(reduction='none')

        def torch_step():
            ref.zero_grad()
            loss = 0
            last = torch.zeros(B, device=dev)
            h1 = torch.zeros(B, H, device=dev)
            h2 = torch.zeros(B, H, device=dev)
            for i in range(U):
                h1 = ref['l1'](ref['emb'](last.long()), h1)
                h2 = ref['l2'](h1, h2)
                out = ref['out'](h2)
                label = y[:, i]
                loss = loss + ce(out, label)
                if random.random() <= 0.9:
                    last = label
                else:
                    last = torch.distributions.Categorical(F.softmax(out, dim=-1)).sample()
            loss = torch.mean(loss)
            loss.backward()
            nn.utils.clip_grad_norm_(ref.parameters(), 5)
            optim.step()
        res['torch_step_ms'] = timed(torch_step, args.steps, args.warmup)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
