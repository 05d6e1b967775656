"""Microseconds per decode step of the one-launch decoders (csrc/infer.hip) at conf/default.yaml's dimensions:
32 utterances, T' = 100 encoder frames each, 200 steps, CharLM hidden 128, for beam size 1 (ssasr_decode_greedy)
and 3, 8 (ssasr_decode_beam).  The encoder outputs are random and encoded once; only the decode launch is timed,
with events around it, warm, median over --steps launches.  A step's time is the launch time over the steps the
slowest utterance ran (n_chars + 1 for greedy, the longest hypothesis for a beam, both capped at 200).  The
comparison that matters: K hypotheses in one workgroup against K x the greedy figure of the same run.

--ctc W adds, per K, the same launch through ssasr_decode_beam_ctc with a random ctc_head at CTC weight W (K = 1
then is the beam kernel at width 1), and with weight 0 (the plain kernel through the new entry).

--length-bonus B, --coverage ETA[,TAU] and --end-margin D add, per K, the same launch through ssasr_decode_beam_ex
with those terms on (K = 1 then is the beam kernel at width 1), and with every term off (the plain kernel through
the new entry); with --ctc W both carry the CTC term too.  These rows report n_steps of the slowest utterance, the
loop iterations the launch lasted, beside the launch time.

    python tools/beam_time.py [--steps 5] [--warmup 2] [--beams 1,3,8] [--ctc 0.3] [--length-bonus 0.5]
                              [--coverage 0.5,0.025] [--end-margin 0]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

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
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--beams', default='1,3,8')
    ap.add_argument('--utts', type=int, default=32)
    ap.add_argument('--frames', type=int, default=100)
    ap.add_argument('--max-steps', type=int, default=200)
    ap.add_argument('--ctc', type=float, default=0.0, help='CTC weight of the additional joint-decoding rows')
    ap.add_argument('--length-bonus', type=float, default=0.0, help='beta of the additional ssasr_decode_beam_ex rows')
    ap.add_argument('--coverage', default=None, metavar='ETA[,TAU]', help='coverage weight and threshold (default 0.5)')
    ap.add_argument('--end-margin', type=float, default=None, help='delta >= 0 of the end detection')
    args = ap.parse_args()
    terms = dict(length_bonus=args.length_bonus, end_margin=args.end_margin)
    if args.coverage is not None:
        eta_tau = [float(v) for v in args.coverage.split(',')]
        terms.update(coverage_weight=eta_tau[0], coverage_threshold=eta_tau[1] if len(eta_tau) > 1 else 0.5)
    terms_on = args.length_bonus != 0 or terms.get('coverage_weight', 0) != 0 or args.end_margin is not None
    from ss_asr_amd import ops
    from ss_asr_amd.asr import ASR
    from ss_asr_amd.charlm import CharLM
    dev, V, S, N, T = 'cuda:0', 50, args.max_steps, args.utts, args.frames
    torch.manual_seed(0)
    asr = ASR(V, 256, 256, 128, 80, 1.0).to(dev).eval()
    lm = CharLM(V, 128).to(dev).eval()
    feat = torch.tanh(torch.randn(N, T, 512, device=dev))          # bounded, as a BiLSTM's outputs are
    enc_len = torch.full((N,), T, device=dev, dtype=torch.int32)
    call = (feat, enc_len, asr._decoder_params(), (asr.attention.psi.weight, asr.attention.psi.bias), lm, 0.5, 1, S)
    res = {'shape': dict(N=N, T=T, S=S, E=512, A=128, D=256, Hl=128, V=V), 'launches': args.steps}
    for K in [int(k) for k in args.beams.split(',')]:
        held = {}
        if K == 1:
            def fn():
                held['out'] = ops.decode_greedy(*call, want_att=False)
        else:
            ws = torch.empty(int(ops._lib.load().ssasr_decode_beam_ws_bytes(N, K, T, 512, 128, 256, V, 128, S)) // 4,
                             device=dev)

            def fn(K=K, ws=ws):
                held['out'] = ops.decode_beam(*call, K, ws=ws)
        ms = timed(fn, args.steps, args.warmup)
        n_chars = held['out'][1].cpu().numpy()
        ran = int(min(n_chars.max() + 1, S))
        res['K%d' % K] = dict(launch_ms=ms, steps_run=ran, us_per_step=1e3 * ms / ran,
                              mean_chars=float(n_chars[n_chars > 0].mean()) if (n_chars > 0).any() else 0.0)
        if terms_on:
            head = torch.nn.Linear(512, V).to(dev) if args.ctc > 0 else None
            ctc = (head.weight, head.bias, args.ctc) if head is not None else None
            for tag, kw in (('terms', terms), ('terms_entry_off', {})):
                ws = torch.empty(int(ops._lib.load().ssasr_decode_beam_ex_ws_bytes(
                    N, K, T, 512, 128, 256, V, 128, S, int(ctc is not None), int(kw.get('coverage_weight', 0) != 0))) // 4,
                    device=dev)

                def fn(K=K, ws=ws, kw=kw):
                    held['out'] = ops.decode_beam_ex(*call, K, ctc, ws=ws, **kw)
                ms = timed(fn, args.steps, args.warmup)
                ran = int(held['out'][4].max())
                res['K%d_%s' % (K, tag)] = dict(launch_ms=ms, n_steps=ran, us_per_step=1e3 * ms / ran,
                                                mean_hyps=float(held['out'][3].float().mean()))
        if args.ctc > 0:
            head = torch.nn.Linear(512, V).to(dev)
            ws = torch.empty(int(ops._lib.load().ssasr_decode_beam_ctc_ws_bytes(N, K, T, 512, 128, 256, V, 128, S)) // 4,
                             device=dev)
            for tag, weight in (('ctc', args.ctc), ('ctc_entry_weight0', 0.0)):
                def fn(K=K, ws=ws, weight=weight):
                    held['out'] = ops.decode_beam_ctc(*call, K, (head.weight, head.bias, weight), ws=ws)
                ms = timed(fn, args.steps, args.warmup)
                n_chars = held['out'][1].cpu().numpy()
                ran = int(min(n_chars.max() + 1, S))
                res['K%d_%s' % (K, tag)] = dict(launch_ms=ms, steps_run=ran, us_per_step=1e3 * ms / ran)
    if 'K1' in res:
        for k, v in res.items():
            if k.startswith('K') and k != 'K1' and '_' not in k:
                v['vs_K_greedy_workgroups'] = v['us_per_step'] / (int(k[1:]) * res['K1']['us_per_step'])
    print(json.dumps(res))


if __name__ == '__main__':
    main()
