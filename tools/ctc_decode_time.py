"""Milliseconds per launch of CTC-only decoding (ssasr_ctc_decode, csrc/ctc.hip) at beam widths 0 (best path), 1, 8
and 32 on tools/beam_time.py's shape: 32 utterances, T' = 100 encoder frames each, V = 50, random weights.  The
encoder outputs are random and the head's logits are formed once; the decode launch alone is timed, with events
around it, warm, median over --steps launches.  The head product (ops.ctc_head_decode's GEMM) is timed beside it, and
in the same sitting ssasr_decode_beam at K = 8 with tools/beam_time.py's call, the attention search that the
CTC-only pass stands in front of.

    python tools/ctc_decode_time.py [--steps 5] [--warmup 2] [--beams 0,1,8,32] [--frames 100]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from beam_time import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--beams', default='0,1,8,32')
    ap.add_argument('--utts', type=int, default=32)
    ap.add_argument('--frames', type=int, default=100)
    ap.add_argument('--max-steps', type=int, default=200)
    args = ap.parse_args()
    from ss_asr_amd import ops
    from ss_asr_amd.asr import ASR
    from ss_asr_amd.charlm import CharLM
    dev, V, S, N, T = 'cuda:0', 50, args.max_steps, args.utts, args.frames
    torch.manual_seed(0)
    asr = ASR(V, 256, 256, 128, 80, 1.0).to(dev).eval()
    lm = CharLM(V, 128).to(dev).eval()
    head = torch.nn.Linear(512, V).to(dev)
    feat = torch.tanh(torch.randn(N, T, 512, device=dev))          # bounded, as a BiLSTM's outputs are
    enc_len = torch.full((N,), T, device=dev, dtype=torch.int32)
    res = {'shape': dict(N=N, T=T, E=512, V=V), 'launches': args.steps}
    held = {}
    with torch.no_grad():
        def product():
            held['logits'] = ops.gemm(feat.view(N * T, 512), head.weight, bias=head.bias).view(N, T, V)
        res['head_gemm_ms'] = timed(product, args.steps, args.warmup)
        logits = held['logits']
        for K in [int(k) for k in args.beams.split(',')]:
            def fn(K=K):
                held['out'] = ops.ctc_decode(logits, enc_len, K)
            ms = timed(fn, args.steps, args.warmup)
            n_chars = held['out'][1][:, 0].float()
            res['ctc_K%d' % K] = dict(launch_ms=ms, us_per_frame=1e3 * ms / T, mean_chars=float(n_chars.mean()),
                                      mean_hyps=float(held['out'][3].float().mean()))
        call = (feat, enc_len, asr._decoder_params(), (asr.attention.psi.weight, asr.attention.psi.bias), lm, 0.5, 1, S)
        ws = torch.empty(int(ops._lib.load().ssasr_decode_beam_ws_bytes(N, 8, T, 512, 128, 256, V, 128, S)) // 4, device=dev)

        def beam():
            held['beam'] = ops.decode_beam(*call, 8, ws=ws)
        ms = timed(beam, args.steps, args.warmup)
        ran = int(min(int(held['beam'][1].max()) + 1, S))
        res['attention_beam_K8'] = dict(launch_ms=ms, steps_run=ran, us_per_step=1e3 * ms / ran)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
