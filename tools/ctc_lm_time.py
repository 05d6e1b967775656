"""Milliseconds per launch of the CTC prefix beam search with the CharLM in the search (ssasr_ctc_decode_lm,
csrc/infer.hip) on tools/beam_time.py's shape: 32 utterances, T' = 100 encoder frames each, V = 50, K = 8, random
weights, the CharLM's hidden size that of the default configuration (char_lm.mdl.hidden_size: 128; --lm-hidden).  The
head's logits are formed once; each launch is timed alone, with events around it, warm, median over --steps launches.
Timed in the same sitting: ssasr_ctc_decode at the same K, ssasr_decode_beam at K = 8 with step cap 68, and the
two-pass path (ssasr_ctc_decode, then ops.rescore with the CharLM).  Also reported: the share of frames that ran an LM
step.  On random weights the beam turns over far more often than behind a trained head: the unfavourable end.

    python tools/ctc_lm_time.py [--steps 5] [--warmup 2] [--beam 8] [--frames 100] [--lm-hidden 128]
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
    ap.add_argument('--beam', type=int, default=8)
    ap.add_argument('--utts', type=int, default=32)
    ap.add_argument('--frames', type=int, default=100)
    ap.add_argument('--max-steps', type=int, default=68)
    ap.add_argument('--lm-hidden', type=int, default=128)
    ap.add_argument('--lm-weight', type=float, default=0.5)
    args = ap.parse_args()
    from ss_asr_amd import ops
    from ss_asr_amd.asr import ASR
    from ss_asr_amd.charlm import CharLM
    dev, V, S, N, T, K, H = 'cuda:0', 50, args.max_steps, args.utts, args.frames, args.beam, args.lm_hidden
    torch.manual_seed(0)
    asr = ASR(V, 256, 256, 128, 80, 1.0).to(dev).eval()
    lm = CharLM(V, H).to(dev).eval()
    head = torch.nn.Linear(512, V).to(dev)
    feat = torch.tanh(torch.randn(N, T, 512, device=dev))          # bounded, as a BiLSTM's outputs are
    enc_len = torch.full((N,), T, device=dev, dtype=torch.int32)
    res = {'shape': dict(N=N, T=T, E=512, V=V, K=K, lm_hidden=H), 'launches': args.steps}
    held = {}
    with torch.no_grad():
        logits = ops.gemm(feat.view(N * T, 512), head.weight, bias=head.bias).view(N, T, V)

        def fused():
            held['lm'] = ops.ctc_decode_lm(logits, enc_len, K, lm, args.lm_weight, 0.0, 1)
        ms_lm = timed(fused, args.steps, args.warmup)
        frames = held['lm']['lm_frames'].float()
        res['ctc_lm'] = dict(launch_ms=ms_lm, us_per_frame=1e3 * ms_lm / T, lm_frame_share=float(frames.mean()) / T,
                             mean_chars=float(held['lm']['n_chars'][:, 0].float().mean()))

        def plain():
            held['ctc'] = ops.ctc_decode(logits, enc_len, K)
        ms_ctc = timed(plain, args.steps, args.warmup)
        res['ctc'] = dict(launch_ms=ms_ctc, us_per_frame=1e3 * ms_ctc / T)

        params, psi = asr._decoder_params(), (asr.attention.psi.weight, asr.attention.psi.bias)
        call = (feat, enc_len, params, psi, lm, args.lm_weight, 1, S)
        ws = torch.empty(int(ops._lib.load().ssasr_decode_beam_ws_bytes(N, 8, T, 512, 128, 256, V, H, S)) // 4, device=dev)

        def beam():
            held['beam'] = ops.decode_beam(*call, 8, ws=ws)
        ms_beam = timed(beam, args.steps, args.warmup)
        res['attention_beam_K8'] = dict(launch_ms=ms_beam, steps_run=int(min(int(held['beam'][1].max()) + 1, S)))

        def two_pass():
            chars, n_chars, scores, n_hyps = ops.ctc_decode(logits, enc_len, K)
            held['two'] = ops.rescore(feat, enc_len, params, psi, chars, n_chars, n_hyps, scores, 1, lm,
                                      lm_weight=args.lm_weight, att_weight=0.7, first_weight=0.3)
        ms_two = timed(two_pass, args.steps, args.warmup)
        res['two_pass'] = dict(total_ms=ms_two)
        res['ratio'] = dict(to_ctc=ms_lm / ms_ctc, to_attention_beam=ms_lm / ms_beam, to_two_pass=ms_lm / ms_two)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
