"""Milliseconds per launch of the CTC prefix beam search with a character graph in the search (ssasr_ctc_decode_graph,
csrc/ctc.hip) on tools/beam_time.py's shape: 32 utterances, T' = 100 encoder frames each, V = 50, K in --beams, random
weights behind the head, the graph the order-4 character n-gram LM of tests/golden/charlm_dataset.txt (--order).  The
head's logits are formed once; each launch is timed alone, with events around it, warm, median over --steps launches.
Timed in the same sitting at every K: ssasr_ctc_decode (the number to approach) and ssasr_ctc_decode_lm with a CharLM of
the default hidden size (the number to beat).  One JSON line per K.  On random weights the beam turns over far more often
than behind a trained head: the unfavourable end for the row loads.

    python tools/ctc_graph_time.py [--steps 5] [--warmup 2] [--beams 1,8,32] [--frames 100] [--order 4]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from beam_time import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--beams', default='1,8,32')
    ap.add_argument('--utts', type=int, default=32)
    ap.add_argument('--frames', type=int, default=100)
    ap.add_argument('--order', type=int, default=4)
    ap.add_argument('--graph-weight', type=float, default=0.5)
    ap.add_argument('--lm-hidden', type=int, default=128)
    args = ap.parse_args()
    from ss_asr_amd import ops
    from ss_asr_amd.char_graph import CharGraph
    from ss_asr_amd.charlm import CharLM
    from ss_asr_amd.LMDataset import LMDataset
    dev, V, N, T = 'cuda:0', 50, args.utts, args.frames
    text = LMDataset(os.path.join(ROOT, 'tests', 'golden', 'charlm_dataset.txt'), 8)
    graph = CharGraph.ngram([[text.char2idx[ch] for ch in w] for w in text.file.split(' ') if w], args.order, V, 1)
    torch.manual_seed(0)
    lm = CharLM(V, args.lm_hidden).to(dev).eval()
    head = torch.nn.Linear(512, V).to(dev)
    feat = torch.tanh(torch.randn(N, T, 512, device=dev))          # bounded, as a BiLSTM's outputs are
    enc_len = torch.full((N,), T, device=dev, dtype=torch.int32)
    held = {}
    with torch.no_grad():
        logits = ops.gemm(feat.view(N * T, 512), head.weight, bias=head.bias).view(N, T, V)
        for K in [int(k) for k in args.beams.split(',')]:
            def fused():
                held['graph'] = ops.ctc_decode_graph(logits, enc_len, K, graph, args.graph_weight)

            def plain():
                held['ctc'] = ops.ctc_decode(logits, enc_len, K)

            def charlm():
                held['lm'] = ops.ctc_decode_lm(logits, enc_len, K, lm, args.graph_weight, 0.0, 1)
            ms_graph = timed(fused, args.steps, args.warmup)
            ms_ctc = timed(plain, args.steps, args.warmup)
            ms_lm = timed(charlm, args.steps, args.warmup)
            print(json.dumps({'shape': dict(N=N, T=T, V=V, K=K, order=args.order, states=graph.n_states,
                                            lm_hidden=args.lm_hidden), 'launches': args.steps,
                              'ctc_graph_ms': ms_graph, 'ctc_ms': ms_ctc, 'ctc_lm_ms': ms_lm,
                              'us_per_frame': 1e3 * ms_graph / T, 'to_ctc': ms_graph / ms_ctc, 'to_ctc_lm': ms_graph / ms_lm,
                              'mean_chars': float(held['graph']['n_chars'][:, 0].float().mean())}), flush=True)


if __name__ == '__main__':
    main()
