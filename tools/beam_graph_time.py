"""Milliseconds per launch of the attention beam search with a character graph in the search (ssasr_decode_beam_graph,
csrc/infer.hip) on tools/beam_time.py's shape: 32 utterances, T' = 100 encoder frames each, V = 50, 200 steps, random
weights, K in --beams; the graph is the order-4 character n-gram LM of tests/golden/charlm_dataset.txt (--order) at
weight 0.5.  The encoder outputs are random and formed once; each launch is timed alone, with events around it, warm,
median over --steps launches.  Timed in the same sitting at every K: ssasr_decode_beam_ex without the graph and without
a language model (the number to approach: the graph launch is reported as a ratio to it) and the same search with the
CharLM of the default hidden size at the same weight (the language model this path had before).  One JSON line per K.

    python tools/beam_graph_time.py [--steps 5] [--warmup 2] [--beams 1,8,32] [--frames 100] [--order 4]
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
    ap.add_argument('--max-steps', type=int, default=200)
    ap.add_argument('--order', type=int, default=4)
    ap.add_argument('--graph-weight', type=float, default=0.5)
    ap.add_argument('--lm-hidden', type=int, default=128)
    args = ap.parse_args()
    from ss_asr_amd import ops
    from ss_asr_amd.asr import ASR
    from ss_asr_amd.char_graph import CharGraph
    from ss_asr_amd.charlm import CharLM
    from ss_asr_amd.LMDataset import LMDataset
    dev, V, S, N, T = 'cuda:0', 50, args.max_steps, args.utts, args.frames
    text = LMDataset(os.path.join(ROOT, 'tests', 'golden', 'charlm_dataset.txt'), 8)
    graph = CharGraph.ngram([[text.char2idx[ch] for ch in w] for w in text.file.split(' ') if w], args.order, V, 1)
    torch.manual_seed(0)
    asr = ASR(V, 256, 256, 128, 80, 1.0).to(dev).eval()
    lm = CharLM(V, args.lm_hidden).to(dev).eval()
    feat = torch.tanh(torch.randn(N, T, 512, device=dev))          # bounded, as a BiLSTM's outputs are
    enc_len = torch.full((N,), T, device=dev, dtype=torch.int32)
    params, psi = asr._decoder_params(), (asr.attention.psi.weight, asr.attention.psi.bias)
    no_lm = (feat, enc_len, params, psi, None, 0.0, 1, S)
    with_lm = (feat, enc_len, params, psi, lm, args.graph_weight, 1, S)
    held = {}
    for K in [int(k) for k in args.beams.split(',')]:
        def fused():
            held['graph'] = ops.decode_beam_graph(*no_lm, K, None, graph=graph, graph_weight=args.graph_weight)

        def plain():
            held['plain'] = ops.decode_beam_ex(*no_lm, K, None)

        def charlm():
            held['lm'] = ops.decode_beam_ex(*with_lm, K, None)
        ms_graph = timed(fused, args.steps, args.warmup)
        ms_plain = timed(plain, args.steps, args.warmup)
        ms_lm = timed(charlm, args.steps, args.warmup)
        steps = {k: int(held[k][4].max()) for k in held}
        print(json.dumps({'shape': dict(N=N, T=T, S=S, V=V, K=K, order=args.order, states=graph.n_states,
                                        lm_hidden=args.lm_hidden), 'launches': args.steps,
                          'beam_graph_ms': ms_graph, 'beam_ms': ms_plain, 'beam_lm_ms': ms_lm, 'n_steps': steps,
                          'us_per_step': {k: 1e3 * ms / steps[k] for k, ms in
                                          (('graph', ms_graph), ('plain', ms_plain), ('lm', ms_lm))},
                          'to_beam': ms_graph / ms_plain, 'to_beam_lm': ms_graph / ms_lm,
                          'step_to_beam': (ms_graph / steps['graph']) / (ms_plain / steps['plain']),
                          'mean_chars': float(held['graph'][1][:, 0].float().mean())}), flush=True)


if __name__ == '__main__':
    main()
