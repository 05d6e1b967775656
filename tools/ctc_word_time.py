"""Milliseconds per launch of the CTC prefix beam search over a lexicon with a word n-gram LM in the search
(ssasr_ctc_decode_word, csrc/ctc.hip) on tools/ctc_graph_time.py's shape: 32 utterances, T' = 100 encoder frames each,
V = 50, K in --beams, random weights behind the head.  Two word graphs: 'golden', the words of
tests/golden/charlm_dataset.txt at order 3 (three long words: the trie forbids most extensions and almost no member
reaches a word end), and 'letters', every letter a one-letter word with an order-3 LM from random sentences (every
node below the root ends a word: the look-up runs for almost every new member, the unfavourable end).  The head's
logits are formed once; each launch is timed alone, with events around it, warm, median over --steps launches.  Timed
in the same sitting at every K: ssasr_ctc_decode and ssasr_ctc_decode_graph with the order-4 character n-gram.
The share of new members that ran a look-up and the mean number of rows a look-up searched are counted on the host,
by postprocess.ctc_prefix_beam_word_reference's trace over the first --stat-utts utterances.  One JSON line per K and
graph, also written to --out.

    python tools/ctc_word_time.py [--steps 5] [--warmup 2] [--beams 1,8,32] [--frames 100] [--out profiles/ctc_word_time.txt]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from beam_time import timed  # noqa: E402


def lookup_stats(graph, logits, K, weight):
    """(new members, those that ran a look-up, the rows their look-ups searched) over the utterances of logits, as the
    float64 checker's beams say."""
    from ss_asr_amd.postprocess import ctc_prefix_beam_word_reference
    new, ran, rows = 0, 0, []
    for z in logits:
        lp = torch.log_softmax(z.double(), -1).cpu().numpy()
        trace = []
        ctc_prefix_beam_word_reference(lp, K, graph, weight, trace=trace)
        before = frozenset({()})
        for beam in trace:
            for text in beam - before:
                new += 1
                n, h = graph.score(text)[1]
                if graph.word[n] >= 0:
                    ran += 1
                    graph.lookup(h, int(graph.word[n]), rows)
            before = beam
    return new, ran, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--beams', default='1,8,32')
    ap.add_argument('--utts', type=int, default=32)
    ap.add_argument('--frames', type=int, default=100)
    ap.add_argument('--order', type=int, default=3)
    ap.add_argument('--graph-weight', type=float, default=0.5)
    ap.add_argument('--stat-utts', type=int, default=2)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ctc_word_time.txt'))
    args = ap.parse_args()
    from ss_asr_amd import ops
    from ss_asr_amd.char_graph import CharGraph
    from ss_asr_amd.LMDataset import LMDataset
    from ss_asr_amd.word_graph import WordGraph
    dev, V, N, T = 'cuda:0', 50, args.utts, args.frames
    text = LMDataset(os.path.join(ROOT, 'tests', 'golden', 'charlm_dataset.txt'), 8)
    words = [w for w in text.file.split(' ') if w]
    space = text.char2idx[' ']
    chars = CharGraph.ngram([[text.char2idx[ch] for ch in w] for w in words], 4, V, 1)
    letters = sorted(set(''.join(words)))
    rng = np.random.default_rng(0)
    graphs = {
        'golden': WordGraph.build([words], args.order, lambda w: [text.char2idx[ch] for ch in w], V, space),
        'letters': WordGraph.build([[letters[i] for i in rng.integers(0, len(letters), rng.integers(1, 9))]
                                    for _ in range(400)], args.order, lambda w: [text.char2idx[w]], V, space,
                                   lexicon=letters)}
    torch.manual_seed(0)
    head = torch.nn.Linear(512, V).to(dev)
    feat = torch.tanh(torch.randn(N, T, 512, device=dev))          # bounded, as a BiLSTM's outputs are
    enc_len = torch.full((N,), T, device=dev, dtype=torch.int32)
    held, lines = {}, []
    with torch.no_grad():
        logits = ops.gemm(feat.view(N * T, 512), head.weight, bias=head.bias).view(N, T, V)
        for K in [int(k) for k in args.beams.split(',')]:
            ms_ctc = timed(lambda: held.update(ctc=ops.ctc_decode(logits, enc_len, K)), args.steps, args.warmup)
            ms_graph = timed(lambda: held.update(graph=ops.ctc_decode_graph(logits, enc_len, K, chars, args.graph_weight)),
                             args.steps, args.warmup)
            for name, graph in graphs.items():
                ms_word = timed(lambda: held.update(word=ops.ctc_decode_word(logits, enc_len, K, graph, args.graph_weight)),
                                args.steps, args.warmup)
                new, ran, rows = lookup_stats(graph, logits[:args.stat_utts], K, args.graph_weight)
                lines.append(json.dumps({
                    'shape': dict(N=N, T=T, V=V, K=K, order=args.order, lexicon=name, words=graph.n_words,
                                  nodes=graph.n_nodes, lm_states=graph.n_states, entries=graph.n_entries),
                    'launches': args.steps, 'ctc_word_ms': ms_word, 'ctc_ms': ms_ctc, 'ctc_graph_ms': ms_graph,
                    'us_per_frame': 1e3 * ms_word / T, 'to_ctc': ms_word / ms_ctc, 'to_ctc_graph': ms_word / ms_graph,
                    'new_members': new, 'lookup_share': ran / max(new, 1),
                    'mean_rows_searched': float(np.mean(rows)) if rows else 0.0,
                    'mean_chars': float(held['word']['n_chars'][:, 0].float().mean())}))
                print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
