"""Records every output of the three CTC prefix beam searches (ops.ctc_decode, ops.ctc_decode_graph,
ops.ctc_decode_lm) at NON-ZERO weights on small seeded inputs, as one compressed .npz.  Run against a library built
from the commit whose bits are to be kept (SSASR_LIB names it); tests/test_gpu_ctc_prefix_parent.py regenerates the
same inputs through cases() and compares the build under test with the file, integers as they are and float32 scores
as bits.

Cells: T' in {1, 12, 40} x V in {4, 50, 64} x K in {1, 3, 32}, four rows of lengths T', T' - 1, 1 and 0.  V = 64 and
K = 32 are the limits; K = 32 at V = 64 gives a frame more than eight new members (the LM step's batches, the slot
allocator).  Per cell: plain; a random graph of 300 states with a tenth of its arcs -inf at graph_weight 0.7 and
length_bonus 0.3; a random CharLM of hidden size 16 (and 40 at one cell) at lm_weight 0.5 and length_bonus 0.3, with
eos = 1 and with eos = -1.

    SSASR_LIB=/path/to/libssasr_hip.so python tools/record_ctc_prefix.py [--out tests/golden/ctc_prefix_parent.npz]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES, CLASSES, BEAMS = (1, 12, 40), (4, 50, 64), (1, 3, 32)
GRAPH_STATES, GRAPH_WEIGHT, LM_WEIGHT, LENGTH_BONUS = 300, 0.7, 0.5, 0.3
LM_HIDDEN, LM_HIDDEN_WIDE, WIDE_CELL = 16, 40, (12, 50, 3)


def inputs_of(T, V):
    """(logits [4, T, V] float32, frame_lens [4] int32) of a cell's four rows."""
    z = (4.0 * np.random.default_rng([T, V, 101]).standard_normal((4, T, V))).astype(np.float32)
    return z, np.array([T, T - 1, 1, 0], dtype=np.int32)


def graph_of(V):
    """next, arc, fin, start of a random graph: a tenth of the arcs forbidden, the blank (0) a free self-loop."""
    S = GRAPH_STATES
    rng = np.random.default_rng([S, V, 103])
    nxt, arc = rng.integers(0, S, (S, V)), rng.standard_normal((S, V))
    arc[rng.random((S, V)) < 0.1] = -np.inf
    nxt[:, 0], arc[:, 0] = np.arange(S), 0.0
    return nxt, arc, rng.standard_normal(S), S - 1


def lm_of(V, H):
    """The CharLM's eleven arrays in ops._CHARLM_NAMES' order, float32."""
    rng = np.random.default_rng([V, H, 107])
    shapes = [(V, H), (3 * H, H), (3 * H, H), (3 * H,), (3 * H,), (3 * H, H), (3 * H, H), (3 * H,), (3 * H,), (V, H), (V,)]
    return [(0.5 * rng.standard_normal(s)).astype(np.float32) for s in shapes]


def cases():
    """Yields (key, variant, T, V, K, extra): variant 'plain', 'graph' or 'lm'; extra the LM's (H, eos) or None."""
    for T in FRAMES:
        for V in CLASSES:
            for K in BEAMS:
                cell = 'T%d_V%d_K%d' % (T, V, K)
                yield cell + '/plain', 'plain', T, V, K, None
                yield cell + '/graph', 'graph', T, V, K, None
                for H in (LM_HIDDEN,) + ((LM_HIDDEN_WIDE,) if (T, V, K) == WIDE_CELL else ()):
                    for eos in (1, -1):
                        yield '%s/lm_H%d_eos%d' % (cell, H, eos), 'lm', T, V, K, (H, eos)


_held = {}


def run_case(variant, T, V, K, extra, device='cuda:0'):
    """-> {name: numpy array} of every output of the variant's op on the cell's inputs."""
    import torch
    from ss_asr_amd import ops
    from ss_asr_amd.char_graph import CharGraph
    from ss_asr_amd.charlm import CharLM
    z, lens = inputs_of(T, V)
    z, lens = torch.from_numpy(z).to(device), torch.from_numpy(lens).to(device)
    if variant == 'plain':
        out = dict(zip(('chars', 'n_chars', 'scores', 'n_hyps'), ops.ctc_decode(z, lens, K)))
    elif variant == 'graph':
        if ('graph', V) not in _held:
            _held['graph', V] = CharGraph(*graph_of(V))
        out = ops.ctc_decode_graph(z, lens, K, _held['graph', V], GRAPH_WEIGHT, LENGTH_BONUS)
    else:
        H, eos = extra
        if ('lm', V, H) not in _held:
            lm = CharLM(V, H).to(device)
            with torch.no_grad():
                for name, a in zip(ops._CHARLM_NAMES, lm_of(V, H)):
                    dict(lm.named_parameters())[name].copy_(torch.from_numpy(a))
            _held['lm', V, H] = lm
        out = ops.ctc_decode_lm(z, lens, K, _held['lm', V, H], LM_WEIGHT, LENGTH_BONUS, eos)
    return {name: t.cpu().numpy() for name, t in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'ctc_prefix_parent.npz'))
    args = ap.parse_args()
    arrays = {}
    for key, variant, T, V, K, extra in cases():
        for name, a in run_case(variant, T, V, K, extra).items():
            arrays['%s/%s' % (key, name)] = a
    np.savez_compressed(args.out, **arrays)
    print('%d arrays, %d bytes -> %s' % (len(arrays), os.path.getsize(args.out), args.out))


if __name__ == '__main__':
    main()
