"""BUILD-DEFINED: character graphs for the CTC prefix beam search (ssasr_ctc_decode_graph, include/ssasr.h; DESIGN.md
section 4.22).  A graph over V classes is a complete deterministic weighted automaton: next [S, V] int32, arc [S, V]
float32 (finite, or -inf: the extension is forbidden), fin [S] float32 (finite) and a start state.  For a text
w = c_1 .. c_n: s_0 = start, s_i = next[s_{i-1}][c_i], G(w) = sum_i arc[s_{i-1}][c_i], state(w) = s_n; a finished text
scores G(w) + fin[state(w)].  The blank's column is never read by the search: the builders put next = s, arc = 0 there.

Builders: ``CharGraph.ngram`` (a count-based character n-gram LM, Witten-Bell interpolation, every arc fully backed
off), ``CharGraph.hotwords`` (the Aho-Corasick automaton of a phrase list: contextual biasing) and
``CharGraph.product`` (two graphs in one search).  All of it runs on the host in numpy; ``to(device)`` uploads the three
tables once and holds the struct the C entry takes."""
import math
from collections import deque

import numpy as np

MAX_STATES = 1 << 20           # ssasr_ctc_decode_graph's limit on S
MAX_CLASSES = 64               # the prefix search's limit on V


class CharGraph:
    def __init__(self, next, arc, fin, start=0):
        """Validates the tables (ValueError): next [S, V] integers in [0, S), arc [S, V] finite or -inf and never NaN
        or +inf, fin [S] finite, 1 <= S <= 1,048,576, 2 <= V <= 64, 0 <= start < S.  The tables are kept as int32 /
        float32 copies."""
        nxt, arc, fin = np.asarray(next), np.asarray(arc), np.asarray(fin)
        if nxt.ndim != 2 or arc.shape != nxt.shape or fin.shape != nxt.shape[:1]:
            raise ValueError('CharGraph: next and arc must be [S, V] and fin [S], got %r, %r, %r'
                             % (nxt.shape, arc.shape, fin.shape))
        S, V = nxt.shape
        if not 1 <= S <= MAX_STATES or not 2 <= V <= MAX_CLASSES:
            raise ValueError('CharGraph: 1 <= S <= %d and 2 <= V <= %d, got S=%d V=%d' % (MAX_STATES, MAX_CLASSES, S, V))
        if nxt.dtype.kind not in 'iu':
            raise ValueError('CharGraph: next must hold integers, got %s' % nxt.dtype)
        if nxt.min() < 0 or nxt.max() >= S:
            raise ValueError('CharGraph: next must lie in [0, %d), got %d .. %d' % (S, nxt.min(), nxt.max()))
        if arc.dtype.kind != 'f' or fin.dtype.kind != 'f':
            raise ValueError('CharGraph: arc and fin must hold floats, got %s, %s' % (arc.dtype, fin.dtype))
        arc32, fin32 = arc.astype(np.float32), fin.astype(np.float32)
        if np.isnan(arc32).any() or (arc32 == np.inf).any():
            raise ValueError('CharGraph: an arc is finite or -inf, never NaN or +inf')
        if not np.isfinite(fin32).all():
            raise ValueError('CharGraph: fin must be finite')
        if isinstance(start, bool) or not isinstance(start, (int, np.integer)) or not 0 <= start < S:
            raise ValueError('CharGraph: start must be a state in [0, %d), got %r' % (S, start))
        self.next = np.ascontiguousarray(nxt, dtype=np.int32)
        self.arc = np.ascontiguousarray(arc32)
        self.fin = np.ascontiguousarray(fin32)
        self.start = int(start)
        self._device = {}

    @property
    def n_states(self):
        return self.next.shape[0]

    @property
    def n_classes(self):
        return self.next.shape[1]

    def to(self, device):
        """Uploads the tables to `device` once and holds them; -> (struct ssasr_char_graph, the tensors it points
        into)."""
        import torch
        from . import _lib
        key = str(torch.device(device))
        if key not in self._device:
            keep = [torch.from_numpy(a).to(device) for a in (self.next, self.arc, self.fin)]
            s = _lib.CharGraph(keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), self.n_states,
                               self.n_classes, self.start)
            self._device[key] = (s, keep)
        return self._device[key]

    def save(self, path):
        """One .npz: next, arc, fin, start."""
        with open(path, 'wb') as f:
            np.savez(f, next=self.next, arc=self.arc, fin=self.fin, start=np.int64(self.start))

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            missing = {'next', 'arc', 'fin', 'start'} - set(z.files)
            if missing:
                raise ValueError('CharGraph.load: %s lacks %s' % (path, sorted(missing)))
            return cls(z['next'], z['arc'], z['fin'], int(z['start']))

    def score(self, labels):
        """(G(labels), state(labels)): the walk in float64 over the float32 table."""
        s, total = self.start, 0.0
        for c in labels:
            c = int(c)
            if not 0 <= c < self.n_classes:
                raise ValueError('CharGraph.score: %d is no class of V=%d' % (c, self.n_classes))
            total += float(self.arc[s, c])
            s = int(self.next[s, c])
        return total, s

    def scaled(self, weight):
        """The graph whose arcs and fin are weight times this one's (finite weight >= 0; a forbidden arc stays
        forbidden): how a factor of a product takes its weight."""
        weight = float(weight)
        if not (math.isfinite(weight) and weight >= 0.0):
            raise ValueError('CharGraph.scaled: the weight must be finite and >= 0, got %r' % (weight,))
        arc = self.arc.astype(np.float64)
        arc[np.isfinite(arc)] *= weight
        return CharGraph(self.next, arc, self.fin.astype(np.float64) * weight, self.start)

    @staticmethod
    def product(a, b, max_states=MAX_STATES):
        """The graph of the pairs (state of a, state of b) reachable from the two starts over arcs that neither
        factor forbids: arcs and fin add, so G = G_a + G_b and fin = fin_a + fin_b on every text.  An arc that a
        factor forbids is forbidden (next: the pair itself).  ValueError once more than max_states pairs are
        reached."""
        if a.n_classes != b.n_classes:
            raise ValueError('CharGraph.product: the factors have %d and %d classes' % (a.n_classes, b.n_classes))
        V = a.n_classes
        ids = {(a.start, b.start): 0}
        queue = deque(ids)
        nxt, arc, fin = [], [], []
        arc_a, arc_b = a.arc.astype(np.float64), b.arc.astype(np.float64)
        while queue:
            sa, sb = queue.popleft()
            me = ids[(sa, sb)]
            row_arc = arc_a[sa] + arc_b[sb]
            row_next = np.full(V, me, dtype=np.int64)
            for c in np.nonzero(np.isfinite(row_arc))[0]:
                pair = (int(a.next[sa, c]), int(b.next[sb, c]))
                if pair not in ids:
                    if len(ids) >= max_states:
                        raise ValueError('CharGraph.product: more than max_states = %d reachable pairs' % max_states)
                    ids[pair] = len(ids)
                    queue.append(pair)
                row_next[c] = ids[pair]
            nxt.append(row_next)
            arc.append(row_arc)
            fin.append(float(a.fin[sa]) + float(b.fin[sb]))
        return CharGraph(np.stack(nxt), np.stack(arc), np.asarray(fin), 0)

    @classmethod
    def ngram(cls, sequences, order, n_classes, eos, blank=0):
        """A character n-gram LM with Witten-Bell interpolation (no discount to tune).  sequences: label sequences
        without <SOS>; each is counted with the end class `eos` appended, from its first label on (no padding: a
        history of length n is counted where n labels precede).  With count(h c) the times c followed the history h,
        count(h) = sum_c count(h c) and N1+(h) the number of distinct classes seen after h:
          P(c | h) = (count(h c) + N1+(h) P(c | h')) / (count(h) + N1+(h)),   h' = h without its oldest label,
          the empty history backing off to the uniform distribution over the non-blank classes.
        States: the empty history and every history of length < order that was followed by a label; next[h][c] is the
        longest suffix of h.c that is a state; arc[h][c] = log P(c | h), fully resolved, so the search never backs
        off; fin[h] = arc[h][eos].  Counts are exact integers, probabilities float64, the tables float32."""
        order, V, eos, blank = int(order), int(n_classes), int(eos), int(blank)
        if order < 1:
            raise ValueError('CharGraph.ngram: order must be >= 1, got %d' % order)
        if not 2 <= V <= MAX_CLASSES or not 0 <= blank < V or not 0 <= eos < V or eos == blank:
            raise ValueError('CharGraph.ngram: eos %d and blank %d must be two classes of V=%d (2..%d)'
                             % (eos, blank, V, MAX_CLASSES))
        follow = {(): {}}                                      # history -> {class: count}
        for seq in sequences:
            seq = tuple(int(c) for c in seq)
            if any(not 0 <= c < V or c == blank or c == eos for c in seq):
                raise ValueError('CharGraph.ngram: a sequence holds labels in [0, %d) without blank and eos' % V)
            seq += (eos,)
            for i, c in enumerate(seq):
                for n in range(min(i, order - 1) + 1):
                    row = follow.setdefault(seq[i - n:i], {})
                    row[c] = row.get(c, 0) + 1
        states = sorted(follow, key=lambda h: (len(h), h))     # the empty history is state 0
        if len(states) > MAX_STATES:
            raise ValueError('CharGraph.ngram: %d histories, more than %d states' % (len(states), MAX_STATES))
        ids = {h: i for i, h in enumerate(states)}
        uniform = np.zeros(V)
        uniform[[c for c in range(V) if c != blank]] = 1.0 / (V - 1)
        prob = {}
        for h in states:                                       # shorter histories first: h' is done
            row = follow[h]
            lower = prob[h[1:]] if h else uniform
            counts = np.zeros(V)
            for c, k in row.items():
                counts[c] = k
            total, distinct = sum(row.values()), len(row)
            prob[h] = (counts + distinct * lower) / (total + distinct) if total else lower
        nxt = np.zeros((len(states), V), dtype=np.int64)
        arc = np.zeros((len(states), V))
        for h, i in ids.items():
            with np.errstate(divide='ignore'):
                arc[i] = np.log(prob[h])
            for c in range(V):
                hc = (h + (c,))[-(order - 1):] if order > 1 else ()
                while hc not in ids:
                    hc = hc[1:]
                nxt[i, c] = ids[hc]
            nxt[i, blank], arc[i, blank] = i, 0.0
        return cls(nxt, arc, arc[:, eos].copy(), 0)

    @classmethod
    def hotwords(cls, phrases, bonus, n_classes, blank=0):
        """Contextual biasing: the Aho-Corasick automaton of `phrases` (label sequences, non-empty, without the blank;
        a phrase given twice counts once), all at one bonus per character.
          G(w) = bonus * (sum of len(p) over every occurrence of every phrase p as a substring of w + pend(state(w))),
          pend(s) = depth(s) - (the length of the longest phrase that is a suffix of s's string, else 0): the advance
          paid for a partial match, retracted on a failure transition; fin[s] = -bonus * pend(s), so a FINISHED text
          scores exactly bonus * the summed length of the phrase occurrences in it.
        The arcs are the differences G(w.c) - G(w), which depend on the state alone."""
        V, blank, bonus = int(n_classes), int(blank), float(bonus)
        if not 2 <= V <= MAX_CLASSES or not 0 <= blank < V:
            raise ValueError('CharGraph.hotwords: blank %d must be a class of V=%d (2..%d)' % (blank, V, MAX_CLASSES))
        if not math.isfinite(bonus):
            raise ValueError('CharGraph.hotwords: bonus must be finite, got %r' % (bonus,))
        words = sorted({tuple(int(c) for c in p) for p in phrases})
        if not words:
            raise ValueError('CharGraph.hotwords: no phrase given')
        for p in words:
            if not p or any(not 0 <= c < V or c == blank for c in p):
                raise ValueError('CharGraph.hotwords: a phrase is a non-empty sequence of labels in [0, %d) without the '
                                 'blank, got %r' % (V, p))
        goto, depth, ends = [{}], [0], [0]                     # the trie; ends: the phrase's length where one ends
        for p in words:
            s = 0
            for c in p:
                if c not in goto[s]:
                    goto[s][c] = len(goto)
                    goto.append({})
                    depth.append(depth[s] + 1)
                    ends.append(0)
                s = goto[s][c]
            ends[s] = len(p)
        S = len(goto)
        if S > MAX_STATES:
            raise ValueError('CharGraph.hotwords: %d trie nodes, more than %d states' % (S, MAX_STATES))
        nxt = np.zeros((S, V), dtype=np.int64)
        fail = [0] * S
        longest = list(ends)                                   # the longest phrase that is a suffix of the node
        gained = list(ends)                                    # the summed length of every phrase that is one
        queue = deque()
        for c in range(V):
            if c in goto[0]:
                nxt[0, c] = goto[0][c]
                queue.append(goto[0][c])
        while queue:                                           # breadth first: a node's failure target is done
            s = queue.popleft()
            f = fail[s]
            longest[s] = longest[s] or longest[f]
            gained[s] += gained[f]
            for c in range(V):
                if c in goto[s]:
                    t = goto[s][c]
                    nxt[s, c] = t
                    fail[t] = int(nxt[f, c])
                    queue.append(t)
                else:
                    nxt[s, c] = nxt[f, c]
        pend = np.asarray(depth, dtype=np.float64) - np.asarray(longest, dtype=np.float64)
        gained = np.asarray(gained, dtype=np.float64)
        arc = bonus * (gained[nxt] + pend[nxt] - pend[:, None])
        nxt[:, blank], arc[:, blank] = np.arange(S), 0.0
        return cls(nxt, arc, -bonus * pend, 0)
