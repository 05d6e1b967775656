"""BUILD-DEFINED: word graphs for the CTC prefix beam search (ssasr_ctc_decode_word, include/ssasr.h; DESIGN.md section
4.26): the output is restricted to the words of a lexicon and ranked by a word-level n-gram LM.  Two parts over V
classes with a space class:

  the TRIE of the lexicon's spellings: child [N, V] int32, carc [N, V] float32 (finite, or -inf: forbidden), word [N]
  int32 (the word that ends at the node, -1: none), pen [N] float32;
  the WORD LM in back-off form: off [H + 1] delimits the states' rows of (wid, wlp, wnext), wid strictly ascending in a
  row; bow [H], bnext [H] (the back-off state, -1 for state 0), eos [H] = log P(</s> | h).  State 0 is the empty
  history and its row is dense (wid[e] == e).

A text's state is (n, h), the empty text's (0, 0).  A class c != space moves along the trie: arc carc[n][c], state
(child[n][c], h).  The space is allowed only where a word ends (word[n] >= 0): with (lp, h') = lookup(h, word[n]) the
arc is float32(pen[n] + lp) and the state (0, h').  G(text) is the sum of the arcs; a finished text adds fin(n, h) =
pen[n] + eos[h] where no word ends at n, and (the space arc) + eos[h'] where one does.

``WordGraph.build`` counts a Witten-Bell word n-gram from sentences and spreads each word's unigram score over its
spelling as a lookahead; ``to_char_graph`` expands the reachable (n, h) pairs into a dense char_graph.CharGraph (small
lexicons, and the tests' independent yardstick); ``to(device)`` uploads the tables once and holds the struct the C entry
takes.  All of it runs on the host in numpy."""
import bisect
import math
from collections import deque

import numpy as np

MAX_NODES = 1 << 20            # ssasr_ctc_decode_word's limit on N, H and W
MAX_CLASSES = 64               # the prefix search's limit on V
MAX_ORDER = 8                  # SSASR_WORD_MAX_ORDER: the rounds of a look-up
NEG = -math.inf

_INT_TABLES = ('child', 'word', 'off', 'wid', 'wnext', 'bnext')
_FLOAT_TABLES = ('carc', 'pen', 'wlp', 'bow', 'eos')
TABLES = ('child', 'carc', 'word', 'pen', 'off', 'wid', 'wlp', 'wnext', 'bow', 'bnext', 'eos')   # the struct's order


class WordGraph:
    def __init__(self, child, carc, word, pen, off, wid, wlp, wnext, bow, bnext, eos, space, blank=0):
        """Validates every table (ValueError) as the module's header states them; the tables are kept as int32 /
        float32 copies.  A look-up from any state must reach state 0 within MAX_ORDER rounds."""
        t = dict(child=child, carc=carc, word=word, pen=pen, off=off, wid=wid, wlp=wlp, wnext=wnext, bow=bow,
                 bnext=bnext, eos=eos)
        t = {k: np.asarray(v) for k, v in t.items()}
        for k in _INT_TABLES:
            if t[k].dtype.kind not in 'iu':
                raise ValueError('WordGraph: %s must hold integers, got %s' % (k, t[k].dtype))
        for k in _FLOAT_TABLES:
            if t[k].dtype.kind != 'f':
                raise ValueError('WordGraph: %s must hold floats, got %s' % (k, t[k].dtype))
            t[k] = t[k].astype(np.float32)
        if t['child'].ndim != 2 or t['carc'].shape != t['child'].shape or \
                t['word'].shape != t['child'].shape[:1] or t['pen'].shape != t['word'].shape:
            raise ValueError('WordGraph: child and carc must be [N, V], word and pen [N], got %r, %r, %r, %r'
                             % (t['child'].shape, t['carc'].shape, t['word'].shape, t['pen'].shape))
        N, V = t['child'].shape
        if not 1 <= N <= MAX_NODES or not 2 <= V <= MAX_CLASSES:
            raise ValueError('WordGraph: 1 <= N <= %d and 2 <= V <= %d, got N=%d V=%d' % (MAX_NODES, MAX_CLASSES, N, V))
        for name, v in (('space', space), ('blank', blank)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v < V:
                raise ValueError('WordGraph: %s must be a class in [0, %d), got %r' % (name, V, v))
        if space == blank:
            raise ValueError('WordGraph: the space class %d is the blank' % space)
        if t['off'].ndim != 1 or t['off'].shape[0] < 2 or t['bow'].shape != (t['off'].shape[0] - 1,) or \
                t['bnext'].shape != t['bow'].shape or t['eos'].shape != t['bow'].shape:
            raise ValueError('WordGraph: off must be [H + 1], bow, bnext and eos [H], got %r, %r, %r, %r'
                             % (t['off'].shape, t['bow'].shape, t['bnext'].shape, t['eos'].shape))
        H = t['bow'].shape[0]
        if t['wid'].ndim != 1 or t['wlp'].shape != t['wid'].shape or t['wnext'].shape != t['wid'].shape:
            raise ValueError('WordGraph: wid, wlp and wnext must be [E], got %r, %r, %r'
                             % (t['wid'].shape, t['wlp'].shape, t['wnext'].shape))
        E = t['wid'].shape[0]
        off = t['off'].astype(np.int64)
        if off[0] != 0 or off[-1] != E or (np.diff(off) < 0).any():
            raise ValueError('WordGraph: off must rise from 0 to E = %d' % E)
        W = int(off[1])
        if not 1 <= H <= MAX_NODES or not 1 <= W <= MAX_NODES:
            raise ValueError('WordGraph: 1 <= H <= %d and 1 <= W <= %d, got H=%d W=%d' % (MAX_NODES, MAX_NODES, H, W))
        if not np.array_equal(t['wid'][:W], np.arange(W)):
            raise ValueError('WordGraph: state 0\'s row must be dense: wid[e] == e for e < W = %d' % W)
        if E and (t['wid'].min() < 0 or t['wid'].max() >= W):
            raise ValueError('WordGraph: wid must lie in [0, %d)' % W)
        inner = np.ones(E, dtype=bool)                          # entries that have a predecessor in their own row
        inner[off[:-1][off[:-1] < E]] = False
        if (np.diff(t['wid'].astype(np.int64), prepend=-1)[inner] <= 0).any():
            raise ValueError('WordGraph: wid must be strictly ascending inside a state\'s row')
        if E and (t['wnext'].min() < 0 or t['wnext'].max() >= H):
            raise ValueError('WordGraph: wnext must lie in [0, %d)' % H)
        for k in ('pen', 'wlp', 'bow', 'eos'):
            if not np.isfinite(t[k]).all():
                raise ValueError('WordGraph: %s must be finite' % k)
        if np.isnan(t['carc']).any() or (t['carc'] == np.inf).any():
            raise ValueError('WordGraph: an arc is finite or -inf, never NaN or +inf')
        live = np.isfinite(t['carc'])
        live[:, [space, blank]] = False                         # those two columns are never read
        if live.any() and (t['child'][live].min() < 0 or t['child'][live].max() >= N):
            raise ValueError('WordGraph: child must lie in [0, %d) where the arc is finite' % N)
        if t['word'][0] != -1 or t['word'].min() < -1 or t['word'].max() >= W:
            raise ValueError('WordGraph: word must lie in [-1, %d) with word[0] == -1' % W)
        bnext = t['bnext'].astype(np.int64)
        if bnext[0] != -1 or (bnext[1:] < 0).any() or (bnext[1:] >= H).any():
            raise ValueError('WordGraph: bnext must be -1 for state 0 and a state in [0, %d) elsewhere' % H)
        at = np.arange(H)
        for _ in range(MAX_ORDER - 1):                          # MAX_ORDER rounds: the last one must be state 0's
            at = np.where(at > 0, bnext[at], 0)
        if at.any():
            raise ValueError('WordGraph: a back-off chain does not reach state 0 within %d rounds' % MAX_ORDER)
        for k in _INT_TABLES:
            setattr(self, k, np.ascontiguousarray(t[k], dtype=np.int32))
        for k in _FLOAT_TABLES:
            setattr(self, k, np.ascontiguousarray(t[k]))
        self.space, self.blank = int(space), int(blank)
        self._device, self._py = {}, None

    n_nodes = property(lambda self: self.child.shape[0])
    n_classes = property(lambda self: self.child.shape[1])
    n_states = property(lambda self: self.bow.shape[0])
    n_words = property(lambda self: int(self.off[1]))
    n_entries = property(lambda self: self.wid.shape[0])

    def to(self, device):
        """Uploads the tables to `device` once and holds them; -> (struct ssasr_word_graph, the tensors it points
        into)."""
        import torch
        from . import _lib
        key = str(torch.device(device))
        if key not in self._device:
            keep = [torch.from_numpy(getattr(self, k)).to(device) for k in TABLES]
            s = _lib.WordGraph(*[k.data_ptr() for k in keep], self.n_nodes, self.n_classes, self.n_states,
                               self.n_words, self.n_entries, self.space)
            self._device[key] = (s, keep)
        return self._device[key]

    def save(self, path):
        """One .npz: the eleven tables, space and blank."""
        with open(path, 'wb') as f:
            np.savez(f, space=np.int64(self.space), blank=np.int64(self.blank), **{k: getattr(self, k) for k in TABLES})

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            missing = (set(TABLES) | {'space', 'blank'}) - set(z.files)
            if missing:
                raise ValueError('WordGraph.load: %s lacks %s' % (path, sorted(missing)))
            return cls(*[z[k] for k in TABLES], int(z['space']), int(z['blank']))

    # ---- the walk in float64 over the float32 tables ----
    def _lists(self):
        """The tables as Python lists (float64 values of the float32 entries), made once: the walk is scalar code."""
        if self._py is None:
            self._py = {k: getattr(self, k).tolist() for k in TABLES}
        return self._py

    def lookup(self, h, w, rounds=None):
        """(log P(w | h) through the back-off chain, the state after w); rounds: a list that receives the number of
        rows searched."""
        t = self._lists()
        off, wid = t['off'], t['wid']
        acc, n = 0.0, 0
        while True:
            n += 1
            e = bisect.bisect_left(wid, w, off[h], off[h + 1])
            if e < off[h + 1] and wid[e] == w:
                if rounds is not None:
                    rounds.append(n)
                return acc + t['wlp'][e], t['wnext'][e]
            acc += t['bow'][h]
            h = t['bnext'][h]                                   # validated: state 0's dense row ends the chain

    def space_arc(self, n, h):
        """(the arc of the space out of (n, h) as the float32 value the search adds, the LM state behind it);
        (-inf, h) where no word ends at n."""
        t = self._lists()
        if t['word'][n] < 0:
            return NEG, h
        lp, h2 = self.lookup(h, t['word'][n])
        return float(np.float32(t['pen'][n] + lp)), h2

    def step(self, n, h, c):
        """(arc, (n', h')) of class c out of (n, h); a forbidden arc keeps the state."""
        if c == self.space:
            arc, h2 = self.space_arc(n, h)
            return arc, ((0, h2) if arc > NEG else (n, h))
        t = self._lists()
        arc = t['carc'][n][c]
        return arc, ((t['child'][n][c], h) if arc > NEG else (n, h))

    def fin(self, n, h):
        t = self._lists()
        if t['word'][n] < 0:
            return t['pen'][n] + t['eos'][h]
        arc, h2 = self.space_arc(n, h)
        return arc + t['eos'][h2]

    def score(self, labels):
        """(G(labels), (n, h)); (-inf, the state before the forbidden arc) once an arc is forbidden."""
        state, total = (0, 0), 0.0
        for c in labels:
            c = int(c)
            if not 0 <= c < self.n_classes or c == self.blank:
                raise ValueError('WordGraph.score: %d is no non-blank class of V=%d' % (c, self.n_classes))
            arc, nxt = self.step(*state, c)
            if arc == NEG:
                return NEG, state
            total, state = total + arc, nxt
        return total, state

    def to_char_graph(self, max_states=1 << 16):
        """The dense char_graph.CharGraph of the (n, h) pairs reachable from (0, 0): the same arcs, so the same G on
        every text, and fin rounded to float32.  ValueError once more than max_states pairs are reached."""
        from .char_graph import CharGraph
        V = self.n_classes
        ids = {(0, 0): 0}
        queue = deque(ids)
        nxt, arc, fin = [], [], []
        while queue:
            pair = queue.popleft()
            me = ids[pair]
            row_next, row_arc = np.full(V, me, dtype=np.int64), np.full(V, NEG)
            row_arc[self.blank] = 0.0
            for c in range(V):
                if c == self.blank:
                    continue
                a, to = self.step(*pair, c)
                if a == NEG:
                    continue
                if to not in ids:
                    if len(ids) >= max_states:
                        raise ValueError('WordGraph.to_char_graph: more than max_states = %d reachable pairs' % max_states)
                    ids[to] = len(ids)
                    queue.append(to)
                row_next[c], row_arc[c] = ids[to], a
            nxt.append(row_next)
            arc.append(row_arc)
            fin.append(self.fin(*pair))
        return CharGraph(np.stack(nxt), np.stack(arc), np.asarray(fin), 0)

    # ---- the builder ----
    @classmethod
    def build(cls, sentences, order, encode, n_classes, space, lexicon=None, lookahead=True, unfinished=-20.0, blank=0):
        """A lexicon trie with a Witten-Bell word n-gram LM (no discount to tune).  sentences: lists of words; each is
        counted with </s> appended, from its first word on (no padding).  encode(word) -> the word's class ids (non-empty,
        without space and blank; two words may not share a spelling).  lexicon: the words of the trie in id order
        (default: the sorted words seen); a word of it that no sentence holds gets the back-off floor; a sentence word
        outside it is a ValueError.  With c(h w) the times w followed the history h, c(h) = sum_w c(h w) and N1+(h) the
        number of distinct words (and </s>) seen after h:
          P(w | h) = (c(h w) + N1+(h) P(w | h')) / (c(h) + N1+(h)),   h' = h without its oldest word,
          the empty history backing off to the uniform distribution over the W words and </s>.
        States: the empty history and every history of length < order that was followed by something.  A state's row
        holds the words seen after it with the full interpolated value; bow[h] = log(N1+ / (c(h) + N1+)); wnext is the
        longest suffix of h.w that is a state; eos[h] = log P(</s> | h), fully resolved.
        The trie's arcs carry a lookahead: look[n] = the largest unigram log-probability of a word at or below n
        (look[0] = 0; all 0 with lookahead=False), carc[n][c] = look[child] - look[n], pen[n] = -look[n] where a word
        ends and unfinished - look[n] where none does (pen[0] = 0): G of whole words telescopes to sum_i
        log P(w_i | history), and the lookahead only steers the pruning.  Counts are exact integers, probabilities
        float64, the tables float32."""
        order, V, space, blank, unfinished = int(order), int(n_classes), int(space), int(blank), float(unfinished)
        if not 1 <= order <= MAX_ORDER:
            raise ValueError('WordGraph.build: order must be in 1..%d, got %d' % (MAX_ORDER, order))
        if not 2 <= V <= MAX_CLASSES or not 0 <= blank < V or not 0 <= space < V or space == blank:
            raise ValueError('WordGraph.build: space %d and blank %d must be two classes of V=%d (2..%d)'
                             % (space, blank, V, MAX_CLASSES))
        if not math.isfinite(unfinished):
            raise ValueError('WordGraph.build: unfinished must be finite, got %r' % (unfinished,))
        sentences = [list(s) for s in sentences]
        words = list(lexicon) if lexicon is not None else sorted({w for s in sentences for w in s})
        if not words or len(set(words)) != len(words):
            raise ValueError('WordGraph.build: the lexicon must hold at least one word and none twice')
        W = len(words)
        if W > MAX_NODES:
            raise ValueError('WordGraph.build: %d words, more than %d' % (W, MAX_NODES))
        wid_of = {w: i for i, w in enumerate(words)}
        end = W                                                 # </s> as a count key
        follow = {(): {}}                                       # history -> {word id or end: count}
        for s in sentences:
            try:
                seq = tuple(wid_of[w] for w in s) + (end,)
            except KeyError as e:
                raise ValueError('WordGraph.build: the word %r of a sentence is not in the lexicon' % (e.args[0],))
            for i, w in enumerate(seq):
                for n in range(min(i, order - 1) + 1):
                    row = follow.setdefault(seq[i - n:i], {})
                    row[w] = row.get(w, 0) + 1
        states = sorted(follow, key=lambda h: (len(h), h))      # the empty history is state 0
        if len(states) > MAX_NODES:
            raise ValueError('WordGraph.build: %d histories, more than %d states' % (len(states), MAX_NODES))
        ids = {h: i for i, h in enumerate(states)}
        uniform = 1.0 / (W + 1)
        prob, off, wid, wlp, wnext, bow, bnext, eos = {}, [0], [], [], [], [], [], []
        for h in states:                                        # shorter histories first: h' is done
            row = follow[h]
            total, distinct = sum(row.values()), len(row)
            lower = prob[h[1:]] if h else None
            seen = range(W) if not h else sorted(w for w in row if w != end)
            p = {}
            for w in list(seen) + [end]:
                below = lower[w] if h else uniform              # h w seen -> h' w seen; </s> is kept in every state
                p[w] = (row.get(w, 0) + distinct * below) / (total + distinct) if total else below
            prob[h] = p
            for w in seen:
                hw = (h + (w,))[-(order - 1):] if order > 1 else ()
                while hw not in ids:
                    hw = hw[1:]
                wid.append(w)
                wlp.append(math.log(p[w]))
                wnext.append(ids[hw])
            off.append(len(wid))
            bow.append(math.log(distinct / (total + distinct)) if total else 0.0)
            bnext.append(ids[h[1:]] if h else -1)
            eos.append(math.log(p[end]))
        # the trie
        kids, ends = [{}], [-1]
        for i, w in enumerate(words):
            spelling = [int(c) for c in encode(w)]
            if not spelling or any(not 0 <= c < V or c in (space, blank) for c in spelling):
                raise ValueError('WordGraph.build: the word %r is spelled %r: a non-empty sequence of classes in [0, %d) '
                                 'without space and blank' % (w, spelling, V))
            n = 0
            for c in spelling:
                if c not in kids[n]:
                    kids[n][c] = len(kids)
                    kids.append({})
                    ends.append(-1)
                n = kids[n][c]
            if ends[n] >= 0:
                raise ValueError('WordGraph.build: the words %r and %r share a spelling' % (words[ends[n]], w))
            ends[n] = i
        N = len(kids)
        if N > MAX_NODES:
            raise ValueError('WordGraph.build: %d trie nodes, more than %d' % (N, MAX_NODES))
        look = np.zeros(N)
        if lookahead:
            look[:] = NEG
            for n in range(N - 1, -1, -1):                      # a child has a larger index than its parent
                if ends[n] >= 0:
                    look[n] = max(look[n], wlp[ends[n]])        # state 0's row: the unigram
                for c in kids[n].values():
                    look[n] = max(look[n], look[c])
            look[0] = 0.0
        child = np.zeros((N, V), dtype=np.int64)
        carc = np.full((N, V), NEG)
        pen = np.zeros(N)
        for n in range(N):
            for c, to in kids[n].items():
                child[n, c], carc[n, c] = to, look[to] - look[n]
            if n:
                pen[n] = (0.0 if ends[n] >= 0 else unfinished) - look[n]
        return cls(child, carc, np.asarray(ends), pen, np.asarray(off), np.asarray(wid, dtype=np.int64), np.asarray(wlp),
                   np.asarray(wnext, dtype=np.int64), np.asarray(bow), np.asarray(bnext), np.asarray(eos), space, blank)
