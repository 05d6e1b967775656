"""The float64 CPU checker of the attention beam search with a character graph (ssasr_decode_beam_graph), written from
the semantics of include/ssasr.h: decode_checker.Model with the graph state carried by root / entries / child, so that
decode_checker.beam_search runs UNCHANGED on it -- a non-<EOS> entry gains graph_weight * arc[state][v], the <EOS> entry
graph_weight * fin[state], a forbidden arc gives -inf, and beam_search already drops -inf candidates.  It reads the
graph's three tables and start; it does not call CharGraph.score and shares nothing with the library's host code.

`RowModel` is a toy with the same interface whose score rows are a function of the prefix alone (no encoder, no
decoder), for properties that enumeration can check."""
import math

import numpy as np

import decode_checker as dc

NEG = -math.inf
EOS = dc.EOS


class GraphMixin:
    """The graph state on top of a model that has root / entries / child.  graph None or graph_weight 0: the term is
    left out (the tables are unread) and every result is the underlying model's."""

    def set_graph(self, graph, graph_weight):
        assert graph_weight >= 0.0 and math.isfinite(graph_weight) and (graph is not None or graph_weight == 0.0)
        self.graph, self.gw = graph, float(np.float32(graph_weight))       # the weight the kernel holds is a float
        self.on = graph is not None and graph_weight != 0.0
        if self.on:
            assert graph.n_classes == self.V
            self.arc, self.fin, self.nxt = graph.arc.astype(np.float64), graph.fin.astype(np.float64), graph.next
        self.walked = {}                    # prefix -> (state, G), filled as the search creates its hypotheses
        self.forbidden = 0                  # finite candidates that a forbidden arc removed

    def root(self):
        h = super().root()
        if self.on:
            h['gstate'], h['G'] = self.graph.start, 0.0
            self.walked = {(): (h['gstate'], 0.0)}
            self.forbidden = 0
        return h

    def entries(self, h, lam, lm_weight):
        entry, psi, alpha, nxt = super().entries(h, lam, lm_weight)
        if self.on:
            s = h['gstate']
            term = self.gw * self.arc[s]
            term[EOS] = self.gw * self.fin[s]
            self.forbidden += int(np.sum((np.asarray(entry) > NEG) & (term == NEG)))
            entry = np.asarray(entry, dtype=np.float64) + term
        return entry, psi, alpha, nxt

    def child(self, h, nxt, v, score, lam, psi):
        c = super().child(h, nxt, v, score, lam, psi)
        if self.on:
            s = h['gstate']
            c['gstate'], c['G'] = int(self.nxt[s, v]), h['G'] + self.arc[s, v]
            self.walked[tuple(c['prefix'])] = (c['gstate'], c['G'])
        return c

    def part(self, text, capped):
        """The graph part the search carried for an emitted hypothesis: G, + fin[state] when <EOS> ended it."""
        if not self.on:
            return 0.0
        s, G = self.walked[tuple(text)]
        return G if capped else G + self.fin[s]


class GraphModel(GraphMixin, dc.Model):
    """decode_checker.Model of a (fixture, frames) with a graph."""

    def __init__(self, fx, frames, graph=None, graph_weight=0.0, head_seed=dc.HEAD_SEED):
        super().__init__(fx, frames, head_seed)
        self.set_graph(graph, graph_weight)


def with_graph(m, graph, graph_weight):
    """A GraphModel that shares the (expensive) float64 model of the decode_checker.Model m."""
    g = GraphModel.__new__(GraphModel)
    g.__dict__.update(m.__dict__)
    g.set_graph(graph, graph_weight)
    return g


def beam_search(m, K, S, lm_weight, lam=0.0, beta=0.0, eta=0.0, tau=0.5, delta=None):
    """decode_checker.beam_search on a model with a graph -> its dict, with `parts`: each emitted hypothesis' graph
    part in output order, and `forbidden`: how many finite candidates a forbidden arc removed."""
    r = dc.beam_search(m, K, S, lm_weight, lam, beta, eta, tau, delta)
    r['parts'] = [m.part(h[0], h[3]) for h in r['hyps']]
    r['forbidden'] = m.forbidden
    return r


class _Rows:
    """A toy model for decode_checker.beam_search / forced: the score row of a prefix is log_softmax of a seeded
    N(0, 1) row that depends on the prefix alone, or, with `table`, the log of the same hand-built probabilities after
    every prefix.  No LM, no CTC, no attention (one frame that is never counted)."""
    T = 1

    def __init__(self, V, seed, scale=1.0, table=None):
        self.V, self.seed, self.scale, self.table = V, seed, scale, table

    def row(self, prefix):
        if self.table is not None:          # hand-built: the probabilities after every prefix
            return np.log(np.asarray(self.table, dtype=np.float64))
        rng = np.random.default_rng([self.seed, len(prefix)] + [int(c) for c in prefix])
        x = self.scale * rng.standard_normal(self.V)
        return x - (x.max() + math.log(np.exp(x - x.max()).sum()))

    def root(self):
        return dict(score=0.0, prefix=[], last=0, ctc=None, cum=np.zeros(1), cov=0)

    def entries(self, h, lam, lm_weight):
        assert lam == 0 and lm_weight is None
        return self.row(h['prefix']), None, np.zeros(1), {}

    def child(self, h, nxt, v, score, lam, psi):
        return dict(nxt, score=score, prefix=h['prefix'] + [v], last=v, ctc=None)


class RowModel(GraphMixin, _Rows):
    def __init__(self, V, seed, graph=None, graph_weight=0.0, scale=1.0, table=None):
        super().__init__(V, seed, scale, table)
        self.set_graph(graph, graph_weight)
