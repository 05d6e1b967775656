"""The float64 CPU checker of the K-hypothesis decoders (ssasr_decode_beam / _ctc / _ex, ssasr_decode_sample), written
from the semantics of include/ssasr.h: ONE model of the decoder + LM step (las_oracle's OracleASR parts and the float64
GRU of test_gpu_decode), ONE beam search with the CTC term and the three extra terms as options, and the teacher-forced
score of a given text.  It shares nothing with the library's host code.  The CTC prefix scorer is the one that
test_ctc_decode_cpu.py pins by brute force and against torch's ctc_loss; the head's weights come from a seed
(las_oracle.seeded_generic_weights on an nn.Linear)."""
import math

import numpy as np
import torch
import torch.nn as nn

import las_oracle as lo
import test_ctc_decode_cpu as tcc
from test_gpu_decode import gru_cell64

EOS = 1
HEAD_SEED = 1
NEG = -math.inf
STATE = ('h1', 'c1', 'h2', 'c2', 'l1', 'l2')


class Model:
    """The float64 model of one (fixture, frames): encoder output, comp, the seeded head's lp (float64, and float32
    from a float32 product for the noise figure), and one decoder + LM step for any number of rows (the rows of a
    batch do not interact: every product is row by row)."""

    def __init__(self, fx, frames, head_seed=HEAD_SEED):
        from ss_asr_amd.charlm import CharLM
        dims = tuple(int(v) for v in fx['dims'])
        self.V, self.D, self.Hl = dims[0], dims[2], int(fx['lm_hidden'])
        torch.manual_seed(0)
        self.asr = lo.seeded_weights(lo.OracleASR(*dims, 1.0), int(fx['asr_weights_seed'])).double().eval()
        lm = lo.seeded_generic_weights(CharLM(self.V, self.Hl), int(fx['lm_weights_seed']))
        self.sd = {k: v.detach().double() for k, v in lm.state_dict().items()}
        self.gru = [[self.sd['layer_%d.%s' % (l, n)] for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')]
                    for l in (1, 2)]
        x = torch.from_numpy(fx['x'][:, :frames]).double()
        with torch.no_grad():
            feat, enc_len = self.asr.encoder(x, [x.shape[1]])
            self.feat = feat[0, :enc_len[0]]
            self.comp = torch.tanh(self.asr.attention.psi(feat))[0, :enc_len[0]]
            head = lo.seeded_generic_weights(nn.Linear(self.feat.shape[1], self.V), head_seed)
            self.lp = torch.log_softmax(self.feat @ head.weight.double().t() + head.bias.double(), -1).numpy()
            self.lp32 = torch.log_softmax(self.feat.float() @ head.weight.t() + head.bias, -1).numpy()
        self.T = self.lp.shape[0]

    def start(self, n=1):
        """Zero states of n rows."""
        z, zl = torch.zeros(n, self.D, dtype=torch.float64), torch.zeros(n, self.Hl, dtype=torch.float64)
        return dict(h1=z, c1=z, h2=z, c2=z, l1=zl, l2=zl)

    def step(self, st, last, lm=True):
        """States of n rows fed the characters `last` -> (log_softmax(speller) [n, V], log_softmax(lm) [n, V] (None
        and the LM states untouched without lm), the attention rows [n, T'], the advanced states)."""
        asr, sd = self.asr, self.sd
        with torch.no_grad():
            last = torch.tensor(last, dtype=torch.long)
            q = torch.tanh(asr.attention.phi(st['h1']))
            alpha = torch.softmax(q @ self.comp.t(), 1)
            inp = torch.cat([asr.embed.weight[last], alpha @ self.feat], 1)
            h1, c1 = asr.decoder.layer_1(inp, (st['h1'], st['c1']))
            h2, c2 = asr.decoder.layer_2(h1, (st['h2'], st['c2']))
            row = torch.log_softmax(asr.char_trans(h2), 1).numpy()
            l1, l2, lm_row = st['l1'], st['l2'], None
            if lm:
                l1 = gru_cell64(sd['emb.weight'][last], l1, *self.gru[0])
                l2 = gru_cell64(l1, l2, *self.gru[1])
                lm_row = torch.log_softmax(l2 @ sd['out.weight'].t() + sd['out.bias'], 1).numpy()
        return row, lm_row, alpha.numpy(), dict(h1=h1, c1=c1, h2=h2, c2=c2, l1=l1, l2=l2)

    def step_fn(self, lm_weight):
        """test_sample_cpu.sample_walk's step_fn; lm_weight None: no language model."""
        def fn(st, last):
            row, lm_row, _, nxt = self.step(st, last, lm=lm_weight is not None)
            return (row if lm_weight is None else row + lm_weight * lm_row).tolist(), nxt
        return fn

    def root(self):
        """The empty hypothesis."""
        return dict(self.start(), score=0.0, prefix=[], last=0, ctc=tcc.empty_prefix(self.lp), cum=np.zeros(self.T), cov=0)

    def entries(self, h, lam, lm_weight):
        """One hypothesis' step -> (its candidates' score entries [V] before the extra terms (-inf: never chosen), their
        CTC psi [V] (None at lam = 0), the attention row, the advanced states).  lm_weight None: no language model."""
        row, lm_row, alpha, nxt = self.step(h, [h['last']], lm=lm_weight is not None)
        entry, psi = row[0], None
        if lam > 0:
            psi = tcc.candidate_psi(self.lp, h['ctc'], EOS)
            with np.errstate(invalid='ignore'):
                entry = (1.0 - lam) * entry + lam * (psi - h['ctc'].psi)
        if lm_weight is not None:
            entry = entry + lm_weight * lm_row[0]
        return entry, psi, alpha[0], nxt

    def child(self, h, nxt, v, score, lam, psi):
        """h extended by the character v."""
        ctc = tcc.extend(self.lp, h['ctc'], v, psi[v]) if lam > 0 else h['ctc']
        return dict(nxt, score=score, prefix=h['prefix'] + [v], last=v, ctc=ctc)


def beam_search(m, K, S, lm_weight, lam=0.0, beta=0.0, eta=0.0, tau=0.5, delta=None):
    """The beam search of include/ssasr.h in float64: lam > 0 adds the CTC prefix score, beta / eta, tau / delta (None:
    off) the length bonus, the coverage term and the end detection.  -> dict(hyps = [(chars, score, step it ended at,
    capped, cov of the prefix)] in output order; gap: the smallest kept / dropped, kept / kept, emitted / emitted
    distance and stop-rule margin; tau_gap: the smallest |cum' - tau|; n_steps; fired: the stop rule ended the loop
    (with something live, by definition); early: it did so before the cap's last step; ran_out: a hypothesis was ended
    by <EOS> at a step where all its other candidates were at -inf)."""
    V = m.V
    live, done, gaps, tau_gap, n_steps, fired, ran_out = [m.root()], [], [], math.inf, 0, False, False
    for step in range(S):
        if not live:
            break
        n_steps = step + 1
        cands, nxt, psis, stuck = [], [], [], []
        for b, h in enumerate(live):
            entry, psi, alpha, n = m.entries(h, lam, lm_weight)
            inc = 0.0
            if eta != 0:
                n['cum'] = h['cum'] + alpha
                n['cov'] = int((n['cum'] > tau).sum())
                tau_gap = min(tau_gap, float(np.abs(n['cum'] - tau).min()))
                inc = eta * (n['cov'] - h['cov'])
            else:
                n['cum'], n['cov'] = h['cum'], 0
            nxt.append(n)
            psis.append(psi)
            stuck.append(all(entry[v] == NEG for v in range(V) if v != EOS))
            cands += [(h['score'] + float(entry[v]) + (beta if v != EOS else 0.0) + inc, b * V + v)
                      for v in range(V) if entry[v] > NEG]
        width = min(K - len(done), len(cands))
        order = sorted(cands, key=lambda c: (-c[0], c[1]))
        kept = order[:width]
        if len(order) > width:
            gaps.append(kept[-1][0] - order[width][0])
        gaps += [a[0] - b[0] for a, b in zip(kept, kept[1:])]
        new = []
        for score, flat in kept:
            b, v = divmod(flat, V)
            if v == EOS:
                done.append((list(live[b]['prefix']), score, step, False, nxt[b]['cov']))
                ran_out |= stuck[b]
            else:
                new.append(m.child(live[b], nxt[b], v, score, lam, psis[b]))
        live = new
        if delta is not None and done and live:
            ml, mf = max(h['score'] for h in live), max(d[1] for d in done)
            gaps.append(abs(ml - (mf - delta)))
            if ml < mf - delta:
                fired, live = True, []
                break
    done += [(h['prefix'], h['score'], S, True, h['cov']) for h in live]
    order = sorted(range(len(done)), key=lambda i: (-done[i][1], i))
    hyps = [done[i] for i in order]
    gaps += [a[1] - b[1] for a, b in zip(hyps, hyps[1:])]
    return dict(hyps=hyps, gap=float(min(gaps)) if gaps else math.inf, tau_gap=tau_gap, n_steps=n_steps, fired=fired,
                early=fired and n_steps < S, ran_out=ran_out)


def forced(m, text, ended, lam, lm_weight, tau=math.inf):
    """(the score without the extra terms of exactly `text` (ended: by <EOS>), cov(text) at tau counting <EOS>'s step
    when ended, the smallest |cum' - tau| on the way), teacher-forced through the float64 model."""
    h, total, cum, tau_gap = m.root(), 0.0, np.zeros(m.T), math.inf
    for v in list(text) + ([EOS] if ended else []):
        entry, psi, alpha, nxt = m.entries(h, lam, lm_weight)
        total += float(entry[v])
        cum = cum + alpha
        tau_gap = min(tau_gap, float(np.abs(cum - tau).min()))
        if v != EOS:
            h = m.child(h, nxt, v, total, lam, psi)
    return total, int((cum > tau).sum()), tau_gap


_models = {}


def model(golden, name, frames):
    """The Model of a golden fixture's first `frames` frames, built once."""
    if (name, frames) not in _models:
        _models[(name, frames)] = Model(golden(name), frames)
    return _models[(name, frames)]
