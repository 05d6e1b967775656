"""Host-side metrics of the reference (src/postprocess.py): character
accuracy, word-level edit-distance error, attention images, EOS trimming.
The reference uses the `editdistance` package; a small Levenshtein routine
replaces it here."""
import math

import numpy as np
import torch


def trim_eos(sequence):
    """Keep everything up to and including the first '>' (index 1)."""
    out = []
    for ch in sequence:
        out.append(int(ch))
        if int(ch) == 1:
            break
    return out


def edit_distance(a, b):
    """Levenshtein distance between two sequences of hashables."""
    if len(a) < len(b):
        a, b = b, a
    prev = list(range(len(b) + 1))
    for i, ca in enumerate(a, 1):
        cur = [i]
        for j, cb in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (ca != cb)))
        prev = cur
    return prev[-1]


def edit_ops(hyp, ref):
    """BUILD-DEFINED: (S, D, I) of hypothesis `hyp` against reference `ref` (sequences of hashables), defined so
    that it is exact: an alignment costs (S + D + I, S) and the result is the lexicographic minimum over all
    alignments -- fewest edits, among those fewest substitutions.  With I - D = len(hyp) - len(ref) and S + D + I =
    the distance the three counts are unique (no traceback, no traversal order).  Reference 'ab' against
    hypothesis 'ba' is (0, 1, 1), not (2, 0, 0).  The checker of ssasr_edit_score (include/ssasr.h) and ASR.score's
    path for rows past the kernel's limits."""
    prev = [(j, 0) for j in range(len(ref) + 1)]
    for i, ch in enumerate(hyp, 1):
        cur = [(i, 0)]
        for j, cr in enumerate(ref, 1):
            ne = int(ch != cr)
            d, s = prev[j - 1]
            cur.append(min((d + ne, s + ne), (prev[j][0] + 1, prev[j][1]), (cur[j - 1][0] + 1, cur[j - 1][1])))
        prev = cur
    dist, s = prev[-1]
    return s, (dist - s - len(hyp) + len(ref)) // 2, (dist - s + len(hyp) - len(ref)) // 2


def score_sequences(ids, space, first_char=2):
    """What the scorer compares for one row of token ids: (characters, words).  Ids < first_char are dropped (with
    the Mapper: `<`, which is also the pad, and `>`; `$` stays); words are the maximal runs of tokens != space as
    tuples, i.e. str.split(): no empty words, none at all in an empty row."""
    chars = [int(c) for c in ids if int(c) >= first_char]
    words, cur = [], []
    for c in chars:
        if c == space:
            if cur:
                words.append(tuple(cur))
            cur = []
        else:
            cur.append(c)
    if cur:
        words.append(tuple(cur))
    return chars, words


def edit_counts(hyp_ids, ref_ids, space, first_char=2):
    """One row of ssasr_edit_score on the host: [char S, D, I, N, word S, D, I, N] (N: the reference's count)."""
    hc, hw = score_sequences(hyp_ids, space, first_char)
    rc, rw = score_sequences(ref_ids, space, first_char)
    return list(edit_ops(hc, rc)) + [len(rc)] + list(edit_ops(hw, rw)) + [len(rw)]


def mwer_reference(logits, rows, n_hyps, counts, unit, ce_w=None, *, posterior='renorm'):
    """BUILD-DEFINED: the MWER loss of ssasr_mwer_loss_fwd (include/ssasr.h) restated in float64 torch, on any
    device, differentiable by autograd -- what the kernel is defined and tested against.
    logits [R, U, V] of R = G * M teacher-forced rows (row g * M + k: candidate k of group g); rows [R, >= U + 1]
    integer labels (the label of step t is rows[r, t + 1], 0 unlabelled); n_hyps [G]: the hypothesis set of group g
    is its first clamp(n_hyps[g], 0, M) rows; counts [R, 8]: ssasr_edit_score's rows; unit 0 | 'char' or 1 | 'word';
    ce_w [R] or None: absolute weights of the rows' negative log-likelihoods.
      logP_r = sum over labelled t of log_softmax(logits[r, t])[label];  p_hat = softmax of logP over the set;
      risk_g = sum_k p_hat_k (S + D + I)_k;  loss = mean_g risk_g + sum_r ce_w[r] (-logP_r).
    posterior 'uniform' (ssasr_mwer_loss_fwd_ex's Monte-Carlo form, for sets of samples drawn from the model):
    p_hat_k = 1 / |S_g| inside the set, whatever logP is; risk_g is then the set's mean risk and does not depend on
    the logits, so the risk term enters the graph as the score-function surrogate sum_r c_r logP_r with the detached
    c_r = (1 / G) (1 / |S_g|) (risk_r - risk_g), its own value subtracted again: the loss VALUE is as above, its
    gradient is the estimator's (the baseline risk_g includes the row itself; a set of one gets no risk gradient).
    -> (loss, risk [G], p_hat [R] with 0 outside the sets), all float64."""
    if posterior not in ('renorm', 'uniform'):
        raise ValueError("mwer_reference: posterior must be 'renorm' or 'uniform', got %r" % (posterior,))
    unit = {'char': 0, 'word': 1}.get(unit, unit)
    if unit not in (0, 1):
        raise ValueError("mwer_reference: unit must be 'char' or 'word', got %r" % (unit,))
    z = logits.to(torch.float64)
    R, U, V = z.shape
    G = int(n_hyps.shape[0])
    M = R // G if G else 1
    lab = torch.zeros(R, U, dtype=torch.long, device=z.device)
    have = min(U, rows.shape[1] - 1)
    lab[:, :have] = rows[:, 1:1 + have].to(torch.long)
    if bool(((lab < 0) | (lab >= V)).any()):
        raise ValueError('mwer_reference: a label names no class')
    logp = (torch.log_softmax(z, -1).gather(2, lab.unsqueeze(2)).squeeze(2) * (lab != 0)).sum(1)
    err = counts.to(torch.float64)[:, 4 * unit:4 * unit + 3].sum(1).view(G, M)
    inside = torch.arange(M, device=z.device).unsqueeze(0) < n_hyps.to(torch.long).clamp(0, M).unsqueeze(1)
    # an empty set is left unmasked (a row of -inf would put NaNs into the graph) and zeroed with the rest below
    masked = ~inside & inside.any(1, keepdim=True)
    p_hat = torch.softmax(logp.view(G, M).masked_fill(masked, -math.inf), 1)
    p_hat = torch.where(inside, p_hat, torch.zeros_like(p_hat))
    if posterior == 'uniform':
        p_hat = inside.to(torch.float64) / inside.sum(1, keepdim=True).clamp(min=1)
    risk = (p_hat * err).sum(1)
    loss = risk.sum() / max(G, 1)
    if posterior == 'uniform':
        surrogate = ((p_hat * (err - risk.unsqueeze(1))).reshape(R) * logp).sum() / max(G, 1)
        loss = loss + surrogate - surrogate.detach()
    if ce_w is not None:
        loss = loss - (ce_w.to(torch.float64) * logp).sum()
    return loss, risk, p_hat.reshape(R)


def edit_total(a, b):
    """S + D + I of edit_ops(a, b), the plain edit distance.  A common prefix and a common suffix are cut first: the
    distance (not the split into S, D, I) is unchanged by that, and the entries of an n-best list share most of
    their length."""
    lo, n = 0, min(len(a), len(b))
    while lo < n and a[lo] == b[lo]:
        lo += 1
    hi = 0
    while hi < n - lo and a[len(a) - 1 - hi] == b[len(b) - 1 - hi]:
        hi += 1
    return sum(edit_ops(a[lo:len(a) - hi], b[lo:len(b) - hi]))


def mbr_reference(hyps, n_hyps, scores, space, first_char=2, unit='word', posterior='softmax', scale=1.0):
    """BUILD-DEFINED: minimum-Bayes-risk selection, ssasr_mbr_select (include/ssasr.h) restated in pure Python /
    float64 on top of edit_ops and score_sequences -- what the kernel is defined and tested against, and ASR.mbr's
    path for groups past the kernel's limits.
    hyps[n][k]: the token ids of hypothesis k of utterance n, already cut to its length (every utterance has the same
    number K of rows); n_hyps[n]: the set S_n is the rows k < clamp(n_hyps[n], 0, K); scores[n][k] (None with
    posterior 'uniform'); unit 'char' | 'word' (or 0 | 1); posterior 'softmax' | 'uniform' (or 0 | 1).
      pair[n][k][j] = [character, word] S + D + I of hypothesis k against hypothesis j, -1 outside the set;
      p_j = exp(x_j - LSE x) over the finite x_j = scale * score_j (0 for a non-finite one; uniform if none is
      finite), or 1 / |S_n|;  risk[n][k] = sum_j p_j pair[n][k][j][unit] in the order j = 0 .. K - 1, inf outside the
      set;  best[n] = the lowest k of minimal risk, -1 for an empty set.
    -> (best [N], risk [N][K], pair [N][K][K][2]) as lists."""
    unit = {'char': 0, 'word': 1}.get(unit, unit)
    if unit not in (0, 1):
        raise ValueError("mbr_reference: unit must be 'char' or 'word', got %r" % (unit,))
    posterior = {'softmax': 0, 'uniform': 1}.get(posterior, posterior)
    if posterior not in (0, 1):
        raise ValueError("mbr_reference: posterior must be 'softmax' or 'uniform', got %r" % (posterior,))
    scale = float(scale)
    if not (math.isfinite(scale) and scale >= 0.0):
        raise ValueError('mbr_reference: scale must be finite and >= 0, got %r' % (scale,))
    best, risks, pairs = [], [], []
    for n, rows in enumerate(hyps):
        K = len(rows)
        nh = min(max(int(n_hyps[n]), 0), K)
        seqs = [score_sequences(rows[k], space, first_char) for k in range(nh)]
        pair = [[[-1, -1] for _ in range(K)] for _ in range(K)]
        for k in range(nh):
            pair[k][k] = [0, 0]
            for j in range(k):
                pair[k][j] = pair[j][k] = [edit_total(seqs[k][u], seqs[j][u]) for u in (0, 1)]
        p = [1.0 / nh] * nh if nh else []
        if posterior == 0 and nh:
            with np.errstate(all='ignore'):     # inf * 0 is the non-finite entry the definition names
                # the entry takes scale and scores as floats; the product is formed in double
                x = [float(np.float64(np.float32(scale)) * np.float64(np.float32(scores[n][k]))) for k in range(nh)]
            finite = [v for v in x if math.isfinite(v)]
            if finite:
                m = max(finite)
                lse = m + math.log(sum(math.exp(v - m) for v in x if math.isfinite(v)))
                p = [math.exp(v - lse) if math.isfinite(v) else 0.0 for v in x]
        risk = [math.inf] * K
        for k in range(nh):
            acc = 0.0
            for j in range(nh):
                acc = acc + p[j] * float(pair[k][j][unit])
            risk[k] = acc
        best.append(min(range(nh), key=lambda k: (risk[k], k)) if nh else -1)
        risks.append(risk)
        pairs.append(pair)
    return best, risks, pairs


def rescore_reference(logits, lm_logits, rows, n_hyps, first, n_chars, steps, *, att_weight=1.0, lm_weight=0.0,
                      first_weight=0.0, length_bonus=0.0, dtype=np.float64):
    """BUILD-DEFINED: n-best rescoring, ssasr_rescore (include/ssasr.h) restated over numpy rows and Python lists --
    what the kernel is defined and tested against.  logits [R, U, V] of R = G * M teacher-forced rows (row g * M + k:
    candidate k of group g); lm_logits the same shape or None; rows [R, cols] integer labels (the label of step t is
    rows[r][t + 1]; 0, an id outside 1 .. V - 1 and a column past cols are unlabelled); n_hyps [G]; first [G][K]
    first-pass scores and n_chars [G][K], K <= M; steps: the list's row length, which caps a length.  Every sum runs
    in `dtype` (float64; float32 measures the arithmetic's noise).
      att_k = sum over labelled t of log_softmax(logits[r, t])[label], in ascending t; lm_k the same over lm_logits
      (0 without); len_k = clamp(n_chars, 0, steps); total_k = att_weight att_k + lm_weight lm_k + first_weight
      first_k + length_bonus len_k, a term whose weight is exactly 0 being left out; the weights and first are taken
      as float32 values.  Rank: non-increasing total as rounded to float32, equal values in slot order, NaN as -inf.
    -> (order [G][K], total [G][K], parts [G][K][3] = (att, lm, first)) as lists in rank order, unrounded; ranks from
    clamp(n_hyps[g], 0, K) on hold -1, 0.0 and zeros."""
    z = np.asarray(logits, dtype=dtype)
    zl = None if lm_logits is None else np.asarray(lm_logits, dtype=dtype)
    rows = np.asarray(rows)
    R, U, V = z.shape
    G = len(n_hyps)
    M = R // G if G else 1
    K = len(first[0]) if G else 0
    w = [dtype(np.float32(v)) for v in (att_weight, lm_weight, first_weight, length_bonus)]

    def seq_logp(zr, r):
        acc = dtype(0)
        for t in range(U):
            lab = int(rows[r][t + 1]) if t + 1 < rows.shape[1] else 0
            if not 0 < lab < V:
                continue
            m = zr[t].max()
            acc = acc + (zr[t][lab] - (m + np.log(np.exp(zr[t] - m).sum(dtype=dtype))))
        return acc

    orders, totals, parts = [], [], []
    with np.errstate(all='ignore'):
        for g in range(G):
            n = min(max(int(n_hyps[g]), 0), K)
            cand = []
            for k in range(n):
                r = g * M + k
                att = seq_logp(z[r], r)
                lm = seq_logp(zl[r], r) if zl is not None else dtype(0)
                f = dtype(np.float32(first[g][k]))
                length = min(max(int(n_chars[g][k]), 0), int(steps))
                total = dtype(0)
                for weight, term in zip(w, (att, lm, f, dtype(length))):
                    if weight != 0:
                        total = total + weight * term
                key = np.float32(total)
                cand.append((-math.inf if np.isnan(key) else float(key), k, float(total), [float(att), float(lm), float(f)]))
            ranked = sorted(cand, key=lambda c: (-c[0], c[1]))
            orders.append([c[1] for c in ranked] + [-1] * (K - n))
            totals.append([c[2] for c in ranked] + [0.0] * (K - n))
            parts.append([c[3] for c in ranked] + [[0.0, 0.0, 0.0] for _ in range(K - n)])
    return orders, totals, parts


def ctc_prefix_beam_reference(lp, K, blank=0, dtype=np.float64, trace=None):
    """BUILD-DEFINED: CTC-only decoding, ssasr_ctc_decode (include/ssasr.h) restated over Python tuples as texts --
    what the kernel is defined and tested against.  lp [T, V]: one utterance's log-probabilities, already cut to its
    frames; every sum runs in `dtype` (float64; float32 measures the arithmetic's noise).
    K = 0, the best path: per frame the class of the largest entry (the lowest index among equals), repeats merged,
    blanks removed; score = the sum of the chosen entries.
    K >= 1, prefix beam search over TEXTS, a dict from text to (g_b, g_n): the log-probabilities of the labellings of
    the frames so far that collapse to the text and end in a blank / a non-blank, restricted to labellings whose
    every earlier prefix was in its frame's beam.  Frame t's candidates are the members u and every u + (c,) for a
    non-blank c; with either(u) = logaddexp(g_b(u), g_n(u)) a candidate w = p + (c,) gets
      g_b'(w) = lp[t, blank] + either(w) if w is a member, else -inf
      g_n'(w) = lp[t, c] + logaddexp(g_n(w) if w is a member, (g_b(p) if p ends in c else either(p)) if p is a member)
    (an absent term is -inf; the empty text has g_n' = -inf), and the K finite candidates with the largest
    logaddexp(g_b', g_n') are the next members.
    -> ([(text, score)] best first, the smallest gap that any frame left between the lowest kept and the highest
    dropped total -- inf when nothing finite was ever dropped: below it a rounding can change the search).  trace: a
    list that receives each frame's beam as a frozenset of texts (K >= 1)."""
    lp = np.asarray(lp, dtype=dtype)
    K, blank = int(K), int(blank)
    if lp.ndim != 2:
        raise ValueError('ctc_prefix_beam_reference: lp must be [T, V], got %r' % (lp.shape,))
    if K < 0:
        raise ValueError('ctc_prefix_beam_reference: K must be >= 0, got %d' % K)
    if np.dtype(dtype) == np.float64:                           # Python floats ARE float64, and ten times faster
        rows, zero, neg = lp.tolist(), 0.0, -math.inf

        def lae(a, b):
            if a < b:
                a, b = b, a
            return a if b == -math.inf else a + math.log1p(math.exp(b - a))
    else:
        rows, zero, neg, lae = [list(row) for row in lp], dtype(0), dtype(-np.inf), np.logaddexp
    if K == 0:
        path = [int(np.argmax(row)) for row in lp]
        text = tuple(c for t, c in enumerate(path) if c != blank and (t == 0 or c != path[t - 1]))
        score = zero
        for t, c in enumerate(path):
            score = score + rows[t][c]
        return [(text, float(score))], math.inf
    beam = {(): (zero, neg)}
    gap = math.inf
    classes = [c for c in range(lp.shape[1]) if c != blank]
    for row in rows:
        either = {u: lae(g[0], g[1]) for u, g in beam.items()}
        new, total = {}, {}
        for w in set(beam) | {u + (c,) for u in beam for c in classes}:
            g_b = row[blank] + either[w] if w in beam else neg
            g_n = neg
            if w:
                p, c = w[:-1], w[-1]
                stay = beam[w][1] if w in beam else neg
                grow = neg
                if p in beam:
                    grow = beam[p][0] if p and p[-1] == c else either[p]
                g_n = row[c] + lae(stay, grow)
            new[w] = (g_b, g_n)
            total[w] = lae(g_b, g_n)
        ranked = sorted((w for w in new if total[w] > neg), key=lambda w: (-total[w], w))
        if len(ranked) > K:
            gap = min(gap, float(total[ranked[K - 1]] - total[ranked[K]]))
        beam = {w: new[w] for w in ranked[:K]}
        if trace is not None:
            trace.append(frozenset(beam))
    return sorted(((w, float(lae(g[0], g[1]))) for w, g in beam.items()), key=lambda e: (-e[1], e[0])), gap


CHARLM_FIELDS = ('emb', 'w_ih1', 'w_hh1', 'b_ih1', 'b_hh1', 'w_ih2', 'w_hh2', 'b_ih2', 'b_hh2', 'w_out', 'b_out')


def ctc_prefix_beam_lm_reference(lp, K, lm, lm_weight=0.0, length_bonus=0.0, eos=-1, blank=0, dtype=np.float64,
                                 trace=None, parts=None):
    """BUILD-DEFINED: CTC prefix beam search with the CharLM in the ranking, ssasr_ctc_decode_lm (include/ssasr.h)
    restated over Python tuples as texts -- what the kernel is defined and tested against.  lp, K, blank, dtype and
    trace as ctc_prefix_beam_reference takes them (K >= 1); lm: the CharLM's eleven arrays in struct ssasr_charlm's
    field order (CHARLM_FIELDS; a dict by those names or a sequence; None at lm_weight 0), evaluated here in `dtype`.
      L(w) = sum_i log_softmax(lm_out(0, c_1 .. c_{i-1}))[c_i]: class 0 is fed from zero states, then each character;
      two GRU cells (r, z, n) and the output layer; a row is y - max - log(sum exp(y - max)) over all V classes.
      Frame t: the candidates and their g_b', g_n' are ctc_prefix_beam_reference's; a candidate's key is
      logaddexp(g_b', g_n') + lm_weight L(w) + length_bonus len(w), a term whose weight is exactly 0 left out (the
      weights are taken as float32 values); the K finite candidates with the largest keys are the next members.
      L(u + (c,)) = L(u) + row(u)[c]: only members are ever fed to the LM.
      After the last frame, with eos >= 0 and lm_weight != 0: total = key + lm_weight row(w)[eos].
    -> ([(text, total)] best first, gap): gap is the smallest difference that any frame left between the lowest kept
    and the highest dropped key, or that the final order left between adjacent totals (inf when neither occurred).
    parts: a list that receives (CTC part, LM part with the end term) per returned entry."""
    lp = np.asarray(lp, dtype=dtype)
    K, blank, eos = int(K), int(blank), int(eos)
    if lp.ndim != 2:
        raise ValueError('ctc_prefix_beam_lm_reference: lp must be [T, V], got %r' % (lp.shape,))
    if K < 1:
        raise ValueError('ctc_prefix_beam_lm_reference: K must be >= 1, got %d' % K)
    V = lp.shape[1]
    if eos >= V:
        raise ValueError('ctc_prefix_beam_lm_reference: eos %d is no class of V=%d' % (eos, V))
    f64 = np.dtype(dtype) == np.float64
    alpha, beta = float(np.float32(lm_weight)), float(np.float32(length_bonus))
    if not (math.isfinite(alpha) and math.isfinite(beta)):
        raise ValueError('ctc_prefix_beam_lm_reference: the weights must be finite')
    use_lm = alpha != 0.0
    if f64:                                                     # Python floats ARE float64, and ten times faster
        rows, zero, neg = lp.tolist(), 0.0, -math.inf

        def lae(a, b):
            if a < b:
                a, b = b, a
            return a if b == -math.inf else a + math.log1p(math.exp(b - a))
    else:
        rows, zero, neg, lae = [list(row) for row in lp], dtype(0), dtype(-np.inf), np.logaddexp
        alpha, beta = dtype(alpha), dtype(beta)
    states, L = {}, {(): zero}
    if use_lm:
        if lm is None:
            raise ValueError('ctc_prefix_beam_lm_reference: lm_weight %g needs a language model' % alpha)
        arrs = [np.asarray(lm[n] if isinstance(lm, dict) else lm[i], dtype=dtype) for i, n in enumerate(CHARLM_FIELDS)]
        emb, w_ih1, w_hh1, b_ih1, b_hh1, w_ih2, w_hh2, b_ih2, b_hh2, w_out, b_out = arrs
        H = emb.shape[1]
        if emb.shape[0] != V:
            raise ValueError('ctc_prefix_beam_lm_reference: the language model has %d classes, lp %d' % (emb.shape[0], V))
        one = dtype(1)

        def gru(x, h, w_ih, w_hh, b_ih, b_hh):
            gi, gh = w_ih @ x + b_ih, w_hh @ h + b_hh
            r = one / (one + np.exp(-(gi[:H] + gh[:H])))
            z = one / (one + np.exp(-(gi[H:2 * H] + gh[H:2 * H])))
            n = np.tanh(gi[2 * H:] + r * gh[2 * H:])
            return (one - z) * n + z * h

        def lm_state(w):
            """(h1, h2, the log-softmax row) after <SOS> and the characters of w"""
            if w not in states:
                if w:
                    h1, h2, _ = lm_state(w[:-1])
                    x = emb[w[-1]]
                else:
                    h1 = h2 = np.zeros(H, dtype=dtype)
                    x = emb[0]
                h1 = gru(x, h1, w_ih1, w_hh1, b_ih1, b_hh1)
                h2 = gru(h1, h2, w_ih2, w_hh2, b_ih2, b_hh2)
                y = w_out @ h2 + b_out
                m = y.max()
                row = y - m - np.log(np.exp(y - m).sum(dtype=dtype))
                states[w] = (h1, h2, row.tolist() if f64 else row)
            return states[w]

    def lm_logp(w):
        if w not in L:
            L[w] = lm_logp(w[:-1]) + lm_state(w[:-1])[2][w[-1]]
        return L[w]

    def key_of(w, total):
        if not total > neg:
            return neg
        if use_lm:
            total = total + alpha * lm_logp(w)
        if beta != 0:
            total = total + beta * len(w)
        return total

    beam = {(): (zero, neg)}
    gap = math.inf
    classes = [c for c in range(V) if c != blank]
    with np.errstate(all='ignore'):
        for row in rows:
            either = {u: lae(g[0], g[1]) for u, g in beam.items()}
            new, key = {}, {}
            for w in set(beam) | {u + (c,) for u in beam for c in classes}:
                g_b = row[blank] + either[w] if w in beam else neg
                g_n = neg
                if w:
                    p, c = w[:-1], w[-1]
                    stay = beam[w][1] if w in beam else neg
                    grow = neg
                    if p in beam:
                        grow = beam[p][0] if p and p[-1] == c else either[p]
                    g_n = row[c] + lae(stay, grow)
                new[w] = (g_b, g_n)
                key[w] = key_of(w, lae(g_b, g_n))
            ranked = sorted((w for w in new if key[w] > neg), key=lambda w: (-key[w], w))
            if len(ranked) > K:
                gap = min(gap, float(key[ranked[K - 1]] - key[ranked[K]]))
            beam = {w: new[w] for w in ranked[:K]}
            if trace is not None:
                trace.append(frozenset(beam))
        out = []
        for w, g in beam.items():
            ctc = lae(g[0], g[1])
            total, l = key_of(w, ctc), lm_logp(w) if use_lm else zero
            if use_lm and eos >= 0:
                e = lm_state(w)[2][eos]
                l, total = l + e, total + alpha * e
            out.append((w, float(total), float(ctc), float(l)))
    out.sort(key=lambda e: (-e[1], e[0]))
    for a, b in zip(out, out[1:]):
        gap = min(gap, a[1] - b[1])
    if parts is not None:
        parts.extend((e[2], e[3]) for e in out)
    return [(e[0], e[1]) for e in out], gap


def ctc_prefix_beam_graph_reference(lp, K, graph, graph_weight=0.0, length_bonus=0.0, blank=0, dtype=np.float64,
                                    trace=None, parts=None):
    """BUILD-DEFINED: CTC prefix beam search with a character graph in the ranking, ssasr_ctc_decode_graph
    (include/ssasr.h) restated over Python tuples as texts -- what the kernel is defined and tested against.  lp, K,
    blank, dtype and trace as ctc_prefix_beam_reference takes them (K >= 1); graph: a char_graph.CharGraph (anything
    with next [S][V], arc [S][V], fin [S] and start; None at graph_weight 0), its float32 tables evaluated in `dtype`.
      G(w) = sum_i arc[s_{i-1}][c_i] along s_0 = start, s_i = next[s_{i-1}][c_i]; an arc of -inf forbids the extension.
      Frame t: the candidates and their g_b', g_n' are ctc_prefix_beam_reference's; a candidate's key is
      logaddexp(g_b', g_n') + graph_weight G(w) + length_bonus len(w), a term whose weight is exactly 0 left out (the
      weights are taken as float32 values; graph_weight >= 0); a key of -inf is no candidate; the K candidates with the
      largest keys are the next members.  G(u + (c,)) = G(u) + arc[state(u)][c]: only members are ever extended.
      After the last frame: total = key + graph_weight fin[state(w)].
    -> ([(text, total)] best first, gap): gap is the smallest difference that any frame left between the lowest kept
    and the highest dropped key, or that the final order left between adjacent totals (inf when neither occurred).
    parts: a list that receives (CTC part, graph part G + fin) per returned entry."""
    lp = np.asarray(lp, dtype=dtype)
    K, blank = int(K), int(blank)
    if lp.ndim != 2:
        raise ValueError('ctc_prefix_beam_graph_reference: lp must be [T, V], got %r' % (lp.shape,))
    if K < 1:
        raise ValueError('ctc_prefix_beam_graph_reference: K must be >= 1, got %d' % K)
    V = lp.shape[1]
    f64 = np.dtype(dtype) == np.float64
    gw, beta = float(np.float32(graph_weight)), float(np.float32(length_bonus))
    if not (math.isfinite(gw) and math.isfinite(beta)) or gw < 0:
        raise ValueError('ctc_prefix_beam_graph_reference: graph_weight must be finite and >= 0, length_bonus finite')
    use_g = gw != 0.0
    if f64:                                                     # Python floats ARE float64, and ten times faster
        rows, zero, neg = lp.tolist(), 0.0, -math.inf

        def lae(a, b):
            if a < b:
                a, b = b, a
            return a if b == -math.inf else a + math.log1p(math.exp(b - a))
    else:
        rows, zero, neg, lae = [list(row) for row in lp], dtype(0), dtype(-np.inf), np.logaddexp
        gw, beta = dtype(gw), dtype(beta)
    walked = {}
    if use_g:
        if graph is None:
            raise ValueError('ctc_prefix_beam_graph_reference: graph_weight %g needs a graph' % gw)
        nxt = np.asarray(graph.next)
        arc, fin = np.asarray(graph.arc, dtype=dtype), np.asarray(graph.fin, dtype=dtype)
        if nxt.ndim != 2 or nxt.shape[1] != V or arc.shape != nxt.shape or fin.shape != nxt.shape[:1]:
            raise ValueError('ctc_prefix_beam_graph_reference: the graph has tables %r, %r, %r, lp %d classes'
                             % (nxt.shape, arc.shape, fin.shape, V))
        nxt = nxt.tolist()
        arc, fin = (arc.tolist(), fin.tolist()) if f64 else ([list(r) for r in arc], list(fin))
        walked[()] = (zero, int(graph.start))

    def walk(w):
        """(G(w), state(w))"""
        if w not in walked:
            g, s = walk(w[:-1])
            walked[w] = (g + arc[s][w[-1]], nxt[s][w[-1]])
        return walked[w]

    return _prefix_beam_ranked(rows, K, blank, V, lae, zero, neg, gw, beta, walk if use_g else None,
                               lambda s: fin[s], trace, parts)


def _prefix_beam_ranked(rows, K, blank, V, lae, zero, neg, gw, beta, walk, fin_of, trace, parts):
    """The search of ctc_prefix_beam_graph_reference and ctc_prefix_beam_word_reference over the frames `rows`:
    walk(w) -> (G(w), state(w)) (None: no graph term) and fin_of(state) are the graph's; lae, zero and neg carry the
    dtype.  -> ([(text, total)] best first, gap); parts as those two take it."""
    use_g = walk is not None

    def key_of(w, total):
        if not total > neg:
            return neg
        if use_g:
            total = total + gw * walk(w)[0]
        if beta != 0:
            total = total + beta * len(w)
        return total

    beam = {(): (zero, neg)}
    gap = math.inf
    classes = [c for c in range(V) if c != blank]
    with np.errstate(all='ignore'):
        for row in rows:
            either = {u: lae(g[0], g[1]) for u, g in beam.items()}
            new, key = {}, {}
            for w in set(beam) | {u + (c,) for u in beam for c in classes}:
                g_b = row[blank] + either[w] if w in beam else neg
                g_n = neg
                if w:
                    p, c = w[:-1], w[-1]
                    stay = beam[w][1] if w in beam else neg
                    grow = neg
                    if p in beam:
                        grow = beam[p][0] if p and p[-1] == c else either[p]
                    g_n = row[c] + lae(stay, grow)
                new[w] = (g_b, g_n)
                key[w] = key_of(w, lae(g_b, g_n))
            ranked = sorted((w for w in new if key[w] > neg), key=lambda w: (-key[w], w))
            if len(ranked) > K:
                gap = min(gap, float(key[ranked[K - 1]] - key[ranked[K]]))
            beam = {w: new[w] for w in ranked[:K]}
            if trace is not None:
                trace.append(frozenset(beam))
        out = []
        for w, g in beam.items():
            ctc = lae(g[0], g[1])
            total, part = key_of(w, ctc), zero
            if use_g:
                part, s = walk(w)
                part, total = part + fin_of(s), total + gw * fin_of(s)
            out.append((w, float(total), float(ctc), float(part)))
    out.sort(key=lambda e: (-e[1], e[0]))
    for a, b in zip(out, out[1:]):
        gap = min(gap, a[1] - b[1])
    if parts is not None:
        parts.extend((e[2], e[3]) for e in out)
    return [(e[0], e[1]) for e in out], gap


def ctc_prefix_beam_word_reference(lp, K, graph, graph_weight=0.0, length_bonus=0.0, blank=0, dtype=np.float64,
                                   trace=None, parts=None):
    """BUILD-DEFINED: CTC prefix beam search over a lexicon with a word n-gram LM in the ranking, ssasr_ctc_decode_word
    (include/ssasr.h) restated over Python tuples as texts -- what the kernel is defined and tested against.  Every
    argument, the search, the keys, the ties, the end ranking, gap and parts are ctc_prefix_beam_graph_reference's;
    graph: a word_graph.WordGraph (None at graph_weight 0), whose float32 tables are evaluated in `dtype`:
      a text's state is (n, h), the empty text's (0, 0); class c != space: arc carc[n][c], state (child[n][c], h);
      the space where word[n] < 0: -inf; else, with (lp, h') = lookup(h, word[n]) summed in float64, the arc is
      float32(pen[n] + lp) and the state (0, h');
      G(w) = the sum of the arcs; fin(n, h) = pen[n] + eos[h] where word[n] < 0, else (the space arc) + eos[h']."""
    lp = np.asarray(lp, dtype=dtype)
    K, blank = int(K), int(blank)
    if lp.ndim != 2:
        raise ValueError('ctc_prefix_beam_word_reference: lp must be [T, V], got %r' % (lp.shape,))
    if K < 1:
        raise ValueError('ctc_prefix_beam_word_reference: K must be >= 1, got %d' % K)
    V = lp.shape[1]
    gw, beta = float(np.float32(graph_weight)), float(np.float32(length_bonus))
    if not (math.isfinite(gw) and math.isfinite(beta)) or gw < 0:
        raise ValueError('ctc_prefix_beam_word_reference: graph_weight must be finite and >= 0, length_bonus finite')
    if np.dtype(dtype) == np.float64:                           # Python floats ARE float64, and ten times faster
        rows, zero, neg, cast = lp.tolist(), 0.0, -math.inf, float

        def lae(a, b):
            if a < b:
                a, b = b, a
            return a if b == -math.inf else a + math.log1p(math.exp(b - a))
    else:
        rows, zero, neg, lae, cast = [list(row) for row in lp], dtype(0), dtype(-np.inf), np.logaddexp, dtype
        gw, beta = dtype(gw), dtype(beta)
    walk = None
    if gw != 0:
        if graph is None:
            raise ValueError('ctc_prefix_beam_word_reference: graph_weight %g needs a graph' % gw)
        if graph.n_classes != V or graph.space == blank:
            raise ValueError('ctc_prefix_beam_word_reference: the graph has %d classes and the space %d, lp %d classes '
                             'and the blank %d' % (graph.n_classes, graph.space, V, blank))
        walked = {(): (zero, (0, 0))}

        def walk(w):
            """(G(w), (n, h))"""
            if w not in walked:
                g, state = walk(w[:-1])
                arc, state = graph.step(*state, w[-1])
                walked[w] = (g + cast(arc), state)
            return walked[w]

    return _prefix_beam_ranked(rows, K, blank, V, lae, zero, neg, gw, beta, walk,
                               lambda state: cast(graph.fin(*state)), trace, parts)


def _segment_frame(dp, lp_t, lab, pen, neg, zero):
    """One frame of ctc_segment_reference's lattice.  dp [S + 2]: the values of the frame before behind two -inf
    pads; pen [S]: 0 where the skip is allowed, -inf elsewhere.  -> (the new padded values, the back-pointer codes
    0 stay / 1 s - 1 / 2 s - 2 / 3 start)."""
    d, one, two = dp[2:], dp[1:-1], dp[:-2] + pen
    m1 = one > d                                                # stay wins a tie, then s - 1, then s - 2, then the start
    best = np.where(m1, one, d)
    m2 = two > best
    best = np.where(m2, two, best)
    code = m1.astype(np.int8)
    code[m2] = 2
    for s in range(min(d.shape[0], 2)):
        if zero > best[s]:
            best[s], code[s] = zero, 3
    out = np.empty_like(dp)
    out[:2] = neg
    np.add(best, lp_t[lab], out=out[2:])
    return out, code


def _segment_margin(dp, s, pen, neg, zero):
    """The margin of state s's decision on the padded values dp of the frame before: the winner minus the best
    loser."""
    cand = sorted(float(c) for c in (dp[s + 2], dp[s + 1], dp[s] + pen[s], zero if s < 2 else neg))
    return math.inf if cand[-2] == -math.inf else cand[-1] - cand[-2]


def ctc_segment_reference(lp, y, utt_ends, window, blank=0, dtype=np.float64):
    """BUILD-DEFINED: CTC segmentation, ssasr_ctc_segment (include/ssasr.h) restated in numpy -- what the kernel is
    defined and tested against.  lp [T, V]: one recording's NORMALISED log-probabilities, already cut to its frames;
    y: the whole text's labels; utt_ends: each utterance's exclusive end in y; every sum runs in `dtype` (float64;
    float32 measures the arithmetic's noise).  The same operations in the same order as the header states them,
    vectorised over the states of a frame:
      d[t][s] = best(d[t-1][s], d[t-1][s-1], d[t-1][s-2] if the skip is allowed, 0 if s < 2) + lp[t][lab_s]
    the larger value wins, among equals stay, then s - 1, then s - 2, then the start; the end is the largest d[t][s]
    over every frame and s in {S - 1, S - 2}, among equals the earliest frame, then S - 1.
    -> None when nothing can be segmented (no frame, no label, malformed utt_ends, no finite end), else a namespace of
    score, path [T] (-1 outside the span), first / last / char_logp [L], utt_first / utt_last / utt_conf [N] and gap:
    the smallest difference between the winner and the best loser over the decisions ON the returned path (each
    frame's choice among stay / s - 1 / s - 2 / start) and the end choice -- below it a rounding can change the path.
    The lattice is run twice, the second time to read the margins along the path, so that no [T, S] table of values
    is kept."""
    import types
    lp = np.asarray(lp).astype(dtype)
    if lp.ndim != 2:
        raise ValueError('ctc_segment_reference: lp must be [T, V], got %r' % (lp.shape,))
    window, blank = int(window), int(blank)
    if window < 1:
        raise ValueError('ctc_segment_reference: window must be >= 1, got %d' % window)
    y, ends = [int(c) for c in y], [int(e) for e in utt_ends]
    T, L = lp.shape[0], len(y)
    if T < 1 or L < 1 or not ends or ends[-1] != L or any(b <= a for a, b in zip([0] + ends, ends)):
        return None
    neg, zero = dtype(-np.inf), dtype(0)
    S = 2 * L + 1
    lab = np.full(S, blank, dtype=np.int64)
    lab[1::2] = y
    skip = np.zeros(S, dtype=bool)
    skip[3::2] = lab[3::2] != lab[1:-2:2]
    pen = np.where(skip, zero, neg).astype(dtype)
    back = np.zeros((T, S), dtype=np.int8)
    dp = np.full(S + 2, neg, dtype=dtype)
    ends_seen = []                                              # (value, frame, state) of every end candidate
    best_end = None
    for t in range(T):
        dp, back[t] = _segment_frame(dp, lp[t], lab, pen, neg, zero)
        for s in (S - 1, S - 2):
            v = dp[s + 2]
            ends_seen.append(v)
            if v > neg and (best_end is None or v > best_end[0]):         # strict: the earliest frame, then S - 1
                best_end = (v, t, s)
    if best_end is None:
        return None
    score, t_end, s = best_end
    top = np.sort(np.asarray(ends_seen, dtype=dtype))
    gap = float(top[-1] - top[-2]) if top[-2] > neg else math.inf
    path = np.full(T, -1, dtype=np.int64)
    t = t_end
    while True:
        path[t] = s
        code = int(back[t, s])
        if code == 3:
            break
        s -= code
        t -= 1
    t_start = t
    del back
    dp = np.full(S + 2, neg, dtype=dtype)
    for t in range(t_end + 1):                                  # again, for the margins along the path
        if t >= t_start:
            gap = min(gap, _segment_margin(dp, int(path[t]), pen, neg, zero))
        dp, _ = _segment_frame(dp, lp[t], lab, pen, neg, zero)
    q = np.zeros(T, dtype=dtype)
    span = np.arange(t_start, t_end + 1)
    q[span] = lp[span, lab[path[span]]]

    def total(lo, hi):                                          # q[lo .. hi] summed in frame order
        return np.cumsum(q[lo:hi + 1], dtype=dtype)[-1]
    first, last = np.zeros(L, dtype=np.int64), np.zeros(L, dtype=np.int64)
    logp = np.zeros(L, dtype=dtype)
    for j in range(L):
        frames = np.nonzero(path == 2 * j + 1)[0]
        first[j], last[j] = frames[0], frames[-1]
        logp[j] = total(first[j], last[j])
    N = len(ends)
    utt_first = np.array([first[a] for a in [0] + ends[:-1]], dtype=np.int64)
    utt_last = np.array([last[e - 1] for e in ends], dtype=np.int64)
    conf = np.zeros(N, dtype=dtype)
    for n in range(N):
        means = [total(lo, min(lo + window - 1, utt_last[n])) / dtype(min(lo + window - 1, utt_last[n]) - lo + 1)
                 for lo in range(utt_first[n], utt_last[n] + 1, window)]
        conf[n] = min(means)
    return types.SimpleNamespace(score=float(score), path=path, first=first, last=last, char_logp=logp,
                                 utt_first=utt_first, utt_last=utt_last, utt_conf=conf, gap=gap, span=(t_start, t_end))


def _segment_skip_frame(dp, lp_t, lab, pen, junc, skip_pen, fill_pen, blank, others, neg, zero):
    """One frame of ctc_segment_skip_reference's lattice: _segment_frame with the junctions' emission and skip.
    junc: the junction states J_0 .. J_N; others: the classes that are not the blank.
    -> (the new padded values, the codes, whether the filler won this frame's junction emission, its margin, the
    states' emissions)."""
    dtype = dp.dtype.type
    d, one, two = dp[2:], dp[1:-1], dp[:-2] + pen
    two[junc[1:]] = dp[junc[:-1] + 2] + skip_pen                # a blank has no s - 2: the skip takes its place
    m1 = one > d                                                # stay, then s - 1, then s - 2 / the skip, then the start
    best = np.where(m1, one, d)
    m2 = two > best
    best = np.where(m2, two, best)
    code = m1.astype(np.int8)
    code[m2] = 2
    for s in range(min(d.shape[0], 2)):
        if zero > best[s]:
            best[s], code[s] = zero, 3
    x = lp_t[others]
    m = x.max()
    fv = dtype(m + np.log(np.exp(x - m).sum(dtype=dtype))) + fill_pen
    lpb = lp_t[blank]
    fill = bool(fv > lpb)                                       # the blank wins a tie
    emit = lp_t[lab]
    emit[junc] = fv if fill else lpb
    out = np.empty_like(dp)
    out[:2] = neg
    np.add(best, emit, out=out[2:])
    return out, code, fill, (math.inf if fv == neg else abs(float(fv) - float(lpb))), emit


def ctc_segment_skip_reference(lp, y, utt_ends, window, skip_penalty=-math.inf, fill_penalty=-math.inf, blank=0,
                               dtype=np.float64):
    """BUILD-DEFINED: CTC segmentation with utterance skips and a filler, ssasr_ctc_segment_skip (include/ssasr.h)
    restated in numpy -- what the kernel is defined and tested against.  Arguments as ctc_segment_reference takes
    them; skip_penalty, fill_penalty: finite and <= 0, or -inf (that mechanism off; with both off every output is
    ctc_segment_reference's).  The junction J_n is the blank state 2 * utt_ends[n - 1] (J_0 = 0, J_N = S - 1).
      f_t = log sum_{v != blank} exp(lp[t][v]); a junction state's emission is max(lp[t][blank], f_t + fill_penalty),
      the blank winning a tie; J_{n+1} has one more predecessor, d[t-1][J_n] + skip_penalty, which takes the place of
      s - 2 in the tie rule (stay, s - 1, skip, start).
    -> None when nothing can be segmented, else ctc_segment_reference's namespace with utt_skipped [N] (1 / 0) and
    is_fill [T] (1 on a junction frame of the path where the filler won, 0 on the other scored frames, -1 outside
    the span); a skipped utterance has utt_first = utt_last = -1, utt_conf = 0, its characters first = last = -1 and
    char_logp = 0.  gap also covers the filler-versus-blank choice on every junction frame of the path."""
    import types
    lp = np.asarray(lp).astype(dtype)
    if lp.ndim != 2:
        raise ValueError('ctc_segment_skip_reference: lp must be [T, V], got %r' % (lp.shape,))
    window, blank = int(window), int(blank)
    if window < 1:
        raise ValueError('ctc_segment_skip_reference: window must be >= 1, got %d' % window)
    for name, p in (('skip_penalty', skip_penalty), ('fill_penalty', fill_penalty)):
        if not p <= 0:                                          # a NaN too
            raise ValueError('ctc_segment_skip_reference: %s must be <= 0 or -inf, got %r' % (name, p))
    y, ends = [int(c) for c in y], [int(e) for e in utt_ends]
    T, L = lp.shape[0], len(y)
    if T < 1 or L < 1 or not ends or ends[-1] != L or any(b <= a for a, b in zip([0] + ends, ends)):
        return None
    neg, zero = dtype(-np.inf), dtype(0)
    skip_pen, fill_pen = dtype(skip_penalty), dtype(fill_penalty)
    S, N = 2 * L + 1, len(ends)
    lab = np.full(S, blank, dtype=np.int64)
    lab[1::2] = y
    skip = np.zeros(S, dtype=bool)
    skip[3::2] = lab[3::2] != lab[1:-2:2]
    pen = np.where(skip, zero, neg).astype(dtype)
    junc = np.array([0] + [2 * e for e in ends], dtype=np.int64)
    is_junc = np.zeros(S, dtype=bool)
    is_junc[junc] = True
    others = np.array([v for v in range(lp.shape[1]) if v != blank], dtype=np.int64)
    frame = lambda dp, t: _segment_skip_frame(dp, lp[t], lab, pen, junc, skip_pen, fill_pen, blank, others, neg, zero)
    back = np.zeros((T, S), dtype=np.int8)
    dp = np.full(S + 2, neg, dtype=dtype)
    ends_seen = []
    best_end = None
    with np.errstate(invalid='ignore'):
        for t in range(T):
            dp, back[t] = frame(dp, t)[:2]
            for s in (S - 1, S - 2):
                v = dp[s + 2]
                ends_seen.append(v)
                if v > neg and (best_end is None or v > best_end[0]):
                    best_end = (v, t, s)
        if best_end is None:
            return None
        score, t_end, s = best_end
        top = np.sort(np.asarray(ends_seen, dtype=dtype))
        gap = float(top[-1] - top[-2]) if top[-2] > neg else math.inf
        path = np.full(T, -1, dtype=np.int64)
        t = t_end
        while True:
            path[t] = s
            code = int(back[t, s])
            if code == 3:
                break
            if code == 2 and is_junc[s]:
                s = int(junc[int(np.searchsorted(junc, s)) - 1])
            else:
                s -= code
            t -= 1
        t_start = t
        del back
        q = np.zeros(T, dtype=dtype)
        is_fill = np.full(T, -1, dtype=np.int64)
        dp = np.full(S + 2, neg, dtype=dtype)
        for t in range(t_end + 1):                              # again, for the margins along the path
            s = int(path[t])
            if t >= t_start:
                cand = [dp[s + 2], dp[s + 1], dp[s] + pen[s], zero if s < 2 else neg]
                if is_junc[s] and s:
                    cand[2] = dp[junc[int(np.searchsorted(junc, s)) - 1] + 2] + skip_pen
                cand = sorted(float(c) for c in cand)
                gap = min(gap, math.inf if cand[-2] == -math.inf else cand[-1] - cand[-2])
            dp, _, fill, margin, emit = frame(dp, t)
            if t >= t_start:
                is_fill[t] = int(fill and is_junc[s])
                if is_junc[s]:
                    gap = min(gap, margin)
                q[t] = emit[s]

    def total(lo, hi):
        return np.cumsum(q[lo:hi + 1], dtype=dtype)[-1]
    first, last = np.full(L, -1, dtype=np.int64), np.full(L, -1, dtype=np.int64)
    logp = np.zeros(L, dtype=dtype)
    for j in range(L):
        frames = np.nonzero(path == 2 * j + 1)[0]
        if len(frames):
            first[j], last[j] = frames[0], frames[-1]
            logp[j] = total(first[j], last[j])
    utt_first = np.array([first[a] for a in [0] + ends[:-1]], dtype=np.int64)
    utt_last = np.array([last[e - 1] for e in ends], dtype=np.int64)
    utt_skipped = (utt_first < 0).astype(np.int64)
    conf = np.zeros(N, dtype=dtype)
    for n in range(N):
        if utt_skipped[n]:
            utt_last[n] = -1
            continue
        means = [total(lo, min(lo + window - 1, utt_last[n])) / dtype(min(lo + window - 1, utt_last[n]) - lo + 1)
                 for lo in range(utt_first[n], utt_last[n] + 1, window)]
        conf[n] = min(means)
    return types.SimpleNamespace(score=float(score), path=path, first=first, last=last, char_logp=logp,
                                 utt_first=utt_first, utt_last=utt_last, utt_conf=conf, gap=gap, span=(t_start, t_end),
                                 utt_skipped=utt_skipped, is_fill=is_fill)


class ErrorStats:
    """Corpus-level error rates: sums (S, D, I, N) rows of characters and of words; cer / wer =
    sum(S + D + I) / sum(N), nan when N == 0.  (calc_err below stays the reference's mean of per-utterance ratios.)"""

    def __init__(self):
        self.chars = [0, 0, 0, 0]
        self.words = [0, 0, 0, 0]

    def add(self, chars, words):
        """chars, words: (S, D, I, N) of one utterance."""
        for total, row in ((self.chars, chars), (self.words, words)):
            for k in range(4):
                total[k] += int(row[k])
        return self

    @staticmethod
    def rate(counts):
        s, d, i, n = counts
        return (s + d + i) / n if n else float('nan')

    @property
    def cer(self):
        return self.rate(self.chars)

    @property
    def wer(self):
        return self.rate(self.words)


def calc_acc(predict, label):
    """src/postprocess.py:7-29: mean over utterances of the fraction of label
    positions (up to the first pad) predicted correctly."""
    predict = np.argmax(predict.detach().cpu().numpy(), axis=-1)
    label = label.cpu().numpy()
    accs = []
    for p, l in zip(predict, label):
        correct, total = 0.0, 0
        for pp, ll in zip(p, l):
            if ll == 0:
                break
            correct += int(pp == ll)
            total += 1
        accs.append(correct / total)
    return sum(accs) / len(accs)


def calc_err(predict, label, mapper):
    """src/postprocess.py:31-49: word-level edit distance over label words."""
    label = label.cpu()
    predict = np.argmax(predict.detach().cpu().numpy(), axis=-1)
    hyp = [mapper.translate(p) for p in predict]
    ref = [mapper.translate(l) for l in label]
    ds = [float(edit_distance(p.split(' '), l.split(' '))) / len(l.split(' '))
          for p, l in zip(hyp, ref)]
    return sum(ds) / len(ds)


def draw_att(att_maps, hyps):
    """src/postprocess.py:51-62: [3, len, T'] image per utterance."""
    out = []
    for i in range(att_maps.shape[0]):
        att_i = att_maps[i, :, :]
        n = len(trim_eos(hyps[i]))
        out.append(torch.stack([att_i, att_i, att_i], dim=0)[:, :n, :])
    return out
