"""Host-side metrics of the reference (src/postprocess.py): character
accuracy, word-level edit-distance error, attention images, EOS trimming.
The reference uses the `editdistance` package; a small Levenshtein routine
replaces it here."""
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
