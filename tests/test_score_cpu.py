"""Edit-distance scoring without a GPU: postprocess.edit_ops (the tuple DP that ssasr_edit_score restates on the
device, and the checker of tests/test_gpu_score.py) against a brute force over every monotone alignment, the word
split against str.split(), ErrorStats' arithmetic, and the entry point's argument errors."""
import itertools
import math

import pytest

from ss_asr_amd.ASRDataset import Mapper
from ss_asr_amd.postprocess import ErrorStats, edit_counts, edit_distance, edit_ops, score_sequences

SPACE = Mapper().char_to_ind(' ')


def brute_force(hyp, ref):
    """The set of (S, D, I) over ALL monotone alignments of hyp against ref: at each point a pair is matched
    (substitution when the symbols differ), a reference symbol is deleted or a hypothesis symbol is inserted."""
    seen = {}

    def walk(i, j):
        if (i, j) in seen:
            return seen[i, j]
        if i == len(hyp) and j == len(ref):
            out = {(0, 0, 0)}
        else:
            out = set()
            if i < len(hyp) and j < len(ref):
                ne = int(hyp[i] != ref[j])
                out |= {(s + ne, d, n) for s, d, n in walk(i + 1, j + 1)}
            if j < len(ref):
                out |= {(s, d + 1, n) for s, d, n in walk(i, j + 1)}
            if i < len(hyp):
                out |= {(s, d, n + 1) for s, d, n in walk(i + 1, j)}
        seen[i, j] = out
        return out

    return walk(0, 0)


SEQUENCES = [seq for n in range(5) for seq in itertools.product('abc', repeat=n)]


def test_edit_ops_is_the_lexicographic_minimum_over_every_alignment():
    assert len(SEQUENCES) == 121
    for hyp in SEQUENCES:
        for ref in SEQUENCES:
            s, d, i = edit_ops(hyp, ref)
            assert min(s, d, i) >= 0
            assert s + d + i == edit_distance(hyp, ref)
            assert i - d == len(hyp) - len(ref)
            best = min((a + b + c, a) for a, b, c in brute_force(hyp, ref))
            assert (s + d + i, s) == best, (hyp, ref)
            assert (s, d, i) in brute_force(hyp, ref)


def test_ab_against_ba_is_one_deletion_and_one_insertion():
    assert edit_ops('ba', 'ab') == (0, 1, 1)            # reference ab, hypothesis ba: not S = 2
    assert edit_ops('', '') == (0, 0, 0)
    assert edit_ops('abc', '') == (0, 0, 3) and edit_ops('', 'abc') == (0, 3, 0)
    assert edit_ops('kitten', 'sitting') == (2, 1, 0)


@pytest.mark.parametrize('text', ['', ' ', '    ', 'a', ' a', 'a ', '  ab  c ', 'ab  ab', 'a b c', ' $ a$ ', 'halló  þú .'])
def test_words_are_str_split(text):
    m = Mapper()
    ids = [0] + [m.char_to_ind(c) for c in text] + [1, 0, 0]                 # <sos>, <eos> and pads are dropped
    chars, words = score_sequences(ids, SPACE)
    assert ''.join(m.ind_to_char(c) for c in chars) == text
    assert [''.join(m.ind_to_char(c) for c in w) for w in words] == text.split()
    # pads in the middle of a row change nothing
    holes = [v for c in ids for v in (c, 0)]
    assert score_sequences(holes, SPACE) == (chars, words)


def test_edit_counts_rows():
    m = Mapper()
    enc = lambda s: [m.char_to_ind(c) for c in s]
    assert edit_counts(enc('<the cat sat>'), enc('<the cat sat>'), SPACE) == [0, 0, 0, 11, 0, 0, 0, 3]
    assert edit_counts(enc('the bat  sat on'), enc('the cat sat'), SPACE) == [1, 0, 4, 11, 1, 0, 1, 3]
    assert edit_counts(enc('<>'), enc('  '), SPACE) == [0, 2, 0, 2, 0, 0, 0, 0]
    assert edit_counts(enc('$'), enc(''), SPACE) == [0, 0, 1, 0, 0, 0, 1, 0]     # `$` (id 2) is a character


def test_error_stats_arithmetic():
    st = ErrorStats()
    assert math.isnan(st.cer) and math.isnan(st.wer)
    st.add((1, 2, 3, 10), (1, 0, 0, 2)).add((0, 0, 1, 5), (0, 0, 0, 0))
    assert st.chars == [1, 2, 4, 15] and st.words == [1, 0, 0, 2]
    assert st.cer == 7 / 15 and st.wer == 0.5
    st = ErrorStats().add((0, 0, 2, 0), (0, 0, 1, 0))       # errors against nothing: no rate
    assert math.isnan(st.cer) and math.isnan(st.wer)
    # corpus-level, not a mean of ratios: (1 + 3) / (2 + 10), not (1 / 2 + 3 / 10) / 2
    assert ErrorStats().add((1, 0, 0, 2), (0, 0, 0, 1)).add((3, 0, 0, 10), (0, 0, 0, 1)).cer == 4 / 12


def test_edit_score_argument_errors_are_negative_and_need_no_gpu():
    import ctypes
    from ss_asr_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(hyp=p, hyp_ld=8, hyp_lens=p, ref=p, ref_ld=8, ref_lens=p, ref_of=None, P=1, Hmax=8, Rmax=8, out=p):
        return lib.ssasr_edit_score(hyp, hyp_ld, hyp_lens, ref, ref_ld, ref_lens, ref_of, P, Hmax, Rmax, 2, SPACE, out,
                                    None)

    for name in ('hyp', 'hyp_lens', 'ref', 'ref_lens', 'out'):
        assert call(**{name: None}) < 0, name
    assert call(P=-1) < 0
    assert call(Rmax=1024, ref_ld=1024) < 0 and call(Hmax=8192, hyp_ld=8192) < 0
    assert call(Rmax=-1) < 0 and call(Hmax=-1) < 0
    assert call(hyp_ld=7) < 0 and call(ref_ld=7) < 0            # a leading dimension below the maximum length
    assert call(P=0) == 0                                       # legal, launches nothing
    assert call(P=0, hyp=None, ref=None, hyp_lens=None, ref_lens=None, out=None) == 0
