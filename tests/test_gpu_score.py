"""Edit-distance scoring on the GPU (ssasr_edit_score through ops.edit_score; ASR.score; ASRTester with
asr.decode_score) against postprocess.edit_counts, the host restatement that tests/test_score_cpu.py pins by brute
force.  The metric is the lexicographic minimum of (S + D + I, S), so the counts are unique: every comparison is
equality, with no tolerance and no excluded case.  The shapes are the smallest at which each mechanism can fail: the
wave boundary and the exchange slot (64 / 65 / 128 / 129 columns), hypotheses longer than a block, the limits
(1,023 reference ids, 8,191 hypothesis ids), rows that are empty before or only after dropping, small alphabets
(most pairs have several minimal alignments), padded layouts with a poison id in the slack."""
import os
import shutil
import types

import numpy as np
import pytest
import torch

import test_gpu_beam as tgb
import test_gpu_decode as tgd
from conftest import GOLDEN
from test_host_cpu import make_corpus

from ss_asr_amd.postprocess import ErrorStats, edit_counts

pytestmark = pytest.mark.gpu

DEV = tgd.DEV
Mapper = tgd.Mapper
SPACE = Mapper().char_to_ind(' ')
POISON = 7                      # a kept character: a kernel that reads slack or past a row's length counts it


def run(pairs, pad=3, ref_of=None, refs=None, min_cols=(0, 0)):
    """ops.edit_score over pairs [(hyp ids, ref ids)] (or hyps against refs through ref_of), the rows laid out in
    matrices `pad` columns wider than the longest row and filled with POISON.  -> [P][8] as lists."""
    from ss_asr_amd import ops
    hyps = [h for h, _ in pairs]
    if refs is None:
        refs = [r for _, r in pairs]

    def matrix(rows, least):
        width = max([len(r) for r in rows] + [least])
        m = np.full((len(rows), width + pad), POISON, dtype=np.int32)
        for i, r in enumerate(rows):
            m[i, :len(r)] = r
        t = torch.from_numpy(m).to(DEV)
        return t[:, :width], torch.tensor([len(r) for r in rows], dtype=torch.int32, device=DEV)

    hyp, hyp_lens = matrix(hyps, min_cols[0])
    ref, ref_lens = matrix(refs, min_cols[1])
    if ref_of is not None:
        ref_of = torch.tensor(ref_of, dtype=torch.int32, device=DEV)
    out = ops.edit_score(hyp, hyp_lens, ref, ref_lens, ref_of, space=SPACE)
    assert out.shape == (len(hyps), 8) and out.dtype == torch.int32 and out.is_cuda
    return out.cpu().tolist()


def host(pairs):
    return [edit_counts(h, r, SPACE) for h, r in pairs]


def draw(rng, n, alphabet):
    return [int(v) for v in rng.choice(alphabet, size=n)]


_long = {}


def long_pair():
    """R = H = 1023 over {a, b, space} and its host counts, computed once."""
    if not _long:
        rng = np.random.default_rng(3)
        _long['pair'] = (draw(rng, 1023, [3, 4, 4, SPACE]), draw(rng, 1023, [3, 4, 4, SPACE]))
        _long['want'] = edit_counts(*_long['pair'], SPACE)
    return _long['pair'], _long['want']


def test_edge_lengths_across_wave_boundaries():
    rng = np.random.default_rng(0)
    alphabet = [3, 4, 5, SPACE]
    pairs = [(draw(rng, H, alphabet), draw(rng, cols - 1, alphabet))
             for cols in (1, 2, 63, 64, 65, 128, 129) for H in (0, 1, 64, 65, 200)]
    # empty before dropping, empty only after dropping (pads, <sos>, <eos>), on either side and on both
    dropped = [0, 1, 0, 0, 1]
    pairs += [([], []), (dropped, []), ([], dropped), (dropped, dropped), (dropped, [3, SPACE, 4]), ([3, 4], dropped),
              ([SPACE], []), ([], [SPACE, SPACE])]
    assert run(pairs) == host(pairs)


def test_the_limits_and_a_batch_that_mixes_one_column_with_1024():
    (hyp, ref), want = long_pair()
    pairs = [([3, 4, SPACE, 3], []), (hyp, ref), ([], []), ([], [4]), ([4, 4], [4])]
    assert run(pairs) == [edit_counts(h, r, SPACE) if (h, r) != (hyp, ref) else want for h, r in pairs]
    rng = np.random.default_rng(4)
    pairs = [(draw(rng, 8191, [3, 4, 5, SPACE, SPACE]), [3, SPACE, 4, 4, 3])]
    assert run(pairs, pad=0) == host(pairs)


def test_ties_on_small_alphabets():
    rng = np.random.default_rng(1)
    pairs = []
    for n in range(512):
        alphabet = [3, 4, SPACE] if n % 2 else [3, 4, 5, SPACE]
        pairs.append((draw(rng, int(rng.integers(0, 41)), alphabet), draw(rng, int(rng.integers(0, 41)), alphabet)))
    got, want = run(pairs), host(pairs)
    assert got == want
    assert sum(g[0] + g[1] + g[2] > 0 for g in got) > 400          # the pairs do differ
    assert run([([4, 3], [3, 4])])[0][:4] == [0, 1, 1, 2]          # reference ab, hypothesis ba


def test_words():
    m = Mapper()
    enc = lambda s: [m.char_to_ind(c) for c in s]
    pairs = [(enc('abcd abce abc'), enc('abce abcd abcd')),         # a shared prefix, the last token differs
             (enc('aa aaa a aaaa'), enc('a aa aaa aaaa')),          # equal tokens, different word lengths
             (enc('the the cat the'), enc('the cat the the')),      # a repeated word on both sides
             (enc('    '), enc(' ')), (enc('   '), enc('a')), (enc('a b'), enc('  ')),      # only spaces
             (enc('  ab  cd '), enc('ab cd')), (enc('ab cd'), enc(' ab   cd  ')),
             (enc('$ a$ $'), enc('$ a $')),                         # `$` (id 2) is kept as a character
             ([0, 3, 0, 0, SPACE, 1, 4, 0], [3, 0, SPACE, 0, 0, 4, 1, 0, 0]),           # pads in the middle of a row
             ([0, 3, 0, 4, 1], enc('a b'))]
    got = run(pairs)
    assert got == host(pairs)
    assert got[2][4:] == [0, 1, 1, 4] and got[3] == [0, 0, 3, 1, 0, 0, 0, 0] and got[9] == [0] * 3 + [3] + [0] * 3 + [2]
    assert got[8][:4] == [0, 0, 1, 5] and got[8][4:] == [1, 0, 0, 3]


def test_layout():
    from ss_asr_amd import ops
    rng = np.random.default_rng(2)
    alphabet = [3, 4, 5, SPACE]
    refs = [draw(rng, 30, alphabet), draw(rng, 70, alphabet)]
    hyps = [draw(rng, int(rng.integers(0, 90)), alphabet) for _ in range(32)]
    ref_of = [0] * 16 + [1] * 16
    pairs = [(h, refs[r]) for h, r in zip(hyps, ref_of)]
    want = host(pairs)
    shared = run(pairs, pad=5, ref_of=ref_of, refs=refs)
    assert shared == want and run(pairs, pad=5) == want and run(pairs, pad=0) == want
    # wider matrices than any row needs: Hmax / Rmax beyond the longest row, the slack poisoned
    assert run(pairs, pad=2, min_cols=(130, 100)) == want
    # no pairs: nothing is launched
    empty = torch.empty(0, 4, dtype=torch.int32, device=DEV)
    lens = torch.empty(0, dtype=torch.int32, device=DEV)
    assert ops.edit_score(empty, lens, empty, lens, space=SPACE).shape == (0, 8)
    # what the wrapper refuses
    one = torch.zeros(1, 4, dtype=torch.int32, device=DEV)
    n1 = torch.ones(1, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        ops.edit_score(one, n1, one, n1, torch.tensor([1], dtype=torch.int32, device=DEV), space=SPACE)
    with pytest.raises(ValueError):
        ops.edit_score(torch.zeros(1, 8192, dtype=torch.int32, device=DEV), n1, one, n1, space=SPACE)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.edit_score(one.cpu(), n1, one, n1, space=SPACE)


def host_scores(nbest, refs):
    """ASR.score's result from the returned strings: [(texts of one utterance, best first)] against reference ids."""
    from ss_asr_amd.asr import Score
    m = Mapper()
    out = []
    for texts, ref in zip(nbest, refs):
        rows = [edit_counts([m.char_to_ind(c) for c in t], ref, SPACE) for t in texts]
        k = min(range(len(rows)), key=lambda k: (sum(rows[k][4:7]), sum(rows[k][:3]), k))
        out.append(Score(tuple(rows[0][:4]), tuple(rows[0][4:]), (k, tuple(rows[k][:4]), tuple(rows[k][4:]))))
    return out


def test_model_level_scores_are_the_host_scores_of_the_returned_strings(golden):
    from ss_asr_amd.asr import ASR
    fx = golden(tgb.SMALL[0])
    asr, lm = tgd.models(fx)
    m = Mapper()
    x = torch.from_numpy(fx['x']).to(DEV)
    xs, lens = [x[:, :40], x[:, :24]], [[40], [24]]
    greedy = asr.decode_many(xs, lens, lm, m, 0.3, max_decoding_steps=tgb.STEPS)
    refs = ['<' + greedy[0][:5] + ' ' + greedy[0][7:] + '>', 'no hay $']
    ref_ids = [[m.char_to_ind(c) for c in r] for r in refs]
    want = host_scores([[t] for t in greedy], ref_ids)
    got = asr.score(refs, m)
    assert got == want and all(s.oracle == (0, s.chars, s.words) for s in got)
    assert got[0].chars[3] == sum(c >= 2 for c in ref_ids[0]) and sum(got[0].chars[:3]) > 0
    # label rows as the loader gives them: <sos> first, <eos> and pads behind
    rows = [torch.tensor([0] + ids + [1, 0, 0]) for ids in ref_ids]
    assert asr.score(rows, m) == want and asr.score([r.tolist() for r in rows], m) == want
    with pytest.raises(ValueError):
        asr.score(refs[:1], m)
    with pytest.raises(ValueError):
        ASR(*[int(v) for v in fx['dims']], 1.0).score(refs, m)
    # an n-best list: the best entry's counts and the oracle entry under the tie rule
    nbest = asr.decode_nbest(xs, lens, lm, m, 0.3, 4, max_decoding_steps=tgb.STEPS)
    assert all(len(entry) > 1 for entry in nbest)
    refs = ['<' + nbest[0][-1][0] + '>', nbest[1][1][0][:-1]]       # the last entry itself; the second one, cut
    ref_ids = [[m.char_to_ind(c) for c in r] for r in refs]
    want = host_scores([[t for t, _ in entry] for entry in nbest], ref_ids)
    got = asr.score(refs, m)
    assert got == want
    assert sum(got[0].oracle[1][:3]) == 0 and got[0].oracle[0] > 0 and sum(got[0].chars[:3]) > 0
    # the greedy decode after it is scored again, not the beam
    assert asr.decode_many(xs, lens, lm, m, 0.3, max_decoding_steps=tgb.STEPS) == greedy
    assert asr.score(refs, m) == host_scores([[t] for t in greedy], ref_ids)


def test_asr_tester_with_decode_score(tmp_path):
    from ss_asr_amd.ASRDataset import prepare_y
    from ss_asr_amd.trainer import ASRTester
    fx = np.load(os.path.join(GOLDEN, 'dataset_ref.npz'), allow_pickle=False)
    dims = [int(v) for v in fx['cpt_dims']]
    root = str(tmp_path)
    index, _ = make_corpus(root, n=5, t_max=40, feat=dims[4], seed=5)
    os.makedirs(os.path.join(root, 'result', 'dec'))
    shutil.copy(os.path.join(GOLDEN, 'ref_small_asr.cpt'), os.path.join(root, 'result', 'dec', 'asr.cpt'))

    def tester(beam, **decode_keys):
        config = {'asr': dict({'mdl': {'encoder_state_size': dims[1], 'decoder_state_size': dims[2],
                                       'mlp_out_size': dims[3], 'feature_dim': dims[4], 'tf_rate': 1.0},
                               'test_index': index, 'decode_lm_weight': 0.5, 'decode_beam_size': beam, 'decode_jobs': 1,
                               'max_decode_step_ratio': 0.25, 'loader_jobs': 0}, **decode_keys),
                  'char_lm': {'mdl': {'hidden_size': 16}}}
        paras = types.SimpleNamespace(name='dec', logdir=os.path.join(root, 'runs'), ckpdir=os.path.join(root, 'result'),
                                      verbose=False, seed=1)
        torch.manual_seed(3)
        t = ASRTester(config, paras)
        t.load_data()
        t.set_model()
        t.decode_group = 2                                          # three launches: 2 + 2 + 1
        return t

    for beam in (1, 3):
        t0 = tester(beam)
        plain = t0.exec()
        assert not hasattr(t0, 'last_scores') and not hasattr(t0, 'last_error_rates')
        t = tester(beam, decode_score=True)
        assert t.decode_file == t0.decode_file
        t.lm = t0.lm
        said = []
        t.verbose = said.append
        assert t.exec() == plain and len(t.last_scores) == 5
        assert said[-1].startswith('CER ') and 'WER' in said[-1]
        ref_ids = [prepare_y(y)[0][0].tolist() for _, y in t.test_set]
        # the n-best lists, decoded again one utterance at a time
        from ss_asr_amd.ASRDataset import prepare_x
        nbest = []
        for x, _ in t.test_set:
            x, l = prepare_x(x, t.device)
            nbest.append([s for s, _ in t.asr_model.decode_nbest([x[:, :l[0]]], [l], t.lm, t.mapper, 0.5, beam)[0]])
        assert [n[0] for n in nbest] == plain
        want = host_scores(nbest, ref_ids)
        assert t.last_scores == want
        best, oracle = ErrorStats(), ErrorStats()
        for s in want:
            best.add(s.chars, s.words)
            oracle.add(s.oracle[1], s.oracle[2])
        assert t.last_error_rates == {'cer': best.cer, 'wer': best.wer, 'oracle_cer': oracle.cer,
                                      'oracle_wer': oracle.wer, 'chars': tuple(best.chars), 'words': tuple(best.words)}
        assert best.chars[3] == sum(sum(c >= 2 for c in r) for r in ref_ids) > 0
        assert oracle.wer <= best.wer and best.cer > 0
