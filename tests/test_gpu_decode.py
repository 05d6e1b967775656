"""Inference on the GPU: ASR.decode / decode_many (ssasr_decode_greedy), CharLM.forward (ssasr_charlm_step) and
trainer.ASRTester against what the REFERENCE's ASR.decode + CharLM decoded on CPU (tests/golden/decode_*.npz,
written by tools/make_decode_golden.py: inputs, weight seeds, and per lm_weight the emitted characters, their
count and every step's `final_predict` row).

Score tolerance: SCORE_ATOL = 5e-5 absolute, the bound test_forward_matches_reference holds for logits.  Every
fixture case keeps a top-1 / top-2 gap >= 1e-3 at every step, so a difference inside the bound cannot flip an
argmax and the character sequences must be EQUAL."""
import glob
import os
import shutil
import types

import numpy as np
import pytest
import torch

import las_oracle as lo
from conftest import GOLDEN
from test_host_cpu import make_corpus

pytestmark = pytest.mark.gpu

SCORE_ATOL = 5e-5
CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, 'decode_*.npz')))
DEV = 'cuda:0'


class Mapper:
    chars = lo.TOKENS + lo.ALL_CHARS

    def char_to_ind(self, c):
        return self.chars.index(c)

    def ind_to_char(self, i):
        return self.chars[i]


_models = {}


def models(fx):
    """(ASR, CharLM) of a fixture on the GPU, built once per (dims, seeds)."""
    from ss_asr_amd.asr import ASR
    from ss_asr_amd.charlm import CharLM
    dims = tuple(int(v) for v in fx['dims'])
    key = (dims, int(fx['asr_weights_seed']), int(fx['lm_weights_seed']), int(fx['lm_hidden']))
    if key not in _models:
        torch.manual_seed(0)
        asr = lo.seeded_weights(ASR(*dims, 1.0), key[1]).to(DEV).eval()
        lm = lo.seeded_generic_weights(CharLM(dims[0], key[3]), key[2]).to(DEV).eval()
        _models[key] = (asr, lm)
    return _models[key]


def decoded(asr):
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in asr.last_decode]


def test_the_fixtures_cover_what_they_must(golden):
    tags = set()
    for name in CASES:
        fx = golden(name)
        tags |= set(str(t) for t in fx['tags'])
        assert min(float(fx['w0_min_gap']), float(fx['w1_min_gap'])) >= 1e-3
    assert {'eos_late', 'eos_early', 'cap', 'lm_changes_text'} <= tags
    assert any(golden(n)['x'].shape[1] // 8 > 128 for n in CASES)


@pytest.mark.parametrize('k', [0, 1])
@pytest.mark.parametrize('name', CASES)
def test_decode_matches_the_reference(golden, name, k):
    fx = golden(name)
    asr, lm = models(fx)
    x = torch.from_numpy(fx['x']).to(DEV)
    text = asr.decode(x, [x.shape[1]], lm, Mapper(), float(fx['lm_weights'][k]))
    chars, n_chars, scores, att = decoded(asr)
    n, ref = int(fx['w%d_n_chars' % k]), fx['w%d_scores' % k]
    steps = ref.shape[0]
    err = float(np.abs(scores[0, :steps] - ref).max())
    print('%s lm_weight %.1f: %d characters, %d steps, max |score - reference| %.3e' % (
        name, float(fx['lm_weights'][k]), n, steps, err))
    assert int(n_chars[0]) == n
    assert np.array_equal(chars[0, :n], fx['w%d_chars' % k])
    assert text == str(fx['w%d_text' % k])
    assert err <= SCORE_ATOL
    # rows past the last executed step are zero
    assert not scores[0, steps:].any() and not chars[0, steps:].any() and not att[0, steps:].any()
    np.testing.assert_allclose(att[0, :steps].sum(-1), 1.0, atol=1e-5)


def gru_cell64(x, h, w_ih, w_hh, b_ih, b_hh):
    """nn.GRUCell in float64, gate order r, z, n."""
    H = h.shape[1]
    gi, gh = x @ w_ih.t() + b_ih, h @ w_hh.t() + b_hh
    r = torch.sigmoid(gi[:, :H] + gh[:, :H])
    z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
    n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
    return (1 - z) * n + z * h


@pytest.mark.parametrize('batch', [1, 3])
@pytest.mark.parametrize('hidden', [16, 128])
def test_charlm_forward_matches_a_float64_grucell(golden, batch, hidden):
    from ss_asr_amd.charlm import CharLM
    seed = int(golden(CASES[0])['lm_weights_seed'])
    lm = lo.seeded_generic_weights(CharLM(50, hidden), seed)
    sd = {k: v.double() for k, v in lm.state_dict().items()}
    lm = lm.to(DEV)
    rng = np.random.default_rng(hidden + batch)
    h1, h2 = lm.init_hidden(batch, DEV)
    r1, r2 = h1.double().cpu(), h2.double().cpu()
    for step in range(3):
        x = torch.from_numpy(rng.integers(0, 50, size=batch))
        out, (h1, h2) = lm(x.to(DEV), h1, h2)
        e = sd['emb.weight'][x]
        r1 = gru_cell64(e, r1, *[sd['layer_1.' + n] for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')])
        r2 = gru_cell64(r1, r2, *[sd['layer_2.' + n] for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')])
        ref = r2 @ sd['out.weight'].t() + sd['out.bias']
        torch.cuda.synchronize()
        errs = [float((a.double().cpu() - b).abs().max()) for a, b in ((out, ref), (h1, r1), (h2, r2))]
        print('batch %d hidden %d step %d: max errors out %.2e h1 %.2e h2 %.2e' % (batch, hidden, step, *errs))
        assert out.shape == (batch, 50) and max(errs) <= SCORE_ATOL


@pytest.mark.parametrize('name', CASES)
def test_decode_without_lm_follows_the_greedy_forward(golden, name):
    fx = golden(name)
    asr, _ = models(fx)
    x = torch.from_numpy(fx['x']).to(DEV)
    text = asr.decode(x, [x.shape[1]], None, Mapper(), 0.7)
    chars, n_chars, scores, _ = decoded(asr)
    n = int(n_chars[0])
    steps = min(n + 1, 200)
    with torch.no_grad():
        _, logits, _ = asr(x, steps, teacher=None, state_len=[x.shape[1]])
    want = logits[0].argmax(-1).cpu().numpy()
    assert np.array_equal(chars[0, :steps], want)
    assert (n == 200 and 1 not in want) or (want[n] == 1 and 1 not in want[:n])
    assert text == ''.join(Mapper.chars[c] for c in want[:n])
    # without an LM the scores are the speller's log_softmax alone
    ref = torch.log_softmax(logits[0], -1).cpu().numpy()
    assert np.abs(scores[0, :steps] - ref).max() <= SCORE_ATOL


@pytest.mark.parametrize('group', ['small', 'full'])
def test_a_batch_decodes_every_utterance_as_it_decodes_alone(golden, group):
    names = [n for n in CASES if ('small' in n) == (group == 'small')]
    # the model of the group's first fixture (full: the one whose own utterance stops at <EOS> without the LM and
    # runs into the cap with it)
    fx = golden(names[0])
    asr, lm = models(fx)
    xs = [torch.from_numpy(golden(n)['x']).to(DEV) for n in names]
    xs += [xs[0][:, :72], xs[-1][:, :9], xs[0][:, :25]]            # T' = 9, 1, 3 beside the fixtures' own
    lens = [[x.shape[1]] for x in xs]
    for k, w in enumerate((0.0, 0.5)):
        texts = asr.decode_many(xs, lens, lm, Mapper(), w)
        batch = decoded(asr)
        assert int(batch[1][0]) == int(fx['w%d_n_chars' % k])         # utterance 0 is the model's own fixture
        assert batch[0].shape[0] == len(xs) and batch[3].shape[2] == max(l[0] // 8 for l in lens)
        for i, (x, l) in enumerate(zip(xs, lens)):
            assert asr.decode(x, l, lm, Mapper(), w) == texts[i]
            alone = decoded(asr)
            for a, b in zip(alone[:3], batch[:3]):
                assert np.array_equal(a[0], b[i]), (i, w)
            t = alone[3].shape[2]
            assert np.array_equal(alone[3][0], batch[3][i, :, :t]) and not batch[3][i, :, t:].any()
    if group == 'full':
        # the cap and an early <EOS> in ONE launch: with lm_weight 0.5 the reference decodes utterance 0 into the
        # 200-step cap (its fixture) and, with the same weights, utterance 1 to 5 characters (top-2 gap 9e-4)
        n = batch[1]
        assert 'eos_late' in fx['tags'] and n.max() == 200 and n.min() < 200, n


def test_asr_tester_end_to_end(tmp_path):
    from ss_asr_amd.trainer import ASRTester
    fx = np.load(os.path.join(GOLDEN, 'dataset_ref.npz'), allow_pickle=False)
    dims = [int(v) for v in fx['cpt_dims']]
    root = str(tmp_path)
    index, lens = make_corpus(root, n=5, t_max=40, feat=dims[4], seed=5)
    os.makedirs(os.path.join(root, 'result', 'dec'))
    shutil.copy(os.path.join(GOLDEN, 'ref_small_asr.cpt'), os.path.join(root, 'result', 'dec', 'asr.cpt'))
    config = {'asr': {'mdl': {'encoder_state_size': dims[1], 'decoder_state_size': dims[2], 'mlp_out_size': dims[3],
                              'feature_dim': dims[4], 'tf_rate': 1.0},
                      'test_index': index, 'decode_lm_weight': 0.5, 'decode_beam_size': 1, 'decode_jobs': 1,
                      'max_decode_step_ratio': 0.25, 'loader_jobs': 0},
              'char_lm': {'mdl': {'hidden_size': 16}}}
    paras = types.SimpleNamespace(name='dec', logdir=os.path.join(root, 'runs'), ckpdir=os.path.join(root, 'result'),
                                  verbose=False, seed=1)
    torch.manual_seed(3)
    tester = ASRTester(config, paras)
    assert tester.decode_file == 'decode_beam_1_len_0.25'
    tester.load_data()
    tester.set_model()
    assert tester.decode_file == 'decode_beam_1_len_0.25_lm0.5' and len(tester.test_set) == 5
    tester.decode_group = 2                                         # three launches: 2 + 2 + 1
    got = tester.exec()
    from ss_asr_amd.ASRDataset import prepare_x
    xs, x_lens = [], []
    for x, _ in tester.test_set:
        x, l = prepare_x(x, tester.device)
        xs.append(x[:, :l[0]])
        x_lens.append(l)
    assert [l[0] for l in x_lens] == lens
    assert got == tester.asr_model.decode_many(xs, x_lens, tester.lm, tester.mapper, 0.5) and len(got) == 5
    assert all(isinstance(s, str) for s in got)
    no_lm = tester.exec(lm_weight=0.0)
    assert no_lm == tester.asr_model.decode_many(xs, x_lens, tester.lm, tester.mapper, 0.0)
    assert no_lm == tester.asr_model.decode_many(xs, x_lens, None, tester.mapper, 0.0)
