"""Joint CTC / attention decoding on the GPU (ssasr_decode_beam_ctc; ASR.decode / decode_many / decode_nbest with
ctc_weight; ASRTester with asr.decode_ctc_weight) against the float64 CPU beam search of tests/decode_checker.py with
its CTC term on: the prefix scorer is the one that test_ctc_decode_cpu.py pins by brute force and against torch's
ctc_loss.  The head's weights come from a seed (HEAD_SEED, las_oracle.seeded_generic_weights on an nn.Linear).

Tolerance of a hypothesis' score: 5e-5 * steps for the attention and LM rows (SCORE_ATOL, unchanged) plus
lambda * C for the CTC part: the CTC terms of a hypothesis telescope to lambda * psi(final prefix), one term.
C = 8 * CTC_NOISE, CTC_NOISE = max |psi32 - psi64| of the checker's scorer run in float32 (head product and
log_softmax included) and in float64 over the compared hypotheses (the rule of test_gpu_charlm_train.py); the test
recomputes and prints the noise.  Measured on an MI355X: the worst
|score error| of a compared hypothesis is printed by every test below and recorded in DESIGN 4.12.

A (case, K, lambda) triple is compared only when every kept / dropped, kept / kept and emitted / emitted gap of the
checker is >= MIN_GAP = 1e-3 (the project's rule); the N-best lists must then be EQUAL.  HEAD_SEED is the seed among
0..15 that keeps the most triples."""
import math
import os
import shutil
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import decode_checker as dc
import las_oracle as lo
import test_ctc_decode_cpu as tcc
import test_gpu_beam as tgb
import test_gpu_decode as tgd
from conftest import GOLDEN
from test_host_cpu import make_corpus

pytestmark = pytest.mark.gpu

SCORE_ATOL = tgd.SCORE_ATOL
MIN_GAP = tgb.MIN_GAP
DEV = tgd.DEV
Mapper = tgd.Mapper
EOS, BLANK, STEPS = 1, 0, 24
BEAMS = (2, 3, 5)
LAMBDAS = (0.3, 1.0)
HEAD_SEED = dc.HEAD_SEED
# test_gpu_beam's shapes (T' = 5, 3 and 20), and T' = 1 (9 frames) beside them.  With these near-uniform seeded heads no hypothesis of the
# 40- / 24- / 160-frame cases is ended by frames running out under any head seed 0..15 (checked with the checker on
# the CPU: the <EOS> candidates of the shorter prefixes fill the beam before a prefix as long as the utterance is
# kept), so that path is compared on one-frame utterances, where every kept character must be ended at step 1.
# They do not count towards the 12 triples.
EXTRA_FRAMES = 9
CASES = tgb.PAIR_CASES + [(n, EXTRA_FRAMES, k) for n in tgb.SMALL for k in (0, 1)]
CTC_NOISE = 1.3e-5           # max |psi32 - psi64| over every compared hypothesis (1.04e-5 on the triples, 1.30e-5 at K = 12), CPU
CTC_C = 8 * CTC_NOISE
NEG = -math.inf


def joint_beam(ref, K, S, lam, lm_weight):
    """The beam search with the CTC prefix score over the float64 model ref.  -> (hyps, min_gap, ran_out): hyps =
    [(chars, score, step it ended at, capped)] in output order; ran_out: a hypothesis was ended by <EOS> at a step
    where all its other candidates were at -inf."""
    r = dc.beam_search(ref, K, S, lm_weight, lam)
    return [h[:4] for h in r['hyps']], r['gap'], r['ran_out']


def final_psi(lp, text, ended):
    """What a hypothesis' CTC terms telescope to: psi(text), or log p(text) when <EOS> ended it."""
    st = tcc.prefix_chain(lp, text, EOS)[-1]
    return float(np.logaddexp(st.gn[-1], st.gb[-1])) if ended else float(st.psi)


def psi_noise(ref, hyps):
    """max |psi32 - psi64| of the hypotheses' final prefixes (the finite ones)."""
    worst = 0.0
    for chars, _, _, was_capped in hyps:
        a, b = final_psi(ref.lp, chars, not was_capped), final_psi(ref.lp32, chars, not was_capped)
        if a > NEG:
            worst = max(worst, abs(a - b))
    return worst


def bound(steps, lam):
    return SCORE_ATOL * steps + lam * CTC_C


_beams, _joint = {}, {}
ref_of = dc.model


def reference(golden, name, frames, k, K, lam):
    key = (name, frames, k, K, lam)
    if key not in _beams:
        w = None if k is None else float(golden(name)['lm_weights'][k])
        _beams[key] = joint_beam(ref_of(golden, name, frames), K, STEPS, lam, w)
    return _beams[key]


def models(fx):
    """(JointCTCASR with tgd.models' weights and the seeded head, CharLM) on the GPU."""
    from ss_asr_amd.ctc import JointCTCASR
    dims = tuple(int(v) for v in fx['dims'])
    key = (dims, int(fx['asr_weights_seed']))
    if key not in _joint:
        torch.manual_seed(0)
        asr = lo.seeded_weights(JointCTCASR(*dims, 1.0), key[1])
        lo.seeded_generic_weights(asr.ctc_head, HEAD_SEED)
        _joint[key] = asr.to(DEV).eval()
    plain, lm = tgd.models(fx)
    joint = _joint[key]
    assert torch.equal(joint.char_trans.weight, plain.char_trans.weight)
    return joint, lm


def entry_args(asr, lm, x, lm_weight):
    with torch.no_grad():
        feat, enc_lens = asr._encode_packed([x], [[x.shape[1]]])
    return (feat, enc_lens, asr._decoder_params(), (asr.attention.psi.weight, asr.attention.psi.bias), lm, lm_weight,
            EOS, STEPS)


def head_of(asr, lam):
    return asr.ctc_head.weight, asr.ctc_head.bias, lam


@pytest.mark.parametrize('K', [1, 3])
def test_weight_zero_is_the_plain_beam_kernel_and_leaves_the_head_unread(golden, K):
    from ss_asr_amd import ops
    for name in (tgb.SMALL[0], tgb.FULL_CASE):
        fx = golden(name)
        asr, lm = models(fx)
        args = entry_args(asr, lm, torch.from_numpy(fx['x']).to(DEV), 0.5)
        plain = [t.cpu().numpy() for t in ops.decode_beam(*args, K)]
        nan_head = (torch.full_like(asr.ctc_head.weight, math.nan), torch.full_like(asr.ctc_head.bias, math.nan), 0.0)
        got = [t.cpu().numpy() for t in ops.decode_beam_ctc(*args, K, nan_head)]
        for a, b in zip(plain, got):
            assert a.dtype == b.dtype and np.array_equal(a, b)
        assert int(plain[3][0]) >= 1 and np.isfinite(got[2]).all()


def test_joint_beam_search_matches_the_float64_checker(golden):
    triples = differs = ran_out = full = 0
    noise = worst = 0.0
    for name, frames, k in CASES:
        fx = golden(name)
        asr, lm = models(fx)
        ref = ref_of(golden, name, frames)
        w = float(fx['lm_weights'][k])
        x = torch.from_numpy(fx['x'][:, :frames]).to(DEV)
        for K in BEAMS:
            plain_best = tgb.reference(golden, name, frames, k, K)[0][0][0]
            for lam in LAMBDAS:
                hyps, gap, out = reference(golden, name, frames, k, K, lam)
                if gap < MIN_GAP:
                    print('%s frames %d lm_weight %.1f K %d lambda %.1f: smallest gap %.2e, not compared'
                          % (name, frames, w, K, lam, gap))
                    continue
                nbest = asr.decode_nbest([x], [[frames]], lm, Mapper(), w, K, max_decoding_steps=STEPS, ctc_weight=lam)[0]
                chars, n_chars, scores, n_hyps = tgb.beam_arrays(asr)
                assert asr.decode(x, [frames], lm, Mapper(), w, max_decoding_steps=STEPS, beam_size=K,
                                  ctc_weight=lam) == nbest[0][0]
                errs = [abs(float(scores[0, i]) - h[1]) for i, h in enumerate(hyps[:int(n_hyps[0])])]
                noise = max(noise, psi_noise(ref, hyps))
                worst = max(worst, max(errs))
                print('%s frames %d lm_weight %.1f K %d lambda %.1f: smallest gap %.2e, %d hypotheses, ended at %s, '
                      'frames ran out %s, max |score error| %.2e' % (name, frames, w, K, lam, gap, len(hyps),
                                                                      [h[2] for h in hyps], out, max(errs)))
                assert int(n_hyps[0]) == len(hyps) == len(nbest) <= K
                for i, (ref_chars, ref_score, ended, was_capped) in enumerate(hyps):
                    n = int(n_chars[0, i])
                    assert n == len(ref_chars) and np.array_equal(chars[0, i, :n], ref_chars), (name, frames, k, K, lam, i)
                    assert not chars[0, i, n:].any()
                    assert nbest[i][0] == tgb.text_of(ref_chars) and nbest[i][1] == float(scores[0, i])
                    assert abs(float(scores[0, i]) - ref_score) <= bound(min(ended + 1, STEPS), lam)
                rest = slice(len(hyps), None)
                assert not chars[0, rest].any() and not n_chars[0, rest].any() and not scores[0, rest].any()
                triples += frames != EXTRA_FRAMES
                full += name == tgb.FULL_CASE
                differs += hyps[0][0] != plain_best
                ran_out += out
    print('%d triples compared: best differs from the lambda = 0 best in %d, frames ran out in %d, full dims %d; '
          'psi noise (float32 against float64) %.3e, worst |score error| %.3e' % (triples, differs, ran_out, full, noise, worst))
    assert triples >= 12 and differs >= 1 and ran_out >= 1 and full >= 1


def test_every_emitted_score_is_the_joint_score_of_its_text_at_twelve_hypotheses(golden):
    """K * V = 600 candidates: a second scoring pass over the waves, and matmat's second pass (K > 8).  No gap is
    needed: whatever the kernel chose, an emitted score must be the joint score of that exact text."""
    name, frames, K, lam = tgb.FULL_CASE, 160, 12, 0.3
    fx = golden(name)
    assert K * int(fx['dims'][0]) > 512
    asr, lm = models(fx)
    ref = ref_of(golden, name, frames)
    w = float(fx['lm_weights'][0])
    x = torch.from_numpy(fx['x'][:, :frames]).to(DEV)
    nbest = asr.decode_nbest([x], [[frames]], lm, Mapper(), w, K, max_decoding_steps=STEPS, ctc_weight=lam)[0]
    chars, n_chars, scores, n_hyps = tgb.beam_arrays(asr)
    nh = int(n_hyps[0])
    assert 1 <= nh <= K == chars.shape[1] and len(nbest) == nh
    assert np.all(np.diff(scores[0, :nh]) <= 0) and np.isfinite(scores[0, :nh]).all()
    seen = set()
    for i in range(nh):
        n = int(n_chars[0, i])
        text, ended = [int(c) for c in chars[0, i, :n]], n < STEPS
        want = dc.forced(ref, text, ended, lam, w)[0]
        err = abs(float(scores[0, i]) - want)
        print('hypothesis %d: %d characters, %s, score %.6f, joint score of the text %.6f, error %.2e'
              % (i, n, 'ended' if ended else 'capped', float(scores[0, i]), want, err))
        assert BLANK not in text and EOS not in text
        assert err <= bound(n + ended, lam)
        seen.add((tuple(text), ended))
    assert len(seen) == nh
    assert not scores[0, nh:].any() and not chars[0, nh:].any() and not n_chars[0, nh:].any()


def test_frames_run_out(golden):
    name, frames, K, lam = tgb.SMALL[0], 24, 5, 0.3
    fx = golden(name)
    asr, lm = models(fx)
    x = torch.from_numpy(fx['x'][:, :frames]).to(DEV)
    for k in (0, 1):
        nbest = asr.decode_nbest([x], [[frames]], lm, Mapper(), float(fx['lm_weights'][k]), K, max_decoding_steps=STEPS,
                                 ctc_weight=lam)[0]
        chars, n_chars, scores, n_hyps = tgb.beam_arrays(asr)
        nh = int(n_hyps[0])
        assert 1 <= nh <= K and np.isfinite(scores[0, :nh]).all()
        for i in range(nh):
            n = int(n_chars[0, i])
            text = [int(c) for c in chars[0, i, :n]]
            repeats = sum(a == b for a, b in zip(text, text[1:]))
            print('lm %d hypothesis %d: %s score %.5f' % (k, i, text, float(scores[0, i])))
            assert n < STEPS and n + repeats <= 3 and BLANK not in text


def test_at_weight_one_without_lm_a_score_is_torch_ctc_loss_of_the_text(golden):
    name, frames, K = tgb.SMALL[0], 40, 3
    fx = golden(name)
    asr, _ = models(fx)
    ref = ref_of(golden, name, frames)
    x = torch.from_numpy(fx['x'][:, :frames]).to(DEV)
    asr.decode_nbest([x], [[frames]], None, Mapper(), 0.0, K, max_decoding_steps=STEPS, ctc_weight=1.0)
    chars, n_chars, scores, n_hyps = tgb.beam_arrays(asr)
    nh = int(n_hyps[0])
    assert 1 <= nh <= K
    lp = torch.from_numpy(ref.lp).unsqueeze(1)
    for i in range(nh):
        n = int(n_chars[0, i])
        assert n < STEPS                          # five frames hold at most five characters: all end with <EOS>
        text = [int(c) for c in chars[0, i, :n]]
        want = -float(F.ctc_loss(lp, torch.tensor([text], dtype=torch.long), torch.tensor([ref.T]), torch.tensor([n]),
                                 blank=BLANK, reduction='sum'))
        err = abs(float(scores[0, i]) - want)
        print('hypothesis %d: %s score %.6f, -ctc_loss %.6f, error %.2e' % (i, text, float(scores[0, i]), want, err))
        assert err <= bound(n + 1, 1.0)


def test_a_group_decodes_every_utterance_as_it_decodes_alone(golden):
    fx = golden(tgb.SMALL[0])
    asr, lm = models(fx)
    x = torch.from_numpy(fx['x']).to(DEV)
    other = torch.from_numpy(golden(tgb.SMALL[1])['x']).to(DEV)
    both = torch.cat([x, other, x, other], 1)
    xs = [both[:, :f] for f in (160, 72, 40, 25, 9)]                # T' = 20, 9, 5, 3, 1
    lens = [[t.shape[1]] for t in xs]
    texts = asr.decode_many(xs, lens, lm, Mapper(), 0.5, max_decoding_steps=STEPS, beam_size=3, ctc_weight=0.3)
    group = tgb.beam_arrays(asr)
    assert group[0].shape == (5, 3, STEPS) and group[3].shape == (5,)
    for i, (t, l) in enumerate(zip(xs, lens)):
        assert asr.decode(t, l, lm, Mapper(), 0.5, max_decoding_steps=STEPS, beam_size=3, ctc_weight=0.3) == texts[i]
        alone = tgb.beam_arrays(asr)
        for a, b in zip(alone, group):
            assert np.array_equal(a[0], b[i]), i
        nh = int(group[3][i])
        assert 1 <= nh <= 3 and np.isfinite(group[2][i, :nh]).all()
        assert not group[0][i, nh:].any() and not group[1][i, nh:].any() and not group[2][i, nh:].any()
        assert (group[1][i, :nh] <= l[0] // 8).all()                # no more characters than frames


def test_limits(golden):
    import ctypes
    from ss_asr_amd import _lib, ops
    fx = golden(tgb.SMALL[0])
    asr, lm = models(fx)
    args = entry_args(asr, lm, torch.from_numpy(fx['x']).to(DEV), 0.5)
    lib = _lib.load()
    d, outs, keep = ops.beam_struct(*args, 3, ctc=True)
    N, T, E = args[0].shape
    A, D = asr.attention.phi.weight.shape
    need = int(lib.ssasr_decode_beam_ctc_ws_bytes(N, 3, T, E, A, D, 50, lm.hidden_size, STEPS))
    assert d.ws_bytes == need > int(lib.ssasr_decode_beam_ws_bytes(N, 3, T, E, A, D, 50, lm.hidden_size, STEPS))
    for t in outs:
        t.fill_(7)

    def call(weight=0.3, blank=BLANK, ws_bytes=need):
        c, c_keep = ops.ctc_prefix_struct(head_of(asr, weight), blank)
        d.ws_bytes = ws_bytes
        return lib.ssasr_decode_beam_ctc(ctypes.byref(d), ctypes.byref(c), ops._stream())
    for bad in (-0.1, 1.5, math.nan):
        assert call(weight=bad) == -1
    assert call(blank=EOS) == -1 and call(blank=50) == -1 and call(blank=-1) == -1
    assert call(ws_bytes=need - 1) == -1 and call(weight=0.0, ws_bytes=need - 1) == -1
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in outs)
    assert call() == 0
    torch.cuda.synchronize()
    assert 1 <= int(outs[3][0]) <= 3
    with pytest.raises(RuntimeError, match='invalid argument'):
        ops.decode_beam_ctc(*args, 33, head_of(asr, 0.3))
    # beam sizes 1 and 32 through the Python surface
    x = torch.from_numpy(fx['x']).to(DEV)
    for K in (1, 32):
        nbest = asr.decode_nbest([x], [[x.shape[1]]], lm, Mapper(), 0.5, K, max_decoding_steps=STEPS, ctc_weight=0.3)[0]
        chars, n_chars, scores, n_hyps = tgb.beam_arrays(asr)
        assert chars.shape == (1, K, STEPS) and 1 <= int(n_hyps[0]) == len(nbest) <= K
        assert np.isfinite(scores[0, :len(nbest)]).all() and np.all(np.diff(scores[0, :len(nbest)]) <= 0)


def test_asr_tester_with_a_joint_model(tmp_path):
    from ss_asr_amd.ASRDataset import prepare_x
    from ss_asr_amd.ctc import JointCTCASR
    from ss_asr_amd.trainer import ASRTester
    fx = np.load(os.path.join(GOLDEN, 'dataset_ref.npz'), allow_pickle=False)
    dims = [int(v) for v in fx['cpt_dims']]
    root = str(tmp_path)
    index, lens = make_corpus(root, n=5, t_max=40, feat=dims[4], seed=5)
    os.makedirs(os.path.join(root, 'result', 'dec'))
    torch.manual_seed(11)
    trained = JointCTCASR(*dims[:5], 1.0, ctc_weight=0.3)
    trained.load_state_dict(torch.load(os.path.join(GOLDEN, 'ref_small_asr.cpt'), map_location='cpu'))
    lo.seeded_generic_weights(trained.ctc_head, HEAD_SEED)
    torch.save(trained.state_dict(), os.path.join(root, 'result', 'dec', 'asr.cpt'))
    assert 'ctc_head.weight' in trained.state_dict()

    def tester(**decode_keys):
        config = {'asr': dict({'mdl': {'encoder_state_size': dims[1], 'decoder_state_size': dims[2],
                                       'mlp_out_size': dims[3], 'feature_dim': dims[4], 'tf_rate': 1.0, 'ctc_weight': 0.3},
                               'test_index': index, 'decode_lm_weight': 0.5, 'decode_beam_size': 3, 'decode_jobs': 1,
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
    t = tester(decode_ctc_weight=0.3)
    assert isinstance(t.asr_model, JointCTCASR) and t.decode_file == 'decode_beam_3_len_0.25_lm0.5_ctc0.3'
    assert torch.equal(t.asr_model.ctc_head.weight.cpu(), trained.ctc_head.weight)
    said = []
    t.verbose = said.append
    got = t.exec()
    assert 'beam search, beam size 3' in said[0] and 'CTC weight 0.3' in said[0]
    xs, x_lens = [], []
    for x, _ in t.test_set:
        x, l = prepare_x(x, t.device)
        xs.append(x[:, :l[0]])
        x_lens.append(l)
    nbest = t.asr_model.decode_nbest(xs, x_lens, t.lm, t.mapper, 0.5, 3, ctc_weight=0.3)
    assert got == [n[0][0] for n in nbest] and len(got) == 5 and all(isinstance(s, str) for s in got)
    # the same model without the key: the attention / LM scores alone, under the old file name
    t0 = tester()
    assert isinstance(t0.asr_model, JointCTCASR) and t0.decode_file == 'decode_beam_3_len_0.25_lm0.5'
    t0.lm = t.lm
    t0.verbose = said.append
    plain = t0.exec()
    assert 'CTC' not in said[-2]
    assert plain == t0.asr_model.decode_many(xs, x_lens, t0.lm, t0.mapper, 0.5, beam_size=3) and len(plain) == 5
    t0.decode_ctc_weight = 1.5
    with pytest.raises(ValueError, match='decode_ctc_weight'):
        t0.exec()
