"""CharLM training on the GPU: ssasr_charlm_train_fwd / _bwd (csrc/charlm_train.hip), engine.CharLMTrainStep and
trainer.CHARLMTrainer against what the REFERENCE's CharLM, CrossEntropyLoss, clip_grad_norm_ and Adam computed on
CPU for 3 consecutive steps (tests/golden/charlm_*.npz, written by tools/make_charlm_golden.py).

Bound: every fixture quantity comes with noise = max |fp32 - fp64| of the reference's own trajectory; the kernels
may differ from the reference's fp32 by summation order only (MFMA k order within a step, K = U * B in the gradient
products), which the factor FACTOR = 8 covers.  The loss and the gradient norm are ONE number per step: the distance of a single
fp32 number from its fp64 twin can fall far below the resolution of fp32 by chance (charlm_small, step 2: the
reference's norm 2.3147 lies 5.8e-9 from its fp64 twin, half an ulp is 1.2e-7), so for these two scalars the noise is
the max over the three steps of the trajectory; the arrays (per-row losses, gradients, weights) take each step's own."""
import os
import shutil
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

import las_oracle as lo
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
FACTOR = 8.0
CASES = ('charlm_small', 'charlm_tile', 'charlm_full')


def _fx(name):
    return np.load(os.path.join(GOLDEN, name + '.npz'), allow_pickle=False)


def _model(fx):
    from ss_asr_amd.charlm import CharLM
    return lo.seeded_generic_weights(CharLM(int(fx['V']), int(fx['H'])), int(fx['weights_seed'])).to(DEV)


def _sample_index(seed, k, numel, size):
    if numel <= size:
        return np.arange(numel)
    return np.sort(np.random.default_rng(seed * 1000 + k).choice(numel, size, replace=False))


def _close(tag, got, want, noise, report):
    err = float(np.max(np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))))
    ratio = err / noise if noise > 0 else (0.0 if err == 0 else float('inf'))
    report.append('%-22s err %.3e noise %.3e ratio %.2f' % (tag, err, noise, ratio))
    print(report[-1])
    return err <= FACTOR * noise


@pytest.mark.parametrize('case', CASES)
def test_three_steps_match_the_reference(case):
    from ss_asr_amd.engine import CharLMTrainStep
    fx = _fx(case)
    lm = _model(fx)
    names = [n for n, _ in lm.named_parameters()]
    assert names == [str(n) for n in fx['names']]
    U, B = int(fx['U']), int(fx['B'])
    step = CharLMTrainStep(lm, float(fx['tf_rate']), lr=float(fx['lr']), eps=float(fx['eps']),
                           grad_clip=float(fx['max_norm']))
    sampled, size, seed = bool(fx['sampled']), int(fx['sample_size']), int(fx['weights_seed'])
    report, bad = [], []
    for s in range(3):
        y = torch.from_numpy(fx['y'][s]).to(DEV)
        fed = fx['fed'][s]                                     # [U+1, B]; feed[b][t] = what step t + 1 was fed
        feed = torch.from_numpy(np.ascontiguousarray(fed[1:].T)).to(DEV)
        # the gradients the optimizer sees are the CLIPPED ones (norm < 5 in every case: unchanged); read them
        # before the update kernel zeroes the buffer
        chunk = None
        from ss_asr_amd import ops
        if not step.flat.clean:
            step.flat.zero_grad()
        chunk = ops.charlm_chunk(lm, y, feed=feed, modes=torch.zeros(U, device=DEV, dtype=torch.int32))
        ops.charlm_chunk_backward(lm, chunk, dloss=1.0 / B)
        torch.cuda.synchronize()
        grads = [p.grad.detach().cpu().numpy().reshape(-1).copy() for p in lm.parameters()]
        step.flat.clean = False
        step.optim.clip_and_step(step.grad_clip, zero_grad=True)
        step.flat.clean = True
        norm, skipped = step.optim.poll(wait=True)
        assert not skipped and float(fx['grad_norm'][s]) < float(fx['max_norm'])
        assert np.array_equal(chunk.fed.cpu().numpy(), fed)
        rows = chunk.loss_rows.cpu().numpy()
        ok = [_close('s%d loss_rows' % s, rows, fx['loss_rows'][s], float(fx['noise_loss_rows'][s]), report),
              _close('s%d loss' % s, rows.astype(np.float64).mean(), fx['loss'][s], float(fx['noise_loss'].max()), report),
              _close('s%d grad_norm' % s, norm, fx['grad_norm'][s], float(fx['noise_grad_norm'].max()), report)]
        weights = [p.detach().cpu().numpy().reshape(-1) for p in lm.parameters()]
        for kind, mine in (('grads', grads), ('weights', weights)):
            got, want = [], []
            for k, t in enumerate(mine):
                keep = _sample_index(seed, k, t.size, size) if sampled else np.arange(t.size)
                got.append(t[keep])
                want.append(fx['%s_s%d_%d' % (kind, s, k)])
            ok.append(_close('s%d %s' % (s, kind), np.concatenate(got), np.concatenate(want),
                             float(fx['noise_' + kind][s]), report))
            norms = np.array([np.sqrt((t.astype(np.float64) ** 2).sum()) for t in mine])
            assert np.allclose(norms, fx['%s_norms_s%d' % (kind, s)], rtol=1e-4, atol=1e-7)
        bad += [report[-len(ok) + i] for i, o in enumerate(ok) if not o]
    assert not bad, '\n'.join(bad)


def test_rows_are_independent_of_the_batch():
    """charlm_tile's 17 rows (two tiles, the second with one live row) against rows 0, 15, 16 run alone."""
    from ss_asr_amd import ops
    fx = _fx('charlm_tile')
    lm = _model(fx)
    U = int(fx['U'])
    y = torch.from_numpy(fx['y'][0]).to(DEV)
    modes = torch.tensor([0, 1, 0, 1][:U], device=DEV, dtype=torch.int32)
    uni = torch.from_numpy(np.random.default_rng(3).random((U, y.shape[0])).astype(np.float32)).to(DEV)
    full = ops.charlm_chunk(lm, y, modes=modes, uniforms=uni, want_logits=True)
    for b in (0, 15, 16):
        one = ops.charlm_chunk(lm, y[b:b + 1].contiguous(), modes=modes, uniforms=uni[:, b:b + 1].contiguous(),
                               want_logits=True)
        assert torch.equal(one.loss_rows, full.loss_rows[b:b + 1])
        assert torch.equal(one.fed, full.fed[:, b:b + 1])
        assert torch.equal(one.logits, full.logits[:, b:b + 1])


def _cpu_chunk(lm_cpu, y, modes, uni):
    """Plain torch on CPU: nn.GRUCell loop, CE, the inverse-CDF draw (oracle/las_oracle.py, inverse_cdf_bounds).
    -> (loss, loss_rows, fed [U+1, B], smallest distance of a draw from a cumulative boundary / total)."""
    B, U = y.shape
    h1 = torch.zeros(B, lm_cpu.hidden_size)
    h2 = torch.zeros(B, lm_cpu.hidden_size)
    last = torch.zeros(B, dtype=torch.long)
    fed, rows, margin = [last.clone()], 0, 1.0
    for t in range(U):
        h1 = lm_cpu.layer_1(lm_cpu.emb(last), h1)
        h2 = lm_cpu.layer_2(h1, h2)
        out = lm_cpu.out(h2)
        rows = rows + nn.functional.cross_entropy(out, y[:, t], reduction='none')
        if modes[t] == 0:
            last = y[:, t].clone()
        else:
            last = torch.zeros(B, dtype=torch.long)
            for b in range(B):
                run, total = lo.inverse_cdf_bounds(out[b].detach().numpy())
                target = np.float32(uni[t, b]) * np.float32(total)
                v = int(np.argmax(run > target))
                margin = min(margin, float(np.min(np.abs(run.astype(np.float64) - float(target)))) / total)
                last[b] = v
        fed.append(last.clone())
    return rows.mean(), rows, torch.stack(fed), margin


@pytest.mark.parametrize('H,B,U,seed', [(16, 17, 3, 31), (256, 2, 3, 6)])
def test_sampled_steps_match_a_cpu_restatement(H, B, U, seed):
    """Sampled steps at fixed positions (odd t) with seeded uniforms; B = 17 crosses the tile edge, H = 256 is the
    upper end of the supported sizes.  The seeds are chosen so that every draw keeps 1e-3 * total from both
    neighbouring cumulative boundaries (with 50 boundaries a draw lands that close to one with probability 0.1, so
    the batches are small: 17 and 2 draws per sampled step).
    Bound: the fixture noise of the parity test scales with the magnitudes involved, so the CPU fp32 run is compared
    with its own float64 twin here (the same fed characters), and the kernel must be within FACTOR x that."""
    import copy
    from ss_asr_amd import ops
    from ss_asr_amd.charlm import CharLM
    V = 50
    lm_cpu = lo.seeded_generic_weights(CharLM(V, H), 40 + seed)
    rng = np.random.default_rng(seed)
    y = torch.from_numpy(rng.integers(0, V, (B, U)))
    modes = [1 if t % 2 == 1 else 0 for t in range(U)]
    uni = rng.random((U, B)).astype(np.float32)
    loss, rows, fed, margin = _cpu_chunk(lm_cpu, y, modes, uni)
    assert margin >= 1e-3, margin                       # no draw close enough to a boundary for rounding to move it
    lm_cpu.zero_grad()
    loss.backward()
    # float64 twin on the same trajectory: feed the fp32 run's characters
    lm64 = copy.deepcopy(lm_cpu).double()
    lm64.zero_grad()
    h1 = torch.zeros(B, H, dtype=torch.float64)
    h2 = torch.zeros(B, H, dtype=torch.float64)
    rows64 = 0
    for t in range(U):
        h1 = lm64.layer_1(lm64.emb(fed[t]), h1)
        h2 = lm64.layer_2(h1, h2)
        rows64 = rows64 + nn.functional.cross_entropy(lm64.out(h2), y[:, t], reduction='none')
    rows64.mean().backward()
    noise_rows = float((rows.detach().double() - rows64.detach()).abs().max())
    noise_grad = max(float((p.grad.double() - q.grad).abs().max()) for p, q in zip(lm_cpu.parameters(), lm64.parameters()))

    lm = copy.deepcopy(lm_cpu).to(DEV)
    lm.zero_grad()
    chunk = ops.charlm_chunk(lm, y.to(DEV), modes=torch.tensor(modes, dtype=torch.int32, device=DEV),
                             uniforms=torch.from_numpy(uni).to(DEV))
    ops.charlm_chunk_backward(lm, chunk)
    assert torch.equal(chunk.fed.cpu().long(), fed)     # every fed character, none excused
    report = []
    ok = _close('loss_rows', chunk.loss_rows.cpu().numpy(), rows.detach().numpy(), noise_rows, report)
    got = np.concatenate([p.grad.cpu().numpy().reshape(-1) for p in lm.parameters()])
    want = np.concatenate([p.grad.numpy().reshape(-1) for p in lm_cpu.parameters()])
    ok = _close('grads', got, want, noise_grad, report) and ok
    assert ok, '\n'.join(report)


def test_edges():
    from ss_asr_amd import _lib, ops
    from ss_asr_amd.charlm import CharLM
    lib = _lib.load()
    lm = lo.seeded_generic_weights(CharLM(50, 16), 9).to(DEV)
    y = torch.tensor([[7]], device=DEV)
    a = ops.charlm_chunk(lm, y, want_logits=True)                   # U = 1, B = 1
    out, _, _ = ops.charlm_step(lm, torch.zeros(1, device=DEV, dtype=torch.int32), torch.zeros(1, 16, device=DEV),
                                torch.zeros(1, 16, device=DEV))
    want = nn.functional.cross_entropy(out.cpu(), y.cpu()[:, 0], reduction='none')
    assert torch.allclose(a.loss_rows.cpu(), want, atol=2e-6) and a.fed.cpu().tolist() == [[0], [7]]
    assert torch.allclose(a.logits[0].cpu(), out.cpu(), atol=2e-6)
    lm.zero_grad()
    ops.charlm_chunk_backward(lm, a)
    assert all(torch.isfinite(p.grad).all() for p in lm.parameters())
    # a second call into the same workspace: the same bits
    y2 = torch.from_numpy(np.random.default_rng(1).integers(0, 50, (5, 7))).to(DEV)
    first = ops.charlm_chunk(lm, y2, want_logits=True)
    keep = (first.loss_rows.clone(), first.fed.clone(), first.logits.clone(), first.ws.clone())
    ops.charlm_chunk_backward(lm, first)                            # rewrites parts of the workspace
    again = ops.charlm_chunk(lm, y2, want_logits=True, ws=first.ws)
    assert again.ws.data_ptr() == first.ws.data_ptr()
    assert torch.equal(again.loss_rows, keep[0]) and torch.equal(again.fed, keep[1])
    assert torch.equal(again.logits, keep[2]) and torch.equal(again.ws, keep[3])
    # unsupported sizes: the query says 0, the entry points a negative code, before any launch
    for H in (8, 24, 272):
        assert int(lib.ssasr_charlm_train_ws_floats(4, 4, H, 50)) == 0
        with pytest.raises(RuntimeError):
            ops.charlm_chunk(CharLM(50, H).to(DEV), y2)
    assert int(lib.ssasr_charlm_train_ws_floats(4, 4, 16, 65)) == 0


def test_trainer_end_to_end(tmp_path):
    from test_host_cpu import make_corpus
    from ss_asr_amd import trainer
    from ss_asr_amd.charlm import CharLM
    chars = lo.TOKENS + lo.ALL_CHARS
    rng = np.random.default_rng(2)
    words = [''.join(chars[i] for i in rng.integers(3, 29, n)) for n in (3, 5, 4, 6)]
    text = ' '.join(words[i] for i in rng.integers(0, 4, 500))[:2048]
    root = str(tmp_path)
    path = os.path.join(root, 'text.txt')
    with open(path, 'w') as f:
        f.write(text)
    config = {'char_lm': {'opt': {'type': 'Adam', 'learning_rate': 0.01}, 'mdl': {'hidden_size': 16, 'tf_rate': 0.9},
                          'train_index': path, 'chunk_size': 8, 'train_batch_size': 4, 'n_epochs': 1,
                          'valid_step': 20, 'logging_step': 1, 'save_step': 1000}}
    paras = types.SimpleNamespace(name='dec', logdir=os.path.join(root, 'runs'), ckpdir=os.path.join(root, 'result'),
                                  verbose=False, seed=1)
    torch.manual_seed(4)
    t = trainer.LMTrainer(config, paras)
    assert type(t) is trainer.CHARLMTrainer
    t.load_data()
    t.set_model()
    assert len(t.train_set) == (2048 // 8) // 4
    first = []
    t.lg.scalar = lambda key, val, step, _f=first: _f.append(val)
    t.exec()
    t.close()
    assert len(first) == 64 and abs(first[0] - np.log(50)) < 0.5
    assert np.mean(first[-8:]) < np.log(50) - 0.3, (first[0], first[-8:])
    assert os.path.isfile(os.path.join(root, 'result', 'dec', 'char_lm_best.cpt'))
    sd = torch.load(os.path.join(root, 'result', 'dec', 'char_lm.cpt'), map_location='cpu')
    ref_layout = CharLM(50, 16)
    ref_layout.load_state_dict(sd, strict=True)
    for a, b in zip(ref_layout.parameters(), t.lm.parameters()):
        assert torch.equal(a, b.detach().cpu())
    assert isinstance(t.generate(length=5), str)
    # ASRTester picks the file up
    fx = np.load(os.path.join(GOLDEN, 'dataset_ref.npz'), allow_pickle=False)
    dims = [int(v) for v in fx['cpt_dims']]
    index, _ = make_corpus(root, n=2, t_max=40, feat=dims[4], seed=5)
    shutil.copy(os.path.join(GOLDEN, 'ref_small_asr.cpt'), os.path.join(root, 'result', 'dec', 'asr.cpt'))
    config['asr'] = {'mdl': {'encoder_state_size': dims[1], 'decoder_state_size': dims[2], 'mlp_out_size': dims[3],
                             'feature_dim': dims[4], 'tf_rate': 1.0},
                     'test_index': index, 'decode_lm_weight': 0.5, 'decode_beam_size': 1, 'decode_jobs': 1,
                     'max_decode_step_ratio': 0.25, 'loader_jobs': 0}
    tester = trainer.ASRTester(config, paras)
    tester.load_data()
    tester.set_model()
    for a, b in zip(tester.lm.parameters(), t.lm.parameters()):
        assert torch.equal(a, b)
