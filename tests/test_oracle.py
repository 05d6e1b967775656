"""Pins oracle/las_oracle.py against the golden vectors captured from the real
reference (oracle/make_golden.py).  CPU only."""
import random

import numpy as np
import pytest
import torch

import las_oracle as lo
from conftest import fixture_att, fixture_xy

CASES = ['small_tf1', 'small_odd', 'small_padded', 'small_greedy', 'small_sampled',
         'full_b4', 'edge_b1', 'edge_short', 'full_b40', 'bench_b32_t800', 'bench_b32_median', 'long_b32_t3000']


def build(fx):
    dims = [int(v) for v in fx['dims']]
    torch.manual_seed(0)
    model = lo.OracleASR(*dims, float(fx['tf_rate']))
    ws = int(fx['weights_seed'])
    if ws >= 0:
        lo.seeded_weights(model, ws)
    else:
        sd = {k[3:]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith('w0/')}
        model.load_state_dict(sd)
    return model


def run(fx, model):
    x, y = fixture_xy(fx)
    lens = [int(v) for v in fx['lens']]
    ans_len = int(fx['ans_len'])
    s = int(fx['rng_seed'])
    random.seed(s); np.random.seed(s); torch.manual_seed(s)
    enc_len, logits, att = model(x, int(fx['decode_steps']),
                                 teacher=y if int(fx['teacher']) else None,
                                 state_len=lens)
    loss = lo.masked_ce_loss(logits[:, :ans_len], y, ans_len)
    return enc_len, logits, att, loss


@pytest.mark.parametrize('name', CASES)
def test_forward_matches_reference(golden, name):
    fx = golden(name)
    model = build(fx)
    enc_len, logits, att, loss = run(fx, model)
    assert enc_len == [int(v) for v in fx['enc_len']]
    np.testing.assert_allclose(logits.detach().numpy(), fx['logits'], atol=1e-5, rtol=0)
    np.testing.assert_allclose(fixture_att(fx, att.numpy()), fx['att'], atol=1e-6, rtol=0)
    assert abs(float(loss) - float(fx['loss'])) < 1e-5


@pytest.mark.parametrize('name', ['small_tf1', 'small_odd', 'full_b4', 'edge_b1', 'edge_short', 'full_b40'])
def test_backward_and_step_match_reference(golden, name):
    fx = golden(name)
    model = build(fx)
    optim = lo.make_optimizer(model)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    _, _, _, loss = run(fx, model)
    loss.backward()
    names = [str(n) for n in fx['param_names']]
    params = dict(model.named_parameters())
    got = np.array([params[n].grad.double().norm().item() for n in names])
    np.testing.assert_allclose(got, fx['grad_norms'], rtol=2e-4, atol=1e-7)
    norm, stepped = lo.solver_step(list(model.parameters()), optim)
    assert stepped and abs(norm - float(fx['grad_norm'])) < 1e-5
    after = model.state_dict()
    upd = np.array([(after[n] - before[n]).double().norm().item() for n in names])
    np.testing.assert_allclose(upd, fx['update_norms'], rtol=2e-4, atol=1e-7)
    if name == 'small_tf1':
        for n in names:
            np.testing.assert_allclose(after[n].numpy(), fx['w1/' + n], atol=2e-6, rtol=0)


def test_explicit_encoder_matches_reference_activations(golden):
    """The gate-by-gate restatement reproduces the reference's packed BiLSTM,
    pyramid reshape and the utterance-axis recurrence of blstm_4."""
    for name in ('small_tf1', 'small_odd', 'small_padded'):
        fx = golden(name)
        model = build(fx)
        sd = model.state_dict()
        x = torch.from_numpy(fx['x'])
        lens = [int(v) for v in fx['lens']]
        for layer in ('blstm_1', 'blstm_2', 'blstm_3'):
            w = [sd['encoder.%s.layer.%s_l0%s' % (layer, k, sfx)]
                 for sfx in ('', '_reverse')
                 for k in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')]
            x, lens = lo.pyramid_explicit(x, lens, w)
            np.testing.assert_allclose(x.numpy(), fx['act_' + layer], atol=2e-6, rtol=0)
        w = [sd['encoder.blstm_4.%s_l0%s' % (k, sfx)] for sfx in ('', '_reverse')
             for k in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')]
        out = lo.bilstm_explicit(x, None, w)     # time axis = utterance axis
        np.testing.assert_allclose(out.numpy(), fx['act_blstm_4'], atol=2e-6, rtol=0)
        assert lens == [int(v) for v in fx['enc_len']]


def test_explicit_clip_adadelta_matches_reference(golden):
    fx = golden('small_tf1')
    names = [str(n) for n in fx['param_names']]
    params = [torch.from_numpy(fx['w0/' + n]).clone() for n in names]
    grads = [torch.from_numpy(fx['g/' + n]).clone() for n in names]
    sq = [torch.zeros_like(p) for p in params]
    ad = [torch.zeros_like(p) for p in params]
    norm, stepped = lo.clip_adadelta_explicit(params, grads, sq, ad)
    assert stepped and abs(norm - float(fx['grad_norm'])) < 1e-6
    for p, n in zip(params, names):
        np.testing.assert_allclose(p.numpy(), fx['w1/' + n], atol=1e-6, rtol=0)


def test_length_recovery_helpers(golden):
    fx = golden('small_padded')
    assert lo.frame_lengths(torch.from_numpy(fx['x'])) == [int(v) for v in fx['lens']]
    y = torch.from_numpy(fx['y'])
    assert max(lo.label_lengths(y)) - 1 == int(fx['ans_len'])


@pytest.mark.slow
def test_config1_shape_b16_t400(golden):
    fx = golden('full_b16_t400')
    model = build(fx)
    enc_len, logits, att, loss = run(fx, model)
    assert enc_len == [int(v) for v in fx['enc_len']]
    assert abs(float(loss) - float(fx['loss'])) < 1e-4


@pytest.mark.parametrize('name', ['tae_full_b12', 'tae_full_b40', 'tae_small_tf05'])
def test_text_autoencoder_oracle_matches_reference(golden, name):
    """the oracle's TextAutoEncoder + TAETrainer loss against the fixture captured
    from the reference's (src/text_autoencoder.py:31-94, src/trainer.py:662-672), including the
    sampled steps of the tf_rate 0.5 case (same RNG consumption) and every gradient norm."""
    fx = golden(name)
    dims = [int(v) for v in fx['dims']]
    torch.manual_seed(0)
    asr = lo.OracleASR(*dims, float(fx['tf_rate']))
    lo.seeded_weights(asr, int(fx['asr_weights_seed']))
    tae = lo.OracleTextAutoEncoder(dims[0], *[int(v) for v in fx['tae_dims']])
    lo.seeded_tae_weights(tae, int(fx['tae_weights_seed']))
    y, y_noise = torch.from_numpy(fx['y']), torch.from_numpy(fx['y_noise'])
    s = int(fx['rng_seed'])
    random.seed(s); np.random.seed(s); torch.manual_seed(s)
    _, logits = tae(asr, y, y_noise, int(fx['decode_step']), noise_lens=[int(v) for v in fx['noise_lens']])
    np.testing.assert_allclose(logits.detach().numpy(), fx['logits'], atol=1e-5, rtol=0)
    loss = lo.tae_loss(logits, y)
    assert abs(float(loss) - float(fx['loss'])) < 1e-5
    loss.backward()
    grads = {('tae.' + k): p.grad for k, p in tae.named_parameters()}
    grads.update({('asr.' + k): p.grad for k, p in asr.named_parameters() if p.grad is not None})
    names = [str(n) for n in fx['grad_names']]
    assert sorted(grads) == names
    got = np.array([grads[k].double().norm().item() for k in names])
    np.testing.assert_allclose(got, fx['grad_norms'], rtol=2e-4, atol=1e-7)


def _seed(s):
    random.seed(s); np.random.seed(s); torch.manual_seed(s)


@pytest.mark.parametrize('name', ['tae_traj_full_b12', 'seed_alt_small'])
def test_tae_trainer_trajectory_oracle_matches_reference(golden, name):
    """Config 5's first leg as a TRAINER: the oracle's tae_train_step (src/trainer.py:652-677 + Solver.step on
    the text autoencoder's parameters, Adam over the text autoencoder and the shared ASR decoder half)
    against the trajectory captured from the reference's classes -- three steps at full layer sizes, and
    three rounds of (ASRTrainer step, TAETrainer step) alternating on ONE shared ASR object."""
    fx = golden(name)
    dims = [int(v) for v in fx['dims']]
    torch.manual_seed(0)
    asr = lo.OracleASR(*dims, float(fx['tf_rate']))
    lo.seeded_weights(asr, int(fx['asr_weights_seed']))
    tae = lo.OracleTextAutoEncoder(dims[0], *[int(v) for v in fx['tae_dims']])
    lo.seeded_tae_weights(tae, int(fx['tae_weights_seed']))
    tae_opt = lo.make_tae_optimizer(tae, asr, lr=float(fx['lr']))
    asr_opt = lo.make_optimizer(asr) if int(fx['with_asr']) else None
    w0 = {('tae.' + k): v.clone() for k, v in tae.state_dict().items()}
    w0.update({('asr.' + k): v.clone() for k, v in asr.state_dict().items()})
    for r in range(int(fx['rounds'])):
        if asr_opt is not None:
            _seed(int(fx['asr_rng_seed%d' % r]))
            loss, norm = lo.train_step(asr, asr_opt, torch.from_numpy(fx['asr_x%d' % r]), torch.from_numpy(fx['asr_y%d' % r]))
            assert abs(loss - float(fx['asr_loss'][r])) < 1e-5, (r, loss)
            assert abs(norm - float(fx['asr_norm'][r])) < 1e-5 * max(1.0, norm), (r, norm)
        _seed(int(fx['rng_seed%d' % r]))
        loss, norm = lo.tae_train_step(asr, tae, tae_opt, torch.from_numpy(fx['y%d' % r]), torch.from_numpy(fx['y_noise%d' % r]))
        assert abs(loss - float(fx['tae_loss'][r])) < 1e-5, (r, loss)
        assert abs(norm - float(fx['tae_norm'][r])) < 1e-5 * max(1.0, norm), (r, norm)
    w1 = {('tae.' + k): v for k, v in tae.state_dict().items()}
    w1.update({('asr.' + k): v for k, v in asr.state_dict().items()})
    names = [str(n) for n in fx['param_names']]
    assert sorted(w1) == names
    upd = np.array([(w1[k] - w0[k]).double().norm().item() for k in names])
    np.testing.assert_allclose(upd, fx['update_norms'], rtol=1e-4, atol=1e-9)
    for k in fx.files:
        if k.startswith('w1/'):
            np.testing.assert_allclose(w1[k[3:]].numpy(), fx[k], atol=2e-6, rtol=0, err_msg=k)
        if k.startswith('w1_head/'):
            np.testing.assert_allclose(w1[k[8:]].reshape(-1)[:256].numpy(), fx[k], atol=2e-6, rtol=0, err_msg=k)


def _check_final_weights(fx, w0, w1, atol=2e-6):
    names = [str(n) for n in fx['param_names']]
    assert sorted(w1) == names
    upd = np.array([(w1[k].double() - w0[k].double()).norm().item() for k in names])
    np.testing.assert_allclose(upd, fx['update_norms'], rtol=1e-4, atol=1e-9)
    for k in fx.files:
        if k.startswith('w1/'):
            np.testing.assert_allclose(w1[k[3:]].numpy(), fx[k], atol=atol, rtol=0, err_msg=k)
        if k.startswith('w1_head/'):
            np.testing.assert_allclose(w1[k[8:]].reshape(-1)[:256].numpy(), fx[k], atol=atol, rtol=0, err_msg=k)


@pytest.mark.parametrize('name', ['adv_traj_full_b8', 'adv_traj_small_adam'])
def test_adv_trainer_trajectory_oracle_matches_reference(golden, name):
    """Config 5's second leg: the oracle's adv_train_step (src/trainer.py:968-1032 with the undefined
    `loss_metric` as nn.BCELoss) against three iterations captured from the reference's Discriminator / Listener /
    text encoder classes -- the yaml's Adadelta pair at full layer sizes, Adam on a small model."""
    from ss_asr_amd.synthetic import make_batch
    fx = golden(name)
    assert str(fx['loss_metric']) == 'BCELoss'
    dims = [int(v) for v in fx['dims']]
    torch.manual_seed(0)
    asr = lo.OracleASR(*dims, 1.0)
    lo.seeded_weights(asr, int(fx['asr_weights_seed']))
    tae = lo.OracleTextAutoEncoder(dims[0], *[int(v) for v in fx['tae_dims']])
    lo.seeded_tae_weights(tae, int(fx['tae_weights_seed']))
    disc = lo.OracleDiscriminator(2 * dims[1], int(fx['hidden']))
    lo.seeded_generic_weights(disc, int(fx['disc_weights_seed']))
    opt = lambda a: (str(a[0]), float(a[1]))
    G, D = lo.make_adv_optimizers(asr, disc, opt(fx['g_opt']), opt(fx['d_opt']))
    w0 = {('disc.' + k): v.clone() for k, v in disc.state_dict().items()}
    w0.update({('asr.' + k): v.clone() for k, v in asr.state_dict().items()})
    for r in range(int(fx['rounds'])):
        x, y, _ = make_batch(fx['lens%d' % r], fx['ylens%d' % r], dims[4], int(fx['batch_seed%d' % r]))
        got = lo.adv_train_step(asr, tae.encoder, disc, G, D, x, y, float(fx['label_smoothing']))
        want = [float(fx[k][r]) for k in ('d_real', 'd_fake', 'g_loss', 'd_norm', 'g_norm')]
        np.testing.assert_allclose(got, want, rtol=2e-5, atol=1e-6, err_msg='round %d' % r)
    w1 = {('disc.' + k): v for k, v in disc.state_dict().items()}
    w1.update({('asr.' + k): v for k, v in asr.state_dict().items()})
    _check_final_weights(fx, w0, w1)


def _sae_from_fixture(fx, cls):
    dims = [int(v) for v in fx['dims']]
    sae = cls(2 * dims[1], dims[4], [list(map(int, k)) for k in fx['kernel_sizes']], [int(v) for v in fx['num_filters']],
              [list(map(int, k)) for k in fx['pool_kernel_sizes']])
    lo.seeded_generic_weights(sae, int(fx['sae_weights_seed']))
    return sae


@pytest.mark.parametrize('name', ['sae_traj_full_b8', 'sae_traj_small'])
def test_sae_trainer_trajectory_oracle_matches_reference(golden, name):
    """Config 5's third leg: the oracle's SpeechAutoEncoder and sae_train_step (src/trainer.py:803-820) against
    three iterations captured from the reference's classes -- losses, clipped norms (the speech autoencoder's
    alone), every final weight and batch-norm buffer of both models, and an eval-mode prediction."""
    from ss_asr_amd.synthetic import make_batch
    fx = golden(name)
    dims = [int(v) for v in fx['dims']]
    torch.manual_seed(0)
    asr = lo.OracleASR(*dims, 1.0)
    lo.seeded_weights(asr, int(fx['asr_weights_seed']))
    sae = _sae_from_fixture(fx, lo.OracleSpeechAutoEncoder)
    optim = lo.make_sae_optimizer(sae, asr, lr=float(fx['opt'][1]), kind=str(fx['opt'][0]))
    state = lambda: {**{('sae.' + k): v.clone().float() for k, v in sae.state_dict().items()},
                     **{('asr.' + k): v.clone() for k, v in asr.state_dict().items()}}
    w0 = state()
    for r in range(int(fx['rounds'])):
        lens = fx['lens%d' % r]
        x, _, _ = make_batch(lens, np.full(len(lens), 3), dims[4], int(fx['batch_seed%d' % r]), pad_to=int(fx['pad_to']))
        loss, norm = lo.sae_train_step(asr, sae, optim, x)
        assert abs(loss - float(fx['loss'][r])) < 1e-5, (r, loss)
        assert abs(norm - float(fx['norm'][r])) < 1e-5 * max(1.0, norm), (r, norm)
        if r == 0:
            with torch.no_grad():
                sae.eval()
                lis, _ = asr.encoder(x, [int(v) for v in lens])
                np.testing.assert_allclose(sae(x, lis).reshape(-1)[:512].numpy(), fx['eval_pred_head'], atol=1e-5, rtol=0)
                sae.train()
    _check_final_weights(fx, w0, state())


def test_decoder_replay_is_the_loop_of_the_pinned_forward():
    """lo.decoder_replay (the float64 decoder-only reference of tests/test_gpu_decoder_forms.py) against
    OracleASR.forward, which the fixtures above pin: fed the oracle encoder's output and teacher steps it gives
    forward's logits and attention to 1e-12; with sampled and greedy steps mixed in, forward replayed on the
    characters it fed (forced_chars) gives its logits again, every greedy pick is the argmax and every draw
    lies inside its own inverse-CDF bracket."""
    dims = (11, 8, 8, 4, 6)
    torch.manual_seed(0)
    model = lo.seeded_weights(lo.OracleASR(*dims, 1.0), 3).double()
    rng = np.random.default_rng(7)
    lens, U = [40, 33, 16], 6
    x = torch.from_numpy(rng.standard_normal((3, 40, 6)))
    for b, l in enumerate(lens):
        x[b, l:] = 0
    y = torch.from_numpy(rng.integers(1, 11, (3, U + 2)))
    y[:, 0] = 0
    with torch.no_grad():
        enc_len, logits, att = model(x, U, teacher=y, state_len=lens)
        feat, enc_len2 = model.encoder(x, lens)
        assert enc_len == enc_len2 == [5, 4, 2]
        r_logits, r_att, fed, margin = lo.decoder_replay(model, feat, enc_len, y, [0] * U)
        assert r_logits.dtype == torch.float64 and (margin == np.inf).all()
        assert torch.equal(fed, torch.cat([torch.zeros(1, 3, dtype=torch.long), y[:, 1:U + 1].t()]))
        assert float((r_logits - logits).abs().max()) <= 1e-12 and float((r_att - att).abs().max()) <= 1e-12
        assert float(r_att[1, :, 4:].abs().sum()) == 0.0 and float(r_att[2, :, 2:].abs().sum()) == 0.0

        modes = [1, 0, 2, 1, 2, 0]
        uni = rng.random((U, 3)).astype(np.float32)
        r_logits, r_att, fed, margin = lo.decoder_replay(model, feat, enc_len, y, modes, uni)
        _, logits, att = model(x, U, teacher=y, state_len=lens, forced_chars=fed)
        assert float((r_logits - logits).abs().max()) <= 1e-12 and float((r_att - att).abs().max()) <= 1e-12
        for t, mode in enumerate(modes):
            assert np.isfinite(margin[t]).all() == (mode != 0) and (margin[t] >= 0).all()
            for b in range(3):
                c = int(fed[t + 1, b])
                if mode == 0:
                    assert c == int(y[b, t + 1])
                elif mode == 2:
                    assert c == int(torch.argmax(logits[b, t]))
                    top = torch.sort(logits[b, t], descending=True).values
                    assert abs(float(top[0] - top[1]) - margin[t, b]) <= 1e-12
                else:
                    run, tot = lo.inverse_cdf_bounds(logits[b, t].numpy())
                    target = float(uni[t, b]) * tot
                    assert (float(run[c - 1]) if c else 0.0) <= target < float(run[c])
                    assert abs(np.abs(run.astype(np.float64) - target).min() / tot - margin[t, b]) <= 1e-12
    # differentiable in feat and the parameters
    f = feat.clone().requires_grad_(True)
    lo.decoder_replay(model, f, enc_len, y, modes, uni)[0].sum().backward()
    assert float(f.grad[1, 4:].abs().sum()) == 0.0 and float(f.grad[1, :4].abs().min()) > 0.0
    assert model.attention.psi.weight.grad is not None and model.encoder.blstm_1.layer.weight_hh_l0.grad is None


@pytest.mark.parametrize('lens', [[9, 8, 4, 1], [12, 9, 1, 30], None], ids=['inside', 'above_T', 'none'])
def test_attention_step_explicit_is_masked_softmax_and_bmm(lens):
    """lo.attention_step_explicit (the float64 reference of tests/test_gpu_attention_forms.py and of the
    attention cases in tests/test_gpu_kernels.py) against an independent formulation: an additive -inf mask,
    torch.softmax and torch.bmm, with autograd on both sides.  Lengths 1, T', above T' (which must act as T')
    and None (every utterance full length); frames at or past an utterance's length get alpha exactly 0 and
    carry no gradient."""
    B, T, A, E, D = 4, 9, 8, 12, 6
    g = torch.Generator().manual_seed(11)
    draw = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)       # noqa: E731
    vals = [draw(B, D), draw(B, T, E), torch.tanh(draw(B, T, A)), draw(A, D)]
    ga, gc = draw(B, T), draw(B, E)
    eff = [T] * B if lens is None else [min(int(l), T) for l in lens]

    a = [v.clone().requires_grad_(True) for v in vals]
    alpha, ctx = lo.attention_step_explicit(a[0], a[1], a[2], lens, a[3])
    ((alpha * ga).sum() + (ctx * gc).sum()).backward()

    b = [v.clone().requires_grad_(True) for v in vals]
    state, feat, comp, w_phi = b
    q = torch.tanh(torch.nn.functional.linear(state, w_phi))
    mask = torch.zeros(B, T, dtype=torch.float64)
    for i, l in enumerate(eff):
        mask[i, l:] = float('-inf')
    want_alpha = torch.softmax(torch.bmm(comp, q.unsqueeze(2)).squeeze(2) + mask, dim=1)
    want_ctx = torch.bmm(want_alpha.unsqueeze(1), feat).squeeze(1)
    ((want_alpha * ga).sum() + (want_ctx * gc).sum()).backward()

    assert alpha.dtype == torch.float64 and alpha.shape == (B, T) and ctx.shape == (B, E)
    alpha, ctx, want_alpha, want_ctx = (t.detach() for t in (alpha, ctx, want_alpha, want_ctx))
    assert float((alpha - want_alpha).abs().max()) <= 1e-14 and float((ctx - want_ctx).abs().max()) <= 1e-13
    assert float((alpha.sum(1) - 1).abs().max()) <= 1e-14
    for x, y, name in zip(a, b, ['state', 'feat', 'comp', 'w_phi']):
        assert float((x.grad - y.grad).abs().max()) <= 1e-12, name
    for i, l in enumerate(eff):
        assert float(alpha[i, l:].abs().sum()) == 0.0
        assert float(a[1].grad[i, l:].abs().sum()) == 0.0 and float(a[2].grad[i, l:].abs().sum()) == 0.0
        assert float(alpha[i, :l].min()) > 0.0
    if lens is not None and max(lens) > T:       # an entry above T' is the full-length utterance
        full, _ = lo.attention_step_explicit(vals[0], vals[1], vals[2], eff, vals[3])
        assert torch.equal(full, alpha)
