"""Every launch form of the decode loop (csrc/decoder.hip: short / long persistent forward or one launch
per stage and step; persistent backward chain of 2 / 4 / 6 frame slices or the per-step backward) at the
shape limits that select it, against the float64 decoder-only reference lo.decoder_replay
(tests/test_oracle.py ties it to the pinned OracleASR.forward): fed characters exactly, attention,
logits and EVERY gradient tensor element by element.  Widths are the production ones (A = 128, E = 512,
D = 256); only B, T', U, V and the lengths vary.  Needs an MI355X."""
import collections
import functools

import numpy as np
import pytest
import torch

import las_oracle as lo

pytestmark = pytest.mark.gpu

A, E, D = 128, 512, 256
WEIGHTS_SEED = 47
ATT_ATOL = 2e-6            # the project's tolerances for these quantities (test_gpu_model.py)
LOGITS_ATOL = 5e-5
DFEAT_ATOL = 5e-5          # the loosest values test_gpu_kernels.py uses for the same kind of quantity, through close()
DWEIGHT_ATOL = 3e-4
GREEDY_GAP = 1e-3          # precondition on the reference alone: no decision of a step that is not teacher forced
DRAW_GAP = 1e-4            # is close enough to a tie for fp32 rounding to turn it

GRADS = ['attention.psi.weight', 'attention.psi.bias', 'attention.phi.weight',
         'decoder.layer_1.weight_ih', 'decoder.layer_1.weight_hh', 'decoder.layer_1.bias_ih', 'decoder.layer_1.bias_hh',
         'decoder.layer_2.weight_ih', 'decoder.layer_2.weight_hh', 'decoder.layer_2.bias_ih', 'decoder.layer_2.bias_hh',
         'embed.weight', 'char_trans.weight', 'char_trans.bias']

# fwd: the forward form the default switches take; the backward chain is taken exactly for T' <= 384
Case = collections.namedtuple('Case', 'name B Tp U V lens modes fwd seed')
CASES = [
    Case('smallest_teacher', 1, 1, 1, 50, [1], [0], 'short', 0),                    # the chain's second slice is empty
    Case('smallest_greedy', 1, 1, 1, 50, [1], [2], 'short', 0),
    Case('one_row_slices', 3, 2, 3, 50, [2, 1, 1], [2, 0, 1], 'short', 0),          # U = depth of the exchange rings
    Case('two_steps', 5, 33, 2, 50, [33, 32, 17, 16, 1], [2, 1], 'short', 0),
    Case('odd_t_tiny_v', 17, 127, 5, 3, [127, 126, 113, 112, 111, 97, 96, 80, 65, 64, 63, 48, 33, 32, 17, 16, 1],
         [0, 1, 2, 0, 1], 'short', 0),                                              # unequal chain slices, 16-tile + 1 column
    Case('short_limits', 32, 128, 9, 64, [128, 128, 127, 124, 120, 116, 112, 108, 104, 100, 97, 96, 95, 88, 81, 80, 79, 72,
                                          66, 65, 64, 63, 56, 49, 48, 47, 33, 32, 17, 16, 2, 1],
         [0, 1, 0, 0, 2, 0, 1, 0, 0], 'short', 9),                                  # T' = 128, B = 32 and V = 64 together
    Case('v65_step_fwd_chain_bwd', 4, 40, 6, 65, [40, 39, 17, 5], [1, 0, 2, 0, 1, 2], 'step', 0),
    Case('long_first', 2, 129, 3, 50, [129, 128], [0, 1, 2], 'long', 0),            # NS = 3, 4 chain slices
    Case('chain4_last', 3, 256, 7, 50, [256, 193, 192], [0, 2, 1, 0, 1, 2, 0], 'long', 0),
    Case('chain6_first', 3, 257, 4, 50, [257, 256, 1], [1, 0, 2, 0], 'long', 0),    # NS = 5
    Case('chain_off_first', 2, 385, 4, 50, [385, 384], [0, 2, 1, 1], 'long', 0),    # NS = 7, per-step backward
    Case('ns8_192_workgroups', 24, 512, 5, 50, [512, 512, 511, 449, 448, 447, 385, 384, 383, 321, 320, 319, 257, 256, 255,
                                                193, 192, 191, 129, 128, 127, 65, 64, 1], [2, 1, 0, 1, 0], 'long', 2),
    Case('ns10_v64', 19, 640, 4, 64, [640 - 33 * k for k in range(19)], [0, 1, 2, 0], 'long', 8),     # 190 workgroups
    Case('ns12_both_limits', 16, 768, 8, 50, [768, 705, 704, 641, 640, 577, 512, 449, 384, 321, 256, 193, 128, 65, 64, 1],
         [0, 1, 2, 0, 0, 1, 0, 1], 'long', 1),
    Case('fallback_204_workgroups', 17, 768, 2, 50, [768] * 17, [1, 2], 'step', 1),
    Case('fallback_ns13', 2, 769, 2, 50, [769] * 2, [0, 1], 'step', 0),
]


def close(got, want, atol, what=''):
    got = got.detach().double().cpu()
    want = want.detach().double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = (got - want).abs().max().item()
    tol = atol * max(1.0, want.abs().max().item())     # absolute for O(1) data, relative above
    assert err <= tol, '%s: max abs err %.3e > %.1e' % (what, err, tol)


def seed_weights(model):
    """lo.seeded_weights, then small non-zero biases in the decoder half (the law leaves them at 0 and 1, which
    would hide a kernel that drops one); drawn by name, so both model classes get the same values."""
    lo.seeded_weights(model, WEIGHTS_SEED)
    rng = np.random.default_rng(WEIGHTS_SEED + 1)
    params = dict(model.named_parameters())
    with torch.no_grad():
        for name in GRADS:
            if params[name].dim() == 1:
                params[name] += torch.from_numpy((0.1 * rng.standard_normal(params[name].shape)).astype(np.float32))
    return model


@functools.lru_cache(maxsize=None)
def oracle_model(V):
    torch.manual_seed(0)
    return seed_weights(lo.OracleASR(V, 256, 256, A, 80, 0.5)).double()


@functools.lru_cache(maxsize=None)
def gpu_model(V):
    from ss_asr_amd.asr import ASR
    torch.manual_seed(0)
    return seed_weights(ASR(V, 256, 256, A, 80, 0.5)).to('cuda:0')


def inputs(case):
    """Seeded float32 inputs of a case: feat (zero past each length), labels, uniforms, upstream gradient."""
    rng = np.random.default_rng([case.seed, case.B, case.Tp, case.U, case.V])
    feat = rng.standard_normal((case.B, case.Tp, E)).astype(np.float32)
    for b, l in enumerate(case.lens):
        feat[b, l:] = 0
    teacher = rng.integers(1, case.V, (case.B, case.U + 2)).astype(np.int32)
    uniforms = rng.random((case.U, case.B), dtype=np.float32)
    dlogits = rng.standard_normal((case.B, case.U, case.V)).astype(np.float32)
    return tuple(torch.from_numpy(v) for v in (feat, teacher, uniforms, dlogits))


def reference(case):
    """The float64 replay of a case and its gradients.  Needs no device.  Asserts the precondition that makes
    an exact comparison of the fed characters sound."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    assert len(case.lens) == case.B and max(case.lens) == case.Tp and len(case.modes) == case.U
    assert case.U < 3 or set(case.modes) == {0, 1, 2}
    ref = oracle_model(case.V)
    feat, teacher, uniforms, dlogits = inputs(case)
    f = feat.double().requires_grad_(True)
    ref.zero_grad()
    logits, att, fed, margin = lo.decoder_replay(ref, f, case.lens, teacher, case.modes, uniforms.numpy())
    for t, mode in enumerate(case.modes):
        if mode:
            assert margin[t].min() >= (GREEDY_GAP if mode == 2 else DRAW_GAP), \
                '%s: step %d (mode %d) decides within %.2e: pick another seed' % (case.name, t, mode, margin[t].min())
    (logits * dlogits.double()).sum().backward()
    params = dict(ref.named_parameters())
    grads = {n: params[n].grad.clone() for n in GRADS}
    grads['feat'] = f.grad
    for b, l in enumerate(case.lens):
        assert float(f.grad[b, l:].abs().sum()) == 0.0 and float(att[b, :, l:].abs().sum()) == 0.0
    return logits.detach(), att, fed, grads


def run_gpu(case, per_step):
    """One forward + backward through ops.attn_precompute and ops.decoder_loop with the form switches at
    `per_step`; (logits, att, chars, gradients) on the host."""
    from ss_asr_amd import _lib, ops
    model = gpu_model(case.V)
    feat, teacher, uniforms, dlogits = (v.cuda() for v in inputs(case))
    enc_len = torch.tensor(case.lens, dtype=torch.int32, device='cuda')
    try:
        _lib.set_option('SSASR_NO_PERSISTENT_DECODER', per_step)
        _lib.set_option('SSASR_NO_PERSISTENT_DECODER_BWD', per_step)
        f = feat.clone().requires_grad_(True)
        model.zero_grad()
        comp = ops.attn_precompute(f, model.attention.psi.weight, model.attention.psi.bias)
        logits, att, chars = ops.decoder_loop(f, comp, enc_len, teacher, case.modes, uniforms, model._decoder_params())
        (logits * dlogits).sum().backward()
        ops.join_side_stream()
        torch.cuda.synchronize()
        ops.check_persistent_status()
    finally:
        _lib.set_option('SSASR_NO_PERSISTENT_DECODER', 0)
        _lib.set_option('SSASR_NO_PERSISTENT_DECODER_BWD', 0)
    params = dict(model.named_parameters())
    grads = {n: params[n].grad.cpu().clone() for n in GRADS}
    grads['feat'] = f.grad.cpu()
    return logits.detach().cpu(), att.cpu(), chars.cpu().long(), grads


@pytest.mark.parametrize('case', CASES, ids=[c.name for c in CASES])
def test_decode_loop_form_matches_the_float64_replay(case):
    """Both runs of a case -- the forms its shape selects, then SSASR_NO_PERSISTENT_DECODER(_BWD) = 1 -- against
    the float64 replay; which form ran is asserted, so that a silent fall-back cannot make a case vacuous."""
    from ss_asr_amd import _lib
    lib = _lib.load()
    want_logits, want_att, want_fed, want_grads = reference(case)
    part = int(lib.ssasr_decoder_fwd_part_floats(case.B, case.Tp, A, E, D, case.V))
    chain = int(lib.ssasr_decoder_bwd_chain_floats(case.U, case.B, case.Tp, A, E, D))
    assert (part > 0) == (case.fwd == 'long'), (case.fwd, part)
    assert (chain > 0) == (case.Tp <= 384), chain
    runs = {}
    failures = []
    for per_step in (0, 1):
        logits, att, chars, grads = runs[per_step] = run_gpu(case, per_step)
        tag = '%s/%s' % (case.name, 'per-step' if per_step else 'default')
        if not torch.equal(chars, want_fed):
            failures.append('%s: fed characters differ at (step, utterance) %s'
                            % (tag, (chars != want_fed).nonzero().tolist()[:8]))
        worst = {}
        for b, l in enumerate(case.lens):
            if float(att[b, :, l:].abs().sum()) != 0.0:
                failures.append('%s: utterance %d attends past its %d frames' % (tag, b, l))
        checks = [('att', att, want_att, ATT_ATOL, None), ('logits', logits, want_logits, LOGITS_ATOL, None),
                  ('dfeat', grads['feat'], want_grads['feat'], DFEAT_ATOL, close)]
        checks += [('d' + n, grads[n], want_grads[n], DWEIGHT_ATOL, close) for n in GRADS]
        for what, got, want, atol, rule in checks:
            err = float((got.double() - want).abs().max())
            scale = max(1.0, float(want.abs().max())) if rule else 1.0
            kind = what if what in ('att', 'logits', 'dfeat') else 'dweight'
            if err / scale >= worst.get(kind, (-1.0, ''))[0]:
                worst[kind] = (err / scale, what)
            try:
                if rule:
                    rule(got, want, atol, tag + ' ' + what)
                else:
                    np.testing.assert_allclose(got.numpy(), want.numpy(), atol=atol, rtol=0, err_msg=tag + ' ' + what)
            except AssertionError:
                failures.append('%s %s: max abs err %.3e > %.1e' % (tag, what, err, atol * scale))
        print('%s: max error (over max(1, |reference|max) for gradients) %s' % (
            tag, ', '.join('%s %.2e%s' % (k, v[0], ' (%s)' % v[1] if k == 'dweight' else '') for k, v in worst.items())))
    if case.fwd == 'short':
        # no query names the short form: the two forms sum in different orders, so equal bits mean it never ran
        assert not torch.equal(runs[0][0], runs[1][0]), 'the short persistent forward was not taken'
    assert not failures, '\n'.join(failures)
