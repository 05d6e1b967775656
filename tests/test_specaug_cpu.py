"""CPU-only checks of SpecAugment in batch assembly and label smoothing in the CE loss: the host plan function
(the code the kernel runs) equals a numpy restatement of the generator include/ssasr.h writes out, its draws stay
in range and cover their range, the counters change the plan, argument errors are negative before any GPU work,
the four entries are declared and bound under ABI 16, and ASRTrainer validates its two keys."""
import ctypes
import math

import numpy as np
import pytest

from test_host_cpu import header_prototypes

EARG = -1
M32 = np.uint64(0xFFFFFFFF)


def _mix(x):
    """The header's finaliser on uint64 arrays holding 32-bit values."""
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7feb352d)) & M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846ca68b)) & M32
    return x ^ (x >> np.uint64(16))


def numpy_plan(spec, utt_ids, length, F):
    """int64 [len(utt_ids), n_freq + n_time, 2] = (start, width): include/ssasr.h restated, unsigned integers only."""
    seed, epoch = np.uint64(spec['seed']), np.uint64(spec['epoch'])
    h = _mix((seed & M32) ^ np.uint64(0x9e3779b9))
    h = _mix(h ^ (seed >> np.uint64(32)))
    h = _mix(h ^ (epoch & M32))
    h = _mix(h ^ (epoch >> np.uint64(32)))
    hu = _mix(h ^ (np.asarray(utt_ids, dtype=np.int64).astype(np.uint64) & M32))

    def draw(k, n):
        return (_mix(hu ^ np.uint64(k)) * np.asarray(n, dtype=np.uint64)) >> np.uint64(32)

    cap = min(spec['max_time'], length * spec['time_permille'] // 1000)
    out = np.zeros((len(utt_ids), spec['n_freq'] + spec['n_time'], 2), dtype=np.int64)
    for j in range(spec['n_freq'] + spec['n_time']):
        limit, extent = (spec['max_freq'], F) if j < spec['n_freq'] else (cap, length)
        w = draw(2 * j, limit + 1)
        out[:, j, 1] = w
        out[:, j, 0] = draw(2 * j + 1, np.uint64(extent + 1) - w)
    return out


def _spec(**kw):
    d = dict(n_freq=2, max_freq=27, n_time=2, max_time=40, time_permille=200, fill=0.0, seed=2019, epoch=0)
    d.update(kw)
    return d


def _struct(d):
    from ss_asr_amd import _lib
    return _lib.SpecAug(d['n_freq'], d['max_freq'], d['n_time'], d['max_time'], d['time_permille'], d['fill'],
                        d['seed'], d['epoch'])


def lib_plan(d, utt_ids, length, F):
    from ss_asr_amd import _lib
    lib = _lib.load()
    s = _struct(d)
    n = d['n_freq'] + d['n_time']
    out = np.zeros((len(utt_ids), n, 2), dtype=np.int64)
    masks = (ctypes.c_int32 * (2 * max(n, 1)))()
    for i, u in enumerate(utt_ids):
        assert lib.ssasr_specaug_plan(ctypes.byref(s), int(u), length, F, masks) == 0
        out[i] = np.asarray(masks[:2 * n], dtype=np.int64).reshape(n, 2)
    return out


def test_the_entries_are_declared_and_bound_under_abi_16():
    from ss_asr_amd import _lib
    protos, header = header_prototypes()
    new = {'ssasr_gather_batch_aug', 'ssasr_specaug_plan', 'ssasr_ce_loss_ls_fwd', 'ssasr_ce_loss_ls_bwd'}
    assert new <= set(protos) & set(_lib.SIGNATURES)
    lib = _lib.load()
    for name in new:
        assert hasattr(lib, name), name
    assert lib.ssasr_abi_version() == 16 == _lib.ABI_VERSION            # additions: nothing older changed
    assert 'typedef struct ssasr_specaug {' in header
    assert [f[0] for f in _lib.SpecAug._fields_] == ['n_freq', 'max_freq', 'n_time', 'max_time', 'time_permille',
                                                     'fill', 'seed', 'epoch']
    assert ctypes.sizeof(_lib.SpecAug) == 40 and _lib.SpecAug.seed.offset == 24 and _lib.SpecAug.fill.offset == 20


@pytest.mark.parametrize('F', [13, 80])
@pytest.mark.parametrize('length', [1, 2, 7, 100, 3000])
def test_the_plan_equals_the_numpy_restatement_of_the_header(length, F):
    utts = [0, 1, 2, 77, 4095, 123456, 2 ** 31 - 1]
    for n_freq in (0, 1, 2, 8):
        for n_time in (0, 1, 2, 8):
            for d in (_spec(n_freq=n_freq, n_time=n_time, max_freq=min(27, F)),
                      _spec(n_freq=n_freq, n_time=n_time, max_freq=F, max_time=5000, time_permille=1000,
                            seed=2 ** 64 - 1, epoch=2 ** 33 + 5)):
                got, want = lib_plan(d, utts, length, F), numpy_plan(d, utts, length, F)
                assert got.shape == (len(utts), n_freq + n_time, 2)
                assert np.array_equal(got, want), (d, length, F)


def test_draws_stay_in_range_and_cover_it():
    F, length, ids = 80, 100, np.arange(4096)
    d = _spec()
    got = lib_plan(d, ids, length, F)
    assert np.array_equal(got, numpy_plan(d, ids, length, F))
    freq, time = got[:, :2], got[:, 2:]
    cap = min(d['max_time'], length * d['time_permille'] // 1000)
    assert cap == 20
    for m, limit, extent in ((freq, 27, F), (time, cap, length)):
        start, width = m[..., 0], m[..., 1]
        assert (width >= 0).all() and (width <= limit).all()
        assert (start >= 0).all() and (start + width <= extent).all()
    assert set(np.unique(freq[..., 1])) == set(range(28))               # every width 0 .. 27 occurs
    assert set(np.unique(time[..., 1])) == set(range(cap + 1))
    assert ((freq[..., 0] + freq[..., 1] == F) & (freq[..., 1] > 0)).any()          # a mask that ends exactly at F
    assert ((time[..., 0] + time[..., 1] == length) & (time[..., 1] > 0)).any()     # ... and one exactly at len
    assert (freq[..., 0] == 0).any() and (time[..., 0] == 0).any()
    # len = 1 at 200 permille: cap 0, width 0, start 0 or 1; len = 0 plans without faulting
    short = lib_plan(_spec(n_freq=0, n_time=8), ids[:64], 1, F)
    assert (short[..., 1] == 0).all() and (short[..., 0] >= 0).all() and (short[..., 0] <= 1).all()
    empty = lib_plan(_spec(n_freq=0, n_time=8), ids[:8], 0, F)
    assert (empty == 0).all()
    # max_freq = F: the whole axis can be masked, and never more
    full = lib_plan(_spec(n_freq=8, n_time=0, max_freq=13), ids, 50, 13)
    assert full[..., 1].max() == 13 and (full[..., 0] + full[..., 1] <= 13).all()


def test_the_counters_change_the_plan_and_equal_arguments_repeat_it():
    ids = np.arange(64)
    a = lib_plan(_spec(), ids, 100, 80)
    assert np.array_equal(a, lib_plan(_spec(), ids, 100, 80))
    assert np.array_equal(a, lib_plan(_spec(fill=-7.5), ids, 100, 80))           # the fill value is not a counter
    for other in (_spec(epoch=1), _spec(seed=2020), _spec(seed=2019 + 2 ** 32), _spec(epoch=2 ** 32)):
        assert not np.array_equal(a, lib_plan(other, ids, 100, 80)), other
    assert not np.array_equal(a[0], a[1])                                        # utterances differ
    # time masks are numbered after the frequency masks; the frequency masks do not depend on len
    assert np.array_equal(a[:, :2], lib_plan(_spec(), ids, 3000, 80)[:, :2])
    assert np.array_equal(a[:, :2], lib_plan(_spec(n_time=0), ids, 100, 80))


def test_out_of_range_arguments_are_negative_and_need_no_gpu():
    from ss_asr_amd import _lib
    lib = _lib.load()
    masks = (ctypes.c_int32 * 32)()
    buf = (ctypes.c_float * 64)()
    at = ctypes.c_void_p(ctypes.addressof(buf))
    good = _struct(_spec())
    assert lib.ssasr_specaug_plan(ctypes.byref(good), 3, 100, 80, masks) == 0
    assert lib.ssasr_specaug_plan(None, 3, 100, 80, masks) == EARG
    assert lib.ssasr_specaug_plan(ctypes.byref(good), 3, 100, 80, None) == EARG
    assert lib.ssasr_specaug_plan(ctypes.byref(good), 3, -1, 80, masks) == EARG
    assert lib.ssasr_specaug_plan(ctypes.byref(good), 3, 100, 0, masks) == EARG
    assert lib.ssasr_specaug_plan(ctypes.byref(_struct(_spec(n_freq=0, n_time=0))), 3, 100, 80, None) == 0
    bad = [_spec(n_freq=9), _spec(n_freq=-1), _spec(n_time=9), _spec(n_time=-1), _spec(max_freq=81),
           _spec(max_freq=-1), _spec(max_time=-1), _spec(time_permille=1001), _spec(time_permille=-1)]
    for d in bad:
        s = _struct(d)
        assert lib.ssasr_specaug_plan(ctypes.byref(s), 3, 100, 80, masks) == EARG, d
        # pointers that are not NULL and never dereferenced: the checks come first
        assert lib.ssasr_gather_batch_aug(at, at, at, at, 2, 8, 80, ctypes.byref(s), at, None) == EARG, d
    assert lib.ssasr_gather_batch_aug(at, at, at, at, 2, 8, 80, None, at, None) == EARG
    for args in ((None, at, at, at, 2, 8, 80), (at, None, at, at, 2, 8, 80), (at, at, None, at, 2, 8, 80),
                 (at, at, at, None, 2, 8, 80), (at, at, at, at, 0, 8, 80), (at, at, at, at, 2, 0, 80),
                 (at, at, at, at, 65536, 8, 80)):
        assert lib.ssasr_gather_batch_aug(*args, ctypes.byref(good), at, None) == EARG, args
    assert lib.ssasr_gather_batch_aug(at, at, at, at, 2, 8, 80, ctypes.byref(good), None, None) == EARG
    # with the masks off the limits are ssasr_gather_batch's own
    off = _struct(_spec(n_freq=0, n_time=0))
    assert lib.ssasr_gather_batch_aug(at, at, at, None, 0, 8, 80, ctypes.byref(off), at, None) == EARG
    # label smoothing: eps outside [0, 1) is refused before anything else is looked at
    for eps in (-0.1, 1.0, 1.5, math.nan, math.inf):
        assert lib.ssasr_ce_loss_ls_fwd(at, at, 4, 4, 1, 3, 5, eps, at, at, None) == EARG, eps
        assert lib.ssasr_ce_loss_ls_bwd(at, at, 4, at, at, 1, 3, 5, eps, at, None) == EARG, eps
    for eps in (0.0, 0.1):
        assert lib.ssasr_ce_loss_ls_fwd(None, at, 4, 4, 1, 3, 5, eps, at, at, None) == EARG
        assert lib.ssasr_ce_loss_ls_fwd(at, at, 4, 3, 1, 3, 5, eps, at, at, None) == EARG      # y_cols < U + 1
        assert lib.ssasr_ce_loss_ls_bwd(at, at, 3, at, at, 1, 3, 5, eps, at, None) == EARG     # y_ld < U + 1


def test_the_python_surface_checks_its_arguments_before_anything_runs():
    import torch
    from ss_asr_amd import ops
    logits, y = torch.zeros(1, 3, 5), torch.ones(1, 4, dtype=torch.long)
    for eps in (-0.1, 1.0, math.nan):
        with pytest.raises(ValueError, match='label_smoothing'):
            ops.masked_ce_loss(logits, y, 3, label_smoothing=eps)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.masked_ce_loss(logits, y, 3, label_smoothing=0.1)
    s = ops.specaug_params(dict(n_freq=2, max_freq=27, n_time=1, max_time=40, time_ratio=0.2, fill=-1.5, seed=7), epoch=3)
    assert (s.n_freq, s.max_freq, s.n_time, s.max_time, s.time_permille, s.fill, s.seed, s.epoch) == (
        2, 27, 1, 40, 200, -1.5, 7, 3)
    assert ops.specaug_params(dict(time_ratio=0.0625)).time_permille == 62          # round(62.5): to even
    with pytest.raises(ValueError, match='unknown'):
        ops.specaug_params(dict(freq_masks=2))
    assert ops.specaug_plan(s, 5, 100, 80) == [tuple(r) for r in numpy_plan(
        dict(n_freq=2, max_freq=27, n_time=1, max_time=40, time_permille=200, seed=7, epoch=3), [5], 100, 80)[0]]


def test_asr_trainer_validates_its_two_keys():
    from ss_asr_amd.trainer import ASRTrainer
    reg = ASRTrainer.regularisers
    assert reg({}) == (0.0, None) and reg({'mdl': {'feature_dim': 80}, 'wer_step': 5}) == (0.0, None)
    assert reg({'label_smoothing': 0}) == (0.0, None) and reg({'label_smoothing': 0.1}) == (0.1, None)
    for v in (-0.1, 1, 1.0, 2.5, math.nan, math.inf, '0.1', True, [0.1]):
        with pytest.raises(ValueError, match='label_smoothing'):
            reg({'label_smoothing': v})
    full = {'freq_masks': 2, 'freq_width': 27, 'time_masks': 2, 'time_width': 40, 'time_ratio': 0.2, 'fill': -1.0,
            'seed': 11}
    assert reg({'label_smoothing': 0.1, 'mdl': {'feature_dim': 80}, 'spec_augment': full}) == (
        0.1, dict(n_freq=2, max_freq=27, n_time=2, max_time=40, time_ratio=0.2, fill=-1.0, seed=11))
    assert reg({'spec_augment': {}}) == (0.0, dict(n_freq=0, max_freq=0, n_time=0, max_time=0, time_ratio=1.0,
                                                   fill=0.0, seed=0))
    bad = {'freq_masks': (9, -1, 1.5, '2', True), 'freq_width': (81, -1, 2.0), 'time_masks': (9, -1, None),
           'time_width': (-1, 1.5, '40'), 'time_ratio': (-0.1, 1.1, math.nan, 'x', True),
           'fill': (math.nan, math.inf, '0', False), 'seed': (-1, 2 ** 64, 1.0)}
    for key, values in bad.items():
        for v in values:
            with pytest.raises(ValueError, match='spec_augment.' + key):
                reg({'mdl': {'feature_dim': 80}, 'spec_augment': dict(full, **{key: v})})
    with pytest.raises(ValueError, match='unknown'):
        reg({'spec_augment': dict(full, time_warp=5)})
    with pytest.raises(ValueError, match='spec_augment'):
        reg({'spec_augment': [2, 27]})
