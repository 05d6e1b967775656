"""SpecAugment inside batch assembly (ssasr_gather_batch_aug) on the GPU: exact equality with a numpy
gather-and-mask built from the planned masks (the plan itself is pinned against the header's generator in
tests/test_specaug_cpu.py), on the float4, scalar and unaligned paths; the masks-off and loader-off paths are
today's bits; an utterance's masks do not depend on its batch or slot; the loader redraws them every epoch."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T = 40
LENS = (40, 8, 5, 2, 1)
FILL = -7.5            # data ~ N(0, 1), padding 0: masked cells, zero padding and data are three distinct values


def dev():
    return torch.device('cuda:0')


_corpora = {}


def corpus(F, B):
    """B utterances with lengths cycling through LENS, back to back: (frames [rows, F] float32, offsets, lens)."""
    if (F, B) not in _corpora:
        lens = np.asarray([LENS[i % len(LENS)] for i in range(B)], dtype=np.int32)
        offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
        frames = np.random.default_rng(100 * F + B).standard_normal((int(lens.sum()), F)).astype(np.float32)
        assert not (frames == 0).any() and not (frames == FILL).any()
        _corpora[(F, B)] = (frames, offs, lens)
    return _corpora[(F, B)]


def spec_of(**kw):
    from ss_asr_amd import ops
    d = dict(n_freq=2, max_freq=27, n_time=2, max_time=12, time_ratio=1.0, fill=FILL, seed=2019)
    d.update(kw)
    return ops.specaug_params(d, epoch=d.pop('epoch', 0))


def reference(frames, offs, lens, ids, F, spec):
    """numpy gather-and-mask from the planned masks; also returns every utterance's plan."""
    from ss_asr_amd import ops
    out = np.zeros((len(lens), T, F), dtype=np.float32)
    plans = []
    for b, n in enumerate(lens):
        n = int(n)
        out[b, :n] = frames[offs[b]:offs[b] + n]
        plan = ops.specaug_plan(spec, int(ids[b]), n, F)
        plans.append(plan)
        for j, (s, w) in enumerate(plan):
            if j < spec.n_freq:
                out[b, :n, s:s + w] = spec.fill
            else:
                assert s + w <= n
                out[b, s:s + w, :] = spec.fill
    return out, plans


def run(frames, offs, lens, ids, spec, out=None):
    from ss_asr_amd import ops
    d = dev()
    return ops.gather_batch_aug(torch.from_numpy(frames).to(d), torch.from_numpy(offs).to(d),
                                torch.from_numpy(lens).to(d), torch.from_numpy(np.asarray(ids, dtype=np.int32)).to(d),
                                T, spec, out=out)


def same_bits(got, want):
    return np.array_equal(got.cpu().numpy().view(np.int32), np.ascontiguousarray(want).view(np.int32))


CASES = {
    'float4_F80_B33': dict(F=80, B=33),
    'scalar_F13_B33_max_freq_F': dict(F=13, B=33, max_freq=13, n_freq=1),
    'float4_F80_B1': dict(F=80, B=1),
    'scalar_F13_B1': dict(F=13, B=1, max_freq=5),
    'unaligned_out_F80_B33': dict(F=80, B=33, unaligned=True),
    'unaligned_out_F80_B1': dict(F=80, B=1, unaligned=True),
    'eight_and_eight_F80_B33': dict(F=80, B=33, n_freq=8, n_time=8, max_freq=6, max_time=3),
    'eight_and_eight_F13_B33': dict(F=13, B=33, n_freq=8, n_time=8, max_freq=2, max_time=3),
    'max_freq_F_F80_B33': dict(F=80, B=33, max_freq=80, n_freq=1, n_time=1),
    'frequency_only_F80_B33': dict(F=80, B=33, n_time=0),
    'time_only_capped_F80_B33': dict(F=80, B=33, n_freq=0, time_ratio=0.5, max_time=7),
    'float4_F272_two_trips_B5': dict(F=272, B=5, max_freq=100, n_freq=3),
}


@pytest.mark.parametrize('name', sorted(CASES))
def test_gather_batch_aug_equals_the_numpy_gather_and_mask(name):
    case = dict(CASES[name])
    F, B, unaligned = case.pop('F'), case.pop('B'), case.pop('unaligned', False)
    frames, offs, lens = corpus(F, B)
    ids = 1000 + 7 * np.arange(B)
    spec = spec_of(**case)
    want, plans = reference(frames, offs, lens, ids, F, spec)
    out = None
    if unaligned:
        buf = torch.full((B * T * F + 8,), 123.0, device=dev())
        out = buf[1:1 + B * T * F].view(B, T, F)                    # one float past a 16-byte boundary
        assert out.data_ptr() % 16 == 4
    got = run(frames, offs, lens, ids, spec, out=out)
    assert same_bits(got, want)
    if unaligned:
        assert float(buf[0]) == 123.0 and bool((buf[1 + B * T * F:] == 123.0).all())       # nothing outside the view
    # the case holds what it is there for: the three values, and masks that overlap where it asks for them
    if B > 1:
        live = np.arange(T)[None, :, None] < lens[:, None, None]
        assert (want[np.broadcast_to(live, want.shape)] == FILL).any()
        assert (want[np.broadcast_to(live, want.shape)] != FILL).any()
        assert (want[np.broadcast_to(~live, want.shape)] == 0).all()
    if name.startswith('eight_and_eight'):
        def overlaps(masks):
            return any(a[1] > 0 and b[1] > 0 and a[0] < b[0] + b[1] and b[0] < a[0] + a[1]
                       for i, a in enumerate(masks) for b in masks[i + 1:])
        assert any(overlaps(p[:8]) for p in plans) and any(overlaps(p[8:]) for p in plans)
    if case.get('max_freq') == F:
        assert max(w for p in plans for (s, w) in p[:spec.n_freq]) > F // 2


def test_two_overlapping_masks():
    """Two frequency masks and two time masks that overlap: searched for among the epochs, then gathered."""
    F, B = 80, 5
    frames, offs, lens = corpus(F, B)
    ids = np.arange(B)
    from ss_asr_amd import ops
    for epoch in range(4096):
        spec = spec_of(epoch=epoch)
        (fa, fb, ta, tb) = ops.specaug_plan(spec, 0, 40, F)
        if (min(fa[1], fb[1], ta[1], tb[1]) > 1 and fa[0] < fb[0] < fa[0] + fa[1] < fb[0] + fb[1]
                and ta[0] < tb[0] < ta[0] + ta[1] < tb[0] + tb[1]):
            break
    else:
        raise AssertionError('no epoch with overlapping masks')
    want, _ = reference(frames, offs, lens, ids, F, spec)
    assert (want[0, ta[0]:tb[0] + tb[1]] == FILL).all() and (want[0, :, fa[0]:fb[0] + fb[1]] == FILL).all()
    assert same_bits(run(frames, offs, lens, ids, spec), want)


@pytest.mark.parametrize('F', [80, 13])
def test_masks_off_is_gather_batch_bit_for_bit(F):
    from ss_asr_amd import ops
    frames, offs, lens = corpus(F, 33)
    d = dev()
    plain = ops.gather_batch(torch.from_numpy(frames).to(d), torch.from_numpy(offs).to(d), torch.from_numpy(lens).to(d), T)
    off = run(frames, offs, lens, np.arange(33), spec_of(n_freq=0, n_time=0, max_freq=F))
    assert torch.equal(plain.view(torch.int32), off.view(torch.int32))
    # masks of width 0 change nothing either (the augmented kernel itself)
    zero = run(frames, offs, lens, np.arange(33), spec_of(max_freq=0, max_time=0))
    assert torch.equal(plain.view(torch.int32), zero.view(torch.int32))


def test_an_utterances_masks_do_not_depend_on_its_batch_or_slot():
    F = 80
    frames, offs, lens = corpus(F, 33)
    spec = spec_of(n_freq=3, n_time=3)
    u = 10                                                   # length 40
    alone = run(frames, offs[u:u + 1], lens[u:u + 1], [u], spec)
    first = run(frames, offs[[u, 1, 2, 3]], lens[[u, 1, 2, 3]], [u, 1, 2, 3], spec)
    sixth = run(frames, offs[[0, 5, 6, 7, 8, u, 11]], lens[[0, 5, 6, 7, 8, u, 11]], [0, 5, 6, 7, 8, u, 11], spec)
    assert (alone == FILL).any() and (alone != FILL).any()
    assert torch.equal(alone[0], first[0]) and torch.equal(alone[0], sixth[5])
    other = run(frames, offs[u:u + 1], lens[u:u + 1], [u + 1], spec)          # another id: other masks
    assert not torch.equal(alone, other)


def test_the_loader_redraws_the_masks_every_epoch_and_is_unchanged_without_them():
    from ss_asr_amd import ops
    from ss_asr_amd.gpu_loader import GpuResidentLoader
    F, bs = 80, 4
    rng = np.random.default_rng(5)
    lens = [37, 30, 22, 16, 12, 9, 5, 3, 2]                                   # two whole batches of 4
    utts = [rng.standard_normal((n, F)).astype(np.float32) for n in lens]
    labels = [[1] + [int(c) for c in rng.integers(3, 30, size=2 + k % 3)] + [2] for k in range(len(lens))]
    conf = dict(n_freq=2, max_freq=27, n_time=2, max_time=10, time_ratio=0.5, fill=FILL, seed=3)
    plain = GpuResidentLoader.from_arrays(utts, labels, bs, dev())
    a = GpuResidentLoader.from_arrays(utts, labels, bs, dev(), spec_augment=conf)
    b = GpuResidentLoader.from_arrays(utts, labels, bs, dev(), spec_augment=dict(conf))
    other_seed = GpuResidentLoader.from_arrays(utts, labels, bs, dev(), spec_augment=dict(conf, seed=4))
    assert plain.spec_augment is None and a.spec_augment.time_permille == 500
    base = list(plain)
    a0, a1, b0, b1, s0 = list(a), list(a), list(b), list(b), list(other_seed)
    assert len(base) == len(a0) == 2 and (a.epoch, b.epoch, plain.epoch) == (1, 1, 0)
    for k in range(2):
        for it in (a0, a1, b0, s0):                          # x_lens and labels are untouched
            assert it[k][0] == base[k][0] and it[k][2] == base[k][2] and it[k][4] == base[k][4]
            assert torch.equal(it[k][3], base[k][3])
        assert torch.equal(a0[k][1], b0[k][1]) and torch.equal(a1[k][1], b1[k][1])      # same epoch and seed
        assert not torch.equal(a0[k][1], a1[k][1])                                       # the next epoch
        assert not torch.equal(a0[k][1], s0[k][1]) and not torch.equal(a0[k][1], base[k][1])
        # today's output without the argument, bit for bit
        s = plain.starts[k]
        want = ops.gather_batch(plain.frames, plain.offsets[s:s + bs], plain.lens_dev[s:s + bs], base[k][1].shape[1])
        assert torch.equal(base[k][1].view(torch.int32), want.view(torch.int32))
        # the ids are the utterances' indices in the corpus
        for e, it in ((0, a0), (1, a1)):
            x = it[k][1].cpu().numpy()
            for i in range(bs):
                n = lens[s + i]
                ref = np.zeros(x.shape[1:], dtype=np.float32)
                ref[:n] = utts[s + i]
                spec = ops.specaug_params(conf, epoch=e)
                for j, (st, w) in enumerate(ops.specaug_plan(spec, s + i, n, F)):
                    if j < 2:
                        ref[:n, st:st + w] = FILL
                    else:
                        ref[st:st + w] = FILL
                assert np.array_equal(x[i], ref), (e, k, i)
    a.set_epoch(0)                                            # resuming: the pass after set_epoch(e) is epoch e
    again = list(a)
    assert a.epoch == 0 and all(torch.equal(again[k][1], a0[k][1]) for k in range(2))
    with pytest.raises(ValueError, match='spec_augment'):
        GpuResidentLoader.from_arrays(utts, labels, bs, dev(), spec_augment=dict(conf, max_freq=F + 1))
