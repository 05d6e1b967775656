"""CPU-only checks of the CharLM training surface: LMDataset against what the reference's returned
(tests/golden/charlm_dataset.npz, written by tools/make_charlm_golden.py), the resident loader's chunk set, the
names the reference's CLI resolves, the new C prototypes, and the refusals (non-Adam optimizer, CPU tensors)."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_host_cpu import _ctypes_class, header_prototypes

TEXT = os.path.join(GOLDEN, 'charlm_dataset.txt')


def _fx():
    return np.load(os.path.join(GOLDEN, 'charlm_dataset.npz'), allow_pickle=False)


def test_lmdataset_matches_the_reference():
    from ss_asr_amd.LMDataset import LMDataset, load_lm_dataset
    fx = _fx()
    chunk = int(fx['chunk_size'])
    ds = LMDataset(TEXT, chunk)
    ds.device = torch.device('cpu')
    assert ds.file == str(fx['text']) and ds.chars == str(fx['chars'])
    assert len(ds) == int(fx['length']) and ds.get_num_chars() == int(fx['num_chars']) == 50
    for tag, i in (('first', 0), ('last', len(ds) - 1)):
        (sx, sy), (x, y) = ds[i]
        assert sx == str(fx[tag + '_sx']) and sy == str(fx[tag + '_sy'])
        assert x.dtype == torch.float32 and np.array_equal(x.numpy(), fx[tag + '_x'])
        assert y.dtype == torch.float32 and np.array_equal(y.numpy(), fx[tag + '_y'])
    probe = str(fx['probe'])
    assert np.array_equal(ds.s2l(probe).numpy(), fx['probe_s2l'])
    assert np.array_equal(ds.s2oh(probe).numpy(), fx['probe_s2oh'])
    assert np.array_equal(LMDataset(TEXT, chunk, label_format=True).s2oh(probe).numpy(), fx['probe_s2l'])
    with pytest.raises(KeyError):
        ds.s2l('abc#')
    with pytest.raises(AssertionError):
        ds.s2l(['a'])
    _, dl = load_lm_dataset(TEXT, chunk, 4, shuffle=False)
    assert len(dl) == int(fx['batches_drop_last'])
    assert dl.drop_last and dl.batch_size == 4


def test_resident_loader_yields_the_reference_chunk_set(tmp_path):
    from ss_asr_amd.LMDataset import LMDataset, ResidentLMLoader
    fx = _fx()
    chunk = int(fx['chunk_size'])
    ds = LMDataset(TEXT, chunk)
    for shuffle in (False, True):
        torch.manual_seed(0)
        loader = ResidentLMLoader(ds, 4, shuffle=shuffle, device='cpu')
        assert len(loader) == int(fx['batches_drop_last'])
        ys = [y for (_, (_, y)) in loader]
        assert all(y.shape == (4, chunk) and y.dtype == torch.int64 for y in ys)
        got = torch.cat(ys).numpy()
        want = fx['all_y']
        if not shuffle:
            assert np.array_equal(got, want[:len(got)])         # drop_last: the tail that fills no batch is left out
        rows = {r.tobytes() for r in want.astype(np.int64)}
        assert all(r.tobytes() in rows for r in got) and len(got) == 4 * len(loader)
    bad = tmp_path / 'bad.txt'
    bad.write_text('abc#def ghi jkl mno')
    with pytest.raises(KeyError):
        ResidentLMLoader(LMDataset(str(bad), 4), 2, device='cpu')


def test_trainer_names_resolve_through_flat():
    import importlib
    import sys
    saved = {n: sys.modules.get(n) for n in ('trainer', 'LMDataset')}
    try:
        from ss_asr_amd import flat
        flat.install()
        trainer = importlib.import_module('trainer')
        assert trainer.LMTrainer is trainer.CHARLMTrainer and issubclass(trainer.CHARLMTrainer, trainer.Solver)
        for method in ('load_data', 'set_model', 'exec', 'generate', 'close'):
            assert callable(getattr(trainer.CHARLMTrainer, method))
        lmds = importlib.import_module('LMDataset')
        assert lmds.LMDataset is importlib.import_module('ss_asr_amd.LMDataset').LMDataset
        assert callable(lmds.load_lm_dataset)
    finally:
        for n, m in saved.items():
            if m is None:
                sys.modules.pop(n, None)
            else:
                sys.modules[n] = m


def test_training_prototypes_match_the_ctypes_table():
    from ss_asr_amd import _lib, ops
    protos, _ = header_prototypes()
    names = ('ssasr_charlm_train_ws_floats', 'ssasr_charlm_train_fwd', 'ssasr_charlm_train_bwd')
    for name in names:
        res, args = _lib.SIGNATURES[name]
        assert (_ctypes_class(res), [_ctypes_class(a) for a in args]) == protos[name], name
    lib = _lib.load()
    assert lib.ssasr_abi_version() == 16
    # the size query and the Python mirror of the layout agree; unsupported shapes give 0 / a negative code
    for B, U, H, V in ((1, 1, 16, 50), (17, 4, 16, 50), (128, 200, 128, 50), (3, 5, 256, 64)):
        assert int(lib.ssasr_charlm_train_ws_floats(B, U, H, V)) == ops.charlm_ws_layout(B, U, H, V)['total'] > 0
    for B, U, H, V in ((0, 1, 16, 50), (1, 0, 16, 50), (1, 1, 8, 50), (1, 1, 24, 50), (1, 1, 272, 50), (1, 1, 16, 65)):
        assert int(lib.ssasr_charlm_train_ws_floats(B, U, H, V)) == 0
    bad = _lib.CharLM(50, 24)
    assert lib.ssasr_charlm_train_fwd(ctypes.byref(bad), None, None, None, None, 1, 1, None, None, None, None, None) < 0
    assert lib.ssasr_charlm_train_bwd(ctypes.byref(bad), None, 1, 1, 1.0, None, None) < 0
    assert lib.ssasr_charlm_train_fwd(ctypes.byref(_lib.CharLM(50, 16)), None, None, None, None, 1, 1, None, None, None,
                                      None, None) < 0                      # NULL parameters


def _trainer(tmp_path, opt_type='Adam', lr=0.002):
    from ss_asr_amd import trainer
    root = str(tmp_path)
    config = {'char_lm': {'opt': {'type': opt_type, 'learning_rate': lr}, 'mdl': {'hidden_size': 16, 'tf_rate': 0.75},
                          'train_index': TEXT, 'chunk_size': 8, 'train_batch_size': 4, 'n_epochs': 1,
                          'valid_step': 7, 'logging_step': 3, 'save_step': 5}}
    paras = types.SimpleNamespace(name='lm', logdir=os.path.join(root, 'runs'), ckpdir=os.path.join(root, 'result'),
                                  verbose=False, seed=1)
    return trainer.CHARLMTrainer(config, paras)


def test_yaml_keys_are_read(tmp_path):
    t = _trainer(tmp_path)
    assert t.module_id == 'char_lm' and t.ckppath.endswith(os.path.join('lm', 'char_lm.cpt'))
    assert t.best_ckppath.endswith('char_lm_best.cpt')
    assert (t.valid_step, t.logging_step, t.save_step, t.n_epochs, t.train_batch_size) == (7, 3, 5, 1, 4)
    t.load_data()
    assert (t.chunk_size, t.tf_rate) == (8, 0.75) and t.ds.get_num_chars() == 50
    assert len(t.train_set) == int(_fx()['batches_drop_last'])


def test_a_non_adam_optimizer_raises(tmp_path):
    from ss_asr_amd.charlm import CharLM
    from ss_asr_amd.engine import CharLMTrainStep
    t = _trainer(tmp_path, opt_type='Adadelta')
    t.load_data()
    with pytest.raises(NotImplementedError, match='char_lm.opt.type'):
        t.set_model()
    with pytest.raises(NotImplementedError, match='char_lm.opt.type'):
        CharLMTrainStep(CharLM(50, 16), 0.9, opt_type='SGD')


def test_cpu_tensors_are_refused(tmp_path):
    from ss_asr_amd import ops
    from ss_asr_amd.charlm import CharLM
    from ss_asr_amd.engine import CharLMTrainStep
    lm = CharLM(50, 16)
    with pytest.raises(RuntimeError, match='no CPU path'):
        CharLMTrainStep(lm, 0.9)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.charlm_chunk(lm, torch.zeros(2, 3, dtype=torch.int64))
