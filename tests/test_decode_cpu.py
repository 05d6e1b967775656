"""CPU-only checks of the inference surface: CharLM's state_dict is the reference's (names and shapes stored in
tests/golden/decode_*.npz by tools/make_decode_golden.py from the reference's own CharLM), the flat names
resolve, the new entry points refuse NULL arguments without a GPU, their ctypes structs equal the header's, and
the reference's train.py form drives ASRTester up to the first arithmetic."""
import glob
import os
import re
import subprocess
import sys

import numpy as np
import torch
import yaml

from conftest import GOLDEN
from test_host_cpu import ROOT, _c_class, _ctypes_class, header_prototypes, make_corpus, write_entry_script


def test_charlm_state_dict_is_the_references():
    from ss_asr_amd.charlm import CharLM
    fx = np.load(sorted(glob.glob(os.path.join(GOLDEN, 'decode_*.npz')))[0], allow_pickle=False)
    sd = CharLM(50, 128).state_dict()
    assert list(sd.keys()) == [str(n) for n in fx['charlm_names']]
    for v, shape in zip(sd.values(), fx['charlm_shapes']):
        assert list(v.shape) == [int(s) for s in shape[:v.dim()]]
    # a state_dict of those names and shapes loads strictly
    CharLM(50, 128).load_state_dict({k: torch.zeros_like(v) for k, v in sd.items()}, strict=True)
    h1, h2 = CharLM(50, 16).init_hidden(3, torch.device('cpu'))
    assert h1.shape == h2.shape == (3, 16) and not h1.any()


def test_flat_names_resolve_charlm_and_the_tester():
    code = ("import ss_asr_amd.flat; import charlm, trainer; import ss_asr_amd.charlm as c, ss_asr_amd.trainer as t; "
            "assert charlm is c and charlm.CharLM is c.CharLM and trainer.ASRTester is t.ASRTester; print('bound')")
    res = subprocess.run([sys.executable, '-c', code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         text=True, timeout=120)
    assert res.returncode == 0 and 'bound' in res.stdout, res.stdout[-2000:]


def test_null_arguments_are_negative_and_need_no_gpu():
    import ctypes
    from ss_asr_amd import _lib
    lib = _lib.load()
    assert lib.ssasr_decode_greedy(None, None) < 0
    assert lib.ssasr_decode_greedy(ctypes.byref(_lib.Infer()), None) < 0            # all sizes zero, all pointers NULL
    d = _lib.Infer()
    d.N, d.T, d.E, d.A, d.D, d.V, d.max_steps = 1, 5, 64, 16, 32, 50, 200           # sizes fine, pointers NULL
    assert lib.ssasr_decode_greedy(ctypes.byref(d), None) < 0
    d.V = 65                                                                        # a score row is one wave
    assert lib.ssasr_decode_greedy(ctypes.byref(d), None) < 0
    assert lib.ssasr_charlm_step(None, None, None, None, 0, None, None, None, None) < 0
    assert lib.ssasr_charlm_step(ctypes.byref(_lib.CharLM()), None, None, None, 1, None, None, None, None) < 0


def test_ctypes_structs_equal_the_header():
    """The method of test_library_exports_every_declared_symbol, for the two structs of the inference entries."""
    from ss_asr_amd import _lib
    protos, header = header_prototypes()
    assert {'ssasr_decode_greedy', 'ssasr_charlm_step'} <= set(protos) & set(_lib.SIGNATURES)
    for cname, cls in (('ssasr_charlm', _lib.CharLM), ('ssasr_infer', _lib.Infer)):
        body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (cname, cname), header, re.S).group(1)
        fields = []
        for decl in body.split(';'):
            decl = decl.strip()
            if decl:
                names = re.sub(r'^(const\s+)?\w+\s*\**', '', decl, count=1).split(',')
                fields += [(f.strip().lstrip('*').strip(), _c_class(decl)) for f in names]
        assert fields == [(f[0], _ctypes_class(f[1])) for f in cls._fields_], cname


def test_the_reference_entry_point_drives_asr_tester(tmp_path):
    """`python -m ss_asr_amd.run_reference <reference>/src/train.py ASRTester ...` (src/train.py:66-71): construction,
    load_data and set_model run anywhere; exec() stops at the first arithmetic without a GPU."""
    root = str(tmp_path)
    entry = write_entry_script(root)
    index, _ = make_corpus(root, n=3, t_max=24, feat=80, seed=2)
    conf = {'asr': {'mdl': {'encoder_state_size': 32, 'mlp_out_size': 16, 'decoder_state_size': 32, 'tf_rate': 0.9,
                            'feature_dim': 80},
                    'test_index': index, 'decode_lm_weight': 0.5, 'decode_beam_size': 20, 'decode_jobs': 8,
                    'max_decode_step_ratio': 0.25, 'loader_jobs': 0},
            'char_lm': {'mdl': {'hidden_size': 16}}}
    conf_path = os.path.join(root, 'conf.yaml')
    with open(conf_path, 'w') as f:
        yaml.safe_dump(conf, f)
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE='1')
    env.pop('PYTHONPATH', None)
    res = subprocess.run([sys.executable, '-m', 'ss_asr_amd.run_reference', entry, 'ASRTester', 'dec', conf_path,
                          os.path.join(root, 'runs'), os.path.join(root, 'result')], cwd=ROOT, env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    out = res.stdout
    assert 'ModuleNotFoundError' not in out and 'ImportError' not in out, out[-2000:]
    assert 'Start decoding' in out and 'No language model found' in out, out[-2000:]
    if torch.cuda.is_available():
        assert res.returncode == 0, out[-2000:]
    else:
        assert res.returncode != 0 and 'no CPU path' in out, out[-2000:]
    assert os.path.isdir(os.path.join(root, 'result', 'dec'))
