"""CPU-only checks of the beam-search surface: the new entry points are exported and bound, struct ssasr_beam in
ctypes equals the header's, argument errors are negative before any GPU work, the workspace query refuses what
the entry refuses, and the Python surface refuses a beam size outside 1..32."""
import ctypes
import re

import pytest
import torch

from test_host_cpu import _c_class, _ctypes_class, header_prototypes


def test_the_beam_entries_are_exported_and_bound():
    from ss_asr_amd import _lib
    protos, header = header_prototypes()
    assert {'ssasr_decode_beam', 'ssasr_decode_beam_ws_bytes'} <= set(protos) & set(_lib.SIGNATURES)
    lib = _lib.load()
    assert hasattr(lib, 'ssasr_decode_beam') and hasattr(lib, 'ssasr_decode_beam_ws_bytes')
    assert lib.ssasr_abi_version() == 16                      # an addition: nothing older changed
    body = re.search(r'typedef struct ssasr_beam \{(.*?)\} ssasr_beam;', header, re.S).group(1)
    fields = []
    for decl in body.split(';'):
        decl = decl.strip()
        if decl:
            names = re.sub(r'^(const\s+)?\w+\s*\**', '', decl, count=1).split(',')
            fields += [(f.strip().lstrip('*').strip(), _c_class(decl)) for f in names]
    assert fields == [(f[0], _ctypes_class(f[1])) for f in _lib.Beam._fields_]
    # the inputs of ssasr_infer, in its order
    infer = [f[0] for f in _lib.Infer._fields_ if f[0] not in ('chars', 'n_chars', 'scores', 'att')]
    beam = [f[0] for f in _lib.Beam._fields_]
    assert [f for f in beam if f in infer] == infer


def test_null_and_zero_arguments_are_negative_and_need_no_gpu():
    from ss_asr_amd import _lib
    lib = _lib.load()
    assert lib.ssasr_decode_beam(None, None) < 0
    assert lib.ssasr_decode_beam(ctypes.byref(_lib.Beam()), None) < 0               # all sizes zero, all pointers NULL
    d = _lib.Beam()
    d.N, d.T, d.E, d.A, d.D, d.V, d.max_steps, d.K = 1, 5, 64, 16, 32, 50, 24, 3     # sizes fine, pointers NULL
    assert lib.ssasr_decode_beam(ctypes.byref(d), None) < 0


def test_the_workspace_query_follows_the_limits():
    from ss_asr_amd import _lib
    lib = _lib.load()
    sizes = (5, 64, 16, 32, 50, 16, 24)                                             # T, E, A, D, V, Hl, S
    one = lib.ssasr_decode_beam_ws_bytes(1, 3, *sizes)
    assert one > 0 and one % 16 == 0
    assert lib.ssasr_decode_beam_ws_bytes(7, 3, *sizes) == 7 * one                  # a slice per utterance
    assert lib.ssasr_decode_beam_ws_bytes(1, 32, *sizes) > lib.ssasr_decode_beam_ws_bytes(1, 20, *sizes) > one
    # two state buffers of (4 D + 2 Hl) floats per hypothesis are part of it
    assert one >= 4 * 3 * 2 * (4 * 32 + 2 * 16)
    for K in (0, 33, -1):
        assert lib.ssasr_decode_beam_ws_bytes(1, K, *sizes) == 0
    assert lib.ssasr_decode_beam_ws_bytes(1, 3, 5, 64, 16, 32, 65, 16, 24) == 0     # a score row is one wave
    assert lib.ssasr_decode_beam_ws_bytes(1, 3, 5, 62, 16, 32, 50, 16, 24) == 0     # E % 4
    assert lib.ssasr_decode_beam_ws_bytes(0, 3, *sizes) == 0
    assert lib.ssasr_decode_beam_ws_bytes(1, 3, 5, 64, 16, 32, 50, 0, 24) > 0       # no language model


def test_the_python_surface_refuses_a_beam_outside_1_to_32():
    from ss_asr_amd.asr import ASR
    model = ASR(50, 32, 32, 16, 12, 1.0)
    x = torch.zeros(1, 16, 12)
    for K in (0, 33):
        with pytest.raises(ValueError, match='beam_size'):
            model.decode_nbest([x], [[16]], None, None, 0.0, K)
        with pytest.raises(ValueError, match='beam_size'):
            model.decode(x, [16], None, None, 0.0, beam_size=K)
    with pytest.raises(RuntimeError, match='no CPU path'):                          # a valid beam reaches the encoder
        model.decode(x, [16], None, None, 0.0, beam_size=3)
    assert model.last_beam is None
