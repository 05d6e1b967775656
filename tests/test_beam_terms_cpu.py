"""CPU-only checks of the beam search's length bonus, coverage term and end detection: the new entries are exported
and bound, struct ssasr_beam_terms in ctypes equals the header's, argument errors are negative before any GPU work,
the workspace query follows the plain / CTC ones, the Python surface refuses bad values before it reaches the
encoder, and ASRTester validates its keys and builds the `decode_file` names."""
import ctypes
import math
import re

import pytest
import torch

from test_host_cpu import _c_class, _ctypes_class, header_prototypes

SIZES = (100, 512, 128, 256, 50, 128, 200)                                              # T E A D V Hl S


def test_the_entries_are_exported_and_bound():
    from ss_asr_amd import _lib
    protos, header = header_prototypes()
    assert {'ssasr_decode_beam_ex', 'ssasr_decode_beam_ex_ws_bytes'} <= set(protos) & set(_lib.SIGNATURES)
    lib = _lib.load()
    assert hasattr(lib, 'ssasr_decode_beam_ex') and hasattr(lib, 'ssasr_decode_beam_ex_ws_bytes')
    assert lib.ssasr_abi_version() == 16                      # an addition: nothing older changed
    body = re.search(r'typedef struct ssasr_beam_terms \{(.*?)\} ssasr_beam_terms;', header, re.S).group(1)
    fields = []
    for decl in body.split(';'):
        decl = decl.strip()
        if decl:
            names = re.sub(r'^(const\s+)?\w+\s*\**', '', decl, count=1).split(',')
            fields += [(f.strip().lstrip('*').strip(), _c_class(decl)) for f in names]
    assert fields == [(f[0], _ctypes_class(f[1])) for f in _lib.BeamTerms._fields_]
    assert [f[0] for f in fields] == ['length_bonus', 'coverage_weight', 'coverage_threshold', 'end_margin', 'n_steps']
    assert ctypes.sizeof(_lib.BeamTerms) == 24


def test_null_zero_and_out_of_range_arguments_are_negative_and_need_no_gpu():
    from ss_asr_amd import _lib
    lib = _lib.load()
    d, c = _lib.Beam(), _lib.CtcPrefix()

    def terms(beta=0.0, eta=0.0, tau=0.5, delta=-1.0):
        return _lib.BeamTerms(beta, eta, tau, delta, None)
    assert lib.ssasr_decode_beam_ex(None, None, None, None) < 0
    assert lib.ssasr_decode_beam_ex(ctypes.byref(d), None, None, None) < 0              # no terms
    assert lib.ssasr_decode_beam_ex(None, None, ctypes.byref(terms()), None) < 0
    assert lib.ssasr_decode_beam_ex(ctypes.byref(d), None, ctypes.byref(terms()), None) < 0        # all sizes zero
    assert lib.ssasr_decode_beam_ex(ctypes.byref(d), ctypes.byref(c), ctypes.byref(terms()), None) < 0
    d.N, d.T, d.E, d.A, d.D, d.V, d.max_steps, d.K = 1, 5, 64, 16, 32, 50, 24, 3     # sizes fine, pointers NULL
    assert lib.ssasr_decode_beam_ex(ctypes.byref(d), None, ctypes.byref(terms(beta=0.5)), None) < 0
    # out of range, in a description whose pointers are not NULL (never dereferenced: the checks come first)
    buf = (ctypes.c_float * 4096)()
    at = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    for name, _ in _lib.Beam._fields_:
        if name not in ('N', 'T', 'E', 'A', 'D', 'V', 'max_steps', 'K', 'lm', 'lm_weight', 'eos', 'ws_bytes'):
            setattr(d, name, at)
    d.eos, d.ws_bytes = 1, 1 << 40
    bad = [terms(beta=math.nan), terms(beta=math.inf), terms(eta=math.nan), terms(eta=-math.inf),
           terms(eta=0.3, tau=0.0), terms(eta=0.3, tau=-0.5), terms(eta=0.3, tau=math.nan), terms(eta=0.3, tau=math.inf),
           terms(delta=math.nan), terms(beta=0.5, delta=math.nan)]
    for t in bad:
        assert lib.ssasr_decode_beam_ex(ctypes.byref(d), None, ctypes.byref(t), None) == -1, list(
            getattr(t, f[0]) for f in t._fields_)
    # the workspace must hold the coverage block when eta != 0
    plain = lib.ssasr_decode_beam_ws_bytes(1, 3, 5, 64, 16, 32, 50, 0, 24)
    d.ws_bytes = plain
    assert lib.ssasr_decode_beam_ex(ctypes.byref(d), None, ctypes.byref(terms(eta=0.3)), None) == -1


def test_the_size_query_follows_the_plain_and_ctc_queries():
    from ss_asr_amd import _lib
    lib = _lib.load()
    for N, K in ((32, 8), (1, 1), (3, 32)):
        plain, ctc = lib.ssasr_decode_beam_ws_bytes(N, K, *SIZES), lib.ssasr_decode_beam_ctc_ws_bytes(N, K, *SIZES)
        assert lib.ssasr_decode_beam_ex_ws_bytes(N, K, *SIZES, 0, 0) == plain > 0
        assert lib.ssasr_decode_beam_ex_ws_bytes(N, K, *SIZES, 1, 0) == ctc > plain
        for flag, base in ((0, plain), (1, ctc)):
            cov = lib.ssasr_decode_beam_ex_ws_bytes(N, K, *SIZES, flag, 1)
            one = lib.ssasr_decode_beam_ex_ws_bytes(1, K, *SIZES, flag, 1)
            assert cov > base and cov % 16 == 0 and cov == N * one                      # linear in N
            # the coverage block: at most about 3 K up4(T) floats an utterance; here cum, twice
            assert cov - base == N * 4 * 2 * K * 100 <= N * 4 * 3 * K * 100
    odd = lib.ssasr_decode_beam_ex_ws_bytes(1, 3, 137, 512, 128, 256, 50, 128, 200, 0, 1)
    assert odd - lib.ssasr_decode_beam_ws_bytes(1, 3, 137, 512, 128, 256, 50, 128, 200) == 4 * 2 * 3 * 140
    for ctc in (0, 1):
        for cov in (0, 1):
            for N, K in ((0, 8), (32, 0), (32, 33)):
                assert lib.ssasr_decode_beam_ex_ws_bytes(N, K, *SIZES, ctc, cov) == 0
            assert lib.ssasr_decode_beam_ex_ws_bytes(1, 8, 16385, 512, 128, 256, 50, 128, 200, ctc, cov) == 0
            assert lib.ssasr_decode_beam_ex_ws_bytes(1, 8, 100, 512, 128, 256, 65, 128, 200, ctc, cov) == 0
            assert lib.ssasr_decode_beam_ex_ws_bytes(1, 8, 100, 510, 128, 256, 50, 128, 200, ctc, cov) == 0
    assert lib.ssasr_decode_beam_ex_ws_bytes(1, 32, 16384, 512, 128, 256, 50, 128, 200, 1, 1) > 2 ** 24


class _Mapper:
    def char_to_ind(self, c):
        return 1

    def ind_to_char(self, i):
        return '?'


def test_the_python_surface_checks_the_terms_before_anything_runs():
    from ss_asr_amd.asr import ASR
    model = ASR(50, 32, 32, 16, 12, 1.0)
    x = torch.zeros(1, 16, 12)
    bad = [('length_bonus', dict(length_bonus=math.nan)), ('length_bonus', dict(length_bonus=math.inf)),
           ('coverage_weight', dict(coverage_weight=math.nan)), ('coverage_weight', dict(coverage_weight=-math.inf)),
           ('coverage_threshold', dict(coverage_weight=0.3, coverage_threshold=0.0)),
           ('coverage_threshold', dict(coverage_weight=0.3, coverage_threshold=-1.0)),
           ('coverage_threshold', dict(coverage_weight=0.3, coverage_threshold=math.nan)),
           ('end_margin', dict(end_margin=-0.5)), ('end_margin', dict(end_margin=math.nan)),
           ('end_margin', dict(end_margin=math.inf))]
    for word, kw in bad:
        for beam in (1, 3):
            with pytest.raises(ValueError, match=word):
                model.decode(x, [16], None, _Mapper(), 0.0, beam_size=beam, **kw)
            with pytest.raises(ValueError, match=word):
                model.decode_many([x], [[16]], None, _Mapper(), 0.0, beam_size=beam, **kw)
            with pytest.raises(ValueError, match=word):
                model.decode_nbest([x], [[16]], None, _Mapper(), 0.0, beam, **kw)
    with pytest.raises(TypeError):                                  # keyword-only
        model.decode_nbest([x], [[16]], None, _Mapper(), 0.0, 3, 200, 0.0, 0.5)
    # with eta = 0 the threshold is not looked at; good values get as far as the device check
    for kw in (dict(coverage_threshold=math.nan), dict(length_bonus=0.5), dict(coverage_weight=0.2),
               dict(end_margin=0.0), dict(length_bonus=-0.5, coverage_weight=-0.1, coverage_threshold=2.0, end_margin=3)):
        with pytest.raises(RuntimeError, match='no CPU path'):
            model.decode(x, [16], None, _Mapper(), 0.0, **kw)
    assert model.last_beam is None and model.last_beam_steps is None
    assert ASR._beam_terms(0.0, 0.0, math.nan, None) is None and ASR._beam_terms(0, 0, 0.5, None) is None
    assert ASR._beam_terms(0.0, 0.0, 0.5, 0.0) == dict(length_bonus=0.0, coverage_weight=0.0, coverage_threshold=0.5,
                                                       end_margin=0.0)


def test_asr_tester_validates_its_keys_and_names_the_decode_file():
    from ss_asr_amd.trainer import ASRTester
    terms = ASRTester.decode_terms
    assert terms({}) == ({}, '') and terms({'decode_beam_size': 3, 'decode_lm_weight': 0.5}) == ({}, '')
    # absent or zero: off, no suffix; the threshold alone turns nothing on
    assert terms({'decode_length_bonus': 0, 'decode_coverage_weight': 0.0, 'decode_coverage_threshold': 0.3}) == ({}, '')
    assert terms({'decode_length_bonus': 0.5}) == ({'length_bonus': 0.5}, '_lb0.5')
    assert terms({'decode_coverage_weight': 0.2}) == ({'coverage_weight': 0.2, 'coverage_threshold': 0.5}, '_cov0.2')
    assert terms({'decode_end_margin': 0}) == ({'end_margin': 0}, '_end0')
    assert terms({'decode_length_bonus': 0.5, 'decode_coverage_weight': 0.2, 'decode_coverage_threshold': 0.4,
                  'decode_end_margin': 1.0}) == (
        {'length_bonus': 0.5, 'coverage_weight': 0.2, 'coverage_threshold': 0.4, 'end_margin': 1.0},
        '_lb0.5_cov0.2_end1.0')
    for key, values in (('decode_length_bonus', (math.nan, math.inf, '0.5', True, [1])),
                        ('decode_coverage_weight', (math.nan, -math.inf, 'x', False)),
                        ('decode_end_margin', (-0.1, math.nan, math.inf, '1', True))):
        for v in values:
            with pytest.raises(ValueError, match=key):
                terms({key: v})
    for tau in (0, -0.5, math.nan, 'a'):
        with pytest.raises(ValueError, match='decode_coverage_threshold'):
            terms({'decode_coverage_weight': 0.2, 'decode_coverage_threshold': tau})
