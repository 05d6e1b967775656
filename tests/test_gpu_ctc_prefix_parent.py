"""The three CTC prefix beam searches (ssasr_ctc_decode, ssasr_ctc_decode_graph, ssasr_ctc_decode_lm: one frame body in
csrc/ctc_prefix.h) at NON-ZERO weights against the outputs recorded from the last build that held three separate
copies of that body (tests/golden/ctc_prefix_parent.npz, written by tools/record_ctc_prefix.py, which also makes the
inputs here).  The zero-weight tests of the three suites compare the variants with each other, that is the shared body
with itself; this one pins what the body computes: every integer output equal, every float32 score equal as bits."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

OUTPUTS = {'plain': ('chars', 'n_chars', 'scores', 'n_hyps'),
           'graph': ('chars', 'n_chars', 'scores', 'ctc_scores', 'graph_scores', 'n_hyps'),
           'lm': ('chars', 'n_chars', 'scores', 'ctc_scores', 'lm_scores', 'n_hyps', 'lm_frames')}


@pytest.fixture(scope='module')
def recorded():
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'ctc_prefix_parent.npz')) as f:
        return {name: f[name] for name in f.files}


@pytest.mark.parametrize('variant', sorted(OUTPUTS))
def test_every_output_is_the_recorded_one_bit_for_bit(recorded, variant):
    import record_ctc_prefix as rec
    keys = [c for c in rec.cases() if c[1] == variant]
    assert len(keys) == {'plain': 27, 'graph': 27, 'lm': 56}[variant]
    assert sum(len(OUTPUTS[c[1]]) for c in rec.cases()) == len(recorded)
    for key, _, T, V, K, extra in keys:
        got = rec.run_case(variant, T, V, K, extra)
        assert sorted(got) == sorted(OUTPUTS[variant]), key
        for name in OUTPUTS[variant]:
            want, have = recorded['%s/%s' % (key, name)], got[name]
            assert want.dtype == have.dtype and want.shape == have.shape, (key, name)
            if want.dtype == np.float32:
                want, have = want.view(np.int32), have.view(np.int32)
            else:
                assert want.dtype == np.int32, (key, name)
            assert np.array_equal(want, have), (key, name, np.argwhere(want != have)[:4].tolist())
