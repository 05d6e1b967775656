"""Generates tests/golden/decode_*.npz by RUNNING THE REAL REFERENCE's ASR.decode (src/asr.py:112-173) with its
CharLM (src/charlm.py) on CPU, imported through oracle/ref_harness.py.  Build-container tool: no test imports it,
and it needs the reference sources (SSASR_REFERENCE_SRC).

    python tools/make_decode_golden.py

A fixture holds data only: the input x, the SEEDS of the weights (las_oracle.seeded_weights for the ASR,
seeded_generic_weights for the LM; never the weights) and, for lm_weight 0 and 0.5, what the reference decoded:
the emitted character ids, their count, the `final_predict` row of every executed step and the smallest
top-1 / top-2 gap over those rows.  The score rows are captured by watching torch.argmax for the duration of the
call (decode takes three argmaxes per step: asr, lm, final); the loop is not restated.

Seeds are searched until every kept case has a smallest gap >= MIN_GAP for both weights (20 x the 5e-5 logit
parity of the project, so that an fp32 rounding difference cannot flip an argmax) and the kept cases cover:
an <EOS> stop after >= 20 steps, a stop within 5 steps, a run into the 200-step cap, and a transcript that
differs between the two weights.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
from ref_harness import import_reference  # noqa: E402
import las_oracle as lo  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden')
MIN_GAP = 1e-3
LM_WEIGHTS = (0.0, 0.5)
CAP = 200                                  # src/asr.py:128
SMALL = (50, 32, 32, 16, 12)               # output, enc H, dec H, mlp, feat: the small_* fixtures
FULL = (50, 256, 256, 128, 80)             # conf/default.yaml with feature_dim 80
# (shape name, dims, LM hidden, frames, seeds tried, cases kept at most)
SHAPES = [('small', SMALL, 16, 40, 60, 2), ('full', FULL, 128, 160, 60, 4), ('long', FULL, 128, 1100, 12, 1)]


class MapperStub:
    """char_to_ind / ind_to_char of the reference's Mapper (src/ASRDataset.py:228-262) over its vocabulary."""
    chars = lo.TOKENS + lo.ALL_CHARS

    def char_to_ind(self, c):
        return self.chars.index(c)

    def ind_to_char(self, i):
        return self.chars[i]


def ref_decode(model, lm, x, lm_weight):
    """The reference's decode with every argmax input recorded: (string, final_predict rows [steps, V])."""
    seen = []
    real = torch.argmax

    def watching(t, *a, **k):
        seen.append(t.detach().clone())
        return real(t, *a, **k)

    torch.argmax = watching
    try:
        with torch.no_grad():
            text = model.decode(x, [x.shape[1]], lm, MapperStub(), lm_weight)
    finally:
        torch.argmax = real
    assert len(seen) % 3 == 0
    return text, torch.stack([s.reshape(-1) for s in seen[2::3]]).numpy()


def run_case(asr_mod, charlm_mod, dims, hl, frames, seed):
    torch.manual_seed(0)
    model = lo.seeded_weights(asr_mod.ASR(*dims, 1.0), seed).eval()
    lm = lo.seeded_generic_weights(charlm_mod.CharLM(dims[0], hl), seed + 100).eval()
    x = torch.from_numpy(np.random.default_rng(seed + 1000).standard_normal((1, frames, dims[4])).astype(np.float32))
    out = dict(x=x.numpy(), dims=np.array(dims), lm_hidden=np.int64(hl), asr_weights_seed=np.int64(seed),
               lm_weights_seed=np.int64(seed + 100), lm_weights=np.array(LM_WEIGHTS), eos=np.int64(1),
               max_steps=np.int64(CAP))
    info = []
    for k, w in enumerate(LM_WEIGHTS):
        text, rows = ref_decode(model, lm, x, w)
        ids = rows.argmax(-1)
        stopped = ids[-1] == 1 and len(ids) <= CAP
        n = len(ids) - 1 if stopped else len(ids)
        assert text == ''.join(MapperStub.chars[i] for i in ids[:n]) and (stopped or n == CAP)
        top = np.sort(rows, -1)
        gap = float((top[:, -1] - top[:, -2]).min())
        out['w%d_chars' % k] = ids[:n].astype(np.int32)
        out['w%d_n_chars' % k] = np.int64(n)
        out['w%d_scores' % k] = rows.astype(np.float32)
        out['w%d_min_gap' % k] = np.float64(gap)
        out['w%d_text' % k] = np.array(text)
        info.append((n, stopped, gap, text))
    return out, info


def tags(info):
    t = set()
    for n, stopped, _, _ in info:
        if stopped and n >= 20:
            t.add('eos_late')
        if stopped and n <= 5:
            t.add('eos_early')
        if stopped and n == 0:
            t.add('empty')
        if not stopped:
            t.add('cap')
    if info[0][3] != info[1][3]:
        t.add('lm_changes_text')
    return t


def main():
    asr_mod = import_reference()
    import charlm as charlm_mod                  # the reference's, from the same REF_SRC
    assert os.path.abspath(charlm_mod.__file__).startswith(os.path.abspath(os.environ.get(
        'SSASR_REFERENCE_SRC', '/root/reference/src')))
    lm_sd = charlm_mod.CharLM(50, 128).state_dict()
    meta = dict(charlm_names=np.array(list(lm_sd.keys())),
                charlm_shapes=np.array([list(v.shape) + [0] * (2 - v.dim()) for v in lm_sd.values()]))
    need = {'eos_late', 'eos_early', 'cap', 'lm_changes_text'}
    covered = set()
    for name, dims, hl, frames, tries, keep_max in SHAPES:
        kept = 0
        for seed in range(tries):
            if kept >= keep_max:
                break
            out, info = run_case(asr_mod, charlm_mod, dims, hl, frames, seed)
            t = tags(info)
            ok = min(i[2] for i in info) >= MIN_GAP
            new = (t & need) - covered
            print('%-5s seed %2d  steps %3d / %3d  gap %.2e / %.2e  %s%s' % (
                name, seed, info[0][0], info[1][0], info[0][2], info[1][2], sorted(t), '' if ok else '  (gap too small)'))
            # a shape keeps the seeds that add a condition not covered yet (or its first usable seed, or an empty string)
            if not ok or not (new or kept == 0 or 'empty' in t):
                continue
            covered |= t
            kept += 1
            out.update(meta, tags=np.array(sorted(t)), min_gap_required=np.float64(MIN_GAP))
            path = os.path.join(OUT, 'decode_%s_s%d.npz' % (name, seed))
            np.savez_compressed(path, **out)
            print('  kept -> %s (%.0f KB)' % (os.path.basename(path), os.path.getsize(path) / 1024))
    assert need <= covered, 'conditions not covered: %s' % sorted(need - covered)


if __name__ == '__main__':
    main()
