"""Builds libssasr_hip.so (gfx950 only) in-tree with hipcc.

``python -m ss_asr_amd.build`` or ``ss_asr_amd.build.build()``.  The shared
object is git-ignored but travels with the source snapshot to the GPU box.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
LIB = os.path.join(HERE, 'libssasr_hip.so')
SOURCES = ['gemm.hip', 'rnn.hip', 'decoder.hip', 'loss_opt.hip', 'ctc.hip', 'frontend.hip', 'seed.hip', 'sae.hip', 'infer.hip', 'charlm_train.hip',
           'options.hip', 'score.hip', 'mwer.hip', 'mbr.hip', 'rescore.hip', 'segment.hip']
HEADERS = ['common.h', 'rnn_kernels.h', 'attn_kernels.h', 'decoder_persistent.h', 'decoder_long.h',
           'decoder_bwd_persistent.h', 'edit_dp.h', 'seq_logp.h', 'ctc_prefix.h',
           os.path.join('..', '..', 'include', 'ssasr.h')]
FLAGS = ['-O3', '--offload-arch=gfx950', '-fPIC', '-std=c++17', '-Wno-pass-failed']


def _hipcc():
    for cand in (os.environ.get('HIPCC'), '/opt/rocm/bin/hipcc', 'hipcc'):
        if cand and (os.path.isabs(cand) and os.path.exists(cand) or not os.path.isabs(cand)):
            return cand
    raise RuntimeError('hipcc not found')


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps if os.path.exists(d))


def build(force=False, verbose=False):
    hipcc = _hipcc()
    hdrs = [os.path.join(CSRC, h) for h in HEADERS]
    srcs = [s for s in SOURCES if os.path.exists(os.path.join(CSRC, s))]
    objs = []
    jobs = []
    for s in srcs:
        src = os.path.join(CSRC, s)
        obj = os.path.join(CSRC, s.replace('.hip', '.o'))
        objs.append(obj)
        if force or _stale(obj, [src] + hdrs):
            jobs.append([hipcc] + FLAGS + ['-c', src, '-o', obj])

    def run(cmd):
        if verbose:
            print(' '.join(cmd), flush=True)
        res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if res.returncode != 0:
            raise RuntimeError('hipcc failed:\n%s\n%s' % (' '.join(cmd), res.stdout))
        return res.stdout

    with ThreadPoolExecutor(max_workers=4) as ex:
        list(ex.map(run, jobs))
    if force or jobs or _stale(LIB, objs):
        run([hipcc, '--offload-arch=gfx950', '-shared', '-fPIC', '-o', LIB] + objs)
    return LIB


if __name__ == '__main__':
    print(build(force='--force' in sys.argv, verbose=True))
