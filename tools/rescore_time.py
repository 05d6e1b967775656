"""Milliseconds of the second pass of two-pass decoding (ops.rescore, csrc/rescore.hip) on tools/beam_time.py's shape:
32 utterances, T' = 100 encoder frames each, V = 50, K = 8, random weights.  Events around each piece, warm, median
over --steps runs:
  1. the ssasr_rescore launch alone (with and without the LM term);
  2. the teacher-forced pass over the list's rows: chunks of 32 rows (every decoder_loop call in the single-launch
     persistent form) beside ONE call over all rows (one launch per stage and step), each with and without the idle
     reference row of every packed group;
  3. the whole second pass (ops.rescore) and ctc_head_decode + rescore end to end, the encoder left out on both sides;
  4. in the same sitting ssasr_decode_beam at K = 8, with its step cap at the longest list entry + 1 and at
     --max-steps (an untrained model never emits <EOS>, so the cap is the number of steps it runs).

    python tools/rescore_time.py [--steps 5] [--warmup 2] [--beam 8] [--frames 100]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from beam_time import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--beam', type=int, default=8)
    ap.add_argument('--utts', type=int, default=32)
    ap.add_argument('--frames', type=int, default=100)
    ap.add_argument('--max-steps', type=int, default=200)
    args = ap.parse_args()
    from ss_asr_amd import ops
    from ss_asr_amd.asr import ASR
    from ss_asr_amd.charlm import CharLM
    dev, V, N, T, K = 'cuda:0', 50, args.utts, args.frames, args.beam
    torch.manual_seed(0)
    asr = ASR(V, 256, 256, 128, 80, 1.0).to(dev).eval()
    lm = CharLM(V, 128).to(dev).eval()
    head = torch.nn.Linear(512, V).to(dev)
    feat = torch.tanh(torch.randn(N, T, 512, device=dev))          # bounded, as a BiLSTM's outputs are
    enc_len = torch.full((N,), T, device=dev, dtype=torch.int32)
    params, psi = asr._decoder_params(), (asr.attention.psi.weight, asr.attention.psi.bias)
    res = {'shape': dict(N=N, T=T, E=512, V=V, K=K), 'runs': args.steps}
    held = {}
    t = lambda fn: timed(fn, args.steps, args.warmup)
    with torch.no_grad():
        def first_pass():
            held['ctc'] = ops.ctc_head_decode(feat, head.weight, head.bias, enc_len, K)
        res['ctc_first_pass_ms'] = t(first_pass)
        chars, n_chars, scores, n_hyps, _ = held['ctc']
        rows, hyp_lens = ops.mwer_pack(chars, n_chars, n_hyps, torch.empty(N, 0, device=dev, dtype=torch.int32), 1)
        U = int(hyp_lens.max()) + 1
        kept = rows.view(N, K + 1, -1)[:, :K].reshape(N * K, -1)
        res['list'] = dict(U=U, mean_chars=float(n_chars.float().mean()), mean_hyps=float(n_hyps.float().mean()))
        for name, r, M in (('rows_%d' % (N * K), kept, K), ('rows_%d_with_idle' % (N * (K + 1)), rows, K + 1)):
            for mode, loop_rows in (('chunks_of_32', ops.rescore_loop_rows(T)), ('one_call', 0)):
                def loop(r=r, M=M, loop_rows=loop_rows):
                    held['logits', M] = ops.rescore_logits(feat, enc_len, params, psi, r, M, U, loop_rows=loop_rows)
                res['teacher_forced_%s_%s_ms' % (name, mode)] = t(loop)

        def lm_pass():
            held['lm'] = ops.charlm_chunk(lm, kept[:, 1:U + 1].contiguous(), want_logits=True).logits.permute(1, 0, 2)
        res['charlm_chunk_ms'] = t(lm_pass)
        for name, lm_logits, w in (('no_lm', None, 0.0), ('lm', held['lm'], 0.5)):
            def kernel(lm_logits=lm_logits, w=w):
                held['out'] = ops.rescore_launch(held['logits', K], lm_logits, kept, n_hyps, scores, chars, n_chars,
                                                 att_weight=0.7, lm_weight=w, first_weight=0.3)
            res['rescore_launch_%s_ms' % name] = t(kernel)

        def second():
            held['out'] = ops.rescore(feat, enc_len, params, psi, chars, n_chars, n_hyps, scores, 1, lm, att_weight=0.7,
                                      lm_weight=0.5, first_weight=0.3)
        res['second_pass_ms'] = t(second)

        def both():
            first_pass()
            second()
        res['two_pass_ms'] = t(both)
        res['moved_to_rank_0'] = float((held['out'][0][:, 0] != 0).float().mean())
        for cap in (U, args.max_steps):
            call = (feat, enc_len, params, psi, lm, 0.5, 1, cap)
            ws = torch.empty(int(ops._lib.load().ssasr_decode_beam_ws_bytes(N, K, T, 512, 128, 256, V, 128, cap)) // 4,
                             device=dev)

            def beam(call=call, ws=ws):
                held['beam'] = ops.decode_beam(*call, K, ws=ws)
            ms = t(beam)
            ran = int(min(int(held['beam'][1].max()) + 1, cap))
            res['attention_beam_K%d_cap%d' % (K, cap)] = dict(launch_ms=ms, steps_run=ran, us_per_step=1e3 * ms / ran)
        ops.check_persistent_status()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
