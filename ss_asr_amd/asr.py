"""Listen-Attend-Spell model with the nn.Module surface of the reference's
``src/asr.py`` (ASR :15-212, Listener :214-264, Speller :267-326, Attention
:328-392, pBLSTM :394-450), computing on MI355X through libssasr_hip.so.

The torch.nn modules held below (nn.LSTM, nn.LSTMCell, nn.Linear,
nn.Embedding) are parameter containers only: they give the same
``state_dict`` keys, parameter order and constructor-time RNG consumption as
the reference, so checkpoints and seeded initialisations interchange.  Their
``forward`` is never called; all arithmetic goes through ``ss_asr_amd.ops``.
"""
import collections
import math
import os
import random

import torch
import torch.nn as nn

from . import ops, postprocess
from .preprocess import EOS_TKN, SOS_TKN, TOKENS, UNK_TKN


def _dev_i32(values, device):
    """Host list of lengths -> int32 device tensor.  Staged through pinned memory and
    copied asynchronously: a copy from pageable memory (torch.tensor(..., device=cuda))
    waits for the stream to drain, which stalled the host 3.5 ms twice per train step."""
    t = torch.tensor([int(v) for v in values], dtype=torch.int32)
    if torch.device(device).type != 'cuda':
        return t.to(device)
    return t.pin_memory().to(device, non_blocking=True)

EOS_INDEX = 1   # '>' in TOKENS + ALL_CHARS (src/preprocess.py:17-27)

ENCODER_STRIDE = 8      # input frames per encoder frame: three pBLSTM layers, each halving the time axis

# ASR.align's result for one utterance (BUILD-DEFINED).  score: log-probability of the best CTC path (float, -inf
# when no alignment fits); chars: [(char, first_frame, last_frame_exclusive, logp)] in input frames (seconds with
# frame_shift), or None when no alignment fits.
Alignment = collections.namedtuple('Alignment', ('score', 'chars'))

# ASR.segment's result for one recording (BUILD-DEFINED).  score: log-probability of the best CTC path of the whole
# text inside the recording (float, -inf when nothing fits); span: (start, end exclusive) of the text in input frames
# (seconds with frame_shift); utterances: [Segment(text, start, end, confidence)], confidence the min-mean of the path's
# log-probabilities over blocks of `window` encoder frames; chars as in Alignment.  span, utterances and chars are None
# when nothing fits.  With ASR.segment's skip_penalty / fill_penalty: an utterance that was passed over has skipped True,
# start = end = None and confidence 0.0 (its characters (char, None, None, 0.0)); fillers: [(start, end exclusive)] of the
# runs of frames taken as unwritten speech at an utterance boundary, in the spans' unit (None without the penalties).
Segmentation = collections.namedtuple('Segmentation', ('score', 'span', 'utterances', 'chars', 'fillers'), defaults=(None,))
Segment = collections.namedtuple('Segment', ('text', 'start', 'end', 'confidence', 'skipped'), defaults=(False,))

# ASR.score's result for one utterance (BUILD-DEFINED).  chars, words: (S, D, I, N) of the best hypothesis against
# the reference, N the reference's count; oracle: (k, chars, words) of the n-best entry with the fewest word errors
# (ties: fewest character errors, then lowest k), the best entry itself for a greedy decode.
Score = collections.namedtuple('Score', ('chars', 'words', 'oracle'))

# ASR.mbr's result for one utterance (BUILD-DEFINED).  k: the slot with the lowest expected error count under the
# list's own posterior (-1 for an empty list); text: its transcript; risk: that expectation; risks: the tuple of
# expectations over the list's entries.
MBR = collections.namedtuple('MBR', ('k', 'text', 'risk', 'risks'))


def input_span(first, last, n_frames, frame_shift=None):
    """Encoder frames first .. last (inclusive) -> the input frames [lo, hi) they cover: encoder frame j covers
    input frames [8 j, 8 j + 8), clipped to the utterance's n_frames.  frame_shift (seconds per input frame): both
    ends in seconds."""
    lo, hi = min(ENCODER_STRIDE * first, n_frames), min(ENCODER_STRIDE * (last + 1), n_frames)
    if frame_shift is None:
        return lo, hi
    return lo * float(frame_shift), hi * float(frame_shift)


def _check_lengths(state_len, tmax):
    """pack_padded_sequence's input contract (src/asr.py:413)."""
    prev = None
    for l in state_len:
        if l <= 0:
            raise RuntimeError('Length of all samples has to be greater than 0, '
                               'but found an element in \'lengths\' that is <= 0')
        if prev is not None and l > prev:
            raise RuntimeError('`lengths` array must be sorted in decreasing order when '
                               '`enforce_sorted` is True.')
        prev = l
    if state_len[0] > tmax:
        raise RuntimeError('Expected sequence length to be larger than or equal to the '
                           'maximum length in `lengths`')


def _lstm_weights(lstm):
    return [getattr(lstm, n + sfx) for sfx in ('', '_reverse')
            for n in ('weight_ih_l0', 'weight_hh_l0', 'bias_ih_l0', 'bias_hh_l0')]


class pBLSTM(nn.Module):
    """src/asr.py:394-450: packed BiLSTM, then concatenation of frame pairs."""

    def __init__(self, in_dim, out_dim):
        super().__init__()
        self.layer = nn.LSTM(in_dim, out_dim, bidirectional=True, batch_first=True)

    def forward(self, input_x, state=None, state_len=None, pack_input=False, len_dev=None, slots=None):
        if state is not None:
            raise NotImplementedError('initial states are always zero on the hot path')
        if pack_input:
            assert state_len is not None, \
                "Please specify seq len for pack_padded_sequence."
            state_len = [int(s) for s in state_len]
            _check_lengths(state_len, input_x.shape[1])
            steps = state_len[0]
            if len_dev is None:
                len_dev = _dev_i32(state_len, input_x.device)
        else:
            steps, len_dev = input_x.shape[1], None
        output = ops.bilstm(input_x, len_dev, steps, True, _lstm_weights(self.layer), slots=slots)
        output = self.downsample(output)
        if state_len is not None:
            return output, None, [int(s / 2) for s in state_len]
        return output, None

    def downsample(self, x):
        """[B, T, F] -> [B, T//2, 2F]; an odd last frame is dropped (src/asr.py:429-450)."""
        t_dim, f_dim = x.shape[1], x.shape[2]
        if t_dim % 2 != 0:
            # a view, not a copy: pairs of frames merge into rows of 2F floats whatever the utterance stride is, and
            # the next layer's kernels take strides (ops._BiLSTM.forward)
            x = x[:, :t_dim - 1, :]
            t_dim -= 1
            if x.stride(2) == 1 and x.stride(1) == f_dim and os.environ.get('SSASR_DOWNSAMPLE_COPY') != '1':
                return x.view([x.shape[0], int(t_dim / 2), f_dim * 2])
        return x.contiguous().view([-1, int(t_dim / 2), f_dim * 2])


class Listener(nn.Module):
    """src/asr.py:214-264."""

    def __init__(self, state_size, feature_dim):
        super().__init__()
        self.state_size = state_size
        self.out_dim = 2 * self.state_size
        self.blstm_1 = pBLSTM(feature_dim, self.state_size)
        self.blstm_2 = pBLSTM(self.state_size * 2 * 2, self.state_size)
        self.blstm_3 = pBLSTM(self.state_size * 2 * 2, self.state_size)
        # Not batch_first in the reference (src/asr.py:237-238): the recurrence
        # runs over the utterance axis, independently per encoder time index.
        self.blstm_4 = nn.LSTM(self.state_size * 2 * 2, self.state_size, bidirectional=True)

    def get_outdim(self):
        return self.out_dim

    @staticmethod
    def layer_lengths(state_len):
        """Frame counts seen by blstm_1..3 and by the decoder (each pBLSTM halves them,
        src/asr.py:425)."""
        out = [[int(s) for s in state_len]]
        for _ in range(3):
            out.append([int(s / 2) for s in out[-1]])
        return out

    def forward(self, x, state_len, pack_input=True, len_devs=None, arenas=None):
        """len_devs: the first three lists of layer_lengths(state_len) as int32 device
        tensors when the caller has uploaded them already.  arenas: (forward, backward)
        ops.ExchangeArena of this pass; the four layers' exchange workspaces are reserved in
        them so that one fill arms all of them."""
        if pack_input and len_devs is None:
            len_devs = ops.upload_i32(x.device, *self.layer_lengths(state_len)[:3])
        slots = [None] * 4
        if arenas is not None and pack_input:
            lens = self.layer_lengths(state_len)
            B, H = x.shape[0], self.state_size
            shapes = [(lens[0][0], B), (lens[1][0], B), (lens[2][0], B), (B, lens[3][0])]   # (steps, columns)
            for k, (S, N) in enumerate(shapes):
                hx, ring = ops.bilstm_exchange_floats(S, N, H)
                slots[k] = (arenas[0], arenas[0].reserve(hx) if hx else None,
                            arenas[1], arenas[1].reserve(ring) if ring else None)
        for k, layer in enumerate((self.blstm_1, self.blstm_2, self.blstm_3)):
            x, _, state_len = layer(x, state_len=state_len, pack_input=pack_input,
                                    len_dev=len_devs[k] if pack_input else None, slots=slots[k])
        x = ops.bilstm(x, None, x.shape[0], False, _lstm_weights(self.blstm_4), slots=slots[3])      # src/asr.py:262
        return x, state_len


class Speller(nn.Module):
    """src/asr.py:267-326."""

    def __init__(self, state_size, encoder_out_size):
        super().__init__()
        self.layer_1 = nn.LSTMCell(input_size=encoder_out_size + state_size, hidden_size=state_size)
        self.layer_2 = nn.LSTMCell(input_size=state_size, hidden_size=state_size)
        self._zero_state = None
        self._state_list = []
        self._cell_list = []
        self.state_size = state_size
        self.num_layers = 2

    def init_rnn(self, batch_size, device):
        """Zero states (src/asr.py:284-290).  Allocated on first use: the fused decode loop
        never reads them, only step-by-step callers do."""
        self._zero_state = (batch_size, device)
        self._state_list = self._cell_list = None

    def _materialise(self):
        if self._state_list is None and self._zero_state is not None:
            b, dev = self._zero_state
            self._state_list = [torch.zeros(b, self.state_size, device=dev)] * self.num_layers
            self._cell_list = [torch.zeros(b, self.state_size, device=dev)] * self.num_layers

    @property
    def state_list(self):
        self._materialise()
        return self._state_list

    @state_list.setter
    def state_list(self, v):
        self._materialise()
        self._state_list = v

    @property
    def cell_list(self):
        self._materialise()
        return self._cell_list

    @cell_list.setter
    def cell_list(self, v):
        self._materialise()
        self._cell_list = v

    @property
    def hidden_state(self):
        return [s.clone().detach().cpu() for s in self.state_list], \
            [c.clone().detach().cpu() for c in self.cell_list]

    @hidden_state.setter
    def hidden_state(self, state):
        device = self.state_list[0].device
        self.state_list = [s.to(device) for s in state[0]]
        self.cell_list = [c.to(device) for c in state[1]]

    def forward(self, input_context):
        l1, l2 = self.layer_1, self.layer_2
        self.state_list[0], self.cell_list[0] = ops.lstm_cell(
            input_context, self.state_list[0], self.cell_list[0],
            l1.weight_ih, l1.weight_hh, l1.bias_ih, l1.bias_hh)
        self.state_list[1], self.cell_list[1] = ops.lstm_cell(
            self.state_list[0], self.state_list[1], self.cell_list[1],
            l2.weight_ih, l2.weight_hh, l2.bias_ih, l2.bias_hh)
        return self.state_list[-1]


class Attention(nn.Module):
    """src/asr.py:328-392 (content based; psi projection cached per utterance batch)."""

    def __init__(self, mlp_out_size, encoder_out_size, decoder_state_size):
        super().__init__()
        self.phi = nn.Linear(decoder_state_size, mlp_out_size, bias=False)
        self.psi = nn.Linear(encoder_out_size, mlp_out_size)
        self.comp_listener_feature = None
        self.state_mask = None      # here: int32 lengths on the device

    def reset_enc_mem(self):
        self.comp_listener_feature = None
        self.state_mask = None

    def forward(self, decoder_state, listener_feature, state_len):
        if self.comp_listener_feature is None:
            self.state_mask = _dev_i32(state_len, listener_feature.device)
            self.comp_listener_feature = ops.attn_precompute(
                listener_feature, self.psi.weight, self.psi.bias)
        return ops.attn_step(decoder_state, self.phi.weight, self.comp_listener_feature,
                             listener_feature, self.state_mask)


class ASR(nn.Module):
    """src/asr.py:15-212; same constructor arguments and state_dict."""

    def __init__(self, output_dim, encoder_state_size, decoder_state_size, mlp_out_size,
                 feature_dim, tf_rate):
        super().__init__()
        enc_out_dim = encoder_state_size * 2
        self.encoder = Listener(encoder_state_size, feature_dim)
        self.attention = Attention(mlp_out_size, enc_out_dim, decoder_state_size)
        self.decoder = Speller(decoder_state_size, enc_out_dim)
        self.embed = nn.Embedding(output_dim, decoder_state_size)
        self.char_trans = nn.Linear(decoder_state_size, output_dim)
        self.tf_rate = tf_rate
        # When True (default) the training-mode attention map is copied to the
        # host asynchronously (pinned memory); call torch.cuda.synchronize()
        # or self.att_event.synchronize() before reading it.  eval() mode
        # always returns a finished copy.
        self.async_att = True
        # False: the attention map stays on the device (ASRTrainStep sets this around a train step)
        self.att_on_host = True
        self.att_event = None
        self.last_chars = self.last_modes = self.last_uniforms = None
        self.last_encoded = None
        # decode_many's device results: (chars [N, steps] int32, n_chars [N] int32, scores [N, steps, V], att [N, steps, T'])
        self.last_decode = None
        # decode_nbest's device results for beam_size > 1: (chars [N, K, steps] int32, n_chars [N, K] int32,
        # hyp_scores [N, K], n_hyps [N] int32)
        self.last_beam = None
        # n_steps [N] int32 of the last decode_nbest call that had a length bonus, a coverage term or end detection on
        self.last_beam_steps = None
        # graph_scores [N, K] of the last decode_nbest call if it had a character graph at a weight > 0, else None
        self.last_beam_graph = None
        # _encode_packed's most recent result: (features [N, T'max, E], int32 [N] frame counts), what align() reuses
        self.last_encoded_packed = None
        # align's device results: (path [N, T'], first [N, Lmax], last [N, Lmax], char_logp [N, Lmax], score [N] double,
        # logits [N, T', V])
        self.last_align = None
        self.last_segment = None
        # what the most recent decode_many / decode_nbest call left to score(): (chars [N, K, steps] int32,
        # n_chars [N, K] int32, n_hyps [N] int32), views of last_decode (K = 1) or last_beam
        self.last_hyps = None
        # the scores [N, K] float32 that belong to last_hyps, and whether last_hyps are draws (sample) -- what mbr()
        # forms its posterior from; mbr's device results (best [N] int32, risk [N, K], pair [N, K, K, 2] int32)
        self.last_hyp_scores = None
        self.last_hyps_sampled = False
        self.last_mbr = None
        # sample's device results: (chars [N, K, steps] int32 in slot order, n_chars [N, K] int32, hyp_scores [N, K],
        # n_hyps [N] int32, logq [N, K])
        self.last_samples = None
        # decode_ctc's device results: (chars [N, Kr, T'] int32, n_chars [N, Kr] int32, scores [N, Kr], n_hyps [N] int32,
        # logits [N, T', V])
        self.last_ctc_decode = None
        # rescore's device results: (order [N, K] int32, total [N, K], parts [N, K, 3] = (att, lm, first)), in rank order
        self.last_rescore = None
        self.init_parameters()

    def init_parameters(self):
        """src/asr.py:175-212."""
        for p in self.parameters():
            data = p.data
            if data.dim() == 1:
                data.zero_()
            elif data.dim() == 2:
                data.normal_(0, 1. / math.sqrt(data.size(1)))
            else:
                raise NotImplementedError
        self.embed.weight.data.normal_(0, 1)
        for bias in (self.decoder.layer_1.bias_ih, self.decoder.layer_2.bias_ih):
            n = bias.size(0)
            bias.data[n // 4:n // 2].fill_(1.)

    def _decoder_params(self):
        l1, l2 = self.decoder.layer_1, self.decoder.layer_2
        return dict(w_phi=self.attention.phi.weight,
                    w_ih1=l1.weight_ih, w_hh1=l1.weight_hh, b_ih1=l1.bias_ih, b_hh1=l1.bias_hh,
                    w_ih2=l2.weight_ih, w_hh2=l2.weight_hh, b_ih2=l2.bias_ih, b_hh2=l2.bias_hh,
                    embed=self.embed.weight, w_ct=self.char_trans.weight,
                    b_ct=self.char_trans.bias)

    def encode(self, audio_feature, state_len, decode_step=None, modes=()):
        """The Listener on a batch, the half of forward() before the decode loop (src/asr.py:60-66), for callers
        that run the loop themselves (engine.MWERTrainStep encodes ONCE and decodes K + 1 rows per utterance).
        decode_step: the loop length whose exchange workspaces are reserved beside the encoder's, None for no
        reservation; modes: per-step integers uploaded with the lengths.
        Returns (features [B, T', E], encode_len list, the same as an int32 device tensor, the decode loop's
        `slots` or None, modes on the device or None)."""
        dev = audio_feature.device
        # every per-step integer the device needs, in one upload
        lens = Listener.layer_lengths(state_len)
        l1, l2, l3, enc_len_dev, modes_dev = ops.upload_i32(dev, lens[0], lens[1], lens[2], lens[3], modes)
        # exchange workspaces of the whole pass: two allocations, each armed by one fill
        arenas = (ops.ExchangeArena(dev), ops.ExchangeArena(dev))
        dec_slots = None
        if decode_step is not None:
            dec_slots = ops.decoder_reserve(arenas[0], arenas[1], audio_feature.shape[0], lens[3][0], decode_step,
                                            A=self.attention.phi.weight.shape[0], E=self.encoder.out_dim,
                                            D=self.decoder.state_size, V=self.char_trans.weight.shape[0])
        encode_feature, encode_len = self.encoder(audio_feature, state_len, len_devs=(l1, l2, l3), arenas=arenas)
        # what a second head on the encoder (ss_asr_amd/ctc.py) reads: output and its int32 frame counts
        self.last_encoded = (encode_feature, enc_len_dev)
        self.decoder.init_rnn(encode_feature.shape[0], dev)
        self.attention.reset_enc_mem()
        return encode_feature, encode_len, enc_len_dev, dec_slots, modes_dev if len(modes) else None

    def forward(self, audio_feature, decode_step, teacher=None, state_len=None):
        """Returns (encode_len: list[int], logits [B,U,V] on the device,
        attention [B,U,T'] on the host, detached) -- src/asr.py:52-110."""
        dev = audio_feature.device
        # One host coin flip per step, as the reference draws them (src/asr.py:94).
        if teacher is not None:
            modes = [0 if random.random() <= self.tf_rate else 1 for _ in range(decode_step)]
            teacher_i32 = ops.as_i32(teacher)
        else:
            modes = [2] * decode_step
            teacher_i32 = None
        encode_feature, encode_len, enc_len_dev, dec_slots, modes_dev = self.encode(audio_feature, state_len,
                                                                                    decode_step, modes)
        uniforms = None
        if 1 in modes:
            # Categorical(...).sample() of the reference (src/asr.py:97): one
            # uniform per (step, utterance), inverse-CDF draw inside the kernel.
            uniforms = torch.rand(decode_step, encode_feature.shape[0], device=dev)
        # (the cached projection tanh(psi(h)) of src/asr.py:381 is computed inside the loop's node)
        logits, att, chars = ops.decoder_loop(encode_feature, None, enc_len_dev, teacher_i32,
                                              modes, uniforms, self._decoder_params(),
                                              modes_dev=modes_dev if decode_step else None,
                                              psi=(self.attention.psi.weight, self.attention.psi.bias),
                                              slots=dec_slots)
        # what the loop was driven by: characters fed to each step [U+1, B], the per-step modes
        # (0 teacher, 1 sample, 2 argmax) and the uniforms of the sampled steps [U, B] or None
        self.last_chars, self.last_modes, self.last_uniforms = chars, modes, uniforms
        if not self.att_on_host:
            host = att.detach()         # left on the device (train steps never look at it)
        elif self.training and self.async_att:
            host = torch.empty(att.shape, dtype=att.dtype, pin_memory=True)
            host.copy_(att.detach(), non_blocking=True)
            self.att_event = torch.cuda.Event()
            self.att_event.record()
        else:
            host = att.detach().cpu()
        return encode_len, logits, host

    _NO_CTC_HEAD = 'ctc_weight > 0 needs a model with a ctc_head (ctc.JointCTCASR); %s has none'

    def _ctc_head(self, ctc_weight):
        """None for ctc_weight 0 (today's path), else (ctc_head weight, bias, ctc_weight) of a model that has one."""
        ctc_weight = float(ctc_weight)
        if not 0.0 <= ctc_weight <= 1.0:
            raise ValueError('ctc_weight must lie in [0, 1], got %r' % (ctc_weight,))
        if ctc_weight == 0.0:
            return None
        head = getattr(self, 'ctc_head', None)
        if head is None:
            raise ValueError(self._NO_CTC_HEAD % type(self).__name__)
        return head.weight, head.bias, ctc_weight

    @staticmethod
    def _beam_terms(length_bonus, coverage_weight, coverage_threshold, end_margin):
        """None with every term at its default (today's path), else ops.decode_beam_ex's keywords."""
        length_bonus, coverage_weight = float(length_bonus), float(coverage_weight)
        if not math.isfinite(length_bonus):
            raise ValueError('length_bonus must be finite, got %r' % (length_bonus,))
        if not math.isfinite(coverage_weight):
            raise ValueError('coverage_weight must be finite, got %r' % (coverage_weight,))
        if coverage_weight != 0.0:
            coverage_threshold = float(coverage_threshold)
            if not (math.isfinite(coverage_threshold) and coverage_threshold > 0.0):
                raise ValueError('coverage_threshold must be finite and > 0, got %r' % (coverage_threshold,))
        if end_margin is not None:
            end_margin = float(end_margin)
            if not (math.isfinite(end_margin) and end_margin >= 0.0):
                raise ValueError('end_margin must be None or finite and >= 0, got %r' % (end_margin,))
        if length_bonus == 0.0 and coverage_weight == 0.0 and end_margin is None:
            return None
        return dict(length_bonus=length_bonus, coverage_weight=coverage_weight,
                    coverage_threshold=coverage_threshold if coverage_weight != 0.0 else 0.5, end_margin=end_margin)

    def _beam_graph_weight(self, graph, graph_weight):
        """The beam search's graph keywords, checked as _ctc_graph_weight checks decode_ctc's: the weight as a float,
        0.0 when no graph term runs (today's path)."""
        from .char_graph import CharGraph
        if isinstance(graph_weight, bool) or not isinstance(graph_weight, (int, float)) or \
                not (math.isfinite(graph_weight) and graph_weight >= 0.0):
            raise ValueError('graph_weight must be a finite number >= 0, got %r' % (graph_weight,))
        if graph is not None and not isinstance(graph, CharGraph):
            raise ValueError('graph must be a char_graph.CharGraph, got %s' % type(graph).__name__)
        if graph_weight == 0.0:
            return 0.0
        if graph is None:
            raise ValueError('graph_weight %g needs graph' % graph_weight)
        if graph.n_classes != self.char_trans.weight.shape[0]:
            raise ValueError('the graph has %d classes, the model %d'
                             % (graph.n_classes, self.char_trans.weight.shape[0]))
        return float(graph_weight)

    def decode(self, x, x_len, rnn_lm, mapper, lm_weight, max_decoding_steps=200, *, beam_size=1, ctc_weight=0.0,
               length_bonus=0.0, coverage_weight=0.0, coverage_threshold=0.5, end_margin=None, graph=None,
               graph_weight=0.0):
        """src/asr.py:112-173: greedy decoding of ONE utterance (x [1, seq, features], x_len from prepare_x)
        until <EOS> or max_decoding_steps (200 in the reference, :128), every step's character scores being
        log_softmax(speller) + lm_weight * log_softmax(rnn_lm).  Returns the decoded string.  rnn_lm None: no LM
        term.  The whole loop is one launch (ssasr_decode_greedy).  beam_size > 1: the best hypothesis of a beam
        search of that width (decode_many).  ctc_weight > 0: joint CTC / attention decoding (decode_nbest).
        length_bonus, coverage_weight / coverage_threshold, end_margin: the beam search's terms (decode_nbest).
        graph / graph_weight: a character graph in the beam search (decode_nbest)."""
        assert len(x.shape) == 3 and x.shape[0] == 1
        return self.decode_many([x], [x_len], rnn_lm, mapper, lm_weight, max_decoding_steps=max_decoding_steps,
                                beam_size=beam_size, ctc_weight=ctc_weight, length_bonus=length_bonus,
                                coverage_weight=coverage_weight, coverage_threshold=coverage_threshold,
                                end_margin=end_margin, graph=graph, graph_weight=graph_weight)[0]

    def _encode_packed(self, xs, x_lens):
        """Each utterance encoded alone, packed to ([N, T'max, E], int32 [N] frame counts on the device)."""
        feats, enc_lens = [], []
        for x, x_len in zip(xs, x_lens):
            assert len(x.shape) == 3 and x.shape[0] == 1
            feat, enc_len = self.encoder(x, x_len)
            feats.append(feat)
            enc_lens.append(int(enc_len[0]))
        dev = feats[0].device
        tmax = max(f.shape[1] for f in feats)
        if len(feats) == 1:
            packed = feats[0]
        else:
            packed = torch.zeros(len(feats), tmax, feats[0].shape[2], device=dev, dtype=torch.float32)
            for n, f in enumerate(feats):
                packed[n, :f.shape[1]] = f[0]
        self.last_encoded_packed = (packed, _dev_i32(enc_lens, dev))
        return self.last_encoded_packed

    def align(self, xs, x_lens, texts, mapper, *, frame_shift=None, encoded=None):
        """BUILD-DEFINED: CTC forced alignment of texts[i] to utterance i (xs, x_lens as decode_many takes them) on a
        model with a ctc_head: the most probable CTC path of the text through the head's frames (ssasr_ctc_align,
        include/ssasr.h).  `<` and `>` are stripped from the texts, <eos> is not aligned; a character the mapper does
        not know is a ValueError.  Each utterance is encoded alone (_encode_packed), then ONE align launch serves the
        group.  encoded: a (features, frame counts) pair that _encode_packed already returned for these utterances
        (last_encoded_packed after a decode), used instead of encoding again.
        Returns one Alignment(score, chars) per utterance: chars = [(char, first_frame, last_frame_exclusive, logp)]
        in INPUT frames (input_span: encoder frame j covers input frames [8 j, 8 j + 8), clipped to the utterance's
        length; seconds when frame_shift, the seconds per input frame, is given), logp = the head's log-probability
        of the character summed over its frames; chars is None and score -inf when no alignment fits.  last_align
        keeps (path, first, last, char_logp, score, logits) on the device, in encoder frames."""
        head = getattr(self, 'ctc_head', None)
        if head is None:
            raise ValueError(self._NO_CTC_HEAD % type(self).__name__)
        if not len(xs) == len(x_lens) == len(texts):
            raise ValueError('align: %d utterances, %d lengths, %d texts' % (len(xs), len(x_lens), len(texts)))
        texts = [t.replace(SOS_TKN, '').replace(EOS_TKN, '') for t in texts]
        labels = []
        for text in texts:
            try:
                labels.append([int(mapper.char_to_ind(c)) for c in text])
            except (KeyError, ValueError):
                raise ValueError('align: %r has a character the mapper does not know' % (text,)) from None
        lmax = max(len(row) for row in labels)
        with torch.no_grad():
            packed, enc_lens = encoded if encoded is not None else self._encode_packed(xs, x_lens)
            if packed.shape[0] != len(texts):
                raise ValueError('align: the encoded group holds %d utterances, not %d' % (packed.shape[0], len(texts)))
            y = torch.zeros(len(labels), max(lmax, 1), dtype=torch.int32)
            for i, row in enumerate(labels):
                y[i, :len(row)] = torch.tensor(row, dtype=torch.int32)
            y = y.to(packed.device)
            self.last_align = ops.ctc_head_align(packed, head.weight, head.bias, enc_lens, y,
                                                 _dev_i32([len(row) for row in labels], packed.device), lmax,
                                                 ops.CTC_BLANK)
        _, first, last, char_logp, score, _ = self.last_align
        first, last, char_logp, score = first.cpu().tolist(), last.cpu().tolist(), char_logp.cpu().tolist(), score.cpu().tolist()
        out = []
        for i, text in enumerate(texts):
            if score[i] == -math.inf:
                out.append(Alignment(score[i], None))
                continue
            n = int(x_lens[i][0])
            out.append(Alignment(score[i], [(c,) + input_span(first[i][j], last[i][j], n, frame_shift) + (char_logp[i][j],)
                                            for j, c in enumerate(text)]))
        return out

    def segment(self, xs, x_lens, texts, mapper, *, window=30, frame_shift=None, encoded=None, skip_penalty=None,
                fill_penalty=None):
        """BUILD-DEFINED: CTC segmentation of recording i (xs, x_lens as align takes them) with the running transcript
        texts[i], the LIST of its utterance strings, on a model with a ctc_head: where inside the recording the text
        was spoken and where each utterance starts and ends (ssasr_ctc_segment, include/ssasr.h: align's lattice on
        normalised values, with a free start and a free end, so audio before, after and beyond the text is left
        out).  `<` and `>` are stripped as in align; an unknown character or an empty utterance is a ValueError.  Each
        recording is encoded alone and whole (_encode_packed; at most ops.CTC_SEGMENT_MAX_FRAMES encoder frames and
        ops.CTC_SEGMENT_MAX_LABELS characters per recording -- encoding in chunks is not done here), then ONE launch
        serves the group.  encoded: as in align.  window: the confidence's block length in encoder frames.
        Returns one Segmentation(score, span, utterances, chars) per recording, spans in INPUT frames through
        input_span (seconds when frame_shift is given); utterances is None and score -inf when nothing fits.
        last_segment keeps (path, first, last, char_logp, score, utt_first, utt_last, utt_conf, logits) on the device,
        in encoder frames.
        skip_penalty / fill_penalty (None: off; else a finite number <= 0), for transcripts that are not verbatim
        (ssasr_ctc_segment_skip): an utterance that was never spoken may be passed over at skip_penalty -- it comes
        back with skipped True and no span -- and frames of speech that nobody wrote down may be taken at an utterance
        boundary at fill_penalty each -- they come back as Segmentation.fillers.  last_segment then holds utt_skipped
        and is_fill before the logits.  With both None nothing changes."""
        head = getattr(self, 'ctc_head', None)
        if head is None:
            raise ValueError(self._NO_CTC_HEAD % type(self).__name__)
        if not len(xs) == len(x_lens) == len(texts):
            raise ValueError('segment: %d recordings, %d lengths, %d texts' % (len(xs), len(x_lens), len(texts)))
        if not len(texts):
            raise ValueError('segment: no recording')
        if isinstance(window, bool) or not isinstance(window, int) or window < 1:
            raise ValueError('segment: window must be an integer >= 1, got %r' % (window,))
        ops._segment_penalty('skip_penalty', skip_penalty)       # a ValueError for anything but None or a finite number <= 0
        ops._segment_penalty('fill_penalty', fill_penalty)
        with_skip = skip_penalty is not None or fill_penalty is not None
        clean, labels, ends = [], [], []
        for utts in texts:
            if isinstance(utts, str) or not len(utts):
                raise ValueError('segment: a recording\'s text is the non-empty list of its utterances, got %r' % (utts,))
            utts = [u.replace(SOS_TKN, '').replace(EOS_TKN, '') for u in utts]
            row, row_ends = [], []
            for u in utts:
                if not u:
                    raise ValueError('segment: an utterance is empty')
                try:
                    row.extend(int(mapper.char_to_ind(c)) for c in u)
                except (KeyError, ValueError):
                    raise ValueError('segment: %r has a character the mapper does not know' % (u,)) from None
                row_ends.append(len(row))
            if len(row) > ops.CTC_SEGMENT_MAX_LABELS:
                raise ValueError('segment: a text of %d characters; the kernel takes at most %d'
                                 % (len(row), ops.CTC_SEGMENT_MAX_LABELS))
            clean.append(utts)
            labels.append(row)
            ends.append(row_ends)
        lmax, nmax = max(len(row) for row in labels), max(len(row) for row in ends)
        if with_skip and nmax > ops.CTC_SEGMENT_SKIP_MAX_UTTS:
            raise ValueError('segment: a text of %d utterances; with skip_penalty / fill_penalty the kernel takes at most '
                             '%d' % (nmax, ops.CTC_SEGMENT_SKIP_MAX_UTTS))
        with torch.no_grad():
            if encoded is None:
                for x_len in x_lens:
                    if -(-int(x_len[0]) // ENCODER_STRIDE) > ops.CTC_SEGMENT_MAX_FRAMES:
                        raise ValueError('segment: a recording of %d input frames; the kernel takes at most %d encoder '
                                         'frames (%d input frames)' % (int(x_len[0]), ops.CTC_SEGMENT_MAX_FRAMES,
                                                                       ops.CTC_SEGMENT_MAX_FRAMES * ENCODER_STRIDE))
                try:
                    encoded = self._encode_packed(xs, x_lens)
                except ValueError as err:                      # what ops raise for a shape that has no kernel
                    raise ValueError('segment: encoding failed for recordings of up to %d input frames (the '
                                     'segmentation kernel takes %d; a recording is encoded whole, not in chunks): %s'
                                     % (max(int(l[0]) for l in x_lens), ops.CTC_SEGMENT_MAX_FRAMES * ENCODER_STRIDE,
                                        err)) from err
            packed, enc_lens = encoded
            if packed.shape[0] != len(texts):
                raise ValueError('segment: the encoded group holds %d recordings, not %d' % (packed.shape[0], len(texts)))
            y = torch.zeros(len(labels), lmax, dtype=torch.int32)
            ue = torch.zeros(len(labels), nmax, dtype=torch.int32)
            for i, (row, row_ends) in enumerate(zip(labels, ends)):
                y[i, :len(row)] = torch.tensor(row, dtype=torch.int32)
                ue[i, :len(row_ends)] = torch.tensor(row_ends, dtype=torch.int32)
            dev = packed.device
            self.last_segment = ops.ctc_head_segment(packed, head.weight, head.bias, enc_lens, y.to(dev),
                                                     _dev_i32([len(row) for row in labels], dev), ue.to(dev),
                                                     _dev_i32([len(row) for row in ends], dev), lmax, nmax, window,
                                                     ops.CTC_BLANK, skip_penalty=skip_penalty,
                                                     fill_penalty=fill_penalty)
        path, first, last, char_logp, score, utt_first, utt_last, utt_conf = [
            t.cpu().tolist() for t in self.last_segment[:8]]
        utt_skipped, is_fill = [t.cpu().tolist() for t in self.last_segment[8:10]] if with_skip else (None, None)
        out = []
        for i, utts in enumerate(clean):
            if score[i] == -math.inf:
                out.append(Segmentation(score[i], None, None, None))
                continue
            n = int(x_lens[i][0])
            frames = [t for t, s in enumerate(path[i]) if s >= 0]
            text = ''.join(utts)
            if not with_skip:
                out.append(Segmentation(
                    score[i], input_span(frames[0], frames[-1], n, frame_shift),
                    [Segment(u, *(input_span(utt_first[i][k], utt_last[i][k], n, frame_shift) + (utt_conf[i][k],)))
                     for k, u in enumerate(utts)],
                    [(c,) + input_span(first[i][j], last[i][j], n, frame_shift) + (char_logp[i][j],)
                     for j, c in enumerate(text)]))
                continue
            span_of = lambda lo, hi: (None, None) if lo < 0 else input_span(lo, hi, n, frame_shift)
            runs = []                                           # maximal runs of filler frames, (first, last)
            for t in frames:
                if is_fill[i][t] == 1:
                    if runs and runs[-1][1] == t - 1:
                        runs[-1][1] = t
                    else:
                        runs.append([t, t])
            out.append(Segmentation(
                score[i], input_span(frames[0], frames[-1], n, frame_shift),
                [Segment(u, *(span_of(utt_first[i][k], utt_last[i][k]) + (utt_conf[i][k], bool(utt_skipped[i][k]))))
                 for k, u in enumerate(utts)],
                [(c,) + span_of(first[i][j], last[i][j]) + (char_logp[i][j],) for j, c in enumerate(text)],
                [input_span(lo, hi, n, frame_shift) for lo, hi in runs]))
        return out

    def score(self, refs, mapper):
        """BUILD-DEFINED: edit-distance scores of the hypotheses that the last decode_many / decode_nbest call left on
        the device (last_hyps) against refs, one per utterance of that call: a row of label ids (list or tensor; pads,
        `<` and `>` are dropped) or a string.  ONE launch scores every (hypothesis, reference) pair of the group at
        character and word level (ssasr_edit_score, include/ssasr.h); no transcript is copied to the host to be
        scored.  Returns one Score(chars=(S, D, I, N), words=(S, D, I, N), oracle=(k, chars, words)) per utterance:
        chars / words of the best hypothesis, oracle the n-best entry with the fewest word errors (ties: fewest
        character errors, then lowest k).  Rows past the kernel's limits (a reference of more than 1,023 ids, more
        than 8,191 decoding steps) are scored by postprocess.edit_counts on the host.  A call before any decode, or
        with another number of references than that decode had utterances, is a ValueError."""
        if self.last_hyps is None:
            raise ValueError('score: nothing decoded yet (decode_many / decode_nbest leave the hypotheses)')
        chars, n_chars, n_hyps = self.last_hyps
        N, K, steps = chars.shape
        if len(refs) != N:
            raise ValueError('score: %d references for the %d utterances of the last decode' % (len(refs), N))
        rows = []
        for ref in refs:
            if isinstance(ref, str):
                try:
                    rows.append([int(mapper.char_to_ind(c)) for c in ref])
                except (KeyError, ValueError):
                    raise ValueError('score: %r has a character the mapper does not know' % (ref,)) from None
            else:
                rows.append([int(c) for c in (ref.reshape(-1).tolist() if torch.is_tensor(ref) else ref)])
        space, first_char = int(mapper.char_to_ind(' ')), TOKENS.index(UNK_TKN)
        rmax = max(len(row) for row in rows) if rows else 0
        n_hyps_host = n_hyps.cpu().tolist()
        if rmax <= ops.EDIT_SCORE_MAX_REF and steps <= ops.EDIT_SCORE_MAX_HYP:
            dev = chars.device
            ref = torch.zeros(N, max(rmax, 1), dtype=torch.int32)
            for i, row in enumerate(rows):
                ref[i, :len(row)] = torch.tensor(row, dtype=torch.int32)
            ref_of = torch.arange(N, dtype=torch.int32).repeat_interleave(K)
            out = ops.edit_score(chars.reshape(N * K, steps), n_chars.reshape(N * K), ref.to(dev),
                                 _dev_i32([len(row) for row in rows], dev), ref_of.to(dev),
                                 first_char=first_char, space=space).view(N, K, 8).cpu().tolist()
        else:
            hyp, lens = chars.cpu().tolist(), n_chars.cpu().tolist()
            out = [[postprocess.edit_counts(hyp[i][k][:max(lens[i][k], 0)], rows[i], space, first_char)
                    for k in range(K)] for i in range(N)]
        self.last_score_rows = out          # [N][K][8]: every hypothesis' counts, for callers that choose another slot
        scores = []
        for i in range(N):
            cand = out[i][:max(min(n_hyps_host[i], K), 1)]
            k = min(range(len(cand)), key=lambda k: (sum(cand[k][4:7]), sum(cand[k][0:3]), k))
            scores.append(Score(tuple(cand[0][:4]), tuple(cand[0][4:]), (k, tuple(cand[k][:4]), tuple(cand[k][4:]))))
        return scores

    def mbr(self, mapper, *, unit='word', posterior=None, scale=1.0):
        """BUILD-DEFINED: minimum-Bayes-risk selection among the hypotheses that the last decode_many / decode_nbest /
        sample call left on the device (last_hyps, last_hyp_scores): per utterance the entry with the lowest expected
        number of errors (unit 'word' | 'char') against the other entries, weighted by the list's own posterior.  ONE
        launch forms the pairwise distances, the posterior, the risks and the choice (ssasr_mbr_select,
        include/ssasr.h).  posterior 'softmax': p_j = softmax(scale * score_j) over the list; 'uniform': every entry
        weighs the same, which is right for draws from the model; None: 'uniform' after sample(), 'softmax' otherwise.
        Returns one MBR(k, text, risk, risks) per utterance; last_mbr keeps (best [N], risk [N, K], pair [N, K, K, 2])
        on the device.  A group past the kernel's limits (more than 1,023 columns, or more than 8,192 over an
        utterance's K rows) is selected by postprocess.mbr_reference on the host, last_mbr then holding its results.
        A call before any decode is a ValueError."""
        if self.last_hyps is None or self.last_hyp_scores is None:
            raise ValueError('mbr: nothing decoded yet (decode_many / decode_nbest / sample leave the hypotheses)')
        if posterior is None:
            posterior = 'uniform' if self.last_hyps_sampled else 'softmax'
        if posterior not in ops.MBR_POSTERIORS:
            raise ValueError("mbr: posterior must be 'softmax', 'uniform' or None, got %r" % (posterior,))
        if unit not in ops.MBR_UNITS:
            raise ValueError("mbr: unit must be 'char' or 'word', got %r" % (unit,))
        chars, n_chars, n_hyps = self.last_hyps
        N, K, steps = chars.shape
        space, first_char = int(mapper.char_to_ind(' ')), TOKENS.index(UNK_TKN)
        rows, lens = chars.cpu().tolist(), n_chars.cpu().tolist()
        hmax = min(steps, max([max(max(r), 0) for r in lens] + [0]))
        if ops.mbr_fits(K, hmax) and N <= 65535:
            self.last_mbr = ops.mbr_select(chars[:, :, :hmax], n_chars, n_hyps, self.last_hyp_scores,
                                           first_char=first_char, space=space, unit=unit, posterior=posterior,
                                           scale=scale)
            best, risk = self.last_mbr[0].cpu().tolist(), self.last_mbr[1].cpu().tolist()
        else:
            hyps = [[rows[i][k][:max(lens[i][k], 0)] for k in range(K)] for i in range(N)]
            best, risk, pair = postprocess.mbr_reference(hyps, n_hyps.cpu().tolist(), self.last_hyp_scores.cpu().tolist(),
                                                         space, first_char, unit, posterior, scale)
            dev = chars.device
            self.last_mbr = (torch.tensor(best, dtype=torch.int32, device=dev).reshape(N),
                             torch.tensor(risk, dtype=torch.float32, device=dev).reshape(N, K),
                             torch.tensor(pair, dtype=torch.int32, device=dev).reshape(N, K, K, 2))
        out = []
        for i, nh in enumerate(n_hyps.cpu().tolist()):
            k = best[i]
            text = ''.join(mapper.ind_to_char(c) for c in rows[i][k][:max(lens[i][k], 0)]) if k >= 0 else ''
            out.append(MBR(k, text, risk[i][k] if k >= 0 else math.inf, tuple(risk[i][:min(max(nh, 0), K)])))
        return out

    def decode_mbr(self, xs, x_lens, rnn_lm, mapper, lm_weight, beam_size, max_decoding_steps=200, *, unit='word',
                   scale=1.0, **nbest_args):
        """decode_nbest (its keywords pass through), then mbr(unit=unit, scale=scale) over each n-best list with the
        softmax of the hypothesis scores as the posterior: returns the N chosen strings, the entries with the lowest
        expected error count, not the highest-scoring ones.  last_beam / last_hyps stay in the beam's order, so
        score() afterwards still scores slot 0, the MAP entry; last_mbr[0] names the chosen slots."""
        self.decode_nbest(xs, x_lens, rnn_lm, mapper, lm_weight, beam_size, max_decoding_steps=max_decoding_steps,
                          **nbest_args)
        return [m.text for m in self.mbr(mapper, unit=unit, posterior='softmax', scale=scale)]

    def decode_many(self, xs, x_lens, rnn_lm, mapper, lm_weight, max_decoding_steps=200, *, beam_size=1,
                    ctc_weight=0.0, length_bonus=0.0, coverage_weight=0.0, coverage_threshold=0.5, end_margin=None,
                    graph=None, graph_weight=0.0):
        """decode() for a list of single utterances in ONE decode launch.  Each utterance is encoded alone
        (blstm_4 recurs over the utterance axis, src/asr.py:237-238, :262: a batched encoder would change every
        transcript); the encoder outputs are packed to [N, T'max, E] and every utterance gets a workgroup of its
        own.  Returns the N strings; last_decode keeps (chars, n_chars, scores, att) on the device.
        beam_size > 1 (at most 32): beam search of that width in one launch (ssasr_decode_beam; no length
        normalisation); returns each utterance's best hypothesis and keeps (chars [N, K, steps], n_chars [N, K],
        hyp_scores [N, K], n_hyps [N]) on the device in last_beam; last_decode is left as it was.
        ctc_weight > 0, a length bonus, a coverage term or end detection on, or a graph at a weight > 0: as
        beam_size > 1, for any beam_size in 1..32 (decode_nbest)."""
        nbest = self.decode_nbest(xs, x_lens, rnn_lm, mapper, lm_weight, beam_size,
                                  max_decoding_steps=max_decoding_steps, ctc_weight=ctc_weight,
                                  length_bonus=length_bonus, coverage_weight=coverage_weight,
                                  coverage_threshold=coverage_threshold, end_margin=end_margin, graph=graph,
                                  graph_weight=graph_weight)
        return [hyps[0][0] for hyps in nbest]

    def _decode_args(self, packed, enc_lens, lm, lm_weight, mapper_or_eos, max_steps):
        """What every decode entry of ops takes first: the encoded group, the decoder's and psi's parameters, the
        language model and its weight, <EOS> (an index, or the mapper that knows it) and the step cap."""
        eos = mapper_or_eos if isinstance(mapper_or_eos, int) else mapper_or_eos.char_to_ind(EOS_TKN)
        return (packed, enc_lens, self._decoder_params(), (self.attention.psi.weight, self.attention.psi.bias), lm,
                lm_weight, eos, max_steps)

    def _keep_hyps(self, chars, n_chars, n_hyps, scores, sampled):
        """What score() and mbr() read: the last call's hypotheses [N, K, steps], [N, K], [N] and scores [N, K]."""
        self.last_hyps = (chars, n_chars, n_hyps)
        self.last_hyp_scores, self.last_hyps_sampled = scores, sampled

    @staticmethod
    def _texts(chars, n_chars, n_hyps, scores, mapper):
        """Per utterance the list of (text, score) of its first n_hyps[i] (a tensor [N], or one count for all) slots."""
        chars, n_chars, scores = [t.cpu().tolist() for t in (chars, n_chars, scores)]
        n_hyps = [n_hyps] * len(chars) if isinstance(n_hyps, int) else n_hyps.cpu().tolist()
        return [[(''.join(mapper.ind_to_char(c) for c in chars[i][k][:n_chars[i][k]]), scores[i][k])
                 for k in range(n_hyps[i])] for i in range(len(chars))]

    def decode_nbest(self, xs, x_lens, rnn_lm, mapper, lm_weight, beam_size, max_decoding_steps=200, *,
                     ctc_weight=0.0, length_bonus=0.0, coverage_weight=0.0, coverage_threshold=0.5, end_margin=None,
                     graph=None, graph_weight=0.0):
        """Beam search over a list of single utterances in ONE launch: per utterance the list of (text, score),
        best first, score = the sum of the chosen characters' log_softmax(speller) + lm_weight *
        log_softmax(rnn_lm) entries (<EOS>'s included when it ended the hypothesis; no length normalisation).
        beam_size 1 is greedy decoding (ssasr_decode_greedy, last_decode); beam_size 2 .. 32 sets last_beam.
        ctc_weight in (0, 1] (a model with a ctc_head): joint CTC / attention decoding, ssasr_decode_beam_ctc for
        any beam_size in 1..32 (width 1 is the beam kernel at K = 1); a character's score entry is then
        (1 - ctc_weight) * log_softmax(speller) + ctc_weight * (the CTC prefix score's increase) + lm_weight *
        log_softmax(rnn_lm), and characters that the utterance's frames cannot hold are never chosen.  Sets
        last_beam.  ctc_weight 0 is the path above exactly.
        length_bonus (beta, added per character), coverage_weight / coverage_threshold (eta times the number of
        frames whose summed attention exceeds the threshold) and end_margin (None: off; delta >= 0: the loop ends once
        the best live score is below the best finished one by more than delta, the live prefixes being dropped) are
        the terms of ssasr_decode_beam_ex (include/ssasr.h).  With any of them on, any beam_size in 1..32 runs the
        beam kernel (width 1 is the beam kernel at K = 1), last_beam is set and last_beam_steps keeps n_steps [N],
        the loop iterations each utterance executed.  With all at their defaults every call takes the path above
        exactly.
        graph / graph_weight: a char_graph.CharGraph (an n-gram LM, hotwords, their product) INSIDE the beam search
        (ssasr_decode_beam_graph, include/ssasr.h; graph_weight finite and >= 0): a candidate character gains
        graph_weight * arc[state][character], <EOS> gains graph_weight * fin[state], and a forbidden arc is never
        taken.  With a graph at a weight > 0 any beam_size in 1..32 runs the beam kernel (width 1 is the beam kernel at
        K = 1), last_beam and last_beam_steps are set and last_beam_graph keeps graph_scores [N, K], each hypothesis'
        graph part G (+ fin when <EOS> ended it); every other call sets last_beam_graph to None.  With graph None or
        graph_weight 0 every call takes the path it takes without the keywords exactly."""
        beam_size = int(beam_size)
        if not 1 <= beam_size <= ops.MAX_BEAM:
            raise ValueError('beam_size must be in 1..%d, got %d' % (ops.MAX_BEAM, beam_size))
        ctc = self._ctc_head(ctc_weight)
        terms = self._beam_terms(length_bonus, coverage_weight, coverage_threshold, end_margin)
        graph_weight = self._beam_graph_weight(graph, graph_weight)
        with torch.no_grad():
            packed, enc_lens = self._encode_packed(xs, x_lens)
            args = self._decode_args(packed, enc_lens, rnn_lm, lm_weight, mapper, max_decoding_steps)
            self.last_beam_graph = None
            if graph_weight != 0.0:
                out = ops.decode_beam_graph(*args, beam_size, ctc, graph=graph, graph_weight=graph_weight,
                                            **(terms or {}))
                self.last_beam, self.last_beam_steps, self.last_beam_graph = out[:4], out[4], out[5]
                hyps = (self.last_beam[0], self.last_beam[1], self.last_beam[3], self.last_beam[2])
            elif beam_size == 1 and ctc is None and terms is None:
                self.last_decode = ops.decode_greedy(*args)
                chars, n_chars, scores, _ = self.last_decode
                # the transcript's score: the chosen entries of the executed steps, <EOS>'s too
                taken = torch.gather(scores, 2, chars.long().unsqueeze(2)).squeeze(2)
                executed = torch.clamp(n_chars + 1, max=max_decoding_steps).unsqueeze(1)
                mask = torch.arange(chars.shape[1], device=chars.device).unsqueeze(0) < executed
                hyps = (chars.unsqueeze(1), n_chars.unsqueeze(1), torch.ones_like(n_chars),
                        (taken * mask).sum(1, keepdim=True))
            else:
                if terms is not None:
                    out = ops.decode_beam_ex(*args, beam_size, ctc, **terms)
                    self.last_beam, self.last_beam_steps = out[:4], out[4]
                else:
                    self.last_beam = (ops.decode_beam(*args, beam_size) if ctc is None else
                                      ops.decode_beam_ctc(*args, beam_size, ctc))
                hyps = (self.last_beam[0], self.last_beam[1], self.last_beam[3], self.last_beam[2])
            self._keep_hyps(*hyps, sampled=False)
        return self._texts(*hyps, mapper)

    def decode_ctc(self, xs, x_lens, mapper, *, beam_size=8, rnn_lm=None, lm_weight=0.0, length_bonus=0.0, graph=None,
                   graph_weight=0.0, word_graph=None):
        """BUILD-DEFINED: transcripts from the ctc_head's posteriors alone, for a list of single utterances in ONE
        launch with no Speller step (ssasr_ctc_decode, include/ssasr.h): per utterance the list of (text, score), best
        first.  beam_size 0: the best path (per frame the most probable class, repeats merged, blanks removed; score =
        the path's log-probability); 1 .. 32: CTC prefix beam search of that width, score = the log-probability that
        the search found for the text.  Each utterance is encoded alone, as in decode_nbest.  last_ctc_decode keeps
        (chars [N, Kr, T'], n_chars [N, Kr], scores [N, Kr], n_hyps [N], logits [N, T', V]) on the device, Kr =
        max(beam_size, 1); last_hyps is set, so score(), mbr() and align() follow it as they follow decode_nbest.
        rnn_lm / lm_weight / length_bonus: CharLM shallow fusion INSIDE the prefix search (ssasr_ctc_decode_lm,
        include/ssasr.h; beam_size >= 1): a text is ranked by its CTC score + lm_weight * log P_lm(text) + length_bonus
        * len(text) at every frame, and by that + lm_weight * log P_lm(<EOS> | text) at the end.  The score returned
        (and last_hyp_scores) is then the fused total, and last_ctc_decode gains two tensors [N, K] after the logits:
        the CTC part and the LM part.  With both weights 0 (the default) the call is the one above exactly.
        graph / graph_weight: a char_graph.CharGraph (an n-gram LM, hotwords, their product) INSIDE the prefix search
        (ssasr_ctc_decode_graph, include/ssasr.h; beam_size >= 1, graph_weight finite and >= 0): a text is ranked by its
        CTC score + graph_weight * G(text) + length_bonus * len(text) at every frame, and by that + graph_weight *
        fin[state(text)] at the end; last_ctc_decode gains the CTC part and the graph part (G + fin) after the logits.
        At graph_weight 0 the graph plays no part.  Together with rnn_lm at a non-zero lm_weight it is a ValueError:
        the two terms in one search are not built.
        word_graph: a word_graph.WordGraph in place of `graph` (ssasr_ctc_decode_word, include/ssasr.h): the texts are
        restricted to the words of its lexicon and ranked with its word n-gram LM at graph_weight, G and fin being the
        word graph's; last_ctc_decode gains the same two tensors.  Together with `graph`, or with rnn_lm at a non-zero
        lm_weight, it is a ValueError."""
        head = getattr(self, 'ctc_head', None)
        if head is None:
            raise ValueError(self._NO_CTC_HEAD % type(self).__name__)
        if isinstance(beam_size, bool) or not isinstance(beam_size, int) or not 0 <= beam_size <= ops.CTC_DECODE_MAX_BEAM:
            raise ValueError('beam_size must be an integer in 0..%d, got %r' % (ops.CTC_DECODE_MAX_BEAM, beam_size))
        if len(xs) != len(x_lens) or not len(xs):
            raise ValueError('decode_ctc: %d utterances, %d lengths' % (len(xs), len(x_lens)))
        fused = self._ctc_lm_terms(rnn_lm, lm_weight, length_bonus, beam_size)
        if word_graph is not None and graph is not None:
            raise ValueError('decode_ctc: graph and word_graph in one search are not built; give one of them')
        graph_weight = self._ctc_graph_weight(graph, graph_weight, fused, beam_size, word_graph)
        if word_graph is not None:
            graph = word_graph
        if graph_weight != 0.0 and graph.n_classes != head.weight.shape[0]:
            raise ValueError('decode_ctc: the graph has %d classes, the ctc_head %d'
                             % (graph.n_classes, head.weight.shape[0]))
        with torch.no_grad():
            packed, enc_lens = self._encode_packed(xs, x_lens)
            if graph_weight != 0.0:
                decode = ops.ctc_head_decode_graph if word_graph is None else ops.ctc_head_decode_word
                out = decode(packed, head.weight, head.bias, enc_lens, beam_size, graph, graph_weight,
                             float(length_bonus), ops.CTC_BLANK)
                self.last_ctc_decode = tuple(out[k] for k in ('chars', 'n_chars', 'scores', 'n_hyps', 'logits',
                                                              'ctc_scores', 'graph_scores'))
            elif fused is None:
                self.last_ctc_decode = ops.ctc_head_decode(packed, head.weight, head.bias, enc_lens, beam_size,
                                                           ops.CTC_BLANK)
            else:
                out = ops.ctc_head_decode_lm(packed, head.weight, head.bias, enc_lens, beam_size, rnn_lm, *fused,
                                             int(mapper.char_to_ind(EOS_TKN)), ops.CTC_BLANK)
                self.last_ctc_decode = tuple(out[k] for k in ('chars', 'n_chars', 'scores', 'n_hyps', 'logits',
                                                              'ctc_scores', 'lm_scores'))
            chars, n_chars, scores, n_hyps = self.last_ctc_decode[:4]
            self._keep_hyps(chars, n_chars, n_hyps, scores, sampled=False)
        return self._texts(chars, n_chars, n_hyps, scores, mapper)

    @staticmethod
    def _ctc_lm_terms(rnn_lm, lm_weight, length_bonus, beam_size):
        """decode_ctc's fusion keywords checked: None when both weights are 0 (the plain search), else (lm_weight,
        length_bonus) as floats."""
        terms = []
        for name, value in (('lm_weight', lm_weight), ('length_bonus', length_bonus)):
            if isinstance(value, bool) or not isinstance(value, (int, float)) or not math.isfinite(value):
                raise ValueError('decode_ctc: %s must be a finite number, got %r' % (name, value))
            terms.append(float(value))
        if terms == [0.0, 0.0]:
            return None
        if terms[0] != 0.0 and rnn_lm is None:
            raise ValueError('decode_ctc: lm_weight %g needs rnn_lm' % terms[0])
        if beam_size < 1:
            raise ValueError('decode_ctc: beam_size 0, the best path, has no LM term or length bonus; use beam_size >= 1')
        return tuple(terms)

    @staticmethod
    def _ctc_graph_weight(graph, graph_weight, fused, beam_size, word_graph=None):
        """decode_ctc's graph keywords checked against the rest (fused: _ctc_lm_terms' result; word_graph: given in
        place of graph): the weight as a float, 0.0 when no graph term runs."""
        from .char_graph import CharGraph
        from .word_graph import WordGraph
        if isinstance(graph_weight, bool) or not isinstance(graph_weight, (int, float)) or \
                not (math.isfinite(graph_weight) and graph_weight >= 0.0):
            raise ValueError('decode_ctc: graph_weight must be a finite number >= 0, got %r' % (graph_weight,))
        if graph is not None and not isinstance(graph, CharGraph):
            raise ValueError('decode_ctc: graph must be a char_graph.CharGraph, got %s' % type(graph).__name__)
        if word_graph is not None and not isinstance(word_graph, WordGraph):
            raise ValueError('decode_ctc: word_graph must be a word_graph.WordGraph, got %s' % type(word_graph).__name__)
        if graph_weight == 0.0:
            return 0.0
        if graph is None and word_graph is None:
            raise ValueError('decode_ctc: graph_weight %g needs graph' % graph_weight)
        if beam_size < 1:
            raise ValueError('decode_ctc: beam_size 0, the best path, has no graph term; use beam_size >= 1')
        if fused is not None and fused[0] != 0.0:
            raise ValueError('decode_ctc: a graph and rnn_lm at lm_weight %g in one search are not built; give one of them'
                             % fused[0])
        return float(graph_weight)

    def rescore(self, mapper, *, rnn_lm=None, lm_weight=0.0, att_weight=1.0, first_weight=0.0, length_bonus=0.0):
        """BUILD-DEFINED: attention rescoring of the list that the last decode_nbest / decode_ctc / sample call left on
        the device (last_hyps, last_hyp_scores), on that call's encoder output (last_encoded_packed: no second encode).
        The K texts of every utterance are teacher-forced through the Speller (and, with rnn_lm and lm_weight != 0,
        the CharLM), and one launch scores, ranks and reorders each list (ops.rescore; ssasr_rescore, include/ssasr.h):
          total = att_weight * log P_speller(text, <EOS>) + lm_weight * log P_lm(text, <EOS>)
                  + first_weight * (the first pass's score) + length_bonus * len(text).
        Returns per utterance the list of (text, total), best first.  last_rescore keeps (order, total, parts) on the
        device; the list is re-kept in rank order with `total` as its scores (the sampled flag unchanged), so score(),
        mbr() and align() follow it.  A call before any decode, a non-finite weight, or all four weights zero is a
        ValueError."""
        if self.last_hyps is None or self.last_hyp_scores is None or self.last_encoded_packed is None:
            raise ValueError('rescore: nothing decoded yet (decode_nbest / decode_ctc / sample leave the hypotheses)')
        weights = dict(att_weight=att_weight, lm_weight=lm_weight, first_weight=first_weight, length_bonus=length_bonus)
        for name, value in weights.items():
            weights[name] = float(value)
            if not math.isfinite(weights[name]):
                raise ValueError('rescore: %s must be finite, got %r' % (name, value))
        if not any(weights.values()):
            raise ValueError('rescore: att_weight, lm_weight, first_weight and length_bonus are all zero')
        chars, n_chars, n_hyps = self.last_hyps
        packed, enc_lens = self.last_encoded_packed
        if packed.shape[0] != chars.shape[0]:
            raise ValueError('rescore: the encoded group holds %d utterances, the list %d'
                             % (packed.shape[0], chars.shape[0]))
        with torch.no_grad():
            order, total, parts, chars, n_chars, n_hyps = ops.rescore(
                packed, enc_lens, self._decoder_params(), (self.attention.psi.weight, self.attention.psi.bias),
                chars, n_chars, n_hyps, self.last_hyp_scores, int(mapper.char_to_ind(EOS_TKN)), rnn_lm, **weights)
        self.last_rescore = (order, total, parts)
        self._keep_hyps(chars, n_chars, n_hyps, total, sampled=self.last_hyps_sampled)
        return self._texts(chars, n_chars, n_hyps, total, mapper)

    def decode_two_pass(self, xs, x_lens, rnn_lm, mapper, lm_weight, *, beam_size=8, ctc_weight=0.3, length_bonus=0.0,
                        first_lm_weight=0.0):
        """BUILD-DEFINED: two-pass decoding on a model with a ctc_head: decode_ctc(beam_size >= 1), the CTC prefix beam
        search with no Speller step, then rescore() of its list with att_weight = 1 - ctc_weight, first_weight =
        ctc_weight and the CharLM at lm_weight -- decode_nbest's joint weighting applied to whole texts.  ctc_weight in
        [0, 1].  Returns per utterance the list of (text, total), best first; last_ctc_decode keeps the first pass,
        last_rescore the second.  first_lm_weight > 0: the first pass searches with the CharLM at that weight
        (decode_ctc's rnn_lm / lm_weight), so a text the LM favours is still in the list; rescore() then takes the
        first pass's pure CTC part as its `first` score, and the final total counts the LM once."""
        if isinstance(ctc_weight, bool) or not isinstance(ctc_weight, (int, float)) or not 0.0 <= ctc_weight <= 1.0:
            raise ValueError('ctc_weight must be a number in [0, 1], got %r' % (ctc_weight,))
        if isinstance(beam_size, bool) or not isinstance(beam_size, int) or not 1 <= beam_size <= ops.CTC_DECODE_MAX_BEAM:
            raise ValueError('beam_size must be an integer in 1..%d, got %r' % (ops.CTC_DECODE_MAX_BEAM, beam_size))
        if isinstance(first_lm_weight, bool) or not isinstance(first_lm_weight, (int, float)) or \
                not (math.isfinite(first_lm_weight) and first_lm_weight >= 0.0):
            raise ValueError('first_lm_weight must be a finite number >= 0, got %r' % (first_lm_weight,))
        if first_lm_weight > 0.0 and rnn_lm is None:
            raise ValueError('first_lm_weight %g needs rnn_lm' % first_lm_weight)
        self.decode_ctc(xs, x_lens, mapper, beam_size=beam_size, rnn_lm=rnn_lm if first_lm_weight > 0.0 else None,
                        lm_weight=float(first_lm_weight))
        if first_lm_weight > 0.0:
            self.last_hyp_scores = self.last_ctc_decode[5]      # the CTC part: the LM enters the total in rescore()
        return self.rescore(mapper, rnn_lm=rnn_lm, lm_weight=lm_weight, att_weight=1.0 - float(ctc_weight),
                            first_weight=float(ctc_weight), length_bonus=length_bonus)

    def sample(self, xs, x_lens, mapper, n_samples, *, temperature=1.0, rnn_lm=None, lm_weight=0.0,
               max_decoding_steps=200, generator=None, uniforms=None):
        """BUILD-DEFINED: n_samples (1 .. 32) transcripts per utterance DRAWN from the model's own distribution, for a
        list of single utterances in ONE launch (ssasr_decode_sample, include/ssasr.h): every step draws a character
        from softmax(score row / temperature), the score row being log_softmax(speller) + lm_weight *
        log_softmax(rnn_lm); a drawn <EOS> ends a sample.  Each utterance is encoded alone, as in decode_nbest.  The
        uniforms [N, n_samples, max_decoding_steps] come from torch.rand on the device (`generator`: a device
        torch.Generator, for reproducible draws) unless `uniforms` is given.  Returns per utterance the list of
        (text, score) in SLOT order (unsorted; score as decode_nbest's).  last_samples keeps (chars, n_chars,
        hyp_scores, n_hyps, logq) on the device; last_hyps is set, so score() scores the samples: its chars / words
        are slot 0's and its oracle entry is the best of the draws."""
        n_samples = int(n_samples)
        if not 1 <= n_samples <= ops.MAX_BEAM:
            raise ValueError('n_samples must be in 1..%d, got %d' % (ops.MAX_BEAM, n_samples))
        temperature = float(temperature)
        if not (math.isfinite(temperature) and temperature > 0.0):
            raise ValueError('temperature must be finite and > 0, got %r' % (temperature,))
        with torch.no_grad():
            packed, enc_lens = self._encode_packed(xs, x_lens)
            shape = (packed.shape[0], n_samples, int(max_decoding_steps))
            if uniforms is None:
                uniforms = torch.rand(shape, device=packed.device, dtype=torch.float32, generator=generator)
            elif tuple(uniforms.shape) != shape:
                raise ValueError('sample: uniforms must be %r, got %r' % (shape, tuple(uniforms.shape)))
            self.last_samples = ops.decode_sample(
                *self._decode_args(packed, enc_lens, rnn_lm, lm_weight, mapper, max_decoding_steps), n_samples,
                uniforms.to(device=packed.device, dtype=torch.float32), temperature)
            chars, n_chars, hyp_scores, n_hyps, _ = self.last_samples
            self._keep_hyps(chars, n_chars, n_hyps, hyp_scores, sampled=True)
        return self._texts(chars, n_chars, n_samples, hyp_scores, mapper)
