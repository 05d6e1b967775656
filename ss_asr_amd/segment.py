"""BUILD-DEFINED: from a segmented recording to training utterances.  ASR.segment places a running transcript inside
a long recording (ssasr_ctc_segment, include/ssasr.h); write_segments cuts the recording's feature matrix at the
utterances it found and appends them to an index that ASRDataset loads.  Host code only."""
import collections
import csv
import os

import numpy as np

from .ASRDataset import COLUMNS
from .preprocess import EOS_TKN, SOS_TKN, zero_pad

# what write_segments did with one utterance: the Segment, its index row as a dict (None when dropped)
Written = collections.namedtuple('Written', ('segment', 'row'))


class WrittenSegments(tuple):
    """write_segments' result: the pair (kept, dropped), which unpacks and compares as that tuple, and `skipped`: how
    many of the dropped utterances the segmentation had passed over as never spoken."""

    def __new__(cls, kept, dropped, skipped=0):
        self = super().__new__(cls, (kept, dropped))
        self.skipped = skipped
        return self


def write_segments(segmentation, fbank, out_dir, index_path, *, min_confidence, name, pad_to=None):
    """Cuts fbank [frames, features], the recording that `segmentation` (one ASR.segment result, spans in INPUT
    frames, i.e. made without frame_shift) belongs to, at every utterance whose confidence is >= min_confidence:
    rows [start, end) go to out_dir/<name>_<k>.npy (k: the utterance's place in the transcript, four digits), zero-
    padded to pad_to rows (default: the longest kept slice of this call) in float64, as the corpus files are, so that
    a batch of them stacks.  One row per kept utterance is APPENDED to index_path in ASRDataset.COLUMNS order, written
    as preprocess.sort_index writes (tab separated, minimal quoting, '\\n' line ends): normalized_text = '<' + text +
    '>', s_len = its length (normalize_string's count: the text's characters + 2), unpadded_num_frames = end - start,
    text_fname 'na', wav_fname = <name>_<k>.wav.  A recording that could not be segmented (utterances None) keeps
    nothing.  An utterance that ASR.segment passed over (skipped True: it was never spoken) is never written and has
    no span to check; it is counted among the dropped ones, and the result's `skipped` is their number.
    -> (kept, dropped): lists of Written(segment, row), row None for the dropped ones; the pair is a WrittenSegments,
    a tuple that also carries `skipped`."""
    fbank = np.asarray(fbank)
    if fbank.ndim != 2:
        raise ValueError('write_segments: fbank must be [frames, features], got %r' % (fbank.shape,))
    utterances = segmentation.utterances or []
    kept, dropped = [], []
    for k, seg in enumerate(utterances):
        if getattr(seg, 'skipped', False):
            dropped.append((k, seg))
            continue
        if isinstance(seg.start, float) or isinstance(seg.end, float):
            raise ValueError('write_segments: spans must be in input frames (ASR.segment without frame_shift)')
        if not 0 <= seg.start < seg.end <= fbank.shape[0]:
            raise ValueError('write_segments: span [%d, %d) lies outside the %d frames of the recording'
                             % (seg.start, seg.end, fbank.shape[0]))
        (kept if seg.confidence >= min_confidence else dropped).append((k, seg))
    if pad_to is None:
        pad_to = max([seg.end - seg.start for _, seg in kept], default=0)
    if any(seg.end - seg.start > pad_to for _, seg in kept):
        raise ValueError('write_segments: pad_to %d is shorter than a kept utterance' % pad_to)
    os.makedirs(out_dir, exist_ok=True)
    rows = []
    for k, seg in kept:
        stem = '%s_%04d' % (name, k)
        path = os.path.join(out_dir, stem + '.npy')
        np.save(path, zero_pad(fbank[seg.start:seg.end], pad_to))
        text = SOS_TKN + seg.text + EOS_TKN
        rows.append(dict(zip(COLUMNS, [text, path, len(text), seg.end - seg.start, 'na', stem + '.wav'])))
    with open(index_path, 'a', encoding='utf-8', newline='') as f:
        w = csv.writer(f, delimiter='\t', quoting=csv.QUOTE_MINIMAL, lineterminator='\n')
        for r in rows:
            w.writerow([r[c] for c in COLUMNS])
    return WrittenSegments([Written(seg, r) for (_, seg), r in zip(kept, rows)], [Written(seg, None) for _, seg in dropped],
                           sum(1 for _, seg in dropped if getattr(seg, 'skipped', False)))
