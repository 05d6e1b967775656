"""The language model's text dataset with the surface of the reference's ``src/LMDataset.py`` (LMDataset :5-76,
load_lm_dataset :78-85): item i is the chunk ``file[i : i + chunk_size + 1]`` for i < len(file) // chunk_size,
returned as ((x_text, y_text), (one-hot or label x, label y)); a character outside TOKENS + ALL_CHARS is a KeyError.

For training the file's ids live on the device once (``ResidentLMLoader``): a batch's label matrix y is ONE index
op over them, and no one-hot x is built -- CHARLMTrainer never reads it (src/trainer.py:225-246 uses y alone).
The set of chunks and drop_last are the reference's (DataLoader(ds, batch_size, shuffle, drop_last=True)); the
shuffle order is torch.randperm's, not the DataLoader sampler's."""
import torch
from torch.utils.data import DataLoader, Dataset

from .preprocess import ALL_CHARS, EOS_TKN, SOS_TKN, TOKENS  # noqa: F401


class LMDataset(Dataset):
    def __init__(self, filename=None, chunk_size=0, chars: str = TOKENS + ALL_CHARS, label_format=False):
        self.label_format = label_format
        self.file = None
        self.len_file = 0
        if filename is not None:
            with open(filename) as f:
                self.file = f.read()
            self.len_file = len(self.file)
        self.chunk_size = chunk_size
        self.chars = chars
        self.char2idx = {chars[i]: i for i in range(len(chars))}
        self.idx2char = {v: k for k, v in self.char2idx.items()}
        self.device = torch.device('cuda') if torch.cuda.is_available() else torch.device('cpu')

    def s2l(self, s):
        """The label-index tensor (float, as the reference's) of a string."""
        assert type(s) == str
        return torch.tensor([self.char2idx[ch] for ch in s], dtype=torch.float32).reshape(len(s))

    def s2oh(self, s):
        """The one-hot tensor [len, chars] of a string (labels with label_format)."""
        if self.label_format:
            return self.s2l(s)
        out = torch.zeros(len(s), self.get_num_chars())
        for i in range(len(s)):
            out[i, self.char2idx[s[i]]] = 1
        return out

    def get_num_chars(self):
        return len(self.chars)

    def __len__(self):
        return int(self.len_file / self.chunk_size)

    def __getitem__(self, i):
        chunk = self.file[i: i + self.chunk_size + 1]
        return (chunk[:-1], chunk[1:]), (self.s2oh(chunk[:-1]).to(self.device), self.s2l(chunk[1:]).to(self.device))

    def ids(self):
        """int64 ids of the whole file (KeyError for a foreign character)."""
        return torch.tensor([self.char2idx[ch] for ch in self.file], dtype=torch.int64)


class ResidentLMLoader:
    """The training batches of load_lm_dataset(..., drop_last=True) without the per-item work: iterating yields
    ((None, None), (None, y)) with y int64 [batch_size, chunk_size] on `device`, row j of a batch being the labels
    of item i_j, file[i_j + 1 : i_j + chunk_size + 1].  Items whose chunk runs off the end of the file (the
    reference's DataLoader would fail to stack them) cannot occur: i < len // chunk means i + chunk + 1 <= len
    whenever chunk >= 2 or the file is longer than one chunk; a file too short for that raises here."""

    def __init__(self, ds, batch_size, shuffle=True, device=None):
        self.ds, self.batch_size, self.shuffle = ds, int(batch_size), shuffle
        self.device = torch.device(device) if device is not None else ds.device
        n = len(ds)
        if n and n - 1 + ds.chunk_size + 1 > ds.len_file:
            raise ValueError('the last chunk runs past the end of the text (file too short for chunk_size)')
        self.ids = ds.ids().to(self.device)
        self.offsets = torch.arange(1, ds.chunk_size + 1, device=self.device)

    def __len__(self):
        return len(self.ds) // self.batch_size

    def item_order(self):
        n = len(self.ds)
        return torch.randperm(n) if self.shuffle else torch.arange(n)

    def __iter__(self):
        order = self.item_order().to(self.device)
        for k in range(len(self)):
            start = order[k * self.batch_size:(k + 1) * self.batch_size]
            yield (None, None), (None, self.ids[start[:, None] + self.offsets[None, :]])


def load_lm_dataset(filename, chunk_size, batch_size, shuffle=True, label_format=False, resident=False):
    """(dataset, loader); the loader yields batch-first batches, x.shape = [batch_size, chunk_size].
    resident=True: the device-resident loader the trainer uses."""
    ds = LMDataset(filename, chunk_size, label_format=label_format)
    if resident:
        return ds, ResidentLMLoader(ds, batch_size, shuffle=shuffle)
    return ds, DataLoader(ds, batch_size=batch_size, shuffle=shuffle, drop_last=True)
