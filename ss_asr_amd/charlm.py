"""Character language model with the nn.Module surface of the reference's ``src/charlm.py`` (CharLM :5-61):
the same constructor, ``state_dict`` names, order and shapes (``emb.weight``, ``layer_1.*``, ``layer_2.*``,
``out.*``), so a reference-trained checkpoint loads strictly.  The nn.Embedding / nn.GRUCell / nn.Linear held
here are parameter containers only; ``forward`` computes through ``ssasr_charlm_step`` (csrc/infer.hip), and
``ASR.decode`` fuses the same step into its decode launch (``ssasr_decode_greedy``).  ``forward`` itself carries
no autograd graph: training runs a whole chunk through ``ssasr_charlm_train_fwd`` / ``_bwd``
(csrc/charlm_train.hip, ops.charlm_chunk, engine.CharLMTrainStep), driven by ``trainer.CHARLMTrainer``."""
import torch
import torch.nn as nn

from . import ops


class CharLM(nn.Module):
    def __init__(self, input_size, hidden_size):
        super().__init__()
        self.input_size = input_size
        self.hidden_size = hidden_size
        self.emb = nn.Embedding(input_size, hidden_size)
        self.layer_1 = nn.GRUCell(input_size=hidden_size, hidden_size=hidden_size)
        self.layer_2 = nn.GRUCell(input_size=hidden_size, hidden_size=hidden_size)
        self.out = nn.Linear(hidden_size, input_size)

    def forward(self, x, h_1, h_2):
        """x: [batch] character ids; h_1, h_2: [batch, hidden] -> (out [batch, input_size], (h_1, h_2));
        src/charlm.py:46-57."""
        out, h_1, h_2 = ops.charlm_step(self, x, h_1, h_2)
        return out, (h_1, h_2)

    def init_hidden(self, batch_size, device):
        return (torch.zeros(batch_size, self.hidden_size).to(device),
                torch.zeros(batch_size, self.hidden_size).to(device))
