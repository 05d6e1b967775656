"""The epoch loop and close() of ASRTrainer, TAETrainer, ADVTrainer and SAETrainer as ordered event lists.

Each trainer is built on the CPU (Solver.__init__ only), given a stub train step, stub models, four in-memory
batches and two epochs, with logging_step 2, valid_step 3 and save_step 5: over the global steps 0 .. 7 every
action fires alone (2, 3, 5), all three fire together (0), two do (6), and none does (1, 7).  The stub reports one
skipped update in its sixth call.  What is asserted is everything exec() and close() do that can be seen from outside,
in order: the batch each step was given, every logged scalar with its value and step, valid(), finish(), every
checkpoint with its path, every line printed without a carriage return, the tracker's step, and the barrier.
`expected` spells the list out; it was first checked against the four hand-written loops that the shared loop
replaced, and what differs between the trainers is an argument of it."""
import os
import types

import pytest
import torch

from ss_asr_amd import dist as sdist
from ss_asr_amd import trainer as trainer_mod

B, T, F, L, V = 2, 4, 3, 6, 50
LABELS = torch.tensor([[3, 10, 11, 12, 1, 0], [3, 13, 14, 1, 0, 0]])     # prepare_y: lengths 6 and 5, ans_len 5


class Model:
    """Stands for a module at a checkpoint: its state dict names it."""

    def __init__(self, name):
        self.name = name

    def state_dict(self):
        return {'model': self.name}


class Step:
    """A train step as the loops see it: called with device tensors, `skipped_steps`, `finish()`.  `unpack` picks the
    batch's number (planted in the data) out of the call's arguments, `result` makes the return value of it."""

    def __init__(self, events, unpack, result):
        self.events, self.unpack, self.result = events, unpack, result
        self.calls = self.skipped_steps = 0
        self.last_logits = self.last_risk = None

    def __call__(self, *args):
        b = self.unpack(self, *args)
        self.events.append(('step', b))
        self.calls += 1
        if self.calls == 6:
            self.skipped_steps += 1
        return self.result(b)

    def finish(self):
        self.events.append(('finish',))


def fbank_batches():
    """Four (x [1, B, T, F], y [1, B, L]) batches; batch b's features are all b + 1."""
    return [(torch.full((1, B, T, F), b + 1.0), LABELS.unsqueeze(0)) for b in range(4)]


def batch_of(x):
    return int(x.flatten()[0]) - 1


def loss_of(b):
    return torch.tensor(0.5 + b)


def asr_unpack(step, x, y, x_lens, ans_len):
    assert x.shape == (B, T, F) and x_lens == [T, T] and ans_len == L - 1 and torch.equal(y, LABELS)
    step.last_logits = torch.nn.functional.one_hot(y[:, 1:ans_len + 1], V).float()
    if batch_of(x) == 2:                           # batch 2: one wrong character of the first row's four
        step.last_logits[0, 0] = step.last_logits[0, 1]
    return batch_of(x)


def mwer_unpack(step, x, y, x_lens):
    step.last_risk = torch.tensor([1.0, 2.0]) * (batch_of(x) + 1)
    right = torch.nn.functional.one_hot(y[:, 1:], V).float()
    step.last_logits = torch.zeros(B * 3, L + 1, V)                  # K = 2: rows 2 and 5 are the references'
    step.last_logits[2::3, :L - 1] = right
    return batch_of(x)


def tae_unpack(step, y, y_noise, y_lens, noise_lens):
    assert y_lens == [6, 5] and noise_lens == [5, 5] and torch.equal(y, LABELS)
    return int(y_noise[0, 0]) - 20


def adv_unpack(step, x, x_lens, y):
    assert x_lens == [T, T] and torch.equal(y, LABELS)
    return batch_of(x)


def sae_unpack(step, x, x_lens):
    assert x_lens == [T, T]
    return batch_of(x)


def make(kind, tmp_path, monkeypatch, rank=0, world=1):
    """-> (trainer ready for exec(), its event list)."""
    events = []
    module = {'asr': 'asr', 'mwer': 'asr', 'tae': 'tae', 'adv': 'adv', 'sae': 'sae'}[kind]
    cls = {'asr': trainer_mod.ASRTrainer, 'tae': trainer_mod.TAETrainer, 'adv': trainer_mod.ADVTrainer,
           'sae': trainer_mod.SAETrainer}[module]
    config = {module: {'logging_step': 2, 'valid_step': 3, 'save_step': 5, 'n_epochs': 2}}
    paras = types.SimpleNamespace(name='t', logdir=os.path.join(str(tmp_path), 'runs'),
                                  ckpdir=os.path.join(str(tmp_path), 'result'), verbose=True, seed=1)
    monkeypatch.setattr(trainer_mod, 'print', lambda *a, **kw: None, raising=False)
    tr = cls(config, paras)
    tr.rank, tr.world = rank, world
    tr.device = torch.device('cpu')                # (the stubs take host tensors, whatever the machine has)

    def record_print(msg, end='\n'):
        if end == '\n':                            # (the carriage-return progress lines are not pinned)
            events.append(('print', msg))
    monkeypatch.setattr(trainer_mod, 'print', record_print, raising=False)
    monkeypatch.setattr(sdist, 'save_atomic',
                        lambda obj, path: events.append(('save', obj['model'], os.path.basename(path))))
    monkeypatch.setattr(sdist, 'barrier', lambda: events.append(('barrier',)))
    tr.lg = types.SimpleNamespace(scalar=lambda tag, val, step: events.append(('scalar', tag, round(float(val), 6), step)))
    tr.valid = lambda: events.append(('valid', tr.tr.step))
    do_step = tr.tr.do_step

    def recorded_do_step():
        do_step()
        events.append(('do_step', tr.tr.step))
    tr.tr.do_step = recorded_do_step

    tr.asr_model = Model('asr')
    tr.asrpath_out = os.path.join(tr.ckpdir, 'asr_out.cpt')
    tr.train_set = fbank_batches()
    if module == 'asr':
        from ss_asr_amd.ASRDataset import Mapper
        tr.mapper, tr.wer_step, tr.gpu_loader = Mapper(), 4, None
        if kind == 'mwer':
            tr.mwer = {'beam_size': 2}
            tr.train_step = Step(events, mwer_unpack, loss_of)
        else:
            tr.train_step = Step(events, asr_unpack, loss_of)
    elif kind == 'tae':
        noised = LABELS[:, :4]
        tr.train_set = [(LABELS.unsqueeze(0), torch.cat([torch.full((B, 1), 20 + b), noised[:, 1:]], 1).unsqueeze(0))
                        for b in range(4)]
        tr.text_autoenc = Model('tae')
        tr.train_step = Step(events, tae_unpack, loss_of)
    elif kind == 'adv':
        tr.discriminator = Model('disc')
        tr.train_step = Step(events, adv_unpack,
                             lambda b: (torch.tensor(1.0 + b), torch.tensor(0.25), torch.tensor(2.0 * b)))
    else:
        tr.speech_autoenc = Model('sae')
        tr.train_step = Step(events, sae_unpack, loss_of)
    return tr, events


def info(module, msg):
    return ('print', '[INFO ({} / t)] {}'.format(module, msg))


def expected(module, batches_line, logs, saves, close_line, asr_order=False, extra=None):
    """The event list of two epochs over four batches on rank 0.  logs(b, step): the scalars of a logging step;
    saves: (model, file) pairs of a checkpoint; asr_order: the checkpoint comes BEFORE valid() (ASRTrainer), not after
    it (the Seed legs); extra(b, step): scalars ASRTrainer logs on a cadence of its own."""
    ev = [info(module, batches_line)]
    step = 0
    for epoch in range(2):
        ev.append(info(module, 'Starting epoch {} out of 2'.format(epoch + 1)))
        for b in range(4):
            ev.append(('step', b))
            if step == 5:                          # the stub's sixth call reported a skipped update
                ev.append(info(module, 'Error : grad norm is NaN @ step 4'))
            if step % 2 == 0:
                ev += logs(b, step)
            if extra is not None:
                ev += extra(b, step)
            save = []
            if step % 5 == 0:
                save = [('finish',), info(module, 'Model saved at step {}'.format(step))]
                save += [('save', m, f) for m, f in saves]
            valid = [('valid', step)] if step % 3 == 0 else []
            ev += save + valid if asr_order else valid + save
            step += 1
            ev.append(('do_step', step))
    ev.append(('finish',))                         # the last step's verdict, at the end of exec()
    ev.append(info(module, close_line))
    ev.append(('finish',))
    ev += [('save', m, f) for m, f in saves]
    ev.append(('barrier',))
    return ev


def run(tr):
    tr.exec()
    tr.close()


ASR_CLOSE = 'Finished training! The most recent model willbe saved at step 8'
SEED_CLOSE = ASR_CLOSE + ' as well as the ASR model'


def asr_logs(b, step):
    return [('scalar', 'train_loss', 0.5 + b, step), ('scalar', 'train_acc', (3 / 4 + 1) / 2 if b == 2 else 1.0, step)]


def asr_err(b, step):
    # batch 0 at steps 0 and 4 (wer_step 4): every character right
    return [('scalar', 'train_error', 0.0, step)] if step % 4 == 0 else []


def test_asr_loop_saves_before_it_validates(tmp_path, monkeypatch):
    tr, events = make('asr', tmp_path, monkeypatch)
    run(tr)
    assert events == expected('asr', 'Training set total 4 batches', asr_logs, [('asr', 'asr.cpt')], ASR_CLOSE,
                              asr_order=True, extra=asr_err)


def test_asr_loop_with_the_mwer_step_logs_its_risk_and_the_reference_rows(tmp_path, monkeypatch):
    tr, events = make('mwer', tmp_path, monkeypatch)
    run(tr)

    def logs(b, step):
        return [('scalar', 'train_loss', 0.5 + b, step), ('scalar', 'mwer_risk', 1.5 * (b + 1), step),
                ('scalar', 'train_acc', 1.0, step)]
    assert events == expected('asr', 'Training set total 4 batches', logs, [('asr', 'asr.cpt')], ASR_CLOSE,
                              asr_order=True, extra=asr_err)


def test_tae_loop(tmp_path, monkeypatch):
    tr, events = make('tae', tmp_path, monkeypatch)
    run(tr)
    assert events == expected('tae', 'Training set total 4 batches',
                              lambda b, step: [('scalar', 'train_loss', 0.5 + b, step)],
                              [('tae', 'tae.cpt'), ('asr', 'asr_out.cpt')], SEED_CLOSE)


def test_adv_loop(tmp_path, monkeypatch):
    tr, events = make('adv', tmp_path, monkeypatch)
    run(tr)

    def logs(b, step):
        return [('scalar', 'discrim_real_loss_train', 1.0 + b, step), ('scalar', 'discrim_fake_loss_train', 0.25, step),
                ('scalar', 'discrim_loss_train', 1.25 + b, step), ('scalar', 'gen_loss_train', 2.0 * b, step)]
    assert events == expected('adv', 'Training set total 4 batches', logs,
                              [('disc', 'adv.cpt'), ('asr', 'asr_out.cpt')], SEED_CLOSE)


def test_sae_loop(tmp_path, monkeypatch):
    tr, events = make('sae', tmp_path, monkeypatch)
    run(tr)
    assert events == expected('sae', 'Training set total 4 batches.',
                              lambda b, step: [('scalar', 'train_loss', 0.5 + b, step)],
                              [('sae', 'sae.cpt'), ('asr', 'asr_out.cpt')], SEED_CLOSE)


@pytest.mark.parametrize('kind', ['asr', 'mwer', 'tae', 'adv', 'sae'])
def test_rank_one_of_two_steps_its_own_batches_and_writes_nothing(tmp_path, monkeypatch, kind):
    """Rank 1 of 2 runs batches 1 and 3 of each epoch; it validates with the others (step 0 and 3), waits for its
    last step's verdict and meets the barrier, but logs, prints and saves nothing -- and so never calls finish()
    for a checkpoint."""
    tr, events = make(kind, tmp_path, monkeypatch, rank=1, world=2)
    run(tr)
    assert events == [('step', 1), ('valid', 0), ('do_step', 1), ('step', 3), ('do_step', 2),
                      ('step', 1), ('do_step', 3), ('step', 3), ('valid', 3), ('do_step', 4),
                      ('finish',), ('finish',), ('barrier',)]
