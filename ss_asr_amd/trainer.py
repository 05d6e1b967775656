"""Solver / ASRTrainer with the surface of the reference's src/trainer.py
(Solver :33-195, CHARLMTrainer :197-372, ASRTrainer :374-545, ASRTester :547-592, TAETrainer :594-758, SAETrainer :760-907, ADVTrainer :909-1124,
asr_seed_train :1126-1177) so that ``src/train.py`` drives it unchanged:
``getattr(trainer, 'ASRTrainer')(config, paras)`` then ``load_data()``, ``set_model()``, ``exec()``.

Differences, all inside the same call surface:
  * the model computes through libssasr_hip.so (MI355X only);
  * with Adadelta (conf/default.yaml) one iteration of exec() is ONE call of
    engine.ASRTrainStep -- the object bench.py times: zero_grad folded into the
    update kernel, forward, masked CE, backward with the weight gradients on a
    second stream, two-bucket gradient all-reduce, fused clip + NaN guard +
    Adadelta (optim.py), no device-to-host copy -- fed by the device-resident
    loader (gpu_loader.py).  Any other optimizer type takes the reference's
    sequence (zero_grad, forward, backward, Solver.step with clip_grad_norm_);
  * launched under torchrun (WORLD_SIZE > 1) rank r takes batches r, r + world,
    ... of every full round of `world` batches (a tail that does not fill a round
    is dropped, so every rank runs the same number of steps) and gradients are
    averaged over RCCL (dist.py); rank 0 alone logs and checkpoints;
  * valid() no longer dies on the undefined names of src/trainer.py:531.
"""
import math
import warnings
import os

import numpy as np
import torch
import torch.nn as nn

from . import dist as sdist
from . import ops
from .ASRDataset import load_asr_dataset, prepare_x, prepare_y
from .LogHandler import LogHandler
from .TrackerHandler import TrackerHandler
from .asr import ASR
from .charlm import CharLM
from .LMDataset import load_lm_dataset
from .preprocess import EOS_TKN, SOS_TKN
from .optim import FusedAdadelta
from .postprocess import ErrorStats, calc_acc, calc_err, draw_att


class Solver:
    def __init__(self, config, paras, module_id):
        self.config = config
        self.paras = paras
        self.module_id = module_id
        self.rank, self.world, local = sdist.init_from_env()

        if torch.cuda.is_available():
            torch.cuda.set_device(local)
            self.device = torch.device('cuda', local)
            self.verbose("A cuda device is available and will be used.")
            self.paras.gpu = True
        else:
            # Kept for the plumbing tests; the model's forward refuses CPU tensors.
            self.device = torch.device('cpu')
            self.verbose("No cuda device available.")
            self.paras.gpu = False

        os.makedirs(paras.ckpdir, exist_ok=True)
        self.ckpdir = os.path.join(self.paras.ckpdir, self.paras.name)
        os.makedirs(self.ckpdir, exist_ok=True)
        suffix = '' if self.rank == 0 else '.rank%d' % self.rank
        self.tr = TrackerHandler(os.path.join(self.ckpdir, 'tracker%s.json' % suffix),
                                 self.module_id)
        self.lg = LogHandler(os.path.join(self.paras.logdir, self.paras.name,
                                          self.module_id + suffix), self.module_id)
        self.ckppath = os.path.join(self.ckpdir, self.module_id + '.cpt')
        self.best_ckppath = os.path.join(self.ckpdir, self.module_id + '_best.cpt')

        self.valid_step = self.set_if_exists('valid_step', 500)
        self.logging_step = self.set_if_exists('logging_step', 250)
        self.save_step = self.set_if_exists('save_step', 1000)
        self.n_epochs = self.set_if_exists('n_epochs', 5)
        self.train_batch_size = self.set_if_exists('train_batch_size', 32)
        self.valid_batch_size = self.set_if_exists('valid_batch_size', 32)
        self.test_batch_size = self.set_if_exists('test_batch_size', 1)
        self.verbose_summary()

    def verbose_summary(self):
        self.verbose("-------SUMMARY-------")
        self.verbose("Current step : {}".format(self.tr.step))
        self.verbose("Best metric value : {}".format(self.tr.get_best()))
        self.verbose("Number of epochs: {}".format(self.n_epochs))
        self.verbose("Steps: [Logging {}], [Saving {}], [Validation {}]".format(
            self.logging_step, self.save_step, self.valid_step))
        self.verbose("Batch sizes: [Train {}], [Validation{}], [Testing {}]".format(
            self.train_batch_size, self.valid_batch_size, self.test_batch_size))
        self.verbose("---------------------")

    def set_if_exists(self, key, default):
        return self.config[self.module_id].get(key, default)

    def verbose(self, msg, progress=False):
        end = '\r' if progress else '\n'
        if progress:
            msg += '                              '
        else:
            msg = '[INFO ({} / {})] '.format(self.module_id, self.paras.name) + str(msg)
        if self.paras.verbose and getattr(self, 'rank', 0) == 0:
            print(msg, end=end)

    def step(self, params, optim, grad_clip=5):
        """src/trainer.py:131-148: clip the global gradient norm, skip the update
        (with a message) when the norm is NaN, otherwise step the optimizer.
        With FusedAdadelta everything happens on the device; the NaN message of
        a step is printed when its flag has reached the host (at the latest on
        the next call)."""
        if isinstance(optim, FusedAdadelta):
            done = optim.poll()
            if done is not None and done[1]:
                self.verbose('Error : grad norm is NaN @ step {}'.format(self.tr.step - 1))
            scale = sdist.allreduce_grad(optim._grad)
            optim.clip_and_step(max_norm=float(grad_clip), grad_scale=scale)
            return
        # Any other torch.optim type a config names (conf/default.yaml selects none): the reference's own sequence on
        # torch's optimizer -- NOT the MI355X-native step (no fused clip + update kernel, no overlapped all-reduce).
        params = list(params)
        if not getattr(self, '_warned_torch_optim', False):
            self._warned_torch_optim = True
            warnings.warn('%s has no fused MI355X form here: Solver.step runs torch.optim and clip_grad_norm_ '
                          '(Adadelta and Adam are the native ones)' % type(optim).__name__, RuntimeWarning)
        if sdist.is_active():
            # every parameter the optimizer updates is averaged, not only the list the norm is clipped over
            # (TAETrainer / SAETrainer hand `params` of ONE module to an optimizer over two: src/trainer.py:633-641, :676)
            seen = set()
            for grp in optim.param_groups:
                for p in grp['params']:
                    if p.grad is not None and id(p) not in seen:
                        seen.add(id(p))
                        torch.distributed.all_reduce(p.grad)
                        p.grad.div_(sdist.world_size())
        grad_norm = nn.utils.clip_grad_norm_(params, grad_clip)
        if math.isnan(grad_norm):
            self.verbose('Error : grad norm is NaN @ step {}'.format(self.tr.step))
        else:
            optim.step()

    def setup_module(self, module, ckp_path, *para, **model_para):
        model = module(*para, **model_para)
        if os.path.isfile(ckp_path):
            self.verbose('Loading a pretrained model from {}'.format(ckp_path))
            model.load_state_dict(torch.load(ckp_path, map_location='cpu'))
        else:
            self.verbose('No model found at {}. A new model will be created'.format(ckp_path))
        return model.to(self.device)

    def genpath(self, p, module_id):
        if p is None:
            path = os.path.join(self.ckpdir, '{}.cpt'.format(module_id))
            return (path, path)
        if isinstance(p, str):
            return (p, p)
        assert len(p) == 2
        return p

    def close(self):
        return None


class Trainer(Solver):
    """The epoch loop, the best-checkpoint rule and close() of ASRTrainer, TAETrainer, ADVTrainer and SAETrainer.  A
    subclass supplies `_prepare` (a loader's batch on the device: the arguments of its engine step object, which is
    `self.train_step`, or None when the config's optimizer has no fused form), `_reference` (the reference's sequence
    with a torch optimizer), `_log` (rank 0's scalars at a logging step) and `_checkpoint` (what is saved where)."""

    # Within an iteration the reference's ASRTrainer checkpoints BEFORE it validates (src/trainer.py:448-455); its
    # TAETrainer (:682-686), SAETrainer (:827-831) and ADVTrainer (:1035-1040) validate first.
    save_before_valid = False
    batches_line = 'Training set total {} batches'
    close_line_end = ' as well as the ASR model'
    # valid() of the reference's ADVTrainer says nothing when the metric is no better (src/trainer.py:1106-1112);
    # the others do (:534, :748, :894)
    reports_worse = True

    def _train_batches(self):
        """(batch index, _prepare's batch) for this rank's batches of one epoch.  Every rank yields the same number:
        a tail that does not fill a round of `world` batches is dropped (a rank alone in an all-reduce would wait
        for ever)."""
        from .gpu_loader import rank_batches
        mine = set(rank_batches(len(self.train_set), self.rank, self.world))
        for b_ind, raw in enumerate(self.train_set):
            if b_ind in mine:
                yield b_ind, self._prepare(raw)

    def _fused(self, batch):
        """One call of the engine step object on _prepare's batch -> what _log takes."""
        return self.train_step(*batch)

    def _log_own_cadence(self, result):
        """Rank 0, every iteration: scalars on a step count of the trainer's own."""

    def _save(self):
        for module, path in self._checkpoint():
            sdist.save_atomic(module.state_dict(), path)

    def exec(self):
        self.verbose(self.batches_line.format(len(self.train_set)))
        nan_reported = self.train_step.skipped_steps if self.train_step is not None else 0
        for epoch in range(self.n_epochs):
            self.verbose("Starting epoch {} out of {}".format(epoch + 1, self.n_epochs))
            for b_ind, batch in self._train_batches():
                self.verbose('Batch: {}/{}, global step: {}'.format(b_ind, len(self.train_set), self.tr.step),
                             progress=True)
                if self.train_step is not None:
                    # one fused step; a persistent launch that timed out in the previous step raises here (its status
                    # words arrive with the optimizer's)
                    result = self._fused(batch)
                    if self.train_step.skipped_steps > nan_reported:
                        nan_reported = self.train_step.skipped_steps
                        self.verbose('Error : grad norm is NaN @ step {}'.format(self.tr.step - 1))
                else:
                    result = self._reference(batch)
                    if self.tr.step % self.logging_step == 0:
                        ops.check_persistent_status()      # the host synchronises here anyway
                if self.rank == 0:
                    if self.tr.step % self.logging_step == 0:
                        self._log(result)
                    self._log_own_cadence(result)
                if self.save_before_valid:
                    self._save_at_save_step()
                if self.tr.step % self.valid_step == 0:
                    self.valid()
                if not self.save_before_valid:
                    self._save_at_save_step()
                self.tr.do_step()
        if self.train_step is not None:
            self.train_step.finish()           # the last step's verdict (raises on a timeout)

    def _save_at_save_step(self):
        if self.rank == 0 and self.tr.step % self.save_step == 0:
            if self.train_step is not None:
                self.train_step.finish()       # this step's verdict first: never checkpoint after a time-out
            self.verbose("Model saved at step {}".format(self.tr.step))
            self._save()

    def _keep_best(self, avg_loss, module, lines=('Best validation loss : {:.4f} @ global step {}',)):
        """The tail of valid() on rank 0: a metric below the tracker's best becomes the best, is announced with
        `lines` and `module` goes to the best-checkpoint file.  -> whether it was."""
        if avg_loss < self.tr.get_best():
            self.tr.set_best(avg_loss)
            for line in lines:
                self.verbose(line.format(self.tr.get_best(), self.tr.step))
            sdist.save_atomic(module.state_dict(), self.best_ckppath)
            return True
        if self.reports_worse:
            self.verbose("Validation metric worse : ({:.4f} vs. {:.4f})".format(avg_loss, self.tr.get_best()))
        return False

    def close(self):
        self.verbose("Finished training! The most recent model will" +
                     "be saved at step {}{}".format(self.tr.step, self.close_line_end))
        if getattr(self, 'train_step', None) is not None:
            self.train_step.finish()
        if self.rank == 0:
            self._save()
        sdist.barrier()        # the next reader of these files (the Seed loop's next leg) runs on every rank


class CHARLMTrainer(Solver):
    """Trains the character language model, src/trainer.py:197-372: the same config keys (char_lm.chunk_size,
    mdl.tf_rate, mdl.hidden_size, opt.type, opt.learning_rate, train_index), loss per character, tracker best,
    char_lm_best.cpt / char_lm.cpt (the file ASRTester loads) and text logging.  One iteration of exec() is ONE
    engine.CharLMTrainStep call fed by the device-resident loader (LMDataset.ResidentLMLoader).  `generate` runs on
    CharLM.forward, one step per call.  `predict` (:280-317) is left out: only the reference's dead lm_predict.py
    calls it.  Also reachable as trainer.LMTrainer, the spelling src/train.py:19 offers."""

    def __init__(self, config, paras):
        super().__init__(config, paras, 'char_lm')

    def load_data(self):
        self.chunk_size = self.config['char_lm']['chunk_size']
        self.tf_rate = self.config['char_lm']['mdl']['tf_rate']
        self.ds, self.train_set = load_lm_dataset(self.config['char_lm']['train_index'], self.chunk_size,
                                                  self.train_batch_size, shuffle=True, resident=True)

    def set_model(self):
        from .engine import CharLMTrainStep
        opt = self.config['char_lm']['opt']
        if opt['type'] != 'Adam':
            raise NotImplementedError("char_lm.opt.type '%s': this build trains the CharLM with its fused Adam step "
                                      "only" % opt['type'])
        self.lm = self.setup_module(CharLM, self.ckppath, self.ds.get_num_chars(),
                                    self.config['char_lm']['mdl']['hidden_size'])
        self.train_step = CharLMTrainStep(self.lm, self.tf_rate, lr=opt['learning_rate'], eps=1e-8, grad_clip=5.0,
                                          opt_type=opt['type'])
        self.optim = self.train_step.optim

    def exec(self):
        self.verbose('Training set total {} batches.'.format(len(self.train_set)))
        epoch = 0
        while epoch < self.n_epochs:
            self.verbose("Starting epoch {} out of {}".format(epoch + 1, self.n_epochs))
            for b_ind, (_, (_, y)) in enumerate(self.train_set):
                self.verbose('Batch: {}/{}, global step: {}'.format(b_ind, len(self.train_set), self.tr.step),
                             progress=True)
                loss = self.train_step(y)
                done = self.train_step.last_done
                if done is not None and done[1]:
                    self.verbose('Error : grad norm is NaN @ step {}'.format(self.tr.step - 1))
                wants = (self.tr.step % self.logging_step == 0 or self.tr.step % self.valid_step == 0)
                if wants:                                     # the only host reads of the loss
                    loss_by_char = loss.item() / self.chunk_size
                    self.last_loss_by_char = loss_by_char
                if self.tr.step % self.logging_step == 0:
                    self.lg.scalar('train_loss', loss_by_char, self.tr.step)
                if self.tr.step % self.valid_step == 0:
                    generated = self.generate()
                    self.lg.text('text_generate', generated, self.tr.step)
                    if loss_by_char < self.tr.get_best():
                        self.tr.set_best(loss_by_char)
                        torch.save(self.lm.state_dict(), self.best_ckppath)
                if self.tr.step % self.save_step == 0:
                    self.verbose("Model saved at step {}".format(self.tr.step))
                    torch.save(self.lm.state_dict(), self.ckppath)
                self.tr.do_step()
            self.verbose('Epoch {} finished'.format(epoch))
            epoch += 1

    def generate(self, length=100, temp=0.8, start=SOS_TKN):
        """src/trainer.py:319-364: `length` characters sampled at temperature `temp` after feeding `start`."""
        with torch.no_grad():
            h_1, h_2 = self.lm.init_hidden(1, self.device)
            x = self.ds.s2l(start).to(self.device)
            out_string = start
            for i in range(x.shape[0] - 1):
                out, (h_1, h_2) = self.lm(x[i].view(-1), h_1, h_2)
            x = x[-1].view(-1)
            for i in range(length):
                out, (h_1, h_2) = self.lm(x, h_1, h_2)
                dist = torch.softmax(out, dim=-1)
                dist = dist ** (1 / temp)
                dist = dist / torch.sum(dist, dim=-1)
                predict = torch.multinomial(dist, 1)[0]
                predict_str = self.ds.idx2char[predict.item()]
                out_string += predict_str
                x = self.ds.s2l(predict_str).to(self.device)
        return out_string

    def close(self):
        self.verbose("Finished training! The most recent model will" +
                     "be saved at step {}".format(self.tr.step))
        self.train_step.finish()
        torch.save(self.lm.state_dict(), self.ckppath)


LMTrainer = CHARLMTrainer


class ASRTrainer(Trainer):
    """src/trainer.py:377-537.  BUILD-DEFINED keys (the reference's recipe has neither; both absent: off, and
    training is the reference's plain masked CE on unaugmented filterbanks):
    asr.label_smoothing in [0, 1): the train loss is the smoothed CE of ops.masked_ce_loss (the attention branch
    only under the joint CTC loss); the logged `train_loss` is then the SMOOTHED loss, while valid() keeps
    reporting the unsmoothed metrics.
    asr.spec_augment: {freq_masks, freq_width, time_masks, time_width, time_ratio, fill, seed}: SpecAugment
    masks (at most 8 of a kind; widths drawn from 0 .. *_width, time masks no wider than time_ratio of the
    utterance) applied by the resident loader's batch assembly (GpuResidentLoader, ssasr_gather_batch_aug),
    redrawn every epoch; it needs that loader and raises where it is not in use.
    asr.mwer: {beam_size, ce_weight, unit, max_decoding_steps, sampling, seed}: minimum word error rate training
    (engine.MWERTrainStep) instead of the CE step: the expected number of `unit` (word | char) errors over a beam of
    2 .. 32 hypotheses searched on the training batch, plus ce_weight (>= 0) times the masked CE.  `train_loss` is
    then that loss and `mwer_risk`, the mean expected errors per utterance, is logged beside it.  It needs the fused
    step (Adadelta on the GPU) and is not defined together with asr.label_smoothing.  With a ctc_weight model the CTC
    branch takes no part in the step.  sampling: true draws the beam_size hypotheses from the model's own distribution
    instead of searching for them (seed: an integer >= 0 for the step's generator)."""
    SPEC_AUGMENT_KEYS = ('freq_masks', 'freq_width', 'time_masks', 'time_width', 'time_ratio', 'fill', 'seed')
    MWER_KEYS = ('beam_size', 'ce_weight', 'unit', 'max_decoding_steps', 'sampling', 'seed')

    @classmethod
    def mwer_options(cls, asr_config):
        """engine.MWERTrainStep's keywords of asr_config's `mwer` mapping, validated; None when it is absent."""
        import math
        conf = asr_config.get('mwer')
        if conf is None:
            return None
        if not isinstance(conf, dict):
            raise ValueError('asr.mwer must be a mapping of {}, got {!r}'.format(cls.MWER_KEYS, conf))
        unknown = sorted(set(conf) - set(cls.MWER_KEYS))
        if unknown:
            raise ValueError('asr.mwer: unknown keys {} (known: {})'.format(unknown, cls.MWER_KEYS))
        if asr_config.get('label_smoothing'):
            raise ValueError('asr.label_smoothing and asr.mwer are not defined together: drop one of them')

        def integer(key, v, lo, hi):
            if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
                raise ValueError('asr.mwer.{} must be an integer in {} .. {}, got {!r}'.format(key, lo, hi, v))
            return v

        if 'beam_size' not in conf:
            raise ValueError('asr.mwer.beam_size is required (an integer in 2 .. 32)')
        ce_weight = conf.get('ce_weight', 0.01)
        if (isinstance(ce_weight, bool) or not isinstance(ce_weight, (int, float)) or not math.isfinite(ce_weight)
                or ce_weight < 0):
            raise ValueError('asr.mwer.ce_weight must be a finite number >= 0, got {!r}'.format(ce_weight))
        unit = conf.get('unit', 'word')
        if unit not in ('word', 'char'):
            raise ValueError("asr.mwer.unit must be 'word' or 'char', got {!r}".format(unit))
        out = dict(beam_size=integer('beam_size', conf['beam_size'], 2, 32), ce_weight=float(ce_weight), unit=unit,
                   max_decoding_steps=integer('max_decoding_steps', conf.get('max_decoding_steps', 200), 1, 8189))
        # the sampled form's keys are passed on only when the config names them
        if 'sampling' in conf:
            if not isinstance(conf['sampling'], bool):
                raise ValueError('asr.mwer.sampling must be true or false, got {!r}'.format(conf['sampling']))
            out['sampling'] = conf['sampling']
        if 'seed' in conf:
            out['seed'] = integer('seed', conf['seed'], 0, 2 ** 63 - 1)
        return out

    @classmethod
    def regularisers(cls, asr_config):
        """(label smoothing, GpuResidentLoader's spec_augment dict or None) of asr_config, validated."""
        import math

        def number(key, v):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
                raise ValueError('asr.{} must be a finite number, got {!r}'.format(key, v))
            return v

        def integer(key, v, lo, hi):
            if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
                raise ValueError('asr.{} must be an integer in {} .. {}, got {!r}'.format(key, lo, hi, v))
            return v

        eps = asr_config.get('label_smoothing')
        eps = 0.0 if eps is None else float(number('label_smoothing', eps))
        if not 0.0 <= eps < 1.0:
            raise ValueError('asr.label_smoothing must lie in [0, 1), got {!r}'.format(eps))
        conf = asr_config.get('spec_augment')
        if conf is None:
            return eps, None
        if not isinstance(conf, dict):
            raise ValueError('asr.spec_augment must be a mapping of {}, got {!r}'.format(cls.SPEC_AUGMENT_KEYS, conf))
        unknown = sorted(set(conf) - set(cls.SPEC_AUGMENT_KEYS))
        if unknown:
            raise ValueError('asr.spec_augment: unknown keys {} (known: {})'.format(unknown, cls.SPEC_AUGMENT_KEYS))
        feat = asr_config.get('mdl', {}).get('feature_dim')
        ratio = number('spec_augment.time_ratio', conf.get('time_ratio', 1.0))
        if not 0.0 <= ratio <= 1.0:
            raise ValueError('asr.spec_augment.time_ratio must lie in [0, 1], got {!r}'.format(ratio))
        return eps, dict(
            n_freq=integer('spec_augment.freq_masks', conf.get('freq_masks', 0), 0, 8),
            max_freq=integer('spec_augment.freq_width', conf.get('freq_width', 0), 0,
                             feat if isinstance(feat, int) else 2 ** 31 - 1),
            n_time=integer('spec_augment.time_masks', conf.get('time_masks', 0), 0, 8),
            max_time=integer('spec_augment.time_width', conf.get('time_width', 0), 0, 2 ** 31 - 1),
            time_ratio=ratio, fill=float(number('spec_augment.fill', conf.get('fill', 0.0))),
            seed=integer('spec_augment.seed', conf.get('seed', 0), 0, 2 ** 64 - 1))

    def __init__(self, config, paras):
        super().__init__(config, paras, 'asr')
        self.label_smoothing, self.spec_augment = self.regularisers(self.config['asr'])
        self.mwer = self.mwer_options(self.config['asr'])

    def load_data(self):
        """Index files must be sorted so that every batch is in decreasing
        frame-length order (conf/README.md:16)."""
        n_jobs = self.set_if_exists('loader_jobs', 8)
        (self.mapper, _, self.train_set) = load_asr_dataset(
            self.config['asr']['train_index'], batch_size=self.train_batch_size,
            n_jobs=n_jobs, use_gpu=self.paras.gpu)
        (_, _, self.valid_set) = load_asr_dataset(
            self.config['asr']['valid_index'], batch_size=self.valid_batch_size,
            n_jobs=n_jobs, use_gpu=self.paras.gpu)
        self.wer_step = self.config['asr']['wer_step']
        # Training batches come from a device-resident copy of the corpus when it fits
        # comfortably; ``asr.gpu_resident_loader: false`` keeps the DataLoader.
        self.gpu_loader = None
        if self.device.type == 'cuda' and self.config['asr'].get('gpu_resident_loader', True):
            from .gpu_loader import GpuResidentLoader
            free, _ = torch.cuda.mem_get_info(self.device)
            est = 4 * int(self.config['asr']['mdl']['feature_dim']) * sum(
                r['unpadded_num_frames'] for r in self.train_set.dataset._rows)
            if est < free // 4:
                self.gpu_loader = GpuResidentLoader(self.config['asr']['train_index'], self.train_batch_size,
                                                    self.device, rank=self.rank, world=self.world,
                                                    spec_augment=self.spec_augment)
                self.verbose('Training corpus resident on the GPU: {:.1f} MB'.format(
                    self.gpu_loader.bytes_resident() / 1e6))
        if self.spec_augment is not None and self.gpu_loader is None:
            raise RuntimeError('asr.spec_augment is applied by the GPU-resident loader\'s batch assembly, which is '
                               'not in use here (no GPU, asr.gpu_resident_loader: false, or a corpus too large to '
                               'keep on the device): refusing to train unaugmented')

    def _train_batches(self):
        """The resident loader deals this rank's batches itself, already on the device."""
        if self.gpu_loader is None:
            return super()._train_batches()
        return ((b_ind, batch) for b_ind, *batch in self.gpu_loader)

    def _prepare(self, raw):
        """-> [x, x_lens, y, y_lens]"""
        return [*prepare_x(raw[0], device=self.device), *prepare_y(raw[1], device=self.device)]

    def set_model(self, asrpath=None):
        """asrpath (this build; the Seed loop passes it): (checkpoint to load, checkpoint to save) instead of
        <ckpdir>/asr.cpt for both, as the other trainers of the reference take it (src/trainer.py:623)."""
        if asrpath is not None:
            self.ckppath_in, self.ckppath = self.genpath(asrpath, 'asr')
        # `ctc_weight` under asr.mdl is a key of this build (BASELINE.json configs[3], ss_asr_amd/ctc.py);
        # the reference's configs do not carry it and get the reference's model and loss
        joint = 'ctc_weight' in self.config['asr']['mdl']
        if joint:
            from .ctc import JointCTCASR, JointCTCTrainStep
        self.asr_model = self.setup_module(JointCTCASR if joint else ASR, getattr(self, 'ckppath_in', self.ckppath),
                                           self.mapper.get_dim(),
                                           **self.config['asr']['mdl'])
        opt = self.config['asr']['opt']
        self.train_step = None
        if opt['type'] == 'Adadelta' and self.device.type == 'cuda':
            # the fused step (engine.ASRTrainStep): what bench.py times is what trains
            from .engine import ASRTrainStep, MWERTrainStep
            if self.mwer is not None:
                self.train_step = MWERTrainStep(self.asr_model, lr=opt['learning_rate'], eps=1e-8, grad_clip=5.0,
                                                eos=self.mapper.char_to_ind(EOS_TKN),
                                                space=self.mapper.char_to_ind(' '), **self.mwer)
            else:
                step_cls = JointCTCTrainStep if joint else ASRTrainStep
                self.train_step = step_cls(self.asr_model, lr=opt['learning_rate'], eps=1e-8, grad_clip=5.0,
                                           label_smoothing=self.label_smoothing)
            self.flat, self.optim = self.train_step.flat, self.train_step.optim
        elif self.mwer is not None:
            raise RuntimeError('asr.mwer runs on the fused step only (Adadelta on the GPU)')
        elif joint:
            raise RuntimeError('the joint CTC+attention loss runs on the fused step only (Adadelta on the GPU)')
        else:
            self.optim = getattr(torch.optim, opt['type'])(
                self.asr_model.parameters(), lr=opt['learning_rate'], eps=1e-8)

    def _loss(self, prediction, y, ans_len, label_smoothing=0.0):
        """src/trainer.py:426-434 (valid() calls it unsmoothed)."""
        if prediction.is_cuda:
            return ops.masked_ce_loss(prediction, y, ans_len, label_smoothing)
        raise RuntimeError('ss_asr_amd computes on the GPU only')

    save_before_valid = True
    close_line_end = ''

    def _fused(self, batch):
        """src/trainer.py:419-438 as one fused step -> (loss, logits [B, ans_len, V], labels [B, ans_len])."""
        x, x_lens, y, y_lens = batch
        ans_len = max(y_lens) - 1
        if self.mwer is None:
            loss = self.train_step(x, y, x_lens, ans_len)
            prediction = self.train_step.last_logits
        else:
            loss = self.train_step(x, y, x_lens)
            # the reference rows of the teacher-forced pass are the CE step's logits
            prediction = self.train_step.last_logits[self.mwer['beam_size']::self.mwer['beam_size'] + 1]
            prediction = prediction[:, :ans_len]
        return loss, prediction, y[:, 1:ans_len + 1]

    def _reference(self, batch):
        x, x_lens, y, y_lens = batch
        ans_len = max(y_lens) - 1
        self.optim.zero_grad()
        _, prediction, _ = self.asr_model(x, ans_len, teacher=y, state_len=x_lens)
        loss = self._loss(prediction, y, ans_len, self.label_smoothing)
        loss.backward()
        self.step(self.asr_model.parameters(), self.optim)
        return loss, prediction, y[:, 1:ans_len + 1]

    def _log(self, result):
        loss, prediction, label = result
        self.lg.scalar('train_loss', loss.item(), self.tr.step)
        if self.mwer is not None:
            self.lg.scalar('mwer_risk', self.train_step.last_risk.mean().item(), self.tr.step)
        self.lg.scalar('train_acc', calc_acc(prediction, label), self.tr.step)

    def _log_own_cadence(self, result):
        if self.tr.step % self.wer_step == 0:
            self.lg.scalar('train_error', calc_err(result[1], result[2], mapper=self.mapper), self.tr.step)

    def _checkpoint(self):
        return ((self.asr_model, self.ckppath),)

    def valid(self):
        """Greedy decoding for ans_len + 30 steps without a teacher, loss on the
        first ans_len outputs (src/trainer.py:460-537)."""
        self.asr_model.eval()
        total_loss, total_acc, total_err, num_batches = 0.0, 0.0, 0.0, 0
        prediction = label = att_map = None
        # Under torchrun the validation batches are dealt to the ranks round-robin (every rank holds the same
        # weights: the sums below are all-reduced, the averages are the single-process ones); rank 0 also takes
        # the LAST batch, whose hypotheses it logs as the reference does (src/trainer.py:505-519).
        n_valid = len(self.valid_set)
        mine = lambda b: self.world == 1 or b % self.world == self.rank or (self.rank == 0 and b == n_valid - 1)
        counted = lambda b: self.world == 1 or b % self.world == self.rank
        with torch.no_grad():
            for b_idx, (x, y) in enumerate(self.valid_set):
                if not mine(b_idx):
                    continue
                self.verbose('Validation step - ( {} / {} )'.format(b_idx, len(self.valid_set)),
                             progress=True)
                (x, x_lens) = prepare_x(x, device=self.device)
                (y, y_lens) = prepare_y(y, device=self.device)
                ans_len = max(y_lens) - 1
                _, prediction, att_map = self.asr_model(x, ans_len + 30, state_len=x_lens)
                label = y[:, 1:ans_len + 1].contiguous()
                if not counted(b_idx):
                    continue                       # (rank 0's copy of the last batch: for its log only)
                loss = self._loss(prediction, y, ans_len)
                total_loss += float(loss)
                total_acc += calc_acc(prediction, label)
                total_err += calc_err(prediction, label, mapper=self.mapper)
                num_batches += 1
        # the persistent launches of the greedy passes report into status words of their own (they run
        # outside a train step's shared row): a hand-off that timed out must not become a "best" model
        # or a best_hyp.txt (float(loss) above has synchronised already)
        ops.check_persistent_status()
        if sdist.is_active() and self.world > 1:
            sums = torch.tensor([total_loss, total_acc, total_err, float(num_batches)], dtype=torch.float64,
                                device=self.device)
            torch.distributed.all_reduce(sums)
            total_loss, total_acc, total_err, num_batches = (float(sums[0]), float(sums[1]), float(sums[2]),
                                                             int(round(float(sums[3]))))
        if num_batches == 0:
            self.asr_model.train()
            return
        avg_loss = total_loss / num_batches
        avg_err = total_err / num_batches
        avg_acc = total_acc / num_batches
        if self.rank == 0:
            self.lg.scalar('eval_loss', avg_loss, self.tr.step)
            self.lg.scalar('eval_error', avg_err, self.tr.step)
            self.lg.scalar('eval_acc', avg_acc, self.tr.step)
            hyp_idx = np.argmax(prediction.cpu().numpy(), axis=-1)
            val_hyp = [self.mapper.translate(p) for p in hyp_idx]
            val_txt = [self.mapper.translate(l) for l in label.cpu()]
            for idx, attmap in enumerate(draw_att(att_map, hyp_idx)):
                self.lg.image('eval_att_' + str(idx), attmap, self.tr.step)
                self.lg.text('eval_hyp_' + str(idx), "{} |predict vs. real| {}".format(
                    val_hyp[idx], val_txt[idx]), self.tr.step)
            if self._keep_best(avg_loss, self.asr_model, ('Best validation loss for ASR : {:.4f} @ global step {}',
                                                          'Saving best model.')):
                with open(os.path.join(self.ckpdir, 'best_hyp.txt'), 'w') as f:
                    for hyp, txt in zip(val_hyp, val_txt):
                        f.write(hyp + ',' + txt + '\n')
        self.asr_model.train()


class ASRTester(Solver):
    """Inference over a test index, src/trainer.py:547-592: the same config keys (asr.test_index,
    decode_lm_weight, decode_beam_size, decode_jobs, max_decode_step_ratio, char_lm.mdl.hidden_size) and the same
    `decode_file` name.  asr.decode_beam_size is honoured: 1 decodes greedily, 2 .. 32 runs a beam search of that
    width (the reference announces one and leaves it a TODO, :590), `decode_group` utterances per launch
    (ASR.decode_many).  The reference constructs a CharLM and never loads
    it (:567-569); here <ckpdir>/char_lm.cpt is loaded when it exists.
    BUILD-DEFINED: with 'ctc_weight' in asr.mdl the model is ctc.JointCTCASR, as ASRTrainer builds it, and
    asr.decode_ctc_weight (absent: 0) in (0, 1] decodes with the CTC prefix score at that weight (joint CTC /
    attention decoding, ssasr_decode_beam_ctc, any beam size); `decode_file` then ends in `_ctc<weight>`.
    asr.decode_length_bonus, asr.decode_coverage_weight (with asr.decode_coverage_threshold, absent: 0.5) and
    asr.decode_end_margin (absent: off) are the beam search's length bonus, coverage term and end detection
    (ssasr_decode_beam_ex, any beam size); `decode_file` gains `_lb<bonus>`, `_cov<weight>`, `_end<margin>` for the
    terms that are on.
    asr.decode_hotwords (a list of strings) with asr.decode_hotword_bonus (>= 0, absent: 1.0) and asr.decode_ngram_lm
    (the path of a char_graph.CharGraph.save file) with asr.decode_ngram_weight (>= 0, absent: 0.5) put a character
    graph INSIDE the attention beam search (ASR.decode_many(graph=..., graph_weight=...), ssasr_decode_beam_graph, any
    beam size; no ctc_head needed): contextual biasing towards the phrases, a count-based n-gram LM, or with both
    their product, built and validated in set_model as asr.decode_ctc_only's graph keys are; `decode_file` gains
    `_hw<n>x<bonus>` / `_ng<weight>` only when a key is present.  Together with asr.decode_ctc_only, which has its own
    graph keys, they are an error.
    asr.decode_align: true (absent: off; needs 'ctc_weight' in asr.mdl, else set_model raises): after each group is
    decoded its hypotheses are force-aligned to the group's encoder outputs (ASR.align, ssasr_ctc_align); exec()
    still returns the strings, `last_alignments` holds one asr.Alignment per utterance in index order, and
    `decode_file` gains `_align`.
    asr.decode_score: true (absent: off): each utterance's labels are kept and every decoded group is scored against
    them in one launch (ASR.score, ssasr_edit_score) after the decode and before the optional align.  exec() still
    returns the strings and `decode_file` is unchanged (scoring alters no transcript); `last_scores` holds one
    asr.Score per utterance in index order and `last_error_rates` the corpus-level {'cer', 'wer', 'oracle_cer',
    'oracle_wer', 'chars': (S, D, I, N), 'words': (S, D, I, N)} (postprocess.ErrorStats: summed errors over summed
    reference lengths; oracle_*: of each n-best list's entry with the fewest word errors), printed as one verbose
    line.
    asr.decode_mbr: {unit: word, scale: 1.0} (absent: off; unit 'word' | 'char', scale finite and >= 0, both
    optional; needs decode_beam_size >= 2, else set_model raises): every decoded group's written transcript is the
    minimum-Bayes-risk choice of its n-best list (ASR.mbr, ssasr_mbr_select: the entry with the lowest expected error
    count under the softmax of scale * the hypothesis scores) instead of its first entry; `decode_file` gains
    `_mbr<unit>` and `last_mbr_choices` holds the chosen slot per utterance in index order.  With asr.decode_score on,
    `last_scores` keeps scoring slot 0 and `last_error_rates` gains 'mbr_cer' / 'mbr_wer', the corpus-level rates of
    the chosen slots (read from the scorer's per-hypothesis rows, no second launch); an align then aligns the chosen
    transcripts.
    asr.decode_ctc_only: {beam_size: 8} (absent: off; beam_size an integer in 0..32, 0 the best path; needs
    'ctc_weight' in asr.mdl, else set_model raises): every group is transcribed from the ctc_head's posteriors alone,
    with no Speller step (ASR.decode_ctc, ssasr_ctc_decode); asr.decode_beam_size, the language model and
    max_decode_step_ratio then play no part, and `decode_file` gains `_ctconly<beam_size>`.  The optional keys
    lm_weight and length_bonus (finite numbers, absent: 0; beam_size >= 1) put the tester's language model INSIDE the
    prefix search (ssasr_ctc_decode_lm: a text is ranked by its CTC score + lm_weight log P_lm + length_bonus *
    length); `decode_file` then gains `_clm<lm_weight>` (and `_clb<length_bonus>`) when lm_weight != 0, and with
    asr.decode_rescore lm_weight (>= 0) is decode_two_pass's first_lm_weight.  The optional keys hotwords (a list of
    strings) with hotword_bonus (>= 0, absent: 1.0) and ngram_lm (the path of a char_graph.CharGraph.save file) with
    ngram_weight (>= 0, absent: 0.5) put a character graph INSIDE the prefix search (ssasr_ctc_decode_graph;
    beam_size >= 1): contextual biasing towards the phrases, a count-based n-gram LM, or with both their product;
    everything is validated in set_model, length_bonus goes with it, and `decode_file` gains `_hw<n>x<bonus>` /
    `_ng<weight>` (and `_clb<length_bonus>`) only when a key is present.  Together with asr.decode_rescore or a
    non-zero lm_weight they are an error (not built).  The optional keys word_lm (the path of a
    word_graph.WordGraph.save file) with word_lm_weight (>= 0, absent: 0.5) restrict the texts to a lexicon and rank
    them with a word n-gram LM INSIDE the prefix search (ssasr_ctc_decode_word; beam_size >= 1; length_bonus goes with
    it); `decode_file` gains `_wlm<weight>` (and `_clb<length_bonus>`) only when the key is present; together with
    hotwords / ngram_lm, a non-zero lm_weight or asr.decode_rescore they are an error (not built).  It composes with
    decode_score, decode_mbr (which then needs THIS beam_size >= 2) and decode_align; together with a positive
    asr.decode_ctc_weight or any of the beam search's terms it is an error.
    asr.decode_rescore: {ctc_weight: 0.3, length_bonus: 0.0} (absent: off; ctc_weight a number in [0, 1], length_bonus
    finite, both optional; valid only together with asr.decode_ctc_only at beam_size >= 1, else set_model raises):
    two-pass decoding -- every group's CTC list is teacher-forced through the Speller and re-ranked by (1 - ctc_weight)
    log P_speller + ctc_weight * the CTC score + asr.decode_lm_weight * log P_lm + length_bonus * length
    (ASR.decode_two_pass, ssasr_rescore) with the tester's language model; `decode_file` gains `_rescore<ctc_weight>`.
    decode_score, decode_mbr and decode_align then see the re-ranked list."""
    decode_group = 32
    TERM_KEYS = ('decode_length_bonus', 'decode_coverage_weight', 'decode_coverage_threshold', 'decode_end_margin')

    @classmethod
    def decode_terms(cls, asr_config):
        """(ASR.decode_many's keywords for the terms asr_config turns on, their `decode_file` suffix), validated."""
        import math
        vals = {}
        for key in cls.TERM_KEYS:
            v = asr_config.get(key)
            if v is None:
                continue
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
                raise ValueError('asr.{} must be a finite number, got {!r}'.format(key, v))
            vals[key] = v
        kw, suffix = {}, ''
        if vals.get('decode_length_bonus', 0) != 0:
            kw['length_bonus'] = vals['decode_length_bonus']
            suffix += '_lb{:}'.format(vals['decode_length_bonus'])
        if vals.get('decode_coverage_weight', 0) != 0:
            tau = vals.get('decode_coverage_threshold', 0.5)
            if not tau > 0:
                raise ValueError('asr.decode_coverage_threshold must be > 0, got {!r}'.format(tau))
            kw['coverage_weight'], kw['coverage_threshold'] = vals['decode_coverage_weight'], tau
            suffix += '_cov{:}'.format(vals['decode_coverage_weight'])
        if 'decode_end_margin' in vals:
            if vals['decode_end_margin'] < 0:
                raise ValueError('asr.decode_end_margin must be >= 0, got {!r}'.format(vals['decode_end_margin']))
            kw['end_margin'] = vals['decode_end_margin']
            suffix += '_end{:}'.format(vals['decode_end_margin'])
        return kw, suffix

    @staticmethod
    def mbr_args(asr_config):
        """ASR.mbr's keywords from asr.decode_mbr, validated; None when the key is absent (or false)."""
        import math
        conf = asr_config.get('decode_mbr')
        if conf is None or conf is False:
            return None
        if conf is True:
            conf = {}
        if not isinstance(conf, dict) or set(conf) - {'unit', 'scale'}:
            raise ValueError('asr.decode_mbr must be a mapping with the keys unit and scale, got {!r}'.format(conf))
        unit, scale = conf.get('unit', 'word'), conf.get('scale', 1.0)
        if unit not in ('word', 'char'):
            raise ValueError("asr.decode_mbr.unit must be 'word' or 'char', got {!r}".format(unit))
        if isinstance(scale, bool) or not isinstance(scale, (int, float)) or not math.isfinite(scale) or scale < 0:
            raise ValueError('asr.decode_mbr.scale must be a finite number >= 0, got {!r}'.format(scale))
        ctc_only = ASRTester.ctc_only_beam(asr_config)
        beam = asr_config.get('decode_beam_size') if ctc_only is None else ctc_only
        if isinstance(beam, bool) or not isinstance(beam, int) or beam < 2:
            raise ValueError('asr.decode_mbr chooses among an n-best list: asr.decode_{} must be >= 2, '
                             'got {!r}'.format('beam_size' if ctc_only is None else 'ctc_only.beam_size', beam))
        return {'unit': unit, 'scale': float(scale)}

    @staticmethod
    def ctc_only_beam(asr_config):
        """ASR.decode_ctc's beam_size from asr.decode_ctc_only, validated; None when the key is absent (or false)."""
        conf = asr_config.get('decode_ctc_only')
        if conf is None or conf is False:
            return None
        if conf is True:
            conf = {}
        if not isinstance(conf, dict) or \
                set(conf) - ({'beam_size', 'lm_weight', 'length_bonus'} | set(ASRTester.GRAPH_KEYS) | set(ASRTester.WORD_KEYS)):
            raise ValueError('asr.decode_ctc_only must be a mapping with the key beam_size (and, optionally, lm_weight, '
                             'length_bonus, hotwords, hotword_bonus, ngram_lm, ngram_weight, word_lm and '
                             'word_lm_weight), got {!r}'.format(conf))
        beam = conf.get('beam_size', 8)
        if isinstance(beam, bool) or not isinstance(beam, int) or not 0 <= beam <= 32:
            raise ValueError('asr.decode_ctc_only.beam_size must be an integer in 0..32, got {!r}'.format(beam))
        return beam

    @staticmethod
    def ctc_only_lm(asr_config):
        """ASR.decode_ctc's lm_weight and length_bonus from asr.decode_ctc_only, validated: {'lm_weight': 0.0,
        'length_bonus': 0.0} when the keys (or the whole mapping) are absent."""
        import math
        beam = ASRTester.ctc_only_beam(asr_config)
        conf = asr_config.get('decode_ctc_only')
        conf = conf if isinstance(conf, dict) else {}
        out = {}
        for key in ('lm_weight', 'length_bonus'):
            v = conf.get(key, 0.0)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
                raise ValueError('asr.decode_ctc_only.{} must be a finite number, got {!r}'.format(key, v))
            out[key] = float(v)
        if beam == 0 and any(out.values()):
            raise ValueError('asr.decode_ctc_only: beam_size 0, the best path, has no LM term or length bonus; '
                             'got {!r}'.format(conf))
        if asr_config.get('decode_rescore') not in (None, False) and (out['lm_weight'] < 0 or out['length_bonus'] != 0):
            raise ValueError('asr.decode_ctc_only with asr.decode_rescore: the first pass takes lm_weight >= 0 and no '
                             'length_bonus (asr.decode_rescore.length_bonus is the second pass\'s), got {!r}'.format(conf))
        return out

    GRAPH_KEYS = ('hotwords', 'hotword_bonus', 'ngram_lm', 'ngram_weight')

    @staticmethod
    def _graph_keys(conf, name):
        """The four character-graph keys of the mapping conf, validated (name(key): what an error calls the key): None
        when none of them is present, else {'hotwords': [strings] or None, 'hotword_bonus': float, 'ngram_lm': path or
        None, 'ngram_weight': float}."""
        import math
        if not set(conf) & set(ASRTester.GRAPH_KEYS):
            return None
        words, path = conf.get('hotwords'), conf.get('ngram_lm')
        if words is None and path is None:
            raise ValueError('{} / {} need {} / {}, got {!r}'.format(
                name('hotword_bonus'), name('ngram_weight'), name('hotwords'), name('ngram_lm'), conf))
        if words is not None and (not isinstance(words, (list, tuple)) or not words or
                                  any(not isinstance(w, str) or not w for w in words)):
            raise ValueError('{} must be a non-empty list of non-empty strings, got {!r}'.format(name('hotwords'), words))
        if path is not None and (not isinstance(path, str) or not path):
            raise ValueError('{} must be the path of a CharGraph.save file, got {!r}'.format(name('ngram_lm'), path))
        out = {'hotwords': list(words) if words is not None else None, 'ngram_lm': path}
        for key, default, need in (('hotword_bonus', 1.0, words), ('ngram_weight', 0.5, path)):
            v = conf.get(key, default)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
                raise ValueError('{} must be a finite number >= 0, got {!r}'.format(name(key), v))
            if key in conf and need is None:
                raise ValueError('{} needs {}'.format(name(key), name('hotwords' if key == 'hotword_bonus' else 'ngram_lm')))
            out[key] = float(v)
        return out

    @staticmethod
    def beam_graph(asr_config):
        """The attention search's character-graph keys asr.decode_hotwords, asr.decode_hotword_bonus,
        asr.decode_ngram_lm and asr.decode_ngram_weight, validated as ctc_only_graph validates its own: None when none
        of them is present."""
        conf = {k: asr_config['decode_' + k] for k in ASRTester.GRAPH_KEYS if 'decode_' + k in asr_config}
        out = ASRTester._graph_keys(conf, 'asr.decode_{}'.format)
        if out is not None and asr_config.get('decode_ctc_only') not in (None, False):
            raise ValueError('asr.decode_{} with asr.decode_ctc_only: that mapping has its own graph keys '
                             '(asr.decode_ctc_only.hotwords, .ngram_lm); the attention beam search does not run'
                             .format(' / asr.decode_'.join(sorted(conf))))
        return out

    @staticmethod
    def ctc_only_graph(asr_config):
        """The character-graph keys of asr.decode_ctc_only, validated: None when none of them is present, else
        {'hotwords': [strings] or None, 'hotword_bonus': float, 'ngram_lm': path or None, 'ngram_weight': float}."""
        beam = ASRTester.ctc_only_beam(asr_config)
        conf = asr_config.get('decode_ctc_only')
        conf = conf if isinstance(conf, dict) else {}
        out = ASRTester._graph_keys(conf, 'asr.decode_ctc_only.{}'.format)
        if out is None:
            return None
        if beam == 0:
            raise ValueError('asr.decode_ctc_only: beam_size 0, the best path, has no graph term; got {!r}'.format(conf))
        if asr_config.get('decode_rescore') not in (None, False):
            raise ValueError('asr.decode_ctc_only: hotwords / ngram_lm with asr.decode_rescore is not built '
                             '(ASR.rescore has no graph term)')
        if ASRTester.ctc_only_lm(asr_config)['lm_weight'] != 0:
            raise ValueError('asr.decode_ctc_only: hotwords / ngram_lm together with a CharLM lm_weight in one search is '
                             'not built; give one of them')
        return out

    WORD_KEYS = ('word_lm', 'word_lm_weight')

    @staticmethod
    def ctc_only_word(asr_config):
        """The word-graph keys of asr.decode_ctc_only, validated: None when neither is present, else {'word_lm': path,
        'word_lm_weight': float}."""
        import math
        beam = ASRTester.ctc_only_beam(asr_config)
        conf = asr_config.get('decode_ctc_only')
        conf = conf if isinstance(conf, dict) else {}
        if not set(conf) & set(ASRTester.WORD_KEYS):
            return None
        path, weight = conf.get('word_lm'), conf.get('word_lm_weight', 0.5)
        if path is None:
            raise ValueError('asr.decode_ctc_only.word_lm_weight needs asr.decode_ctc_only.word_lm, got {!r}'.format(conf))
        if not isinstance(path, str) or not path:
            raise ValueError('asr.decode_ctc_only.word_lm must be the path of a WordGraph.save file, got {!r}'.format(path))
        if isinstance(weight, bool) or not isinstance(weight, (int, float)) or not math.isfinite(weight) or weight < 0:
            raise ValueError('asr.decode_ctc_only.word_lm_weight must be a finite number >= 0, got {!r}'.format(weight))
        if beam == 0:
            raise ValueError('asr.decode_ctc_only: beam_size 0, the best path, has no word LM; got {!r}'.format(conf))
        clash = sorted(set(conf) & {'hotwords', 'ngram_lm'})
        if clash:
            raise ValueError('asr.decode_ctc_only: word_lm together with {} in one search is not built; give one of '
                             'them'.format(' / '.join(clash)))
        if asr_config.get('decode_rescore') not in (None, False):
            raise ValueError('asr.decode_ctc_only: word_lm with asr.decode_rescore is not built (ASR.rescore has no '
                             'graph term)')
        if ASRTester.ctc_only_lm(asr_config)['lm_weight'] != 0:
            raise ValueError('asr.decode_ctc_only: word_lm together with a CharLM lm_weight in one search is not built; '
                             'give one of them')
        return {'word_lm': path, 'word_lm_weight': float(weight)}

    def load_word_graph(self, conf):
        """(WordGraph, graph_weight) of ctc_only_word's keys, checked against the model's classes and space."""
        from .word_graph import WordGraph
        if not os.path.isfile(conf['word_lm']):
            raise ValueError('asr.decode_ctc_only.word_lm: no file {!r}'.format(conf['word_lm']))
        wg = WordGraph.load(conf['word_lm'])
        V, space = self.mapper.get_dim(), self.mapper.char_to_ind(' ')
        if wg.n_classes != V or wg.space != space or wg.blank != ops.CTC_BLANK:
            raise ValueError('asr.decode_ctc_only.word_lm: the graph has {} classes, the space {} and the blank {}, the '
                             'model {}, {} and {}'.format(wg.n_classes, wg.space, wg.blank, V, space, ops.CTC_BLANK))
        return wg, conf['word_lm_weight']

    def build_ctc_graph(self, conf, name='asr.decode_ctc_only.{}'.format):
        """(CharGraph, graph_weight) of ctc_only_graph's (or, with its name(key), beam_graph's) keys: the hotwords'
        graph at weight 1, the n-gram graph at ngram_weight, or the product of the two, each factor pre-scaled, at
        weight 1."""
        from .char_graph import CharGraph
        V, hot, lm = self.mapper.get_dim(), None, None
        if conf['hotwords'] is not None:
            try:
                phrases = [[self.mapper.char_to_ind(ch) for ch in w] for w in conf['hotwords']]
            except KeyError as e:
                raise ValueError('{}: {!r} is no character of the model'.format(name('hotwords'), e.args[0]))
            hot = CharGraph.hotwords(phrases, conf['hotword_bonus'], V, ops.CTC_BLANK)
        if conf['ngram_lm'] is not None:
            if not os.path.isfile(conf['ngram_lm']):
                raise ValueError('{}: no file {!r}'.format(name('ngram_lm'), conf['ngram_lm']))
            lm = CharGraph.load(conf['ngram_lm'])
            if lm.n_classes != V:
                raise ValueError('{}: the graph has {} classes, the model {}'.format(name('ngram_lm'), lm.n_classes, V))
        if hot is not None and lm is not None:
            return CharGraph.product(lm.scaled(conf['ngram_weight']), hot), 1.0
        return (hot, 1.0) if hot is not None else (lm, conf['ngram_weight'])

    @staticmethod
    def rescore_args(asr_config):
        """ASR.decode_two_pass's keywords from asr.decode_rescore, validated; None when the key is absent (or false)."""
        import math
        conf = asr_config.get('decode_rescore')
        if conf is None or conf is False:
            return None
        if conf is True:
            conf = {}
        if not isinstance(conf, dict) or set(conf) - {'ctc_weight', 'length_bonus'}:
            raise ValueError('asr.decode_rescore must be a mapping with the keys ctc_weight and length_bonus, '
                             'got {!r}'.format(conf))
        ctc_weight, bonus = conf.get('ctc_weight', 0.3), conf.get('length_bonus', 0.0)
        if (isinstance(ctc_weight, bool) or not isinstance(ctc_weight, (int, float)) or not math.isfinite(ctc_weight)
                or not 0 <= ctc_weight <= 1):
            raise ValueError('asr.decode_rescore.ctc_weight must be a number in [0, 1], got {!r}'.format(ctc_weight))
        if isinstance(bonus, bool) or not isinstance(bonus, (int, float)) or not math.isfinite(bonus):
            raise ValueError('asr.decode_rescore.length_bonus must be a finite number, got {!r}'.format(bonus))
        ctc_only = ASRTester.ctc_only_beam(asr_config)
        if ctc_only is None or ctc_only < 1:
            raise ValueError('asr.decode_rescore re-ranks the CTC prefix search\'s list: it needs '
                             'asr.decode_ctc_only with beam_size >= 1, got {!r}'.format(asr_config.get('decode_ctc_only')))
        return {'ctc_weight': ctc_weight, 'length_bonus': float(bonus)}

    def __init__(self, config, paras):
        super().__init__(config, paras, 'asr')
        self.decode_file = "_".join(
            ['decode', 'beam', str(self.config['asr']['decode_beam_size']),
             'len', str(self.config['asr']['max_decode_step_ratio'])])

    def load_data(self):
        (self.mapper, self.ds, self.test_set) = load_asr_dataset(
            self.config['asr']['test_index'], batch_size=self.test_batch_size,
            n_jobs=self.set_if_exists('loader_jobs', 8), use_gpu=self.paras.gpu)

    def set_model(self):
        self.decode_score = bool(self.config['asr'].get('decode_score', False))
        self.decode_align = bool(self.config['asr'].get('decode_align', False))
        if self.decode_align and 'ctc_weight' not in self.config['asr']['mdl']:
            raise ValueError('asr.decode_align needs a model with a ctc_head: set asr.mdl.ctc_weight '
                             '(ctc.JointCTCASR)')
        self.decode_ctc_only = self.ctc_only_beam(self.config['asr'])
        self.decode_rescore = self.rescore_args(self.config['asr'])
        self.decode_ctc_lm = self.ctc_only_lm(self.config['asr'])
        graph_conf = self.ctc_only_graph(self.config['asr'])
        self.decode_ctc_graph = None if graph_conf is None else self.build_ctc_graph(graph_conf)
        word_conf = self.ctc_only_word(self.config['asr'])
        self.decode_ctc_word = None if word_conf is None else self.load_word_graph(word_conf)
        beam_graph_conf = self.beam_graph(self.config['asr'])
        self.decode_beam_graph = None if beam_graph_conf is None else self.build_ctc_graph(
            beam_graph_conf, 'asr.decode_{}'.format)
        if self.decode_ctc_only is not None:
            if 'ctc_weight' not in self.config['asr']['mdl']:
                raise ValueError('asr.decode_ctc_only needs a model with a ctc_head: set asr.mdl.ctc_weight '
                                 '(ctc.JointCTCASR)')
            clash = ['decode_ctc_weight'] if self.config['asr'].get('decode_ctc_weight', 0) != 0 else []
            clash += ['decode_' + k for k in self.decode_terms(self.config['asr'])[0] if k != 'coverage_threshold']
            if clash:
                raise ValueError('asr.decode_ctc_only runs no attention beam search: it cannot be combined with '
                                 'asr.{}'.format(', asr.'.join(clash)))
        asr_cls = ASR
        if 'ctc_weight' in self.config['asr']['mdl']:
            from .ctc import JointCTCASR
            asr_cls = JointCTCASR
        self.asr_model = self.setup_module(asr_cls, self.ckppath, self.mapper.get_dim(),
                                           **self.config['asr']['mdl'])
        self.asr_model.eval()
        lm_conf = self.config['char_lm']            # conf/default.yaml:84-89 keeps it under mdl; src/trainer.py:568 reads it beside mdl
        hidden = lm_conf['mdl']['hidden_size'] if 'mdl' in lm_conf else lm_conf['hidden_size']
        lm_path = os.path.join(self.ckpdir, 'char_lm.cpt')
        if os.path.isfile(lm_path):
            self.lm = self.setup_module(CharLM, lm_path, self.ds.get_char_dim(), hidden)
        else:
            self.verbose('No language model found at {}: decoding with a freshly initialised CharLM, '
                         'as the reference does'.format(lm_path))
            self.lm = CharLM(self.ds.get_char_dim(), hidden).to(self.device)
        self.lm.eval()
        self.lm_weight = self.config['asr']['decode_lm_weight']
        self.decode_beam_size = self.config['asr']['decode_beam_size']
        self.njobs = self.config['asr']['decode_jobs']
        self.decode_step_ratio = self.config['asr']['max_decode_step_ratio']
        self.decode_file += '_lm{:}'.format(self.config['asr']['decode_lm_weight'])
        self.decode_ctc_weight = self.config['asr'].get('decode_ctc_weight', 0)
        if self.decode_ctc_weight > 0:
            self.decode_file += '_ctc{:}'.format(self.decode_ctc_weight)
        if self.decode_ctc_only is not None:
            self.decode_file += '_ctconly{:}'.format(self.decode_ctc_only)
            if self.decode_ctc_lm['lm_weight'] != 0:
                self.decode_file += '_clm{:}'.format(self.decode_ctc_lm['lm_weight'])
                if self.decode_ctc_lm['length_bonus'] != 0:
                    self.decode_file += '_clb{:}'.format(self.decode_ctc_lm['length_bonus'])
            if graph_conf is not None:
                if graph_conf['hotwords'] is not None:
                    self.decode_file += '_hw{:}x{:}'.format(len(graph_conf['hotwords']), graph_conf['hotword_bonus'])
                if graph_conf['ngram_lm'] is not None:
                    self.decode_file += '_ng{:}'.format(graph_conf['ngram_weight'])
                if self.decode_ctc_lm['length_bonus'] != 0:
                    self.decode_file += '_clb{:}'.format(self.decode_ctc_lm['length_bonus'])
            if word_conf is not None:
                self.decode_file += '_wlm{:}'.format(word_conf['word_lm_weight'])
                if self.decode_ctc_lm['length_bonus'] != 0:
                    self.decode_file += '_clb{:}'.format(self.decode_ctc_lm['length_bonus'])
        if self.decode_rescore is not None:
            self.decode_file += '_rescore{:}'.format(self.decode_rescore['ctc_weight'])
        if beam_graph_conf is not None:
            if beam_graph_conf['hotwords'] is not None:
                self.decode_file += '_hw{:}x{:}'.format(len(beam_graph_conf['hotwords']), beam_graph_conf['hotword_bonus'])
            if beam_graph_conf['ngram_lm'] is not None:
                self.decode_file += '_ng{:}'.format(beam_graph_conf['ngram_weight'])
        self.decode_term_args, suffix = self.decode_terms(self.config['asr'])
        self.decode_file += suffix
        if self.decode_align:
            self.decode_file += '_align'
        self.decode_mbr = self.mbr_args(self.config['asr'])
        if self.decode_mbr is not None:
            self.decode_file += '_mbr{}'.format(self.decode_mbr['unit'])

    def exec(self, lm_weight=None):
        """-> the decoded strings, one per utterance of the test index, in index order."""
        if lm_weight is None:
            lm_weight = self.lm_weight
        beam = self.decode_beam_size
        if isinstance(beam, bool) or not isinstance(beam, int) or not 1 <= beam <= 32:
            raise ValueError('asr.decode_beam_size must be an integer in 1..32, got {!r}'.format(beam))
        ctc_weight = self.decode_ctc_weight
        if isinstance(ctc_weight, bool) or not isinstance(ctc_weight, (int, float)) or not 0 <= ctc_weight <= 1:
            raise ValueError('asr.decode_ctc_weight must be a number in [0, 1], got {!r}'.format(ctc_weight))
        terms = self.decode_term_args
        if self.decode_beam_graph is not None:       # the attention search's character graph: two more keywords
            terms = dict(terms, graph=self.decode_beam_graph[0], graph_weight=self.decode_beam_graph[1])
        ctc_only = self.decode_ctc_only
        self.verbose('Start decoding ({}{}{})'.format(
            ('CTC only, ' + ('prefix beam search, beam size {}'.format(ctc_only) if ctc_only else 'best path'))
            if ctc_only is not None else
            'beam search, beam size {}'.format(beam) if beam > 1 else 'greedy, beam size 1',
            ', joint CTC / attention scores, CTC weight {}'.format(ctc_weight) if ctc_weight > 0 else '',
            ''.join(', {} {}'.format(k.replace('_', ' '), v) for k, v in self.decode_term_args.items()) +
            (', character graph of {} states at weight {}'.format(self.decode_beam_graph[0].n_states,
                                                                  self.decode_beam_graph[1])
             if self.decode_beam_graph is not None else '')))
        self.verbose('Number of utts to decode : {}, {} per launch.'.format(len(self.test_set), self.decode_group))
        results, xs, x_lens, ys = [], [], [], []
        if self.decode_align:
            self.last_alignments = []
        if self.decode_score:
            self.last_scores = []
        mbr_stats = ErrorStats()
        if self.decode_mbr is not None:
            self.last_mbr_choices = []

        def flush():
            if xs:
                if self.decode_rescore is not None:
                    texts = [hyps[0][0] for hyps in
                             self.asr_model.decode_two_pass(xs, x_lens, self.lm, self.mapper, lm_weight,
                                                            beam_size=ctc_only, **self.decode_rescore,
                                                            first_lm_weight=self.decode_ctc_lm['lm_weight'])]
                elif ctc_only is not None and self.decode_ctc_graph is not None:
                    texts = [hyps[0][0] for hyps in
                             self.asr_model.decode_ctc(xs, x_lens, self.mapper, beam_size=ctc_only,
                                                       length_bonus=self.decode_ctc_lm['length_bonus'],
                                                       graph=self.decode_ctc_graph[0],
                                                       graph_weight=self.decode_ctc_graph[1])]
                elif ctc_only is not None and self.decode_ctc_word is not None:
                    texts = [hyps[0][0] for hyps in
                             self.asr_model.decode_ctc(xs, x_lens, self.mapper, beam_size=ctc_only,
                                                       length_bonus=self.decode_ctc_lm['length_bonus'],
                                                       word_graph=self.decode_ctc_word[0],
                                                       graph_weight=self.decode_ctc_word[1])]
                elif ctc_only is not None:
                    texts = [hyps[0][0] for hyps in
                             self.asr_model.decode_ctc(xs, x_lens, self.mapper, beam_size=ctc_only, rnn_lm=self.lm,
                                                       **self.decode_ctc_lm)]
                else:
                    texts = self.asr_model.decode_many(xs, x_lens, self.lm, self.mapper, lm_weight,
                                                       beam_size=beam, ctc_weight=ctc_weight, **terms)
                if self.decode_mbr is not None:  # the n-best lists are still on the device: one launch for the group
                    chosen = self.asr_model.mbr(self.mapper, posterior='softmax', **self.decode_mbr)
                    texts = [m.text for m in chosen]
                    self.last_mbr_choices.extend(m.k for m in chosen)
                results.extend(texts)
                if self.decode_score:            # the hypotheses are still on the device: one launch for the group
                    self.last_scores.extend(self.asr_model.score(ys, self.mapper))
                    if self.decode_mbr is not None:
                        for rows, m in zip(self.asr_model.last_score_rows, chosen):
                            mbr_stats.add(rows[max(m.k, 0)][:4], rows[max(m.k, 0)][4:])
                if self.decode_align:            # on the group's encoder outputs: no second encode
                    self.last_alignments.extend(self.asr_model.align(
                        xs, x_lens, texts, self.mapper, encoded=self.asr_model.last_encoded_packed))
                del xs[:], x_lens[:], ys[:]

        for b_ind, (x, y) in enumerate(self.test_set):
            x, x_len = prepare_x(x, self.device)
            for i in range(x.shape[0]):              # test_batch_size is 1 in the reference's configs
                xs.append(x[i:i + 1, :x_len[i]])
                x_lens.append([x_len[i]])
                if self.decode_score:
                    ys.append(y.squeeze(0)[i])
            if len(xs) >= self.decode_group:
                flush()
        flush()
        if self.decode_score:
            best, oracle = ErrorStats(), ErrorStats()
            for sc in self.last_scores:
                best.add(sc.chars, sc.words)
                oracle.add(sc.oracle[1], sc.oracle[2])
            self.last_error_rates = {'cer': best.cer, 'wer': best.wer, 'oracle_cer': oracle.cer,
                                     'oracle_wer': oracle.wer, 'chars': tuple(best.chars), 'words': tuple(best.words)}
            if self.decode_mbr is not None:
                self.last_error_rates.update(mbr_cer=mbr_stats.cer, mbr_wer=mbr_stats.wer)
                self.verbose('MBR choice ({}s, scale {}): CER {:.4f} WER {:.4f}'.format(
                    self.decode_mbr['unit'], self.decode_mbr['scale'], mbr_stats.cer, mbr_stats.wer))
            self.verbose('CER {:.4f} WER {:.4f} (oracle CER {:.4f} WER {:.4f}); characters S/D/I/N {}/{}/{}/{}, '
                         'words S/D/I/N {}/{}/{}/{}'.format(best.cer, best.wer, oracle.cer, oracle.wer,
                                                            *(best.chars + best.words)))
        return results


class TAETrainer(Trainer):
    """Trains the text autoencoder, and through it the ASR model's attention / speller / embedding /
    char_trans (src/trainer.py:594-758; config 5's first leg).  With Adam (conf/default.yaml:43-45) on the
    GPU one iteration of exec() is ONE engine.TAETrainStep call; any other optimizer type takes the
    reference's sequence (zero_grad, forward, backward, Solver.step over the text autoencoder's parameters)."""

    def __init__(self, config, paras):
        super().__init__(config, paras, 'tae')

    def load_data(self):
        """Text only, with noise: the loaders yield (clean_y, noised_y) (src/trainer.py:601-614)."""
        (self.mapper, self.dataset, self.train_set) = load_asr_dataset(
            self.config['tae']['train_index'], batch_size=self.train_batch_size, use_gpu=self.paras.gpu,
            text_only=True, drop_rate=self.config['tae']['drop_rate'],
            n_jobs=self.set_if_exists('loader_jobs', 8))
        (_, _, self.valid_set) = load_asr_dataset(
            self.config['tae']['valid_index'], batch_size=self.valid_batch_size, use_gpu=self.paras.gpu,
            text_only=True, drop_rate=self.config['tae']['drop_rate'],
            n_jobs=self.set_if_exists('loader_jobs', 8))

    def set_model(self, asrpath=None, asr_model=None):
        """src/trainer.py:616-644.  asr_model (this build): an ASR object that is already in memory -- the
        Seed loop's legs then train the SAME parameters in turn without going through a checkpoint."""
        from .text_autoencoder import TextAutoEncoder
        (self.asrpath_in, self.asrpath_out) = self.genpath(asrpath, 'asr')
        self.asr_model = asr_model if asr_model is not None else self.setup_module(
            ASR, self.asrpath_in, self.mapper.get_dim(), **self.config['asr']['mdl'])
        self.text_autoenc = self.setup_module(TextAutoEncoder, self.ckppath, self.mapper.get_dim(),
                                              **self.config['tae']['mdl'])
        opt = self.config['tae']['opt']
        self.train_step = None
        if opt['type'] == 'Adam' and self.device.type == 'cuda':
            from .engine import TAETrainStep
            self.train_step = TAETrainStep(self.asr_model, self.text_autoenc, lr=opt['learning_rate'], eps=1e-8,
                                           grad_clip=5.0)
            self.optim = self.train_step.optim
        else:
            # the optimizer steps the text autoencoder, the ASR character embedding, attention module,
            # speller and char_trans layer (src/trainer.py:625-641)
            self.optim = getattr(torch.optim, opt['type'])(
                list(self.text_autoenc.parameters()) + list(self.asr_model.embed.parameters()) +
                list(self.asr_model.attention.parameters()) + list(self.asr_model.decoder.parameters()) +
                list(self.asr_model.char_trans.parameters()), lr=opt['learning_rate'], eps=1e-8)

    def _loss(self, enc_out, y):
        """src/trainer.py:662-672."""
        from .text_autoencoder import tae_loss
        if not enc_out.is_cuda:
            raise RuntimeError('ss_asr_amd computes on the GPU only')
        return tae_loss(enc_out, y)

    def _prepare(self, raw):
        """-> (y, y_noise, y_lens, y_noise_lens)"""
        (y, y_lens), (y_noise, y_noise_lens) = (prepare_y(r, device=self.device) for r in raw)
        return y, y_noise, y_lens, y_noise_lens

    def _reference(self, batch):
        y, y_noise, y_lens, y_noise_lens = batch
        self.optim.zero_grad()
        # decode steps == longest target
        _, enc_out = self.text_autoenc(self.asr_model, y, y_noise, max(y_lens), noise_lens=y_noise_lens)
        loss = self._loss(enc_out, y)
        loss.backward()
        self.step(self.text_autoenc.parameters(), self.optim)
        return loss

    def _log(self, loss):
        self.lg.scalar('train_loss', loss.item(), self.tr.step)

    def _checkpoint(self):
        return ((self.text_autoenc, self.ckppath), (self.asr_model, self.asrpath_out))

    def valid(self):
        """src/trainer.py:683-748."""
        self.text_autoenc.eval()
        self.asr_model.eval()
        total, n_batches = 0.0, 0
        y = enc_out = None
        with torch.no_grad():
            for b_idx, (y, y_noise) in enumerate(self.valid_set):
                self.verbose('Validation step -( {} / {} )'.format(b_idx, len(self.valid_set)), progress=True)
                y, y_lens = prepare_y(y, device=self.device)
                y_noise, y_noise_lens = prepare_y(y_noise, device=self.device)
                _, enc_out = self.text_autoenc(self.asr_model, y, y_noise, max(y_lens), noise_lens=y_noise_lens)
                total += float(self._loss(enc_out, y))
                n_batches += 1
        ops.check_persistent_status()
        self.text_autoenc.train()
        self.asr_model.train()
        if n_batches == 0:
            return
        avg_loss = total / n_batches
        if self.rank != 0:
            return
        # compare the strings of the last batch
        labels = [self.mapper.translate(l) for l in y.cpu()]
        predicts = [self.mapper.translate(p) for p in np.argmax(enc_out.cpu().numpy(), axis=-1)]
        for i in range(min(self.valid_batch_size, len(labels))):
            self.lg.text('eval_text' + str(i), '{} |vs.| {}'.format(labels[i], predicts[i]), self.tr.step)
        self.lg.scalar('eval_loss', avg_loss, self.tr.step)
        if self._keep_best(avg_loss, self.text_autoenc):
            self.verbose("Both the text autoencoder and ASR have been saved")


class ADVTrainer(Trainer):
    """Adversarial training of the Listener against the text encoder's frames (src/trainer.py:909-1124;
    config 5's second leg).  Generator: the ASR model's Listener; data distribution: the text autoencoder's
    encoder; discriminator: discriminator.Discriminator.  One iteration of exec() is ONE engine.ADVTrainStep
    call when G_opt / D_opt are Adadelta or Adam; any other optimizer type takes the reference's sequence with
    torch optimizers (`_reference`).

    The reference's ADVTrainer cannot run as shipped; what is fixed here, and
    nothing else: `self.loss_metric` (used at :984, never set) is nn.BCELoss -- on the ssasr_bce kernels; the
    validation index is `adv.eval_index` when the config has it (:918) and `adv.valid_index` (the key
    conf/default.yaml:74 carries) otherwise; the character-LM dataset of :922-924 (`chunk_size`,
    `lm_train_index`: absent from the yaml, and never read by exec or valid) is not loaded."""

    def __init__(self, config, paras):
        super().__init__(config, paras, 'adv')

    def load_data(self):
        n_jobs = self.set_if_exists('loader_jobs', 8)
        (self.mapper, self.dataset, self.train_set) = load_asr_dataset(
            self.config['adv']['train_index'], batch_size=self.train_batch_size, use_gpu=self.paras.gpu,
            n_jobs=n_jobs)
        eval_index = self.config['adv'].get('eval_index', self.config['adv'].get('valid_index'))
        (_, _, self.valid_set) = load_asr_dataset(eval_index, batch_size=self.valid_batch_size,
                                                  use_gpu=self.paras.gpu, n_jobs=n_jobs)

    def set_model(self, asrpath=None, taepath=None, asr_model=None, text_autoenc=None):
        """src/trainer.py:926-948.  asr_model / text_autoenc (this build): objects already in memory."""
        from .discriminator import Discriminator
        from .engine import ADVTrainStep
        from .text_autoencoder import TextAutoEncoder
        (self.asrpath_in, self.asrpath_out) = self.genpath(asrpath, 'asr')
        (taepath_in, _) = self.genpath(taepath, 'tae')
        self.asr_model = asr_model if asr_model is not None else self.setup_module(
            ASR, self.asrpath_in, self.mapper.get_dim(), **self.config['asr']['mdl'])
        self.text_autoenc = text_autoenc if text_autoenc is not None else self.setup_module(
            TextAutoEncoder, taepath_in, self.mapper.get_dim(), **self.config['tae']['mdl'])
        self.discriminator = self.setup_module(Discriminator, self.ckppath, self.asr_model.encoder.get_outdim(),
                                               **self.config['adv']['mdl'])
        self.data_distribution = self.text_autoenc.encoder
        g, d = self.config['adv']['G_opt'], self.config['adv']['D_opt']
        fused = ('Adadelta', 'Adam')
        self.train_step = None
        if g['type'] in fused and d['type'] in fused and self.device.type == 'cuda':
            self.train_step = ADVTrainStep(self.asr_model, self.text_autoenc, self.discriminator,
                                           g_opt=(g['type'], g['learning_rate']), d_opt=(d['type'], d['learning_rate']),
                                           label_smoothing=self.config['adv']['label_smoothing'], grad_clip=5.0)
            self.G_optim, self.D_optim = self.train_step.G_optim, self.train_step.D_optim
        else:
            # any other optimizer type: the reference's sequence with torch optimizers (src/trainer.py:938-948)
            self.G_optim = getattr(torch.optim, g['type'])(self.asr_model.encoder.parameters(), lr=g['learning_rate'], eps=1e-8)
            self.D_optim = getattr(torch.optim, d['type'])(self.discriminator.parameters(), lr=d['learning_rate'], eps=1e-8)

    def _frames(self, x, x_lens, y):
        """(text-encoder frames without a graph, Listener frames with theirs)."""
        if self.train_step is not None:
            return self.train_step.frames(x, x_lens, y)
        if not x.is_cuda:
            raise RuntimeError('ss_asr_amd computes on the GPU only (no CPU path)')
        with torch.no_grad():
            real = self.data_distribution(y)
        fake, _ = self.asr_model.encoder(x, x_lens)
        return real, fake

    reports_worse = False

    def _prepare(self, raw):
        """-> (x, x_lens, y)"""
        return (*prepare_x(raw[0], device=self.device), prepare_y(raw[1], device=self.device)[0])

    def _reference(self, batch):
        """src/trainer.py:968-1032 with torch optimizers (the fused form is engine.ADVTrainStep)."""
        from .seed_ops import bce_loss
        x, x_lens, y = batch
        self.discriminator.zero_grad()
        real, fake = self._frames(x, x_lens, y)
        D_realloss = bce_loss(self.discriminator(real), 1.0 - self.config['adv']['label_smoothing'])
        D_realloss.backward()
        D_fakeloss = bce_loss(self.discriminator(fake.detach()), 0.0)
        D_fakeloss.backward()
        self.step(self.discriminator.parameters(), self.D_optim)
        self.asr_model.encoder.zero_grad()
        G_loss = bce_loss(self.discriminator(fake, frozen=True), 1.0)
        G_loss.backward()
        self.step(self.asr_model.encoder.parameters(), self.G_optim)
        return D_realloss, D_fakeloss, G_loss

    def _log(self, losses):
        D_realloss, D_fakeloss, G_loss = losses
        self.lg.scalar('discrim_real_loss_train', D_realloss.item(), self.tr.step)
        self.lg.scalar('discrim_fake_loss_train', D_fakeloss.item(), self.tr.step)
        self.lg.scalar('discrim_loss_train', (D_realloss + D_fakeloss).item(), self.tr.step)
        self.lg.scalar('gen_loss_train', G_loss.item(), self.tr.step)

    def _checkpoint(self):
        return ((self.discriminator, self.ckppath), (self.asr_model, self.asrpath_out))

    def valid(self):
        """src/trainer.py:1038-1113: the discriminator's two losses (real labels unsmoothed here, :1059) averaged
        over the validation batches; the last batch's first utterance goes to the embedding log."""
        from .seed_ops import bce_loss
        self.asr_model.eval()
        self.discriminator.eval()
        real_sum = fake_sum = 0.0
        n_batches = 0
        real_data = fake_data = None
        with torch.no_grad():
            for b_idx, (x, y) in enumerate(self.valid_set):
                self.verbose('Validation step - {} ( {} / {} )'.format(self.tr.step, b_idx, len(self.valid_set)),
                             progress=True)
                x, x_lens = prepare_x(x, device=self.device)
                y, _ = prepare_y(y, device=self.device)
                real_data, fake_data = self._frames(x, x_lens, y)
                real_sum += float(bce_loss(self.discriminator(real_data), 1.0))
                fake_sum += float(bce_loss(self.discriminator(fake_data), 0.0))
                n_batches += 1
        ops.check_persistent_status()
        self.asr_model.train()
        self.discriminator.train()
        if n_batches == 0 or self.rank != 0:
            return
        avg_real, avg_fake = real_sum / n_batches, fake_sum / n_batches
        real_emb, fake_emb = real_data[0], fake_data[0]
        self.lg.embedding('validation_emb', torch.cat((real_emb, fake_emb)).cpu(),
                          ['real'] * real_emb.shape[0] + ['fake'] * fake_emb.shape[0], self.tr.step)
        avg_loss = avg_real + avg_fake
        self.lg.scalar('discrim_real_loss_eval', avg_real, self.tr.step)
        self.lg.scalar('discrim_fake_loss_eval', avg_fake, self.tr.step)
        self.lg.scalar('discrim_loss_eval', avg_loss, self.tr.step)
        if self._keep_best(avg_loss, self.discriminator):
            self.verbose("Both the discriminator and ASR have been saved")


class SAETrainer(Trainer):
    """Trains the speech autoencoder and, through it, the ASR model's Listener on audio alone
    (src/trainer.py:760-907; config 5's third leg).  With Adam (conf/default.yaml:24-26) one iteration of
    exec() is ONE engine.SAETrainStep call; any other optimizer type takes the reference's sequence (zero_grad,
    forward, backward, Solver.step over the speech autoencoder's parameters) with the torch optimizer.  The spectrogram figures of valid()
    (:871-887, matplotlib + librosa's specshow) are logged as the pair of arrays they would draw."""

    def __init__(self, config, paras):
        super().__init__(config, paras, 'sae')

    def load_data(self):
        n_jobs = self.set_if_exists('loader_jobs', 8)
        (self.mapper, _, self.train_set) = load_asr_dataset(
            self.config['sae']['train_index'], batch_size=self.train_batch_size, use_gpu=self.paras.gpu, n_jobs=n_jobs)
        (_, _, self.valid_set) = load_asr_dataset(
            self.config['sae']['valid_index'], batch_size=self.valid_batch_size, use_gpu=self.paras.gpu, n_jobs=n_jobs)

    def set_model(self, asrpath=None, asr_model=None):
        """src/trainer.py:774-796.  asr_model (this build): an ASR object already in memory."""
        from .engine import SAETrainStep
        from .speech_autoencoder import SpeechAutoEncoder
        (self.asrpath_in, self.asrpath_out) = self.genpath(asrpath, 'asr')
        self.asr_model = asr_model if asr_model is not None else self.setup_module(
            ASR, self.asrpath_in, self.mapper.get_dim(), **self.config['asr']['mdl'])
        self.speech_autoenc = self.setup_module(SpeechAutoEncoder, self.ckppath, self.asr_model.encoder.out_dim,
                                                self.config['asr']['mdl']['feature_dim'], **self.config['sae']['mdl'])
        opt = self.config['sae']['opt']
        self.train_step = None
        if opt['type'] == 'Adam' and self.device.type == 'cuda':
            self.train_step = SAETrainStep(self.asr_model, self.speech_autoenc, opt=(opt['type'], opt['learning_rate']),
                                           grad_clip=5.0)
            self.optim = self.train_step.optim
        else:
            # any other optimizer type: the reference's sequence (zero_grad, forward, backward, Solver.step over the
            # speech autoencoder's parameters) with the torch optimizer over both parameter lists (src/trainer.py:789-794)
            self.optim = getattr(torch.optim, opt['type'])(
                list(self.speech_autoenc.parameters()) + list(self.asr_model.encoder.parameters()),
                lr=opt['learning_rate'], eps=1e-8)

    def _forward_loss(self, x, x_lens):
        """(loss, prediction [B, 8 T', F]) of src/trainer.py:805-818."""
        if self.train_step is not None:
            return self.train_step.forward_loss(x, x_lens)
        from .seed_ops import sae_loss
        if not x.is_cuda:
            raise RuntimeError('ss_asr_amd computes on the GPU only (no CPU path)')
        listener_out, _ = self.asr_model.encoder(x, x_lens)
        pred = self.speech_autoenc(x, listener_out)
        return sae_loss(pred, x, max(x_lens)), pred

    batches_line = 'Training set total {} batches.'

    def _prepare(self, raw):
        """-> (x, x_lens)"""
        return prepare_x(raw[0], device=self.device)

    def _reference(self, batch):
        self.optim.zero_grad()
        loss, _ = self._forward_loss(*batch)
        loss.backward()
        self.step(self.speech_autoenc.parameters(), self.optim)
        return loss

    def _log(self, loss):
        self.lg.scalar('train_loss', loss.item(), self.tr.step)

    def _checkpoint(self):
        return ((self.speech_autoenc, self.ckppath), (self.asr_model, self.asrpath_out))

    def valid(self):
        """src/trainer.py:840-897: the eval-mode loss (running batch-norm statistics) averaged over the
        validation batches; the last batch's utterances against their reconstructions go to the figure log."""
        self.speech_autoenc.eval()
        self.asr_model.eval()
        total, n_batches = 0.0, 0
        x = x_lens = pred = None
        with torch.no_grad():
            for b_idx, (x, y) in enumerate(self.valid_set):
                self.verbose('Validation step - {} ( {} / {} )'.format(self.tr.step, b_idx, len(self.valid_set)),
                             progress=True)
                x, x_lens = prepare_x(x, device=self.device)
                loss, pred = self._forward_loss(x, x_lens)
                total += float(loss)
                n_batches += 1
        ops.check_persistent_status()
        self.speech_autoenc.train()
        self.asr_model.train()
        if n_batches == 0 or self.rank != 0:
            return
        batch_t = max(x_lens)
        enc_final = torch.zeros(pred.shape[0], batch_t, pred.shape[2])
        enc_final[:, :pred.shape[1], :] = pred.cpu()
        for i in range(min(self.valid_batch_size, x.shape[0])):
            label_img = x[i, :x_lens[i], :].cpu().permute(1, 0)
            predict_img = enc_final[i, :x_lens[i], :].permute(1, 0)
            self.lg.figure('encode_compare_' + str(i), [label_img.numpy(), predict_img.numpy()], self.tr.step)
        avg_loss = total / n_batches
        self.lg.scalar('eval_loss', avg_loss, self.tr.step)
        self._keep_best(avg_loss, self.speech_autoenc)


# src/train.py:19-20 offers the choice 'AdvTrainer' and resolves it with getattr(trainer, ...); the reference's
# trainer.py only defines ADVTrainer -- here the CLI's spelling resolves
AdvTrainer = ADVTrainer


def asr_seed_train(config, paras):
    """The Seed loop, src/trainer.py:1126-1177 (`train.py Seed`): super-iterations in which three trainers take
    turns on ONE ASR model, handed from leg to leg through checkpoints under <ckpdir>/<name>/ exactly as the
    reference chains them -- TAETrainer reads and writes asr_1.cpt (it trains the attention / speller half),
    ADVTrainer reads asr_1.cpt and the text autoencoder's checkpoint and writes asr_2.cpt (it trains the Listener
    against the text encoder), SAETrainer reads asr_2.cpt and writes asr_3.cpt (Listener again, through the speech
    autoencoder).  The count of super-iterations is `seed_train.its` (the key :1146 reads) or, when the config
    only has it, `seed_train.super_its` (the key conf/default.yaml:103-104 carries).

    `seed_train.legs` (this build; default ['tae', 'adv', 'sae'], the reference's sequence) may also name 'asr':
    a supervised ASRTrainer leg on the checkpoint the previous leg wrote."""
    ckpdir = os.path.join(paras.ckpdir, paras.name)
    seed = config['seed_train']
    its = seed['its'] if 'its' in seed else seed['super_its']
    legs = seed.get('legs', ['tae', 'adv', 'sae'])
    cpt = lambda k: os.path.join(ckpdir, 'asr_%d.cpt' % k)
    for i in range(its):
        print('Starting Super Iteration {}'.format(i + 1))
        tae_path, last = None, cpt(1)
        for leg in legs:
            if leg == 'tae':
                print('Starting TAE training')
                solver = TAETrainer(config, paras)
                solver.load_data()
                solver.set_model(asrpath=(cpt(1), cpt(1)))
                tae_path, last = solver.ckppath, cpt(1)
            elif leg == 'adv':
                print('Starting ADV training')
                solver = ADVTrainer(config, paras)
                solver.load_data()
                solver.set_model(taepath=tae_path, asrpath=(cpt(1), cpt(2)))
                last = cpt(2)
            elif leg == 'sae':
                print('Starting SAE training')
                solver = SAETrainer(config, paras)
                solver.load_data()
                solver.set_model(asrpath=(cpt(2), cpt(3)))
                last = cpt(3)
            elif leg == 'asr':
                print('Starting ASR training')
                solver = ASRTrainer(config, paras)
                solver.load_data()
                solver.set_model(asrpath=(last, last))
            else:
                raise ValueError("seed_train leg %r (known: 'tae', 'adv', 'sae', 'asr')" % (leg,))
            solver.exec()
            solver.close()
            del solver
