"""The epoch level of training: the reference's Solver (src/solver.py:97-275,353-425) around `trainer.TrainStep`.

    eval_sets         <- train.py:59-75          the validation (`dset.valid`) and test (`dset.test`) sets: whole files, one per forward
    Solver.load       <- solver.py:103-134       continue from `checkpoint_file`, or from `continue_from` (`continue_best`, `keep_history`)
    Solver.run_epoch  <- solver.py:281-349       one pass over the training set in `data.EpochSampler` order
    Solver.run_pass   <- solver.py:172-199,353-425 and evaluate.py:136-170: validation losses and / or LSD and samples over a file set
    Solver.train      <- solver.py:136-274       epochs from len(history); validation, best states, evaluation, history file, checkpoint

What runs on the device is what already ran there: the generator's inference forward, `TrainStep.losses_of` (the same terms in the same
order as a training step) and `evaluate.lsd` (HIP STFT).  A pass adds the per-file loss vectors on the device and reads them ONCE.

Deviations from the reference, all deliberate:
  * no wandb and no spectrogram PNGs (`save_specs`);
  * LSD is measured on the tensors of the pass, not on 16-bit files read back from `samples_dir`;
  * the enhanced file names are a list of stems (`total_filenames += filename` of solver.py:372 appends characters);
  * best states loaded from a checkpoint are KEPT (solver.py:154 drops them, so `evaluate_on_best` after a resume tests the last state);
  * `steps=N` caps the training steps of this process;
  * `engines` in the checkpoint, and engines rebuilt at every epoch's start (see `run_epoch`).
As in the reference, every rank writes the samples of the files it owns (file i -> rank i mod W: its `tt_loader` is sharded and each
rank calls save_wavs); history, checkpoint and best files are rank 0's.
"""
import contextlib
import json
import logging
import os
import time

import torch

from . import data, distrib
from . import evaluate as ev
from .enhance import load_package, match_signal, save_wavs

logger = logging.getLogger(__name__)


def has_lists(path):
    """a json_dir counts as a data set when both of its file lists exist (the rule of `trainer.data_source`)"""
    return bool(path) and os.path.exists(os.path.join(str(path), 'lr.json')) and os.path.exists(os.path.join(str(path), 'hr.json'))


class EvalSet:
    """A validation / test set of one process: whole files, B = 1.  `item(i)` is (lr [1, 1, L], hr [1, 1, L']) on the device -- cut out of
    the device-resident store (`kind` "device": `DeviceLrHrStore.batch([i])`) or read by the host `LrHrSet` ("host"); the same tensors."""

    def __init__(self, dataset, store, device):
        self.dataset, self.store, self.device = dataset, store, torch.device(device)
        self.kind = 'host' if store is None else 'device'

    def __len__(self):
        return len(self.dataset)

    def stem(self, i):
        """whole-file items: item i is file i of the sorted hr list"""
        return os.path.splitext(os.path.basename(str(self.dataset.hr_set.files[self.dataset.hr_set.locate(i)[0]][0])))[0]

    def item(self, i):
        if self.store is not None:
            return self.store.batch([i])
        lr, hr = self.dataset[i]
        if self.dataset.with_path:
            lr, hr = lr[0], hr[0]
        return lr[None].to(self.device), hr[None].to(self.device)


def eval_sets(args, device, used_bytes=0, lib=None):
    """train.py:59-75 -> (cv, tt, valid_equals_test): each an `EvalSet` or None where `dset.valid` / `dset.test` has no lr.json / hr.json.
    The decoded files live on the device while they fit into what `used_bytes` (the training store) leaves of the ONE `+data_max_bytes`
    budget of the process; a set that does not fit, or `+data_on_device=false`, is read by the host.  Equal paths share one set."""
    exp = args.experiment
    dset = args.get('dset') or {}
    left = int(args.get('data_max_bytes', data.DEFAULT_MAX_BYTES)) - used_bytes

    def build(path, with_path):
        nonlocal left
        if not has_lists(path):
            return None
        ds = data.LrHrSet(str(path), exp.lr_sr, exp.hr_sr, stride=None, segment=None, with_path=with_path, upsample=exp.upsample)
        store = None
        if args.get('data_on_device', True):
            store = data.DeviceLrHrStore(ds, device, max(left, 0), lib=lib)
            if store is not None:
                left -= store.nbytes
        return EvalSet(ds, store, device)

    valid, test = dset.get('valid'), dset.get('test')
    same = bool(valid) and str(valid) == str(test)
    tt = build(test, True)
    cv = tt if same else build(valid, False)
    return cv, tt, same


def copy_state(state):
    return {k: v.detach().cpu().clone() for k, v in state.items()}


def repack(model):
    """weights written by load_state_dict: the packed images of the device engines follow"""
    if hasattr(model, 'repack'):
        model.repack()


@contextlib.contextmanager
def swap_state(model, state):
    """src/utils.py swap_state: `state` in the model for the duration, the model's own state back afterwards, bit for bit"""
    old = copy_state(model.state_dict())
    model.load_state_dict(state)
    repack(model)
    try:
        yield
    finally:
        model.load_state_dict(old)
        repack(model)


def pull_metric(history, name):
    return [h[name] for h in history if name in h]


class Solver:
    def __init__(self, args, models, optimizers, step, source, device, per_rank, lib=None):
        """models / optimizers / step: what `trainer.build_models`, `build_optimizers` and `TrainStep` made; source: `trainer.data_source`.
        lib: tests' explicitly loaded library for the stores of the validation and test sets."""
        self.args, self.models, self.optimizers, self.step, self.source = args, models, optimizers, step, source
        self.device, self.per_rank = torch.device(device), per_rank
        self.epochs = int(args.epochs)
        used = source.store.nbytes if getattr(source, 'store', None) is not None else 0
        self.cv, self.tt, self.valid_equals_test = eval_sets(args, self.device, used, lib=lib)
        self.history, self.best_states = [], {}
        self.done = 0                                            # training steps of this process (`steps=N`)
        cap = args.get('steps')
        self.cap = None if cap is None else int(cap)
        self.valid_files = []                                    # the last pass, per file: (stem, {term: value}) of this rank

    # ------------------------------------------------------------------ resume (solver.py:103-134)
    def load(self):
        """call once, after the optimizers exist and before the first step -> the file that was loaded, or None"""
        args = self.args
        load_from, best, keep_history = None, False, True
        if args.checkpoint and os.path.exists(str(args.checkpoint_file)) and not args.restart:
            load_from = str(args.checkpoint_file)
        elif args.continue_from:
            load_from, best, keep_history = str(args.continue_from), bool(args.continue_best), bool(args.keep_history)
        if load_from is None:
            return None
        logger.info('Loading checkpoint model: %s', load_from)
        package = load_package(load_from)
        if best:
            states = package['best_states']
            states = {n: p['state'] for n, p in states['models'].items()} if 'models' in states else states
            if not states:
                raise ValueError(f'continue_best: {load_from} holds no best states')
        else:
            states = {n: p['state'] for n, p in package['models'].items()}
        for name, state in states.items():
            self.models[name].load_state_dict(state)
            repack(self.models[name])
        if not best:
            for name, sd in package['optimizers'].items():
                self.optimizers[name].load_state_dict(sd)
            for name, sd in (package.get('engines') or {}).items():      # the training engine's forward count and LayerScale boosts
                self.models[name].load_train_state(sd)
        if keep_history:
            self.history = list(package['history'])
        self.best_states = {n: copy_state(s) for n, s in package['best_states'].items() if n in self.models}
        return load_from

    # ------------------------------------------------------------------ one training epoch (solver.py:281-349)
    def run_epoch(self, epoch):
        """-> the epoch's record (today's keys), or None when `steps=N` is used up"""
        if self.cap is not None and self.done >= self.cap:
            return None
        source, dev = self.source, self.device
        # every epoch starts from the engine state a resumed run starts from: weight images built from the weights, the gather replay
        # compiled again at the first step -- so that "epoch k" is one computation, whichever process runs it
        for m in self.models.values():
            if hasattr(m, 'reset_train_engine'):
                m.reset_train_engine()
            if hasattr(m, 'reset_pack'):
                m.reset_pack()
        batches = source.batches(epoch, self.per_rank)
        if self.cap is not None:
            batches = batches[:self.cap - self.done]
        if dev.type == 'cuda':
            torch.cuda.synchronize()
        distrib.barrier()
        t0 = time.time()
        acc, keys, seen = None, None, 0
        for lr, hr in source.load(batches):
            rec = self.step(lr, hr)
            if keys is None:
                keys = sorted(rec)
            vals = torch.stack([rec[k].float() for k in keys])
            acc = vals if acc is None else acc + vals            # (on the device: no host round trip per step)
            seen += lr.shape[0]
        if dev.type == 'cuda':
            torch.cuda.synchronize()
        dt = distrib.max_over_ranks(time.time() - t0)
        n = len(batches)
        self.done += n
        avg = distrib.average([v / n for v in acc.tolist()], seen)               # solver.py's logged losses: averaged over ranks
        vals = dict(zip(keys, avg))
        if any(v != v or abs(v) == float('inf') for v in vals.values()):
            raise RuntimeError(f'epoch {epoch}: non-finite loss {vals}')
        return {'epoch': epoch, 'steps': n, 'ms_per_step': round(1e3 * dt / n, 2), 'world_size': distrib.world_size,
                'batch_per_rank': self.per_rank, 'data': source.kind, **{k: round(v, 6) for k, v in vals.items()}}

    # ------------------------------------------------------------------ validation / evaluation over whole files
    def run_pass(self, eset, want_losses, want_lsd=False, samples=False):
        """One forward per file of this rank's shard (file i -> rank i mod W), generator in eval() under no_grad:
        pr = match_signal(dmodel(lr), len(hr)); with want_losses the terms of `TrainStep.losses_of(pr, hr)` and their `total`, summed as
        a training step sums them; with want_lsd `evaluate.lsd(hr, pr)`; with samples `<samples_dir>/<stem>_{lr,hr,pr}.wav` of the first
        `enhance_samples_limit` files.  -> ({term: mean over the files of all ranks}, stems of the files whose samples were written).
        The per-file vectors stay on the device and are read once; the pass leaves the generator in the mode it found and no record
        in the critics."""
        args, exp = self.args, self.args.experiment
        if len(eset) < distrib.world_size:
            raise ValueError(f'{len(eset)} files for {distrib.world_size} ranks: every rank needs one')
        gen = self.models['generator']
        was_training = gen.training
        limit = int(args.get('enhance_samples_limit', -1))
        if samples:
            os.makedirs(str(args.samples_dir), exist_ok=True)
        rows, keys, stems, written = [], None, [], []
        gen.eval()
        try:
            with torch.no_grad():
                for i in distrib.shard_indices(len(eset)):
                    lr, hr = eset.item(i)
                    pr = match_signal(self.step.dmodel(lr), hr.shape[-1])
                    vals = {}
                    if want_losses:
                        ls = self.step.losses_of(pr, hr)
                        vals['total'] = sum(ls['generator'].values())
                        vals.update({'generator_' + k: v for k, v in ls['generator'].items()})
                        vals.update({'discriminator_' + k: v for k, v in ls['discriminator'].items()})
                    if want_lsd:
                        vals['lsd'] = ev.lsd(hr.squeeze(1).float(), pr.squeeze(1).float())
                    if keys is None:
                        keys = list(vals)
                    rows.append(torch.stack([vals[k].detach().float() for k in keys]))
                    stems.append(eset.stem(i))
                    if samples and (limit < 0 or i < limit):
                        save_wavs([pr[0]], [lr[0]], [hr[0]], [os.path.join(str(args.samples_dir), stems[-1])], exp.lr_sr, exp.hr_sr)
                        written.append(stems[-1])
        finally:
            gen.train(was_training)
            for m in self.models.values():                       # a record of D(fake) || D(real) made here must not outlive the pass
                if hasattr(m, 'drop_record'):
                    m.drop_record()
        mat = torch.stack(rows)
        host = torch.cat([mat, mat.sum(0, keepdim=True)]).tolist()               # the ONE host read of the pass
        self.valid_files = [(s, dict(zip(keys, r))) for s, r in zip(stems, host[:-1])]
        n = len(rows)
        mean = dict(zip(keys, distrib.average([v / n for v in host[-1]], n)))
        if any(v != v or abs(v) == float('inf') for v in mean.values()):
            raise RuntimeError(f'non-finite value in a validation / evaluation pass: {mean}')
        return mean, written

    def validate(self, epoch, enhance=False):
        """solver.py:172-199 -> ({'total', 'evaluation' (the same number), every term}, lsd or None).  With `valid_equals_test` the pass runs
        over the test set and, on an evaluation epoch (`enhance`), measures LSD and writes the samples on the way."""
        if self.valid_equals_test:
            mean, _ = self.run_pass(self.tt, True, want_lsd=enhance, samples=enhance)
        else:
            mean, _ = self.run_pass(self.cv, True)
        lsd = mean.pop('lsd', None)
        out = {'total': mean['total'], 'evaluation': mean['total']}
        out.update({k: v for k, v in mean.items() if k != 'total'})
        return out, lsd

    def evaluate(self, epoch):
        """solver.py:214-259 -> mean LSD over the test set, with the best generator swapped in under `evaluate_on_best`"""
        gen = self.models['generator']
        best = self.best_states.get('generator') if self.args.evaluate_on_best else None
        with swap_state(gen, best) if best is not None else contextlib.nullcontext():
            mean, _ = self.run_pass(self.tt, False, want_lsd=True, samples=True)
        return mean['lsd']

    # ------------------------------------------------------------------ solver.py:136-274
    def train(self):
        args = self.args
        best_loss = (pull_metric(self.history, 'best_loss') or [None])[-1]
        for epoch in range(len(self.history), self.epochs):
            rec = self.run_epoch(epoch)
            if rec is None:
                break
            last = epoch == self.epochs - 1
            eval_now = self.tt is not None and ((epoch + 1) % int(args.eval_every) == 0 or last)
            evaluation_loss, lsd = None, None
            if args.cross_valid and self.cv is not None and ((epoch + 1) % int(args.cross_valid_every) == 0 or last):
                # (one pass serves validation and evaluation -- unless the best state is to be evaluated: then `evaluate` below measures and
                # writes, and this pass does neither, instead of doing both twice)
                valid, lsd = self.validate(epoch, enhance=eval_now and self.valid_equals_test and not args.evaluate_on_best)
                evaluation_loss = valid['evaluation']
                rec.update({'valid_' + k + '_loss': v for k, v in valid.items()})
                best_loss = min(pull_metric(self.history, 'valid_evaluation_loss') + [evaluation_loss])
                if evaluation_loss == best_loss:
                    logger.info('New best valid loss %.4f', evaluation_loss)
                    self.best_states = {name: copy_state(m.state_dict()) for name, m in self.models.items()}
            if evaluation_loss is not None:
                rec['evaluation_loss'] = evaluation_loss
            if best_loss is not None:
                rec['best_loss'] = best_loss
            if eval_now:
                if lsd is None:
                    lsd = self.evaluate(epoch)
                rec.update({'lsd': lsd, 'visqol': 0})
            self.history.append(rec)
            if distrib.rank == 0:
                print(json.dumps(rec), flush=True)
                with open(str(args.history_file), 'w') as f:
                    json.dump(self.history, f, indent=2)
                if args.checkpoint:
                    data.serialize(self.models, self.optimizers, self.history, self.best_states, args)
        return self.history
