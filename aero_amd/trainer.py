"""One training step of BASELINE config 5 as the reference's entry point runs it (`train.py ddp=true`):

    build_models      <- src/models/modelFactory.py:6-29   generator + the critics (`msd_melgan`, `mpd`) of the experiment file
    build_optimizers  <- train.py:83-96                    Adam(generator), Adam(chained critics), lr / betas from the config
    TrainStep         <- src/solver.py:51 (every model through distrib.wrap), :296-320 (forward, losses, optimise),
                         :428-470 (which losses), :475-520 (MelGAN hinge / feature matching), :602-611 (the two optimiser steps)

    data_source       <- train.py:54-57                    LrHrSet of `dset.train`, device-resident (aero_amd/data.py) or read by the host

The Solver around it -- epochs, validation, best states, evaluation, history, checkpoint and resume -- is aero_amd/solver.py.  This module
is the part that touches the device.  Everything runs on the HIP kernels: the generator through `AeroFunction`, the criterion through
`losses.MultiResolutionSTFTLoss`, the critic through `Discriminator.generator_losses / discriminator_loss`, both optimisers as
`FlatAdam`.  With world_size > 1 the gradients of BOTH models are averaged over the ranks inside their backward passes.
"""
import torch

from . import distrib, losses
from .optim import FlatAdam


def build_models(args):
    """modelFactory.py:6-29 for what the experiment files use: `model: aero` or `model: seanet` (the time-domain baseline, kwargs from
    `experiment.seanet`; inference only, aero_amd/seanet.py) and, with `adversarial: true`, the critics of
    `discriminator_models`: the MelGAN multi-scale critic `msd_melgan` and the HiFi-GAN multi-period critic `mpd`, constructed in
    modelFactory.py's fixed order (msd_melgan, then mpd) whatever the list order, so a seed draws the reference's initial weights.
    `mpd` takes its kwargs from `experiment.mpd`; without that block the constructor's defaults are used (the reference would fail on the
    missing key).  The critics `msd_hifi` / `hifi` stay NotImplementedError: the reference cannot run them either."""
    exp = args.experiment
    if exp.model == 'aero':
        from .modules import Aero
        models = {'generator': Aero(**dict(exp.aero))}
    elif exp.model == 'seanet':
        from .seanet import Seanet
        models = {'generator': Seanet(**dict(exp.seanet))}
    else:
        raise NotImplementedError(f"model '{exp.model}': the generators implemented on MI355X are aero and seanet")
    if exp.get('adversarial'):
        names = list(exp.discriminator_models)
        for name in names:
            if name in ('msd_hifi', 'hifi'):
                raise NotImplementedError(
                    f"critic '{name}': not built -- the reference cannot run it (modelFactory.py:18-27 registers the module as 'msd' while "
                    f"solver.py:525,558 / train.py:92-94 look up 'msd_hifi', and 'hifi' needs a melspec_transform only created under an "
                    f"experiment key no config sets, solver.py:89-94)")
            if name not in ('msd_melgan', 'mpd'):
                raise NotImplementedError(f"critic '{name}': only msd_melgan and mpd are implemented")
        if 'msd_melgan' in names:
            from .discriminators import Discriminator
            models['msd_melgan'] = Discriminator(**dict(exp.melgan_discriminator))
        if 'mpd' in names:
            from .mpd import MultiPeriodDiscriminator
            models['mpd'] = MultiPeriodDiscriminator(**dict(exp.get('mpd') or {}))
    return models


def build_optimizers(models, args, lib=None):
    """train.py:83-96: Adam(lr, betas=(0.9, beta2)) for the generator and one Adam over the critics' parameters chained in
    `discriminator_models` order."""
    if args.optim != 'adam':
        raise ValueError('Invalid optimizer %s' % args.optim)
    gen = models['generator']
    opts = {'optimizer': FlatAdam(gen.parameters(), lr=args.lr, betas=(0.9, args.beta2), lib=lib, model=gen)}
    order = [n for n in args.experiment.get('discriminator_models', []) if n in models] if args.experiment.get('adversarial') else []
    order += [k for k in models if k != 'generator' and k not in order]
    critics = [models[k] for k in order]
    if critics:
        params = [p for m in critics for p in m.parameters()]
        opts['disc_optimizer'] = FlatAdam(params, lr=args.lr, betas=(0.9, args.beta2), lib=lib,
                                          model=critics[0] if len(critics) == 1 else critics)
    return opts


class TrainStep:
    def __init__(self, models, optimizers, args):
        self.args = args
        exp = args.experiment
        self.adversarial = bool(exp.get('adversarial'))
        self.models = models
        self.dmodels = {k: distrib.wrap(m) for k, m in models.items()}            # solver.py:51
        self.dmodel = self.dmodels['generator']
        self.optimizer = optimizers['optimizer']
        self.disc_optimizer = optimizers.get('disc_optimizer')
        if self.adversarial and self.disc_optimizer is None:
            raise ValueError('adversarial experiment without a disc_optimizer')
        self.mrstft = None
        if 'stft' in args.losses:
            self.mrstft = losses.MultiResolutionSTFTLoss(factor_sc=args.stft_sc_factor, factor_mag=args.stft_mag_factor)

    def losses_of(self, pr, hr):
        """solver.py:428-470 -> {'generator': {...}, 'discriminator': {...}}"""
        import torch.nn.functional as F
        out = {'generator': {}, 'discriminator': {}}
        if 'l1' in self.args.losses:
            out['generator']['l1'] = F.l1_loss(pr, hr)
        if 'l2' in self.args.losses:
            out['generator']['l2'] = F.mse_loss(pr, hr)
        if self.mrstft is not None:
            sc, mag = self.mrstft(pr.squeeze(1), hr.squeeze(1))
            out['generator']['stft'] = sc + mag
        exp = self.args.experiment
        # (this order fixes the order in which the generator's terms are summed, and with it the fp32 total)
        for name, tag in (('msd_melgan', 'melgan'), ('mpd', 'mpd')):
            if not self.adversarial or name not in self.dmodels:
                continue
            critic, kw = self.dmodels[name], {}
            if name == 'msd_melgan':
                md = exp.melgan_discriminator
                if md.num_D != critic.num_D:
                    raise ValueError('melgan_discriminator.num_D does not match the critic')
                kw['n_layers'] = md.n_layers
            adv, feat = critic.generator_losses(pr, hr, features_loss_lambda=exp.features_loss_lambda, **kw)   # solver.py:498-520,587-600
            if not exp.get('only_features_loss'):
                out['generator']['adversarial_' + tag] = adv
            if not exp.get('only_adversarial_loss'):
                out['generator']['features_' + tag] = feat
            # D(fake.detach()), D(real) on the weights the generator's losses just used (solver.py:478-480): the critic keeps that
            # record, so this costs no second forward (a caller that takes no critic step, as validation does, drops it: drop_record)
            out['discriminator'][name] = critic.discriminator_loss(pr.detach(), hr)
        return out

    def __call__(self, lr, hr):
        """one batch in training mode; returns {'generator_<name>': value, 'discriminator_<name>': value, 'total': value} (device scalars)"""
        pr = self.dmodel(lr)
        ls = self.losses_of(pr, hr)
        total = sum(ls['generator'].values())
        self.optimizer.zero_grad()                                                # solver.py:602-605
        total.backward()
        self.optimizer.step()
        if self.adversarial:                                                      # solver.py:607-611
            d_total = sum(ls['discriminator'].values())
            self.disc_optimizer.zero_grad()
            d_total.backward()
            self.disc_optimizer.step()
        rec = {'total': total.detach()}
        rec.update({'generator_' + k: v.detach() for k, v in ls['generator'].items()})
        rec.update({'discriminator_' + k: v.detach() for k, v in ls['discriminator'].items()})
        return rec


def synthetic_batch(args, batch, device, seed=0):
    """white-noise (lr, hr) pair of the experiment's geometry: `segment` seconds at lr_sr / hr_sr (BASELINE.json: synthetic data; the
    reference's LrHrSet file reader is host code outside the path)"""
    exp = args.experiment
    g = torch.Generator().manual_seed(seed)
    n_lr, n_hr = int(exp.segment * exp.lr_sr), int(exp.segment * exp.hr_sr)
    lr = torch.randn(batch, 1, n_lr, generator=g)
    hr = 0.1 * torch.randn(batch, 1, n_hr, generator=g)
    return lr.to(device), hr.to(device)


class DataSource:
    """The training set of one rank: `batches(epoch, per_rank)` are the index lists of the epoch in `data.EpochSampler` order (the
    last may be short), `load(batches)` yields their (lr, hr) on the device -- cut out of the device-resident store (`kind` "device"),
    or read by the host `LrHrSet` in DataLoader workers ("host").  Both give the same tensors for the same indices."""

    def __init__(self, dataset, store, device, seed, num_workers=0):
        self.dataset, self.store, self.device, self.seed, self.num_workers = dataset, store, device, seed, num_workers
        self.kind = 'host' if store is None else 'device'

    def batches(self, epoch, per_rank):
        from .data import EpochSampler
        idx = EpochSampler(len(self.dataset), distrib.world_size, distrib.rank, shuffle=True, seed=self.seed, epoch=epoch).indices()
        return [idx[i:i + per_rank] for i in range(0, len(idx), per_rank)]

    def load(self, batches):
        if self.store is not None:
            for b in batches:
                yield self.store.batch(b)
            return
        from torch.utils.data import DataLoader
        # (not distrib.loader: its sampler would draw an order of its own; the order here is the one `batches` fixed)
        for lr, hr in DataLoader(self.dataset, batch_sampler=batches, num_workers=self.num_workers):
            yield lr.to(self.device), hr.to(self.device)


def data_source(args, device, lib=None):
    """train.py:54-57: the training set of `dset.train` if its lr.json / hr.json exist (and `+synthetic=true` is not given), else None.
    `+data_on_device=false`, or a set whose decoded samples exceed `+data_max_bytes` (default data.DEFAULT_MAX_BYTES), is read by the host.
    lib: tests' explicitly loaded library for the store."""
    import os

    from . import data
    train = (args.get('dset') or {}).get('train')
    if args.get('synthetic') or not train:
        return None
    if not (os.path.exists(os.path.join(str(train), 'lr.json')) and os.path.exists(os.path.join(str(train), 'hr.json'))):
        return None
    exp = args.experiment
    dataset = data.LrHrSet(train, exp.lr_sr, exp.hr_sr, exp.stride, exp.segment, upsample=exp.upsample)
    store = None
    if args.get('data_on_device', True):
        store = data.DeviceLrHrStore(dataset, device, int(args.get('data_max_bytes', data.DEFAULT_MAX_BYTES)), lib=lib)
    return DataSource(dataset, store, device, int(args.seed), int(args.get('num_workers', 0)))
