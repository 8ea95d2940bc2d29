"""Shared by tests/test_solver.py (CPU, emulator library), tests/test_gpu_solver.py (MI355X, train.py as a child process) and
tests/test_distrib_gloo_solver.py: the wav sets, the command line, an in-process run of what train.py does for real data, and the
comparisons of two checkpoints.

Shapes.  The narrowest generator the training engine accepts (channels=16 of aero_4-16_512_64, see tests/test_gpu_data.py); training on
three PCM16 clips cut into 1-second items (one shorter than a second, so it is padded; three items at batch 2 make a full and a short
batch); validation and test on whole files of 4100, 8001 and 9000 low-rate samples: no multiple of the hop (16 at 4 kHz), all different,
so every file is a B = 1 forward of another odd length whose output is longer than the target and is cut by match_signal.  That is
the geometry on the MI355X (`GPU`).  The emulator executes one training step of it in about two minutes, so the CPU tests keep the
experiment file, the 16 channels and the 1-second items and scale the clock: 300 -> 1200 Hz with nfft 128 / hop 32 (`EMU`; a second
is 300 low-rate samples, the hop 8), whole files of 261, 275 and 290 samples -- again no multiple of the hop and all different, and
their 1044 to 1160 high-rate samples are just above the 1024 the reflect padding of the losses' largest STFT (2048) needs."""
import contextlib
import json
import os

import torch

import data_cases as DC
from conftest import ROOT


class Geometry:
    def __init__(self, lr_sr, hr_sr, train_lr, valid_lr, extra):
        self.lr_sr, self.hr_sr, self.train_lr, self.valid_lr, self.extra = lr_sr, hr_sr, train_lr, valid_lr, extra


GPU = Geometry(4000, 16000, (4000, 3000, 4000), (4100, 8001, 9000), [])
EMU = Geometry(300, 1200, (300, 225, 300), (261, 275, 290),
               ['experiment.lr_sr=300', 'experiment.hr_sr=1200', 'experiment.nfft=128', 'experiment.hop_length=32'])
BASE = ['experiment=aero_4-16_512_64', 'experiment.aero.channels=16', 'experiment.segment=1', 'experiment.stride=1',
        'experiment.batch_size=2', 'num_workers=0']
NO_CRITIC = ['experiment.adversarial=false']
# The msd_melgan critic.  On the device: exactly as the experiment file has it (ndf 16, three scales, four layers), the one geometry
# whose weight and bias gradients are all added in a fixed order (aero_gconv4 and the edge layers' ordered slabs need Cin = 4 x groups,
# stride 4, a first layer of 16 and a last layer of a multiple of 512 channels); any other critic has layers on the generic
# aero_gconv1d_bwd path, which adds them with float atomics, so its last bits change from run to run and a bit-equality between two
# runs would measure nothing.  On the emulator that critic costs seventy seconds a step, so the CPU tests take one scale and two layers
# of the same width (a second a step) and run the critic's launches through `OrderedLib`: the emulator then executes a launch's blocks
# one after the other, and the atomics add in block order -- the same order every time.
CRITIC = ['experiment.adversarial=true', 'experiment.discriminator_models=[msd_melgan]']
CRITIC_EMU = CRITIC + ['experiment.melgan_discriminator={n_layers: 2, num_D: 1, downsampling_factor: 4, ndf: 16}']


class OrderedLib:
    """the emulator library with every launch on ONE worker thread (AERO_EMU_THREADS is read per launch)"""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def call(self, *args):
        old = os.environ.get('AERO_EMU_THREADS')
        os.environ['AERO_EMU_THREADS'] = '1'
        try:
            return self._lib.call(*args)
        finally:
            if old is None:
                del os.environ['AERO_EMU_THREADS']
            else:
                os.environ['AERO_EMU_THREADS'] = old


def write_set(d, lr_lengths, seed, geo=GPU):
    """PCM16 noise clips at the geometry's rates under d/lr and d/hr with their lr.json / hr.json"""
    up = geo.hr_sr // geo.lr_sr
    os.makedirs(os.path.join(d, 'lr'))
    os.makedirs(os.path.join(d, 'hr'))
    lr, hr = [], []
    for k, n in enumerate(lr_lengths):
        lp, hp = os.path.join(d, 'lr', f'clip{k}.wav'), os.path.join(d, 'hr', f'clip{k}.wav')
        DC.write_wav(lp, DC.noise_i16(n, seed + k) // 8, geo.lr_sr, False)
        DC.write_wav(hp, DC.noise_i16(up * n, seed + 50 + k) // 8, geo.hr_sr, False)
        lr.append([lp, n])
        hr.append([hp, up * n])
    json.dump(lr, open(os.path.join(d, 'lr.json'), 'w'))
    json.dump(hr, open(os.path.join(d, 'hr.json'), 'w'))
    return d


def write_sets(tmp, geo=GPU):
    """-> (train, valid, test) directories"""
    return (write_set(os.path.join(str(tmp), 'tr'), geo.train_lr, 300, geo), write_set(os.path.join(str(tmp), 'cv'), geo.valid_lr, 400, geo),
            write_set(os.path.join(str(tmp), 'tt'), geo.valid_lr[::-1], 500, geo))


def load_args(overrides):
    from aero_amd.config import load_config
    return load_config(os.path.join(ROOT, 'conf'), list(overrides))


@contextlib.contextmanager
def in_dir(d):
    os.makedirs(d, exist_ok=True)
    old = os.getcwd()
    os.chdir(d)
    try:
        yield
    finally:
        os.chdir(old)


def build(args, lib, device='cpu'):
    """what train.py's run() builds before the epochs, on the emulator library -> (models, optimizers, step, source)"""
    from aero_amd import distrib, losses, trainer
    from aero_amd.engine import HipEngine
    dev = torch.device(device)
    torch.manual_seed(args.seed)
    models = trainer.build_models(args)
    for name, m in models.items():
        m.to(dev).train()
        if lib is None:                                          # the MI355X: the product's own library
            continue
        if name == 'generator':
            object.__setattr__(m, '_engine', HipEngine(m, lib=lib))
        else:
            m.use_library(OrderedLib(lib))
    if lib is not None:
        losses.use_library(lib)
    optimizers = trainer.build_optimizers(models, args, lib=lib)
    step = trainer.TrainStep(models, optimizers, args)
    source = trainer.data_source(args, dev, lib=lib)
    assert source is not None
    return models, optimizers, step, source, args.experiment.batch_size // distrib.world_size


def make_solver(cwd, overrides, lib, load=True, device='cpu'):
    """a Solver as train.py makes it, for the working directory the caller is in (`in_dir`); lib=None on the MI355X"""
    from aero_amd.solver import Solver
    args = load_args(list(overrides) + [f'device={device}'])
    models, optimizers, step, source, per_rank = build(args, lib, device)
    s = Solver(args, models, optimizers, step, source, device, per_rank, lib=lib)
    if load:
        s.load()
    return s


def run_cpu(cwd, overrides, lib):
    """train.py's real-data mode in this process, in directory `cwd`, on the emulator -> the Solver after training"""
    from aero_amd import losses
    with in_dir(cwd):
        try:
            s = make_solver(cwd, overrides, lib)
            s.train()
        finally:
            losses.use_library(None)
    return s


LOSS_KEYS = ('total', 'generator_', 'discriminator_', 'valid_', 'evaluation_loss', 'best_loss', 'lsd')


def losses_of_history(history):
    return [{k: v for k, v in h.items() if k.startswith(LOSS_KEYS)} for h in history]


def assert_same_state(a, b):
    """two checkpoint packages (or the live counterparts in the same layout): torch.equal on every model tensor, every Adam moment, and
    the step counts"""
    assert set(a['models']) == set(b['models'])
    n = 0
    for name in a['models']:
        sa, sb = a['models'][name]['state'], b['models'][name]['state']
        assert list(sa) == list(sb)
        for k in sa:
            assert torch.equal(sa[k].cpu(), sb[k].cpu()), (name, k)
            n += 1
    assert set(a['optimizers']) == set(b['optimizers'])
    for name in a['optimizers']:
        oa, ob = a['optimizers'][name]['state'], b['optimizers'][name]['state']
        assert list(oa) == list(ob) and len(oa) > 0
        for i in oa:
            assert float(oa[i]['step']) == float(ob[i]['step']), (name, i)
            assert torch.equal(oa[i]['exp_avg'].cpu(), ob[i]['exp_avg'].cpu()), (name, i, 'exp_avg')
            assert torch.equal(oa[i]['exp_avg_sq'].cpu(), ob[i]['exp_avg_sq'].cpu()), (name, i, 'exp_avg_sq')
            n += 2
    return n


def package_of(solver):
    """the live state of a Solver in the checkpoint's layout"""
    return {'models': {n: {'state': {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}} for n, m in solver.models.items()},
            'optimizers': {n: o.state_dict() for n, o in solver.optimizers.items()}}


def direct_validation(step, gen, eset, indices):
    """the definition: per file, the terms of losses_of on match_signal(gen.eval()(lr), len(hr)) -> [(stem, {term: device scalar})]"""
    from aero_amd.enhance import match_signal
    was = gen.training
    gen.eval()
    out = []
    try:
        with torch.no_grad():
            for i in indices:
                lr, hr = eset.item(i)
                pr = match_signal(gen(lr), hr.shape[-1])
                ls = step.losses_of(pr, hr)
                vals = {'total': sum(ls['generator'].values())}
                vals.update({'generator_' + k: v for k, v in ls['generator'].items()})
                vals.update({'discriminator_' + k: v for k, v in ls['discriminator'].items()})
                out.append((eset.stem(i), {k: v.detach().float() for k, v in vals.items()}))
    finally:
        gen.train(was)
        for m in step.models.values():
            if hasattr(m, 'drop_record'):
                m.drop_record()
    return out


def mean_of(per_file):
    """the mean a pass records: the per-file fp32 vectors added in file order on the device, read once, divided by the file count"""
    keys = list(per_file[0][1])
    mat = torch.stack([torch.stack([v[k] for k in keys]) for _, v in per_file])
    return {k: s / len(per_file) for k, s in zip(keys, mat.sum(0).tolist())}
