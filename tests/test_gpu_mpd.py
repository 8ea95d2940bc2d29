"""HiFi-GAN multi-period critic `mpd` on the MI355X: the reference's forward, losses and gradients at the width the reference builds
(hidden 32), the full-width gradients against torch.autograd on the module's own convolutions, and the training step with
[msd_melgan, mpd]."""
import math

import pytest
import torch

import mpd_cases as mc
from conftest import seeded


@pytest.mark.gpu
@pytest.mark.parametrize('L', [4001, 8192])
def test_mpd_forward_losses_and_gradients_on_the_mi355x(L):
    mc.check_io(mc.case_io('cuda', 32, L), map_bar=1.5e-3)


@pytest.mark.gpu
def test_mpd_gradients_per_period_at_full_width_on_the_mi355x():
    """hidden 32 on 2 x 44 100 samples (long rows, reflect padding at p = 11) against torch.autograd through the module's own weight-normed
    nn.Conv2d on IDENTICAL inputs (fp32), per period: every parameter gradient of the critic loss within 2e-2 rel-L2 (conv 0's weight
    direction 5e-2: the fp16 input and activation storage, mpd_cases.check_io), and no period more than 4x the median period's error"""
    d = mc.seeded_mpd(32).cuda()
    fake = (0.3 * seeded((2, 1, 44100), 11)).half().float().cuda()
    real = (0.3 * seeded((2, 1, 44100), 12)).half().float().cuda()
    ref = mc.torch_period_gradients(d, fake, real)
    d.zero_grad()
    d.discriminator_loss(fake, real).backward()
    got = dict(d.named_parameters())
    errs = {}
    for k, want in ref.items():
        g = got[k].grad
        errs[k] = float((g.double() - want.double()).norm() / want.double().norm().clamp_min(1e-30))
    bad = {k: v for k, v in errs.items() if not v < (5e-2 if '.convs.0.weight_' in k else 2e-2)}
    assert not bad, bad
    per = {}
    for k, v in errs.items():
        if '.convs.0.' not in k:
            per.setdefault(k.split('.')[1], []).append(v)
    worst = {p: max(v) for p, v in per.items()}
    med = sorted(worst.values())[len(worst) // 2]
    assert max(worst.values()) <= 4 * max(med, 1e-4), worst


def _gan_args():
    from aero_amd.config import _wrap
    gen = dict(channels=16, nfft=512, hop_length=256, lr_sr=4000, hr_sr=16000)
    return _wrap(dict(optim='adam', lr=3e-4, beta2=0.999, losses=['stft'], stft_sc_factor=0.5, stft_mag_factor=0.5,
                      experiment=dict(model='aero', aero=gen, adversarial=True, features_loss_lambda=100, only_features_loss=False,
                                      only_adversarial_loss=False, discriminator_models=['msd_melgan', 'mpd'], mpd=dict(hidden=8),
                                      melgan_discriminator=dict(n_layers=4, num_D=3, downsampling_factor=4, ndf=16))))


@pytest.mark.gpu
def test_adversarial_training_with_mpd_is_finite_and_reproducible():
    """TrainStep with [msd_melgan, mpd] (solver.py:457-463,580-611): every loss of the reference's keys is finite, the critic step moves
    both critics, and two runs from one seed give bit-identical generator and critic parameters after four steps"""
    from aero_amd import trainer
    args = _gan_args()

    def run():
        torch.manual_seed(77)
        models = {k: m.cuda().train() for k, m in trainer.build_models(args).items()}
        opts = trainer.build_optimizers(models, args)
        step = trainer.TrainStep(models, opts, args)
        d0 = opts['disc_optimizer'].flat_p.clone()
        for i in range(4):
            lr = seeded((2, 1, 8000), 300 + i).cuda()
            hr = (0.1 * seeded((2, 1, 32000), 400 + i)).cuda()
            rec = step(lr, hr)
        torch.cuda.synchronize()
        n_mel = sum(p.numel() for p in models['msd_melgan'].parameters())
        return ({k: float(v) for k, v in rec.items()}, opts['optimizer'].flat_p.clone(), opts['disc_optimizer'].flat_p.clone(), d0,
                models['mpd'], n_mel)

    r1, g1, d1, d0, mpd, n_mel = run()
    for k in ('generator_stft', 'generator_adversarial_melgan', 'generator_features_melgan', 'generator_adversarial_mpd',
              'generator_features_mpd', 'discriminator_msd_melgan', 'discriminator_mpd'):
        assert k in r1 and math.isfinite(r1[k]), (k, r1)
    # both critics took their step (the chained parameters: msd_melgan's first, then mpd's)
    assert not torch.equal(d1[:n_mel], d0[:n_mel]) and not torch.equal(d1[n_mel:], d0[n_mel:])
    r2, g2, d2, _, _, _ = run()
    assert r1 == r2, (r1, r2)
    assert torch.equal(g1, g2), float((g1 - g2).abs().max())
    assert torch.equal(d1, d2), float((d1 - d2).abs().max())


@pytest.mark.gpu
def test_adversarial_training_with_mpd_tracks_the_reference_trajectory():
    """the reference's own step with discriminator_models [msd_melgan, mpd] (tools/make_golden_train_mpd.py ->
    tests/golden/train_mpd_trajectory.npz: its generator, both critics, its losses, two torch.optim.Adam, 12 steps on one batch, fp32 CPU)
    against aero_amd.trainer.TrainStep term by term: step 0 within 1e-4; over 12 steps the STFT, both feature-matching, both critic terms and
    adversarial_mpd within 1e-2; adversarial_melgan within 1.5e-2 over 4 steps and 8e-2 over 12 (the conditioning reason documented at
    tests/test_gpu_train.py::test_adversarial_training_tracks_the_reference_trajectory)"""
    import json
    import numpy as np
    from aero_amd import trainer
    from aero_amd.config import _wrap
    from conftest import GOLDEN
    z = np.load(f'{GOLDEN}/train_mpd_trajectory.npz')
    cfgt = json.loads(str(z['cfg']))
    gold = torch.from_numpy(z['loss'])
    args = _wrap(dict(optim='adam', lr=cfgt['lr'], beta2=cfgt['betas'][1], losses=['stft'], stft_sc_factor=0.5, stft_mag_factor=0.5,
                      experiment=dict(model='aero', aero=cfgt['gen_cfg'], adversarial=True, features_loss_lambda=cfgt['features_loss_lambda'],
                                      only_features_loss=False, only_adversarial_loss=False, discriminator_models=cfgt['discriminator_models'],
                                      melgan_discriminator=cfgt['disc_cfg'], mpd=cfgt['mpd_cfg'])))
    torch.manual_seed(cfgt['seed'])
    models = {k: m.cuda().train() for k, m in trainer.build_models(args).items()}
    opts = trainer.build_optimizers(models, args)
    step = trainer.TrainStep(models, opts, args)
    x = seeded((2, 1, cfgt['L']), cfgt['x_seed']).cuda()
    hr = (cfgt['hr_scale'] * seeded((2, 1, 4 * cfgt['L']), cfgt['hr_seed'])).cuda()
    keys = ['generator_stft', 'generator_adversarial_melgan', 'generator_features_melgan', 'generator_adversarial_mpd',
            'generator_features_mpd', 'discriminator_msd_melgan', 'discriminator_mpd']
    got = []
    for _ in range(cfgt['steps']):
        rec = step(x, hr)
        got.append([float(rec[k]) for k in keys])
    got = torch.tensor(got, dtype=torch.float64)
    rel = (got - gold).abs() / gold.abs()
    print('mpd trajectory: worst relative deviation per term %s' % dict(zip(cfgt['columns'], [f'{float(v):.2e}' for v in rel.max(0).values])))
    assert float(rel[0].max()) < 1e-4, rel[0].tolist()
    for c in (0, 2, 3, 4, 5, 6):
        assert float(rel[:, c].max()) < 1e-2, (cfgt['columns'][c], rel[:, c].tolist())
    assert float(rel[:4, 1].max()) < 1.5e-2 and float(rel[:, 1].max()) < 8e-2, rel[:, 1].tolist()


@pytest.mark.gpu
def test_train_entry_point_with_mpd_on_the_mi355x():
    """`python train.py experiment=aero_11-44_512_256 'experiment.discriminator_models=[msd_melgan,mpd]' steps=2` (config 5, the mpd at the
    constructor's defaults: the experiment file has no `mpd` block) prints finite losses, the mpd terms among them"""
    import json
    import os
    import subprocess
    import sys
    from conftest import ROOT
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'train.py'), 'experiment=aero_11-44_512_256',
                          'experiment.discriminator_models=[msd_melgan,mpd]', 'steps=2'], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    recs = [json.loads(line) for line in out.stdout.splitlines() if line.startswith('{"step"')]
    assert len(recs) == 2, out.stdout[-2000:]
    for r in recs:
        for k in ('generator_adversarial_mpd', 'generator_features_mpd', 'discriminator_mpd', 'discriminator_msd_melgan', 'generator_stft'):
            assert k in r and math.isfinite(r[k]), (k, r)
    print('train.py with [msd_melgan, mpd]:', [r['ms'] for r in recs], 'ms per step')
