"""Golden LOSS TRAJECTORY of the reference's adversarial training step with BOTH critics, `discriminator_models: [msd_melgan, mpd]`: the
small generator of oracle/make_golden_train_gan.py, the reference's MelGAN critic and its MultiPeriodDiscriminator (hidden 8), its
MultiResolutionSTFTLoss, and two torch.optim.Adam -- the critic one over the chained critics' parameters, msd_melgan first, as
train.py:91-96 builds it.  Per step, solver.py:428-470 and :475-520 / :580-600: generator forward, STFT loss, each critic on
pr.detach() / hr for its own loss and on pr / hr for the generator's adversarial and feature losses, then the generator step and the
critic step (solver.py:602-611).  12 steps on ONE fixed batch, fp32 on the CPU.  tests/test_gpu_mpd.py holds aero_amd.trainer.TrainStep
to it.  Runs only in the build container (imports the reference checkout, argv[1], default /root/reference):

    python -B tools/make_golden_train_mpd.py

Writes tests/golden/train_mpd_trajectory.npz (12 x 7 loss values and the configuration as JSON): no weights, nothing of the reference."""
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

sys.dont_write_bytecode = True
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden')
GEN_CFG = dict(channels=16, nfft=512, hop_length=256, lr_sr=4000, hr_sr=16000)
DISC_CFG = dict(num_D=3, ndf=16, n_layers=4, downsampling_factor=4)
MPD_CFG = dict(hidden=8)
STEPS, LR, LAMBDA, SEED, L = 12, 3e-4, 100.0, 77, 8000
COLUMNS = ['stft', 'adversarial_melgan', 'features_melgan', 'adversarial_mpd', 'features_mpd', 'discriminator_msd_melgan',
           'discriminator_mpd']


def seeded(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def main():
    sys.path.insert(0, sys.argv[1] if len(sys.argv) > 1 else '/root/reference')
    torch.set_num_threads(8)
    sys.modules.setdefault('cv2', types.ModuleType('cv2'))          # (src.utils imports cv2, absent here and unused by the critics)
    from src.models.aero import Aero
    from src.models.discriminators import Discriminator, MultiPeriodDiscriminator, discriminator_loss, feature_loss, generator_loss
    import src.models.stft_loss as ref_loss
    real_stft = torch.stft

    def stft_compat(x, n_fft, hop_length=None, win_length=None, window=None, **kw):       # stft_loss.py:22 predates return_complex
        return torch.view_as_real(real_stft(x, n_fft, hop_length, win_length, window, return_complex=True, **kw))
    torch.manual_seed(SEED)                                        # modelFactory.py's order: generator, msd_melgan, mpd
    gen = Aero(**GEN_CFG).train()
    mel = Discriminator(**DISC_CFG).train()
    mpd = MultiPeriodDiscriminator(**MPD_CFG).train()
    x, hr = seeded((2, 1, L), 300), 0.1 * seeded((2, 1, 4 * L), 400)
    crit = ref_loss.MultiResolutionSTFTLoss(factor_sc=0.5, factor_mag=0.5)
    opt = torch.optim.Adam(gen.parameters(), lr=LR, betas=(0.9, 0.999))
    opt_d = torch.optim.Adam(list(mel.parameters()) + list(mpd.parameters()), lr=LR, betas=(0.9, 0.999))
    w_feat = (4.0 / (DISC_CFG['n_layers'] + 1)) * (1.0 / DISC_CFG['num_D'])
    traj = []
    for i in range(STEPS):
        pr = gen(x)
        torch.stft = stft_compat
        try:
            sc, mag = crit(pr.squeeze(1), hr.squeeze(1))
        finally:
            torch.stft = real_stft
        d_fake_det, d_real, d_fake = mel(pr.detach()), mel(hr), mel(pr)
        d_mel = sum(F.relu(1 + s[-1]).mean() for s in d_fake_det) + sum(F.relu(1 - s[-1]).mean() for s in d_real)
        feat_mel = LAMBDA * sum(w_feat * F.l1_loss(d_fake[a][j], d_real[a][j].detach()) for a in range(DISC_CFG['num_D'])
                                for j in range(len(d_fake[a]) - 1))
        adv_mel = sum(F.relu(1 - s[-1]).mean() for s in d_fake)
        y_d_rs, y_d_gs, _, _ = mpd(hr, pr.detach())                 # solver.py:580-600
        d_mpd = discriminator_loss(y_d_rs, y_d_gs)
        y_d_rs, y_d_gs, fmap_rs, fmap_gs = mpd(hr, pr)
        feat_mpd = LAMBDA * feature_loss(fmap_rs, fmap_gs)
        adv_mpd = generator_loss(y_d_gs)
        total = sc + mag + adv_mel + feat_mel + adv_mpd + feat_mpd
        opt.zero_grad()
        total.backward()
        opt.step()
        opt_d.zero_grad()
        (d_mel + d_mpd).backward()
        opt_d.step()
        traj.append([float(v.detach()) for v in (sc + mag, adv_mel, feat_mel, adv_mpd, feat_mpd, d_mel, d_mpd)])
        print(i, traj[-1], flush=True)
    cfg = dict(seed=SEED, gen_cfg=GEN_CFG, disc_cfg=DISC_CFG, mpd_cfg=MPD_CFG, x_seed=300, hr_seed=400, hr_scale=0.1, L=L, steps=STEPS,
               lr=LR, betas=[0.9, 0.999], features_loss_lambda=LAMBDA, discriminator_models=['msd_melgan', 'mpd'], columns=COLUMNS)
    np.savez_compressed(os.path.join(OUT, 'train_mpd_trajectory.npz'), loss=np.array(traj, dtype=np.float64), cfg=np.array(json.dumps(cfg)))


if __name__ == '__main__':
    main()
