"""BASELINE config 5 on one GPU: aero_11-44_512_256 (11.025 -> 44.1 kHz, n_fft 512, hop 256), 10-s segments, train mode:
forward -> multi-resolution STFT loss -> backward -> FlatAdam.step.  usage: config5.py [B] [steps] [--gan] [--mpd]
(--gan: + the msd_melgan critic; --mpd: + msd_melgan AND the multi-period critic mpd at the reference's width, both in one critic Adam as
train.py:91-96 chains them; every step prints its whole time, `step ms`)"""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from aero_amd import Aero, losses  # noqa: E402
from aero_amd.config import load_config  # noqa: E402
from aero_amd.optim import FlatAdam  # noqa: E402


def main():
    gan = '--gan' in sys.argv                                   # + the msd_melgan critic: adversarial / feature losses and the critic's own step
    use_mpd = '--mpd' in sys.argv                               # + the multi-period critic (solver.py:457-463,580-600)
    gan = gan or use_mpd
    sys.argv = [a for a in sys.argv if not a.startswith('--')]
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 2
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    args = load_config(os.path.join(ROOT, 'conf'), ['experiment=aero_11-44_512_256'])
    torch.manual_seed(2036)
    model = Aero(**dict(args.experiment.aero)).cuda().train()
    opt = FlatAdam(model.parameters(), lr=3e-4, betas=(0.9, 0.999), model=model)
    crit = losses.MultiResolutionSTFTLoss(factor_sc=0.5, factor_mag=0.5)                  # main_config.yaml:64-65
    disc = opt_d = None
    if gan:
        from aero_amd.discriminators import Discriminator
        disc = Discriminator(num_D=3, ndf=16, n_layers=4, downsampling_factor=4).cuda()
        mpd = None
        if use_mpd:
            from aero_amd.mpd import MultiPeriodDiscriminator
            mpd = MultiPeriodDiscriminator().cuda()
            opt_d = FlatAdam(list(disc.parameters()) + list(mpd.parameters()), lr=3e-4, betas=(0.9, 0.999), model=[disc, mpd])
        else:
            opt_d = FlatAdam(disc.parameters(), lr=3e-4, betas=(0.9, 0.999), model=disc)
    g = torch.Generator().manual_seed(0)
    lr = torch.randn(B, 1, 110250, generator=g).cuda()
    hr = (0.1 * torch.randn(B, 1, 441000, generator=g)).cuda()
    for s in range(steps):
        torch.cuda.synchronize()
        t0 = time.time()
        y = model(lr)
        torch.cuda.synchronize()
        t1 = time.time()
        sc, mg = crit(y.squeeze(1), hr.squeeze(1))
        loss = sc + mg
        extra = ''
        if gan:
            adv, feat = disc.generator_losses(y, hr, n_layers=4, features_loss_lambda=100.0)      # solver.py:498-520
            loss = loss + adv + feat
            extra = f' adv {float(adv.detach()):.4f} feat {float(feat.detach()):.4f}'
            if use_mpd:
                adv_p, feat_p = mpd.generator_losses(y, hr, features_loss_lambda=100.0)               # solver.py:587-600
                loss = loss + adv_p + feat_p
                extra += f' adv_mpd {float(adv_p.detach()):.4f} feat_mpd {float(feat_p.detach()):.4f}'
        opt.zero_grad()
        loss.backward()
        torch.cuda.synchronize()
        t2 = time.time()
        opt.step()
        torch.cuda.synchronize()
        t3 = time.time()
        td = 0.0
        if gan:                                                  # solver.py:607-611: the critic's own step on the detached prediction
            d_loss = disc.discriminator_loss(y.detach(), hr)
            if use_mpd:
                d_loss = d_loss + mpd.discriminator_loss(y.detach(), hr)
            opt_d.zero_grad()
            d_loss.backward()
            opt_d.step()
            torch.cuda.synchronize()
            td = time.time() - t3
            extra += f' d_loss {float(d_loss.detach()):.4f}  critic step {1e3 * td:.1f} ms'
        gn = float(opt.flat_g.norm())
        print(f'step {s}: step ms {1e3 * (time.time() - t0):.2f}  loss {float(loss.detach()):.5f} (sc {float(sc.detach()):.5f} mag {float(mg.detach()):.5f}{extra})  |grad| {gn:.4e}  forward {1e3 * (t1 - t0):.1f} ms  '
              f'loss+backward {1e3 * (t2 - t1):.1f} ms  adam {1e3 * (t3 - t2):.2f} ms  y {tuple(y.shape)}  mem {torch.cuda.max_memory_allocated() / 2**30:.2f} GiB')
        assert torch.isfinite(loss) and gn == gn and gn > 0


if __name__ == '__main__':
    main()
