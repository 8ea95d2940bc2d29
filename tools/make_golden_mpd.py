"""Golden fixtures of the HiFi-GAN multi-period critic `mpd` (reference src/models/discriminators.py:85-147, losses :210-243, solver.py:580-600)
for aero_amd/mpd.py.  Runs only in the build container (imports the reference checkout given as argv[1], default /root/reference):

    python -B tools/make_golden_mpd.py [REFERENCE_ROOT]

Writes tests/golden/mpd_meta.json (seeds, configuration, per-key (sum, |sum|) checksums of the seeded state dict at hidden 32 and 8) and
tests/golden/mpd_io.npz (for both widths and signal lengths 4001 / 8192: every feature map of D(fake) subsampled, the full logits, the three loss
values, the full gradient of adv + lambda * feat w.r.t. the fake waveform, and 64 fixed elements plus the norm of every parameter's
gradient of the critic loss).  Nothing of the reference is copied: the fixtures are seeds, checksums and recorded values."""
import json
import os
import sys
import types

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, '..', 'tests', 'golden')
SEED = {32: 81, 8: 82}
LENGTHS = (4001, 8192)
SIG_SEED = {4001: (91, 92), 8192: (93, 94)}
LAMBDA = 100.0


def seeded(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def sub(fm):
    """[B, C, H, p] -> channels and rows subsampled to about 4 x 16 (every period column kept)"""
    return fm[:, ::max(1, fm.shape[1] // 4), ::max(1, fm.shape[2] // 16), :]


def sample_idx(n):
    return np.unique(np.linspace(0, n - 1, 64).round().astype(np.int64))


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else '/root/reference'
    sys.path.insert(0, ref)
    torch.set_num_threads(8)
    sys.modules.setdefault('cv2', types.ModuleType('cv2'))          # (src.utils imports cv2, absent here and unused by the critic)
    from src.models.discriminators import MultiPeriodDiscriminator, discriminator_loss, feature_loss, generator_loss
    meta = {'seeds': {str(h): s for h, s in SEED.items()}, 'cfg': {'periods': [2, 3, 5, 7, 11]}, 'features_loss_lambda': LAMBDA,
            'lengths': list(LENGTHS), 'signal_seeds': {str(L): list(s) for L, s in SIG_SEED.items()}, 'signal_scale': 0.3, 'batch': 2,
            'checksums': {}, 'sample': 'numpy.unique(numpy.linspace(0, n - 1, 64).round())',
            'subsample': 'fm[:, ::max(1, C // 4), ::max(1, H // 16), :]'}
    io = {}
    for hidden, seed in SEED.items():
        torch.manual_seed(seed)
        mpd = MultiPeriodDiscriminator(hidden=hidden)
        meta['checksums'][str(hidden)] = {k: [float(v.double().sum()), float(v.double().abs().sum())] for k, v in mpd.state_dict().items()}
        for L in LENGTHS:
            pre = f'h{hidden}.L{L}.'
            fake = (0.3 * seeded((2, 1, L), SIG_SEED[L][0])).requires_grad_(True)
            real = 0.3 * seeded((2, 1, L), SIG_SEED[L][1])
            y_d_rs, y_d_gs, fmap_rs, fmap_gs = mpd(real, fake)
            adv = generator_loss(y_d_gs)
            feat = LAMBDA * feature_loss(fmap_rs, fmap_gs)
            dfake, = torch.autograd.grad(adv + feat, fake)
            for i in range(len(mpd.discriminators)):
                for j, (fr, fg) in enumerate(zip(fmap_rs[i], fmap_gs[i])):
                    io[pre + f'fake.{i}.{j}'] = sub(fg.detach()).numpy()
                io[pre + f'logits_fake.{i}'] = y_d_gs[i].detach().numpy()
                io[pre + f'logits_real.{i}'] = y_d_rs[i].detach().numpy()
            mpd.zero_grad()
            y_d_rs, y_d_gs, _, _ = mpd(real, fake.detach())
            d_loss = discriminator_loss(y_d_rs, y_d_gs)
            d_loss.backward()
            io[pre + 'losses'] = np.array([float(d_loss.detach()), float(adv.detach()), float(feat.detach())], dtype=np.float64)
            io[pre + 'dfake'] = dfake.numpy()
            for k, p in mpd.named_parameters():
                g = p.grad.detach().double().reshape(-1).numpy()
                io[pre + 'd.' + k] = g[sample_idx(g.size)]
                io[pre + 'dnorm.' + k] = np.array([np.linalg.norm(g)])
            print(hidden, L, io[pre + 'losses'], flush=True)
    np.savez_compressed(os.path.join(OUT, 'mpd_io.npz'), **io)
    json.dump(meta, open(os.path.join(OUT, 'mpd_meta.json'), 'w'), indent=1)


if __name__ == '__main__':
    main()
