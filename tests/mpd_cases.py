"""HiFi-GAN multi-period critic (aero_amd/mpd.py, csrc/k_mpd.h) against the REFERENCE's MultiPeriodDiscriminator
(tests/golden/mpd_io.npz / mpd_meta.json from tools/make_golden_mpd.py: discriminators.py:85-147 with its losses :210-243)."""
import functools
import json
import os

import numpy as np
import torch

from conftest import GOLDEN, load_npz, rel_l2, seeded


def meta():
    return json.load(open(os.path.join(GOLDEN, 'mpd_meta.json')))


def seeded_mpd(hidden):
    from aero_amd.mpd import MultiPeriodDiscriminator
    torch.manual_seed(meta()['seeds'][str(hidden)])
    return MultiPeriodDiscriminator(hidden=hidden)


def checksum_errors(hidden):
    """per key: max of the relative deviations of (sum, |sum|) from the reference's seeded state dict"""
    d = seeded_mpd(hidden)
    ref = meta()['checksums'][str(hidden)]
    assert set(d.state_dict()) == set(ref), set(d.state_dict()) ^ set(ref)
    out = {}
    for k, v in d.state_dict().items():
        s, a = ref[k]
        out[k] = max(abs(float(v.double().sum()) - s) / max(1.0, a), abs(float(v.double().abs().sum()) - a) / a)
    return out


def signals(L):
    m = meta()
    s1, s2 = m['signal_seeds'][str(L)]
    return m['signal_scale'] * seeded((m['batch'], 1, L), s1), m['signal_scale'] * seeded((m['batch'], 1, L), s2)


def sample_idx(n):
    return np.unique(np.linspace(0, n - 1, 64).round().astype(np.int64))


@functools.lru_cache(maxsize=None)
def case_io(dev, hidden, L, emulator=False):
    """forward (every feature map of D(fake), both logits), the three losses, the fake waveform's gradient of adv + lambda * feat and the
    critic loss's parameter gradients -> {name: relative error}"""
    lib = None
    if emulator:
        from aero_amd import _lib
        from emu.build_emu import build
        lib = _lib.load(build())
    io = load_npz('mpd_io.npz')
    pre = f'h{hidden}.L{L}.'
    d = seeded_mpd(hidden)
    if lib is not None:
        d.use_library(lib)
    d.to(dev)
    fake, real = (s.to(dev) for s in signals(L))
    errs = {}
    y_d_rs, y_d_gs, fmap_rs, fmap_gs = d(real, fake)
    assert len(fmap_gs) == 5 and all(len(f) == 6 for f in fmap_gs)
    for i in range(5):
        for j, fm in enumerate(fmap_gs[i]):
            fm = fm.float().cpu()
            ref = io[pre + f'fake.{i}.{j}']
            got = fm[:, ::max(1, fm.shape[1] // 4), ::max(1, fm.shape[2] // 16), :]
            assert got.shape == ref.shape, (i, j, got.shape, ref.shape)
            errs[f'map.{i}.{j}'] = rel_l2(got, ref)
        errs[f'logits_fake.{i}'] = rel_l2(y_d_gs[i].float().cpu(), io[pre + f'logits_fake.{i}'])
        errs[f'logits_real.{i}'] = rel_l2(y_d_rs[i].float().cpu(), io[pre + f'logits_real.{i}'])
    fk = fake.clone().requires_grad_(True)
    dl = d.discriminator_loss(fk, real)
    adv, feat = d.generator_losses(fk, real, meta()['features_loss_lambda'])
    lo = io[pre + 'losses']
    for k, v, r in zip(('d_loss', 'adv', 'feat'), (dl, adv, feat), lo):
        errs[k] = abs(float(v) - r) / abs(r)
    (adv + feat).backward()
    errs['dx'] = rel_l2(fk.grad.cpu(), io[pre + 'dfake'])
    dl.backward()
    for k, p in d.named_parameters():
        g = p.grad.detach().double().reshape(-1).cpu().numpy()
        n_ref = io[pre + 'dnorm.' + k][0]
        errs['d.' + k] = max(rel_l2(g[sample_idx(g.size)], io[pre + 'd.' + k]), abs(np.linalg.norm(g) - n_ref) / n_ref)
    return errs


def check_io(errs, map_bar=1e-3):
    """all 5 periods x 6 maps and both logits <= map_bar rel-L2 (1e-3; 1.5e-3 at hidden 32: the fp16 storage itself costs that there --
    float64 torch on the reference module with ONLY the input, the MFMA layers' weights and every activation rounded to fp16 is 1.08e-3
    off the fp32 reference on map 4.3 (period 11, conv 3) at L 4001, where the kernels measured 1.12e-3); losses <= 1e-4 relative; the fake waveform's gradient <= 1e-2; every
    parameter gradient of the critic loss <= 1e-2 (sampled elements and norm) -- except conv 0's weight_v / weight_g: 4e-2.
    Why conv 0: the critic stores its input and every activation in fp16 (as the MelGAN critic does).  In float64 torch.autograd on the
    reference module, rounding ONLY the input to fp16 moves conv 0's weight_v gradient by up to 1.2e-2, and rounding every feature map
    as well by up to 3.2e-2 (period 2 at hidden 8, L 4001) -- the kernels reproduce that rounding to within their own fp32 error
    (test_mpd_ops_on_the_emulator), so conv 0's weight-direction gradient carries the fp16 boundary, not a kernel defect."""
    maps = {k: v for k, v in errs.items() if k.startswith(('map.', 'logits'))}
    assert len(maps) == 40 and max(maps.values()) < map_bar, sorted(maps.items(), key=lambda kv: -kv[1])[:5]
    assert errs['d_loss'] < 1e-4 and errs['adv'] < 1e-4 and errs['feat'] < 1e-4, errs
    assert errs['dx'] < 1e-2, errs['dx']
    bad = {k: v for k, v in errs.items() if k.startswith('d.') and not v < (4e-2 if '.convs.0.weight_' in k else 1e-2)}
    assert not bad, bad
    assert sum(1 for k in errs if k.startswith('d.')) == 90


def torch_period_gradients(d, fake, real):
    """per period: the critic loss's parameter gradients through torch's own modules (the weight-normed nn.Conv2d of `d`, fp32) ->
    {name: gradient}, and the fake waveform's gradient of the generator losses"""
    import torch.nn.functional as F
    out = {}
    for i, dp in enumerate(d.discriminators):
        def run(x):
            b, c, t = x.shape
            if t % dp.period:
                x = F.pad(x, (0, dp.period - t % dp.period), 'reflect')
            x = x.view(b, c, -1, dp.period)
            for conv in dp.convs:
                x = F.leaky_relu(conv(x), 0.1)
            return torch.flatten(dp.conv_post(x), 1, -1)
        dp.zero_grad()
        loss = torch.mean((1 - run(real)) ** 2) + torch.mean(run(fake.detach()) ** 2)
        grads = torch.autograd.grad(loss, list(dp.parameters()))
        for (k, _), g in zip(dp.named_parameters(), grads):
            out[f'discriminators.{i}.{k}'] = g
    return out
