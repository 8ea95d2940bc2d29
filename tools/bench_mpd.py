"""The multi-period critic `mpd` at BASELINE config 5's shapes (2 clips x 441 000 samples, hidden 32): one critic step's device work --
the forward of D(fake) || D(real), the generator losses' backward to the fake waveform, the critic loss's backward to every parameter --
timed on the HIP path (aero_amd/mpd.py) and, as a yardstick, through torch's own modules (the same weight-normed nn.Conv2d, fp32
autograd).  Prints the algorithmic GFLOP of the forward per conv layer (not the 6/5 of the 2-tap form) and the milliseconds.
usage: python tools/bench_mpd.py [iters]   (rocprofv3 --kernel-trace --stats -- python tools/bench_mpd.py 3: per-kernel times)"""
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aero_amd.mpd import MultiPeriodDiscriminator  # noqa: E402


def layer_gflop(mpd, L, B):
    """algorithmic forward GFLOP per conv layer j (summed over the periods) for B clips of L samples"""
    out = [0.0] * 6
    for d in mpd.discriminators:
        H = -(-L // d.period)
        for j, conv in enumerate(d.layers()):
            Cout, Cin, K = conv.weight_v.shape[:3]
            H = (H + 2 * conv.padding[0] - K) // conv.stride[0] + 1
            out[j] += 2.0 * B * d.period * H * Cout * Cin * K / 1e9
    return out


def main():
    iters = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    torch.manual_seed(0)
    mpd = MultiPeriodDiscriminator().cuda()
    g = torch.Generator().manual_seed(1)
    fake = (0.3 * torch.randn(2, 1, 441000, generator=g)).cuda()
    real = (0.3 * torch.randn(2, 1, 441000, generator=g)).cuda()
    gf = layer_gflop(mpd, 441000, 4)                              # the forward runs fake || real
    print('forward GFLOP per conv layer (fake || real):', [round(v, 1) for v in gf], 'total', round(sum(gf), 1))

    def hip_step():
        fk = fake.clone().requires_grad_(True)
        mpd.repack()                                              # (a fresh forward every iteration, as after an optimizer step)
        adv, feat = mpd.generator_losses(fk, real, 100.0)
        (adv + feat).backward()
        mpd.zero_grad()
        mpd.discriminator_loss(fk.detach(), real).backward()

    def torch_step():
        fk = fake.clone().requires_grad_(True)
        tot = 0
        for dp in mpd.discriminators:
            def run(x):
                b, c, t = x.shape
                if t % dp.period:
                    x = F.pad(x, (0, dp.period - t % dp.period), 'reflect')
                x = x.view(b, c, -1, dp.period)
                for conv in dp.convs:
                    x = F.leaky_relu(conv(x), 0.1)
                return dp.conv_post(x)
            tot = tot + torch.mean((1 - run(fk)) ** 2) + torch.mean(run(real) ** 2)
        tot.backward()

    for name, fn in (('hip', hip_step), ('torch', torch_step), ('hip', hip_step), ('torch', torch_step)):
        fn()
        torch.cuda.synchronize()
        t0 = time.time()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        print(f'{name}: {1e3 * (time.time() - t0) / iters:.2f} ms per critic step (forward + generator backward + critic backward)', flush=True)


if __name__ == '__main__':
    main()
