"""What fp16 storage alone costs the multi-period critic `mpd` against the reference's fp32 goldens (tests/golden/mpd_io.npz): the
reference's own MultiPeriodDiscriminator (discriminators.py:85-147) in FLOAT64 torch, with rounding to fp16 exactly where aero_amd/mpd.py
stores fp16 -- (a) the critic's input only; (b) the input, the weights of the MFMA convs 1-4 (their fp16 image) and every feature map
(straight-through: the gradient itself is not rounded).  Prints, per golden case, the rel-L2 of every feature map of D(fake) (subsampled
as the golden) and the relative error of every critic-loss parameter gradient (64 sampled elements and the norm, as tests/mpd_cases.py),
sorted, worst last.  The bars of tests/mpd_cases.check_io for the maps at hidden 32 and for conv 0's weight_v / weight_g rest on this.
Runs only in the build container (imports the reference checkout, argv[1], default /root/reference):

    python -B tools/dbg/mpd_fp16_storage.py > profiles/mpd_fp16_storage.txt"""
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

sys.dont_write_bytecode = True
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..', 'tests', 'golden')


def seeded(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def r16(t):
    return t.half().double()


def st16(t):
    return t + (r16(t) - t).detach()                                 # fp16 value, unrounded gradient


def run(mpd, x, mode):
    """-> per period ([6 feature maps], logits) of the float64 module with the fp16 rounding of `mode` ('input' / 'storage')"""
    x = r16(x)
    out = []
    for d in mpd.discriminators:
        b, c, t = x.shape
        h = F.pad(x, (0, d.period - t % d.period), 'reflect') if t % d.period else x
        h = h.view(b, c, -1, d.period)
        maps = []
        for j, conv in enumerate(list(d.convs) + [d.conv_post]):
            w = conv.weight_g * conv.weight_v / conv.weight_v.flatten(1).norm(dim=1).view(-1, 1, 1, 1)
            if mode == 'storage' and 1 <= j <= 4:
                w = st16(w)
            h = F.conv2d(h, w, conv.bias, conv.stride, conv.padding)
            if j < 5:
                h = F.leaky_relu(h, 0.1)
            if mode == 'storage':
                h = st16(h)
            maps.append(h)
        out.append((maps, torch.flatten(h, 1, -1)))
    return out


def main():
    sys.path.insert(0, sys.argv[1] if len(sys.argv) > 1 else '/root/reference')
    sys.modules.setdefault('cv2', types.ModuleType('cv2'))          # (src.utils imports cv2, absent here and unused by the critic)
    from src.models.discriminators import MultiPeriodDiscriminator
    torch.set_num_threads(8)
    meta = json.load(open(os.path.join(GOLDEN, 'mpd_meta.json')))
    io = dict(np.load(os.path.join(GOLDEN, 'mpd_io.npz')))
    idx = lambda n: np.unique(np.linspace(0, n - 1, 64).round().astype(np.int64))          # noqa: E731
    for hidden in (8, 32):
        for L in meta['lengths']:
            pre = f'h{hidden}.L{L}.'
            s1, s2 = meta['signal_seeds'][str(L)]
            fake = (meta['signal_scale'] * seeded((meta['batch'], 1, L), s1)).double()
            real = (meta['signal_scale'] * seeded((meta['batch'], 1, L), s2)).double()
            for mode in ('input', 'storage'):
                torch.manual_seed(meta['seeds'][str(hidden)])
                mpd = MultiPeriodDiscriminator(hidden=hidden).double()
                rows = []
                of, orr = run(mpd, fake, mode), run(mpd, real, mode)
                for i, (maps, _) in enumerate(of):
                    for j, fm in enumerate(maps):
                        got = fm.detach()[:, ::max(1, fm.shape[1] // 4), ::max(1, fm.shape[2] // 16), :]
                        ref = torch.from_numpy(io[pre + f'fake.{i}.{j}']).double()
                        rows.append((float((got - ref).norm() / ref.norm()), f'map.{i}.{j}'))
                loss = sum(torch.mean((1 - lr) ** 2) + torch.mean(lf ** 2) for (_, lf), (_, lr) in zip(of, orr))
                loss.backward()
                for k, p in mpd.named_parameters():
                    g = p.grad.reshape(-1).numpy()
                    ref, nref = io[pre + 'd.' + k], io[pre + 'dnorm.' + k][0]
                    e = max(float(np.linalg.norm(g[idx(g.size)] - ref) / np.linalg.norm(ref)), abs(np.linalg.norm(g) - nref) / nref)
                    rows.append((e, 'd.' + k))
                maps_ = sorted(r for r in rows if r[1].startswith('map'))
                grads = sorted(r for r in rows if r[1].startswith('d.'))
                print(f'hidden {hidden}  L {L}  fp16 {mode:8s}  worst maps: ' + ', '.join(f'{n} {e:.2e}' for e, n in maps_[-3:]))
                print(f'hidden {hidden}  L {L}  fp16 {mode:8s}  worst gradients: ' + ', '.join(f'{n} {e:.2e}' for e, n in grads[-4:]))
                other = [e for e, n in grads if '.convs.0.weight_' not in n]
                print(f'hidden {hidden}  L {L}  fp16 {mode:8s}  worst gradient outside conv 0 weight_v / weight_g: {max(other):.2e}', flush=True)


if __name__ == '__main__':
    main()
