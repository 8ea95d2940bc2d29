"""Seanet forward on the MI355X at the shipped shape (seanet_4-16.yaml: 2-s clips, 4 -> 16 kHz, ngf 32), ms per forward (HIP events, warm-up,
the median and the spread of the timed forwards) for
  (i)   the HIP path with the fused ResnetBlock kernel,
  (ii)  the same with AERO_SEANET_FUSE=0 (three launches of the general conv per block),
  (iii) a from-scratch restatement of the same net in fp16 through torch's own modules (its input already resampled: the conv stack only),
and the C = 32 ResnetBlock alone: achieved bytes/s against its algorithmic bytes (x read once, y written once).

    python tools/bench_seanet.py [--batches 16 64] [--iters 30]"""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch
from torch import nn
from torch.nn import functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


def timed(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


class TorchBlock(nn.Module):
    def __init__(self, dim, d):
        super().__init__()
        self.d = d
        self.c1, self.c2, self.sc = nn.Conv1d(dim, dim, 3, dilation=d), nn.Conv1d(dim, dim, 1), nn.Conv1d(dim, dim, 1)

    def forward(self, x):
        return self.sc(x) + self.c2(F.leaky_relu(self.c1(F.pad(F.leaky_relu(x, 0.2), (self.d, self.d), mode='reflect')), 0.2))


class TorchSeanet(nn.Module):
    """the same layers through torch's modules (weights random: only the time is of interest)"""

    def __init__(self, ngf=32, ratios=(8, 8, 2, 2), nres=3, latent=128):
        super().__init__()
        self.enc, self.dec = nn.ModuleList(), nn.ModuleList()
        mult = 2 ** len(ratios)
        self.enc.insert(0, nn.Conv1d(mult * ngf, latent, 7))
        self.dec.append(nn.Conv1d(latent, mult * ngf, 7))
        for r in ratios:
            p = r // 2 + r % 2
            e = [TorchBlock(mult * ngf // 2, 3 ** j) for j in range(nres)] + [nn.LeakyReLU(0.2), nn.Conv1d(mult * ngf // 2, mult * ngf, 2 * r, r, p)]
            d = [nn.LeakyReLU(0.2), nn.ConvTranspose1d(mult * ngf, mult * ngf // 2, 2 * r, r, p, output_padding=r % 2)]
            d += [TorchBlock(mult * ngf // 2, 3 ** j) for j in range(nres)]
            mult //= 2
            self.enc.insert(0, nn.Sequential(*e))
            self.dec.append(nn.Sequential(*d))
        self.enc.insert(0, nn.Conv1d(1, ngf, 7))
        self.dec.append(nn.Conv1d(ngf, 1, 7))

    def forward(self, x):
        n, skips = len(self.enc), []
        for i, m in enumerate(self.enc):
            skips.append(x)
            if i == 0:
                x = torch.tanh(m(F.pad(x, (3, 3), mode='reflect')))
            elif i == n - 1:
                x = m(F.pad(F.leaky_relu(x, 0.2), (3, 3), mode='reflect'))
            else:
                x = m(x)
        for j, m in enumerate(self.dec):
            if j == 0 or j == n - 1:
                x = m(F.pad(F.leaky_relu(x, 0.2), (3, 3), mode='reflect'))
                x = torch.tanh(x) if j == n - 1 else x
            else:
                x = m(x)
            x = x + skips.pop()
        return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[16, 64])
    ap.add_argument('--iters', type=int, default=30)
    a = ap.parse_args()
    from aero_amd import _lib
    from aero_amd.seanet import Seanet, mfma_image
    torch.manual_seed(0)
    model = Seanet(lr_sr=4000, hr_sr=16000).eval().cuda()
    ref = TorchSeanet().half().eval().cuda()
    print(f'device {torch.cuda.get_device_name(0)}; {a.iters} timed forwards after 5 warm-up; ms = median [min, max]')
    for B in a.batches:
        x = 0.3 * torch.randn(B, 1, 8000, device='cuda')
        xr = 0.3 * torch.randn(B, 1, 32000, device='cuda', dtype=torch.float16)
        with torch.no_grad():
            os.environ['AERO_SEANET_FUSE'] = '1'
            fused = timed(lambda: model(x), a.iters)
            os.environ['AERO_SEANET_FUSE'] = '0'
            layers = timed(lambda: model(x), a.iters)
            os.environ['AERO_SEANET_FUSE'] = '1'
            tt = timed(lambda: ref(xr), a.iters)
        for name, t in (('(i) fused', fused), ('(ii) AERO_SEANET_FUSE=0', layers), ('(iii) torch fp16 modules', tt)):
            print(f'B={B:3d} {name:28s} {t[0]:8.3f} ms [{t[1]:.3f}, {t[2]:.3f}]')
    # the C = 32 block alone at T = 32000 (decoder 4 / encoder 1)
    lib = _lib.load()
    for B in a.batches:
        Cc, T, d = 32, 32000, 3
        h = torch.randn(B, T, Cc, device='cuda').half()
        y = torch.empty_like(h)
        w1, w2s = mfma_image(0.1 * torch.randn(Cc, 3 * Cc), 'cuda'), mfma_image(0.1 * torch.randn(Cc, 2 * Cc), 'cuda')
        b1, b2 = torch.zeros(Cc, device='cuda'), torch.zeros(Cc, device='cuda')
        r = _lib.SeanetResDesc()
        r.x, r.w1, r.w2s, r.b1, r.b2s, r.add, r.y = h.data_ptr(), w1.data_ptr(), w2s.data_ptr(), b1.data_ptr(), b2.data_ptr(), None, y.data_ptr()
        r.B, r.T, r.C, r.d, r.ks1, r.ks2, r.slope = B, T, Cc, d, 3, 2, 0.2
        st = torch.cuda.current_stream().cuda_stream
        t = timed(lambda: lib.call('aero_seanet_resblock', C.byref(r), st), a.iters)
        nbytes = 2 * h.numel() * 2
        flops = 2 * 5 * Cc * Cc * B * T
        print(f'resblock C=32 d=3 B={B} T={T}: {t[0] * 1e3:.1f} us [{t[1] * 1e3:.1f}, {t[2] * 1e3:.1f}]; algorithmic {nbytes / 1e6:.1f} MB -> '
              f'{nbytes / t[0] / 1e6:.0f} GB/s, {flops / t[0] / 1e9:.1f} TFLOP/s')


if __name__ == '__main__':
    main()
