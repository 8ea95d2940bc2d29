"""The serving path on the MI355X for one long file at BASELINE config 2's geometry (4 -> 16 kHz, aero_4-16_512_64, random weights): ms per
`enhance.predict_signal` of a 10-minute mono recording (HIP events around the whole call, upload and download included; median of
`--iters` after `--warmup`), with independent chunks (overlap = 0: the parent's path, 60 chunk forwards) and with overlapped chunks
stitched on the device (overlap = 0.5 s: 64 chunk forwards), and the two new launches alone with their achieved bytes per second.

    python tools/bench_predict.py [--minutes 10] [--iters 10] [--warmup 2] [--overlap-sec 0.5]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
LR_SR, HR_SR = 4000, 16000


def timed(fn, iters, warmup):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--minutes', type=float, default=10)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--overlap-sec', type=float, default=0.5)
    a = ap.parse_args()
    from aero_amd import _lib, enhance
    from aero_amd.config import load_config
    args = load_config(os.path.join(ROOT, 'conf'), ['experiment=aero_4-16_512_64', '+random_init=true'])
    torch.manual_seed(1)
    model = enhance.load_generator(args, device='cuda')
    N = int(a.minutes * 60 * LR_SR)
    sig = 0.1 * torch.randn(1, N, generator=torch.Generator().manual_seed(2))
    pcm = (sig * 32768.0).round().clamp(-32768, 32767).to(torch.int16)
    ov = round(a.overlap_sec * LR_SR)
    n0, n1 = len(enhance.chunk_ranges(N, LR_SR)), len(enhance.overlap_ranges(N, LR_SR, ov))
    print(f'file: {a.minutes:g} min mono at {LR_SR} Hz = {N} samples; {n0} chunks without overlap, {n1} with {ov} samples ({a.overlap_sec:g} s) of overlap')
    runs = [('overlap = 0 (independent chunks, host concatenation: the parent\'s path)', lambda: enhance.predict_signal(model, sig, LR_SR)),
            (f'overlap = {ov} (stitched on the device, fp32 upload, one download)', lambda: enhance.predict_signal(model, sig, LR_SR, overlap=ov)),
            (f'overlap = {ov}, PCM16 upload', lambda: enhance.predict_signal(model, pcm, LR_SR, overlap=ov)),
            (f'overlap = {ov}, result left on the device', lambda: enhance.predict_signal(model, sig, LR_SR, overlap=ov, return_device=True))]
    base = None
    for name, fn in runs + runs[:2]:                             # (the first two once more at the end: the run-to-run spread of this visit)
        med, lo, hi = timed(fn, a.iters, a.warmup)
        base = base or med
        print(f'predict_signal, {name}: median {med:.1f} ms (min {lo:.1f}, max {hi:.1f}) over {a.iters} calls; x{med / base:.3f} of the first line '
              f'(chunk forwards alone would be x{n1 / n0:.3f})')
    # the two new launches alone, at the sizes of that file: one group of all the full chunks, then the whole payload
    lib = _lib.load()
    hop, V = enhance.output_hop(LR_SR, ov, HR_SR // LR_SR)
    g = n1 - 1
    y = torch.randn(g, 1, hop + V, device='cuda')
    fade = enhance.fade_table(max(V, 1)).cuda()
    out = torch.empty(1, g * hop + hop + V, device='cuda')
    peak = torch.zeros(1, dtype=torch.int32, device='cuda')
    med, lo, hi = timed(lambda: enhance.overlap_stitch(lib, y, None, fade, V, hop, 0, False, out, peak), 50, 5)
    nbytes = 4 * (g * hop + (g - 1) * V) + 4 * g * hop
    print(f'aero_overlap_stitch alone, {g} chunks of {hop + V} samples: median {med * 1e3:.1f} us (min {lo * 1e3:.1f}, max {hi * 1e3:.1f}); '
          f'{nbytes / 1e6:.1f} MB read + written -> {nbytes / (med * 1e-3) / 1e9:.0f} GB/s')
    med, lo, hi = timed(lambda: enhance.wav_finalize(lib, out, peak), 50, 5)
    nbytes = 8 * out.numel()
    print(f'aero_wav_finalize alone, {out.numel()} samples (the output allocation included): median {med * 1e3:.1f} us (min {lo * 1e3:.1f}, '
          f'max {hi * 1e3:.1f}); {nbytes / 1e6:.1f} MB read + written -> {nbytes / (med * 1e-3) / 1e9:.0f} GB/s')


if __name__ == '__main__':
    main()
