"""The training data path on the MI355X at BASELINE config 5's per-GPU batch (2 clips of 10 s, 11.025 / 44.1 kHz): ms per
`DeviceLrHrStore.batch` (HIP events around the whole call: two table uploads and one aero_segment_gather launch per side), the two gather
launches alone and their achieved bytes per second (arena bytes read + fp32 bytes written), next to the host reader for the same batch.

    python tools/bench_data.py [--files 20] [--iters 50] [--batch 2]
    python tools/bench_data.py --make-set DIR [--files 20]      # only write the set: PCM16 noise files + lr.json / hr.json (for train.py runs)"""
import argparse
import json
import os
import statistics
import struct
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
LR_SR, HR_SR, SECONDS = 11025, 44100, 10


def write_pcm16(path, a, sr):
    pcm = a.astype('<i2').tobytes()
    hdr = b'RIFF' + struct.pack('<I', 36 + len(pcm)) + b'WAVE' + b'fmt ' + struct.pack('<IHHIIHH', 16, 1, 1, sr, sr * 2, 2, 16)
    with open(path, 'wb') as f:
        f.write(hdr + b'data' + struct.pack('<I', len(pcm)) + pcm)


def make_set(d, files):
    """`files` clips of exactly one segment: one item per file"""
    rng = np.random.default_rng(5)
    lists = {'lr': [], 'hr': []}
    for side, sr in (('lr', LR_SR), ('hr', HR_SR)):
        os.makedirs(os.path.join(d, side), exist_ok=True)
        for k in range(files):
            path = os.path.join(d, side, f'clip{k:03d}.wav')
            write_pcm16(path, rng.integers(-3000, 3000, size=SECONDS * sr), sr)
            lists[side].append([path, SECONDS * sr])
        json.dump(lists[side], open(os.path.join(d, side + '.json'), 'w'))
    return d


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--files', type=int, default=20)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--batch', type=int, default=2)
    ap.add_argument('--make-set')
    a = ap.parse_args()
    if a.make_set:
        print(make_set(a.make_set, a.files))
        return
    from aero_amd import data
    with tempfile.TemporaryDirectory() as d:
        make_set(d, a.files)
        ds = data.LrHrSet(d, LR_SR, HR_SR, SECONDS, SECONDS, upsample=False)
        t0 = time.time()
        store = data.DeviceLrHrStore(ds, 'cuda')
        torch.cuda.synchronize()
        print(f'store: {len(ds)} items, {store.nbytes / 1e6:.1f} MB of {store.sides[0].arena.dtype} arenas, decoded and uploaded in {time.time() - t0:.2f} s')
        order = data.EpochSampler(len(ds), shuffle=True, seed=1).indices()
        batches = [order[i:i + a.batch] for i in range(0, len(order) - a.batch + 1, a.batch)]
        k = [0]

        def whole():
            k[0] += 1
            return store.batch(batches[k[0] % len(batches)])
        med, lo, hi = timed(whole, a.iters)
        print(f'store.batch, B = {a.batch}: median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}) over {a.iters} calls')
        lo_s, hi_s = store.sides
        B = a.batch
        files = torch.tensor(batches[0], dtype=torch.int32).cuda()
        starts = torch.zeros(B, dtype=torch.int64).cuda()
        outs = [torch.empty(B, SECONDS * LR_SR, device='cuda'), torch.empty(B, SECONDS * HR_SR, device='cuda')]

        def launches():
            data.segment_gather(store.lib, hi_s.arena, hi_s.file_off, hi_s.file_len, files, starts, SECONDS * HR_SR, outs[1])
            data.segment_gather(store.lib, lo_s.arena, lo_s.file_off, lo_s.file_len, files, starts, SECONDS * LR_SR, outs[0])
        med, lo, hi = timed(launches, a.iters)
        nbytes = B * SECONDS * (LR_SR + HR_SR) * (lo_s.arena.element_size() + 4)
        print(f'the two aero_segment_gather launches alone: median {med * 1e3:.1f} us (min {lo * 1e3:.1f}, max {hi * 1e3:.1f}); '
              f'{nbytes / 1e6:.2f} MB read + written -> {nbytes / (med * 1e-3) / 1e9:.0f} GB/s (for context: launch-bound at this size)')
        t0 = time.time()
        n = min(10, len(batches))
        for b in batches[:n]:
            data.host_batch(ds, b, 'cuda')
        torch.cuda.synchronize()
        print(f'host reader (audio_io.load per item, stack, upload), same batches, in-process: {1e3 * (time.time() - t0) / n:.2f} ms per batch')


if __name__ == '__main__':
    main()
