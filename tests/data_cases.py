"""Shared by tests/test_data.py (CPU, emulator library) and tests/test_gpu_data.py (MI355X): wav files written by the tests, the gather
cases of aero_segment_gather against the host reader, the upsample cases against audio_io.resample."""
import json
import os
import struct
from fractions import Fraction

import numpy as np
import torch

from aero_amd import audio_io, data

SENT_I16, SENT_F32 = 12345, 7.0          # the sample behind every file in the test arenas; no file holds it
GATHER_FILES = (1, 5, 64, 257)
# (file, start): inside a file; crossing its end; files shorter than L; two (and more) of one file; odd starts; the first sample of the first
# file; the last of the last; a start that makes the window 16-byte aligned in the arena (offset of file 3 is 73: 73 + 7 = 80)
GATHER_ITEMS = ((3, 16), (3, 200), (1, 0), (0, 0), (3, 33), (2, 1), (3, 7), (3, 256), (2, 0), (1, 3), (2, 63), (3, 193))
GATHER_L = (64, 100)


def emu_lib():
    from aero_amd import _lib
    from emu.build_emu import build
    return _lib.load(build())


def write_wav(path, a, sr, f32):
    """a: int16 [frames] or [frames, channels] as PCM16, or the same values / 32768 as float32"""
    a = np.asarray(a)
    a = a[:, None] if a.ndim == 1 else a
    nch = a.shape[1]
    if f32:
        pcm, tag, bits = (a.astype(np.float32) / 32768.0).astype('<f4').tobytes(), 3, 32
    else:
        pcm, tag, bits = a.astype('<i2').tobytes(), 1, 16
    hdr = b'RIFF' + struct.pack('<I', 36 + len(pcm)) + b'WAVE' + b'fmt ' + struct.pack('<IHHIIHH', 16, tag, nch, sr, sr * nch * bits // 8,
                                                                                       nch * bits // 8, bits)
    with open(path, 'wb') as f:
        f.write(hdr + b'data' + struct.pack('<I', len(pcm)) + pcm)


def noise_i16(n, seed, channels=None):
    shape = (n,) if channels is None else (n, channels)
    a = np.random.default_rng(seed).integers(-32768, 32768, size=shape).astype(np.int16)
    a[a == SENT_I16] = 0
    return a


def gather_case(tmp, f32, device):
    """files of GATHER_FILES samples on disk and in one arena with a sentinel behind each -> (arena, file_off, file_len, paths)"""
    parts, offs, paths = [], [], []
    pos = 0
    for k, n in enumerate(GATHER_FILES):
        a = noise_i16(n, 40 + k)
        path = os.path.join(str(tmp), f'g{k}_{int(f32)}.wav')
        write_wav(path, a, 16000, f32)
        paths.append(path)
        offs.append(pos)
        if f32:
            parts += [a.astype(np.float32) / 32768.0, np.array([SENT_F32], np.float32)]
        else:
            parts += [a, np.array([SENT_I16], np.int16)]
        pos += n + 1
    arena = torch.from_numpy(np.concatenate(parts)).to(device)
    return (arena, torch.tensor(offs, dtype=torch.int64).to(device), torch.tensor(GATHER_FILES, dtype=torch.int64).to(device), paths)


def host_items(paths, items, L):
    """what Audioset.__getitem__ returns for (file, start): a partial read, zero padded to L -- stacked [B, L]"""
    rows = []
    for f, s in items:
        out, _ = audio_io.load(paths[f], frame_offset=s, num_frames=L)
        rows.append(torch.nn.functional.pad(out, (0, L - out.shape[-1]))[0])
    return torch.stack(rows)


def check_gather(lib, tmp, f32, L, device):
    arena, off, ln, paths = gather_case(tmp, f32, device)
    files = torch.tensor([f for f, _ in GATHER_ITEMS], dtype=torch.int32).to(device)
    starts = torch.tensor([s for _, s in GATHER_ITEMS], dtype=torch.int64).to(device)
    out = data.segment_gather(lib, arena, off, ln, files, starts, L).cpu()
    ref = host_items(paths, GATHER_ITEMS, L)
    assert out.shape == ref.shape and out.dtype == torch.float32
    sentinel = SENT_F32 if f32 else SENT_I16 / 32768.0
    assert not bool((out == sentinel).any()), 'a sample from behind a file reached the output'
    assert torch.equal(out, ref), [i for i in range(len(GATHER_ITEMS)) if not torch.equal(out[i], ref[i])]


def make_set(tmp, name, lr_sr, hr_sr, lr_lengths, seg_lr, f32=False, upsample=False, shuffle_lists=True):
    """a json_dir of PCM16 (or float32) files: hr files of lr_length * hr_sr / lr_sr samples; segment = stride = seg_lr lr samples
    (None: whole files).  The seconds are exact fractions, so int(segment * sr) is the intended sample count on both sides."""
    d = os.path.join(str(tmp), name)
    os.makedirs(os.path.join(d, 'lr'))
    os.makedirs(os.path.join(d, 'hr'))
    lr, hr = [], []
    for k, n in enumerate(lr_lengths):
        nh = n * hr_sr // lr_sr
        lp, hp = os.path.join(d, 'lr', f's{k:02d}.wav'), os.path.join(d, 'hr', f's{k:02d}.wav')
        write_wav(lp, noise_i16(n, 100 + k) // 4, lr_sr, f32)
        write_wav(hp, noise_i16(nh, 200 + k) // 4, hr_sr, f32)
        lr.append([lp, n])
        hr.append([hp, nh])
    if shuffle_lists:
        lr, hr = lr[::-1], hr[1:] + hr[:1]
    json.dump(lr, open(os.path.join(d, 'lr.json'), 'w'))
    json.dump(hr, open(os.path.join(d, 'hr.json'), 'w'))
    seg = None if seg_lr is None else Fraction(seg_lr, lr_sr)
    return data.LrHrSet(d, lr_sr, hr_sr, stride=seg, segment=seg, upsample=upsample)


def stacked(ds, indices):
    items = [ds[i] for i in indices]
    return torch.stack([a for a, _ in items]), torch.stack([b for _, b in items])


UPSAMPLE_CASES = [(4000, 16000, 37), (4000, 16000, 256), (11025, 44100, 37), (11025, 44100, 256)]


def check_upsample(lib, tmp, lr_sr, hr_sr, seg, device, rel_l2):
    """lr files of 100, 600 and 30 samples: segments inside a file that continues on both sides, segments cut by the file's end, a file
    shorter than the segment.  hr is bit-equal; lr within rel-L2 2e-6 of audio_io.resample + match_signal of the host segment."""
    ds = make_set(tmp, f'up_{lr_sr}_{seg}', lr_sr, hr_sr, (100, 600, 30), seg, upsample=True)
    store = data.DeviceLrHrStore(ds, device, lib=lib)
    idx = list(range(len(ds)))
    lr, hr = store.batch(idx)
    lr_ref, hr_ref = stacked(ds, idx)
    assert lr.shape == lr_ref.shape == hr_ref.shape and tuple(hr.shape) == (len(ds), 1, seg * hr_sr // lr_sr)
    assert torch.equal(hr.cpu(), hr_ref)
    e = rel_l2(lr.cpu(), lr_ref)                               # (over the whole batch, as tests/test_seanet.py takes this resampler's bar)
    print(f'upsample {lr_sr} -> {hr_sr}, segment {seg}: rel-L2 {e:.3e}; per item {[round(rel_l2(lr[i].cpu(), lr_ref[i]), 9) for i in idx]}')
    assert e <= 2e-6
