"""Minimal WAV I/O (host plumbing) so predict.py / test.py run without torchaudio (absent from the image).

`load(path) -> (float32 tensor [channels, samples] in [-1, 1], sample_rate)` and `save(path, wav, sr)` follow
torchaudio.load / torchaudio.save as used by the reference (predict.py:53, enhance.py:18-21); `load(path, frame_offset, num_frames)` reads
only that range and `info(path)` only the header (the dataset readers, src/data/audio.py:49-51, data_prep/create_meta_files.py:20-27).
PCM16 and IEEE float32 RIFF files are supported; torchaudio is used instead when importable.
"""
import struct

import numpy as np
import torch


def _header(f, path):
    """walk the RIFF chunks of an open file without reading their bodies -> (fmt tuple, data offset, data bytes)"""
    head = f.read(12)
    if head[:4] != b'RIFF' or head[8:12] != b'WAVE':
        raise ValueError(f'{path}: not a RIFF/WAVE file')
    end = f.seek(0, 2)
    pos, fmt, data = 12, None, None
    while pos + 8 <= end:
        f.seek(pos)
        cid, size = struct.unpack('<4sI', f.read(8))
        if cid == b'fmt ':
            fmt = struct.unpack('<HHIIHH', f.read(16))
        elif cid == b'data':
            data = (pos + 8, min(size, end - pos - 8))
        pos += 8 + size + (size & 1)
    if fmt is None or data is None:
        raise ValueError(f'{path}: missing fmt/data chunk')
    tag, _, _, _, _, bits = fmt
    if (tag, bits) not in ((1, 16), (3, 32)):
        raise ValueError(f'{path}: unsupported WAV encoding (tag {tag}, {bits} bit)')
    return fmt, data[0], data[1]


def info(path):
    """`torchaudio.info` as data_prep/create_meta_files.py uses it -> (n_frames, sample_rate, channels); reads the header only"""
    try:
        import torchaudio
        i = torchaudio.info(str(path))
        return i.num_frames, i.sample_rate, i.num_channels
    except ImportError:
        pass
    with open(path, 'rb') as f:
        (_, nch, sr, _, _, bits), _, nbytes = _header(f, path)
    return nbytes // (bits // 8) // nch, sr, nch


def encoding(path):
    """'pcm16' or 'f32': how the samples of a supported file are stored"""
    with open(path, 'rb') as f:
        fmt, _, _ = _header(f, path)
    return 'pcm16' if fmt[0] == 1 else 'f32'


def load_raw(path, frame_offset=0, num_frames=-1):
    """the samples as stored: (int16 or float32 array [frames, channels], sample_rate); only the bytes asked for are read"""
    with open(path, 'rb') as f:
        (tag, nch, sr, _, _, bits), pos, nbytes = _header(f, path)
        step = bits // 8 * nch
        total = nbytes // step
        first = min(max(int(frame_offset), 0), total)
        count = total - first if num_frames is None or num_frames < 0 else min(int(num_frames), total - first)
        f.seek(pos + first * step)
        raw = f.read(count * step)
    a = np.frombuffer(raw, dtype='<i2' if tag == 1 else '<f4')
    return a[:len(a) // nch * nch].reshape(-1, nch), sr


def load(path, frame_offset=0, num_frames=-1):
    """frames [frame_offset, frame_offset + num_frames) of the file (to its end with num_frames = -1; fewer, possibly none, where the file
    ends first), as torchaudio.load's arguments of the same names (src/data/audio.py:49-51)"""
    try:
        import torchaudio
        return torchaudio.load(str(path), frame_offset=frame_offset, num_frames=num_frames)
    except ImportError:
        pass
    a, sr = load_raw(path, frame_offset, num_frames)
    if a.dtype == np.int16:
        a = a.astype(np.float32) / 32768.0
    else:
        a = a.astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray(a.T)), sr


def save(path, wav, sr):
    """float32 WAV, [channels, samples]."""
    try:
        import torchaudio
        return torchaudio.save(str(path), wav.cpu(), sr)
    except ImportError:
        pass
    a = wav.detach().cpu().float().numpy()
    if a.ndim == 1:
        a = a[None]
    _write_f32(path, np.ascontiguousarray(a.T), sr)


def _write_f32(path, frames, sr):
    """frames: float32 array [samples, channels], contiguous -- the file's payload as it is stored"""
    nch = frames.shape[1]
    pcm = frames.astype('<f4').tobytes()
    hdr = b'RIFF' + struct.pack('<I', 36 + len(pcm)) + b'WAVE' + b'fmt ' + struct.pack('<IHHIIHH', 16, 3, nch, sr, sr * nch * 4, nch * 4, 32)
    with open(path, 'wb') as f:
        f.write(hdr + b'data' + struct.pack('<I', len(pcm)) + pcm)


def save_frames(path, frames, sr):
    """`save` of a payload that is already interleaved: frames float32 [samples, channels] (enhance.write_device) -- the same file as
    save(path, frames.T, sr)"""
    try:
        import torchaudio
        return torchaudio.save(str(path), frames.cpu().T, sr)
    except ImportError:
        pass
    _write_f32(path, np.ascontiguousarray(frames.detach().cpu().float().numpy()), sr)


def resample(waveform, orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99):
    """`torchaudio.functional.resample(waveform, orig_freq, new_freq)` with its defaults (Hann-windowed sinc interpolation), which the
    reference calls before the model when `experiment.upsample` is set (predict.py:55-57, datasets.py:144).  Host plumbing outside the hot
    path: torchaudio is used when importable; otherwise its published algorithm is restated here (polyphase sinc kernel of
    `new_freq / gcd` phases, width ceil(lowpass_filter_width * orig / (rolloff * min(orig, new))), a strided conv1d, output cropped to
    ceil(new * length / orig) samples).  torchaudio is absent from this image; the restatement is PINNED TO THE PUBLISHED ALGORITHM: a direct
    float64 evaluation of its interpolation formula at three rate ratios (tests/test_callers.py::
    test_resample_against_the_published_interpolation_formula) next to the defining properties (identity, length rule, a tone, linearity)."""
    try:
        from torchaudio.functional import resample as ta_resample
        return ta_resample(waveform, orig_freq, new_freq)
    except ImportError:
        pass
    import math
    orig_freq, new_freq = int(orig_freq), int(new_freq)
    if orig_freq <= 0 or new_freq <= 0:
        raise ValueError('resample: frequencies must be positive integers')
    if orig_freq == new_freq:
        return waveform
    g = math.gcd(orig_freq, new_freq)
    orig, new = orig_freq // g, new_freq // g
    base = min(orig, new) * rolloff
    width = math.ceil(lowpass_filter_width * orig / base)
    idx = torch.arange(-width, width + orig, dtype=torch.float64)[None, None] / orig
    t = torch.arange(0, -new, -1, dtype=torch.float64)[:, None, None] / new + idx
    t = (t * base).clamp_(-lowpass_filter_width, lowpass_filter_width)
    window = torch.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t = t * math.pi
    kernels = torch.where(t == 0, torch.ones_like(t), t.sin() / t) * window * (base / orig)
    kernels = kernels.to(torch.float32)
    shape = waveform.shape
    w = waveform.reshape(-1, shape[-1]).to(torch.float32)
    length = w.shape[-1]
    w = torch.nn.functional.pad(w, (width, width + orig))
    out = torch.nn.functional.conv1d(w[:, None], kernels, stride=orig)
    out = out.transpose(1, 2).reshape(w.shape[0], -1)
    target = int(math.ceil(new * length / orig))
    return out[..., :target].reshape(shape[:-1] + (target,))
