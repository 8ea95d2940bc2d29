"""Training data: the reference's wav-file datasets (src/data/audio.py:9-67, src/data/datasets.py:82-161) restated on `audio_io`, the
sampler of its training loader, and a device-resident store that cuts a batch out of the decoded samples with one kernel launch per side.

    Audioset          <- src/data/audio.py:9-67        which segment of which file an index is; a partial read, zero padded on the right
    LrHrSet           <- src/data/datasets.py:82-161   the sorted lr.json / hr.json lists as two Audiosets, optional resampling of the lr side
    EpochSampler      <- torch.utils.data.distributed.DistributedSampler as distrib.loader builds it (distrib.py:86-88)
    DeviceLrHrStore   every file decoded ONCE into a device arena per side (int16 as stored, or fp32); `batch(indices)` is
                      aero_segment_gather (csrc/k_data.h) per side, bit-equal to the stacked host items

The index arithmetic is integer-exact to the reference (tests/golden/data_index.json records the reference's own load calls).  Why a
store at all: a config-5 step is 18-26 ms for two 10-second clips per GPU, parsing a wav file in Python per item is slower than that, the
whole VCTK set as PCM16 is about 6 GB and an MI355X has 288 GB.
"""
import json
import math
import os

import numpy as np
import torch

from . import audio_io
from .enhance import match_signal

DEFAULT_MAX_BYTES = 16 << 30            # per process: the machines are shared


class Audioset:
    def __init__(self, files=None, length=None, stride=None, pad=True, with_path=False, sample_rate=None, channels=None):
        """files: [(file, length in samples)] (audio.py:13-15)"""
        self.files = files
        self.num_examples = []
        self.length = length
        self.stride = stride or length
        self.with_path = with_path
        self.sample_rate = sample_rate
        self.channels = channels
        for _, file_length in self.files:
            if length is None:
                examples = 1
            elif file_length < length:
                examples = 1 if pad else 0
            elif pad:
                examples = int(math.ceil((file_length - self.length) / self.stride) + 1)
            else:
                examples = (file_length - self.length) // self.stride + 1
            self.num_examples.append(examples)

    def __len__(self):
        return sum(self.num_examples)

    def locate(self, index):
        """-> (position in `files`, frame_offset, num_frames; 0 = the whole file) of item `index` (audio.py:39-47)"""
        for i, examples in enumerate(self.num_examples):
            if index >= examples:
                index -= examples
                continue
            if self.length is None:
                return i, 0, 0
            return i, self.stride * index, self.length
        raise IndexError(index)

    def check(self, file, sr, channels):
        if sr != self.sample_rate:
            raise RuntimeError(f"Expected {file} to have sample rate of {self.sample_rate}, but got {sr}")
        if channels != self.channels:
            raise RuntimeError(f"Expected {file} to have shape of {self.channels}, but got {channels}")

    def __getitem__(self, index):
        i, offset, num_frames = self.locate(index)
        file = self.files[i][0]
        out, sr = audio_io.load(str(file), frame_offset=offset, num_frames=num_frames or -1)
        self.check(file, sr, out.shape[0])
        if num_frames:
            out = torch.nn.functional.pad(out, (0, num_frames - out.shape[-1]))
        return (out, file) if self.with_path else out


class LrHrSet(torch.utils.data.Dataset):
    def __init__(self, json_dir, lr_sr, hr_sr, stride=None, segment=None, pad=True, with_path=False, stft=False, upsample=True):
        """json_dir holds lr.json and hr.json, each [[path, n_samples], ...]; stride / segment in seconds (datasets.py:86-99)"""
        if stft:
            raise NotImplementedError('LrHrSet(stft=True): spectrogram items are not built (no entry point of the reference sets it)')
        self.lr_sr, self.hr_sr = lr_sr, hr_sr
        self.with_path = with_path
        self.upsample = upsample
        with open(os.path.join(json_dir, 'lr.json')) as f:
            lr = json.load(f)
        with open(os.path.join(json_dir, 'hr.json')) as f:
            hr = json.load(f)
        lr_stride = int(stride * lr_sr) if stride else None
        hr_stride = int(stride * hr_sr) if stride else None
        lr_length = int(segment * lr_sr) if segment else None
        hr_length = int(segment * hr_sr) if segment else None
        lr.sort()                                                # match_files (datasets.py:24-31)
        hr.sort()
        self.lr_set = Audioset(lr, sample_rate=lr_sr, length=lr_length, stride=lr_stride, pad=pad, channels=1, with_path=with_path)
        self.hr_set = Audioset(hr, sample_rate=hr_sr, length=hr_length, stride=hr_stride, pad=pad, channels=1, with_path=with_path)
        assert len(self.hr_set) == len(self.lr_set)
        # stricter than the reference, which compares the totals only: two files whose counts differ in opposite directions would leave
        # every later index pairing an lr segment with the hr segment of another file or another position
        for (lf, _), (hf, _), nl, nh in zip(lr, hr, self.lr_set.num_examples, self.hr_set.num_examples):
            if nl != nh:
                raise ValueError(f'{lf} gives {nl} segments but {hf} gives {nh}: the lr and hr lists do not describe the same recordings')

    def __getitem__(self, index):
        if self.with_path:
            hr_sig, hr_path = self.hr_set[index]
            lr_sig, lr_path = self.lr_set[index]
        else:
            hr_sig = self.hr_set[index]
            lr_sig = self.lr_set[index]
        if self.upsample:
            lr_sig = audio_io.resample(lr_sig, self.lr_sr, self.hr_sr)
            lr_sig = match_signal(lr_sig, hr_sig.shape[-1])
        if self.with_path:
            return (lr_sig, lr_path), (hr_sig, hr_path)
        return lr_sig, hr_sig

    def __len__(self):
        return len(self.lr_set)


class EpochSampler:
    """The indices of `DistributedSampler(dataset, num_replicas=world_size, rank=rank, shuffle=shuffle, seed=seed)` after
    `set_epoch(epoch)`, drop_last=False: a permutation drawn from a generator seeded with seed + epoch, padded to a multiple of the world
    size by repeating its head, of which the rank takes every world_size-th from its own position.

    The reference only assigns `loader.epoch` (solver.py:283), which never reaches the sampler: it draws the SAME order every epoch.
    Here the epoch does reach the sampler, so every epoch is a different permutation."""

    def __init__(self, n, world_size=1, rank=0, shuffle=True, seed=0, epoch=0):
        if not 0 <= rank < world_size:
            raise ValueError(f'rank {rank} outside [0, {world_size})')
        self.n, self.world_size, self.rank, self.shuffle, self.seed, self.epoch = n, world_size, rank, shuffle, seed, epoch
        self.num_samples = math.ceil(n / world_size)
        self.total_size = self.num_samples * world_size

    def set_epoch(self, epoch):
        self.epoch = epoch

    def indices(self):
        if self.shuffle:
            g = torch.Generator()
            g.manual_seed(self.seed + self.epoch)
            idx = torch.randperm(self.n, generator=g).tolist()
        else:
            idx = list(range(self.n))
        pad = self.total_size - len(idx)
        if pad <= len(idx):
            idx += idx[:pad]
        else:
            idx += (idx * math.ceil(pad / len(idx)))[:pad]
        return idx[self.rank:self.total_size:self.world_size]

    def __iter__(self):
        return iter(self.indices())

    def __len__(self):
        return self.num_samples


def _ptr(t):
    return None if t is None else t.data_ptr()


def segment_gather(lib, arena, file_off, file_len, item_file, item_start, L, out=None):
    """aero_segment_gather on the current stream: arena int16 / fp32 [n], tables on the arena's device -> fp32 [B, L]"""
    B = item_file.numel()
    if out is None:
        out = torch.empty(B, L, dtype=torch.float32, device=arena.device)
    stream = torch.cuda.current_stream(arena.device).cuda_stream if arena.is_cuda else 0
    lib.call('aero_segment_gather', _ptr(arena), int(arena.dtype == torch.float32), _ptr(file_off), _ptr(file_len), file_off.numel(),
             _ptr(item_file), _ptr(item_start), B, L, _ptr(out), stream)
    return out


class _Side:
    """one side's arena: the samples of its files back to back, and where each file lies"""

    def __init__(self, audioset, raw, device):
        f32 = any(a.dtype != np.int16 for a in raw)
        self.dtype = torch.float32 if f32 else torch.int16
        lens = [len(a) for a in raw]
        offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64) if raw else np.zeros(0, np.int64)
        self.arena = torch.empty(max(1, sum(lens)), dtype=self.dtype, device=device)
        for o, a in zip(offs, raw):
            if f32 and a.dtype == np.int16:
                a = a.astype(np.float32) / 32768.0
            if len(a):
                self.arena[int(o):int(o) + len(a)].copy_(torch.from_numpy(np.array(a)))
        self.file_off = torch.from_numpy(offs).to(device)
        self.file_len = torch.tensor(lens, dtype=torch.int64).to(device)
        self.lens = lens
        self.set = audioset


class DeviceLrHrStore:
    """`LrHrSet` with every file decoded once and resident on `device`.  `DeviceLrHrStore(lr_hr_set, device, max_bytes)` is None when
    the two arenas would take more than `max_bytes` (the caller then reads `lr_hr_set` through distrib.loader)."""

    def __new__(cls, lr_hr_set, device='cuda', max_bytes=DEFAULT_MAX_BYTES, lib=None):
        need = 0
        for s in (lr_hr_set.lr_set, lr_hr_set.hr_set):
            enc = [audio_io.encoding(str(f)) for f, _ in s.files]
            size = 2 if all(e == 'pcm16' for e in enc) else 4
            need += size * sum(audio_io.info(str(f))[0] for f, _ in s.files)
        if need > max_bytes:
            return None
        self = super().__new__(cls)
        self.nbytes = need
        return self

    def __init__(self, lr_hr_set, device='cuda', max_bytes=DEFAULT_MAX_BYTES, lib=None):
        from . import _lib
        self.set = lr_hr_set
        self.device = torch.device(device)
        self.lib = lib or _lib.load()
        self.sides = []
        for s in (lr_hr_set.lr_set, lr_hr_set.hr_set):
            raw = []
            for f, _ in s.files:
                a, sr = audio_io.load_raw(str(f))
                s.check(f, sr, a.shape[1])
                raw.append(a[:, 0])
            self.sides.append(_Side(s, raw, self.device))
        self.table = None
        if lr_hr_set.upsample and lr_hr_set.lr_sr != lr_hr_set.hr_sr:
            from .seanet import resample_table
            t, og, nw, width = resample_table(lr_hr_set.lr_sr, lr_hr_set.hr_sr)
            self.table = (t.to(self.device), og, nw, width)

    def __len__(self):
        return len(self.set)

    def _items(self, side, indices):
        """-> (file per item, start per item, L): `length=None` items are whole files, so they must all be equally long"""
        loc = [side.set.locate(int(i)) for i in indices]
        files = [f for f, _, _ in loc]
        Ls = {n or side.lens[f] for f, _, n in loc}
        if len(Ls) != 1:
            raise ValueError(f'whole-file items of different lengths {sorted(Ls)} do not stack into a batch')
        return files, [o for _, o, _ in loc], Ls.pop()

    def batch(self, indices):
        """-> (lr [B, 1, Llr], hr [B, 1, Lhr]) fp32 on the device, equal to the stacked `LrHrSet` items of `indices`"""
        lo, hi = self.sides
        lf, ls, Llr = self._items(lo, indices)
        hf, hs, Lhr = self._items(hi, indices)
        files = torch.tensor([lf, hf], dtype=torch.int32).to(self.device)
        starts = torch.tensor([ls, hs], dtype=torch.int64).to(self.device)
        hr = segment_gather(self.lib, hi.arena, hi.file_off, hi.file_len, files[1], starts[1], Lhr)
        lr = segment_gather(self.lib, lo.arena, lo.file_off, lo.file_len, files[0], starts[0], Llr)
        if self.set.upsample:
            lr = self._upsample(lr, Lhr)
        return lr.unsqueeze(1), hr.unsqueeze(1)

    def _upsample(self, lr, Lhr):
        """audio_io.resample of the cut and padded segments, then match_signal to the hr length (datasets.py:143-145): the front-end
        resampler of the Seanet path (aero_seanet_front, no normalisation) on rows that hold nothing but the segment, so taps outside
        it are zero whatever the file holds there; its zero fill / early stop is match_signal"""
        if self.table is None:                                   # equal rates: resample is the identity
            return match_signal(lr, Lhr)
        table, og, nw, width = self.table
        B, L = lr.shape
        Lup = min(-((-nw * L) // og), Lhr)
        out = torch.empty(B, Lhr, dtype=torch.float32, device=lr.device)
        stream = torch.cuda.current_stream(lr.device).cuda_stream if lr.is_cuda else 0
        self.lib.call('aero_seanet_front', _ptr(lr), None, _ptr(table), _ptr(out), B, L, Lup, Lhr, og, nw, width, stream)
        return out


def host_batch(lr_hr_set, indices, device):
    """the same batch through the host reader: what a DataLoader's default collate makes of the items"""
    items = [lr_hr_set[int(i)] for i in indices]
    return torch.stack([a for a, _ in items]).to(device), torch.stack([b for _, b in items]).to(device)


def serialize(models, optimizers, history, best_states, args):
    """model_serializer.py:19-63: the package `enhance.load_generator` (and the reference's predict.py / test.py) read, written to
    `<checkpoint_file>.tmp` and renamed into place; then, for every entry of `best_states` ({model name: state dict}), that model's
    package with the best state in it as `<model>_<best_file's name>` next to `best_file`, the same way.  Without best states nothing
    but the checkpoint is written."""
    package = {
        'models': {name: {'class': m.__class__, 'args': m._init_args_kwargs[0], 'kwargs': m._init_args_kwargs[1],
                          'state': {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}} for name, m in models.items()},
        'optimizers': {name: o.state_dict() for name, o in optimizers.items()},
        'history': history,
        'best_states': best_states,
        'args': args,
    }
    # (beyond the reference's keys) the training engines' host-side state, without which a resumed run is not the interrupted one
    engines = {name: m.train_state() for name, m in models.items() if hasattr(m, 'train_state')}
    if any(v is not None for v in engines.values()):
        package['engines'] = engines
    path = str(args.checkpoint_file)
    torch.save(package, path + '.tmp')
    os.rename(path + '.tmp', path)
    best_file = str(args.best_file) if best_states else ''
    for name, state in best_states.items():
        best = os.path.join(os.path.dirname(best_file), name + '_' + os.path.basename(best_file))
        torch.save(dict(package['models'][name], state=state), best + '.tmp')
        os.rename(best + '.tmp', best)
    return package
