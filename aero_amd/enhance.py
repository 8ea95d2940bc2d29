"""Inference helpers mirroring the reference's src/enhance.py and predict.py (host plumbing around Aero.forward)."""
import math
import os
from fractions import Fraction

import torch

from . import audio_io

SEGMENT_DURATION_SEC = 10            # predict.py:22


def chunk_ranges(n_samples, sr, segment_sec=SEGMENT_DURATION_SEC):
    """predict.py:61-69: independent [start, end) chunks of `segment_sec` seconds, last one short (integer-exact)."""
    seg = sr * segment_sec
    n_chunks = math.ceil(n_samples / seg)
    return [(i * seg, min((i + 1) * seg, n_samples)) for i in range(n_chunks)]


def get_estimate(model, lr_sig):
    """enhance.py:11-15."""
    with torch.no_grad():
        return model(lr_sig)


MAX_CLIPS_PER_FORWARD = 64         # bound on chunk-channels per forward: activation memory stays constant for any file length


PIPELINE_DEPTH = 3                 # forwards in flight on separate HIP streams (aero_amd/pipeline.py)


def _forward_groups(model, groups, device):
    """Run the [n_i, 1, L] host batches of `groups` through the model, one forward each.  On the GPU up to PIPELINE_DEPTH groups are in
    flight, each on its own HIP stream (BatchPipeline): a group's pinned upload, its kernels and its pinned download are ordered on that
    stream and run next to the kernels and copies of the neighbouring groups (predict.py:76-80 moves one chunk at a time, synchronously)."""
    dev = torch.device(device)
    # the pipelined loop needs the generator itself (its engine, eval mode); anything else that is callable -- a distrib.wrap()'ed model, a
    # model left in training mode, a reference-style nn.Module -- takes the plain loop the reference runs (predict.py:76-80)
    core = getattr(model, 'module', model)
    if dev.type != 'cuda' or len(groups) == 0 or not hasattr(core, '_get_engine') or getattr(core, 'training', False):
        return [model(g.to(dev)).cpu() for g in groups]
    try:
        depth = max(1, int(os.environ.get('AERO_PIPELINE', PIPELINE_DEPTH)))
    except ValueError:                                   # (a malformed AERO_PIPELINE must not take the serving path down)
        depth = PIPELINE_DEPTH
    from .pipeline import BatchPipeline
    pipe = BatchPipeline(core, depth=depth)
    return pipe.run(groups, to_host=True)


DEFAULT_MAX_BYTES = 8 << 30         # the resident input and output of one overlapped file: the machines are shared


def overlap_ranges(n_samples, sr, overlap, segment_sec=SEGMENT_DURATION_SEC):
    """chunks of `segment_sec` seconds that share `overlap` input samples with their neighbours: chunk k is [k H, min(k H + L, N)) with the
    hop H = L - overlap, n = 1 if N <= L else ceil((N - overlap) / H) of them (integer-exact).  overlap = 0 is `chunk_ranges`; for n >= 2
    the last chunk is longer than the overlap."""
    L = sr * segment_sec
    overlap = int(overlap)
    if not 0 <= overlap <= L // 2:
        raise ValueError(f'overlap = {overlap} samples: 0 <= overlap <= {L // 2} (half a chunk) is required')
    H = L - overlap
    if n_samples <= 0:
        return []
    n = 1 if n_samples <= L else -((overlap - n_samples) // H)
    return [(k * H, min(k * H + L, n_samples)) for k in range(n)]


def output_hop(sr, overlap, scale, segment_sec=SEGMENT_DURATION_SEC):
    """-> (hop, V): the hop and the overlap in OUTPUT samples, `scale` = hr_sr / lr_sr as a Fraction; both must be whole numbers"""
    H = sr * segment_sec - int(overlap)
    hop, V = H * Fraction(scale), int(overlap) * Fraction(scale)
    if hop.denominator != 1 or V.denominator != 1:
        raise ValueError(f'hop {H} and overlap {int(overlap)} input samples are {float(hop)} and {float(V)} output samples at the rate ratio {scale}: '
                         f'choose an overlap that makes both whole')
    return int(hop), int(V)


def fade_table(V):
    """fade[j] = sin^2(pi (j + 1/2) / (2 V)) in fp64, rounded to fp32: the weight of the LATER chunk; fade[j] + fade[V - 1 - j] = 1"""
    j = torch.arange(V, dtype=torch.float64)
    return (torch.sin(math.pi * (j + 0.5) / (2 * max(V, 1))) ** 2).to(torch.float32)


def _rate_ratio(core):
    """output samples per input sample of a generator, as a Fraction"""
    if hasattr(core, 'spec_upsample'):                           # Aero (modules.py: self.scale)
        return Fraction(int(core.hr_sr), int(core.lr_sr)) if core.spec_upsample else Fraction(1)
    if hasattr(core, 'scale_factor') and hasattr(core, 'upsample'):        # Seanet (seanet.py: target_len)
        return Fraction(int(core.scale_factor)) if core.upsample else Fraction(1)
    if hasattr(core, 'lr_sr') and hasattr(core, 'hr_sr'):
        return Fraction(int(core.hr_sr), int(core.lr_sr))
    raise ValueError('predict_signal(overlap > 0): the model has no lr_sr / hr_sr to place its chunk outputs by')


def _library(core):
    """the kernel library the model itself runs on (tests: the emulated one)"""
    if hasattr(core, '_get_engine'):
        return core._get_engine().lib
    if hasattr(core, '_get_ops'):
        return core._get_ops().lib
    from . import _lib
    return _lib.load()


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream if t.is_cuda else 0


def overlap_stitch(lib, y, prev, fade, V, hop, k0, last, out, peak_bits):
    """aero_overlap_stitch on the current stream: y [g, ch, Ly] = chunks k0 .. k0 + g - 1 as one forward returns them, prev [ch, Lprev] = chunk
    k0 - 1 (None for k0 = 0) -> [k0 hop, (k0 + g) hop) of out [ch, N_out] (to the end of the last chunk with `last`), peak_bits raised"""
    g, ch, Ly = y.shape
    lib.call('aero_overlap_stitch', y.data_ptr(), Ly, None if prev is None else prev.data_ptr(), 0 if prev is None else prev.shape[-1],
             fade.data_ptr(), V, hop, k0, g, ch, int(bool(last)), out.data_ptr(), out.shape[-1], peak_bits.data_ptr(), _stream(out))


def _predict_overlapped(model, lr_sig, sr, device, overlap, per, max_bytes, return_device):
    """predict_signal with overlapped chunks, stitched on the device: one upload (the file as an arena of one "file" per channel, PCM16 as
    stored or fp32), per group one aero_segment_gather, one forward and one aero_overlap_stitch, one download."""
    from .data import segment_gather
    core = getattr(model, 'module', model)
    dev = torch.device(device)
    ch, N = lr_sig.shape
    L = sr * SEGMENT_DURATION_SEC
    ranges = overlap_ranges(N, sr, overlap)
    ratio = _rate_ratio(core)
    hop, V = output_hop(sr, overlap, ratio)
    if not ranges:
        raise ValueError('predict_signal: an empty signal')
    n, H = len(ranges), L - int(overlap)
    last_in = ranges[-1][1] - ranges[-1][0]
    Ly_last = hop + V if last_in == L else int(last_in * (ratio.numerator / ratio.denominator))        # aero.py:513
    N_out = (n - 1) * hop + Ly_last
    if lr_sig.dtype not in (torch.int16, torch.float32):
        lr_sig = lr_sig.float()
    need = lr_sig.numel() * lr_sig.element_size() + 4 * ch * N_out
    if need > max_bytes:
        raise ValueError(f'predict_signal: the resident input and output of this file take {need} bytes, more than max_bytes = {max_bytes}')
    lib = _library(core)
    if dev.type != 'cuda' and not lib.is_emulator:
        raise RuntimeError('predict_signal(overlap > 0) stitches on the MI355X: pass device="cuda"')
    # every table the launches need, uploaded with the file: nothing but launches until the download
    arena = lr_sig.contiguous().reshape(-1).to(dev)
    file_off = (torch.arange(ch, dtype=torch.int64) * N).to(dev)
    file_len = torch.full((ch,), N, dtype=torch.int64).to(dev)
    item_file = torch.arange(ch, dtype=torch.int32).repeat(n).to(dev)
    item_start = (torch.arange(n, dtype=torch.int64) * H).repeat_interleave(ch).to(dev)
    fade = fade_table(max(V, 1)).to(dev)
    out = torch.empty(ch, N_out, dtype=torch.float32, device=dev)
    peak_bits = torch.zeros(1, dtype=torch.int32, device=dev)
    n_full = n if last_in == L else n - 1
    jobs = [(k0, min(per, n_full - k0), L) for k0 in range(0, n_full, per)]
    if n_full < n:
        jobs.append((n - 1, 1, last_in))                         # the short last chunk: its own forward, its own stitch
    state = {'prev': None}

    def gather(k0, g, Lin):
        rows = slice(k0 * ch, (k0 + g) * ch)
        return segment_gather(lib, arena, file_off, file_len, item_file[rows], item_start[rows], Lin).unsqueeze(1)

    def stitch(y, k0, g, Lin):
        want = hop + V if Lin == L else Ly_last
        if y.shape[0] != g * ch or y.shape[-1] != want:
            raise RuntimeError(f'predict_signal: the forward of {g} chunk(s) of {Lin} samples returned {tuple(y.shape)}, expected {want} samples each')
        y = y.reshape(g, ch, want).float().contiguous()
        overlap_stitch(lib, y, state['prev'], fade, V, hop, k0, k0 + g == n, out, peak_bits)
        state['prev'] = y[g - 1]                                 # kept alive as the next group's prev

    pipelined = dev.type == 'cuda' and hasattr(core, '_get_engine') and not getattr(core, 'training', False)
    with torch.no_grad():
        if pipelined:
            try:
                depth = max(1, int(os.environ.get('AERO_PIPELINE', PIPELINE_DEPTH)))
            except ValueError:
                depth = PIPELINE_DEPTH
            from .pipeline import BatchPipeline
            pipe = BatchPipeline(core, depth=depth)
            pending = []                                         # (not pipe.run: at most depth + 1 group outputs are alive)
            for job in jobs:
                pending.append((pipe.submit(gather(*job)), job))
                if len(pending) > depth:
                    t, j = pending.pop(0)
                    stitch(pipe.result(t), *j)                   # on the caller's stream, behind the batch
            for t, j in pending:
                stitch(pipe.result(t), *j)
        else:
            for job in jobs:
                stitch(model(gather(*job)), *job)
    if return_device:
        return out, peak_bits
    return out.cpu()


def predict_signal(model, lr_sig, sr, device=None, batch_chunks=True, max_clips=MAX_CLIPS_PER_FORWARD, overlap=0, return_device=False,
                   max_bytes=DEFAULT_MAX_BYTES):
    """predict.py:61-85 for one file: lr_sig [channels, samples] -> [channels, samples*scale].

    The full-length chunks are independent (predict.py:76-80 loops over them): they are batched, at most `max_clips`
    chunk-channels per forward (bounded activation memory whatever the file length), with host<->device copies
    overlapped with compute; the short tail chunk is run separately.  Results are identical per chunk.

    overlap > 0 (input samples, at most half a chunk): neighbouring chunks share `overlap` samples and their outputs are cross-faded on
    the device (csrc/k_stitch.h) -- the file is uploaded once (fp32, or int16 PCM as stored), the result downloaded once,
    or with `return_device` left there as (out [channels, N_out], peak_bits: one int32 holding the fp32 bits of max |out|) for
    `write_device`.  Input and output together must fit `max_bytes`.  overlap = 0 without `return_device` is the path above, unchanged.
    """
    device = device or next(model.parameters()).device
    if overlap or return_device:
        model.eval()
        per = max(1, max_clips // lr_sig.shape[0]) if batch_chunks else 1
        return _predict_overlapped(model, lr_sig, sr, device, overlap, per, max_bytes, return_device)
    ranges = chunk_ranges(lr_sig.shape[-1], sr)
    out = [None] * len(ranges)
    model.eval()
    ch = lr_sig.shape[0]
    with torch.no_grad():
        full = [i for i, (a, b) in enumerate(ranges) if b - a == sr * SEGMENT_DURATION_SEC]
        if batch_chunks and len(full) > 1:
            per = max(1, max_clips // ch)                                                     # chunks per forward
            idx_groups = [full[k:k + per] for k in range(0, len(full), per)]
            groups = [torch.stack([lr_sig[:, ranges[i][0]:ranges[i][1]] for i in g], 0).reshape(len(g) * ch, 1, -1)
                      for g in idx_groups]
            for g, y in zip(idx_groups, _forward_groups(model, groups, device)):
                y = y.reshape(len(g), ch, -1)
                for k, i in enumerate(g):
                    out[i] = y[k]
        for i, (a, b) in enumerate(ranges):
            if out[i] is None:
                out[i] = model(lr_sig[:, a:b].unsqueeze(1).to(device)).squeeze(1).cpu()
    return torch.cat(out, dim=-1)


def write(wav, filename, sr):
    """enhance.py:18-21: divide by max(|wav|max, 1) only if it prevents clipping, then save."""
    wav = wav / max(wav.abs().max().item(), 1)
    audio_io.save(filename, wav.cpu(), sr)


def write_device(out, peak_bits, filename, sr, lib=None):
    """`write` of a signal that is still on the device (predict_signal(..., return_device=True)): aero_wav_finalize divides by
    max(peak, 1) and interleaves, one download, the same file as `write` byte for byte.  (`lib`: tests pass the emulated library.)"""
    if lib is None:
        from . import _lib
        lib = _lib.load()
    if not out.is_cuda and not lib.is_emulator:
        raise RuntimeError('write_device takes the device result of predict_signal(..., return_device=True); use write() for a host tensor')
    audio_io.save_frames(filename, wav_finalize(lib, out, peak_bits).cpu(), sr)


def wav_finalize(lib, out, peak_bits):
    """aero_wav_finalize on the current stream: out [ch, N_out], peak_bits -> the file's payload [N_out, ch] = out.T / max(peak, 1)"""
    ch, n = out.shape
    out = out.contiguous()
    wav = torch.empty(n, ch, dtype=torch.float32, device=out.device)
    lib.call('aero_wav_finalize', out.data_ptr(), peak_bits.data_ptr(), ch, n, wav.data_ptr(), _stream(out))
    return wav


def save_wavs(processed_sigs, lr_sigs, hr_sigs, filenames, lr_sr, hr_sr):
    """enhance.py:24-29."""
    for lr, hr, pr, filename in zip(lr_sigs, hr_sigs, processed_sigs, filenames):
        write(lr, filename + '_lr.wav', sr=lr_sr)
        write(hr, filename + '_hr.wav', sr=hr_sr)
        write(pr, filename + '_pr.wav', sr=hr_sr)


def match_signal(signal, ref_len):
    """src/utils.py:211-217."""
    sig_len = signal.shape[-1]
    if sig_len < ref_len:
        signal = torch.nn.functional.pad(signal, (0, ref_len - sig_len))
    elif sig_len > ref_len:
        signal = signal[..., :ref_len]
    return signal


class _Inert:
    """Stand-in for classes a reference checkpoint pickles but the generator path never needs: the GAN critics
    (`src.models.discriminators.*`, every aero config trains with `adversarial: true`), the Seanet baseline and the
    omegaconf / hydra containers of the `args` entry (model_serializer.py:22,47).  Accepts any construction/state."""

    def __init__(self, *a, **k):
        pass

    def __call__(self, *a, **k):
        return _Inert()

    def __setstate__(self, state):
        self.__dict__['_state'] = state

    def __reduce_ex__(self, protocol):
        return (_Inert, ())


def _tolerant_pickle():
    """A `pickle_module` for torch.load whose Unpickler maps classes that cannot be imported here (or that live in the
    reference's training-only modules) to inert stubs instead of raising ModuleNotFoundError / AttributeError."""
    import importlib
    import pickle
    import types

    class Unpickler(pickle.Unpickler):
        def find_class(self, module, name):
            try:
                return super().find_class(module, name)
            except (ImportError, AttributeError):
                root = module.split('.')[0]
                if root in ('src', 'omegaconf', 'hydra', 'antlr4', 'wandb') or module.startswith('src.'):
                    return type(name, (_Inert,), {'__module__': module})
                raise

    mod = types.ModuleType('aero_amd_tolerant_pickle')
    mod.__dict__.update({k: getattr(pickle, k) for k in dir(pickle) if not k.startswith('__')})
    mod.Unpickler = Unpickler
    mod.load = lambda f, **kw: Unpickler(f, **kw).load()
    importlib.invalidate_caches()
    return mod


def load_package(path):
    """torch.load of a checkpoint written by the reference's serializer (model_serializer.py:40-54), tolerant of the
    pickled training-only classes."""
    return torch.load(str(path), map_location='cpu', weights_only=False, pickle_module=_tolerant_pickle())


def load_generator(args, device='cuda'):
    """predict.py:24-38 / test.py:25-39: build the generator from the experiment config and load a checkpoint written
    by the reference's serializer ({'models': {'generator': {'state': ...}}, 'best_states': ..., 'args': ...}).
    Like the reference (torch.load on a missing path raises), a configured but absent checkpoint is an error; random
    weights are only used when the caller says so (`+random_init=true`), e.g. for plumbing runs and benchmarks."""
    name = args.experiment.get('model', 'aero')                  # modelFactory.py:7-10
    if name == 'seanet':
        from .seanet import Seanet
        model = Seanet(**args.experiment.seanet)
    elif name == 'aero':
        from .modules import Aero
        model = Aero(**args.experiment.aero)
    else:
        raise NotImplementedError(f"model '{name}': the generators implemented on MI355X are aero and seanet")
    ckpt = args.get('checkpoint_file')
    if args.get('random_init'):
        return model.to(device).eval()
    if not ckpt or not os.path.exists(str(ckpt)):
        raise FileNotFoundError(f"checkpoint_file '{ckpt}' not found (pass +random_init=true to run with random-init weights)")
    package = load_package(ckpt)
    if args.get('continue_best'):
        best = package['best_states']
        state = best['models']['generator']['state'] if 'models' in best else best['generator']
    else:
        state = package['models']['generator']['state']
    model.load_state_dict(state)
    return model.to(device).eval()
