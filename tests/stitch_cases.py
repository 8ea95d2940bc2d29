"""Shared by tests/test_stitch.py (CPU, emulator library) and tests/test_gpu_stitch.py (MI355X): aero_overlap_stitch and aero_wav_finalize
(csrc/k_stitch.h) against a host restatement of the stitch, and enhance.predict_signal(overlap > 0) against the host stitch of the same
forwards.  Each check takes the library and a device."""
import math

import torch

from aero_amd import enhance
from conftest import build_model, rel_l2, seeded

LY = 64                                   # chunk output length of the kernel cases: hop = LY - V
KERNEL_V = (1, 3, 16, 32)                 # hop 63, 61 (odd: every vector path misaligned), 48, 32
KERNEL_N = (1, 2, 3, 5)
KERNEL_GROUP = (1, 2)
SENTINEL = -77.25
EPS = 2.0 ** -24


def emu_lib():
    from aero_amd import _lib
    from emu.build_emu import build
    return _lib.load(build())


def host_stitch(ys, hop, V, fade):
    """DESIGN.md 4.8 restated on the host: ys = the chunk outputs [ch, len_k] in order, fade fp32 [V] ->
    (out fp32 as p + fade (c - p) evaluates in fp32, the same in fp64 on the same fp32 operands, the bound 4 * 2^-24 (|p| + |c|), the fade mask)"""
    n = len(ys)
    N_out = (n - 1) * hop + ys[-1].shape[-1]
    out = torch.empty(ys[0].shape[0], N_out)
    exact, bound, mask = out.double(), torch.zeros_like(out, dtype=torch.float64), torch.zeros(N_out, dtype=torch.bool)
    for k, y in enumerate(ys):
        end = y.shape[-1] if k == n - 1 else hop                 # k = min(t // hop, n - 1), j = t - k hop
        out[:, k * hop:k * hop + end] = y[:, :end]
        exact[:, k * hop:k * hop + end] = y[:, :end].double()
        v = min(V, end) if k >= 1 else 0
        if v:
            p, c, f = ys[k - 1][:, hop:hop + v], y[:, :v], fade[:v]
            out[:, k * hop:k * hop + v] = p + f * (c - p)
            exact[:, k * hop:k * hop + v] = p.double() + f.double() * (c.double() - p.double())
            bound[:, k * hop:k * hop + v] = 4 * EPS * (p.abs().double() + c.abs().double())
            mask[k * hop:k * hop + v] = True
    return out, exact, bound, mask


def assert_stitched(got, ys, hop, V, fade, what=''):
    """bit-equal outside the fades; inside, every sample within 4 * 2^-24 (|p| + |c|) of the fp64 evaluation on the same fp32 table"""
    ref, exact, bound, mask = host_stitch(ys, hop, V, fade)
    assert got.shape == ref.shape and got.dtype == torch.float32, (what, got.shape, ref.shape)
    assert torch.equal(got[:, ~mask], ref[:, ~mask]), what
    diff = (got.double() - exact).abs()[:, mask]
    if mask.any():
        worst = float((diff / bound[:, mask].clamp_min(1e-300)).max())
        print(f'{what}: {int(mask.sum())} fade samples per channel, worst |diff| / bound {worst:.3f}')
    assert bool((diff <= bound[:, mask]).all()), what


def run_stitch(lib, device, ys, hop, V, group):
    """the launches predict_signal issues for these chunk outputs: the equal-length chunks in groups of `group`, a short last chunk on its
    own.  `out` starts as sentinels; after every launch everything outside the ranges written so far must still hold them.
    -> (out [ch, N_out], peak_bits) on the host"""
    n, ch = len(ys), ys[0].shape[0]
    N_out = (n - 1) * hop + ys[-1].shape[-1]
    fade = enhance.fade_table(max(V, 1)).to(device)              # (V = 0: never read, but no null pointer)
    buf =torch.full((3 + ch * N_out + 5,), SENTINEL, device=device)       # (3: the rows start off a 16-byte boundary)
    out = buf[3:3 + ch * N_out].view(ch, N_out)
    peak = torch.zeros(1, dtype=torch.int32, device=device)
    n_full = n if ys[-1].shape[-1] == LY else n - 1
    jobs = [(k0, min(group, n_full - k0)) for k0 in range(0, n_full, group)] + ([(n - 1, 1)] if n_full < n else [])
    prev = None
    for k0, g in jobs:
        y = torch.stack(ys[k0:k0 + g]).to(device)
        last = k0 + g == n
        enhance.overlap_stitch(lib, y, prev, fade, V, hop, k0, last, out, peak)
        prev = y[g - 1]
        done = N_out if last else (k0 + g) * hop
        host = buf.cpu()
        assert bool((host[:3] == SENTINEL).all()) and bool((host[3 + ch * N_out:] == SENTINEL).all()), 'wrote outside out'
        assert bool((host[3:3 + ch * N_out].view(ch, N_out)[:, done:] == SENTINEL).all()), f'launch k0={k0} g={g} wrote behind its range'
    return out.cpu(), peak.cpu()


def kernel_chunks(ch, V, n, last_len, seed):
    return [seeded((ch, LY if k < n - 1 else last_len), seed + k) for k in range(n)]


def check_kernel(lib, device, ch, V):
    """every n, grouping and last-chunk length for one (ch, V)"""
    hop = LY - V
    fade = enhance.fade_table(V)
    assert torch.allclose(fade + fade.flip(0), torch.ones(V), atol=2 * EPS, rtol=0)
    for n in KERNEL_N:
        for group in KERNEL_GROUP:
            for last_len in sorted({V + 1, V + 2, 37, LY}):
                ys = kernel_chunks(ch, V, n, last_len, 1000 * V + 10 * n + ch)
                out, peak = run_stitch(lib, device, ys, hop, V, group)
                assert bool((out != SENTINEL).all())
                assert_stitched(out, ys, hop, V, fade, f'ch={ch} V={V} n={n} group={group} last={last_len}')
                assert int(peak) == int(out.abs().max().view(torch.int32)), 'peak_bits is not the fp32 bits of max |out|'


def check_agreeing_chunks(lib, device, ch, V):
    """chunks cut out of ONE signal agree wherever they overlap (c == p): the output is that signal bit for bit"""
    hop = LY - V
    for n, last_len in ((2, V + 1), (3, 37), (5, LY)):
        sig = seeded((ch, (n - 1) * hop + last_len), 50 + n)
        ys = [sig[:, k * hop:k * hop + (LY if k < n - 1 else last_len)].contiguous() for k in range(n)]
        out, _ = run_stitch(lib, device, ys, hop, V, 2)
        assert torch.equal(out, sig), (ch, V, n)


def check_finalize(lib, device, ch, peak_target, tmp):
    """aero_wav_finalize == (out / max(peak, 1)).T on the host, and write_device's file == write's, byte for byte"""
    x = seeded((ch, 203), 7 + ch)
    x = x / x.abs().max() * peak_target
    out, peak = run_stitch(lib, device, [x], LY, 0, 1)           # one chunk: a copy, and the peak
    assert torch.equal(out, x)
    pk = float(peak.view(torch.float32))
    assert pk == float(x.abs().max()) and abs(pk - peak_target) < 1e-5 * peak_target
    wav = enhance.wav_finalize(lib, x.to(device), peak.to(device)).cpu()
    ref = (x / max(x.abs().max().item(), 1)).T.contiguous()
    assert wav.shape == (203, ch) and torch.equal(wav, ref)
    a, b = str(tmp / f'host{ch}.wav'), str(tmp / f'dev{ch}.wav')
    enhance.write(x, a, 16000)
    enhance.write_device(x.to(device), peak.to(device), b, 16000, lib=lib)
    assert open(a, 'rb').read() == open(b, 'rb').read()


# ------------------------------------------------------------------ end to end: the tiny model, 10 "seconds" = 400 samples
SR, OVERLAP = 40, 40
E2E_SAMPLES = 2 * 360 + 400 + 123


def tiny_model(meta, lib=None, device='cpu'):
    from aero_amd.engine import HipEngine
    m = build_model(meta, 'tiny')
    if lib is not None:
        object.__setattr__(m, '_engine', HipEngine(m, lib=lib))
    return m.to(device)


def e2e_signal(ch, seed=8):
    return seeded((ch, E2E_SAMPLES), seed)


def chunk_forwards(model, sig, ranges, device):
    """the per-chunk forwards of the reference loop: model(sig[:, a:b]) with the channels as the batch"""
    with torch.no_grad():
        return [model(sig[:, a:b].unsqueeze(1).to(device)).squeeze(1).cpu() for a, b in ranges]


def check_e2e_per_chunk(model, device, ch, bit_exact):
    """predict_signal(overlap) against the host stitch of the per-chunk forwards: bit-equal outside the fades and within the bound inside
    them where a batched forward is bit-equal to single ones (the emulator); rel-L2 < 1e-5 otherwise (the bar of batched against single)"""
    sig = e2e_signal(ch)
    ranges = enhance.overlap_ranges(E2E_SAMPLES, SR, OVERLAP)
    assert ranges == [(0, 400), (360, 760), (720, 1120), (1080, 1243)]
    hop, V = enhance.output_hop(SR, OVERLAP, 4)
    assert (hop, V) == (1440, 160)
    pr = enhance.predict_signal(model, sig, SR, device=device, overlap=OVERLAP, max_clips=2 * ch)     # full chunks in groups of 2 + 1
    assert pr.shape == (ch, 3 * hop + 4 * 163) and pr.device.type == 'cpu'
    ys = chunk_forwards(model, sig, ranges, device)
    if bit_exact:
        assert_stitched(pr, ys, hop, V, enhance.fade_table(V), f'e2e ch={ch}')
    else:
        e = rel_l2(pr, host_stitch(ys, hop, V, enhance.fade_table(V))[0])
        print(f'e2e ch={ch}: rel-L2 against the stitched per-chunk forwards {e:.3e}')
        assert e < 1e-5
    return pr


def check_e2e_grouped(model, device, ch):
    """on the device: predict_signal(overlap) against the host stitch of the SAME grouped forwards (full chunks in groups of 2 and 1, the
    short last chunk alone, each through BatchPipeline as predict_signal runs them) -- bit-equal outside the fades, the bound inside"""
    from aero_amd.pipeline import BatchPipeline
    sig = e2e_signal(ch)
    ranges = enhance.overlap_ranges(E2E_SAMPLES, SR, OVERLAP)
    hop, V = enhance.output_hop(SR, OVERLAP, 4)
    pr = enhance.predict_signal(model, sig, SR, device=device, overlap=OVERLAP, max_clips=2 * ch)
    pipe = BatchPipeline(model, depth=enhance.PIPELINE_DEPTH)
    ys = []
    with torch.no_grad():
        for grp in (ranges[0:2], ranges[2:3], ranges[3:4]):
            x = torch.stack([sig[:, a:b] for a, b in grp]).reshape(len(grp) * ch, 1, -1).to(device)
            ys += list(pipe.result(pipe.submit(x)).reshape(len(grp), ch, -1).cpu())
        pipe.drain()
    assert_stitched(pr, ys, hop, V, enhance.fade_table(V), f'e2e grouped ch={ch}')
    return pr


def check_refusals(lib):
    """every refusal of the two entry points: a negative code and a message naming the entry point -- no launch"""
    y, prev, fade, out = torch.zeros(2, 64), torch.zeros(1, 64), torch.zeros(16), torch.zeros(1, 112)
    peak = torch.zeros(1, dtype=torch.int32)
    # y, Ly, prev, Lprev, fade, V, hop, k0, g, ch, last, out, N_out, peak_bits, stream
    ok0 = [y.data_ptr(), 64, None, 0, fade.data_ptr(), 16, 48, 0, 2, 1, 1, out.data_ptr(), 112, peak.data_ptr(), None]
    ok1 = [y.data_ptr(), 64, prev.data_ptr(), 64, fade.data_ptr(), 16, 48, 1, 1, 1, 1, out.data_ptr(), 112, peak.data_ptr(), None]
    bad = [(ok0, {0: None}), (ok0, {4: None}), (ok0, {11: None}), (ok0, {13: None}),                 # a null pointer
           (ok0, {5: 40, 6: 24}),                                                                    # V > hop
           (ok0, {1: 63}), (ok0, {1: 63, 8: 1, 10: 0, 12: 1000}),                                    # a non-last chunk with Ly < hop + V
           (ok1, {3: 63}),                                                                           # prev with Lprev < hop + V
           (ok1, {2: None}), (ok0, {2: prev.data_ptr(), 3: 64}),                                     # prev null with k0 > 0, and the reverse
           (ok0, {12: 111}), (ok1, {7: 2}), (ok0, {10: 0, 12: 95}),                                  # a written range outside [0, N_out)
           (ok0, {0: y.data_ptr() + 2}), (ok0, {11: out.data_ptr() + 1}), (ok0, {4: fade.data_ptr() + 2}),
           (ok1, {2: prev.data_ptr() + 2}), (ok0, {13: peak.data_ptr() + 1})]                        # a pointer off 4 bytes
    for base, change in bad:
        args = list(base)
        for pos, val in change.items():
            args[pos] = val
        rc = lib.cdll.aero_overlap_stitch(*args)
        assert rc < 0 and b'aero_overlap_stitch' in lib.cdll.aero_last_error(), change
    wav = torch.zeros(112)
    okf = [out.data_ptr(), peak.data_ptr(), 1, 112, wav.data_ptr(), None]
    for change in ({0: None}, {1: None}, {4: None}, {2: 0}, {3: 0}, {0: out.data_ptr() + 2}, {4: wav.data_ptr() + 1}, {1: peak.data_ptr() + 2}):
        args = list(okf)
        for pos, val in change.items():
            args[pos] = val
        rc = lib.cdll.aero_wav_finalize(*args)
        assert rc < 0 and b'aero_wav_finalize' in lib.cdll.aero_last_error(), change
    return ok0, ok1, okf


def fade_bound_on_the_host(rows=10000):
    """the fp32 restatement p + f (c - p) against fp64 over `rows` random rows: the worst |diff| / (2^-24 (|p| + |c|)); the kernel's bound is
    4 (three roundings give at most 3), an FMA contraction only lowers it"""
    g = torch.Generator().manual_seed(1)
    p, c = torch.randn(rows, 64, generator=g), torch.randn(rows, 64, generator=g)
    f = enhance.fade_table(64)
    got = p + f * (c - p)
    exact = p.double() + f.double() * (c.double() - p.double())
    return float(((got.double() - exact).abs() / (EPS * (p.abs() + c.abs()).double())).max())


def n_chunks_by_the_rule(N, L, ov):
    return 1 if N <= L else math.ceil((N - ov) / (L - ov))
