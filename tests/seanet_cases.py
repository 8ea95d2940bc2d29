"""Seanet baseline generator (aero_amd/seanet.py, csrc/k_seanet.h) against the REFERENCE's Seanet (tests/golden/seanet_io.npz /
seanet_meta.json from tools/make_golden_seanet.py) and against float64 restatements of the single kernels."""
import ctypes as C
import functools
import json
import os

import torch
import torch.nn.functional as F

from conftest import GOLDEN, load_npz, rel_l2

SLOPE = 0.2


@functools.lru_cache(maxsize=None)
def meta():
    return json.load(open(os.path.join(GOLDEN, 'seanet_meta.json')))


def emu_lib():
    from aero_amd import _lib
    from emu.build_emu import build
    return _lib.load(build())


def seeded_seanet(seed, **cfg):
    from aero_amd.seanet import Seanet
    torch.manual_seed(seed)
    return Seanet(**cfg)


def checksum_errors(ngf):
    """per key: max of the relative deviations of (sum, |sum|) from the reference's seeded state dict"""
    m = seeded_seanet(meta()['seeds'][str(ngf)], ngf=ngf, upsample=False)
    ref = meta()['checksums'][str(ngf)]
    assert set(m.state_dict()) == set(ref), set(m.state_dict()) ^ set(ref)
    out = {}
    for k, v in m.state_dict().items():
        s, a = ref[k]
        out[k] = max(abs(float(v.double().sum()) - s) / max(1.0, a), abs(float(v.double().abs().sum()) - a) / a)
    return out


def bar(floor):
    """the issue's tolerance: max(1e-3, 3 x the fp16-operand floor of the reference itself)"""
    return max(1e-3, 3.0 * floor)


def sub(fm):
    return fm[:, ::max(1, fm.shape[1] // 8), ::max(1, fm.shape[2] // 256)]


def case_errors(name, dev, emulator=False):
    """run golden case `name` -> {stage or 'out': (relative error, its bar)}; prints every figure"""
    case = meta()['cases'][name]
    io = load_npz('seanet_io.npz')
    model = seeded_seanet(case['seed'], **case['cfg']).eval()
    if emulator:
        model.use_library(emu_lib())
    model.to(dev)
    x = torch.from_numpy(io[f'{name}.x']).to(dev)
    with torch.no_grad():
        y, stages = model.forward_stages(x)
    assert list(y.shape) == case['out_shape'] and y.dtype == torch.float32
    n = len(model.encoder)
    named = {f'enc{i}': s for i, s in enumerate(stages[:n])}
    named.update({f'dec{j}': s for j, s in enumerate(stages[n:])})
    errs = {'out': (rel_l2(y.cpu(), io[f'{name}.y']), bar(case['fp16_floor']['out']))}
    for k in case['stages']:
        got = sub(named[k].float().cpu())
        ref = io[f'{name}.{k}']
        assert tuple(got.shape) == ref.shape, (k, got.shape, ref.shape)
        errs[k] = (rel_l2(got, ref), bar(case['fp16_floor'][k]))
    for k, (e, b) in errs.items():
        print(f'seanet case {name} {k}: rel-L2 {e:.3e} (bar {b:.2e}, fp16 floor {case["fp16_floor"][k]:.2e})')
    return errs


def check_case(errs):
    bad = {k: v for k, v in errs.items() if not v[0] <= v[1]}
    assert not bad, bad


# ------------------------------------------------------------------ single kernels against float64 restatements on fp16-exact operands
def f16(shape, seed, scale=1.0):
    """fp16-exact values as fp32"""
    return (scale * torch.randn(*shape, generator=torch.Generator().manual_seed(seed))).half().float()


def lrelu(x, slope=SLOPE):
    return torch.where(x > 0, x, x * slope)


def run_conv(lib, x, w, bias, *, stride=1, dil=1, pad=0, reflect=0, in_slope=1.0, act=0, add=None, transposed=False, opad=0):
    """aero_seanet_conv on x [B, Cin, T] (fp16-exact), w Conv1d [Cout, Cin, K] or ConvTranspose1d [Cin, Cout, K] -> [B, Cout, Tout] fp32"""
    from aero_amd import _lib, seanet
    B, Cin, T = x.shape
    h = x.transpose(1, 2).contiguous().half()
    if transposed:
        r = stride
        Cout, K = w.shape[1], 2
        wt = w.permute(2, 1, 0)
        wm = torch.stack([wt[r:], wt[:r]], 2).reshape(r * Cout, 2 * Cin)
        geo = dict(stride=1, dil=1, pad=1, reflect=0, R=r, P=pad, Tq=T + 1, Tout=(T - 1) * r + 2 * r - 2 * pad + opad)
        bias = bias.repeat(r)
    else:
        Cout, K = w.shape[0], w.shape[2]
        wm = w.permute(0, 2, 1).reshape(Cout, K * Cin)
        Tout = (T + 2 * pad - dil * (K - 1) - 1) // stride + 1
        geo = dict(stride=stride, dil=dil, pad=pad, reflect=reflect, R=1, P=0, Tq=Tout, Tout=Tout)
    img = seanet.mfma_image(wm, 'cpu')
    bias = bias.float().contiguous()
    y = torch.empty(B, geo['Tout'], Cout, dtype=torch.float16)
    a = None if add is None else add.transpose(1, 2).contiguous().half()
    d = _lib.SeanetConvDesc()
    d.x, d.wimg, d.bias, d.add, d.y = h.data_ptr(), img.data_ptr(), bias.data_ptr(), None if a is None else a.data_ptr(), y.data_ptr()
    d.B, d.Tin, d.Cin, d.Tq, d.M, d.K, d.stride, d.dil, d.pad = B, T, Cin, geo['Tq'], geo['R'] * Cout, K, geo['stride'], geo['dil'], geo['pad']
    d.reflect, d.ksteps, d.R, d.P, d.Tout, d.Cout, d.act, d.in_slope = geo['reflect'], (K * Cin + 31) // 32, geo['R'], geo['P'], geo['Tout'], Cout, act, in_slope
    lib.call('aero_seanet_conv', C.byref(d), None)
    return y.float().transpose(1, 2)


def res_weights(Cc, seed):
    """(w1 [C, C, 3], b1, w2 [C, C, 1], b2, ws [C, C, 1], bs), weights fp16-exact"""
    s = 1.0 / (3 * Cc) ** 0.5
    return (f16((Cc, Cc, 3), seed, s), 0.1 * f16((Cc,), seed + 1), f16((Cc, Cc, 1), seed + 2, 2 * s), 0.1 * f16((Cc,), seed + 3),
            f16((Cc, Cc, 1), seed + 4, 2 * s), 0.1 * f16((Cc,), seed + 5))


def run_resblock(lib, x, wts, d, add=None):
    """aero_seanet_resblock on x [B, C, T] -> [B, C, T] fp32"""
    from aero_amd import _lib, seanet
    w1, b1, w2, b2, ws, bs = wts
    B, Cc, T = x.shape
    h = x.transpose(1, 2).contiguous().half()
    i1 = seanet.mfma_image(w1.permute(0, 2, 1).reshape(Cc, 3 * Cc), 'cpu')
    i2 = seanet.mfma_image(torch.cat([w2[:, :, 0], ws[:, :, 0]], 1), 'cpu')
    b1, b2s = b1.float().contiguous(), (b2 + bs).float().contiguous()
    y = torch.empty(B, T, Cc, dtype=torch.float16)
    a = None if add is None else add.transpose(1, 2).contiguous().half()
    r = _lib.SeanetResDesc()
    r.x, r.w1, r.w2s, r.b1, r.b2s, r.add, r.y = h.data_ptr(), i1.data_ptr(), i2.data_ptr(), b1.data_ptr(), b2s.data_ptr(), None if a is None else a.data_ptr(), y.data_ptr()
    r.B, r.T, r.C, r.d, r.ks1, r.ks2, r.slope = B, T, Cc, d, (3 * Cc + 31) // 32, (2 * Cc + 31) // 32, SLOPE
    rc = lib.cdll.aero_seanet_resblock(C.byref(r), None)
    if rc != 0:
        raise RuntimeError(lib.cdll.aero_last_error().decode())
    return y.float().transpose(1, 2)


def resblock_f64(x, wts, d, add=None, hidden_fp16=True):
    """float64 restatement of ResnetBlock(C, dilation d) (seanet.py:10-23) on fp16-exact operands; the hidden activation rounded to fp16
    where the kernels store it (before and after its LeakyReLU)"""
    w1, b1, w2, b2, ws, bs = (t.double() for t in wts)
    xd = x.double()
    a = lrelu(xd).half().double()                                # (lrelu of an fp16 value is rounded to fp16 as the MFMA operand)
    hid = F.conv1d(F.pad(a, (d, d), mode='reflect'), w1, b1, dilation=d)
    if hidden_fp16:
        hid = lrelu(hid.half().double()).half().double()
    else:
        hid = lrelu(hid)
    y = F.conv1d(hid, w2, b2) + F.conv1d(xd, ws, bs)
    return y if add is None else y + add.double()


def resblock_layers(lib, x, wts, d, add=None):
    """the layer-by-layer form (AERO_SEANET_FUSE=0): three launches of the general conv"""
    w1, b1, w2, b2, ws, bs = wts
    s = run_conv(lib, x, ws, bs, add=add)
    hid = run_conv(lib, x, w1, b1, dil=d, pad=d, reflect=1, in_slope=SLOPE)
    return run_conv(lib, hid, w2, b2, in_slope=SLOPE, add=s)


def run_front(lib, x, lr_sr, hr_sr, Tpad=None, stats=None):
    """aero_seanet_front with the resampling table of (lr_sr, hr_sr): x [B, L] fp32 -> [B, Tpad]"""
    from aero_amd import seanet
    B, L = x.shape
    table, og, nw, width = seanet.resample_table(lr_sr, hr_sr)
    Lup = -((-nw * L) // og)
    Tpad = Tpad or Lup
    y = torch.empty(B, Tpad, dtype=torch.float32)
    x = x.contiguous()
    lib.call('aero_seanet_front', x.data_ptr(), None if stats is None else stats.data_ptr(), table.data_ptr(), y.data_ptr(), B, L, Lup, Tpad, og, nw,
             width, None)
    return y, Lup
