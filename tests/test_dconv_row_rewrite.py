"""aero_dconv_row_rewrite_fwd (k_dconv.h, RW tail): a DConv branch and the encoder's rewrite conv + GLU (+ frequency embedding row)
behind it in one launch.  Two bars per case:
  * against fp32 torch on the fp16-ROUNDED DConv output the unfused kernel writes (what the rewrite sees today): TOL16;
  * against the composition of today's launches (aero_dconv_row_fwd, then aero_pw_fwd): rel-L2 < 1e-3.
The cases run on the CPU emulation of the kernels and, marked gpu, on the device."""
import math

import pytest
import torch
import torch.nn.functional as F

import op_cases as oc
from aero_amd import _lib, pack
from aero_amd.engine import Ops
from conftest import rel_l2

PAIR_TOL = 1e-3


def case_dconv_row_rewrite(lib, dev, Cc, T, Fq=3, B=2, depth=2, act='gelu', norm=True, post=True, seed=500):
    ops = Ops(lib)
    hid = Cc // 4
    g = oc._g(seed)
    x = oc.q16(oc._rand((B, Fq, T, Cc), seed))
    actc = {'relu': _lib.ACT_RELU, 'gelu': _lib.ACT_GELU, 'snake': _lib.ACT_SNAKE}[act]
    layers = []
    for l in range(depth):
        w1 = oc.q16(oc._rand((hid, Cc, 3), seed + 10 * l + 1, 1.0 / math.sqrt(3 * Cc)))
        b1 = oc._rand((hid,), seed + 10 * l + 2, 0.3)
        w2 = oc.q16(oc._rand((2 * Cc, hid), seed + 10 * l + 3, 1.0 / math.sqrt(hid)))
        b2 = oc._rand((2 * Cc,), seed + 10 * l + 4, 0.3)
        g1, be1 = 1 + oc._rand((hid,), seed + 10 * l + 5, 0.2), oc._rand((hid,), seed + 10 * l + 6, 0.2)
        g2, be2 = 1 + oc._rand((2 * Cc,), seed + 10 * l + 7, 0.2), oc._rand((2 * Cc,), seed + 10 * l + 8, 0.2)
        scale = oc._rand((Cc,), seed + 10 * l + 9, 0.5)
        n = (lambda v: v) if norm else (lambda v: None)                               # noqa: E731
        Lr = pack.dconv_row_layer(w1, b1, n(g1), n(be1), w2, b2, n(g2), n(be2), scale, 2 ** l, dev)
        Lr['snake_a'] = (0.5 + torch.rand(Fq, generator=oc._g(seed + 10 * l + 10)) * 2).float().to(dev).contiguous() if act == 'snake' else None
        layers.append(Lr)
    wr = oc.q16(torch.randn(2 * Cc, Cc, generator=g) / math.sqrt(Cc))
    br = torch.randn(2 * Cc, generator=g)
    pe = torch.randn(Fq, Cc, generator=g) if post else None
    maxdil = 2 ** (depth - 1)
    assert ops.dconv_row_fits(T, Cc, hid, maxdil) and ops.dconv_row_fits(T, Cc, hid, maxdil, rewrite=True)
    xd = x.half().to(dev)
    # today's launches: the branch (its own parity with torch is tests/op_cases.py::case_dconv_row), then the streaming pointwise kernel
    yd = ops.dconv_row(xd, layers, actc, Fq)
    spec = pack.make_pw_spec(wr, br, _lib.ACT_GLU, lib, dev)
    assert spec is not None
    ped = None if pe is None else pe.to(dev).contiguous()
    pair = ops.pw(spec, yd, B, Fq, T, post_add=ped)
    # float reference on the same fp16-rounded DConv output
    v = torch.einsum('mc,bftc->bftm', wr, yd.float().cpu()) + br
    ref = F.glu(v, -1)
    if pe is not None:
        ref = ref + pe.view(1, Fq, 1, Cc)
    rw = pack.dconv_rewrite_image(wr, br, dev)
    assert rw is not None
    out = ops.dconv_row(xd, layers, actc, Fq, rewrite=rw, post_add=ped)
    assert out.shape == (B, Fq, T, Cc) and out.dtype == torch.float16
    e_ref, e_pair = rel_l2(out.float().cpu(), ref), rel_l2(out.float().cpu(), pair.float().cpu())
    print(f'dconv_row_rewrite C={Cc} T={T} depth={depth} act={act} post={post}: vs float reference {e_ref:.3e}, vs dconv_row + pw {e_pair:.3e}')
    assert e_ref < oc.TOL16, e_ref
    assert e_pair < PAIR_TOL, e_pair


EMU_CASES = [dict(Cc=48, T=501, Fq=1, B=1), dict(Cc=96, T=501, Fq=1, B=1, act='snake', post=False),
             dict(Cc=48, T=139, act='snake', post=False), dict(Cc=96, T=70, Fq=2, depth=1),
             dict(Cc=48, T=37, depth=1, post=False), dict(Cc=96, T=203, Fq=1, B=2, act='snake'),
             dict(Cc=16, T=33, Fq=2, B=1, act='relu', norm=False), dict(Cc=32, T=50, Fq=1), dict(Cc=64, T=20, Fq=2, B=1)]
GPU_CASES = [dict(Cc=48, T=501, Fq=64, B=2), dict(Cc=96, T=501, Fq=16, B=2, act='snake', post=False),
             dict(Cc=48, T=501, Fq=64, B=2, act='snake', post=False, depth=1), dict(Cc=96, T=501, Fq=16, B=2, depth=1),
             dict(Cc=48, T=139, act='snake'), dict(Cc=96, T=203, Fq=5, post=False), dict(Cc=48, T=37, depth=1, post=False),
             dict(Cc=16, T=33, Fq=2, B=1, act='relu', norm=False), dict(Cc=32, T=50, Fq=1), dict(Cc=64, T=600, Fq=2, B=1)]


@pytest.fixture(scope='module')
def emu():
    from emu.build_emu import build
    return _lib.load(build())


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available()
    lib = _lib.load()
    assert not lib.is_emulator
    return lib


@pytest.mark.parametrize('kw', EMU_CASES)
def test_dconv_row_rewrite_emu(emu, kw):
    case_dconv_row_rewrite(emu, 'cpu', **kw)


@pytest.mark.gpu
@pytest.mark.parametrize('kw', GPU_CASES)
def test_dconv_row_rewrite(lib, kw):
    case_dconv_row_rewrite(lib, 'cuda', **kw)


def test_rewrite_fits_accounts_for_the_weight_image(emu):
    """the bench geometries fit with the tail (C = 48 within the 80 KiB of two blocks per CU is a property of the launcher's wave count:
    aero_dconv_nw); a row that fits alone but not with the [2C][C] image is refused, and so is C % 16 != 0"""
    f, frw = emu.cdll.aero_dconv_row_fits, emu.cdll.aero_dconv_row_rewrite_fits
    assert frw(501, 48, 12, 2) == 1 and frw(501, 96, 24, 2) == 1
    assert f(390, 128, 32, 2) == 1 and frw(390, 128, 32, 2) == 0
    assert f(100, 24, 4, 1) == 0 and frw(100, 24, 4, 1) == 0
    assert frw(2000, 48, 12, 2) == 0


def test_argument_errors(emu):
    import ctypes as C
    d = _lib.DconvRewriteDesc()
    assert emu.cdll.aero_dconv_row_rewrite_fwd(None, None) == -1
    assert emu.cdll.aero_dconv_row_rewrite_fwd(C.byref(d), None) == -1 and b'dconv' in emu.cdll.aero_last_error()
