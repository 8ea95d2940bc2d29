"""Numeric parity for every conv kernel aero_conv_plan can pick under the default environment (k_conv.h, k_conv_ring.h): one named case
per kernel instantiation and tile edge, shared by tests/test_conv_family.py (CPU: the dispatch of every case, the checker itself, the
emulator) and tests/test_gpu_conv_family.py (the MI355X).

Every case goes the real way -- pack.conv2d_taps / conv1d_taps / convtr_taps / convtr_stacked_spec, pack.make_conv_spec, Ops.conv on real
tensors -- and states the ONE kernel name it is meant to reach (`want`); check_case asks aero_conv_kernel_name about the very descriptor
Ops.conv is about to launch and refuses to launch anything else.  The sources are interior views of buffers whose one-step border in
frequency and time is NaN, the destination starts as NaN, and the result is compared with a float64 reference on the fp16-rounded operands
twice: rel-L2 of the whole output (TOL16, the project's bar) and rel-L2 of every 16-channel x 64-step block of every (batch item,
frequency row) (BLOCK_BAR) -- a wrong last time column, a ragged last M-tile or a K-chunk that was not zero-padded costs a few per cent of
ONE block and next to nothing of the whole output of a production-sized launch."""
import math
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from conftest import rel_l2                                      # (first: conftest puts the repository root on sys.path)
from aero_amd import _lib, pack
from aero_amd.engine import Ops
from op_cases import TOL16

ACTS = {'none': _lib.ACT_NONE, 'relu': _lib.ACT_RELU, 'gelu': _lib.ACT_GELU, 'glu': _lib.ACT_GLU}
BLOCK_M, BLOCK_T = 16, 64
# The reference's own floor: the largest block rel-L2, over every case of CASES, between an fp32-accumulate conv (torch, CPU) on the
# fp16-rounded operands with its output rounded to the destination's type and the float64 reference.  Measured 4.47e-4, on a 1-row x
# 2-step edge block of 'carry<1> one output channel' (an fp16 rounding is at most 2^-11 = 4.9e-4 of its value; the median block of every
# case sits at 1.8e-4 - 2.2e-4).  The bar is 4 x that = 1.79e-3 (MFMA against torch summation order, a rounding that flips), never above
# TOL16; tests/test_conv_family.py measures the floor again and fails if this constant no longer follows it.
REF_FLOOR = 4.47e-4
BLOCK_BAR = min(4 * REF_FLOOR, TOL16)


def _rand(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def q16(x):
    return x.half().float()


# ---------------------------------------------------------------------------------------------------------------------------------
# the table.  kind 'conv': Conv2d [kF, kT], frequency stride `stride`, low-side padding (padF, padT), time dilation `dil`, Fout rows
# (default: the symmetric-padding count); `pick`: only these taps of the kF x kT grid are kept (an irregular tap list).
# kind 'convtr': ConvTranspose2d [K, 1] / [stride, 1], trimmed by (K - stride) / 2 rows on both sides.  kind 'stacked': the same from the
# input side (pack.convtr_stacked_spec, row scatter).  C1 > 0: two sources; null0: src0 = None (its channels are zero).
# dst: 'dense' | 'strided' (time steps `Mout + 8` apart) | 'freq' (the [B, T, F*M] layout of the tiny kernel) | 'f32' | 'own' (Ops.conv
# allocates: tap split).  stats = G: epilogue statistics (stat_mode 1) over G groups.  res / post / affine: the epilogue's residual, frequency
# embedding row (post_add) and per-item scale and shift (batch_scale / batch_shift), applied in that order after the activation.
def _c(name, want, **kw):
    c = dict(name=name, want=want, kind='conv', C0=32, C1=0, M=64, kF=1, kT=1, stride=1, padF=None, padT=None, dil=1, Fin=2, T=65, B=2,
             act='none', null0=False, res=False, post=False, affine=False, stats=0, per_row=False, dst='dense', tap_split=1, pick=None, K=0)
    assert not set(kw) - set(c), set(kw) - set(c)
    c.update(kw)
    if c['padF'] is None:
        c['padF'] = (c['kF'] - 1) // 2
    if c['padT'] is None:
        c['padT'] = c['dil'] * (c['kT'] - 1) // 2
    return c


def _ring(t):
    return f'aero_conv_ring_kernel<{t}, 0>'


def _st(flag):
    return 'true' if flag else 'false'


def _table():
    out = []
    # -- software-pipelined ring tiles (k_conv_ring.h), the smallest M and K aero_conv_ring_pick_bm accepts --------------------------
    # 256 rows, K = 3 time taps x 128 channels = 384: 128-step tiles on four waves when their count is odd, 256-step tiles otherwise
    r256 = dict(M=256, C0=128, kT=3)
    for T, tile, kw in ((127, '2, 2, 4, 3', dict(act='relu')), (128, '2, 2, 4, 3', {}), (129, '2, 4, 4, 3', dict(act='gelu')), (255, '2, 4, 4, 3', {}),
                        (256, '2, 4, 4, 3', dict(act='glu')), (257, '2, 2, 4, 3', dict(act='gelu')), (383, '2, 2, 4, 3', dict(act='glu')),
                        (384, '2, 2, 4, 3', dict(C0=72, C1=56)), (385, '2, 4, 4, 3', dict(act='relu')), (2, '2, 2, 4, 3', {})):
        out.append(_c(f'ring256 T={T}', _ring(tile), T=T, **{**r256, **kw}))
    out += [_c('ring256 3x3 null src0', _ring('2, 4, 4, 3'), M=256, C0=64, C1=64, kF=3, kT=3, null0=True, Fin=3, T=130),
            _c('ring256 stats', _ring('2, 2, 4, 3'), T=70, stats=4, **r256),
            _c('ring256 one tap', _ring('2, 4, 4, 1'), M=256, C0=384, T=129, act='relu'),
            _c('ring256 strided [4,1]', _ring('2, 4, 4, 1'), M=256, C0=128, kF=4, stride=2, padF=1, Fin=6, T=257, act='gelu'),
            _c('ring256 one tap glu', _ring('2, 4, 4, 1'), M=256, C0=360, C1=24, T=64, act='glu')]
    # 192 rows x 128 steps, K = 768
    r192 = dict(M=192, C0=48, C1=48, kF=3, kT=3, Fin=3)
    out += [_c('ring192 T=127 glu', _ring('2, 2, 3, 3'), T=127, act='glu', **r192), _c('ring192 T=128', _ring('2, 2, 3, 3'), T=128, **r192),
            _c('ring192 T=129 relu', _ring('2, 2, 3, 3'), T=129, act='relu', **r192),
            _c('ring192 T=1 gelu', _ring('2, 2, 3, 3'), M=192, C0=256, kT=3, T=1, act='gelu')]
    # 96 rows x 256 steps on four waves (M = 96 only), K = 768
    r96 = dict(M=96, C0=256, kT=3)
    out += [_c('ring96 T=255', _ring('1, 4, 3, 3'), T=255, **r96), _c('ring96 T=256 relu', _ring('1, 4, 3, 3'), T=256, act='relu', **r96),
            _c('ring96 T=257 dilation 2', _ring('1, 4, 3, 3'), T=257, dil=2, act='gelu', **r96),
            _c('ring96 3x3 glu', _ring('1, 4, 3, 3'), M=96, C0=88, kF=3, kT=3, Fin=3, T=70, act='glu')]
    # 128 / 64 rows x 512 steps
    r128, r64 = dict(M=128, C0=256, kT=3), dict(M=64, C0=256, kT=3)
    out += [_c('ring128 T=511', _ring('1, 8, 4, 3'), T=511, act='gelu', **r128), _c('ring128 T=513 glu', _ring('1, 8, 4, 3'), T=513, act='glu', **r128),
            _c('ring128 T=2', _ring('1, 8, 4, 3'), T=2, act='relu', **r128),
            _c('ring128 3x3', _ring('1, 8, 4, 3'), M=128, C0=48, C1=48, kF=3, kT=3, Fin=3, T=130),
            _c('ring64 T=512', _ring('1, 8, 2, 3'), T=512, **r64), _c('ring64 T=513 relu', _ring('1, 8, 2, 3'), T=513, act='relu', **r64),
            _c('ring64 T=3 gelu', _ring('1, 8, 2, 3'), T=3, act='gelu', **r64),
            _c('ring64 3x3 glu', _ring('1, 8, 2, 3'), M=64, C0=96, kF=3, kT=3, Fin=3, T=70, act='glu')]
    # -- the 8-wave glds tiles: the ring has to decline (residual, statistics groups it does not take, a non-slab tap grid, K < 768) ---
    out += [_c('glds8 256 res', 'aero_conv_glds8_kernel<4, 32, false>', M=256, C0=120, kF=3, kT=3, Fin=3, T=129, res=True, act='gelu'),
            _c('glds8 256 stats G=16', 'aero_conv_glds8_kernel<4, 32, true>', M=256, C0=128, kF=3, kT=3, Fin=3, T=127, stats=16),
            _c('glds8 256 glu T=2', 'aero_conv_glds8_kernel<4, 32, false>', M=256, C0=128, kF=3, kT=3, Fin=2, T=2, res=True, act='glu'),
            _c('glds8 192 [3,1]', 'aero_conv_glds8_kernel<3, 32, false>', M=192, C0=72, C1=56, kF=3, Fin=3, T=128, act='relu'),
            _c('glds8 192 stats', 'aero_conv_glds8_kernel<3, 32, true>', M=192, C0=128, kF=3, Fin=3, T=129, stats=4),
            _c('glds8 192 strided [8,1]', 'aero_conv_glds8_kernel<3, 32, false>', M=192, C0=64, kF=8, stride=2, padF=3, Fin=6, T=65)]
    # -- the 4-wave glds tiles <MF, WM>: KC 32 / KC 64, without / with statistics.  Ragged M, C0 no multiple of 32 where they can be
    ragged = {(4, 2): 104, (3, 2): 88, (4, 1): 56, (3, 1): 40, (2, 1): 24, (1, 1): 12}
    whole = {(4, 2): 128, (3, 2): 96, (4, 1): 64, (3, 1): 48, (2, 1): 32, (1, 1): 16}
    acts = ['none', 'relu', 'gelu', 'glu']
    for i, (mf, wm) in enumerate(ragged):
        big = wm == 2                                            # (KC 64: K >= 1024 on the 128- / 96-row tiles, K >= 2048 on a small grid below)
        k64 = dict(C0=104, kT=9) if big else dict(C0=232, kF=9, Fin=4)
        for st in (0, 1):
            M = whole[mf, wm] if st else ragged[mf, wm]
            act = 'none' if st else acts[i % 4]
            M += M % 2 if act == 'glu' else 0
            keep = dict(res=True) if M <= 16 and not st else {}    # (keeps M <= 16 off the skinny kernels)
            out.append(_c(f'glds<{mf},{wm}> KC32 M={M}{" stats" if st else ""}', f'aero_conv_glds_kernel<{mf}, {wm}, 32, {_st(st)}>',
                          M=M, C0=40 if st else (40, 72)[i % 2], kF=3, kT=3, Fin=3, T=(127, 128, 129, 2, 130, 65)[i], act=act, stats=st, **keep))
            out.append(_c(f'glds<{mf},{wm}> KC64 M={M}{" stats" if st else ""}', f'aero_conv_glds_kernel<{mf}, {wm}, 64, {_st(st)}>',
                          M=M, T=(129, 127, 70, 128, 66, 130)[i], act=acts[(i + 1) % 4] if not st and M % 2 == 0 else 'none', stats=st,
                          per_row=bool(st and i % 2), **k64, **keep))
    out += [_c('glds two sources 40+24', 'aero_conv_glds_kernel<4, 1, 32, false>', M=56, C0=40, C1=24, kF=3, kT=3, Fin=3, T=129, act='gelu'),
            _c('glds null src0', 'aero_conv_glds_kernel<3, 1, 32, false>', M=40, C0=40, C1=24, kF=3, kT=3, Fin=3, T=70, null0=True),
            _c('glds tap split', 'aero_conv_glds_kernel<4, 1, 32, false>', M=64, C0=64, kT=3, T=129, act='relu', tap_split=3, dst='own'),
            _c('glds scatter', 'aero_conv_glds_kernel<4, 1, 32, false>', kind='stacked', M=32, C0=64, K=4, stride=2, Fin=3, T=65),
            _c('glds f32 dst', 'aero_conv_glds_kernel<4, 1, 32, false>', M=64, C0=72, kF=3, Fin=3, T=128, dst='f32'),
            _c('glds per-item affine', 'aero_conv_glds_kernel<4, 1, 32, false>', M=56, C0=40, kF=3, kT=3, Fin=3, T=129, act='relu', res=True, affine=True),
            _c('glds frequency embedding', 'aero_conv_glds_kernel<3, 2, 32, false>', M=80, C0=72, kF=3, kT=3, Fin=4, T=127, act='glu', post=True),
            _c('glds f32 affine', 'aero_conv_glds_kernel<2, 1, 32, false>', M=24, C0=40, kT=3, T=65, dst='f32', affine=True, post=True),
            _c('glds strided [8,1]', 'aero_conv_glds_kernel<3, 1, 32, false>', M=48, C0=24, kF=8, stride=4, padF=2, Fin=8, T=127, act='gelu')]
    # -- the generic (register-staged) kernel: 4-channel pieces (C0 = 12), irregular taps
    for i, (mf, wm) in enumerate(ragged):
        for st in (0, 1):
            M = whole[mf, wm] if st else ragged[mf, wm]
            act = 'none' if st else acts[(i + 2) % 4]
            keep = dict(res=True) if M <= 16 and not st else {}
            out.append(_c(f'generic<{mf},{wm}> M={M}{" stats" if st else ""}', f'aero_conv_kernel<{mf}, {wm}, {_st(st)}>', M=M, C0=12, kF=3, kT=3,
                          Fin=3, T=(129, 128, 127, 65, 2, 130)[i], act=act, stats=st, **keep))
    out += [_c('generic irregular taps', 'aero_conv_kernel<4, 1, false>', M=56, C0=40, kF=2, kT=2, padF=0, padT=0, pick=[0, 3], Fin=3, T=129),
            _c('generic per-item affine', 'aero_conv_kernel<3, 1, false>', M=40, C0=12, kF=3, kT=3, Fin=3, T=129, act='gelu', affine=True),
            _c('generic strided [4,1] 2 channels', 'aero_conv_kernel<2, 1, false>', M=24, C0=2, kF=4, stride=2, padF=1, Fin=6, T=70, act='relu')]
    # -- M <= 16: skinny<8 / 4 / 2 / 1> by the widest aligned load piece, the lean streaming form, the carried-tap transposed conv
    sk = 'aero_conv_skinny_kernel'
    out += [_c('skinny8 two sources T=63', f'{sk}<8>', M=8, C0=32, C1=32, kF=3, kT=3, Fin=3, T=63, act='gelu'),
            _c('skinny8 strided dst T=64', f'{sk}<8>', M=8, C0=32, T=64, dst='strided', act='relu'),
            _c('skinny8 T=65 M=16', f'{sk}<8>', M=16, C0=40, C1=24, kF=3, kT=3, Fin=3, T=65),
            _c('skinny4 T=2', f'{sk}<4>', M=16, C0=4, kF=3, kT=3, Fin=3, T=2, act='relu'),
            _c('skinny4 transposed', f'{sk}<4>', kind='convtr', M=4, C0=4, K=4, stride=2, Fin=3, T=65),
            _c('skinny2 T=64', f'{sk}<2>', M=16, C0=2, kF=3, kT=3, Fin=4, T=64, act='gelu'),
            _c('skinny2 6 channels', f'{sk}<2>', M=7, C0=6, kT=3, T=63),
            _c('skinny1 T=65', f'{sk}<1>', M=16, C0=1, kF=3, kT=3, Fin=3, T=65),
            _c('skinny1 3 channels strided dst', f'{sk}<1>', M=5, C0=3, kF=3, T=64, dst='strided', act='relu')]
    stm = 'aero_conv_stream_kernel'
    out += [_c('stream T=65', stm, M=8, C0=32, T=65, act='relu'), _c('stream two frequency taps', stm, M=8, C0=32, kF=2, padF=1, Fin=3, T=64),
            _c('stream three time taps T=2', stm, M=16, C0=32, kT=3, T=2, act='gelu'), _c('stream [3,1] T=63', stm, M=12, C0=64, kF=3, Fin=3, T=63),
            _c('stream transposed', stm, kind='convtr', M=4, C0=32, K=8, stride=4, Fin=3, T=65)]
    for n, (T, Fin, act) in zip((1, 2, 3), ((64, 10, 'relu'), (65, 7, 'none'), (63, 21, 'gelu'))):   # Fin + 1 source rows: 11 = 6 + 5, 8, 22 = 6 + 6 + 6 + 4
        out.append(_c(f'carry<{n}> T={T} Fin={Fin}', f'aero_convtr_carry_kernel<{n}>', kind='convtr', M=2, C0=32 * n, K=8, stride=4, Fin=Fin, T=T, act=act))
    out.append(_c('carry<1> one output channel', 'aero_convtr_carry_kernel<1>', kind='convtr', M=1, C0=32, K=8, stride=4, Fin=5, T=130))
    out.append(_c('carry<3> f32 affine', 'aero_convtr_carry_kernel<3>', kind='convtr', M=2, C0=96, K=8, stride=4, Fin=5, T=66, dst='f32', affine=True))
    # -- the transposing pointwise kernel: T and F just past its 64 x 32 tile
    out += [_c('tiny T=65 F=33', 'aero_conv_tiny_kernel', M=5, C0=2, Fin=33, T=65, dst='freq', act='relu'),
            _c('tiny T=64 F=32', 'aero_conv_tiny_kernel', M=8, C0=8, Fin=32, T=64, dst='freq'),
            _c('tiny T=63 F=3', 'aero_conv_tiny_kernel', M=3, C0=3, Fin=3, T=63, dst='freq', act='gelu')]
    return out


CASES = _table()
BY_NAME = {c['name']: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def family(want):
    return want.split('<')[0].replace('aero_', '').replace('_kernel', '')


# time-tile widths of each family's kernels (ring: 128 / 256 / 512 by tile), the activations its plan branch accepts, and whether its
# descriptors can carry time taps / frequency taps at all
FAMILIES = {'conv_ring': dict(widths=(128, 256, 512), acts='none relu gelu glu', ttaps=True, ftaps=True),
            'conv_glds8': dict(widths=(128,), acts='none relu gelu glu', ttaps=True, ftaps=True),
            'conv_glds': dict(widths=(128,), acts='none relu gelu glu', ttaps=True, ftaps=True),
            'conv': dict(widths=(128,), acts='none relu gelu glu', ttaps=True, ftaps=True),
            'conv_skinny': dict(widths=(64,), acts='none relu gelu', ttaps=True, ftaps=True),
            'conv_stream': dict(widths=(64,), acts='none relu gelu', ttaps=True, ftaps=True),
            'convtr_carry': dict(widths=(64,), acts='none relu gelu', ttaps=False, ftaps=True),
            'conv_tiny': dict(widths=(64,), acts='none relu gelu', ttaps=False, ftaps=False)}


def _reaches_both_ways(c):
    """a frequency tap reads above row 0 AND below the last source row"""
    if c['kind'] != 'conv':
        return True                                              # (a transposed conv's first / last output rows have a tap outside by construction)
    lo = -c['padF']
    hi = (_fout(c) - 1) * c['stride'] + c['kF'] - 1 - c['padF']
    return lo < 0 and hi > c['Fin'] - 1


def check_table():
    """the edges every family has to see, asserted from the table itself"""
    fams = {}
    for c in CASES:
        fams.setdefault(family(c['want']), []).append(c)
    assert set(fams) == set(FAMILIES), set(fams) ^ set(FAMILIES)
    for f, info in FAMILIES.items():
        cs = fams[f]
        Ts = {c['T'] for c in cs}
        for w in info['widths']:
            assert {w - 1, w, w + 1} <= Ts, (f, w, sorted(Ts))
        if info['ttaps']:
            assert any(c['kT'] == 3 and c['T'] <= 2 for c in cs), f'{f}: no case with T below the reach of three time taps'
        if info['ftaps']:
            assert any(_reaches_both_ways(c) for c in cs), f'{f}: no frequency tap outside the rows'
        assert {c['act'] for c in cs} == set(info['acts'].split()), (f, {c['act'] for c in cs})
    assert any(c['stride'] > 1 and c['kind'] == 'conv' for c in CASES)
    assert all(c['B'] == 2 and (2 <= c['Fin'] <= 4 or family(c['want']) in ('convtr_carry', 'conv_tiny') or c['stride'] > 1) for c in CASES)


# ---------------------------------------------------------------------------------------------------------------------------------
def _fout(c):
    if c['kind'] == 'conv':
        return (c['Fin'] + 2 * c['padF'] - c['kF']) // c['stride'] + 1
    return (c['Fin'] - 1) * c['stride'] + c['K']                  # untrimmed rows of the transposed conv


def _weights(c, seed):
    Cin = c['C0'] + c['C1']
    if c['kind'] == 'conv':
        w = _rand((c['M'], Cin, c['kF'], c['kT']), seed, 1.0 / math.sqrt(Cin * (len(c['pick']) if c['pick'] else c['kF'] * c['kT'])))
        if c['pick']:                                            # the taps that are not kept do not exist
            keep = torch.zeros(c['kF'] * c['kT'])
            keep[c['pick']] = 1
            w = w * keep.view(1, 1, c['kF'], c['kT'])
    else:
        w = _rand((Cin, c['M'], c['K'], 1), seed, 1.0 / math.sqrt(Cin * c['K'] / c['stride']))
    return q16(w)


def linear64(c, x, w):
    """the convolution alone (no bias) in float64: x [B, Cin, Fin, T], w as _weights gives it -> [B, M, Fout', T]"""
    x, w = x.double(), w.double()
    if c['kind'] == 'conv':
        hi_f = (_fout(c) - 1) * c['stride'] + c['kF'] - c['padF'] - c['Fin']
        hi_t = (c['kT'] - 1) * c['dil'] - c['padT']
        assert hi_f >= 0 and hi_t >= 0
        return F.conv2d(F.pad(x, (c['padT'], hi_t, c['padF'], hi_f)), w, None, stride=(c['stride'], 1), dilation=(1, c['dil']))
    y = F.conv_transpose2d(x, w, None, stride=(c['stride'], 1))
    pad = (c['K'] - c['stride']) // 2
    return y[:, :, pad:y.shape[2] - pad] if pad else y


def finish(c, lin, ops):
    """bias, activation, residual, frequency embedding, per-item affine (the epilogue order of include/aero_hip.h) in lin's precision"""
    t = lin.dtype
    v = lin + ops['b'].to(t).view(1, -1, 1, 1)
    v = {'none': lambda u: u, 'relu': F.relu, 'gelu': F.gelu, 'glu': lambda u: F.glu(u, 1)}[c['act']](v)
    if ops['r'] is not None:
        v = v + ops['r'].to(t)
    if ops['post'] is not None:
        v = v + ops['post'].to(t).t()[None, :, :, None]
    if ops['sc'] is not None:
        v = v * ops['sc'].to(t).view(-1, 1, 1, 1) + ops['sh'].to(t).view(-1, 1, 1, 1)
    return v


def make(c):
    """seeded operands and the float64 reference of a case (CPU; no library involved)"""
    seed = zlib.crc32(c['name'].encode()) % 100000              # (a case keeps its operands when the table grows)
    Cin = c['C0'] + c['C1']
    w = _weights(c, seed)
    b = _rand((c['M'],), seed + 1)
    x = q16(_rand((c['B'], Cin, c['Fin'], c['T']), seed + 2))
    if c['null0']:
        x[:, :c['C0']] = 0
    lin = linear64(c, x, w)
    Mout = c['M'] // 2 if c['act'] == 'glu' else c['M']
    ops = dict(w=w, b=b, x=x, lin=lin, r=q16(_rand((c['B'], Mout, lin.shape[2], c['T']), seed + 3)) if c['res'] else None,
               post=_rand((lin.shape[2], Mout), seed + 4) if c['post'] else None,
               sc=_rand((c['B'],), seed + 5).abs() + 0.5 if c['affine'] else None, sh=_rand((c['B'],), seed + 6) if c['affine'] else None)
    ops['ref'] = finish(c, lin, ops)
    return ops


def floor_output(c, ops):
    """what the reference's own arithmetic gives: fp32 accumulation (torch, CPU) on the same operands, the output rounded to the
    destination's type"""
    x, w = ops['x'].float(), ops['w'].float()
    if c['kind'] == 'conv':
        hi_f = (_fout(c) - 1) * c['stride'] + c['kF'] - c['padF'] - c['Fin']
        lin = F.conv2d(F.pad(x, (c['padT'], (c['kT'] - 1) * c['dil'] - c['padT'], c['padF'], hi_f)), w, None, stride=(c['stride'], 1), dilation=(1, c['dil']))
    else:
        lin = F.conv_transpose2d(x, w, None, stride=(c['stride'], 1))
        pad = (c['K'] - c['stride']) // 2
        lin = lin[:, :, pad:lin.shape[2] - pad] if pad else lin
    v = finish(c, lin, ops)
    return v if c['dst'] == 'f32' else q16(v)


# ---------------------------------------------------------------------------------------------------------------------------------
# the comparison
def block_errors(got, ref):
    """got, ref [B, M, F, T] -> (rel-L2 per block [B, ceil(M/16), F, ceil(T/64)], the reference's norm per block); partial edge blocks
    are blocks of their own"""
    got, ref = got.double(), ref.double()
    B, M, Fq, T = ref.shape
    assert got.shape == ref.shape, (got.shape, ref.shape)
    pm, pt = -M % BLOCK_M, -T % BLOCK_T

    def blocks(v):
        v = F.pad(v.permute(0, 2, 1, 3), (0, pt, 0, pm))         # [B, F, M', T']
        return v.reshape(B, Fq, (M + pm) // BLOCK_M, BLOCK_M, (T + pt) // BLOCK_T, BLOCK_T).sum((3, 5)).permute(0, 2, 1, 3)
    den = blocks(ref * ref).sqrt()
    return blocks((got - ref) ** 2).sqrt() / den, den


def judge(got, ref, block_bar=None):
    """-> dict(glob, worst, where, ok_global, ok): `ok` is what check_case asserts.  A NaN anywhere fails both."""
    bar = BLOCK_BAR if block_bar is None else block_bar
    err, den = block_errors(got, ref)
    assert bool((den > 0).all()), 'a block of the reference is all zero'
    glob = rel_l2(got, ref)
    bad = ~(err < bar)                                           # (NaN compares false: a poisoned block is a failed block)
    flat = torch.nan_to_num(err, nan=float('inf')).flatten()
    where = tuple(int(i) for i in np.unravel_index(int(flat.argmax()), tuple(err.shape)))     # (batch item, channel block, row, time block)
    ok_global = bool(glob < TOL16)
    return dict(glob=glob, worst=float(flat.max()), where=where, nbad=int(bad.sum()), nblocks=err.numel(), ok_global=ok_global, ok=ok_global and not bool(bad.any()))


# ---------------------------------------------------------------------------------------------------------------------------------
def _poisoned_source(x_cl, dev):
    """x_cl fp16 [B, F, T, C] -> the interior view of a [B, F + 2, T + 2, C] buffer whose border is NaN"""
    B, Fq, T, Cc = x_cl.shape
    buf = torch.full((B, Fq + 2, T + 2, Cc), float('nan'), dtype=torch.float16)
    buf[:, 1:-1, 1:-1] = x_cl
    return buf.to(dev)[:, 1:-1, 1:-1]


def _cl(x):
    return x.permute(0, 2, 3, 1).contiguous().half()


def launch(lib, dev, c, ops, dry=False):
    """build the case's spec, sources and destination on `dev` and run Ops.conv; -> (output in the reference's layout [B, Mout, F, T]
    on the CPU, the kernel name asked about the launched descriptor, leftovers to check).  dry: nothing is launched, only the name."""
    o = Ops(lib)
    C0, B, T, Fin = c['C0'], c['B'], c['T'], c['Fin']
    act = ACTS[c['act']]
    kw = {}
    if c['kind'] == 'conv':
        if c['kF'] == 1 and c['dil'] > 1:
            taps, df, dt = pack.conv1d_taps(ops['w'][:, :, 0], c['dil'], c['padT'])
        else:
            taps, df, dt = pack.conv2d_taps(ops['w'], c['padF'], c['padT'])
        if c['pick']:
            taps, df, dt = taps[:, :, c['pick']], [df[i] for i in c['pick']], [dt[i] for i in c['pick']]
        spec = pack.make_conv_spec(taps, ops['b'], C0, c['C1'], df, dt, dev, fstride=c['stride'], act=act)
        Fout = rows = _fout(c)
    elif c['kind'] == 'convtr':
        taps, df, dt = pack.convtr_taps(ops['w'], c['stride'])
        spec = pack.make_conv_spec(taps, ops['b'], C0, 0, df, dt, dev, transposed=1, fstride=c['stride'], act=act)
        pad = (c['K'] - c['stride']) // 2
        Fout, rows = _fout(c), _fout(c) - 2 * pad
        kw.update(dst_f_off=pad, dst_F=rows)
    else:
        spec = pack.convtr_stacked_spec(ops['w'], ops['b'], c['stride'], dev, act=act)
        pad = (c['K'] - c['stride']) // 2
        rows = _fout(c) - 2 * pad
        Fout = Fin - 1 + len(spec.df)
        kw.update(dst_F=Fout, scatter=(c['M'], c['stride'], pad, rows))
    xcl = _cl(ops['x'])
    s0 = None if c['null0'] else _poisoned_source(xcl[..., :C0], dev)
    s1 = _poisoned_source(xcl[..., C0:], dev) if c['C1'] else None
    Mout = c['M'] // 2 if c['act'] == 'glu' else c['M']
    nan = float('nan')
    buf = None
    # every destination is a view of a NaN buffer with one more time step (and, 'strided', eight more channels per step) than the conv writes
    if c['dst'] == 'own':
        dst = None
    elif c['dst'] == 'freq':
        buf = torch.full((B, T + 1, rows * Mout), nan, dtype=torch.float16, device=dev)
        dst, kw['dst_strides'] = buf, ((T + 1) * rows * Mout, Mout, rows * Mout)
    else:
        buf = torch.full((B, rows, T + 1, Mout + (8 if c['dst'] == 'strided' else 0)), nan, dtype=torch.float32 if c['dst'] == 'f32' else torch.float16, device=dev)
        dst = buf[:, :, :T, :Mout]
    if c['res']:
        kw['res'] = _cl(ops['r']).to(dev)
    if c['post']:
        kw['post_add'] = ops['post'].to(dev).contiguous()
    if c['affine']:
        kw.update(batch_scale=ops['sc'].to(dev), batch_shift=ops['sh'].to(dev))
    st = None
    if c['stats']:
        st = o.new_stats(B, Fout, c['stats'], c['per_row'], dev)
        kw['stat'] = dict(mode=1, stats=st, G=c['stats'], per_row=c['per_row'])
    if c['tap_split'] > 1:
        kw['tap_split'] = c['tap_split']
    if c['dst'] == 'f32':
        kw['dst_f32'] = True
    if dry:
        return None, o.conv(spec, s0, s1, B, Fin, Fout, T, dst=dst, dry=True, **kw), None
    asked = []

    def before_launch(d):                                        # the very descriptor: a case that would reach another kernel launches nothing
        if not asked:                                            # (a tap split's second call is aero_split_finish, not a conv)
            asked.append(o.conv_kernel_name(d))
            assert asked[0] == c['want'], f'{c["name"]}: meant for {c["want"]}, the plan picks {asked[0]}'
    o.on_conv_desc = before_launch
    y = o.conv(spec, s0, s1, B, Fin, Fout, T, dst=dst, **kw)
    last = lib.cdll.aero_last_kernel_name().decode()
    if c['tap_split'] > 1:
        last = c['want'] if 'split_finish' in last else last      # (the conv's name was checked before its launch; the finish pass ran last)
    if c['dst'] == 'freq':
        got = buf.cpu().float()[:, :T].reshape(B, T, rows, Mout).permute(0, 3, 2, 1)
        spare = buf.cpu()[:, T:]
    else:
        got = y.cpu().float().permute(0, 3, 1, 2)
        spare = None
        if buf is not None:
            spare = buf.cpu().clone()
            spare[:, :, :T, :Mout] = nan
    return got, asked[0], dict(last=last, spare=spare, stats=None if st is None else st.cpu())


def kernel_for(lib, c):
    """the kernel name the plan of `lib` answers for the case's descriptor built from CPU tensors (nothing is launched)"""
    return launch(lib, 'cpu', c, make_operands_only(c), dry=True)[1]


def make_operands_only(c):
    """make() without the reference (the name query needs shapes, strides and alignment only)"""
    Cin = c['C0'] + c['C1']
    Mr = c['M'] // 2 if c['act'] == 'glu' else c['M']
    rows = _fout(c) - (0 if c['kind'] == 'conv' else 2 * ((c['K'] - c['stride']) // 2))
    return dict(w=_weights(c, 1), b=torch.zeros(c['M']), x=torch.zeros(c['B'], Cin, c['Fin'], c['T']),
                r=torch.zeros(c['B'], Mr, rows, c['T']) if c['res'] else None, post=torch.zeros(rows, Mr) if c['post'] else None,
                sc=torch.ones(c['B']) if c['affine'] else None, sh=torch.zeros(c['B']) if c['affine'] else None)


def check_stats(c, ops, st):
    """the epilogue's GroupNorm sums against float64 sums of the conv + bias (tolerances of op_cases.case_conv_stats)"""
    v = ops['lin'] + ops['b'].double().view(1, -1, 1, 1)
    B, M, Fq, T = v.shape
    G = c['stats']
    r = v.view(B, G, M // G, Fq, T)
    if c['per_row']:
        s1, s2 = r.sum((2, 4)).permute(0, 2, 1), (r * r).sum((2, 4)).permute(0, 2, 1)
    else:
        s1, s2 = r.sum((2, 3, 4)), (r * r).sum((2, 3, 4))
    got = st.view(*s1.shape, 2)
    assert torch.allclose(got[..., 1], s2, rtol=2e-4), (c['name'], got[..., 1].flatten()[:4], s2.flatten()[:4])
    assert torch.allclose(got[..., 0], s1, rtol=1e-3, atol=1e-3 * float(s2.sqrt().mean())), c['name']


def check_case(lib, dev, c, verbose=False):
    ops = make(c)
    got, asked, left = launch(lib, dev, c, ops)
    assert asked == c['want']
    token = c['want'].split('<')[0]
    assert (token if lib.is_emulator else c['want']) in left['last'], (c['name'], c['want'], left['last'])
    v = judge(got, ops['ref'])
    if verbose:
        print(f'{c["name"]:44s} {c["want"]:46s} global {v["glob"]:.2e} worst block {v["worst"]:.2e} ({v["nbad"]} of {v["nblocks"]} over {BLOCK_BAR:.2e})', flush=True)
    assert not bool(torch.isnan(got).any()), f'{c["name"]}: NaN in the output (poisoned border read, or destination not written)'
    assert v['ok'], (c['name'], v)
    if left['spare'] is not None:                                # the bytes between and behind the destination's rows are still the poison
        assert bool(torch.isnan(left['spare']).all()), f'{c["name"]}: wrote outside the destination rows'
    if c['stats']:
        check_stats(c, ops, left['stats'])
    return v


# ---------------------------------------------------------------------------------------------------------------------------------
# faults for the checker's own test (tests/test_conv_family.py): what a broken kernel would leave, applied to the reference
def fault_last_column(c, ops, everywhere):
    y = ops['ref'].clone()
    sel = slice(None) if everywhere else slice(-1, None)
    y[sel, :, sel, -1] = y[sel, :, sel, -2]
    return y


def fault_last_m_tile(c, ops, bm, everywhere):
    """the rows of the last (ragged) M-tile of height bm zeroed"""
    y = ops['ref'].clone()
    sel = slice(None) if everywhere else slice(-1, None)
    m0 = (c['M'] - 1) // bm * bm
    if c['act'] == 'glu':
        m0 //= 2
    y[sel, m0:, sel] = 0
    return y


def fault_k_chunk(c, ops, everywhere):
    """the contribution of the first 32-channel chunk of the first tap removed"""
    w = torch.zeros_like(ops['w'])
    if c['kind'] == 'conv':
        w[:, :32, 0, 0] = ops['w'][:, :32, 0, 0]
    else:
        w[:32, :, 0, 0] = ops['w'][:32, :, 0, 0]
    part = linear64(c, ops['x'], w)
    if not everywhere:
        part[:-1] = 0
        part[:, :, :-1] = 0
    return finish(c, ops['lin'] - part, ops)


def table_lines():
    """per kernel name: the cases that reach it with their (M, K, T), K = taps x channels rounded up to 32"""
    by = {}
    for c in CASES:
        if c['kind'] == 'conv':
            nt = len(c['pick']) if c['pick'] else c['kF'] * c['kT']
            M = c['M']
        else:
            nt = -(-c['K'] // c['stride'])
            M = c['M'] * (c['stride'] if c['kind'] == 'stacked' else 1)
        K = nt * (-(-(c['C0'] + c['C1']) // 32) * 32)
        by.setdefault(c['want'], []).append(f'{c["name"]} ({M}, {K}, {c["T"]})')
    return [f'{k}: ' + '; '.join(v) for k, v in sorted(by.items())]


if __name__ == '__main__':
    print('\n'.join(table_lines()))
