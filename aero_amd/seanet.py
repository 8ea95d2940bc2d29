"""The Seanet baseline generator on the MI355X (reference src/models/seanet.py; `model: seanet`, experiment file seanet_4-16.yaml), inference.

Same constructor arguments, module tree and state-dict keys (`encoder.{i}.{j}...`, `decoder.{i}.{j}...`, `block.{2,4}` / `shortcut` inside a
`ResnetBlock`; weight-normed Conv1d / ConvTranspose1d: `weight_g`, `weight_v`, `bias`), same RNG draws at construction (default init, weight
norm, then `weights_init`), so a seed reproduces the reference's initial weights and a reference checkpoint loads with strict keys.

The forward (seanet.py:153-179) runs on the kernels of csrc/k_seanet.h, nothing but allocations and views in between:
  * aero_seanet_stats / aero_seanet_front: per-item std, x / (floor + std), torchaudio's sinc resampling as a polyphase FIR (the formula
    of audio_io.resample; the table is built once per rate pair on the host), the right zero pad to the valid length;
  * aero_seanet_conv_in / aero_seanet_conv_out: the k = 7 convs at the waveform ends (tanh; the tail also adds the skip, trims, scales by std);
  * aero_seanet_resblock: a ResnetBlock in ONE launch (AERO_SEANET_FUSE=0: three launches of the general conv);
  * aero_seanet_conv: every other conv -- the strided convs directly (K = 2 r taps), the transposed convs as 2-tap convs that produce r
    phases x Cout channels per input row and scatter them to r output rows, the latent k = 7 convs; the decoder's skip addition rides in
    the epilogue of each stage's last kernel.
Training (the backward) is not built: a training-mode forward with gradients enabled raises NotImplementedError."""
import ctypes as C
import math
import os

import torch
from torch import nn
from torch.nn.utils import weight_norm

from . import _lib
from .discriminators import WNConv1d, weights_init
from .engine import Ops, _ptr
from .modules import capture_init

SLOPE = 0.2


def WNConvTranspose1d(*args, **kwargs):
    return weight_norm(nn.ConvTranspose1d(*args, **kwargs))    # modules.py:14-15


class ResnetBlock(nn.Module):
    """seanet.py:10-23 (parameters only; the forward is Seanet's)"""

    def __init__(self, dim, dilation=1):
        super().__init__()
        self.dilation = dilation
        self.block = nn.Sequential(
            nn.LeakyReLU(SLOPE),
            nn.ReflectionPad1d(dilation),
            WNConv1d(dim, dim, kernel_size=3, dilation=dilation),
            nn.LeakyReLU(SLOPE),
            WNConv1d(dim, dim, kernel_size=1),
        )
        self.shortcut = WNConv1d(dim, dim, kernel_size=1)

    def forward(self, x):  # pragma: no cover
        raise RuntimeError('run the block through Seanet.forward (HIP kernels)')


def mfma_image(wm, dev):
    """W fp32 [M][Kred] -> the A-fragment image of csrc/k_seanet.h: fp16 [ceil(M / 32) * 2][ceil(Kred / 32)][64][8], element
    (tile, ks, lane, e) = W[16 tile + (lane & 15)][32 ks + 8 (lane >> 4) + e], zero padded"""
    M, K = wm.shape
    Mp, Kp = (M + 31) // 32 * 32, (K + 31) // 32 * 32
    p = torch.zeros(Mp, Kp, dtype=torch.float32, device=wm.device)
    p[:M, :K] = wm
    img = p.view(Mp // 16, 16, Kp // 32, 4, 8).permute(0, 2, 3, 1, 4)
    return img.to(device=dev, dtype=torch.float16).contiguous()


def resample_table(orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99):
    """the polyphase kernels of torchaudio.functional.resample's defaults, as audio_io.resample states them: (fp32 [new][2 width + orig],
    orig, new, width) with the rates reduced by their gcd"""
    g = math.gcd(int(orig_freq), int(new_freq))
    orig, new = int(orig_freq) // g, int(new_freq) // g
    base = min(orig, new) * rolloff
    width = math.ceil(lowpass_filter_width * orig / base)
    idx = torch.arange(-width, width + orig, dtype=torch.float64)[None] / orig
    t = torch.arange(0, -new, -1, dtype=torch.float64)[:, None] / new + idx
    t = (t * base).clamp_(-lowpass_filter_width, lowpass_filter_width)
    window = torch.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t = t * math.pi
    kernels = torch.where(t == 0, torch.ones_like(t), t.sin() / t) * window * (base / orig)
    return kernels.to(torch.float32).contiguous(), orig, new, width


class Seanet(nn.Module):
    _ops, _packed, _key = None, None, None

    @capture_init
    def __init__(self, latent_space_size=128, ngf=32, n_residual_layers=3, resample=1, normalize=True, floor=1e-3,
                 ratios=[8, 8, 2, 2], in_channels=1, out_channels=1, lr_sr=16000, hr_sr=16000, upsample=True):   # noqa: B006 (the reference's signature)
        super().__init__()
        if in_channels != 1 or out_channels != 1:
            raise NotImplementedError('Seanet: in_channels = out_channels = 1 (every reference config) is what the HIP forward implements')
        if not isinstance(ngf, int) or ngf < 8 or ngf % 8:
            raise NotImplementedError(f'Seanet ngf={ngf}: a multiple of 8 (the MFMA convs read 8 channels per lane)')
        if latent_space_size % 8:
            raise NotImplementedError(f'Seanet latent_space_size={latent_space_size}: a multiple of 8')
        self.resample = resample
        self.normalize = normalize
        self.floor = floor
        self.lr_sr = lr_sr
        self.hr_sr = hr_sr
        self.scale_factor = int(self.hr_sr / self.lr_sr)
        self.upsample = upsample
        self.encoder = nn.ModuleList()
        self.decoder = nn.ModuleList()
        self.ratios = list(ratios)
        mult = int(2 ** len(ratios))
        # (construction order = the reference's: it fixes the RNG stream; seanet.py:57-119)
        decoder_wrapper = [nn.LeakyReLU(SLOPE), nn.ReflectionPad1d(3), WNConv1d(latent_space_size, mult * ngf, kernel_size=7, padding=0)]
        encoder_wrapper = [nn.LeakyReLU(SLOPE), nn.ReflectionPad1d(3), WNConv1d(mult * ngf, latent_space_size, kernel_size=7, padding=0)]
        self.encoder.insert(0, nn.Sequential(*encoder_wrapper))
        self.decoder.append(nn.Sequential(*decoder_wrapper))
        for r in self.ratios:
            encoder_block = [nn.LeakyReLU(SLOPE),
                             WNConv1d(mult * ngf // 2, mult * ngf, kernel_size=r * 2, stride=r, padding=r // 2 + r % 2)]
            decoder_block = [nn.LeakyReLU(SLOPE),
                             WNConvTranspose1d(mult * ngf, mult * ngf // 2, kernel_size=r * 2, stride=r, padding=r // 2 + r % 2,
                                               output_padding=r % 2)]
            for j in range(n_residual_layers - 1, -1, -1):
                encoder_block = [ResnetBlock(mult * ngf // 2, dilation=3 ** j)] + encoder_block
            for j in range(n_residual_layers):
                decoder_block += [ResnetBlock(mult * ngf // 2, dilation=3 ** j)]
            mult //= 2
            self.encoder.insert(0, nn.Sequential(*encoder_block))
            self.decoder.append(nn.Sequential(*decoder_block))
        self.encoder.insert(0, nn.Sequential(nn.ReflectionPad1d(3), WNConv1d(in_channels, ngf, kernel_size=7, padding=0), nn.Tanh()))
        self.decoder.append(nn.Sequential(nn.LeakyReLU(SLOPE), nn.ReflectionPad1d(3), WNConv1d(ngf, out_channels, kernel_size=7, padding=0),
                                          nn.Tanh()))
        self.apply(weights_init)
        self._tables = {}

    # ------------------------------------------------------------------ host arithmetic (seanet.py:123-151)
    def estimate_output_length(self, length):
        """the nearest valid length: no time step left over in any strided conv (integer-exact)"""
        length = int(length)
        for stride in reversed(self.ratios):
            padding = stride // 2 + stride % 2
            length = max(-((2 * stride - 2 * padding - length) // stride) + 1, 1)      # ceil((length - 2 stride + 2 padding) / stride) + 1
        for stride in self.ratios:
            padding = stride // 2 + stride % 2
            length = (length - 1) * stride + 2 * stride - 2 * padding + stride % 2
        return int(length)

    def pad_to_valid_length(self, signal):
        padding_len = self.estimate_output_length(signal.shape[-1]) - signal.shape[-1]
        return torch.nn.functional.pad(signal, (0, padding_len)), padding_len

    # ------------------------------------------------------------------ library, packed weights
    def use_library(self, lib):
        """tests: an explicitly loaded library (the CPU-emulated test double)"""
        self._ops = Ops(lib)

    def _get_ops(self):
        if self._ops is None:
            self._ops = Ops(_lib.load())
        return self._ops

    def repack(self):
        self._key = None

    def _weight(self, conv, dev):
        """w = g v / |v| (fp32, aero_weightnorm_fwd)"""
        ops = self._get_ops()
        v, g = conv.weight_v.detach().float().contiguous(), conv.weight_g.detach().float().contiguous()
        w = torch.empty_like(v)
        ops.lib.call('aero_weightnorm_fwd', _ptr(v), _ptr(g), _ptr(w), v.shape[0], v[0].numel(), ops.stream(w))
        return w

    def _conv_entry(self, conv, dev, in_slope, reflect_pad, act):
        w = self._weight(conv, dev)
        bias = conv.bias.detach().float().contiguous()
        if isinstance(conv, nn.ConvTranspose1d):
            Cin, Cout, K = w.shape
            r, = conv.stride
            if K != 2 * r or conv.dilation != (1,) or reflect_pad:
                raise NotImplementedError('Seanet: ConvTranspose1d with kernel_size = 2 stride only')
            wt = w.permute(2, 1, 0)                               # [2 r][Cout][Cin]
            wm = torch.stack([wt[r:], wt[:r]], 2).reshape(r * Cout, 2 * Cin)      # tap 0 = x[q - 1] (k = ph + r), tap 1 = x[q] (k = ph)
            return dict(kind='conv', transposed=True, Cin=Cin, Cout=Cout, K=2, stride=1, dil=1, pad=1, reflect=0, R=r, P=conv.padding[0],
                        opad=conv.output_padding[0], img=mfma_image(wm, dev), bias=bias.repeat(r).contiguous(), in_slope=in_slope, act=act)
        Cout, Cin, K = w.shape
        if conv.groups != 1:
            raise NotImplementedError('Seanet: grouped convs are not part of the model')
        if Cin == 1 or Cout == 1:
            if K != 7 or reflect_pad != 3 or conv.stride != (1,) or conv.dilation != (1,) or act != 1 or in_slope != (1.0 if Cin == 1 else SLOPE):
                raise NotImplementedError('Seanet: the 1-channel convs are the k = 7 reflect-padded tanh convs at the waveform ends')
            w16 = w.to(torch.float16)
            if Cin == 1:
                return dict(kind='conv_in', Cout=Cout, w=w16.float().reshape(Cout, 7).contiguous(), bias=bias)
            return dict(kind='conv_out', Cin=Cin, w=w16[0].t().contiguous(), bias=bias)             # [7][C]
        wm = w.permute(0, 2, 1).reshape(Cout, K * Cin)            # column k Cin + c
        return dict(kind='conv', transposed=False, Cin=Cin, Cout=Cout, K=K, stride=conv.stride[0], dil=conv.dilation[0],
                    pad=reflect_pad if reflect_pad else conv.padding[0], reflect=1 if reflect_pad else 0, R=1, P=0, img=mfma_image(wm, dev),
                    bias=bias, in_slope=in_slope, act=act)

    def _stage_entries(self, seq, dev):
        """the kernels of one nn.Sequential: activations and paddings fold into the conv that follows (LeakyReLU, ReflectionPad1d) or
        precedes (Tanh) them"""
        ents, slope, rpad = [], 1.0, 0
        mods = list(seq)
        for i, m in enumerate(mods):
            if isinstance(m, nn.LeakyReLU):
                slope = float(m.negative_slope)
            elif isinstance(m, nn.ReflectionPad1d):
                rpad = int(m.padding[0])
            elif isinstance(m, nn.Tanh):
                pass                                              # (taken by the conv in front of it, below)
            elif isinstance(m, ResnetBlock):
                if slope != 1.0 or rpad:
                    raise NotImplementedError('Seanet: an activation or padding in front of a ResnetBlock')
                c1, c2, cs = m.block[2], m.block[4], m.shortcut
                e1 = self._conv_entry(c1, dev, SLOPE, m.dilation, 0)
                e2 = self._conv_entry(c2, dev, SLOPE, 0, 0)
                es = self._conv_entry(cs, dev, 1.0, 0, 0)
                w2s = torch.cat([self._weight(c2, dev)[:, :, 0], self._weight(cs, dev)[:, :, 0]], 1)
                ents.append(dict(kind='res', C=e1['Cin'], d=m.dilation, w1=e1['img'], w2s=mfma_image(w2s, dev), b1=e1['bias'],
                                 b2s=(e2['bias'] + es['bias']).contiguous(), parts=(es, e1, e2)))
            elif isinstance(m, (nn.Conv1d, nn.ConvTranspose1d)):
                act = 1 if i + 1 < len(mods) and isinstance(mods[i + 1], nn.Tanh) else 0
                ents.append(self._conv_entry(m, dev, slope, rpad, act))
                slope, rpad = 1.0, 0
            else:
                raise NotImplementedError(f'Seanet: no kernel for {type(m).__name__}')
        return ents

    def _pack(self, dev):
        dev = torch.device(dev)
        key = (str(dev),) + tuple((p.data_ptr(), p._version) for p in self.parameters())
        if key != self._key:
            self._packed = ([self._stage_entries(s, dev) for s in self.encoder], [self._stage_entries(s, dev) for s in self.decoder])
            self._key = key
        return self._packed

    # ------------------------------------------------------------------ launches
    def _conv(self, ops, e, h, T, add):
        """the general conv on h fp16 [B][T][Cin] -> (y fp16 [B][Tout][Cout], Tout)"""
        B = h.shape[0]
        if e['transposed']:
            r = e['R']
            Tq, Tout = T + 1, (T - 1) * r + 2 * r - 2 * e['P'] + e['opad']
        else:
            span = e['dil'] * (e['K'] - 1) + 1
            Tout = (T + 2 * e['pad'] - span) // e['stride'] + 1
            Tq = Tout
            if e['reflect'] and e['pad'] >= T:
                raise RuntimeError(f'Padding size should be less than the corresponding input dimension, but got: padding ({e["pad"]}, {e["pad"]}) '
                                   f'at dimension 2 of input [{B}, {e["Cin"]}, {T}]')
        if Tout < 1:
            raise RuntimeError(f'Seanet: a conv (kernel {e["K"]}, stride {e["stride"]}) has no output for {T} input steps')
        y = torch.empty(B, Tout, e['Cout'], dtype=torch.float16, device=h.device)
        if add is not None and add.shape != y.shape:
            raise ValueError(f'Seanet: skip {tuple(add.shape)} does not match the stage output {tuple(y.shape)}')
        d = _lib.SeanetConvDesc()
        d.x, d.wimg, d.bias, d.add, d.y = _ptr(h), _ptr(e['img']), _ptr(e['bias']), _ptr(add), _ptr(y)
        d.B, d.Tin, d.Cin, d.Tq, d.M, d.K, d.stride, d.dil, d.pad = B, T, e['Cin'], Tq, e['R'] * e['Cout'], e['K'], e['stride'], e['dil'], e['pad']
        d.reflect, d.ksteps, d.R, d.P, d.Tout, d.Cout, d.act, d.in_slope = e['reflect'], (e['K'] * e['Cin'] + 31) // 32, e['R'], e['P'], Tout, e['Cout'], e['act'], e['in_slope']
        ops.lib.call('aero_seanet_conv', C.byref(d), ops.stream(y))
        return y, Tout

    def _res(self, ops, e, h, T, add, fuse):
        B, Cc = h.shape[0], e['C']
        if e['d'] >= T:
            raise RuntimeError(f'Padding size should be less than the corresponding input dimension, but got: padding ({e["d"]}, {e["d"]}) '
                               f'at dimension 2 of input [{B}, {Cc}, {T}]')
        if not fuse:
            es, e1, e2 = e['parts']
            s, _ = self._conv(ops, es, h, T, add)
            hid, _ = self._conv(ops, e1, h, T, None)
            return self._conv(ops, e2, hid, T, s)
        y = torch.empty(B, T, Cc, dtype=torch.float16, device=h.device)
        d = _lib.SeanetResDesc()
        d.x, d.w1, d.w2s, d.b1, d.b2s, d.add, d.y = _ptr(h), _ptr(e['w1']), _ptr(e['w2s']), _ptr(e['b1']), _ptr(e['b2s']), _ptr(add), _ptr(y)
        d.B, d.T, d.C, d.d, d.ks1, d.ks2, d.slope = B, T, Cc, e['d'], (3 * Cc + 31) // 32, (2 * Cc + 31) // 32, SLOPE
        ops.lib.call('aero_seanet_resblock', C.byref(d), ops.stream(y))
        return y, T

    def _table(self, dev):
        key = (self.lr_sr, self.hr_sr, str(dev))
        if key not in self._tables:
            k, og, nw, width = resample_table(self.lr_sr, self.hr_sr)
            self._tables[key] = (k.to(dev), og, nw, width)
        return self._tables[key]

    def _forward(self, signal, stages=None):
        ops = self._get_ops()
        if not signal.is_cuda and not ops.lib.is_emulator:
            raise RuntimeError('aero_amd.seanet runs on the MI355X: move the signal to "cuda"')
        if signal.dim() != 3 or signal.shape[1] != 1:
            raise ValueError('expected a [B, 1, T] waveform')
        fuse = os.environ.get('AERO_SEANET_FUSE', '1') != '0'
        dev = signal.device
        enc, dec = self._pack(dev)
        B, L = signal.shape[0], signal.shape[2]
        x = signal.detach().reshape(B, L).float().contiguous()
        target_len = L * self.scale_factor if self.upsample else L
        stats = None
        if self.normalize:
            stats = torch.empty(B, 2, dtype=torch.float32, device=dev)
            ops.lib.call('aero_seanet_stats', _ptr(x), B, L, C.c_float(self.floor), _ptr(stats), ops.stream(x))
        table, og, nw, width, Lup = None, 1, 1, 0, L
        if self.upsample and int(self.lr_sr) != int(self.hr_sr):
            table, og, nw, width = self._table(dev)
            Lup = -((-nw * L) // og)
        T = self.estimate_output_length(Lup)
        x0 = torch.empty(B, T, dtype=torch.float32, device=dev)
        ops.lib.call('aero_seanet_front', _ptr(x), _ptr(stats), _ptr(table), _ptr(x0), B, L, Lup, T, og, nw, width, ops.stream(x0))
        h, skips, out = x0, [], None
        for stage in enc:
            skips.append((h, T))
            for e in stage:
                if e['kind'] == 'conv_in':
                    if T < 4:
                        raise RuntimeError(f'Padding size should be less than the corresponding input dimension, but got: padding (3, 3) at '
                                           f'dimension 2 of input [{B}, 1, {T}]')
                    y = torch.empty(B, T, e['Cout'], dtype=torch.float16, device=dev)
                    ops.lib.call('aero_seanet_conv_in', _ptr(h), _ptr(e['w']), _ptr(e['bias']), _ptr(y), B, T, e['Cout'], ops.stream(y))
                    h = y
                elif e['kind'] == 'res':
                    h, T = self._res(ops, e, h, T, None, fuse)
                else:
                    h, T = self._conv(ops, e, h, T, None)
            if stages is not None:
                stages.append(h.transpose(1, 2))
        for stage in dec:
            skip, Ts = skips.pop()
            for i, e in enumerate(stage):
                add = skip if i == len(stage) - 1 else None
                if e['kind'] == 'conv_out':
                    if Ts != T:
                        raise ValueError(f'Seanet: the input skip has {Ts} steps, the decoder output {T}')
                    if T < 4:
                        raise RuntimeError(f'Padding size should be less than the corresponding input dimension, but got: padding (3, 3) at '
                                           f'dimension 2 of input [{B}, {e["Cin"]}, {T}]')
                    Tout = min(target_len, T)
                    out = torch.empty(B, 1, Tout, dtype=torch.float32, device=dev)
                    ops.lib.call('aero_seanet_conv_out', _ptr(h), _ptr(e['w']), _ptr(e['bias']), _ptr(add), _ptr(stats), _ptr(out), B, T, e['Cin'],
                                 Tout, C.c_float(SLOPE), ops.stream(out))
                elif e['kind'] == 'res':
                    h, T = self._res(ops, e, h, T, add, fuse)
                else:
                    h, T = self._conv(ops, e, h, T, add)
            if stages is not None:
                stages.append(out if out is not None else h.transpose(1, 2))
        return out

    def forward(self, signal):
        """seanet.py:153-179: [B, 1, L] -> [B, 1, L * scale] (fp32, no graph)"""
        if self.training and torch.is_grad_enabled():
            raise NotImplementedError('Seanet: the backward pass is not built on the MI355X -- inference only (call .eval(), or run the '
                                      'training-mode forward under torch.no_grad())')
        return self._forward(signal)

    def forward_stages(self, signal):
        """(output, [what follows each encoder stage, then each decoder stage with its skip added]) as [B, C, T] views: the last one is the
        output itself (skip added, trimmed and scaled by std)"""
        stages = []
        return self._forward(signal, stages), stages
