"""HiFi-GAN multi-period discriminator on the MI355X (reference src/models/discriminators.py:85-147 `DiscriminatorP` /
`MultiPeriodDiscriminator`, the critic `mpd` of solver.py:457-463,580-600; its losses discriminators.py:210-243).

Same constructor arguments, module tree and state-dict keys (`discriminators.{i}.convs.{0..4}.{bias, weight_g, weight_v}`,
`discriminators.{i}.conv_post.*`: weight-normed nn.Conv2d), same RNG draws at construction (default Conv2d init, then weight norm), so a
seed reproduces the reference's initial weights and reference checkpoints load unchanged.

Every FLOP runs on the HIP kernels.  Column j of clip b of the period-p view [B, 1, H, p] is item b p + j of a channels-last row signal
[B p][rows][C] (include/aero_hip.h, aero_mpd_*), so each (5, 1) conv is a Conv1d over the rows:
  * fold (reflect pad + columns + fp16) and its adjoint: aero_mpd_fold / aero_mpd_unfold_add;
  * conv 0 (1 -> hidden, stride 3): aero_mpd_conv0_fwd / _bwd;
  * convs 1-3 (stride 3) on the MFMA conv family as STRIDE-1, 2-TAP convs over 3 C channels: rows [H][C] are the memory of [H / 3][3 C], so
    y[o] = sum_k w_k x[3 o + k - 2] reads taps dt = -1 (phases 1, 2 = k 0, 1) and dt = 0 (phases 0, 1, 2 = k 2, 3, 4) -- one zero weight
    block, 6/5 of the FLOPs.  The producer of such an input stores 3 ceil(H / 3) rows with a zero tail (aero_mpd_act).  The data gradient
    is again a stride-1 conv (taps dt = 0, +1, 3 C output channels) written straight into the input's [H][C] layout; the weight gradient
    is aero_conv_wgrad of the same 2-tap form (slabs added in a fixed order) with the unused phase-0 block of tap -1 dropped;
  * conv 4 (stride 1) as a 5-tap conv on the same family; conv_post (-> 1 channel) on aero_gconv1d_fwd / _bwd;
  * LeakyReLU(0.1) behind the MFMA convs: aero_mpd_act; its derivative: aero_loss_grad mode 2; weight norm: aero_weightnorm_fwd / _bwd;
  * least-squares losses: aero_loss_sum mode 2 / aero_loss_grad mode 3; feature matching: modes 1.
The cached D(fake) || D(real) pair, the critic's own step and the delivery of its gradients: aero_amd/critic.py."""
import ctypes as C

import torch
from torch import nn
from torch.nn.utils import weight_norm

from . import _lib, pack
from .critic import HipCritic, _loss_sum, _scaled_grad, _upstream
from .engine import _ptr, _strides4
from .modules import capture_init

LRELU_SLOPE = 0.1                                                # discriminators.py:12


class DiscriminatorP(nn.Module):
    """discriminators.py:89-100 (parameters only; the forward is MultiPeriodDiscriminator's)"""

    @capture_init
    def __init__(self, period, kernel_size=5, stride=3, use_spectral_norm=False, hidden=32):
        super().__init__()
        if kernel_size != 5 or stride != 3 or use_spectral_norm:
            raise NotImplementedError('DiscriminatorP: the HIP critic implements kernel_size 5, stride 3 and weight norm (what '
                                      'MultiPeriodDiscriminator builds)')
        self.period = period
        self.convs = nn.ModuleList([
            weight_norm(nn.Conv2d(1, hidden, (5, 1), (3, 1), padding=(2, 0))),
            weight_norm(nn.Conv2d(hidden, hidden * 4, (5, 1), (3, 1), padding=(2, 0))),
            weight_norm(nn.Conv2d(hidden * 4, hidden * 16, (5, 1), (3, 1), padding=(2, 0))),
            weight_norm(nn.Conv2d(hidden * 16, hidden * 32, (5, 1), (3, 1), padding=(2, 0))),
            weight_norm(nn.Conv2d(hidden * 32, hidden * 32, (5, 1), 1, padding=(2, 0))),
        ])
        self.conv_post = weight_norm(nn.Conv2d(hidden * 32, 1, (3, 1), 1, padding=(1, 0)))

    def layers(self):
        return list(self.convs) + [self.conv_post]

    def forward(self, x):  # pragma: no cover
        raise RuntimeError('run the critic through MultiPeriodDiscriminator (HIP kernels)')


def _rows3(h):
    """rows stored for an input of a stride-3 layer: 3 ceil(h / 3)"""
    return 3 * ((h + 2) // 3)


def stride3_images(w, bias, dev):
    """w fp32 [M, C, 5] (weight norm applied) of a (5, 1) / stride (3, 1) / padding (2, 0) conv -> (forward spec: the 2-tap conv over 3 C
    channels, taps dt = -1, 0; data-gradient spec: 3 C output channels from M, taps dt = 0, +1)"""
    M, Cc, K = w.shape
    t = torch.zeros(M, 2, 3, Cc, dtype=torch.float32, device=w.device)
    t[:, 0, 1], t[:, 0, 2] = w[:, :, 0], w[:, :, 1]               # tap -1: x[3 o - 2], x[3 o - 1] = phases 1, 2 of row o - 1
    t[:, 1, 0], t[:, 1, 1], t[:, 1, 2] = w[:, :, 2], w[:, :, 3], w[:, :, 4]
    fwd = pack.make_conv_spec(t.reshape(1, M, 2, 3 * Cc), bias, 3 * Cc, 0, [0, 0], [-1, 0], dev)
    wt = w.permute(1, 2, 0)                                        # [C, 5, M]
    d = torch.zeros(3, Cc, 2, M, dtype=torch.float32, device=w.device)
    for ph in range(3):
        d[ph, :, 0] = wt[:, ph + 2]                                # dx[3 o + ph] <- dy[o] through k = ph + 2
        if ph:
            d[ph, :, 1] = wt[:, ph - 1]                            #              <- dy[o + 1] through k = ph - 1
    dgrad = pack.make_conv_spec(d.reshape(1, 3 * Cc, 2, M), None, M, 0, [0, 0], [0, 1], dev)
    return fwd, dgrad


class MultiPeriodDiscriminator(HipCritic):
    # discriminators.py:222-233: sum over periods of mean(D(fake)^2) + mean((1 - D(real))^2): (sign, mode) of aero_loss_sum, of aero_loss_grad
    _loss_terms, _grad_terms = ((0.0, 2), (1.0, 2)), ((0.0, 3), (1.0, 3))

    @capture_init
    def __init__(self, hidden=32, periods=[2, 3, 5, 7, 11]):   # noqa: B006 (the reference's signature)
        super().__init__()
        if not isinstance(hidden, int) or hidden % 8 or not 8 <= hidden <= 64:
            raise NotImplementedError(f'mpd hidden={hidden}: multiples of 8 from 8 to 64 -- the MFMA convs need 8-channel multiples, and '
                                      f'widths above 64 (conv 3 / 4 with more than 2048 output channels) have not been run on these kernels')
        if any(int(p) != p or p < 1 for p in periods):
            raise ValueError(f'periods must be positive integers: {periods}')
        self.hidden = hidden
        self.discriminators = nn.ModuleList([DiscriminatorP(period, hidden=hidden) for period in periods])

    def _pack(self, dev):
        """weight norm of every conv (one launch each into a flat fp32 buffer), then the kernels' images of those weights"""
        dev, key = self._pack_key(dev)
        if key == self._key:
            return self._packed
        # a FRESH buffer per pack: an older record (a cached pair whose backward has not run yet) keeps views of the weights it was
        # computed with (conv 0's data gradient reads them), so they must not be rewritten in place under it
        ws = iter(self._weightnorm_fwd([conv for d in self.discriminators for conv in d.layers()], dev)[1])
        packed = []
        for d in self.discriminators:
            ents = []
            for j, conv in enumerate(d.layers()):
                w = next(ws)
                Cout, Cin, K = w.shape
                b = conv.bias.detach().float().contiguous()
                ent = dict(j=j, Cin=Cin, Cout=Cout, K=K, w=w, bias=b)
                if j == 0:
                    ent['kind'] = 'c0'
                elif j <= 3:
                    ent['kind'] = 's3'
                    ent['spec'], ent['dspec'] = stride3_images(w, b, dev)
                elif j == 4:
                    from . import backward as bw
                    ent['kind'] = 's1'
                    taps, df, dt = pack.conv1d_taps(w, 1, 2)
                    ent['spec'] = pack.make_conv_spec(taps, b, Cin, 0, df, dt, dev)
                    ent['dspec'] = bw.dgrad_conv1d(w, 1, 2, dev)
                else:
                    ent['kind'] = 'post'
                    ent['w16'] = w.permute(0, 2, 1).contiguous().to(torch.float16)            # [1][3][C]
                ents.append(ent)
            packed.append((d.period, ents))
        self._packed, self._key = packed, key
        return packed

    def _run(self, x):
        """x [Bt, 1, L] -> per period: dict(p, L, H, n = Bt, xf fp16 [Bt p][H], ys = [(entry, output fp16 [Bt p][rows][C], valid rows)])"""
        self._check_input(x)
        ops = self._get_ops()
        dev = x.device
        packed = self._pack(dev)
        Bt, L = x.shape[0], x.shape[2]
        x32 = x.detach().reshape(Bt, L).float().contiguous()
        out = []
        for p, ents in packed:
            if L < p:
                raise ValueError(f'signal of {L} samples is shorter than the period {p} (reflect padding)')
            H = (L + p - 1) // p
            N = Bt * p
            xf = torch.empty(N, H, dtype=torch.float16, device=dev)
            ops.lib.call('aero_mpd_fold', _ptr(x32), Bt, L, p, _ptr(xf), ops.stream(xf))
            ys, h, Hc = [], xf, H
            for ent in ents:
                kind, M = ent['kind'], ent['Cout']
                if kind == 'c0':
                    Ho = (Hc + 2) // 3
                    y = torch.empty(N, _rows3(Ho), M, dtype=torch.float16, device=dev)
                    ops.lib.call('aero_mpd_conv0_fwd', _ptr(h), _ptr(ent['w']), _ptr(ent['bias']), _ptr(y), N, Hc, M, y.shape[1],
                                 C.c_float(LRELU_SLOPE), ops.stream(y))
                elif kind in ('s3', 's1'):
                    if kind == 's3':
                        Ho = (Hc + 2) // 3
                        src = h.view(N, 1, Ho, 3 * ent['Cin'])             # (h holds 3 Ho rows, the tail zero)
                        rows = _rows3(Ho) if ent['j'] < 3 else Ho          # the next layer is stride-3 again (convs 1, 2) or not (conv 3)
                    else:
                        Ho = Hc
                        src = h[:, :Hc].view(N, 1, Hc, ent['Cin'])
                        rows = Ho
                    y = torch.empty(N, rows, M, dtype=torch.float16, device=dev)
                    ops.conv(ent['spec'], src, None, N, 1, 1, Ho, dst=y.view(N, 1, rows, M))
                    ops.lib.call('aero_mpd_act', _ptr(y), N, Ho, rows, M, C.c_float(LRELU_SLOPE), ops.stream(y))
                else:
                    Ho = Hc
                    y = torch.empty(N, Ho, 1, dtype=torch.float16, device=dev)
                    d = _lib.GconvDesc()
                    d.x, d.w, d.bias, d.y = _ptr(h), _ptr(ent['w16']), _ptr(ent['bias']), _ptr(y)
                    d.B, d.Tin, d.Cin, d.Cout, d.groups, d.K, d.stride, d.pad, d.reflect = N, Hc, ent['Cin'], 1, 1, 3, 1, 1, 0
                    d.slope = 1.0
                    ops.lib.call('aero_gconv1d_fwd', C.byref(d), ops.stream(y))
                ys.append((ent, y, Ho))
                h, Hc = y, Ho
            out.append(dict(p=p, L=L, H=H, n=Bt, xf=xf, ys=ys))
        return out

    @staticmethod
    def _half(runs, lo, hi):
        """the record of clips [lo, hi) of a run (views)"""
        out = []
        for r in runs:
            p = r['p']
            out.append(dict(r, n=hi - lo, xf=r['xf'][lo * p:hi * p], ys=[(e, y[lo * p:hi * p], Ho) for (e, y, Ho) in r['ys']]))
        return out

    @staticmethod
    def _maps(r, lo, hi):
        """feature maps of clips [lo, hi) in the reference's layout [B, C, H, p] (views) and the logits [B, H p] (discriminators.py:117-123)"""
        p, nb = r['p'], hi - lo
        fm = [y[lo * p:hi * p, :Ho].view(nb, p, Ho, e['Cout']).permute(0, 3, 2, 1) for (e, y, Ho) in r['ys']]
        return fm, fm[-1].reshape(nb, -1)

    def forward(self, y, y_hat):
        """discriminators.py:131-147: (y_d_rs, y_d_gs, fmap_rs, fmap_gs) for real y and generated y_hat ([B, 1, T] on the device); values
        (fp16), without a graph -- the differentiable entry points are `discriminator_loss` and `generator_losses`"""
        runs, B = self._run_pair(y_hat, y)
        y_d_rs, y_d_gs, fmap_rs, fmap_gs = [], [], [], []
        for r in runs:
            fg, lg = self._maps(r, 0, B)
            fr, lr = self._maps(r, B, 2 * B)
            y_d_rs.append(lr)
            y_d_gs.append(lg)
            fmap_rs.append(fr)
            fmap_gs.append(fg)
        return y_d_rs, y_d_gs, fmap_rs, fmap_gs

    # ------------------------------------------------------------------ losses with their HIP backward (solver.py:580-600)
    def _logit_heads(self, runs, B):
        """per period: (logits of the 2B batch fp16 [2B p][H4][1], rows of D(fake))"""
        return [(r['ys'][-1][1], B * r['p']) for r in runs]

    def generator_losses(self, fake, real, features_loss_lambda=100.0):
        """solver.py:587-600: (adversarial = sum over periods of mean((1 - D(fake))^2), lambda * feature matching = lambda * the mean over
        every (period, layer) pair -- the logits included -- of mean |D(real) - D(fake)|); differentiable w.r.t. `fake`"""
        return _MPDGeneratorLoss.apply(self, fake, real.detach(), float(features_loss_lambda))

    def _backward(self, runs, dtop, dfeat, want_params, want_input, out=None, gl=None, L=None):
        """runs: record (or half of one); dtop[i]: (gradient of period i's logits fp16 [n p][H4][1], {S, 1/S}); dfeat[i][j]: the same for
        feature map j < 5 (the layer's stored buffer) or None.  Returns ({parameter name: fp32 gradient}, d waveform fp32 [n, L] or None).
        out: {name: fp32 destination} the gradients are ADDED to; gl: 0-dim fp32 device tensor, the upstream factor of the loss."""
        from . import backward as bw
        ops = self._get_ops()
        grads = {}
        dwave = None
        for i, r in enumerate(runs):
            p, n, H, ys = r['p'], r['n'], r['H'], r['ys']
            N = n * p
            dev = r['xf'].device
            if want_input and dwave is None:
                dwave = torch.zeros(n, r['L'], dtype=torch.float32, device=dev)
            disc = self.discriminators[i]
            g, sc = dtop[i]
            dx = None
            for j in reversed(range(len(ys))):
                ent, y, Ho = ys[j]
                h = ys[j - 1][1] if j else r['xf']
                Hin = ys[j - 1][2] if j else H
                kind, M, Cin = ent['kind'], ent['Cout'], ent['Cin']
                need_dx = want_input or j > 0
                if j < len(ys) - 1:
                    g, sc = self._join_feature_grad(dx, sc, dfeat, i, j)
                prefix = f'discriminators.{i}.' + (f'convs.{j}.' if j < 5 else 'conv_post.')
                if kind == 'post':
                    d = _lib.GconvBwdDesc()
                    dx = torch.empty(N, Hin, Cin, dtype=torch.float16, device=dev) if need_dx else None
                    # the weight gradient: the edge kernel's slab form where it takes the width (C a multiple of 512: hidden 16, 32, 64),
                    # else aero_conv_wgrad as a 3-tap conv (slabs as well) -- never the VALU kernel's fp32 atomics (run-to-run order)
                    nsl = ops.lib.cdll.aero_gconv1d_wgrad_slabs(N, Hin, Cin, 1, 1, 3, 1, 1, 0) if want_params else 0
                    edge_wg = want_params and nsl > 0
                    if edge_wg:
                        dwk = torch.zeros(1, 3, Cin, dtype=torch.float32, device=dev)
                        db = torch.zeros(4, dtype=torch.float32, device=dev)[:1]              # (room for a float4)
                        slabs = torch.empty(nsl, 3 * Cin + 4, dtype=torch.float32, device=dev)
                        d.slabs, d.nslab = _ptr(slabs), nsl
                    d.x, d.w, d.y, d.dy, d.dx = _ptr(h), _ptr(ent['w16']), _ptr(y), _ptr(g), _ptr(dx)
                    d.dw, d.db = (_ptr(dwk), _ptr(db)) if edge_wg else (None, None)
                    d.B, d.Tin, d.Cin, d.Cout, d.groups, d.K, d.stride, d.pad, d.reflect = N, Hin, Cin, 1, 1, 3, 1, 1, 0
                    d.slope = 1.0
                    if need_dx or edge_wg:
                        ops.lib.call('aero_gconv1d_bwd', C.byref(d), ops.stream(g))
                    dw_strides = (3 * Cin, 1, Cin)                                   # [Cout, K, C]: element (o, c, k)
                    if want_params and not edge_wg:
                        dwk, db = bw.conv_wgrad(ops, g.view(N, 1, Hin, 1), h.view(N, 1, Hin, Cin), [0, 0, 0], [-1, 0, 1])   # [3][1][C]
                        dw_strides = (Cin, 1, Cin)
                else:
                    dyp = torch.empty_like(g)
                    ops.lib.call('aero_loss_grad', _ptr(g), _ptr(y), g.numel(), C.c_float(0.0), C.c_float(LRELU_SLOPE), 2, _ptr(dyp), None,
                                 ops.stream(g))
                    if kind == 'c0':
                        dxf = torch.empty(N, H, dtype=torch.float32, device=dev) if want_input else None
                        if want_params:
                            nsl = ops.lib.cdll.aero_mpd_conv0_slabs(N, H)
                            slabs = torch.empty(nsl, 6 * M, dtype=torch.float32, device=dev)
                            dwk = torch.empty(M, 5, dtype=torch.float32, device=dev)
                            db = torch.empty(M, dtype=torch.float32, device=dev)
                        ops.lib.call('aero_mpd_conv0_bwd', _ptr(dyp), _ptr(h), _ptr(ent['w']), sc[1:].data_ptr(), _ptr(dxf),
                                     _ptr(slabs) if want_params else None, nsl if want_params else 0, _ptr(dwk) if want_params else None,
                                     _ptr(db) if want_params else None, N, H, M, dyp.shape[1], ops.stream(dyp))
                        if want_input:
                            ops.lib.call('aero_mpd_unfold_add', _ptr(dxf), n, r['L'], p, _ptr(dwave), ops.stream(dxf))
                        dx = None
                        dw_strides = (5, 0, 1)
                    elif kind == 's3':
                        dy4 = dyp.view(N, 1, dyp.shape[1], M)[:, :, :Ho]
                        x4 = h.view(N, 1, Ho, 3 * Cin)
                        if want_params:
                            dw2, db = bw.conv_wgrad(ops, dy4, x4, [0, 0], [-1, 0])     # [2][M][3 C]; phases 1, 2 of tap -1 = k 0, 1
                            dwk = torch.stack([dw2[0, :, Cin:2 * Cin], dw2[0, :, 2 * Cin:], dw2[1, :, :Cin], dw2[1, :, Cin:2 * Cin],
                                               dw2[1, :, 2 * Cin:]], -1).contiguous()          # [M][C][5]
                            dw_strides = (5 * Cin, 5, 1)
                        dx = None
                        if need_dx:
                            dx = ops.conv(ent['dspec'], dy4, None, N, 1, 1, Ho, src0_strides=_strides4(dy4)).view(N, 3 * Ho, Cin)
                            if Hin < 3 * Ho:                 # rows Hin.. are the gradient of the zero padding: zeroed, so that they do not
                                ops.lib.call('aero_mpd_act', _ptr(dx), N, Hin, 3 * Ho, Cin, C.c_float(1.0), ops.stream(dx))   # set the fp16 scale
                    else:
                        dy4 = dyp.view(N, 1, Ho, M)
                        if want_params:
                            spec = ent['spec']
                            dwk, db = bw.conv_wgrad(ops, dy4, h[:, :Hin].reshape(N, 1, Hin, Cin), spec.df, spec.dt)   # [5][M][C]
                            dw_strides = (Cin, 1, M * Cin)
                        dx = ops.conv(ent['dspec'], dy4, None, N, 1, 1, Ho).view(N, Hin, Cin) if need_dx else None
                if want_params:
                    grads.update(self._weightnorm_bwd(disc.layers()[j], prefix, dwk, dw_strides, db, sc, gl, out))
        return grads, dwave


class _MPDGeneratorLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, disc, fake, real, lam):
        ops = disc._get_ops()
        runs, B = disc._run_pair(fake, real)
        rf, rr = disc._half(runs, 0, B), disc._half(runs, B, 2 * B)
        npairs = sum(len(r['ys']) for r in rf)
        acc = torch.zeros(2, dtype=torch.float64, device=fake.device)        # {adversarial, lambda * feature matching}
        for a, b in zip(rf, rr):
            lg = a['ys'][-1][1]
            _loss_sum(ops, lg, None, 1.0, 2, acc[0:1], 1.0 / lg.numel())
            for (e, ya, Ho), (_, yb, _) in zip(a['ys'], b['ys']):
                nvalid = a['n'] * a['p'] * Ho * e['Cout']                     # (rows past Ho are zero in both: no contribution)
                _loss_sum(ops, ya, yb, 0.0, 1, acc[1:2], lam / (npairs * nvalid))
        ctx.disc, ctx.runs, ctx.cfg, ctx.shape = disc, (rf, rr), (lam, npairs), fake.shape
        out = acc.float()
        return out[0], out[1]

    @staticmethod
    def backward(ctx, gadv, gfeat):
        from . import train_ops as TO
        disc, ops = ctx.disc, ctx.disc._get_ops()
        rf, rr = ctx.runs
        lam, npairs = ctx.cfg
        ga, gf = _upstream(gadv), _upstream(gfeat)
        dtop = [_scaled_grad(ops, a['ys'][-1][1], None, a['ys'][-1][1].numel(), 1.0, 1.0, 3, gl=ga) for a in rf]
        dfeat = [[_scaled_grad(ops, ya, yb, a['n'] * a['p'] * Ho * e['Cout'], 0.0, lam / npairs, 1, gl=gf)
                  for (e, ya, Ho), (_, yb, _) in zip(a['ys'][:-1], b['ys'][:-1])] + [None] for a, b in zip(rf, rr)]
        # the logits' own feature-matching term joins their adversarial gradient
        for i, (a, b) in enumerate(zip(rf, rr)):
            e, ya, Ho = a['ys'][-1]
            fl = _scaled_grad(ops, ya, b['ys'][-1][1], a['n'] * a['p'] * Ho, 0.0, lam / npairs, 1, gl=gf)
            dtop[i] = TO.rescale_f16(ops, dtop[i][0], dtop[i][1], fl[0], fl[1])
        _, dx = disc._backward(rf, dtop, dfeat, False, True)
        ctx.runs = None
        return None, dx.view(ctx.shape), None, None


def mpd_losses(disc, fake, real, features_loss_lambda=100.0):
    """discriminators.py:210-243 / solver.py:580-600 on the critic's HIP outputs (values, no graph): (critic loss, generator adversarial
    loss, lambda * feature matching) as 0-dim device tensors for real / generated signals [B, 1, T]"""
    with torch.no_grad():
        d = disc.discriminator_loss(fake, real)
        adv, feat = disc.generator_losses(fake, real, features_loss_lambda)
    return d, adv, feat

