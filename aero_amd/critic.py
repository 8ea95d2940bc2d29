"""What the HIP critics (discriminators.Discriminator, mpd.MultiPeriodDiscriminator) share: how a critic caches its D(fake) || D(real)
pair, takes its losses and delivers its gradients.

  * `HipCritic`: the library handle, the pack key, the cached pair (`_run_pair`), the weight-norm launches in both directions and the
    join of a feature map's gradient into the layer walk;
  * `CriticLoss`: the critic's own loss (solver.py:607-611) as ONE autograd function.  A critic supplies the (sign, mode) of its loss
    terms (`_loss_terms`, `_grad_terms`: fake, real) and its logits per head (`_logit_heads`); the backward writes into FlatAdam's flat
    gradient buffer where it may and, wrapped by `distrib.wrap`, averages over the ranks with one flat all-reduce (`_grad_sync`);
  * `_loss_sum`, `_scaled_grad`, `_scale_pair`: the loss kernels' host side.
The generator-side losses differ per critic (weights, feature sets) and live with the critics."""
import ctypes as C
import math

import torch
from torch import nn

from . import _lib, train_ops as TO
from .engine import Ops, _ptr
from .optim import flat_offsets


def _loss_sum(ops, a, b, sign, mode, out, weight=1.0):
    a = a.contiguous()
    b = None if b is None else b.contiguous()                    # (named: the buffers must outlive the call)
    n = a.numel()
    npart = min(1024, (n + 255) // 256)
    part = torch.empty(npart, dtype=torch.float64, device=a.device)
    ops.lib.call('aero_loss_sum', _ptr(a), _ptr(b), n, C.c_float(sign), mode, _ptr(part), npart, _ptr(out), C.c_double(weight), ops.stream(a))


def _scaled_grad(ops, a, b, n_mean, sign, coef, mode, out=None, gl=None):
    """gradient of coef * mean(...) as fp16 with a host-chosen power-of-two scale: returns (tensor, {S, 1/S} on the device)"""
    c = coef / n_mean
    S = 2.0 ** round(math.log2(32.0 / max(abs(c), 1e-30)))
    g = torch.empty(a.shape, dtype=torch.float16, device=a.device) if out is None else out
    assert a.is_contiguous() and g.is_contiguous() and (b is None or b.is_contiguous())
    ops.lib.call('aero_loss_grad', _ptr(a), _ptr(b), a.numel(), C.c_float(sign), C.c_float(c * S), mode, _ptr(g), _ptr(gl), ops.stream(a))
    return g, _scale_pair(S, a.device)


_SCALES = {}


def _scale_pair(S, dev):
    """{S, 1/S} on the device (cached: host-chosen powers of two, a handful of distinct values)"""
    key = (S, str(dev))
    if key not in _SCALES:
        _SCALES[key] = torch.tensor([S, 1.0 / S], dtype=torch.float32, device=dev)
    return _SCALES[key]


def _upstream(g):
    """an upstream loss factor (1 in solver.py:314-316) as a 0-dim fp32 tensor that stays on the device: the loss-gradient and weight-norm
    kernels multiply it in (a float() here would stall the host in the middle of a backward until the device had caught up)"""
    return g.detach().float().contiguous()


class HipCritic(nn.Module):
    """base of a critic whose forward and backward run on the HIP kernels.  A subclass has `_pack(dev)`, `_run(x)` (the record of a batch),
    `_backward(runs, dtop, dfeat, want_params, want_input, out=None, gl=None)` and, for `CriticLoss`, `_loss_terms`, `_grad_terms` and
    `_logit_heads(runs, B)`."""
    _supports_grad_sync = True                                   # distrib.wrap: the backward of `discriminator_loss` averages the gradients itself
    _ops, _packed, _key, _pair, _epoch = None, None, None, None, 0

    def repack(self):
        """the weights were edited behind autograd's version counters (FlatAdam's fused step): re-pack on the next forward"""
        self._pair = None
        self._epoch += 1

    def drop_record(self):
        """forget the cached D(fake) || D(real) pair (and let go of the signals and activations it keeps alive): after a pass that
        evaluates the losses without the critic's own step, e.g. validation, so that nothing of it is left for a training step to find"""
        self._pair = None

    def reset_pack(self):
        """forget the packed images AND how they are kept up to date (the gather replay compiled at the first weight change): the next
        forward builds them from the weights by their closures, as the first forward of a process does.  The Solver calls this at
        every epoch's start, so that an epoch begins from the same engine state whether its process ran the epoch before or loaded it."""
        self._pair, self._packed, self._key = None, None, None
        if hasattr(self, '_replay'):
            self._wflat, self._replay, self._builders = None, None, {}
        self._epoch += 1

    def use_library(self, lib):
        """tests: an explicitly loaded library (the CPU-emulated test double)"""
        self._ops = Ops(lib)

    def _get_ops(self):
        if self._ops is None:
            self._ops = Ops(_lib.load())
        return self._ops

    def _check_input(self, x):
        if not x.is_cuda and not self._get_ops().lib.is_emulator:
            raise RuntimeError(f'{type(self).__module__} runs on the MI355X: move the signals to "cuda"')
        if x.dim() != 3 or x.shape[1] != 1:
            raise ValueError('expected a [B, 1, T] waveform')

    def _weights_key(self):
        return tuple((p.data_ptr(), p._version) for p in self.parameters()) + (self._epoch,)

    def _pack_key(self, dev):
        """-> (the device with its index filled in, the key the packed images of the current weights are cached under)"""
        dev = torch.device(dev)
        if dev.type == 'cuda' and dev.index is None:
            dev = torch.device('cuda', torch.cuda.current_device())
        return dev, (str(dev),) + self._weights_key()

    def _weightnorm_fwd(self, convs, dev, wflat=None):
        """w = g v / |v| of every conv, one launch each into a flat fp32 buffer (`wflat`, or a new one): returns (the buffer, the weights as
        views [Cout, Cin / groups, K] of it; a Conv2d's (K, 1) kernel is a Conv1d's K)"""
        ops = self._get_ops()
        offs, n = flat_offsets(conv.weight_v.numel() for conv in convs)
        if wflat is None:
            wflat = torch.empty(n, dtype=torch.float32, device=dev)
        ws = []
        for conv, o in zip(convs, offs):
            v, g = conv.weight_v.detach(), conv.weight_g.detach()
            w = wflat[o:o + v.numel()].view(v.shape[:3])
            ops.lib.call('aero_weightnorm_fwd', _ptr(v.contiguous()), _ptr(g.contiguous()), _ptr(w), v.shape[0], v[0].numel(), ops.stream(w))
            ws.append(w)
        return wflat, ws

    def _run_pair(self, fake, real):
        """D(fake) and D(real) as ONE batch of 2B signals (the reference runs the critic twice per loss, solver.py:478-480,505-506: the
        same arithmetic per signal, half the launches), kept until the weights or the signals change: the critic's own step
        (solver.py:607-611) evaluates D on exactly the signals and weights the generator's adversarial / feature losses just used, so
        its forward pass is this record again.  Returns (record of the 2B batch, B)."""
        if fake.shape != real.shape:
            raise ValueError('fake and real must have the same shape')
        key = (fake.data_ptr(), fake._version, real.data_ptr(), real._version, tuple(fake.shape), str(fake.device)) + self._weights_key()
        if self._pair is None or self._pair[0] != key:
            # (the record keeps the two signals alive: while it is cached their memory cannot be recycled for other data at the same
            # address and version -- a key built from pointers alone would then hit a stale record, e.g. in a validation loop)
            self._pair = (key, self._run(torch.cat([fake.detach(), real.detach()], 0)), fake.detach(), real.detach())
        return self._pair[1], fake.shape[0]

    def _join_feature_grad(self, dx, sc, dfeat, i, j):
        """the gradient flowing into feature map j of head i: the layer walk's `dx` (scale pair `sc`) plus that map's own loss gradient
        dfeat[i][j] = (tensor, scale pair), if there is one, as fp16 under a fresh scale"""
        f = dfeat[i][j] if dfeat is not None else None
        return TO.rescale_f16(self._get_ops(), dx, sc, *(f or ()))

    def _weightnorm_bwd(self, conv, prefix, dwk, dw_strides, db, sc, gl, out):
        """weight norm (w = g v / |v| per output channel), the 1 / S of the fp16 gradient path and the upstream loss factor `gl` in ONE launch
        (aero_weightnorm_bwd) -- the same bookkeeping in torch ops was ~20 parameter-sized kernels per conv.  dwk: the gradient of w, its
        element (o, c, k) at strides `dw_strides`; db: the bias gradient.  out: {parameter name: fp32 destination} the gradients are ADDED
        to, or None: then they are returned as {parameter name: new tensor}."""
        ops = self._get_ops()
        v, g = conv.weight_v.detach(), conv.weight_g.detach()
        assert v.dtype == torch.float32 and v.is_contiguous() and g.is_contiguous()
        names3 = (prefix + 'weight_g', prefix + 'weight_v', prefix + 'bias')
        if out is not None:
            dst, acc = [out[n] for n in names3], 1
        else:
            dst, acc = [torch.empty_like(g), torch.empty_like(v), torch.empty(v.shape[0], dtype=torch.float32, device=v.device)], 0
        ops.lib.call('aero_weightnorm_bwd', _ptr(dwk), dw_strides[0], dw_strides[1], dw_strides[2], _ptr(v), _ptr(g), _ptr(db),
                     sc[1:].data_ptr(), _ptr(gl), _ptr(dst[0]), _ptr(dst[1]), _ptr(dst[2]), v.shape[0], v.shape[1], v[0, 0].numel(), acc,
                     ops.stream(v))
        return {} if acc else dict(zip(names3, dst))

    def discriminator_loss(self, fake, real):
        """the critic's own loss on D(real), D(fake.detach()) (solver.py:479,607-611), summed over the heads; differentiable w.r.t. the
        critic's parameters"""
        names, params = zip(*self.named_parameters())
        return CriticLoss.apply(self, names, fake.detach(), real.detach(), *params)


class CriticLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, disc, names, fake, real, *params):
        ops = disc._get_ops()
        runs, B = disc._run_pair(fake, real)
        (sf, mf), (sr, mr) = disc._loss_terms
        loss = torch.zeros(1, dtype=torch.float64, device=fake.device)
        for logits, nh in disc._logit_heads(runs, B):
            w = 1.0 / logits[:nh].numel()                        # (the means and the sum over the heads accumulate in one device scalar)
            _loss_sum(ops, logits[:nh], None, sf, mf, loss, w)
            _loss_sum(ops, logits[nh:], None, sr, mr, loss, w)
        ctx.disc, ctx.names, ctx.runs, ctx.B = disc, names, runs, B
        ctx.param_ptrs, ctx.shapes = [p.data_ptr() for p in params], [p.shape for p in params]
        return loss[0].float()

    @staticmethod
    def backward(ctx, gl):
        disc, ops = ctx.disc, ctx.disc._get_ops()
        (sf, mf), (sr, mr) = disc._grad_terms
        # one backward pass over the 2B batch: the fake term's gradient on the first half of every head's logits, the real term's on the second
        dtop = []
        for logits, nh in disc._logit_heads(ctx.runs, ctx.B):
            g = torch.empty_like(logits)
            _, sc = _scaled_grad(ops, logits[:nh], None, logits[:nh].numel(), sf, 1.0, mf, out=g[:nh])
            _scaled_grad(ops, logits[nh:], None, logits[nh:].numel(), sr, 1.0, mr, out=g[nh:])
            dtop.append((g, sc))
        # FlatAdam keeps every parameter's .grad as a view of one flat buffer: write there (freshly zeroed by zero_grad) and hand autograd no
        # per-parameter gradients (its AccumulateGrad nodes were one `grad += g` launch per parameter) -- as aero_amd.train.AeroFunction does
        glf = _upstream(gl)
        # distrib.wrap(critic) (solver.py:51): the mean over ranks.  1 / world rides in the upstream factor the weight-norm kernel
        # multiplies in anyway; the sum is ONE all-reduce over the flat gradient range once the pass is done (the critic's backward is a
        # few milliseconds: nothing to overlap it with but the optimizer step that needs its result)
        sync = getattr(disc, '_grad_sync', None)
        if sync is not None and not sync.active():
            sync = None
        if sync is not None:
            glf = glf * sync.mean_factor()
        sink = getattr(disc, '_grad_sink', None)
        sink = sink() if sink is not None else None
        offs, n = flat_offsets(shp.numel() for shp in ctx.shapes)
        params = dict(disc.named_parameters())
        # (a buffer that already holds gradients must not go through the collective a second time: then this pass gets its own tensors)
        if sink is not None and sink.accepts(ctx.param_ptrs, offs, n, glf.device) and (sync is None or sink.fresh):
            out = {nme: params[nme].grad for nme in ctx.names}
            sink.fresh = False
            disc._backward(ctx.runs, dtop, None, True, False, out=out, gl=glf)
            ctx.runs = None
            if sync is not None:
                sync.reduce_async(sink.flat_g)
                sync.wait()
            return (None, None, None, None) + (None,) * len(ctx.names)
        total, _ = disc._backward(ctx.runs, dtop, None, True, False, gl=glf)
        ctx.runs = None
        if sync is not None:
            flat = torch.cat([total[nme].reshape(-1) for nme in ctx.names])
            sync.reduce_async(flat)
            sync.wait()
            o = 0
            for nme in ctx.names:
                k = total[nme].numel()
                total[nme] = flat[o:o + k].view_as(total[nme])
                o += k
        return (None, None, None, None) + tuple(total[nme] for nme in ctx.names)
