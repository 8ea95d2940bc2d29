"""HiFi-GAN multi-period critic `mpd` without a GPU: construction against the reference's seeded weights, the trainer's critic list, and
the HIP kernels on the CPU emulation of the library (hidden 8) against the reference's forward, losses and gradients (mpd_cases.py)."""
import ctypes as C

import pytest
import torch

import mpd_cases as mc


@pytest.mark.parametrize('hidden', [32, 8])
def test_mpd_state_dict_matches_the_reference_seed(hidden):
    errs = mc.checksum_errors(hidden)
    assert len(errs) == 90 and max(errs.values()) < 1e-6, max(errs.items(), key=lambda kv: kv[1])


def test_mpd_loads_a_reference_layout_state_dict():
    """a dict built from the reference's key set (mpd_meta.json) with the shapes of discriminators.py:93-100 -- weight_g [Cout, 1, 1, 1],
    weight_v [Cout, Cin, K, 1], bias [Cout] -- loads with strict key matching and lands where the reference would put it"""
    hidden = 8
    chans = [(1, hidden), (hidden, 4 * hidden), (4 * hidden, 16 * hidden), (16 * hidden, 32 * hidden), (32 * hidden, 32 * hidden),
             (32 * hidden, 1)]
    g = torch.Generator().manual_seed(9)
    sd = {}
    for k in mc.meta()['checksums'][str(hidden)]:
        _, i, kind, rest = k.split('.', 3)
        j = 5 if kind == 'conv_post' else int(rest.split('.')[0])
        cin, cout = chans[j]
        K = 3 if j == 5 else 5
        shape = {'weight_g': (cout, 1, 1, 1), 'weight_v': (cout, cin, K, 1), 'bias': (cout,)}[k.rsplit('.', 1)[1]]
        sd[k] = torch.randn(*shape, generator=g)
    assert len(sd) == 90
    d = mc.seeded_mpd(hidden)
    d.load_state_dict(sd)                                                    # strict: same keys, same shapes
    got = d.state_dict()
    assert all(torch.equal(got[k], sd[k]) for k in sd)


def test_mpd_rejects_what_the_kernels_do_not_take():
    from aero_amd.mpd import MultiPeriodDiscriminator
    for hidden in (12, 4, 128):
        with pytest.raises(NotImplementedError):
            MultiPeriodDiscriminator(hidden=hidden)


def _args(models):
    from aero_amd.config import _wrap
    gen = dict(channels=8, nfft=512, hop_length=256, lr_sr=4000, hr_sr=16000)
    return _wrap(dict(optim='adam', lr=3e-4, beta2=0.999, losses=['stft'], stft_sc_factor=0.5, stft_mag_factor=0.5,
                      experiment=dict(model='aero', aero=gen, adversarial=True, features_loss_lambda=100, only_features_loss=False,
                                      only_adversarial_loss=False, discriminator_models=models, mpd=dict(hidden=8),
                                      melgan_discriminator=dict(n_layers=4, num_D=3, downsampling_factor=4, ndf=16))))


def test_trainer_builds_mpd_in_the_reference_order():
    from aero_amd import trainer
    from aero_amd.discriminators import Discriminator
    from aero_amd.mpd import MultiPeriodDiscriminator
    for names in (['msd_melgan', 'mpd'], ['mpd', 'msd_melgan']):
        torch.manual_seed(5)
        models = trainer.build_models(_args(names))
        assert isinstance(models['msd_melgan'], Discriminator) and isinstance(models['mpd'], MultiPeriodDiscriminator)
        sd = {k: v.clone() for k, v in models['mpd'].state_dict().items()}
        if names[0] == 'msd_melgan':
            first = sd
        else:                                                            # modelFactory.py's fixed order: same draws either way
            assert all(torch.equal(first[k], sd[k]) for k in sd)
    for name in ('msd_hifi', 'hifi'):
        with pytest.raises(NotImplementedError, match='reference cannot run it'):
            trainer.build_models(_args(['msd_melgan', name]))


def test_mpd_forward_and_losses_on_the_emulator():
    errs = mc.case_io('cpu', 8, 4001, emulator=True)
    maps = {k: v for k, v in errs.items() if k.startswith(('map.', 'logits'))}
    assert len(maps) == 40 and max(maps.values()) < 1e-3, max(maps.items(), key=lambda kv: kv[1])
    assert errs['d_loss'] < 1e-4 and errs['adv'] < 1e-4 and errs['feat'] < 1e-4, errs


def test_mpd_backward_on_the_emulator():
    mc.check_io(mc.case_io('cpu', 8, 4001, emulator=True))


def test_mpd_ops_on_the_emulator():
    """the kernels one by one against a float64 restatement on fp16-exact operands, odd row counts and all five periods: fold and its
    adjoint, conv 0 forward / data / weight gradient, a stride-3 layer as the 2-tap conv (forward, data gradient, weight gradient), the
    LeakyReLU + zero tail -- exact to fp32 rounding"""
    import torch.nn.functional as F
    from aero_amd import _lib, backward as bw
    from aero_amd.engine import Ops, _ptr, _strides4
    from aero_amd.mpd import _rows3, stride3_images
    from emu.build_emu import build
    lib = _lib.load(build())
    ops = Ops(lib)
    g = torch.Generator().manual_seed(3)
    q = lambda *s: torch.randn(*s, generator=g).half().double()             # noqa: E731  (fp16-exact operands)
    for p in (2, 3, 5, 7, 11):
        L = 97 + p
        x = q(2, L)
        H = -(-L // p)
        xf = torch.empty(2 * p, H, dtype=torch.float16)
        x32 = x.float().contiguous()                                        # (named: the buffers must outlive the calls)
        lib.call('aero_mpd_fold', _ptr(x32), 2, L, p, _ptr(xf), 0)
        xp = F.pad(x.view(2, 1, L), (0, H * p - L), 'reflect') if H * p > L else x.view(2, 1, L)
        ref = xp.view(2, H, p).permute(0, 2, 1).reshape(2 * p, H)
        assert torch.equal(xf.double(), ref), p
        gcol = q(2 * p, H)
        dx = torch.zeros(2, L)
        g32 = gcol.float().contiguous()
        lib.call('aero_mpd_unfold_add', _ptr(g32), 2, L, p, _ptr(dx), 0)
        xv = x.clone().requires_grad_(True)
        xpv = F.pad(xv.view(2, 1, L), (0, H * p - L), 'reflect') if H * p > L else xv.view(2, 1, L)
        (xpv.view(2, H, p).permute(0, 2, 1).reshape(2 * p, H) * gcol).sum().backward()
        assert float((dx.double() - xv.grad).abs().max()) < 1e-5, p
    # conv 0: 1 -> 8 channels, stride 3, on H = 37 rows
    N, H, Cc = 3, 37, 8
    x = q(N, H)
    w, b = q(Cc, 5) * 0.3, q(Cc) * 0.1
    Ho = (H + 2) // 3
    y = torch.empty(N, _rows3(Ho), Cc, dtype=torch.float16)
    x16, w32, b32 = x.half(), w.float().contiguous(), b.float().contiguous()
    lib.call('aero_mpd_conv0_fwd', _ptr(x16), _ptr(w32), _ptr(b32), _ptr(y), N, H, Cc, y.shape[1], C.c_float(0.1), 0)
    ref = F.leaky_relu(F.conv1d(x.view(N, 1, H), w.view(Cc, 1, 5), b, stride=3, padding=2), 0.1).permute(0, 2, 1)
    assert float((y[:, :Ho].double() - ref).abs().max()) < 2e-3 * float(ref.abs().max()) and not y[:, Ho:].any()
    dyp = torch.zeros(N, y.shape[1], Cc, dtype=torch.float16)
    dyp[:, :Ho] = q(N, Ho, Cc).half()
    dxf = torch.empty(N, H)
    nsl = lib.cdll.aero_mpd_conv0_slabs(N, H)
    slabs, dw, db = torch.empty(nsl, 6 * Cc), torch.empty(Cc, 5), torch.empty(Cc)
    lib.call('aero_mpd_conv0_bwd', _ptr(dyp), _ptr(x16), _ptr(w32), None, _ptr(dxf), _ptr(slabs), nsl, _ptr(dw), _ptr(db), N, H, Cc,
             dyp.shape[1], 0)
    xv, wv, bv = x.view(N, 1, H).clone().requires_grad_(True), w.view(Cc, 1, 5).clone().requires_grad_(True), b.clone().requires_grad_(True)
    (F.conv1d(xv, wv, bv, stride=3, padding=2) * dyp[:, :Ho].double().permute(0, 2, 1)).sum().backward()
    for got, want in ((dxf, xv.grad.view(N, H)), (dw, wv.grad.view(Cc, 5)), (db, bv.grad)):
        assert float((got.double() - want).abs().max()) < 1e-5 * max(1.0, float(want.abs().max())), (got, want)
    # a stride-3 layer (8 -> 32 channels) as the 2-tap conv over 24 channels, input H = 37 rows stored as 39 with a zero tail
    M = 32
    Hin, Ho = 37, 13
    xin = torch.zeros(N, 3 * Ho, Cc, dtype=torch.float16)
    xin[:, :Hin] = q(N, Hin, Cc).half()
    w = q(M, Cc, 5) * 0.25                                                  # (fp16-exact: the MFMA image is fp16)
    b = q(M) * 0.1
    spec, dspec = stride3_images(w.float(), b.float(), torch.device('cpu'))
    y = torch.empty(N, _rows3(Ho), M, dtype=torch.float16)
    ops.conv(spec, xin.view(N, 1, Ho, 3 * Cc), None, N, 1, 1, Ho, dst=y.view(N, 1, y.shape[1], M))
    lib.call('aero_mpd_act', _ptr(y), N, Ho, y.shape[1], M, C.c_float(0.1), 0)
    xr = xin[:, :Hin].double().permute(0, 2, 1)
    ref = F.leaky_relu(F.conv1d(xr, w, b, stride=3, padding=2), 0.1).permute(0, 2, 1)
    assert float((y[:, :Ho].double() - ref).abs().max()) < 2e-3 * float(ref.abs().max()) and not y[:, Ho:].any()
    dy = q(N, Ho, M).half()
    dy4 = torch.zeros(N, 1, _rows3(Ho), M, dtype=torch.float16)
    dy4[:, 0, :Ho] = dy
    dy4 = dy4[:, :, :Ho]
    dx = ops.conv(dspec, dy4, None, N, 1, 1, Ho, dst_f32=True, src0_strides=_strides4(dy4)).view(N, 3 * Ho, Cc)
    dw2, dbb = bw.conv_wgrad(ops, dy4, xin.view(N, 1, Ho, 3 * Cc), [0, 0], [-1, 0])
    dwk = torch.stack([dw2[0, :, Cc:2 * Cc], dw2[0, :, 2 * Cc:], dw2[1, :, :Cc], dw2[1, :, Cc:2 * Cc], dw2[1, :, 2 * Cc:]], -1)
    xv, wv, bv = xr.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    (F.conv1d(xv, wv, bv, stride=3, padding=2) * dy.double().permute(0, 2, 1)).sum().backward()
    for got, want in ((dx[:, :Hin], xv.grad.permute(0, 2, 1)), (dwk, wv.grad), (dbb, bv.grad)):
        assert float((got.double() - want).abs().max()) < 1e-5 * max(1.0, float(want.abs().max())), float((got.double() - want).abs().max())
