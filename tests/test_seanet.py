"""CPU: the Seanet baseline generator (aero_amd/seanet.py, csrc/k_seanet.h) -- construction against the reference's seed, the host
arithmetic, every new kernel on the emulator against a float64 restatement, the golden cases end to end on the emulator, the wiring.

Bounds of the single-kernel checks (operands are fp16-exact, the restatements float64, so what is measured is the kernels' own fp32
accumulation and their fp16 OUTPUT rounding): one rounding to fp16 is at most 2^-11 = 4.9e-4 relative per element, and so in rel-L2.
  * one kernel, one output rounding: 6e-4 (2^-11 plus room for fp32 accumulation, ~1e-6, and for the rare hidden value whose fp16 rounding
    flips between an fp32 and a float64 sum: one fp16 ulp on one of C inputs of the last product);
  * the layer-by-layer block rounds the shortcut to fp16 as well before adding it: 2 x 2^-11 -> 1.1e-3;
  * fused against layer-by-layer: both of the above -> 3 x 2^-11 = 1.5e-3 ("agree to fp16 rounding of the hidden activation").
fp32 outputs (stats, front end, tail) have no fp16 rounding: 2e-6, the bar the STFT kernels carry against the pinned oracle."""
import os
import types

import pytest
import torch
import torch.nn.functional as F

import seanet_cases as SC
from conftest import ROOT, rel_l2

ONE_ROUNDING, TWO_ROUNDINGS, THREE_ROUNDINGS = 6e-4, 1.1e-3, 1.5e-3


@pytest.fixture(scope='module')
def lib():
    return SC.emu_lib()


# ------------------------------------------------------------------ the feature exists
def test_build_models_returns_a_seanet():
    from aero_amd import trainer
    from aero_amd.config import load_config
    from aero_amd.seanet import Seanet
    args = load_config(os.path.join(ROOT, 'conf'), ['experiment=seanet_4-16'])
    assert args.experiment.model == 'seanet'
    models = trainer.build_models(args)
    g = models['generator']
    assert isinstance(g, Seanet) and 'msd_melgan' in models
    assert (g.lr_sr, g.hr_sr, g.scale_factor, g.upsample, g.ratios, g.floor) == (4000, 16000, 4, True, [8, 8, 2, 2], 1e-3)
    from src.models.modelFactory import get_model
    from src.models.seanet import Seanet as Shim
    assert Shim is Seanet and isinstance(get_model(args)['generator'], Seanet)
    with pytest.raises(NotImplementedError):
        args.experiment.model = 'demucs'
        trainer.build_models(args)


def test_load_generator_chooses_the_class_from_the_experiment():
    from aero_amd import enhance
    from aero_amd.config import load_config
    from aero_amd.modules import Aero
    from aero_amd.seanet import Seanet
    c = load_config(os.path.join(ROOT, 'conf'), ['experiment=seanet_4-16', '+random_init=true'])
    assert isinstance(enhance.load_generator(c, device='cpu'), Seanet)
    c = load_config(os.path.join(ROOT, 'conf'), ['experiment=aero_4-16_512_64', '+random_init=true'])
    assert isinstance(enhance.load_generator(c, device='cpu'), Aero)


def test_constructor_limits():
    from aero_amd.seanet import Seanet
    for kw in (dict(in_channels=2), dict(out_channels=2), dict(ngf=12), dict(ngf=4)):
        with pytest.raises(NotImplementedError):
            Seanet(**kw)
    m = Seanet(ngf=8, ratios=[4, 2], n_residual_layers=2, upsample=False)
    assert m._init_args_kwargs == ((), dict(ngf=8, ratios=[4, 2], n_residual_layers=2, upsample=False))


# ------------------------------------------------------------------ construction, host arithmetic
@pytest.mark.parametrize('ngf', [8, 32])
def test_seanet_state_dict_matches_the_reference_seed(ngf):
    errs = SC.checksum_errors(ngf)
    assert max(errs.values()) < 1e-6, sorted(errs.items(), key=lambda kv: -kv[1])[:5]


@pytest.mark.parametrize('ngf', [8, 32])
def test_a_reference_state_dict_loads_strictly(ngf):
    from aero_amd.seanet import Seanet
    shapes = SC.meta()['shapes_' + str(ngf)]
    state = {k: torch.full(s, 0.25) for k, s in shapes.items()}
    m = Seanet(ngf=ngf, upsample=False)
    m.load_state_dict(state, strict=True)
    assert all(float(v.flatten()[0]) == 0.25 for v in m.state_dict().values())
    assert any('.block.2.weight_v' in k for k in shapes) and any('.shortcut.weight_g' in k for k in shapes)


def test_estimate_output_length_matches_the_reference():
    from aero_amd.seanet import Seanet
    rec = SC.meta()['lengths']
    assert set(rec) == {'8,8,2,2', '4,2'}
    for key, table in rec.items():
        m = Seanet(ngf=8, ratios=[int(r) for r in key.split(',')], upsample=False)
        assert set(table) == {'1', '7', '999', '2003', '8000', '32000', '32001'}
        for n, want in table.items():
            assert m.estimate_output_length(int(n)) == want, (key, n)
        x, pad = m.pad_to_valid_length(torch.ones(1, 1, 2003))
        assert x.shape[-1] == table['2003'] and pad == table['2003'] - 2003 and float(x[..., 2003:].abs().sum()) == 0


# ------------------------------------------------------------------ kernels on the emulator
@pytest.mark.parametrize('d', [1, 3, 9])
@pytest.mark.parametrize('T', [40, 128, 200])
def test_fused_resblock_against_float64(lib, d, T):
    """T shorter than, equal to and not a multiple of the 128-step tile; C = 16"""
    x, w = SC.f16((2, 16, T), 300 + T + d), SC.res_weights(16, 310 + d)
    ref = SC.resblock_f64(x, w, d)
    fused, layers = SC.run_resblock(lib, x, w, d), SC.resblock_layers(lib, x, w, d)
    e = (rel_l2(fused, ref), rel_l2(layers, ref), rel_l2(fused, layers))
    print(f'resblock d={d} T={T}: fused {e[0]:.3e}, layer by layer {e[1]:.3e}, fused vs layers {e[2]:.3e}')
    assert e[0] <= ONE_ROUNDING and e[1] <= TWO_ROUNDINGS and e[2] <= THREE_ROUNDINGS


@pytest.mark.parametrize('Cc', [8, 48, 64])
def test_fused_resblock_widths_and_skip(lib, Cc):
    """C = 8 (half an MFMA tile), 48 (K = 144, 96: not multiples of 32), 64; with the decoder's skip added in the epilogue"""
    x, w, add = SC.f16((1, Cc, 150), 320 + Cc), SC.res_weights(Cc, 330 + Cc), SC.f16((1, Cc, 150), 340 + Cc)
    ref = SC.resblock_f64(x, w, 3, add=add)
    e = (rel_l2(SC.run_resblock(lib, x, w, 3, add=add), ref), rel_l2(SC.resblock_layers(lib, x, w, 3, add=add), ref))
    print(f'resblock C={Cc} + skip: fused {e[0]:.3e}, layer by layer {e[1]:.3e}')
    assert e[0] <= ONE_ROUNDING and e[1] <= TWO_ROUNDINGS


@pytest.mark.parametrize('d', [1, 3, 9])
def test_resblock_short_inputs_behave_as_reflection_pad(lib, d):
    """ReflectionPad1d(d) needs d < T: T = d + 1 works, T = d is refused -- by the kernel's entry point and by the module"""
    w = SC.res_weights(8, 350)
    x = SC.f16((1, 8, d + 1), 351 + d)
    assert rel_l2(SC.run_resblock(lib, x, w, d), SC.resblock_f64(x, w, d)) <= ONE_ROUNDING
    with pytest.raises(RuntimeError, match='smaller than the input length'):
        SC.run_resblock(lib, SC.f16((1, 8, d), 352), w, d)
    with pytest.raises(RuntimeError):
        F.pad(torch.zeros(1, 8, d), (d, d), mode='reflect')     # (what the reference's block does with such an input)


@pytest.mark.parametrize('r', [8, 2, 3])
def test_strided_and_transposed_convs_against_float64(lib, r):
    """kernel 2 r, stride r, padding r // 2 + r % 2 (output_padding r % 2), LeakyReLU on the input (seanet.py:73-93)"""
    p = r // 2 + r % 2
    Cin, Cout, T = 16, 24, 37 * r
    x = SC.f16((2, Cin, T), 360 + r)
    w, b = SC.f16((Cout, Cin, 2 * r), 361 + r, 0.1), 0.1 * SC.f16((Cout,), 362 + r)
    a = SC.lrelu(x.double()).half().double()
    ref = F.conv1d(a, w.double(), b.double(), stride=r, padding=p)
    e1 = rel_l2(SC.run_conv(lib, x, w, b, stride=r, pad=p, in_slope=SC.SLOPE), ref)
    xt = SC.f16((2, Cout, 37), 363 + r)
    wt = SC.f16((Cout, Cin, 2 * r), 364 + r, 0.1)
    bt = 0.1 * SC.f16((Cin,), 365 + r)
    add = SC.f16((2, Cin, T), 366 + r)
    at = SC.lrelu(xt.double()).half().double()
    reft = F.conv_transpose1d(at, wt.double(), bt.double(), stride=r, padding=p, output_padding=r % 2) + add.double()
    got = SC.run_conv(lib, xt, wt, bt, stride=r, pad=p, in_slope=SC.SLOPE, transposed=True, opad=r % 2, add=add)
    assert got.shape == reft.shape == (2, Cin, T)
    e2 = rel_l2(got, reft)
    print(f'r={r}: strided conv {e1:.3e}, transposed conv + skip {e2:.3e}')
    assert e1 <= ONE_ROUNDING and e2 <= ONE_ROUNDING


def test_latent_conv_with_tanh_and_skip(lib):
    """k = 7, reflect padding 3, LeakyReLU in, tanh out, skip added behind it; 40 -> 8 channels, T not a multiple of anything"""
    x, w, b, add = SC.f16((2, 40, 133), 370), SC.f16((8, 40, 7), 371, 0.05), 0.1 * SC.f16((8,), 372), SC.f16((2, 8, 133), 373)
    a = F.pad(SC.lrelu(x.double()).half().double(), (3, 3), mode='reflect')
    ref = torch.tanh(F.conv1d(a, w.double(), b.double())) + add.double()
    assert rel_l2(SC.run_conv(lib, x, w, b, pad=3, reflect=1, in_slope=SC.SLOPE, act=1, add=add), ref) <= ONE_ROUNDING
    with pytest.raises(Exception, match='smaller than the input length'):
        SC.run_conv(lib, SC.f16((1, 40, 3), 374), w, b, pad=3, reflect=1)


def test_stats_front_and_the_end_convs(lib):
    x = 0.3 * torch.randn(3, 2003, generator=torch.Generator().manual_seed(380)) + 0.05
    stats = torch.empty(3, 2)
    lib.call('aero_seanet_stats', x.data_ptr(), 3, 2003, SC.C.c_float(1e-3), stats.data_ptr(), None)
    sd = x.double().std(dim=-1)
    assert rel_l2(stats[:, 0], sd) <= 2e-6 and rel_l2(stats[:, 1], 1.0 / (1e-3 + sd)) <= 2e-6
    # front without resampling: scale and right zero pad
    y = torch.empty(3, 2048)
    lib.call('aero_seanet_front', x.data_ptr(), stats.data_ptr(), None, y.data_ptr(), 3, 2003, 2003, 2048, 1, 1, 0, None)
    assert rel_l2(y[:, :2003], x.double() / (1e-3 + sd)[:, None]) <= 2e-6 and float(y[:, 2003:].abs().sum()) == 0
    # ... and with resampling: x / (floor + std), then 4 -> 16 kHz
    from aero_amd import audio_io
    yr, Lup = SC.run_front(lib, x, 4000, 16000, Tpad=8016, stats=stats)
    assert Lup == 8012 and rel_l2(yr[:, :Lup], audio_io.resample((x.double() / (1e-3 + sd)[:, None]).float(), 4000, 16000)) <= 2e-6
    # conv_in: 1 -> 16 channels, tanh; the waveform is rounded to fp16 as it is read
    w, b = SC.f16((16, 1, 7), 381, 0.3), 0.1 * SC.f16((16,), 382)
    h = torch.empty(3, 2048, 16, dtype=torch.float16)
    lib.call('aero_seanet_conv_in', y.data_ptr(), w.reshape(16, 7).contiguous().data_ptr(), b.contiguous().data_ptr(), h.data_ptr(), 3, 2048, 16, None)
    ref = torch.tanh(F.conv1d(F.pad(y.half().double()[:, None], (3, 3), mode='reflect'), w.double(), b.double()))
    assert rel_l2(h.float().transpose(1, 2), ref) <= ONE_ROUNDING
    # conv_out: 16 -> 1, tanh, + skip, trim to 2003, times std; fp32 out
    wo, bo = SC.f16((1, 16, 7), 383, 0.2), torch.tensor([0.05])
    out = torch.empty(3, 2003)
    w16 = wo[0].t().contiguous().half()
    lib.call('aero_seanet_conv_out', h.data_ptr(), w16.data_ptr(), bo.data_ptr(), y.data_ptr(), stats.data_ptr(), out.data_ptr(), 3, 2048, 16, 2003,
             SC.C.c_float(SC.SLOPE), None)
    a = F.pad(SC.lrelu(h.double().transpose(1, 2)).half().double(), (3, 3), mode='reflect')
    ref = (torch.tanh(F.conv1d(a, wo.double(), bo.double()))[:, 0] + y.double())[:, :2003] * stats[:, :1].double()
    e = rel_l2(out, ref)
    print(f'conv_out: {e:.3e}')
    assert e <= 2e-6


@pytest.mark.parametrize('rates', [(4000, 16000), (8000, 16000), (8000, 24000), (11025, 44100)])
@pytest.mark.parametrize('L', [1, 63, 2003])
def test_resampler_kernel_against_audio_io(lib, rates, L):
    from aero_amd import audio_io
    x = torch.randn(2, L, generator=torch.Generator().manual_seed(390 + L))
    ref = audio_io.resample(x, *rates)
    y, Lup = SC.run_front(lib, x, *rates, Tpad=-(-rates[1] * L // rates[0]) + 5)
    assert Lup == ref.shape[-1] and float(y[:, Lup:].abs().sum()) == 0
    e = rel_l2(y[:, :Lup], ref)
    print(f'resample {rates} L={L}: {e:.3e}')
    assert e <= 2e-6


# ------------------------------------------------------------------ the model end to end on the emulator
@pytest.mark.parametrize('name', ['a', 'c', 'd'])
def test_golden_cases_on_the_emulator(name):
    SC.check_case(SC.case_errors(name, 'cpu', emulator=True))


def test_fused_and_layer_by_layer_models_agree(monkeypatch):
    """the AERO_SEANET_FUSE=0 switch changes the launches, not the function: per block the two differ by fp16 roundings (above); over the
    whole ngf = 8 net the outputs stay within the forward bar of each other"""
    case = SC.meta()['cases']['d']
    x = torch.from_numpy(SC.load_npz('seanet_io.npz')['d.x'])
    m = SC.seeded_seanet(case['seed'], **case['cfg']).eval()
    m.use_library(SC.emu_lib())
    calls = []
    real = m._get_ops().lib.call
    m._get_ops().lib = types.SimpleNamespace(call=lambda name, *a: (calls.append(name), real(name, *a))[1], is_emulator=True)
    y1 = m(x)
    n_fused = calls.count('aero_seanet_resblock')
    monkeypatch.setenv('AERO_SEANET_FUSE', '0')
    del calls[:]
    y0 = m(x)
    assert n_fused == 8 and calls.count('aero_seanet_resblock') == 0 and calls.count('aero_seanet_conv') == 6 + 3 * 8
    e = rel_l2(y1, y0)
    print(f'fused vs layer by layer, case d: {e:.3e}')
    assert 0 < e <= 1e-3


def test_upsampling_forward_on_the_emulator():
    """upsample=True (no golden: the reference needs torchaudio there): the front end is the resampler checked above, so the model must equal
    the upsample=False model fed audio_io.resample's output, up to the resampler's own 2e-6 and the fp16 roundings it can flip (the
    scaling by 1 / (floor + std) in front of the resampler: test_stats_front_and_the_end_convs)"""
    from aero_amd import audio_io
    kw = dict(ngf=8, ratios=[4, 2], n_residual_layers=2, lr_sr=4000, hr_sr=16000, normalize=False)
    up, plain = SC.seeded_seanet(400, upsample=True, **kw).eval(), SC.seeded_seanet(400, upsample=False, **kw).eval()
    for m in (up, plain):
        m.use_library(SC.emu_lib())
    x = 0.3 * torch.randn(2, 1, 501, generator=torch.Generator().manual_seed(401))
    y = up(x)
    ref = plain(audio_io.resample(x, 4000, 16000))
    assert y.shape == (2, 1, 2004) and ref.shape == (2, 1, 2004)
    e = rel_l2(y, ref)
    print(f'upsample=True vs resample + upsample=False: {e:.3e}')
    assert e <= 1e-3


def test_training_forward_is_refused_and_eval_is_graphless():
    m = SC.seeded_seanet(410, ngf=8, ratios=[4, 2], n_residual_layers=1, upsample=False)
    m.use_library(SC.emu_lib())
    x = torch.randn(1, 1, 256, generator=torch.Generator().manual_seed(411))
    m.train()
    with pytest.raises(NotImplementedError, match='backward pass is not built'):
        m(x)
    with torch.no_grad():
        assert m(x).shape == (1, 1, 256)
    y = m.eval()(x.requires_grad_(True))
    assert not y.requires_grad and y.grad_fn is None and y.dtype == torch.float32 and bool(torch.isfinite(y).all())
