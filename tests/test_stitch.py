"""CPU: overlapped chunks stitched by aero_overlap_stitch / aero_wav_finalize (csrc/k_stitch.h) on the emulator -- the chunk arithmetic, the
kernels against the host restatement of DESIGN.md 4.8 (tests/stitch_cases.py), every refusal, and enhance.predict_signal(overlap > 0)
against the host stitch of the per-chunk forwards."""
import pytest
import torch

import stitch_cases as SC
from aero_amd import enhance


@pytest.fixture(scope='module')
def lib():
    return SC.emu_lib()


# ------------------------------------------------------------------ host arithmetic
@pytest.mark.parametrize('L', [64, 400])
def test_chunk_arithmetic_is_integer_exact(L):
    """(a 1-"second" chunk at sr = L)  with overlap 0 the chunks are chunk_ranges; with any overlap they cover the file, share exactly `ov`
    samples, all but the last are L long and for n >= 2 the last is longer than the overlap"""
    for ov in (0, 1, L // 10, L // 2):
        for N in range(1, 3 * L + 51):
            r = enhance.overlap_ranges(N, L, ov, segment_sec=1)
            assert len(r) == SC.n_chunks_by_the_rule(N, L, ov)
            if ov == 0:
                assert r == enhance.chunk_ranges(N, L, segment_sec=1)
            assert r[0][0] == 0 and r[-1][1] == N and all(b - a == L for a, b in r[:-1])
            assert all(a2 == a1 + L - ov and b1 - a2 == ov for (a1, b1), (a2, _) in zip(r, r[1:]))
            assert len(r) == 1 or r[-1][1] - r[-1][0] > ov


def test_overlap_and_rate_validation():
    with pytest.raises(ValueError):
        enhance.overlap_ranges(1000, 40, 201)                    # more than half a chunk
    with pytest.raises(ValueError):
        enhance.overlap_ranges(1000, 40, -1)
    assert enhance.output_hop(40, 40, 4) == (1440, 160)
    from fractions import Fraction
    assert enhance.output_hop(40, 40, Fraction(12000, 8000)) == (540, 60)
    with pytest.raises(ValueError):
        enhance.output_hop(40, 41, Fraction(12000, 8000))        # hop 359 input samples = 538.5 output samples


def test_fade_table_is_complementary_and_the_host_bound_holds():
    for V in (1, 3, 16, 160):
        f = enhance.fade_table(V)
        assert f.dtype == torch.float32 and f.shape == (V,) and bool((f > 0).all()) and bool((f < 1).all())
        assert torch.allclose(f + f.flip(0), torch.ones(V), atol=2 * SC.EPS, rtol=0)
    assert float(enhance.fade_table(1)[0]) == 0.5
    worst = SC.fade_bound_on_the_host()
    print(f'fp32 p + f (c - p) against fp64 over 10000 rows: worst |diff| = {worst:.3f} * 2^-24 (|p| + |c|)')
    assert worst <= 3.0


# ------------------------------------------------------------------ the kernels on the emulator
@pytest.mark.parametrize('ch', [1, 2])
@pytest.mark.parametrize('V', SC.KERNEL_V)
def test_overlap_stitch_equals_the_host_stitch(lib, ch, V):
    SC.check_kernel(lib, 'cpu', ch, V)


@pytest.mark.parametrize('ch', [1, 2])
@pytest.mark.parametrize('V', SC.KERNEL_V)
def test_agreeing_chunks_come_through_bit_for_bit(lib, ch, V):
    SC.check_agreeing_chunks(lib, 'cpu', ch, V)


@pytest.mark.parametrize('ch', [1, 2])
@pytest.mark.parametrize('peak', [0.8, 3.7])
def test_wav_finalize_and_write_device(lib, tmp_path, ch, peak):
    SC.check_finalize(lib, 'cpu', ch, peak, tmp_path)


def test_refusals_name_their_entry_point(lib):
    ok0, ok1, okf = SC.check_refusals(lib)
    assert lib.cdll.aero_overlap_stitch(*ok0) == 0 and lib.cdll.aero_overlap_stitch(*ok1) == 0 and lib.cdll.aero_wav_finalize(*okf) == 0


# ------------------------------------------------------------------ predict_signal on the emulated model
@pytest.mark.parametrize('ch', [1, 2])
def test_predict_signal_with_overlap_equals_the_stitched_chunk_forwards(lib, meta, ch):
    m = SC.tiny_model(meta, lib)
    sizes = []
    fwd = m.forward
    object.__setattr__(m, 'forward', lambda x, *a, **k: (sizes.append(tuple(x.shape)), fwd(x, *a, **k))[1])
    SC.check_e2e_per_chunk(m, 'cpu', ch, bit_exact=True)
    assert sizes[:3] == [(2 * ch, 1, 400), (ch, 1, 400), (ch, 1, 163)]          # two groups of full chunks, the short last one on its own


def test_predict_signal_without_overlap_is_unchanged(lib, meta):
    m = SC.tiny_model(meta, lib)
    sig = SC.e2e_signal(1)[:, :400 + 123]
    a = enhance.predict_signal(m, sig, SC.SR, device='cpu')
    b = enhance.predict_signal(m, sig, SC.SR, device='cpu', overlap=0)
    assert torch.equal(a, b)
    # ... and the device result of overlap = 0 is the same concatenation, with its peak
    short = sig[:, :123]
    out, peak = enhance.predict_signal(m, short, SC.SR, device='cpu', overlap=0, return_device=True)
    ref = enhance.predict_signal(m, short, SC.SR, device='cpu')
    assert torch.equal(out, ref) and int(peak) == int(ref.abs().max().view(torch.int32))


def test_predict_signal_refuses_bad_overlaps_rates_and_sizes(lib, meta):
    m = SC.tiny_model(meta, lib)
    sig = SC.e2e_signal(1)
    with pytest.raises(ValueError, match='overlap'):
        enhance.predict_signal(m, sig, SC.SR, device='cpu', overlap=400 // 2 + 1)
    with pytest.raises(ValueError, match='max_bytes'):
        enhance.predict_signal(m, sig, SC.SR, device='cpu', overlap=SC.OVERLAP, max_bytes=1000)

    class Rates(torch.nn.Linear):
        lr_sr, hr_sr = 8000, 12000
    with pytest.raises(ValueError, match='whole'):
        enhance.predict_signal(Rates(1, 1), sig, SC.SR, device='cpu', overlap=41)


def test_pcm16_input_equals_its_float_form(lib, meta):
    m = SC.tiny_model(meta, lib)
    pcm = torch.randint(-32768, 32768, (1, 400 + 123), generator=torch.Generator().manual_seed(3), dtype=torch.int16)
    a = enhance.predict_signal(m, pcm, SC.SR, device='cpu', overlap=SC.OVERLAP)
    b = enhance.predict_signal(m, pcm.float() / 32768.0, SC.SR, device='cpu', overlap=SC.OVERLAP)
    assert a.shape == (1, 4 * 523) and torch.equal(a, b)


def test_seanet_takes_the_plain_loop(lib):
    import seanet_cases as NC
    m = NC.seeded_seanet(5, ngf=8, upsample=False, ratios=[4, 2], n_residual_layers=2).eval()
    m.use_library(lib)
    sig = 0.3 * SC.e2e_signal(1, seed=4)[:, :400 + 300]
    ranges = enhance.overlap_ranges(sig.shape[-1], SC.SR, SC.OVERLAP)
    assert ranges == [(0, 400), (360, 700)]
    pr = enhance.predict_signal(m, sig, SC.SR, device='cpu', overlap=SC.OVERLAP, max_clips=1)
    assert pr.shape == (1, 700)
    ys = SC.chunk_forwards(m, sig, ranges, 'cpu')
    SC.assert_stitched(pr, ys, 360, 40, enhance.fade_table(40), 'seanet')
