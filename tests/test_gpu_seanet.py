"""GPU: the Seanet baseline generator on the MI355X against the reference's goldens (tests/seanet_cases.py; bar max(1e-3, 3 x the
reference's own fp16-operand floor) per recorded stage), the shipped configuration's shape, and the predict path."""
import pytest
import torch

import seanet_cases as SC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', ['a', 'b', 'c', 'd'])
def test_golden_cases_on_the_gpu(name):
    SC.check_case(SC.case_errors(name, 'cuda'))


def shipped(seed=500):
    """seanet_4-16.yaml's generator: ngf 32, ratios 8 8 2 2, 4 -> 16 kHz, upsampling inside the model"""
    return SC.seeded_seanet(seed, lr_sr=4000, hr_sr=16000).eval().cuda()


def test_shipped_shape_is_finite_and_deterministic():
    """B = 16 clips of 8 000 low-rate samples (2 s): right length, finite, bit-equal on two runs and between one forward of 16 and 2 x 8"""
    m = shipped()
    x = (0.3 * torch.randn(16, 1, 8000, generator=torch.Generator().manual_seed(501))).cuda()
    with torch.no_grad():
        y1 = m(x)
        y2 = m(x)
        halves = torch.cat([m(x[:8]), m(x[8:])], 0)
    torch.cuda.synchronize()
    assert y1.shape == (16, 1, 32000) and y1.dtype == torch.float32 and bool(torch.isfinite(y1).all())
    assert float(y1.abs().max()) > 0
    assert torch.equal(y1, y2)
    assert torch.equal(y1, halves)


def test_fused_and_layer_by_layer_agree_on_the_gpu(monkeypatch):
    """AERO_SEANET_FUSE=0 on the shipped width: the two forms differ by fp16 roundings inside each block, within the forward bar overall"""
    m = shipped(502)
    x = (0.3 * torch.randn(2, 1, 4000, generator=torch.Generator().manual_seed(503))).cuda()
    with torch.no_grad():
        y1 = m(x)
        monkeypatch.setenv('AERO_SEANET_FUSE', '0')
        y0 = m(x)
    e = SC.rel_l2(y1.cpu(), y0.cpu())
    print(f'fused vs layer by layer, ngf 32: {e:.3e}')
    assert e <= 1e-3


def test_predict_signal_equals_chunk_by_chunk_forwards():
    """enhance.predict_signal on 25 s at 4 kHz: two full 10-s chunks batched, a 5-s tail -- exactly the per-chunk forwards"""
    from aero_amd import enhance
    m = shipped(504)
    sig = 0.3 * torch.randn(1, 25 * 4000, generator=torch.Generator().manual_seed(505))
    out = enhance.predict_signal(m, sig, 4000, device='cuda')
    assert out.shape == (1, 25 * 16000)
    with torch.no_grad():
        ref = torch.cat([m(sig[:, a:b].unsqueeze(1).cuda()).squeeze(1).cpu() for a, b in enhance.chunk_ranges(sig.shape[-1], 4000)], -1)
    assert torch.equal(out, ref)
