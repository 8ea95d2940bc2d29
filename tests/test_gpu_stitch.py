"""GPU: overlapped chunks stitched on the MI355X -- the kernel cases of tests/stitch_cases.py on the device, predict_signal(overlap > 0)
through BatchPipeline against the host stitch of the same forwards, and predict.py +overlap_sec writing a file of N_out frames."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import data_cases as DC
import stitch_cases as SC
from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def lib():
    from aero_amd import _lib
    return _lib.load()


@pytest.mark.parametrize('ch', [1, 2])
@pytest.mark.parametrize('V', SC.KERNEL_V)
def test_overlap_stitch_equals_the_host_stitch(lib, ch, V):
    SC.check_kernel(lib, 'cuda', ch, V)


@pytest.mark.parametrize('ch', [1, 2])
@pytest.mark.parametrize('V', SC.KERNEL_V)
def test_agreeing_chunks_come_through_bit_for_bit(lib, ch, V):
    SC.check_agreeing_chunks(lib, 'cuda', ch, V)


@pytest.mark.parametrize('ch', [1, 2])
@pytest.mark.parametrize('peak', [0.8, 3.7])
def test_wav_finalize_and_write_device(lib, tmp_path, ch, peak):
    SC.check_finalize(lib, 'cuda', ch, peak, tmp_path)


@pytest.mark.parametrize('ch', [1, 2])
def test_predict_signal_with_overlap_on_the_device(meta, ch):
    m = SC.tiny_model(meta, device='cuda')
    SC.check_e2e_grouped(m, 'cuda', ch)                          # the same grouped forwards: bit-equal outside the fades
    SC.check_e2e_per_chunk(m, 'cuda', ch, bit_exact=False)       # the per-chunk forwards: the bar of batched against single


def test_pcm16_input_and_device_result(meta):
    from aero_amd import enhance
    m = SC.tiny_model(meta, device='cuda')
    pcm = torch.randint(-32768, 32768, (1, 400 + 123), generator=torch.Generator().manual_seed(3), dtype=torch.int16)
    a = enhance.predict_signal(m, pcm, SC.SR, overlap=SC.OVERLAP)
    out, peak = enhance.predict_signal(m, pcm.float() / 32768.0, SC.SR, overlap=SC.OVERLAP, return_device=True)
    assert out.is_cuda and peak.is_cuda and torch.equal(a, out.cpu())
    assert int(peak) == int(a.abs().max().view(torch.int32))


def test_predict_py_with_overlap_sec(tmp_path):
    """predict.py +overlap_sec=0.5 at 4 -> 16 kHz: 50001 samples are two chunks with a hop of 38000, the file has 4 * 50001 frames"""
    from aero_amd import audio_io
    src = str(tmp_path / 'in.wav')
    DC.write_wav(src, DC.noise_i16(50001, 3) // 8, 4000, False)
    spec = importlib.util.spec_from_file_location('aero_predict_cli', os.path.join(ROOT, 'predict.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(['experiment=aero_4-16_512_64', 'experiment.aero.channels=16', '+random_init=true', f'+filename={src}',
                    f'+output={tmp_path}', '+overlap_sec=0.5'])
    assert audio_io.info(out) == (38000 * 4 + 12001 * 4, 16000, 1)
    wav, _ = audio_io.load(out)
    assert bool(torch.isfinite(wav).all()) and 0 < float(wav.abs().max()) <= 1.0 and np.isfinite(float(wav.std()))
