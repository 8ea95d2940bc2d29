"""GPU: the training data path on the MI355X -- aero_segment_gather bit-equal to the host reader, the resampled lr side within the
resampler's bar (tests/data_cases.py), and `train.py` on wav files: two epochs from the device-resident store, a checkpoint that
load_generator loads, and the same losses to the last digit when the host reader feeds the same batches."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import data_cases as DC
from conftest import ROOT, rel_l2

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def lib():
    from aero_amd import _lib
    return _lib.load()


@pytest.mark.parametrize('f32', [False, True])
@pytest.mark.parametrize('L', DC.GATHER_L)
def test_segment_gather_is_bit_equal_to_the_host_reader(lib, tmp_path, f32, L):
    DC.check_gather(lib, tmp_path, f32, L, 'cuda')


@pytest.mark.parametrize('lr_sr,hr_sr,seg', DC.UPSAMPLE_CASES)
def test_store_upsamples_the_cut_segment(lib, tmp_path, lr_sr, hr_sr, seg):
    DC.check_upsample(lib, tmp_path, lr_sr, hr_sr, seg, 'cuda', rel_l2)


def test_store_batches_equal_the_stacked_host_items(lib, tmp_path):
    """more than one block per item (L = 16000 hr samples is 8 blocks of 256 vectors), both arena types, files shorter than a segment"""
    from aero_amd import data
    for f32 in (False, True):
        ds = DC.make_set(tmp_path, f'set{int(f32)}', 4000, 16000, (4000, 9001, 1, 2500), 4000, f32=f32)
        store = data.DeviceLrHrStore(ds, 'cuda', lib=lib)
        idx = list(range(len(ds)))[::-1] + [0]
        lr, hr = store.batch(idx)
        lr_ref, hr_ref = DC.stacked(ds, idx)
        assert torch.equal(lr.cpu(), lr_ref) and torch.equal(hr.cpu(), hr_ref)


SECONDS = (0.6, 0.9, 1.3, 1.7, 2.0, 2.3)


def write_training_set(d):
    """six PCM16 files of seeded noise at 16 kHz, the lr side their audio_io.resample to 4 kHz -> the number of 1-second items"""
    from aero_amd import audio_io
    os.makedirs(os.path.join(d, 'lr'))
    os.makedirs(os.path.join(d, 'hr'))
    lr, hr, items = [], [], 0
    for k, sec in enumerate(SECONDS):
        n = int(sec * 16000)
        x = 0.1 * torch.randn(1, n, generator=torch.Generator().manual_seed(700 + k))
        y = audio_io.resample(x, 16000, 4000)
        for side, sig, sr, lst in (('hr', x, 16000, hr), ('lr', y, 4000, lr)):
            path = os.path.join(d, side, f'clip{k}.wav')
            DC.write_wav(path, np.clip(np.round(sig[0].numpy() * 32768.0), -32768, 32767).astype(np.int16), sr, False)
            lst.append([path, sig.shape[-1]])
        items += max(1, math.ceil((n - 16000) / 16000) + 1) if n >= 16000 else 1
    json.dump(lr, open(os.path.join(d, 'lr.json'), 'w'))
    json.dump(hr, open(os.path.join(d, 'hr.json'), 'w'))
    return items


def run_train(d, cwd, *extra):
    """channels=16 is the narrowest generator the training engine trains: with the experiment's norm_groups = 4 a narrower one has
    GroupNorm groups of fewer than 8 channels in its decoder, which aero_norm_bwd_reduce refuses (the first device run of this test, at
    channels=8, stopped there: "norm_bwd: needs ... groups of >= 8 channels"; tests/test_gpu_train.py trains at 16 for the same reason)"""
    cmd = [sys.executable, os.path.join(ROOT, 'train.py'), 'experiment=aero_4-16_512_64', 'experiment.aero.channels=16', 'experiment.segment=1',
           'experiment.stride=1', 'experiment.batch_size=2', 'experiment.adversarial=false', 'epochs=2', f'dset.train={d}', *extra]
    os.makedirs(cwd)
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK')}
    out = subprocess.run(cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    return [json.loads(ln) for ln in out.stdout.splitlines() if ln.startswith('{')]


def test_train_py_on_wav_files(tmp_path):
    from aero_amd import audio_io, enhance
    from aero_amd.config import load_config
    d = str(tmp_path / 'tr')
    items = write_training_set(d)
    assert items == 11
    dev_run = run_train(d, str(tmp_path / 'a'))
    print(dev_run)
    assert [r['epoch'] for r in dev_run] == [0, 1] and all(r['data'] == 'device' for r in dev_run)
    assert all(r['steps'] == math.ceil(items / 2) for r in dev_run)
    loss_keys = [k for k in dev_run[0] if k == 'total' or k.startswith('generator_')]
    assert 'total' in loss_keys and 'generator_stft' in loss_keys
    assert all(math.isfinite(r[k]) for r in dev_run for k in loss_keys)
    ckpt = str(tmp_path / 'a' / 'checkpoint.th')
    assert os.path.exists(ckpt) and not os.path.exists(ckpt + '.tmp')
    args = load_config(os.path.join(ROOT, 'conf'), ['experiment=aero_4-16_512_64', 'experiment.aero.channels=16', f'checkpoint_file={ckpt}'])
    pkg = enhance.load_package(ckpt)
    assert [h['epoch'] for h in pkg['history']] == [0, 1] and pkg['history'][1]['total'] == dev_run[1]['total']
    assert pkg['optimizers']['optimizer']['state'][0]['step'] == 2 * math.ceil(items / 2)
    model = enhance.load_generator(args, device='cuda')
    sig, sr = audio_io.load(os.path.join(d, 'lr', 'clip2.wav'))
    with torch.no_grad():
        y = model(sig[None].cuda())
    assert y.shape == (1, 1, 4 * sig.shape[-1]) and bool(torch.isfinite(y).all()) and float(y.abs().max()) > 0
    # the host reader feeds the same batches in the same order, and the step is bit-reproducible: the same losses to the last digit
    host_run = run_train(d, str(tmp_path / 'b'), '+data_on_device=false')
    print(host_run)
    assert all(r['data'] == 'host' for r in host_run) and len(host_run) == 2
    for a, b in zip(dev_run, host_run):
        assert {k: a[k] for k in loss_keys} == {k: b[k] for k in loss_keys}
