"""GPU (-m gpu): bench.py's plain run -- exactly K timed steps in the result line, no secondary measurements, and --dump-outputs
writing the last timed step's waveform, which equals a one-at-a-time forward of the same seeded model on the same seeded clips."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, rel_l2


@pytest.mark.gpu
def test_plain_run_dumps_the_last_timed_step(tmp_path):
    B = 4
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', '--batch', str(B),
                          '--dump-outputs', str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    r = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith('{')][-1])
    assert r['steps'] == 3 and r['warmup'] == 1 and r['ms_per_step'] > 0 and r['value'] > 0 and r['higher_is_better'] is True
    assert r['unit'] == 'audio-sec/wall-sec' and r['dtype'] == 'f16'
    assert r['roofline'] is None and r['cpu_baseline'] is None and r['extra_configs'] is None and r['ms_per_step_one_at_a_time'] is None
    y = np.load(tmp_path / 'waveform.npy')
    assert y.dtype == np.float32 and y.shape == (B, 1, 4 * 8000) and np.isfinite(y).all()

    from bench import FULL_CFG
    from aero_amd import Aero
    torch.manual_seed(2036)
    model = Aero(**FULL_CFG).eval().cuda()
    x = torch.randn(B, 1, 8000, generator=torch.Generator().manual_seed(1000)).cuda()
    with torch.no_grad():
        y1 = model(x).float().cpu()
    assert rel_l2(torch.from_numpy(y), y1) < 1e-6
