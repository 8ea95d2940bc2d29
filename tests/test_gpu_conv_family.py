"""GPU (-m gpu): every conv kernel the dispatch table can pick, on the MI355X, against float64 -- the table and the comparison of
tests/conv_family_cases.py (global 2e-3 and the per-block bar, poisoned borders, the kernel name asked before and read after the launch)."""
import json
import os
import subprocess
import sys

import pytest
import torch

import conv_family_cases as cf

pytestmark = pytest.mark.gpu
DEV = 'cuda'
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def lib():
    from aero_amd import _lib
    assert torch.cuda.is_available()
    lib = _lib.load()
    assert not lib.is_emulator
    return lib


@pytest.mark.parametrize('name', [c['name'] for c in cf.CASES])
def test_conv_family(lib, name):
    cf.check_case(lib, DEV, cf.BY_NAME[name], verbose=True)


# AERO_RING_192X128=0 (README.md): the 192-row ring tile on eight waves over 256 time steps, a kernel outside NAMES that the fused tail
# also accepts.  The library reads its switches once per process: ONE fresh child runs both cases and prints its verdict.
WIDE192 = 'aero_conv_ring_kernel<2, 4, 3, 3, 0>'
_CHILD = """
import json, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import conv_family_cases as cf
from aero_amd import _lib
lib = _lib.load()
out = []
for T in (255, 257):
    c = dict(cf.BY_NAME['ring192 T=129 relu'], name='ring192 wide T=%%d' %% T, want=%r, T=T)
    v = cf.check_case(lib, 'cuda', c)
    out.append(dict(T=T, glob=v['glob'], worst=v['worst'], ok=v['ok']))
print('VERDICT ' + json.dumps(out))
"""


def test_wide_192_row_ring_tile_behind_its_switch(lib):
    code = _CHILD % (os.path.dirname(HERE), HERE, WIDE192)
    out = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, AERO_RING_192X128='0'), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    verdict = json.loads([line for line in out.stdout.splitlines() if line.startswith('VERDICT ')][-1][8:])
    assert [v['T'] for v in verdict] == [255, 257] and all(v['ok'] and v['worst'] < cf.BLOCK_BAR for v in verdict), verdict
