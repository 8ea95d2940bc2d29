"""CPU: the conv dispatch table.  aero_conv_kernel_name is a pure host function of the descriptor (and of the A/B switches in the
environment), so the built gfx950 library answers it without a device: every entry of tests/golden/conv_dispatch.json -- the conv launches
of the `full` model at four (B, T) and of the music model, plus hand-written descriptors for what the models do not reach and one per
error text -- must give exactly the recorded kernel name, or the recorded (return code, error text).

The fixture was recorded from the library of the commit BEFORE the dispatch was split into check / plan / issue (tools/list_convs.py
--json with AERO_HIP_LIB pointing at that build): a pull request that moves an entry changes the fixture with the same tool and says why."""
import importlib.util
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

_spec = importlib.util.spec_from_file_location('list_convs', os.path.join(ROOT, 'tools', 'list_convs.py'))
list_convs = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(list_convs)

FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'conv_dispatch.json')
GLDS_TILES = [(4, 2), (3, 2), (4, 1), (3, 1), (2, 1), (1, 1)]
# every name the library prints under the default environment (aero_convtr_carry_kernel<4> is instantiated but not reachable: 128
# channels are eight K-chunks of two taps, and the stream form the carried-tap kernel branches off takes at most six)
NAMES = (['aero_conv_tiny_kernel', 'aero_conv_stream_kernel'] + [f'aero_convtr_carry_kernel<{n}>' for n in (1, 2, 3)] +
         [f'aero_conv_skinny_kernel<{v}>' for v in (8, 4, 2, 1)] +
         [f'aero_conv_ring_kernel<{t}, 0>' for t in ('2, 2, 4, 3', '2, 4, 4, 3', '2, 4, 4, 1', '1, 4, 3, 3', '2, 2, 3, 3', '1, 8, 4, 3', '1, 8, 2, 3')] +
         [f'aero_conv_glds8_kernel<{mf}, 32, {st}>' for mf in (3, 4) for st in ('false', 'true')] +
         [f'aero_conv_glds_kernel<{mf}, {wm}, {kc}, {st}>' for mf, wm in GLDS_TILES for kc in (32, 64) for st in ('false', 'true')] +
         [f'aero_conv_kernel<{mf}, {wm}, {st}>' for mf, wm in GLDS_TILES for st in ('false', 'true')])
ERRORS = 28                                                    # distinct error texts of the check and the plan


@pytest.fixture(scope='module')
def entries():
    return json.load(open(FIXTURE))


def _built():
    if not os.path.exists(os.path.join(ROOT, 'aero_amd', 'libaero_hip.so')):
        import __graft_entry__ as g
        g.build()


def test_every_entry_dispatches_as_recorded(entries):
    _built()
    _lib, lib = list_convs.load_lib()
    assert 'gfx950' in lib.version
    wrong = [(e['origin'], e['expect'], got) for e in entries for got in [list_convs.query(_lib, lib, e['desc'])] if got != e['expect']]
    assert not wrong, f'{len(wrong)} of {len(entries)} descriptors moved: {wrong[:8]}'


def test_the_table_covers_every_kernel_and_every_error(entries):
    names = {e['expect'] for e in entries if isinstance(e['expect'], str)}
    assert names == set(NAMES), (sorted(set(NAMES) - names), sorted(names - set(NAMES)))
    errors = {e['expect'][1] for e in entries if not isinstance(e['expect'], str)}
    assert len(errors) == ERRORS and all(t.startswith('conv: ') for t in errors)
    origins = {e['origin'].split(' #')[0] for e in entries}
    for shape in ('full (64, 501)', 'full (16, 501)', 'full (1, 501)', 'full (64, 376)', 'music (2, 1724)'):
        assert shape in origins


@pytest.mark.parametrize('switch', list_convs.SWITCHES)
def test_switches_move_what_was_recorded(entries, switch):
    """the library reads its switches once per process: a fresh child (ctypes only, no torch) per value"""
    _built()
    k, v = switch.split('=')
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'list_convs.py'), '--query', FIXTURE], env=dict(os.environ, **{k: v}),
                         check=True, capture_output=True, text=True, timeout=120).stdout
    got = json.loads(out)
    assert len(got) == len(entries)
    wrong = [(e['origin'], e.get('env', {}).get(switch, e['expect']), g) for e, g in zip(entries, got) if g != e.get('env', {}).get(switch, e['expect'])]
    assert not wrong, f'{switch}: {len(wrong)} of {len(entries)} descriptors moved: {wrong[:8]}'
    assert any(switch in e.get('env', {}) for e in entries), f'{switch} moves nothing in the table'
