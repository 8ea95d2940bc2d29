"""CPU: the conv-family parity table (tests/conv_family_cases.py) without a device.

* every case's descriptor, built by Ops.conv from CPU tensors, asked of the built gfx950 library (aero_conv_kernel_name is a pure host
  function): the case reaches the one kernel it names, and the table reaches exactly NAMES of tests/test_conv_dispatch.py;
* the edges check_table() demands of every family;
* the comparison itself: three faults a broken kernel would leave, applied to the float64 reference -- the block bar rejects every one,
  the global 2e-3 bar alone lets some through;
* the reference's own floor, from which BLOCK_BAR follows;
* the same cases, same shapes, on the CPU emulator (tests/emu)."""
import pytest
import torch

import conv_family_cases as cf
from aero_amd import _lib
from op_cases import TOL16
from test_conv_dispatch import NAMES, _built

# Left out on the emulator only (one fiber per GPU thread: more than about 20 s each there); at most a quarter of the table
EMU_OMITTED = ()


@pytest.fixture(scope='module')
def hip():
    _built()
    lib = _lib.load()
    assert 'gfx950' in lib.version and not lib.is_emulator
    return lib


@pytest.fixture(scope='module')
def emu():
    from emu.build_emu import build
    return _lib.load(build())


def test_table_covers_every_dispatched_kernel(hip):
    wrong = [(c['name'], c['want'], got) for c in cf.CASES for got in [cf.kernel_for(hip, c)] if got != c['want']]
    assert not wrong, wrong
    reached = {c['want'] for c in cf.CASES}
    assert reached == set(NAMES), (sorted(set(NAMES) - reached), sorted(reached - set(NAMES)))


def test_table_sees_every_edge():
    cf.check_table()
    assert set(EMU_OMITTED) <= set(cf.BY_NAME) and 4 * len(EMU_OMITTED) <= len(cf.CASES)


def test_block_bar_follows_the_reference_floor():
    """the floor is measured here, on the CPU, for every case; no block of any reference is all zero"""
    floor = 0.0
    for c in cf.CASES:
        ops = cf.make(c)
        err, den = cf.block_errors(cf.floor_output(c, ops), ops['ref'])
        assert bool((den > 0).all()), c['name']
        floor = max(floor, float(err.max()))
    print(f'reference floor {floor:.3e}, block bar {cf.BLOCK_BAR:.3e}')
    assert 0.9 * cf.REF_FLOOR <= floor <= cf.REF_FLOOR * 1.001, floor
    assert cf.BLOCK_BAR == min(4 * cf.REF_FLOOR, TOL16)


# one ring tile, one ragged glds tile (M = 104 on the 128-row tile, C0 = 40), one skinny launch: the table's shapes, and the skinny one
# once more with long rows -- only there is a single wrong column small enough, relative to the WHOLE output, for the global bar to miss
BITE = [('ring256 T=385', 256), ('glds<4,2> KC32 M=104', 96), ('skinny8 T=65 M=16', 8)]


def _long_skinny():
    return dict(cf.BY_NAME['skinny4 T=2'], name='skinny4 long rows', B=4, Fin=64, T=4097, act='none')


@pytest.fixture(scope='module')
def faulted():
    out = []
    for c, bm in [(cf.BY_NAME[n], bm) for n, bm in BITE] + [(_long_skinny(), 8)]:
        ops = cf.make(c)
        assert cf.judge(ops['ref'], ops['ref'])['ok'] and cf.judge(cf.floor_output(c, ops), ops['ref'])['ok']
        for everywhere in (True, False):
            for what, y in (('last column', cf.fault_last_column(c, ops, everywhere)), ('last M-tile', cf.fault_last_m_tile(c, ops, bm, everywhere)),
                            ('K-chunk', cf.fault_k_chunk(c, ops, everywhere))):
                out.append((f'{c["name"]}: {what} {"everywhere" if everywhere else "in the last (item, row)"}', cf.judge(y, ops['ref'])))
    return out


def test_the_checker_rejects_every_planted_fault(faulted):
    """(for the ring case `bm` is the tile height, so its "last M-tile" is every row -- the glds case's last tile of 96 is rows 96..103)"""
    passed = [(name, v) for name, v in faulted if v['ok']]
    assert not passed, passed
    assert all(v['worst'] > 10 * cf.BLOCK_BAR for _, v in faulted), [(n, v['worst']) for n, v in faulted]


def test_the_global_bar_alone_misses_some(faulted):
    """At the table's small shapes a fault that hits a whole column of every row is visible to the global rel-L2 as well
    (sqrt(2 / T) >= 6 %); it is a fault in ONE (item, row) of a long launch -- what one broken block leaves -- that the 2e-3 bar passes."""
    missed = [name for name, v in faulted if v['ok_global']]
    print('the global bar alone passes:', missed)
    assert missed
    assert 'skinny4 long rows: last column in the last (item, row)' in missed


def test_nan_and_shape_are_failures():
    ref = torch.randn(2, 20, 3, 70, dtype=torch.float64)
    got = ref.clone()
    got[1, 19, 2, 69] = float('nan')
    v = cf.judge(got, ref)
    assert not v['ok'] and v['nbad'] == 1 and v['where'] == (1, 1, 2, 1)
    with pytest.raises(AssertionError):
        cf.block_errors(ref[:, :16], ref)


@pytest.mark.parametrize('name', [c['name'] for c in cf.CASES if c['name'] not in EMU_OMITTED])
def test_emulator(emu, name):
    cf.check_case(emu, 'cpu', cf.BY_NAME[name])
