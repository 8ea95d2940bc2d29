"""CPU: the training data path (aero_amd/data.py, csrc/k_data.h, the additions to aero_amd/audio_io.py) -- the index arithmetic against the
reference's recorded load calls, the wav reader, aero_segment_gather on the emulator bit-equal to the host reader, the resampled lr side,
the sampler against torch's DistributedSampler, the checkpoint package through enhance.load_generator, train.py's choice of mode."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import data_cases as DC
from aero_amd import audio_io, data
from conftest import GOLDEN, ROOT, rel_l2


@pytest.fixture(scope='module')
def lib():
    return DC.emu_lib()


@pytest.fixture(scope='module')
def golden():
    with open(os.path.join(GOLDEN, 'data_index.json')) as f:
        return json.load(f)


# ------------------------------------------------------------------ index arithmetic against the reference's record
PARAMS = [(None, None, True), (10, 10, True), (10, 10, False), (10, 4, True), (10, 15, True), (300, 300, True), (300, 300, False)]


@pytest.mark.parametrize('length,stride,pad', PARAMS)
def test_audioset_index_arithmetic(golden, length, stride, pad):
    assert golden['file_lengths'] == [5, 10, 20, 25, 257]
    case = next(c for c in golden['audioset'] if (c['length'], c['stride'], c['pad']) == (length, stride, pad))
    files = [[f'f{n}.wav', n] for n in golden['file_lengths']]
    ds = data.Audioset(files, length=length, stride=stride, pad=pad, sample_rate=16000, channels=1)
    assert len(ds) == case['len'] == len(case['loads'])
    for i, (name, offset, frames) in enumerate(case['loads']):
        f, o, n = ds.locate(i)
        assert (files[f][0], o, n or -1) == (name, offset, frames), i
    with pytest.raises(IndexError):
        ds.locate(len(ds))


def test_lrhrset_index_arithmetic_and_file_order(golden, tmp_path):
    assert len(golden['lrhr']) == 5
    for k, case in enumerate(golden['lrhr']):
        d = tmp_path / f'c{k}'
        d.mkdir()
        lr = [[f'lr/{nm}', n] for nm, n in zip(case['names'], case['lr_lengths'])]
        hr = [[f'hr/{nm}', n * case['hr_sr'] // case['lr_sr']] for nm, n in zip(case['names'], case['lr_lengths'])]
        json.dump(lr, open(d / 'lr.json', 'w'))
        json.dump(hr, open(d / 'hr.json', 'w'))
        ds = data.LrHrSet(str(d), case['lr_sr'], case['hr_sr'], stride=case['stride'], segment=case['segment'], pad=case['pad'], upsample=False)
        assert len(ds) == case['len']
        assert [os.path.basename(f) for f, _ in ds.lr_set.files] == case['lr_order']
        assert [os.path.basename(f) for f, _ in ds.hr_set.files] == case['hr_order']
        for i, rec in enumerate(case['loads']):
            for side, s in (('lr', ds.lr_set), ('hr', ds.hr_set)):
                f, o, n = s.locate(i)
                assert [os.path.basename(s.files[f][0]), o, n or -1] == rec[side], (k, i, side)


def test_lrhrset_refuses_what_the_reference_would_misalign(tmp_path):
    """equal totals, different counts per file: lr (25, 5) gives 3 + 1 segments of 10, hr (20, 50) at twice the rate gives 1 + 3 of 20"""
    json.dump([['a.wav', 25], ['b.wav', 5]], open(tmp_path / 'lr.json', 'w'))
    json.dump([['a.wav', 20], ['b.wav', 50]], open(tmp_path / 'hr.json', 'w'))
    with pytest.raises(ValueError, match='segments'):
        data.LrHrSet(str(tmp_path), 2, 4, stride=5, segment=5)
    with pytest.raises(NotImplementedError):
        data.LrHrSet(str(tmp_path), 2, 4, stft=True)


def test_audioset_raises_the_references_errors(tmp_path):
    p = str(tmp_path / 'x.wav')
    DC.write_wav(p, DC.noise_i16(50, 1, channels=2), 8000, False)
    with pytest.raises(RuntimeError, match='sample rate of 16000, but got 8000'):
        data.Audioset([[p, 50]], length=10, sample_rate=16000, channels=2)[0]
    with pytest.raises(RuntimeError, match='shape of 1, but got 2'):
        data.Audioset([[p, 50]], length=10, sample_rate=8000, channels=1)[0]
    out, path = data.Audioset([[p, 50]], length=20, sample_rate=8000, channels=2, with_path=True)[2]
    assert path == p and out.shape == (2, 20) and float(out[:, 10:].abs().sum()) == 0 and float(out[:, :10].abs().sum()) > 0


# ------------------------------------------------------------------ audio_io
@pytest.mark.parametrize('f32', [False, True])
@pytest.mark.parametrize('channels', [1, 2])
def test_info_and_partial_load(tmp_path, f32, channels):
    p = str(tmp_path / 'a.wav')
    a = DC.noise_i16(101, 7, channels=channels)
    DC.write_wav(p, a, 11025, f32)
    assert audio_io.info(p) == (101, 11025, channels)
    assert audio_io.encoding(p) == ('f32' if f32 else 'pcm16')
    full, sr = audio_io.load(p)
    assert sr == 11025 and full.dtype == torch.float32
    assert torch.equal(full, torch.from_numpy(a.astype(np.float32) / 32768.0).T)
    for off, n in ((0, -1), (0, 10), (7, 20), (95, 20), (100, 1), (101, 5), (300, 5), (13, -1), (0, 101)):
        part, sr = audio_io.load(p, frame_offset=off, num_frames=n)
        assert sr == 11025 and torch.equal(part, full[:, off:] if n < 0 else full[:, off:off + n]), (off, n)


def test_load_skips_other_chunks_and_odd_padding(tmp_path):
    """a LIST chunk of odd size between fmt and data: found by walking the headers, not by reading the bodies"""
    p = str(tmp_path / 'b.wav')
    a = DC.noise_i16(33, 8)
    DC.write_wav(p, a, 16000, False)
    raw = open(p, 'rb').read()
    extra = b'LIST' + (3).to_bytes(4, 'little') + b'abc\x00'
    open(p, 'wb').write(raw[:36] + extra + raw[36:])
    assert audio_io.info(p) == (33, 16000, 1)
    assert torch.equal(audio_io.load(p, 30, 10)[0], torch.from_numpy(a[30:].astype(np.float32) / 32768.0)[None])


# ------------------------------------------------------------------ aero_segment_gather on the emulator
@pytest.mark.parametrize('f32', [False, True])
@pytest.mark.parametrize('L', DC.GATHER_L)
def test_segment_gather_is_bit_equal_to_the_host_reader(lib, tmp_path, f32, L):
    DC.check_gather(lib, tmp_path, f32, L, 'cpu')


def test_segment_gather_argument_errors(lib):
    a = torch.zeros(16, dtype=torch.int16)
    t64, t32, out = torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), torch.empty(1, 8)
    ok = [a.data_ptr(), 0, t64.data_ptr(), t64.data_ptr(), 1, t32.data_ptr(), t64.data_ptr(), 1, 8, out.data_ptr(), None]
    for pos, bad in ((7, 0), (7, -3), (2, None), (5, None), (0, None), (9, None), (8, 0), (4, 0), (0, a.data_ptr() + 1)):
        args = list(ok)
        args[pos] = bad
        rc = lib.cdll.aero_segment_gather(*args)
        assert rc < 0 and b'aero_segment_gather' in lib.cdll.aero_last_error(), (pos, bad)
    assert lib.cdll.aero_segment_gather(*ok) == 0


def test_segment_gather_out_of_table_file_and_negative_start(lib):
    """an item_file outside the table is a zero row; samples in front of a file's first are zero like those behind its last"""
    arena = torch.arange(1, 41, dtype=torch.float32)
    off, ln = torch.tensor([4, 20]), torch.tensor([10, 20])
    out = data.segment_gather(lib, arena, off, ln, torch.tensor([0, 5, -1, 1], dtype=torch.int32), torch.tensor([-3, 0, 0, 18]), 16)
    ref = torch.zeros(4, 16)
    ref[0, 3:13] = arena[4:14]
    ref[3, :2] = arena[38:40]
    assert torch.equal(out, ref)


# ------------------------------------------------------------------ the store against the host set
@pytest.mark.parametrize('f32', [False, True])
@pytest.mark.parametrize('seg', [64, 100, None])
def test_store_batches_equal_the_stacked_host_items(lib, tmp_path, f32, seg):
    lengths = (257, 257) if seg is None else (1, 5, 64, 257, 300)
    ds = DC.make_set(tmp_path, 'set', 4000, 16000, lengths, seg, f32=f32)
    store = data.DeviceLrHrStore(ds, 'cpu', lib=lib)
    assert store.sides[0].arena.dtype == (torch.float32 if f32 else torch.int16) and len(store) == len(ds)
    idx = list(range(len(ds)))[::-1] + [0, 0]
    lr, hr = store.batch(idx)
    lr_ref, hr_ref = DC.stacked(ds, idx)
    assert torch.equal(lr, lr_ref) and torch.equal(hr, hr_ref)
    lr1, hr1 = data.host_batch(ds, idx, 'cpu')
    assert torch.equal(lr1, lr_ref) and torch.equal(hr1, hr_ref)


def test_store_mixed_encodings_use_an_fp32_arena_and_the_budget_is_kept(lib, tmp_path):
    ds = DC.make_set(tmp_path, 'mix', 4000, 16000, (70, 130), 64)
    p = ds.lr_set.files[1][0]
    DC.write_wav(p, DC.noise_i16(130, 9), 4000, True)
    store = data.DeviceLrHrStore(ds, 'cpu', lib=lib)
    assert store.sides[0].arena.dtype == torch.float32 and store.sides[1].arena.dtype == torch.int16
    assert store.nbytes == 4 * 200 + 2 * 800
    idx = list(range(len(ds)))
    lr_ref, hr_ref = DC.stacked(ds, idx)
    lr, hr = store.batch(idx)
    assert torch.equal(lr, lr_ref) and torch.equal(hr, hr_ref)
    assert data.DeviceLrHrStore(ds, 'cpu', max_bytes=store.nbytes - 1, lib=lib) is None
    assert data.DeviceLrHrStore(ds, 'cpu', max_bytes=store.nbytes, lib=lib) is not None


@pytest.mark.parametrize('lr_sr,hr_sr,seg', DC.UPSAMPLE_CASES)
def test_store_upsamples_the_cut_segment(lib, tmp_path, lr_sr, hr_sr, seg):
    DC.check_upsample(lib, tmp_path, lr_sr, hr_sr, seg, 'cpu', rel_l2)


# ------------------------------------------------------------------ the sampler
@pytest.mark.parametrize('n', [1, 7, 16])
@pytest.mark.parametrize('world', [1, 2, 8])
def test_epoch_sampler_equals_distributed_sampler(n, world):
    from torch.utils.data.distributed import DistributedSampler
    for shuffle in (True, False):
        for epoch in (0, 1):
            seen = []
            for rank in range(world):
                ref = DistributedSampler(range(n), num_replicas=world, rank=rank, shuffle=shuffle, seed=2036)
                ref.set_epoch(epoch)
                mine = data.EpochSampler(n, world, rank, shuffle=shuffle, seed=2036, epoch=epoch)
                assert list(mine) == list(ref) and len(mine) == len(ref)
                seen += list(mine)
            assert set(seen) == set(range(n))
    if n > 2:
        assert data.EpochSampler(n, 1, 0, True, 2036, 0).indices() != data.EpochSampler(n, 1, 0, True, 2036, 1).indices()


# ------------------------------------------------------------------ checkpoint, mode
def tiny_args(tmp_path, *extra):
    from aero_amd.config import load_config
    return load_config(os.path.join(ROOT, 'conf'), ['experiment=aero_4-16_512_64', 'experiment.aero.channels=8',
                                                    f'checkpoint_file={tmp_path}/checkpoint.th', *extra])


def test_checkpoint_package_loads_through_load_generator(tmp_path):
    from aero_amd import enhance, trainer
    args = tiny_args(tmp_path, 'experiment.adversarial=false')
    torch.manual_seed(3)
    models = trainer.build_models(args)
    opt = {'optimizer': torch.optim.Adam(models['generator'].parameters(), lr=args.lr)}
    hist = [{'epoch': 0, 'steps': 2, 'total': 1.5}]
    data.serialize(models, opt, hist, {}, args)
    assert os.listdir(tmp_path) == ['checkpoint.th']                                    # (the .tmp file was renamed into place)
    pkg = enhance.load_package(args.checkpoint_file)
    assert set(pkg) == {'models', 'optimizers', 'history', 'best_states', 'args'}
    g = pkg['models']['generator']
    assert g['class'] is type(models['generator']) and g['args'] == () and g['kwargs'] == dict(args.experiment.aero)
    assert pkg['history'] == hist and pkg['best_states'] == {} and pkg['args'].experiment.name == args.experiment.name
    assert pkg['optimizers']['optimizer']['param_groups'][0]['lr'] == args.lr
    loaded = enhance.load_generator(args, device='cpu')
    want = models['generator'].state_dict()
    got = loaded.state_dict()
    assert set(got) == set(want) and all(torch.equal(got[k], want[k]) for k in want)


def test_train_py_takes_real_data_only_where_the_lists_exist(tmp_path):
    from aero_amd import trainer
    assert trainer.data_source(tiny_args(tmp_path), torch.device('cpu')) is None                       # conf/dset/debug.yaml: no such directory
    ds = DC.make_set(tmp_path, 'tr', 4000, 16000, (9000, 4100, 8000), 8000)
    d = os.path.join(str(tmp_path), 'tr')
    assert trainer.data_source(tiny_args(tmp_path, f'dset.train={d}', '+synthetic=true'), torch.device('cpu')) is None
    os.rename(os.path.join(d, 'hr.json'), os.path.join(d, 'hr.json.off'))
    assert trainer.data_source(tiny_args(tmp_path, f'dset.train={d}'), torch.device('cpu')) is None
    os.rename(os.path.join(d, 'hr.json.off'), os.path.join(d, 'hr.json'))
    src = trainer.data_source(tiny_args(tmp_path, f'dset.train={d}', '+data_on_device=false', 'num_workers=0'), torch.device('cpu'))
    assert src.kind == 'host' and len(src.dataset) == len(ds) == 4                      # segment 2 s = 8000 lr samples: 2 + 1 + 1
    batches = src.batches(1, 3)
    assert batches == [data.EpochSampler(4, 1, 0, True, 2036, 1).indices()[:3], data.EpochSampler(4, 1, 0, True, 2036, 1).indices()[3:]]
    got = list(src.load(batches))
    assert [tuple(lr.shape) for lr, _ in got] == [(3, 1, 8000), (1, 1, 8000)] and got[0][1].shape == (3, 1, 32000)
    lr_ref, hr_ref = DC.stacked(ds, batches[0])
    assert torch.equal(got[0][0], lr_ref) and torch.equal(got[0][1], hr_ref)


def test_create_meta_files(tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location('create_meta_files', os.path.join(ROOT, 'data_prep', 'create_meta_files.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for k, (spk, n) in enumerate((('p3', 30), ('p1', 10), ('p2', 20), ('p1', 11))):
        os.makedirs(tmp_path / 'wav' / spk, exist_ok=True)
        DC.write_wav(str(tmp_path / 'wav' / spk / f'{spk}_{k}_mic1.wav'), DC.noise_i16(n, k), 16000, k % 2 == 0)
    DC.write_wav(str(tmp_path / 'wav' / 'p1' / 'p1_9_mic2.wav'), DC.noise_i16(5, 9), 16000, False)          # not the pattern
    mod.main([str(tmp_path / 'wav'), str(tmp_path / 'egs'), 'hr', '--n_train_dirs', '2'])
    tr = json.load(open(tmp_path / 'egs' / 'tr' / 'hr.json'))
    val = json.load(open(tmp_path / 'egs' / 'val' / 'hr.json'))
    assert [(os.path.basename(f), n) for f, n in tr] == [('p1_1_mic1.wav', 10), ('p1_3_mic1.wav', 11), ('p2_2_mic1.wav', 20)]
    assert [(os.path.basename(f), n) for f, n in val] == [('p3_0_mic1.wav', 30)]
    with pytest.raises(SystemExit):
        mod.main([str(tmp_path / 'wav'), str(tmp_path / 'egs'), 'hr'])                    # the default 100 of 3 directories
