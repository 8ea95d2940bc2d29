"""CPU, world_size 2 over gloo, emulated kernels: the epoch level of training (aero_amd/solver.py) on two ranks -- the validation
record averaged over the ranks (the msd_melgan critic's terms included), the best decision, who writes files, and a resumed run.  Geometry: tests/solver_cases.py (`EMU`)."""
import os
import sys

import torch
import torch.multiprocessing as mp

from conftest import ROOT


def _worker(rank, world, port, q, cwd, over):
    try:
        _body(rank, world, port, q, cwd, over)
    except BaseException:
        import traceback
        q.put((rank, 'error', traceback.format_exc()))
        raise


def _plain(o):
    """tensors as numpy arrays: they travel through the queue by value (a tensor's shared-memory handle dies with the worker)"""
    if isinstance(o, torch.Tensor):
        return o.detach().cpu().numpy().copy()
    if isinstance(o, dict):
        return {k: _plain(v) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return [_plain(v) for v in o]
    return o


def _body(rank, world, port, q, cwd, over):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), LOCAL_RANK=str(rank),
                      AERO_EMU_THREADS='4')
    torch.set_num_threads(1)
    import data_cases as DC
    import solver_cases as SC
    from aero_amd import data, distrib, solver
    lib = DC.emu_lib()
    if world > 1:
        distrib.init_from_env(backend='gloo')
    os.chdir(cwd)                                                # one working directory for all ranks, as `train.py ddp=true` has
    writes = {'serialize': 0, 'history': 0}
    serialize, dump = data.serialize, solver.json.dump

    def counted_serialize(*a, **k):
        writes['serialize'] += 1
        return serialize(*a, **k)

    class Json:
        dumps = staticmethod(solver.json.dumps)

        @staticmethod
        def dump(*a, **k):
            writes['history'] += 1
            return dump(*a, **k)
    data.serialize, solver.json = counted_serialize, Json
    s = SC.make_solver(cwd, over + ['epochs=1'], lib)
    assert s.history == [] and len(s.cv) == 3
    valid, _ = s.validate(0)                                     # on the weights of `continue_from`: the same in every world
    out = {'valid': valid, 'files': [st for st, _ in s.valid_files]}
    if world > 1:
        s.train()
        s2 = SC.make_solver(cwd, over + ['epochs=2'], lib)       # finds checkpoint.th in the directory: continues at epoch 1
        assert [h['epoch'] for h in s2.history] == [0]
        s2.train()
        out.update(history=s2.history, writes=writes, best={k: v.clone() for k, v in s2.best_states['generator'].items()},
                   weights={n: o.flat_p.clone() for n, o in s2.optimizers.items()},
                   moments={n: o.exp_avg.clone() for n, o in s2.optimizers.items()}, steps=s2.optimizers['optimizer'].step_count)
    q.put((rank, 'ok', _plain(out)))
    if world > 1:
        distrib.barrier()
        distrib.close()


def _run(world, port, cwd, over):
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, cwd, over)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    try:
        for _ in range(world):
            r = q.get(timeout=1800)
            assert r[1] != 'error', r[2]
            res[r[0]] = r[2]
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.terminate()
    return res


def test_two_rank_validation_best_state_files_and_resume(tmp_path):
    import data_cases as DC
    import solver_cases as SC
    from aero_amd import data, trainer
    DC.emu_lib()
    tr, cv, tt = SC.write_sets(tmp_path, SC.EMU)
    base = SC.BASE + SC.EMU.extra + SC.CRITIC_EMU + [f'dset.train={tr}', f'dset.valid={cv}', f'dset.test={tt}', 'cross_valid=true', 'cross_valid_every=1',
                                                     'eval_every=1', 'enhance_samples_limit=-1']
    # the weights both worlds validate: a seeded, untrained generator in a checkpoint
    start = str(tmp_path / 'start.th')
    args = SC.load_args(base + [f'checkpoint_file={start}'])
    torch.manual_seed(11)
    models = trainer.build_models(args)
    data.serialize(models, {}, [], {}, args)
    over = base + [f'continue_from={start}']
    one_dir, two_dir = str(tmp_path / 'one'), str(tmp_path / 'two')
    os.makedirs(one_dir)
    os.makedirs(two_dir)
    two = _run(2, 41500 + os.getpid() % 2000, two_dir, over)
    one = _run(1, 43500 + os.getpid() % 2000, one_dir, over)[0]
    assert one['files'] == ['clip0', 'clip1', 'clip2'] and two[0]['files'] == ['clip0', 'clip2'] and two[1]['files'] == ['clip1']
    # a file-weighted fp32 mean of three values: only the summation order differs between one rank and two -> 1e-6 relative
    assert two[0]['valid'] == two[1]['valid'] and set(one['valid']) == set(two[0]['valid']) == {
        'total', 'evaluation', 'generator_stft', 'generator_adversarial_melgan', 'generator_features_melgan', 'discriminator_msd_melgan'}
    for k, v in one['valid'].items():
        assert abs(two[0]['valid'][k] - v) <= 1e-6 * abs(v), (k, v, two[0]['valid'][k])
    # both ranks took the same best decision, on the same numbers
    assert two[0]['history'] == two[1]['history'] and [h['epoch'] for h in two[0]['history']] == [0, 1]
    assert [('best_loss' in h, 'valid_evaluation_loss' in h) for h in two[0]['history']] == [(True, True)] * 2
    # (every weight; the BatchNorm running statistics are each rank's own after the last step of an epoch, as under DistributedDataParallel,
    # whose buffers follow rank 0 at the NEXT training forward: distrib.DataParallel._broadcast_buffers)
    differ = [k for k, v in two[0]['best'].items() if not (v == two[1]['best'][k]).all()]
    assert all(k.endswith(('running_mean', 'running_var')) for k in differ), differ
    # only rank 0 wrote: one checkpoint and one history file per epoch, none from rank 1
    assert two[0]['writes'] == {'serialize': 2, 'history': 2} and two[1]['writes'] == {'serialize': 0, 'history': 0}
    assert sorted(os.listdir(two_dir)) == ['checkpoint.th', 'generator_best.th', 'history.json', 'msd_melgan_best.th', 'samples']
    # the samples are each rank's own files, as in the reference: together, every file of the test set
    assert sorted(os.listdir(os.path.join(two_dir, 'samples'))) == sorted(f'clip{k}_{w}.wav' for k in range(3) for w in ('lr', 'hr', 'pr'))
    assert all('lsd' in h and h['visqol'] == 0 for h in two[0]['history'])
    # the resumed two-rank run leaves both ranks with identical weights and moments
    assert two[0]['steps'] == two[1]['steps'] == 4
    for key in ('weights', 'moments'):
        for n, v in two[0][key].items():
            assert v.shape == two[1][key][n].shape and (v == two[1][key][n]).all(), (key, n)
