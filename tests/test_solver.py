"""CPU: the epoch level of training (aero_amd/solver.py) on the CPU emulation of the kernels (test double), as tests/test_emu_train.py
trains -- resume, validation, best states, evaluation.  Geometry and helpers: tests/solver_cases.py (`EMU`).  The emulated runs are
made once per module and shared; the bars are bit-equalities, because the step is bit-reproducible and any difference is lost state.
Both variants run: `adversarial=false` and the msd_melgan critic (`SC.CRITIC_EMU`: the experiment's width, one scale)."""
import copy
import json
import os

import pytest
import torch

import data_cases as DC
import solver_cases as SC

VARIANTS = {'plain': SC.NO_CRITIC, 'msd_melgan': SC.CRITIC_EMU}


@pytest.fixture(scope='module')
def lib():
    return DC.emu_lib()


@pytest.fixture(scope='module')
def sets(tmp_path_factory):
    return SC.write_sets(tmp_path_factory.mktemp('solver_sets'), SC.EMU)


@pytest.fixture(scope='module')
def runs(lib, sets, tmp_path_factory):
    """run(variant, kind) -> (Solver after training, its directory); every emulated run happens once.
    full: two epochs in one run, validation after each; first: one epoch; resumed: a second run in `first`'s directory with epochs=2;
    blind: two epochs without validation."""
    tr, cv, _ = sets
    root, done = str(tmp_path_factory.mktemp('solver_runs')), {}

    def run(variant, kind):
        if (variant, kind) in done:
            return done[variant, kind]
        base = SC.BASE + SC.EMU.extra + VARIANTS[variant] + [f'dset.train={tr}', 'dset.test=']
        valid = [f'dset.valid={cv}', 'cross_valid=true', 'cross_valid_every=1']
        if kind == 'resumed':
            _, d = run(variant, 'first')
        else:
            d = os.path.join(root, f'{variant}_{kind}')
        over = {'full': valid + ['epochs=2'], 'first': valid + ['epochs=1'], 'resumed': valid + ['epochs=2'],
                'blind': ['dset.valid=', 'epochs=2']}[kind]
        if kind == 'resumed':                                    # (`first`'s own files, before the second run rewrites them)
            first_pkg = torch.load(os.path.join(d, 'checkpoint.th'), weights_only=False)
            assert len(first_pkg['history']) == 1
        done[variant, kind] = (SC.run_cpu(d, base + over, lib), d)
        return done[variant, kind]
    return run


@pytest.mark.parametrize('variant', list(VARIANTS))
def test_resume_is_exact(runs, variant):
    """two epochs in one run == one epoch, then a second run on the same directory with epochs=2: equal history losses, torch.equal on
    every model tensor, every Adam moment, the step counts"""
    full, dfull = runs(variant, 'full')
    res, dres = runs(variant, 'resumed')
    assert [h['epoch'] for h in res.history] == [0, 1] and res.done == full.done // 2      # the second run trained epoch 1 only
    assert SC.losses_of_history(res.history) == SC.losses_of_history(full.history)
    assert 'valid_total_loss' in full.history[0] and 'best_loss' in full.history[1]
    n = SC.assert_same_state(SC.package_of(full), SC.package_of(res))
    a = torch.load(os.path.join(dfull, 'checkpoint.th'), weights_only=False)
    b = torch.load(os.path.join(dres, 'checkpoint.th'), weights_only=False)
    assert SC.assert_same_state(a, b) == n > 100
    assert SC.losses_of_history(a['history']) == SC.losses_of_history(b['history'])
    if variant == 'msd_melgan':
        assert set(a['models']) == {'generator', 'msd_melgan'} and set(a['optimizers']) == {'optimizer', 'disc_optimizer'}
    for name, st in a['best_states'].items():                    # (and the best states travelled with it)
        assert all(torch.equal(st[k], b['best_states'][name][k]) for k in st)


@pytest.mark.parametrize('variant', list(VARIANTS))
def test_validation_leaves_no_trace(runs, variant):
    """two epochs with a validation pass after each and two epochs without end in bit-equal weights and equal training losses"""
    full, _ = runs(variant, 'full')
    blind, _ = runs(variant, 'blind')
    assert not any(k.startswith('valid_') for k in blind.history[1])
    keys = [k for k in blind.history[0] if k == 'total' or k.startswith(('generator_', 'discriminator_'))]
    assert len(keys) >= 2
    for a, b in zip(full.history, blind.history):
        assert {k: a[k] for k in keys} == {k: b[k] for k in keys}
    assert SC.assert_same_state(SC.package_of(full), SC.package_of(blind)) > 100
    assert all(m.training for m in full.models.values())


@pytest.mark.parametrize('variant', list(VARIANTS))
def test_validation_numbers_are_the_definition(runs, lib, variant):
    """per file the recorded terms equal losses_of on match_signal(model.eval()(lr), len(hr)) computed here, the recorded mean is their
    mean, and the host reader gives the records of the device store"""
    from aero_amd import losses
    from aero_amd.solver import EvalSet
    s, _ = runs(variant, 'full')
    losses.use_library(lib)
    try:
        assert s.cv.kind == 'device' and len(s.cv) == 3
        direct = SC.direct_validation(s.step, s.models['generator'], s.cv, range(3))
        mean, _ = s.run_pass(s.cv, True)
        assert [st for st, _ in s.valid_files] == [st for st, _ in direct] == ['clip0', 'clip1', 'clip2']
        for (_, got), (_, want) in zip(s.valid_files, direct):
            assert got == {k: float(v) for k, v in want.items()}
        assert mean == SC.mean_of(direct)
        terms = {'total', 'generator_stft'} | ({'generator_adversarial_melgan', 'generator_features_melgan', 'discriminator_msd_melgan'}
                                              if variant == 'msd_melgan' else set())
        assert set(mean) == terms
        # the last epoch's record is this pass (the weights have not moved since)
        last = s.history[-1]
        assert {k: last[f'valid_{k}_loss'] for k in mean} == mean and last['valid_evaluation_loss'] == mean['total'] == last['evaluation_loss']
        device_files = s.valid_files
        host = EvalSet(s.cv.dataset, None, 'cpu')
        mean_host, _ = s.run_pass(host, True)
        assert host.kind == 'host' and mean_host == mean and s.valid_files == device_files
    finally:
        losses.use_library(None)


def _stubbed(tmp_path, sets, lib, extra, values, lsds=None):
    """a Solver whose training epoch nudges the weights and whose validation returns `values` in turn (host only: no kernel runs)"""
    tr, cv, tt = sets
    over = SC.BASE + SC.EMU.extra + SC.NO_CRITIC + [f'dset.train={tr}', f'dset.valid={cv}', f'dset.test={tt}', 'cross_valid=true',
                                                    'cross_valid_every=1', f'epochs={len(values)}'] + extra
    s = SC.make_solver(str(tmp_path), over, lib)
    seen = {'after': [], 'eval': []}

    def run_epoch(epoch):
        with torch.no_grad():
            for p in s.models['generator'].parameters():
                p.add_(0.01 * (epoch + 1))
        seen['after'].append(copy.deepcopy({k: v.clone() for k, v in s.models['generator'].state_dict().items()}))
        return {'epoch': epoch, 'steps': 1, 'total': 1.0}

    def validate(epoch, enhance=False):
        return {'total': values[epoch], 'evaluation': values[epoch]}, None

    def evaluate(epoch):
        seen['eval'].append(epoch)
        return 7.0 + epoch
    s.run_epoch, s.validate, s.evaluate = run_epoch, validate, evaluate
    return s, seen


def test_best_state_bookkeeping(tmp_path, sets, lib):
    from aero_amd import enhance, losses
    try:
        with SC.in_dir(str(tmp_path)):
            s, seen = _stubbed(tmp_path, sets, lib, ['eval_every=2'], [3.0, 2.0, 2.5])
            s.train()
    finally:
        losses.use_library(None)
    assert [h['best_loss'] for h in s.history] == [3.0, 2.0, 2.0]
    assert [h['valid_evaluation_loss'] for h in s.history] == [3.0, 2.0, 2.5] == [h['evaluation_loss'] for h in s.history]
    assert seen['eval'] == [1, 2] and ['lsd' in h for h in s.history] == [False, True, True] and s.history[2]['visqol'] == 0
    after2 = seen['after'][1]
    assert all(torch.equal(s.best_states['generator'][k], after2[k]) for k in after2)
    assert not torch.equal(seen['after'][2]['decoder.3.conv_tr.weight'], after2['decoder.3.conv_tr.weight'])
    files = sorted(os.listdir(str(tmp_path)))
    assert files == ['checkpoint.th', 'generator_best.th', 'history.json'], files
    pkg = torch.load(str(tmp_path / 'checkpoint.th'), weights_only=False)
    assert json.load(open(str(tmp_path / 'history.json'))) == pkg['history'] == s.history
    best = torch.load(str(tmp_path / 'generator_best.th'), weights_only=False)
    assert set(best) == {'class', 'args', 'kwargs', 'state'} and all(torch.equal(best['state'][k], after2[k]) for k in after2)
    args = SC.load_args(SC.BASE + SC.EMU.extra + [f'checkpoint_file={tmp_path / "checkpoint.th"}', 'continue_best=true'])
    m = enhance.load_generator(args, device='cpu')
    assert all(torch.equal(v, after2[k]) for k, v in m.state_dict().items())
    args.continue_best = False
    m = enhance.load_generator(args, device='cpu')
    assert all(torch.equal(v, seen['after'][2][k]) for k, v in m.state_dict().items())


def test_serialize_without_best_states_writes_the_checkpoint_only(tmp_path, sets, lib):
    from aero_amd import data, losses
    try:
        with SC.in_dir(str(tmp_path)):
            s, _ = _stubbed(tmp_path, sets, lib, [], [1.0])
            data.serialize(s.models, s.optimizers, [], {}, s.args)
    finally:
        losses.use_library(None)
    assert os.listdir(str(tmp_path)) == ['checkpoint.th']


def test_resume_switches(tmp_path, sets, lib):
    """restart=true ignores an existing checkpoint; continue_from with keep_history=false starts at epoch 0 with the loaded weights;
    continue_best=true loads the best weights and fresh optimizers; a plain second run continues (history, optimizers, best states)"""
    from aero_amd import losses
    d = str(tmp_path / 'a')
    try:
        with SC.in_dir(d):
            s, seen = _stubbed(d, sets, lib, [], [3.0, 2.0, 2.5])
            fresh = {k: v.clone() for k, v in s.models['generator'].state_dict().items()}
            s.optimizers['optimizer'].step_count = 5                  # (a state to find again)
            s.optimizers['optimizer'].exp_avg.fill_(0.25)
            s.train()
            last, best = seen['after'][2], seen['after'][1]
            ckpt = os.path.join(d, 'checkpoint.th')
            # a second run in the directory continues
            s2, _ = _stubbed(d, sets, lib, [], [3.0, 2.0, 2.5, 2.25])
            gen = s2.models['generator'].state_dict()
            assert len(s2.history) == 3 and all(torch.equal(gen[k], last[k]) for k in last)
            assert s2.optimizers['optimizer'].step_count == 5 and all(bool((st['exp_avg'] == 0.25).all()) for st in s2.optimizers['optimizer'].state_dict()['state'].values())
            assert all(torch.equal(s2.best_states['generator'][k], best[k]) for k in best)
            s2.train()
            assert [h['epoch'] for h in s2.history] == [0, 1, 2, 3] and [h['best_loss'] for h in s2.history] == [3.0, 2.0, 2.0, 2.0]
            # restart=true
            s3, _ = _stubbed(d, sets, lib, ['restart=true'], [3.0])
            gen = s3.models['generator'].state_dict()
            assert s3.history == [] and s3.best_states == {} and all(torch.equal(gen[k], fresh[k]) for k in fresh)
            assert s3.optimizers['optimizer'].step_count == 0
        pkg = torch.load(ckpt, weights_only=False)
        last, best = pkg['models']['generator']['state'], pkg['best_states']['generator']
        assert not torch.equal(last['decoder.3.conv_tr.weight'], best['decoder.3.conv_tr.weight'])
        with SC.in_dir(str(tmp_path / 'b')):
            s4, _ = _stubbed(tmp_path / 'b', sets, lib, [f'continue_from={ckpt}', 'keep_history=false'], [3.0])
            gen = s4.models['generator'].state_dict()
            assert s4.history == [] and all(torch.equal(gen[k], last[k]) for k in last) and s4.optimizers['optimizer'].step_count == 5
            s4.train()
            assert [h['epoch'] for h in s4.history] == [0]
        with SC.in_dir(str(tmp_path / 'c')):
            s5, _ = _stubbed(tmp_path / 'c', sets, lib, [f'continue_from={ckpt}', 'continue_best=true'], [3.0])
            gen = s5.models['generator'].state_dict()
            assert all(torch.equal(gen[k], best[k]) for k in best) and s5.optimizers['optimizer'].step_count == 0
            assert not bool(s5.optimizers['optimizer'].exp_avg.any()) and len(s5.history) == 4
    finally:
        losses.use_library(None)


def test_evaluation(runs, sets, lib, tmp_path):
    """the lsd of an evaluation equals evaluate.evaluate on the same files with the same weights; with evaluate_on_best it is the best
    state's and the live weights are untouched; samples exist for exactly enhance_samples_limit files"""
    from aero_amd import evaluate, losses
    from aero_amd.solver import EvalSet, eval_sets
    s, _ = runs('plain', 'full')
    first, _ = runs('plain', 'first')                            # (another state of the same model: the weights after epoch 1)
    gen = s.models['generator']
    args = copy.deepcopy(s.args)
    args.dset.test, args.samples_dir, args.enhance_samples_limit = sets[2], str(tmp_path / 'samples'), 2
    old_args, old_best, s.args = s.args, s.best_states, args
    losses.use_library(lib)
    try:
        _, s.tt, same = eval_sets(args, 'cpu', lib=lib)
        assert isinstance(s.tt, EvalSet) and not same and s.tt.dataset.with_path
        pairs = [s.tt.item(i) for i in range(3)]

        def reference():
            tot, n, _ = evaluate.evaluate(gen, pairs, device='cpu')
            return tot / n
        live = {k: v.clone() for k, v in gen.state_dict().items()}
        lsd = s.evaluate(1)
        # a file-weighted fp32 mean of three values against their sum in double: 1e-6 relative covers the summation order
        assert abs(lsd - reference()) <= 1e-6 * reference()
        wavs = sorted(os.listdir(args.samples_dir))
        assert wavs == sorted(f'clip{k}_{w}.wav' for k in (0, 1) for w in ('lr', 'hr', 'pr')), wavs
        # evaluate_on_best
        args.evaluate_on_best = True
        s.best_states = {'generator': {k: v.clone() for k, v in first.models['generator'].state_dict().items()}}
        lsd_best = s.evaluate(1)
        assert all(torch.equal(v, live[k]) for k, v in gen.state_dict().items()) and gen.training
        assert abs(lsd - reference()) <= 1e-6 * reference()       # the live weights measure as before
        gen.load_state_dict(s.best_states['generator'])
        gen.repack()
        want = reference()
        gen.load_state_dict(live)
        gen.repack()
        assert abs(lsd_best - want) <= 1e-6 * want and lsd_best != lsd
    finally:
        s.args, s.tt, s.best_states = old_args, None, old_best
        losses.use_library(None)
