"""GPU: the epoch level of training on the MI355X -- `train.py` as a child process on wav files (as tests/test_gpu_data.py runs it), then
its checkpoints, history files and samples compared: resume, validation, evaluation.  Geometry and helpers: tests/solver_cases.py
(`GPU`: 1-second items at 4 kHz, whole files of 4100, 8001 and 9000 low-rate samples).  Every child run happens once per module."""
import json
import os
import subprocess
import sys

import pytest
import torch

import solver_cases as SC
from conftest import ROOT

pytestmark = pytest.mark.gpu

VARIANTS = {'plain': SC.NO_CRITIC, 'msd_melgan': SC.CRITIC}
EVAL = ['eval_every=1', 'enhance_samples_limit=2']


@pytest.fixture(scope='module')
def sets(tmp_path_factory):
    return SC.write_sets(tmp_path_factory.mktemp('solver_sets'), SC.GPU)


def overrides(sets, variant, kind):
    tr, cv, tt = sets
    base = SC.BASE + VARIANTS[variant] + [f'dset.train={tr}']
    valid = [f'dset.valid={cv}', f'dset.test={tt}', 'cross_valid=true', 'cross_valid_every=1'] + EVAL
    return base + {'full': valid + ['epochs=2'], 'first': valid + ['epochs=1'], 'resumed': valid + ['epochs=2'],
                   'host': valid + ['epochs=1', '+data_on_device=false'], 'blind': ['dset.valid=', 'dset.test=', 'epochs=2']}[kind]


@pytest.fixture(scope='module')
def runs(sets, tmp_path_factory):
    """run(variant, kind) -> (the JSON lines train.py printed, its directory).  full: two epochs in one process, validation and
    evaluation after each; first: one epoch; resumed: a second process in `first`'s directory with epochs=2; host: `first` with the host
    reader; blind: two epochs without validation or test set."""
    root, done = str(tmp_path_factory.mktemp('solver_runs')), {}

    def run(variant, kind):
        if (variant, kind) in done:
            return done[variant, kind]
        d = run(variant, 'first')[1] if kind == 'resumed' else os.path.join(root, f'{variant}_{kind}')
        os.makedirs(d, exist_ok=True)
        cmd = [sys.executable, os.path.join(ROOT, 'train.py')] + overrides(sets, variant, kind)
        env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK')}
        out = subprocess.run(cmd, cwd=d, env=env, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-3000:]
        done[variant, kind] = ([json.loads(ln) for ln in out.stdout.splitlines() if ln.startswith('{')], d)
        return done[variant, kind]
    return run


def package(d):
    return torch.load(os.path.join(d, 'checkpoint.th'), map_location='cpu', weights_only=False)


@pytest.mark.parametrize('variant', list(VARIANTS))
def test_resume_is_exact(runs, variant):
    """two epochs in one process == one epoch, then a second process on the same directory with epochs=2"""
    full, dfull = runs(variant, 'full')
    first, dres = runs(variant, 'first')
    assert [r['epoch'] for r in first] == [0]
    res, _ = runs(variant, 'resumed')
    assert [r['epoch'] for r in full] == [0, 1] and [r['epoch'] for r in res] == [1]         # the second process ran epoch 1 only
    a, b = package(dfull), package(dres)
    assert [h['epoch'] for h in b['history']] == [0, 1]
    print(SC.losses_of_history(a['history']), SC.losses_of_history(b['history']))
    assert SC.losses_of_history(a['history']) == SC.losses_of_history(b['history'])
    assert SC.assert_same_state(a, b) > 100
    assert json.load(open(os.path.join(dres, 'history.json'))) == b['history']
    assert all(k in b['history'][1] for k in ('valid_total_loss', 'valid_evaluation_loss', 'evaluation_loss', 'best_loss', 'lsd', 'visqol'))
    if variant == 'msd_melgan':
        assert set(a['models']) == {'generator', 'msd_melgan'} and set(a['optimizers']) == {'optimizer', 'disc_optimizer'}
        assert 'valid_discriminator_msd_melgan_loss' in b['history'][1] and 'valid_generator_features_melgan_loss' in b['history'][1]
    assert os.path.exists(os.path.join(dres, 'generator_best.th')) and set(b['best_states']) == set(b['models'])
    for name, st in a['best_states'].items():
        assert all(torch.equal(st[k], b['best_states'][name][k]) for k in st)
    wavs = sorted(os.listdir(os.path.join(dres, 'samples')))
    assert wavs == sorted(f'clip{k}_{w}.wav' for k in (0, 1) for w in ('lr', 'hr', 'pr')), wavs


@pytest.mark.parametrize('variant', list(VARIANTS))
def test_validation_leaves_no_trace(runs, variant):
    full, dfull = runs(variant, 'full')
    blind, dblind = runs(variant, 'blind')
    assert not any(k.startswith('valid_') or k == 'lsd' for k in blind[1])
    keys = [k for k in blind[0] if k == 'total' or k.startswith(('generator_', 'discriminator_'))]
    assert len(keys) >= 2
    for a, b in zip(full, blind):
        assert {k: a[k] for k in keys} == {k: b[k] for k in keys}
    assert SC.assert_same_state(package(dfull), package(dblind)) > 100


def live_solver(sets, variant, d, extra=()):
    """the Solver of a finished run in this process, on the device, continued from the run's checkpoint (no file is written here)"""
    ckpt = os.path.join(d, 'checkpoint.th')
    over = overrides(sets, variant, 'full') + [f'continue_from={ckpt}', 'checkpoint=false', f'samples_dir={os.path.join(d, "again")}'] + list(extra)
    s = SC.make_solver(d, over, None, device='cuda')
    assert len(s.history) == 2
    return s


@pytest.mark.parametrize('variant', list(VARIANTS))
def test_validation_numbers_are_the_definition(runs, sets, variant):
    """the recorded mean of the last epoch equals the mean of losses_of on match_signal(model.eval()(lr), len(hr)) computed here on the
    checkpoint's weights (per file: the pass's own per-file values equal these, bit for bit); the host reader records the same"""
    from aero_amd.solver import EvalSet
    _, dfull = runs(variant, 'full')
    s = live_solver(sets, variant, dfull)
    assert s.cv.kind == 'device' and s.tt.kind == 'device' and not s.valid_equals_test
    direct = SC.direct_validation(s.step, s.models['generator'], s.cv, range(3))
    mean, _ = s.run_pass(s.cv, True)
    for (st, got), (st2, want) in zip(s.valid_files, direct):
        assert st == st2 and got == {k: float(v) for k, v in want.items()}, (st, got, want)
    assert mean == SC.mean_of(direct)
    last = s.history[-1]
    print({k: (last[f'valid_{k}_loss'], v) for k, v in mean.items()})
    assert {k: last[f'valid_{k}_loss'] for k in mean} == mean     # the child process measured the same weights: the same numbers
    assert last['valid_evaluation_loss'] == last['evaluation_loss'] == mean['total']
    device_files = s.valid_files
    mean_host, _ = s.run_pass(EvalSet(s.cv.dataset, None, 'cuda'), True)
    assert mean_host == mean and s.valid_files == device_files
    # ... and as train.py runs it: +data_on_device=false
    first, _ = runs(variant, 'first')
    host, _ = runs(variant, 'host')
    assert first[0]['data'] == 'device' and host[0]['data'] == 'host'
    assert SC.losses_of_history(first) == SC.losses_of_history(host)
    assert all(m.training for m in s.models.values())


def test_evaluation(runs, sets):
    """the lsd of an evaluation epoch equals evaluate.evaluate on the same files with the same weights; with evaluate_on_best it is the
    best state's, and the live weights are untouched afterwards"""
    from aero_amd import evaluate
    _, dfull = runs('plain', 'full')
    s = live_solver(sets, 'plain', dfull)
    gen = s.models['generator']
    pairs = [s.tt.item(i) for i in range(3)]

    def reference():
        tot, n, _ = evaluate.evaluate(gen, pairs, device='cuda')
        return tot / n
    want = reference()
    print('lsd', s.history[-1]['lsd'], want)
    # a file-weighted fp32 mean of three values against their sum in double: 1e-6 relative covers the summation order
    assert abs(s.history[-1]['lsd'] - want) <= 1e-6 * want
    live = {k: v.clone() for k, v in gen.state_dict().items()}
    s.args.evaluate_on_best = True
    # another state of the same model that is known to differ from the live weights: the generator as another seed draws it
    from aero_amd import trainer
    torch.manual_seed(4242)
    other = {k: v.detach().clone() for k, v in trainer.build_models(s.args)['generator'].state_dict().items()}
    assert not torch.equal(other['decoder.3.conv_tr.weight'], live['decoder.3.conv_tr.weight'].cpu())
    s.best_states = {'generator': other}
    lsd_best = s.evaluate(1)
    assert all(torch.equal(v, live[k]) for k, v in gen.state_dict().items()) and gen.training
    s.args.evaluate_on_best = False
    assert abs(s.evaluate(1) - want) <= 1e-6 * want               # the live weights measure as before
    gen.load_state_dict(other)
    gen.repack()
    want_best = reference()
    assert abs(lsd_best - want_best) <= 1e-6 * want_best and lsd_best != want
    wavs = sorted(os.listdir(os.path.join(dfull, 'again')))
    assert wavs == sorted(f'clip{k}_{w}.wav' for k in (0, 1) for w in ('lr', 'hr', 'pr')), wavs
