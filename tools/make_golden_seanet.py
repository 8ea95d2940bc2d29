"""Golden fixtures of the Seanet baseline generator (reference src/models/seanet.py) for aero_amd/seanet.py.  Runs only in the build container
(imports the reference checkout given as argv[1], default /root/reference):

    python -B tools/make_golden_seanet.py [REFERENCE_ROOT]

Writes tests/golden/seanet_meta.json (seeds, configurations, per-key (sum, |sum|) checksums of the seeded state dict at ngf 8 and 32, the
valid lengths `estimate_output_length` returns, per case and recorded stage the fp16-operand floor) and tests/golden/seanet_io.npz (per
case the input, the full output and a subsample of the recorded stage outputs).

torchaudio is absent here and the reference module imports `torchaudio.functional.resample` at import time: a stub module stands in for that
import and ONLY `upsample=False` cases are generated, where the reference never calls it -- every golden is the reference's own arithmetic.
Stage outputs are taken with forward hooks on the reference's own `encoder[i]` / `decoder[j]` (its forward runs untouched); a decoder
stage is recorded WITH its skip added (decoder output + the input of the matching encoder stage), which is what the next stage reads.

The fp16-operand floor of a case: the same reference module run in fp32 with the input and the weight of every conv rounded to fp16 (a
forward pre-hook behind the weight-norm hook) -- the arithmetic the kernels are designed to do -- and its rel-L2 distance to the pure-fp32
run, per recorded stage.  Nothing of the reference is copied: the fixtures are seeds, checksums and recorded values."""
import json
import os
import sys
import types

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, '..', 'tests', 'golden')
SEED = {8: 101, 32: 102}
LENGTHS = (1, 7, 999, 2003, 8000, 32000, 32001)
RATIOS = ([8, 8, 2, 2], [4, 2])
CASES = {
    'a': dict(cfg=dict(ngf=8, upsample=False), seed=111, sig_seed=121, B=2, L=2003, stages='all'),
    'b': dict(cfg=dict(ngf=32, upsample=False), seed=112, sig_seed=122, B=2, L=8000, stages=['enc1', 'dec4']),
    'c': dict(cfg=dict(ngf=8, upsample=False, normalize=False), seed=113, sig_seed=123, B=2, L=2003, stages='all'),
    'd': dict(cfg=dict(ngf=8, upsample=False, ratios=[4, 2], n_residual_layers=2), seed=114, sig_seed=124, B=2, L=2003, stages='all'),
}
SIGNAL_SCALE = 0.3


def sub(fm):
    """[B, C, T] -> at most 8 channels x about 256 steps"""
    return fm[:, ::max(1, fm.shape[1] // 8), ::max(1, fm.shape[2] // 256)]


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def run_with_stages(model, x):
    """the reference's own forward; -> (output, {'enc{i}' / 'dec{j}': stage output, decoder stages with their skip added})"""
    enc_in, enc_out, dec_out, hooks = {}, {}, {}, []
    def enc_hook(i):
        def hook(mod, inp, out):
            enc_in[i], enc_out[i] = inp[0].detach(), out.detach()
        return hook

    def dec_hook(j):
        def hook(mod, inp, out):
            dec_out[j] = out.detach()
        return hook
    hooks += [m.register_forward_hook(enc_hook(i)) for i, m in enumerate(model.encoder)]
    hooks += [m.register_forward_hook(dec_hook(j)) for j, m in enumerate(model.decoder)]
    with torch.no_grad():
        y = model(x)
    for h in hooks:
        h.remove()
    n = len(model.encoder)
    stages = {f'enc{i}': enc_out[i] for i in range(n)}
    stages.update({f'dec{j}': dec_out[j] + enc_in[n - 1 - j] for j in range(n)})
    return y, stages


def fp16_operands(model):
    """round every conv's input and weight to fp16 (values kept in fp32): hooks registered behind torch's weight-norm pre-hook"""
    def pre(mod, inp):
        mod.weight = mod.weight.half().float()
        return (inp[0].half().float(),)
    return [m.register_forward_pre_hook(pre) for m in model.modules() if isinstance(m, (torch.nn.Conv1d, torch.nn.ConvTranspose1d))]


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else '/root/reference'
    sys.path.insert(0, ref)
    torch.set_num_threads(8)
    try:
        import torchaudio.functional  # noqa: F401
    except ImportError:
        ta, taf = types.ModuleType('torchaudio'), types.ModuleType('torchaudio.functional')

        def resample(*a, **k):
            raise RuntimeError('torchaudio is not installed: only upsample=False cases are generated')
        taf.resample, ta.functional = resample, taf
        sys.modules['torchaudio'], sys.modules['torchaudio.functional'] = ta, taf
    from src.models.seanet import Seanet
    meta = {'seeds': {str(k): v for k, v in SEED.items()}, 'checksums': {}, 'lengths': {}, 'signal_scale': SIGNAL_SCALE, 'cases': {},
            'subsample': 'fm[:, ::max(1, C // 8), ::max(1, T // 256)]',
            'stages': 'enc{i}: output of encoder[i]; dec{j}: output of decoder[j] + its skip; the last decoder stage is the model output'}
    io = {}
    for ngf, seed in SEED.items():
        torch.manual_seed(seed)
        m = Seanet(ngf=ngf, upsample=False)
        meta['checksums'][str(ngf)] = {k: [float(v.double().sum()), float(v.double().abs().sum())] for k, v in m.state_dict().items()}
        meta['shapes_' + str(ngf)] = {k: list(v.shape) for k, v in m.state_dict().items()}
    for ratios in RATIOS:
        m = Seanet(ngf=8, ratios=ratios, upsample=False)
        meta['lengths'][','.join(map(str, ratios))] = {str(n): m.estimate_output_length(n) for n in LENGTHS}
    for name, case in CASES.items():
        torch.manual_seed(case['seed'])
        model = Seanet(**case['cfg']).eval()
        x = SIGNAL_SCALE * torch.randn(case['B'], 1, case['L'], generator=torch.Generator().manual_seed(case['sig_seed']))
        y, stages = run_with_stages(model, x)
        hooks = fp16_operands(model)
        y16, stages16 = run_with_stages(model, x)
        for h in hooks:
            h.remove()
        n = len(model.encoder)
        stages[f'dec{n - 1}'], stages16[f'dec{n - 1}'] = y, y16     # (the last stage as the model returns it: trimmed, times std)
        keep = sorted(stages) if case['stages'] == 'all' else case['stages']
        floors = {'out': rel_l2(y16, y)}
        io[f'{name}.x'] = x.numpy()
        io[f'{name}.y'] = y.numpy()
        for k in keep:
            io[f'{name}.{k}'] = sub(stages[k]).numpy()
            floors[k] = rel_l2(sub(stages16[k]), sub(stages[k]))
        meta['cases'][name] = dict(cfg=case['cfg'], seed=case['seed'], sig_seed=case['sig_seed'], B=case['B'], L=case['L'], stages=keep,
                                   out_shape=list(y.shape), fp16_floor=floors)
        print(name, tuple(y.shape), {k: f'{v:.2e}' for k, v in floors.items()}, flush=True)
    np.savez_compressed(os.path.join(OUT, 'seanet_io.npz'), **io)
    json.dump(meta, open(os.path.join(OUT, 'seanet_meta.json'), 'w'), indent=1)


if __name__ == '__main__':
    main()
