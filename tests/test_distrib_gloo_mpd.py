"""CPU, world_size 2 over gloo, emulated kernels: adversarial steps of `train.py ddp=true` with BOTH critics, discriminator_models
[msd_melgan, mpd] (solver.py:51 wraps every model; train.py:91-96 chains the critics into one Adam).  Each critic's backward averages its
own gradients over the ranks -- one all-reduce per critic per step -- into its range of the shared critic Adam's flat buffer."""
import os
import sys

import torch
import torch.multiprocessing as mp

from conftest import ROOT


def _args():
    from aero_amd.config import _wrap
    gen = dict(channels=16, nfft=128, hop_length=32, lr_sr=4000, hr_sr=16000, enc_freq_attn=4)      # (as test_distrib_gloo.py: no FTB)
    return _wrap(dict(optim='adam', lr=1e-3, beta2=0.999, losses=['l1'], stft_sc_factor=0.5, stft_mag_factor=0.5,
                      experiment=dict(model='aero', aero=gen, adversarial=True, features_loss_lambda=100, only_features_loss=False,
                                      only_adversarial_loss=False, discriminator_models=['msd_melgan', 'mpd'], mpd=dict(hidden=8),
                                      melgan_discriminator=dict(n_layers=4, num_D=2, downsampling_factor=4, ndf=4))))


def _worker(rank, world, port, q, steps):
    try:
        _body(rank, world, port, q, steps)
    except BaseException:
        import traceback
        q.put((rank, 'error', traceback.format_exc()))
        raise


def _body(rank, world, port, q, steps):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), LOCAL_RANK=str(rank),
                      AERO_EMU_THREADS='2')
    torch.set_num_threads(1)
    from aero_amd import _lib, distrib, losses, trainer
    from aero_amd.engine import HipEngine
    from emu.build_emu import build
    lib = _lib.load(build())
    losses.use_library(lib)
    if world > 1:
        distrib.init_from_env(backend='gloo')
    args = _args()
    torch.manual_seed(100 + (rank if world > 1 else 0))       # different initial weights per rank: wrap() must hand out rank 0's
    models = trainer.build_models(args)
    gen, mel, mpd = models['generator'].train(), models['msd_melgan'].train(), models['mpd'].train()
    object.__setattr__(gen, '_engine', HipEngine(gen, lib=lib))
    mel.use_library(lib)
    mpd.use_library(lib)
    opts = trainer.build_optimizers(models, args, lib=lib)
    step = trainer.TrainStep(models, opts, args)
    og, od = opts['optimizer'], opts['disc_optimizer']
    d_start = od.flat_p.clone()
    g_first = None
    for i in range(steps):
        lr = torch.randn(2, 1, 136, generator=torch.Generator().manual_seed(10 + i))
        hr = 0.1 * torch.randn(2, 1, 544, generator=torch.Generator().manual_seed(20 + i))
        rec = step(distrib.shard_batch(lr), distrib.shard_batch(hr))
        assert all(torch.isfinite(v) for v in rec.values()), rec
        assert 'generator_adversarial_mpd' in rec and 'discriminator_mpd' in rec, rec
        if i == 0:
            g_first = od.flat_g.clone()                        # (the buffer still holds the gradients the critic step just used)
    nsync = [mel._grad_sync.launched, mpd._grad_sync.launched] if world > 1 else []
    n_mel = sum((p.numel() + 3) // 4 * 4 for p in mel.parameters())     # the critic Adam's flat buffer: msd_melgan's range, then mpd's
    q.put((rank, og.flat_p.numpy().copy(), od.flat_p.numpy().copy(), d_start.numpy().copy(), g_first.numpy().copy(), nsync, n_mel))
    if world > 1:
        distrib.barrier()
        distrib.close()


def _run(world, port, steps):
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, steps)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    try:
        for _ in range(world):
            r = q.get(timeout=1200)
            assert not (isinstance(r[1], str) and r[1] == 'error'), r[2]
            res[r[0]] = [torch.from_numpy(v) if hasattr(v, 'dtype') else v for v in r]
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.terminate()
    return res


def test_two_rank_adversarial_steps_with_mpd_keep_both_critics_in_sync():
    """2 ranks, one clip of a 2-clip batch each, 2 steps: generator and BOTH critics bit-identical on the two ranks; each critic all-reduced
    exactly once per step; the critics' averaged first-step gradient is the one-process gradient of the whole batch, range by range
    (tolerances of test_distrib_gloo.py::test_two_rank_adversarial_steps_keep_generator_and_critic_in_sync)"""
    from emu.build_emu import build
    build()
    steps = 2
    two = _run(2, 37500 + os.getpid() % 2000, steps)
    one = _run(1, 39500 + os.getpid() % 2000, 1)
    (_, g0, d0, ds0, gd0, n0, nm), (_, g1, d1, ds1, gd1, n1, _) = two[0], two[1]
    assert torch.equal(ds0, ds1)                                  # wrap(): both ranks start from rank 0's critics
    assert torch.equal(gd0, gd1)                                  # the same averaged critic gradients on both ranks ...
    assert torch.equal(g0, g1), float((g0 - g1).abs().max())      # ... generator and both critics in sync, bit for bit
    assert torch.equal(d0, d1), float((d0 - d1).abs().max())
    assert n0 == n1 == [steps, steps], n0                          # msd_melgan and mpd: one all-reduce each per step
    assert not torch.equal(d0[:nm], ds0[:nm]) and not torch.equal(d0[nm:], ds0[nm:])
    _, _, _, Ds, Gd, _, _ = one[0]
    assert torch.equal(Ds, ds0)
    cos = lambda a, b: float((a.double() * b.double()).sum() / a.double().norm() / b.double().norm())   # noqa: E731
    for lo, hi in ((0, nm), (nm, gd0.numel())):
        c, r = cos(gd0[lo:hi], Gd[lo:hi]), float(gd0[lo:hi].norm() / Gd[lo:hi].norm())
        assert c > 0.999 and abs(r - 1) < 1e-2, (lo, c, r)
