"""List every conv launch of Aero.forward (full config) with the kernel aero_conv_kernel_name dispatches it to.
Runs on the CPU emulation (test double) -- the dispatch is a pure function of the descriptor -- at a small batch/length,
with the descriptors rescaled to the bench shape (B, T) before the name query.  python tools/list_convs.py [B] [T]

python tools/list_convs.py --json OUT   writes the dispatch table tests/test_conv_dispatch.py pins (tests/golden/conv_dispatch.json):
the same spy over the `full` and the music model at the shapes of MODEL_SHAPES plus the hand-written descriptors of hand_entries(), each
with what aero_conv_kernel_name of the gfx950 library (AERO_HIP_LIB, default the in-tree build) answers: under the default environment
(`expect`) and, where it differs, under each switch of SWITCHES (`env`; one child process per switch, the library caches them).
python tools/list_convs.py --query FIXTURE   prints the answers of the loaded library for every entry of FIXTURE as one JSON list
(no torch, no model: ctypes calls on descriptors with fake, correctly aligned pointers)."""
import ctypes as C
import importlib.util
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MODEL_SHAPES = {'full': [(64, 501), (16, 501), (1, 501), (64, 376)], 'music': [(2, 1724)]}
# the conv switches documented in README.md, one child process each
SWITCHES = ['AERO_CONV_RING=0', 'AERO_CONV_RING=1', 'AERO_CONV_BM256=0', 'AERO_CONV_BM256=1', 'AERO_CONV_GLDS=0', 'AERO_CONV_MODE=1',
            'AERO_CONV_MODE=2', 'AERO_CONV_SKINNY=0', 'AERO_CONV_STREAM=0', 'AERO_CONV_TINY_OFF=1', 'AERO_CONVTR_CARRY=0',
            'AERO_RING_192X128=0', 'AERO_RING_256X128=0', 'AERO_RING_256X128=1', 'AERO_RING_TILE192=0', 'AERO_RING_HALF=0',
            'AERO_RING_HALF=2', 'AERO_RING_KMIN256=1024', 'AERO_CONV_KMIN192=768']


def load_lib():
    """aero_amd/_lib.py by path: the package itself imports torch, the binding does not"""
    spec = importlib.util.spec_from_file_location('aero_lib_binding', os.path.join(ROOT, 'aero_amd', '_lib.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, mod.load()


def _is_ptr(ctype):
    return ctype is C.c_void_p


def desc_to_entry(_lib, d):
    """numeric fields that are not zero; every pointer field as None (NULL) or its address mod 16; df / dt cut to ntaps"""
    e = {}
    for name, ctype in _lib.ConvDesc._fields_:
        v = getattr(d, name)
        if _is_ptr(ctype):
            e[name] = None if not v else v % 16
        elif name in ('df', 'dt'):
            e[name] = list(v)[:max(0, min(9, d.ntaps))]
        elif v:
            e[name] = v
    return e


def fill_desc(_lib, e):
    d = _lib.ConvDesc()
    for name, ctype in _lib.ConvDesc._fields_:
        v = e.get(name)
        if _is_ptr(ctype):
            setattr(d, name, None if v is None else (1 << 20) + v)
        elif name in ('df', 'dt'):
            for j, x in enumerate(v or []):
                getattr(d, name)[j] = x
        elif v:
            setattr(d, name, v)
    return d


def query(_lib, lib, e):
    """the kernel name, or [return code, error text]"""
    buf = C.create_string_buffer(128)
    rc = lib.cdll.aero_conv_kernel_name(C.byref(fill_desc(_lib, e)), buf, 128)
    return buf.value.decode() if rc == 0 else [rc, lib.cdll.aero_last_error().decode()]


def hand(**kw):
    """a plain aligned fp16 conv, channels-last and dense; kw overrides (pointers: None, or the address mod 16)"""
    g = dict(C0=64, C1=0, M=64, B=2, Fin=8, Fout=8, T=300, ntaps=1)
    g.update({k: kw[k] for k in g if k in kw})
    cin = g['C0']
    e = dict(src0=0, s0_t=cin, s0_f=g['T'] * cin, s0_b=g['Fin'] * g['T'] * cin, src1=None, weight=0, bias=None, dst=0,
             d_t=g['M'], d_f=g['T'] * g['M'], d_b=g['Fout'] * g['T'] * g['M'], dst_F=g['Fout'], fstride=1, df=[0] * g['ntaps'],
             dt=[0] * g['ntaps'], res=None, post_add=None, batch_scale=None, batch_shift=None, stats=None, gamma=None, beta=None,
             layer_scale=None, weight_tiled=None, split_acc=None, tail_w=None, tail_lo=None, tail_hi=None)
    e.update(g)
    e.update(kw)
    return {k: v for k, v in e.items() if v or v is None or k in ('df', 'dt') or (k in POINTERS and v == 0)}


POINTERS = ('src0', 'src1', 'weight', 'bias', 'dst', 'res', 'post_add', 'batch_scale', 'batch_shift', 'stats', 'gamma', 'beta', 'layer_scale',
            'weight_tiled', 'split_acc', 'tail_w', 'tail_lo', 'tail_hi')
T3 = dict(ntaps=3, dt=[-1, 0, 1])                               # three unit-stride time taps
T9 = dict(ntaps=9, df=[-1] * 3 + [0] * 3 + [1] * 3, dt=[-1, 0, 1] * 3)
STATS = dict(stat_mode=1, stats=0, stat_G=1)
RES = dict(res=0, r_t=8, r_f=8, r_b=8)                          # (keeps an M = 16 conv off the skinny kernel)
TAIL = dict(M=192, C0=256, act=3, tail_w=0, tail_lo=0, tail_hi=0, tail_cp=96, **T3)


def hand_entries():
    """what the models do not reach: (label, descriptor)"""
    out = [('tiny', hand(C0=2, M=2, d_f=2, d_t=16, d_b=300 * 16)),
           ('stream', hand(C0=32, M=8)),
           ('skinny8 two sources', hand(C0=32, C1=32, M=8, src1=0, s1_t=32, s1_f=300 * 32, s1_b=8 * 300 * 32)),
           ('skinny8 strided dst', hand(C0=32, M=8, d_t=16, d_f=300 * 16, d_b=8 * 300 * 16)),
           ('skinny4', hand(C0=4, M=16)), ('skinny2', hand(C0=2, M=16)), ('skinny1', hand(C0=1, M=16)),
           ('skinny4 src at 8 mod 16', hand(C0=32, M=8, src0=8))]
    for c in (32, 64, 96, 128):                 # (128 channels: eight K-chunks, two more than the stream form's slots -- not carried)
        out.append((f'carry C0={c}', hand(C0=c, M=2, transposed=1, fstride=2, Fin=8, Fout=16, dst_F=16, ntaps=2, df=[0, -1], dt=[0, 0])))
    ring = dict(C0=256, weight_tiled=0, **T3)
    out += [('ring 256x128', hand(M=256, tiled_bm=256, T=300, **ring)), ('ring 256x256', hand(M=256, tiled_bm=256, T=501, **ring)),
            ('ring 256 one tap', hand(M=256, C0=384, weight_tiled=0, tiled_bm=256)), ('ring 96', hand(M=96, tiled_bm=96, **ring)),
            ('ring 192', hand(M=192, tiled_bm=192, **ring)), ('ring 128', hand(M=128, tiled_bm=128, **ring)),
            ('ring 64', hand(M=64, tiled_bm=64, **ring)), ('ring 256 stats', hand(M=256, tiled_bm=256, **ring, **STATS)),
            ('ring declined: wrong weight image', hand(M=192, tiled_bm=128, **ring)),
            ('ring 192 fused tail', hand(weight_tiled=0, tiled_bm=192, **TAIL))]
    for st in ({}, STATS):
        out += [('glds8 256', hand(M=256, C0=1024, **st)), ('glds8 192', hand(M=192, C0=384, **st))]
        for M in (128, 96, 64, 48, 32, 16):
            keep = RES if M == 16 and not st else {}
            out += [(f'glds M={M} KC 32', hand(M=M, C0=32, **st, **keep)),
                    (f'glds M={M} KC 64', hand(M=M, C0=256, B=1, Fout=2, Fin=2, T=128, **T9, **st, **keep)),
                    (f'generic M={M}', hand(M=M, C0=12, **st, **keep))]
    out += [('glds KC 64 wide', hand(M=128, C0=1024)), ('glds tap split', hand(M=64, C0=64, tap_split=3, split_acc=0, dst=None, **T3)),
            ('glds scatter', hand(M=64, scatter_M=32, scatter_stride=64, scatter_F=8)), ('glds f32 dst', hand(M=64, dst_f32=1)),
            ('generic irregular taps', hand(M=64, ntaps=2, df=[0, 1], dt=[0, 1]))]
    # one per error text, in the order the checks run
    out += [('err', hand(weight=None)), ('err', hand(**dict(TAIL, tail_lo=None))), ('err', hand(**dict(TAIL, M=96))),
            ('err', hand(tap_split=2)), ('err', hand(ntaps=10, df=[0] * 9, dt=[0] * 9)), ('err', hand(M=0)),
            ('err', hand(C1=8)), ('err', hand(src0=None)), ('err', hand(fstride=0)), ('err', hand(M=63, act=3)), ('err', hand(act=5)),
            ('err', hand(stat_mode=4)), ('err', hand(stat_mode=1)), ('err', hand(**dict(STATS, stat_G=8))),
            ('err', hand(act=1, **STATS)), ('err', hand(**dict(STATS, stat_mode=3))),
            ('err', hand(gamma=0, stat_count=4.0, **dict(STATS, stat_mode=3))), ('err', hand(dst_f_off=1, dst_F=7, **STATS)),
            ('err', hand(scatter_M=4)), ('err', hand(dst_f32=1, **STATS)), ('err', hand(post_add=0, **STATS)),
            ('err', hand(B=1 << 20, Fout=1 << 11)), ('err', hand(src0=8, scatter_M=32, scatter_stride=64, scatter_F=8)),
            ('err', hand(tap_split=2, split_acc=0, **T3)), ('err', hand(**TAIL)),
            ('err', hand(scatter_M=32, scatter_stride=64, scatter_F=8, ntaps=2, df=[0, 1], dt=[0, 1])),
            ('err', hand(C0=12, tap_split=3, split_acc=0, **T3)), ('err', hand(**dict(TAIL, C0=12)))]
    return out


def spy_model(which, on_desc):
    """one forward of the `which` model on the CPU emulation; on_desc(lib, d) sees every aero_conv_fwd descriptor before its launch"""
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from conftest import build_model
    from aero_amd import _lib
    from aero_amd.engine import HipEngine
    from emu.build_emu import build
    meta = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'meta.json')))
    lib = _lib.load(build())
    m = build_model(meta, which)
    object.__setattr__(m, '_engine', HipEngine(m, lib=lib))
    orig_call = lib.call

    def call(name, *args):
        if name == 'aero_conv_fwd':
            on_desc(lib, args[0]._obj)
        orig_call(name, *args)

    lib.call = call
    try:
        with torch.no_grad():
            m(torch.randn(1, 1, 1000))
    finally:
        lib.call = orig_call


def model_entries(_lib):
    """every conv descriptor of the models of MODEL_SHAPES, rescaled to each (B, T) listed there"""
    out = []
    for which, shapes in MODEL_SHAPES.items():
        n = [0]

        def on_desc(lib, d):
            b, t = d.B, d.T
            for Bq, Tq in shapes:
                d.B, d.T = Bq, Tq
                out.append((f'{which} ({Bq}, {Tq}) #{n[0]}', desc_to_entry(_lib, d)))
            d.B, d.T = b, t
            n[0] += 1

        spy_model(which, on_desc)
    return out


def write_json(path):
    _lib, lib = load_lib()
    assert not lib.is_emulator, 'the table is recorded from the gfx950 library'
    entries, seen = [], {}
    for origin, e in model_entries(_lib) + hand_entries():
        key = json.dumps(e, sort_keys=True)
        if key in seen:
            continue
        seen[key] = True
        entries.append(dict(origin=origin, desc=e, expect=query(_lib, lib, e)))
    json.dump(entries, open(path, 'w'))
    for sw in SWITCHES:
        k, v = sw.split('=')
        got = json.loads(subprocess.run([sys.executable, os.path.abspath(__file__), '--query', path], env=dict(os.environ, **{k: v}),
                                        check=True, capture_output=True, text=True).stdout)
        moved = 0
        for e, g in zip(entries, got):
            if g != e['expect']:
                e.setdefault('env', {})[sw] = g
                moved += 1
        print(f'{sw}: {moved} of {len(entries)} entries move')
    with open(path, 'w') as f:
        f.write('[\n' + ',\n'.join(json.dumps(e) for e in entries) + '\n]\n')
    print(f'{len(entries)} entries, {len({json.dumps(e["expect"]) for e in entries})} distinct answers -> {path}')


def table(Bq, Tq):
    rows = []

    def on_desc(lib, d):
        b, t = d.B, d.T
        d.B, d.T = Bq, Tq
        buf = C.create_string_buffer(128)
        lib.cdll.aero_conv_kernel_name(C.byref(d), buf, 128)
        d.B, d.T = b, t
        cin = d.C1 + (d.C0 if d.src0 else 0)
        rows.append((buf.value.decode(), d.M, cin, d.ntaps, d.Fin, d.Fout, d.transposed, d.fstride, d.act, d.stat_mode))

    spy_model('full', on_desc)
    print(f'{"kernel":42s} {"M":>4s} {"Cin":>4s} taps {"Fin":>4s} {"Fout":>4s} tr fs act sm   GFLOP at B={Bq} T={Tq}')
    for r in rows:
        gf = 2.0 * Bq * r[5] * Tq * r[1] * r[3] * r[2] / 1e9
        print(f'{r[0]:42s} {r[1]:4d} {r[2]:4d} {r[3]:4d} {r[4]:4d} {r[5]:4d} {r[6]:2d} {r[7]:2d} {r[8]:3d} {r[9]:2d}   {gf:8.2f}')


def main():
    if len(sys.argv) > 2 and sys.argv[1] == '--json':
        write_json(sys.argv[2])
    elif len(sys.argv) > 2 and sys.argv[1] == '--query':
        _lib, lib = load_lib()
        print(json.dumps([query(_lib, lib, e['desc']) for e in json.load(open(sys.argv[2]))]))
    else:
        table(int(sys.argv[1]) if len(sys.argv) > 1 else 64, int(sys.argv[2]) if len(sys.argv) > 2 else 501)


if __name__ == '__main__':
    main()
