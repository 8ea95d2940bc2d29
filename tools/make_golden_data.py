"""Golden fixture of the dataset index arithmetic (reference src/data/audio.py, src/data/datasets.py) for aero_amd/data.py.  Runs only in the
build container (imports the reference checkout given as argv[1], default /root/reference):

    python -B tools/make_golden_data.py [REFERENCE_ROOT]

Writes tests/golden/data_index.json.  torchaudio is absent here: a stub module stands in whose `load` RECORDS its arguments
(file, frame_offset, num_frames) and returns zeros of the length a real file of the listed size would give, so the reference's own
`Audioset.__getitem__` / `LrHrSet.__init__` run untouched and what they ask of the file reader is the record.  Per case the file holds
`len(dataset)`, the load call of every index and, for the LrHrSet cases, the order of both file lists after `match_files`.  Data only:
nothing of the reference is copied."""
import json
import os
import sys
import tempfile
import types

import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, '..', 'tests', 'golden', 'data_index.json')
FILE_LENGTHS = [5, 10, 20, 25, 257]
PARAMS = [(None, None, True), (10, 10, True), (10, 10, False), (10, 4, True), (10, 15, True), (300, 300, True), (300, 300, False)]
# LrHrSet cases: (lr_sr, hr_sr, segment s, stride s, pad), whole seconds (the reference's own F.pad refuses the float lengths that
# fractional seconds give it); the hr files are `hr_sr / lr_sr` times as long as the lr files
PAIRS = [(2, 4, 5, 5, True), (2, 4, 5, 2, True), (2, 4, 5, 5, False), (2, 4, None, None, True), (4, 16, 2, 1, True)]
# listed in this order in the json files; match_files sorts them
NAMES = ['p3_c.wav', 'p1_a.wav', 'p10_e.wav', 'p2_b.wav', 'p1_d.wav']


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else '/root/reference'
    sys.path.insert(0, ref)
    calls, lengths, rates = [], {}, {}
    ta = types.ModuleType('torchaudio')
    taf, tat = types.ModuleType('torchaudio.functional'), types.ModuleType('torchaudio.transforms')

    def load(path, frame_offset=0, num_frames=-1):
        calls.append([os.path.basename(path), frame_offset, num_frames])
        n = lengths[path] - min(frame_offset, lengths[path])
        return torch.zeros(1, n if num_frames < 0 else min(n, num_frames)), rates[path]
    ta.load, ta.get_audio_backend = load, lambda: 'soundfile'
    taf.resample = lambda sig, a, b: sig
    tat.Spectrogram = object
    ta.functional, ta.transforms = taf, tat
    sys.modules.update({'torchaudio': ta, 'torchaudio.functional': taf, 'torchaudio.transforms': tat})
    for name in ('cv2',):                                        # imported by src/utils.py at module level, not used here
        try:
            __import__(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
    from src.data.audio import Audioset
    from src.data.datasets import LrHrSet
    out = {'file_lengths': FILE_LENGTHS, 'audioset': [], 'lrhr': []}
    files = [[f'f{n}.wav', n] for n in FILE_LENGTHS]
    for f, n in files:
        lengths[f], rates[f] = n, 16000
    for length, stride, pad in PARAMS:
        ds = Audioset(files, length=length, stride=stride, pad=pad, sample_rate=16000, channels=1)
        del calls[:]
        shapes = [int(ds[i].shape[-1]) for i in range(len(ds))]
        out['audioset'].append(dict(length=length, stride=stride, pad=pad, len=len(ds), loads=list(calls), item_frames=shapes))
    for lr_sr, hr_sr, segment, stride, pad in PAIRS:
        with tempfile.TemporaryDirectory() as d:
            lr = [[os.path.join(d, 'lr', nm), n] for nm, n in zip(NAMES, FILE_LENGTHS)]
            hr = [[os.path.join(d, 'hr', nm), n * hr_sr // lr_sr] for nm, n in zip(NAMES, FILE_LENGTHS)]
            for lst, sr in ((lr, lr_sr), (hr, hr_sr)):
                for f, n in lst:
                    lengths[f], rates[f] = n, sr
            json.dump(lr, open(os.path.join(d, 'lr.json'), 'w'))
            json.dump(hr, open(os.path.join(d, 'hr.json'), 'w'))
            ds = LrHrSet(d, lr_sr, hr_sr, stride=stride, segment=segment, pad=pad, upsample=False)
            loads = []
            for i in range(len(ds)):
                del calls[:]
                ds[i]                                            # (reads hr, then lr)
                loads.append({'hr': calls[0], 'lr': calls[1]})
            out['lrhr'].append(dict(lr_sr=lr_sr, hr_sr=hr_sr, segment=segment, stride=stride, pad=pad, names=NAMES, lr_lengths=FILE_LENGTHS,
                                    len=len(ds), loads=loads,
                                    lr_order=[os.path.basename(f) for f, _ in ds.lr_set.files],
                                    hr_order=[os.path.basename(f) for f, _ in ds.hr_set.files]))
    with open(OUT, 'w') as f:
        json.dump(out, f, indent=1)
    print(OUT, {'audioset': [c['len'] for c in out['audioset']], 'lrhr': [c['len'] for c in out['lrhr']]})


if __name__ == '__main__':
    main()
