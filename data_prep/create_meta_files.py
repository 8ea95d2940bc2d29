"""`python data_prep/create_meta_files.py <data_dir> <target_dir> <json_filename> [--n_samples_limit N] [--n_train_dirs K]`

The reference's data_prep/create_meta_files.py on `audio_io.info` (header reads only; neither torchaudio nor sox): walks the speaker
directories of <data_dir> in sorted order, lists every `*_mic1.wav` with its length in samples, and writes
<target_dir>/tr/<json_filename>.json from the first K directories and <target_dir>/val/<json_filename>.json from the rest, each
`[[path, n_samples], ...]`, sorted -- the lists `aero_amd.data.LrHrSet` reads (run it once per side: json_filename `lr`, then `hr`).
The reference asserts VCTK's 108 speakers, 100 of them for training; here that split is `--n_train_dirs` (default 100) and any number
of directories is accepted."""
import argparse
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FILE_PATTERN = '*_mic1.wav'


def subdirs_meta(paths, n_samples_limit, pattern=FILE_PATTERN):
    from aero_amd import audio_io
    meta = []
    for d in paths:
        for file in glob.glob(os.path.join(d, pattern)):
            meta.append((file, audio_io.info(file)[0]))
    meta.sort()
    return meta[:n_samples_limit] if n_samples_limit else meta


def create_meta(data_dir, n_samples_limit=None, n_train_dirs=100, pattern=FILE_PATTERN):
    root, subdirs, _ = next(os.walk(data_dir, topdown=True))
    subdirs.sort()
    if not 0 < n_train_dirs <= len(subdirs):
        raise SystemExit(f'{data_dir} has {len(subdirs)} directories: --n_train_dirs {n_train_dirs} leaves no training set')
    train = subdirs_meta([os.path.join(root, d) for d in subdirs[:n_train_dirs]], n_samples_limit, pattern)
    test = subdirs_meta([os.path.join(root, d) for d in subdirs[n_train_dirs:]], n_samples_limit, pattern)
    return train, test


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description='List the wav files of a data directory with their lengths.')
    parser.add_argument('data_dir', help='directory containing source files')
    parser.add_argument('target_dir', help='output directory for created json files')
    parser.add_argument('json_filename', help='filename for created json files')
    parser.add_argument('--n_samples_limit', type=int, help='limit number of files')
    parser.add_argument('--n_train_dirs', type=int, default=100, help='how many of the sorted directories are the training set')
    return parser.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    print(args)
    train_meta, test_meta = create_meta(args.data_dir, args.n_samples_limit, args.n_train_dirs)
    for part, meta in (('tr', train_meta), ('val', test_meta)):
        os.makedirs(os.path.join(args.target_dir, part), exist_ok=True)
        with open(os.path.join(args.target_dir, part, args.json_filename + '.json'), 'w') as f:
            f.write(json.dumps(meta, indent=4))
    print(f'Done creating meta for {args.data_dir}.')


if __name__ == '__main__':
    main()
