#!/usr/bin/env python
"""What feeds the train step: the DataLoader path against the resident set (daft_exprt/resident_set.py, csrc/collate.hip).

Fabricates a data set in a temporary directory -- `--utterances` utterances with the length statistics of `SyntheticUtterances`,
written in the reference's file formats (`.npy` mel, `.markers`, one-float-per-line text files) -- and prints one JSON line:
  * loader: utterances/s of `prepare_data_loaders(num_workers=8)` over one epoch (host collate, pinned memory; no step runs);
  * resident_load: the one-off read + pack + upload of the training list, seconds and packed bytes;
  * resident_batches: batches/s of one epoch of the `ResidentLoader` between two device events (order + gather launches only);
  * train_loader_path / train_resident: `train()` over the same `--iterations` iterations on each path: iterations/s from the
    per-iteration durations of metrics.jsonl (the first `--skip` left out) and the wall time of the whole call.
A development aid: `bench.py` does not call it.  At most 8 loader workers + 16 reader threads; reads nothing outside its directory.
Usage: python tools/bench_loader.py [--utterances 2048] [--batch 48] [--iterations 50] [--skip 5]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'ubisoft-laforge-daft-exprt_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

from daft_exprt.data_loader import SyntheticUtterances, prepare_data_loaders  # noqa: E402
from daft_exprt.hparams import HyperParams  # noqa: E402

SPEAKERS = ['spkA', 'spkB', 'spkC', 'spkD']


def _hp(tmp, batch, **kw):
    hp = HyperParams(verbose=False, training_files=os.path.join(tmp, 'train_english.txt'),
                     validation_files=os.path.join(tmp, 'validation_english.txt'), output_directory=os.path.join(tmp, 'out'),
                     language='english', speakers=SPEAKERS, batch_size=batch, accumulation_steps=1, **kw)
    hp.stats = {f'spk {i}': {'energy': {'mean': 30., 'std': 15.}, 'pitch': {'mean': 5., 'std': 0.3}} for i in range(len(SPEAKERS))}
    return hp


def _floats(path, values):
    with open(path, 'w', encoding='utf-8') as f:
        f.write('\n'.join(repr(float(v)) for v in values) + '\n')


def fabricate(tmp, hp, n_items, n_val):
    ds = SyntheticUtterances(hp, n_items, seed=hp.seed, force_first_full=False, n_speakers=len(SPEAKERS))
    lines = []
    for i in range(n_items):
        sym, dur_f, dur_i, s_en, s_pi, f_en, f_pi, mel, spk, _, _ = ds[i]
        fdir = os.path.join(tmp, 'features', SPEAKERS[spk])
        os.makedirs(fdir, exist_ok=True)
        base = os.path.join(fdir, f'utt{i:06d}')
        np.save(base + '.npy', mel.numpy())
        ends = np.cumsum(dur_f.numpy().astype(np.float64))
        with open(base + '.markers', 'w', encoding='utf-8') as f:
            for l in range(len(sym)):
                begin = float(ends[l - 1]) if l else 0.
                f.write(f'{begin!r}\t{float(ends[l])!r}\t{int(dur_i[l])}\t{hp.symbols[int(sym[l])]}\tw\t0\n')
        _floats(base + '.symbols_nrg', s_en.numpy() * 15. + 30.)
        _floats(base + '.symbols_f0', s_pi.numpy() * 0.3 + 5.)
        _floats(base + '.frames_nrg', f_en.numpy())
        _floats(base + '.frames_f0', f_pi.numpy())
        lines.append(f'{fdir}|utt{i:06d}|{spk}')
    with open(hp.training_files, 'w', encoding='utf-8') as f:
        f.write('\n'.join(lines) + '\n')
    with open(hp.validation_files, 'w', encoding='utf-8') as f:
        f.write('\n'.join(lines[:n_val]) + '\n')


def bench_loader_path(hp):
    train_loader, _, _, n = prepare_data_loaders(hp, num_workers=8, distributed=False)
    t0 = time.perf_counter()
    seen = sum(len(batch[11]) for batch in train_loader)
    dt = time.perf_counter() - t0
    return {'utterances': seen, 'seconds': round(dt, 3), 'utterances_per_s': round(seen / dt, 1), 'num_workers': 8}


def bench_resident(hp, dev):
    from daft_exprt.resident_set import ResidentLoader, ResidentSet
    t0 = time.perf_counter()
    rs = ResidentSet.from_list(hp.training_files, hp, dev)
    load_s = time.perf_counter() - t0
    loader = ResidentLoader(rs, hp.batch_size, shuffle=True, drop_last=True)
    frames = sum(b.frames for b in loader)       # warm-up epoch (code objects, allocator)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    n = sum(1 for _ in loader)
    e1.record()
    host_s = time.perf_counter() - t0
    e1.synchronize()
    ms = e0.elapsed_time(e1)
    return ({'seconds': round(load_s, 3), 'utterances': len(rs), 'utterances_per_s': round(len(rs) / load_s, 1), 'packed_bytes': rs.nbytes},
            {'batches': n, 'device_ms': round(ms, 3), 'batches_per_s': round(n / (ms * 1e-3), 1), 'host_enqueue_s': round(host_s, 4),
             'utterances_per_s': round(n * hp.batch_size / (ms * 1e-3), 1), 'frames_per_epoch': frames})


def bench_train(tmp, batch, iterations, skip, resident):
    from daft_exprt.train import train
    out = os.path.join(tmp, 'out_resident' if resident else 'out_loader')
    hp = _hp(tmp, batch, nb_iterations=iterations, iters_per_checkpoint=10 ** 9, iters_check_for_model_improvement=10 ** 9,
             resident_data_set=resident)
    hp.output_directory = out
    hp.rank, hp.world_size, hp.multiprocessing_distributed, hp.ngpus_per_node = 0, 1, False, 1
    os.makedirs(os.path.join(out, 'logs'), exist_ok=True)
    t0 = time.perf_counter()
    train(0, hp, os.path.join(out, 'logs', 'train.log'))
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    recs = [json.loads(l) for l in open(os.path.join(out, 'logs', 'metrics.jsonl'))]
    durs = [r['DaftExprt.optimization/duration'] for r in recs if 'DaftExprt.training/loss' in r][skip:]
    return {'iterations': len(durs) + skip, 'timed': len(durs), 'iterations_per_s': round(len(durs) / sum(durs), 2),
            'utterances_per_s': round(len(durs) * batch / sum(durs), 1), 'wall_s': round(wall, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--utterances', type=int, default=2048)
    ap.add_argument('--batch', type=int, default=48)
    ap.add_argument('--iterations', type=int, default=50)
    ap.add_argument('--skip', type=int, default=5)
    args = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix='dx_bench_loader_')
    try:
        hp = _hp(tmp, args.batch)
        t0 = time.perf_counter()
        fabricate(tmp, hp, args.utterances, n_val=min(args.utterances, args.batch))
        out = {'metric': 'loader_paths', 'utterances': args.utterances, 'batch': args.batch, 'fabricate_s': round(time.perf_counter() - t0, 1)}
        out['loader'] = bench_loader_path(hp)
        out['resident_load'], out['resident_batches'] = bench_resident(hp, torch.device('cuda:0'))
        out['train_loader_path'] = bench_train(tmp, args.batch, args.iterations, args.skip, resident=False)
        out['train_resident'] = bench_train(tmp, args.batch, args.iterations, args.skip, resident=True)
        print(json.dumps(out))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == '__main__':
    main()
