#!/usr/bin/env python
"""Measure the vocoder fine-tuning data set path on the configs[3]-sized synthesis batch (B = 256, T <= 1000 frames).

Prints one JSON line:
  * resample_16k / resample_48k: device-event time of one `resample_batch` to 22.05 kHz over the batch's audio, as audio-seconds
    per second and as a share of the HBM peak (bytes in + bytes out over the time; the bank sits in L2);
  * ft_pack_ms: one `dx_ft_pack` of the batch (mel (256, 80, 1000) + int16 crops);
  * forward_eval_ms: the teacher-forced eval forward of the batch (what `fine_tuning` runs per batch);
  * end_to_end: `fine_tuning` over a fabricated on-disk data set (`--utterances`, 10 % of them stored at 16 kHz), utterances/s
    and the host I/O share (main thread waiting for the wav reader, writer thread busy);
  * cpu_baseline: the float64 restatement (tests/resample_oracle.py) on a few utterances, audio-seconds per second.
Usage: python tools/bench_fine_tune.py [--reps 20] [--utterances 320] [--out FILE]
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

from daft_exprt import audio as A  # noqa: E402
from daft_exprt.hparams import HyperParams  # noqa: E402

HBM_PEAK = 8.0e12     # B/s, MI355X spec
FS, HOP, B = 22050, 256, 256


def _hp(tmp, **kw):
    return HyperParams(verbose=False, training_files=os.path.join(tmp, 'train_english.txt'),
                       validation_files=os.path.join(tmp, 'validation_english.txt'), output_directory=os.path.join(tmp, 'out'),
                       language='english', speakers=['spkA', 'spkB'], **kw)


def _timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / reps


def bench_resample(frames, sr_in, reps):
    dev = torch.device('cuda:0')
    n_out = frames * HOP
    n_in = np.array([-(-int(n) * sr_in // FS) for n in n_out])
    x = torch.rand((B, int(n_in.max())), device=dev) * 2 - 1
    n = torch.from_numpy(n_in).to(dev)
    ms = _timed(lambda: A.resample_batch(x, n, sr_in, FS), reps)
    audio_s = float(sum(A.out_length(int(k), sr_in, FS) for k in n_in)) / FS
    S_out = A.out_length(x.shape[1], sr_in, FS)
    nbytes = 4 * B * (x.shape[1] + S_out)
    return {'ms': round(ms, 4), 'audio_s': round(audio_s, 1), 'audio_s_per_s': round(audio_s / (ms * 1e-3), 1),
            'us_per_audio_s': round(ms * 1e3 / audio_s, 4), 'hbm_share': round(nbytes / (ms * 1e-3) / HBM_PEAK, 3)}


def bench_pack(frames, reps):
    dev = torch.device('cuda:0')
    T = int(frames.max())
    mel = torch.randn((B, 80, T), device=dev)
    lengths = torch.from_numpy(frames).to(dev)
    wavs = torch.rand((B, T * HOP + 4000), device=dev) * 2 - 1
    crops = [(1000, (int(t) - 1) * HOP + 100) for t in frames]
    crop = torch.tensor(crops, dtype=torch.int64, device=dev)
    mel_total, wav_total = 80 * int(frames.sum()), sum(c for _, c in crops)
    ms = _timed(lambda: A.ft_pack(mel, lengths, wavs, crop, mel_total, wav_total), reps)
    return round(ms, 4)


def bench_forward(reps):
    from daft_exprt.data_loader import synthetic_batch
    from daft_exprt.model import DaftExprt
    tmp = tempfile.mkdtemp()
    try:
        hp = _hp(tmp, n_speakers=11)
        model = DaftExprt(hp).cuda(0).eval()
        inputs, _, _ = model.parse_batch(0, synthetic_batch(hp, B, t_max=1000))
        with torch.no_grad():
            return round(_timed(lambda: model(inputs), reps), 3)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def _fabricate(root, hp, n_utts, rng):
    lines = []
    for u in range(n_utts):
        sid = u % 2
        spk = hp.speakers[sid]
        name = f'u{u:05d}'
        T = int(rng.randint(95, 400))
        n_c = (T - 1) * HOP + int(rng.randint(0, HOP))
        a = int(rng.randint(300, 3000))
        e = a + n_c
        n_total = e + int(rng.randint(0, 2000))
        dirs = [os.path.join(root, 'data', spk, d) for d in ('wavs', 'align')] + [os.path.join(root, 'features', spk)]
        for d in dirs:
            os.makedirs(d, exist_ok=True)
        if u % 10 == 5:
            n16 = -(-n_total * 16000 // FS) + 5
            A.write_wav_int16(os.path.join(dirs[0], f'{name}.wav'), 16000, (rng.randn(n16) * 3000).astype(np.int16))
        else:
            A.write_wav_int16(os.path.join(dirs[0], f'{name}.wav'), FS, (rng.randn(n_total) * 3000).astype(np.int16))
        L = int(rng.randint(20, 60))
        dur = np.ones(L, dtype=np.int64)
        np.add.at(dur, rng.randint(0, L, size=T - L), 1)
        t, rows = (a + 0.5) / FS, []
        for i, d in enumerate(dur):
            stop = (e + 0.5) / FS if i == L - 1 else t + d * HOP / FS
            rows.append(f'{t:.10f}\t{stop:.10f}\t{d}\t{hp.symbols[int(rng.randint(1, hp.n_symbols))]}\tw\t0')
            t = stop
        for d in dirs[1:]:
            with open(os.path.join(d, f'{name}.markers'), 'w') as f:
                f.write('\n'.join(rows) + '\n')
        base = os.path.join(dirs[2], name)
        np.save(base + '.npy', rng.randn(80, T).astype(np.float32) - 5)
        for ext, v in (('.symbols_nrg', rng.uniform(2, 30, size=L)), ('.symbols_f0', np.log(rng.uniform(90, 250, size=L))),
                       ('.frames_nrg', rng.uniform(0, 40, size=T)), ('.frames_f0', np.log(rng.uniform(90, 250, size=T)))):
            with open(base + ext, 'w') as f:
                f.write('\n'.join(f'{x:.4f}' for x in v) + '\n')
        lines.append(f'{dirs[2]}|{name}|{sid}')
    for f in (hp.training_files, hp.validation_files):
        with open(f, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


def bench_end_to_end(n_utts):
    from daft_exprt.fine_tune import fine_tuning
    from daft_exprt.model import DaftExprt
    tmp = tempfile.mkdtemp()
    try:
        stats = {f'spk {i}': {'energy': {'mean': 15., 'std': 8.}, 'pitch': {'mean': 5., 'std': 0.3}} for i in range(2)}
        hp = _hp(tmp, stats=stats)
        hp.data_set_dir = os.path.join(tmp, 'data')
        t0 = time.time()
        _fabricate(tmp, hp, n_utts, np.random.RandomState(0))
        fabricate_s = time.time() - t0
        ckpt = os.path.join(tmp, 'ckpt')
        torch.save({'state_dict': {'module.' + k: v for k, v in DaftExprt(hp).state_dict().items()}}, ckpt)
        hp.checkpoint = ckpt
        r = fine_tuning(hp)
        return {'utterances': r['utterances'], 'written': r['written'], 'batch_size': hp.batch_size, 'seconds': round(r['seconds'], 2),
                'utt_per_s': round(r['utterances'] / r['seconds'], 1), 'read_wait_share': round(r['read_wait_s'] / r['seconds'], 3),
                'writer_busy_share': round(r['write_s'] / r['seconds'], 3), 'fabricate_s': round(fabricate_s, 1)}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def bench_cpu_baseline(n=3):
    from tests import resample_oracle as RO
    rng = np.random.RandomState(1)
    xs = [rng.uniform(-1, 1, size=16000) for _ in range(n)]
    t0 = time.time()
    for x in xs:
        RO.resample(x, 16000, FS)
    dt = time.time() - t0
    return {'utterances': n, 'audio_s': float(n), 'audio_s_per_s': round(n / dt, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--utterances', type=int, default=320)
    ap.add_argument('--out', type=str, default='')
    args = ap.parse_args()
    frames = np.random.RandomState(0).randint(250, 1001, size=B).astype(np.int64)
    res = {'batch': B, 'frames_max': int(frames.max()), 'audio_s_batch': round(float(frames.sum()) * HOP / FS, 1),
           'resample_16k': bench_resample(frames, 16000, args.reps), 'resample_48k': bench_resample(frames, 48000, args.reps),
           'ft_pack_ms': bench_pack(frames, args.reps), 'forward_eval_ms': bench_forward(max(3, args.reps // 4)),
           'end_to_end': bench_end_to_end(args.utterances), 'cpu_baseline': bench_cpu_baseline()}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
