#!/usr/bin/env python
"""Prosody cloning (`clone.clone_batch`) of a fabricated batch (B = 256: the recordings and symbols of tools/bench_align.py) on
one MI355X.

One JSON line: utterances per second of `clone_batch` as a whole with Griffin-Lim audio (wall time, synchronised, median of --reps
after a warm-up), the wall time of its stages as `clone_batch` reports them (alignment + pooling, the second pass, audio + scores;
each ends with a synchronisation) and device-event times of the K29 kernels alone on the batch's own shapes: `dx_clone_pool`, and
`dx_prosody_impose` + `dx_int_durations` + `dx_prosody_impose_durations` against `dx_int_durations` alone.  The weights are random:
the times depend on the shapes only, the scores mean nothing.  Nothing is gated.
Run:  python tools/bench_clone.py [--reps 5] [--batch 256]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'tools'), ROOT, os.path.join(ROOT, 'ubisoft-laforge-daft-exprt_amd')):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--batch', type=int, default=256)
    args = ap.parse_args()
    import bench
    from bench_align import _recordings, _timed
    from daft_exprt import ops
    from daft_exprt.clone import clone_batch
    from daft_exprt.data_loader import centre_duration_head, synthetic_inference_batch
    from daft_exprt.extract_features import mel_spectrogram_batch, pitch_batch
    from daft_exprt.model import DaftExprt
    dev = torch.device('cuda:0')
    hp = bench.make_hparams(args.batch, 'bf16')
    hp.stats = {f'spk {i}': {'energy': {'mean': 2.0, 'std': 1.0}, 'pitch': {'mean': 5.0, 'std': 0.3}} for i in range(hp.n_speakers)}
    torch.manual_seed(hp.seed)
    model = DaftExprt(hp).to(dev).eval()
    centre_duration_head(model)
    inputs = synthetic_inference_batch(hp, args.batch, seed=1234)
    symbols, input_lengths, speaker_ids = inputs[0].to(dev), inputs[4].to(dev), inputs[9].to(dev)
    wavs, n_samples = _recordings(args.batch, int(hp.sampling_rate), 7)
    wavs = wavs.to(dev)

    def whole(seconds=None):
        out = clone_batch(model, symbols, input_lengths, wavs, n_samples, speaker_ids, speaker_ids, hp, use_griffin_lim=True, seconds=seconds)
        torch.cuda.synchronize()
        return out
    whole()                                                       # warm-up (tables, workspaces, code objects)
    walls = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        out = whole()
        walls.append(time.perf_counter() - t0)
    wall = float(np.median(walls))
    stages = {}
    whole(stages)

    # the K29 kernels alone, on the batch's shapes
    n_dev = torch.tensor(n_samples, dtype=torch.int64, device=dev)
    _, energy, _ = mel_spectrogram_batch(wavs, n_dev, hp, min_samples=min(n_samples))
    log_pitch, _ = pitch_batch(wavs, n_dev, hp)
    T = min(energy.shape[1], log_pitch.shape[1])
    info, targets = out['info'], out['targets']
    pool_ms, _ = _timed(lambda: ops.clone_pool(energy[:, :T], log_pitch[:, :T], info['begin'], targets.durations, input_lengths), args.reps)
    B, L = symbols.shape
    ones = torch.ones((B, L), dtype=torch.float32, device=dev)
    dur0 = torch.full((B, L), 0.08, dtype=torch.float32, device=dev)

    def k16():
        return ops.int_durations(dur0.clone(), hp, ones)

    def imposed():
        dur, energy_, pitch_ = dur0.clone(), ones.clone(), ones.clone()
        exact = ops.prosody_impose(dur, energy_, pitch_, targets, input_lengths, ones, hp)
        dint, totals, status = ops.int_durations(dur, hp, ones)
        ops.prosody_impose_durations(exact, targets, input_lengths, dur, dint, totals, status, hp)
        return exact
    k16_ms, _ = _timed(k16, args.reps)
    impose_ms, exact = _timed(imposed, args.reps)
    scores = {k: v[torch.isfinite(v)] for k, v in out['scores'].items()}
    result = {'metric': 'clone_batch', 'batch': args.batch, 'utterances_per_s': args.batch / wall, 'clone_batch_wall_ms': 1e3 * wall,
              'stage_wall_ms': {k: 1e3 * v for k, v in stages.items()}, 'clone_pool_ms': pool_ms, 'int_durations_ms': k16_ms,
              'impose_int_durations_override_ms': impose_ms, 'audio_seconds': sum(n_samples) / float(hp.sampling_rate),
              'frames': int(info['frames'].sum()), 'symbols': int(input_lengths.sum()), 'status_ok': int((info['status'] == 0).sum()),
              'frame_exact': int(out['frame_exact'].sum()), 'stage_exact': int((exact == 1).sum()),
              'scored': {k: int(v.numel()) for k, v in scores.items()}}
    print(json.dumps(result))


if __name__ == '__main__':
    main()
