#!/usr/bin/env python
"""Synthesis-based alignment (`align.align_batch`) of a fabricated batch (B = 256: noise bursts of 2 to 8 s between silences, the
symbols of `synthetic_inference_batch`) on one MI355X.

One JSON line: utterances per second of `align_batch` as a whole (wall time, synchronised, median of --reps after a warm-up), and
device-event times of its four stages run one after the other on the same batch: the front-end (energies of the whole recording,
`dx_active_span`, the crop, pitch and mel of the crop), the synthesis (`model.inference` with the crop as prosody reference), the
DTW (two `dx_mel_cepstrum` launches and `dx_dtw_align`) and the transfer (`dx_dtw_transfer`).  The weights are random: the times
depend on the shapes only, the boundaries mean nothing.
Run:  python tools/bench_align.py [--reps 5] [--batch 256]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'ubisoft-laforge-daft-exprt_amd')):
    sys.path.insert(0, p)


def _timed(fn, reps):
    ts, out = [], None
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out = fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    return float(np.median(ts)), out


def _recordings(batch, fs, seed):
    ''' (wavs (B, S) fp32, sample counts): 0.2 s of near-silence, noise at a slowly varying level, 0.3 s of near-silence '''
    rng = np.random.RandomState(seed)
    n = (rng.uniform(2.0, 8.0, size=batch) * fs).astype(np.int64)
    wavs = np.zeros((batch, int(n.max())), dtype=np.float32)
    for b in range(batch):
        x = 1e-4 * rng.standard_normal(n[b])
        lo, hi = int(0.2 * fs), n[b] - int(0.3 * fs)
        level = 0.1 + 0.08 * np.sin(2 * np.pi * rng.uniform(1.0, 4.0) * np.arange(hi - lo) / fs)
        x[lo:hi] += level * rng.standard_normal(hi - lo)
        wavs[b, :n[b]] = x
    return torch.from_numpy(wavs), n.tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--batch', type=int, default=256)
    args = ap.parse_args()
    import bench
    from daft_exprt import align as A
    from daft_exprt import evaluate as E
    from daft_exprt.data_loader import centre_duration_head, synthetic_inference_batch
    from daft_exprt.extract_features import mel_spectrogram_batch, pitch_batch, wav_crop_batch
    from daft_exprt.model import DaftExprt
    dev = torch.device('cuda:0')
    hp = bench.make_hparams(args.batch, 'bf16')
    hp.stats = {f'spk {i}': {'pitch': {'mean': 5.0, 'std': 0.3}} for i in range(hp.n_speakers)}
    torch.manual_seed(hp.seed)
    model = DaftExprt(hp).to(dev).eval()
    centre_duration_head(model)
    inputs = synthetic_inference_batch(hp, args.batch, seed=1234)
    symbols, input_lengths, speaker_ids = inputs[0].to(dev), inputs[4].to(dev), inputs[9].to(dev)
    wavs, n_samples = _recordings(args.batch, int(hp.sampling_rate), 7)
    wavs = wavs.to(dev)
    hop = int(hp.hop_length)

    def whole():
        out = A.align_batch(model, symbols, input_lengths, wavs, n_samples, speaker_ids, hp)
        torch.cuda.synchronize()
        return out
    whole()                                                       # warm-up (tables, workspace, code objects)
    walls = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        out = whole()
        walls.append(time.perf_counter() - t0)
    wall = float(np.median(walls))

    n_dev = torch.tensor(n_samples, dtype=torch.int64, device=dev)

    def front_end():
        _, energy, n_frames = mel_spectrogram_batch(wavs, n_dev, hp, min_samples=min(n_samples))
        begin, end = A.active_span_batch(energy, n_frames, -40.0)
        first = begin * hop
        length = torch.minimum(end * hop, n_dev) - first
        crop = torch.stack([first, length], dim=1).contiguous()
        cropped = wav_crop_batch(wavs, crop, wavs.shape[1])
        pitch, _ = pitch_batch(cropped, length, hp)
        mel, energy, n_mel = mel_spectrogram_batch(cropped, length, hp, min_samples=hp.filter_length)
        return energy, pitch, mel, n_mel
    front_ms, (energy, pitch, mel_rec, n_rec) = _timed(front_end, args.reps)
    T = int(n_rec.max())
    energy, pitch, mel_rec = energy[:, :T].contiguous(), pitch[:, :T].contiguous(), mel_rec[:, :, :T].contiguous()
    ones = torch.ones(symbols.shape, dtype=torch.float32, device=dev)

    def synthesis():
        with torch.no_grad():
            enc, (mel_gen, n_gen), _ = model.inference((symbols, ones, ones, torch.zeros_like(ones), input_lengths, energy, pitch, mel_rec,
                                                        n_rec, speaker_ids), 'add', hp)
        return enc[1].long().contiguous(), mel_gen.float().contiguous(), n_gen.long()
    synthesis_ms, (gen_dur, mel_gen, n_gen) = _timed(synthesis, args.reps)

    def dtw():
        cep_rec, cep_gen = E.mel_cepstrum_batch(mel_rec, n_rec), E.mel_cepstrum_batch(mel_gen, n_gen)
        return E.dtw_align_batch(cep_rec, n_rec, cep_gen, n_gen)
    dtw_ms, (_, path, path_len) = _timed(dtw, args.reps)
    transfer_ms, (rec, moved, status) = _timed(lambda: A._transfer(path, path_len, n_rec, n_gen, gen_dur, input_lengths, 3,
                                                                   mel_rec.shape[2], mel_gen.shape[2]), args.reps)
    result = {'metric': 'align_batch', 'batch': args.batch, 'utterances_per_s': args.batch / wall, 'align_batch_wall_ms': 1e3 * wall,
              'front_end_ms': front_ms, 'synthesis_ms': synthesis_ms, 'dtw_ms': dtw_ms, 'transfer_ms': transfer_ms,
              'audio_seconds': sum(n_samples) / float(hp.sampling_rate), 'T_rec': int(mel_rec.shape[2]), 'T_gen': int(mel_gen.shape[2]),
              'symbols': int(input_lengths.sum()), 'status_ok': int((out['status'] == 0).sum()), 'moved': int(out['moved'].sum()),
              'stage_status_ok': int((status == 0).sum())}
    print(json.dumps(result))


if __name__ == '__main__':
    main()
