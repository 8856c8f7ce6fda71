#!/usr/bin/env python
"""Prosody-transfer scoring of a configs[3]-shaped synthesis batch (B = 256, `synthetic_inference_batch`) on one MI355X.

One JSON line: device-event times (median of --reps after a warm-up) of `evaluate.prosody_transfer_scores` on the batch's
Griffin-Lim audio against its collated reference curves, of its stages (pitch tracking, mel front-end, the two `dx_curve_pcc`
launches), of the Griffin-Lim preview itself in the same run, and of `dx_curve_pcc` alone at the length limit (B rows of
4096 fully voiced frames against 4095: the largest direct sums the kernel takes).
Run:  python tools/bench_prosody_eval.py [--reps 5] [--batch 256]
"""
import argparse
import json
import os
import sys

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--batch', type=int, default=256)
    args = ap.parse_args()
    import bench
    from daft_exprt import evaluate as E
    from daft_exprt import griffin_lim as G
    from daft_exprt.data_loader import centre_duration_head, synthetic_inference_batch
    from daft_exprt.extract_features import mel_spectrogram_batch, pitch_batch
    from daft_exprt.model import DaftExprt
    dev = torch.device('cuda:0')
    hp = bench.make_hparams(args.batch, 'bf16')
    hp.stats = {f'spk {i}': {'pitch': {'mean': 5.0, 'std': 0.3}} for i in range(hp.n_speakers)}
    torch.manual_seed(hp.seed)
    model = DaftExprt(hp).to(dev).eval()
    centre_duration_head(model)
    inputs = tuple(t.to(dev) for t in synthetic_inference_batch(hp, args.batch, seed=1234))
    energy_refs, pitch_refs, ref_lengths = inputs[5].float().contiguous(), inputs[6].float().contiguous(), inputs[8]
    with torch.no_grad():
        _, (mel, lengths), _ = model.inference(tuple(t.clone() for t in inputs), 'add', hp)
    mel = mel.float().contiguous()
    wavs, n = G.griffin_lim_batch(mel, lengths, hp)                           # warm-up (tables, code objects)
    E.prosody_transfer_scores(wavs, n, pitch_refs, energy_refs, ref_lengths, hp)
    torch.cuda.synchronize()
    gl_ms, _ = _timed(lambda: G.griffin_lim_batch(mel, lengths, hp), args.reps)
    total_ms, scores = _timed(lambda: E.prosody_transfer_scores(wavs, n, pitch_refs, energy_refs, ref_lengths, hp), args.reps)
    pitch_ms, (pitch, n_pitch) = _timed(lambda: pitch_batch(wavs, n, hp), args.reps)
    mel_ms, (_, energy, n_frames) = _timed(lambda: mel_spectrogram_batch(wavs, n, hp), args.reps)
    pcc_pitch_ms, _ = _timed(lambda: E.curve_pcc_batch(pitch_refs, ref_lengths, pitch, n_pitch, True), args.reps)
    pcc_energy_ms, _ = _timed(lambda: E.curve_pcc_batch(energy_refs, ref_lengths, energy, n_frames, False), args.reps)
    L = E.max_curve_length()
    g = torch.Generator().manual_seed(0)
    ref = (5.0 + 0.3 * torch.rand((args.batch, L), generator=g)).to(dev)
    dut = (5.0 + 0.3 * torch.rand((args.batch, L - 1), generator=g)).to(dev)
    n_r = torch.full((args.batch,), L, dtype=torch.int64, device=dev)
    E.curve_pcc_batch(ref, n_r, dut, n_r - 1)
    torch.cuda.synchronize()
    limit_ms, _ = _timed(lambda: E.curve_pcc_batch(ref, n_r, dut, n_r - 1), args.reps)
    pcc = scores['pitch_pcc'].cpu().numpy()
    out = {'metric': 'prosody_transfer_scores', 'batch': int(mel.shape[0]), 'T_gen': int(pitch.shape[1]), 'T_ref': int(pitch_refs.shape[1]),
           'gen_frames': int(n_frames.sum()), 'voiced_gen': int(scores['voiced_gen'].sum()), 'voiced_ref': int(scores['voiced_ref'].sum()),
           'pitch_pcc_defined': int(np.isfinite(pcc).sum()), 'griffin_lim_ms': gl_ms, 'scores_ms': total_ms,
           'scores_over_griffin_lim': total_ms / gl_ms, 'pitch_batch_ms': pitch_ms, 'mel_spectrogram_ms': mel_ms,
           'curve_pcc_pitch_ms': pcc_pitch_ms, 'curve_pcc_energy_ms': pcc_energy_ms, 'limit_len': L, 'curve_pcc_limit_ms': limit_ms}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
