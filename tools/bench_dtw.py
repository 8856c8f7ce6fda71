#!/usr/bin/env python
"""DTW-aligned copy-synthesis scoring of a configs[3]-shaped synthesis batch (B = 256, `synthetic_inference_batch`) on one MI355X.

One JSON line: device-event times (median of --reps after a warm-up) of `evaluate.dtw_scores_batch` on the batch's decoder mel
against its reference mels (T_ref ~ U{250..1000}) with pitch curves on both sides, of its three stages (the two `dx_mel_cepstrum`
launches, `dx_dtw_align`, `dx_dtw_path_scores`), and of `dx_dtw_align` alone on one pair at the length limit (4096 x 4096 frames,
16.8 M cells).  For context, the host time of the float64 oracle (tests/dtw_oracle.py, NumPy by anti-diagonals) on one pair of the
batch's median lengths.
Run:  python tools/bench_dtw.py [--reps 5] [--batch 256]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--batch', type=int, default=256)
    args = ap.parse_args()
    import bench
    from daft_exprt import evaluate as E
    from daft_exprt.data_loader import centre_duration_head, synthetic_inference_batch
    from daft_exprt.model import DaftExprt
    from tests import dtw_oracle as O
    dev = torch.device('cuda:0')
    hp = bench.make_hparams(args.batch, 'bf16')
    hp.stats = {f'spk {i}': {'pitch': {'mean': 5.0, 'std': 0.3}} for i in range(hp.n_speakers)}
    torch.manual_seed(hp.seed)
    model = DaftExprt(hp).to(dev).eval()
    centre_duration_head(model)
    inputs = tuple(t.to(dev) for t in synthetic_inference_batch(hp, args.batch, seed=1234))
    pitch_ref, mel_ref, n_ref = inputs[6].float().contiguous(), inputs[7].float().contiguous(), inputs[8]
    with torch.no_grad():
        _, (mel_gen, n_gen), _ = model.inference(tuple(t.clone() for t in inputs), 'add', hp)
    mel_gen, n_gen = mel_gen.float().contiguous(), n_gen.long()
    g = torch.Generator().manual_seed(0)
    voiced = torch.rand((args.batch, mel_gen.shape[2]), generator=g) >= 0.3
    pitch_gen = (torch.where(voiced, 5.0 + 0.3 * torch.randn((args.batch, mel_gen.shape[2]), generator=g), torch.zeros(()))).to(dev)

    E.dtw_scores_batch(mel_ref, n_ref, mel_gen, n_gen, pitch_ref, pitch_gen)      # warm-up (table, workspace, code objects)
    torch.cuda.synchronize()
    total_ms, scores = _timed(lambda: E.dtw_scores_batch(mel_ref, n_ref, mel_gen, n_gen, pitch_ref, pitch_gen), args.reps)
    cep_ms, (cep_ref, cep_gen) = _timed(lambda: (E.mel_cepstrum_batch(mel_ref, n_ref), E.mel_cepstrum_batch(mel_gen, n_gen)), args.reps)
    align_ms, (_, path, path_len) = _timed(lambda: E.dtw_align_batch(cep_ref, n_ref, cep_gen, n_gen), args.reps)
    scores_ms, _ = _timed(lambda: E.dtw_path_scores_batch(cep_ref, n_ref, cep_gen, n_gen, path, path_len, pitch_ref, pitch_gen), args.reps)

    L = E.max_dtw_length()
    lim_ref = torch.randn((1, L, 13), generator=g).to(dev)
    lim_gen = torch.randn((1, L, 13), generator=g).to(dev)
    n_lim = torch.full((1,), L, dtype=torch.int64, device=dev)
    E.dtw_align_batch(lim_ref, n_lim, lim_gen, n_lim)
    torch.cuda.synchronize()
    limit_ms, _ = _timed(lambda: E.dtw_align_batch(lim_ref, n_lim, lim_gen, n_lim), args.reps)

    nr, ng = int(n_ref.median()), int(n_gen.median())
    ref64, gen64 = O.real_pair(nr, ng, 1)
    t0 = time.perf_counter()
    O.dtw(ref64, gen64)
    oracle_ms = 1e3 * (time.perf_counter() - t0)

    cells = int((n_ref * n_gen).sum())
    mcd = scores['mcd_db'].cpu().numpy()
    out = {'metric': 'dtw_scores_batch', 'batch': int(mel_ref.shape[0]), 'T_ref': int(mel_ref.shape[2]), 'T_gen': int(mel_gen.shape[2]),
           'cells': cells, 'path_entries': int(path_len.sum()), 'mcd_defined': int(np.isfinite(mcd).sum()), 'scores_ms': total_ms,
           'mel_cepstrum_ms': cep_ms, 'dtw_align_ms': align_ms, 'path_scores_ms': scores_ms, 'cells_per_us': cells / (1e3 * align_ms),
           'limit_len': L, 'dtw_align_limit_ms': limit_ms, 'oracle_pair': [nr, ng], 'oracle_host_ms': oracle_ms}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
