#!/usr/bin/env python
"""What the validation report costs beside a validation pass, on one MI355X, for one B = 48 validation batch of the bench's shape.

One JSON line: wall time (synchronised, median of --reps after a warm-up) of `train.validate` without and with a
`ValidationReport` plus its `write` (no figures), the host time the report accounts to itself (`ValidationReport.seconds`, what
`train()` logs), and device-event times of its kernels alone: `dx_alignment_score` on the batch's (B, L, T) weights and the two
`dx_film_hist_*` passes with their edge-table round trip on the decoder's FiLM tensor.
Run:  python tools/bench_validation_report.py [--reps 5] [--batch 48]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'ubisoft-laforge-daft-exprt_amd')):
    sys.path.insert(0, p)


def _events(fn, reps):
    ts = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    return float(np.median(ts))


def _wall(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        begin = time.time()
        fn()
        torch.cuda.synchronize()
        ts.append((time.time() - begin) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--batch', type=int, default=48)
    args = ap.parse_args()
    import bench
    from daft_exprt.data_loader import synthetic_batch
    from daft_exprt.model import DaftExprt
    from daft_exprt.loss import DaftExprtLoss
    from daft_exprt.train import validate
    from daft_exprt.validation_report import ValidationReport, alignment_scores, film_histograms
    dev = torch.device('cuda:0')
    hp = bench.make_hparams(args.batch, 'bf16')
    torch.manual_seed(hp.seed)
    model = DaftExprt(hp).to(dev)
    criterion = DaftExprtLoss(0, hp)
    loader = [synthetic_batch(hp, args.batch, seed=1234, t_max=1000, force_first_full=True)]
    out_dir = tempfile.mkdtemp()
    seconds = []

    def with_report():
        report = ValidationReport(hp, 1, len(loader))
        validate(0, model, criterion, loader, hp, report=report)
        report.write(out_dir)
        seconds.append(report.seconds * 1e3)

    validate(0, model, criterion, loader, hp)
    with_report()
    seconds.clear()
    plain_ms = _wall(lambda: validate(0, model, criterion, loader, hp), args.reps)
    report_ms = _wall(with_report, args.reps)
    model.eval()
    with torch.no_grad():
        inputs, _, _ = model.parse_batch(0, loader[0])
        outputs = model(inputs)
    weights, film = outputs[4], outputs[1][3].float().contiguous()
    align_ms = _events(lambda: alignment_scores(weights, inputs[2], inputs[5], inputs[9]), args.reps)
    hist_ms = _events(lambda: film_histograms(film), args.reps)
    print(json.dumps({'metric': 'validation_report', 'batch': args.batch, 'L': int(weights.shape[1]), 'T': int(weights.shape[2]),
                      'validate_ms': plain_ms, 'validate_with_report_and_write_ms': report_ms,
                      'report_seconds_logged_ms': float(np.median(seconds)), 'alignment_score_ms': align_ms,
                      'film_histograms_ms': hist_ms, 'film_shape': list(film.shape)}))


if __name__ == '__main__':
    main()
