#!/usr/bin/env python
"""The phone recogniser (`daft_exprt/recognizer.py`, K31) on a fabricated batch on one MI355X: B = 256 utterances of 300 to 1 000
frames (150 to 500 steps at stride 2) and frames / 7 phones each, the 69 phones of the English table plus the blank.

One JSON line.  `train_step_ms` / `train_utterances_per_s`: one Adam step of the recogniser (encoder forward, `dx_uctc_loss`,
encoder backward, Adam) on the batch.  `score_ms` / `score_utterances_per_s`: `phone_error_rates` on it (encoder, `dx_uctc_greedy`,
`dx_edit_distance`).  `kernel_ms`: device-event times (median of --reps after a warm-up) of the three entry points alone, and
`uctc_share`: `dx_uctc_loss` over the training step.  `torch_ctc_ms`: `F.ctc_loss` forward and backward on the same logits on the
device (log_softmax included on both sides: the kernel has it inside), and `agree`: the largest relative difference of the per-row
losses of the two.  The weights are random: the times depend on the shapes only.  Single samples, nothing here is a gate.
Run:  python tools/bench_recognizer.py [--reps 5] [--batch 256]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'ubisoft-laforge-daft-exprt_amd')):
    sys.path.insert(0, p)


def _timed(fn, reps):
    fn()
    torch.cuda.synchronize()
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
    from daft_exprt import recognizer as R
    dev = torch.device('cuda:0')
    hp = bench.make_hparams(args.batch, 'bf16')
    B, reps = args.batch, args.reps
    rng = np.random.RandomState(3)
    n_frm = rng.randint(300, 1001, size=B)
    n_frm[0] = 1000
    n_sym = n_frm // 7
    T, L = int(n_frm.max()), int(n_sym.max())
    torch.manual_seed(3)
    model = R.Recognizer(hp.symbols, int(hp.n_mel_channels)).to(dev)
    first = len(hp.symbols) - len(model.phones)
    symbols = torch.zeros((B, L), dtype=torch.int64)
    for b in range(B):
        symbols[b, :n_sym[b]] = torch.from_numpy(rng.randint(first, len(hp.symbols), size=n_sym[b]))
    symbols, mel = symbols.to(dev), (2.0 * torch.randn(B, int(hp.n_mel_channels), T) - 5.0).to(dev)
    n_frm, n_sym = torch.from_numpy(n_frm).to(dev), torch.from_numpy(n_sym).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    labels, n_labels = model.labels_of(symbols, n_sym)

    def step():
        logits, n_steps = model(mel, n_frm)
        loss, skipped = R.uctc_loss(logits, n_steps, labels, n_labels)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        return skipped
    step_ms, skipped = _timed(step, reps)
    model.eval()
    score_ms, scores = _timed(lambda: R.phone_error_rates(model, mel, n_frm, symbols, n_sym), reps)
    with torch.no_grad():
        logits, n_steps = model(mel, n_frm)
        kernel = {}
        kernel['uctc_loss'], (loss, status, grad) = _timed(lambda: R.uctc_loss_and_grad(logits, n_steps, labels, n_labels), reps)
        kernel['uctc_greedy'], (ids, n_out, _) = _timed(lambda: R.uctc_greedy(logits, n_steps), reps)
        ref = labels.to(torch.int32)
        kernel['edit_distance'], _ = _timed(lambda: R.edit_distance(ref, n_labels, ids, n_out.long()), reps)

    def torch_ctc():
        x = logits.detach().requires_grad_()
        per = F.ctc_loss(F.log_softmax(x, dim=2).transpose(0, 1), labels, n_steps, n_labels, blank=0, reduction='none')
        per.sum().backward()
        return per.detach()
    torch_ms, per = _timed(torch_ctc, reps)
    ok = status == 0
    agree = float(((loss[ok] - per[ok]).abs() / per[ok].abs()).max())
    print(json.dumps({'metric': 'recognizer', 'batch': B, 'frames': T, 'steps': int(logits.shape[1]), 'labels': L, 'classes': int(logits.shape[2]),
                      'train_step_ms': step_ms, 'train_utterances_per_s': 1e3 * B / step_ms, 'score_ms': score_ms,
                      'score_utterances_per_s': 1e3 * B / score_ms, 'kernel_ms': kernel, 'uctc_share': kernel['uctc_loss'] / step_ms,
                      'torch_ctc_ms': torch_ms, 'uctc_over_torch': kernel['uctc_loss'] / torch_ms, 'agree_loss_max_rel': agree,
                      'rows_skipped': int(skipped), 'rows_ok': int(ok.sum()), 'mean_per_untrained': float(scores['per'].mean())}))


if __name__ == '__main__':
    main()
