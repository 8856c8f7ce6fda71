#!/usr/bin/env python
"""The learned aligner (`daft_exprt/aligner.py`, K28) on a fabricated batch on one MI355X: B = 64 utterances of 300 to 1 000
frames and 40 to 150 symbols, A = 80.

One JSON line.  `kernel_ms`: device-event times (median of --reps after a warm-up) of the five entry points -- soft alignment
forward and backward, forward sum forward and backward, MAS -- and `torch_ms` the same five quantities computed with torch ops in
fp32 on the device: the restatement of tests/aligner_oracle.py a user would write without the kernels (a (B, T, L, A) difference
tensor and log_softmax; a Python loop over the frames with `torch.logaddexp` and autograd through it, -1e30 standing in for
-inf; a loop with `torch.maximum` and a batched backtrack).  `train_step_ms`: one Adam step of `aligner.train_step` on the same
shapes, `encoders_ms` the part of it spent in the two encoders (forward and backward, plain torch modules).
`align_batch_utterances_per_s`: `Aligner.align_batch` as a whole on recordings of 2 to 8 s (wall time, synchronised).
The weights are random: the times depend on the shapes only.  Single samples, nothing here is a gate.
Run:  python tools/bench_aligner.py [--reps 5] [--batch 64]
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

NEG = -1e30


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


def torch_logprob(q, k, n_frm, n_sym, tau, sigma):
    s = -tau * ((q[:, :, None, :] - k[:, None, :, :]) ** 2).sum(-1)
    T, L = s.shape[1], s.shape[2]
    ar_t, ar_l = torch.arange(T, device=q.device), torch.arange(L, device=q.device)
    if sigma > 0:
        ft = (ar_t[None, :, None] + .5) / n_frm[:, None, None]
        fl = (ar_l[None, None, :] + .5) / n_sym[:, None, None]
        s = s - (fl - ft) ** 2 / (2 * sigma ** 2)
    return torch.log_softmax(s.masked_fill(ar_l[None, None, :] >= n_sym[:, None, None], NEG), dim=2)


def torch_forward_sum(logp, n_frm, n_sym):
    B, T, L = logp.shape
    a = torch.full((B, L), NEG, device=logp.device)
    a[:, 0] = logp[:, 0, 0]
    outs, edge = [a], torch.full((B, 1), NEG, device=logp.device)
    for t in range(1, T):
        a = logp[:, t] + torch.logaddexp(a, torch.cat([edge, a[:, :-1]], 1))
        outs.append(a)
    return -torch.stack(outs, 1)[torch.arange(B, device=logp.device), n_frm - 1, n_sym - 1]


def torch_mas(logp, n_frm, n_sym):
    B, T, L = logp.shape
    dev = logp.device
    live = torch.arange(L, device=dev)[None] < n_sym[:, None]
    v = torch.full((B, L), NEG, device=dev)
    v[:, 0] = logp[:, 0, 0]
    steps, edge = [torch.zeros((B, L), dtype=torch.bool, device=dev)], torch.full((B, 1), NEG, device=dev)
    for t in range(1, T):
        left = torch.cat([edge, v[:, :-1]], 1)
        steps.append((left > v) & live)
        v = logp[:, t] + torch.maximum(v, left)
    steps = torch.stack(steps, 1)
    pos, rows, labels = n_sym - 1, torch.arange(B, device=dev), []
    for t in range(T - 1, -1, -1):
        inside = t < n_frm
        labels.append(torch.where(inside, pos, torch.full_like(pos, -1)))
        go = inside & (pos > 0) & ((pos == t) | steps[rows, t, pos])
        pos = pos - go.long()
    return torch.stack(labels[::-1], 1)


def _recordings(batch, fs, seed):
    rng = np.random.RandomState(seed)
    n = (rng.uniform(2.0, 8.0, size=batch) * fs).astype(np.int64)
    wavs = np.zeros((batch, int(n.max())), dtype=np.float32)
    for b in range(batch):
        x = 1e-4 * rng.standard_normal(n[b])
        lo, hi = int(0.2 * fs), n[b] - int(0.3 * fs)
        x[lo:hi] += (0.1 + 0.08 * np.sin(2 * np.pi * rng.uniform(1.0, 4.0) * np.arange(hi - lo) / fs)) * rng.standard_normal(hi - lo)
        wavs[b, :n[b]] = x
    return torch.from_numpy(wavs), n.tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--batch', type=int, default=64)
    args = ap.parse_args()
    import bench
    from daft_exprt import aligner as G
    dev = torch.device('cuda:0')
    hp = bench.make_hparams(args.batch, 'bf16')
    B, A, tau, sigma = args.batch, 80, 0.05, 0.2
    rng = np.random.RandomState(3)
    n_frm = torch.tensor(rng.randint(300, 1001, size=B), dtype=torch.int64)
    n_sym = torch.tensor(rng.randint(40, 151, size=B), dtype=torch.int64)
    n_frm[0], n_sym[0] = 1000, 150
    T, L = int(n_frm.max()), int(n_sym.max())
    n_frm, n_sym = n_frm.to(dev), n_sym.to(dev)
    torch.manual_seed(3)
    q, k = (0.3 * torch.randn(B, T, A, device=dev)).requires_grad_(), (0.3 * torch.randn(B, L, A, device=dev)).requires_grad_()
    g, w = torch.randn(B, T, L, device=dev), torch.full((B,), 1.0 / B, device=dev)
    reps = args.reps
    kernel, torch_ms = {}, {}

    with torch.no_grad():
        kernel['logprob_fwd'], logp = _timed(lambda: G.logprob_fwd(q, k, n_frm, n_sym, tau, sigma), reps)
        kernel['logprob_bwd'], _ = _timed(lambda: G.logprob_bwd(q, k, logp, g, n_frm, n_sym, tau), reps)
        kernel['forward_sum'], (alpha, loss, status) = _timed(lambda: G.forward_sum(logp, n_frm, n_sym), reps)
        kernel['forward_sum_bwd'], _ = _timed(lambda: G.forward_sum_bwd(logp, alpha, w, n_frm, n_sym), reps)
        kernel['mas'], (path, path_len, score, _) = _timed(lambda: G.mas_path(logp, n_frm, n_sym), reps)
        torch_ms['logprob_fwd'], t_logp = _timed(lambda: torch_logprob(q, k, n_frm, n_sym, tau, sigma), reps)
        torch_ms['forward_sum'], t_loss = _timed(lambda: torch_forward_sum(t_logp, n_frm, n_sym), reps)
        torch_ms['mas'], t_labels = _timed(lambda: torch_mas(t_logp, n_frm, n_sym), reps)

    def torch_logprob_bwd():
        out = torch_logprob(q, k, n_frm, n_sym, tau, sigma)
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        torch.autograd.grad(out, (q, k), g)
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e)

    def torch_forward_sum_bwd():
        lp = t_logp.detach().requires_grad_()
        out = torch_forward_sum(lp, n_frm, n_sym)
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        torch.autograd.grad(out, lp, w)
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e)
    for name, fn in (('logprob_bwd', torch_logprob_bwd), ('forward_sum_bwd', torch_forward_sum_bwd)):
        fn()
        torch_ms[name] = float(np.median([fn() for _ in range(reps)]))

    # the two agree (loosely: this is a benchmark, the tests pin the arithmetic)
    live = torch.arange(T, device=dev)[None] < n_frm[:, None]
    labels = torch.where(live, path[:, :T, 1].long(), torch.full((B, T), -1, device=dev))
    agree = {'loss_max_rel': float(((loss - t_loss).abs() / t_loss.abs()).max()), 'mas_labels_equal': float((labels == t_labels).float().mean())}

    # one training step, and the encoders' part of it
    model = G.Aligner(len(hp.symbols), int(hp.n_mel_channels), 256, A, tau, sigma).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    items = [(torch.randint(1, len(hp.symbols), (int(n_sym[b]),), device=dev), torch.randn(int(hp.n_mel_channels), int(n_frm[b]), device=dev))
             for b in range(B)]
    step_ms, _ = _timed(lambda: G.train_step(model, opt, items, dev), reps)
    symbols, ns, mel, nf = G._collate(items, dev)

    def encoders():
        eq, ek = model.encode(symbols, ns, mel, nf)
        torch.autograd.backward((eq, ek), (torch.ones_like(eq), torch.ones_like(ek)))
    enc_ms, _ = _timed(encoders, reps)

    wavs, n_samples = _recordings(B, int(hp.sampling_rate), 7)
    wavs = wavs.to(dev)
    sym = torch.zeros((B, L), dtype=torch.int64, device=dev)
    for b in range(B):
        sym[b, :int(n_sym[b])] = items[b][0]
    n_small = torch.clamp(n_sym, max=100)

    def whole():
        out = model.align_batch(sym, n_small, wavs, n_samples, None, hp)
        torch.cuda.synchronize()
        return out
    whole()
    walls = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = whole()
        walls.append(time.perf_counter() - t0)
    wall = float(np.median(walls))
    print(json.dumps({'metric': 'aligner', 'batch': B, 'T': T, 'L': L, 'A': A, 'kernel_ms': kernel, 'torch_ms': torch_ms, 'agree': agree,
                      'train_step_ms': step_ms, 'encoders_ms': enc_ms, 'encoders_share': enc_ms / step_ms,
                      'align_batch_utterances_per_s': B / wall, 'align_batch_wall_ms': 1e3 * wall,
                      'align_batch_status_ok': int((out['status'] == 0).sum())}))


if __name__ == '__main__':
    main()
