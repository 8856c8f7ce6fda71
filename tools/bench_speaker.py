#!/usr/bin/env python
"""The speaker encoder (`daft_exprt/speaker.py`, K32) on a fabricated batch on one MI355X: B = 256 utterances of 300 to 1 000 frames
(150 to 500 steps at stride 2) of 20 speakers, and the trial histograms of a set the size of a corpus.

One JSON line.  `train_step_ms` / `train_utterances_per_s`: one Adam step of the encoder (forward, `dx_attn_stat_pool_fwd`,
additive-margin softmax, `dx_attn_stat_pool_bwd`, encoder backward, Adam) on the batch.  `score_ms` / `score_utterances_per_s`:
`speaker_scores` on it.  `pool_ms`: device-event times (median of --reps after a warm-up) of the pooling forward + backward through
autograd on the encoder's own (B, steps, 256) frames, `pool_torch_ms`: the same arithmetic stated in plain torch on the device
(masked softmax, two weighted sums, autograd), and `pool_agree`: the largest difference of the two outputs.  `trial_ms`:
`dx_trial_counts` at N = 20 000, D = 128 with the fp32 FLOP/s it achieves (N (N - 1) D over the time: one multiply-add per pair and
column), `trial_torch_ms`: chunked `torch.matmul` + `torch.histc` over the same pairs, and `trial_agree_abs_diff`: the summed
absolute difference of the two histograms (pairs whose score sits at a bin edge may fall either way; the tests judge that, not this
tool).  The weights are random: the times depend on the shapes only.  Single samples, nothing here is a gate.
Run:  python tools/bench_speaker.py [--reps 5] [--batch 256] [--rows 20000]
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


def pool_torch(h, a, n_steps):
    ''' attentive statistics pooling in plain torch on the device '''
    live = torch.arange(h.shape[1], device=h.device)[None] < n_steps[:, None]
    w = torch.softmax(a.masked_fill(~live, float('-inf')), dim=1)
    mu = (w[:, :, None] * h).sum(dim=1)
    d = (h - mu[:, None]) * live[:, :, None]
    return torch.cat([mu, torch.sqrt((w[:, :, None] * d * d).sum(dim=1) + 1e-5)], dim=1)


def trials_torch(E, spk, chunk=2048):
    ''' the two histograms with chunked matrix products and `torch.histc` '''
    N = E.shape[0]
    counts = torch.zeros((2, 4096), dtype=torch.float64, device=E.device)
    idx = torch.arange(N, device=E.device)
    for i0 in range(0, N, chunk):
        s = E[i0: i0 + chunk] @ E.t()
        upper = idx[None] > idx[i0: i0 + chunk, None]
        same = spk[i0: i0 + chunk, None] == spk[None]
        b = ((s + 1.0) * 2048.0).floor().clamp(0, 4095)
        for row, mask in ((0, upper & same), (1, upper & ~same)):
            counts[row] += torch.histc(b[mask], bins=4096, min=0, max=4096).double()
    return counts.long()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--rows', type=int, default=20000)
    args = ap.parse_args()
    from daft_exprt import speaker as S
    dev = torch.device('cuda:0')
    B, reps, n_mel, speakers = args.batch, args.reps, 80, 20
    rng = np.random.RandomState(3)
    n_frm = rng.randint(300, 1001, size=B)
    n_frm[0] = 1000
    T = int(n_frm.max())
    torch.manual_seed(3)
    enc = S.SpeakerEncoder(n_mel).to(dev)
    weights = torch.nn.Parameter(torch.randn((speakers, enc.args['dim']), device=dev))
    mel = (2.0 * torch.randn(B, n_mel, T) - 5.0).to(dev)
    n_frm = torch.from_numpy(n_frm).to(dev)
    spk = torch.from_numpy(rng.randint(0, speakers, size=B)).to(dev)
    opt = torch.optim.Adam(list(enc.parameters()) + [weights], lr=1e-3)

    def step():
        loss = S.am_softmax_loss(enc(mel, n_frm), weights, spk)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        return loss
    step_ms, _ = _timed(step, reps)
    enc.eval()
    with torch.no_grad():
        enc.set_speakers(list(range(speakers)), S.speaker_centroids(enc.embed(mel, n_frm), spk, speakers), threshold=0.5)
        h, a, n_steps = enc.frames(mel, n_frm)
    score_ms, _ = _timed(lambda: S.speaker_scores(enc, mel, n_frm, spk), reps)

    def pool(fn):
        def run():
            x, y = h.detach().requires_grad_(), a.detach().requires_grad_()
            out = fn(x, y, n_steps)
            out.sum().backward()
            return out.detach()
        return run
    pool_ms, out = _timed(pool(S.attn_stat_pool), reps)
    pool_torch_ms, want = _timed(pool(pool_torch), reps)

    N, D = args.rows, 128
    E = F.normalize(torch.randn(N, D, device=dev), dim=1)
    ids = torch.from_numpy(rng.randint(0, 100, size=N).astype(np.int32)).to(dev)
    trial_ms, counts = _timed(lambda: S.trial_counts(E, ids), reps)
    trial_torch_ms, want_counts = _timed(lambda: trials_torch(E, ids), reps)
    print(json.dumps({'metric': 'speaker', 'batch': B, 'frames': T, 'steps': int(h.shape[1]), 'channels': int(h.shape[2]),
                      'train_step_ms': step_ms, 'train_utterances_per_s': 1e3 * B / step_ms, 'score_ms': score_ms,
                      'score_utterances_per_s': 1e3 * B / score_ms, 'pool_ms': pool_ms, 'pool_torch_ms': pool_torch_ms,
                      'pool_over_torch': pool_ms / pool_torch_ms, 'pool_share': pool_ms / step_ms, 'pool_agree': float((out - want).abs().max()),
                      'trial_rows': N, 'trial_dim': D, 'trials': int(counts.sum()), 'trial_ms': trial_ms,
                      'trial_fp32_tflops': N * (N - 1.0) * D / (trial_ms * 1e-3) / 1e12, 'trial_torch_ms': trial_torch_ms,
                      'trial_over_torch': trial_ms / trial_torch_ms, 'trial_agree_abs_diff': int((counts - want_counts).abs().sum())}))


if __name__ == '__main__':
    main()
