#!/usr/bin/env python
"""The g2p model (`daft_exprt/g2p.py`, K30) on a fabricated lexicon on one MI355X: 10^5 toy words of 2 to 10 letters
(`tests/ctc_oracle.toy_lexicon`), 3 output slots per letter, 19 classes.

One JSON line.  `train_words_per_s`: Adam steps of --batch words as `train_g2p` runs them (encoder forward, `dx_ctc_loss`, encoder
backward, Adam; batches cut from one permutation per epoch and sorted by length, `g2p.length_sorted_batches`), wall time over --steps steps after a warm-up, synchronised at
the ends only.  `step_ms` the same per step; `ctc_loss_ms` the device-event time (median of --reps) of the one K30 launch of a step
on a batch of that shape, `ctc_share` its share of a step; `torch_ctc_ms`: `F.ctc_loss` forward and backward on the same logits
on the device, the comparison a user would write without the kernel.  `phonemize_words_per_s`: `G2P.phonemize` over all 10^5 words
(host packing, encoder, `dx_ctc_greedy`, read-back; wall time), `ctc_greedy_ms` the decode launch alone on --batch words.
The weights are random: the times depend on the shapes only.  Single samples, nothing here is a gate.
Run:  python tools/bench_g2p.py [--words 100000] [--batch 1024] [--steps 50] [--reps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'ubisoft-laforge-daft-exprt_amd')):
    sys.path.insert(0, p)


def _timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    return float(np.median(ts))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--words', type=int, default=100000)
    parser.add_argument('--batch', type=int, default=1024)
    parser.add_argument('--steps', type=int, default=50)
    parser.add_argument('--reps', type=int, default=5)
    parser.add_argument('--hidden', type=int, default=128)
    args = parser.parse_args()
    from daft_exprt.g2p import G2P, ctc_greedy, ctc_loss, ctc_loss_and_grad, length_sorted_batches
    from tests import ctc_oracle as O
    dev = torch.device('cuda:0')
    lexicon = O.toy_lexicon(seed=99, words=args.words)
    g, n, lab, nl = (t.to(dev) for t in O.toy_pack(lexicon))
    lengths = [len(w) for w, _ in lexicon]
    torch.manual_seed(0)
    model = G2P(O.TOY_PHONES, hidden=args.hidden).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=2e-3)
    gen = torch.Generator().manual_seed(0)

    batches = length_sorted_batches(lengths, args.batch, gen)

    def draw():
        idx, L = next(batches)
        return idx.to(dev), L

    def step():
        idx, L = draw()
        logits, n_steps = model(g[idx, :L].contiguous(), n[idx])
        loss, _ = ctc_loss(logits, n_steps, lab[idx].contiguous(), nl[idx].contiguous())
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()

    for _ in range(5):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    step_ms = (time.perf_counter() - t0) * 1e3 / args.steps

    idx, L = draw()
    with torch.no_grad():
        logits, n_steps = model(g[idx, :L].contiguous(), n[idx])
    labels, n_labels = lab[idx].contiguous(), nl[idx].contiguous()
    ctc_ms = _timed(lambda: ctc_loss_and_grad(logits, n_steps, labels, n_labels), args.reps)
    greedy_ms = _timed(lambda: ctc_greedy(logits, n_steps), args.reps)

    def torch_ctc():
        x = logits.detach().requires_grad_()
        F.ctc_loss(F.log_softmax(x, 2).transpose(0, 1), labels, n_steps, n_labels, reduction='none').mean().backward()
    try:
        torch_ms = round(_timed(torch_ctc, args.reps), 3)
    except RuntimeError as err:                                   # (this build's F.ctc_loss may not take these inputs on the device)
        print(f'F.ctc_loss on the device failed: {err}', file=sys.stderr)
        torch_ms = None

    words = [w for w, _ in lexicon]
    model.phonemize(words[:2048])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model.phonemize(words)
    torch.cuda.synchronize()
    phon_s = time.perf_counter() - t0
    print(json.dumps(dict(words=len(lexicon), batch=args.batch, hidden=args.hidden, steps=args.steps, step_ms=round(step_ms, 3),
                          train_words_per_s=round(args.batch / step_ms * 1e3), ctc_loss_ms=round(ctc_ms, 4),
                          ctc_share=round(ctc_ms / step_ms, 4), torch_ctc_ms=torch_ms,ctc_greedy_ms=round(greedy_ms, 4),
                          phonemize_words_per_s=round(len(words) / phon_s), logits_shape=list(logits.shape),
                          device=torch.cuda.get_device_name(0))))


if __name__ == '__main__':
    main()
