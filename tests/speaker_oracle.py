"""Oracles of K32 and daft_exprt/speaker.py, written from the K32 comment of include/daft_exprt_hip.h.

(1) Attentive statistics pooling and its gradient in NumPy for a given dtype -- float64 is the oracle, float32 the restatement that
sets the bound of the GPU test -- with the variance about the mean, and `pool_one_pass`, the shortcut sum w h^2 - mu^2 the kernel
must not take.  (2) The trial histograms as a float64 matrix product plus binning, `trial_counts_loops` the same as a plain double
loop, and two statements of the equal error rate that share nothing with `speaker.eer_from_counts`: `eer_loop` over the bins in
exact fractions, `eer_sorted` over sorted scores.  (3) The ragged cases of the GPU tests.  (4) The toy corpus of the learnability
test -- `recognizer_oracle`'s fabricated phone templates plus a fixed per-channel offset per speaker -- and the plain-torch float64
CPU restatement of the encoder on it: the tests take their ceilings from it, never from the code under test.
"""
from fractions import Fraction

import numpy as np

from tests import recognizer_oracle as RO

VAR_EPS = 1e-5
BINS = 4096


# ---- the pooling ---------------------------------------------------------------------------------------------------------------------------

def _weights(a, n, dtype):
    x = np.asarray(a[:n], dtype=dtype)
    m = x.max()
    e = np.exp(x - m)
    l = e.sum(dtype=dtype)
    return e / l, m, l


def pool(h, a, n_steps, dtype=np.float64):
    ''' h (B, T, C), a (B, T), n_steps (B,) -> out (B, 2 C) = [mu, sd], stat (B, 2) = (max, normaliser), every operation in `dtype`;
        nothing at or past n_steps is read; a row without steps is zeros '''
    B, T, C = h.shape
    out, stat = np.zeros((B, 2 * C), dtype=dtype), np.zeros((B, 2), dtype=dtype)
    for b in range(B):
        n = int(min(max(n_steps[b], 0), T))
        if n == 0:
            continue
        w, m, l = _weights(a[b], n, dtype)
        x = np.asarray(h[b, :n], dtype=dtype)
        mu = (w[:, None] * x).sum(axis=0, dtype=dtype)
        d = x - mu
        var = (w[:, None] * d * d).sum(axis=0, dtype=dtype)
        out[b, :C], out[b, C:] = mu, np.sqrt(var + dtype(VAR_EPS))
        stat[b] = m, l
    return out, stat


def pool_one_pass(h, a, n_steps, dtype=np.float32):
    ''' the same with var = sum w h^2 - mu^2 in one pass (clamped at 0): what the kernel must NOT compute '''
    B, T, C = h.shape
    out = np.zeros((B, 2 * C), dtype=dtype)
    for b in range(B):
        n = int(min(max(n_steps[b], 0), T))
        if n == 0:
            continue
        w, _, _ = _weights(a[b], n, dtype)
        x = np.asarray(h[b, :n], dtype=dtype)
        mu = (w[:, None] * x).sum(axis=0, dtype=dtype)
        var = np.maximum((w[:, None] * x * x).sum(axis=0, dtype=dtype) - mu * mu, dtype(0))
        out[b, :C], out[b, C:] = mu, np.sqrt(var + dtype(VAR_EPS))
    return out


def pool_grad(h, a, n_steps, g_out, dtype=np.float64):
    ''' the gradients (g_h (B, T, C), g_a (B, T)) of sum(out * g_out), zeros at and past n_steps '''
    B, T, C = h.shape
    g_h, g_a = np.zeros((B, T, C), dtype=dtype), np.zeros((B, T), dtype=dtype)
    out, _ = pool(h, a, n_steps, dtype)
    for b in range(B):
        n = int(min(max(n_steps[b], 0), T))
        if n == 0:
            continue
        w, _, _ = _weights(a[b], n, dtype)
        mu, sd = out[b, :C], out[b, C:]
        g_mu, g_sd = np.asarray(g_out[b, :C], dtype=dtype), np.asarray(g_out[b, C:], dtype=dtype)
        d = np.asarray(h[b, :n], dtype=dtype) - mu
        g_h[b, :n] = w[:, None] * (g_mu + g_sd * d / sd)
        q = (g_mu * d + g_sd * d * d / (dtype(2) * sd)).sum(axis=1, dtype=dtype)
        g_a[b, :n] = w * (q - (w * q).sum(dtype=dtype))
    return g_h, g_a


def pool_torch(h, a, n_steps):
    ''' the plain masked-softmax statement in torch, differentiable: the definition `pool` is pinned against '''
    import torch
    B, T, C = h.shape
    live = torch.arange(T)[None] < n_steps[:, None]
    w = torch.softmax(a.masked_fill(~live, float('-inf')), dim=1)
    w = torch.where(live, w, torch.zeros_like(w))                      # (a row without steps: softmax of all -inf is NaN)
    x = torch.where(live[:, :, None], h, torch.zeros_like(h))
    mu = (w[:, :, None] * x).sum(dim=1)
    d = torch.where(live[:, :, None], x - mu[:, None], torch.zeros_like(x))
    sd = torch.sqrt((w[:, :, None] * d * d).sum(dim=1) + VAR_EPS)
    out = torch.cat([mu, sd], dim=1)
    return torch.where((n_steps > 0)[:, None], out, torch.zeros_like(out))


POOL_CHANNELS = (20, 64, 192, 260)
POOL_STEPS = (0, 1, 2, 63, 64, 65, 255, 256, 257, 1000)


def pool_case(C, seed=0):
    ''' the ragged batch of the GPU test: rows of POOL_STEPS steps, h ~ 2 x normal + a channel offset, a ~ 2 x normal, g_out normal '''
    rng = np.random.RandomState(100 * seed + C)
    B, T = len(POOL_STEPS), max(POOL_STEPS)
    h = (2.0 * rng.standard_normal((B, T, C)) + rng.standard_normal((1, 1, C))).astype(np.float32)
    a = (2.0 * rng.standard_normal((B, T))).astype(np.float32)
    g_out = rng.standard_normal((B, 2 * C)).astype(np.float32)
    return dict(C=C, B=B, T=T, h=h, a=a, n_steps=np.array(POOL_STEPS, dtype=np.int64), g_out=g_out)


def offset_case(n=257, C=64, seed=9):
    ''' one row whose channels have mean 100 and standard deviation 0.1: the variance is 1e-2 beside a mean square of 1e+4 '''
    rng = np.random.RandomState(seed)
    h = (100.0 + 0.1 * rng.standard_normal((1, n, C))).astype(np.float32)
    a = rng.standard_normal((1, n)).astype(np.float32)
    return dict(C=C, B=1, T=n, h=h, a=a, n_steps=np.array([n], dtype=np.int64), g_out=rng.standard_normal((1, 2 * C)).astype(np.float32))


# ---- the trials ----------------------------------------------------------------------------------------------------------------------------

def _bins(s):
    return np.clip(np.floor((s + 1.0) * (BINS / 2)), 0, BINS - 1).astype(np.int64)


def trial_scores(E, spk):
    ''' (float64 scores of all pairs i < j, same-speaker flags), pairs in row-major order of the upper triangle '''
    E = np.asarray(E, dtype=np.float64)
    i, j = np.triu_indices(E.shape[0], 1)
    return (E @ E.T)[i, j], np.asarray(spk)[i] == np.asarray(spk)[j]


def trial_counts(E, spk):
    ''' counts (2, 4096) int64: row 0 the pairs of one speaker, row 1 the others, over bin = clamp(floor((s + 1) 2048), 0, 4095) '''
    s, same = trial_scores(E, spk)
    b = _bins(s)
    return np.stack([np.bincount(b[same], minlength=BINS), np.bincount(b[~same], minlength=BINS)]).astype(np.int64)


def trial_counts_loops(E, spk):
    ''' the definition as a plain double loop over all pairs '''
    counts = np.zeros((2, BINS), dtype=np.int64)
    for i in range(len(E)):
        for j in range(i + 1, len(E)):
            s = sum(float(x) * float(y) for x, y in zip(E[i], E[j]))
            counts[0 if spk[i] == spk[j] else 1, min(max(int(np.floor((s + 1.0) * 2048.0)), 0), BINS - 1)] += 1
    return counts


def exact_rows(N, D, n_speakers, seed=0):
    ''' rows of unit length whose dot products are exact in fp32 in any order: 64 entries of +-1/8 among D >= 64 columns, or 16 of
        +-1/4 among D < 64.  Every fifth row repeats an earlier one (s = 1: the top bin by the clamp), every seventh negates one
        (s = -1: bin 0).  Speakers 0 .. n_speakers - 1 at random '''
    rng = np.random.RandomState(1000 * seed + 7 * N + D)
    k, v = (64, 0.125) if D >= 64 else (16, 0.25)
    E = np.zeros((N, D), dtype=np.float32)
    for r in range(N):
        if r >= 2 and r % 5 == 0:
            E[r] = E[rng.randint(0, r)]
        elif r >= 2 and r % 7 == 0:
            E[r] = -E[rng.randint(0, r)]
        else:
            E[r, rng.choice(D, k, replace=False)] = v * rng.choice([-1.0, 1.0], size=k)
    return E, rng.randint(0, n_speakers, size=N).astype(np.int32)


def eer_loop(counts):
    ''' the equal error rate over the thresholds k = 0 .. 4096 (accept bin >= k) in exact fractions: (eer, k), None without a class '''
    tar, non = [int(v) for v in counts[0]], [int(v) for v in counts[1]]
    n_tar, n_non = sum(tar), sum(non)
    if n_tar == 0 or n_non == 0:
        return None
    best, rejected, accepted = None, 0, n_non
    for k in range(BINS + 1):
        far, frr = Fraction(accepted, n_non), Fraction(rejected, n_tar)
        if best is None or abs(far - frr) < best[0]:
            best = (abs(far - frr), (far + frr) / 2, k)
        if k < BINS:
            rejected, accepted = rejected + tar[k], accepted - non[k]
    return float(best[1]), best[2]


def eer_sorted(target_scores, other_scores, thresholds):
    ''' the equal error rate over the given ascending thresholds (accept s >= threshold) from the scores themselves, by sorting and
        searching: (eer, threshold) '''
    tar, non = np.sort(np.asarray(target_scores, dtype=np.float64)), np.sort(np.asarray(other_scores, dtype=np.float64))
    best = None
    for th in thresholds:
        rejected = int(np.searchsorted(tar, th, side='left'))              # targets below the threshold
        accepted = len(non) - int(np.searchsorted(non, th, side='left'))   # non-targets at or above it
        far, frr = Fraction(accepted, len(non)), Fraction(rejected, len(tar))
        if best is None or abs(far - frr) < best[0]:
            best = (abs(far - frr), (far + frr) / 2, th)
    return float(best[1]), float(best[2])


# ---- the toy corpus: the recogniser's phone templates plus a spectral envelope per speaker, and the restated encoder -----------------------

TOY = dict(speakers=6, n_mel=16, per_speaker=40, held_out=10, noise=0.3, offset=0.25, hidden=64, layers=2, stride=2, dim=32, steps=300,
           batch=32, lr=3e-3, scale=30.0, margin=0.2, corpus_seed=8642)
# toy_restatement(seed), seeds 0 .. 5: the held-out identification error and equal error rate of the float64 CPU restatement, and the
# ceilings of the GPU tests: the maximum over the seeds plus their spread (max - min)
# (untrained: identification error 0.35 to 0.47, equal error rate 0.41 to 0.46)
RESTATEMENT_ID = (2 / 60, 1 / 60, 0.0, 0.0, 0.0, 0.0)                                  # ceiling 0.0667: 4 of the 60 held-out utterances
RESTATEMENT_EER = (0.037185, 0.015741, 0.000333, 0.014741, 0.014741, 0.000667)        # ceiling 0.074037
CEILING_ID = max(RESTATEMENT_ID) + (max(RESTATEMENT_ID) - min(RESTATEMENT_ID))
CEILING_EER = max(RESTATEMENT_EER) + (max(RESTATEMENT_EER) - min(RESTATEMENT_EER))


def toy_offsets():
    ''' (speakers, n_mel) float64: the fixed random per-channel offset -- a spectral envelope -- of every speaker '''
    import torch
    g = torch.Generator().manual_seed(TOY['corpus_seed'])
    return TOY['offset'] * torch.randn(TOY['speakers'], TOY['n_mel'], generator=g, dtype=torch.float64)


def toy_corpus(seed=TOY['corpus_seed']):
    ''' (train, held): lists of (speaker 0 .. 5, mel (T, n_mel) float64).  Every speaker has 40 utterances of 4 to 12 phones of
        `recognizer_oracle`'s templates, 2 to 7 frames each, plus 0.3 x Gaussian noise, plus the speaker's offset on every frame;
        the first 30 of a speaker train, the last 10 are held out '''
    import torch
    g = torch.Generator().manual_seed(seed + 1)
    offsets = toy_offsets()
    train, held = [], []
    for s in range(TOY['speakers']):
        for u in range(TOY['per_speaker']):
            L = int(torch.randint(4, 13, (1,), generator=g))
            cls = []
            while len(cls) < L:
                c = int(torch.randint(1, RO.TOY['classes'] + 1, (1,), generator=g))
                if not cls or cls[-1] != c:
                    cls.append(c)
            dur = torch.randint(2, 8, (L,), generator=g)
            noise = TOY['noise'] * torch.randn(int(dur.sum()), TOY['n_mel'], generator=g, dtype=torch.float64)
            mel = RO.toy_fabricate(torch.tensor(cls), dur, noise) + offsets[s]
            (train if u < TOY['per_speaker'] - TOY['held_out'] else held).append((s, mel))
    return train, held


def toy_collate(utts, dtype):
    ''' -> mel (B, n_mel, T) zero-padded, n_frames (B,) int64, speakers (B,) int64 '''
    import torch
    B, T = len(utts), max(u[1].shape[0] for u in utts)
    mel = torch.zeros(B, TOY['n_mel'], T, dtype=dtype)
    for b, (_, m) in enumerate(utts):
        mel[b, :, :m.shape[0]] = m.T.to(dtype)
    return mel, torch.tensor([u[1].shape[0] for u in utts]), torch.tensor([u[0] for u in utts])


def toy_batches(seed, n_train):
    ''' the utterance indices of every training step '''
    import torch
    g = torch.Generator().manual_seed(seed)
    return [torch.randperm(n_train, generator=g)[:TOY['batch']].tolist() for _ in range(TOY['steps'])]


def toy_restatement(seed, return_untrained=False):
    ''' trains the restated encoder (the architecture, loss, data and schedule of the learnability test) in float64 on the CPU with
        `pool_torch` and returns (held-out identification error, held-out equal error rate) -- centroids from the training
        utterances, the EER over all held-out pairs through `trial_counts` and `eer_loop` of this file '''
    import torch
    import torch.nn as nn
    import torch.nn.functional as F
    dt = torch.float64
    Hd, R, M, S, Dm = TOY['hidden'], TOY['stride'], TOY['n_mel'], TOY['speakers'], TOY['dim']

    class Toy(nn.Module):
        def __init__(s):
            super().__init__()
            s.c1, s.c2 = nn.Conv1d(M * R, Hd, 3, padding=1), nn.Conv1d(Hd, Hd, 3, padding=1)
            s.a1, s.a2, s.out = nn.Linear(Hd, 64), nn.Linear(64, 1), nn.Linear(2 * Hd, Dm)

        def forward(s, mel, n):
            T = mel.shape[2]
            live = (torch.arange(T)[None] < n[:, None]).to(dt)[:, None]
            cnt = (n * M).to(dt)[:, None, None]
            mean = (mel * live).sum((1, 2), keepdim=True) / cnt
            cen = (mel - mean) * live
            x = cen * torch.rsqrt((cen * cen).sum((1, 2), keepdim=True) / cnt + 1e-5)
            Ts = (T + R - 1) // R
            x = F.pad(x, (0, Ts * R - T)).transpose(1, 2).reshape(mel.shape[0], Ts, R * M).transpose(1, 2)
            ns = (n + R - 1) // R
            m = (torch.arange(Ts)[None] < ns[:, None]).to(dt)[:, None]
            h = torch.relu(s.c2(torch.relu(s.c1(x * m)) * m)).transpose(1, 2)
            a = s.a2(torch.tanh(s.a1(h)))[:, :, 0]
            return F.normalize(s.out(pool_torch(h, a, ns)), dim=1)

    train, held = toy_corpus()
    tmel, tn, tspk = toy_collate(train, dt)
    hmel, hn, hspk = toy_collate(held, dt)

    def rates(model):
        with torch.no_grad():
            sums = torch.zeros(S, Dm, dtype=dt).index_add_(0, tspk, model(tmel, tn))
            centroids = F.normalize(sums / torch.bincount(tspk, minlength=S)[:, None], dim=1)
            emb = model(hmel, hn)
        wrong = (emb @ centroids.t()).argmax(dim=1) != hspk
        return float(wrong.double().mean()), eer_loop(trial_counts(emb.numpy(), hspk.numpy()))[0]

    torch.manual_seed(seed)
    model = Toy().to(dt)
    classes = nn.Parameter(torch.randn(S, Dm, dtype=dt))
    untrained = rates(model)
    opt = torch.optim.Adam(list(model.parameters()) + [classes], lr=TOY['lr'])
    for idx in toy_batches(seed, len(train)):
        idx = torch.tensor(idx)
        cos = model(tmel[idx], tn[idx]) @ F.normalize(classes, dim=1).t()
        loss = F.cross_entropy(TOY['scale'] * (cos - TOY['margin'] * F.one_hot(tspk[idx], S).to(dt)), tspk[idx])
        opt.zero_grad()
        loss.backward()
        opt.step()
    return (rates(model), untrained) if return_untrained else rates(model)


if __name__ == '__main__':
    import sys
    for seed in range(int(sys.argv[1]) if len(sys.argv) > 1 else 6):
        print(seed, [[round(v, 6) for v in pair] for pair in toy_restatement(seed, return_untrained=True)], flush=True)
