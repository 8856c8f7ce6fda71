"""NumPy restatement of the contracts of K30 (include/daft_exprt_hip.h: dx_ctc_loss, dx_ctc_greedy), written from the header text.

Every function takes `dtype`: np.float64 is the oracle; np.float32 is the same recurrences in the kernels' precision, which the GPU
tests use to learn what rounding alone does.  Sums over the class axis and over the states of a class are NumPy's (pairwise, or in
order of s): the kernel's butterflies add in another order, which is why the GPU tests allow a multiple of the measured deviation.
`enumerate_loss` sums over ALL alignments of a tiny case and shares nothing with the recurrence.  Loops over the batch and over time
are plain Python: the shapes of the tests are small.

The second half is the toy lexicon of the learnability test and the plain-torch float64 CPU restatement of the whole g2p model on
it (encoder, expansion, `F.ctc_loss`, Adam, greedy decode): the test takes its ceiling from it, never from the code under test.
"""
import itertools

import numpy as np

GRAPHEMES = "abcdefghijklmnopqrstuvwxyz'"       # id 1 + index; id 0 pads


def repeats_of(labels):
    return sum(1 for u in range(1, len(labels)) if labels[u] == labels[u - 1])


def status_of(n_steps, labels, V):
    ''' 2: no step; else 3: a label outside [1, V - 1]; else 1: fewer steps than labels + adjacent equal pairs; else 0 '''
    if n_steps <= 0:
        return 2
    if any(l < 1 or l >= V for l in labels):
        return 3
    return 1 if n_steps < len(labels) + repeats_of(labels) else 0


def lse3(a, b, c, dtype):
    ''' log(exp(a) + exp(b) + exp(c)), the terms added in this order; -inf for three -inf '''
    a, b, c = (np.asarray(v, dtype=dtype) for v in (a, b, c))
    m = np.maximum(np.maximum(a, b), c)
    with np.errstate(invalid='ignore', divide='ignore'):
        ms = np.where(np.isneginf(m), dtype(0), m)
        r = m + np.log((np.exp(a - ms) + np.exp(b - ms)) + np.exp(c - ms))
    return np.where(np.isneginf(m), dtype(-np.inf), r).astype(dtype)


def logaddexp(a, b, dtype):
    m, n = max(a, b), min(a, b)
    return dtype(m) if np.isneginf(m) else dtype(dtype(m) + np.log1p(np.exp(dtype(n) - dtype(m)), dtype=dtype))


def step_lse(x, dtype):
    ''' x (T, V) -> z (T,): max + log(sum(exp(x - max))) '''
    x = np.asarray(x, dtype=dtype)
    m = x.max(axis=1)
    return (m + np.log(np.exp(x - m[:, None]).sum(axis=1, dtype=dtype))).astype(dtype)


def ctc_loss(logits, n_steps, labels, n_labels, w=None, dtype=np.float64):
    ''' logits (B, T, V), labels (B, U) -> loss (B,) (NaN where status != 0), status (B,) int32, grad (B, T, V) = w[b] dloss[b]/dlogits '''
    logits = np.asarray(logits, dtype=dtype)
    B, T, V = logits.shape
    w = np.ones((B,), dtype=dtype) if w is None else np.asarray(w, dtype=dtype)
    loss, status, grad = np.full((B,), np.nan, dtype=dtype), np.zeros((B,), dtype=np.int32), np.zeros((B, T, V), dtype=dtype)
    ninf = dtype(-np.inf)
    for b in range(B):
        nT, nL = int(n_steps[b]), int(n_labels[b])
        lab = [int(l) for l in np.asarray(labels)[b, :nL]] if nL else []
        status[b] = status_of(nT, lab, V)
        if status[b] != 0:
            continue
        S = 2 * nL + 1
        ext = np.zeros((S,), dtype=np.int64)
        ext[1::2] = lab
        skip = np.zeros((S,), dtype=bool)
        for s in range(3, S, 2):
            skip[s] = ext[s] != ext[s - 2]
        x = logits[b, :nT]
        z = step_lse(x, dtype)
        lp = (x - z[:, None]).astype(dtype)
        em = lp[:, ext]                                           # (nT, S)
        alpha = np.full((nT, S), ninf, dtype=dtype)
        alpha[0, 0] = em[0, 0]
        if S > 1:
            alpha[0, 1] = em[0, 1]
        for t in range(1, nT):
            a = alpha[t - 1]
            p1 = np.concatenate([[ninf], a[:-1]]).astype(dtype)
            p2 = np.where(skip, np.concatenate([[ninf, ninf], a[:-2]])[:S], ninf).astype(dtype)
            alpha[t] = (em[t] + lse3(a, p1, p2, dtype)).astype(dtype)
        ll = logaddexp(alpha[nT - 1, S - 1], alpha[nT - 1, S - 2] if S > 1 else ninf, dtype)
        loss[b] = -ll
        beta = np.full((S,), ninf, dtype=dtype)
        beta[S - 1] = 0
        if S > 1:
            beta[S - 2] = 0
        skipf = np.concatenate([skip[2:], [False, False]])[:S]
        gamma = np.zeros((nT, S), dtype=dtype)
        with np.errstate(invalid='ignore'):
            for t in range(nT - 1, -1, -1):
                if t + 1 < nT:
                    c = (em[t + 1] + beta).astype(dtype)
                    n1 = np.concatenate([c[1:], [ninf]]).astype(dtype)
                    n2 = np.where(skipf, np.concatenate([c[2:], [ninf, ninf]])[:S], ninf).astype(dtype)
                    beta = lse3(c, n1, n2, dtype)
                gamma[t] = np.exp((alpha[t] + beta).astype(dtype) - ll)
        gamma = np.where(np.isnan(gamma), 0, gamma).astype(dtype)
        post = np.zeros((nT, V), dtype=dtype)
        for s in range(S):                                        # the states of a class in order of s
            post[:, ext[s]] = (post[:, ext[s]] + gamma[:, s]).astype(dtype)
        grad[b, :nT] = (w[b] * (np.exp(lp) - post)).astype(dtype)
    return loss, status, grad


def collapse(path):
    ''' runs of one class to one entry, then the blanks dropped '''
    out, prev = [], 0
    for p in path:
        if p != 0 and p != prev:
            out.append(int(p))
        prev = p
    return out


def greedy(logits, n_steps, dtype=np.float64):
    ''' -> ids (B, T) int32 zero-filled, n_out (B,) int32, score (B,): sum_t max_v log-probability; the lowest class wins a tie '''
    logits = np.asarray(logits, dtype=dtype)
    B, T, V = logits.shape
    ids, n_out, score = np.zeros((B, T), dtype=np.int32), np.zeros((B,), dtype=np.int32), np.zeros((B,), dtype=dtype)
    for b in range(B):
        nT = int(n_steps[b])
        if nT == 0:
            continue
        x = logits[b, :nT]
        out = collapse(np.argmax(x, axis=1))                      # (np.argmax returns the first maximum)
        ids[b, :len(out)], n_out[b] = out, len(out)
        sc = dtype(0)
        for t in range(nT):                                       # in order of t
            sc = dtype(sc + (-np.log(np.exp(x[t] - x[t].max()).sum(dtype=dtype))))
        score[b] = sc
    return ids, n_out, score


def enumerate_loss(logits, labels):
    ''' -log of the summed probability of ALL T-step paths over V classes that collapse to `labels`; inf when there is none.
        logits (T, V) float64.  No recurrence: V ** T products. '''
    x = np.asarray(logits, dtype=np.float64)
    T, V = x.shape
    p = np.exp(x - x.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    total = 0.0
    for path in itertools.product(range(V), repeat=T):
        if collapse(path) == list(labels):
            total += float(np.prod([p[t, c] for t, c in enumerate(path)]))
    return -np.log(total) if total > 0 else np.inf


def edit_distance(a, b):
    ''' Levenshtein distance of two sequences '''
    row = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        prev, row[0] = row[0], i
        for j, y in enumerate(b, 1):
            prev, row[j] = row[j], min(row[j] + 1, row[j - 1] + 1, prev + (x != y))
    return row[len(b)]


def phone_error_rate(decodes, references):
    ''' summed edit distance / summed reference length; a decode of None counts as empty '''
    dist = sum(edit_distance(d or [], r) for d, r in zip(decodes, references))
    return dist / max(1, sum(len(r) for r in references))


# ---- the shapes of the GPU tests (tests/test_gpu_g2p.py), shared with the host test that pins this oracle on them ---------------------------

# (n_steps, n_labels): the smallest, two equal labels with exactly the steps they need, S = 2 U + 1 across one wave (63 / 65 states),
# several states per lane, and the two limits together; then a row without a path (two equal labels, two steps) and a row without steps
SHAPES = ((1, 0), (1, 1), (2, 1), (3, 2), (5, 2), (64, 31), (65, 32), (192, 64), (256, 127))
DEAD = ((2, 2), (0, 3))
CLASSES = (2, 29, 77, 128)


def gpu_case(V, seed=0):
    ''' a ragged batch over V classes: logits (B, T, V) fp32 = 2 x standard normal, labels (B, U) int64 that repeat their
        neighbour 3 times in 10 (the (3, 2) row and the (2, 2) row always), w (B,) fp32 in [0.5, 2] '''
    rng = np.random.RandomState(1000 * seed + V)
    shapes = SHAPES + DEAD
    B, T, U = len(shapes), max(s[0] for s in shapes), max(s[1] for s in shapes)
    logits = (2.0 * rng.standard_normal((B, T, V))).astype(np.float32)
    labels = np.zeros((B, U), dtype=np.int64)
    for b, (nT, nL) in enumerate(shapes):
        for u in range(nL):
            again = u > 0 and (rng.uniform() < 0.3 or (nT, nL) in ((3, 2), (2, 2)))
            labels[b, u] = labels[b, u - 1] if again else rng.randint(1, V)
    return dict(V=V, B=B, T=T, U=U, logits=logits, labels=labels, n_steps=np.array([s[0] for s in shapes], dtype=np.int64),
                n_labels=np.array([s[1] for s in shapes], dtype=np.int64), w=rng.uniform(0.5, 2.0, size=B).astype(np.float32),
                status=np.array([0] * len(SHAPES) + [1, 2], dtype=np.int32))


# ---- the toy lexicon: random spellings over 12 letters, pronounced by deterministic context rules ------------------------------------------

TOY_LETTERS = 'aeiobdkshtxn'
TOY_VOWELS = {'a': ('AE1', 'EY1'), 'e': ('EH1', 'IY1'), 'i': ('IH1', 'AY1'), 'o': ('AA1', 'OW1')}     # (plain, before consonant + final e)
TOY_DIGRAPHS = {'sh': 'SH', 'th': 'TH', 'kh': 'CH'}
TOY_CONSONANTS = {'b': ['B'], 'd': ['D'], 's': ['S'], 'h': ['HH'], 't': ['T'], 'n': ['N'], 'x': ['K', 'S']}
TOY_PHONES = sorted({p for pair in TOY_VOWELS.values() for p in pair} | set(TOY_DIGRAPHS.values()) | {'K'}
                    | {p for ps in TOY_CONSONANTS.values() for p in ps})
TOY = dict(words=2000, held_out=400, hidden=64, expand=3, steps=400, batch=64, lr=4e-3, lexicon_seed=1234)


def toy_pronounce(word):
    ''' the rules, left to right: a final `e` behind vowel + consonant is silent and lengthens that vowel; the digraphs sh, th, kh
        give one phone; a doubled consonant gives its phones once; x gives K S; k is S before e or i and K otherwise '''
    n = len(word)
    silent = n >= 3 and word[-1] == 'e' and word[-2] not in TOY_VOWELS and word[-3] in TOY_VOWELS
    phones, i = [], 0
    while i < n:
        c = word[i]
        if silent and i == n - 1:
            break
        if c in TOY_VOWELS:
            phones.append(TOY_VOWELS[c][1 if silent and i == n - 3 else 0])
            i += 1
            continue
        if word[i:i + 2] in TOY_DIGRAPHS:
            phones.append(TOY_DIGRAPHS[word[i:i + 2]])
            i += 2
            continue
        step = 2 if i + 1 < n and word[i + 1] == c else 1            # a doubled consonant
        if c == 'k':
            phones.append('S' if i + step < n and word[i + step] in 'ei' else 'K')
        else:
            phones.extend(TOY_CONSONANTS[c])
        i += step
    return phones


def toy_lexicon(seed=TOY['lexicon_seed'], words=TOY['words']):
    ''' [(spelling, [phones])]: `words` different spellings of 2 to 10 letters, in the order drawn.  With 3 output slots per letter
        every word has a CTC path: a letter gives at most two phones, and those two differ, so labels + equal neighbours <=
        2 n + (n - 1) < 3 n. '''
    rng = np.random.RandomState(seed)
    seen, out = set(), []
    while len(out) < words:
        word = ''.join(TOY_LETTERS[i] for i in rng.randint(0, len(TOY_LETTERS), size=rng.randint(2, 11)))
        if word not in seen:
            seen.add(word)
            out.append((word, toy_pronounce(word)))
    return out


def toy_split(lexicon, held_out=TOY['held_out']):
    ''' (train, held-out): the last `held_out` words drawn are held out '''
    return lexicon[:-held_out], lexicon[-held_out:]


def toy_pack(pairs, phones=TOY_PHONES):
    ''' -> graphemes (N, L) int64, n_graphemes (N,), labels (N, U) int64, n_labels (N,) as torch tensors; ids start at 1 '''
    import torch
    N, L, U = len(pairs), max(len(w) for w, _ in pairs), max(len(p) for _, p in pairs)
    g, lab = torch.zeros(N, L, dtype=torch.long), torch.zeros(N, U, dtype=torch.long)
    for i, (word, pron) in enumerate(pairs):
        g[i, :len(word)] = torch.tensor([GRAPHEMES.index(c) + 1 for c in word])
        lab[i, :len(pron)] = torch.tensor([phones.index(p) + 1 for p in pron])
    return g, torch.tensor([len(w) for w, _ in pairs]), lab, torch.tensor([len(p) for _, p in pairs])


def toy_batches(seed, n_train):
    ''' the word indices of every training step '''
    import torch
    g = torch.Generator().manual_seed(seed)
    return [torch.randperm(n_train, generator=g)[:TOY['batch']].tolist() for _ in range(TOY['steps'])]


def toy_restatement(seed, return_untrained=False):
    ''' trains the restated g2p (the architecture, data and schedule of the learnability test) in float64 on the CPU with
        `F.ctc_loss` and returns the held-out phone error rate of its greedy decode '''
    import torch
    import torch.nn as nn
    import torch.nn.functional as F
    dt = torch.float64
    H, R, P = TOY['hidden'], TOY['expand'], len(TOY_PHONES)

    class Toy(nn.Module):
        def __init__(s):
            super().__init__()
            s.emb = nn.Embedding(len(GRAPHEMES) + 1, H)
            s.c1, s.c2 = nn.Conv1d(H, H, 5, padding=2), nn.Conv1d(H, H, 5, padding=2)
            s.expand, s.out = nn.Linear(H, R * H), nn.Linear(H, P + 1)

        def forward(s, g, n):
            m = (torch.arange(g.shape[1])[None] < n[:, None]).to(dt)[:, None]
            h = torch.relu(s.c1(s.emb(g).transpose(1, 2) * m)) * m
            h = (torch.relu(s.c2(h)) * m).transpose(1, 2)
            y = torch.relu(s.expand(h)).reshape(g.shape[0], g.shape[1] * R, H)
            return s.out(y)

    train, held = toy_split(toy_lexicon())
    g, n, lab, nl = toy_pack(train)
    hg, hn, _, _ = toy_pack(held)

    def rate(model):
        with torch.no_grad():
            logits = model(hg, hn).numpy()
        ids, n_out, _ = greedy(logits, (hn * R).numpy())
        decodes = [[TOY_PHONES[i - 1] for i in ids[b, :n_out[b]]] for b in range(len(held))]
        return phone_error_rate(decodes, [p for _, p in held])

    torch.manual_seed(seed)
    model = Toy().to(dt)
    untrained = rate(model)
    opt = torch.optim.Adam(model.parameters(), lr=TOY['lr'])
    for idx in toy_batches(seed, len(train)):
        idx = torch.tensor(idx)
        L, U = int(n[idx].max()), int(nl[idx].max())
        logp = F.log_softmax(model(g[idx, :L], n[idx]), dim=2).transpose(0, 1)
        loss = F.ctc_loss(logp, lab[idx, :U], n[idx] * R, nl[idx], blank=0, reduction='none').mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
    return (rate(model), untrained) if return_untrained else rate(model)


if __name__ == '__main__':
    import sys
    for seed in range(int(sys.argv[1]) if len(sys.argv) > 1 else 6):
        print(seed, [round(v, 4) for v in toy_restatement(seed, return_untrained=True)], flush=True)
