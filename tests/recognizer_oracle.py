"""Oracles of K31 and daft_exprt/recognizer.py, written from the K31 comment of include/daft_exprt_hip.h.

The CTC loss and the greedy decode of K31 are K30's mathematics: their float64 oracle is tests/ctc_oracle.py, imported, not restated.
Here are (1) the edit distance with its counts -- `edit_counts` is the definition as two plain Python loops, `edit_counts_diagonals`
the same recurrence walked along anti-diagonals with NumPy for the sizes at which plain loops take minutes, and `enumerate_alignments`
shares nothing with either: it lists every alignment of two tiny sequences; (2) the ragged batches of the GPU tests; (3) the toy
corpus of the learnability test and the plain-torch float64 CPU restatement of the recogniser on it (`F.ctc_loss`, Adam, greedy
decode): the test takes its ceiling from it, never from the code under test.
"""
import itertools

import numpy as np

from tests import ctc_oracle as C

DIAGONAL, DELETION, INSERTION = 0, 1, 2         # the order of preference among equal costs


# ---- the edit distance -------------------------------------------------------------------------------------------------------------------

def edit_counts(ref, hyp):
    ''' (sub, del, ins, match) of the canonical cheapest alignment: cell (i, 0) is i deletions, (0, j) j insertions, otherwise the
        cheapest of diagonal (match or substitution), deletion (i - 1 -> i), insertion (j - 1 -> j); the first of equal costs '''
    R, H = len(ref), len(hyp)
    prev = [(0, 0, j, 0) for j in range(H + 1)]
    for i in range(1, R + 1):
        row = [(0, i, 0, 0)]
        for j in range(1, H + 1):
            s, d, n, m = prev[j - 1]
            best = (s, d, n, m + 1) if ref[i - 1] == hyp[j - 1] else (s + 1, d, n, m)
            s, d, n, m = prev[j]
            if s + d + 1 + n < sum(best[:3]):
                best = (s, d + 1, n, m)
            s, d, n, m = row[j - 1]
            if s + d + n + 1 < sum(best[:3]):
                best = (s, d, n + 1, m)
            row.append(best)
        prev = row
    return prev[H]


def edit_counts_diagonals(ref, hyp):
    ''' `edit_counts` along the anti-diagonals i + j = s, vectorised over i: for the sequences of thousands of entries '''
    ref, hyp = np.asarray(ref, dtype=np.int64), np.asarray(hyp, dtype=np.int64)
    R, H = len(ref), len(hyp)
    sub = np.zeros((3, R + 1), dtype=np.int64)
    dele, ins = np.zeros_like(sub), np.zeros_like(sub)
    for s in range(R + H + 1):
        cur, p1, p2 = s % 3, (s + 2) % 3, (s + 1) % 3
        lo, hi = max(0, s - H), min(s, R)
        i = np.arange(lo, hi + 1)
        j = s - i
        inner = (i > 0) & (j > 0)
        ii, jj = i[inner], j[inner]
        ns, nd, nn = np.zeros(len(i), dtype=np.int64), np.where(j == 0, i, 0), np.where(i == 0, j, 0)
        if len(ii):
            diff = (ref[ii - 1] != hyp[jj - 1]).astype(np.int64)
            bs, bd, bn = sub[p2, ii - 1] + diff, dele[p2, ii - 1], ins[p2, ii - 1]
            ds, dd, dn = sub[p1, ii - 1], dele[p1, ii - 1] + 1, ins[p1, ii - 1]
            take = ds + dd + dn < bs + bd + bn
            bs, bd, bn = np.where(take, ds, bs), np.where(take, dd, bd), np.where(take, dn, bn)
            xs, xd, xn = sub[p1, ii], dele[p1, ii], ins[p1, ii] + 1
            take = xs + xd + xn < bs + bd + bn
            ns[inner], nd[inner], nn[inner] = np.where(take, xs, bs), np.where(take, xd, bd), np.where(take, xn, bn)
        sub[cur, lo:hi + 1], dele[cur, lo:hi + 1], ins[cur, lo:hi + 1] = ns, nd, nn
    e = (R + H) % 3
    return int(sub[e, R]), int(dele[e, R]), int(ins[e, R]), int(R - sub[e, R] - dele[e, R])


def enumerate_alignments(ref, hyp):
    ''' every alignment of two tiny sequences as (cost, moves from the END backwards, (sub, del, ins, match)).  An alignment is a
        monotone lattice path from (0, 0) to (R, H); nothing is minimised here '''
    R, H = len(ref), len(hyp)
    out = []

    def walk(i, j, moves):
        if i == R and j == H:
            s = sum(1 for m, a, b in moves if m == DIAGONAL and ref[a] != hyp[b])
            k = sum(1 for m, a, b in moves if m == DIAGONAL and ref[a] == hyp[b])
            d, n = sum(1 for m, _, _ in moves if m == DELETION), sum(1 for m, _, _ in moves if m == INSERTION)
            out.append((s + d + n, tuple(m for m, _, _ in reversed(moves)), (s, d, n, k)))
            return
        if i < R and j < H:
            walk(i + 1, j + 1, moves + [(DIAGONAL, i, j)])
        if i < R:
            walk(i + 1, j, moves + [(DELETION, i, j)])
        if j < H:
            walk(i, j + 1, moves + [(INSERTION, i, j)])
    walk(0, 0, [])
    return out


def first_cheapest(ref, hyp):
    ''' the counts of the first cheapest alignment under the stated preference: the cell's choice is the LAST move of the alignment
        that ends in it, so among the cheapest alignments the one whose moves, read from the end backwards, come first with
        diagonal < deletion < insertion.  Returns (cost, counts) '''
    every = enumerate_alignments(ref, hyp)
    cost = min(a[0] for a in every)
    return cost, min((a for a in every if a[0] == cost), key=lambda a: a[1])[2]


def edit_cases(limit):
    ''' [(name, ref, hyp)] of the GPU test: an empty side each and both, equal sequences, nothing in common, the lengths around
        the wave and workgroup sizes and the limit on either side, random ones, and a two-symbol alphabet where ties are the rule '''
    rng = np.random.RandomState(31)
    seq = lambda n, k: rng.randint(1, k + 1, size=n).astype(np.int32)
    cases = [('both empty', seq(0, 5), seq(0, 5)), ('empty ref', seq(0, 5), seq(7, 5)), ('empty hyp', seq(9, 5), seq(0, 5))]
    same = seq(70, 40)
    cases += [('equal', same, same.copy()), ('nothing in common', seq(65, 20), seq(63, 20) + 20)]
    for n in (1, 63, 64, 65, 255, 256):
        cases += [(f'ref {n}', seq(n, 12), seq(max(1, n - 3), 12)), (f'hyp {n}', seq(max(1, n // 2), 12), seq(n, 12))]
    base = seq(200, 30)
    noisy = np.delete(base, rng.choice(200, 15, replace=False))
    noisy[rng.choice(len(noisy), 20, replace=False)] = 31
    cases += [('a noisy copy', base, np.insert(noisy, 40, [7, 7, 7]))]
    cases += [('two symbols 257 x 300', seq(257, 2), seq(300, 2)), ('two symbols 64 x 64', seq(64, 2), seq(64, 2))]
    cases += [(f'limit x 1', seq(limit, 3), seq(1, 3)), ('1 x limit', seq(1, 3), seq(limit, 3)),
              ('limit x limit, two symbols', seq(limit, 2), seq(limit, 2))]
    return cases


# ---- the ragged batches of the CTC tests ------------------------------------------------------------------------------------------------

EXACT = -1      # n_steps = labels + adjacent equal pairs: a single path
# (n_steps, n_labels).  SHORT holds the lane edges of K = 1, 2 (S = 63 / 65 at 31 / 32 labels, 127 / 129 at 63 / 64) and the steps around
# K30's limit; its last three rows are the statuses 1 (two equal labels, two steps), 2 (no step) and 3 (a label out of range).
# LONG holds the edges of K = 4, 8 (S = 255 / 257 at 127 / 128 labels, 383 at 191) and both limits together.
SHORT = ((1, 0), (1, 1), (2, 1), (EXACT, 31), (255, 32), (256, 63), (257, 64), (2, 2), (0, 3), (9, 4))
SHORT_STATUS = (0, 0, 0, 0, 0, 0, 0, 1, 2, 3)
LONG = ((EXACT, 127), (600, 128), (700, 191), (2048, 255))
CLASSES = (2, 65, 128)


def uctc_case(V, which, seed=0):
    ''' a ragged batch over V classes in the layout of `ctc_oracle.gpu_case`: logits 2 x standard normal, labels that repeat their
        neighbour 3 times in 10 (always in the status-1 row), w in [0.5, 2]; the status-3 row carries a label V '''
    shapes = SHORT if which == 'short' else LONG
    rng = np.random.RandomState(7000 * seed + 10 * V + (which == 'long'))
    B, U = len(shapes), max(s[1] for s in shapes)
    labels = np.zeros((B, U), dtype=np.int64)
    n_steps = np.zeros((B,), dtype=np.int64)
    for b, (nT, nL) in enumerate(shapes):
        for u in range(nL):
            again = u > 0 and (rng.uniform() < 0.3 or (nT, nL) == (2, 2))
            labels[b, u] = labels[b, u - 1] if again else rng.randint(1, V)
        n_steps[b] = nL + C.repeats_of(labels[b, :nL].tolist()) if nT == EXACT else nT
    status = np.array(SHORT_STATUS if which == 'short' else (0,) * B, dtype=np.int32)
    if which == 'short':
        labels[9, 2] = V
    T = int(n_steps.max())
    logits = (2.0 * rng.standard_normal((B, T, V))).astype(np.float32)
    return dict(V=V, B=B, T=T, U=U, logits=logits, labels=labels, n_steps=n_steps, n_labels=np.array([s[1] for s in shapes], dtype=np.int64),
                w=rng.uniform(0.5, 2.0, size=B).astype(np.float32), status=status)


GREEDY_STEPS = (0, 1, 257, 2048)


def greedy_case(V, seed=5):
    ''' logits on a grid of multiples of 1/8 drawn from few values, so ties abound '''
    rng = np.random.RandomState(seed + V)
    B, T = len(GREEDY_STEPS), max(GREEDY_STEPS)
    x = (rng.randint(0, 4, size=(B, T, V)) * rng.choice([0.125, 0.5, 1.0], size=(B, T, 1))).astype(np.float32)
    return x, np.array(GREEDY_STEPS, dtype=np.int64)


# ---- the toy corpus: fixed random templates plus noise, and the restated recogniser --------------------------------------------------------

TOY = dict(classes=15, n_mel=16, utterances=200, held_out=40, noise=0.3, hidden=64, layers=2, stride=2, steps=400, batch=32, lr=3e-3,
           corpus_seed=4321)
TOY_SYMBOLS = ['_', '~', ' ', ','] + [f'P{i:02d}' for i in range(1, TOY['classes'] + 1)]      # a symbol table: the phones are P01 .. P15
TOY_FIRST = 4                                                                                 # the symbol id of P01


def toy_templates():
    import torch
    g = torch.Generator().manual_seed(TOY['corpus_seed'])
    return torch.randn(TOY['classes'] + 1, TOY['n_mel'], generator=g, dtype=torch.float64)    # row c: class c (row 0 unused)


def toy_fabricate(classes, durations, noise):
    ''' the mel (T, n_mel) float64 of a class sequence: each frame its class's template plus the given noise frames (T, n_mel) '''
    import torch
    frames = torch.repeat_interleave(torch.as_tensor(classes), torch.as_tensor(durations))
    return toy_templates()[frames] + noise[:len(frames)]


def toy_corpus(seed=TOY['corpus_seed']):
    ''' [(classes (L,) int64 in 1 .. 15, durations (L,) int64 in 2 .. 7, noise (T, n_mel) float64)]: 200 utterances of 4 to 12
        phones without immediate repeats; the mel is `toy_fabricate(classes, durations, noise)`.  With 2 frames per phone at least
        and 2 frames per step every utterance has a CTC path.  The last 40 are held out. '''
    import torch
    g = torch.Generator().manual_seed(seed + 1)
    utts = []
    for _ in range(TOY['utterances']):
        L = int(torch.randint(4, 13, (1,), generator=g))
        cls = []
        while len(cls) < L:
            c = int(torch.randint(1, TOY['classes'] + 1, (1,), generator=g))
            if not cls or cls[-1] != c:
                cls.append(c)
        dur = torch.randint(2, 8, (L,), generator=g)
        noise = TOY['noise'] * torch.randn(int(dur.sum()), TOY['n_mel'], generator=g, dtype=torch.float64)
        utts.append((torch.tensor(cls), dur, noise))
    return utts


def toy_split(utts):
    return utts[:-TOY['held_out']], utts[-TOY['held_out']:]


def toy_collate(utts, dtype):
    ''' -> symbols (B, L) int64 (symbol ids of TOY_SYMBOLS, 0 pads), n_sym (B,), mel (B, n_mel, T), n_frames (B,) '''
    import torch
    mels = [toy_fabricate(u[0], u[1], u[2]) for u in utts]
    B, L, T = len(utts), max(len(u[0]) for u in utts), max(m.shape[0] for m in mels)
    sym, mel = torch.zeros(B, L, dtype=torch.long), torch.zeros(B, TOY['n_mel'], T, dtype=dtype)
    for b, (u, m) in enumerate(zip(utts, mels)):
        sym[b, :len(u[0])] = u[0] + (TOY_FIRST - 1)
        mel[b, :, :m.shape[0]] = m.T.to(dtype)
    return sym, torch.tensor([len(u[0]) for u in utts]), mel, torch.tensor([m.shape[0] for m in mels])


def toy_batches(seed, n_train):
    ''' the utterance indices of every training step '''
    import torch
    g = torch.Generator().manual_seed(seed)
    return [torch.randperm(n_train, generator=g)[:TOY['batch']].tolist() for _ in range(TOY['steps'])]


def toy_edits(held, kind, seed=99):
    ''' the held-out utterances with ONE phone deleted (kind 'delete': its frames and noise go too) or replaced by another class
        (kind 'replace': the frames keep their noise), at a position and with a class that leave no two equal neighbours.  Every
        utterance is edited once: len(held) edits.  The text they are scored against is the unedited one. '''
    import torch
    rng = np.random.RandomState(seed)
    out = []
    for cls, dur, noise in held:
        cls_l, L = cls.tolist(), len(cls)
        while True:
            p = int(rng.randint(0, L))
            left, right = (cls_l[p - 1] if p > 0 else 0), (cls_l[p + 1] if p + 1 < L else 0)
            if kind == 'delete':
                if left != right or left == 0:
                    break
            else:
                c = int(rng.randint(1, TOY['classes'] + 1))
                if c not in (left, right, cls_l[p]):
                    break
        if kind == 'delete':
            start = int(dur[:p].sum())
            keep = torch.ones(L, dtype=torch.bool)
            keep[p] = False
            out.append((cls[keep], dur[keep], torch.cat([noise[:start], noise[start + int(dur[p]):]])))
        else:
            new = cls.clone()
            new[p] = c
            out.append((new, dur, noise))
    return out


def toy_restatement(seed, return_untrained=False):
    ''' trains the restated recogniser (the architecture, data and schedule of the learnability test) in float64 on the CPU with
        `F.ctc_loss(reduction='mean')` and returns the held-out phone error rate of its greedy decode '''
    import torch
    import torch.nn as nn
    import torch.nn.functional as F
    dt = torch.float64
    Hd, R, M, V = TOY['hidden'], TOY['stride'], TOY['n_mel'], TOY['classes'] + 1

    class Toy(nn.Module):
        def __init__(s):
            super().__init__()
            s.c1, s.c2 = nn.Conv1d(M * R, Hd, 3, padding=1), nn.Conv1d(Hd, Hd, 3, padding=1)
            s.out = nn.Linear(Hd, V)

        def forward(s, mel, n):
            T = mel.shape[2]
            live = (torch.arange(T)[None] < n[:, None]).to(dt)[:, None]
            cnt = n.to(dt)[:, None, None]
            mean = (mel * live).sum(2, keepdim=True) / cnt
            cen = (mel - mean) * live
            x = cen * torch.rsqrt((cen * cen).sum(2, keepdim=True) / cnt + 1e-5)
            Ts = (T + R - 1) // R
            x = F.pad(x, (0, Ts * R - T)).transpose(1, 2).reshape(mel.shape[0], Ts, R * M).transpose(1, 2)
            ns = (n + R - 1) // R
            m = (torch.arange(Ts)[None] < ns[:, None]).to(dt)[:, None]
            h = torch.relu(s.c2(torch.relu(s.c1(x * m)) * m))
            return s.out(h.transpose(1, 2)), ns

    train, held = toy_split(toy_corpus())
    hsym, hnl, hmel, hnt = toy_collate(held, dt)

    def rate(model):
        with torch.no_grad():
            logits, ns = model(hmel, hnt)
        ids, n_out, _ = C.greedy(logits.numpy(), ns.numpy())
        return C.phone_error_rate([ids[b, :n_out[b]].tolist() for b in range(len(held))], [u[0].tolist() for u in held])

    torch.manual_seed(seed)
    model = Toy().to(dt)
    untrained = rate(model)
    opt = torch.optim.Adam(model.parameters(), lr=TOY['lr'])
    for idx in toy_batches(seed, len(train)):
        sym, nl, mel, nt = toy_collate([train[i] for i in idx], dt)
        logits, ns = model(mel, nt)
        labels = torch.where(sym > 0, sym - (TOY_FIRST - 1), torch.zeros_like(sym))
        loss = F.ctc_loss(F.log_softmax(logits, dim=2).transpose(0, 1), labels, ns, nl, blank=0, reduction='mean')
        opt.zero_grad()
        loss.backward()
        opt.step()
    return (rate(model), untrained) if return_untrained else rate(model)


if __name__ == '__main__':
    import sys
    for seed in range(int(sys.argv[1]) if len(sys.argv) > 1 else 6):
        print(seed, [round(v, 4) for v in toy_restatement(seed, return_untrained=True)], flush=True)
