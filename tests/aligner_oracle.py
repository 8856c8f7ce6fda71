"""NumPy restatement of the five contracts of K28 (include/daft_exprt_hip.h: dx_aln_*), written from the header text alone.

Every function takes `dtype`: np.float64 is the oracle; np.float32 is the same recurrences in the same order in the kernels'
precision, which the GPU tests use to learn what rounding alone does (their tolerance is 2 x the deviation of the float32
restatement from the float64 one on the same inputs).  Loops over the batch and over time are plain Python: the shapes of the
tests are small.

The second half is the plain-torch float64 CPU restatement of the whole learned aligner on a toy corpus (encoders, soft
alignment, forward-sum loss, Adam, MAS): the learnability test takes its floor from it, never from the code under test.
"""
import numpy as np


def status_of(n_frm, n_sym):
    ''' 2: an empty axis; 1: fewer frames than symbols; 0 otherwise (2 is decided first) '''
    return 2 if n_frm <= 0 or n_sym <= 0 else 1 if n_frm < n_sym else 0


def prior(n_frm, n_sym, prior_sigma, dtype=np.float64):
    t = ((np.arange(n_frm, dtype=dtype) + dtype(0.5)) / dtype(n_frm))[:, None]
    l = ((np.arange(n_sym, dtype=dtype) + dtype(0.5)) / dtype(n_sym))[None, :]
    if prior_sigma <= 0:
        return np.zeros((n_frm, n_sym), dtype=dtype)
    d = l - t
    return -(d * d) / dtype(2.0 * float(prior_sigma) ** 2)


def _logsumexp(x, axis, dtype):
    m = x.max(axis=axis, keepdims=True)
    return (m + np.log(np.exp(x - m).sum(axis=axis, keepdims=True, dtype=dtype))).astype(dtype)


def logprob_fwd(q, k, n_frm, n_sym, temperature, prior_sigma, dtype=np.float64):
    ''' q (B, T, A), k (B, L, A) -> logp (B, T, L); dead cells 0 '''
    q, k = np.asarray(q, dtype=dtype), np.asarray(k, dtype=dtype)
    B, T, A = q.shape
    L = k.shape[1]
    out = np.zeros((B, T, L), dtype=dtype)
    for b in range(B):
        nf, ns = int(n_frm[b]), int(n_sym[b])
        if nf <= 0 or ns <= 0:
            continue
        d = np.zeros((nf, ns), dtype=dtype)
        for a in range(A):                                       # the channels in order
            diff = q[b, :nf, a][:, None] - k[b, :ns, a][None, :]
            d = d + diff * diff
        s = dtype(-float(temperature)) * d + prior(nf, ns, prior_sigma, dtype)
        out[b, :nf, :ns] = s - _logsumexp(s, 1, dtype)
    return out


def _sum_in_order(x, axis, dtype):
    ''' x_0 + x_1 + ... along `axis`, one term after the other as the kernels add them (np.sum adds pairwise) '''
    return np.take(np.cumsum(x, axis=axis, dtype=dtype), -1, axis=axis)


def logprob_bwd(q, k, logp, g, n_frm, n_sym, temperature, dtype=np.float64):
    ''' -> dq (B, T, A), dk (B, L, A); dead rows 0.  The sums over l (dq) and over t (dk) run in order. '''
    q, k, logp, g = (np.asarray(x, dtype=dtype) for x in (q, k, logp, g))
    B, T, A = q.shape
    L = k.shape[1]
    dq, dk = np.zeros((B, T, A), dtype=dtype), np.zeros((B, L, A), dtype=dtype)
    two_tau = dtype(2.0 * float(temperature))
    for b in range(B):
        nf, ns = int(n_frm[b]), int(n_sym[b])
        if nf <= 0 or ns <= 0:
            continue
        gg, lp = g[b, :nf, :ns], logp[b, :nf, :ns]
        ds = gg - np.exp(lp) * gg.sum(axis=1, keepdims=True, dtype=dtype)
        for a in range(A):
            diff = q[b, :nf, a][:, None] - k[b, :ns, a][None, :]
            dq[b, :nf, a] = -two_tau * _sum_in_order(ds * diff, 1, dtype)
            dk[b, :ns, a] = two_tau * _sum_in_order(ds * diff, 0, dtype)
    return dq, dk


def logaddexp(a, b, dtype=np.float64):
    ''' log(exp(a) + exp(b)); -inf for two -inf, never NaN '''
    a, b = np.asarray(a, dtype=dtype), np.asarray(b, dtype=dtype)
    m, n = np.maximum(a, b), np.minimum(a, b)
    with np.errstate(invalid='ignore', over='ignore'):
        d = np.where(np.isneginf(m), dtype(0), n - m)
        r = m + np.log1p(np.exp(d))
    return np.where(np.isneginf(m), dtype(-np.inf), r).astype(dtype)


def _shift_right(v, dtype):
    return np.concatenate([np.array([-np.inf], dtype=dtype), v[:-1]])


def forward_sum(logp, n_frm, n_sym, dtype=np.float64):
    ''' -> alpha (B, T, L), loss (B,), status (B,) int32 '''
    logp = np.asarray(logp, dtype=dtype)
    B, T, L = logp.shape
    alpha, loss, status = np.zeros((B, T, L), dtype=dtype), np.full((B,), np.nan, dtype=dtype), np.zeros((B,), dtype=np.int32)
    for b in range(B):
        nf, ns = int(n_frm[b]), int(n_sym[b])
        status[b] = status_of(nf, ns)
        if status[b] != 0:
            continue
        a = np.full((ns,), -np.inf, dtype=dtype)
        a[0] = logp[b, 0, 0]
        alpha[b, 0, :ns] = a
        for t in range(1, nf):
            a = (logp[b, t, :ns] + logaddexp(a, _shift_right(a, dtype), dtype)).astype(dtype)
            alpha[b, t, :ns] = a
        loss[b] = -a[ns - 1]
    return alpha, loss, status


def forward_sum_bwd(logp, alpha, w, n_frm, n_sym, dtype=np.float64, return_gamma=False):
    ''' -> dlogp (B, T, L) = -w[b] * gamma; rows with status != 0 and dead cells 0 '''
    logp, alpha, w = np.asarray(logp, dtype=dtype), np.asarray(alpha, dtype=dtype), np.asarray(w, dtype=dtype)
    B, T, L = logp.shape
    gamma = np.zeros((B, T, L), dtype=dtype)
    for b in range(B):
        nf, ns = int(n_frm[b]), int(n_sym[b])
        if status_of(nf, ns) != 0:
            continue
        end = alpha[b, nf - 1, ns - 1]
        beta = np.full((ns,), -np.inf, dtype=dtype)
        beta[ns - 1] = 0
        with np.errstate(invalid='ignore'):
            gamma[b, nf - 1, :ns] = np.exp(alpha[b, nf - 1, :ns] + beta - end)
            for t in range(nf - 2, -1, -1):
                c = (logp[b, t + 1, :ns] + beta).astype(dtype)
                beta = logaddexp(c, np.concatenate([c[1:], np.array([-np.inf], dtype=dtype)]), dtype)
                gamma[b, t, :ns] = np.exp(alpha[b, t, :ns] + beta - end)
    gamma = np.where(np.isnan(gamma), 0, gamma).astype(dtype)
    if return_gamma:
        return gamma
    dlogp = -w[:, None, None] * gamma
    return np.where(gamma == 0, dtype(0), dlogp).astype(dtype)


def mas(logp, n_frm, n_sym, dtype=np.float64):
    ''' -> path (B, T + L - 1, 2) int32, path_len (B,) int32, score (B,), status (B,) int32 '''
    logp = np.asarray(logp, dtype=dtype)
    B, T, L = logp.shape
    path = np.full((B, T + L - 1, 2), -1, dtype=np.int32)
    path_len, status = np.zeros((B,), dtype=np.int32), np.zeros((B,), dtype=np.int32)
    score = np.full((B,), np.nan, dtype=dtype)
    for b in range(B):
        nf, ns = int(n_frm[b]), int(n_sym[b])
        status[b] = status_of(nf, ns)
        if status[b] != 0:
            continue
        V = np.full((ns,), -np.inf, dtype=dtype)
        V[0] = logp[b, 0, 0]
        adv = np.zeros((nf, ns), dtype=bool)
        for t in range(1, nf):
            left = _shift_right(V, dtype)
            adv[t] = left > V                                    # (t-1, l-1) only when strictly greater
            V = (logp[b, t, :ns] + np.maximum(V, left)).astype(dtype)
        score[b] = V[ns - 1]
        l = ns - 1
        for t in range(nf - 1, -1, -1):
            path[b, t] = (t, l)
            if t > 0 and l > 0 and (t == l or adv[t, l]):        # forced at l = 0 (stay) and at t = l (step)
                l -= 1
        path_len[b] = nf
    return path, path_len, score, status


def durations_of_path(path, path_len, n_sym, L):
    ''' frames per symbol along a path of `mas`: (B, L) int64 '''
    B = path.shape[0]
    out = np.zeros((B, L), dtype=np.int64)
    for b in range(B):
        if path_len[b] > 0:
            out[b, :int(n_sym[b])] = np.bincount(path[b, :int(path_len[b]), 1], minlength=int(n_sym[b]))
    return out


def monotone_paths(T, L):
    ''' every l(0) = 0 <= ... <= l(T - 1) = L - 1 with steps of 0 or 1: lists of T symbol indices '''
    paths = []

    def walk(prefix):
        if len(prefix) == T:
            if prefix[-1] == L - 1:
                paths.append(list(prefix))
            return
        for step in (0, 1):
            if prefix[-1] + step < L:
                walk(prefix + [prefix[-1] + step])
    if T >= 1 and L >= 1:
        walk([0])
    return paths


# ---- the whole aligner on a toy corpus, plain torch float64 on the CPU ---------------------------------------------------------------

TOY = dict(utterances=64, symbols=15, n_mel=80, noise=0.5, hidden=64, att_dim=32, temperature=0.05, prior_sigma=0.2, steps=150,
           lr=4e-3, batch=32, corpus_seed=1234)
NEG = -1e30


def toy_corpus(seed=TOY['corpus_seed']):
    ''' [(symbols (L,) int64 in 1 .. 15, durations (L,) int64 in 2 .. 7, mel (T, 80) float64)]: 64 utterances of 4 to 12
        symbols without immediate repeats, each frame its symbol's fixed random template plus 0.5 x Gaussian noise; id 0 pads '''
    import torch
    g = torch.Generator().manual_seed(seed)
    S = TOY['symbols'] + 1
    tmpl = torch.randn(S, TOY['n_mel'], generator=g, dtype=torch.float64)
    tmpl[0] = 0
    utts = []
    for _ in range(TOY['utterances']):
        L = int(torch.randint(4, 13, (1,), generator=g))
        sym = []
        while len(sym) < L:
            s = int(torch.randint(1, S, (1,), generator=g))
            if not sym or sym[-1] != s:
                sym.append(s)
        dur = torch.randint(2, 8, (L,), generator=g)
        frames = torch.repeat_interleave(torch.tensor(sym), dur)
        mel = tmpl[frames] + TOY['noise'] * torch.randn(len(frames), TOY['n_mel'], generator=g, dtype=torch.float64)
        utts.append((torch.tensor(sym), dur, mel))
    return utts


def toy_collate(utts, dtype):
    import torch
    B, L, T = len(utts), max(len(u[0]) for u in utts), max(u[2].shape[0] for u in utts)
    sym, mel = torch.zeros(B, L, dtype=torch.long), torch.zeros(B, T, TOY['n_mel'], dtype=dtype)
    nl, nt = torch.tensor([len(u[0]) for u in utts]), torch.tensor([u[2].shape[0] for u in utts])
    for b, u in enumerate(utts):
        sym[b, :len(u[0])] = u[0]
        mel[b, :u[2].shape[0]] = u[2].to(dtype)
    return sym, nl, mel, nt


def toy_batches(seed):
    ''' the utterance indices of every training step '''
    import torch
    g = torch.Generator().manual_seed(seed)
    return [torch.randperm(TOY['utterances'], generator=g)[:TOY['batch']].tolist() for _ in range(TOY['steps'])]


def frames_correct(utts, labels):
    ''' share of frames whose label (index into the utterance's symbols) is the true one '''
    import torch
    ok = tot = 0
    for u, p in zip(utts, labels):
        truth = torch.repeat_interleave(torch.arange(len(u[0])), u[1])
        ok += int((truth == torch.as_tensor(p)).sum())
        tot += len(truth)
    return ok / tot


def toy_restatement(seed):
    ''' trains the restated aligner (same architecture, data and schedule as the learnability test) in float64 on the CPU and
        returns the share of frames MAS (prior off) gives their true symbol '''
    import torch
    import torch.nn as nn
    dt = torch.float64

    class Toy(nn.Module):
        def __init__(s):
            super().__init__()
            H, A = TOY['hidden'], TOY['att_dim']
            s.emb = nn.Embedding(TOY['symbols'] + 1, H)
            s.k1, s.k2 = nn.Conv1d(H, H, 3, padding=1), nn.Conv1d(H, A, 1)
            s.q1, s.q2, s.q3 = nn.Conv1d(TOY['n_mel'], H, 3, padding=1), nn.Conv1d(H, H, 3, padding=1), nn.Conv1d(H, A, 1)

        def forward(s, sym, nl, mel, nt):
            ml = (torch.arange(sym.shape[1])[None] < nl[:, None]).to(dt)[:, None]
            mt = (torch.arange(mel.shape[1])[None] < nt[:, None]).to(dt)[:, None]
            k = s.k2(torch.relu(s.k1(s.emb(sym).transpose(1, 2) * ml)) * ml).transpose(1, 2)
            q = s.q3(torch.relu(s.q2(torch.relu(s.q1(mel.transpose(1, 2) * mt)) * mt)) * mt).transpose(1, 2)
            return q, k

    def logprob(q, k, nt, nl, sigma):
        s = -TOY['temperature'] * ((q[:, :, None, :] - k[:, None, :, :]) ** 2).sum(-1)
        if sigma > 0:
            ft = (torch.arange(s.shape[1])[None, :, None] + .5) / nt[:, None, None]
            fl = (torch.arange(s.shape[2])[None, None, :] + .5) / nl[:, None, None]
            s = s - (fl - ft) ** 2 / (2 * sigma ** 2)
        s = s.masked_fill(torch.arange(s.shape[2])[None, None, :] >= nl[:, None, None], NEG)
        return torch.log_softmax(s, dim=2)

    def fsum(logp, nt, nl):
        B, T, L = logp.shape
        a = torch.full((B, L), NEG, dtype=dt)
        a[:, 0] = logp[:, 0, 0]
        outs = [a]
        for t in range(1, T):
            a = logp[:, t] + torch.logaddexp(a, torch.cat([torch.full((B, 1), NEG, dtype=dt), a[:, :-1]], 1))
            outs.append(a)
        return -torch.stack(outs, 1)[torch.arange(B), nt - 1, nl - 1]

    utts = toy_corpus()
    torch.manual_seed(seed)
    model = Toy().to(dt)
    opt = torch.optim.Adam(model.parameters(), lr=TOY['lr'])
    for idx in toy_batches(seed):
        sym, nl, mel, nt = toy_collate([utts[i] for i in idx], dt)
        q, k = model(sym, nl, mel, nt)
        loss = (fsum(logprob(q, k, nt, nl, TOY['prior_sigma']), nt, nl) / nt).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
    with torch.no_grad():
        sym, nl, mel, nt = toy_collate(utts, dt)
        q, k = model(sym, nl, mel, nt)
        logp = logprob(q, k, nt, nl, 0.).numpy()
    path, path_len, _, _ = mas(logp, nt.numpy(), nl.numpy())
    return frames_correct(utts, [path[b, :path_len[b], 1] for b in range(len(utts))])


if __name__ == '__main__':
    import sys
    for seed in range(int(sys.argv[1]) if len(sys.argv) > 1 else 5):
        print(seed, round(toy_restatement(seed), 4), flush=True)
