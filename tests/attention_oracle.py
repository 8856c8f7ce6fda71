"""Plain-torch restatement of the attention core (header comment of dx_attention_fwd) with its closed-form backward, the two
low-precision restatements that size the tolerances of tests/test_gpu_attention.py, and the builder of the test cases.
Test infrastructure: nothing in the package imports this.  Runs on whatever device its inputs live on.

    S = q k^T / sqrt(d), pad keys -> -inf;   P = softmax(S);   P_drop = P * keep * scale;   o = P_drop v;   lse = logsumexp(S)
    dV = P_drop^T dO;   dP = (dO V^T) * keep * scale;   delta = rowsum(dO * o);   dS = P * (dP - delta)
    dQ = dS K / sqrt(d);   dK = dS^T Q / sqrt(d)

`keep, scale` are those of tests/dropout_masks.attn_keep: the mask that the kernels draw, so forward and backward with dropout on
are deterministic.  Pad keys and pad queries are left out by cutting every utterance to its live rows; what comes back is zero
on the other rows.
"""
import functools
import math

import torch

from tests import dropout_masks as DM
from tests.util import fill_end

TENSORS = ('o', 'lse', 'dq', 'dk', 'dv')
SEED = 0x2B5F1C93A7D4E          # 50 bits
CAP = {torch.float32: 2e-5, torch.bfloat16: 8e-2}       # largest 4 * max|restatement - float64| / max|float64| a case may have

# name -> (N, lengths); E = 128.  What each reaches is said in tests/test_gpu_attention.py
CASES = {
    'A': (150, [150, 97, 33]),
    'B': (259, [259, 257, 256, 255, 129, 128, 127, 33, 32, 31, 1, 0]),
    'C': (1024, [1024, 513, 512, 545, 1]),
    'D': (1030, [1030, 515]),
    'E': (300, [300, 252, 3]),
    'F': (70, None),                # 19 lengths drawn in 0..70, see case_lengths
    'G': (300, [300, 129, 64]),
}
HEADS = {'A': (8, 4, 2, 1), 'B': (8, 4, 2, 1), 'E': (8, 4, 2, 1), 'G': (8, 4, 2, 1), 'C': (8, 2), 'D': (8, 2), 'F': (8, 2)}


def case_lengths(name):
    N, lens = CASES[name]
    if lens is None:
        g = torch.Generator().manual_seed(19)
        lens = torch.randint(0, N + 1, (19,), generator=g)
        lens[5] = lens[14] = N
        lens[9], lens[16] = lens[2], lens[3]            # ties
        lens = lens.tolist()
    return N, list(lens)


def make_case(name, H, dtype, E=128):
    ''' (qkv (B, N, 3E), d_o (B, N, E), lengths) of a case in `dtype`, on the CPU.  Rows in [len, fill_end) hold finite random
        values (the kernels may read them and must keep them out of the live rows), rows from fill_end on hold NaN. '''
    N, lens = case_lengths(name)
    B, d = len(lens), E // H
    g = torch.Generator().manual_seed(1000 + ord(name))
    qkv = torch.randn(B, N, 3 * E, generator=g) * 0.7
    d_o = torch.randn(B, N, E, generator=g)
    if name == 'G':
        # scores of utterance 0 grow with the key index: the running maximum moves at every 32-key block
        qkv *= 4.
        u = torch.randn(H, d, generator=g)
        u = (u / u.norm(dim=1, keepdim=True)).reshape(E)
        qkv[0, :, :E] = 6. * u
        qkv[0, :, E:2 * E] = (torch.arange(N, dtype=torch.float32) / N)[:, None] * u
    fe = fill_end(lens, N)
    for b in range(B):
        qkv[b, int(fe[b]):] = float('nan')
        d_o[b, int(fe[b]):] = float('nan')
    return qkv.to(dtype), d_o.to(dtype), torch.tensor(lens, dtype=torch.int64)


@functools.lru_cache(maxsize=4)
def _keep_np(B, H, N, p):
    return DM.attn_keep(SEED, range(B), H, N, p)


def keep_of(B, H, N, p, device='cpu'):
    ''' (keep (B, H, N, N) bool or None, scale) for dropout p under SEED '''
    if p <= 0.:
        return None, 1.
    keep, scale = _keep_np(B, H, N, float(p))
    return torch.from_numpy(keep).to(device), scale


def _heads(t, n, H):
    return t[:n].reshape(n, H, -1).transpose(0, 1)          # (H, n, d)


def forward_one(q, k, v, kp):
    ''' one utterance cut to its live rows: q, k, v (H, n, d), kp = keep * scale (H, n, n) or None -> o (H, n, d), lse (H, n), P '''
    s = (q @ k.transpose(1, 2)) / math.sqrt(q.shape[2])
    lse = torch.logsumexp(s, dim=2)
    P = torch.softmax(s, dim=2)
    return ((P if kp is None else P * kp) @ v), lse, P


def forward(qkv, lengths, H, keep, scale, dtype):
    ''' o (B, N, E) and lse (B, H, N) in `dtype`, zero on pad rows; differentiable '''
    B, N, E3 = qkv.shape
    E = E3 // 3
    o, lse = [], []
    for b in range(B):
        n = int(lengths[b])
        x = qkv[b].to(dtype)
        kp = None if keep is None else keep[b, :, :n, :n].to(dtype) * scale
        ob, lb, _ = forward_one(_heads(x[:, :E], n, H), _heads(x[:, E:2 * E], n, H), _heads(x[:, 2 * E:], n, H), kp)
        o.append(torch.cat([ob.transpose(0, 1).reshape(n, E), ob.new_zeros(N - n, E)]))
        lse.append(torch.cat([lb, lb.new_zeros(H, N - n)], dim=1))
    return torch.stack(o), torch.stack(lse)


def _empty_result(B, N, E, H, dtype, device):
    z = lambda *s: torch.zeros(*s, dtype=dtype, device=device)
    return {'o': z(B, N, E), 'lse': z(B, H, N), 'dq': z(B, N, E), 'dk': z(B, N, E), 'dv': z(B, N, E)}


def reference(qkv, d_o, lengths, H, keep, scale, dtype):
    ''' forward and closed-form backward in `dtype` (torch.float64: THE reference; torch.float32: the restatement that sizes the
        fp32 bounds and lse's).  keep (B, H, N, N) bool or None (p = 0: everything kept, scale 1).  Returns a dict of o, dq, dk,
        dv (B, N, E) and lse (B, H, N), zero outside the live rows. '''
    B, N, E3 = qkv.shape
    E = E3 // 3
    sm = 1. / math.sqrt(E // H)
    R = _empty_result(B, N, E, H, dtype, qkv.device)
    with torch.no_grad():
        for b in range(B):
            n = int(lengths[b])
            if n == 0:
                continue
            x, g = qkv[b].to(dtype), _heads(d_o[b].to(dtype), n, H)
            q, k, v = _heads(x[:, :E], n, H), _heads(x[:, E:2 * E], n, H), _heads(x[:, 2 * E:], n, H)
            kp = None if keep is None else keep[b, :, :n, :n].to(dtype) * scale
            o, lse, P = forward_one(q, k, v, kp)
            dv = (P if kp is None else P * kp).transpose(1, 2) @ g
            dP = g @ v.transpose(1, 2)
            if kp is not None:
                dP = dP * kp
            delta = (g * o).sum(dim=2, keepdim=True)
            dS = P * (dP - delta)
            dq, dk = (dS @ k) * sm, (dS.transpose(1, 2) @ q) * sm
            R['lse'][b, :, :n] = lse
            for name, t in (('o', o), ('dq', dq), ('dk', dk), ('dv', dv)):
                R[name][b, :n] = t.transpose(0, 1).reshape(n, E)
    return R


def emulate_bf16(qkv, d_o, lengths, H, keep, scale):
    ''' the same function with bf16 operands and fp32 arithmetic, rounded to bf16 where the bf16 kernels round: the inputs; P_drop
        as an MFMA operand (forward: exp(S - max) * keep, the normaliser sums the unrounded values and 1 / l and the keep scale are
        applied in fp32 to the output row; backward: P * keep with P rebuilt from lse); dS as an MFMA operand; o as stored, which
        is what delta reads; the stored o / dq / dk / dv.  Returned as float32. '''
    bf = lambda t: t.to(torch.bfloat16).float()
    B, N, E3 = qkv.shape
    E = E3 // 3
    sm = 1. / math.sqrt(E // H)
    R = _empty_result(B, N, E, H, torch.float32, qkv.device)
    for b in range(B):
        n = int(lengths[b])
        if n == 0:
            continue
        x, g = bf(qkv[b]), _heads(bf(d_o[b]), n, H)
        q, k, v = _heads(x[:, :E], n, H), _heads(x[:, E:2 * E], n, H), _heads(x[:, 2 * E:], n, H)
        k01 = None if keep is None else keep[b, :, :n, :n].float()
        s = (q @ k.transpose(1, 2)) * sm
        m = s.max(dim=2, keepdim=True).values
        e = torch.exp(s - m)
        l = e.sum(dim=2, keepdim=True)
        lse = m + torch.log(l)
        o = bf((bf(e if k01 is None else e * k01) @ v) * (scale / l))
        P = torch.exp(s - lse)
        Pd = bf(P if k01 is None else P * k01)
        dv = bf((Pd.transpose(1, 2) @ g) * scale)
        dP = g @ v.transpose(1, 2)
        if k01 is not None:
            dP = dP * k01 * scale
        delta = (g * o).sum(dim=2, keepdim=True)
        dS = bf(P * (dP - delta))
        dq, dk = bf((dS @ k) * sm), bf((dS.transpose(1, 2) @ q) * sm)
        R['lse'][b, :, :n] = lse[:, :, 0]
        for name, t in (('o', o), ('dq', dq), ('dk', dk), ('dv', dv)):
            R[name][b, :n] = t.transpose(0, 1).reshape(n, E)
    return R


def live(t, name, b, n):
    ''' the live rows of utterance b of a result tensor '''
    return t[b, :, :n] if name == 'lse' else t[b, :n]


def restatement_of(name, dtype):
    ''' which restatement sizes the bound of tensor `name` of a kernel with operand type `dtype` '''
    return 'bf16' if (dtype == torch.bfloat16 and name != 'lse') else 'fp32'


def cancellation_floor(qkv, d_o, lengths, H, scale, b, name):
    ''' an utterance of ONE key has P = 1, so dS = dP - delta = dO . v * (keep * scale) - dO . o is zero in exact arithmetic and dq,
        dk are zero with it.  In fp32 the two dot products of d terms are summed in different orders and each is within
        (d - 1) 2^-24 sum|dO_c v_c| keep * scale of the exact value: what is left is at most twice that, times |k| / sqrt(d) for dq and
        |q| / sqrt(d) for dk.  Neither restatement can size this (theirs may cancel exactly); it is added to their bound. '''
    if int(lengths[b]) != 1 or name not in ('dq', 'dk'):
        return 0.
    E = qkv.shape[2] // 3
    d = E // H
    x, g = qkv[b, 0].double(), d_o[b, 0].double()
    terms = (g * x[2 * E:]).abs().reshape(H, d).sum(dim=1) * scale
    other = (x[E:2 * E] if name == 'dq' else x[:E]).abs().reshape(H, d).max(dim=1).values
    return float((2. * (d - 1) * 2. ** -24 * terms * other / math.sqrt(d)).max())


def bound(low, ref, name, b, n):
    ''' 4 * max|restatement - float64| + 1e-6 * max|float64| over the live rows of utterance b; also the first term over the largest
        element (what CAP limits) '''
    r = live(ref[name], name, b, n).double()
    own = float((live(low[name], name, b, n).double() - r).abs().max())
    top = float(r.abs().max())
    return 4. * own + 1e-6 * top, (4. * own / top if top > 0. else 0.)


# ----------------------------------------------------------------------------- mask readout
def readout_inputs(N, lens, H, dtype, pattern, E=128):
    ''' q = 0, so P = 1 / len exactly for a power-of-two length.
        pattern 0 / 1: k = 0, v[j] = e_(j mod d), d_o[i] = e_(i mod d) / e_((i // d) mod d): o[i, c] * len / scale counts the kept keys of
            query i in class c, dv[j, c] * len / scale the kept queries of key j in class c;
        pattern 2: k[j] = e_(j mod d), v = 1, d_o = e_0: dP = 1 everywhere and delta_i = o[i, 0], so dq[i, c] sums keep * scale - delta_i
            over the keys of class c (`decode_dq_counts`) -- the kept keys of query i again, as the dQ kernel draws them '''
    B, d = len(lens), E // H
    idx = torch.arange(N)
    qkv = torch.zeros(B, N, 3, H, d)
    d_o = torch.zeros(B, N, H, d)
    if pattern == 2:
        qkv[:, idx, 1, :, idx % d] = 1.
        qkv[:, :, 2] = 1.
        d_o[:, :, :, 0] = 1.
    else:
        qkv[:, idx, 2, :, idx % d] = 1.
        d_o[:, idx, :, ((idx // d) if pattern == 1 else idx) % d] = 1.
    return qkv.reshape(B, N, 3 * E).to(dtype), d_o.reshape(B, N, E).to(dtype), torch.tensor(lens, dtype=torch.int64)


def readout_counts(keep, lens, H, pattern, E=128):
    ''' the integer counts that readout_inputs (pattern 0 / 1) makes o and dv hold: (B, N, E) int64 each, zero on pad rows '''
    B, _, N, _ = keep.shape
    d = E // H
    idx = torch.arange(N, device=keep.device)
    key_class = torch.nn.functional.one_hot(idx % d, d).double()
    qry_class = torch.nn.functional.one_hot(((idx // d) if pattern == 1 else idx) % d, d).double()
    co, cv = torch.zeros(B, N, H, d, dtype=torch.float64, device=keep.device), torch.zeros(B, N, H, d, dtype=torch.float64, device=keep.device)
    for b, n in enumerate(lens):
        kb = keep[b, :, :n, :n].double()
        co[b, :n] = (kb @ key_class[:n]).transpose(0, 1)
        cv[b, :n] = (kb.transpose(1, 2) @ qry_class[:n]).transpose(0, 1)
    return co.reshape(B, N, E).round().long(), cv.reshape(B, N, E).round().long()


def decode_counts(t, lens, scale):
    ''' o or dv (B, N, E) of a readout run -> float64 counts (zero on pad rows) '''
    out = torch.zeros(t.shape, dtype=torch.float64, device=t.device)
    for b, n in enumerate(lens):
        out[b, :n] = t[b, :n].double() * (n / scale)
    return out


def decode_dq_counts(dq, o, lens, H, scale):
    ''' dq and o (B, N, E) of a pattern 2 readout run -> float64 counts of the kept keys of query i in class c.  delta is read from
        the run's own stored o, as the kernels do; every class has len / d keys (the lengths are multiples of d) '''
    B, N, E = dq.shape
    d = E // H
    out = torch.zeros(B, N, H, d, dtype=torch.float64, device=dq.device)
    for b, n in enumerate(lens):
        assert n % d == 0
        delta = o[b, :n].double().reshape(n, H, d)[:, :, :1]
        out[b, :n] = (dq[b, :n].double().reshape(n, H, d) * (n * math.sqrt(d)) + delta * (n // d)) / scale
    return out.reshape(B, N, E)
