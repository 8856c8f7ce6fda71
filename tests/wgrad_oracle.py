"""Float64 oracle, case table and host-side restatements for the conv weight-gradient kernels of csrc/conv_wgrad.hip
(ops.conv1d_wgrad / ops.conv1d_wgrad_multi), shared by tests/test_wgrad_host.py and tests/test_gpu_wgrad.py.

The contract, as read from conv_wgrad_kernel (`fetch`) and wgrad_ring_body (`issue_item`), taps in {1, 3}, h = taps // 2:
    dW[co, ci, t] += sum over b and n < nlim_b of dY[b, n, co] * X[b, n + t - h, ci]
    db[co]        += sum over b and n < nlim_b of dY[b, n, co]
    nlim_b = min(N, len_b + 2), or N without a lengths tensor;  X outside [0, N) is zero.
    rows read: dY rows n < nlim_b and X rows n <= min(len_b + 2, N - 1) of every utterance, and NOTHING else -- the staged kernel
    guards its loads with `n < flim` / `n <= flim && n < N`, the ring kernel points every other row at the zero page.
    X row nlim_b (where it is below N) is read: tap 2 of the last contracted row meets it.
    Both operands are rounded to the compute type before they are multiplied (`cvt8<TA, TC>`: a plain `(TC)` cast, round to
    nearest even, torch's `.to(bfloat16)`); products and sums are fp32.
`contract` computes this as one float64 einsum per tap over the contracted rows only, and on request the absolute-value sums
A = sum |dY| |X| and Ab = sum |dY| per element, which size the rounding bound of the Gaussian tests and the exactness headroom of the
integer ones.

Integer draws make the comparison exact: with dY in [-127, 127] and X in [-3, 3] (draw 'dy8'; 'x8' swaps the roles, so that each
operand is met once with all 8 significand bits of bf16 in play) every operand is exact in bf16 and in fp32, and every product and
every partial sum -- whatever its order: an MFMA chain, the reduce kernel's tree, fp32 atomics -- is an integer below 2^24, which fp32
holds exactly.  dW and db start from integers in [-100, 100] (both are accumulated into); tests/test_wgrad_host.py holds
max(A) + 100 < 2^24 for every exact case.  The operands hold NaN in every row the kernels must not read.

The work list (both kernels): utterance b owns cdiv(nlim_b, 64) items of 64 rows; split s of `nsplit` contracts the items
[total * s // nsplit, total * (s + 1) // nsplit) for each of the cdiv(Cout, 128) * cdiv(Cin, 128) tiles.  `nsplit` restates
`wgrad_nsplit`, `items` / `split_items` the list; the host test compares `nsplit` with dx_conv1d_wgrad_ws_floats.

Cases (B, N, lens) and what each reaches (asserted in tests/test_wgrad_host.py):
    W1  4,  130, 130 62 63 0                  one split; nlim 130 (clipped at N, no multiple of 64), 64 (ends on an item), 65 (a one-row
                                              item), 2 (the halo rows of an empty utterance)
    W2  3,  700, 700 433 31                   two splits, the second starts at row 576 of utterance 0 and crosses two utterance ends;
                                              also with every operand a channel slice of a wider tensor (lddy != Cout, ldx != Cin)
    W3  6, 1024, 1024 1000 517 126 64 1       nsplit 6: the reduce kernels' four groups take 2, 2, 2, 0 splits
    W4 16,  512, drawn, lens[0] 512, one 0    nsplit 8: `by_split` with 2, 3 and 8 tiles, index order with 1 tile
    W5  8, 2048, drawn, all <= 62             nsplit 16 over 8 items: half of the workgroups have none
    W6 520,   8, drawn in 0..8                B > DX_SCAN_MAXB: the serial walk; nsplit 32, `by_split`
    W7  4,  512, 512 70 10 0                  the 64-tile weights only: (1024, 1024, 3) with nsplit 2 (the ring kernel's tile
                                              permutation), (1024, 1024, 1) with nsplit 1
    W8  7,    1, none                         N = 1, no lengths tensor
Channel sets (Cin, Cout, taps) per case: CASE_SETS.  Every set of SETS and RAGGED meets W2, every set of SETS meets W4.
"""
import functools
import types

import numpy as np
import torch

F32, BF16 = torch.float32, torch.bfloat16
WG_P, WG_TILE, TILE_FLOATS_PER_TAP = 64, 128, 2 * 16 * 512          # WG_P, WG_CO = WG_CI, TILE_FLOATS / taps of conv_wgrad.hip
SCAN_MAXB = 512                                                      # DX_SCAN_MAXB of dx_common.h
TARGET_K3, TARGET_K1 = 192, 64                                       # DX_WG_TARGET and the k = 1 target of wgrad_nsplit

# kernel family -> (dY storage, X storage, compute type)
FAMILIES = {'f32': (F32, F32, F32), 'cast': (F32, F32, BF16), 'dy32': (F32, BF16, BF16), 'x32': (BF16, F32, BF16), 'ring': (BF16, BF16, BF16)}


def _drawn(seed, lo, hi, n, fixed=()):
    r = np.random.RandomState(seed).randint(lo, hi + 1, n)
    for i, v in fixed:
        r[i] = v
    return tuple(int(v) for v in r)


CASES = {
    'W1': (4, 130, (130, 62, 63, 0)),
    'W2': (3, 700, (700, 433, 31)),
    'W3': (6, 1024, (1024, 1000, 517, 126, 64, 1)),
    'W4': (16, 512, _drawn(4, 1, 512, 16, fixed=((0, 512), (9, 0)))),
    'W5': (8, 2048, _drawn(5, 0, 62, 8)),
    'W6': (520, 8, _drawn(6, 0, 8, 520)),
    'W7': (4, 512, (512, 70, 10, 0)),
    'W8': (7, 1, None),
}
SETS = ((128, 128, 3), (128, 256, 3), (128, 1024, 3), (1024, 128, 3), (128, 384, 1), (128, 128, 1), (384, 128, 1))
RAGGED = ((136, 200, 3), (80, 72, 1))
CASE_SETS = {
    'W1': ((128, 128, 3), (128, 384, 1)) + RAGGED,
    'W2': SETS + RAGGED,
    'W3': ((128, 128, 3), (128, 1024, 3), (128, 384, 1)) + RAGGED,
    'W4': SETS,
    'W5': ((128, 128, 3), (128, 256, 3), (128, 384, 1), (128, 128, 1)),
    'W6': ((128, 256, 3), (128, 128, 3), (128, 128, 1)),
    'W7': ((1024, 1024, 3), (1024, 1024, 1)),
    'W8': ((128, 128, 3), (128, 384, 1)),
}
# the split count every (case, channel set) above must land on (W7: by tap count)
CASE_NSPLIT = {'W1': 1, 'W2': 2, 'W3': 6, 'W4': 8, 'W5': 16, 'W6': 32, 'W7': {3: 2, 1: 1}, 'W8': 1}
EXACT_DRAWS = ('dy8', 'x8')


def cdiv(a, b):
    return -(-a // b)


def tiles(cin, cout):
    return cdiv(cout, WG_TILE) * cdiv(cin, WG_TILE)


def nsplit(B, N, cin, cout, taps):
    ''' wgrad_nsplit of conv_wgrad.hip '''
    ns = (TARGET_K1 if taps == 1 else TARGET_K3) // tiles(cin, cout)
    ns = min(ns, B * cdiv(N, WG_P) // 16)
    if ns >= 8:
        ns = (ns + 3) // 8 * 8
    return max(ns, 1)


def expected_nsplit(case, chset):
    e = CASE_NSPLIT[case]
    return e[chset[2]] if isinstance(e, dict) else e


def by_split(ns, ntiles, ring):
    ''' the split index runs fastest over the workgroups (both kernels; the ring kernel keeps index order for 64 tiles) '''
    return ntiles > 1 and ns % 8 == 0 and not (ring and ntiles == 64)


def nlims(case):
    B, N, lens = CASES[case]
    return [N] * B if lens is None else [min(N, l + 2) for l in lens]


def xlims(case):
    ''' last X row of each utterance that the kernels may read '''
    B, N, lens = CASES[case]
    return [N - 1] * B if lens is None else [min(l + 2, N - 1) for l in lens]


def items(case):
    ''' the flat work list: (utterance, first row) of every 64-row item '''
    return [(b, j * WG_P) for b, nl in enumerate(nlims(case)) for j in range(cdiv(nl, WG_P))]


def split_items(case, ns, s):
    it = items(case)
    return it[len(it) * s // ns:len(it) * (s + 1) // ns]


def reduce_shares(ns):
    ''' splits per group of the reduce kernels: per = (nsplit + 3) >> 2, group g takes [g per, min(nsplit, (g + 1) per)) '''
    per = (ns + 3) >> 2
    return [max(0, min(ns, (g + 1) * per) - g * per) for g in range(4)]


def contract(dy, x, nlim, taps, with_abs=False):
    ''' (dW (Cout, Cin, taps), db (Cout), A, Ab, R) in float64 from dy (B, N, Cout) and x (B, N, Cin): one einsum per tap over the
        contracted rows only; A, Ab = the same sums of absolute values (None without with_abs); R = the number of contracted rows '''
    B, N, Cout = dy.shape
    Cin, h = x.shape[2], taps // 2
    dw = torch.zeros(Cout, Cin, taps, dtype=torch.float64)
    A = torch.zeros_like(dw) if with_abs else None
    for t in range(taps):
        ys, xs = [], []
        for b in range(B):
            lo, hi = max(0, h - t), min(nlim[b], N - t + h)          # 0 <= n + t - h < N
            if hi > lo:
                ys.append(dy[b, lo:hi])
                xs.append(x[b, lo + t - h:hi + t - h])
        if not ys:                                                   # (N = 1: the outer taps meet padding only)
            continue
        Y, X = torch.cat(ys).double(), torch.cat(xs).double()
        dw[:, :, t] = torch.einsum('rc,rd->cd', Y, X)
        if with_abs:
            A[:, :, t] = torch.einsum('rc,rd->cd', Y.abs(), X.abs())
    live = torch.cat([dy[b, :nlim[b]] for b in range(B)]).double()
    return dw, live.sum(0), A, (live.abs().sum(0) if with_abs else None), int(live.shape[0])


def _seed(case, chset, draw):
    return 1000 * int(case[1]) + 100 * ('dy8', 'x8', 'gauss').index(draw) + (SETS + RAGGED + CASE_SETS['W7']).index(chset)


def _poison(case, dy, x):
    for b, (nl, xl) in enumerate(zip(nlims(case), xlims(case))):
        dy[b, nl:] = float('nan')
        x[b, xl + 1:] = float('nan')


@functools.lru_cache(maxsize=6)
def problem(case, chset, draw, compute=F32, with_abs=False):
    ''' operands (fp32 on the host, NaN where the kernels must not read), the initial dW / db and the float64 oracle of one
        (case, channel set, draw); draw 'dy8' | 'x8' (integers, exact) | 'gauss' (unit variance, rounded to `compute` for the oracle).
        Built once for the tests that share it and left unchanged '''
    B, N, lens = CASES[case]
    cin, cout, taps = chset
    g = torch.Generator().manual_seed(_seed(case, chset, draw))
    if draw == 'gauss':
        dy, x = torch.randn(B, N, cout, generator=g), torch.randn(B, N, cin, generator=g)
        init_dw, init_db = torch.zeros(cout, cin, taps), torch.zeros(cout)
    else:
        ints = lambda c, m: torch.randint(-m, m + 1, (B, N, c), generator=g).float()
        dy, x = (ints(cout, 127), ints(cin, 3)) if draw == 'dy8' else (ints(cout, 3), ints(cin, 127))
        init_dw = torch.randint(-100, 101, (cout, cin, taps), generator=g).float()
        init_db = torch.randint(-100, 101, (cout,), generator=g).float()
    _poison(case, dy, x)
    nlim = nlims(case)
    dw, db, A, Ab, R = contract(dy.to(compute), x.to(compute), nlim, taps, with_abs)
    assert bool(torch.isfinite(dw).all()) and bool(torch.isfinite(db).all()), 'the oracle met a poisoned row'
    return types.SimpleNamespace(case=case, chset=chset, draw=draw, B=B, N=N, lens=lens, cin=cin, cout=cout, taps=taps, nlim=nlim, dy=dy, x=x,
                                 init_dw=init_dw, init_db=init_db, dw=dw, db=db, A=A, Ab=Ab, R=R, nsplit=nsplit(B, N, cin, cout, taps),
                                 tiles=tiles(cin, cout))


def set_id(chset):
    return f'{chset[0]}x{chset[1]}k{chset[2]}'
