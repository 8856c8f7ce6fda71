"""Plain-torch restatement of the LayerNorm-fused conv GEMMs (dx_conv1d_ln / dx_conv1d_ln_vres and dx_conv1d_lnbwd of
include/daft_exprt_hip.h), the low-precision restatement that sizes the tolerances of tests/test_gpu_conv_ln.py, a Python restatement
of the tile plan (csrc/conv_plan.hip: conv_plan_body), the builder of the test cases and the inputs of the mask readout.  Test
infrastructure: nothing in the package imports this.  Everything runs on the CPU.

    conv = bias + sum_{tap, ci} x[n + tap - taps / 2, ci] * w[co, ci, tap]            (rows outside [0, N) are zero padding)
    s    = keep_pre * scale * conv + residual          residual_ln: residual = (s1 - mean1) * rstd1 * gamma1 + beta1, 0 on n >= len
    mean = sum_c s / 128;   rstd = 1 / sqrt(sum_c (s - mean)^2 / 128 + 1e-5);   xh = (s - mean) * rstd
    y    = film_gamma[b] * (xh * gamma + beta) + film_beta[b],  0 on n >= len;    y_lp = y
    y2   = bf16(y_lp) . w2^T + b2,  0 on n >= len                                   (split-K path)

    gy   = conv(x, w) + y_inout,  0 on n >= len         (w = the transposed, tap-flipped weight of the forward conv 128 -> Cin)
    dfilm[b] += [sum_n gy * (xh * gamma + beta) | sum_n gy];   gl = gy * film_gamma[b]
    dgamma += sum_bn gl * xh;   dbeta += sum_bn gl;   gx = gl * gamma
    ds   = rstd * (gx - mean_c(gx) - xh * mean_c(gx * xh))         (written in place of y_inout)
    dx_lp = keep_pre * scale * ds;    y2 = bf16(dx_lp) . w2^T      (split-K path)

`keep, scale` are tests/dropout_masks.elem_keep of stream 0 over (B, N, 128): the mask both epilogues draw.

ROW CONTRACT, read from csrc/conv_gemm_kernel.h and csrc/conv_sk.hip.  fe = tests.util.fill_end(len, N) (dx_fill_end):
  * y, y_lp, y2, ds, dx_lp and the backward y2 are exact zeros on every row of [len, fe) on every path;
  * rows at or past fe are unspecified (never written: the fixed-tile early-out returns, the padding fill stops at fe);
  * s, mean, rstd on rows >= len differ by path (`computed_rows`):
      plan paths (SPLITK, PLAN_K3, PLAN_K1): the tiles of the plan end at len (halo 0), the padding fill writes exact zeros on [len, fe);
      fixed tiles (ROWS64 / ROWS128, BM = 64 / 128 rows): a tile that starts below len + 2 is live and computes ALL its rows from
      the inputs it finds there, so s, mean, rstd are the formula above up to the end of the tile that holds row len + 1
      (`live_end`, never past fe), and exact zeros from there to fe (the early-out's zero fill);
  * inputs: x, residual, s_in, mean, rstd, y_inout hold values on [0, len + 2), zeros on [len + 2, fe) -- what the producers upstream
    leave there -- and NaN at and past fe: no kernel reads past the fill end (csrc/dx_common.h), so every contract row and every
    per-channel sum stays finite.

The RESTATEMENT is the same computation in fp32 with bf16 rounding exactly where the kernels store bf16 (y_lp, dx_lp, y2) and where
they round an operand: fp32 x in front of bf16 weights is rounded to bf16 when it is staged for the MFMA.  Its contraction is
accumulated as an MFMA chain: one fp32 add per (tap, K-step) partial product in order, K-step = 16 input channels for bf16 weights
(v_mfma_f32_32x32x16_bf16) and 2 for fp32 weights (v_mfma_f32_32x32x2_f32) -- not a blocked GEMM.  The split-K path adds 2 or 4 such
chains; that order is not matched.
"""
import functools
import types

import torch
import torch.nn.functional as F

from tests import dropout_masks as DM
from tests import layernorm_oracle as L
from tests.util import fill_end

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
SEED_PRE = L.SEED_PRE
M63 = L.M63
SPLITK, PLAN_K3, PLAN_K1, ROWS128, ROWS64 = range(5)          # DX_LN_PATH_* of include/daft_exprt_hip.h
PATH_NAME = {SPLITK: 'splitk', PLAN_K3: 'plan_k3', PLAN_K1: 'plan_k1', ROWS128: 'rows128', ROWS64: 'rows64'}
FWD_TENSORS = ('y', 'y_lp', 's', 'mean', 'rstd', 'y2')
BWD_TENSORS = ('ds', 'dx_lp', 'y2b', 'dgamma', 'dbeta', 'dfilm')
BF16_STORED = ('y_lp', 'y2', 'dx_lp', 'y2b')
# largest max|restatement - float64| / max|float64| an utterance's tensor may have (tests/test_conv_ln_host.py measures it over every
# configuration below).  Measured worst: fp32-stored tensors of the bf16 / bf16 and fp32 / fp32 operand pairs 1.2e-6 (F1, Cin 1024, fp32:
# a chain of 1536 fp32 adds); of fp32 x in front of bf16 weights 2.7e-3 (x is rounded to bf16 when staged, 2^-9 per operand, and ds
# subtracts its row means); a bf16-rounded output 3.9e-3 (half an ulp of bf16, 2^-8, when the largest element sits just above a power of two)
CAP = {'fp32': 2.4e-6, 'mixed': 5.5e-3, 'bf16': 7.8e-3}

# name -> (B, N, lengths, tiles of the plan: a count, None = the default plan, 'fixed' = no plan, offset of the residual rows)
CASES = {
    'T1': (4, 128, [128, 96, 33, 1], 4, 0.),
    'T2': (4, 192, [192, 161, 160, 129], 4, 0.),
    'T3': (3, 256, [256, 250, 193], 3, 0.),
    'T4': (3, 700, [700, 433, 257], 9, 0.),
    'T5': (4, 300, [300, 252, 3, 0], None, 0.),
    'F1': (3, 70, [70, 33, 51], 'fixed', 3.),
    'F2': (64, 1001, 'drawn', 'fixed', 0.),
}
# tile heights the plan gives, utterance by utterance (tests/test_conv_ln_host.py holds the restatement below to them)
HEIGHTS = {
    'T1': [[128], [96], [33], [1]],
    'T2': [[192], [161], [160], [129]],
    'T3': [[256], [250], [193]],
    'T4': [[175, 175, 175, 175], [145, 145, 143], [129, 128]],
}
PAIRS = {'bf16': (BF16, BF16), 'mixed': (F32, BF16), 'fp32': (F32, F32)}          # (x, w): the ladders of conv_gemm_ln(bwd).hip
# forward options: (film: None | 'plain' | 'strided', p_pre, save, lp_copy, store_y, residual_ln, n2); the last two on split-K only,
# store_y = False on bf16 / bf16 only (the entry point refuses it elsewhere): other paths and pairs drop them
FWD_OPTS = [('strided', 0.1, True, True, True, False, 384), (None, 0., False, False, True, True, 0),
            ('plain', 0.5, True, True, False, True, 128), (None, 0.1, True, False, True, False, 0)]
# backward options: (film, p_pre, w2 128 x 128 on split-K)
BWD_OPTS = [('strided', 0.1, False), (None, 0., True), ('plain', 0.5, True), (None, 0.1, False)]


def _configs():
    ''' [(path, case, Cin, taps, pair)] of the forward and of the backward '''
    fwd = [(SPLITK, n, c, 3, 'bf16') for n in ('T1', 'T2', 'T3', 'T4', 'T5') for c in (256, 384)]
    fwd += [(SPLITK, n, 1024, 3, 'bf16') for n in ('T2', 'T4')]
    fwd += [(PLAN_K3, n, c, 3, 'bf16') for n in ('T1', 'T2', 'T3', 'T4', 'T5') for c in (128, 1024)]
    fixed = [(ROWS64, 'F1', c, t, p) for t, cs in ((3, (128, 1024)), (1, (128, 384))) for c in cs for p in ('fp32', 'mixed', 'bf16')]
    fixed += [(ROWS64, 'T5', 128, 3, 'bf16')]               # fixed tiles with dead tiles below the fill end, an empty utterance
    fixed += [(ROWS128, 'F2', 128, 3, p) for p in ('fp32', 'bf16')]
    bwd = fwd + [(PLAN_K1, n, 384, 1, 'bf16') for n in ('T2', 'T4', 'T5')] + fixed
    return fwd + fixed, bwd


FWD_CONFIGS, BWD_CONFIGS = _configs()


def config_id(cfg):
    path, name, cin, taps, pair = cfg
    return f'{PATH_NAME[path]}-{name}-C{cin}-k{taps}-{pair}'


def fwd_opts(cfg, o):
    ''' option row o as the configuration can take it '''
    film, p, save, lp_copy, store_y, vres, n2 = FWD_OPTS[o]
    path, pair = cfg[0], cfg[4]
    if path != SPLITK:
        vres, n2 = False, 0
    if pair != 'bf16':
        store_y = True
    return film, p, save, lp_copy or n2 > 0 or not store_y, store_y, vres, n2


def bwd_opts(cfg, o):
    film, p, w2 = BWD_OPTS[o]
    return film, p, w2 and cfg[0] == SPLITK


# ----------------------------------------------------------------------------- tile plan
def plan_tiles(name, B=None):
    ''' number of entries of the case's plan: its `tiles=`, or the default (the worst case rounded up to the 256 compute units) '''
    b, N, _, tiles, _ = CASES[name]
    worst = (B or b) * ((N + 255) // 256)
    if tiles is None:
        return (worst + 255) // 256 * 256
    return max(int(tiles), worst)


def tile_plan(lens, N, T, halo=0):
    ''' conv_plan_body: T entries (b, n0, rows, padding rows each workgroup fills) '''
    work = [min(max(int(l), 0) + halo, N) for l in lens]
    lo, hi = 1, 256
    while lo < hi:
        mid = (lo + hi) >> 1
        if sum((l + mid - 1) // mid for l in work) <= T:
            hi = mid
        else:
            lo = mid + 1
    H = lo
    per = (sum(N - l for l in work) + T - 1) // T
    table = []
    for b, l in enumerate(work):
        t = (l + H - 1) // H
        if t == 0:
            continue
        hb = (l + t - 1) // t
        for j in range(t):
            table.append((b, j * hb, max(min(l - j * hb, hb), 0), per))
    table = table[:T]
    return table + [(0, 0, 0, per)] * (T - len(table))


def splitk_branches(h):
    ''' how conv_sk_kernel runs a tile of h rows: [(rows of the workgroup, NA = live 32-row blocks, KS = K slices)] '''
    parts = [128, h - 128] if h > 192 else [h]
    return [(r, (r + 31) // 32, 2 if (r + 31) // 32 >= 5 else 4) for r in parts]


def live_end(length, N, BM):
    ''' fixed BM-row tiles: end of the last tile that starts below length + 2 '''
    return min(N, ((length + 1) // BM + 1) * BM)


def computed_rows(c, path):
    ''' (B, N) bool: the rows on which `path` computes s, mean, rstd (elsewhere below the fill end: exact zeros) '''
    n = torch.arange(c.N)[None, :]
    if path in (SPLITK, PLAN_K3, PLAN_K1):
        return n < c.L[:, None]
    BM = 128 if path == ROWS128 else 64
    return n < torch.tensor([live_end(l, c.N, BM) for l in c.lens])[:, None]


# ----------------------------------------------------------------------------- cases
def case_lengths(name, B=None):
    b, N, lens, _, _ = CASES[name]
    if lens == 'drawn':
        g = torch.Generator().manual_seed(64)
        lens = torch.randint(2, N, (b,), generator=g)
        lens[0], lens[1], lens[2], lens[3] = N, 0, 1, N
        lens = lens.tolist()
    return lens[:B] if B else lens


def _dress(t, L_, fe):
    ''' rows of [len + 2, fe) zero, rows at and past fe NaN '''
    n = torch.arange(t.shape[1])[None, :]
    t[(n >= L_[:, None] + 2).expand(t.shape[:2])] = 0.
    t[(n >= fe[:, None]).expand(t.shape[:2])] = float('nan')
    return t


def _stats(s):
    s = s.double()
    mean = s.mean(dim=2)
    return mean, torch.rsqrt(((s - mean[:, :, None]) ** 2).mean(dim=2) + 1e-5)


def make_case(name, Cin, taps, pair, backward, film=True, p_pre=0., vres=False, n2=0, salt=0, B=None):
    ''' the inputs of a case on the CPU, in their storage types.  The draws do not depend on the options.  B: the first B utterances
        only (the host test's slice of F2).  Weights are drawn in fp32 and rounded to their storage type here, so that the packed
        operand holds exactly these numbers '''
    B0, N, _, _, offset = CASES[name]
    B = B or B0
    lens = case_lengths(name, B)
    x_dtype, w_dtype = PAIRS[pair]
    g = torch.Generator().manual_seed(9000 + 16 * Cin + 4 * taps + ord(name[0]) + 7 * int(name[1]) + (1 if backward else 0))
    c = types.SimpleNamespace(name=name, B=B, N=N, Cin=Cin, taps=taps, pair=pair, backward=backward, lens=lens, p_pre=float(p_pre),
                              seed_pre=(SEED_PRE + salt) & M63, x_dtype=x_dtype, w_dtype=w_dtype, C=128)
    c.L = torch.tensor(lens, dtype=torch.int64)
    fe = fill_end(c.L, N)
    c.fe = fe.tolist()
    c.live = torch.arange(N)[None, :] < c.L[:, None]
    rnd = lambda shape: torch.randn(*shape, generator=g)
    c.x = _dress(rnd((B, N, Cin)), c.L, fe).to(x_dtype)
    c.gamma, c.beta = torch.rand(128, generator=g) + 0.5, rnd((128,))
    flm = rnd((B, 256))
    c.film = flm if film else None
    w2 = (rnd((384, 128)) / 128 ** 0.5).to(BF16).float()
    if not backward:
        c.w = (rnd((128, Cin, taps)) / (Cin * taps) ** 0.5).to(w_dtype).float()          # (Cout, Cin, taps): pack_conv_weight(w)
        c.w_eff = c.w
        c.bias = rnd((128,))
        c.residual = _dress(rnd((B, N, 128)) + offset, c.L, fe)
        rg, rb = torch.rand(128, generator=g) + 0.5, rnd((128,))
        c.b2 = rnd((384,))[:n2] if n2 else None
        c.w2 = w2[:n2].contiguous() if n2 else None
        c.vres = None
        if vres:           # the residual tensor is s1, the saved input of the LayerNorm whose output is the residual stream
            m1, r1 = _stats(torch.nan_to_num(c.residual))
            c.vres = (_dress(m1.float(), c.L, fe), _dress(r1.float(), c.L, fe), rg, rb)
    else:
        c.w_fwd = (rnd((Cin, 128, taps)) / (128 * taps) ** 0.5).to(w_dtype).float()     # forward conv 128 -> Cin: pack(..., transpose_flip=True)
        c.w_eff = c.w_fwd.permute(1, 0, 2).flip(2).contiguous()
        c.bias = None
        c.yin = _dress(rnd((B, N, 128)), c.L, fe)
        c.s_in = _dress(rnd((B, N, 128)) + offset, c.L, fe)
        m, r = _stats(torch.nan_to_num(c.s_in))
        c.mean, c.rstd = _dress(m.float(), c.L, fe), _dress(r.float(), c.L, fe)
        c.init = (rnd((128,)), rnd((128,)), rnd((B, 256)))
        c.w2 = w2[:128].contiguous() if n2 else None
    return c


@functools.lru_cache(maxsize=8)
def _keep(seed, B, N, p):
    keep, scale = DM.elem_keep(seed, 0, range(B), N, 128, p)
    return torch.from_numpy(keep), scale


def keep_of(c):
    ''' (keep (B, N, 128) bool or None, scale) of the dropout in front of the LayerNorm '''
    if c.p_pre <= 0.:
        return None, 1.
    return _keep(c.seed_pre, c.B, c.N, c.p_pre)


def _kp(c, T):
    keep, scale = keep_of(c)
    return None if keep is None else keep.to(T) * scale


def _clean(t, T):
    return torch.nan_to_num(t.to(T), nan=0.)


# ----------------------------------------------------------------------------- the contraction
def conv(x, w):
    ''' THE reference convolution: x (B, N, Cin), w (Cout, Cin, taps), zero "same" padding, no bias; float64 '''
    return F.conv1d(x.double().transpose(1, 2), w.double(), None, padding=w.shape[2] // 2).transpose(1, 2)


def conv_chain(x, w, step, fp32_products=False):
    ''' the contraction as an MFMA chain: fp32 accumulator, one fp32 add per (tap, `step` input channels) partial product in order.
        The partial product itself is exact (float64, then rounded to fp32) -- products of bf16 operands are exact in fp32 -- or, with
        fp32_products, the fp32 product sum of an fp32 MFMA '''
    B, N, Cin = x.shape
    taps = w.shape[2]
    T = F32 if fp32_products else F64
    xp = F.pad(x.to(T), (0, 0, taps // 2, taps // 2))
    wd = w.to(T)
    acc = torch.zeros(B, N, w.shape[0], dtype=F32)
    for tap in range(taps):
        for k0 in range(0, Cin, step):
            acc += (xp[:, tap:tap + N, k0:k0 + step] @ wd[:, k0:k0 + step, tap].T).float()
    return acc


def _conv_of(c, T, x=None):
    if T == F64:
        return conv(_clean(c.x, F64) if x is None else x, c.w_eff)
    xs = _clean(c.x, F32)
    if c.w_dtype == BF16:
        xs = xs.to(BF16).float()                    # fp32 x in front of bf16 weights: rounded when staged
    if c.w_dtype == BF16:
        return conv_chain(xs, c.w_eff, 16)
    return conv_chain(xs, c.w_eff, 2, fp32_products=True)


# ----------------------------------------------------------------------------- forward / backward
def residual_of(c, T, residual=None):
    r = _clean(c.residual, T) if residual is None else residual
    if c.vres is None:
        return r
    m1, r1, rg, rb = (_clean(t, T) for t in c.vres)
    return ((r - m1[:, :, None]) * r1[:, :, None] * rg + rb).masked_fill(~c.live[:, :, None], 0.)


def forward(c, T, path, x=None, residual=None, gamma=None, beta=None, film=None):
    ''' y, s, mean, rstd of the forward case c in arithmetic T (unrounded); float64: differentiable in the tensors given '''
    pick = lambda given, own: None if own is None else (own.to(T) if given is None else given)
    gamma, beta, film = pick(gamma, c.gamma), pick(beta, c.beta), pick(film, c.film)
    v = _conv_of(c, T, x) + c.bias.to(T)
    kp = _kp(c, T)
    if kp is not None:
        v = v * kp
    s = v + residual_of(c, T, residual)
    mean = s.mean(dim=2)
    d = s - mean[:, :, None]
    rstd = torch.rsqrt((d * d).mean(dim=2) + 1e-5)
    t = d * rstd[:, :, None] * gamma + beta
    if film is not None:
        t = film[:, None, :128] * t + film[:, None, 128:]
    y = t.masked_fill(~c.live[:, :, None], 0.)
    comp = computed_rows(c, path)
    return y, s.masked_fill(~comp[:, :, None], 0.), mean.masked_fill(~comp, 0.), rstd.masked_fill(~comp, 0.)


def backward(c, T, given=None):
    ''' closed form in arithmetic T, unrounded: ds, dx, dgamma, dbeta, dfilm (the last three on top of c.init).  given = (s, mean,
        rstd) in place of the case's own '''
    s, mean, rstd = given if given is not None else (_clean(c.s_in, T), _clean(c.mean, T), _clean(c.rstd, T))
    gamma, beta = c.gamma.to(T), c.beta.to(T)
    gy = (_conv_of(c, T) + _clean(c.yin, T)).masked_fill(~c.live[:, :, None], 0.)
    xh = (s - mean[:, :, None]) * rstd[:, :, None]
    dfilm = None
    if c.film is not None:
        dfilm = c.init[2].to(T) + torch.cat([(gy * (xh * gamma + beta)).sum(dim=1), gy.sum(dim=1)], dim=1)
        gy = gy * c.film.to(T)[:, None, :128]
    dgamma = c.init[0].to(T) + (gy * xh).sum(dim=(0, 1))
    dbeta = c.init[1].to(T) + gy.sum(dim=(0, 1))
    gx = gy * gamma
    ds = rstd[:, :, None] * (gx - gx.mean(dim=2, keepdim=True) - xh * (gx * xh).mean(dim=2, keepdim=True))
    ds = ds.masked_fill(~c.live[:, :, None], 0.)
    kp = _kp(c, T)
    return ds, (ds if kp is None else ds * kp), dgamma, dbeta, dfilm


def _bf(t):
    return t.to(BF16).to(t.dtype)


def _second(c, a, T, bias):
    ''' the second product of the split-K epilogue: bf16(a) . w2^T (+ b2), zero off the live rows '''
    if c.w2 is None:
        return None
    if T == F64:
        out = _bf(a) @ c.w2.double().T
    else:
        out = (_bf(a).double() @ c.w2.double().T).float()
    if bias is not None:
        out = out + bias.to(T)
    return out.masked_fill(~c.live[:, :, None], 0.)


def _fwd(c, T, path):
    with torch.no_grad():
        y, s, mean, rstd = forward(c, T, path)
        low = T != F64
        R = {'y': y, 'y_lp': _bf(y) if low else y, 's': s, 'mean': mean, 'rstd': rstd}
        y2 = _second(c, y, T, c.b2)
        if y2 is not None:
            R['y2'] = _bf(y2) if low else y2
    return R


def _bwd(c, T, given):
    with torch.no_grad():
        ds, dx, dgamma, dbeta, dfilm = backward(c, T, given)
        low = T != F64
        R = {'ds': ds, 'dx_lp': _bf(dx) if low else dx, 'dgamma': dgamma, 'dbeta': dbeta}
        if dfilm is not None:
            R['dfilm'] = dfilm
        y2 = _second(c, dx, T, None)
        if y2 is not None:
            R['y2b'] = _bf(y2) if low else y2
    return R


def reference_fwd(c, path):
    ''' THE reference of the forward: float64 from the stored operands; a dict of FWD_TENSORS (y_lp = y; y2 with w2 only) '''
    return _fwd(c, F64, path)


def restate_fwd(c, path):
    return _fwd(c, F32, path)


def reference_bwd(c, given=None):
    ''' THE reference of the backward; a dict of BWD_TENSORS (dfilm with FiLM, y2b with w2 only) '''
    return _bwd(c, F64, given)


def restate_bwd(c, given=None):
    return _bwd(c, F32, given)


def kind_of(c, name):
    ''' which cap limits tensor `name` of case c '''
    if name in BF16_STORED:
        return 'bf16'
    return 'mixed' if c.pair == 'mixed' else 'fp32'


# ----------------------------------------------------------------------------- mask readout
READOUT_MARGIN = 1.


def readout_case(backward, p, Cin=256):
    ''' case T1 with inputs whose outputs tell kept from dropped exactly.  Forward: bias 10, no residual, |conv| a few tenths:
        s = keep * scale * (conv + 10) is 0 or at least 9.  Backward: gamma 1, no FiLM, y_inout = +-(4 + u) with signs + + - - ...,
        s_in = +-(1 + u' / 8) with signs + - + - ..., the conv a tenth of that: gx and gx * xh sum to almost nothing over a row, so no
        ds is near zero and dx_lp = keep * scale * ds is 0 exactly where dropped '''
    c = make_case('T1', Cin, 3, 'bf16', backward, film=False, p_pre=p)
    g = torch.Generator().manual_seed(4242 + Cin)
    fe = torch.tensor(c.fe)
    ch = torch.arange(128)
    c.x = (c.x.float() * 0.1).to(BF16)
    if not backward:
        c.bias = torch.full((128,), 10.)
        c.residual = _dress(torch.zeros(c.B, c.N, 128), c.L, fe)
    else:
        u = torch.randint(0, 64, (c.B, c.N, 128), generator=g).float() / 64.
        v = torch.randint(0, 64, (c.B, c.N, 128), generator=g).float() / 64.
        c.gamma = torch.ones(128)
        c.yin = _dress((1. - 2. * ((ch // 2) % 2).float()) * (4. + v), c.L, fe)
        c.s_in = _dress((1. - 2. * (ch % 2).float()) * (1. + u / 8.), c.L, fe)
        m, r = _stats(torch.nan_to_num(c.s_in))
        c.mean, c.rstd = _dress(m.float(), c.L, fe), _dress(r.float(), c.L, fe)
    return c
