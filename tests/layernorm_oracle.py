"""Plain-torch restatement of the fused LayerNorm (header comment of csrc/layernorm.hip) with its closed-form backward, the
low-precision restatement that sizes the tolerances of tests/test_gpu_layernorm.py, the builder of the test cases and the inputs
of the mask readout.  Test infrastructure: nothing in the package imports this.  Everything runs on the CPU.

    s    = keep_pre * scale_pre * x + residual
    mean = sum_c s / C;   rstd = 1 / sqrt(sum_c (s - mean)^2 / C + 1e-5);   xh = (s - mean) * rstd
    ln   = xh * gamma + beta
    y    = film_gamma[b] * (keep_post * scale_post * ln) + film_beta[b]
    y = 0 on rows n >= lengths[b];   y, y_lp, s, mean, rstd = 0 on rows n >= skip[b] + 2

    gy   = dy, zero on the rows where y is zero
    dfilm[b] = [sum_n gy * keep_post * scale_post * ln | sum_n gy];   gl = gy * film_gamma[b] * keep_post * scale_post
    dgamma = sum_bn gl * xh;   dbeta = sum_bn gl;   gx = gl * gamma
    ds   = rstd * (gx - mean_c(gx) - xh * mean_c(gx * xh));   ds = 0 where s <= 0 (relu_input; ds only, the sums are not gated)
    dx_pre = keep_pre * scale_pre * ds

`keep, scale` are those of tests/dropout_masks.elem_keep, stream 0 in front of the LayerNorm and stream 1 behind it: the masks
the kernels draw.  The rows of [lengths, skip + 2) are computed (s, mean, rstd) and take part in the backward with a zero
upstream gradient -- or with the given one when `lengths` is None.
"""
import functools
import types

import torch

from tests import dropout_masks as DM
from tests.util import fill_end

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
SEED_PRE, SEED_POST = 0x5DEECE66D1234ABC, 0x7A3C96E17B2D4F08          # 63 bits each
M63 = (1 << 63) - 1
FWD_TENSORS = ('y', 'y_lp', 's', 'mean', 'rstd')
BWD_TENSORS = ('ds', 'dx_pre', 'dx_pre_lp', 'dgamma', 'dbeta', 'dfilm')
# largest max|restatement - float64| / max|float64| an utterance's tensor may have (tests/test_layernorm_host.py).  The worst measured
# over the cases below: fp32 3.3e-7 at row offsets 0 and 3 and 6.9e-6 at offset 100 (case D: s - mean loses 100 / spread of fp32's
# 2^-24); a bf16-rounded output 3.8e-3 (half an ulp of bf16, 2^-8, when the largest element sits just above a power of two)
CAP = {'fp32': 1.2e-5, 'bf16': 7.8e-3}

# name -> (B, N, lengths, row offset of x).  What each reaches is said in tests/test_gpu_layernorm.py
CASES = {
    'A': (3, 70, [70, 33, 51], 3.),
    'B': (4, 300, [300, 252, 3, 0], 0.),
    'C': (30, 900, 'drawn', 0.),
    'D': (2, 37, None, 100.),
    'E': (3, 70, [70, 33, 51], 0.),
}
WIDTHS = {'A': (128, 256, 512, 1024), 'B': (128, 256, 512, 1024), 'C': (128,), 'D': (128, 1024), 'E': (128, 1024)}
# how lengths / skip_lengths are handed over: None = `lengths` alone (no row is NaN: the kernels read the pad rows of s then);
# 'same' = skip_lengths = lengths; 'grouped' = skip_lengths = max(lengths - 2, 0) beside lengths (the grouped step's form);
# 'skip_only' = skip_lengths alone, the rows of [lengths, lengths + 2) carry a gradient
VARIANTS = {'A': (None,), 'B': ('same', 'grouped', 'skip_only'), 'C': ('same',), 'D': (None,), 'E': (None,)}


def case_lengths(name):
    B, N, lens, _ = CASES[name]
    if lens == 'drawn':
        g = torch.Generator().manual_seed(30)
        lens = torch.randint(0, N + 1, (B,), generator=g)
        lens[0], lens[7], lens[11], lens[19] = N, 0, 1, 250          # fill ends 257, 513, 769 and N all occur
        lens = lens.tolist()
    return lens


def make_case(name, C, variant=None, x_dtype=F32, dy_dtype=F32, residual=True, film=True, p_pre=0., p_post=0., s_given=False, salt=0):
    ''' the inputs of a case, on the CPU, in their storage types.  gamma in [0.5, 1.5]; beta, FiLM, the residual and dy standard
        normal; x standard normal plus the case's row offset (case E: relu of it, with exact zeros).  The draws do not depend on
        the options.  `s_given`: x IS the normalised tensor s (the backward alone: no dropout_pre, no residual in the forward;
        p_pre still masks dx_pre).  With a skip, the rows at or past skip + 2 of x, residual and dy hold NaN. '''
    B, N, _, offset = CASES[name]
    lens = case_lengths(name)
    g = torch.Generator().manual_seed(7000 + 16 * C + ord(name))
    c = types.SimpleNamespace(name=name, B=B, N=N, C=C, variant=variant, p_pre=float(p_pre), p_post=float(p_post), s_given=s_given,
                              relu=(name == 'E'), seed_pre=(SEED_PRE + salt) & M63, seed_post=(SEED_POST + salt) & M63)
    x = torch.randn(B, N, C, generator=g) + offset
    res = torch.randn(B, N, C, generator=g)
    c.gamma, c.beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    flm = torch.randn(B, 2 * C, generator=g)
    dy = torch.randn(B, N, C, generator=g)
    c.init = (torch.randn(C, generator=g), torch.randn(C, generator=g), torch.randn(B, 2 * C, generator=g))      # dgamma, dbeta, dfilm before
    if name == 'E':
        x = torch.relu(x)
    n = torch.arange(N)[None, :]
    every = torch.ones(B, N, dtype=torch.bool)
    c.lengths = c.skip = None
    c.live = c.comp = every
    if lens is not None:
        L = torch.tensor(lens, dtype=torch.int64)
        if variant != 'skip_only':
            c.lengths, c.live = L, n < L[:, None]
        if variant is not None:
            c.skip = torch.clamp(L - 2, min=0) if variant == 'grouped' else L
            c.comp = n < (c.skip[:, None] + 2)
    c.fe = (fill_end(c.skip, N) if c.skip is not None else torch.full((B,), N)).tolist()      # contract rows of utterance b: [0, fe[b])
    for t in (x, res, dy):
        t[~c.comp] = float('nan')
    c.x, c.dy = x.to(x_dtype), dy.to(dy_dtype)
    c.residual = res if (residual and not s_given and name != 'E') else None
    c.film = flm if film else None
    return c


@functools.lru_cache(maxsize=8)
def _keep(seed, stream, B, N, C, p):
    keep, scale = DM.elem_keep(seed, stream, range(B), N, C, p)
    return torch.from_numpy(keep), scale


def keep_of(c, stream):
    ''' (keep (B, N, C) bool or None, scale) of the dropout in front of (stream 0) / behind (stream 1) the LayerNorm of case c '''
    p, seed = (c.p_pre, c.seed_pre) if stream == 0 else (c.p_post, c.seed_post)
    if p <= 0.:
        return None, 1.
    return _keep(seed, stream, c.B, c.N, c.C, p)


def _kp(c, stream, T):
    keep, scale = keep_of(c, stream)
    return None if keep is None else keep.to(T) * scale


def forward(c, T, x=None, residual=None, gamma=None, beta=None, film=None):
    ''' y, s, mean, rstd of case c in arithmetic T (unrounded); differentiable in the tensors given in place of the case's own '''
    pick = lambda given, own: None if own is None else (own.to(T) if given is None else given)
    x, residual, film = pick(x, c.x), pick(residual, c.residual), pick(film, c.film)
    gamma, beta = pick(gamma, c.gamma), pick(beta, c.beta)
    dead = ~c.comp[:, :, None]
    s = x.masked_fill(dead, 0.)
    if not c.s_given:
        kp = _kp(c, 0, T)
        if kp is not None:
            s = s * kp
        if residual is not None:
            s = s + residual.masked_fill(dead, 0.)
    mean = s.mean(dim=2)
    d = s - mean[:, :, None]
    rstd = torch.rsqrt((d * d).mean(dim=2) + 1e-5)
    t = d * rstd[:, :, None] * gamma + beta
    kq = _kp(c, 1, T)
    if kq is not None:
        t = t * kq
    if film is not None:
        t = film[:, None, :c.C] * t + film[:, None, c.C:]
    y = t.masked_fill(~(c.live & c.comp)[:, :, None], 0.)
    return y, s, mean.masked_fill(~c.comp, 0.), rstd.masked_fill(~c.comp, 0.)


def backward(c, T, s, mean, rstd):
    ''' closed form, arithmetic T, unrounded: ds, dx_pre, dgamma, dbeta, dfilm (the last three on top of c.init) '''
    gamma, beta = c.gamma.to(T), c.beta.to(T)
    gy = c.dy.to(T).masked_fill(~(c.live & c.comp)[:, :, None], 0.)
    xh = (s - mean[:, :, None]) * rstd[:, :, None]
    kq = _kp(c, 1, T)
    dfilm = None
    if c.film is not None:
        ln = xh * gamma + beta
        lnk = ln if kq is None else ln * kq
        dfilm = c.init[2].to(T) + torch.cat([(gy * lnk).sum(dim=1), gy.sum(dim=1)], dim=1)
        gy = gy * c.film.to(T)[:, None, :c.C]
    gl = gy if kq is None else gy * kq
    dgamma = c.init[0].to(T) + (gl * xh).sum(dim=(0, 1))
    dbeta = c.init[1].to(T) + gl.sum(dim=(0, 1))
    gx = gl * gamma
    m1 = gx.mean(dim=2, keepdim=True)
    m2 = (gx * xh).mean(dim=2, keepdim=True)
    ds = rstd[:, :, None] * (gx - m1 - xh * m2)
    if c.relu:
        ds = ds.masked_fill(~(s > 0.), 0.)
    ds = ds.masked_fill(~c.comp[:, :, None], 0.)
    kp = _kp(c, 0, T)
    dx_pre = ds if kp is None else ds * kp
    return ds, dx_pre, dgamma, dbeta, dfilm


def _compute(c, T, y_dtype, d_dtype, stats):
    rnd = lambda t, dtype: t if (T == F64 or dtype is None) else t.to(dtype).to(T)
    with torch.no_grad():
        y, s, mean, rstd = forward(c, T)
        R = {'y': rnd(y, y_dtype), 'y_lp': rnd(y, BF16), 's': s, 'mean': mean, 'rstd': rstd}
        if stats is not None:
            mean, rstd = (t.reshape(c.B, c.N).to(T).masked_fill(~c.comp, 0.) for t in stats)
        ds, dx_pre, dgamma, dbeta, dfilm = backward(c, T, s, mean, rstd)
        R.update(ds=rnd(ds, d_dtype), dx_pre=rnd(dx_pre, d_dtype), dx_pre_lp=rnd(dx_pre, BF16), dgamma=dgamma, dbeta=dbeta)
        if dfilm is not None:
            R['dfilm'] = dfilm
    return R


def reference(c):
    ''' THE reference: forward and closed-form backward of case c in float64 from the stored inputs; a dict of FWD_TENSORS and
        BWD_TENSORS (y_lp = y, dx_pre_lp = dx_pre; dfilm only with FiLM) '''
    return _compute(c, F64, None, None, None)


def restate(c, y_dtype=F32, d_dtype=F32, stats=None):
    ''' the same computation in fp32 arithmetic with bf16 rounding exactly where the kernels round: the inputs as stored in the
        case, y as `y_dtype`, ds and dx_pre as `d_dtype`, y_lp and dx_pre_lp always bf16; s, the statistics and the per-channel sums
        are never rounded.  `stats` = (mean, rstd) fp32: what the backward kernel is handed in place of this forward's own. '''
    return _compute(c, F32, y_dtype, d_dtype, stats)


def region(t, name, b, fe):
    ''' the part of tensor `name` ((B, N, C); mean, rstd (B, N); dfilm (B, 2C)) that belongs to utterance b: its contract rows
        [0, fe) -- or the whole of dgamma / dbeta (b = None) '''
    if name in ('dgamma', 'dbeta'):
        return t
    if name == 'dfilm':
        return t[b]
    return t[b, :fe]


def regions(c, name):
    ''' [(b, fe)] to hand to `region`: one per utterance, or the single (None, None) of dgamma / dbeta '''
    return [(None, None)] if name in ('dgamma', 'dbeta') else [(b, c.fe[b]) for b in range(c.B)]


def bound(low, ref, name, b, fe):
    ''' 4 * max|restatement - float64| + 1e-6 * max|float64| over utterance b's part of tensor `name`; also
        max|restatement - float64| / max|float64| (what CAP limits) '''
    r = region(ref[name], name, b, fe).double()
    own = float((region(low[name], name, b, fe).double() - r).abs().max())
    top = float(r.abs().max())
    return 4. * own + 1e-6 * top, (own / top if top > 0. else 0.)


def restatement_kind(name, y_dtype, d_dtype):
    ''' which cap limits tensor `name`: 'bf16' for a tensor stored in bf16, 'fp32' for the others '''
    if name in ('y_lp', 'dx_pre_lp'):
        return 'bf16'
    if name == 'y':
        return 'bf16' if y_dtype == BF16 else 'fp32'
    if name in ('ds', 'dx_pre'):
        return 'bf16' if d_dtype == BF16 else 'fp32'
    return 'fp32'


# ----------------------------------------------------------------------------- mask readout
READOUT_MARGIN = 1.
READOUT_B, READOUT_N = 3, 37


def readout_inputs(C, dtype):
    ''' inputs whose outputs tell kept from dropped exactly (gamma = 1, beta = 10, no residual, no FiLM, no lengths):
          x  = +-(1 + u / 8), signs + - + - ...:  s = keep_pre * scale * x is 0 or at least 1 in size            (stream 0, forward: s_out)
          y  = keep_post * scale * (xh + 10):     0 or at least 10 - |xh|                                       (stream 1, forward)
          dy = +-(4 + u'), signs + + - - ...:      gx, gx * xh sum to almost nothing over a row, so
               ds / rstd = keep_post * scale * dy - m1 - xh * m2 is well below or well above 2 * scale in size   (stream 1, backward)
               and with p_post = 0 no ds is near zero: dx_pre = keep_pre * scale * ds is 0 exactly where dropped (stream 0, backward)
        u, u' uniform in [0, 1) on a grid of 1 / 64 (exact in bf16).  tests/test_layernorm_host.py holds the margins. '''
    g = torch.Generator().manual_seed(4242 + C)
    ch = torch.arange(C)
    u = torch.randint(0, 64, (READOUT_B, READOUT_N, C), generator=g).float() / 64.
    v = torch.randint(0, 64, (READOUT_B, READOUT_N, C), generator=g).float() / 64.
    x = (1. - 2. * (ch % 2).float()) * (1. + u / 8.)
    dy = (1. - 2. * ((ch // 2) % 2).float()) * (4. + v)
    return x.to(dtype), dy.to(dtype), torch.ones(C), torch.full((C,), 10.)


def readout_case(C, dtype, p, stream, s_given=False):
    ''' the readout inputs as a case with dropout p on `stream` alone; s_given: the backward is handed x as s '''
    x, dy, gamma, beta = readout_inputs(C, dtype)
    B, N = READOUT_B, READOUT_N
    every = torch.ones(B, N, dtype=torch.bool)
    return types.SimpleNamespace(name='readout', B=B, N=N, C=C, variant=None, p_pre=float(p) if stream == 0 else 0.,
                                 p_post=float(p) if stream == 1 else 0., s_given=s_given, relu=False,
                                 seed_pre=SEED_PRE, seed_post=SEED_POST, x=x, dy=dy, residual=None, film=None,
                                 gamma=gamma, beta=beta, init=(torch.zeros(C), torch.zeros(C), None), lengths=None, skip=None,
                                 live=every, comp=every, fe=[N] * B)


def decode_forward(stream, y, s_out):
    ''' the keep bits a forward run shows: s_out != 0 (stream 0), y != 0 (stream 1) '''
    return (s_out if stream == 0 else y) != 0


def decode_backward(stream, ds, dx_pre, rstd, scale):
    ''' the keep bits a backward run shows: dx_pre != 0 (stream 0; ds itself is nowhere near zero), |ds| / rstd > 2 * scale (stream 1:
        at least 4 * scale less m1 + xh * m2 where kept, m1 + xh * m2 alone where dropped) '''
    if stream == 0:
        return dx_pre != 0
    return ds.double().abs() > 2. * scale * rstd.double().reshape(ds.shape[0], ds.shape[1], 1)
