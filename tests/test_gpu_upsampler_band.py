"""The banded Gaussian upsampler (csrc/upsample.hip): the forward and backward kernels evaluate a (phoneme, frame) pair only inside
the phoneme's reach [tlo, thi], on a compacted per-tile list.  These are the smallest shapes at which that logic can go wrong,
compared with a float64 restatement -- tests/upsampler_oracle.py where the case can be drawn by `make_inputs`, and the same
formula written here (`_restate`) where means and sigmas are set by hand.

Bound, per tensor and per case, as in tests/test_gpu_upsampler.py:
    4 * max|fp32 restatement - float64| + 1e-6 * max|float64|          (absolute)
with the fp32 restatement's own distance held under 2e-5 of the tensor's largest element (CAP), checked on the CPU.

Sigma path finite only: `gap_*`.  Their narrow phonemes hold weight 1 - 1e-3 on the frame under their mean and exactly 0 or 1
elsewhere, so dr and drin are the difference dw - Dsum of two numbers that agree to 1e-3, times sigmoid(r_pre) = 0.05: fp32
holds mostly cancellation noise there (the restatement's own distance is 4e-5 .. 6e-5 of the largest element, over CAP whatever
the seed), as in cases C1 and F of the existing test.  Their forward, d_enc and the upsample path d_enc - drin = sum_t w g are held
to the bound.  Every other case, the narrow `empty_tiles` and `on_mean_*` included, meets CAP on every tensor and is held to it.

Lists: `gap_*` has one sigma of 40 among sigmas of 0.05, so the phonemes reaching a tile are not an interval in l, and frames
64..95 lie past the durations' total: only the wide phoneme reaches that tile.  `ties_*` repeats means at the start, in the middle
and at the end.  `wide_long` puts 77 .. 177 (median 158) of the 600 phonemes on a tile's list: three rounds of 256 candidates, on most
tiles more rows than the 128 kept in LDS; `default_long` 7 .. 24.  `empty_tiles` has 217 frames of row 0 that nothing reaches.

Measured on an MI355X, kernel error / bound (absolute):
                  weights          x_up             dec_in           d_enc            drin             dr               d_enc - drin
    wide_long     1.2e-6/3.8e-6    7.2e-6/2.3e-5    9.0e-7/7.0e-6    1.1e-6/8.6e-6    7.5e-7/4.6e-6    1.5e-6/9.2e-6    8.4e-7/6.9e-6
    default_long  1.3e-6/6.6e-6    5.9e-6/3.5e-5    5.9e-6/3.5e-5    7.7e-5/3.2e-4    7.7e-5/3.2e-4    8.8e-4/3.6e-3    3.2e-6/2.7e-5
    empty_tiles   1.8e-6/1.2e-5    5.6e-6/5.0e-5    5.7e-6/5.1e-5    1.1e-4/1.3e-3    1.1e-4/1.3e-3    1.2e-3/1.5e-2    6.9e-6/4.9e-5
    gap_first     4.8e-8/1.2e-6    2.3e-7/4.2e-6    3.0e-7/7.0e-6    2.7e-6/5.1e-5    (finite)         (finite)         2.5e-6/5.0e-5
    gap_last      5.0e-8/1.2e-6    2.2e-7/4.2e-6    4.4e-7/7.2e-6    2.8e-6/4.8e-5    (finite)         (finite)         2.5e-6/4.7e-5
    gap_middle    3.5e-8/1.1e-6    2.7e-7/4.6e-6    2.8e-7/6.9e-6    3.9e-6/4.0e-5    (finite)         (finite)         3.3e-6/4.3e-5
    ties_8        5.8e-8/1.3e-6    3.6e-7/4.6e-6    3.6e-7/5.6e-6    6.2e-7/5.0e-6    4.4e-7/2.1e-6    2.0e-6/9.0e-6    3.9e-7/4.7e-6
    ties_33       3.4e-7/3.5e-6    1.1e-6/9.5e-6    1.0e-6/1.1e-5    2.9e-5/1.9e-4    2.9e-5/1.9e-4    9.8e-5/6.5e-4    3.8e-6/1.9e-5
    on_mean_a     5.9e-8/1.4e-6    1.7e-7/4.0e-6    2.4e-7/5.8e-6    2.2e-5/1.6e-4    2.2e-5/1.6e-4    7.4e-5/5.3e-4    7.8e-7/9.7e-6
    on_mean_b     5.9e-8/1.4e-6    1.7e-7/4.0e-6    2.4e-7/5.8e-6    9.0e-6/8.2e-5    9.0e-6/7.9e-5    3.1e-5/2.6e-4    4.6e-7/8.5e-6
The largest ratio is 0.32 (weights and x_up of wide_long).  In every case weights, x_up and dec_in are bit for bit what the dense
kernels before the band gave on the same inputs.  The whole file takes 3 s, nearly all of it the first import.
"""
import functools
import math
import types

import pytest
import torch
import torch.nn.functional as F

from tests import upsampler_oracle as U

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
CAP = 2e-5
C = U.C
FWD = ('weights', 'x_up', 'dec_in')
BWD = ('d_enc', 'drin', 'dr')

# ---------------------------------------------------------------- cases drawn by upsampler_oracle.make_inputs: (L_b), (T_b), knobs
ORACLE_CASES = {
    'wide_long': ([600, 40], [1800, 100], dict(b_range_shift=18.3, w_range_scale=5.7)),
    'default_long': ([600, 40], [1800, 100], {}),
    'empty_tiles': ([5, 70], [40, 257], dict(b_range_shift=-3.)),
}


# ---------------------------------------------------------------- cases with durations and sigmas set by hand
def _gap(wide):
    ''' L = 12, T = 96: durations sum to 64, sigma 0.05 except phoneme `wide` (40) '''
    sig = [0.05] * 12
    sig[wide] = 40.
    return dict(dur=[[3] * 11 + [31]], sigma=[sig], T=96, seed=11 + wide)


HAND_CASES = {
    'gap_first': _gap(0),
    'gap_last': _gap(11),
    'gap_middle': _gap(6),
    'ties_8': dict(dur=[[0, 0, 3, 0, 5, 0, 0]], sigma=None, T=8, seed=3),
    'ties_33': dict(dur=[[0, 0, 13, 0, 20, 0, 0], [0, 4, 0, 0, 0, 2, 0]], sigma=None, T=33, seed=4),
    # sigma 0.3 < 1 (-log sigma > 0) for phoneme 1, whose mean 9.5 is frame 9's centre exactly; then one frame further (10.5)
    'on_mean_a': dict(dur=[[9, 1, 13, 17]], sigma=[[0.05, 0.3, 0.05, 0.05]], T=40, seed=5),
    'on_mean_b': dict(dur=[[9, 3, 11, 17]], sigma=[[0.05, 0.3, 0.05, 0.05]], T=40, seed=5),
}
SIGMA_NOISE = ('gap_first', 'gap_last', 'gap_middle')


def _hand_inputs(dur, sigma, T, seed):
    g = torch.Generator().manual_seed(seed)
    d = torch.tensor(dur, dtype=torch.int64)
    B, L = d.shape
    if sigma is None:
        r_pre = torch.randn(B, L, generator=g) * 0.3          # softplus -> sigma ~ 0.7
    else:
        s = torch.tensor(sigma, dtype=torch.float64)
        r_pre = torch.where(s > 20., s, torch.log(torch.expm1(s))).float()
    means = (d.double() / 2 + (torch.cumsum(d, 1) - d).double()).float()      # exact: halves of small integers
    return {'xp': torch.randn(B, L, C, generator=g), 'r_pre': r_pre, 'means': means, 'w_range': torch.randn(1, C, generator=g) / math.sqrt(C),
            'in_lengths': torch.full((B,), L, dtype=torch.int64), 'out_lengths': torch.full((B,), T, dtype=torch.int64),
            'pos': torch.randn(T, C, generator=g), 'g': torch.randn(B, T, C, generator=g)}


def _restate(inp, dtype):
    ''' the upsampler from (x', r_pre, means) on, as upsampler_oracle.upsample lines 75-82, with the gradients of sum(dec_in * g):
        r_pre depends on x' through the range projection (d r_pre / d x' = w_range), which is where drin = dr * w_range comes from '''
    f = lambda name: inp[name].to(dtype)
    xp = f('xp').requires_grad_(True)
    r0 = f('r_pre').requires_grad_(True)
    rin = torch.zeros_like(xp).requires_grad_(True)
    w_r = f('w_range')[0]
    r_pre = r0 + ((xp - xp.detach() + rin) * w_r).sum(2)
    B, L, _ = xp.shape
    T = inp['g'].shape[1]
    pad = torch.arange(L)[None, :] >= inp['in_lengths'][:, None]
    ranges = F.softplus(r_pre).masked_fill(pad, 1.)
    t = torch.arange(T, dtype=dtype) + 0.5
    mu, sigma = f('means').unsqueeze(2), ranges.unsqueeze(2)
    logp = -((t - mu) ** 2) / (2 * sigma ** 2) - sigma.log() - math.log(math.sqrt(2 * math.pi))
    p = torch.exp(logp).masked_fill(pad.unsqueeze(2), 0.)
    weights = p / (p.sum(dim=1, keepdim=True) + U.EPS)
    x_up = weights.transpose(1, 2) @ xp
    live = (torch.arange(T)[None, :] < inp['out_lengths'][:, None]).unsqueeze(2)
    dec_in = (x_up + f('pos')[:T]).masked_fill(~live, 0.)
    d_enc, drin, dr = torch.autograd.grad((dec_in * f('g')).sum(), [xp, rin, r0])
    out = {'weights': weights, 'x_up': x_up, 'dec_in': dec_in, 'd_enc': d_enc, 'drin': drin, 'dr': dr}
    return {k: v.detach() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def _reference(name):
    ''' CPU only: float32 inputs and both restatements of a case '''
    c = types.SimpleNamespace(name=name)
    if name in ORACLE_CASES:
        c.Ls, c.Ts, knobs = ORACLE_CASES[name]
        c.cpu = U.make_inputs(c.Ls, c.Ts, seed=sum(c.Ts), **knobs)
        c.o32, c.o64 = U.upsample(c.cpu, torch.float32), U.upsample(c.cpu, torch.float64)
    else:
        c.cpu = _hand_inputs(**HAND_CASES[name])
        c.Ls, c.Ts = c.cpu['in_lengths'].tolist(), c.cpu['out_lengths'].tolist()
        c.o32, c.o64 = _restate(c.cpu, torch.float32), _restate(c.cpu, torch.float64)
    for o in (c.o32, c.o64):
        o['d_up'] = o['d_enc'] - o['drin']          # the upsample path alone: sum_t w[l,t] g[t,:]
    return c


def _run(c, inp):
    ''' one run of the kernels on a case's device inputs: forward with and without the positional table, then backward '''
    from daft_exprt import ops
    T = inp['g'].shape[1]
    k = {}
    if c.name in ORACLE_CASES:
        P = {n: inp[n] for n in U.PARAMS}
        xp, ranges, r_pre, _ = ops.gu_prepare(inp['enc'], inp['dur_float'], inp['energy'], inp['pitch'], inp['in_lengths'], P, save=True)
        means, _ = ops.gu_means(inp['dur_int'])
    else:
        xp, r_pre, means = inp['xp'], inp['r_pre'], inp['means']
        ranges = F.softplus(r_pre)
    k['dec_in'], k['weights'] = ops.gu_upsample_fwd(xp, ranges, means, inp['in_lengths'], T, inp['out_lengths'], inp['pos'])
    k['x_up'], k['weights_raw'] = ops.gu_upsample_fwd(xp, ranges, means, inp['in_lengths'], T)
    k['d_enc'], k['drin'], k['dr'] = ops.gu_upsample_bwd(inp['g'], xp, k['weights'], means, ranges, r_pre, inp['w_range'],
                                                         inp['in_lengths'], inp['out_lengths'])
    k['d_up'] = k['d_enc'] - k['drin']
    return k


@functools.lru_cache(maxsize=None)
def _case(name):
    c = _reference(name)
    c.inp = {k: v.to(DEV) for k, v in c.cpu.items()}
    c.k = _run(c, c.inp)
    torch.cuda.synchronize()
    return c


def cap_misses(c, names):
    ''' the tensors whose fp32 restatement is further than CAP of their largest element from float64 (CPU only) '''
    bad = []
    for n in names:
        own, top = float((c.o32[n].double() - c.o64[n]).abs().max()), float(c.o64[n].abs().max())
        if not own <= CAP * top:
            bad.append((c.name, n, own, top))
    return bad


def _check(c, names):
    bad, line = [], []
    for n in names:
        err = float((c.k[n].double().cpu() - c.o64[n]).abs().max())
        bound = U.bound(c.o32, c.o64, n)
        line.append(f'{n} {err:.2g}/{bound:.2g}')
        if not err <= bound:
            bad.append((n, err, bound))
    print(f'{c.name}:', '  '.join(line))
    assert not cap_misses(c, names), ('fp32 restatement too far from float64: change the inputs', cap_misses(c, names))
    assert not bad, (c.name, bad)


ALL = list(ORACLE_CASES) + list(HAND_CASES)


@pytest.mark.parametrize('name', ALL)
def test_forward(name):
    c = _case(name)
    _check(c, FWD)
    assert torch.equal(c.k['weights'].view(torch.int32), c.k['weights_raw'].view(torch.int32))
    for b, (Lb, Tb) in enumerate(zip(c.Ls, c.Ts)):
        assert not c.k['weights'][b, Lb:].any(), 'weights of padding phonemes must be exactly 0'
        assert not c.k['dec_in'][b, Tb:].any(), 'decoder input past out_lengths must be exactly 0'


@pytest.mark.parametrize('name', [n for n in ALL if n not in SIGMA_NOISE])
def test_backward(name):
    c = _case(name)
    _check(c, BWD + ('d_up',))
    for b, Lb in enumerate(c.Ls):
        assert not c.k['d_enc'][b, Lb:].any() and not c.k['drin'][b, Lb:].any() and not c.k['dr'][b, Lb:].any()


@pytest.mark.parametrize('name', SIGMA_NOISE)
def test_backward_of_nearly_one_hot_weights(name):
    ''' the sigma path of the gap cases is cancellation noise in fp32 (module docstring): dr and drin finite only; d_enc, and the
        upsample path alone, which does not pass through sigma, within the bound '''
    c = _case(name)
    for n in BWD:
        assert bool(torch.isfinite(c.k[n]).all()), n
    _check(c, ('d_enc', 'd_up'))


def test_frames_nothing_reaches_are_exact_zeros():
    c = _case('empty_tiles')
    assert not c.k['weights'][0, :, 64:].any() and not c.k['weights_raw'][0, :, 64:].any()
    assert not c.k['dec_in'][0, 40:].any()
    assert not c.k['x_up'][0, 64:].any()
    # the live frames next to them: normalised where a Gaussian holds its own against the 1e-20, ~0 where even the nearest is
    # far below it or underflows (sigma ~ 0.05; 6 of the 40 frames are of the first kind)
    total = c.k['weights'][0, :, :40].sum(0)
    assert bool(((total > 0.999) | (total < 1e-5)).all()) and int((total > 0.999).sum()) >= 5
    assert torch.equal(total > 0.999, (c.o64['weights'][0, :, :40].sum(0) > 0.999).to(DEV))


def test_gap_tile_holds_the_wide_phoneme_alone():
    ''' frames 64..95 lie past every narrow phoneme: the wide one has weight 1 there, whichever l it has '''
    for name, wide in (('gap_first', 0), ('gap_last', 11), ('gap_middle', 6)):
        w = _case(name).k['weights'][0]
        assert bool((w[wide, 70:] == 1.).all()), name
        others = [l for l in range(12) if l != wide]
        assert not w[others, 70:].any(), name


def test_a_frame_on_the_mean_and_one_further():
    ''' phoneme 1 (sigma 0.3) owns the frame its mean sits on, in both placements, and its Gaussian reaches the same number of
        frames around it: the band's two ends move with the mean '''
    wa, wb = _case('on_mean_a').k['weights'][0, 1], _case('on_mean_b').k['weights'][0, 1]
    assert float(wa[9]) > 0.99 and float(wb[10]) > 0.99
    assert not wa[:4].any() and not wa[16:].any() and not wb[:5].any() and not wb[17:].any()      # 0.3 * sqrt(2 * 90) = 4 frames


def test_forward_and_backward_are_reproducible():
    c = _case('ties_33')
    k = _run(c, c.inp)
    for n in ('weights', 'weights_raw', 'dec_in', 'x_up') + BWD:
        assert torch.equal(k[n].view(torch.int32), c.k[n].view(torch.int32)), n
