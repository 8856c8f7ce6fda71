"""The Gaussian upsampler's kernels (csrc/upsample.hip) called directly and compared with the float64 restatement of
tests/upsampler_oracle.py, plus the three launches of model.py that turn their outputs into the eight parameter gradients.

Tolerance, per tensor and per case, computed here on the same inputs (`upsampler_oracle.bound`):
    4 * max|fp32 restatement - float64| + 1e-6 * max|float64|          (absolute)
and the fp32 restatement's own distance is itself held under 2e-5 of the tensor's largest element (cases A-E), so the
bound cannot go slack.  Two places where the sigma-path gradient is zero by construction and fp32 only carries cancellation
noise there: case F (every weight is 0 or 1) and the one-phoneme case C1 (the only weight is 1 whatever sigma is).

Measured on an MI355X, kernel error / bound (absolute; means and totals equal the int64 values exactly in every case):
         r_pre            ranges           weights          x_up             d_enc            dr               dw_range       db_range         dw_dur           dw_en
    A    2.5e-7/4.1e-6    1.9e-7/2.6e-6    3.4e-6/4.8e-6    1.6e-5/2.0e-5    9.8e-5/3.0e-4    1.1e-3/3.2e-3    5.9e-3/1.4e-2  1.0e-3/3.6e-3    3.1e-5/1.3e-4    2.1e-4/3.9e-4
    B    2.6e-7/4.1e-6    1.8e-7/3.0e-6    4.2e-6/1.0e-5    2.2e-5/5.3e-5    5.4e-5/1.3e-4    5.7e-4/1.4e-3    2.7e-3/1.0e-2  4.8e-4/8.6e-4    3.3e-6/1.2e-5    1.2e-4/5.0e-4
    C1   8.3e-8/2.0e-7    1.5e-8/8.1e-7    0/1.0e-6         2.6e-7/3.5e-6    2.2e-16/3.2e-6   1.3e-15/2.8e-6   4.3e-15/9.1e-6 1.3e-15/2.8e-6   1.4e-18/2.9e-9   1.2e-7/4.0e-6
    C2   6.8e-8/2.1e-6    3.5e-8/2.1e-6    7.0e-8/1.4e-6    4.3e-7/5.6e-6    4.9e-7/6.4e-6    2.1e-6/9.8e-6    9.3e-6/4.5e-5  5.9e-7/1.5e-6    4.4e-9/1.6e-8    9.0e-7/1.2e-5
    D    1.4e-7/1.9e-6    6.4e-8/1.7e-6    4.8e-7/2.9e-6    2.0e-6/1.1e-5    9.4e-6/3.1e-5    1.1e-4/2.8e-4    4.0e-4/1.1e-3  2.0e-5/9.9e-5    3.4e-7/6.0e-7    1.7e-5/5.3e-5
    E    1.6e-6/3.7e-5    2.5e-6/3.7e-5    1.2e-6/3.6e-6    4.2e-6/1.8e-5    1.1e-6/7.2e-6    2.7e-7/2.9e-6    3.8e-6/2.6e-5  5.2e-7/2.8e-6    2.3e-8/2.4e-7    4.5e-6/2.9e-5
    F    3.5e-7/9.4e-6    4.8e-9/1.0e-6    0/1.0e-6         4.0e-7/6.3e-6    (backward: finite only)
The tensors left out (xp, rin, dec_in, drin, the other biases and dw_pi) sit at the same fractions of their bounds; the largest
ratio anywhere is x_up / dec_in in case A (0.8).  Largest element, for scale: weights 1, x_up 5, and in case A dr 470, dw_range 2000.
Started from a non-zero buffer the parameter gradients land within 0.5 of the bound of that test.  In case E 36 % of the
rows have r_pre > 20 (8.9 ... 28.7).  Each test takes under half a second, most a few milliseconds.
"""
import functools
import types

import pytest
import torch

from tests import upsampler_oracle as U

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'

# (L_b), (T_b), knobs of upsampler_oracle.make_inputs
CASES = {
    'A': ([70, 65, 64, 2], [257, 129, 128, 65], {}),      # T % 32 != 0; L across the 64-row LDS chunk; rows with many frames past their total
    'B': ([200, 131, 7], [600, 333, 40], {}),             # four LDS chunks and four wave-chunks of the carried scan; mostly skipped bands
    'C1': ([1], [1], {}),                                  # one phoneme, one frame
    'C2': ([3, 1], [5, 2], {}),
    'D': ([9, 0], [33, 0], {}),                            # an empty utterance
    'E': ([70, 33], [257, 100], dict(b_range_shift=18.3, w_range_scale=5.7)),     # r_pre straddles softplus' threshold 20
    'F': ([70, 33], [257, 100], dict(b_range_shift=-6.)),                         # ranges ~ 1e-3: one-hot weights, frames where every Gaussian underflows
}
WITH_BACKWARD = ['A', 'B', 'C1', 'C2', 'D', 'E']
FWD = ('xp', 'rin', 'r_pre', 'ranges', 'weights', 'x_up', 'dec_in')
BWD = ('d_enc', 'drin', 'dr')
DPARAMS = tuple('d' + name for name in U.PARAMS)
SIGMA_ONLY = ('drin', 'dr', 'dw_range', 'db_range', 'dw_dur', 'db_dur')      # gradients that flow through sigma alone
# one phoneme: w = p / (p + 1e-20) = 1 whatever sigma is, so these are 0 up to the 1e-20 and the fp32 restatement holds cancellation
# noise only -- its distance cannot be measured against the tensor's largest element
NO_CAP = {('C1', name) for name in SIGMA_ONLY}
CAP = 2e-5


def _forward(inp, pos=True):
    from daft_exprt import ops
    P = {k: inp[k] for k in ('w_dur', 'b_dur', 'w_en', 'b_en', 'w_pi', 'b_pi', 'w_range', 'b_range')}
    k = {}
    k['xp'], k['ranges'], k['r_pre'], k['rin'] = ops.gu_prepare(inp['enc'], inp['dur_float'], inp['energy'], inp['pitch'],
                                                                inp['in_lengths'], P, save=True)
    k['means'], k['totals'] = ops.gu_means(inp['dur_int'])
    T = inp['g'].shape[1]
    if pos:
        k['dec_in'], k['weights'] = ops.gu_upsample_fwd(k['xp'], k['ranges'], k['means'], inp['in_lengths'], T, inp['out_lengths'], inp['pos'])
    else:
        k['x_up'], k['weights'] = ops.gu_upsample_fwd(k['xp'], k['ranges'], k['means'], inp['in_lengths'], T)
    return k


def _backward(inp, k, g=None, out_lengths='given'):
    from daft_exprt import ops
    return ops.gu_upsample_bwd(inp['g'] if g is None else g, k['xp'], k['weights'], k['means'], k['ranges'], k['r_pre'], inp['w_range'],
                               inp['in_lengths'], inp['out_lengths'] if out_lengths == 'given' else out_lengths)


def _param_grads(inp, k, d_enc, drin, dr, start):
    ''' the three launches of DaftExprt's backward after the upsampler's; all accumulate into their outputs, which begin at `start` '''
    from daft_exprt import ops
    G = {name: start[name].clone() for name in DPARAMS}
    ops.linear_small_bwd(dr.unsqueeze(2), None, k['rin'], inp['w_range'], G['dw_range'], G['db_range'], need_dx=False)
    ops.scalar_embed_bwd(drin, [inp['dur_float']], [G['dw_dur']], [G['db_dur']])
    ops.scalar_embed_bwd(d_enc, [inp['energy'], inp['pitch']], [G['dw_en'], G['dw_pi']], [G['db_en'], G['db_pi']])
    return G


@functools.lru_cache(maxsize=None)
def _case(name):
    ''' inputs, both restatements and one run of every kernel for a case, shared by the tests and left unchanged '''
    Ls, Ts, knobs = CASES[name]
    c = types.SimpleNamespace(name=name, Ls=Ls, Ts=Ts)
    cpu = U.make_inputs(Ls, Ts, seed=sum(Ts), **knobs)
    c.o32, c.o64 = U.upsample(cpu, torch.float32), U.upsample(cpu, torch.float64)
    c.inp = {k: v.to(DEV) for k, v in cpu.items()}
    c.k = _forward(c.inp)
    c.raw = _forward(c.inp, pos=False)
    c.k['d_enc'], c.k['drin'], c.k['dr'] = _backward(c.inp, c.k)
    c.start = {n: torch.randn_like(c.inp[n[1:]]) * float(c.o64[n].abs().max()) for n in DPARAMS}
    c.k.update(_param_grads(c.inp, c.k, c.k['d_enc'], c.k['drin'], c.k['dr'], {n: torch.zeros_like(s) for n, s in c.start.items()}))
    c.accumulated = _param_grads(c.inp, c.k, c.k['d_enc'], c.k['drin'], c.k['dr'], c.start)
    torch.cuda.synchronize()
    return c


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _check(c, names, got=None, extra=None):
    ''' every tensor of `names` within its bound of the float64 restatement; prints error / bound, asserts after printing '''
    got = c.k if got is None else got
    bad, line = [], []
    for n in names:
        err = float((got[n].double().cpu() - c.o64[n]).abs().max())
        bound = U.bound(c.o32, c.o64, n) + (extra[n] if extra else 0.)
        line.append(f'{n} {err:.2g}/{bound:.2g}')
        if not err <= bound:
            bad.append((n, err, bound))
        if c.name != 'F' and (c.name, n) not in NO_CAP:
            own, top = float((c.o32[n].double() - c.o64[n]).abs().max()), float(c.o64[n].abs().max())
            assert own <= CAP * top, ('fp32 restatement too far from float64: change the inputs', c.name, n, own, top)
    print(f'{c.name}:', '  '.join(line))
    assert not bad, (c.name, bad)


@pytest.mark.parametrize('name', list(CASES))
def test_forward(name):
    c = _case(name)
    assert torch.equal(c.k['totals'].cpu(), c.o64['totals']) and torch.equal(c.k['totals'].cpu(), torch.tensor(c.Ts))
    assert torch.equal(c.k['means'].double().cpu(), c.o64['means'])
    _check(c, ('xp', 'rin', 'r_pre', 'ranges', 'weights', 'dec_in'))
    _check(c, ('weights', 'x_up'), got=c.raw)
    assert _bits_equal(c.k['weights'], c.raw['weights'])
    for b, (Lb, Tb) in enumerate(zip(c.Ls, c.Ts)):
        assert not c.k['weights'][b, Lb:].any(), 'weights of padding phonemes must be exactly 0'
        assert not c.k['dec_in'][b, Tb:].any(), 'decoder input past out_lengths must be exactly 0'


@pytest.mark.parametrize('name', WITH_BACKWARD)
def test_backward(name):
    c = _case(name)
    _check(c, BWD + DPARAMS)
    for b, Lb in enumerate(c.Ls):
        assert not c.k['d_enc'][b, Lb:].any() and not c.k['drin'][b, Lb:].any() and not c.k['dr'][b, Lb:].any()


@pytest.mark.parametrize('name', WITH_BACKWARD)
def test_parameter_gradients_accumulate(name):
    ''' dx_linear_small_bwd and dx_scalar_embed_bwd add to dw / db with one fp32 atomic per workgroup: started from a non-zero
        buffer the result is start + gradient.  Each of those adds rounds a value no larger than |start| + |gradient| once, and
        there are at most B * ceil(L / 64) workgroups (64 rows each), which is what the bound gains over the from-zeros one. '''
    c = _case(name)
    adds = len(c.Ls) * -(-max(c.Ls) // 64)
    extra = {n: adds * 2. ** -24 * (float(c.start[n].abs().max()) + float(c.o64[n].abs().max())) for n in DPARAMS}
    _check(c, DPARAMS, got={n: c.accumulated[n].double() - c.start[n].double() for n in DPARAMS}, extra=extra)


def test_case_e_reaches_both_softplus_branches():
    c = _case('E')
    live = (torch.arange(max(c.Ls))[None, :] < torch.tensor(c.Ls)[:, None])
    r_pre = c.k['r_pre'].cpu()[live]
    above = float((r_pre > 20.).float().mean())
    print('E: share of rows with r_pre > 20:', above, ' min', float(r_pre.min()), ' max', float(r_pre.max()))
    assert 0.2 < above < 0.5 and float(r_pre.min()) < 20.


def test_case_f_backward_is_finite():
    ''' ranges ~ 1e-3: a Gaussian is 0 half a frame from its mean, so every weight is exactly 0 or 1 and the output does not depend
        on sigma -- the true sigma-path gradient is ~0 and what fp32 computes for it (here and in the restatement, which is off by
        1e8 relative) is cancellation noise.  There is no reference to hold that noise to; it must not be inf or NaN. '''
    c = _case('F')
    w = c.k['weights']
    assert bool(((w == 0.) | (w == 1.)).all()) and torch.equal(c.o32['weights'].double(), c.o64['weights'])
    for n in BWD + DPARAMS:
        assert bool(torch.isfinite(c.k[n]).all()), n


def test_upstream_gradient_past_out_lengths_is_never_read():
    c = _case('A')
    g = c.inp['g'].clone()
    for b, Tb in enumerate(c.Ts):
        g[b, Tb:] = float('nan')
    for got, ref in zip(_backward(c.inp, c.k, g=g), (c.k['d_enc'], c.k['drin'], c.k['dr'])):
        assert _bits_equal(got, ref)


def test_backward_without_out_lengths_equals_masked_call():
    c = _case('A')
    g = c.inp['g'].clone()
    for b, Tb in enumerate(c.Ts):
        g[b, Tb:] = 0.
    for got, ref in zip(_backward(c.inp, c.k, g=g, out_lengths=None), (c.k['d_enc'], c.k['drin'], c.k['dr'])):
        assert _bits_equal(got, ref)


def test_backward_reads_no_workspace_element_it_did_not_write(monkeypatch):
    ''' with POISON, `ops._empty` pre-fills dw_ws, dsum_ws and the outputs with NaN: bwd2 must read only the dw elements that bwd1
        wrote (both skip the phonemes / frames whose weight is exactly 0) '''
    from daft_exprt import config
    c = _case('A')
    monkeypatch.setattr(config, 'POISON', True)
    for got, ref in zip(_backward(c.inp, c.k), (c.k['d_enc'], c.k['drin'], c.k['dr'])):
        assert _bits_equal(got, ref)


def test_forward_and_backward_are_reproducible():
    c = _case('A')
    k = _forward(c.inp)
    for n in ('xp', 'rin', 'r_pre', 'ranges', 'means', 'weights', 'dec_in'):
        assert _bits_equal(k[n], c.k[n]), n
    for got, ref in zip(_backward(c.inp, k), (c.k['d_enc'], c.k['drin'], c.k['dr'])):
        assert _bits_equal(got, ref)


def test_an_utterance_does_not_depend_on_its_batch():
    c = _case('A')
    batched = ('enc', 'dur_float', 'dur_int', 'energy', 'pitch', 'in_lengths', 'out_lengths', 'g')
    one = {n: (v[:1].contiguous() if n in batched else v) for n, v in c.inp.items()}
    k = _forward(one)
    k['d_enc'], k['drin'], k['dr'] = _backward(one, k)
    for n in ('xp', 'rin', 'r_pre', 'ranges', 'means', 'weights', 'dec_in') + BWD:
        assert _bits_equal(k[n], c.k[n][:1]), n
