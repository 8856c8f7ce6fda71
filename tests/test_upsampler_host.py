"""The float64 reference of the upsampler's GPU tests (tests/upsampler_oracle.py) pinned to the reference's arithmetic: run at
float32 it agrees with `oracle.daft_exprt_cpu.gaussian_upsampling` (which the goldens pin) to summation-order noise, and the
gradient it gives for r_pre is the closed form that `gu_upsample_bwd2_kernel` implements."""
import torch

from oracle import daft_exprt_cpu as O
from tests import upsampler_oracle as U

LS, TS = [9, 8, 7], [33, 32, 31]


def test_fp32_restatement_matches_the_model_oracle():
    inp = U.make_inputs(LS, TS, seed=5)
    o32, o64 = U.upsample(inp, torch.float32, grads=False), U.upsample(inp, torch.float64, grads=False)
    pre = 'gaussian_upsampling.'
    P = {pre + 'duration_projection.conv.weight': inp['w_dur'], pre + 'duration_projection.conv.bias': inp['b_dur'],
         pre + 'energy_projection.conv.weight': inp['w_en'], pre + 'energy_projection.conv.bias': inp['b_en'],
         pre + 'pitch_projection.conv.weight': inp['w_pi'], pre + 'pitch_projection.conv.bias': inp['b_pi'],
         pre + 'projection.0.linear_layer.weight': inp['w_range'], pre + 'projection.0.linear_layer.bias': inp['b_range']}
    x_up, weights = O.gaussian_upsampling(P, None, inp['enc'], inp['dur_float'], inp['dur_int'], inp['energy'], inp['pitch'],
                                          inp['in_lengths'])
    assert x_up.shape == o32['x_up'].shape and weights.shape == o32['weights'].shape      # T = the largest total
    for name, ref in (('x_up', x_up), ('weights', weights)):
        err, bound = float((ref - o32[name]).abs().max()), U.bound(o32, o64, name)
        print(f'{name}: |model oracle - fp32 restatement| {err:.3g}  bound {bound:.3g}')
        assert err <= bound, (name, err, bound)
    # the integer part: float32 and float64 carry the same exact values
    d = inp['dur_int']
    excl = torch.cumsum(d, dim=1) - d
    assert torch.equal(o32['means'].double(), o64['means'])
    assert torch.equal(o64['means'] * 2, (d + 2 * excl).double())
    assert torch.equal(o32['totals'], torch.tensor(TS)) and torch.equal(o64['totals'], torch.tensor(TS))


def test_autograd_dr_is_the_kernels_closed_form():
    ''' dr[l] = sum_t w (dw - Dsum) (d^2 / s^3 - 1 / s) * softplus'(r_pre), dw[l,t] = g[t] . x'[l], Dsum[t] = sum_l w dw, d = t + .5 - mu
        (header comment of gu_upsample_bwd2_kernel), in float64 from the forward's outputs alone '''
    inp = U.make_inputs(LS, TS, seed=5)
    o = U.upsample(inp, torch.float64)
    T = inp['g'].shape[1]
    live = torch.arange(T)[None, :] < inp['out_lengths'][:, None]
    g = inp['g'].double() * live.unsqueeze(2)
    w, s, mu = o['weights'], o['ranges'].unsqueeze(2), o['means'].unsqueeze(2)
    dw = o['xp'] @ g.transpose(1, 2)                                   # (B, L, T)
    dsum = (w * dw).sum(dim=1, keepdim=True)
    dlt = torch.arange(T, dtype=torch.float64) + 0.5 - mu
    dsigma = (w * (dw - dsum) * (dlt ** 2 / s ** 3 - 1. / s)).sum(dim=2)
    slope = torch.where(o['r_pre'] > 20., torch.ones_like(o['r_pre']), torch.sigmoid(o['r_pre']))
    dr = dsigma * slope
    err = float((dr - o['dr']).abs().max())
    assert float(o['dr'].abs().max()) > 1e-3                          # a live comparison, not 0 against 0
    assert err <= 1e-12 * float(o['dr'].abs().max()), err
