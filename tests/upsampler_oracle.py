"""Plain-torch restatement of the Gaussian upsampler (the length regulator) with its gradients by autograd, and a builder of
padded input batches for it.  CPU only, no project imports: the HIP kernels of csrc/upsample.hip are compared against THIS at
float64, and the distance between its float32 and float64 runs on the same inputs sets the tolerance.

    x'      = enc + conv3(energy) + conv3(pitch)                    1 -> C channels, three taps, zero "same" padding
    rin     = x' + conv3(dur_float)
    r_pre   = rin . w_range + b_range;   range = softplus(r_pre), 1 at pad l
    mu_l    = d_l / 2 + sum_{j<l} d_j                               d = int64 durations, summed as integers
    p[l,t]  = exp(-(t + .5 - mu_l)^2 / (2 range_l^2) - log range_l - log sqrt(2 pi)), 0 at pad l
    w[l,t]  = p[l,t] / (sum_l p[l,t] + 1e-20)
    x_up[t] = sum_l w[l,t] x'_l;   dec_in = (x_up + pos) masked by out_lengths
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

C = 128
EPS = 1e-20
PARAMS = ('w_range', 'b_range', 'w_dur', 'b_dur', 'w_en', 'b_en', 'w_pi', 'b_pi')


def make_inputs(Ls, Ts, seed, b_range_shift=0., w_range_scale=1.):
    ''' float32 / int64 inputs for utterances of L_b phonemes and T_b frames, padded to (max L, max T).  Durations are drawn by
        throwing T_b frames at L_b phonemes (zero durations occur); energy and pitch are zero where the duration is zero;
        everything past L_b is zero.  The projections are drawn like torch's default init (uniform, +-1/sqrt(fan_in)), then
        w_range is scaled and b_range shifted; `pos` is the sinusoid table, `g` an upstream gradient for dec_in. '''
    rng = np.random.RandomState(seed)
    B, L, T = len(Ls), max(max(Ls), 1), max(max(Ts), 1)
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    dur = np.zeros((B, L), dtype=np.int64)
    enc, energy, pitch = np.zeros((B, L, C)), np.zeros((B, L)), np.zeros((B, L))
    for b, (Lb, Tb) in enumerate(zip(Ls, Ts)):
        for _ in range(Tb):
            dur[b, rng.randint(0, Lb)] += 1
        enc[b, :Lb] = rng.randn(Lb, C)
        energy[b, :Lb] = rng.randn(Lb) * (dur[b, :Lb] > 0)
        pitch[b, :Lb] = rng.randn(Lb) * (dur[b, :Lb] > 0)
    uni = lambda fan_in, *shape: rng.uniform(-1., 1., shape) / math.sqrt(fan_in)
    inp = {'enc': f32(enc), 'dur_int': torch.from_numpy(dur), 'dur_float': f32(dur * 256. / 22050.), 'energy': f32(energy),
           'pitch': f32(pitch), 'in_lengths': torch.tensor(Ls, dtype=torch.int64), 'out_lengths': torch.tensor(Ts, dtype=torch.int64)}
    for name in ('dur', 'en', 'pi'):
        inp['w_' + name], inp['b_' + name] = f32(uni(3, C, 1, 3)), f32(uni(3, C))
    inp['w_range'], inp['b_range'] = f32(uni(C, 1, C) * w_range_scale), f32(uni(C, 1) + b_range_shift)
    pos = np.arange(T, dtype=np.float64)[:, None] * np.exp(np.arange(0, C, 2) * (-math.log(10000.) / C))[None, :]
    inp['pos'] = f32(np.stack([np.sin(pos), np.cos(pos)], axis=2).reshape(T, C))
    inp['g'] = f32(rng.randn(B, T, C))
    return inp


def _conv3(feat, w, b):
    ''' (B, L) scalar feature -> (B, L, C): out[l, c] = w[c, 0] f[l-1] + w[c, 1] f[l] + w[c, 2] f[l+1] + b[c], zeros outside [0, L) '''
    f = F.pad(feat, (1, 1))
    return f[:, :-2, None] * w[:, 0, 0] + f[:, 1:-1, None] * w[:, 0, 1] + f[:, 2:, None] * w[:, 0, 2] + b


def upsample(inp, dtype, grads=True):
    ''' every intermediate and output of the upsampler on T = inp['g'].shape[1] frames, computed in `dtype` from the float32 inputs
        (means and totals from int64), as a dict; with `grads`, also the gradients of sum(dec_in * g): d_enc (= the gradient of
        x'), drin, dr (of r_pre) and the eight projection parameters as 'd' + name. '''
    f = lambda name: inp[name].to(dtype)
    P = {name: f(name).requires_grad_(grads) for name in PARAMS}
    enc = f('enc').requires_grad_(grads)
    B, L, _ = enc.shape
    T = inp['g'].shape[1]
    pad = torch.arange(L)[None, :] >= inp['in_lengths'][:, None]
    xp = enc + _conv3(f('energy'), P['w_en'], P['b_en']) + _conv3(f('pitch'), P['w_pi'], P['b_pi'])
    rin = xp + _conv3(f('dur_float'), P['w_dur'], P['b_dur'])
    r_pre = (rin @ P['w_range'].t() + P['b_range']).squeeze(2)
    ranges = F.softplus(r_pre).masked_fill(pad, 1.)
    d = inp['dur_int']
    csum = torch.cumsum(d, dim=1)
    means = (d.to(dtype) / 2 + (csum - d).to(dtype)).detach()
    t = torch.arange(T, dtype=dtype) + 0.5
    mu, sigma = means.unsqueeze(2), ranges.unsqueeze(2)
    logp = -((t - mu) ** 2) / (2 * sigma ** 2) - sigma.log() - math.log(math.sqrt(2 * math.pi))
    p = torch.exp(logp).masked_fill(pad.unsqueeze(2), 0.)
    weights = p / (p.sum(dim=1, keepdim=True) + EPS)
    x_up = weights.transpose(1, 2) @ xp
    live = (torch.arange(T)[None, :] < inp['out_lengths'][:, None]).unsqueeze(2)
    dec_in = (x_up + f('pos')[:T]).masked_fill(~live, 0.)
    out = {'xp': xp, 'rin': rin, 'r_pre': r_pre, 'ranges': ranges, 'means': means, 'totals': csum[:, -1], 'weights': weights,
           'x_up': x_up, 'dec_in': dec_in}
    if grads:
        wrt = [enc, rin, r_pre] + [P[name] for name in PARAMS]
        got = torch.autograd.grad((dec_in * f('g')).sum(), wrt)
        out.update(zip(['d_enc', 'drin', 'dr'] + ['d' + name for name in PARAMS], got))
    return {k: v.detach() for k, v in out.items()}


def bound(o32, o64, name):
    ''' absolute tolerance for a float32 kernel's `name` against the float64 run: four times the float32 restatement's own
        distance from it (a different summation order and a few ulp of expf / logf), plus 1e-6 of the tensor's largest element '''
    return 4. * float((o32[name].double() - o64[name]).abs().max()) + 1e-6 * float(o64[name].abs().max())
