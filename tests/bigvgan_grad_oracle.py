"""Float64 gradients of BigVGAN's anti-aliased activation and of the whole BigVGAN generator: torch autograd through
tests/bigvgan_oracle.py (`activation`, `final_params`, `generator`), imported unchanged -- the reference every BigVGAN-training test
compares with, never the code under test.  The bf16 form wraps the generator in `vocoder_grad_oracle._rounded_gradients()`:
`bigvgan_oracle.generator` calls `O.conv` / `O.upsample` through the module, so the operand and gradient rounding of the convolutions
applies; the activation itself stays unrounded, forward and backward, as in the kernels.

`snake_grad_loops` states the backward a second time, as the plain index sums of the kernel's contract (K35, `dx_vocoder_snake_bwd`);
tests/test_bigvgan_train_host.py pins it against autograd.  Layout is torch's (B, C, T)."""
import numpy as np
import torch

from tests import bigvgan_oracle as BO
from tests import vocoder_grad_oracle as G
from tests import vocoder_oracle as O


def snake_grad_loops(x, dy, alpha, inv_beta, f_up, f_down):
    ''' one utterance, every row live: x, dy (C, n) float64 NumPy, alpha, inv_beta (C,), f_up, f_down (12,)
        -> (dx (C, n), dalpha (C,), dinv_beta (C,)) by the index sums of the contract '''
    c, n = x.shape
    clamp = lambda i, lo, hi: min(max(i, lo), hi)                      # noqa: E731
    u = np.zeros((c, 2 * n))
    for t in range(2 * n):
        for i in range(n + 10):
            if 0 <= t + 15 - 2 * i < 12:
                u[:, t] += f_up[t + 15 - 2 * i] * x[:, clamp(i - 5, 0, n - 1)]
    u *= 2.
    ds = np.zeros((c, 2 * n))
    for m in range(n):
        for k in range(12):
            ds[:, clamp(2 * m + k - 5, 0, 2 * n - 1)] += f_down[k] * dy[:, m]
    w = 2. * alpha[:, None] * u
    du = ds * (1. + inv_beta[:, None] * alpha[:, None] * np.sin(w))
    dx = np.zeros((c, n))
    for t in range(2 * n):
        for i in range(n + 10):
            if 0 <= t + 15 - 2 * i < 12:
                dx[:, clamp(i - 5, 0, n - 1)] += 2. * f_up[t + 15 - 2 * i] * du[:, t]
    dalpha = (ds * inv_beta[:, None] * u * np.sin(w)).sum(axis=1)
    dinv_beta = (ds * (1. - np.cos(w)) / 2.).sum(axis=1)
    return dx, dalpha, dinv_beta


def snake_grads(x, dy, alpha, inv_beta, taps, dtype=torch.float64, n=None):
    ''' autograd through `bigvgan_oracle.activation`, one utterance at a time at its own length: x, dy (B, C, N), alpha, inv_beta (C,),
        taps = (f_up, f_down), n the live rows per utterance (default: all N)
        -> (dx (B, C, N) with zeros past n[b], dalpha (C,), dinv_beta (C,)), in `dtype`; loss = sum(activation(x) * dy) '''
    B, _, N = x.shape
    n = [N] * B if n is None else [int(v) for v in n]
    a, ib = (t.detach().to(dtype).requires_grad_(True) for t in (alpha, inv_beta))
    dx = torch.zeros(x.shape, dtype=dtype)
    loss = 0.
    leaves = []
    for b, rows in enumerate(n):
        if rows == 0:
            continue
        xb = x[b:b + 1, :, :rows].detach().to(dtype).requires_grad_(True)
        y = BO.activation(xb, a, ib, taps[0], taps[1])
        loss = loss + (y * dy[b:b + 1, :, :rows].to(dtype)).sum()
        leaves.append((b, rows, xb))
    grads = torch.autograd.grad(loss, [xb for _, _, xb in leaves] + [a, ib])
    for (b, rows, _), g in zip(leaves, grads):
        dx[b, :, :rows] = g[0]
    return dx, grads[-2], grads[-1]


def act_keys(cfg):
    ''' {conv the activation feeds: (state-dict key of its raw alpha, of its raw beta or None)} '''
    snakebeta = cfg['activation'] == 'snakebeta'
    return {conv: (f'{name}.act.alpha', f'{name}.act.beta' if snakebeta else None) for conv, name in BO.fed_convs(cfg)}


def final_params_differentiable(alpha, beta, logscale):
    ''' `bigvgan_oracle.final_params` with autograd through it: the same values -- formed in float64, rounded to fp32 once, as the
        kernels receive them -- and the gradient of the unrounded expression (the rounding is passed straight through) '''
    a = alpha.double().exp() if logscale else alpha.double()
    b = a if beta is None else (beta.double().exp() if logscale else beta.double())
    ib = 1. / (b + 1e-9)
    want_a, want_ib = BO.final_params(alpha.detach(), None if beta is None else beta.detach(), logscale)
    return ((a + (want_a.double() - a).detach()).to(alpha.dtype), (ib + (want_ib.double() - ib).detach()).to(alpha.dtype))


def generator_grads(cfg, sd, mel, lengths, proj, rounding=False, dtype=torch.float64):
    ''' sd: a BigVGAN state dict with weight-normed convs (`<layer>.weight_g` / `.weight_v` / `.bias`, `ups.I.*` not nested) and the raw
        `...act.alpha` / `.act.beta`; filter buffers, where present, are used and get no gradient.  loss = sum(generator(mel) * proj).
        Returns (waveform, {parameter name: gradient}, gradient of the mel), all in `dtype` '''
    is_filter = lambda k: k.endswith('.filter')                         # noqa: E731
    params = {k: v.detach().to(dtype).requires_grad_(True) for k, v in sd.items() if not is_filter(k)}
    mel = mel.detach().to(dtype).requires_grad_(True)
    weights = {}
    for name, _, n_out, _ in O.layer_shapes(cfg):
        bias = params.get(f'{name}.bias')
        if bias is None:                                                # use_bias_at_final false: the generator zeroes it anyway
            bias = torch.zeros((n_out,), dtype=dtype)
        weights[name] = (G.normed(params[f'{name}.weight_g'], params[f'{name}.weight_v']), bias)
    logscale = bool(cfg.get('snake_logscale', False))
    acts = {}
    for conv, (ka, kb) in act_keys(cfg).items():
        acts[conv] = final_params_differentiable(params[ka], params[kb] if kb else None, logscale)
    name0 = BO.fed_convs(cfg)[0][1]
    if f'{name0}.upsample.filter' in sd:
        filters = (sd[f'{name0}.upsample.filter'].reshape(-1).float(), sd[f'{name0}.downsample.lowpass.filter'].reshape(-1).float())
    else:
        filters = tuple(BO.kaiser_sinc_filter().float() for _ in range(2))
    with G._rounded_gradients():
        wav = BO.generator(cfg, weights, acts, filters, mel, lengths, rounding=rounding, dtype=dtype)
    names = list(params)
    grads = torch.autograd.grad((wav * proj.to(dtype)).sum(), [params[k] for k in names] + [mel], allow_unused=True)
    out = {k: (g if g is not None else torch.zeros_like(params[k])) for k, g in zip(names, grads[:-1])}
    return wav.detach(), out, grads[-1]
