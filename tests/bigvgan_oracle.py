"""Float64 restatement of the BigVGAN generator (Lee et al., ICLR 2023) on the CPU -- the reference every BigVGAN test compares
with (never the code under test).  It is the HiFi-GAN generator of tests/vocoder_oracle.py with every leaky-ReLU replaced by an
anti-aliased periodic activation (upstream's `Activation1d` with ratio 2 and 12-tap Kaiser-sinc filters around `Snake` /
`SnakeBeta`), none in front of the transposed convs, and tanh or a clamp at the end:

    x = conv_pre(mel)
    per stage i:  x = ups.i(x);  x = 1 / nk * sum_j AMPBlock[i * nk + j](x)
    AMPBlock1:    r = r + convs2.m(act[2 m + 1](convs1.m(act[2 m](r))))        AMPBlock2:  r = r + convs.m(act[m](r))
    y = tanh or clamp(conv_post(act_post(x)))

The activation is stated twice: `activation` in the F.pad(mode='replicate') / grouped conv_transpose1d / conv1d form upstream is
written in (as restated from memory: no copy of upstream was at hand), and `activation_loops` as the plain index sums the kernel's
contract gives; tests/test_bigvgan_host.py pins one against the other.  No upstream file was available: the key names, the pad
geometry and the filter formula are a restatement, and the tests prove the kernels against this restatement only.

The generator runs one utterance at a time at its own length and zero-fills past it: replicate padding then lands on the
utterance's own last row, which is what the strict dead-row contract of the kernels equals.  Switches as in vocoder_oracle.generator:
`dtype` (float64 reference / float32 cost of fp32 arithmetic) and `rounding` (weights and every conv's input rounded to bf16; the
activation itself stays unrounded, conv_post is exempt).  The activation's parameters enter in their final form, rounded to fp32
once -- (alpha', 1 / (beta' + 1e-9)) from `final_params` -- and the filter taps as fp32 values, as the kernel receives them.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests import vocoder_oracle as O

FIRST_TAPS = (0.0020289664, 0.0093894639, -0.0255434641, -0.0576573755, 0.1285726091, 0.4432098001)


def kaiser_sinc_filter(cutoff=0.25, half_width=0.3, kernel_size=12):
    ''' the low-pass both resamplers use, float64 (12,): Kaiser window x 2 cutoff sinc(2 cutoff t), t = -5.5 .. 5.5, sum 1 '''
    half = kernel_size // 2
    a = 2.285 * (half - 1) * math.pi * 4. * half_width + 7.95
    beta = 0.1102 * (a - 8.7)                                           # a > 50
    t = np.arange(-half, half) + 0.5
    f = 2. * cutoff * np.kaiser(kernel_size, beta) * np.sinc(2. * cutoff * t)
    return torch.from_numpy(f / f.sum())


def final_params(alpha, beta, logscale):
    ''' raw `alpha` / `beta` (C,) of the checkpoint (beta None: `snake`, beta = alpha) -> (alpha', 1 / (beta' + 1e-9)) fp32 '''
    a = alpha.double().exp() if logscale else alpha.double()
    b = a if beta is None else (beta.double().exp() if logscale else beta.double())
    return a.float(), (1. / (b + 1e-9)).float()


def activation(x, alpha, inv_beta, f_up, f_down):
    ''' x (B, C, n), every row live; alpha, inv_beta (C,); f_up, f_down (12,).  Arithmetic in x.dtype. '''
    dt, c = x.dtype, x.shape[1]
    ku, kd = (f.to(dt).reshape(1, 1, 12).expand(c, 1, 12) for f in (f_up, f_down))
    u = 2. * F.conv_transpose1d(F.pad(x, (5, 5), mode='replicate'), ku, stride=2, groups=c)[..., 15:-15]
    s = u + inv_beta.to(dt)[None, :, None] * torch.sin(alpha.to(dt)[None, :, None] * u) ** 2
    return F.conv1d(F.pad(s, (5, 6), mode='replicate'), kd, stride=2, groups=c)


def activation_loops(x, alpha, inv_beta, f_up, f_down):
    ''' the same as index sums over one utterance, x (C, n) float64 NumPy '''
    c, n = x.shape
    u = np.zeros((c, 2 * n))
    for t in range(2 * n):
        for i in range(n + 10):
            j = t + 15 - 2 * i
            if 0 <= j < 12:
                u[:, t] += f_up[j] * x[:, min(max(i - 5, 0), n - 1)]
    u *= 2.
    s = u + inv_beta[:, None] * np.sin(alpha[:, None] * u) ** 2
    y = np.zeros((c, n))
    for m in range(n):
        for k in range(12):
            y[:, m] += f_down[k] * s[:, min(max(2 * m + k - 5, 0), 2 * n - 1)]
    return y


def fed_convs(cfg):
    ''' [(conv the activation feeds, upstream's name of the activation)] in forward order, `activation_post` last '''
    nk, out = len(cfg['resblock_kernel_sizes']), []
    for i in range(len(cfg['upsample_rates'])):
        for j, dils in enumerate(cfg['resblock_dilation_sizes']):
            block = f'resblocks.{i * nk + j}'
            for m in range(len(dils)):
                if str(cfg['resblock']) == '1':
                    out += [(f'{block}.convs1.{m}', f'{block}.activations.{2 * m}'), (f'{block}.convs2.{m}', f'{block}.activations.{2 * m + 1}')]
                else:
                    out.append((f'{block}.convs.{m}', f'{block}.activations.{m}'))
    return out + [('conv_post', 'activation_post')]


def generator(cfg, weights, acts, filters, mel, lengths, rounding=False, dtype=torch.float64, pre_final=False):
    ''' mel (B, num_mels, T), lengths (B,) int64 -> (B, T * hop) in `dtype`; weights {layer: (w, b)} as vocoder_oracle's, acts
        {conv name: (alpha', inv_beta)} in final form, filters (f_up, f_down) '''
    hop = math.prod(cfg['upsample_rates'])
    out = torch.zeros((mel.shape[0], mel.shape[2] * hop), dtype=dtype)
    nk = len(cfg['resblock_kernel_sizes'])
    kw = dict(slope=1., masks=True, rounding=rounding)
    act = lambda name, v: activation(v, *acts[name], *filters)             # noqa: E731
    for b, t in enumerate(int(v) for v in lengths):
        if t == 0:
            continue
        n = torch.tensor([t])
        x = O.conv(mel[b:b + 1, :, :t].to(dtype), *weights['conv_pre'], 1, n, **kw)
        for i, u in enumerate(cfg['upsample_rates']):
            x = O.upsample(x, *weights[f'ups.{i}'], u, n, **kw)
            n = n * u
            total = None
            for j, dils in enumerate(cfg['resblock_dilation_sizes']):
                r, name = x, f'resblocks.{i * nk + j}'
                for m, d in enumerate(dils):
                    if str(cfg['resblock']) == '1':
                        h = O.conv(act(f'{name}.convs1.{m}', r), *weights[f'{name}.convs1.{m}'], d, n, **kw)
                        r = r + O.conv(act(f'{name}.convs2.{m}', h), *weights[f'{name}.convs2.{m}'], 1, n, **kw)
                    else:
                        r = r + O.conv(act(f'{name}.convs.{m}', r), *weights[f'{name}.convs.{m}'], d, n, **kw)
                total = r if total is None else total + r
            x = total / nk
        w, bias = weights['conv_post']
        bias = bias if cfg.get('use_bias_at_final', True) else torch.zeros_like(bias)
        y = O.post(act('conv_post', x), w, bias, n, slope=1., pre_tanh=True)[0]
        if not pre_final:
            y = torch.tanh(y) if cfg.get('use_tanh_at_final', True) else y.clamp(-1., 1.)
        out[b, :t * hop] = y
    return out


def make_weights(cfg, mel, lengths, seed=0, rms=0.3):
    ''' (weights, raw, acts, filters): conv weights as vocoder_oracle.make_weights draws them; raw {conv name: (alpha, beta or None)}
        as the checkpoint stores them -- N(0, 0.5^2) in log scale, so that the channels differ -- and their final form `acts`;
        conv_post scaled so that the float64 pre-tanh rms over the longest utterance is `rms` '''
    g = torch.Generator().manual_seed(3000 + seed)
    weights = {}
    for name, shape, n_out, fan_in in O.layer_shapes(cfg):
        weights[name] = (torch.randn(shape, generator=g) / math.sqrt(fan_in), 0.05 * torch.randn((n_out,), generator=g))
    logscale, snakebeta = bool(cfg.get('snake_logscale', False)), cfg['activation'] == 'snakebeta'
    raw, acts = {}, {}
    for name, _ in fed_convs(cfg):
        c = weights[name][0].shape[1]
        a, b = 0.5 * torch.randn((c,), generator=g), 0.5 * torch.randn((c,), generator=g)
        if not logscale:
            a, b = a.exp(), b.exp()
        raw[name] = (a, b if snakebeta else None)
        acts[name] = final_params(*raw[name], logscale)
    filters = tuple(kaiser_sinc_filter().float() for _ in range(2))
    w, b = weights['conv_post']
    b = b * 0.1
    weights['conv_post'] = (w, b)
    longest = max(range(len(lengths)), key=lambda i: lengths[i])
    y = generator(cfg, weights, acts, filters, mel[longest:longest + 1, :, :lengths[longest]], [lengths[longest]], pre_final=True)
    weights['conv_post'] = ((w.double() * (rms / float(y.pow(2).mean().sqrt()))).float(), b)
    return weights, raw, acts, filters


def state_dict(cfg, weights, raw, filters=None, form='weight_norm', nested_ups=True, seed=0):
    ''' a BigVGAN generator state dict: the convs in one of vocoder_oracle.FORMS, the transposed convs as `ups.I.0.*` (upstream
        wraps each in a ModuleList) or `ups.I.*`, `...activations.A.act.alpha` / `.act.beta`, `activation_post.act.*`, and with
        `filters` = (f_up, f_down) the buffers `...upsample.filter` / `...downsample.lowpass.filter` (1, 1, 12) of every activation '''
    sd = {}
    for key, v in O.state_dict(weights, form, seed).items():
        if key.startswith('ups.') and nested_ups:
            key = '.'.join(key.split('.')[:2] + ['0'] + key.split('.')[2:])
        if key == 'conv_post.bias' and not cfg.get('use_bias_at_final', True):
            continue
        sd[key] = v
    for conv, name in fed_convs(cfg):
        a, b = raw[conv]
        sd[f'{name}.act.alpha'] = a.clone()
        if b is not None:
            sd[f'{name}.act.beta'] = b.clone()
        if filters is not None:
            sd[f'{name}.upsample.filter'] = filters[0].float().reshape(1, 1, -1).clone()
            sd[f'{name}.downsample.lowpass.filter'] = filters[1].float().reshape(1, 1, -1).clone()
    return sd
