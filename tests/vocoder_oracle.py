"""Float64 restatement of the HiFi-GAN generator (Kong et al. 2020) with per-layer sequence masks, on torch.nn.functional conv
ops on the CPU -- the reference every vocoder test compares with (never the code under test).

    x = conv_pre(mel)
    per stage i:  x = ups.i(leaky_relu(x, 0.1));  x = 1 / nk * sum_j ResBlock[i * nk + j](x)
    y = tanh(conv_post(leaky_relu(x, 0.01)))

Layout here is torch's (B, C, T).  Switches of `generator` and of the single layers:
    masks     every layer's output is zeroed at t >= n[b] (n = lengths x the upsampling so far), which makes a batch row equal to
              the utterance alone (zero padding at every layer); off = the plain padded batch (the mel is zeroed past its length
              either way)
    rounding  the weights and each conv's post-activation input are rounded to bf16, accumulation stays in `dtype`; conv_post is
              exempt (its kernel is fp32 throughout)
    dtype     float64 (the reference) or float32 (what fp32 arithmetic costs on the same input)
Weights travel as {layer name: (weight, bias)} in torch's shapes: Conv1d (Cout, Cin, k), ConvTranspose1d (Cin, Cout, k).
"""
import math

import torch
import torch.nn.functional as F

SMALL = {'resblock': '1', 'upsample_rates': [4, 2], 'upsample_kernel_sizes': [8, 4], 'upsample_initial_channel': 64,
         'resblock_kernel_sizes': [3, 7], 'resblock_dilation_sizes': [[1, 3], [1, 3, 5]], 'num_mels': 80, 'hop_size': 8,
         'sampling_rate': 22050}
V1 = {'resblock': '1', 'upsample_rates': [8, 8, 2, 2], 'upsample_kernel_sizes': [16, 16, 4, 4], 'upsample_initial_channel': 512,
      'resblock_kernel_sizes': [3, 7, 11], 'resblock_dilation_sizes': [[1, 3, 5], [1, 3, 5], [1, 3, 5]], 'num_mels': 80,
      'hop_size': 256, 'sampling_rate': 22050}
# 16- and 8-channel stages (what V2's tail looks like): the VALU kernels, and a k 7 / u 3 stage with phases of unequal length
NARROW = {'resblock': '2', 'upsample_rates': [3, 2], 'upsample_kernel_sizes': [7, 4], 'upsample_initial_channel': 32,
          'resblock_kernel_sizes': [3, 5], 'resblock_dilation_sizes': [[1, 2], [2, 6]], 'num_mels': 80, 'hop_size': 6,
          'sampling_rate': 22050}


def lrelu(x, slope):
    return x if slope == 1. else torch.where(x > 0, x, x * slope)


def rnd(x, rounding):
    return x.float().to(torch.bfloat16).to(x.dtype) if rounding else x


def mask_rows(x, n):
    ''' x (B, C, T) with everything at t >= n[b] replaced by zero (NaN included) '''
    live = torch.arange(x.shape[-1])[None, :] < n[:, None]
    return torch.where(live[:, None, :] if x.dim() == 3 else live, x, torch.zeros((), dtype=x.dtype))


def conv(x, w, b, dilation, n, slope=0.1, masks=True, rounding=False):
    ''' Conv1d(k, dilation, padding dilation (k - 1) / 2) of leaky_relu(x, slope) (slope 1: none) '''
    y = F.conv1d(rnd(lrelu(x, slope), rounding), rnd(w.to(x.dtype), rounding), b.to(x.dtype), dilation=dilation,
                 padding=dilation * (w.shape[2] - 1) // 2)
    return mask_rows(y, n) if masks else y


def upsample(x, w, b, u, n, slope=0.1, masks=True, rounding=False):
    ''' ConvTranspose1d(k, stride u, padding (k - u) / 2) of leaky_relu(x, slope); n counts INPUT rows '''
    y = F.conv_transpose1d(rnd(lrelu(x, slope), rounding), rnd(w.to(x.dtype), rounding), b.to(x.dtype), stride=u,
                           padding=(w.shape[2] - u) // 2)
    return mask_rows(y, n * u) if masks else y


def post(x, w, b, n, slope=0.01, masks=True, pre_tanh=False):
    y = F.conv1d(lrelu(x, slope), w.to(x.dtype), b.to(x.dtype), padding=w.shape[2] // 2)[:, 0]
    y = y if pre_tanh else torch.tanh(y)
    return mask_rows(y, n) if masks else y


def generator(cfg, weights, mel, lengths, masks=True, rounding=False, dtype=torch.float64, pre_tanh=False):
    ''' mel (B, num_mels, T) natural-log mel, lengths (B,) int64 -> (B, T * hop) in `dtype` '''
    kw = dict(masks=masks, rounding=rounding)
    nk, n = len(cfg['resblock_kernel_sizes']), lengths.clone()
    x = mask_rows(mel.to(dtype), n)
    x = conv(x, *weights['conv_pre'], 1, n, slope=1., **kw)
    for i, u in enumerate(cfg['upsample_rates']):
        x = upsample(x, *weights[f'ups.{i}'], u, n, **kw)
        n = n * u
        total = None
        for j, dils in enumerate(cfg['resblock_dilation_sizes']):
            r, name = x, f'resblocks.{i * nk + j}'
            for m, d in enumerate(dils):
                if str(cfg['resblock']) == '1':
                    t = conv(r, *weights[f'{name}.convs1.{m}'], d, n, **kw)
                    r = r + conv(t, *weights[f'{name}.convs2.{m}'], 1, n, **kw)
                else:
                    r = r + conv(r, *weights[f'{name}.convs.{m}'], d, n, **kw)
            total = r if total is None else total + r
        x = total / nk
    return post(x, *weights['conv_post'], n, masks=masks, pre_tanh=pre_tanh)


def layer_shapes(cfg):
    ''' [(name, weight shape, n_out, fan_in)] in forward order '''
    c0, nk = cfg['upsample_initial_channel'], len(cfg['resblock_kernel_sizes'])
    out = [('conv_pre', (c0, cfg['num_mels'], 7), c0, cfg['num_mels'] * 7)]
    for i, (u, k) in enumerate(zip(cfg['upsample_rates'], cfg['upsample_kernel_sizes'])):
        c = c0 >> (i + 1)
        out.append((f'ups.{i}', (c0 >> i, c, k), c, (c0 >> i) * k / u))
        for j, (rk, dils) in enumerate(zip(cfg['resblock_kernel_sizes'], cfg['resblock_dilation_sizes'])):
            for m in range(len(dils)):
                names = [f'convs1.{m}', f'convs2.{m}'] if str(cfg['resblock']) == '1' else [f'convs.{m}']
                out += [(f'resblocks.{i * nk + j}.{nm}', (c, c, rk), c, c * rk) for nm in names]
    c = c0 >> len(cfg['upsample_rates'])
    out.append(('conv_post', (1, c, 7), 1, c * 7))
    return out


def make_mel(cfg, lengths, seed=0, garbage=None):
    ''' a log-mel-like batch (B, num_mels, max length) fp32; columns at or past an utterance's length hold `garbage`
        (default: more random values -- they must not matter) '''
    g = torch.Generator().manual_seed(seed)
    mel = torch.randn((len(lengths), cfg['num_mels'], max(lengths)), generator=g) * 1.5 - 4.
    if garbage is not None:
        for b, t in enumerate(lengths):
            mel[b, :, t:] = garbage
    return mel


def make_weights(cfg, mel, lengths, seed=0, rms=0.3):
    ''' {name: (weight fp32, bias fp32)}: weights N(0, 1 / fan-in), biases N(0, 0.05^2); conv_post scaled so that the float64
        pre-tanh rms over the longest utterance of (mel, lengths) is `rms` (tanh then stays far from saturation) '''
    g = torch.Generator().manual_seed(1000 + seed)
    weights = {}
    for name, shape, n_out, fan_in in layer_shapes(cfg):
        weights[name] = (torch.randn(shape, generator=g) / math.sqrt(fan_in), 0.05 * torch.randn((n_out,), generator=g))
    w, b = weights['conv_post']
    b = b * 0.1
    weights['conv_post'] = (w, b)
    longest = max(range(len(lengths)), key=lambda i: lengths[i])
    n = torch.tensor(lengths[longest:longest + 1], dtype=torch.int64)
    y = generator(cfg, weights, mel[longest:longest + 1, :, :lengths[longest]], n, pre_tanh=True)
    scale = rms / float(y.pow(2).mean().sqrt())
    weights['conv_post'] = ((w.double() * scale).float(), b)
    return weights


FORMS = ('plain', 'weight_norm', 'parametrizations')


def state_dict(weights, form='plain', seed=0):
    ''' a HiFi-GAN generator state dict of these weights: `.weight`, `.weight_g` / `.weight_v`, or
        `.parametrizations.weight.original0` / `original1`; g = ||w|| over every axis but 0 and v = w times a random positive
        factor per slice of axis 0, so g v / ||v|| gives w back to rounding '''
    g = torch.Generator().manual_seed(2000 + seed)
    sd = {}
    for name, (w, b) in weights.items():
        sd[f'{name}.bias'] = b.clone()
        if form == 'plain':
            sd[f'{name}.weight'] = w.clone()
            continue
        norm = w.double().flatten(1).norm(dim=1).reshape(-1, 1, 1)
        v = w.double() * (0.5 + torch.rand((w.shape[0], 1, 1), generator=g).double())
        g_key, v_key = ('.weight_g', '.weight_v') if form == 'weight_norm' else \
            ('.parametrizations.weight.original0', '.parametrizations.weight.original1')
        sd[f'{name}{g_key}'], sd[f'{name}{v_key}'] = norm.float(), v.float()
    return sd
