"""HiFi-GAN generator (Kong et al. 2020, `jik876/hifi-gan` `models.py`) as batched inference on the GPU: the vocoder the
`fine_tune` data set exists to train, from a standard HiFi-GAN checkpoint + `config.json` to waveforms.

    x = conv_pre(mel)                                                   Conv1d(num_mels, C0, 7)
    per stage i:  x = ups.i(leaky_relu(x, 0.1))                         ConvTranspose1d(C0 >> i, C0 >> (i + 1), k, stride u)
                  x = mean_j ResBlock[i * nk + j](x)                    kernels / dilations of the config, type "1" or "2"
    wav = tanh(conv_post(leaky_relu(x, 0.01)))                          Conv1d(C_last, 1, 7)

Weight norm is folded once at load time (float64, plain torch: plumbing); every convolution runs in csrc/vocoder.hip
(`dx_voc_conv`, `dx_voc_upsample`, `dx_voc_post`) on time-major fp32 activations with bf16 or fp32 MFMA operands.  Sequence ends
follow the dead-row contract: every layer treats the rows past an utterance's end as zeros without reading them, so an utterance
gets the same bits alone, in a ragged batch and in any sub-batch.  No CPU fallback: without the HIP library / a GPU this raises.

A config with `"activation": "snake"` or `"snakebeta"` is a BigVGAN generator (Lee et al. 2023; same checkpoint layout): the same
convolutions, with every leaky-ReLU replaced by an anti-aliased periodic activation -- csrc/snake.hip (`dx_vocoder_snake`), one launch
into one more workspace buffer in front of every conv, which then runs with in_slope 1 -- none in front of the transposed convs, and
tanh or a clamp at the end:

    per stage i:  x = ups.i(x);  x = mean_j AMPBlock[i * nk + j](x)     AMPBlock1: r += convs2.m(act[2 m + 1](convs1.m(act[2 m](r))))
    wav = tanh | clamp(conv_post(act_post(x)))                          AMPBlock2: r += convs.m(act[m](r))

Its channel counts are zero-padded to multiples of 32 (zero weights and biases, alpha 1 and 1 / beta 0 on the padding, which
therefore stays exactly zero through every layer), so that the 48- and 24-channel tail of the 1536-channel models runs on MFMA too.
No upstream BigVGAN file or source was at hand when this was written: key names, pad geometry and the filter formula are restated
from the released code from memory and tested against that restatement (tests/bigvgan_oracle.py) only.
"""
import ctypes
import json
import math
import os

import torch

from daft_exprt import _hip as H
from daft_exprt import config as _config

LRELU_SLOPE = 0.1
POST_SLOPE = 0.01           # F.leaky_relu's default in front of conv_post (models.py), not the 0.1 used everywhere else
DEFAULT_WORKSPACE_BYTES = 8 << 30
_CONFIG_LISTS = ('upsample_rates', 'upsample_kernel_sizes', 'resblock_kernel_sizes', 'resblock_dilation_sizes')
_CONFIG_KEYS = ('resblock',) + _CONFIG_LISTS + ('upsample_initial_channel', 'num_mels', 'hop_size', 'sampling_rate')
_ACTIVATIONS = ('snake', 'snakebeta')
FILTER_TAPS = 12            # of the 2x resamplers around BigVGAN's activations (upstream's Activation1d defaults)


def load_config(config):
    ''' a dict, or the path of a HiFi-GAN `config.json` '''
    if isinstance(config, (str, os.PathLike)):
        with open(config, 'r', encoding='utf-8') as f:
            config = json.load(f)
    return dict(config)


def validate_config(cfg):
    ''' raises ValueError naming the offending key '''
    for key in _CONFIG_KEYS:
        if key not in cfg:
            raise ValueError(f'vocoder config: "{key}" is missing')
    if str(cfg['resblock']) not in ('1', '2'):
        raise ValueError(f'vocoder config: "resblock" is {cfg["resblock"]!r}, expected "1" or "2"')
    if cfg.get('activation') is not None and cfg['activation'] not in _ACTIVATIONS:
        raise ValueError(f'vocoder config: "activation" is {cfg["activation"]!r}, expected "snake" or "snakebeta" (a BigVGAN '
                         f'generator) or no such key (HiFi-GAN)')
    for key in _CONFIG_LISTS:
        if not isinstance(cfg[key], (list, tuple)) or len(cfg[key]) == 0:
            raise ValueError(f'vocoder config: "{key}" must be a non-empty list')
    rates, kernels = list(cfg['upsample_rates']), list(cfg['upsample_kernel_sizes'])
    if len(kernels) != len(rates):
        raise ValueError(f'vocoder config: "upsample_kernel_sizes" has {len(kernels)} entries for {len(rates)} "upsample_rates"')
    if len(cfg['resblock_dilation_sizes']) != len(cfg['resblock_kernel_sizes']):
        raise ValueError(f'vocoder config: "resblock_dilation_sizes" has {len(cfg["resblock_dilation_sizes"])} lists for '
                         f'{len(cfg["resblock_kernel_sizes"])} "resblock_kernel_sizes"')
    for k in cfg['resblock_kernel_sizes']:
        if int(k) < 1 or int(k) % 2 == 0:
            raise ValueError(f'vocoder config: "resblock_kernel_sizes" holds {k}: kernels must be odd')
    for dils in cfg['resblock_dilation_sizes']:
        if not isinstance(dils, (list, tuple)) or len(dils) == 0 or any(int(d) < 1 for d in dils):
            raise ValueError(f'vocoder config: "resblock_dilation_sizes" holds {dils!r}: expected lists of dilations >= 1')
    for u, k in zip(rates, kernels):
        if int(u) < 1 or int(k) < int(u) or (int(k) - int(u)) % 2:
            raise ValueError(f'vocoder config: "upsample_kernel_sizes" {k} with rate {u}: need k >= u and k - u even')
    c0 = int(cfg['upsample_initial_channel'])
    if c0 < 1 or c0 % (1 << len(rates)):
        raise ValueError(f'vocoder config: "upsample_initial_channel" {c0} is not divisible by 2^{len(rates)}')
    if int(cfg['num_mels']) < 1:
        raise ValueError(f'vocoder config: "num_mels" is {cfg["num_mels"]}')
    if math.prod(int(u) for u in rates) != int(cfg['hop_size']):
        raise ValueError(f'vocoder config: "hop_size" {cfg["hop_size"]} is not the product of "upsample_rates" {rates}')


def layer_table(cfg):
    ''' [(state-dict name, kind, weight shape, dilation)] in forward order; kind: 'conv' (Cout, Cin, k) or 'up' (Cin, Cout, k) '''
    c0, nk = int(cfg['upsample_initial_channel']), len(cfg['resblock_kernel_sizes'])
    layers = [('conv_pre', 'conv', (c0, int(cfg['num_mels']), 7), 1)]
    for i, (u, k) in enumerate(zip(cfg['upsample_rates'], cfg['upsample_kernel_sizes'])):
        c = c0 >> (i + 1)
        layers.append((f'ups.{i}', 'up', (c0 >> i, c, int(k)), 1))
        for j, (rk, dils) in enumerate(zip(cfg['resblock_kernel_sizes'], cfg['resblock_dilation_sizes'])):
            for m, d in enumerate(dils):
                if str(cfg['resblock']) == '1':
                    layers.append((f'resblocks.{i * nk + j}.convs1.{m}', 'conv', (c, c, int(rk)), int(d)))
                    layers.append((f'resblocks.{i * nk + j}.convs2.{m}', 'conv', (c, c, int(rk)), 1))
                else:
                    layers.append((f'resblocks.{i * nk + j}.convs.{m}', 'conv', (c, c, int(rk)), int(d)))
    layers.append(('conv_post', 'conv', (1, c0 >> len(cfg['upsample_rates']), 7), 1))
    return layers


_NORM_FORMS = (('.weight_g', '.weight_v'), ('.parametrizations.weight.original0', '.parametrizations.weight.original1'))


def folded_weight(state_dict, name):
    ''' the layer's weight as float64: plain `.weight`, or g * v / ||v|| with the norm over every axis but 0 (Cout of a Conv1d,
        Cin of a ConvTranspose1d -- torch's weight_norm default dim=0 on either) '''
    if f'{name}.weight' in state_dict:
        return state_dict[f'{name}.weight'].detach().double().cpu()
    for g_key, v_key in _NORM_FORMS:
        if f'{name}{g_key}' in state_dict and f'{name}{v_key}' in state_dict:
            g, v = state_dict[f'{name}{g_key}'].detach().double().cpu(), state_dict[f'{name}{v_key}'].detach().double().cpu()
            if v.dim() != 3 or g.numel() != v.shape[0]:
                raise ValueError(f'vocoder checkpoint: "{name}{g_key}" has shape {tuple(g.shape)} for a weight of {tuple(v.shape)}')
            return g.reshape(-1, 1, 1) * v / v.flatten(1).norm(dim=1).reshape(-1, 1, 1)
    raise ValueError(f'vocoder checkpoint: "{name}" has neither .weight, .weight_g/.weight_v nor .parametrizations.weight.original0/1')


def folded_state(cfg, state_dict):
    ''' {name: (weight float64, bias float64)} of every layer, shapes checked against the config '''
    out = {}
    for layer, _, shape, _ in layer_table(cfg):
        name = layer
        if is_bigvgan(cfg) and layer.startswith('ups.') and any(key.startswith(f'{layer}.0.') for key in state_dict):
            name = f'{layer}.0'                                     # BigVGAN wraps each transposed conv in a ModuleList
        w = folded_weight(state_dict, name)
        if tuple(w.shape) != shape:
            raise ValueError(f'vocoder checkpoint: "{name}" weight has shape {tuple(w.shape)}, the config gives {shape}')
        n_out = shape[1] if layer.startswith('ups.') else shape[0]
        if layer == 'conv_post' and is_bigvgan(cfg) and not cfg.get('use_bias_at_final', True):
            out[layer] = (w, torch.zeros((n_out,), dtype=torch.float64))
            continue
        if f'{name}.bias' not in state_dict:
            raise ValueError(f'vocoder checkpoint: "{name}.bias" is missing')
        b = state_dict[f'{name}.bias'].detach().double().cpu()
        if tuple(b.shape) != (n_out,):
            raise ValueError(f'vocoder checkpoint: "{name}.bias" has shape {tuple(b.shape)}, expected ({n_out},)')
        out[layer] = (w, b)
    return out


def is_bigvgan(cfg):
    return cfg.get('activation') is not None


def activation_table(cfg):
    ''' [(layer the activation feeds, the activation's state-dict name)] of a BigVGAN generator in forward order: in an AMPBlock1
        activations[2 m] feeds convs1[m] and activations[2 m + 1] convs2[m], in an AMPBlock2 activations[m] feeds convs[m] '''
    out = []
    for layer, _, _, _ in layer_table(cfg):
        if layer.startswith('resblocks.'):
            block, convs, m = layer.rsplit('.', 2)
            a = {'convs1': 2 * int(m), 'convs2': 2 * int(m) + 1, 'convs': int(m)}[convs]
            out.append((layer, f'{block}.activations.{a}'))
    return out + [('conv_post', 'activation_post')]


def kaiser_sinc_filter(cutoff=0.25, half_width=0.3, kernel_size=FILTER_TAPS):
    ''' the low-pass of BigVGAN's 2x resamplers, float64 (kernel_size,): a symmetric Kaiser window (beta from the transition width
        4 half_width) times 2 cutoff sinc(2 cutoff t), t = -(kernel_size - 1) / 2 ..., normalised to sum 1 '''
    half = kernel_size // 2
    a = 2.285 * (half - 1) * math.pi * 4. * half_width + 7.95
    beta = 0.1102 * (a - 8.7)                                         # Kaiser's rule for a > 50 (a = 51.02 here)
    t = torch.arange(-half, half, dtype=torch.float64) + 0.5
    f = 2. * cutoff * torch.kaiser_window(kernel_size, periodic=False, beta=beta, dtype=torch.float64) * torch.sinc(2. * cutoff * t)
    return f / f.sum()


def activation_state(cfg, state_dict, name, channels):
    ''' (alpha', 1 / (beta' + 1e-9), f_up, f_down) of the activation `name`, float64: alpha' = exp(alpha) under `snake_logscale`,
        beta' the same transform of `beta` (`snakebeta`) or alpha' itself (`snake`); the filters are the checkpoint's buffers where
        it has them, `kaiser_sinc_filter()` otherwise '''
    keys = ['alpha', 'beta'] if cfg['activation'] == 'snakebeta' else ['alpha']
    raw = []
    for key in keys:
        if f'{name}.act.{key}' not in state_dict:
            raise ValueError(f'vocoder checkpoint: "{name}.act.{key}" is missing')
        v = state_dict[f'{name}.act.{key}'].detach().double().cpu()
        if tuple(v.shape) != (channels,):
            raise ValueError(f'vocoder checkpoint: "{name}.act.{key}" has shape {tuple(v.shape)}, expected ({channels},)')
        raw.append(v.exp() if cfg.get('snake_logscale', False) else v)
    filters = []
    for key in (f'{name}.upsample.filter', f'{name}.downsample.lowpass.filter'):
        if key in state_dict:
            f = state_dict[key].detach().double().cpu()
            if tuple(f.shape) != (1, 1, FILTER_TAPS):
                raise ValueError(f'vocoder checkpoint: "{key}" has shape {tuple(f.shape)}, expected (1, 1, {FILTER_TAPS})')
            filters.append(f.reshape(-1))
        else:
            filters.append(kaiser_sinc_filter())
    return raw[0], 1. / (raw[-1] + 1e-9), filters[0], filters[1]


def _pad32(c):
    return -(-c // 32) * 32


def pad_layer(name, kind, w, b, shape):
    ''' a BigVGAN layer with its channel counts zero-padded to multiples of 32 -- all but conv_pre's mel bins (`pack_conv_weight`
        pads those) and conv_post's single output: (weight, bias, shape) '''
    cin_axis, cout_axis = (0, 1) if kind == 'up' else (1, 0)
    padded = list(shape)
    if name != 'conv_pre':
        padded[cin_axis] = _pad32(shape[cin_axis])
    if name != 'conv_post':
        padded[cout_axis] = _pad32(shape[cout_axis])
    wp = torch.zeros(padded, dtype=torch.float64)
    wp[:shape[0], :shape[1]] = w
    bp = torch.zeros((padded[cout_axis],), dtype=torch.float64)
    bp[:b.numel()] = b
    return wp, bp, tuple(padded)


def pack_conv_weight(w, dtype, cin_pad=None):
    ''' Conv1d weight (Cout, Cin, k) -> [k][Cout][Cin (zero-padded to cin_pad)] '''
    cout, cin, k = w.shape
    p = torch.zeros((k, cout, cin_pad or cin), dtype=torch.float64)
    p[:, :, :cin] = w.permute(2, 0, 1)
    return p.to(dtype).contiguous()


def pack_upsample_weight(w, u, dtype):
    ''' ConvTranspose1d weight (Cin, Cout, k) -> [u][ceil(k / u)][Cout][Cin]: entry (p, s) is tap j = (p + pad) mod u + s u,
        zeros where j >= k '''
    cin, cout, k = w.shape
    pad, taps = (k - u) // 2, -(-k // u)
    p = torch.zeros((u, taps, cout, cin), dtype=torch.float64)
    for phase in range(u):
        for s in range(taps):
            j = (phase + pad) % u + s * u
            if j < k:
                p[phase, s] = w[:, :, j].t()
    return p.to(dtype).contiguous()


def upsample_tap_table(k, u):
    ''' (tap j of entry (p, s) as a (u, ceil(k / u)) int64 tensor, -1 where j >= k; entry p * taps + s that holds tap j, (k,)) of
        `pack_upsample_weight`'s order: every tap j < k sits in exactly one entry '''
    pad, taps = (k - u) // 2, -(-k // u)
    j = (torch.arange(u)[:, None] + pad) % u + torch.arange(taps)[None, :] * u
    j = torch.where(j < k, j, torch.full_like(j, -1))
    entry = torch.empty((k,), dtype=torch.int64)
    live = j.flatten() >= 0
    entry[j.flatten()[live]] = torch.arange(u * taps)[live]
    return j, entry


def pack_conv_dgrad_weight(w, dtype, cout_pad=None):
    ''' Conv1d weight (Cout, Cin, k) -> [k][Cin (zero-padded to cout_pad)][Cout], taps reversed: `dx_voc_conv` over dy with this
        weight, the same dilation, in_slope 1 and no bias is the convolution's data gradient.  Any device; differentiable. '''
    cout, cin, k = w.shape
    p = w.flip(2).permute(2, 1, 0)
    if cout_pad is not None and cout_pad > cin:
        p = torch.cat([p, p.new_zeros((k, cout_pad - cin, cout))], dim=1)
    return p.to(dtype).contiguous()


def upsample_dgrad_taps(k, u):
    ''' taps of the stride-1 convolution that is ConvTranspose1d(k, stride u)'s data gradient over dy viewed as (B, N, u Cout):
        the smallest odd span symmetric about 0 that holds every row offset s - (p + pad) div u (3 for k = 2 u, 5 for k 7 / u 3) '''
    pad, taps = (k - u) // 2, -(-k // u)
    return 2 * max(taps - 1, (u - 1 + pad) // u) + 1


def pack_upsample_dgrad_weight(w, u, dtype):
    ''' ConvTranspose1d weight (Cin, Cout, k) -> [taps'][Cin][u * Cout], taps' = `upsample_dgrad_taps(k, u)`: row offset
        o = s - (p + pad) div u of column block p holds tap j = (p + pad) mod u + s u, zeros where there is none.  `dx_voc_conv` over
        dy (B, N u, Cout) read as (B, N, u Cout) with this weight, dilation 1, in_slope 1 and no bias is the transposed convolution's
        data gradient.  Any device; differentiable. '''
    cin, cout, k = w.shape
    pad, taps_d = (k - u) // 2, upsample_dgrad_taps(k, u)
    half = taps_d // 2
    o = torch.arange(taps_d)[:, None] - half                       # (taps', 1)
    p = torch.arange(u)[None, :]                                   # (1, u)
    s = o + (p + pad) // u
    j = (p + pad) % u + s * u
    live = (s >= 0) & (j < k)
    j = torch.where(live, j, torch.zeros_like(j)).to(w.device)
    g = w[:, :, j] * live.to(device=w.device, dtype=w.dtype)       # (Cin, Cout, taps', u)
    return g.permute(2, 0, 3, 1).reshape(taps_d, cin, u * cout).to(dtype).contiguous()


def pcm16(wavs):
    ''' [-1, 1] fp32 -> int16 as HiFi-GAN's inference writes it (x 32768, truncated toward zero), saturating instead of wrapping '''
    return (wavs * 32768.).clamp(-32768., 32767.).to(torch.int16)


class Vocoder:
    def __init__(self, config, state_dict, compute_dtype='bf16', device=None):
        ''' config: dict or path of `config.json`; state_dict: the checkpoint's 'generator' entry, in any of the three key forms;
            compute_dtype: 'bf16' (bf16 MFMA operands, fp32 accumulation and residual stream) or 'fp32' (exact fp32 MFMA) '''
        self.config = load_config(config)
        validate_config(self.config)
        if compute_dtype not in ('bf16', 'fp32'):
            raise ValueError(f'compute_dtype is {compute_dtype!r}, expected "bf16" or "fp32"')
        cfg = self.config
        self.compute_dtype = compute_dtype
        self.device = H.device(device)
        self.rates = [int(u) for u in cfg['upsample_rates']]
        self.up_kernels = [int(k) for k in cfg['upsample_kernel_sizes']]
        self.res_kernels = [int(k) for k in cfg['resblock_kernel_sizes']]
        self.res_dilations = [[int(d) for d in dils] for dils in cfg['resblock_dilation_sizes']]
        self.resblock = str(cfg['resblock'])
        self.c0, self.num_mels = int(cfg['upsample_initial_channel']), int(cfg['num_mels'])
        self.hop, self.sampling_rate = int(cfg['hop_size']), int(cfg['sampling_rate'])
        folded = folded_state(cfg, state_dict)
        dt = torch.bfloat16 if compute_dtype == 'bf16' else torch.float32
        self._wdt = H.BF16 if compute_dtype == 'bf16' else H.F32
        self.bigvgan = is_bigvgan(cfg)
        # conv_pre on the MFMA kernel: its input channels (80 mel bins) are zero-padded to a multiple of 32
        self.mel_channels = _pad32(self.num_mels) if self.c0 % 32 == 0 or self.bigvgan else self.num_mels
        # channels of conv_pre's output and of every stage; the activation in front of every conv but conv_pre / the transposed ones
        self._chans = [_pad32(self.c0 >> i) if self.bigvgan else self.c0 >> i for i in range(len(self.rates) + 1)]
        self._slope, self._post_slope = (1., 1.) if self.bigvgan else (LRELU_SLOPE, POST_SLOPE)
        self._final_clamp = self.bigvgan and not cfg.get('use_tanh_at_final', True)
        self._buffers = 7 if self.bigvgan else 6
        self._layers, self._acts = {}, {}
        for name, kind, shape, dil in layer_table(cfg):
            w, b = folded[name]
            if self.bigvgan:
                w, b, shape = pad_layer(name, kind, w, b, shape)
            if name == 'conv_post':
                packed = w[0].t().contiguous().float()                                    # [tap][C] fp32
            elif kind == 'up':
                packed = pack_upsample_weight(w, self.rates[int(name.split('.')[1])], dt)
            else:
                packed = pack_conv_weight(w, dt, self.mel_channels if name == 'conv_pre' else None)
            self._layers[name] = (packed.to(self.device), b.float().to(self.device), shape, dil)
        if self.bigvgan:
            live = {name: shape[1] for name, _, shape, _ in layer_table(cfg)}
            for layer, name in activation_table(cfg):
                alpha, inv_beta, f_up, f_down = activation_state(cfg, state_dict, name, live[layer])
                c = self._layers[layer][2][1]
                a, ib = torch.ones((c,), dtype=torch.float64), torch.zeros((c,), dtype=torch.float64)
                a[:live[layer]], ib[:live[layer]] = alpha, inv_beta
                taps = (ctypes.c_float * (2 * FILTER_TAPS))(*f_up.tolist(), *f_down.tolist())      # host side: kernel arguments
                self._acts[layer] = (a.float().to(self.device), ib.float().to(self.device), taps)
        self._ws = self._act = None

    @classmethod
    def from_checkpoint(cls, path, config=None, compute_dtype='bf16', device=None):
        ''' a `torch.save`d dict whose 'generator' entry is the state dict (HiFi-GAN's `g_XXXXXXXX`); `config` defaults to
            `config.json` beside the checkpoint, as HiFi-GAN lays it out '''
        if config is None:
            config = os.path.join(os.path.dirname(os.path.abspath(path)), 'config.json')
        ckpt = torch.load(path, map_location='cpu', weights_only=False)
        if not isinstance(ckpt, dict) or 'generator' not in ckpt:
            raise ValueError(f'{path}: no "generator" entry (expected a HiFi-GAN generator checkpoint)')
        return cls(config, ckpt['generator'], compute_dtype=compute_dtype, device=device)

    def check_hparams(self, hparams):
        ''' raises ValueError unless the vocoder was trained on this front-end's mels '''
        if math.prod(self.rates) != int(hparams.hop_length):
            raise ValueError(f'vocoder "upsample_rates" {self.rates} multiply to {math.prod(self.rates)}, hparams.hop_length is {hparams.hop_length}')
        if self.num_mels != int(hparams.n_mel_channels):
            raise ValueError(f'vocoder "num_mels" is {self.num_mels}, hparams.n_mel_channels is {hparams.n_mel_channels}')
        if self.sampling_rate != int(hparams.sampling_rate):
            raise ValueError(f'vocoder "sampling_rate" is {self.sampling_rate}, hparams.sampling_rate is {hparams.sampling_rate}')

    # ---- launches ---------------------------------------------------------------------------------------------------------
    def _fed(self, name, x, n):
        ''' what the layer `name` reads: x itself (HiFi-GAN: the leaky-ReLU is applied as the conv stages its input), or BigVGAN's
            activation of x, written to the workspace's seventh buffer '''
        if not self.bigvgan:
            return x
        alpha, inv_beta, taps = self._acts[name]
        B, N, c = x.shape
        y = self._act[:B * N * c].view(B, N, c)
        H.check(H.lib().dx_vocoder_snake(H.ptr(x), c, H.ptr(alpha), H.ptr(inv_beta), ctypes.addressof(taps), H.ptr(y), c, H.ptr(n), B, N, c,
                                         H.stream()))
        return y

    def _conv(self, name, x, y, n, res=None, acc=None, acc_scale=0., acc_init=False, slope=None):
        w, b, (cout, cin, k), dil = self._layers[name]
        B, N, ldx = x.shape
        slope = self._slope if slope is None else slope
        H.check(H.lib().dx_voc_conv(H.ptr(x), ldx, H.ptr(w), self._wdt, H.ptr(b), H.ptr(res), cout, H.ptr(y), cout, H.ptr(acc), cout,
                                    float(acc_scale), int(acc_init), H.ptr(n), B, N, w.shape[2], cout, k, dil, float(slope), H.stream()))

    def _upsample(self, name, x, y, n, u):
        w, b, (cin, cout, k), _ = self._layers[name]
        B, N, _ = x.shape
        H.check(H.lib().dx_voc_upsample(H.ptr(x), cin, H.ptr(w), self._wdt, H.ptr(b), H.ptr(y), cout, H.ptr(n), B, N, cin, cout, k, u,
                                        self._slope, H.stream()))

    def _post(self, x, out, n):
        w, bias, _, _ = self._layers['conv_post']
        B, N, c = x.shape
        post = H.lib().dx_vocoder_post_clamp if self._final_clamp else H.lib().dx_voc_post
        H.check(post(H.ptr(x), c, H.ptr(w), H.ptr(bias), H.ptr(out), out.stride(0), H.ptr(n), B, N, c, 7, self._post_slope, H.stream()))

    def _elements_per_utterance(self, T):
        ''' (floats of the largest activation of one utterance of T frames, floats of its padded mel) '''
        rows, most = T, T * self._chans[0]
        for i, u in enumerate(self.rates):
            rows *= u
            most = max(most, rows * self._chans[i + 1])
        return most, T * self.mel_channels

    def _run(self, mel, lengths, out, T):
        ''' one sub-batch: mel (b, num_mels, >= T), lengths (b,) clamped to [0, T], out (b, >= T * hop) '''
        b = mel.shape[0]
        most, mel_el = self._elements_per_utterance(T)
        nb = self._buffers
        need = b * (nb * most + mel_el)
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.float32, device=self.device)
        if _config.POISON:
            self._ws.fill_(float('nan'))
        bufs = [self._ws[i * b * most:(i + 1) * b * most] for i in range(nb)]
        melt = self._ws[nb * b * most:need].view(b, T, self.mel_channels)
        melt[:, :, :self.num_mels] = mel[:, :, :T].transpose(1, 2)
        if self.mel_channels > self.num_mels:
            melt[:, :, self.num_mels:] = 0.
        view = lambda buf, rows, c: buf[:b * rows * c].view(b, rows, c)      # noqa: E731
        x, up, ping, pong, tmp, total = bufs[:6]
        self._act = bufs[6] if self.bigvgan else None
        rows, c, n = T, self._chans[0], lengths
        xv = view(x, rows, c)
        self._conv('conv_pre', melt, xv, n, slope=1.)
        nk = len(self.res_kernels)
        for i, u in enumerate(self.rates):
            c_out = self._chans[i + 1]
            upv = view(up, rows * u, c_out)
            self._upsample(f'ups.{i}', xv, upv, n, u)
            rows, c, n = rows * u, c_out, n * u
            tv, sv = view(tmp, rows, c), view(total, rows, c)
            for j, dils in enumerate(self.res_dilations):
                cur, block = upv, f'resblocks.{i * nk + j}'
                for m in range(len(dils)):
                    nxt = view(ping if cur.data_ptr() != ping.data_ptr() else pong, rows, c)
                    last = m == len(dils) - 1
                    tail = dict(res=cur, acc=sv if last else None, acc_scale=1. / nk, acc_init=j == 0)
                    if self.resblock == '1':
                        self._conv(f'{block}.convs1.{m}', self._fed(f'{block}.convs1.{m}', cur, n), tv, n)
                        self._conv(f'{block}.convs2.{m}', self._fed(f'{block}.convs2.{m}', tv, n), None if last else nxt, n, **tail)
                    else:
                        self._conv(f'{block}.convs.{m}', self._fed(f'{block}.convs.{m}', cur, n), None if last else nxt, n, **tail)
                    cur = nxt
            x, total = total, x
            xv = view(x, rows, c)
        self._post(self._fed('conv_post', xv, n), out, n)

    def __call__(self, mel, lengths, max_workspace_bytes=DEFAULT_WORKSPACE_BYTES):
        ''' mel (B, num_mels, T) natural-log mel on the device (what `inference` returns as `decoder_preds[0]`; columns at or
            past `lengths` may hold anything, they are not read), lengths (B,) int64.
            Returns (wavs (B, T * hop) fp32 in [-1, 1] with zeros past n_samples, n_samples = lengths * hop (B,) int64).
            The activations of the last stage are large (about 8 GB for one fp32 tensor at B = 256, T = 950), so the batch is
            walked in sub-batches whose workspace -- six activation buffers of the largest stage (seven for a BigVGAN generator:
            one more for its activations' output) plus the padded mel -- stays
            under `max_workspace_bytes` (default 8 GB; one utterance at a time when even that does not fit).  The workspace is
            kept and reused across calls; results do not depend on the split. '''
        H.require_gpu(mel, lengths)
        if mel.dim() != 3 or mel.shape[1] != self.num_mels:
            raise ValueError(f'mel has shape {tuple(mel.shape)}, expected (B, {self.num_mels}, T)')
        if lengths.dtype != torch.int64 or lengths.shape != (mel.shape[0],):
            raise ValueError(f'lengths must be int64 of shape ({mel.shape[0]},)')
        B, _, T = mel.shape
        mel = mel.float()
        lengths = lengths.clamp(0, T)
        host = lengths.tolist()
        wavs = torch.zeros((B, T * self.hop), dtype=torch.float32, device=mel.device)
        with torch.cuda.device(mel.device):
            b0 = 0
            while b0 < B:
                b1, t_sub = b0, 1
                while b1 < B:                                             # greedy: as many utterances as fit under the cap
                    t_new = max(t_sub, host[b1])
                    most, mel_el = self._elements_per_utterance(t_new)
                    if b1 > b0 and 4 * (b1 + 1 - b0) * (self._buffers * most + mel_el) > max_workspace_bytes:
                        break
                    b1, t_sub = b1 + 1, t_new
                self._run(mel[b0:b1], lengths[b0:b1].contiguous(), wavs[b0:b1], t_sub)
                b0 = b1
        return wavs, lengths * self.hop
