"""Fine-tuning of the HiFi-GAN vocoder (Kong et al. 2020) on the GPU: from a `fine_tune` data set and a pretrained `g_` / `do_`
pair to the `g_XXXXXXXX` file `Vocoder.from_checkpoint` reads.  A BigVGAN generator (a config with an `activation`) trains through
`daft_exprt/bigvgan_train.py`, which adds the activation's backward (K35) to what is here; `trainable_generator` picks the class, and
the discriminators, losses, sampler, checkpoints and `fine_tune_vocoder` below serve both families.

The generator trains on the kernels it is run with (`daft_exprt/vocoder.py`, K24), under their numerical contract -- dead rows past
each utterance, bf16 or fp32 operands, fp32 accumulation:
    forward          `dx_voc_conv` / `dx_voc_upsample`
    data gradients   `dx_voc_conv` over dy with re-packed weights (`vocoder.pack_conv_dgrad_weight`, `pack_upsample_dgrad_weight`)
    weight gradients `dx_vocoder_wgrad` / `dx_vocoder_upsample_wgrad` (K33, csrc/vocoder_train.hip)
Bias gradients, the leaky-ReLU gates, the residual sums and conv_post's backward are torch pointwise ops and reductions on the device;
none of them depends on what a tensor holds at or past an utterance's end.  Weight norm (g v / ||v||) is formed by torch ops in
float64 and rounded once (the fold of the inference path, so the two forwards agree bit for bit), and autograd carries dW to g and v.  The discriminators (multi-period, multi-scale), the losses and the loss mel are plain torch,
restated from the paper.  No CPU fallback for the generator: without the HIP library / a GPU it raises.
"""
import json
import logging
import math
import os
import time
import warnings
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from daft_exprt import _hip as H
from daft_exprt import config as _config
from daft_exprt import vocoder as V

_logger = logging.getLogger(__name__)
_TDT = {'bf16': torch.bfloat16, 'fp32': torch.float32}
_WDT = {'bf16': H.BF16, 'fp32': H.F32}


# ---- launches -------------------------------------------------------------------------------------------------------------------

_WS = {}       # device -> the weight gradients' workspace (grown on demand, reused)


def _workspace(n_bytes, device):
    ws = _WS.get(device)
    if ws is None or ws.numel() * 4 < n_bytes:
        _WS[device] = None
        ws = _WS[device] = torch.empty((n_bytes + 3) // 4, dtype=torch.float32, device=device)
    if _config.POISON:
        ws.fill_(float('nan'))
    return ws


def _check_rows(x, n, what):
    H.require_gpu(x, n)
    if x.dtype != torch.float32 or x.dim() != 3 or not x.is_contiguous():
        raise ValueError(f'{what}: expected a contiguous fp32 (B, N, C) tensor, got {x.dtype} {tuple(x.shape)}')
    if n.dtype != torch.int64 or n.shape != (x.shape[0],):
        raise ValueError(f'{what}: n_rows must be int64 of shape ({x.shape[0]},)')


def pack_conv_weight(w, dtype, cin_pad=None):
    ''' `vocoder.pack_conv_weight` on any device, differentiable: (Cout, Cin, k) -> [k][Cout][Cin (zero-padded to cin_pad)] '''
    cout, cin, k = w.shape
    p = w.permute(2, 0, 1)
    if cin_pad is not None and cin_pad > cin:
        p = torch.cat([p, p.new_zeros((k, cout, cin_pad - cin))], dim=2)
    return p.to(dtype).contiguous()


def pack_upsample_weight(w, u, dtype):
    ''' `vocoder.pack_upsample_weight` on any device, differentiable: (Cin, Cout, k) -> [u][ceil(k / u)][Cout][Cin] '''
    j, _ = V.upsample_tap_table(w.shape[2], u)
    live = (j >= 0).to(device=w.device, dtype=w.dtype)
    g = w[:, :, j.clamp(min=0).to(w.device)] * live                 # (Cin, Cout, u, taps)
    return g.permute(2, 3, 1, 0).to(dtype).contiguous()


def conv_forward(x, wp, bias, n, cout, k, dilation, slope, compute_dtype):
    ''' `dx_voc_conv`: x (B, N, Cin) time-major fp32, wp [k][Cout][Cin] in the operand type -> (B, N, Cout) '''
    _check_rows(x, n, 'conv_forward')
    B, N, cin = x.shape
    y = torch.empty((B, N, cout), dtype=torch.float32, device=x.device)
    H.check(H.lib().dx_voc_conv(H.ptr(x), cin, H.ptr(wp), _WDT[compute_dtype], H.ptr(bias), None, cout, H.ptr(y), cout, None, cout, 0., 0,
                                H.ptr(n), B, N, cin, cout, k, dilation, float(slope), H.stream()))
    return y


def conv_wgrad(x, dy, n, k, dilation, slope, compute_dtype):
    ''' `dx_vocoder_wgrad`: x (B, N, Cin), dy (B, N, Cout) -> dW [k][Cout][Cin] fp32 '''
    _check_rows(x, n, 'conv_wgrad')
    _check_rows(dy, n, 'conv_wgrad')
    B, N, cin = x.shape
    cout = dy.shape[2]
    dw = torch.empty((k, cout, cin), dtype=torch.float32, device=x.device)
    ws = _workspace(int(H.lib().dx_vocoder_wgrad_workspace(B, N, cin, cout, k, 1)), x.device)
    H.check(H.lib().dx_vocoder_wgrad(H.ptr(x), cin, H.ptr(dy), cout, _WDT[compute_dtype], H.ptr(dw), H.ptr(ws), H.ptr(n), B, N, cin, cout, k,
                                 dilation, float(slope), H.stream()))
    return dw


def upsample_forward(x, wp, bias, n, cout, k, u, slope, compute_dtype):
    ''' `dx_voc_upsample`: x (B, N, Cin), wp [u][ceil(k / u)][Cout][Cin] -> (B, N u, Cout) '''
    _check_rows(x, n, 'upsample_forward')
    B, N, cin = x.shape
    y = torch.empty((B, N * u, cout), dtype=torch.float32, device=x.device)
    H.check(H.lib().dx_voc_upsample(H.ptr(x), cin, H.ptr(wp), _WDT[compute_dtype], H.ptr(bias), H.ptr(y), cout, H.ptr(n), B, N, cin, cout,
                                    k, u, float(slope), H.stream()))
    return y


def upsample_dgrad(dy, wd, n, cin, u, compute_dtype):
    ''' the transposed convolution's data gradient: `dx_voc_conv` over dy (B, N u, Cout) read as (B, N, u Cout) with
        wd = `vocoder.pack_upsample_dgrad_weight` -> (B, N, Cin), before the gate of the forward's leaky-ReLU '''
    B, rows, cout = dy.shape
    return conv_forward(dy.view(B, rows // u, u * cout), wd, None, n, cin, wd.shape[0], 1, 1., compute_dtype)


def upsample_wgrad(x, dy, n, k, u, slope, compute_dtype):
    ''' `dx_vocoder_upsample_wgrad`: x (B, N, Cin), dy (B, N u, Cout) -> dW [u][ceil(k / u)][Cout][Cin] fp32 '''
    _check_rows(x, n, 'upsample_wgrad')
    _check_rows(dy, n, 'upsample_wgrad')
    B, N, cin = x.shape
    cout = dy.shape[2]
    if dy.shape[1] != N * u:
        raise ValueError(f'upsample_wgrad: dy has {dy.shape[1]} rows for {N} x {u}')
    dw = torch.empty((u, -(-k // u), cout, cin), dtype=torch.float32, device=x.device)
    ws = _workspace(int(H.lib().dx_vocoder_wgrad_workspace(B, N, cin, cout, k, u)), x.device)
    H.check(H.lib().dx_vocoder_upsample_wgrad(H.ptr(x), cin, H.ptr(dy), cout, _WDT[compute_dtype], H.ptr(dw), H.ptr(ws), H.ptr(n), B, N, cin,
                                          cout, k, u, float(slope), H.stream()))
    return dw


def _live(n, rows, device):
    ''' (B, rows, 1) bool: row t of utterance b is below n[b] '''
    return (torch.arange(rows, device=device)[None, :] < n[:, None])[:, :, None]


def _gate(x, dx_act, slope):
    ''' the leaky-ReLU's backward; a dead row of dx_act is zero and stays zero whatever x holds there '''
    return dx_act if slope == 1. else torch.where(x > 0, dx_act, dx_act * slope)


def _bias_grad(dy, live):
    return torch.where(live, dy, dy.new_zeros(())).sum(dim=(0, 1))


class _Conv(torch.autograd.Function):
    ''' Conv1d(k, dilation, "same")(leaky_relu(x, slope)) + bias over time-major rows; w (Cout, Cin, k) in torch's layout, its input
        channels zero-padded to x's '''
    @staticmethod
    def forward(ctx, x, w, bias, n, dilation, slope, compute_dtype):
        x = x.contiguous()
        cout, _, k = w.shape
        ctx.save_for_backward(x, w, n)
        ctx.meta = (dilation, slope, compute_dtype)
        return conv_forward(x, pack_conv_weight(w, _TDT[compute_dtype], x.shape[2]), bias, n, cout, k, dilation, slope, compute_dtype)

    @staticmethod
    def backward(ctx, dy):
        x, w, n = ctx.saved_tensors
        dilation, slope, dt = ctx.meta
        dy = dy.contiguous()
        cout, cin, k = w.shape
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            wd = V.pack_conv_dgrad_weight(w, _TDT[dt], x.shape[2])
            dx = _gate(x, conv_forward(dy, wd, None, n, x.shape[2], k, dilation, 1., dt), slope)
        if ctx.needs_input_grad[1]:
            dw = conv_wgrad(x, dy, n, k, dilation, slope, dt).permute(1, 2, 0)[:, :cin]
        if ctx.needs_input_grad[2]:
            db = _bias_grad(dy, _live(n, dy.shape[1], dy.device))
        return dx, dw, db, None, None, None, None


class _Upsample(torch.autograd.Function):
    ''' ConvTranspose1d(k, stride u, padding (k - u) / 2)(leaky_relu(x, slope)) + bias; w (Cin, Cout, k) '''
    @staticmethod
    def forward(ctx, x, w, bias, n, u, slope, compute_dtype):
        x = x.contiguous()
        _, cout, k = w.shape
        ctx.save_for_backward(x, w, n)
        ctx.meta = (u, slope, compute_dtype)
        return upsample_forward(x, pack_upsample_weight(w, u, _TDT[compute_dtype]), bias, n, cout, k, u, slope, compute_dtype)

    @staticmethod
    def backward(ctx, dy):
        x, w, n = ctx.saved_tensors
        u, slope, dt = ctx.meta
        dy = dy.contiguous()
        cin, cout, k = w.shape
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = _gate(x, upsample_dgrad(dy, V.pack_upsample_dgrad_weight(w, u, _TDT[dt]), n, cin, u, dt), slope)
        if ctx.needs_input_grad[1]:
            _, entry = V.upsample_tap_table(k, u)
            dw = upsample_wgrad(x, dy, n, k, u, slope, dt).permute(3, 2, 0, 1).reshape(cin, cout, -1)[:, :, entry.to(dy.device)]
        if ctx.needs_input_grad[2]:
            db = _bias_grad(dy, _live(n * u, dy.shape[1], dy.device))
        return dx, dw, db, None, None, None, None


class _Post(torch.autograd.Function):
    ''' tanh(Conv1d(C, 1, 7)(leaky_relu(x, 0.01)) + bias): `dx_voc_post` forward (fp32 throughout, one output channel, 0.01 of the
        generator's work); its backward is torch: seven shifted products for dx, seven contractions for dW '''
    @staticmethod
    def forward(ctx, x, w, bias, n):
        x = x.contiguous()
        _check_rows(x, n, 'conv_post')
        B, N, c = x.shape
        y = torch.empty((B, N), dtype=torch.float32, device=x.device)
        wp = w[0].t().contiguous().float()
        H.check(H.lib().dx_voc_post(H.ptr(x), c, H.ptr(wp), H.ptr(bias), H.ptr(y), N, H.ptr(n), B, N, c, w.shape[2], V.POST_SLOPE,
                                    H.stream()))
        ctx.save_for_backward(x, w, n, y)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, n, y = ctx.saved_tensors
        B, N, _ = x.shape
        k = w.shape[2]
        h = k // 2
        live = _live(n, N, x.device)
        # the sums over every sample of the batch (dW, db) are taken in float64: one output channel, no MFMA to feed
        dpre64 = torch.where(live[:, :, 0], dy.double() * (1. - y.double() ** 2), dy.new_zeros((), dtype=torch.float64))
        dpre = dpre64.float()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            padded = F.pad(dpre, (h, h))
            acc = None
            for j in range(k):                                      # dx_act[t] = sum_j dpre[t - j + h] w[j], j ascending
                term = padded[:, 2 * h - j:2 * h - j + N, None] * w[0, :, j]
                acc = term if acc is None else acc + term
            dx = torch.where(live, _gate(x, acc, V.POST_SLOPE), acc.new_zeros(()))
        if ctx.needs_input_grad[1]:
            # dW[c, j] = sum_r dpre[r - j + h] lrelu(x)[r, c]: the (B, N) gradient is shifted, x stays in place -- one GEMM
            xa = torch.where(live, torch.where(x > 0, x, x * V.POST_SLOPE), x.new_zeros(())).double()
            padded = F.pad(dpre64, (h, h))
            shifts = torch.stack([padded[:, 2 * h - j:2 * h - j + N] for j in range(k)], dim=2)
            dw = (shifts.reshape(B * N, k).t() @ xa.reshape(B * N, -1)).t()[None].float()
        if ctx.needs_input_grad[2]:
            db = dpre64.sum().float().reshape(1)
        return dx, dw, db, None


# ---- the generator ----------------------------------------------------------------------------------------------------------------

class _WeightNormed(nn.Module):
    ''' the parameters of one weight-normed convolution under HiFi-GAN's names: weight_g (dim 0, 1, 1), weight_v, bias '''
    def __init__(self, w, b):
        super().__init__()
        w = w.double()
        g = w.flatten(1).norm(dim=1).reshape(-1, 1, 1)
        self.weight_g = nn.Parameter(g.float())
        self.weight_v = nn.Parameter(w.float())
        self.bias = nn.Parameter(b.float())

    def weight(self):
        ''' g v / ||v|| formed in float64 and rounded once, as the inference path folds it; autograd carries dW to g and v through
            the same float64 ops '''
        v = self.weight_v.double()
        return (self.weight_g.double() * v / v.flatten(1).norm(dim=1).reshape(-1, 1, 1)).float()


class _ConvList(nn.Module):
    ''' one ResBlock: `convs1` / `convs2` (type "1") or `convs` (type "2") '''
    def __init__(self, lists):
        super().__init__()
        for name, layers in lists.items():
            setattr(self, name, nn.ModuleList(layers))


def _stage_channels(cfg, hint):
    ''' raises ValueError naming the first layer whose channel counts the MFMA kernels do not take (multiples of 32; conv_pre's
        mel bins are zero-padded, conv_post's single output is torch) '''
    for name, kind, shape, _ in V.layer_table(cfg):
        cin, cout = (shape[0], shape[1]) if kind == 'up' else (shape[1], shape[0])
        bad = [c for c, skip in ((cin, name == 'conv_pre'), (cout, name == 'conv_post')) if not skip and c % 32]
        if bad:
            raise ValueError(f'vocoder training: layer "{name}" has {bad[0]} channels; every stage must be a multiple of 32 ({hint})')


def trainable_stages(cfg):
    ''' what `TrainableGenerator` takes: raises ValueError naming the first layer whose channel counts are no multiples of 32, or the
        `activation` of a BigVGAN config -- that generator trains through `bigvgan_train.TrainableBigVGAN` (`trainable_generator`
        picks the class, `trainable_config` the check) '''
    if cfg.get('activation') is not None:
        raise ValueError(f'vocoder training: the config\'s "activation" is {cfg["activation"]!r}: TrainableGenerator covers HiFi-GAN '
                         f'generators only; a BigVGAN generator trains through daft_exprt.bigvgan_train.TrainableBigVGAN '
                         f'(vocoder_train.trainable_generator returns the right class)')
    _stage_channels(cfg, 'HiFi-GAN V1 and V3 qualify, V2\'s 16- / 8-channel tail does not')


def trainable_config(cfg):
    ''' the stage check of the class `trainable_generator` would build; returns the family, "bigvgan" or "hifi-gan" '''
    if V.is_bigvgan(cfg):
        from daft_exprt.bigvgan_train import bigvgan_stages
        bigvgan_stages(cfg)
        return 'bigvgan'
    trainable_stages(cfg)
    return 'hifi-gan'


def trainable_generator(config, state_dict, compute_dtype='fp32'):
    ''' `TrainableGenerator` for a HiFi-GAN config, `bigvgan_train.TrainableBigVGAN` for one with an `activation` '''
    cfg = V.load_config(config)
    V.validate_config(cfg)
    if V.is_bigvgan(cfg):
        from daft_exprt.bigvgan_train import TrainableBigVGAN
        return TrainableBigVGAN(cfg, state_dict, compute_dtype=compute_dtype)
    return TrainableGenerator(cfg, state_dict, compute_dtype=compute_dtype)


class TrainableGenerator(nn.Module):
    def __init__(self, config, state_dict, compute_dtype='fp32'):
        ''' config: dict or path of `config.json`; state_dict: a generator state dict in any of the three key forms
            `vocoder.folded_weight` reads (a plain `.weight` becomes g = ||w||, v = w); compute_dtype: the MFMA operand type of
            every convolution, forward and backward: 'fp32' (exact) or 'bf16' '''
        super().__init__()
        self.config = V.load_config(config)
        V.validate_config(self.config)
        if compute_dtype not in _TDT:
            raise ValueError(f'compute_dtype is {compute_dtype!r}, expected "bf16" or "fp32"')
        self._check_stages()
        cfg = self.config
        self.compute_dtype = compute_dtype
        self.rates = [int(u) for u in cfg['upsample_rates']]
        self.res_dilations = [[int(d) for d in dils] for dils in cfg['resblock_dilation_sizes']]
        self.resblock = str(cfg['resblock'])
        self.num_mels, self.hop = int(cfg['num_mels']), int(cfg['hop_size'])
        self.mel_channels = -(-self.num_mels // 32) * 32
        folded = V.folded_state(cfg, state_dict)                     # (the biases, and every shape check of the inference path)
        layer = lambda name: self._layer(state_dict, self._source_name(state_dict, name), folded[name][1])      # noqa: E731
        self.conv_pre = layer('conv_pre')
        self.ups = nn.ModuleList(layer(f'ups.{i}') for i in range(len(self.rates)))
        nk = len(self.res_dilations)
        blocks = []
        for i in range(len(self.rates)):
            for j, dils in enumerate(self.res_dilations):
                block = f'resblocks.{i * nk + j}'
                names = ('convs1', 'convs2') if self.resblock == '1' else ('convs',)
                blocks.append(_ConvList({nm: [layer(f'{block}.{nm}.{m}') for m in range(len(dils))] for nm in names}))
        self.resblocks = nn.ModuleList(blocks)
        self.conv_post = layer('conv_post')

    def _check_stages(self):
        trainable_stages(self.config)

    @staticmethod
    def _source_name(state_dict, name):
        ''' the layer's prefix in the state dict '''
        return name

    @staticmethod
    def _layer(state_dict, name, bias):
        ''' g and v as the checkpoint holds them (so a fine-tuned file continues the pretrained parametrisation), or g = ||w||, v = w '''
        mod = _WeightNormed(V.folded_weight(state_dict, name), bias)
        for g_key, v_key in V._NORM_FORMS:
            if f'{name}{g_key}' in state_dict and f'{name}{v_key}' in state_dict:
                with torch.no_grad():
                    mod.weight_g.copy_(state_dict[f'{name}{g_key}'].detach().float().reshape(-1, 1, 1))
                    mod.weight_v.copy_(state_dict[f'{name}{v_key}'].detach().float())
        return mod

    _slope = V.LRELU_SLOPE      # of the leaky-ReLU the convs apply to their input (a BigVGAN generator: 1, `_fed` is its activation)

    def _conv(self, name, x, n, dilation, slope=None):
        mod = self.get_submodule(name)
        return _Conv.apply(x, mod.weight(), mod.bias, n, dilation, self._slope if slope is None else slope, self.compute_dtype)

    def _fed(self, name, x, n):
        ''' what the conv `name` reads: x itself (the leaky-ReLU is applied as the conv stages its input) '''
        return x

    def _post(self, x, n):
        return _Post.apply(x, self.conv_post.weight(), self.conv_post.bias, n)

    def forward(self, mel, lengths):
        ''' mel (B, num_mels, T) natural-log mel on the device (columns at or past `lengths` are not read), lengths (B,) int64
            -> waveform (B, T * hop) fp32 in [-1, 1], zeros past lengths * hop; differentiable in the parameters and in mel '''
        H.require_gpu(mel, lengths)
        if mel.dim() != 3 or mel.shape[1] != self.num_mels:
            raise ValueError(f'mel has shape {tuple(mel.shape)}, expected (B, {self.num_mels}, T)')
        if lengths.dtype != torch.int64 or lengths.shape != (mel.shape[0],):
            raise ValueError(f'lengths must be int64 of shape ({mel.shape[0]},)')
        B, _, T = mel.shape
        n = lengths.clamp(0, T)
        x = mel.float().transpose(1, 2)
        if self.mel_channels > self.num_mels:
            x = torch.cat([x, x.new_zeros((B, T, self.mel_channels - self.num_mels))], dim=2)
        with torch.cuda.device(mel.device):
            x = self._conv('conv_pre', x, n, 1, slope=1.)
            nk = len(self.res_dilations)
            for i, u in enumerate(self.rates):
                up = self.ups[i]
                x = _Upsample.apply(x, up.weight(), up.bias, n, u, self._slope, self.compute_dtype)
                n = n * u
                total = None
                for j, dils in enumerate(self.res_dilations):
                    r, block = x, f'resblocks.{i * nk + j}'
                    for m, d in enumerate(dils):
                        if self.resblock == '1':
                            t = self._conv(f'{block}.convs1.{m}', self._fed(f'{block}.convs1.{m}', r, n), n, d)
                            r = r + self._conv(f'{block}.convs2.{m}', self._fed(f'{block}.convs2.{m}', t, n), n, 1)
                        else:
                            r = r + self._conv(f'{block}.convs.{m}', self._fed(f'{block}.convs.{m}', r, n), n, d)
                    total = r if total is None else total + r
                x = total / nk
            return self._post(self._fed('conv_post', x, n), n)


# ---- discriminators (Kong et al. 2020, sections 2.2 - 2.3), plain torch -------------------------------------------------------------

MPD_PERIODS = (2, 3, 5, 7, 11)
_MPD_CHANNELS = (1, 32, 128, 512, 1024)
_MSD_CONVS = ((1, 128, 15, 1, 1), (128, 128, 41, 2, 4), (128, 256, 41, 2, 16), (256, 512, 41, 4, 16), (512, 1024, 41, 4, 16),
              (1024, 1024, 41, 1, 16), (1024, 1024, 5, 1, 1))
D_SLOPE = 0.1


def _normed(conv, spectral=False):
    return nn.utils.spectral_norm(conv) if spectral else nn.utils.weight_norm(conv)


class PeriodDiscriminator(nn.Module):
    ''' the waveform folded to (T / p, p); convolutions along the first axis only: (5, 1) stride (3, 1) to 32 / 128 / 512 / 1024
        channels, (5, 1) stride 1, then (3, 1) to one channel; leaky-ReLU 0.1 after each but the last '''
    def __init__(self, period):
        super().__init__()
        self.period = period
        convs = [nn.Conv2d(cin, cout, (5, 1), (3, 1), padding=(2, 0)) for cin, cout in zip(_MPD_CHANNELS[:-1], _MPD_CHANNELS[1:])]
        convs.append(nn.Conv2d(1024, 1024, (5, 1), 1, padding=(2, 0)))
        self.convs = nn.ModuleList(_normed(c) for c in convs)
        self.conv_post = _normed(nn.Conv2d(1024, 1, (3, 1), 1, padding=(1, 0)))

    def forward(self, x):
        ''' x (B, 1, T) -> (scores (B, -1), feature maps) '''
        B, c, T = x.shape
        if T % self.period:
            x = F.pad(x, (0, self.period - T % self.period), 'reflect')
        x = x.view(B, c, x.shape[2] // self.period, self.period)
        fmap = []
        for conv in self.convs:
            x = F.leaky_relu(conv(x), D_SLOPE)
            fmap.append(x)
        x = self.conv_post(x)
        fmap.append(x)
        return x.flatten(1), fmap


class MultiPeriodDiscriminator(nn.Module):
    def __init__(self):
        super().__init__()
        self.discriminators = nn.ModuleList(PeriodDiscriminator(p) for p in MPD_PERIODS)

    def forward(self, y, y_hat):
        ''' y, y_hat (B, 1, T) -> (scores of y, scores of y_hat, feature maps of y, feature maps of y_hat), one entry per period '''
        out = [[], [], [], []]
        for d in self.discriminators:
            for k, x in enumerate((y, y_hat)):
                score, fmap = d(x)
                out[k].append(score)
                out[2 + k].append(fmap)
        return tuple(out)


class ScaleDiscriminator(nn.Module):
    def __init__(self, spectral=False):
        super().__init__()
        self.convs = nn.ModuleList(_normed(nn.Conv1d(cin, cout, k, s, groups=g, padding=k // 2), spectral)
                                   for cin, cout, k, s, g in _MSD_CONVS)
        self.conv_post = _normed(nn.Conv1d(1024, 1, 3, 1, padding=1), spectral)

    def forward(self, x):
        fmap = []
        for conv in self.convs:
            x = F.leaky_relu(conv(x), D_SLOPE)
            fmap.append(x)
        x = self.conv_post(x)
        fmap.append(x)
        return x.flatten(1), fmap


class MultiScaleDiscriminator(nn.Module):
    ''' three scales, AvgPool1d(4, 2, padding 2) between them; the first spectral-normed, the others weight-normed '''
    def __init__(self):
        super().__init__()
        self.discriminators = nn.ModuleList([ScaleDiscriminator(spectral=True), ScaleDiscriminator(), ScaleDiscriminator()])
        self.meanpools = nn.ModuleList([nn.AvgPool1d(4, 2, padding=2), nn.AvgPool1d(4, 2, padding=2)])

    def forward(self, y, y_hat):
        out = [[], [], [], []]
        for i, d in enumerate(self.discriminators):
            if i:
                y, y_hat = self.meanpools[i - 1](y), self.meanpools[i - 1](y_hat)
            for k, x in enumerate((y, y_hat)):
                score, fmap = d(x)
                out[k].append(score)
                out[2 + k].append(fmap)
        return tuple(out)


# ---- losses, fp32 -------------------------------------------------------------------------------------------------------------------

def discriminator_loss(real_scores, generated_scores):
    ''' sum over the sub-discriminators of mean((1 - D(y))^2) + mean(D(G)^2) '''
    return sum(torch.mean((1. - r) ** 2) + torch.mean(g ** 2) for r, g in zip(real_scores, generated_scores))


def generator_adversarial_loss(generated_scores):
    ''' sum mean((1 - D(G))^2) '''
    return sum(torch.mean((1. - g) ** 2) for g in generated_scores)


def feature_matching_loss(fmaps_real, fmaps_generated):
    ''' 2 * sum over every feature map of mean |fmap_r - fmap_g| '''
    return 2. * sum(torch.mean(torch.abs(r - g)) for dr, dg in zip(fmaps_real, fmaps_generated) for r, g in zip(dr, dg))


MEL_LOSS_WEIGHT = 45.


def mel_l1(mel_a, mel_b):
    return F.l1_loss(mel_a, mel_b)


class LossMel(nn.Module):
    ''' HiFi-GAN's training mel, restated as one matmul autograd differentiates: reflect padding of (n_fft - hop) / 2 per side, no
        centring, frames of win_size under the periodic Hann window times a DFT basis built in float64, sqrt(re^2 + im^2 + 1e-9),
        the filter bank of `extract_features.mel_filter_bank` up to fmax_for_loss, log(clamp(., 1e-5)).  The one place where the mel
        of the front end (`dx_mel_spectrogram`) is restated; tests/test_gpu_vocoder_train.py pins the two against each other. '''
    def __init__(self, cfg):
        super().__init__()
        from daft_exprt.extract_features import mel_filter_bank
        for key in ('n_fft', 'win_size', 'hop_size', 'fmin', 'fmax_for_loss', 'num_mels', 'sampling_rate'):
            if key not in cfg:
                raise ValueError(f'vocoder config: "{key}" is missing')
        self.n_fft, self.win, self.hop = int(cfg['n_fft']), int(cfg['win_size']), int(cfg['hop_size'])
        if self.win > self.n_fft or (self.n_fft - self.hop) % 2:
            raise ValueError(f'vocoder config: win_size {self.win} > n_fft {self.n_fft}, or n_fft - hop_size is odd')
        bins = self.n_fft // 2 + 1
        window = torch.zeros(self.n_fft, dtype=torch.float64)
        left = (self.n_fft - self.win) // 2
        window[left:left + self.win] = 0.5 - 0.5 * torch.cos(2 * math.pi * torch.arange(self.win, dtype=torch.float64) / self.win)
        phase = 2 * math.pi * ((torch.arange(self.n_fft)[:, None] * torch.arange(bins)[None, :]) % self.n_fft).double() / self.n_fft
        basis = torch.cat([torch.cos(phase), -torch.sin(phase)], dim=1) * window[:, None]               # (n_fft, 2 bins)
        self.register_buffer('basis', basis.float(), persistent=False)
        fb = mel_filter_bank(int(cfg['sampling_rate']), self.n_fft, int(cfg['num_mels']), cfg['fmin'], cfg['fmax_for_loss'])
        self.register_buffer('fb', torch.from_numpy(fb).t().contiguous(), persistent=False)            # (bins, n_mels)

    def forward(self, wav):
        ''' wav (B, S) -> log-mel (B, num_mels, S / hop) '''
        pad = (self.n_fft - self.hop) // 2
        frames = F.pad(wav[:, None], (pad, pad), 'reflect')[:, 0].unfold(1, self.n_fft, self.hop)       # (B, T, n_fft)
        spec = frames @ self.basis.to(frames.dtype)
        bins = self.n_fft // 2 + 1
        mag = torch.sqrt(spec[..., :bins] ** 2 + spec[..., bins:] ** 2 + 1e-9)
        return torch.log(torch.clamp(mag @ self.fb.to(frames.dtype), min=1e-5)).transpose(1, 2)


# ---- the data set -------------------------------------------------------------------------------------------------------------------

def front_end(cfg, centered=True):
    ''' the hyper-parameters `extract_features.nb_frames` / `mel_spectrogram_batch` read, from a HiFi-GAN config '''
    return SimpleNamespace(sampling_rate=int(cfg['sampling_rate']), filter_length=int(cfg['n_fft']), hop_length=int(cfg['hop_size']),
                           n_mel_channels=int(cfg['num_mels']), mel_fmin=cfg['fmin'], mel_fmax=cfg['fmax_for_loss'], centered=centered,
                           min_clipping=1e-5)


def read_data_set(data_set_dir, cfg, segment_size, validation_fraction=10, centered=True):
    ''' every `<speaker>/<file>.npy` / `.wav` pair of a `fine_tuning_dataset`, read once.  Returns (train, held_out, skipped): lists
        of (name, mel (num_mels, T) float32, audio (n,) int16 as float32 / 32768) and the count of pairs shorter than a segment.
        One in `validation_fraction` utterances of every speaker, by sorted name, is held out (0: none).  A mel whose frame count
        is not `extract_features.nb_frames` of its audio raises ValueError naming the file. '''
    from daft_exprt.audio import read_wav
    from daft_exprt.extract_features import nb_frames
    hp, hop, frames = front_end(cfg, centered), int(cfg['hop_size']), segment_size // int(cfg['hop_size'])
    train, held_out, skipped = [], [], 0
    speakers = sorted(d for d in os.listdir(data_set_dir) if os.path.isdir(os.path.join(data_set_dir, d)))
    for speaker in speakers:
        root = os.path.join(data_set_dir, speaker)
        names = sorted(f[:-4] for f in os.listdir(root) if f.endswith('.npy') and os.path.isfile(os.path.join(root, f[:-4] + '.wav')))
        for idx, name in enumerate(names):
            mel = np.load(os.path.join(root, name + '.npy')).astype(np.float32)
            x, rate = read_wav(os.path.join(root, name + '.wav'))
            if rate != hp.sampling_rate:
                raise ValueError(f'{os.path.join(root, name)}.wav: {rate} Hz, the vocoder config says {hp.sampling_rate}')
            if mel.ndim != 2 or mel.shape[0] != hp.n_mel_channels:
                raise ValueError(f'{os.path.join(root, name)}.npy: shape {mel.shape}, expected ({hp.n_mel_channels}, T)')
            if nb_frames(x.shape[0], hp) != mel.shape[1]:
                raise ValueError(f'{os.path.join(root, name)}.npy: {mel.shape[1]} frames, its .wav of {x.shape[0]} samples gives '
                                 f'{nb_frames(x.shape[0], hp)}')
            audio = x[:, 0].astype(np.float32) / np.float32(32768.) if x.dtype == np.int16 else x[:, 0].astype(np.float32)
            item = (f'{speaker}/{name}', mel, audio)
            if validation_fraction and idx % validation_fraction == validation_fraction - 1:
                held_out.append(item)
            elif mel.shape[1] < frames + 1 or audio.shape[0] < frames * hop:
                skipped += 1
            else:
                train.append(item)
    return train, held_out, skipped


class SegmentSampler:
    ''' HiFi-GAN's fine-tuning segments from utterances kept on the device: frames = segment_size / hop, start uniform in
        [0, T - frames - 1], audio [start hop, (start + frames) hop), no 0.95 normalisation '''
    def __init__(self, items, hop, segment_size, device, seed=1234):
        if segment_size % hop:
            raise ValueError(f'segment_size {segment_size} is not a multiple of the hop {hop}')
        self.hop, self.frames, self.device = hop, segment_size // hop, device
        self.mels = [torch.from_numpy(mel).to(device) for _, mel, _ in items]
        self.audio = [torch.from_numpy(audio).to(device) for _, _, audio in items]
        self.rng = np.random.RandomState(seed)
        self.order, self.epoch = [], 0

    def draw(self, batch_size):
        ''' (mel (B, num_mels, frames), audio (B, frames * hop)); an epoch is one pass over a permutation of the utterances '''
        mels, audio = [], []
        for _ in range(batch_size):
            if not self.order:
                self.order = list(self.rng.permutation(len(self.mels)))
                self.epoch += 1
            i = self.order.pop()
            start = int(self.rng.randint(0, self.mels[i].shape[1] - self.frames))      # [0, T - frames - 1]
            mels.append(self.mels[i][:, start:start + self.frames])
            audio.append(self.audio[i][start * self.hop:(start + self.frames) * self.hop])
        return torch.stack(mels), torch.stack(audio)


# ---- checkpoints ----------------------------------------------------------------------------------------------------------------

SECOND_DISCRIMINATORS = ('msd', 'mrd')      # what trains beside the MPD: HiFi-GAN's multi-scale or BigVGAN's multi-resolution one


def _second_key(second):
    if second not in SECOND_DISCRIMINATORS:
        raise ValueError(f'second_discriminator is {second!r}, expected "msd" or "mrd"')
    return second


def save_checkpoints(out_dir, config, generator, mpd, msd, optim_g, optim_d, steps, epoch, second='msd'):
    ''' HiFi-GAN's layout: g_%08d = {'generator'}, do_%08d = {'mpd', 'msd', 'optim_g', 'optim_d', 'steps', 'epoch'}, config.json;
        `second` = 'mrd' files the module in the `msd` position under BigVGAN's key 'mrd' '''
    _second_key(second)
    os.makedirs(out_dir, exist_ok=True)
    g_path, do_path = os.path.join(out_dir, f'g_{steps:08d}'), os.path.join(out_dir, f'do_{steps:08d}')
    torch.save({'generator': {k: v.detach().cpu() for k, v in generator.state_dict().items()}}, g_path)
    torch.save({'mpd': mpd.state_dict(), second: msd.state_dict(), 'optim_g': optim_g.state_dict(), 'optim_d': optim_d.state_dict(),
                'steps': steps, 'epoch': epoch}, do_path)
    with open(os.path.join(out_dir, 'config.json'), 'w', encoding='utf-8') as f:
        json.dump(config, f, indent=1)
    return g_path, do_path


def load_discriminator_state(do_checkpoint, mpd, msd, optim_g=None, optim_d=None, second='msd'):
    ''' (steps, epoch) of a `do_` file loaded into the modules; a key the modules expect and the file lacks raises ValueError
        naming the first one.  `second`: the entry the module in the `msd` position is filed under, 'msd' or 'mrd'; a file that holds
        the other kind raises ValueError naming the entry found and the flag to pass '''
    _second_key(second)
    state = torch.load(do_checkpoint, map_location='cpu', weights_only=False)
    for key in ('mpd', second, 'optim_g', 'optim_d', 'steps', 'epoch'):
        other = 'mrd' if second == 'msd' else 'msd'
        if key == second and isinstance(state, dict) and key not in state and other in state:
            raise ValueError(f'{do_checkpoint}: holds an "{other}" entry and no "{second}": it was trained against the '
                             f'{"multi-resolution" if other == "mrd" else "multi-scale"} discriminator; pass '
                             f'second_discriminator="{other}" (scripts/train_vocoder.py --second_discriminator {other})')
        if not isinstance(state, dict) or key not in state:
            raise ValueError(f'{do_checkpoint}: no "{key}" entry (expected a HiFi-GAN discriminator / optimiser checkpoint)')
    for key, module in (('mpd', mpd), (second, msd)):
        missing = [k for k in module.state_dict() if k not in state[key]]
        if missing:
            raise ValueError(f'{do_checkpoint}: "{key}" has no "{missing[0]}" ({len(missing)} keys missing)')
        module.load_state_dict(state[key])
    if optim_g is not None:
        optim_g.load_state_dict(state['optim_g'])
    if optim_d is not None:
        optim_d.load_state_dict(state['optim_d'])
    return int(state['steps']), int(state['epoch'])


# ---- training -------------------------------------------------------------------------------------------------------------------

LEARNING_RATE, ADAM_BETAS, LR_DECAY = 2e-4, (0.8, 0.99), 0.999
MEL_LOSSES = ('single', 'multiscale')       # the reconstruction term: HiFi-GAN's one log-mel, or BigVGAN-v2's seven (mel_loss.py, K37)
MRD_LEARNING_RATE, MRD_CLIP_GRAD_NORM = 1e-4, 1000.      # BigVGAN's recipe (Lee et al. 2023, appendix), where the config gives none


def _clip(optimizer, max_norm):
    if max_norm is not None:
        torch.nn.utils.clip_grad_norm_([p for group in optimizer.param_groups for p in group['params']], max_norm)


def train_step(generator, mpd, msd, optim_g, optim_d, loss_mel, mel, audio, clip_grad_norm=None, mel_loss=None):
    ''' one step of HiFi-GAN's training: the discriminators on the detached synthesis, then the generator.  `msd` is the second
        discriminator, multi-scale or multi-resolution; `clip_grad_norm` (BigVGAN's recipe) clips the gradient norm of each optimiser's
        parameters before its step.  `mel_loss`: None, the L1 of `loss_mel`'s log-mels weighted MEL_LOSS_WEIGHT, or a module such as
        `mel_loss.MultiScaleMelLoss` (K37) whose value of (audio, synthesis) and whose `weight` take their place.
        Returns {'disc', 'adv', 'fm', 'mel'} as device scalars (mel = the unweighted reconstruction term) '''
    B, _, frames = mel.shape
    lengths = torch.full((B,), frames, dtype=torch.int64, device=mel.device)
    y = audio[:, None]
    y_hat = generator(mel, lengths)[:, None]
    optim_d.zero_grad(set_to_none=True)
    loss_d = 0.
    for disc in (mpd, msd):
        real, fake, _, _ = disc(y, y_hat.detach())
        loss_d = loss_d + discriminator_loss(real, fake)
    loss_d.backward()
    _clip(optim_d, clip_grad_norm)
    optim_d.step()
    optim_g.zero_grad(set_to_none=True)
    if mel_loss is None:
        l_mel = mel_l1(loss_mel(audio), loss_mel(y_hat[:, 0]))
        mel_weight = MEL_LOSS_WEIGHT
    else:
        l_mel = mel_loss(audio, y_hat[:, 0])
        mel_weight = mel_loss.weight
    l_adv, l_fm = 0., 0.
    for disc in (mpd, msd):
        _, fake, fmap_r, fmap_g = disc(y, y_hat)
        l_adv = l_adv + generator_adversarial_loss(fake)
        l_fm = l_fm + feature_matching_loss(fmap_r, fmap_g)
    (l_adv + l_fm + mel_weight * l_mel).backward()
    _clip(optim_g, clip_grad_norm)
    optim_g.step()
    return {'disc': loss_d.detach(), 'adv': l_adv.detach(), 'fm': l_fm.detach(), 'mel': l_mel.detach()}


def held_out_mel_l1(config, state_dict, held_out, compute_dtype, device, centered=True):
    ''' the held-out utterances WHOLE through `Vocoder` (the inference path, sub-batch walk included): mean over the utterances of
        the L1 between the log-mel of the synthesis and of the recording, both from `dx_mel_spectrogram`; None without utterances '''
    from daft_exprt.extract_features import mel_spectrogram_batch
    if not held_out:
        return None
    voc = V.Vocoder(config, state_dict, compute_dtype=compute_dtype, device=device)
    hp, total = front_end(config, centered), 0.
    for _, mel, audio in held_out:
        m = torch.from_numpy(mel).to(device)[None]
        wav, _ = voc(m, torch.tensor([m.shape[2]], dtype=torch.int64, device=device))
        n = audio.shape[0]
        count = torch.tensor([n], dtype=torch.int64, device=device)
        rec = torch.from_numpy(audio).to(device)[None].contiguous()
        syn = wav[:, :n].contiguous()
        if syn.shape[1] < n:
            syn = F.pad(syn, (0, n - syn.shape[1]))
        mel_r, _, frames = mel_spectrogram_batch(rec, count, hp, min_samples=n)
        mel_s, _, _ = mel_spectrogram_batch(syn, count, hp, min_samples=n)
        t = int(frames[0])
        total += float(mel_l1(mel_s[:, :, :t], mel_r[:, :, :t]))
    return total / len(held_out)


def fine_tune_vocoder(config, data_set_dir, g_checkpoint, do_checkpoint=None, out_dir=None, steps=1000, batch_size=16,
                      segment_size=8192, compute_dtype='fp32', checkpoint_interval=500, log_interval=50, validation_fraction=10,
                      seed=1234, device=None, centered=True, second_discriminator='msd', mel_loss='single'):
    ''' fine-tunes the generator of `g_checkpoint` on a `fine_tuning_dataset` (single GPU) and writes `g_%08d` / `do_%08d` /
        `config.json` to `out_dir` at every checkpoint interval and at the end.  AdamW, lr 2e-4, betas (0.8, 0.99), decayed by 0.999
        per epoch; the discriminator step before the generator step.  Without `do_checkpoint` the discriminators start from their
        initialisation (a warning).  `second_discriminator`: 'msd', HiFi-GAN's recipe as above for either generator family, or 'mrd',
        BigVGAN's: MPD + the multi-resolution discriminator (`bigvgan_train.MultiResolutionDiscriminator`, over K36), the config's
        `learning_rate` (default 1e-4) and `clip_grad_norm` (default 1000, on both optimisers' parameters before their step), the same
        betas and decay; `do_%08d` then holds 'mrd' in place of 'msd'.  `mel_loss`: 'single', HiFi-GAN's one log-mel weighted 45
        (`LossMel`), or 'multiscale', BigVGAN-v2's sum over seven resolutions weighted 15 (`mel_loss.MultiScaleMelLoss`, over K37);
        independent of `second_discriminator`, and held-out validation is the same either way.  Returns the report
        `scripts/train_vocoder.py` writes. '''
    config = V.load_config(config)
    V.validate_config(config)
    _second_key(second_discriminator)
    if mel_loss not in MEL_LOSSES:
        raise ValueError(f'mel_loss is {mel_loss!r}, expected "single" or "multiscale"')
    device = H.device(device)
    hop = int(config['hop_size'])
    if segment_size < hop or segment_size % hop:
        raise ValueError(f'segment_size {segment_size} is not a positive multiple of the hop {hop}')
    train, held_out, skipped = read_data_set(data_set_dir, config, segment_size, validation_fraction, centered)
    if not train:
        raise ValueError(f'{data_set_dir}: no utterance of at least one segment ({segment_size} samples) to train on')
    ckpt = torch.load(g_checkpoint, map_location='cpu', weights_only=False)
    if not isinstance(ckpt, dict) or 'generator' not in ckpt:
        raise ValueError(f'{g_checkpoint}: no "generator" entry (expected a HiFi-GAN generator checkpoint)')
    torch.manual_seed(seed)
    loss_mel = LossMel(config).to(device)
    multiscale = None
    if mel_loss == 'multiscale':
        from daft_exprt.mel_loss import MultiScaleMelLoss
        multiscale = MultiScaleMelLoss(config)
        multiscale.check_segment(segment_size)
    generator = trainable_generator(config, ckpt['generator'], compute_dtype=compute_dtype).to(device)
    lr, clip = LEARNING_RATE, None
    if second_discriminator == 'mrd':
        from daft_exprt.bigvgan_train import MultiResolutionDiscriminator
        mpd, msd = MultiPeriodDiscriminator().to(device), MultiResolutionDiscriminator(config).to(device)
        msd.check_segment(segment_size)
        lr, clip = float(config.get('learning_rate', MRD_LEARNING_RATE)), float(config.get('clip_grad_norm', MRD_CLIP_GRAD_NORM))
    else:
        mpd, msd = MultiPeriodDiscriminator().to(device), MultiScaleDiscriminator().to(device)
    optim_g = torch.optim.AdamW(generator.parameters(), lr, betas=ADAM_BETAS)
    optim_d = torch.optim.AdamW(list(msd.parameters()) + list(mpd.parameters()), lr, betas=ADAM_BETAS)
    first_step, first_epoch = 0, 0
    if do_checkpoint is not None:
        first_step, first_epoch = load_discriminator_state(do_checkpoint, mpd, msd, optim_g, optim_d, second=second_discriminator)
    else:
        warnings.warn('fine_tune_vocoder: no do_ checkpoint, the discriminators start from their initialisation')
    sampler = SegmentSampler(train, hop, segment_size, device, seed)
    sampler.epoch = first_epoch
    sched_g = torch.optim.lr_scheduler.ExponentialLR(optim_g, gamma=LR_DECAY)
    sched_d = torch.optim.lr_scheduler.ExponentialLR(optim_d, gamma=LR_DECAY)
    report = {'utterances_used': len(train), 'utterances_skipped': skipped, 'utterances_held_out': len(held_out),
              'generator_family': 'bigvgan' if V.is_bigvgan(config) else 'hifi-gan', 'compute_dtype': compute_dtype,
              'batch_size': batch_size, 'segment_size': segment_size, 'first_step': first_step,
              'second_discriminator': second_discriminator, 'mel_loss': mel_loss, 'log': []}
    validate = lambda: held_out_mel_l1(config, generator.state_dict(), held_out, compute_dtype, device, centered)   # noqa: E731
    report['held_out_mel_l1_start'] = validate()
    step, epoch, last_val = first_step, max(sampler.epoch, 1), report['held_out_mel_l1_start']
    torch.cuda.synchronize(device)
    t0, train_s = time.time(), 0.
    with torch.cuda.device(device):
        while step < first_step + steps:
            mel, audio = sampler.draw(batch_size)
            losses = train_step(generator, mpd, msd, optim_g, optim_d, loss_mel, mel, audio, clip_grad_norm=clip, mel_loss=multiscale)
            step += 1
            while epoch < sampler.epoch:                              # the decay of an epoch that ended with this batch's draw
                sched_g.step()
                sched_d.step()
                epoch += 1
            at_ckpt = step % checkpoint_interval == 0 or step == first_step + steps
            if at_ckpt or step % log_interval == 0 or step == first_step + 1:
                values = {k: float(v) for k, v in losses.items()}
                if not all(math.isfinite(v) for v in values.values()):
                    raise FloatingPointError(f'fine_tune_vocoder: step {step}: a loss is not finite: {values}')
                if at_ckpt:
                    torch.cuda.synchronize(device)
                    train_s += time.time() - t0
                    last_val = validate()
                    if out_dir is not None:
                        save_checkpoints(out_dir, config, generator, mpd, msd, optim_g, optim_d, step, sampler.epoch, second=second_discriminator)
                    t0 = time.time()
                report['log'].append(dict(values, step=step, held_out_mel_l1=last_val if at_ckpt else None))
                _logger.info(f'step {step}: ' + ', '.join(f'{k} {v:.4f}' for k, v in values.items()) +
                             (f', held-out mel L1 {last_val}' if at_ckpt else ''))
    report['held_out_mel_l1_final'] = last_val
    report['steps'], report['epoch'] = step, sampler.epoch
    report['steps_per_second'] = steps / train_s if train_s > 0 else None
    if out_dir is not None:
        report['generator'], report['discriminators'] = f'g_{step:08d}', f'do_{step:08d}'
    return report
