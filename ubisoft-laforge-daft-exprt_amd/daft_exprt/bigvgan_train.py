"""Fine-tuning of a BigVGAN generator (Lee et al. 2023) on the GPU: what `daft_exprt/vocoder_train.py` lacks for a config with an
`activation`.  The convolutions, their data and weight gradients, the discriminators, the losses, the sampler and the checkpoint
writer are that module's; this one adds

    the activation   `dx_vocoder_snake` forward (K34, the launch of the inference path, the same bits) and `dx_vocoder_snake_bwd`
                     backward (K35, csrc/snake_bwd.hip): dx and the gradients of the per-channel alpha' and 1 / (beta' + 1e-9), nothing
                     saved by the forward but its inputs
    the parameters   raw `alpha` / `beta` as the checkpoint holds them -> final form as a differentiable host expression (float64,
                     rounded once, as `vocoder.activation_state` forms it), so autograd carries the chain through exp and 1 / (. + 1e-9)
    the last stage   `activation_post`, then conv_post with slope 1, tanh or clamp(-1, 1), with or without its bias

`TrainableBigVGAN` is `TrainableGenerator` (one construction of the layer parameters) with these in its forward, which follows
`vocoder.activation_table`.  Every stage must be a multiple of 32 channels, as for HiFi-GAN: the 512-channel base models qualify, the
1536-channel models' 48- / 24-channel tail is refused (training on zero-padded stages is not built).  No CPU fallback.

    the discriminator   `MultiResolutionDiscriminator` / `DiscriminatorR`, restated from the paper: 2-D conv stacks (plain torch, as
                        MPD / MSD) over the magnitude spectrogram at three STFT resolutions, which with its gradient back to the waveform
                        is K36 (`daft_exprt/spectrogram.py`, csrc/spectrogram.hip).  `fine_tune_vocoder(second_discriminator='mrd')`
                        trains MPD + MRD under BigVGAN's recipe and files it under `mrd` in the `do_` checkpoint.  No upstream `do_` file
                        has been loaded: the module and key names follow what `weight_norm` gives modules of upstream's names.
"""
import ctypes

import torch
import torch.nn as nn
import torch.nn.functional as F

from daft_exprt import _hip as H
from daft_exprt import vocoder as V
from daft_exprt import vocoder_train as VT


def bigvgan_stages(cfg):
    ''' raises ValueError naming the first layer whose channel counts are no multiples of 32 '''
    VT._stage_channels(cfg, 'the 512-channel BigVGAN base models qualify, the 1536-channel models\' 48- / 24-channel tail does not: '
                            'it runs zero-padded at inference, and training on padded stages is not built')


def final_params(alpha, beta, logscale):
    ''' raw `alpha` / `beta` (C,) (beta None: `snake`, where beta = alpha and alpha collects both paths) -> (alpha',
        1 / (beta' + 1e-9)) fp32, formed in float64 and rounded once as the inference path forms them; differentiable '''
    a = alpha.double().exp() if logscale else alpha.double()
    b = a if beta is None else (beta.double().exp() if logscale else beta.double())
    return a.float(), (1. / (b + 1e-9)).float()


def snake_backward(x, dy, alpha, inv_beta, taps, n, tile_rows=0, parameter_grads=True):
    ''' `dx_vocoder_snake_bwd`: x, dy (B, N, C) time-major fp32, alpha, inv_beta (C,) fp32 in final form, taps a host array of 24
        floats, n (B,) int64 -> (dx (B, N, C), dalpha (C,), dinv_beta (C,)); the two sums are None without `parameter_grads` '''
    VT._check_rows(x, n, 'snake_backward')
    VT._check_rows(dy, n, 'snake_backward')
    if dy.shape != x.shape:
        raise ValueError(f'snake_backward: dy has shape {tuple(dy.shape)}, x {tuple(x.shape)}')
    B, N, c = x.shape
    dx = torch.empty_like(x)
    da = db = ws = None
    if parameter_grads:
        da, db = torch.empty((c,), dtype=torch.float32, device=x.device), torch.empty((c,), dtype=torch.float32, device=x.device)
        ws = VT._workspace(int(H.lib().dx_vocoder_snake_bwd_workspace(B, N, c)), x.device)
    H.check(H.lib().dx_vocoder_snake_bwd(H.ptr(x), c, H.ptr(dy), c, H.ptr(alpha), H.ptr(inv_beta), ctypes.addressof(taps), H.ptr(dx), c,
                                         H.ptr(da), H.ptr(db), H.ptr(ws), H.ptr(n), B, N, c, int(tile_rows), H.stream()))
    return dx, da, db


class _Snake(torch.autograd.Function):
    ''' BigVGAN's anti-aliased periodic activation over time-major rows; alpha, inv_beta (C,) fp32 in final form, taps the host array
        `f_up[12], f_down[12]` of the launch '''
    @staticmethod
    def forward(ctx, x, alpha, inv_beta, n, taps):
        x = x.contiguous()
        VT._check_rows(x, n, 'snake')
        alpha, inv_beta = alpha.contiguous(), inv_beta.contiguous()
        B, N, c = x.shape
        y = torch.empty_like(x)
        H.check(H.lib().dx_vocoder_snake(H.ptr(x), c, H.ptr(alpha), H.ptr(inv_beta), ctypes.addressof(taps), H.ptr(y), c, H.ptr(n), B, N, c,
                                         H.stream()))
        ctx.save_for_backward(x, alpha, inv_beta, n)
        ctx.taps = taps
        return y

    @staticmethod
    def backward(ctx, dy):
        x, alpha, inv_beta, n = ctx.saved_tensors
        dx, da, db = snake_backward(x, dy.contiguous(), alpha, inv_beta, ctx.taps, n,
                                    parameter_grads=ctx.needs_input_grad[1] or ctx.needs_input_grad[2])
        return dx, da, db, None, None


class _PostUngated(torch.autograd.Function):
    ''' tanh or clamp(-1, 1) of Conv1d(C, 1, 7)(x) + bias, no leaky-ReLU in front: `dx_voc_post` / `dx_vocoder_post_clamp` with slope 1.
        Its backward is torch, as `vocoder_train._Post`'s: seven shifted products for dx, one contraction in float64 for dW; the
        clamp's gate is |y| < 1 '''
    @staticmethod
    def forward(ctx, x, w, bias, n, clamp):
        x = x.contiguous()
        VT._check_rows(x, n, 'conv_post')
        B, N, c = x.shape
        y = torch.empty((B, N), dtype=torch.float32, device=x.device)
        wp = w[0].t().contiguous().float()
        post = H.lib().dx_vocoder_post_clamp if clamp else H.lib().dx_voc_post
        H.check(post(H.ptr(x), c, H.ptr(wp), H.ptr(bias), H.ptr(y), N, H.ptr(n), B, N, c, w.shape[2], 1., H.stream()))
        ctx.save_for_backward(x, w, n, y)
        ctx.clamp = clamp
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, n, y = ctx.saved_tensors
        B, N, _ = x.shape
        k = w.shape[2]
        h = k // 2
        live = VT._live(n, N, x.device)
        slope = (y.abs() < 1.).double() if ctx.clamp else 1. - y.double() ** 2
        dpre64 = torch.where(live[:, :, 0], dy.double() * slope, dy.new_zeros((), dtype=torch.float64))
        dpre = dpre64.float()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            padded = F.pad(dpre, (h, h))
            acc = None
            for j in range(k):                                      # dx[t] = sum_j dpre[t - j + h] w[j], j ascending
                term = padded[:, 2 * h - j:2 * h - j + N, None] * w[0, :, j]
                acc = term if acc is None else acc + term
            dx = torch.where(live, acc, acc.new_zeros(()))
        if ctx.needs_input_grad[1]:
            xa = torch.where(live, x, x.new_zeros(())).double()
            padded = F.pad(dpre64, (h, h))
            shifts = torch.stack([padded[:, 2 * h - j:2 * h - j + N] for j in range(k)], dim=2)
            dw = (shifts.reshape(B * N, k).t() @ xa.reshape(B * N, -1)).t()[None].float()
        if ctx.needs_input_grad[2]:
            db = dpre64.sum().float().reshape(1)
        return dx, dw, db, None, None


class _Named(nn.Module):
    ''' a node of the checkpoint's key tree '''


class _Activation(nn.Module):
    ''' one `Activation1d` under upstream's names: `act.alpha` (and `act.beta` for `snakebeta`) in the checkpoint's raw form, and the
        two 12-tap filters as buffers that are not trained -- written back to a state dict only where the source had them '''
    def __init__(self, alpha, beta, f_up, f_down, keep_up, keep_down):
        super().__init__()
        self.act = _Named()
        self.act.alpha = nn.Parameter(alpha.float())
        if beta is not None:
            self.act.beta = nn.Parameter(beta.float())
        self.upsample, self.downsample = _Named(), _Named()
        self.downsample.lowpass = _Named()
        self.upsample.register_buffer('filter', f_up.float().reshape(1, 1, -1), persistent=keep_up)
        self.downsample.lowpass.register_buffer('filter', f_down.float().reshape(1, 1, -1), persistent=keep_down)
        # the launch's argument block, from the float64 filters as the inference path builds it
        self.taps = (ctypes.c_float * (2 * V.FILTER_TAPS))(*f_up.tolist(), *f_down.tolist())


class TrainableBigVGAN(VT.TrainableGenerator):
    def __init__(self, config, state_dict, compute_dtype='fp32'):
        ''' config: dict or path of a BigVGAN `config.json` (`activation`: "snake" or "snakebeta"); state_dict: the checkpoint's
            'generator' entry, its transposed convs as `ups.I.0.*` (upstream) or `ups.I.*`; compute_dtype as `TrainableGenerator`'s.
            `state_dict()` gives the source's keys back, so `Vocoder.from_checkpoint` loads what `save_checkpoints` writes. '''
        cfg = V.load_config(config)
        if not V.is_bigvgan(cfg):
            raise ValueError('TrainableBigVGAN: the config has no "activation": a HiFi-GAN generator trains through '
                             'vocoder_train.TrainableGenerator (vocoder_train.trainable_generator returns the right class)')
        self._nested_ups = any(key.startswith('ups.0.0.') for key in state_dict)
        super().__init__(cfg, state_dict, compute_dtype)
        cfg = self.config
        self.logscale, self.snakebeta = bool(cfg.get('snake_logscale', False)), cfg['activation'] == 'snakebeta'
        self.final_clamp = not cfg.get('use_tanh_at_final', True)
        if not cfg.get('use_bias_at_final', True):                  # no such parameter: zeros the optimiser never sees
            del self.conv_post.bias
            self.conv_post.register_buffer('bias', torch.zeros((1,), dtype=torch.float32), persistent=False)
        channels = {name: shape[1] for name, _, shape, _ in V.layer_table(cfg)}
        self._act_of = {}                                           # conv the activation feeds -> its module path
        for layer, name in V.activation_table(cfg):
            f_up, f_down = V.activation_state(cfg, state_dict, name, channels[layer])[2:]       # (and the inference path's checks)
            alpha = state_dict[f'{name}.act.alpha'].detach().cpu()
            beta = state_dict[f'{name}.act.beta'].detach().cpu() if self.snakebeta else None
            mod = _Activation(alpha, beta, f_up, f_down, f'{name}.upsample.filter' in state_dict,
                              f'{name}.downsample.lowpass.filter' in state_dict)
            if name == 'activation_post':
                self.activation_post = mod
            else:
                block, _, a = name.rsplit('.', 2)
                holder = self.get_submodule(block)
                if not hasattr(holder, 'activations'):
                    holder.activations = nn.ModuleList()
                assert len(holder.activations) == int(a), name       # activation_table walks them in order
                holder.activations.append(mod)
            self._act_of[layer] = name

    def _check_stages(self):
        bigvgan_stages(self.config)

    def _source_name(self, state_dict, name):
        return f'{name}.0' if name.startswith('ups.') and self._nested_ups else name

    def state_dict(self, *args, **kwargs):
        ''' under the source's keys: `ups.I.0.*` where the checkpoint had that form '''
        sd = super().state_dict(*args, **kwargs)
        if not self._nested_ups:
            return sd
        prefix = kwargs.get('prefix', args[1] if len(args) > 1 else '')
        out = type(sd)()
        for key, v in sd.items():
            rest = key[len(prefix):]
            parts = rest.split('.')
            out[prefix + '.'.join(parts[:2] + ['0'] + parts[2:]) if parts[0] == 'ups' else key] = v
        return out

    def load_state_dict(self, state_dict, *args, **kwargs):
        if self._nested_ups:
            state_dict = {('.'.join(k.split('.')[:2] + k.split('.')[3:]) if k.startswith('ups.') else k): v
                          for k, v in state_dict.items()}
        return super().load_state_dict(state_dict, *args, **kwargs)

    _slope = 1.

    def _fed(self, layer, x, n):
        ''' the activation in front of the conv `layer`.  `TrainableGenerator.forward` then is the BigVGAN generator, and its waveform
            `Vocoder`'s on the same weights: the same launches in the same order (the mean over the ResBlocks is (r_0 + r_1 + ...) / nk
            here and a chain of fmas with 1 / nk there -- the same bits where nk is a power of two) '''
        mod = self.get_submodule(self._act_of[layer])
        alpha, inv_beta = final_params(mod.act.alpha, mod.act.beta if self.snakebeta else None, self.logscale)
        return _Snake.apply(x, alpha, inv_beta, n, mod.taps)

    def _post(self, x, n):
        return _PostUngated.apply(x, self.conv_post.weight(), self.conv_post.bias, n, self.final_clamp)


# ---- the multi-resolution discriminator (Lee et al. 2023, section 3 and appendix; after UnivNet), plain torch over K36 --------------

MRD_RESOLUTIONS = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))     # (n_fft, hop, win)


def _hip_spectrogram(wav, n_fft, hop, win):
    ''' the default `spectrogram=` hook: `daft_exprt.spectrogram.spectrogram` (K36) over whole rows -> (B, bins, T) '''
    from daft_exprt.spectrogram import spectrogram
    return spectrogram(wav, [wav.shape[1]] * wav.shape[0], n_fft, hop, win=win)[0]


class DiscriminatorR(nn.Module):
    ''' one resolution (n_fft, hop, win): the magnitude spectrogram (B, 1, bins, T) -- reflect padding of (n_fft - hop) div 2, a
        rectangular window of `win` samples, no centring -- through Conv2d(1, 32 c, (3, 9)), three Conv2d(32 c, 32 c, (3, 9)) of stride
        (1, 2), Conv2d(32 c, 32 c, (3, 3)) and conv_post = Conv2d(32 c, 1, (3, 3)); leaky-ReLU 0.1 after each but the last.
        `spectrogram(wav (B, S), n_fft, hop, win) -> (B, bins, T)` replaces the HIP op (the host tests pass the CPU oracle). '''
    def __init__(self, resolution, channel_mult=1, use_spectral_norm=False, spectrogram=None):
        super().__init__()
        if len(resolution) != 3:
            raise ValueError(f'DiscriminatorR: a resolution is (n_fft, hop, win), got {resolution!r}')
        self.resolution = tuple(int(v) for v in resolution)
        self._spectrogram = _hip_spectrogram if spectrogram is None else spectrogram
        c = int(32 * channel_mult)
        convs = [nn.Conv2d(1, c, (3, 9), padding=(1, 4))]
        convs += [nn.Conv2d(c, c, (3, 9), stride=(1, 2), padding=(1, 4)) for _ in range(3)]
        convs.append(nn.Conv2d(c, c, (3, 3), padding=(1, 1)))
        self.convs = nn.ModuleList(VT._normed(conv, use_spectral_norm) for conv in convs)
        self.conv_post = VT._normed(nn.Conv2d(c, 1, (3, 3), padding=(1, 1)), use_spectral_norm)

    def check_segment(self, S):
        ''' raises ValueError naming the resolution where a segment of S samples is too short for it '''
        n_fft, hop, win = self.resolution
        p = (n_fft - hop) // 2
        if S <= p or S + 2 * p < n_fft:
            raise ValueError(f'DiscriminatorR: a segment of {S} samples is too short for the resolution (n_fft {n_fft}, hop {hop}, '
                             f'win {win}): reflect padding of {p} per side needs more than {p} samples')

    def forward(self, x):
        ''' x (B, 1, S) -> (scores (B, -1), feature maps) '''
        n_fft, hop, win = self.resolution
        self.check_segment(x.shape[2])
        x = self._spectrogram(x[:, 0], n_fft, hop, win)[:, None]
        fmap = []
        for conv in self.convs:
            x = F.leaky_relu(conv(x), VT.D_SLOPE)
            fmap.append(x)
        x = self.conv_post(x)
        fmap.append(x)
        return x.flatten(1), fmap


class MultiResolutionDiscriminator(nn.Module):
    ''' one `DiscriminatorR` per entry of the config's `resolutions` (default: the paper's three); `discriminator_channel_mult` and
        `use_spectral_norm` as upstream's config names them.  Returns what MPD / MSD return, so `train_step` takes it in their place. '''
    def __init__(self, config=None, spectrogram=None):
        super().__init__()
        config = config or {}
        resolutions = config.get('resolutions', MRD_RESOLUTIONS)
        if not resolutions:
            raise ValueError('MultiResolutionDiscriminator: the config\'s "resolutions" is empty')
        self.discriminators = nn.ModuleList(
            DiscriminatorR(r, config.get('discriminator_channel_mult', 1), bool(config.get('use_spectral_norm', False)), spectrogram)
            for r in resolutions)

    def check_segment(self, S):
        for d in self.discriminators:
            d.check_segment(S)

    def forward(self, y, y_hat):
        ''' y, y_hat (B, 1, S) -> (scores of y, scores of y_hat, feature maps of y, feature maps of y_hat), one entry per resolution '''
        out = [[], [], [], []]
        for d in self.discriminators:
            for k, x in enumerate((y, y_hat)):
                score, fmap = d(x)
                out[k].append(score)
                out[2 + k].append(fmap)
        return tuple(out)
