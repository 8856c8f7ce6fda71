#!/usr/bin/env python
"""One step of HiFi-GAN's own fine-tuning (V1 generator, batch 16, segment 8192, weights from a seed) on one MI355X through
`daft_exprt/vocoder_train.py`, `fp32` and `bf16` operands.

One JSON line: ms per training step (device events, median of --reps after a warm-up), the share of one instrumented step that
goes to the generator's forward launches, its data-gradient launches, the gate / bias pointwise ops, `dx_vocoder_wgrad` with its reduce
launch, the discriminators (forward + backward, with the backward of the losses and of conv_post: what is left of the backward pass),
the losses and the optimisers (events around each piece: kernel time plus its launch gaps), `dx_vocoder_wgrad`'s TFLOP/s per input
channel width -- and, as yardstick, the same generator's forward + backward through `F.conv1d` / `F.conv_transpose1d` autograd on
the same device, weights and segment.  The yardstick lives here only: it is no path of the package.

`--bigvgan` adds, under "bigvgan", a BigVGAN generator of the base layout (V1's shapes with `snakebeta` activations in log scale,
weights from a seed) on the same batch and segment: its forward + backward ms in both operand types, and per stage the activation's
forward (`dx_vocoder_snake`) and backward (`dx_vocoder_snake_bwd`, with its reduce launch) alone, 20 launches per timed window -- ms, bytes (forward: x read and y
written; backward: x and dy read, dx written), TB/s, the rate against a float copy of the same bytes timed in the same run, the
tile height the backward's launcher chose -- and both launches' share of the generator's forward + backward.

`--mrd` adds, under "mrd", the fp32 step against MPD + BigVGAN's multi-resolution discriminator (`bigvgan_train`, under its recipe's
gradient clipping) beside the step against MPD + MSD, and per resolution the spectrogram launches alone (K36: `dx_spectrogram`, and
`dx_spectrogram_bwd` with its gather launch), 20 calls per timed window, against `torch.stft` + `torch.norm` + autograd on the same
device and waveforms -- a yardstick that lives here only -- and the share of a step that K36 takes: per resolution four forwards (y and
y_hat in either half of the step) and one backward.

`--mel_loss` adds, under "mel_loss", the fp32 step (MPD + MSD) with HiFi-GAN's single mel loss and with BigVGAN-v2's multi-scale one
(`mel_loss.MultiScaleMelLoss`, K37) from the same run, and per scale, 20 calls per timed window: the entry points alone on buffers
allocated once (`dx_mel_loss_log_mel` of the recording + `dx_mel_loss` of the synthesis: three launches), the same through the Python
wrappers with the autograd backward (`log_mel` + `log_mel_l1` + `.backward()`), and `torch.stft` + filter bank + log10 + L1 + autograd
on the same device and waveforms -- a yardstick that lives here only.
Run:  python tools/bench_vocoder_train.py [--reps 5] [--batch 16] [--segment 8192] [--bigvgan] [--mrd] [--mel_loss]
"""
import argparse
import json
import os
import sys
import warnings

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'ubisoft-laforge-daft-exprt_amd')):
    sys.path.insert(0, p)


def _events():
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def _timed(fn, reps):
    ts = []
    for _ in range(reps):
        s, e = _events()
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    return float(np.median(ts))


class Marks:
    ''' device-event pairs per kind; `wrap` times every call of a function, `span` a block '''
    def __init__(self):
        self.marks, self.flop = [], {}

    def wrap(self, fn, kind_of, flop_of=None):
        def f(*a, **kw):
            s, e = _events()
            s.record()
            out = fn(*a, **kw)
            e.record()
            kind = kind_of(*a, **kw)
            self.marks.append((kind, s, e))
            if flop_of is not None:
                key, flop = flop_of(*a, **kw)
                self.flop.setdefault(key, []).append((flop, s, e))
            return out
        return f

    def span(self, kind):
        marks = self.marks

        class _Span:
            def __enter__(self):
                self.s, self.e = _events()
                self.s.record()

            def __exit__(self, *exc):
                self.e.record()
                marks.append((kind, self.s, self.e))
        return _Span()

    def totals(self):
        out = {}
        for kind, s, e in self.marks:
            out[kind] = out.get(kind, 0.) + s.elapsed_time(e)
        return out


def torch_generator(cfg, weights, mel):
    ''' the yardstick: HiFi-GAN's generator on torch's own convolutions, (B, C, T) layout, no sequence ends '''
    nk = len(cfg['resblock_kernel_sizes'])
    lrelu = lambda x, s=0.1: F.leaky_relu(x, s)      # noqa: E731
    conv = lambda x, name, d: F.conv1d(x, *weights[name], dilation=d, padding=d * (weights[name][0].shape[2] - 1) // 2)      # noqa: E731
    x = conv(mel, 'conv_pre', 1)
    for i, (u, k) in enumerate(zip(cfg['upsample_rates'], cfg['upsample_kernel_sizes'])):
        x = F.conv_transpose1d(lrelu(x), *weights[f'ups.{i}'], stride=u, padding=(k - u) // 2)
        total = None
        for j, dils in enumerate(cfg['resblock_dilation_sizes']):
            r, name = x, f'resblocks.{i * nk + j}'
            for m, d in enumerate(dils):
                if str(cfg['resblock']) == '1':
                    r = r + conv(lrelu(conv(lrelu(r), f'{name}.convs1.{m}', d)), f'{name}.convs2.{m}', 1)
                else:
                    r = r + conv(lrelu(r), f'{name}.convs.{m}', d)
            total = r if total is None else total + r
        x = total / nk
    return torch.tanh(conv(lrelu(x, 0.01), 'conv_post', 1))[:, 0]


def instrumented_step(VT, generator, mpd, msd, optim_g, optim_d, loss_mel, mel, audio):
    ''' `vocoder_train.train_step` with events around its pieces; returns (share of the step per piece, wgrad TFLOP/s per width) '''
    mk = Marks()
    saved = {n: getattr(VT, n) for n in ('conv_forward', 'upsample_forward', 'conv_wgrad', 'upsample_wgrad', '_gate', '_bias_grad')}
    VT.conv_forward = mk.wrap(saved['conv_forward'], lambda x, wp, bias, *a, **kw: 'generator_data_gradients' if bias is None else 'generator_forward')
    VT.upsample_forward = mk.wrap(saved['upsample_forward'], lambda *a, **kw: 'generator_forward')
    VT.conv_wgrad = mk.wrap(saved['conv_wgrad'], lambda *a, **kw: 'wgrad',
                            lambda x, dy, n, k, *a, **kw: (x.shape[2], 2. * x.shape[0] * x.shape[1] * x.shape[2] * dy.shape[2] * k))
    VT.upsample_wgrad = mk.wrap(saved['upsample_wgrad'], lambda *a, **kw: 'wgrad',
                                lambda x, dy, n, k, *a, **kw: (x.shape[2], 2. * x.shape[0] * x.shape[1] * x.shape[2] * dy.shape[2] * k))
    VT._gate = mk.wrap(saved['_gate'], lambda *a, **kw: 'gate_bias_pointwise')
    VT._bias_grad = mk.wrap(saved['_bias_grad'], lambda *a, **kw: 'gate_bias_pointwise')
    try:
        B, _, frames = mel.shape
        lengths = torch.full((B,), frames, dtype=torch.int64, device=mel.device)
        y = audio[:, None]
        whole_s, whole_e = _events()
        whole_s.record()
        with mk.span('generator_forward_all'):
            y_hat = generator(mel, lengths)[:, None]
        optim_d.zero_grad(set_to_none=True)
        with mk.span('discriminators'):
            loss_d = 0.
            for disc in (mpd, msd):
                real, fake, _, _ = disc(y, y_hat.detach())
                loss_d = loss_d + VT.discriminator_loss(real, fake)
            loss_d.backward()
        with mk.span('optimisers'):
            optim_d.step()
        optim_g.zero_grad(set_to_none=True)
        with mk.span('losses'):
            l_mel = VT.mel_l1(loss_mel(audio), loss_mel(y_hat[:, 0]))
        l_adv, l_fm = 0., 0.
        with mk.span('discriminators'):
            outs = [disc(y, y_hat) for disc in (mpd, msd)]
        with mk.span('losses'):
            for _, fake, fmap_r, fmap_g in outs:
                l_adv = l_adv + VT.generator_adversarial_loss(fake)
                l_fm = l_fm + VT.feature_matching_loss(fmap_r, fmap_g)
            loss = l_adv + l_fm + VT.MEL_LOSS_WEIGHT * l_mel
        with mk.span('backward_all'):
            loss.backward()
        with mk.span('optimisers'):
            optim_g.step()
        whole_e.record()
        torch.cuda.synchronize()
    finally:
        for n, fn in saved.items():
            setattr(VT, n, fn)
    t = mk.totals()
    whole = whole_s.elapsed_time(whole_e)
    inside = sum(t.get(k, 0.) for k in ('generator_data_gradients', 'wgrad', 'gate_bias_pointwise'))
    # the forward launches of the generator run inside generator_forward_all; what the backward pass holds beside the generator's
    # launches is the discriminators' backward, the losses' and conv_post's
    pieces = {'generator_forward': t.pop('generator_forward_all'), 'generator_data_gradients': t.get('generator_data_gradients', 0.),
              'gate_bias_pointwise': t.get('gate_bias_pointwise', 0.), 'wgrad_with_reduce': t.get('wgrad', 0.),
              'discriminators_forward_backward': t.get('discriminators', 0.) + t['backward_all'] - inside,
              'losses': t.get('losses', 0.), 'optimisers': t.get('optimisers', 0.)}
    share = {k: v / whole for k, v in pieces.items()}
    share['unaccounted'] = 1. - sum(share.values())
    rate = {str(width): sum(f for f, _, _ in calls) / (sum(s.elapsed_time(e) for _, s, e in calls) * 1e-3) / 1e12
            for width, calls in sorted(mk.flop.items())}
    return whole, share, rate


LAUNCHES = 20


def launcher_tile_rows(H, B, N, C):
    ''' the height `dx_vocoder_snake_bwd` picks for tile_rows = 0, by the rule the header states: the largest supported height that
        still gives 65536 threads, else the smallest '''
    heights, i = [], 0
    while H.lib().dx_vocoder_snake_bwd_tile_rows(i) > 0:
        heights.append(H.lib().dx_vocoder_snake_bwd_tile_rows(i))
        i += 1
    fits = [h for h in heights if B * -(-N // h) * (C // 4) >= 65536]
    return max(fits) if fits else min(heights)


def bigvgan(args, base_cfg, mel, proj, lengths, dev):
    ''' the "bigvgan" entry of the result '''
    import ctypes
    from daft_exprt import _hip as H
    from daft_exprt import bigvgan_train as BT
    from daft_exprt import vocoder_train as VT
    from tests import bigvgan_oracle as BO
    from tests import vocoder_oracle as O
    cfg = dict(base_cfg, activation='snakebeta', snake_logscale=True)
    seed_mel = O.make_mel(cfg, (12,), seed=0)
    weights, raw, _, filters = BO.make_weights(cfg, seed_mel, (12,), seed=0)
    sd = BO.state_dict(cfg, weights, raw, filters, form='weight_norm')
    out = {'config': 'V1 + snakebeta (log scale)', 'activations': len(BO.fed_convs(cfg))}
    for dtype in ('fp32', 'bf16'):
        generator = VT.trainable_generator(cfg, sd, compute_dtype=dtype).to(dev)

        def gen_fwd_bwd():
            for p in generator.parameters():
                p.grad = None
            (generator(mel, lengths) * proj).sum().backward()
        for _ in range(2):
            gen_fwd_bwd()
        torch.cuda.synchronize()
        out[dtype] = {'generator_forward_backward_ms': _timed(gen_fwd_bwd, args.reps)}
        del generator
        torch.cuda.empty_cache()
    # the activation alone, per stage: rows and channels of the stage, as many launches per step as the stage has activations
    g = torch.Generator().manual_seed(2)
    taps = (ctypes.c_float * 24)(*filters[0].tolist(), *filters[1].tolist())
    nk, rows, c = len(cfg['resblock_kernel_sizes']), args.segment // cfg['hop_size'], cfg['upsample_initial_channel']
    per_block = sum(2 * len(d) for d in cfg['resblock_dilation_sizes'])
    stages, fwd_total, bwd_total = [], 0., 0.
    for i, u in enumerate(cfg['upsample_rates']):
        rows, c = rows * u, c // 2
        last = i == len(cfg['upsample_rates']) - 1
        count = per_block + (1 if last else 0)                          # activation_post runs at the last stage's shape
        x, dy = (torch.randn((args.batch, rows, c), generator=g).to(dev) for _ in range(2))
        alpha, inv_beta = (t.to(dev) for t in BO.final_params(0.5 * torch.randn((c,), generator=g), 0.5 * torch.randn((c,), generator=g), True))
        n = torch.full((args.batch,), rows, dtype=torch.int64, device=dev)
        y = torch.empty_like(x)
        fwd = lambda: H.check(H.lib().dx_vocoder_snake(H.ptr(x), c, H.ptr(alpha), H.ptr(inv_beta), ctypes.addressof(taps), H.ptr(y), c,      # noqa: E731
                                                       H.ptr(n), args.batch, rows, c, H.stream()))
        bwd = lambda: BT.snake_backward(x, dy, alpha, inv_beta, taps, n)      # noqa: E731
        el = args.batch * rows * c
        entry = {'stage': i, 'rows': rows, 'channels': c, 'launches_per_step': count,
                 'backward_tile_rows': launcher_tile_rows(H, args.batch, rows, c), 'forward_tile_rows': H.lib().dx_vocoder_snake_tile_rows()}
        for name, fn, n_bytes in (('forward', fwd, 8 * el), ('backward', bwd, 12 * el)):
            src = torch.empty(n_bytes // 8, dtype=torch.float32, device=dev).normal_()
            dst = torch.empty_like(src)
            copy = lambda: dst.copy_(src)      # noqa: E731
            for f in (fn, copy):
                f()
                f()
            torch.cuda.synchronize()
            # LAUNCHES calls per timed window: one launch of 0.1 ms between two events is as much the events as the kernel
            ms, copy_ms = (_timed(lambda f=f: [f() for _ in range(LAUNCHES)], args.reps) / LAUNCHES for f in (fn, copy))
            entry[name] = {'ms': ms, 'bytes': n_bytes, 'tbps': n_bytes / (ms * 1e-3) / 1e12, 'copy_ms': copy_ms,
                           'rate_over_copy': copy_ms / ms}
            del src, dst
        fwd_total += count * entry['forward']['ms']
        bwd_total += count * entry['backward']['ms']
        stages.append(entry)
    out['snake_stages'] = stages
    out['snake_forward_ms_per_step'], out['snake_backward_ms_per_step'] = fwd_total, bwd_total
    for dtype in ('fp32', 'bf16'):
        whole = out[dtype]['generator_forward_backward_ms']
        out[dtype]['snake_forward_share'], out[dtype]['snake_backward_share'] = fwd_total / whole, bwd_total / whole
    return out


def mrd(args, cfg, sd, mel, audio, loss_mel, dev):
    ''' the "mrd" entry of the result '''
    from daft_exprt import bigvgan_train as BT
    from daft_exprt import vocoder_train as VT
    from daft_exprt.spectrogram import spectrogram
    out = {}
    for second in ('msd', 'mrd'):
        torch.manual_seed(0)
        generator = VT.TrainableGenerator(cfg, sd, compute_dtype='fp32').to(dev)
        mpd = VT.MultiPeriodDiscriminator().to(dev)
        other = (VT.MultiScaleDiscriminator() if second == 'msd' else BT.MultiResolutionDiscriminator(cfg)).to(dev)
        lr, clip = (VT.LEARNING_RATE, None) if second == 'msd' else (VT.MRD_LEARNING_RATE, VT.MRD_CLIP_GRAD_NORM)
        optim_g = torch.optim.AdamW(generator.parameters(), lr, betas=VT.ADAM_BETAS)
        optim_d = torch.optim.AdamW(list(other.parameters()) + list(mpd.parameters()), lr, betas=VT.ADAM_BETAS)
        step = lambda: VT.train_step(generator, mpd, other, optim_g, optim_d, loss_mel, mel, audio, clip_grad_norm=clip)      # noqa: E731
        for _ in range(2):
            step()
        torch.cuda.synchronize()
        out[f'mpd_{second}_ms_per_step'] = _timed(step, args.reps)
        del generator, mpd, other, optim_g, optim_d
        torch.cuda.empty_cache()
    counts, k36_ms, entries = [args.segment] * args.batch, 0., []
    for n_fft, hop, win in BT.MRD_RESOLUTIONS:
        x = audio.clone().requires_grad_(True)
        mag, frames = spectrogram(x, counts, n_fft, hop, win=win)
        dmag = torch.randn_like(mag)
        p = (n_fft - hop) // 2

        def hip_fwd():
            with torch.no_grad():
                spectrogram(audio, counts, n_fft, hop, win=win)

        def hip_fwd_bwd():
            x.grad = None
            spectrogram(x, counts, n_fft, hop, win=win)[0].backward(dmag)

        def stft_mag(w):
            spec = torch.stft(F.pad(w[:, None], (p, p), mode='reflect')[:, 0], n_fft, hop_length=hop, win_length=win, window=None,
                              center=False, return_complex=True)
            return torch.norm(torch.view_as_real(spec), p=2, dim=-1)

        def torch_fwd():
            with torch.no_grad():
                stft_mag(audio)

        def torch_fwd_bwd():
            x.grad = None
            stft_mag(x).backward(dmag)
        assert tuple(stft_mag(audio).shape) == tuple(mag.shape)
        ms = {}
        for name, fn in (('k36_forward', hip_fwd), ('k36_forward_backward', hip_fwd_bwd), ('torch_stft_forward', torch_fwd),
                         ('torch_stft_forward_backward', torch_fwd_bwd)):
            fn()
            fn()
            torch.cuda.synchronize()
            ms[name + '_ms'] = _timed(lambda fn=fn: [fn() for _ in range(LAUNCHES)], args.reps) / LAUNCHES
        ms['forward_speedup'] = ms['torch_stft_forward_ms'] / ms['k36_forward_ms']
        ms['forward_backward_speedup'] = ms['torch_stft_forward_backward_ms'] / ms['k36_forward_backward_ms']
        k36_ms += 3 * ms['k36_forward_ms'] + ms['k36_forward_backward_ms']
        entries.append(dict({'n_fft': n_fft, 'hop': hop, 'win': win, 'frames_per_batch': int(frames.sum())}, **ms))
    out['resolutions'] = entries
    out['k36_ms_per_step'], out['k36_share_of_step'] = k36_ms, k36_ms / out['mpd_mrd_ms_per_step']
    return out


def mel_loss(args, cfg, sd, mel, audio, loss_mel, dev):
    ''' the "mel_loss" entry of the result '''
    import ctypes
    from daft_exprt import _hip as H
    from daft_exprt import mel_loss as ML
    from daft_exprt import vocoder_train as VT
    out = {}
    module = ML.MultiScaleMelLoss(cfg)
    for kind, mod in (('single', None), ('multiscale', module)):
        torch.manual_seed(0)
        generator = VT.TrainableGenerator(cfg, sd, compute_dtype='fp32').to(dev)
        mpd, msd = VT.MultiPeriodDiscriminator().to(dev), VT.MultiScaleDiscriminator().to(dev)
        optim_g = torch.optim.AdamW(generator.parameters(), VT.LEARNING_RATE, betas=VT.ADAM_BETAS)
        optim_d = torch.optim.AdamW(list(msd.parameters()) + list(mpd.parameters()), VT.LEARNING_RATE, betas=VT.ADAM_BETAS)
        step = lambda: VT.train_step(generator, mpd, msd, optim_g, optim_d, loss_mel, mel, audio, mel_loss=mod)      # noqa: E731
        for _ in range(2):
            step()
        torch.cuda.synchronize()
        out[f'{kind}_ms_per_step'] = _timed(step, args.reps)
        del generator, mpd, msd, optim_g, optim_d
        torch.cuda.empty_cache()
    B, S = audio.shape
    counts = [S] * B
    y_hat = (audio + 0.05 * torch.randn_like(audio)).contiguous()
    entries, launches_ms, call_ms = [], 0., 0.
    for s in module.scales:
        T, M = s.frames(S), s.n_mels
        factor = 1. / (M * B * T)
        tw, win, fb, fb_lo, fb_hi, bin_lo, bin_hi = s.tables(dev)
        nd, nh = torch.tensor(counts, dtype=torch.int64, device=dev), (ctypes.c_int64 * B)(*counts)
        target, loss, dwav = torch.empty((B, T, M), device=dev), torch.empty((B,), device=dev), torch.empty((B, S), device=dev)
        ws = torch.empty((H.lib().dx_mel_loss_workspace(B, T, M, s.n_fft) // 4,), device=dev)
        x = y_hat.clone().requires_grad_(True)
        window = win.clone()

        def launches():
            H.check(H.lib().dx_mel_loss_log_mel(H.ptr(audio), S, H.ptr(nd), ctypes.addressof(nh), H.ptr(tw), H.ptr(win), H.ptr(fb),
                                                H.ptr(fb_lo), H.ptr(fb_hi), H.ptr(target), B, S, T, M, s.n_fft, s.hop, s.pad, s.eps, H.stream()))
            H.check(H.lib().dx_mel_loss(H.ptr(y_hat), S, H.ptr(nd), ctypes.addressof(nh), H.ptr(tw), H.ptr(win), H.ptr(fb), H.ptr(fb_lo),
                                        H.ptr(fb_hi), H.ptr(bin_lo), H.ptr(bin_hi), H.ptr(target), factor, H.ptr(loss), H.ptr(dwav), S, None,
                                        H.ptr(ws), B, S, T, M, s.n_fft, s.hop, s.pad, s.eps, H.stream()))

        def calls():
            x.grad = None
            ML.log_mel_l1(x, ML.log_mel(audio, counts, s), counts, s, factor).backward()

        def torch_log_mel(w):
            spec = torch.stft(w, s.n_fft, hop_length=s.hop, win_length=s.n_fft, window=window, center=True, pad_mode='reflect',
                              return_complex=True)
            return torch.log10(torch.clamp(fb @ spec.abs(), min=s.eps))

        def yardstick():
            x.grad = None
            with torch.no_grad():
                t = torch_log_mel(audio)
            F.l1_loss(torch_log_mel(x), t).backward()
        assert tuple(torch_log_mel(audio).shape) == (B, M, T)
        ms = {}
        for name, fn in (('k37_launches', launches), ('k37_calls_with_autograd', calls), ('torch_stft_autograd', yardstick)):
            fn()
            fn()
            torch.cuda.synchronize()
            ms[name + '_ms'] = _timed(lambda fn=fn: [fn() for _ in range(LAUNCHES)], args.reps) / LAUNCHES
        ms['speedup_of_the_calls'] = ms['torch_stft_autograd_ms'] / ms['k37_calls_with_autograd_ms']
        launches_ms += ms['k37_launches_ms']
        call_ms += ms['k37_calls_with_autograd_ms']
        entries.append(dict({'n_fft': s.n_fft, 'hop': s.hop, 'n_mels': M, 'frames_per_batch': B * T}, **ms))
    out['scales'] = entries
    out['k37_launches_ms_per_step'], out['k37_calls_ms_per_step'] = launches_ms, call_ms
    out['k37_calls_share_of_step'] = call_ms / out['multiscale_ms_per_step']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--segment', type=int, default=8192)
    ap.add_argument('--bigvgan', action='store_true', help='also measure a BigVGAN generator of the base layout (V1 + snakebeta)')
    ap.add_argument('--mrd', action='store_true', help="also measure the step against BigVGAN's multi-resolution discriminator and K36")
    ap.add_argument('--mel_loss', action='store_true', help="also measure the step with BigVGAN-v2's multi-scale mel loss and K37")
    args = ap.parse_args()
    warnings.simplefilter('ignore')
    from daft_exprt import vocoder_train as VT
    from tests import vocoder_oracle as O
    dev = torch.device('cuda:0')
    cfg = dict(O.V1, n_fft=1024, win_size=1024, fmin=0, fmax=8000, fmax_for_loss=None)
    frames = args.segment // cfg['hop_size']
    seed_mel = O.make_mel(cfg, (12,), seed=0)
    weights = O.make_weights(cfg, seed_mel, (12,), seed=0)
    sd = O.state_dict(weights, 'weight_norm')
    g = torch.Generator().manual_seed(1)
    mel = (torch.randn((args.batch, cfg['num_mels'], frames), generator=g) * 1.5 - 4.).to(dev)
    audio = (0.1 * torch.randn((args.batch, args.segment), generator=g)).to(dev)
    proj = torch.randn((args.batch, args.segment), generator=g).to(dev)
    lengths = torch.full((args.batch,), frames, dtype=torch.int64, device=dev)
    out = {'metric': 'hifi_gan_fine_tuning_step', 'config': 'V1', 'batch': args.batch, 'segment': args.segment}
    torch.manual_seed(0)
    loss_mel = VT.LossMel(cfg).to(dev)
    for dtype in ('fp32', 'bf16'):
        generator = VT.TrainableGenerator(cfg, sd, compute_dtype=dtype).to(dev)
        mpd, msd = VT.MultiPeriodDiscriminator().to(dev), VT.MultiScaleDiscriminator().to(dev)
        optim_g = torch.optim.AdamW(generator.parameters(), VT.LEARNING_RATE, betas=VT.ADAM_BETAS)
        optim_d = torch.optim.AdamW(list(msd.parameters()) + list(mpd.parameters()), VT.LEARNING_RATE, betas=VT.ADAM_BETAS)
        step = lambda: VT.train_step(generator, mpd, msd, optim_g, optim_d, loss_mel, mel, audio)      # noqa: E731
        for _ in range(2):                                                    # warm-up: code objects, workspaces, torch's conv choices
            step()
        torch.cuda.synchronize()
        ms = _timed(step, args.reps)
        whole, share, rate = instrumented_step(VT, generator, mpd, msd, optim_g, optim_d, loss_mel, mel, audio)

        def gen_fwd_bwd():
            for p in generator.parameters():
                p.grad = None
            (generator(mel, lengths) * proj).sum().backward()
        gen_fwd_bwd()
        torch.cuda.synchronize()
        out[dtype] = {'ms_per_step': ms, 'instrumented_step_ms': whole, 'share': share, 'wgrad_tflops_by_cin': rate,
                      'generator_forward_backward_ms': _timed(gen_fwd_bwd, args.reps)}
        del generator, mpd, msd, optim_g, optim_d
        torch.cuda.empty_cache()
    tw = {name: (w.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)) for name, (w, b) in weights.items()}

    def torch_fwd_bwd():
        for w, b in tw.values():
            w.grad = b.grad = None
        (torch_generator(cfg, tw, mel) * proj).sum().backward()
    for _ in range(2):
        torch_fwd_bwd()
    torch.cuda.synchronize()
    out['torch_conv1d_generator_forward_backward_ms'] = _timed(torch_fwd_bwd, args.reps)
    del tw
    torch.cuda.empty_cache()
    if args.bigvgan:
        out['bigvgan'] = bigvgan(args, cfg, mel, proj, lengths, dev)
    if args.mrd:
        out['mrd'] = mrd(args, cfg, sd, mel, audio, loss_mel, dev)
    if args.mel_loss:
        out['mel_loss'] = mel_loss(args, cfg, sd, mel, audio, loss_mel, dev)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
