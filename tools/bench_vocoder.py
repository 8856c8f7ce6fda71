#!/usr/bin/env python
"""HiFi-GAN vocoder (V1 configuration, weights from a seed) on the mel of a configs[3]-shaped synthesis batch (B = 256,
`synthetic_inference_batch`) on one MI355X, `bf16` and `fp32` operands.

One JSON line: ms per `Vocoder.__call__` (device events, median of --reps after a warm-up), audio seconds per wall second, and per
layer kind -- conv_pre, the transposed convs, the ResBlock convs of each channel count, conv_post -- the FLOP and the minimum
bytes the algorithm needs (computed from the shapes here: every activation read and written once as fp32, weights once), the
device-event time of that kind's launches in one instrumented call (events around each launch: kernel time plus its launch gap),
the share of the bound and which bound it is (MFMA / vector peak or HBM: 2.5 PFLOP/s bf16, 157.3 TFLOP/s fp32, 8 TB/s, MI355X
spec); the Griffin-Lim preview of the same batch beside it.  Kernel times proper: run under `rocprofv3 --kernel-trace --stats`.
`--bigvgan` adds, under "bigvgan", the same measurement of a BigVGAN generator of the base layout (V1's shapes with `snakebeta`
activations, weights from a seed) on the same batch, with one more kind: `snake`, the launches of the anti-aliased activation
(`dx_vocoder_snake`), their bytes (every activation read and written once), their rate, that rate against the 6.29 TB/s a float4
copy reaches on this chip, and their share of the call.
Run:  python tools/bench_vocoder.py [--reps 5] [--batch 256] [--bigvgan]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'ubisoft-laforge-daft-exprt_amd')):
    sys.path.insert(0, p)

PEAK = {'bf16': 2.5e15, 'fp32': 157.3e12}
PEAK_HBM = 8.0e12
COPY_RATE = 6.29e12          # a float4 copy on this chip (measured; the guide's figure)


def _timed(fn, reps):
    ts, out = [], None
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out = fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    return float(np.median(ts)), out


def layer_costs(cfg, frames, w_bytes):
    ''' {kind: [flop, min bytes]} for `frames` live mel frames in total: 2 * rows * Cin * Cout * taps per conv; bytes = the input
        and the output once each as fp32 (+ the residual read, + the running sum's read-modify-write where it is used) + weights '''
    c0 = cfg['upsample_initial_channel']
    costs = {'conv_pre': [2. * frames * cfg['num_mels'] * c0 * 7, 4. * frames * (cfg['num_mels'] + c0) + w_bytes * cfg['num_mels'] * c0 * 7]}
    rows, c = frames, c0
    for i, (u, k) in enumerate(zip(cfg['upsample_rates'], cfg['upsample_kernel_sizes'])):
        up = costs.setdefault('upsample', [0., 0.])
        up[0] += 2. * rows * c * (c // 2) * k                        # every input row meets every tap once
        up[1] += 4. * rows * (c + u * (c // 2)) + w_bytes * c * (c // 2) * k
        rows, c = rows * u, c // 2
        res = costs.setdefault(f'resblock_c{c}', [0., 0.])
        for j, (rk, dils) in enumerate(zip(cfg['resblock_kernel_sizes'], cfg['resblock_dilation_sizes'])):
            for m in range(len(dils)):
                convs = 2 if str(cfg['resblock']) == '1' else 1
                res[0] += convs * 2. * rows * c * c * rk
                res[1] += convs * (4. * rows * 2 * c + w_bytes * c * c * rk) + 4. * rows * c      # + the residual read
                if m == len(dils) - 1 and j > 0:
                    res[1] += 4. * rows * c                                                    # the running sum is read back
    costs['conv_post'] = [2. * rows * c * 7, 4. * rows * (c + 1)]
    return costs


def snake_cost(cfg, frames):
    ''' [flop, min bytes] of every anti-aliased activation of a BigVGAN generator: per row and channel 24 + 24 multiply-adds of
        the two 12-tap filters (2 x 6 taps per upsampled sample, two of them per row; 12 per output) -- the two sinf are not counted
        -- and the activation read and written once as fp32 '''
    rows, c, flop, byts = frames, cfg['upsample_initial_channel'], 0., 0.
    per_block = sum(len(d) for d in cfg['resblock_dilation_sizes']) * (2 if str(cfg['resblock']) == '1' else 1)
    for i, u in enumerate(cfg['upsample_rates']):
        rows, c = rows * u, c // 2
        launches = per_block + (1 if i == len(cfg['upsample_rates']) - 1 else 0)               # + activation_post
        flop, byts = flop + launches * 2. * 36 * rows * c, byts + launches * 8. * rows * c
    return [flop, byts]


def per_kind_ms(voc, mel, lengths):
    ''' device-event time of each kind's launches in one call '''
    marks = []

    def wrap(fn, kind_of):
        def f(*a, **kw):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            out = fn(*a, **kw)
            e.record()
            marks.append((kind_of(a), s, e))
            return out
        return f
    conv, up, post, fed = voc._conv, voc._upsample, voc._post, voc._fed
    if voc.bigvgan:
        voc._fed = wrap(fed, lambda a: 'snake')
    voc._conv = wrap(conv, lambda a: 'conv_pre' if a[0] == 'conv_pre' else f'resblock_c{a[1].shape[2]}')
    voc._upsample = wrap(up, lambda a: 'upsample')
    voc._post = wrap(post, lambda a: 'conv_post')
    try:
        voc(mel, lengths)
        torch.cuda.synchronize()
    finally:
        voc._conv, voc._upsample, voc._post, voc._fed = conv, up, post, fed
    out = {}
    for kind, s, e in marks:
        out[kind] = out.get(kind, 0.) + s.elapsed_time(e)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--bigvgan', action='store_true', help='also measure a BigVGAN generator of the base layout (V1 + snakebeta)')
    args = ap.parse_args()
    import bench
    from daft_exprt import griffin_lim as G
    from daft_exprt.data_loader import centre_duration_head, synthetic_inference_batch
    from daft_exprt.model import DaftExprt
    from daft_exprt.vocoder import Vocoder
    from tests import vocoder_oracle as O
    dev = torch.device('cuda:0')
    hp = bench.make_hparams(args.batch, 'bf16')
    hp.stats = {f'spk {i}': {'pitch': {'mean': 5.0, 'std': 0.3}} for i in range(hp.n_speakers)}
    torch.manual_seed(hp.seed)
    model = DaftExprt(hp).to(dev).eval()
    centre_duration_head(model)
    inputs = tuple(t.to(dev) for t in synthetic_inference_batch(hp, args.batch, seed=1234))
    with torch.no_grad():
        _, (mel, lengths), _ = model.inference(tuple(t.clone() for t in inputs), 'add', hp)
    mel = mel.float().contiguous()
    del model
    B, _, T = mel.shape
    lens = lengths.cpu().numpy().astype(np.int64)
    frames = int(lens.sum())
    cfg = O.V1
    longest = int(np.argmax(lens))
    seed_mel = mel[longest:longest + 1, :, :12].cpu()                       # scales conv_post: the output stays inside tanh's range
    weights = O.make_weights(cfg, seed_mel, (12,), seed=0)
    audio_s = frames * cfg['hop_size'] / cfg['sampling_rate']
    out = {'metric': 'hifi_gan_vocoder', 'config': 'V1', 'batch': B, 'T_max': T, 'mel_frames': frames, 'audio_seconds': audio_s}

    def measure(cfg, state, dtype):
        voc = Vocoder(cfg, state, compute_dtype=dtype, device=dev)
        voc.check_hparams(hp)
        voc(mel, lengths)                                                    # warm-up: code objects, the workspace
        torch.cuda.synchronize()
        ms, (wavs, _) = _timed(lambda: voc(mel, lengths), args.reps)
        kinds = per_kind_ms(voc, mel, lengths)
        costs = layer_costs(cfg, frames, 2 if dtype == 'bf16' else 4)
        if voc.bigvgan:
            costs['snake'] = snake_cost(cfg, frames)
        layers = {}
        for kind, (flop, byts) in costs.items():
            t = kinds[kind] * 1e-3
            peak = PEAK['fp32'] if kind in ('conv_post', 'snake') else PEAK[dtype]   # VALU work in either mode
            t_c, t_m = flop / peak, byts / PEAK_HBM
            layers[kind] = {'gflop': flop / 1e9, 'gbytes': byts / 1e9, 'flop_per_byte': flop / byts, 'ms': kinds[kind],
                            'tflops': flop / t / 1e12, 'tbps': byts / t / 1e12, 'bound': 'compute' if t_c >= t_m else 'HBM',
                            'share_of_bound': max(t_c, t_m) / t}
        wide = [k for k in layers if k.startswith('resblock_c') and int(k[len('resblock_c'):]) >= 128]
        wide_flop, wide_s = sum(costs[k][0] for k in wide), sum(kinds[k] for k in wide) * 1e-3
        total_flop = sum(f for f, _ in costs.values())
        res = {'ms_per_call': ms, 'audio_s_per_wall_s': audio_s / (ms * 1e-3), 'tflop': total_flop / 1e12,
               'tflops_end_to_end': total_flop / (ms * 1e-3) / 1e12, 'peak_abs': float(wavs.abs().max()),
               'wide_stages_share_of_mfma_peak': wide_flop / wide_s / PEAK[dtype] if wide else None, 'layers': layers}
        if voc.bigvgan:
            res['snake_share_of_call'] = kinds['snake'] / sum(kinds.values())
            res['snake_rate_over_float4_copy'] = layers['snake']['tbps'] * 1e12 / COPY_RATE
        del voc
        torch.cuda.empty_cache()
        return res
    for dtype in ('bf16', 'fp32'):
        out[dtype] = measure(cfg, O.state_dict(weights), dtype)
    if args.bigvgan:
        from tests import bigvgan_oracle as BG
        big = dict(cfg, activation='snakebeta', snake_logscale=True)
        big_weights, raw, _, filters = BG.make_weights(big, seed_mel, (12,), seed=0)
        state = BG.state_dict(big, big_weights, raw, filters, form='plain')
        out['bigvgan'] = {'config': 'V1 + snakebeta'}
        for dtype in ('bf16', 'fp32'):
            out['bigvgan'][dtype] = measure(big, state, dtype)
    G.griffin_lim_batch(mel, lengths, hp)
    torch.cuda.synchronize()
    out['griffin_lim_preview_ms'], _ = _timed(lambda: G.griffin_lim_batch(mel, lengths, hp), args.reps)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
