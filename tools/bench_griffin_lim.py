#!/usr/bin/env python
"""Griffin-Lim preview audio of a configs[3]-shaped synthesis batch (B = 256, `synthetic_inference_batch`) on one MI355X.

One JSON line: device-event times (median of --reps after a warm-up) of mel -> linear (NNLS), 30 Griffin-Lim iterations,
normalise and their total; the synthesis forward (`model.inference`) of the same batch timed in the same run; audio seconds
per wall second; algorithmic FLOPs / bytes per stage from the shapes with the share of peak and the bound that sets it
(157.3 TFLOP/s fp32 vector, 8 TB/s HBM: MI355X spec); a CPU baseline -- the float64 restatement of the reference
(tests/griffin_lim_oracle.py: its Griffin-Lim loop over a frame matrix, the reference's scipy L-BFGS-B NNLS when scipy
imports, else null) on the 2 shortest utterances of the batch.  Kernel times: run under `rocprofv3 --kernel-trace --stats` separately.
Run:  python tools/bench_griffin_lim.py [--reps 5] [--no-cpu]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'ubisoft-laforge-daft-exprt_amd')):
    sys.path.insert(0, p)

PEAK_F32, PEAK_HBM = 157.3e12, 8.0e12


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


def _roof(flop, byts, ms):
    t_c, t_m = flop / PEAK_F32, byts / PEAK_HBM
    return {'gflop': flop / 1e9, 'gbytes': byts / 1e9, 'ms': ms, 'tflops': flop / (ms * 1e-3) / 1e12,
            'tbps': byts / (ms * 1e-3) / 1e12, 'bound': 'fp32 vector' if t_c >= t_m else 'HBM',
            'frac_of_peak': max(t_c, t_m) / (ms * 1e-3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--no-cpu', action='store_true')
    args = ap.parse_args()
    import bench
    from daft_exprt import _hip as H
    from daft_exprt import griffin_lim as G
    from daft_exprt.data_loader import centre_duration_head, synthetic_inference_batch
    from daft_exprt.model import DaftExprt
    from tests import griffin_lim_oracle as O
    dev = torch.device('cuda:0')
    hp = bench.make_hparams(args.batch, 'bf16')
    hp.stats = {f'spk {i}': {'pitch': {'mean': 5.0, 'std': 0.3}} for i in range(hp.n_speakers)}
    torch.manual_seed(hp.seed)
    model = DaftExprt(hp).to(dev).eval()
    centre_duration_head(model)
    inputs = tuple(t.to(dev) for t in synthetic_inference_batch(hp, args.batch, seed=1234))
    n_fft, hop, n_mel, sr = hp.filter_length, hp.hop_length, hp.n_mel_channels, hp.sampling_rate
    nb = n_fft // 2 + 1
    with torch.no_grad():
        for _ in range(3):
            _, (mel, lengths), _ = model.inference(tuple(t.clone() for t in inputs), 'add', hp)
        torch.cuda.synchronize()
        synth_ms, _ = _timed(lambda: model.inference(tuple(t.clone() for t in inputs), 'add', hp), args.reps)
    mel = mel.float().contiguous()
    B, _, T = mel.shape
    S = G.n_samples(T, hp)
    G.griffin_lim_batch(mel, lengths, hp)                                    # warm-up (tables, code objects)
    torch.cuda.synchronize()
    nnls_ms, lin = _timed(lambda: G.mel_to_linear_batch(mel, lengths, hp), args.reps)
    gl_ms, (wav, n) = _timed(lambda: G.griffin_lim_from_linear(lin, lengths, hp, iterations=G.GL_ITERS, seed=0, normalise=False),
                             args.reps)
    norm_ms, _ = _timed(lambda: H.check(H.lib().dx_gl_normalise(H.ptr(wav), S, H.ptr(lengths), B, T, n_fft, hop, H.stream())),
                        args.reps)
    total_ms, _ = _timed(lambda: G.griffin_lim_batch(mel, lengths, hp), args.reps)
    lens = lengths.cpu().numpy().astype(np.int64)
    frames = int(lens.sum())
    gl_frames = int(np.maximum(lens - 2, 0).sum())
    samples = int(n.sum().item())
    fb = O.filterbank(hp)
    nnz = int((fb > 0).sum())
    it = G.NNLS_ITERS
    nnls_flop = frames * (2. * n_mel * nb + it * (2. * nnz + 4. * nb + 5. * nb))    # pinv start; A y, A^T r, FISTA update
    nnls_bytes = frames * (n_mel * 4. + nb * 4.)
    fft_flop = 2.5 * n_fft * np.log2(n_fft)                                          # one real FFT of n_fft points
    gl_flop = G.GL_ITERS * gl_frames * (2 * fft_flop + 6. * n_fft + 10. * nb + 4. * n_fft)
    gl_bytes = G.GL_ITERS * gl_frames * ((hop + nb + n_fft) * 4. + (n_fft + hop) * 4.)
    norm_bytes = 3. * samples * 4.
    audio_s = samples / sr
    out = {'metric': 'griffin_lim_preview', 'batch': B, 'T_max': T, 'mel_frames': frames, 'gl_frames': gl_frames,
           'nnls_iters': it, 'gl_iters': G.GL_ITERS, 'synth_forward_ms': synth_ms,
           'mel_to_linear_ms': nnls_ms, 'griffin_lim_ms': gl_ms, 'normalise_ms': norm_ms, 'total_ms': total_ms,
           'total_over_synth': total_ms / synth_ms, 'gate_4x': total_ms <= 4 * synth_ms, 'aim_1x': total_ms <= synth_ms,
           'audio_seconds': audio_s, 'audio_s_per_wall_s': audio_s / (total_ms * 1e-3),
           'audio_s_per_wall_s_with_synth': audio_s / ((total_ms + synth_ms) * 1e-3),
           'roofline': {'mel_to_linear': _roof(nnls_flop, nnls_bytes, nnls_ms), 'griffin_lim': _roof(gl_flop, gl_bytes, gl_ms),
                        'normalise': _roof(0., norm_bytes, norm_ms)},
           'cpu_baseline': None}
    print(json.dumps(out), file=sys.stderr, flush=True)                     # the device numbers, before the slow CPU leg
    if not args.no_cpu:
        idx = [int(i) for i in np.argsort(lens)[:2]]                             # the two shortest utterances
        cpu = {'utterances': idx, 'mel_frames': [int(lens[i]) for i in idx], 'gl_s': 0., 'nnls_s': None}
        mels = mel.cpu().numpy()
        lin_np = lin.cpu().numpy()
        for i in idx:
            F = int(lens[i]) - 2
            t0 = time.perf_counter()
            O.griffin_lim(lin_np[i, :, :F].astype(np.float64), hop, G.GL_ITERS, np.random.RandomState(i).randn(F * hop + n_fft))
            cpu['gl_s'] += time.perf_counter() - t0
        try:
            import scipy.optimize  # noqa: F401
            cpu['nnls_s'] = 0.
            for i in idx:
                t0 = time.perf_counter()
                O.nnls_lbfgs(fb, np.exp(mels[i, :, :int(lens[i])]))
                cpu['nnls_s'] += time.perf_counter() - t0
        except ImportError:
            pass
        cpu['audio_seconds'] = sum((int(lens[i]) - 2) * hop + n_fft for i in idx) / sr
        cpu['ms_per_frame_gl'] = cpu['gl_s'] * 1e3 / sum(cpu['mel_frames'])
        cpu['ms_per_frame_nnls'] = None if cpu['nnls_s'] is None else cpu['nnls_s'] * 1e3 / sum(cpu['mel_frames'])
        out['cpu_baseline'] = cpu
    print(json.dumps(out))


if __name__ == '__main__':
    main()
