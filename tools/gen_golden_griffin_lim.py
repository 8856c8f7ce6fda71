#!/usr/bin/env python
"""Fixture for the Griffin-Lim preview path: runs the REFERENCE's `griffin_lim.py` (`mel_to_linear`,
`reconstruct_signal_griffin_lim`, `griffin_lim_reconstruction_from_mel_spec`) in the build container and stores inputs +
outputs in tests/golden/griffin_lim.npz.

`librosa.filters.mel` is replaced by the restatement `oracle.mel_frontend_cpu.mel_filterbank`, as in
tools/gen_golden_mel_frontend.py; everything else (scipy's L-BFGS-B NNLS, the Griffin-Lim loop, the normalisation) is the
reference's own code.  Contents:
  nnls_<case>_mel      log-mels (n_mel, T) float32: `dec` (decoder output of tests/golden/inference.npz), `cone` (exactly
                       A x for a random x >= 0), `noisy` (cone + log-domain noise), `edge` (T = 3)
  nnls_<case>_relres   the reference's per-frame || A x - exp(mel) || / || exp(mel) || (float64)
  gl_<T>_seed          np.random.seed used right before the reference drew its start signal
  gl_<T>_sig1 / _sig30 signal after 1 / 30 iterations (float32) from magnitudes tests.griffin_lim_oracle.harmonic_magnitude(T)
                       cropped like the reference ([:, :-2]) (sig1: T < 100 only); gl_24_norm30 = sig30 / max|sig30|
                       (griffin_lim.py:196)
  pipe_mel / pipe_seed / pipe_wav   griffin_lim_reconstruction_from_mel_spec end to end (float32 output)
Run:  python tools/gen_golden_griffin_lim.py
"""
import logging
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import gen_goldens  # noqa: E402  (shims + hparams helper)
from oracle.mel_frontend_cpu import mel_filterbank  # noqa: E402
from tests import griffin_lim_oracle as O  # noqa: E402

GL_T = (3, 24, 64, 100)


def main():
    gen_goldens.install_shims()
    sys.modules['librosa.filters'].mel = lambda sr, n_fft, n_mels, fmin, fmax: mel_filterbank(sr, n_fft, n_mels, fmin, fmax)
    import daft_exprt.hparams as ref_hparams
    import daft_exprt.griffin_lim as ref_gl
    ref_gl.librosa_mel_fn = sys.modules['librosa.filters'].mel
    log = logging.getLogger('gen_golden_griffin_lim')
    hp = gen_goldens.make_hparams(ref_hparams)
    A = O.filterbank(hp)
    rng = np.random.RandomState(2024)
    inf = np.load(os.path.join(gen_goldens.OUT, 'inference.npz'))
    t0 = int(inf['add_out_output_lengths'][0])
    x_cone = np.abs(rng.randn(A.shape[1], 40)) * np.exp(-np.arange(A.shape[1]) / 150.)[:, None]
    cone = np.log(A.astype(np.float64) @ x_cone)
    noisy = cone + 0.3 * rng.randn(*cone.shape)
    mels = {'dec': inf['add_out_mel'][0][:, :t0], 'cone': cone, 'noisy': noisy, 'edge': noisy[:, 5:8] - 1.}
    fx = {}
    for name, mel in mels.items():
        mel = np.asarray(mel, dtype=np.float32)
        b = np.exp(mel)
        lin = ref_gl.mel_to_linear(b, hp)
        fx[f'nnls_{name}_mel'] = mel
        fx[f'nnls_{name}_relres'] = O.rel_residual(A, lin, b)
        print(name, mel.shape, 'relres median %.3e max %.3e' % (np.median(fx[f'nnls_{name}_relres']), fx[f'nnls_{name}_relres'].max()))
    for i, T in enumerate(GL_T):
        mag = O.harmonic_magnitude(T)[:, :-2]
        seed = 100 + i
        np.random.seed(seed)
        sig1, _ = ref_gl.reconstruct_signal_griffin_lim(mag, hp.hop_length, iterations=1, logger=log)
        np.random.seed(seed)
        sig30, _ = ref_gl.reconstruct_signal_griffin_lim(mag, hp.hop_length, iterations=30, logger=log)
        fx[f'gl_{T}_seed'] = np.int64(seed)
        fx[f'gl_{T}_sig30'] = sig30.astype(np.float32)
        if T < 100:                                   # keeps the file small: the longest case carries sig30 only
            fx[f'gl_{T}_sig1'] = sig1.astype(np.float32)
        if T == 24:
            fx[f'gl_{T}_norm30'] = (sig30 / np.max(abs(sig30))).astype(np.float32)
        print('gl', T, sig30.shape)
    np.random.seed(7)
    wav = ref_gl.griffin_lim_reconstruction_from_mel_spec(mels['cone'][:, :24].astype(np.float32), hp, log)
    fx['pipe_mel'], fx['pipe_seed'], fx['pipe_wav'] = mels['cone'][:, :24].astype(np.float32), np.int64(7), wav.astype(np.float32)
    out = os.path.join(gen_goldens.OUT, 'griffin_lim.npz')
    np.savez_compressed(out, **fx)
    print(out, os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    main()
