"""Restatement of the reference's Griffin-Lim preview path (`griffin_lim.py:63-198`) in NumPy float64.

`griffin_lim` is `reconstruct_signal_griffin_lim` (117-173) with the per-frame Python loops written over a frame matrix
(same operations, same frame order in the overlap-add) and the start signal passed in instead of drawn inside;
`reference_start(seed, n)` reproduces the reference's draw (`np.random.randn(len_samples)` after `np.random.seed(seed)`).
`nnls_lbfgs` is the reference's `nnls` / `mel_to_linear` (33-114: clipped lstsq start, L-BFGS-B per block of at most
256 KB of columns) and needs scipy.  tests/test_griffin_lim_host.py pins this module to tests/golden/griffin_lim.npz,
which tools/gen_golden_griffin_lim.py wrote by running the reference itself.
"""
import numpy as np

from oracle.mel_frontend_cpu import mel_filterbank


def filterbank(hparams):
    return mel_filterbank(hparams.sampling_rate, hparams.filter_length, hparams.n_mel_channels, hparams.mel_fmin,
                          hparams.mel_fmax)


def n_frames(T):
    ''' frames Griffin-Lim runs on for a T-frame mel (`linear_spec[:, :-2]`, griffin_lim.py:194) '''
    return max(T - 2, 0)


def n_samples(T, n_fft, hop):
    ''' len_samples of `reconstruct_signal_griffin_lim` (139) for a T-frame mel '''
    return n_frames(T) * hop + n_fft


def reference_start(seed, n):
    ''' the reference's start signal: np.random.randn(len_samples) (142) drawn right after np.random.seed(seed) '''
    return np.random.RandomState(seed).randn(n)


def griffin_lim(mag, hop, iterations, x0):
    ''' mag (n_fft // 2 + 1, F) magnitudes (the reference's argument, already cropped), x0 (F * hop + n_fft,) start.
        Returns (signal after each iteration: list of float64 arrays, last proposal spectrogram (F, n_fft // 2 + 1)). '''
    mag = np.asarray(mag, dtype=np.float64).T
    n_fft = (mag.shape[1] - 1) * 2
    F = mag.shape[0]
    S = F * hop + n_fft
    window = np.hanning(n_fft)
    x = np.asarray(x0, dtype=np.float64).copy()
    assert x.shape == (S,)
    starts = np.arange(0, S - n_fft, hop)
    assert len(starts) == F
    idx = starts[:, None] + np.arange(n_fft)[None, :]
    out, proposal = [], None
    for _ in range(iterations):
        spec = np.fft.rfft(window * x[idx], axis=1)
        proposal = mag * np.exp(1.0j * np.angle(spec))
        frames = window * np.real(np.fft.irfft(proposal, axis=1))
        x = np.zeros(S)
        for i in range(F):                       # overlap-add in frame order, like the reference's loop
            x[starts[i]: starts[i] + n_fft] += frames[i]
        x = x / (n_fft / hop / 2)
        out.append(x)
    return out, proposal


def normalise(x):
    ''' waveform / max|waveform| (196); the reference gives NaN for an all-zero signal, this returns zeros there '''
    m = np.max(np.abs(x)) if x.size else 0.
    return x / m if m > 0 else np.zeros_like(x)


def rel_residual(A, X, Bm):
    ''' per-frame || A x - b || / || b || in float64 '''
    A, X, Bm = (np.asarray(a, dtype=np.float64) for a in (A, X, Bm))
    return np.linalg.norm(A @ X - Bm, axis=0) / np.maximum(np.linalg.norm(Bm, axis=0), 1e-300)


def nnls_lbfgs(A, Bm):
    ''' the reference's `nnls(A, B)` for 2-D B (griffin_lim.py:63-99) '''
    import scipy.optimize

    def obj(x, shape, A, B):
        x = x.reshape(shape)
        diff = A @ x - B
        return 0.5 * np.sum(diff ** 2), (A.T @ diff).flatten()

    def block(A, B, x_init=None):
        if x_init is None:
            x_init = np.linalg.lstsq(A, B, rcond=None)[0]
            np.clip(x_init, 0, None, out=x_init)
        x, _, _ = scipy.optimize.fmin_l_bfgs_b(obj, x_init, args=(x_init.shape, A, B), bounds=[(0, None)] * x_init.size,
                                               m=A.shape[1])
        return x.reshape(x_init.shape)

    n_columns = max((2 ** 8 * 2 ** 10) // (A.shape[-1] * A.itemsize), 1)
    if Bm.shape[-1] <= n_columns:
        return block(A, Bm).astype(A.dtype)
    x = np.linalg.lstsq(A, Bm, rcond=None)[0].astype(A.dtype)
    np.clip(x, 0, None, out=x)
    x_init = x
    for s in range(0, x.shape[-1], n_columns):
        t = min(s + n_columns, Bm.shape[-1])
        x[:, s:t] = block(A, Bm[:, s:t], x_init=x_init[:, s:t])
    return x


def harmonic_magnitude(T, n_fft=1024, sr=22050, f0=140., n_harm=24, gain=8.):
    ''' closed-form voiced magnitude spectrogram (n_fft // 2 + 1, T): harmonics of a gliding f0 with a 1/h roll-off and a
        slow amplitude envelope, Gaussian main lobes of 2 bins, a small noise floor '''
    k = np.arange(n_fft // 2 + 1)[:, None]
    t = np.arange(T)[None, :]
    f = f0 * (1. + 0.25 * np.sin(2 * np.pi * t / 97.))
    env = 0.6 + 0.4 * np.cos(2 * np.pi * t / 53.)
    mag = np.full((n_fft // 2 + 1, T), 1e-3)
    for h in range(1, n_harm + 1):
        c = h * f * n_fft / sr
        mag += gain * env / h * np.exp(-0.5 * ((k - c) / 2.) ** 2)
    return mag
