"""Griffin-Lim preview audio of the synthesis path on the GPU (reference: `griffin_lim.py:63-198`; callers
`generate.py:110-137, 311-314`).

`mel_to_linear`, `reconstruct_signal_griffin_lim` and `griffin_lim_reconstruction_from_mel_spec` keep the reference's
signatures (NumPy in, NumPy out, one utterance); `griffin_lim_batch` is the batched device entry the synthesis driver
uses.  No CPU fallback: without the HIP library / a GPU these functions raise.

Where this differs from the reference, by design:
  * mel -> linear: the reference stops scipy's L-BFGS-B early, so its x is one of many (80 x 513 is underdetermined).
    Here the same start (clipped lstsq = clip(pinv(A) b, 0)) is followed by `NNLS_ITERS` FISTA steps; the contract is the
    objective: per frame, || A x - b || is at least as small as the reference's (tests/test_gpu_griffin_lim.py).
  * start signal: the reference draws unseeded `np.random.randn`; the device draws standard normal noise from a
    counter-based hash of (seed, utterance, sample) -- reproducible, but not the reference's stream.  Pass `x0` to start
    from a given signal.
  * an utterance of at most 2 frames, or an all-zero signal, normalises to zeros (the reference computes 0 / 0 = NaN).
"""
from types import SimpleNamespace

import numpy as np
import torch

from daft_exprt import _hip as H
from daft_exprt.audio import fft_tables, write_wav  # noqa: F401  (write_wav: the preview audio's writer, kept importable here)
from daft_exprt.extract_features import mel_tables

NNLS_ITERS = 500        # FISTA steps after the clipped-pinv start: on tests/golden/griffin_lim.npz the per-frame residual
                        # is within the reference's on every frame from ~400 on in fp32 (200: 4 % of the decoder frames)
GL_ITERS = 30           # griffin_lim.py:194


def _nnls_tables(hparams, device):
    ''' (pinv(A)^T, bin_m, bin_w, step) of the mel -> linear solve for these hparams on `device`; A = the mel filterbank '''
    def make():
        A = mel_tables(hparams, device)[0].cpu().numpy().astype(np.float64)
        pinv_t = np.ascontiguousarray(np.linalg.pinv(A).T).astype(np.float32)       # (n_mel, n_fft/2 + 1)
        step = 1.0 / np.linalg.norm(A, 2) ** 2
        nb = A.shape[1]
        bin_m = np.full((nb, 2), -1, dtype=np.int32)
        bin_w = np.zeros((nb, 2), dtype=np.float32)
        for k in range(nb):
            ms = np.nonzero(A[:, k] > 0)[0]
            if len(ms) > 2:
                raise ValueError(f'mel_to_linear: bin {k} lies in {len(ms)} filters (at most 2 supported)')
            bin_m[k, :len(ms)] = ms
            bin_w[k, :len(ms)] = A[ms, k]
        to = lambda a: torch.from_numpy(a).to(device)  # noqa: E731
        return to(pinv_t), to(bin_m), to(bin_w), float(step)
    return H.device_table('nnls', device, hparams.sampling_rate, hparams.filter_length, hparams.n_mel_channels, hparams.mel_fmin,
                          hparams.mel_fmax, make=make)


def n_samples(T, hparams):
    ''' samples of the waveform made from a T-frame mel: the reference crops 2 frames ([:, :-2], griffin_lim.py:194) and
        allocates frames * hop + n_fft samples (139) '''
    return max(int(T) - 2, 0) * int(hparams.hop_length) + int(hparams.filter_length)


def mel_to_linear_batch(mel, lengths, hparams, nnls_iters=None, input_is_log=True):
    ''' mel (B, n_mel, T) fp32 device tensor (log-mel with `input_is_log`, else linear), lengths (B,) int64 device tensor.
        Returns the linear magnitude (B, n_fft/2 + 1, T) fp32 (a frame-major view: frames are contiguous); frames at or
        past lengths[b] are 0. '''
    H.require_gpu(mel, lengths)
    assert mel.dtype == torch.float32 and lengths.dtype == torch.int64
    mel = mel.contiguous()
    B, n_mel, T = mel.shape
    n_fft = int(hparams.filter_length)
    nb = n_fft // 2 + 1
    fb, lo, hi = mel_tables(hparams, mel.device)
    pinv_t, bin_m, bin_w, step = _nnls_tables(hparams, mel.device)
    lin = torch.empty((B, T, nb), dtype=torch.float32, device=mel.device)
    iters = NNLS_ITERS if nnls_iters is None else int(nnls_iters)
    H.check(H.lib().dx_mel_to_linear(H.ptr(mel), H.ptr(lengths), H.ptr(fb), H.ptr(lo), H.ptr(hi), H.ptr(pinv_t), H.ptr(bin_m),
                                     H.ptr(bin_w), H.ptr(lin), T * nb, 1, nb, B, T, n_mel, n_fft, iters, step,
                                     int(bool(input_is_log)), H.stream()))
    return lin.transpose(1, 2)


def griffin_lim_from_linear(linear, lengths, hparams, iterations=GL_ITERS, seed=0, x0=None, normalise=True):
    ''' linear (B, n_fft/2 + 1, T) fp32 device magnitudes (any strides), lengths (B,) int64: utterance b uses frames
        0 .. lengths[b] - 3.  Returns (wav (B, S) fp32, n_samples (B,) int64), S = max(T - 2, 0) * hop + n_fft, zeros past
        n_samples[b] = max(lengths[b] - 2, 0) * hop + n_fft.  x0 (B, >= S) fp32: start signal; None: device noise from
        `seed` (standard normal, counter-based hash -- not the reference's unseeded np.random.randn stream). '''
    H.require_gpu(linear, lengths, x0)
    assert linear.dtype == torch.float32 and lengths.dtype == torch.int64
    B, nb, T = linear.shape
    n_fft, hop = int(hparams.filter_length), int(hparams.hop_length)
    assert nb == n_fft // 2 + 1, (nb, n_fft)
    dev = linear.device
    twiddle, window = fft_tables(n_fft, True, dev)
    S = n_samples(T, hparams)
    if x0 is not None:
        assert x0.dtype == torch.float32 and x0.dim() == 2 and x0.shape[0] == B and x0.shape[1] >= S and x0.stride(1) == 1
    wav = torch.empty((B, S), dtype=torch.float32, device=dev)
    n_out = torch.empty((B,), dtype=torch.int64, device=dev)
    n_ws = int(H.lib().dx_gl_ws_floats(B, T, n_fft))
    ws = torch.empty((max(n_ws, 1),), dtype=torch.float32, device=dev)
    H.check(H.lib().dx_griffin_lim(H.ptr(linear), linear.stride(0), linear.stride(1), linear.stride(2), H.ptr(lengths),
                                   H.ptr(x0), 0 if x0 is None else x0.stride(0), H.ptr(twiddle), H.ptr(window), H.ptr(wav), S,
                                   H.ptr(n_out), H.ptr(ws), B, T, n_fft, hop, int(iterations), int(seed) & (2 ** 64 - 1),
                                   H.stream()))
    if normalise:
        H.check(H.lib().dx_gl_normalise(H.ptr(wav), S, H.ptr(lengths), B, T, n_fft, hop, H.stream()))
    return wav, n_out


def griffin_lim_batch(mel, lengths, hparams, iterations=GL_ITERS, seed=0, x0=None, nnls_iters=None, normalise=True):
    ''' `griffin_lim_reconstruction_from_mel_spec` (griffin_lim.py:176-198) for a batch: log-mel (B, n_mel, T) fp32 device
        tensor, lengths (B,) int64 device tensor -> (wav (B, S) fp32, n_samples (B,) int64), both on the device, zeros past
        n_samples[b].  S follows from T alone (no host sync).  See `griffin_lim_from_linear` for `seed` / `x0`. '''
    lin = mel_to_linear_batch(mel, lengths, hparams, nnls_iters=nnls_iters, input_is_log=True)
    return griffin_lim_from_linear(lin, lengths, hparams, iterations=iterations, seed=seed, x0=x0, normalise=normalise)


# ---- reference signatures (NumPy in / out, one utterance) -------------------------------------------------------------

def mel_to_linear(mel_spectrogram, hparams, device=None):
    ''' `griffin_lim.py:102-114`: LINEAR mel (n_mels, T) -> linear magnitude (n_fft // 2 + 1, T) float32 '''
    dev = H.device(device)
    mel = torch.as_tensor(np.asarray(mel_spectrogram, dtype=np.float32))
    n_mel, T = mel.shape
    lengths = torch.tensor([T], dtype=torch.int64, device=dev)
    lin = mel_to_linear_batch(mel.reshape(1, n_mel, T).to(dev), lengths, hparams, input_is_log=False)
    return lin[0].cpu().numpy()


def reconstruct_signal_griffin_lim(magnitude_spectrogram, step_size, iterations, logger, seed=0, x0=None, device=None):
    ''' `griffin_lim.py:117-173`: magnitude (n_fft // 2 + 1, F) -> (signal (F * step_size + n_fft,) float64, proposal
        spectrogram (F, n_fft // 2 + 1) complex128).  The start is `x0` if given, else device noise from `seed` (the
        reference draws unseeded np.random.randn).  The proposal -- dropped by every caller of the reference -- is formed
        on the host from the signal before the last iteration. '''
    dev = H.device(device)
    mag = np.asarray(magnitude_spectrogram, dtype=np.float32)
    nb, F = mag.shape
    n_fft, hop = (nb - 1) * 2, int(step_size)
    hp = SimpleNamespace(filter_length=n_fft, hop_length=hop)
    S = F * hop + n_fft
    lin = torch.zeros((1, nb, F + 2), dtype=torch.float32, device=dev)  # the kernels crop 2 frames, as the reference's caller
    lin[0, :, :F] = torch.as_tensor(mag).to(dev)
    lengths = torch.tensor([F + 2], dtype=torch.int64, device=dev)
    if x0 is None:
        prev = device_noise(lengths, hp, F + 2, seed)
    else:
        prev = torch.as_tensor(np.asarray(x0, dtype=np.float32)).reshape(1, S).to(dev)
    if iterations > 1:
        prev, _ = griffin_lim_from_linear(lin, lengths, hp, iterations=iterations - 1, x0=prev, normalise=False)
    sig, _ = griffin_lim_from_linear(lin, lengths, hp, iterations=1, x0=prev, normalise=False)
    xp = prev[0].double().cpu().numpy()
    idx = (np.arange(F) * hop)[:, None] + np.arange(n_fft)[None, :]
    proposal = mag.T.astype(np.float64) * np.exp(1.0j * np.angle(np.fft.rfft(np.hanning(n_fft) * xp[idx], axis=1)))
    if logger is not None:
        logger.debug(f'Griffin-Lim: {iterations} iterations on the device')
    return sig[0].double().cpu().numpy(), proposal


def griffin_lim_reconstruction_from_mel_spec(mel_spec, hparams, logger, seed=0, device=None):
    ''' `griffin_lim.py:176-198`: log-mel (n_mels, T) -> normalised waveform (max(T - 2, 0) * hop + n_fft,) float64
        (zeros for T <= 2, where the reference divides 0 by 0) '''
    dev = H.device(device)
    mel = torch.as_tensor(np.asarray(mel_spec, dtype=np.float32))
    n_mel, T = mel.shape
    lengths = torch.tensor([T], dtype=torch.int64, device=dev)
    wav, _ = griffin_lim_batch(mel.reshape(1, n_mel, T).to(dev), lengths, hparams, seed=seed)
    if logger is not None:
        logger.debug(f'Griffin-Lim: {T} mel frames -> {wav.shape[1]} samples on the device')
    return wav[0].double().cpu().numpy()


def device_noise(lengths, hparams, T, seed=0):
    ''' (B, S) fp32 standard normal start signals as griffin_lim_from_linear draws them from `seed` (zeros past
        n_samples[b]) '''
    H.require_gpu(lengths)
    n_fft, hop = int(hparams.filter_length), int(hparams.hop_length)
    B, S = lengths.shape[0], n_samples(T, hparams)
    x = torch.empty((B, S), dtype=torch.float32, device=lengths.device)
    H.check(H.lib().dx_gl_noise(H.ptr(x), S, H.ptr(lengths), B, int(T), n_fft, hop, int(seed) & (2 ** 64 - 1), H.stream()))
    return x
