"""Mel-spectrogram / frame-energy front-end of the synthesis path on the GPU (reference: `extract_features.py:299-304,
330-359`; callers `generate.py:455-457`, `extract_features.py:429, 465-466`, `fine_tune.py:102`).

`mel_spectrogram_HiFi(wav, hparams)` and `extract_energy(mel_spec)` keep the reference's signatures (NumPy in, NumPy
out, one utterance); `mel_spectrogram_batch` is the batched device entry.  `extract_pitch(wav, fs, hparams)` keeps the
signature of `extract_features.py:222-269` and `pitch_batch` is its batched device entry, but the tracker behind them is this
project's own (csrc/pitch.hip), not the REAPER binary the reference runs.  The mel filterbank is built here from the
published Slaney formula (what `librosa.filters.mel(sr, n_fft, n_mels, fmin, fmax)` computes with its defaults
htk=False, norm='slaney'); librosa itself is not a dependency.  No CPU fallback: without the HIP library / a GPU these
functions raise.
"""
import math

import numpy as np
import torch

from daft_exprt import _hip as H
from daft_exprt.audio import fft_tables
from daft_exprt.audio import rescale_wav_to_float32  # noqa: F401  (the reference keeps it here, `extract_features.py:362`)


PITCH_WINDOW_S = 0.015     # correlation window of the pitch tracker


def _hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, 1e-30) / min_log_hz) / logstep, f / f_sp)


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def mel_filter_bank(sr, n_fft, n_mels, fmin, fmax):
    ''' (n_mels, 1 + n_fft // 2) float32: triangular filters on the Slaney mel scale, each normalised to unit area '''
    fmax = float(sr) / 2 if fmax is None else float(fmax)
    freqs = np.linspace(0., float(sr) / 2, 1 + n_fft // 2)
    edges = _mel_to_hz(np.linspace(_hz_to_mel(fmin), _hz_to_mel(fmax), n_mels + 2))
    width = np.diff(edges)
    ramps = edges[:, None] - freqs[None, :]
    fb = np.maximum(0., np.minimum(-ramps[:-2] / width[:-1, None], ramps[2:] / width[1:, None]))
    fb *= (2.0 / (edges[2:] - edges[:-2]))[:, None]
    return fb.astype(np.float32)


def mel_tables(hparams, device):
    ''' (filterbank (n_mel, n_fft/2 + 1) fp32, lo, hi (n_mel,) int32: filter m is non-zero on bins lo[m] .. hi[m] - 1) on `device` '''
    def make():
        fb = mel_filter_bank(hparams.sampling_rate, int(hparams.filter_length), hparams.n_mel_channels, hparams.mel_fmin, hparams.mel_fmax)
        nz = fb > 0
        lo = np.where(nz.any(1), nz.argmax(1), 0).astype(np.int32)
        hi = np.where(nz.any(1), fb.shape[1] - nz[:, ::-1].argmax(1), 0).astype(np.int32)
        return torch.from_numpy(fb).to(device), torch.from_numpy(lo).to(device), torch.from_numpy(hi).to(device)
    return H.device_table('mel', device, hparams.sampling_rate, hparams.filter_length, hparams.n_mel_channels, hparams.mel_fmin,
                          hparams.mel_fmax, make=make)


def nb_frames(n_samples, hparams):
    ''' frames torch.stft produces for a waveform of n_samples (`extract_features.py:347-348`) '''
    n_fft, hop = int(hparams.filter_length), int(hparams.hop_length)
    if hparams.centered:
        return 1 + n_samples // hop
    return 1 + (n_samples - n_fft) // hop if n_samples >= n_fft else 0


def mel_spectrogram_batch(wavs, n_samples, hparams):
    ''' wavs (B, S) float32 device tensor (right-padded), n_samples (B,) int64 device tensor.
        Returns (log-mel (B, n_mel, T) fp32, frame energies (B, T) fp32, n_frames (B,) int64); frames >= n_frames[b] are 0. '''
    H.require_gpu(wavs, n_samples)
    assert wavs.dtype == torch.float32 and wavs.stride(1) == 1 and n_samples.dtype == torch.int64
    B, S = wavs.shape
    dev = wavs.device
    n_fft, hop, n_mel = int(hparams.filter_length), int(hparams.hop_length), int(hparams.n_mel_channels)
    if hparams.centered and int(n_samples.min()) <= n_fft // 2:
        raise ValueError('mel_spectrogram: reflect padding needs more than filter_length / 2 samples')
    T = max(1, nb_frames(S, hparams))
    basis, window = fft_tables(n_fft, False, dev)
    fb, lo, hi = mel_tables(hparams, dev)
    mel = torch.empty((B, n_mel, T), dtype=torch.float32, device=dev)
    energy = torch.empty((B, T), dtype=torch.float32, device=dev)
    n_frames = torch.empty((B,), dtype=torch.int64, device=dev)
    H.check(H.lib().dx_mel_spectrogram(H.ptr(wavs), wavs.stride(0), H.ptr(n_samples), H.ptr(basis), H.ptr(window), H.ptr(fb),
                                       H.ptr(lo), H.ptr(hi), H.ptr(mel), H.ptr(energy), H.ptr(n_frames), B, T, n_fft,
                                       hop, n_mel, int(bool(hparams.centered)), float(hparams.min_clipping), H.stream()))
    return mel, energy, n_frames


def mel_spectrogram_HiFi(wav, hparams, device='cuda:0'):
    ''' reference signature (`extract_features.py:330`): wav (T,) in [-1, 1] -> log-mel (n_mel_channels, n_frames) NumPy '''
    w = torch.as_tensor(np.asarray(wav, dtype=np.float32)).reshape(1, -1).to(device)
    n = torch.tensor([w.shape[1]], dtype=torch.int64, device=device)
    mel, _, nfr = mel_spectrogram_batch(w, n, hparams)
    return mel[0, :, :int(nfr[0])].cpu().numpy()


def pitch_geometry(hparams, sr=None):
    ''' (sr, step = samples per analysis frame, window, lag_min, lag_max) of the pitch tracker at rate `sr` (default
        hparams.sampling_rate): a 15 ms window and the lags floor(sr / max_f0) .. ceil(sr / min_f0) '''
    sr = int(hparams.sampling_rate if sr is None else sr)
    lag_min, lag_max = int(math.floor(sr / float(hparams.max_f0))), int(math.ceil(sr / float(hparams.min_f0)))
    if not 2 <= lag_min < lag_max:
        raise ValueError(f'pitch: min_f0={hparams.min_f0}, max_f0={hparams.max_f0} give no lag range at {sr} Hz')
    return sr, float(sr) * float(hparams.f0_interval), int(round(PITCH_WINDOW_S * sr)), lag_min, lag_max


def pitch_candidates_batch(wavs, n_samples, hparams, sr=None):
    ''' `dx_pitch_candidates`: (lags, values), each (B, A, K) fp32 on the device, A = 1 + floor(S / step): per analysis frame the
        up to K best maxima of the normalised cross-correlation, in order of value; empty slots are 0 '''
    H.require_gpu(wavs, n_samples)
    assert wavs.dtype == torch.float32 and wavs.dim() == 2 and wavs.stride(1) == 1 and n_samples.dtype == torch.int64
    sr, step, window, lag_min, lag_max = pitch_geometry(hparams, sr)
    B, S = wavs.shape
    A = 1 + int(math.floor(S / step))
    K = int(H.lib().dx_pitch_num_candidates())
    dev = wavs.device
    lags = torch.empty((B, A, K), dtype=torch.float32, device=dev)
    vals = torch.empty((B, A, K), dtype=torch.float32, device=dev)
    mean_sq = torch.empty((B,), dtype=torch.float64, device=dev)
    H.check(H.lib().dx_pitch_candidates(H.ptr(wavs), wavs.stride(0), H.ptr(n_samples), H.ptr(mean_sq), H.ptr(lags), H.ptr(vals),
                                        B, S, A, step, window, lag_min, lag_max, H.stream()))
    return lags, vals


def pitch_track_batch(wavs, n_samples, hparams, sr=None):
    ''' both kernels: (log_pitch (B, T) fp32, n_frames (B,) int64, hz (B, A) fp32 per analysis frame, (lags, values)) '''
    lags, vals = pitch_candidates_batch(wavs, n_samples, hparams, sr)
    sr, step, _, _, lag_max = pitch_geometry(hparams, sr)
    B, S = wavs.shape
    _, A, K = lags.shape
    hop = int(hparams.hop_length)
    T = 1 + S // hop
    dev = wavs.device
    back = torch.empty((B, A, K + 1), dtype=torch.uint8, device=dev)
    hz = torch.empty((B, A), dtype=torch.float32, device=dev)
    log_pitch = torch.empty((B, T), dtype=torch.float32, device=dev)
    n_frames = torch.empty((B,), dtype=torch.int64, device=dev)
    H.check(H.lib().dx_pitch_viterbi(H.ptr(lags), H.ptr(vals), H.ptr(n_samples), H.ptr(back), H.ptr(hz), H.ptr(log_pitch),
                                     H.ptr(n_frames), B, S, A, T, sr, step, hop, lag_max, float(hparams.uv_cost), H.stream()))
    return log_pitch, n_frames, hz, (lags, vals)


def pitch_batch(wavs, n_samples, hparams, sr=None):
    ''' wavs (B, S) float32 device tensor (right-padded), n_samples (B,) int64 device tensor, sampled at `sr` (default
        hparams.sampling_rate).  Returns (log_pitch (B, T) fp32 on the device, n_frames (B,) int64): per mel frame
        (T = 1 + S // hop_length, n_frames[b] = 1 + n_samples[b] // hop_length, as `mel_spectrogram_batch` with `centered`)
        log(Hz), 0 where unvoiced and for frames >= n_frames[b].
        hparams.f0_interval, min_f0, max_f0 and uv_cost mean what they mean to the reference's binary (analysis interval, search
        range, weight of the unvoiced hypothesis).  hparams.uv_interval is accepted and ignored: it spaces REAPER's pitch marks
        in unvoiced regions and has no meaning without pitch marks.  The Hz is not rounded to an integer, as the reference
        binary's output format does. '''
    log_pitch, n_frames, _, _ = pitch_track_batch(wavs, n_samples, hparams, sr)
    return log_pitch, n_frames


def extract_pitch(wav, fs, hparams, device='cuda:0'):
    ''' reference signature (`extract_features.py:222`): wav (n,) in [-1, 1] sampled at fs -> (1 + n // hop_length,) NumPy,
        log(Hz) per mel frame, 0 where unvoiced '''
    w = torch.as_tensor(np.asarray(wav, dtype=np.float32)).reshape(1, -1).to(device)
    n = torch.tensor([w.shape[1]], dtype=torch.int64, device=device)
    log_pitch, nfr = pitch_batch(w, n, hparams, sr=fs)
    return log_pitch[0, :int(nfr[0])].cpu().numpy()


def extract_energy(mel_spec):
    ''' `extract_features.py:299-304`: L2 norm over the mel channels (callers pass np.exp(log-mel)); tiny, host side '''
    return np.linalg.norm(mel_spec, axis=0)
