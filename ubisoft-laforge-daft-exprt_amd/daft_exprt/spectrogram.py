"""The magnitude spectrogram of a waveform with its gradient back to the waveform (K36, csrc/spectrogram.hip): what BigVGAN's
multi-resolution discriminator (`bigvgan_train.DiscriminatorR`) is built over.  It is upstream's `DiscriminatorR.spectrogram` --
reflect padding of (n_fft - hop) div 2 per side, `torch.stft(center=False, window=None, win_length=win)`, `torch.norm(., p=2, dim=-1)`
-- per utterance, so a ragged batch gives every utterance the frames and the bits it has alone.  No CPU fallback.
"""
import ctypes

import torch

from daft_exprt import _hip as H
from daft_exprt import config as _config

N_FFT_SIZES = (256, 512, 1024, 2048, 4096)


def spectrogram_frames(n, n_fft, hop):
    ''' F = 1 + (n + 2 p - n_fft) div hop, p = (n_fft - hop) div 2: the frames of an utterance of n samples.  Raises ValueError where
        the reflect padding is not defined (n <= p, as torch refuses it) or no frame fits '''
    n, n_fft, hop = int(n), int(n_fft), int(hop)
    if hop < 1 or hop > n_fft:
        raise ValueError(f'spectrogram: hop {hop} outside [1, n_fft = {n_fft}]')
    p = (n_fft - hop) // 2
    if n <= p or n + 2 * p < n_fft:
        raise ValueError(f'spectrogram: {n} samples are too few for n_fft {n_fft}, hop {hop}: reflect padding of {p} per side needs '
                         f'more than {p}, and one frame n + 2 p >= n_fft')
    return 1 + (n + 2 * p - n_fft) // hop


def rectangular_window(n_fft, win=None):
    ''' what torch.stft uses for window=None: ones on [l, l + win), l = (n_fft - win) div 2, zeros elsewhere; (n_fft,) fp32 on the CPU '''
    win = n_fft if win is None else int(win)
    if win < 1 or win > n_fft:
        raise ValueError(f'spectrogram: win {win} outside [1, n_fft = {n_fft}]')
    w = torch.zeros(n_fft, dtype=torch.float32)
    left = (n_fft - win) // 2
    w[left:left + win] = 1.
    return w


def _twiddle(device, n_fft):
    def make():
        t = torch.empty(2 * n_fft, dtype=torch.float32, device=device)
        with torch.cuda.device(device):
            H.check(H.lib().dx_spectrogram_tables(H.ptr(t), n_fft, H.stream()))
        return t
    return H.device_table('spectrogram_twiddle', device, n_fft, make=make)


def _window(device, n_fft, win):
    return H.device_table('spectrogram_window', device, n_fft, win, make=lambda: rectangular_window(n_fft, win).to(device))


_WS = {}       # device -> the backward's workspace (grown on demand, reused)


def _workspace(n_bytes, device):
    ws = _WS.get(device)
    if ws is None or ws.numel() * 4 < n_bytes:
        _WS[device] = None
        ws = _WS[device] = torch.empty((n_bytes + 3) // 4, dtype=torch.float32, device=device)
    if _config.POISON:
        ws.fill_(float('nan'))
    return ws


def _host_counts(n_samples, B):
    ''' the B sample counts as a ctypes int64 array for the launcher's checks; a device tensor is read back (one synchronisation) '''
    values = [int(v) for v in (n_samples.tolist() if torch.is_tensor(n_samples) else n_samples)]
    if len(values) != B:
        raise ValueError(f'spectrogram: n_samples has {len(values)} entries for a batch of {B}')
    return (ctypes.c_int64 * B)(*values), values


class _Spectrogram(torch.autograd.Function):
    @staticmethod
    def forward(ctx, wav, n_dev, n_host, twiddle, window, T, n_fft, hop):
        wav = wav.contiguous()
        B, S = wav.shape
        mag = torch.empty((B, n_fft // 2 + 1, T), dtype=torch.float32, device=wav.device)
        with torch.cuda.device(wav.device):
            H.check(H.lib().dx_spectrogram(H.ptr(wav), S, H.ptr(n_dev), ctypes.addressof(n_host), H.ptr(twiddle), H.ptr(window), H.ptr(mag),
                                           B, S, T, n_fft, hop, H.stream()))
        ctx.save_for_backward(wav, n_dev, twiddle, window)
        ctx.meta = (n_host, T, n_fft, hop)
        return mag

    @staticmethod
    def backward(ctx, dmag):
        wav, n_dev, twiddle, window = ctx.saved_tensors
        n_host, T, n_fft, hop = ctx.meta
        B, S = wav.shape
        dmag = dmag.contiguous().float()
        dwav = torch.empty_like(wav)
        with torch.cuda.device(wav.device):
            ws = _workspace(int(H.lib().dx_spectrogram_bwd_workspace(B, T, n_fft)), wav.device)
            H.check(H.lib().dx_spectrogram_bwd(H.ptr(wav), S, H.ptr(n_dev), ctypes.addressof(n_host), H.ptr(twiddle), H.ptr(window),
                                               H.ptr(dmag), H.ptr(dwav), S, H.ptr(ws), B, S, T, n_fft, hop, H.stream()))
        return dwav, None, None, None, None, None, None, None


def spectrogram(wav, n_samples, n_fft, hop, win=None, window=None):
    ''' wav (B, S) fp32 on the device; n_samples (B): an int64 tensor (a device tensor is read back once for the launcher's checks) or a
        host sequence of ints (no synchronisation); window: None for torch.stft's window=None at win_length `win` (ones over the
        centred `win` samples), or an (n_fft,) table -> (mag (B, n_fft / 2 + 1, T) fp32, frames (B,) int64 on the device) with
        T = max frames; samples at or past n_samples[b] are not read, frames at or past frames[b] are zeros.  Differentiable in wav. '''
    H.require_gpu(wav)
    if wav.dim() != 2 or wav.dtype != torch.float32:
        raise ValueError(f'spectrogram: expected an fp32 (B, S) waveform, got {wav.dtype} {tuple(wav.shape)}')
    n_fft, hop = int(n_fft), int(hop)
    if n_fft not in N_FFT_SIZES:
        raise ValueError(f'spectrogram: n_fft {n_fft} is not one of {N_FFT_SIZES}')
    B, S = wav.shape
    n_host, values = _host_counts(n_samples, B)
    frames = []
    for b, n in enumerate(values):
        if n > S:
            raise ValueError(f'spectrogram: utterance {b} has {n} samples, the waveform rows hold {S}')
        try:
            frames.append(spectrogram_frames(n, n_fft, hop))
        except ValueError as e:
            raise ValueError(f'{e} (utterance {b})') from None
    if torch.is_tensor(n_samples) and n_samples.device == wav.device and n_samples.dtype == torch.int64:
        n_dev = n_samples.contiguous()
    else:
        n_dev = torch.tensor(values, dtype=torch.int64, device=wav.device)
    if window is None:
        table = _window(wav.device, n_fft, n_fft if win is None else int(win))
    else:
        if window.shape != (n_fft,):
            raise ValueError(f'spectrogram: window has shape {tuple(window.shape)}, expected ({n_fft},)')
        table = window.to(device=wav.device, dtype=torch.float32).contiguous()
    mag = _Spectrogram.apply(wav, n_dev, n_host, _twiddle(wav.device, n_fft), table, max(frames), n_fft, hop)
    return mag, torch.tensor(frames, dtype=torch.int64, device=wav.device)
