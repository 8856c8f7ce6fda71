"""The multi-scale mel loss of BigVGAN-v2's fine-tuning over K37 (csrc/mel_loss.hip): per scale the log10-mel of the recording
(`log_mel`), and the L1 between it and the log10-mel of the synthesis with its gradient back to the waveform left behind by the same
call (`log_mel_l1`), so the synthesis is analysed once per scale and autograd saves nothing.  `MultiScaleMelLoss` sums the scales.
No CPU fallback: the `log_mel=` hook of the module exists for the host tests, which pass the float64 oracle.

The scales (window lengths 32 ... 2048 with 5 ... 320 bands, hop = length / 4, centred reflect padding, periodic Hann, log10 of the
mel clamped at 1e-5, weight 15) are restated from the BigVGAN-v2 and DAC papers as recalled; no upstream source was at hand:
UNVERIFIED.
"""
import ctypes

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from daft_exprt import _hip as H
from daft_exprt import config as _config

N_FFT_SIZES = (32, 64, 128, 256, 512, 1024, 2048)
WINDOW_LENGTHS = (32, 64, 128, 256, 512, 1024, 2048)
N_MELS = (5, 10, 20, 40, 80, 160, 320)
EPS = 1e-5
WEIGHT = 15.


def mel_frames(n, n_fft, hop, pad):
    ''' F = 1 + (n + 2 p - n_fft) div hop: the frames of an utterance of n samples under a reflect padding of p per side.  Raises
        ValueError where the padding is not defined (n <= p, as torch refuses it) or no frame fits '''
    n, n_fft, hop, pad = int(n), int(n_fft), int(hop), int(pad)
    if hop < 1 or hop > n_fft:
        raise ValueError(f'mel loss: hop {hop} outside [1, n_fft = {n_fft}]')
    if n <= pad or n + 2 * pad < n_fft:
        raise ValueError(f'mel loss: {n} samples are too few for n_fft {n_fft}, hop {hop}: reflect padding of {pad} per side needs '
                         f'more than {pad}, and one frame n + 2 p >= n_fft')
    return 1 + (n + 2 * pad - n_fft) // hop


def band_tables(fb):
    ''' fb (M, bins), non-negative, every row's support contiguous -> (fb_lo, fb_hi (M,), bin_lo, bin_hi (bins,)) int32: filter m is
        non-zero exactly on the bins [fb_lo[m], fb_hi[m]) and bin k is touched by no filter outside [bin_lo[k], bin_hi[k]) (the
        transpose; a bin's filters need not be contiguous, the run is their hull).  An empty row or column has lo = hi = 0.  Raises
        ValueError naming the first row that is negative somewhere or whose support has a gap '''
    fb = np.asarray(fb)
    if fb.ndim != 2 or fb.shape[0] < 1:
        raise ValueError(f'mel loss: the filter bank has shape {fb.shape}, expected (M >= 1, bins)')
    if not np.isfinite(fb).all() or (fb < 0).any():
        bad = int(np.argmax((~np.isfinite(fb) | (fb < 0)).any(1)))
        raise ValueError(f'mel loss: filter {bad} of the filter bank has a negative or non-finite entry')
    nz = fb > 0

    def hull(mask):
        some = mask.any(1)
        lo = np.where(some, mask.argmax(1), 0).astype(np.int32)
        hi = np.where(some, mask.shape[1] - mask[:, ::-1].argmax(1), 0).astype(np.int32)
        return lo, hi
    fb_lo, fb_hi = hull(nz)
    gaps = nz.sum(1) != fb_hi - fb_lo
    if gaps.any():
        m = int(np.argmax(gaps))
        raise ValueError(f'mel loss: filter {m} of the filter bank is zero inside its support [{fb_lo[m]}, {fb_hi[m]}): rows must have '
                         f'contiguous support')
    bin_lo, bin_hi = hull(nz.T)
    return fb_lo, fb_hi, bin_lo, bin_hi


class MelScale:
    ''' one scale: n_fft, hop, the reflect padding per side, a window table (n_fft,) and a filter bank (M, n_fft / 2 + 1), both fp32 on
        the host, and eps.  Its device tables (twiddles, window, filter bank, band tables) are built once per device and kept here '''
    def __init__(self, n_fft, hop, pad, window, fb, eps=EPS):
        self.n_fft, self.hop, self.pad, self.eps = int(n_fft), int(hop), int(pad), float(eps)
        if self.n_fft not in N_FFT_SIZES:
            raise ValueError(f'mel loss: n_fft {self.n_fft} is not one of {N_FFT_SIZES}')
        if self.hop < 1 or self.hop > self.n_fft:
            raise ValueError(f'mel loss: hop {self.hop} outside [1, n_fft = {self.n_fft}]')
        if self.pad < 0:
            raise ValueError(f'mel loss: the padding {self.pad} is negative')
        if not self.eps > 0.:
            raise ValueError(f'mel loss: eps {self.eps} is not positive')
        self.window = torch.as_tensor(window, dtype=torch.float32).contiguous()
        self.fb = torch.as_tensor(np.asarray(fb), dtype=torch.float32).contiguous()
        if self.window.shape != (self.n_fft,):
            raise ValueError(f'mel loss: window has shape {tuple(self.window.shape)}, expected ({self.n_fft},)')
        if self.fb.dim() != 2 or self.fb.shape[1] != self.n_fft // 2 + 1:
            raise ValueError(f'mel loss: the filter bank has shape {tuple(self.fb.shape)}, expected (M, {self.n_fft // 2 + 1})')
        self.n_mels = int(self.fb.shape[0])
        self.bands = band_tables(self.fb.numpy())
        self._device = {}

    def __repr__(self):
        return f'MelScale(n_fft {self.n_fft}, hop {self.hop}, pad {self.pad}, {self.n_mels} bands)'

    def frames(self, n):
        return mel_frames(n, self.n_fft, self.hop, self.pad)

    def tables(self, device):
        ''' (twiddle, window, fb, fb_lo, fb_hi, bin_lo, bin_hi) on `device` '''
        key = str(device)
        if key not in self._device:
            twiddle = torch.empty(2 * self.n_fft, dtype=torch.float32, device=device)
            with torch.cuda.device(device):
                H.check(H.lib().dx_mel_loss_tables(H.ptr(twiddle), self.n_fft, H.stream()))
            self._device[key] = (twiddle, self.window.to(device), self.fb.to(device)) + \
                tuple(torch.from_numpy(t).to(device) for t in self.bands)
        return self._device[key]


def bigvgan_v2_scale(window_length, n_mels, sampling_rate):
    ''' the scale of one window length: n_fft = win = the length, hop = a quarter of it, torch.stft's centred reflect padding, the
        periodic Hann window and the Slaney filter bank from 0 Hz to Nyquist '''
    from daft_exprt.extract_features import mel_filter_bank
    n = int(window_length)
    if n not in N_FFT_SIZES:
        raise ValueError(f'mel loss: the window length {n} is not one of {N_FFT_SIZES}')
    if int(n_mels) < 1:
        raise ValueError(f'mel loss: {n_mels} mel bands for the window length {n}')
    window = torch.hann_window(n, periodic=True, dtype=torch.float64).float()
    return MelScale(n, n // 4, n // 2, window, mel_filter_bank(int(sampling_rate), n, int(n_mels), 0, None), EPS)


_WS = {}       # device -> the loss call's workspace (grown on demand, reused)
_COUNTS = {}   # (device, the B sample counts) -> (device int64 tensor, ctypes int64 array): whole segments repeat every step


def _workspace(n_bytes, device):
    ws = _WS.get(device)
    if ws is None or ws.numel() * 4 < n_bytes:
        _WS[device] = None
        ws = _WS[device] = torch.empty((n_bytes + 3) // 4, dtype=torch.float32, device=device)
    if _config.POISON:
        ws.fill_(float('nan'))
    return ws


def _counts(n_samples, B, device):
    ''' (n on the device, n as a ctypes int64 array, n as a list); a device tensor is read back (one synchronisation), a host
        sequence is uploaded once per distinct value '''
    values = [int(v) for v in (n_samples.tolist() if torch.is_tensor(n_samples) else n_samples)]
    if len(values) != B:
        raise ValueError(f'mel loss: n_samples has {len(values)} entries for a batch of {B}')
    if torch.is_tensor(n_samples) and n_samples.device == device and n_samples.dtype == torch.int64:
        return n_samples.contiguous(), (ctypes.c_int64 * B)(*values), values
    key = (str(device), tuple(values))
    if key not in _COUNTS:
        if len(_COUNTS) >= 64:
            _COUNTS.clear()
        _COUNTS[key] = (torch.tensor(values, dtype=torch.int64, device=device), (ctypes.c_int64 * B)(*values))
    return _COUNTS[key] + (values,)


def _check_wav(wav, what):
    H.require_gpu(wav)
    if wav.dim() != 2 or wav.dtype != torch.float32:
        raise ValueError(f'{what}: expected an fp32 (B, S) waveform, got {wav.dtype} {tuple(wav.shape)}')
    return wav if wav.stride(1) == 1 and wav.stride(0) >= wav.shape[1] else wav.contiguous()


def _frames(values, S, scale):
    frames = []
    for b, n in enumerate(values):
        if n > S:
            raise ValueError(f'mel loss: utterance {b} has {n} samples, the waveform rows hold {S}')
        try:
            frames.append(scale.frames(n))
        except ValueError as e:
            raise ValueError(f'{e} (utterance {b})') from None
    return frames


def log_mel(wav, n_samples, scale):
    ''' wav (B, S) fp32 on the device, n_samples (B): an int64 device tensor or a host sequence, scale: a `MelScale`
        -> L (B, T, M) fp32, T = max frames, zeros in the frames past each utterance's.  No gradient. '''
    wav = _check_wav(wav.detach(), 'log_mel')
    B, S = wav.shape
    n_dev, n_host, values = _counts(n_samples, B, wav.device)
    T = max(_frames(values, S, scale))
    twiddle, window, fb, fb_lo, fb_hi, _, _ = scale.tables(wav.device)
    out = torch.empty((B, T, scale.n_mels), dtype=torch.float32, device=wav.device)
    with torch.cuda.device(wav.device):
        H.check(H.lib().dx_mel_loss_log_mel(H.ptr(wav), wav.stride(0), H.ptr(n_dev), ctypes.addressof(n_host), H.ptr(twiddle), H.ptr(window),
                                            H.ptr(fb), H.ptr(fb_lo), H.ptr(fb_hi), H.ptr(out), B, S, T, scale.n_mels, scale.n_fft,
                                            scale.hop, scale.pad, scale.eps, H.stream()))
    return out


def log_mel_l1_launch(wav_hat, target, n_samples, scale, factor=1., want_log_mel=False):
    ''' the loss entry point as it is: (loss (B,), dwav (B, S) = factor x d sum(loss) / d wav_hat, L of wav_hat (B, T, M) or None) '''
    wav_hat = _check_wav(wav_hat.detach(), 'log_mel_l1')
    H.require_gpu(target)
    B, S = wav_hat.shape
    n_dev, n_host, values = _counts(n_samples, B, wav_hat.device)
    T = max(_frames(values, S, scale))
    M = scale.n_mels
    if target.dtype != torch.float32 or target.dim() != 3 or target.shape[0] != B or target.shape[1] < T or target.shape[2] != M:
        raise ValueError(f'log_mel_l1: the target is {target.dtype} {tuple(target.shape)}, expected fp32 ({B}, >= {T}, {M})')
    target = target.detach().contiguous()
    T = target.shape[1]
    twiddle, window, fb, fb_lo, fb_hi, bin_lo, bin_hi = scale.tables(wav_hat.device)
    loss = torch.empty((B,), dtype=torch.float32, device=wav_hat.device)
    dwav = torch.empty((B, S), dtype=torch.float32, device=wav_hat.device)
    own = torch.empty((B, T, M), dtype=torch.float32, device=wav_hat.device) if want_log_mel else None
    with torch.cuda.device(wav_hat.device):
        ws = _workspace(int(H.lib().dx_mel_loss_workspace(B, T, M, scale.n_fft)), wav_hat.device)
        H.check(H.lib().dx_mel_loss(H.ptr(wav_hat), wav_hat.stride(0), H.ptr(n_dev), ctypes.addressof(n_host), H.ptr(twiddle), H.ptr(window),
                                    H.ptr(fb), H.ptr(fb_lo), H.ptr(fb_hi), H.ptr(bin_lo), H.ptr(bin_hi), H.ptr(target), float(factor),
                                    H.ptr(loss), H.ptr(dwav), S, H.ptr(own), H.ptr(ws), B, S, T, M, scale.n_fft, scale.hop, scale.pad,
                                    scale.eps, H.stream()))
    return loss, dwav, own


class _LogMelL1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, wav_hat, target, n_samples, scale, factor):
        loss, dwav, _ = log_mel_l1_launch(wav_hat, target, n_samples, scale, factor)
        ctx.save_for_backward(dwav)
        return loss.sum() * factor

    @staticmethod
    def backward(ctx, grad):
        dwav, = ctx.saved_tensors
        return dwav * grad, None, None, None, None


def log_mel_l1(wav_hat, target, n_samples, scale, factor=1.):
    ''' factor x sum over the utterances, their frames and the M bands of |target - L(wav_hat)|: a device scalar, differentiable in
        wav_hat (B, S) -- the gradient is formed by the forward call and only multiplied by the incoming scalar in the backward.
        target (B, >= T, M): `log_mel` of the recording at the same n_samples and scale '''
    return _LogMelL1.apply(wav_hat, target, n_samples, scale, float(factor))


class MultiScaleMelLoss(nn.Module):
    ''' sum over the scales of the mean |log10-mel(audio) - log10-mel(y_hat)|, the reconstruction term BigVGAN-v2 trains against.
        Config keys: `mel_loss_window_lengths` (default 32 ... 2048), `mel_loss_n_mels` (default 5 ... 320), `lambda_melloss`
        (`weight`, default 15), `sampling_rate`.  `log_mel(wav (B, S), scale) -> (B, T, M)`, differentiable, replaces the HIP op (the
        host tests pass the CPU oracle). '''
    def __init__(self, cfg=None, log_mel=None):
        super().__init__()
        cfg = cfg or {}
        lengths, bands = cfg.get('mel_loss_window_lengths', WINDOW_LENGTHS), cfg.get('mel_loss_n_mels', N_MELS)
        if not lengths or len(lengths) != len(bands):
            raise ValueError(f'MultiScaleMelLoss: "mel_loss_window_lengths" has {len(lengths)} entries and "mel_loss_n_mels" {len(bands)}; '
                             f'they must pair up, and at least one scale is needed')
        if 'sampling_rate' not in cfg:
            raise ValueError('vocoder config: "sampling_rate" is missing')
        self.scales = [bigvgan_v2_scale(n, m, cfg['sampling_rate']) for n, m in zip(lengths, bands)]
        self.weight = float(cfg.get('lambda_melloss', WEIGHT))
        self._log_mel = log_mel

    def check_segment(self, S):
        ''' raises ValueError naming the first scale a segment of S samples is too short for '''
        for s in self.scales:
            if S <= s.pad or S + 2 * s.pad < s.n_fft:
                raise ValueError(f'MultiScaleMelLoss: a segment of {S} samples is too short for the scale (n_fft {s.n_fft}, hop {s.hop}, '
                                 f'{s.n_mels} bands): reflect padding of {s.pad} per side needs more than {s.pad} samples')

    def forward(self, audio, y_hat):
        ''' audio, y_hat (B, S), whole segments -> the device scalar; differentiable in y_hat '''
        if audio.shape != y_hat.shape or audio.dim() != 2:
            raise ValueError(f'MultiScaleMelLoss: audio {tuple(audio.shape)} and y_hat {tuple(y_hat.shape)} must both be (B, S)')
        B, S = audio.shape
        self.check_segment(S)
        total = 0.
        for s in self.scales:
            if self._log_mel is not None:
                total = total + F.l1_loss(self._log_mel(y_hat, s), self._log_mel(audio, s))
                continue
            n = [S] * B
            target = log_mel(audio, n, s)
            total = total + log_mel_l1(y_hat, target, n, s, 1. / (s.n_mels * B * s.frames(S)))
        return total
