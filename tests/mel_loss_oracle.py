"""Float64 restatement of K37 (one scale of the multi-scale mel loss with its gradient, csrc/mel_loss.hip), independent of the code
under test: an explicit DFT (no FFT, no torch.stft) with reflect indexing, the filter-bank matmul, log10(clamp), abs and autograd, plus
the backward once more as plain index sums.  tests/test_mel_loss_host.py pins it against `torch.stft(center=True, pad_mode='reflect')`
in float64.  The same code runs in float32 (`dtype=torch.float32`): the "o32" of the fp32 rule.  `signs`, where given, stands in place
of sign(Tg - L) in the gradient, so the GPU tests differentiate the float64 oracle on the kernel's own side of every |.|.

Per utterance of n samples and scale (n_fft, hop, p), window table w, filter bank fb (M, bins):
    x~[s] = x[r(s - p)], r the 'reflect' index;  F = 1 + (n + 2 p - n_fft) div hop
    X[f, k] = sum_j w[j] x~[f hop + j] exp(-2 pi i j k / n_fft);  mel = |X| fb^T;  L = log10(max(mel, eps))
"""
import functools
import math
from collections import namedtuple

import torch

EPS = 1e-5
SAMPLING_RATE = 22050
WINDOW_LENGTHS = (32, 64, 128, 256, 512, 1024, 2048)
N_MELS = (5, 10, 20, 40, 80, 160, 320)

# window (n_fft,) and fb (M, bins) are float64 tensors holding fp32 values (the kernel gets the same numbers)
Scale = namedtuple('Scale', 'n_fft hop pad window fb eps')


def frames_of(n, n_fft, hop, pad):
    assert n > pad and n + 2 * pad >= n_fft, (n, n_fft, hop, pad)
    return 1 + (n + 2 * pad - n_fft) // hop


def filter_bank(n_fft, n_mels, fmax=None):
    ''' the Slaney filter bank the project builds for every mel, an input of the kernel: (M, bins) float64 holding fp32 values '''
    from daft_exprt.extract_features import mel_filter_bank
    return torch.from_numpy(mel_filter_bank(SAMPLING_RATE, n_fft, n_mels, 0, fmax)).double()


def make_scale(n_fft, n_mels, hop=None, pad=None, fmax=None):
    ''' the module's scale of one window length (hop a quarter, centred padding, periodic Hann), or a general framing '''
    window = torch.hann_window(n_fft, periodic=True, dtype=torch.float64).float().double()
    return Scale(n_fft, n_fft // 4 if hop is None else hop, n_fft // 2 if pad is None else pad, window, filter_bank(n_fft, n_mels, fmax), EPS)


def reflect_index(n, p):
    ''' r(s - p) for s in [0, n + 2 p) '''
    i = torch.arange(-p, n + p)
    i = torch.where(i < 0, -i, i)
    return torch.where(i >= n, 2 * (n - 1) - i, i)


@functools.lru_cache(maxsize=None)
def dft_basis(n_fft, dtype):
    ''' (cos, sin) of 2 pi j k / n_fft, (n_fft, bins); the angle from j k mod n_fft in float64, rounded once to dtype '''
    bins = n_fft // 2 + 1
    phase = 2 * math.pi * ((torch.arange(n_fft)[:, None] * torch.arange(bins)[None, :]) % n_fft).double() / n_fft
    return torch.cos(phase).to(dtype), torch.sin(phase).to(dtype)


def stft_frames(x, scale):
    ''' x (n,) -> (re, im) (F, bins) of X in x's dtype; differentiable in x '''
    padded = x[reflect_index(x.shape[0], scale.pad)]
    frames = padded.unfold(0, scale.n_fft, scale.hop) * scale.window.to(x.dtype)
    c, s = dft_basis(scale.n_fft, x.dtype)
    return frames @ c, -(frames @ s)


def magnitude(x, scale):
    ''' x (n,) -> |X| (F, bins); torch.norm's gradient: 0 where |X| = 0 '''
    re, im = stft_frames(x, scale)
    return torch.linalg.vector_norm(torch.stack([re, im], dim=-1), dim=-1)


def log_mel_one(x, scale):
    ''' x (n,) -> (L (F, M), mel (F, M)) in x's dtype; differentiable in x (clamp's gradient: 1 where mel >= eps) '''
    mel = magnitude(x, scale) @ scale.fb.to(x.dtype).t()
    return torch.log10(torch.clamp(mel, min=scale.eps)), mel


def log_mel(wav, n, scale, dtype=torch.float64):
    ''' wav (B, S), n the live samples per utterance -> L (B, T, M) in dtype, T = max frames, zeros past each utterance's frames '''
    T = max(frames_of(k, scale.n_fft, scale.hop, scale.pad) for k in n)
    out = torch.zeros((len(n), T, scale.fb.shape[0]), dtype=dtype)
    for b, k in enumerate(n):
        L, _ = log_mel_one(wav[b, :k].to(dtype), scale)
        out[b, :L.shape[0]] = L
    return out


def loss_and_gradient(wav_hat, target, n, scale, dtype=torch.float64, signs=None):
    ''' wav_hat (B, S), target (B, >= T, M) -> (L (B, T, M), loss (B,), dwav (B, S)) in dtype: loss[b] = sum |target - L| over the
        utterance's frames, dwav its gradient (zeros past n[b]).  signs (B, >= T, M) in {-1, 0, 1}: used in place of sign(target - L)
        in the gradient (the loss stays the sum of absolute values) '''
    B, S = wav_hat.shape
    T = max(frames_of(k, scale.n_fft, scale.hop, scale.pad) for k in n)
    own = torch.zeros((B, T, scale.fb.shape[0]), dtype=dtype)
    loss, dwav = torch.zeros((B,), dtype=dtype), torch.zeros((B, S), dtype=dtype)
    for b, k in enumerate(n):
        x = wav_hat[b, :k].to(dtype).clone().requires_grad_(True)
        L, _ = log_mel_one(x, scale)
        d = target[b, :L.shape[0]].to(dtype) - L
        objective = d.abs().sum() if signs is None else (signs[b, :L.shape[0]].to(dtype) * d).sum()
        dwav[b, :k], = torch.autograd.grad(objective, x)
        own[b, :L.shape[0]], loss[b] = L.detach(), d.detach().abs().sum()
    return own, loss, dwav


def backward_index_sums(x, target, scale):
    ''' the gradient of sum |target - L(x)| as the kernel's contract states it, float64, no autograd: x (n,), target (F, M) -> (n,) '''
    x, target = x.double(), target.double()
    n, p, n_fft, hop, bins = x.shape[0], scale.pad, scale.n_fft, scale.hop, scale.n_fft // 2 + 1
    re, im = stft_frames(x, scale)                                  # (F, bins)
    nf = re.shape[0]
    norm = torch.sqrt(re ** 2 + im ** 2)
    mel = norm @ scale.fb.t()
    L = torch.log10(torch.clamp(mel, min=scale.eps))
    g = -torch.sign(target - L) * (mel >= scale.eps).double() / (torch.where(mel > 0, mel, torch.ones_like(mel)) * math.log(10.))
    dmag = g @ scale.fb                                             # (F, bins)
    ratio = torch.where(norm > 0, dmag / torch.where(norm > 0, norm, torch.ones_like(norm)), torch.zeros_like(norm))
    g_re, g_im = ratio * re, ratio * im
    phase = 2 * math.pi * ((torch.arange(n_fft)[:, None] * torch.arange(bins)[None, :]) % n_fft).double() / n_fft
    dy = (g_re @ torch.cos(phase).t() - g_im @ torch.sin(phase).t()) * scale.window        # Re sum_k G exp(+i phase): no bin doubled
    padded = torch.zeros(n + 2 * p, dtype=torch.float64)
    for f in range(nf):                                             # overlap-add, ascending frames
        padded[f * hop:f * hop + n_fft] += dy[f]
    dx = torch.zeros(n, dtype=torch.float64)
    for i in range(n):
        v = padded[i + p]
        if 1 <= i <= p:
            v = v + padded[p - i]
        if n - 1 - p <= i <= n - 2:
            v = v + padded[p + 2 * (n - 1) - i]
        dx[i] = v
    return dx


def conditioning(x, scale):
    ''' min |X| / max |X| over the bins and frames of x (n,) in float64: X / |X| is ill-conditioned near a zero of X '''
    m = magnitude(x.double(), scale)
    return float(m.min() / m.max())


# ---- the cases of tests/test_gpu_mel_loss.py -----------------------------------------------------------------------------------------
# name -> (n_fft, M, hop, pad, fmax, live samples of the B = 3 utterances).  Each first n is p + 1; the second crosses a workgroup of
# frames (32 frames at 32 points: 257 samples give 33; 16 at 64, 8 at 128, 4 at 256, 2 at 512, 1 from 1024 up)
CASES = {
    '32-5': (32, 5, None, None, None, (17, 257, 40)),
    '32-10': (32, 10, None, None, None, (17, 257, 40)),            # M above the frame's 8 threads
    '64-10': (64, 10, None, None, None, (33, 300, 97)),
    '128-20': (128, 20, None, None, None, (65, 515, 130)),
    '256-40': (256, 40, None, None, None, (129, 1100, 300)),
    '512-80': (512, 80, None, None, None, (257, 1500, 700)),
    '1024-160': (1024, 160, None, None, None, (513, 4113, 1100)),
    '2048-320': (2048, 320, None, None, None, (1025, 4113, 2100)),
    '256-general': (256, 40, 100, 78, 8000., (100, 500, 193)),     # HiFi-GAN's framing p = (n_fft - hop) / 2; the first: one frame
    '256-empty': (256, 320, None, None, None, (129, 1100, 300)),   # filters narrower than a bin: rows without a bin
}
SEED_CANDIDATES = 200
# per case the seed among the first SEED_CANDIDATES with the largest min |X| / max |X| of the generated waveform (`best_seed`), and that
# ratio; tests/test_mel_loss_host.py asserts them.  No threshold: at the larger sizes white noise does not reach 1e-3 (2048: no seed)
SEEDS = {
    '32-5': (176, 0.017442054615709374),
    '32-10': (176, 0.017442054615709374),
    '64-10': (21, 0.013454563196360325),
    '128-20': (106, 0.0054578882943928115),
    '256-40': (120, 0.0036882855286937623),
    '512-80': (94, 0.002361941271115919),
    '1024-160': (94, 0.0009509293894970285),
    '2048-320': (148, 0.0005525816113627031),
    '256-general': (107, 0.026502119880372852),
    '256-empty': (120, 0.0036882855286937623),
}
MODULE_SEGMENT, MODULE_BATCH, MODULE_SEED = 2048, 2, 0


def case_scale(name):
    n_fft, n_mels, hop, pad, fmax, _ = CASES[name]
    return make_scale(n_fft, n_mels, hop, pad, fmax)


def case_inputs(name, seed=None):
    ''' (scale, n, the recording (B, S), the generated waveform (B, S)), float64 holding fp32 values; S = max n '''
    n = CASES[name][5]
    g = torch.Generator().manual_seed(SEEDS[name][0] if seed is None else seed)
    audio = (0.3 * torch.randn((len(n), max(n)), generator=g, dtype=torch.float64)).float().double()
    wav_hat = (audio + 0.15 * torch.randn((len(n), max(n)), generator=g, dtype=torch.float64)).float().double()
    return case_scale(name), n, audio, wav_hat


def case_condition(name, seed=None):
    scale, n, _, wav_hat = case_inputs(name, seed)
    return min(conditioning(wav_hat[b, :k], scale) for b, k in enumerate(n))


def best_seed(name):
    ''' (seed, ratio): the best conditioned generated waveform among the first SEED_CANDIDATES seeds (the first of equal ratios) '''
    ratios = [case_condition(name, seed) for seed in range(SEED_CANDIDATES)]
    seed = max(range(SEED_CANDIDATES), key=lambda s: (ratios[s], -s))
    return seed, ratios[seed]


def module_inputs():
    ''' (the recordings, the generated waveforms) (2, 2048), float64 holding fp32 values '''
    g = torch.Generator().manual_seed(MODULE_SEED)
    audio = (0.3 * torch.randn((MODULE_BATCH, MODULE_SEGMENT), generator=g, dtype=torch.float64)).float().double()
    return audio, (audio + 0.15 * torch.randn(audio.shape, generator=g, dtype=torch.float64)).float().double()


def module_scales():
    return [make_scale(n, m) for n, m in zip(WINDOW_LENGTHS, N_MELS)]


def module_loss(audio, y_hat, dtype=torch.float64, signs=None):
    ''' sum over the seven scales of mean |L(audio) - L(y_hat)| -> (value, d value / d y_hat (B, S), [L(y_hat) per scale]);
        signs: per scale a (B, T, M) tensor in place of sign(L(audio) - L(y_hat)) '''
    n = [audio.shape[1]] * audio.shape[0]
    value, grad, owns = 0., torch.zeros(audio.shape, dtype=dtype), []
    for i, scale in enumerate(module_scales()):
        target = log_mel(audio, n, scale, dtype)
        own, loss, dwav = loss_and_gradient(y_hat, target, n, scale, dtype, None if signs is None else signs[i])
        count = target.numel()
        value, grad = value + loss.sum() / count, grad + dwav / count
        owns.append(own)
    return value, grad, owns
