"""Float64 restatement of K36 (the magnitude spectrogram of a waveform and its gradient, csrc/spectrogram.hip) and of BigVGAN's
`DiscriminatorR` (Lee et al. 2023, section 3) over it, independent of the code under test: an explicit DFT (no FFT, no torch.stft)
under autograd, plus the backward once more as plain index sums.  tests/test_spectrogram_host.py pins all of it against
`torch.stft` + `torch.norm` + autograd in float64.  The same code runs in float32 (`dtype=torch.float32`): the "o32" of the fp32 rule.

Per utterance of n samples and resolution (n_fft, hop), window table w:
    p = (n_fft - hop) div 2;  x~[s] = x[r(s - p)], r the 'reflect' index;  F = 1 + (n + 2 p - n_fft) div hop
    X[f, k] = sum_j w[j] x~[f hop + j] exp(-2 pi i j k / n_fft), k in [0, n_fft / 2];  mag[k, f] = |X[f, k]|
"""
import math

import torch
import torch.nn.functional as F

RESOLUTIONS = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))
D_SLOPE = 0.1


def frames_of(n, n_fft, hop):
    p = (n_fft - hop) // 2
    assert n > p and n + 2 * p >= n_fft, (n, n_fft, hop)
    return 1 + (n + 2 * p - n_fft) // hop


def window_table(n_fft, win=None, dtype=torch.float64):
    ''' torch.stft's window=None at win_length win: ones on [l, l + win), l = (n_fft - win) div 2 '''
    win = n_fft if win is None else win
    w = torch.zeros(n_fft, dtype=dtype)
    left = (n_fft - win) // 2
    w[left:left + win] = 1.
    return w


def reflect_index(n, p):
    ''' r(s - p) for s in [0, n + 2 p) '''
    i = torch.arange(-p, n + p)
    i = torch.where(i < 0, -i, i)
    return torch.where(i >= n, 2 * (n - 1) - i, i)


def dft_basis(n_fft, dtype):
    ''' (cos, sin) of 2 pi j k / n_fft, (n_fft, bins); the angle from j k mod n_fft in float64, rounded once to dtype '''
    bins = n_fft // 2 + 1
    phase = 2 * math.pi * ((torch.arange(n_fft)[:, None] * torch.arange(bins)[None, :]) % n_fft).double() / n_fft
    return torch.cos(phase).to(dtype), torch.sin(phase).to(dtype)


def stft_frames(x, n_fft, hop, window):
    ''' x (n,) -> (re, im) (F, bins) of X; differentiable in x '''
    n, p = x.shape[0], (n_fft - hop) // 2
    padded = x[reflect_index(n, p)]
    frames = padded.unfold(0, n_fft, hop) * window.to(x.dtype)
    c, s = dft_basis(n_fft, x.dtype)
    return frames @ c, -(frames @ s)


def magnitude(x, n_fft, hop, window):
    ''' x (n,) -> (bins, F); torch.norm's gradient: 0 where |X| = 0 '''
    re, im = stft_frames(x, n_fft, hop, window)
    return torch.linalg.vector_norm(torch.stack([re, im], dim=-1), dim=-1).t()


def spectrogram(wav, n, n_fft, hop, window, dtype=torch.float64, dmag=None):
    ''' wav (B, S), n the live samples per utterance -> mag (B, bins, T) in dtype, T = max frames, zeros past each utterance's frames;
        with dmag (B, bins, T) also the gradient (B, S) of sum(mag * dmag) in wav, zeros past n (frames of dmag past F_b do not count) '''
    B, S = wav.shape
    T = max(frames_of(k, n_fft, hop) for k in n)
    mag = torch.zeros((B, n_fft // 2 + 1, T), dtype=dtype)
    dwav = torch.zeros((B, S), dtype=dtype)
    for b, k in enumerate(n):
        x = wav[b, :k].to(dtype).clone().requires_grad_(dmag is not None)
        m = magnitude(x, n_fft, hop, window.to(dtype))
        mag[b, :, :m.shape[1]] = m.detach()
        if dmag is not None:
            g = dmag[b, :, :m.shape[1]].to(dtype)
            dwav[b, :k], = torch.autograd.grad((m * g).sum(), x)
    return (mag, dwav) if dmag is not None else mag


def backward_index_sums(x, dmag, n_fft, hop, window):
    ''' the backward of `magnitude` as the kernel's contract states it, float64, no autograd: x (n,), dmag (bins, F) -> dx (n,) '''
    x, dmag, window = x.double(), dmag.double(), window.double()
    n, p, bins = x.shape[0], (n_fft - hop) // 2, n_fft // 2 + 1
    re, im = stft_frames(x, n_fft, hop, window)                     # (F, bins)
    nf = re.shape[0]
    norm = torch.sqrt(re ** 2 + im ** 2)
    scale = torch.where(norm > 0, dmag.t() / torch.where(norm > 0, norm, torch.ones_like(norm)), torch.zeros_like(norm))
    g_re, g_im = scale * re, scale * im
    phase = 2 * math.pi * ((torch.arange(n_fft)[:, None] * torch.arange(bins)[None, :]) % n_fft).double() / n_fft
    # Re sum_k (g_re + i g_im)(cos + i sin) = sum_k g_re cos - g_im sin: the one-sided sum, no bin doubled
    dy = (g_re @ torch.cos(phase).t() - g_im @ torch.sin(phase).t()) * window               # (F, n_fft)
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


def conditioning(x, n_fft, hop, window):
    ''' min |X| / max |X| over the bins and frames of x (n,) in float64: X / |X| is ill-conditioned near a zero of X '''
    m = magnitude(x.double(), n_fft, hop, window.double())
    return float(m.min() / m.max())


# ---- DiscriminatorR ------------------------------------------------------------------------------------------------------------

R_CONVS = (((3, 9), (1, 1), (1, 4)), ((3, 9), (1, 2), (1, 4)), ((3, 9), (1, 2), (1, 4)), ((3, 9), (1, 2), (1, 4)),
           ((3, 3), (1, 1), (1, 1)))                                  # (kernel, stride, padding) of `convs`; conv_post: (3, 3), 1, (1, 1)


def make_r_weights(mult=1, seed=0):
    ''' a `DiscriminatorR` state dict under weight norm's names, float64 '''
    g = torch.Generator().manual_seed(seed)
    c, sd = 32 * mult, {}
    shapes = [(c, 1, 3, 9), (c, c, 3, 9), (c, c, 3, 9), (c, c, 3, 9), (c, c, 3, 3)]
    for name, shape in [(f'convs.{i}', s) for i, s in enumerate(shapes)] + [('conv_post', (1, c, 3, 3))]:
        fan = shape[1] * shape[2] * shape[3]
        v = torch.randn(shape, generator=g, dtype=torch.float64) / fan ** 0.5
        sd[f'{name}.weight_v'] = v
        sd[f'{name}.weight_g'] = v.flatten(1).norm(dim=1).reshape(-1, 1, 1, 1) * (0.8 + 0.4 * torch.rand((shape[0], 1, 1, 1), generator=g,
                                                                                                              dtype=torch.float64))
        sd[f'{name}.bias'] = 0.1 * torch.randn((shape[0],), generator=g, dtype=torch.float64)
    return sd


def _weight(sd, name, dtype):
    v, g = sd[f'{name}.weight_v'].to(dtype), sd[f'{name}.weight_g'].to(dtype)
    return g * v / v.flatten(1).norm(dim=1).reshape(-1, 1, 1, 1), sd[f'{name}.bias'].to(dtype)


def discriminator_r(sd, wav, resolution, dtype=torch.float64, proj=None):
    ''' wav (B, S), every utterance whole -> (scores (B, -1), feature maps); with proj (like scores; True: ones) also
        d sum(scores * proj) / d wav '''
    n_fft, hop, win = resolution
    x = wav.to(dtype).clone().requires_grad_(proj is not None)
    w = window_table(n_fft, win, dtype)
    h = torch.stack([magnitude(x[b], n_fft, hop, w) for b in range(x.shape[0])])[:, None]       # (B, 1, bins, T)
    fmap = []
    for i, (_, stride, pad) in enumerate(R_CONVS):
        weight, bias = _weight(sd, f'convs.{i}', dtype)
        h = F.leaky_relu(F.conv2d(h, weight, bias, stride=stride, padding=pad), D_SLOPE)
        fmap.append(h)
    weight, bias = _weight(sd, 'conv_post', dtype)
    h = F.conv2d(h, weight, bias, padding=(1, 1))
    fmap.append(h)
    scores = h.flatten(1)
    if proj is None:
        return scores.detach(), [t.detach() for t in fmap]
    proj = torch.ones_like(scores) if proj is True else proj.to(dtype)
    dwav, = torch.autograd.grad((scores * proj).sum(), x)
    return scores.detach(), [t.detach() for t in fmap], dwav


# ---- the cases of tests/test_gpu_spectrogram.py, whose conditioning tests/test_spectrogram_host.py asserts ---------------------------

def last_partial_length(n_fft, hop, at_least):
    ''' the smallest n >= at_least with (n + 2 p - n_fft) mod hop = hop - 1: one sample short of another frame '''
    p = (n_fft - hop) // 2
    n = at_least
    while (n + 2 * p - n_fft) % hop != hop - 1:
        n += 1
    return n


def _lengths(n_fft, hop):
    p = (n_fft - hop) // 2
    return (p + 1, 4113, 2 * p + 1), (last_partial_length(n_fft, hop, 2 * p + 2), p + 2, 4113)


# (name, n_fft, hop, win or 'hann', live samples of the B = 3 utterances, seed).  The seeds were searched once (about one in five fails
# `CONDITION` at these sizes) and are fixed
CONDITION = 1e-3
SEEDS = {'512-50-240-a': 1, '512-50-240-b': 1, '1024-120-600-a': 2, '1024-120-600-b': 3, '2048-240-1200-a': 0, '2048-240-1200-b': 3,
         '256-64-hann': 0, '4096-1024-hann': 2}       # each the first seed whose ratio is at least twice CONDITION
CASES = []
for _n_fft, _hop, _win in sorted(RESOLUTIONS):
    for _i, _n in enumerate(_lengths(_n_fft, _hop)):
        CASES.append((f'{_n_fft}-{_hop}-{_win}-{"ab"[_i]}', _n_fft, _hop, _win, _n))
CASES.append(('256-64-hann', 256, 64, 'hann', (97, 500, 193)))
CASES.append(('4096-1024-hann', 4096, 1024, 'hann', (6000, 1537, 3073)))
MODULE_SEGMENT, MODULE_BATCH = 2048, 2
MODULE_SEEDS = {(1024, 120, 600): 0, (2048, 240, 1200): 0, (512, 50, 240): 0}


def case_window(n_fft, win, dtype=torch.float64):
    if win == 'hann':
        return torch.hann_window(n_fft, periodic=True, dtype=torch.float64).float().to(dtype)
    return window_table(n_fft, win, dtype)


def case_inputs(name, seed=None):
    ''' (n_fft, hop, window (n_fft,), n, wav (B, S), dmag (B, bins, T)), float64 holding fp32 values (the kernel gets the same numbers);
        S = max n '''
    _, n_fft, hop, win, n = next(c for c in CASES if c[0] == name)
    g = torch.Generator().manual_seed(SEEDS[name] if seed is None else seed)
    wav = (0.3 * torch.randn((len(n), max(n)), generator=g, dtype=torch.float64)).float().double()
    T = max(frames_of(k, n_fft, hop) for k in n)
    dmag = torch.randn((len(n), n_fft // 2 + 1, T), generator=g, dtype=torch.float64).float().double()
    return n_fft, hop, case_window(n_fft, win), n, wav, dmag


def case_condition(name, seed=None):
    n_fft, hop, window, n, wav, _ = case_inputs(name, seed)
    return min(conditioning(wav[b, :k], n_fft, hop, window) for b, k in enumerate(n))


def module_wav(resolution, seed=None):
    g = torch.Generator().manual_seed(MODULE_SEEDS[tuple(resolution)] if seed is None else seed)
    return (0.3 * torch.randn((MODULE_BATCH, MODULE_SEGMENT), generator=g, dtype=torch.float64)).float().double()


def module_condition(resolution, seed=None):
    n_fft, hop, win = resolution
    wav = module_wav(resolution, seed)
    return min(conditioning(wav[b], n_fft, hop, window_table(n_fft, win)) for b in range(wav.shape[0]))
