"""Restatement of the two audio kernel families that share the in-LDS FFT of csrc/dx_fft.h -- K17, the mel / energy front-end
(csrc/frontend.hip) and K18, the Griffin-Lim preview path (csrc/griffin_lim.hip: NNLS mel -> linear, Griffin-Lim, noise, normalise) --
in NumPy, independent of the code under test and of `daft_exprt.*`: the filterbank is `oracle.mel_frontend_cpu.mel_filterbank`, the
Griffin-Lim loop and `normalise` are those of tests/griffin_lim_oracle.py, the hashes those of tests/dropout_masks.py.

Every function takes `dtype`: np.float64 is the truth ("o64"), np.float32 runs the same statements in float32 (NumPy's FFT, which
Griffin-Lim uses, keeps float32) and is the measured cost of the arithmetic ("o32") in the one tolerance rule of tests/test_gpu_audio_fft.py, `bound`:
    max |y - o64| <= max(8 x max |o32 - o64|, 2e-6 m),   m = max |o64|, per tensor and per utterance
The tables (`tables`) are the float64 definition; the kernels get them rounded to float32, and so does the float32 run.
tests/test_audio_fft_host.py pins this module to the goldens and to the older oracles, and asserts what the tolerances stand on for
every case of `FRONTEND_CASES`, `GL_CASES`, `NNLS_CASES`, `NOISE_CASE` and `NORMALISE_CASES` below."""
import functools

import numpy as np

from oracle.mel_frontend_cpu import mel_filterbank
from tests import griffin_lim_oracle as GO
from tests.dropout_masks import M32, key32, mix32

normalise = GO.normalise
SIZES = (256, 1024, 4096)
SR, FMIN, FMAX, MIN_CLIP = 22050, 0, 8000, 1e-5


def bound(o64, o32, factor=8.):
    ''' (cost = max |o32 - o64|, m = max |o64|, the bound) of one tensor of one utterance '''
    o64 = np.asarray(o64, np.float64)
    if o64.size == 0:
        return 0., 0., 0.
    cost, m = float(np.abs(np.asarray(o32, np.float64) - o64).max()), float(np.abs(o64).max())
    return cost, m, max(factor * cost, 2e-6 * m)


def ulps32(got, want64):
    ''' largest |got - float32(want64)| in units of the float32 spacing at float32(want64) '''
    want = np.asarray(want64, np.float64).astype(np.float32)
    d = np.abs(np.asarray(got, np.float32).astype(np.float64) - want.astype(np.float64))
    return float((d / np.spacing(np.abs(want)).astype(np.float64)).max()) if want.size else 0.


# ---- tables ----------------------------------------------------------------------------------------------------------------------

def _cospi(x):
    ''' cos(pi x), x >= 0 float64: folded to [0, 1/4] first, so that the quarter points are exact '''
    x = np.mod(np.asarray(x, np.float64), 2.0)
    x = np.where(x > 1.0, 2.0 - x, x)
    sign = np.where(x > 0.5, -1.0, 1.0)
    x = np.where(x > 0.5, 1.0 - x, x)
    return sign * np.where(x <= 0.25, np.cos(np.pi * x), np.sin(np.pi * (0.5 - x)))


def _sinpi(x):
    x = np.mod(np.asarray(x, np.float64), 2.0)
    sign = np.where(x > 1.0, -1.0, 1.0)
    x = np.where(x > 1.0, x - 1.0, x)
    x = np.where(x > 0.5, 1.0 - x, x)
    return sign * np.where(x <= 0.25, np.sin(np.pi * x), np.cos(np.pi * (0.5 - x)))


def tables(n_fft, symmetric):
    ''' (twiddle (n_fft, 2): cos, -sin of 2 pi n / n_fft; Hann window (n_fft,): 0.5 - 0.5 cos(2 pi n / n_fft), torch.hann_window, or
        with `symmetric` 0.5 - 0.5 cos(2 pi n / (n_fft - 1)), np.hanning), float64 '''
    n = np.arange(n_fft, dtype=np.float64)
    c, s = _cospi(2.0 * n / n_fft), _sinpi(2.0 * n / n_fft)
    window = 0.5 - 0.5 * (_cospi(2.0 * n / (n_fft - 1)) if symmetric else c)
    return np.stack([c, -s], axis=1), window


@functools.lru_cache(maxsize=1)
def dft_basis(n_fft):
    ''' (cos, sin) of 2 pi j k / n_fft, (n_fft, bins) float64: the table's entries at j k mod n_fft.  The front-end's spectrum is the
        definition X[k] = sum_j w[j] x[j] exp(-2 pi i j k / n_fft) as a matrix product (as tests/spectrogram_oracle.py), no library FFT:
        one that keeps the symmetry of its input is exact on the real spectrum of a centred utterance's first frame (reflect padding
        makes that frame even), and its float32 run then says nothing about what float32 costs there '''
    tw = tables(n_fft, False)[0]
    jk = (np.arange(n_fft, dtype=np.int64)[:, None] * np.arange(n_fft // 2 + 1, dtype=np.int64)[None, :]) % n_fft
    return tw[jk, 0], -tw[jk, 1]


def in_order(A, X):
    ''' A (M, K) @ X (K, F) with every sum taken in index order in the operands' dtype.  The filterbank products of both families go
        through it: a filter of n_mel 1 spans 94 (n_fft 256) to 1488 bins (4096), pinv(A) b cancels heavily at n_fft 256, and a blocked
        sum of that many float32 terms costs less than float32 does in any fixed order -- the kernels sum in index order '''
    if A.dtype == np.float64:                                        # the order moves float64 by 1e-16 m: not what is measured
        return A @ X
    nz = A != 0                                                      # a zero product adds nothing in any order: each row's sum is
    first = np.where(nz.any(1), nz.argmax(1), 0)                     # taken over its own stretch first .. last, W columns at the most
    last = np.where(nz.any(1), A.shape[1] - nz[:, ::-1].argmax(1), 0)
    W = max(int((last - first).max()), 1)
    cols = np.minimum(first[:, None] + np.arange(W)[None, :], A.shape[1] - 1)
    live = (np.arange(W)[None, :] < (last - first)[:, None])
    a = np.where(live, np.take_along_axis(A, cols, 1), A.dtype.type(0))
    return np.cumsum(a[:, :, None] * X[cols], axis=1)[:, -1, :]


# ---- front-end -------------------------------------------------------------------------------------------------------------------

def frame_count(n, n_fft, hop, centered):
    if centered:
        return 1 + n // hop if n >= 1 else 0
    return 1 + (n - n_fft) // hop if n >= n_fft else 0


def filterbank(n_fft, n_mel, fmin=FMIN, fmax=FMAX, sr=SR):
    return mel_filterbank(sr, n_fft, n_mel, fmin, fmax)


def mel_frontend(wav, n, n_fft, hop, n_mel, centered, min_clip=MIN_CLIP, fmin=FMIN, fmax=FMAX, sr=SR, dtype=np.float64):
    ''' wav (>= n,), its first n samples live -> (log-mel (n_mel, F), frame energy (F,)) in dtype, F = frame_count(...) '''
    dtype = np.dtype(dtype).type
    x = np.asarray(wav)[:n].astype(dtype)
    F = frame_count(n, n_fft, hop, centered)
    if F == 0:
        return np.zeros((n_mel, 0), dtype), np.zeros((0,), dtype)
    if centered:                                                     # torch.stft(center=True, pad_mode='reflect')
        p = n_fft // 2
        assert n > p, (n, n_fft)
        i = np.abs(np.arange(-p, n + p))
        x = x[np.where(i >= n, 2 * (n - 1) - i, i)]
    idx = (np.arange(F) * hop)[:, None] + np.arange(n_fft)[None, :]
    frames = x[idx] * tables(n_fft, False)[1].astype(dtype)
    cos, sin = dft_basis(n_fft)
    re, im = frames @ cos.astype(dtype), -(frames @ sin.astype(dtype))
    mag = np.sqrt(re ** 2 + im ** 2 + dtype(1e-9))
    assert mag.dtype == dtype
    c = np.maximum(in_order(filterbank(n_fft, n_mel, fmin, fmax, sr).astype(dtype), mag.T), dtype(np.float32(min_clip)))
    return np.log(c), np.sqrt((c * c).sum(0))


# ---- NNLS ------------------------------------------------------------------------------------------------------------------------

def nnls_tables(A):
    ''' A (n_mel, bins) float32 filterbank -> dict: pinv_t (n_mel, bins) float32 = pinv(A)^T from float64; lo, hi (n_mel,) int32, filter m
        non-zero on bins lo[m] .. hi[m] - 1 (lo = hi = 0 for an empty one); bin_m (bins, 2) int32, bin_w (bins, 2) float32: the at most
        two (filter, weight) pairs of a bin in order of the filter, -1 / 0 where there is none; step = 1 / ||A||_2^2 '''
    A64 = np.asarray(A, np.float32).astype(np.float64)
    n_mel, bins = A64.shape
    lo, hi = np.zeros(n_mel, np.int32), np.zeros(n_mel, np.int32)
    for m in range(n_mel):
        k = np.nonzero(A64[m] > 0)[0]
        if len(k):
            lo[m], hi[m] = k[0], k[-1] + 1
    bin_m, bin_w = np.full((bins, 2), -1, np.int32), np.zeros((bins, 2), np.float32)
    for k in range(bins):
        ms = np.nonzero(A64[:, k] > 0)[0]
        assert len(ms) <= 2, (k, ms)
        bin_m[k, :len(ms)] = ms
        bin_w[k, :len(ms)] = A64[ms, k]
    return dict(pinv_t=np.ascontiguousarray(np.linalg.pinv(A64).T).astype(np.float32), lo=lo, hi=hi, bin_m=bin_m, bin_w=bin_w,
                step=float(1.0 / np.linalg.norm(A64, 2) ** 2))


@functools.lru_cache(maxsize=None)
def case_tables(n_fft, n_mel):
    A = filterbank(n_fft, n_mel)
    return A, nnls_tables(A)


def objective(A, x, b):
    A, x, b = (np.asarray(a, np.float64) for a in (A, x, b))
    return 0.5 * ((A @ x - b) ** 2).sum(0)


def fista(A, b, iters, step, dtype=np.float64, pinv_t=None, trace=None):
    ''' A (n_mel, bins), b (n_mel, F) linear mel -> x (bins, F) after `iters` FISTA steps of size float32(step) from max(pinv(A) b, 0);
        `trace`: a list that receives the float64 objective per frame of the start and of every step '''
    dtype = np.dtype(dtype).type
    pinv_t = nnls_tables(A)['pinv_t'] if pinv_t is None else pinv_t
    A, b, P, step = np.asarray(A).astype(dtype), np.asarray(b).astype(dtype), np.asarray(pinv_t).astype(dtype), dtype(np.float32(step))
    x = np.maximum(in_order(np.ascontiguousarray(P.T), b), dtype(0))
    y, t = x, dtype(1)
    if trace is not None:
        trace.append(objective(A, x, b))
    for _ in range(iters):
        tn = dtype(0.5) * (dtype(1) + np.sqrt(dtype(1) + dtype(4) * t * t))
        mom = (t - dtype(1)) / tn
        xn = np.maximum(y - step * (A.T @ (in_order(A, y) - b)), dtype(0))       # A^T r: at most two terms per bin
        y = xn + mom * (xn - x)
        x, t = xn, tn
        if trace is not None:
            trace.append(objective(A, x, b))
    assert x.dtype == dtype
    return x


def mel_to_linear(mel, A, iters, step, input_is_log, dtype=np.float64, pinv_t=None):
    ''' dx_mel_to_linear of one utterance: mel (n_mel, F), log-mel with `input_is_log` '''
    mel = np.asarray(mel).astype(dtype)
    return fista(A, np.exp(mel) if input_is_log else mel, iters, step, dtype, pinv_t)


# ---- Griffin-Lim -----------------------------------------------------------------------------------------------------------------

def griffin_lim(mag, hop, iterations, x0, dtype=np.float64, spectra=None):
    ''' tests/griffin_lim_oracle.griffin_lim, statement by statement, in dtype (float64: the same bits, tests/test_audio_fft_host.py).
        `spectra`: a list that receives |rfft| (F, bins) of every iteration's input frames '''
    dtype = np.dtype(dtype).type
    mag = np.asarray(mag, dtype=dtype).T
    n_fft = (mag.shape[1] - 1) * 2
    F = mag.shape[0]
    S = F * hop + n_fft
    window = np.hanning(n_fft).astype(dtype)
    x = np.asarray(x0, dtype=dtype).copy()
    assert x.shape == (S,)
    starts = np.arange(0, S - n_fft, hop)
    assert len(starts) == F
    idx = starts[:, None] + np.arange(n_fft)[None, :]
    out, proposal = [], None
    for _ in range(iterations):
        spec = np.fft.rfft(window * x[idx], axis=1)
        if spectra is not None:
            spectra.append(np.abs(spec))
        proposal = mag * np.exp(1.0j * np.angle(spec))
        frames = window * np.real(np.fft.irfft(proposal, axis=1))
        x = np.zeros(S, dtype)
        for i in range(F):                       # overlap-add in frame order, like the reference's loop
            x[starts[i]: starts[i] + n_fft] += frames[i]
        x = x / dtype(n_fft / hop / 2)
        assert x.dtype == dtype
        out.append(x)
    return out, proposal


# ---- noise -----------------------------------------------------------------------------------------------------------------------

def noise(seed, b, s, dtype=np.float64):
    ''' the start signal of utterance b at the samples s (array): Box-Muller of two counter hashes of (seed, b, s) '''
    dtype = np.dtype(dtype).type
    key = np.uint64(key32(seed, b))
    s = np.asarray(s, dtype=np.uint64)
    h1 = mix32(key ^ mix32((np.uint64(2) * s + np.uint64(0x68E31DA4)) & M32))
    h2 = mix32(key ^ mix32((np.uint64(2) * s + np.uint64(0x68E31DA5)) & M32))
    u1 = ((h1 >> np.uint64(8)) + np.uint64(1)).astype(dtype) * dtype(2.0 ** -24)          # (0, 1], exact
    u2 = (h2 >> np.uint64(8)).astype(dtype) * dtype(2.0 ** -24)                           # [0, 1), exact
    v = np.sqrt(dtype(-2) * np.log(u1)) * np.cos(dtype(2 * np.pi) * u2)
    assert v.dtype == dtype
    return v


# ---- the cases of tests/test_gpu_audio_fft.py ------------------------------------------------------------------------------------

def _f32(a):
    ''' float64 holding float32 values: the kernel gets the same numbers '''
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def _odd_hop(n_fft):
    return n_fft // 4 + 3                                             # divides no n_fft


N_MELS = (1, 64, 65, 80)                                              # 65 > the 64 lanes of the front-end at n_fft 256
# name -> (n_fft, hop, centred, live samples per utterance, seed).  Not centred: 0, 1, 1 and 2 frames, each one sample short of or at
# a frame's end; centred: the shortest length reflect padding admits (every sample reflected at both ends), hop k - 1 and hop k
FRONTEND_CASES = {}
for _n in SIZES:
    for _hop in (_n // 4, _odd_hop(_n)):
        FRONTEND_CASES[f'{_n}-{_hop}-c0'] = (_n, _hop, 0, (_n - 1, _n, _n + _hop - 1, _n + _hop), _n + _hop)
        FRONTEND_CASES[f'{_n}-{_hop}-c1'] = (_n, _hop, 1, (_n // 2 + 1, 5 * _hop - 1, 5 * _hop), _n + _hop + 1)


def frontend_inputs(name):
    ''' (n_fft, hop, centred, n, wav (B, max n)) '''
    n_fft, hop, centred, n, seed = FRONTEND_CASES[name]
    wav = _f32(0.3 * np.random.RandomState(seed).randn(len(n), max(n)))
    return n_fft, hop, centred, n, wav


# the three signals of test_front_end_silence_tone_and_clipping: silence, a tone loud enough that no channel is clipped, a quiet low tone
# whose upper channels are all clipped (the host file asserts both properties); centred, hop n_fft / 4, 4 frames
TONE_LOUD, TONE_QUIET = (64., 0.271), (1e-3, 0.013)                   # (amplitude, frequency as a fraction of the n_fft / 2 bins)


def tone_inputs(n_fft):
    ''' (hop, n, wav (3, n)): silence; TONE_LOUD; TONE_QUIET.  The tones sit between two bins: floor(n_fft / 2 * fraction) + 0.37 '''
    hop, n = n_fft // 4, 3 * (n_fft // 4) + 5
    t = np.arange(n)
    wav = np.zeros((3, n))
    for row, (amp, frac) in ((1, TONE_LOUD), (2, TONE_QUIET)):
        k = np.floor(n_fft / 2 * frac) + 0.37
        wav[row] = amp * np.sin(2 * np.pi * k * t / n_fft + 0.5)
    return hop, (n, n, n), _f32(wav)


# name -> (n_fft, hop, seed): B = 5 utterances of GL_LENGTHS mel frames = 5, 2, 1, 0, 0 Griffin-Lim frames, GL_T frames of magnitude
GL_LENGTHS, GL_T = (7, 4, 3, 2, 0), 8
CONDITION = 1e-3                                                      # min |R| >= CONDITION x median |R| over the bins and frames used
GL_CASES = {f'{_n}-{_hop}': (_n, _hop) for _n in SIZES for _hop in (_n // 4, _n // 8, _n // 2)}
GL_SEEDS = {name: 0 for name in GL_CASES}                             # each the first seed whose ratio over two iterations is at least
GL_SEEDS['256-32'] = 1                                                # twice CONDITION (searched once on the CPU, fixed)
# utterance 0 starts from x0 = 0: every bin takes the R = 0 branch.  ONE iteration: the second one's input, the overlap-add of
# w irfft(S), misses CONDITION at 1024 (7.5e-4) and 4096 (1.9e-4) whatever the seed
GL_ZERO_LENGTHS = (5, 4)


def gl_inputs(name, seed=None, lengths=GL_LENGTHS, zero_first=False):
    ''' (n_fft, hop, lengths, mag (B, bins, GL_T), x0 (B, S)), S = (GL_T - 2) hop + n_fft '''
    n_fft, hop = GL_CASES[name]
    rng = np.random.RandomState(GL_SEEDS[name] if seed is None else seed)
    S = GO.n_samples(GL_T, n_fft, hop)
    mag = _f32(np.stack([GO.harmonic_magnitude(GL_T, n_fft=n_fft, f0=110. + 7 * b) for b in range(len(lengths))]))
    x0 = _f32(rng.randn(len(lengths), S))
    if zero_first:
        x0[0] = 0.
    return n_fft, hop, lengths, mag, x0


def gl_oracle(name, iterations, dtype=np.float64, spectra=None, **kw):
    ''' per utterance the signal (n_samples[b],) after `iterations` '''
    n_fft, hop, lengths, mag, x0 = gl_inputs(name, **kw)
    out = []
    for b, T in enumerate(lengths):
        F, Sb = GO.n_frames(T), GO.n_samples(T, n_fft, hop)
        if F == 0:
            out.append(np.zeros(Sb, dtype))
            continue
        seen = None if spectra is None else []
        out.append(griffin_lim(mag[b, :, :F], hop, iterations, x0[b, :Sb], dtype, seen)[0][-1])
        if spectra is not None:
            spectra.extend(seen)
    return out


def gl_condition(name, iterations=2, **kw):
    ''' min over the utterances and iterations of min |R| / median |R|; an input that is zero everywhere (x0 = 0) takes the exact
        R = 0 branch and does not count '''
    spectra = []
    gl_oracle(name, iterations, spectra=spectra, **kw)
    return min(float(r.min() / np.median(r)) for r in spectra if r.max() > 0)


# (n_fft, n_mel) -> seed; B = 3 utterances of (NNLS_T, 1, 0) frames
NNLS_MELS, NNLS_ITERS, NNLS_T = (1, 64, 65, 80, 256), (0, 1, 5, 50), 4
NNLS_CASES = {(_n, _m): 1000 * _i + _m for _i, _n in enumerate(SIZES) for _m in NNLS_MELS}


# Where exp() stands in front of the solve (input_is_log), its last bit is an input error that pinv(A) amplifies: by less than 2 ulp at
# thirteen pairs, by 9 to 37 ulp at (256, 64) and (256, 80), whose pinv(A) has norm 8e7 and 2e6 (the narrow filters of n_fft 256 share their
# one or two bins).  A correctly rounded expf would miss the rule there, so the log-mel comparison is made where the worst case of ONE
# float32 ulp on every b[m], max_k sum_m |pinv(A)[k, m]| b[m] 2^-24, stays below the rule's floor over the rule's factor, 2e-6 m / 8.
# Linear input runs at all fifteen pairs.  tests/test_audio_fft_host.py asserts that this list is what the criterion gives
NNLS_LOG_PAIRS = tuple(k for k in NNLS_CASES if k not in ((256, 64), (256, 80)))


def nnls_log_sensitivity(n_fft, n_mel):
    ''' the largest of that worst case over the utterances of the pair's case, as a fraction of m = max |o64| at the start '''
    A, t = case_tables(n_fft, n_mel)
    P = np.abs(t['pinv_t'].astype(np.float64))
    lengths, mel = nnls_inputs(n_fft, n_mel, 1)
    worst = 0.
    for b, L in enumerate(lengths):
        if L:
            x = mel_to_linear(mel[b, :, :L], A, 0, t['step'], 1, np.float64, t['pinv_t'])
            worst = max(worst, float((P.T @ np.exp(mel[b, :, :L])).max() * 2.0 ** -24 / np.abs(x).max()))
    return worst


def nnls_inputs(n_fft, n_mel, input_is_log):
    ''' (lengths, mel (3, n_mel, NNLS_T)): the filterbank's image of a harmonic magnitude, multiplicative noise on both, clipped like the
        front-end's (the empty filters of n_fft 256 give the floor), as log or linear mel '''
    A = case_tables(n_fft, n_mel)[0].astype(np.float64)
    rng = np.random.RandomState(NNLS_CASES[(n_fft, n_mel)])
    mel = np.empty((3, n_mel, NNLS_T))
    for b in range(3):
        mag = GO.harmonic_magnitude(NNLS_T, n_fft=n_fft, f0=120. + 30 * b) * np.exp(0.3 * rng.randn(n_fft // 2 + 1, NNLS_T))
        mel[b] = np.maximum(A @ mag, MIN_CLIP) * np.exp(0.2 * rng.randn(n_mel, NNLS_T))       # no x >= 0 reaches it exactly
    return (NNLS_T, 1, 0), _f32(np.log(mel) if input_is_log else mel)


# (n_fft, hop, T, lengths, seeds): samples reach past one 256-thread block; seed 2^64 - 1 has every bit of both halves set
NOISE_CASE = (256, 64, 13, (12, 3, 0), (0, 1, 2 ** 64 - 1))

# name -> (n_fft, hop, T, lengths, sign): B = 4: the peak at sample 0; at the last live sample, of the other sign; all zero; at most 2
# frames (zeroed whatever it held)
NORMALISE_CASES = {'256-64': (256, 64, 9, (8, 5, 6, 2), 1.), '1024-512': (1024, 512, 7, (5, 6, 4, 1), -1.)}
HUGE = 1e30                                                           # stands past n_samples[b], below S: finite, so fmaxf would keep it


def normalise_inputs(name):
    ''' (n_fft, hop, T, lengths, x (B, S)) with the dead samples still zero '''
    n_fft, hop, T, lengths, sign = NORMALISE_CASES[name]
    S = GO.n_samples(T, n_fft, hop)
    rng = np.random.RandomState(n_fft)
    x = np.zeros((len(lengths), S))
    for b, L in enumerate(lengths):
        Sb = GO.n_samples(L, n_fft, hop)
        x[b, :Sb] = rng.uniform(-1., 1., Sb)
    x[0, 0] = 1.75 * sign
    x[1, GO.n_samples(lengths[1], n_fft, hop) - 1] = -2.5 * sign
    x[2] = 0.
    return n_fft, hop, T, lengths, _f32(x)
