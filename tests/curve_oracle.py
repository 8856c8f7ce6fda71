"""float64 oracle of the prosody-transfer metric (`dx_curve_pcc`, daft_exprt/evaluate.py), NumPy only.

Restates `scripts/evaluation/compare_pitch_curves.py:5-45` of the reference: unvoiced removal (values > 0 are kept, in order),
`scipy.signal.resample` for real input written with np.fft.rfft / irfft (scipy may be absent where the GPU tests run; the two
agree to 5e-13, tests/test_prosody_eval_host.py checks the fixture to 1e-12), Pearson's correlation in two passes.  One
extension: an empty curve (either one) or a zero standard deviation gives NaN; the reference raises ValueError for an empty
curve to resample and returns NaN (with a warning) for the rest.

Also here, shared by tests/test_prosody_eval_host.py and tests/test_gpu_prosody_eval.py:
  * `direct_f32`: the kernel's arithmetic restated in NumPy float32 -- the curve centred on its mean, twiddles computed in
    double and rounded once, the angle index k n mod N in integers, the two direct sums in float32 (NumPy's pairwise order, not
    the kernel's four interleaved accumulators), the correlation in double;
  * the test curves and the branch cases;
  * F32_PCC_ERR / F32_RESAMPLED_ERR: the largest error of `direct_f32` against the oracle over those cases, measured on the
    host and asserted there.  The GPU tests allow TOL_FACTOR = 10 times that: the headroom this project gives a kernel whose
    sums run in another order than the restatement's (cf. tests/test_gpu_griffin_lim.py), not a figure taken from the kernel.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pitch_pcc.npz')

# largest |pcc - oracle| and |resampled - oracle| of `direct_f32` over `all_cases()` (the limit row included), rounded up
F32_PCC_ERR = 1.5e-6                # measured 1.41e-6 (a 4-point reference curve)
F32_RESAMPLED_ERR = 3.2e-7          # measured 3.09e-7 (the limit row; an ulp of 5.0 is 4.8e-7)
TOL_FACTOR = 10.0
MAX_LEN = 4096                       # dx_curve_pcc_max_len()

# (kept_ref, kept_dut): equal / odd / even lengths on both sides of the Nyquist rule, tiny curves, up- and downsampling
BRANCH_PAIRS = [(64, 64), (63, 64), (64, 63), (65, 64), (64, 66), (4, 6), (6, 4), (3, 2), (2, 3), (200, 137), (777, 1000)]


def remove_unvoiced(x):
    x = np.asarray(x, dtype=np.float64)
    return x[x > 0]


def resample(x, num):
    ''' scipy.signal.resample(x, num) for a real 1-D x (scipy 1.15 `signal/_signaltools.py`, the rfft branch) '''
    x = np.asarray(x, dtype=np.float64)
    Nx = x.shape[0]
    X = np.fft.rfft(x)
    N = min(num, Nx)
    Y = np.zeros(num // 2 + 1, dtype=np.complex128)
    Y[:N // 2 + 1] = X[:N // 2 + 1]
    if N % 2 == 0:
        if num < Nx:
            Y[N // 2] *= 2.0
        elif Nx < num:
            Y[N // 2] *= 0.5
    return np.fft.irfft(Y, num) * (float(num) / float(Nx))


def pearson(x, y):
    ''' `_pcc` (compare_pitch_curves.py:5-13); NaN where it divides by a zero standard deviation '''
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    dx, dy = x - np.mean(x), y - np.mean(y)
    sx, sy = np.sqrt(np.mean(dx * dx)), np.sqrt(np.mean(dy * dy))
    if not (sx > 0 and sy > 0):
        return float('nan')
    return float(np.mean(dx * dy) / (sy * sx))


def curve_pcc(ref, dut, remove=True):
    ''' (pcc, kept_ref, kept_dut, resampled (kept_ref,) float64) of one pair of curves '''
    ref, dut = np.asarray(ref, dtype=np.float64), np.asarray(dut, dtype=np.float64)
    if remove:
        ref, dut = remove_unvoiced(ref), remove_unvoiced(dut)
    if len(ref) == 0 or len(dut) == 0:
        return float('nan'), len(ref), len(dut), np.full(len(ref), np.nan)
    y = resample(dut, len(ref))
    return pearson(ref, y), len(ref), len(dut), y


def _table(N, dtype):
    i = np.arange(N, dtype=np.float64)
    return np.cos(2 * np.pi * i / N).astype(dtype), np.sin(2 * np.pi * i / N).astype(dtype)


def direct_f32(ref, dut, remove=True, dtype=np.float32):
    ''' the direct sums of the kernel in `dtype`: (pcc, resampled (kept_ref,) dtype) of a pair with two non-empty curves '''
    ref, dut = np.asarray(ref, dtype=dtype), np.asarray(dut, dtype=dtype)
    if remove:
        ref, dut = ref[ref > 0], dut[dut > 0]
    num, Nx = len(ref), len(dut)
    mean = dtype(np.mean(dut.astype(np.float64)))
    x = dut - mean
    N = min(num, Nx)
    k = np.arange(N // 2 + 1, dtype=np.int64)
    c, s = _table(Nx, dtype)
    idx = (k[:, None] * np.arange(Nx, dtype=np.int64)[None, :]) % Nx
    w = np.where(k == 0, 1.0, 2.0)
    if N % 2 == 0 and N // 2 > 0 and num >= Nx:
        w[N // 2] = 1.0
    w = (w.astype(dtype) / dtype(Nx)).astype(dtype)
    re = w * np.sum(x[None, :] * c[idx], axis=1, dtype=dtype)
    im = w * np.sum(-x[None, :] * s[idx], axis=1, dtype=dtype)
    c, s = _table(num, dtype)
    idx = (np.arange(num, dtype=np.int64)[:, None] * k[None, :]) % num
    y = mean + np.sum(re[None, :] * c[idx] - im[None, :] * s[idx], axis=1, dtype=dtype)
    return pearson(ref, y), y.astype(dtype)


# ---- test curves: log-Hz like, 5 +- 0.3 with structure (a near-constant curve makes the correlation ill-conditioned in the
# reference itself) ------------------------------------------------------------------------------------------------------------

def _contour(rng):
    ''' a smooth function on [0, 1] around 5 with ~0.3 of swing: a declination line and a few random sinusoids '''
    f = rng.uniform(0.7, 6.0, size=4)
    a = rng.uniform(0.04, 0.12, size=4) * rng.choice([-1.0, 1.0], size=4)
    p = rng.uniform(0, 2 * np.pi, size=4)
    slope = rng.uniform(-0.2, 0.2)
    return lambda t: 5.0 + slope * (t - 0.5) + sum(a[i] * np.sin(2 * np.pi * f[i] * t + p[i]) for i in range(4))


def voiced_pair(n_ref, n_dut, seed):
    ''' two fully voiced float32 curves of the same contour sampled at n_ref / n_dut points, the second one perturbed '''
    rng = np.random.RandomState(seed)
    g, h = _contour(rng), _contour(rng)
    tr, td = (np.arange(n_ref) + 0.5) / n_ref, (np.arange(n_dut) + 0.5) / n_dut
    ref = g(tr) + 0.01 * rng.standard_normal(n_ref)
    dut = g(td) + 0.5 * (h(td) - 5.0) + 0.01 * rng.standard_normal(n_dut)
    return ref.astype(np.float32), dut.astype(np.float32)


def with_unvoiced(x, seed):
    ''' x with runs of unvoiced frames (zeros and negative values) put between its values: about a third more frames '''
    rng = np.random.RandomState(seed)
    out = []
    for v in x:
        if rng.uniform() < 0.1:
            out.extend(rng.choice([0.0, -1.0, -0.25], size=rng.randint(1, 6)))
        out.append(v)
    out.extend([0.0] * rng.randint(0, 4))
    return np.asarray(out, dtype=np.float32)


def branch_cases():
    ''' [(name, ref, dut, remove_unvoiced)] over BRANCH_PAIRS: the flag off on the voiced curves, the flag on with unvoiced runs
        (values <= 0, negatives included) put into both '''
    cases = []
    for i, (nr, nd) in enumerate(BRANCH_PAIRS):
        ref, dut = voiced_pair(nr, nd, 100 + i)
        cases.append((f'{nr}x{nd}-all', ref, dut, False))
        cases.append((f'{nr}x{nd}-voiced', with_unvoiced(ref, 200 + i), with_unvoiced(dut, 300 + i), True))
    return cases


def limit_case():
    ref, dut = voiced_pair(MAX_LEN, MAX_LEN - 1, 7)
    return ('limit', ref, dut, True)


def golden_cases():
    ''' [(name, ref, dut, remove_unvoiced, pcc, resampled)] recorded from the reference (tools/gen_golden_pcc.py) '''
    z = np.load(GOLDEN)
    return [(f'golden{i}', z[f'ref{i}'], z[f'dut{i}'], bool(z['remove'][i]), float(z['pcc'][i]), z[f'resampled{i}'])
            for i in range(len(z['pcc']))]


def all_cases():
    return branch_cases() + [limit_case()] + [c[:4] for c in golden_cases()]
