"""float64 oracle of the copy-synthesis scores (`dx_mel_cepstrum`, `dx_dtw_align`, `dx_dtw_path_scores`; daft_exprt/evaluate.py),
NumPy only, no project imports.

  * `dct_table`, `mel_cepstrum`: coefficients 1..K of the orthonormal DCT-II over the mel axis (c0 dropped), time-major.
  * `dtw`: the unconstrained DTW with local cost d(i, j) = ||ref[i] - gen[j]||_2, D(i, j) = d + min(D(i-1, j-1), D(i-1, j), D(i, j-1)),
    walked by anti-diagonals (one vector operation per diagonal); the predecessor of a cell is the FIRST minimum in the order
    diagonal, (i-1, j), (i, j-1) -- a later candidate replaces an earlier one only when strictly smaller -- and `backtrack` follows
    the recorded codes from the last cell.  tests/test_dtw_host.py pins this function against an enumeration of all monotone paths.
  * `path_scores`: MCD in dB, F0 RMSE in cents, voicing error, doubly voiced pairs and the length of a path.
  * `path_cost64`: the float64 cost of any given path -- what a float32 path that resolved a near-tie the other way is judged by.
  * the float32 restatement of the kernels' arithmetic: `dtw(..., dtype=np.float32)` (the squared differences summed in order of
    k, a float32 square root, D = d + min in float32; NumPy has no fused multiply-add, the kernel uses one per term),
    `mel_cepstrum_f32` (the table rounded once, the sum in order of m in float32) and `path_scores_f32` (float32 d along the path,
    sums in double, results rounded to float32 as the kernel's outputs are).
  * the test cases shared by tests/test_dtw_host.py and tests/test_gpu_dtw.py, and F32_TOTAL_ERR / F32_MCD_ERR / F32_CEP_ERR /
    F32_F0_ERR: the worst deviation of the float32 restatement from float64 over those cases, measured on the host
    (tests/test_dtw_host.py prints and asserts them).  The GPU tests allow TOL_FACTOR = 10 times that, the convention of
    tests/curve_oracle.py: the GPU's fused multiply-adds and its sum order differ from NumPy's by a few ulp per term.
"""
import numpy as np

# measured by tests/test_dtw_host.py::test_float32_restatement_stays_within_the_recorded_errors, rounded up
F32_TOTAL_ERR = 5.0e-7              # relative, on D(n_ref-1, n_gen-1): measured 4.98e-7 (33 x 1000: 1032 float32 additions to 2580)
F32_MCD_ERR = 4.1e-8                # relative, on mcd_db: measured 4.02e-8 (the float32 rounding of the result; half an ulp is 6e-8)
F32_CEP_ERR = 9.3e-6                # absolute, on a cepstral coefficient of a natural-log mel: measured 9.22e-6 (80 terms of size 5)
F32_F0_ERR = 3.2e-8                 # relative, on f0_rmse_cents: measured 3.18e-8 (double sums; the float32 rounding of the result)
TOL_FACTOR = 10.0
MAX_LEN = 4096                       # dx_dtw_max_len()
MCD_SCALE = 10.0 * np.sqrt(2.0) / np.log(10.0)
CENTS = 1200.0 / np.log(2.0)

EXACT_LENGTHS = [(1, 1), (1, 9), (9, 1), (2, 2), (63, 65), (255, 257), (256, 256), (257, 64), (300, 77), (5, 4096), (4096, 5)]
REAL_LENGTHS = [(700, 650), (257, 300), (33, 1000)]
CEP_SHAPES = [(80, 13), (8, 7)]      # (n_mel, K)


def dct_table(n_mel, n_coeffs):
    ''' (K, n_mel) float64: rows 1..K of the orthonormal DCT-II '''
    assert 1 <= n_coeffs < n_mel
    k = np.arange(1, n_coeffs + 1, dtype=np.float64)[:, None]
    m = np.arange(n_mel, dtype=np.float64)[None, :]
    return np.sqrt(2.0 / n_mel) * np.cos(np.pi * (m + 0.5) * k / n_mel)


def mel_cepstrum(mel, n_coeffs=13):
    ''' mel (n_mel, T) -> (T, K) float64 '''
    mel = np.asarray(mel, dtype=np.float64)
    return (dct_table(mel.shape[0], n_coeffs) @ mel).T


def mel_cepstrum_f32(mel, n_coeffs=13):
    ''' the kernel's arithmetic: the table rounded once to float32, one float32 multiply and add per mel channel, in order '''
    mel = np.asarray(mel, dtype=np.float32)
    table = dct_table(mel.shape[0], n_coeffs).astype(np.float32)
    acc = np.zeros((mel.shape[1], n_coeffs), dtype=np.float32)
    for m in range(mel.shape[0]):
        acc = acc + mel[m][:, None] * table[:, m][None, :]
    return acc


def _dist(r, g, dtype):
    ''' ||r - g||_2 per row, the terms summed in order of k in `dtype` '''
    acc = np.zeros(r.shape[0], dtype=dtype)
    for k in range(r.shape[1]):
        t = r[:, k] - g[:, k]
        acc = acc + t * t
    return np.sqrt(acc)


def dtw(ref, gen, dtype=np.float64):
    ''' ref (n_ref, K), gen (n_gen, K) -> (total, path (L, 2) int64 from (0, 0) to (n_ref-1, n_gen-1)) in `dtype` arithmetic;
        (nan, empty path) when a sequence is empty '''
    ref, gen = np.asarray(ref, dtype=dtype), np.asarray(gen, dtype=dtype)
    nr, nd = ref.shape[0], gen.shape[0]
    if nr == 0 or nd == 0:
        return float('nan'), np.zeros((0, 2), dtype=np.int64)
    inf = dtype(np.inf)
    codes = np.zeros((nr, nd), dtype=np.uint8)                  # 0 diagonal, 1 (i-1, j), 2 (i, j-1)
    prev1, prev2 = np.full(nr, inf, dtype=dtype), np.full(nr, inf, dtype=dtype)      # diagonals s-1, s-2 by i
    for s in range(nr + nd - 1):
        i = np.arange(max(0, s - (nd - 1)), min(s, nr - 1) + 1)
        j = s - i
        d = _dist(ref[i], gen[j], dtype)
        diag = np.where((i > 0) & (j > 0), prev2[np.maximum(i - 1, 0)], inf)
        up = np.where(i > 0, prev1[np.maximum(i - 1, 0)], inf)
        left = np.where(j > 0, prev1[i], inf)
        best, code = diag.copy(), np.zeros(len(i), dtype=np.uint8)
        take = up < best
        best[take], code[take] = up[take], 1
        take = left < best
        best[take], code[take] = left[take], 2
        if s == 0:
            best[:] = 0
        cur = np.full(nr, inf, dtype=dtype)
        cur[i] = d + best
        codes[i, j] = code
        prev2, prev1 = prev1, cur
    return prev1[nr - 1], backtrack(codes)


def backtrack(codes):
    i, j = codes.shape[0] - 1, codes.shape[1] - 1
    cells = [(i, j)]
    while i > 0 or j > 0:
        c = 2 if i == 0 else 1 if j == 0 else int(codes[i, j])
        if c == 1:
            i -= 1
        elif c == 2:
            j -= 1
        else:
            i, j = i - 1, j - 1
        cells.append((i, j))
    return np.asarray(cells[::-1], dtype=np.int64)


def path_cost64(path, ref, gen):
    ''' the float64 sum of d(i, j) over the cells of `path` '''
    path = np.asarray(path, dtype=np.int64)
    ref, gen = np.asarray(ref, dtype=np.float64), np.asarray(gen, dtype=np.float64)
    return float(np.sum(np.sqrt(np.sum((ref[path[:, 0]] - gen[path[:, 1]]) ** 2, axis=1))))


def is_valid_path(path, n_ref, n_gen):
    path = np.asarray(path, dtype=np.int64)
    if not (max(n_ref, n_gen) <= len(path) <= n_ref + n_gen - 1):
        return False
    if tuple(path[0]) != (0, 0) or tuple(path[-1]) != (n_ref - 1, n_gen - 1):
        return False
    steps = {tuple(s) for s in np.diff(path, axis=0)}
    return steps <= {(1, 1), (1, 0), (0, 1)}


def path_scores(path, ref, gen, lp_ref=None, lp_gen=None, dtype=np.float64):
    ''' {'mcd_db', 'f0_rmse_cents', 'vuv_error', 'voiced_pairs', 'path_len'} of a path; d in `dtype`, the sums in float64 '''
    path = np.asarray(path, dtype=np.int64).reshape(-1, 2)
    n = len(path)
    nan = float('nan')
    out = {'mcd_db': nan, 'f0_rmse_cents': nan, 'vuv_error': nan, 'voiced_pairs': 0, 'path_len': n}
    if n == 0:
        return out
    ref, gen = np.asarray(ref, dtype=dtype), np.asarray(gen, dtype=dtype)
    d = _dist(ref[path[:, 0]], gen[path[:, 1]], dtype).astype(np.float64)
    out['mcd_db'] = float(MCD_SCALE * (np.sum(d) / n))
    if lp_ref is None or lp_gen is None:
        return out
    a = np.asarray(lp_ref, dtype=np.float32).astype(np.float64)[path[:, 0]]
    g = np.asarray(lp_gen, dtype=np.float32).astype(np.float64)[path[:, 1]]
    both, one = (a > 0) & (g > 0), (a > 0) != (g > 0)
    out['voiced_pairs'] = int(both.sum())
    out['vuv_error'] = float(one.sum() / n)
    if both.any():
        out['f0_rmse_cents'] = float(np.sqrt(np.mean((CENTS * (a[both] - g[both])) ** 2)))
    return out


def path_scores_f32(path, ref, gen, lp_ref=None, lp_gen=None):
    ''' the kernel's arithmetic: float32 d, double sums, float32 results '''
    out = path_scores(path, ref, gen, lp_ref, lp_gen, dtype=np.float32)
    for key in ('mcd_db', 'f0_rmse_cents', 'vuv_error'):
        out[key] = float(np.float32(out[key]))
    return out


# ---- test cases ---------------------------------------------------------------------------------------------------------------

def exact_pair(n_ref, n_gen, seed):
    ''' K = 1, integer cepstra in 0..7: every d and every D is an integer below 2^24, exact in float32; ties are everywhere '''
    rng = np.random.RandomState(seed)
    return (rng.randint(0, 8, size=(n_ref, 1)).astype(np.float32), rng.randint(0, 8, size=(n_gen, 1)).astype(np.float32))


def exact_cases():
    return [(f'{a}x{b}',) + exact_pair(a, b, 1000 + n) for n, (a, b) in enumerate(EXACT_LENGTHS)]


def limit_case():
    return (f'{MAX_LEN}x{MAX_LEN}',) + exact_pair(MAX_LEN, MAX_LEN, 77)


def _trajectory(n, n_coeffs, rng, warp):
    ''' (n, K) cepstrum-like: a smooth trajectory sampled at warped times plus frame noise; coefficient k has a scale of about
        6 / (k + 1)^0.7 -- c1 of a natural-log mel of speech swings by several units, c13 by one '''
    t = np.linspace(0.0, 1.0, n) ** warp
    out = np.zeros((n, n_coeffs))
    for k in range(n_coeffs):
        scale = 6.0 / (k + 1.0) ** 0.7
        out[:, k] = scale * sum(np.sin(2 * np.pi * f * t + p) / np.sqrt(4.0) for f, p in zip(rng[0][k], rng[1][k]))
    return out


def real_pair(n_ref, n_gen, seed, n_coeffs=13):
    ''' two float32 cepstra of the same underlying trajectory, the second one time-warped and perturbed '''
    rs = np.random.RandomState(seed)
    shared = (rs.uniform(0.5, 12.0, size=(n_coeffs, 4)), rs.uniform(0, 2 * np.pi, size=(n_coeffs, 4)))
    ref = _trajectory(n_ref, n_coeffs, shared, 1.0) + 0.3 * rs.standard_normal((n_ref, n_coeffs))
    gen = _trajectory(n_gen, n_coeffs, shared, 1.3) + 0.3 * rs.standard_normal((n_gen, n_coeffs))
    return ref.astype(np.float32), gen.astype(np.float32)


def real_cases():
    return [(f'{a}x{b}',) + real_pair(a, b, 2000 + n) for n, (a, b) in enumerate(REAL_LENGTHS)]


def mel_case(n_mel, n_frames, seed):
    ''' a natural-log mel like the data loader's: clip(N(-5, 2), ln 1e-5, 2) with a spectral tilt '''
    rng = np.random.RandomState(seed)
    tilt = np.linspace(1.5, -1.5, n_mel)[:, None]
    return np.clip(rng.standard_normal((n_mel, n_frames)) * 2.0 - 5.0 + tilt, np.log(1e-5), 2.0).astype(np.float32)


def pitch_pair(n_ref, n_gen, seed, voiced='mixed'):
    ''' two raw log-Hz curves (0 where unvoiced).  'mixed': about 30 % unvoiced runs on each side; 'all': fully voiced;
        'disjoint': the reference voiced, the other side unvoiced throughout (no doubly voiced frame) '''
    rng = np.random.RandomState(seed)

    def curve(n):
        x = 5.0 + 0.3 * np.sin(2 * np.pi * rng.uniform(0.5, 3.0) * np.arange(n) / n + rng.uniform(0, 6)) + 0.02 * rng.standard_normal(n)
        if voiced == 'mixed':
            run = np.repeat(rng.uniform(size=n // 8 + 1) < 0.3, 8)[:n]
            x[run] = 0.0
        return x.astype(np.float32)
    a, g = curve(n_ref), curve(n_gen)
    if voiced == 'disjoint':
        g[:] = 0.0
    return a, g


def score_cases():
    ''' [(name, ref, gen, lp_ref, lp_gen)]: what `dx_dtw_path_scores` is run on, along the oracle's own path '''
    out = []
    for n, (kind, (a, b)) in enumerate((('mixed', (257, 300)), ('all', (120, 95)), ('disjoint', (64, 70)), ('mixed', (700, 650)))):
        ref, gen = real_pair(a, b, 3000 + n)
        lp_ref, lp_gen = pitch_pair(a, b, 4000 + n, kind)
        out.append((f'{kind}-{a}x{b}', ref, gen, lp_ref, lp_gen))
    return out


def rel(a, b):
    return abs(a - b) / abs(b)
