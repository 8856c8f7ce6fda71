"""Inputs, fp32 bounds and comparisons shared by tests/test_pitch_host.py and tests/test_gpu_pitch.py.

The fp32 bounds (u = 2^-24, the unit roundoff of fp32; W = window samples):
  * a correlation value is dot / (sqrt(e0 ek) + floor) with |dot| <= sqrt(e0 ek), the dot a W-term fp32 sum in tap order: its
    rounding error is at most W u sqrt(e0 ek), so the quotient is off by at most W u, plus a few u for the conversions of the
    two energies, the square root, the sum and the division: delta = (W + 8) u.
  * an interpolated candidate value v = rc - (rm - rp) d / 4, d = (rm - rp) / (2 (rm - 2 rc + rp)), |d| <= 1/2 at a local
    maximum.  With (rm - rp) / (rm - 2 rc + rp) = 2 d, the first-order change of v under changes of at most delta in rm, rc, rp
    is at most delta (1 + |d| + 4 d^2) <= 2.5 delta.  VALUE_BOUND = 3 delta leaves room for the roundings of the
    interpolation itself (a handful of u).
  * a path cost is a sum over the A analysis frames of a local cost (a candidate value times a factor <= 1: off by at most
    VALUE_BOUND) and a transition cost (logs of lags: a few u), accumulated on a running cost that is re-based to its minimum at
    every frame and therefore stays of order one (each addition rounds by a few u).  Two paths differ in cost by a quantity
    whose fp32 evaluation is off by at most the sum of these errors over both paths: PATH_BOUND = 2 A (VALUE_BOUND + 8 u).
"""
import os

import numpy as np

from tests import pitch_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pitch_reaper.npz')
U = 2.0 ** -24
FLIP_CAP = 0.01            # frames whose two best path costs are within PATH_BOUND may disagree: at most this share of an utterance's frames


def value_bound(geo):
    return 3.0 * (geo.window + 8) * U


def path_bound(geo, n_analysis):
    return 2.0 * n_analysis * (value_bound(geo) + 8 * U)


class Fixture:
    def __init__(self):
        z = np.load(GOLDEN)
        self.names = [str(n) for n in z['names']]
        self.hop, self.f0_interval, self.min_f0, self.max_f0, self.uv_cost = (float(v) for v in z['hparams'])
        self.hop = int(self.hop)
        self.x = [z[f'x{i}'] for i in range(len(self.names))]                  # int16
        self.sr = [int(z[f'sr{i}']) for i in range(len(self.names))]
        self.hz = [z[f'hz{i}'].astype(np.float64) for i in range(len(self.names))]
        self.err = [tuple(int(v) for v in z[f'err{i}']) for i in range(len(self.names))]
        self.pooled = tuple(int(v) for v in z['pooled'])
        self.n_pooled = len(z['pooled_names'])

    def wav(self, i):
        return self.x[i].astype(np.float32) / np.float32(32768.0)

    def index_at(self, sr):
        return self.sr.index(sr)

    def track(self, x, sr, dtype=np.float64):
        return O.track(x, sr, self.hop, self.f0_interval, self.min_f0, self.max_f0, self.uv_cost, dtype=dtype)

    def geometry(self, sr):
        return O.Geometry(sr, self.f0_interval, self.min_f0, self.max_f0)


def harmonic_tone(f0, sr, seconds, top=4000.0):
    ''' sum of the harmonics of f0 (an array of instantaneous Hz, or one value) up to `top` Hz with amplitudes 1 / h, peak 0.5 '''
    n = int(round(seconds * sr))
    f = np.broadcast_to(np.asarray(f0, dtype=np.float64), (n,))
    phase = 2 * np.pi * np.cumsum(f) / sr
    y = np.zeros(n)
    for h in range(1, int(top // f.min()) + 1):
        y += np.where(h * f <= top, np.sin(h * phase) / h, 0.0)
    return (0.5 * y / np.abs(y).max()).astype(np.float32)


def ragged_batch(fix, sr):
    ''' the four utterances of the GPU tests at `sr`: a fixture recording, a 440 Hz tone of exactly hop * 40 samples, 0.02 s of
        noise (shorter than window + longest lag: every frame reads padding), 1 s of silence '''
    rng = np.random.RandomState(1234)
    tone = harmonic_tone(440.0, sr, fix.hop * 40 / sr)
    assert tone.shape[0] == fix.hop * 40
    noise = (0.1 * rng.standard_normal(int(round(0.02 * sr)))).astype(np.float32)
    assert noise.shape[0] < fix.geometry(sr).span
    return [fix.wav(fix.index_at(sr)), tone, noise, np.zeros(sr, dtype=np.float32)]


def compare_candidates(lags, vals, ref_lags, ref_vals, bound):
    ''' problems (strings) found comparing candidates (A, K) with the oracle's: every oracle candidate that is clear of the
        PEAK_MIN threshold and of the K-th place by more than `bound` has a counterpart (interpolated lag within 1.5) whose value
        is within `bound`, and the other way round; a counterpart in another slot is only allowed across values within 2 * bound '''
    problems = []
    A, K = ref_lags.shape
    for name, (la, va, lb, vb) in (('oracle', (ref_lags, ref_vals, lags, vals)), ('kernel', (lags, vals, ref_lags, ref_vals))):
        for a in range(A):
            na, nb = int((la[a] > 0).sum()), int((lb[a] > 0).sum())
            cut = max(vb[a, K - 1] if nb == K else 0.0, va[a, K - 1] if na == K else 0.0)      # value of the last place taken
            for i in range(na):
                v = float(va[a, i])
                if v <= O.PEAK_MIN + bound or (cut > 0 and v <= cut + bound):
                    continue
                near = np.nonzero((lb[a] > 0) & (np.abs(lb[a] - la[a, i]) < 1.5))[0]
                if near.size == 0:
                    problems.append(f'frame {a}: {name} candidate lag {la[a, i]:.3f} value {v:.6f} has no counterpart')
                    continue
                j = int(near[np.argmin(np.abs(vb[a, near] - v))])
                if abs(float(vb[a, j]) - v) > bound:
                    problems.append(f'frame {a}: {name} candidate lag {la[a, i]:.3f} value {v:.6f} vs {float(vb[a, j]):.6f}')
                elif j != i:
                    lo, hi = min(i, j), max(i, j)
                    if np.abs(va[a, lo:hi + 1] - v).max() > 2 * bound:
                        problems.append(f'frame {a}: {name} candidate lag {la[a, i]:.3f} in slot {i} vs {j} across distinct values')
    return problems


def compare_tracks(hz, ref, bound):
    ''' hz (A,) per analysis frame against the oracle's result `ref` (O.track): (frames that disagree although the oracle's two
        best path costs differ by more than `bound`, frames that disagree where they do not, frames).  Agreement: the same voicing
        decision and voiced Hz within 1e-3 relative. '''
    hz, ref_hz = np.asarray(hz, np.float64), np.asarray(ref['hz_a'], np.float64)
    assert hz.shape == ref_hz.shape, (hz.shape, ref_hz.shape)
    agree = (hz > 0) == (ref_hz > 0)
    both = (hz > 0) & (ref_hz > 0)
    agree[both] &= np.abs(hz[both] / ref_hz[both] - 1.0) <= 1e-3
    exempt = np.asarray(ref['gap']) <= bound
    return int(np.sum(~agree & ~exempt)), int(np.sum(~agree & exempt)), int(hz.size)
