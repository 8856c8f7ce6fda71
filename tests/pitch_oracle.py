"""Oracle of the pitch tracker (csrc/pitch.hip): the same algorithm in NumPy, float64 by default.  This file is
the definition of the arithmetic; the kernels restate it in fp32.

Two stages, separately callable:
  candidates(): per analysis frame, the normalised cross-correlation of a fixed window against itself lagged, and its up
                to K best local maxima (parabolically interpolated lag and value, in order of value);
  viterbi():    the cheapest path over K voiced candidates plus one unvoiced state per frame.
track() chains them and gathers the analysis frames to mel frames (log Hz, 0 where unvoiced).
"""
import math

import numpy as np

K = 16                  # candidates kept per frame: every multiple of the shortest period fits (lag_max / lag_min = 12.5 by default)
WINDOW_S = 0.015        # correlation window, seconds
PEAK_MIN = 0.3          # a local maximum below this is no candidate
FLOOR_REL = 1e-2        # energy floor of the normaliser, relative to the utterance's mean square
FLOOR_ABS = 1e-10       # keeps the normaliser positive on digital silence
LAG_WEIGHT = 0.3        # a candidate at the longest lag is worth (1 - LAG_WEIGHT) of its value: against octave-down errors
UV_BASE = 0.5           # local cost of the unvoiced state is uv_cost * UV_BASE
FREQ_WEIGHT = 1.0       # cost of |log(f_j / f_i)| between voiced states
OCTAVE_COST = 0.35      # an octave jump costs OCTAVE_COST + its distance from the exact octave instead, where that is cheaper
VOICING_COST = 0.4      # cost of a voiced <-> unvoiced change
NO_STATE = 1e30         # cost of a candidate slot that holds no candidate


class Geometry:
    ''' integer sizes of the analysis at one sampling rate '''

    def __init__(self, sr, f0_interval, min_f0, max_f0):
        self.sr = int(sr)
        self.step = float(self.sr) * float(f0_interval)             # samples per analysis frame (not an integer at 22 050 Hz)
        self.window = int(round(WINDOW_S * self.sr))
        self.lag_min = int(math.floor(self.sr / float(max_f0)))
        self.lag_max = int(math.ceil(self.sr / float(min_f0)))
        assert 2 <= self.lag_min < self.lag_max
        self.lag_lo, self.lag_hi = self.lag_min - 1, self.lag_max + 1   # the correlation also covers both neighbours
        self.n_lags = self.lag_hi - self.lag_lo + 1
        self.span = self.window + self.lag_hi                        # samples one frame reads

    def n_analysis(self, n):
        return 1 + int(math.floor(int(n) / self.step))

    def centre(self, a):
        return int(math.floor(a * self.step + 0.5))


def n_mel_frames(n, hop):
    ''' frames of the centred mel front-end, and of `pitch[::hop]` plus the `len % hop == 0` append '''
    return 1 + int(n) // int(hop)


def mel_to_analysis(t, hop, geo, n_analysis):
    return min(int(math.floor(t * int(hop) / geo.step + 0.5)), n_analysis - 1)


def nccf(x, geo, dtype=np.float64):
    ''' (A, n_lags) normalised cross-correlation of x (n,) at lags lag_lo .. lag_hi; samples outside [0, n) read as zero '''
    x = np.asarray(x)
    n = x.shape[0]
    A = geo.n_analysis(n)
    half = geo.window // 2
    mean_sq = float(np.mean(np.asarray(x, np.float64) ** 2)) if n else 0.0
    floor = dtype(geo.window * (FLOOR_REL * mean_sq + FLOOR_ABS))
    pad_l = half                                                      # the last centre is at most n + 1
    xp = np.concatenate([np.zeros(pad_l), np.asarray(x, np.float64), np.zeros(geo.span + 2)])
    sq = np.concatenate([[0.0], np.cumsum(xp * xp)])                 # energies from a running sum, in float64 in every variant
    out = np.zeros((A, geo.n_lags), dtype=dtype)
    xw = xp.astype(dtype)
    lags = np.arange(geo.lag_lo, geo.lag_hi + 1)
    for a in range(A):
        s0 = geo.centre(a) - half + pad_l
        seg = xw[s0:s0 + geo.span]
        dot = np.correlate(seg, seg[:geo.window], mode='valid')[geo.lag_lo:geo.lag_hi + 1]
        e0 = dtype(sq[s0 + geo.window] - sq[s0])
        ek = (sq[s0 + lags + geo.window] - sq[s0 + lags]).astype(dtype)
        out[a] = dot / (np.sqrt(e0 * ek) + floor)
    return out


def pick_peaks(r, geo):
    ''' r (A, n_lags) -> (lags (A, K), values (A, K)) in r's dtype: the up to K largest local maxima above PEAK_MIN at lags
        lag_min .. lag_max, interpolated through their neighbours, in order of value (then of lag); empty slots are 0 '''
    A = r.shape[0]
    dt = r.dtype.type
    lag_out = np.zeros((A, K), dtype=r.dtype)
    val_out = np.zeros((A, K), dtype=r.dtype)
    c, m, p = r[:, 1:-1], r[:, :-2], r[:, 2:]
    is_peak = (c > m) & (c >= p) & (c > dt(PEAK_MIN))
    for a in range(A):
        idx = np.nonzero(is_peak[a])[0]
        if idx.size == 0:
            continue
        rc, rm, rp = c[a, idx], m[a, idx], p[a, idx]
        d = dt(0.5) * (rm - rp) / (rm - dt(2) * rc + rp)
        val = rc - dt(0.25) * (rm - rp) * d
        lag = (idx + geo.lag_min).astype(r.dtype) + d
        order = np.lexsort((lag, -val))[:K]
        lag_out[a, :order.size] = lag[order]
        val_out[a, :order.size] = val[order]
    return lag_out, val_out


def candidates(x, geo, dtype=np.float64):
    return pick_peaks(nccf(x, geo, dtype), geo)


def _local_costs(lags, vals, geo, uv_cost):
    dt = lags.dtype.type
    live = lags > 0
    voiced = dt(1) - vals * (dt(1) - dt(LAG_WEIGHT) * lags / dt(geo.lag_max))
    voiced = np.where(live, voiced, dt(NO_STATE))
    unvoiced = np.full((lags.shape[0], 1), dt(uv_cost) * dt(UV_BASE), dtype=lags.dtype)
    return np.concatenate([voiced, unvoiced], axis=1), live


def _transition(lp, lq):
    ''' cost (K + 1, K + 1) of going from the states of one frame (rows; log lags lp (K,), nan where empty) to the next '''
    dt = lp.dtype.type
    d = np.abs(lq[None, :] - lp[:, None])
    d = np.minimum(d, dt(OCTAVE_COST) + np.abs(d - dt(math.log(2.0))))
    T = np.full((K + 1, K + 1), dt(VOICING_COST), dtype=lp.dtype)
    T[:K, :K] = dt(FREQ_WEIGHT) * d
    T[K, K] = dt(0)
    return T


def viterbi(lags, vals, geo, uv_cost):
    ''' lags, vals (A, K) from candidates().  Returns (state (A,) int: candidate index or K for unvoiced, hz (A,): 0 where
        unvoiced, gap (A,): how much dearer the best path through any other state of that frame is than the best path).
        The running cost is re-based on its minimum at every frame, so that it stays of order one. '''
    A = lags.shape[0]
    dt = lags.dtype.type
    local, live = _local_costs(lags, vals, geo, uv_cost)
    loglag = np.where(live, np.log(np.where(live, lags, dt(1))), dt(0))
    fwd = np.zeros((A, K + 1), dtype=lags.dtype)
    back = np.zeros((A, K + 1), dtype=np.int64)
    trans = [None] * A
    fwd[0] = local[0] - local[0].min()
    for a in range(1, A):
        T = _transition(loglag[a - 1], loglag[a])
        trans[a] = T
        tot = fwd[a - 1][:, None] + T
        back[a] = np.argmin(tot, axis=0)                             # first of equals: the lower state index
        cost = tot[back[a], np.arange(K + 1)] + local[a]
        cost = np.where(local[a] >= dt(NO_STATE), dt(NO_STATE), cost)
        fwd[a] = cost - cost.min()
    state = np.zeros(A, dtype=np.int64)
    state[A - 1] = int(np.argmin(fwd[A - 1]))
    for a in range(A - 1, 0, -1):
        state[a - 1] = back[a, state[a]]
    # min-marginals: cheapest continuation from each state, for the gap
    bwd = np.zeros((A, K + 1), dtype=lags.dtype)
    for a in range(A - 2, -1, -1):
        nxt = np.minimum(bwd[a + 1] + local[a + 1], dt(NO_STATE))
        c = np.min(trans[a + 1] + nxt[None, :], axis=1)
        bwd[a] = c - c.min()
    marg = np.minimum(fwd + bwd, dt(NO_STATE))
    srt = np.sort(marg, axis=1)
    gap = srt[:, 1] - srt[:, 0]
    sel = np.take_along_axis(np.concatenate([lags, np.zeros((A, 1), lags.dtype)], axis=1), state[:, None], axis=1)[:, 0]
    hz = np.where(state < K, dt(geo.sr) / np.where(sel > 0, sel, dt(1)), dt(0))
    return state, hz, gap


def track(x, sr, hop, f0_interval, min_f0, max_f0, uv_cost, dtype=np.float64):
    ''' x (n,) samples in [-1, 1] -> dict: per mel frame `log_pitch` (log Hz, 0 unvoiced) and `hz`, per analysis frame `hz_a`,
        `gap`, `state`, and the candidates '''
    geo = Geometry(sr, f0_interval, min_f0, max_f0)
    lags, vals = candidates(x, geo, dtype)
    state, hz_a, gap = viterbi(lags, vals, geo, uv_cost)
    A = lags.shape[0]
    T = n_mel_frames(len(x), hop)
    idx = np.array([mel_to_analysis(t, hop, geo, A) for t in range(T)], dtype=np.int64)
    hz = hz_a[idx]
    log_pitch = np.where(hz > 0, np.log(np.where(hz > 0, hz, 1)), 0)
    return dict(log_pitch=log_pitch, hz=hz, hz_a=hz_a, gap=gap, state=state, lags=lags, vals=vals, mel_to_analysis=idx, geo=geo)


def errors(hz, hz_ref):
    ''' (voicing decisions that differ, frames, gross errors (> 20 % off), frames both call voiced) '''
    hz, hz_ref = np.asarray(hz, np.float64), np.asarray(hz_ref, np.float64)
    assert hz.shape == hz_ref.shape
    v, vr = hz > 0, hz_ref > 0
    both = v & vr
    gross = int(np.sum(np.abs(hz[both] / hz_ref[both] - 1.0) > 0.2))
    return int(np.sum(v != vr)), int(hz.size), gross, int(both.sum())
