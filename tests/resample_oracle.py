"""Float64 NumPy restatement of the resampler of `librosa.load(path, sr=sr)` (librosa 0.8.1 `resample(res_type='kaiser_best')`
-> resampy 0.2.x), written from the description in daft_exprt/audio.py and NOT pinned to either library (neither is available
to the tests).  It walks every output sample straight from the filter table -- no polyphase bank -- so it checks the bank that
`daft_exprt.audio.resample_bank` builds for the device kernel independently."""
import numpy as np

NUM_ZEROS, PRECISION = 64, 9
ROLLOFF, KAISER_BETA = 0.9475937167399596, 14.769656459379492


def table():
    n_bits = 2 ** PRECISION
    n = n_bits * NUM_ZEROS
    u = np.linspace(0, NUM_ZEROS, n + 1)
    return ROLLOFF * np.sinc(ROLLOFF * u) * np.kaiser(2 * n + 1, KAISER_BETA)[n:], n_bits


def out_lengths(n_in, sr_in, sr_out):
    ''' (resampy's floor(n * ratio), librosa's ceil(n * ratio)) '''
    return n_in * sr_out // sr_in, -(-n_in * sr_out // sr_in)


def resample(x, sr_in, sr_out):
    ''' x (n,) -> (ceil(n * sr_out / sr_in),) float64; equal rates return x '''
    x = np.asarray(x, dtype=np.float64)
    if sr_in == sr_out:
        return x.copy()
    win, n_bits = table()
    win_delta = np.append(np.diff(win), 0.)
    ratio = sr_out / sr_in
    scale = min(1.0, ratio)
    step = int(scale * n_bits)
    nwin = len(win)
    n_in = len(x)
    n_floor, n_ceil = out_lengths(n_in, sr_in, sr_out)
    y = np.zeros(n_ceil)
    for t in range(n_floor):
        n = t * sr_in // sr_out
        f = (t * sr_in - n * sr_out) / sr_out
        acc = 0.
        for frac, count_sig, sign in ((scale * f, n + 1, -1), (scale - scale * f, n_in - n - 1, 1)):
            index = frac * n_bits
            offset = int(index)
            eta = index - offset
            count = min(count_sig, (nwin - offset) // step)
            pos = offset + np.arange(count) * step
            w = win[pos] + eta * win_delta[pos]
            src = n - np.arange(count) if sign < 0 else n + 1 + np.arange(count)
            acc += float(np.dot(w, x[src]))
        y[t] = acc * (scale if ratio < 1 else 1.)
    return y
