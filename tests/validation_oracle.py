"""numpy / float64 restatement of what `csrc/validation.hip` computes (shared by the host and the GPU tests).

`film_hist_oracle` is `numpy.histogram(bins=50)` per group of a FiLM tensor, `alignment_oracle` plain loops over the frames.
"""
import numpy as np

BINS = 50


def film_hist_oracle(film):
    ''' film (rows, nb_blocks, width) float32; group [block, 0 | 1] = the block's first | second half of the last axis
        (gammas | betas, `logger.py:118-125`).  Returns counts (nb_blocks, 2, 50) int64, edges (nb_blocks, 2, 51) float64,
        minmax (nb_blocks, 2, 2) float32, finite (nb_blocks, 2) bool.

        The values are handed to numpy.histogram as float64 (an exact widening): its edges are then numpy.linspace in double between
        the fp32 extremes, the table the device compares against.  (Handed float32 values, numpy builds its edges in a precision that
        differs between numpy 1 and numpy 2.)  A group with a NaN or an infinity -- numpy raises there -- has finite False, zero
        counts, minmax (0, 0) and the edges of a constant 0 group. '''
    film = np.asarray(film, dtype=np.float32)
    rows, nb, width = film.shape
    hw = width // 2
    counts = np.zeros((nb, 2, BINS), np.int64)
    edges = np.zeros((nb, 2, BINS + 1), np.float64)
    minmax = np.zeros((nb, 2, 2), np.float32)
    finite = np.zeros((nb, 2), bool)
    for blk in range(nb):
        for half in range(2):
            values = film[:, blk, half * hw: (half + 1) * hw].ravel()
            finite[blk, half] = np.isfinite(values).all()
            if finite[blk, half]:
                minmax[blk, half] = values.min(), values.max()
                counts[blk, half], edges[blk, half] = np.histogram(values.astype(np.float64), bins=BINS)
            else:
                edges[blk, half] = np.linspace(-0.5, 0.5, BINS + 1)
    return counts, edges, minmax, finite


def target_alignment_oracle(durations_int, in_length, out_length):
    ''' (L, out_length) 0 / 1: symbol l < in_length owns the next durations_int[l] frames, cut at out_length '''
    L = len(durations_int)
    target = np.zeros((L, int(out_length)), np.float64)
    col = 0
    for l in range(min(int(in_length), L)):
        d = max(int(durations_int[l]), 0)
        target[l, col: min(col + d, int(out_length))] = 1.
        col += d
    return target


def alignment_oracle(weights, durations_int, in_lengths, out_lengths):
    ''' weights (B, L, T) float32, durations_int (B, L), lengths (B,).  Returns (frames int64, hits int64, mass float64) per
        utterance: the owned frames, those whose argmax over l < in_length is the owner (numpy.argmax: lowest index among equal
        maxima), the mean of the owner's weight over the owned frames in double (0 without frames). '''
    weights = np.asarray(weights)
    B, L, T = weights.shape
    frames, hits, mass = np.zeros(B, np.int64), np.zeros(B, np.int64), np.zeros(B, np.float64)
    for b in range(B):
        n_in, n_out = min(int(in_lengths[b]), L), min(int(out_lengths[b]), T)
        target = target_alignment_oracle(durations_int[b], n_in, n_out)
        total = 0.
        for t in range(n_out):
            owners = np.nonzero(target[:, t])[0]
            if len(owners) == 0:
                continue
            assert len(owners) == 1
            frames[b] += 1
            hits[b] += int(np.argmax(weights[b, :n_in, t])) == owners[0]
            total += float(weights[b, owners[0], t])
        mass[b] = total / frames[b] if frames[b] else 0.
    return frames, hits, mass
