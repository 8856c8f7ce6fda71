"""Integer oracle of the alignment kernels (`dx_active_span`, `dx_dtw_transfer`; csrc/align.hip) and of the marker writer's time rule
(daft_exprt/align.py), NumPy only, no project imports.  Written from the contract in include/daft_exprt_hip.h (K27), one
utterance at a time and serially: no scans, no tables, a dictionary for the first recording frame of every synthesis frame.

Also the hand-built cases shared by tests/test_align_host.py and tests/test_gpu_align.py.
"""
import numpy as np

MAX_LEN = 4096                       # dx_dtw_max_len()


def active_span(energy, n, rel_db=-40.0):
    ''' energy: float32 row, n frames of it live -> (begin, end).  The factor is 10^(rel_db / 20) in double, rounded once to
        float32; the threshold is one float32 product '''
    e = np.asarray(energy, dtype=np.float32)[:max(int(n), 0)]
    if len(e) == 0:
        return 0, 0
    peak = np.float32(np.fmax.reduce(e))
    if not peak > 0:
        return 0, 0
    thr = np.float32(peak * np.float32(10.0 ** (float(np.float32(rel_db)) / 20.0)))
    hit = np.nonzero(e >= thr)[0]
    return (int(hit[0]), int(hit[-1]) + 1) if len(hit) else (0, 0)


def dtw_transfer(path, n_ref, n_gen, durations, min_frames):
    ''' path: the entries (i, j) below path_len, any (out-of-range ones included); durations: the d_s of the s < n_symbols.
        Returns (rec_durations list as long as durations, moved, status) '''
    d = [int(x) for x in durations]
    zeros = [0] * len(d)
    first = {}
    for i, j in np.asarray(path, dtype=np.int64).reshape(-1, 2).tolist():
        if 0 <= i < n_ref and 0 <= j < n_gen:
            first[j] = min(first.get(j, i), i)
    sounding = [s for s, x in enumerate(d) if x > 0]
    starts = np.concatenate([[0], np.cumsum(d)]).tolist()
    K = len(sounding)
    if len(path) == 0 or K == 0 or any(x < 0 for x in d) or sum(d) != n_gen or any(starts[s] not in first for s in sounding):
        return zeros, 0, 2
    if n_ref < min_frames * K:
        return zeros, 0, 1
    raw = [first[starts[s]] for s in sounding]
    a = list(raw)
    for k in range(1, K):
        a[k] = max(a[k], a[k - 1] + min_frames)
    for k in range(K):
        a[k] = min(a[k], n_ref - min_frames * (K - k))
    out = list(zeros)
    for k, s in enumerate(sounding):
        out[s] = (a[k + 1] if k + 1 < K else n_ref) - a[k]
    return out, sum(x != y for x, y in zip(a, raw)), 0


def boundary_time(frame, begin_frame, n_samples, hop=256, sampling_rate=22050):
    ''' the string a boundary at `frame` of the crop that starts at begin_frame is written as '''
    return '%.6f' % (min(max((begin_frame + frame - 0.5) * hop, 0.0), float(n_samples)) / float(sampling_rate))


def duration_to_integer(spans, nb_samples, sampling_rate=22050, filter_length=1024, hop_length=256):
    ''' the reference's rule for the frames of marker spans (`extract_features.py:69-111`, centered) as
        oracle/daft_exprt_cpu.py `duration_to_integer` states it, with the sample count given -- `extract_features` passes the
        length of the cropped wav -- instead of derived from the spans.  spans: [[begin, end]] in seconds from the sentence
        begin.  IndexError / ValueError as there. '''
    nb_frames = 1 + int((nb_samples - filter_length) / hop_length)
    half = int(filter_length / 2)
    out, assigned, cursor = [], 0, 0
    while assigned + 1 <= nb_frames:
        if cursor >= len(spans):
            raise IndexError('pop from empty list')
        b, e = spans[cursor]
        cursor += 1
        if b == e:
            raise ValueError
        sb, se = int(b * sampling_rate), int(e * sampling_rate)
        n = sum(1 for i in range(nb_frames) if sb < half + hop_length * i <= se)
        out.append(n)
        assigned += n
    edge = int(filter_length / 2 / hop_length)
    out[0] += edge
    if cursor < len(spans):
        out.append(edge)
    else:
        out[-1] += edge
    return out


# ---- hand-built transfer cases: (name, path, n_ref, n_gen, durations, min_frames, want (rec_durations, moved, status)) ------------------

def _diagonal(n):
    return [(i, i) for i in range(n)]


def transfer_cases():
    cases = []
    # identity: the recording is the synthesis
    cases.append(('identity', _diagonal(9), 9, 9, [2, 3, 4], 1, ([2, 3, 4], 0, 0)))
    cases.append(('identity-min3', _diagonal(9), 9, 9, [2, 3, 4], 3, ([3, 3, 3], 2, 0)))
    # a vertical run swallows two symbols: recording frames 0..6 all sit on synthesis frame 0, symbols 1 and 2 start in the
    # recording's frame 7 and 8 -- with min_frames 2 the forward repair keeps pushing, then the end clamp pulls back
    vertical = [(i, 0) for i in range(7)] + [(7, 1), (8, 2), (9, 3)]
    cases.append(('vertical-run', vertical, 10, 4, [1, 1, 1, 1], 1, ([7, 1, 1, 1], 0, 0)))
    cases.append(('vertical-run-min2', vertical, 10, 4, [1, 1, 1, 1], 2, ([4, 2, 2, 2], 3, 0)))
    # a horizontal run: synthesis frames 3, 4, 5 share recording frame 3: the starts 3, 3, 3 are pushed apart forwards (3, 5, 7),
    # and the end clamp (4, 6, 8, 10) leaves them there
    horizontal = [(0, 0), (1, 1), (2, 2), (3, 3), (3, 4), (3, 5), (4, 6), (5, 7), (6, 8), (7, 9), (8, 9), (9, 9), (10, 9), (11, 9)]
    cases.append(('forward-repair', horizontal, 12, 10, [3, 1, 1, 5], 2, ([3, 2, 2, 5], 2, 0)))
    # a clamp at the end: the last symbol starts in the last frame and needs three
    late = _diagonal(5) + [(5, 4), (6, 4), (7, 5)]
    cases.append(('end-clamp', late, 8, 6, [5, 1], 3, ([5, 3], 1, 0)))
    cases.append(('too-short', _diagonal(5), 5, 5, [1, 1, 1, 2], 2, ([0, 0, 0, 0], 0, 1)))
    cases.append(('exactly-enough', _diagonal(8), 8, 8, [1, 1, 1, 5], 2, ([2, 2, 2, 2], 3, 0)))
    # zero-duration symbols interleaved: they get 0 frames and the others are indexed past them
    cases.append(('silent-interleaved', _diagonal(9), 9, 9, [0, 2, 0, 0, 3, 4, 0], 1, ([0, 2, 0, 0, 3, 4, 0], 0, 0)))
    cases.append(('silent-interleaved-min3', _diagonal(9), 9, 9, [0, 2, 0, 0, 3, 4, 0], 3, ([0, 3, 0, 0, 3, 3, 0], 2, 0)))
    cases.append(('empty-path', [], 4, 4, [2, 2], 1, ([0, 0], 0, 2)))
    cases.append(('all-silent', _diagonal(4), 4, 4, [0, 0], 1, ([0, 0], 0, 2)))
    cases.append(('sum-mismatch', _diagonal(4), 4, 4, [2, 1], 1, ([0, 0], 0, 2)))
    cases.append(('negative', _diagonal(4), 4, 4, [3, -1, 2], 1, ([0, 0, 0], 0, 2)))
    cases.append(('unvisited-frame', [(0, 0), (1, 1), (3, 3)], 4, 4, [2, 2], 1, ([0, 0], 0, 2)))
    # entries that are no cell of the pair are skipped: -1 padding inside path_len, and cells past the lengths
    cases.append(('padding-entries', [(-1, -1), (0, 0), (1, 1), (7, 1), (2, 2), (1, 9), (3, 3)], 4, 4, [1, 3], 1, ([1, 3], 0, 0)))
    return cases


def active_span_cases():
    ''' [(name, energy row float32, n, rel_db)]; every row is longer than n and holds large values behind it '''
    rng = np.random.RandomState(11)
    garbage = np.full(7, 1e6, dtype=np.float32)

    def row(values):
        return np.concatenate([np.asarray(values, dtype=np.float32), garbage])
    factor = np.float32(10.0 ** (-40.0 / 20.0))
    at_threshold = np.float32(np.float32(8.0) * factor)
    below = np.nextafter(at_threshold, np.float32(0))
    noise = (rng.uniform(size=300) * 1e-3).astype(np.float32)
    burst = noise.copy()
    burst[70:200] += rng.uniform(0.5, 2.0, size=130).astype(np.float32)
    return [('all-zero', row(np.zeros(9)), 9, -40.0), ('n=0', row([1.0, 2.0]), 0, -40.0), ('n=1', row([0.5]), 1, -40.0),
            ('n=1-zero', row([0.0]), 1, -40.0), ('negative-only', row([-1.0, -2.0]), 2, -40.0),
            ('peak-first', row([5.0, 1.0, 1e-4, 0.0, 0.0]), 5, -40.0), ('peak-last', row([0.0, 0.0, 1e-5, 0.2, 7.0]), 5, -40.0),
            ('at-threshold', row([below, at_threshold, 0.0, 8.0, at_threshold, below]), 6, -40.0),
            ('rel-db-0', row([1.0, 3.0, 3.0, 2.0]), 4, 0.0), ('rel-db-6', row([0.4, 0.6, 1.0, 0.5, 0.49]), 5, -6.0),
            ('burst-300', row(burst), 300, -40.0), ('burst-257', row(burst), 257, -40.0), ('burst-64', row(burst), 64, -40.0)]
