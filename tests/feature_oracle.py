"""Oracle of the feature-extraction kernels (csrc/features.hip): the arithmetic they are held to, in Python
integers and float64 NumPy.  tests/test_features_host.py pins it to results recorded from the reference
(tests/golden/features_kat.json); tests/test_gpu_features.py holds the kernels to it.
"""
import math

import numpy as np

OK, INDEX_ERROR, VALUE_ERROR, ASSERT = 0, 1, 2, 3


def mel_frames(n_samples, filter_length, hop_length, centered):
    ''' frames of the mel-spectrogram of n_samples samples '''
    if centered:
        return 1 + n_samples // hop_length
    return 1 + (n_samples - filter_length) // hop_length if n_samples >= filter_length else 0


def span_frames(begin, end, sampling_rate, filter_length, hop_length, nb_frames):
    ''' how many frame centres filter_length / 2 + hop_length * i, 0 <= i < nb_frames, lie in (int(begin * sr), int(end * sr)] '''
    half = int(filter_length / 2)
    first = max(0, -((half - int(begin * sampling_rate) - 1) // hop_length))       # ceil((sb + 1 - half) / hop)
    last = min(nb_frames - 1, (int(end * sampling_rate) - half) // hop_length)
    return max(0, last - first + 1)


def marker_durations(spans, n_samples, sampling_rate, filter_length, hop_length, centered):
    ''' spans [(begin, end)] in seconds from the sentence begin -> (integer frame durations, status).  Frames go to the rows in
        order until every one of the 1 + int((n_samples - filter_length) / hop_length) uncentred frames has an owner; the frames
        that centring adds go to the first row and to the row after the last owner (to the last owner when it is the last row).
        status: INDEX_ERROR when the rows run out first (or there is no frame), VALUE_ERROR when a row of zero length is reached,
        ASSERT when the list is not one per row, does not add up to the mel's frame count or holds a 0.  The list is empty on
        INDEX_ERROR / VALUE_ERROR. '''
    nb_frames = 1 + int((n_samples - filter_length) / hop_length)
    out, assigned = [], 0
    for begin, end in spans:
        if assigned >= nb_frames:
            break
        if begin == end:
            return [], VALUE_ERROR
        out.append(span_frames(begin, end, sampling_rate, filter_length, hop_length, nb_frames))
        assigned += out[-1]
    if assigned < nb_frames:
        return [], INDEX_ERROR
    if centered:
        if not out:
            return [], INDEX_ERROR
        edge = int(filter_length / 2 / hop_length)
        out[0] += edge
        if len(out) < len(spans):
            out.append(edge)
        else:
            out[-1] += edge
    good = len(out) == len(spans) and sum(out) == mel_frames(n_samples, filter_length, hop_length, centered) and 0 not in out
    return out, OK if good else ASSERT


def symbol_pool(energy, log_pitch, durations):
    ''' (mean energy, mean of the pitch values > 0 or 0) per row over the row's own frames, float64; rows of duration 0 give 0
        and own no frame '''
    energy, log_pitch = np.asarray(energy, dtype=np.float64), np.asarray(log_pitch, dtype=np.float64)
    sym_energy, sym_pitch, frame = np.zeros(len(durations)), np.zeros(len(durations)), 0
    for row, d in enumerate(int(d) for d in durations):
        if d == 0:
            continue
        sym_energy[row] = math.fsum(energy[frame: frame + d]) / d
        voiced = log_pitch[frame: frame + d]
        voiced = voiced[voiced > 0.]
        if len(voiced):
            sym_pitch[row] = math.fsum(voiced) / len(voiced)
        frame += d
    return sym_energy, sym_pitch


def pool_for_markers(values, markers, pitch):
    ''' the oracle pooling over the rows of a features .markers file (int_dur in column 2) '''
    durations = [int(marker[2]) for marker in markers]
    return symbol_pool(values, values, durations)[1 if pitch else 0]
