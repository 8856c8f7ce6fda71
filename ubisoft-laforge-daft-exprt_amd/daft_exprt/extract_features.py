"""Mel-spectrogram / frame-energy front-end of the synthesis path on the GPU (reference: `extract_features.py:299-304,
330-359`; callers `generate.py:455-457`, `extract_features.py:429, 465-466`, `fine_tune.py:102`).

`mel_spectrogram_HiFi(wav, hparams)` and `extract_energy(mel_spec)` keep the reference's signatures (NumPy in, NumPy
out, one utterance); `mel_spectrogram_batch` is the batched device entry.  `extract_pitch(wav, fs, hparams)` keeps the
signature of `extract_features.py:222-269` and `pitch_batch` is its batched device entry, but the tracker behind them is this
project's own (csrc/pitch.hip), not the REAPER binary the reference runs.  The mel filterbank is built here from the
published Slaney formula (what `librosa.filters.mel(sr, n_fft, n_mels, fmin, fmax)` computes with its defaults
htk=False, norm='slaney'); librosa itself is not a dependency.  No CPU fallback: without the HIP library / a GPU these
functions raise.

`extract_features(dataset_dir, features_dir, hparams, n_jobs)` (`extract_features.py:512-553`) turns a data set into the
feature files the trainer reads, a batch of utterances at a time: wavs, markers and sentences are read on one
host thread, the batch is resampled, cropped (`dx_wav_crop`), analysed (`mel_spectrogram_batch`, `pitch_batch`), its aligner
spans become frame counts (`dx_marker_durations`) and its frames symbol means (`dx_symbol_pool`), one copy brings everything
to the host and another thread (`write_behind.WriteBehind`) formats and writes the files.  `duration_to_integer`, `get_symbols_energy` and
`get_symbols_pitch` are the one-utterance wrappers with the signatures of the reference; `update_markers`,
`get_min_phone_duration` and `check_features_config_used` are host text logic.
"""
import collections
import json
import logging
import math
import os
import re
import string
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from daft_exprt import _hip as H
from daft_exprt.audio import crop_range, device_waves, fft_tables, read_wav, resampled_length, to_float_mono
from daft_exprt.audio import rescale_wav_to_float32  # noqa: F401  (the reference keeps it here, `extract_features.py:362`)
from daft_exprt.write_behind import WriteBehind
from daft_exprt.symbols import SIL_WORD_SYMBOL, eos, punctuation, whitespace

_logger = logging.getLogger(__name__)
# the hyper-parameters a features directory depends on (`extract_features.py:26-28`)
FEATURES_HPARAMS = ['centered', 'cutoff', 'f0_interval', 'filter_length', 'hop_length', 'language', 'mel_fmax', 'mel_fmin',
                    'min_clipping', 'max_f0', 'min_f0', 'n_mel_channels', 'order', 'sampling_rate', 'symbols', 'uv_cost',
                    'uv_interval']


PITCH_WINDOW_S = 0.015     # correlation window of the pitch tracker


def _hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, 1e-30) / min_log_hz) / logstep, f / f_sp)


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def mel_filter_bank(sr, n_fft, n_mels, fmin, fmax):
    ''' (n_mels, 1 + n_fft // 2) float32: triangular filters on the Slaney mel scale, each normalised to unit area '''
    fmax = float(sr) / 2 if fmax is None else float(fmax)
    freqs = np.linspace(0., float(sr) / 2, 1 + n_fft // 2)
    edges = _mel_to_hz(np.linspace(_hz_to_mel(fmin), _hz_to_mel(fmax), n_mels + 2))
    width = np.diff(edges)
    ramps = edges[:, None] - freqs[None, :]
    fb = np.maximum(0., np.minimum(-ramps[:-2] / width[:-1, None], ramps[2:] / width[1:, None]))
    fb *= (2.0 / (edges[2:] - edges[:-2]))[:, None]
    return fb.astype(np.float32)


def mel_tables(hparams, device):
    ''' (filterbank (n_mel, n_fft/2 + 1) fp32, lo, hi (n_mel,) int32: filter m is non-zero on bins lo[m] .. hi[m] - 1) on `device` '''
    def make():
        fb = mel_filter_bank(hparams.sampling_rate, int(hparams.filter_length), hparams.n_mel_channels, hparams.mel_fmin, hparams.mel_fmax)
        nz = fb > 0
        lo = np.where(nz.any(1), nz.argmax(1), 0).astype(np.int32)
        hi = np.where(nz.any(1), fb.shape[1] - nz[:, ::-1].argmax(1), 0).astype(np.int32)
        return torch.from_numpy(fb).to(device), torch.from_numpy(lo).to(device), torch.from_numpy(hi).to(device)
    return H.device_table('mel', device, hparams.sampling_rate, hparams.filter_length, hparams.n_mel_channels, hparams.mel_fmin,
                          hparams.mel_fmax, make=make)


def nb_frames(n_samples, hparams):
    ''' frames torch.stft produces for a waveform of n_samples (`extract_features.py:347-348`) '''
    n_fft, hop = int(hparams.filter_length), int(hparams.hop_length)
    if hparams.centered:
        return 1 + n_samples // hop
    return 1 + (n_samples - n_fft) // hop if n_samples >= n_fft else 0


def mel_spectrogram_batch(wavs, n_samples, hparams, min_samples=None):
    ''' wavs (B, S) float32 device tensor (right-padded), n_samples (B,) int64 device tensor.
        Returns (log-mel (B, n_mel, T) fp32, frame energies (B, T) fp32, n_frames (B,) int64); frames >= n_frames[b] are 0.
        min_samples: min(n_samples) when the caller knows it on the host (the length check then reads nothing back). '''
    H.require_gpu(wavs, n_samples)
    assert wavs.dtype == torch.float32 and wavs.stride(1) == 1 and n_samples.dtype == torch.int64
    B, S = wavs.shape
    dev = wavs.device
    n_fft, hop, n_mel = int(hparams.filter_length), int(hparams.hop_length), int(hparams.n_mel_channels)
    if hparams.centered and (int(n_samples.min()) if min_samples is None else int(min_samples)) <= n_fft // 2:
        raise ValueError('mel_spectrogram: reflect padding needs more than filter_length / 2 samples')
    T = max(1, nb_frames(S, hparams))
    basis, window = fft_tables(n_fft, False, dev)
    fb, lo, hi = mel_tables(hparams, dev)
    mel = torch.empty((B, n_mel, T), dtype=torch.float32, device=dev)
    energy = torch.empty((B, T), dtype=torch.float32, device=dev)
    n_frames = torch.empty((B,), dtype=torch.int64, device=dev)
    H.check(H.lib().dx_mel_spectrogram(H.ptr(wavs), wavs.stride(0), H.ptr(n_samples), H.ptr(basis), H.ptr(window), H.ptr(fb),
                                       H.ptr(lo), H.ptr(hi), H.ptr(mel), H.ptr(energy), H.ptr(n_frames), B, T, n_fft,
                                       hop, n_mel, int(bool(hparams.centered)), float(hparams.min_clipping), H.stream()))
    return mel, energy, n_frames


def mel_spectrogram_HiFi(wav, hparams, device='cuda:0'):
    ''' reference signature (`extract_features.py:330`): wav (T,) in [-1, 1] -> log-mel (n_mel_channels, n_frames) NumPy '''
    w = torch.as_tensor(np.asarray(wav, dtype=np.float32)).reshape(1, -1).to(device)
    n = torch.tensor([w.shape[1]], dtype=torch.int64, device=device)
    mel, _, nfr = mel_spectrogram_batch(w, n, hparams)
    return mel[0, :, :int(nfr[0])].cpu().numpy()


def pitch_geometry(hparams, sr=None):
    ''' (sr, step = samples per analysis frame, window, lag_min, lag_max) of the pitch tracker at rate `sr` (default
        hparams.sampling_rate): a 15 ms window and the lags floor(sr / max_f0) .. ceil(sr / min_f0) '''
    sr = int(hparams.sampling_rate if sr is None else sr)
    lag_min, lag_max = int(math.floor(sr / float(hparams.max_f0))), int(math.ceil(sr / float(hparams.min_f0)))
    if not 2 <= lag_min < lag_max:
        raise ValueError(f'pitch: min_f0={hparams.min_f0}, max_f0={hparams.max_f0} give no lag range at {sr} Hz')
    return sr, float(sr) * float(hparams.f0_interval), int(round(PITCH_WINDOW_S * sr)), lag_min, lag_max


def pitch_candidates_batch(wavs, n_samples, hparams, sr=None):
    ''' `dx_pitch_candidates`: (lags, values), each (B, A, K) fp32 on the device, A = 1 + floor(S / step): per analysis frame the
        up to K best maxima of the normalised cross-correlation, in order of value; empty slots are 0 '''
    H.require_gpu(wavs, n_samples)
    assert wavs.dtype == torch.float32 and wavs.dim() == 2 and wavs.stride(1) == 1 and n_samples.dtype == torch.int64
    sr, step, window, lag_min, lag_max = pitch_geometry(hparams, sr)
    B, S = wavs.shape
    A = 1 + int(math.floor(S / step))
    K = int(H.lib().dx_pitch_num_candidates())
    dev = wavs.device
    lags = torch.empty((B, A, K), dtype=torch.float32, device=dev)
    vals = torch.empty((B, A, K), dtype=torch.float32, device=dev)
    mean_sq = torch.empty((B,), dtype=torch.float64, device=dev)
    H.check(H.lib().dx_pitch_candidates(H.ptr(wavs), wavs.stride(0), H.ptr(n_samples), H.ptr(mean_sq), H.ptr(lags), H.ptr(vals),
                                        B, S, A, step, window, lag_min, lag_max, H.stream()))
    return lags, vals


def pitch_track_batch(wavs, n_samples, hparams, sr=None):
    ''' both kernels: (log_pitch (B, T) fp32, n_frames (B,) int64, hz (B, A) fp32 per analysis frame, (lags, values)) '''
    lags, vals = pitch_candidates_batch(wavs, n_samples, hparams, sr)
    sr, step, _, _, lag_max = pitch_geometry(hparams, sr)
    B, S = wavs.shape
    _, A, K = lags.shape
    hop = int(hparams.hop_length)
    T = 1 + S // hop
    dev = wavs.device
    back = torch.empty((B, A, K + 1), dtype=torch.uint8, device=dev)
    hz = torch.empty((B, A), dtype=torch.float32, device=dev)
    log_pitch = torch.empty((B, T), dtype=torch.float32, device=dev)
    n_frames = torch.empty((B,), dtype=torch.int64, device=dev)
    H.check(H.lib().dx_pitch_viterbi(H.ptr(lags), H.ptr(vals), H.ptr(n_samples), H.ptr(back), H.ptr(hz), H.ptr(log_pitch),
                                     H.ptr(n_frames), B, S, A, T, sr, step, hop, lag_max, float(hparams.uv_cost), H.stream()))
    return log_pitch, n_frames, hz, (lags, vals)


def pitch_batch(wavs, n_samples, hparams, sr=None):
    ''' wavs (B, S) float32 device tensor (right-padded), n_samples (B,) int64 device tensor, sampled at `sr` (default
        hparams.sampling_rate).  Returns (log_pitch (B, T) fp32 on the device, n_frames (B,) int64): per mel frame
        (T = 1 + S // hop_length, n_frames[b] = 1 + n_samples[b] // hop_length, as `mel_spectrogram_batch` with `centered`)
        log(Hz), 0 where unvoiced and for frames >= n_frames[b].
        hparams.f0_interval, min_f0, max_f0 and uv_cost mean what they mean to the reference's binary (analysis interval, search
        range, weight of the unvoiced hypothesis).  hparams.uv_interval is accepted and ignored: it spaces REAPER's pitch marks
        in unvoiced regions and has no meaning without pitch marks.  The Hz is not rounded to an integer, as the reference
        binary's output format does. '''
    log_pitch, n_frames, _, _ = pitch_track_batch(wavs, n_samples, hparams, sr)
    return log_pitch, n_frames


def extract_pitch(wav, fs, hparams, device='cuda:0'):
    ''' reference signature (`extract_features.py:222`): wav (n,) in [-1, 1] sampled at fs -> (1 + n // hop_length,) NumPy,
        log(Hz) per mel frame, 0 where unvoiced '''
    w = torch.as_tensor(np.asarray(wav, dtype=np.float32)).reshape(1, -1).to(device)
    n = torch.tensor([w.shape[1]], dtype=torch.int64, device=device)
    log_pitch, nfr = pitch_batch(w, n, hparams, sr=fs)
    return log_pitch[0, :int(nfr[0])].cpu().numpy()


def extract_energy(mel_spec):
    ''' `extract_features.py:299-304`: L2 norm over the mel channels (callers pass np.exp(log-mel)); tiny, host side '''
    return np.linalg.norm(mel_spec, axis=0)


# ---- training features of a data set (`extract_features.py:31-111, 114-219, 272-327, 387-553`) -------------------------------

def check_features_config_used(features_dir, hparams):
    ''' `extract_features.py:31-52`: True when every `*.json` config found under features_dir (the first of each directory)
        agrees with hparams on FEATURES_HPARAMS; every difference is logged '''
    same = True
    for root, _, names in os.walk(os.path.normpath(features_dir)):
        configs = [name for name in names if name.endswith('.json')]
        if not configs:
            continue
        with open(os.path.join(root, configs[0])) as f:
            previous = json.load(f)
        for param in FEATURES_HPARAMS:
            now, was = getattr(hparams, param), previous[param]
            if now != was:
                same = False
                _logger.warning(f'Parameter "{param}" is different in "{root}" -- Was {was} and now is {now}')
    return same


def get_min_phone_duration(lines, min_phone_dur=1000.):
    ''' `extract_features.py:55-66`: the shortest `end - begin` over the rows of a .markers file (and min_phone_dur) '''
    for line in lines:
        begin, end = line.strip().split(sep='\t')[:2]
        min_phone_dur = min(min_phone_dur, float(end) - float(begin))
    return min_phone_dur


def marker_lines_span(lines):
    ''' (sent_begin, sent_end) in seconds of the rows of a .markers file: begin of the first row, end of the last '''
    return float(lines[0].strip().split(sep='\t')[0]), float(lines[-1].strip().split(sep='\t')[1])


def wav_crop_batch(wavs, crop, width):
    ''' `dx_wav_crop`: wavs (B, S) fp32 and crop (B, 2) int64 (begin, length) on the device -> (B, width) fp32, row b holding
        wavs[b, begin_b: begin_b + length_b] left-aligned and zeros behind it '''
    H.require_gpu(wavs, crop)
    assert wavs.dtype == torch.float32 and wavs.dim() == 2 and wavs.stride(1) == 1
    assert crop.dtype == torch.int64 and crop.is_contiguous() and crop.shape == (wavs.shape[0], 2)
    B, S = wavs.shape
    y = torch.empty((B, max(int(width), 1)), dtype=torch.float32, device=wavs.device)
    H.check(H.lib().dx_wav_crop(H.ptr(wavs), wavs.stride(0), H.ptr(crop), H.ptr(y), y.stride(0), B, S, H.stream()))
    return y


def marker_durations_batch(spans, n_rows, n_samples, hparams):
    ''' `dx_marker_durations`: spans (B, L, 2) fp64 (begin, end) in seconds from the sentence begin, n_rows (B,) and n_samples
        (B,) int64, all on the device.  Returns (durations (B, L) int64, n_out (B,) int64: how many of them the list of the
        reference holds, status (B,) int32: 0 ok, 1 IndexError, 2 ValueError, 3 an assert of `extract_features.py:437-439`) '''
    H.require_gpu(spans, n_rows, n_samples)
    assert spans.dtype == torch.float64 and spans.dim() == 3 and spans.shape[2] == 2 and spans.is_contiguous()
    assert n_rows.dtype == torch.int64 and n_samples.dtype == torch.int64
    B, L, _ = spans.shape
    dev = spans.device
    durations = torch.empty((B, L), dtype=torch.int64, device=dev)
    n_out = torch.empty((B,), dtype=torch.int64, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    H.check(H.lib().dx_marker_durations(H.ptr(spans), H.ptr(n_rows), H.ptr(n_samples), H.ptr(durations), H.ptr(n_out), H.ptr(status),
                                        B, L, float(hparams.sampling_rate), int(hparams.filter_length), int(hparams.hop_length),
                                        int(bool(hparams.centered)), H.stream()))
    return durations, n_out, status


def symbol_pool_batch(energy, log_pitch, durations, n_rows):
    ''' `dx_symbol_pool`: energy / log_pitch (B, T) fp32, durations (B, L) int64, n_rows (B,) int64 on the device ->
        (sym_energy, sym_pitch) (B, L) fp32: per row the mean of its frames / of its frames > 0; 0 for rows of duration 0 '''
    H.require_gpu(energy, log_pitch, durations, n_rows)
    assert energy.dtype == torch.float32 and log_pitch.dtype == torch.float32 and energy.shape == log_pitch.shape
    assert energy.stride(1) == 1 and log_pitch.stride(1) == 1 and energy.stride(0) == log_pitch.stride(0)
    assert durations.dtype == torch.int64 and durations.is_contiguous() and n_rows.dtype == torch.int64
    B, T = energy.shape
    L = durations.shape[1]
    sym_energy = torch.empty((B, L), dtype=torch.float32, device=energy.device)
    sym_pitch = torch.empty((B, L), dtype=torch.float32, device=energy.device)
    H.check(H.lib().dx_symbol_pool(H.ptr(energy), H.ptr(log_pitch), energy.stride(0), H.ptr(durations), H.ptr(n_rows),
                                   H.ptr(sym_energy), H.ptr(sym_pitch), B, T, L, H.stream()))
    return sym_energy, sym_pitch


def duration_to_integer(float_durations, hparams, nb_samples=None, device='cuda:0'):
    ''' reference signature (`extract_features.py:69-111`): [[begin, end], ...] in seconds -> list of integer frame durations.
        Raises IndexError / ValueError where the reference does.  Without nb_samples the sample count is int(total duration *
        sampling_rate), summed in the order of the reference on the host. '''
    spans = [[float(begin), float(end)] for begin, end in float_durations]
    if nb_samples is None:
        nb_samples = int(sum([(x[1] - x[0]) for x in spans]) * hparams.sampling_rate)
    dev = H.device(device)
    host = torch.zeros((1, max(len(spans), 1), 2), dtype=torch.float64)
    if spans:
        host[0, :len(spans)] = torch.tensor(spans, dtype=torch.float64)
    durations, n_out, status = marker_durations_batch(host.to(dev), torch.tensor([len(spans)], dtype=torch.int64, device=dev),
                                                      torch.tensor([int(nb_samples)], dtype=torch.int64, device=dev), hparams)
    status = int(status[0])
    if status == 1:
        raise IndexError('duration_to_integer: the markers end before the frames do')
    if status == 2:
        raise ValueError('duration_to_integer: a marker of zero length')
    return durations[0, :int(n_out[0])].cpu().tolist()


def _float_text(values):
    ''' one '%.3f' line per element of a float32 array: what `f'{val:.3f}\\n'` writes for each of them, as one string '''
    values = np.asarray(values).tolist()
    return ('%.3f\n' * len(values)) % tuple(values)


def _pool_one(frames, markers, which, device):
    dev = H.device(device)
    durations = torch.tensor([[int(marker[2]) for marker in markers] or [0]], dtype=torch.int64, device=dev)
    values = torch.as_tensor(np.asarray(frames, dtype=np.float32)).reshape(1, -1).to(dev)
    if values.shape[1] == 0:
        values = torch.zeros((1, 1), dtype=torch.float32, device=dev)
    n_rows = torch.tensor([len(markers)], dtype=torch.int64, device=dev)
    pooled = symbol_pool_batch(values, values, durations, n_rows)[which]
    return _float_text(pooled[0, :len(markers)].cpu().numpy()).splitlines(keepends=True)


def get_symbols_energy(energy, markers, device='cuda:0'):
    ''' reference signature (`extract_features.py:307-327`): mean frame energy per marker row, one '%.3f' line each '''
    return _pool_one(energy, markers, 0, device)


def get_symbols_pitch(pitch, markers, device='cuda:0'):
    ''' reference signature (`extract_features.py:272-296`): mean voiced log-pitch per marker row, one '%.3f' line each '''
    return _pool_one(pitch, markers, 1, device)


def sentence_tokens(sentence):
    ''' (tokens, closing) of a .lab sentence as `update_markers` reads it: lower-cased words and punctuation marks, the marks in
        front of the first word dropped, those behind the last word taken off -- `closing` is the one right behind it, or None '''
    kept = set(string.ascii_letters + punctuation)
    tokens = [t for t in re.findall(rf"[\w']+|[{punctuation}]", sentence.lower().strip()) if kept.intersection(t)]
    while tokens and tokens[0] in punctuation:
        del tokens[0]
    closing = None                               # of a run of closing marks the first one is kept
    while tokens and tokens[-1] in punctuation:
        closing = tokens.pop()
    return tokens, closing


def update_markers(file_name, lines, sentence, sent_begin, int_durations, hparams, logger):
    ''' `extract_features.py:114-219`: the aligner rows `begin end phone word word_idx` of one utterance become the rows
        `begin end int_dur symbol word word_idx` of its feature file: times counted from sent_begin, a word-boundary row (a
        whitespace, or the punctuation mark the sentence has there) between two words -- it takes the timing and frames of the
        `<sil>` row the aligner put there, or is empty --, the closing punctuation mark of the sentence and the EOS row.
        Returns None, with a warning, when the words of the sentence and of the markers cannot be matched.  (Where the
        reference ends in an IndexError or a failed assert -- nothing but punctuation in the sentence, rows left over --
        this returns None as well.) '''
    if hparams.language != 'english':
        raise NotImplementedError()
    tokens, closing = sentence_tokens(sentence)
    rows = [line.strip().split(sep='\t') for line in lines]
    sentence_words = list(tokens)

    def problem(what):
        first_rows = {}
        for row in rows:
            first_rows.setdefault(row[4], row[3])
        logger.warning(f'Correspondance issue between words in the .lab sentence and those in .markers file -- File name: '
                       f'{file_name} -- Sentence: {sentence_words} -- Markers: {list(first_rows.values())} -- {what}')

    def shifted(row):
        return f'{float(row[0]) - sent_begin:.3f}', f'{float(row[1]) - sent_begin:.3f}'

    if not tokens:
        problem('no word in the sentence')
        return None
    pending = collections.deque(tokens)
    out, k, word_idx = [], 0, 0
    while pending:
        token = pending.popleft()
        if k == len(rows):
            problem(f'no marker left for: {token}')
            return None
        word, group = rows[k][3], rows[k][4]
        if word != token:                        # the apostrophe: example' is aligned as example, that's as that + s
            parts = re.findall(rf"[\w]+|[{punctuation}]", token)
            pending.extendleft(reversed(parts[1:]))
            token = parts[0] if parts else token
            if word != token:
                problem(f'Problematic words: {token} -- {word}')
                return None
        while k < len(rows) and rows[k][4] == group:
            begin, end = shifted(rows[k])
            out.append([begin, end, str(int_durations[k]), rows[k][2], rows[k][3], str(word_idx)])
            k += 1
        word_idx += 1
        if pending:
            bound = pending.popleft() if pending[0] in punctuation else whitespace
            if k < len(rows) and rows[k][3] == SIL_WORD_SYMBOL:
                begin, end = shifted(rows[k])
                out.append([begin, end, str(int_durations[k]), bound, bound, str(word_idx)])
                k += 1
            else:
                out.append([out[-1][1], out[-1][1], '0', bound, bound, str(word_idx)])
            word_idx += 1
    if k != len(rows):
        problem(f'{len(rows) - k} marker rows left over')
        return None
    for symbol in ([closing] if closing is not None else []) + [eos]:
        out.append([out[-1][1], out[-1][1], '0', symbol, symbol, str(word_idx)])
        word_idx += 1
    return out


class _FeatureUtterance(object):
    ''' what the reader thread hands over for one utterance '''
    def __init__(self, speaker, name, lines, sentence):
        self.speaker, self.name, self.lines, self.sentence, self.samples, self.rate = speaker, name, lines, sentence, None, None
        self.sent_begin, self.sent_end = marker_lines_span(lines)
        rows = [line.strip().split(sep='\t') for line in lines]
        self.spans = [[float(row[0]) - self.sent_begin, float(row[1]) - self.sent_begin] for row in rows]


def _read_features_batch(dataset_dir, speaker, names, hparams, skipped):
    ''' reader thread: markers, sentence and samples of every utterance of the batch that is long enough '''
    utts = []
    half_window = hparams.filter_length / hparams.sampling_rate / 2
    for name in names:
        markers_file = os.path.join(dataset_dir, speaker, 'align', f'{name}.markers')
        wav_file = os.path.join(dataset_dir, speaker, 'wavs', f'{name}.wav')
        sentence_file = os.path.join(dataset_dir, speaker, 'align', f'{name}.lab')
        for path in (wav_file, sentence_file):
            if not os.path.isfile(path):
                raise FileNotFoundError(f'There is no such file: {path}')
        with open(markers_file, 'r', encoding='utf-8') as f:
            lines = f.readlines()
        # a phone has to span more than half an analysis window to own at least one frame
        min_phone_dur = get_min_phone_duration(lines)
        assert min_phone_dur > half_window, f'{markers_file} -- Min phone duration = {min_phone_dur} -- filter_length / 2 = {half_window}'
        with open(sentence_file, 'r', encoding='utf-8') as f:
            sentence = f.readline()
        utt = _FeatureUtterance(speaker, name, lines, sentence)
        if utt.sent_end - utt.sent_begin < hparams.minimum_wav_duration / 1000:
            _logger.warning(f'Ignoring {wav_file} -- audio has length inferior to {hparams.minimum_wav_duration / 1000}s after trimming')
            skipped.append((speaker, name, 'shorter than minimum_wav_duration'))
            continue
        x, utt.rate = read_wav(wav_file)
        utt.samples = to_float_mono(x)
        utts.append(utt)
    return utts


class _FeatureFiles(object):
    ''' `write` of the pass's `WriteBehind`: formats and writes the files of one batch; counts `written`, appends to `skipped` '''
    STATUS = {1: 'the markers end before the frames do', 2: 'a marker of zero length',
              3: 'the frame durations do not match the markers or the mel-spectrogram'}

    def __init__(self, features_dir, hparams, skipped):
        self.features_dir, self.hparams, self.skipped, self.written = features_dir, hparams, skipped, 0

    def __call__(self, raw, layout, utts):
        parts, off = {}, 0
        for key, dtype, shape in layout:
            size = int(np.prod(shape)) * np.dtype(dtype).itemsize
            parts[key] = raw[off: off + size].view(dtype).reshape(shape)
            off += size
        for b, u in enumerate(utts):
            status, T, L = int(parts['status'][b]), int(parts['n_frames'][b]), len(u.lines)
            if status != 0:
                _logger.warning(f'Ignoring {u.speaker} -- {u.name} -- {self.STATUS[status]}')
                self.skipped.append((u.speaker, u.name, self.STATUS[status]))
                continue
            durations = parts['durations'][b, :L].tolist()
            markers = update_markers(u.name, u.lines, u.sentence, u.sent_begin, durations, self.hparams, _logger)
            if markers is None:
                self.skipped.append((u.speaker, u.name, 'the sentence does not match the markers'))
                continue
            # rows added by update_markers hold no frames: 0.000; the others are the aligner rows, in order
            # (status 0 says no aligner row has 0 frames, so the rows with frames are exactly the aligner rows)
            assert 0 not in durations and sum(marker[2] != '0' for marker in markers) == L, (u.speaker, u.name)
            aligned = iter(range(L))
            pick = [next(aligned) if marker[2] != '0' else -1 for marker in markers]
            sym_energy = np.append(parts['sym_energy'][b, :L], np.float32(0.))[pick]
            sym_pitch = np.append(parts['sym_pitch'][b, :L], np.float32(0.))[pick]
            base = os.path.join(self.features_dir, u.speaker, u.name)
            np.save(base + '.npy', parts['mel'][b, :, :T])
            texts = (('.markers', ''.join('\t'.join(marker) + '\n' for marker in markers)),
                     ('.frames_nrg', _float_text(parts['energy'][b, :T])), ('.symbols_nrg', _float_text(sym_energy)),
                     ('.frames_f0', _float_text(parts['pitch'][b, :T])), ('.symbols_f0', _float_text(sym_pitch)))
            for ext, text in texts:               # .symbols_f0 last: it marks the utterance as done
                with open(base + ext, 'w', encoding='utf-8') as f:
                    f.write(text)
            self.written += 1


def features_batch(utts, hparams, device):
    ''' device side of one batch of `extract_features`: utts carry `.samples`, `.rate`, `.spans` and `.sent_begin / .sent_end`;
        every crop must hold more than filter_length / 2 samples.  Returns (one uint8 device buffer, its layout [(key, dtype,
        shape)]) holding mel (B, n_mel, T), energy, pitch (B, T), n_frames (B,), durations (B, L), status (B,), sym_energy and
        sym_pitch (B, L). '''
    fs = int(hparams.sampling_rate)
    wavs, n_total = device_waves(utts, fs, device)
    crops = [crop_range(u.sent_begin, u.sent_end, fs, n) for u, n in zip(utts, n_total)]
    B, L = len(utts), max(len(u.spans) for u in utts)
    spans = np.zeros((B, L, 2), dtype=np.float64)
    for b, u in enumerate(utts):
        spans[b, :len(u.spans)] = u.spans
    ints = torch.tensor([[begin, n, len(u.spans)] for (begin, n), u in zip(crops, utts)], dtype=torch.int64).pin_memory()
    ints = ints.to(device, non_blocking=True)
    crop, n_samples, n_rows = ints[:, :2].contiguous(), ints[:, 1].contiguous(), ints[:, 2].contiguous()
    spans = torch.from_numpy(spans).pin_memory().to(device, non_blocking=True)
    cropped = wav_crop_batch(wavs, crop, max(n for _, n in crops))
    mel, energy, n_frames = mel_spectrogram_batch(cropped, n_samples, hparams, min_samples=min(n for _, n in crops))
    log_pitch, _ = pitch_batch(cropped, n_samples, hparams)
    durations, _, status = marker_durations_batch(spans, n_rows, n_samples, hparams)
    sym_energy, sym_pitch = symbol_pool_batch(energy, log_pitch, durations, n_rows)
    named = (('mel', mel), ('energy', energy), ('pitch', log_pitch), ('n_frames', n_frames), ('durations', durations),
             ('status', status), ('sym_energy', sym_energy), ('sym_pitch', sym_pitch))
    layout = [(key, str(t.dtype).replace('torch.', ''), tuple(t.shape)) for key, t in named]
    return torch.cat([t.contiguous().view(-1).view(torch.uint8) for _, t in named]), layout


def _plan_batches(names, sizes, batch_size, sample_budget):
    ''' consecutive runs of at most batch_size utterances whose padded batch (count * longest) stays within sample_budget.
        `sizes` are estimates from the byte sizes of the wav files -- bytes / 2, the sample count of 16-bit mono at the target
        rate; a file stored at a lower rate or in 8 bits grows past it -- so the budget is a soft one '''
    batches, current, longest = [], [], 0
    for name, size in zip(names, sizes):
        if current and (len(current) == batch_size or (len(current) + 1) * max(longest, size) > sample_budget):
            batches.append(current)
            current, longest = [], 0
        current.append(name)
        longest = max(longest, size)
    if current:
        batches.append(current)
    return batches


def extract_features(dataset_dir, features_dir, hparams, n_jobs, batch_size=64, sample_budget=64 * 30 * 22050, device='cuda:0'):
    ''' `extract_features.py:512-553`: for every speaker, the feature files (.npy .markers .frames_nrg .symbols_nrg .frames_f0
        .symbols_f0) of every utterance of `<features_dir>/<speaker>/metadata.csv` that has markers and no .symbols_f0 yet, then
        `config.json`.  n_jobs is accepted for the signature of the reference: the work is batched on the device with one
        reader and one writer thread beside it.  An utterance the reference would fail an assert on -- frame durations that do
        not match, a sentence that cannot be matched to its markers -- is skipped with a warning.
        Returns {'written', 'already_done', 'skipped': [(speaker, file, reason)], 'batches', 'seconds', 'read_wait_s', 'write_s'}. '''
    if not hparams.centered:
        raise ValueError('extract_features: the pitch frames line up with the mel frames only with hparams.centered')
    dev = H.device(device)
    for line in ('--' * 30, 'EXTRACTING FEATURES', '--' * 30):
        _logger.info(line)
    skipped = []
    report = {'written': 0, 'already_done': 0, 'skipped': skipped, 'batches': 0, 'seconds': 0., 'read_wait_s': 0., 'write_s': 0.}
    start = time.time()
    fs, min_samples = int(hparams.sampling_rate), int(hparams.filter_length) // 2 + 1
    for speaker in hparams.speakers:
        _logger.info(f'Speaker: "{speaker}"')
        wavs_dir, markers_dir = os.path.join(dataset_dir, speaker, 'wavs'), os.path.join(dataset_dir, speaker, 'align')
        spk_features_dir = os.path.join(features_dir, speaker)
        metadata = os.path.join(spk_features_dir, 'metadata.csv')
        for path, is_there in ((wavs_dir, os.path.isdir), (markers_dir, os.path.isdir), (metadata, os.path.isfile)):
            if not is_there(path):
                raise FileNotFoundError(f'There is no such {"directory" if is_there is os.path.isdir else "file"}: {path}')
        with open(metadata, 'r', encoding='utf-8') as f:
            names = [line.strip().split(sep='|')[0].strip() for line in f.readlines()]
        names = [name for name in names if os.path.isfile(os.path.join(markers_dir, f'{name}.markers'))]
        done = set(x[:-len('.symbols_f0')].strip() for x in os.listdir(spk_features_dir) if x.endswith('.symbols_f0'))
        missing = [name for name in names if name not in done]
        report['already_done'] += len(names) - len(missing)
        _logger.info(f'{len(names) - len(missing)} files already processed. {len(missing)} new files need to be processed')
        if missing:
            wav_files = [os.path.join(wavs_dir, f'{name}.wav') for name in missing]
            sizes = [os.path.getsize(path) // 2 if os.path.isfile(path) else 0 for path in wav_files]
            batches = _plan_batches(missing, sizes, int(batch_size), int(sample_budget))
            files = _FeatureFiles(features_dir, hparams, skipped)
            writer = WriteBehind(files, 'features_writer')
            reader = ThreadPoolExecutor(max_workers=1, thread_name_prefix='features_reader')
            try:
                pending = reader.submit(_read_features_batch, dataset_dir, speaker, batches[0], hparams, skipped)
                for idx in range(len(batches)):
                    t0 = time.time()
                    utts = pending.result()
                    report['read_wait_s'] += time.time() - t0
                    if idx + 1 < len(batches):
                        pending = reader.submit(_read_features_batch, dataset_dir, speaker, batches[idx + 1], hparams, skipped)
                    keep = []
                    for u in utts:                   # the mel front-end reflects half a window at both ends of the crop
                        if crop_range(u.sent_begin, u.sent_end, fs, resampled_length(u, fs))[1] < min_samples:
                            _logger.warning(f'Ignoring {speaker} -- {u.name} -- the wav ends before its markers do')
                            skipped.append((speaker, u.name, 'the wav ends before its markers do'))
                        else:
                            keep.append(u)
                    if not keep:
                        continue
                    buf, layout = features_batch(keep, hparams, dev)
                    writer.put(buf, layout, keep)
                    report['batches'] += 1
            finally:
                reader.shutdown(wait=True)
                writer.close()
                report['written'] += files.written
                report['write_s'] += writer.busy_s
        # the config the features were extracted with
        hparams.save_hyper_params(os.path.join(spk_features_dir, 'config.json'))
        _logger.info('')
    report['seconds'] = time.time() - start
    return report
