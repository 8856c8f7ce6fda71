"""Statistics of the training features (reference: `src/daft_exprt/features_stats.py:90-165`): what `stats.json` holds and
`DaftExprtDataLoader` standardises with.

Taken over the training list only, from the written text files -- the 3-decimal values, as the reference takes them -- in
float64 NumPy on the host: a few million numbers for a corpus, read once.
"""
import collections
import logging
import os

import numpy as np

_logger = logging.getLogger(__name__)


def _non_zero_values(path):
    ''' the values of a one-float-per-line file that are not 0 (silent / unvoiced symbols) '''
    with open(path, 'r', encoding='utf-8') as f:
        values = [float(line.strip()) for line in f.readlines()]
    return [value for value in values if value != 0.]


def _symbols_durations(markers_file, hparams):
    ''' [(symbol, end - begin)] of a features .markers file '''
    out = []
    with open(markers_file, 'r', encoding='utf-8') as f:
        for line in f.readlines():
            begin, end, _, symbol, _, _ = line.strip().split(sep='\t')
            assert symbol in hparams.symbols, f'{markers_file} -- Symbol "{symbol}" does not exist'
            out.append((symbol, float(end) - float(begin)))
    return out


def _summary(values, prefix=''):
    return {f'{prefix}mean': np.mean(values), f'{prefix}std': np.std(values), f'{prefix}min': np.min(values),
            f'{prefix}max': np.max(values)}


def extract_features_stats(hparams, n_jobs):
    ''' {'spk <id>': {'energy': {mean, std, min, max}, 'pitch': {...}}, ..., 'symbols': {symbol: {dur_min, dur_max, dur_mean,
        dur_std}}}: per speaker id over the non-zero symbol energies / pitches of its training files (population std), per
        symbol over its durations in seconds.  n_jobs is accepted for the signature of the reference. '''
    with open(hparams.training_files, 'r', encoding='utf-8') as f:
        training_files = [line.strip().split(sep='|') for line in f.readlines()]
    for line in ('--' * 30, 'EXTRACTING FEATURES STATS', '--' * 30):
        _logger.info(line)
    durations = collections.defaultdict(list)
    stats = {}
    for speaker_id in set(hparams.speakers_id):
        _logger.info(f'Speaker ID: {speaker_id}')
        bases = [os.path.join(features_dir, name) for features_dir, name, sid in training_files if int(sid) == speaker_id]
        energy, pitch = [], []
        for base in bases:
            for symbol, duration in _symbols_durations(base + '.markers', hparams):
                durations[symbol].append(duration)
            energy.extend(_non_zero_values(base + '.symbols_nrg'))
            pitch.extend(_non_zero_values(base + '.symbols_f0'))
        stats[f'spk {speaker_id}'] = {'energy': _summary(energy), 'pitch': _summary(pitch)}
        _logger.info('')
    stats['symbols'] = {symbol: _summary(values, prefix='dur_') for symbol, values in durations.items()}
    return stats
