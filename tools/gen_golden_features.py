#!/usr/bin/env python
"""Record tests/golden/features_kat.json: inputs fabricated here and what the REFERENCE's own feature-extraction host
functions make of them -- `duration_to_integer(..., nb_samples=n)` (plus the three asserts of its caller), `update_markers`,
`get_symbols_energy`, `get_symbols_pitch`, `create_sets` and `extract_features_stats`.  Only data goes into the file.

Run once where a checkout of the reference is readable:
    python tools/gen_golden_features.py --reference <reference checkout>/src
Shims as in tools/gen_goldens.py: stub modules for its absent third-party imports (librosa) and for `daft_exprt.utils`
(matplotlib, multiprocessing pools), whose `launch_multi_process` becomes a plain loop.
"""
import argparse
import json
import logging
import os
import queue
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'features_kat.json')
CONFIGS = [dict(sampling_rate=22050, filter_length=1024, hop_length=256), dict(sampling_rate=16000, filter_length=512, hop_length=128)]


def install_shims(reference_src):
    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m
    librosa = stub('librosa')
    librosa.filters = stub('librosa.filters', mel=lambda *a, **k: None)
    sys.path.insert(0, reference_src)
    import daft_exprt  # noqa: F401  (the package itself imports nothing)

    def launch_multi_process(iterable, func, n_jobs, **kwargs):
        kwargs = {k: v for k, v in kwargs.items() if k not in ('chunksize', 'ordered', 'timer_verbose')}
        log_queue = queue.Queue()
        return [func(item, log_queue=log_queue, **kwargs) for item in iterable]
    stub('daft_exprt.utils', launch_multi_process=launch_multi_process)


# ---- duration KATs ------------------------------------------------------------------------------------------------------------

def duration_cases(rng):
    ''' [(config index, centered, spans, n_samples)]: times rounded to 1e-4 s to keep the file small '''
    cases = []
    for i in range(320):
        c = 0 if i % 4 else 1
        sr, fl, hop = (CONFIGS[c][k] for k in ('sampling_rate', 'filter_length', 'hop_length'))
        centered = i % 7 != 3
        kind = ['plain', 'plain', 'plain', 'wav_short', 'wav_long', 'sub_window', 'near_threshold', 'zero_row', 'one_row', 'gap'][i % 10]
        L = 1 if kind == 'one_row' else int(rng.randint(2, 41))
        seconds = float(rng.uniform(0.3, 2.5))
        cuts = np.sort(rng.uniform(0, seconds, size=L - 1))
        bounds = np.concatenate(([0.], cuts, [seconds]))
        # rows shorter than 1.2 half-windows are widened (the caller of the reference asserts that), except where wanted
        min_dur = 1.2 * fl / 2 / sr
        for k in range(1, L + 1):
            bounds[k] = max(bounds[k], bounds[k - 1] + min_dur)
        bounds = np.round(bounds, 4)
        n = int(bounds[-1] * sr) + int(rng.randint(0, 2))
        spans = [[float(bounds[k]), float(bounds[k + 1])] for k in range(L)]
        if kind == 'wav_short':                       # the audio ends before the markers do: rows past the last frame
            n = max(fl // 2 + 1, n - int(rng.randint(1, 12)) * hop * int(rng.randint(1, 4)))
        elif kind == 'wav_long':                      # ... and after them: the rows run out
            n += int(rng.randint(1, 6)) * hop
        elif kind == 'sub_window':
            n = int(rng.randint(1, fl + hop))
        elif kind == 'near_threshold':                # one phone of about half a window
            k = int(rng.randint(0, L))
            width = round(fl / 2 / sr + float(rng.uniform(-2e-3, 2e-3)), 4)
            shift = width - (spans[k][1] - spans[k][0])
            spans[k][1] = round(spans[k][0] + width, 4)
            for j in range(k + 1, L):
                spans[j] = [round(spans[j][0] + shift, 4), round(spans[j][1] + shift, 4)]
            n = int(spans[-1][1] * sr)
        elif kind == 'zero_row':
            k = int(rng.randint(0, L))
            spans[k][1] = spans[k][0]
        elif kind == 'gap' and L > 2:                 # rows that do not touch
            k = int(rng.randint(1, L - 1))
            spans[k][0] = round(spans[k][0] + 0.4 * (spans[k][1] - spans[k][0]), 4)
        cases.append((c, centered, spans, int(n)))
    return cases


def record_durations(rng):
    from daft_exprt.extract_features import duration_to_integer
    out = []
    for c, centered, spans, n in duration_cases(rng):
        hp = types.SimpleNamespace(centered=centered, **CONFIGS[c])
        fl, hop = hp.filter_length, hp.hop_length
        try:
            durations = duration_to_integer([list(s) for s in spans], hp, nb_samples=n)
            mel_frames = 1 + n // hop if centered else (1 + (n - fl) // hop if n >= fl else 0)
            ok = len(durations) == len(spans) and sum(durations) == mel_frames and 0 not in durations   # its caller's asserts
            status = 0 if ok else 3
        except IndexError:
            durations, status = [], 1
        except ValueError:
            durations, status = [], 2
        out.append({'config': c, 'centered': centered, 'spans': spans, 'n_samples': n, 'durations': [int(d) for d in durations],
                    'status': status})
    return out


# ---- update_markers -----------------------------------------------------------------------------------------------------------

SENTENCES = [
    # (sentence, words of the markers in order; '<sil>' rows where the aligner found a pause)
    (",THAT's, an example'! ' of a sentence. . .'", ['that', 's', 'an', 'example', '<sil>', 'of', 'a', 'sentence']),
    ('Hello world.', ['hello', 'world']),
    ('Hello world', ['hello', 'world']),
    ('Hello, world!', ['hello', '<sil>', 'world']),
    ('Hello, world!', ['hello', 'world']),
    ('Hello world?', ['hello', '<sil>', 'world']),
    ('...Well, well, well.', ['well', '<sil>', 'well', 'well']),
    ('!? What is this?!', ['what', 'is', 'this']),
    ('What is this?!.', ['what', 'is', '<sil>', 'this']),
    ("That's all.", ['that', 's', 'all']),
    ("That's all.", ["that's", 'all']),
    ("It is an example' of it", ['it', 'is', 'an', 'example', 'of', 'it']),
    ("It is an example' of it", ['it', 'is', 'an', "example'", 'of', 'it']),
    ("'Tis the season", ['tis', 'the', 'season']),
    ("Dogs' bones, cats' toys.", ['dogs', 'bones', '<sil>', 'cats', 'toys']),
    ("I can't, I won't!", ['i', 'can', 't', '<sil>', 'i', 'won', 't']),
    ("I can't, I won't!", ['i', "can't", 'i', "won't"]),
    ('One. Two. Three.', ['one', '<sil>', 'two', '<sil>', 'three']),
    ('One. Two. Three.', ['one', 'two', 'three']),
    ('Single', ['single']),
    ('Single!', ['single']),
    ('  Leading spaces and trailing   ', ['leading', 'spaces', 'and', 'trailing']),
    ('UPPER lower MiXeD', ['upper', 'lower', 'mixed']),
    ('Numbers 42 stay out', ['numbers', 'stay', 'out']),
    ('A dash - is dropped', ['a', 'dash', 'is', 'dropped']),
    ('Quote "inside" here.', ['quote', 'inside', 'here']),
    ('Semi; colon: gone', ['semi', 'colon', 'gone']),
    ('Wait; what?', ['wait', '<sil>', 'what']),
    ('Under_score word', ['under_score', 'word']),
    ('Yes! Yes, yes?', ['yes', '<sil>', 'yes', '<sil>', 'yes']),
    ('A b c d e f g', ['a', 'b', '<sil>', 'c', 'd', 'e', '<sil>', 'f', 'g']),
    ('The end, my friend. ', ['the', 'end', 'my', 'friend']),
    ("Rock 'n' roll!", ['rock', 'n', 'roll']),
    ("O'Neil's car", ['o', 'neil', 's', 'car']),
    ('Comma , spaced', ['comma', 'spaced']),
    ('Fin.!?,', ['fin']),
    ('Two  words', ['two', '<sil>', 'words']),
    ('Good morning, everyone.', ['good', 'morning', '<sil>', 'everyone']),
    # two that cannot be matched
    ('Hello there world.', ['hello', 'world']),
    ('A completely different line', ['a', 'completly', 'different', 'line']),
]
PHONES = ['AH0', 'B', 'K', 'IY1', 'S', 'T', 'OW2', 'N', 'M', 'ER0']


def marker_lines(words, rng):
    ''' aligner rows `begin end phone word word_idx` with 1 - 3 phones per word, one SIL phone per <sil>, from a random begin '''
    t = round(float(rng.uniform(0.05, 0.9)), 4)
    lines, durations = [], []
    for idx, word in enumerate(words):
        for _ in range(1 if word == '<sil>' else int(rng.randint(1, 4))):
            end = round(t + float(rng.uniform(0.03, 0.2)), 4)
            phone = 'SIL' if word == '<sil>' else PHONES[int(rng.randint(0, len(PHONES)))]
            lines.append(f'{t}\t{end}\t{phone}\t{word}\t{idx}\n')
            durations.append(int(rng.randint(1, 18)))
            t = end
    return lines, durations


def record_markers(rng):
    from daft_exprt.extract_features import update_markers
    hp = types.SimpleNamespace(language='english')
    logger = logging.getLogger('gen_golden_features')
    out = []
    for i, (sentence, words) in enumerate(SENTENCES):
        lines, durations = marker_lines(words, rng)
        sent_begin = float(lines[0].split('\t')[0])
        expect = update_markers(f'case{i:02d}', list(lines), sentence, sent_begin, list(durations), hp, logger)
        out.append({'sentence': sentence, 'lines': lines, 'sent_begin': sent_begin, 'int_durations': durations, 'expect': expect})
    assert sum(case['expect'] is None for case in out) == 2
    return out


# ---- pooling ------------------------------------------------------------------------------------------------------------------

def record_pooling(rng):
    from daft_exprt.extract_features import get_symbols_energy, get_symbols_pitch
    out = []
    for durations in ([3, 0, 1, 5, 0, 0, 2, 1], [1, 1, 1, 1], [70, 0, 3], [4, 6, 0], [0, 2, 0, 9, 1, 0], [12]):
        T = sum(durations)
        energy = np.round(rng.uniform(0.5, 40., size=T), 3).astype(np.float32)
        pitch = np.round(np.where(rng.rand(T) < 0.35, 0., rng.uniform(4.2, 5.8, size=T)), 3).astype(np.float32)
        first = [sum(durations[:k]) for k in range(len(durations))]
        row = int(np.argmax(durations))
        if len(out) % 2 == 0:                         # a row of unvoiced frames only
            pitch[first[row]: first[row] + durations[row]] = 0.
        markers = [['0.000', '0.000', str(d), 'AH0', 'w', '0'] for d in durations]
        out.append({'durations': durations, 'energy': [float(f'{v:.3f}') for v in energy], 'pitch': [float(f'{v:.3f}') for v in pitch],
                    'symbols_energy': get_symbols_energy(energy, markers), 'symbols_pitch': get_symbols_pitch(pitch, markers)})
    return out


# ---- create_sets and stats ------------------------------------------------------------------------------------------------------

def record_sets_and_stats(rng):
    from daft_exprt.create_sets import create_sets
    from daft_exprt.features_stats import extract_features_stats
    speakers = {'spkA': [f'a{k:02d}' for k in range(8)], 'spkB/sub': [f'b{k:02d}' for k in range(6)]}
    without_npy = {'a03', 'b05'}                       # in metadata.csv, not extracted: 12 files are left
    symbols = ['_', '~', ' ', ',', '.', '!', '?'] + PHONES
    record = {'speakers': list(speakers), 'metadata': speakers, 'without_npy': sorted(without_npy), 'symbols': symbols, 'files': {}}
    with tempfile.TemporaryDirectory() as tmp:
        features = os.path.join(tmp, 'features')
        for speaker, names in speakers.items():
            os.makedirs(os.path.join(features, speaker))
            with open(os.path.join(features, speaker, 'metadata.csv'), 'w', encoding='utf-8') as f:
                f.writelines(f'{name}|some text\n' for name in names)
            for name in names:
                if name in without_npy:
                    continue
                L = int(rng.randint(3, 9))
                base = os.path.join(features, speaker, name)
                np.save(base + '.npy', np.zeros((2, 2), dtype=np.float32))
                t, rows = 0., []
                for _ in range(L):
                    end = t + (0. if rng.rand() < 0.2 else float(rng.uniform(0.03, 0.3)))
                    rows.append(f'{t:.3f}\t{end:.3f}\t1\t{symbols[int(rng.randint(1, len(symbols)))]}\tw\t0\n')
                    t = end
                texts = {'.markers': ''.join(rows),
                         '.symbols_nrg': ''.join(f'{v:.3f}\n' for v in np.where(rng.rand(L) < 0.25, 0., rng.uniform(1, 40, size=L))),
                         '.symbols_f0': ''.join(f'{v:.3f}\n' for v in np.where(rng.rand(L) < 0.3, 0., rng.uniform(4.2, 5.8, size=L)))}
                for ext, text in texts.items():
                    with open(base + ext, 'w', encoding='utf-8') as f:
                        f.write(text)
                record['files'][f'{speaker}/{name}'] = texts
        hp = types.SimpleNamespace(speakers=list(speakers), speakers_id=[0, 1], symbols=symbols,
                                   training_files=os.path.join(tmp, 'lists', 'train.txt'),
                                   validation_files=os.path.join(tmp, 'lists', 'validation.txt'))
        record['sets'] = {}
        for proportion in (50, 10):                   # 10 last: the stats below are taken over its training list
            create_sets(features, hp, proportion_validation=proportion)
            lists = {}
            for key, path in (('training', hp.training_files), ('validation', hp.validation_files)):
                with open(path, 'r', encoding='utf-8') as f:
                    lists[key] = [line.replace(features + os.sep, '') for line in f.readlines()]
            record['sets'][str(proportion)] = lists
        stats = extract_features_stats(hp, 1)
        record['stats'] = json.loads(json.dumps(stats))
    return record


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--reference', required=True, help='the src/ directory of a checkout of the reference')
    args = parser.parse_args()
    install_shims(args.reference)
    rng = np.random.RandomState(20240521)
    golden = {'configs': CONFIGS, 'durations': record_durations(rng), 'markers': record_markers(rng), 'pooling': record_pooling(rng)}
    golden.update(record_sets_and_stats(rng))
    with open(OUT, 'w', encoding='utf-8') as f:
        json.dump(golden, f, separators=(',', ':'))
    by_status = np.bincount([case['status'] for case in golden['durations']], minlength=4)
    print(f'{OUT}: {os.path.getsize(OUT)} bytes; duration cases by status {by_status.tolist()}')


if __name__ == '__main__':
    main()
