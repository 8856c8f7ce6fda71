#!/usr/bin/env python
"""Copy-synthesis scores of a checkpoint against held-out recordings of the same text:
    python scripts/evaluate.py -chk CHECKPOINT -vf FILE_LIST -out OUT_DIR [-bs 50] [-voc G_CKPT [-vcfg JSON]] [-n MAX_UTTERANCES] [-nc 13]
                               [-rec RECOGNIZER] [-spk SPEAKER_ENCODER]

  -chk  training checkpoint: weights, hyper-parameters and speaker statistics, as for `scripts/synthesize.py`
  -vf   a `features_dir|feature_file|speaker_id` list, e.g. the validation list `scripts/pre_process.py` writes; read through
        `DaftExprtDataLoader` and its collate, in the list's order
  -voc  a HiFi-GAN generator checkpoint (-vcfg its `config.json`, default: the one beside it): the `audio` level scores its
        waveform instead of the Griffin-Lim preview
  -n    score the first N utterances of the list only
  -nc   cepstral coefficients 1..K of the distortion (default 13)
  -rec  a phone recogniser (`scripts/train_recognizer.py`): every file also gets `per`, the phone error rate of the recogniser's
        decode against the file's own phones at three levels -- `recording` (the recorded mel: the recogniser's own floor on that
        utterance), `mel` (the decoder's mel) and `audio` (the re-analysed waveform) -- each with sub, del, ins, n_ref, per and n_hyp;
        the summaries get per level the statistics of those keys and `rate`, the summed errors over the summed reference length.
        Without -rec the report is what it always was.  How the rate tracks listeners has not been measured
  -spk  a speaker encoder (`scripts/train_speaker_encoder.py`): every file also gets `speaker`, at the same three levels --
        `recording`, `mel`, `audio`; read them together -- the cosine of its embedding to the centroid of the file's own speaker
        (`cos_target`), that cosine minus the largest to any other centroid (`margin`), whether the nearest centroid is the file's
        speaker (`identified`) and whether cos_target reaches the encoder's threshold (`accepted`); the summaries get per level the
        statistics of the two cosines and the shares identified and accepted.  Without -spk the report is what it always was.
        How the cosines track listeners' judgement of speaker similarity has not been measured

Every utterance is synthesised free-running -- predicted durations, predicted prosody, decoder -- with its own recording as the
prosody reference and its own speaker, and compared with that recording after dynamic time warping (`daft_exprt/evaluate.py`,
`copy_synthesis_scores`).  `<out>/copy_synthesis.json` holds, per file, the speaker id and the scores at two levels -- `mel`: the
decoder's mel against the recorded mel (MCD, frame counts); `audio`: the vocoder's or Griffin-Lim's waveform analysed again
(MCD, F0 RMSE in cents, voicing error, voiced pairs, path length, frame counts); NaN is written as null -- and a `summary`: per
level and key the mean, the median and the count of the finite values, over all files and per speaker."""
import argparse
import json
import logging
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'ubisoft-laforge-daft-exprt_amd')
sys.path.insert(0, PKG)

_logger = logging.getLogger('evaluate')


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description='Score the free-running synthesis of a checkpoint against recordings of the same text')
    parser.add_argument('-chk', '--checkpoint', required=True, help='training checkpoint (weights, hyper-parameters, statistics)')
    parser.add_argument('-vf', '--validation_files', required=True, help='list of features_dir|feature_file|speaker_id lines')
    parser.add_argument('-out', '--output_dir', required=True, help='where copy_synthesis.json goes')
    parser.add_argument('-bs', '--batch_size', type=int, default=50, help='utterances per inference call')
    parser.add_argument('-voc', '--vocoder', default=None, help='HiFi-GAN or BigVGAN generator checkpoint: score its audio instead of the Griffin-Lim preview')
    parser.add_argument('-vcfg', '--vocoder_config', default=None, help='its config.json (default: beside the vocoder checkpoint)')
    parser.add_argument('-n', '--max_utterances', type=int, default=None, help='score the first N utterances of the list only')
    parser.add_argument('-nc', '--n_coeffs', type=int, default=13, help='cepstral coefficients 1..K of the distortion')
    parser.add_argument('-rec', '--recognizer', default=None, help='phone recogniser (scripts/train_recognizer.py): add phone error rates')
    parser.add_argument('-spk', '--speaker_encoder', default=None, help='speaker encoder (scripts/train_speaker_encoder.py): add speaker scores')
    return parser.parse_args(argv)


def score_files(model, hparams, list_file, batch_size, vocoder=None, max_utterances=None, n_coeffs=13, recognizer=None,
                speaker_encoder=None):
    ''' {file: {'speaker_id': id, 'mel': {key: value}, 'audio': {key: value}}} in the list's order; floats may be NaN.  With a
        recogniser every file also has 'per': {level: {key: value}} for `evaluate.PER_LEVELS` and `recognizer.PER_KEYS`; with a
        speaker encoder 'speaker': {level: {key: value}} for `evaluate.SPEAKER_LEVELS` and `speaker.SPEAKER_KEYS` '''
    from daft_exprt.data_loader import DaftExprtDataCollate, DaftExprtDataLoader
    from daft_exprt.evaluate import COPY_LEVELS, DTW_KEYS, PER_LEVELS, SPEAKER_LEVELS, copy_synthesis_scores
    from daft_exprt.recognizer import PER_KEYS, per_to_host
    from daft_exprt.speaker import SPEAKER_KEYS, scores_to_host
    more = {} if speaker_encoder is None else {'speaker_encoder': speaker_encoder}     # (without one the call is the one it always was)
    dataset = DaftExprtDataLoader(list_file, hparams, shuffle=False)
    collate = DaftExprtDataCollate(hparams)
    count = len(dataset) if max_utterances is None else min(len(dataset), max(0, max_utterances))
    records = {}
    for start in range(0, count, batch_size):
        batch = collate([dataset[i] for i in range(start, min(count, start + batch_size))])
        scores = copy_synthesis_scores(model, batch, hparams, vocoder=vocoder, n_coeffs=n_coeffs, recognizer=recognizer, **more)
        host = {level: {key: scores[level][key].cpu().tolist() for key in DTW_KEYS} for level in COPY_LEVELS}
        per = {level: per_to_host(scores['per'][level]) for level in PER_LEVELS} if recognizer is not None else None
        spk = {level: scores_to_host(scores['speaker'][level]) for level in SPEAKER_LEVELS} if speaker_encoder is not None else None
        for row, (features_dir, feature_file) in enumerate(zip(batch[11], batch[12])):
            name = f'{os.path.basename(os.path.normpath(features_dir))}/{feature_file}'
            records[name] = {'speaker_id': int(batch[10][row]),
                             **{level: {key: host[level][key][row] for key in DTW_KEYS} for level in COPY_LEVELS}}
            if per is not None:
                records[name]['per'] = {level: {key: per[level][key][row] for key in PER_KEYS} for level in PER_LEVELS}
            if spk is not None:
                records[name]['speaker'] = {level: {key: spk[level][key][row] for key in SPEAKER_KEYS} for level in SPEAKER_LEVELS}
    order = {f'{os.path.basename(os.path.normpath(line[0]))}/{line[1]}': i for i, line in enumerate(dataset.data)}
    return dict(sorted(records.items(), key=lambda item: order[item[0]]))


def _stats(values):
    finite = [float(v) for v in values if v is not None and math.isfinite(v)]
    return {'mean': statistics.fmean(finite) if finite else None, 'median': statistics.median(finite) if finite else None,
            'count': len(finite)}


def summarise(records, levels, keys):
    ''' per level and key the mean, median and count of the finite values: over all files, and per speaker '''
    def table(entries):
        out = {level: {key: _stats([e[level][key] for e in entries]) for key in keys} for level in levels}
        if entries and 'per' in entries[0]:     # (-rec) per level the statistics of every key, and the corpus-level rate
            out['per'] = {}
            for level in entries[0]['per']:
                rows = [e['per'][level] for e in entries]
                n_ref = sum(r['n_ref'] for r in rows)
                out['per'][level] = {**{key: _stats([r[key] for r in rows]) for key in rows[0]},
                                     'rate': sum(r['sub'] + r['del'] + r['ins'] for r in rows) / n_ref if n_ref else None}
        if entries and 'speaker' in entries[0]:  # (-spk) per level the statistics of the cosines and the shares identified / accepted
            out['speaker'] = {}
            for level in entries[0]['speaker']:
                rows = [e['speaker'][level] for e in entries]
                out['speaker'][level] = {key: sum(bool(r[key]) for r in rows) / len(rows) if key in ('identified', 'accepted')
                                         else _stats([r[key] for r in rows]) for key in rows[0]}
        return out
    summary = {'files': len(records), **table(list(records.values())), 'speakers': {}}
    for speaker in sorted({e['speaker_id'] for e in records.values()}):
        mine = [e for e in records.values() if e['speaker_id'] == speaker]
        summary['speakers'][str(speaker)] = {'files': len(mine), **table(mine)}
    return summary


def write_report(output_dir, records, audio, levels, keys):
    ''' `<out>/copy_synthesis.json`: {'audio': which waveform was scored, 'files': records, 'summary': ...}; NaN becomes null '''
    def clean(v):
        return None if isinstance(v, float) and not math.isfinite(v) else v
    files = {name: {'speaker_id': e['speaker_id'], **{level: {k: clean(v) for k, v in e[level].items()} for level in levels}}
             for name, e in records.items()}
    for name, e in records.items():
        if 'per' in e:
            files[name]['per'] = {level: {k: clean(v) for k, v in values.items()} for level, values in e['per'].items()}
        if 'speaker' in e:
            files[name]['speaker'] = {level: {k: clean(v) for k, v in values.items()} for level, values in e['speaker'].items()}
    report = {'audio': audio, 'files': files, 'summary': summarise(files, levels, keys)}
    os.makedirs(output_dir, exist_ok=True)
    path = os.path.join(output_dir, 'copy_synthesis.json')
    with open(path, 'w', encoding='utf-8') as f:
        json.dump(report, f, indent=1)
    for level in levels:
        for key in ('mcd_db', 'f0_rmse_cents', 'vuv_error'):
            s = report['summary'][level][key]
            if s['count']:
                _logger.info(f'{level} {key}: mean {s["mean"]:.3f}, median {s["median"]:.3f} over {s["count"]} of {len(files)} files')
            else:
                _logger.info(f'{level} {key}: undefined for all {len(files)} files')
    for level, s in report['summary'].get('per', {}).items():
        _logger.info(f'{level} phone error rate: {s["rate"]} over {len(files)} files')
    for level, s in report['summary'].get('speaker', {}).items():
        _logger.info(f'{level} speaker: identified {s["identified"]:.3f}, accepted {s["accepted"]:.3f}, mean cosine to the own centroid '
                     f'{s["cos_target"]["mean"]} over {len(files)} files')
    _logger.info(f'Copy-synthesis scores written to {path}')
    return report


def main(argv=None):
    args = parse_args(argv)
    logging.basicConfig(format='%(asctime)s [%(levelname)s] %(message)s', datefmt='%Y-%m-%d %H:%M:%S', level=logging.INFO)
    for what, path in (('checkpoint', args.checkpoint), ('file list', args.validation_files), ('vocoder checkpoint', args.vocoder),
                       ('recogniser', args.recognizer), ('speaker encoder', args.speaker_encoder)):
        if path is not None and not os.path.isfile(path):
            raise SystemExit(f'evaluate.py: no such {what}: {path}')
    if args.batch_size < 1:
        raise SystemExit(f'evaluate.py: -bs {args.batch_size}: at least one utterance per batch')

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from synthesize import load_model, load_vocoder
    from daft_exprt.evaluate import COPY_LEVELS, DTW_KEYS
    model, hparams = load_model(args.checkpoint)
    vocoder = load_vocoder(args.vocoder, args.vocoder_config, hparams) if args.vocoder else None
    recognizer = None
    if args.recognizer is not None:
        from daft_exprt.recognizer import load_recognizer
        recognizer = load_recognizer(args.recognizer)
    speaker_encoder = None
    if args.speaker_encoder is not None:
        from daft_exprt.speaker import load_speaker_encoder
        speaker_encoder = load_speaker_encoder(args.speaker_encoder)
    records = score_files(model, hparams, args.validation_files, args.batch_size, vocoder, args.max_utterances, args.n_coeffs, recognizer,
                          speaker_encoder)
    write_report(args.output_dir, records, 'hifi-gan' if vocoder is not None else 'griffin-lim', COPY_LEVELS, DTW_KEYS)


if __name__ == '__main__':
    main()
