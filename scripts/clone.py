#!/usr/bin/env python
"""Prosody cloning: speak sentences with the timing, loudness and intonation of recordings of the same sentences:
    python scripts/clone.py -chk CHECKPOINT -tf PHONEMISED -wd WAV_DIR -spk SPEAKER [SPEAKER ...] -out OUT_DIR [-bs 32]
                            [--aligner PATH] [--clone dur,energy,pitch] [--normalise self|source|target] [-src SPEAKER ...]
                            [-voc G_CKPT [-vcfg JSON]] [-mf 3] [-trim -40]

  -chk   training checkpoint: weights, hyper-parameters and speaker statistics, as for `scripts/synthesize.py`
  -tf    phonemised sentences, `NAME|{P1 P2} {P3} , {P4} ? ~` per line as for `scripts/synthesize.py`
  -wd    directory with `NAME.wav` for every sentence: a recording of that sentence by anybody, at any sampling rate
  -spk   who speaks: ids or names of the checkpoint's speakers, one for all the sentences or one per sentence
  -src   who was recorded (default: the same as -spk): used by the synthesis-based alignment and by --normalise source
  --aligner    a learned aligner (`scripts/train_aligner.py`) for the phoneme boundaries; default: the checkpoint's own synthesis
               warped onto the recording (`daft_exprt/align.py`)
  --clone      which of the recording's per-symbol quantities are imposed (default all three).  With `dur` the output has the
               recording's frame counts, symbol by symbol
  --normalise  the statistics that turn the recording's energy and pitch into the model's units: `self` the recording's own (the
               contour relative to itself; default), `source` the recorded speaker's, `target` the speaking speaker's (same Hz)
  -voc / -vcfg a HiFi-GAN generator checkpoint and its config: `NAME.wav` is then its audio (16-bit PCM); default: the Griffin-Lim
               preview (64-bit float)
  -mf / -trim  as for `scripts/align.py`: fewest frames of a sounding symbol, silence threshold below the peak in dB

Writes `<out>/NAME.npz` (key `mel_spec`) and `<out>/NAME.wav` as `scripts/synthesize.py` does, and `<out>/clone_report.json`: per
file the alignment's status, frames, begin, moved and path_cost, `dropped`, `pool_status`, `usable`, `frame_exact` and the scores against the recording
(`mcd_db`, `f0_rmse_cents`, `vuv_error` frame against frame, `pitch_pcc`, `energy_pcc`; null where undefined), and a summary with
the count per status and the means over the scored files.  A recording that could not be aligned (status != 0) is synthesised
free-running and reported (`usable` false; `pool_status` 1 where an aligned recording's rows overran its curves), never cloned.  How close cloned speech sounds to the recording on real data has not been measured."""
import argparse
import logging
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'ubisoft-laforge-daft-exprt_amd')
sys.path.insert(0, PKG)

_logger = logging.getLogger('clone')
QUANTITIES = ('dur', 'energy', 'pitch')


def _quantities(text):
    what = tuple(q.strip() for q in text.split(',') if q.strip())
    if not what or any(q not in QUANTITIES for q in what) or len(set(what)) != len(what):
        raise argparse.ArgumentTypeError(f'"{text}": a comma-separated subset of {",".join(QUANTITIES)}')
    return what


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description='Synthesise sentences with the per-symbol prosody of recordings of the same sentences')
    parser.add_argument('-chk', '--checkpoint', required=True, help='training checkpoint (weights, hyper-parameters, statistics)')
    parser.add_argument('-tf', '--text_file', required=True, help='phonemised sentences: NAME|{P1 P2} {P3} , {P4} ? ~ per line')
    parser.add_argument('-wd', '--wav_dir', required=True, help='directory with NAME.wav for every sentence (any rate)')
    parser.add_argument('-spk', '--speakers', nargs='+', required=True, help='target speaker ids or names: one, or one per sentence')
    parser.add_argument('-src', '--source_speakers', nargs='+', default=None, help='recorded speakers (default: the targets)')
    parser.add_argument('-out', '--output_dir', required=True, help='where the .npz, .wav and clone_report.json go')
    parser.add_argument('-bs', '--batch_size', type=int, default=32, help='sentences per batch')
    parser.add_argument('--aligner', default=None, help='learned aligner checkpoint (default: align with the checkpoint itself)')
    parser.add_argument('--clone', type=_quantities, default=QUANTITIES, help='quantities to impose: dur,energy,pitch')
    parser.add_argument('--normalise', choices=('self', 'source', 'target'), default='self', help='statistics of the energy / pitch targets')
    parser.add_argument('-voc', '--vocoder', default=None, help='HiFi-GAN or BigVGAN generator checkpoint (default: Griffin-Lim preview)')
    parser.add_argument('-vcfg', '--vocoder_config', default=None, help='its config.json (default: beside the vocoder checkpoint)')
    parser.add_argument('-mf', '--min_frames', type=int, default=3, help='fewest frames of a sounding symbol')
    parser.add_argument('-trim', '--trim_db', type=float, default=-40.0, help='silence threshold below the peak frame energy, dB (<= 0)')
    return parser.parse_args(argv)


def check_args(args):
    ''' the mistakes that can be told before the checkpoint is loaded; SystemExit naming the flag '''
    files = [('checkpoint', args.checkpoint), ('phonemised file', args.text_file)]
    files += [('aligner', args.aligner)] if args.aligner else []
    files += [('vocoder checkpoint', args.vocoder)] if args.vocoder else []
    for what, path in files:
        if not os.path.isfile(path):
            raise SystemExit(f'clone.py: no such {what}: {path}')
    if not os.path.isdir(args.wav_dir):
        raise SystemExit(f'clone.py: no such recordings directory: {args.wav_dir}')
    if args.batch_size < 1 or args.min_frames < 1 or args.trim_db > 0:
        raise SystemExit(f'clone.py: -bs {args.batch_size} and -mf {args.min_frames} must be at least 1, -trim {args.trim_db} at most 0')


def speaker_ids(given, n, hparams, flag):
    ''' n speaker ids from the flag's values -- ids or names of the checkpoint's speakers, one for all or one per sentence '''
    if len(given) not in (1, n):
        raise SystemExit(f'clone.py: {flag} takes one speaker, or one per sentence: {len(given)} for {n} sentences')
    ids = []
    for s in given:
        if s in hparams.speakers:
            ids.append(int(hparams.speakers_id[hparams.speakers.index(s)]))
        elif s.lstrip('-').isdigit() and int(s) in [int(i) for i in hparams.speakers_id]:
            ids.append(int(s))
        else:
            raise SystemExit(f'clone.py: {flag} {s}: the checkpoint knows the speakers {hparams.speakers} with the ids {list(hparams.speakers_id)}')
    return ids * n if len(ids) == 1 else ids


def main(argv=None):
    args = parse_args(argv)
    logging.basicConfig(format='%(asctime)s [%(levelname)s] %(message)s', datefmt='%Y-%m-%d %H:%M:%S', level=logging.INFO)
    check_args(args)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from synthesize import load_model, load_vocoder
    from daft_exprt.clone import clone_files
    from daft_exprt.generate import read_phonemised_sentences
    model, hparams = load_model(args.checkpoint)
    sentences, names = read_phonemised_sentences(args.text_file, hparams.symbols)
    wav_files = [os.path.join(args.wav_dir, f'{name}.wav') for name in names]
    missing = [path for path in wav_files if not os.path.isfile(path)]
    if missing:
        raise SystemExit(f'clone.py: no recording for {len(missing)} sentences, the first: {missing[0]}')
    targets = speaker_ids(args.speakers, len(names), hparams, '-spk')
    sources = targets if args.source_speakers is None else speaker_ids(args.source_speakers, len(names), hparams, '-src')
    aligner = None
    if args.aligner:
        from daft_exprt.aligner import load_aligner
        aligner = load_aligner(args.aligner)
    vocoder = load_vocoder(args.vocoder, args.vocoder_config, hparams) if args.vocoder else None
    report = clone_files(model, sentences, names, wav_files, targets, args.output_dir, hparams, aligner=aligner, source_speaker_ids=sources,
                         what=args.clone, normalise=args.normalise, batch_size=args.batch_size, vocoder=vocoder,
                         min_frames=args.min_frames, trim_db=args.trim_db)
    for name, record in report['files'].items():
        if not record['usable']:
            _logger.info(f'{name}: status {record["status"]}, pool_status {record["pool_status"]}, synthesised free-running')


if __name__ == '__main__':
    main()
