#!/usr/bin/env python
"""Phoneme boundaries for new recordings, from a trained checkpoint instead of an external aligner:
    python scripts/align.py -chk CHECKPOINT -dd DATASET_DIR -spks SPEAKER [SPEAKER ...] -tf PHONEMISED [PHONEMISED ...]
                            [-bs 32] [-mf 3] [-trim -40] [--overwrite]

  -chk   training checkpoint: weights, hyper-parameters and speaker statistics, as for `scripts/synthesize.py`
  -dd    data set directory: `<dd>/<speaker>/wavs/NAME.wav` and `<dd>/<speaker>/align/NAME.lab` (the sentence as text)
  -spks  speakers to align; each must be one of the checkpoint's `speakers` -- its id is the one the trainer gave it
  -tf    phonemised sentences, `NAME|{P1 P2} {P3} , {P4} ? ~` per line as for `scripts/synthesize.py`: one file for all the speakers,
         or one per speaker in the order of -spks
  -mf    fewest frames a symbol that sounds in the synthesis keeps in the recording (default 3: more than half an analysis window,
         which `extract_features` asks of every phone)
  -trim  level below the peak frame energy, in dB, under which the ends of a recording count as silence (default -40)

Every recording is trimmed to its sounding stretch, synthesised free-running with itself as prosody reference, and the frames the
model gave each symbol are carried over a dynamic-time-warping path onto the recording (`daft_exprt/align.py`).
`<dd>/<speaker>/align/NAME.markers` is written for every utterance that has none (or for all with --overwrite), in the format
`scripts/pre_process.py` reads, and `<dd>/align_report.json` holds per file the status, how many boundaries the minimum-duration
repair moved, the mean cost along the path and the frame and symbol counts.  How close the boundaries come to a trained aligner's
on real speech has not been measured: look at the files with the most moved boundaries and the highest path cost first."""
import argparse
import logging
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'ubisoft-laforge-daft-exprt_amd')
sys.path.insert(0, PKG)

_logger = logging.getLogger('align')


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description='Write .markers files for recordings by DTW against the checkpoint\'s own synthesis')
    parser.add_argument('-chk', '--checkpoint', required=True, help='training checkpoint (weights, hyper-parameters, statistics)')
    parser.add_argument('-dd', '--data_set_dir', required=True, help='data set directory: <speaker>/wavs/*.wav and <speaker>/align/*.lab')
    parser.add_argument('-spks', '--speakers', nargs='+', required=True, help='speakers to align (names the checkpoint knows)')
    parser.add_argument('-tf', '--text_file', nargs='+', required=True, help='phonemised sentences: one file for all speakers, or one per speaker')
    parser.add_argument('-bs', '--batch_size', type=int, default=32, help='utterances per inference call')
    parser.add_argument('-mf', '--min_frames', type=int, default=3, help='fewest frames of a sounding symbol')
    parser.add_argument('-trim', '--trim_db', type=float, default=-40.0, help='silence threshold below the peak frame energy, dB (<= 0)')
    parser.add_argument('--overwrite', action='store_true', help='write .markers even where one exists')
    return parser.parse_args(argv)


def check_args(args):
    ''' the mistakes that can be told before the checkpoint is loaded; SystemExit naming the flag '''
    for what, path in [('checkpoint', args.checkpoint)] + [('phonemised file', path) for path in args.text_file]:
        if not os.path.isfile(path):
            raise SystemExit(f'align.py: no such {what}: {path}')
    if not os.path.isdir(args.data_set_dir):
        raise SystemExit(f'align.py: no such data set directory: {args.data_set_dir}')
    if len(args.text_file) not in (1, len(args.speakers)):
        raise SystemExit(f'align.py: -tf takes one file, or one per speaker: {len(args.text_file)} files for {len(args.speakers)} speakers')
    if args.batch_size < 1 or args.min_frames < 1 or args.trim_db > 0:
        raise SystemExit(f'align.py: -bs {args.batch_size} and -mf {args.min_frames} must be at least 1, -trim {args.trim_db} at most 0')


def main(argv=None):
    args = parse_args(argv)
    logging.basicConfig(format='%(asctime)s [%(levelname)s] %(message)s', datefmt='%Y-%m-%d %H:%M:%S', level=logging.INFO)
    check_args(args)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from synthesize import load_model
    from daft_exprt.align import align_data_set
    model, hparams = load_model(args.checkpoint)
    unknown = [speaker for speaker in args.speakers if speaker not in hparams.speakers]
    if unknown:
        raise SystemExit(f'align.py: the checkpoint has no speaker {unknown}: it knows {hparams.speakers}')
    files = args.text_file[0] if len(args.text_file) == 1 else args.text_file
    report = align_data_set(args.data_set_dir, args.speakers, files, model, hparams, batch_size=args.batch_size,
                            min_frames=args.min_frames, trim_db=args.trim_db, overwrite=args.overwrite)
    for speaker, name, reason in report['skipped']:
        _logger.info(f'skipped {speaker}/{name}: {reason}')


if __name__ == '__main__':
    main()
