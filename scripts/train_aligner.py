#!/usr/bin/env python
"""Phoneme boundaries for a new corpus with nothing but the corpus: train an aligner on it, then write the .markers
    python scripts/train_aligner.py -dd DATASET_DIR -spks SPEAKER [SPEAKER ...] -tf PHONEMISED [PHONEMISED ...] -o ALIGNER.pt
                                    [-st 2000] [-bs 32] [-lr 1e-3] [-mf 3] [-trim -40] [-lg english] [--overwrite]

  -dd    data set directory: `<dd>/<speaker>/wavs/NAME.wav` and `<dd>/<speaker>/align/NAME.lab` (the sentence as text)
  -spks  speakers to train on and to align (any names: the aligner is not conditioned on the speaker)
  -tf    phonemised sentences, `NAME|{P1 P2} {P3} , {P4} ? ~` per line as for `scripts/synthesize.py`: one file for all the speakers,
         or one per speaker in the order of -spks
  -o     where the trained aligner is saved (weights and constructor arguments, `daft_exprt.aligner.load_aligner` reads it)
  -st    Adam steps;  -bs utterances per step and per alignment call;  -lr learning rate
  -mf    fewest frames a symbol keeps (default 3: more than half an analysis window, which `extract_features` asks of every phone)
  -trim  level below the peak frame energy, in dB, under which the ends of a recording count as silence (default -40)

The aligner (`daft_exprt/aligner.py`: a text and a mel encoder, their soft alignment, the forward-sum loss, monotonic alignment
search) is trained on the sounding stretches of the recordings, saved, and then `<dd>/<speaker>/align/NAME.markers` is written for
every utterance that has none (or for all with --overwrite), in the format `scripts/pre_process.py` reads, with
`<dd>/align_report.json` as `scripts/align.py` writes it (path_cost is the negative alignment score per frame).  How close the
boundaries come to a trained forced aligner's on real speech has not been measured: look at the files with the most moved
boundaries and the highest path cost first."""
import argparse
import logging
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'ubisoft-laforge-daft-exprt_amd')
sys.path.insert(0, PKG)

_logger = logging.getLogger('train_aligner')


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description='Train an aligner on a data set and write its .markers files')
    parser.add_argument('-dd', '--data_set_dir', required=True, help='data set directory: <speaker>/wavs/*.wav and <speaker>/align/*.lab')
    parser.add_argument('-spks', '--speakers', nargs='+', required=True, help='speakers to train on and to align')
    parser.add_argument('-tf', '--text_file', nargs='+', required=True, help='phonemised sentences: one file for all speakers, or one per speaker')
    parser.add_argument('-o', '--output', required=True, help='file the trained aligner is saved to')
    parser.add_argument('-st', '--steps', type=int, default=2000, help='Adam steps')
    parser.add_argument('-bs', '--batch_size', type=int, default=32, help='utterances per step and per alignment call')
    parser.add_argument('-lr', '--learning_rate', type=float, default=1e-3, help='Adam learning rate')
    parser.add_argument('-mf', '--min_frames', type=int, default=3, help='fewest frames of a symbol')
    parser.add_argument('-trim', '--trim_db', type=float, default=-40.0, help='silence threshold below the peak frame energy, dB (<= 0)')
    parser.add_argument('-lg', '--language', type=str, default='english', help='language of the symbol set')
    parser.add_argument('--seed', type=int, default=1234, help='seed of the initial weights and of the batches')
    parser.add_argument('--overwrite', action='store_true', help='write .markers even where one exists')
    return parser.parse_args(argv)


def check_args(args):
    ''' the mistakes that can be told before anything is read; SystemExit naming the flag '''
    for path in args.text_file:
        if not os.path.isfile(path):
            raise SystemExit(f'train_aligner.py: no such phonemised file: {path}')
    if not os.path.isdir(args.data_set_dir):
        raise SystemExit(f'train_aligner.py: no such data set directory: {args.data_set_dir}')
    if len(args.text_file) not in (1, len(args.speakers)):
        raise SystemExit(f'train_aligner.py: -tf takes one file, or one per speaker: {len(args.text_file)} files for '
                         f'{len(args.speakers)} speakers')
    if args.batch_size < 1 or args.min_frames < 1 or args.trim_db > 0:
        raise SystemExit(f'train_aligner.py: -bs {args.batch_size} and -mf {args.min_frames} must be at least 1, -trim {args.trim_db} '
                         f'at most 0')
    if args.steps < 1 or not args.learning_rate > 0:
        raise SystemExit(f'train_aligner.py: -st {args.steps} must be at least 1 and -lr {args.learning_rate} positive')
    out_dir = os.path.dirname(os.path.abspath(args.output))
    if not os.path.isdir(out_dir):
        raise SystemExit(f'train_aligner.py: no such directory for -o: {out_dir}')


def main(argv=None):
    args = parse_args(argv)
    logging.basicConfig(format='%(asctime)s [%(levelname)s] %(message)s', datefmt='%Y-%m-%d %H:%M:%S', level=logging.INFO)
    check_args(args)
    from daft_exprt.align import align_data_set
    from daft_exprt.aligner import save_aligner, train_aligner
    from daft_exprt.hparams import HyperParams
    hparams = HyperParams(verbose=False, training_files='none', validation_files='none', output_directory=os.path.dirname(
        os.path.abspath(args.output)), language=args.language, speakers=list(args.speakers))
    files = args.text_file[0] if len(args.text_file) == 1 else args.text_file
    aligner = train_aligner(args.data_set_dir, args.speakers, files, hparams, steps=args.steps, batch_size=args.batch_size,
                            lr=args.learning_rate, seed=args.seed, trim_db=args.trim_db)
    save_aligner(aligner, args.output)
    _logger.info(f'aligner saved to {args.output}')
    report = align_data_set(args.data_set_dir, args.speakers, files, aligner, hparams, batch_size=args.batch_size,
                            min_frames=args.min_frames, trim_db=args.trim_db, overwrite=args.overwrite)
    for speaker, name, reason in report['skipped']:
        _logger.info(f'skipped {speaker}/{name}: {reason}')


if __name__ == '__main__':
    main()
