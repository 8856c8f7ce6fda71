#!/usr/bin/env python
"""Train a grapheme-to-phoneme model on a pronunciation dictionary, for the words the dictionary lacks
    python scripts/train_g2p.py -dict DICTIONARY -o G2P.pt [-st 5000] [-bs 256] [-lr 2e-3] [-ho 0.05] [-hid 128] [-lg english]

  -dict  pronunciation dictionary: `word P1 P2 ...` per line (the Montreal Forced Aligner's format; CMUdict's `word(2)` variant
         marks and `;;;` comments are understood), the phones those of the symbol table
  -o     where the trained model is saved (weights and constructor arguments, `daft_exprt.g2p.load_g2p` reads it)
  -st    Adam steps;  -bs pronunciations per step;  -lr learning rate;  -hid width of the encoder
  -ho    share of the WORDS held out (with all their pronunciations) to measure the error rates

The model (`daft_exprt/g2p.py`: a convolutional grapheme encoder, three output slots per grapheme, CTC) is trained on the GPU and
saved; `g2p_report.json` beside it holds the report of `train_g2p` -- the held-out phone and word error rates, the rows skipped
for want of a CTC path -- and up to 20 held-out words with their decodes.  How accurate such a model is on a real dictionary has
not been measured: read the report."""
import argparse
import json
import logging
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'ubisoft-laforge-daft-exprt_amd')
sys.path.insert(0, PKG)

_logger = logging.getLogger('train_g2p')


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description='Train a g2p model on a pronunciation dictionary')
    parser.add_argument('-dict', '--dictionary', required=True, help='pronunciation dictionary: word P1 P2 ... per line')
    parser.add_argument('-o', '--output', required=True, help='file the trained g2p model is saved to')
    parser.add_argument('-st', '--steps', type=int, default=5000, help='Adam steps')
    parser.add_argument('-bs', '--batch_size', type=int, default=256, help='pronunciations per step')
    parser.add_argument('-lr', '--learning_rate', type=float, default=2e-3, help='Adam learning rate')
    parser.add_argument('-ho', '--held_out', type=float, default=0.05, help='share of the words held out for the report')
    parser.add_argument('-hid', '--hidden', type=int, default=128, help='width of the encoder')
    parser.add_argument('-lg', '--language', type=str, default='english', help='language of the symbol set')
    parser.add_argument('--seed', type=int, default=1234, help='seed of the initial weights, the split and the batches')
    return parser.parse_args(argv)


def check_args(args):
    ''' the mistakes that can be told before anything is read; SystemExit naming the flag '''
    if not os.path.isfile(args.dictionary):
        raise SystemExit(f'train_g2p.py: no such dictionary: {args.dictionary}')
    if args.steps < 1 or args.batch_size < 1 or not args.learning_rate > 0 or args.hidden < 1:
        raise SystemExit(f'train_g2p.py: -st {args.steps}, -bs {args.batch_size} and -hid {args.hidden} must be at least 1 and '
                         f'-lr {args.learning_rate} positive')
    if not 0 <= args.held_out < 1:
        raise SystemExit(f'train_g2p.py: -ho {args.held_out} must be in [0, 1)')
    out_dir = os.path.dirname(os.path.abspath(args.output))
    if not os.path.isdir(out_dir):
        raise SystemExit(f'train_g2p.py: no such directory for -o: {out_dir}')


def main(argv=None):
    args = parse_args(argv)
    logging.basicConfig(format='%(asctime)s [%(levelname)s] %(message)s', datefmt='%Y-%m-%d %H:%M:%S', level=logging.INFO)
    check_args(args)
    from daft_exprt.g2p import save_g2p, train_g2p
    from daft_exprt.hparams import HyperParams
    from daft_exprt.text import load_dictionary
    out_dir = os.path.dirname(os.path.abspath(args.output))
    hparams = HyperParams(verbose=False, training_files='none', validation_files='none', output_directory=out_dir,
                          language=args.language, speakers=['none'])
    dictionary = load_dictionary(args.dictionary, hparams.symbols)
    g2p, report = train_g2p(dictionary, hparams, steps=args.steps, batch_size=args.batch_size, lr=args.learning_rate, seed=args.seed,
                            held_out=args.held_out, hidden=args.hidden)
    save_g2p(g2p, args.output)
    _logger.info(f'g2p model saved to {args.output}')
    path = os.path.join(out_dir, 'g2p_report.json')
    with open(path, 'w', encoding='utf-8') as f:
        json.dump(report, f, indent=1)
    _logger.info(f'held-out phone error rate {report["phone_error_rate"]}, word error rate {report["word_error_rate"]}, '
                 f'{report["skipped_rows"]} rows skipped; report written to {path}')
    return report


if __name__ == '__main__':
    main()
