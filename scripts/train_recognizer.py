#!/usr/bin/env python
"""Train the CTC phone recogniser that scores intelligibility, on the corpus's own feature files
    python scripts/train_recognizer.py (-chk CHECKPOINT | -cfg CONFIG_JSON) -tf TRAIN_LIST -vf VALIDATION_LIST -o RECOGNIZER.pt
                                       [-st 2000] [-bs 32] [-lr 1e-3] [-hid 256] [-ly 3] [-str 2]

  -chk   a training checkpoint, read for its hyper-parameters and speaker statistics only (as `scripts/evaluate.py` reads them);
  -cfg   or a JSON file of the hyper-parameters (`config_params`), when there is no checkpoint yet
  -tf    a `features_dir|feature_file|speaker_id` list to train on, e.g. the training list `scripts/pre_process.py` writes
  -vf    such a list of held-out utterances: the phone error rate of the report is measured on it
  -o     where the trained recogniser is saved (weights and constructor arguments, `daft_exprt.recognizer.load_recognizer` reads it)
  -st    Adam steps;  -bs utterances per step;  -lr learning rate;  -hid width;  -ly convolutions;  -str frames stacked per step

The model (`daft_exprt/recognizer.py`: per-utterance normalised log-mel, frames stacked, convolutions, CTC) is trained on the GPU and
saved; `recognizer_report.json` beside it holds the report of `train_recognizer` -- the held-out phone error rate with and without
the stress folded, the utterances left out, the rows skipped -- and up to 20 held-out utterances with their decodes.  What the
recogniser's error rate is on real speech, and how its error rate on a synthesis tracks listeners, has not been measured: read the
report, and read a synthesis's rate beside the rate of the recording (`scripts/evaluate.py -rec`)."""
import argparse
import json
import logging
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'ubisoft-laforge-daft-exprt_amd')
sys.path.insert(0, PKG)

_logger = logging.getLogger('train_recognizer')


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description='Train the CTC phone recogniser of the intelligibility score on feature files')
    parser.add_argument('-chk', '--checkpoint', default=None, help='training checkpoint: its hyper-parameters and statistics are used')
    parser.add_argument('-cfg', '--config', default=None, help='JSON file of hyper-parameters, instead of a checkpoint')
    parser.add_argument('-tf', '--training_files', required=True, help='list of features_dir|feature_file|speaker_id lines to train on')
    parser.add_argument('-vf', '--validation_files', required=True, help='such a list of held-out utterances')
    parser.add_argument('-o', '--output', required=True, help='file the trained recogniser is saved to')
    parser.add_argument('-st', '--steps', type=int, default=2000, help='Adam steps')
    parser.add_argument('-bs', '--batch_size', type=int, default=32, help='utterances per step')
    parser.add_argument('-lr', '--learning_rate', type=float, default=1e-3, help='Adam learning rate')
    parser.add_argument('-hid', '--hidden', type=int, default=256, help='width of the convolutions')
    parser.add_argument('-ly', '--layers', type=int, default=3, help='convolutions')
    parser.add_argument('-str', '--stride', type=int, default=2, help='adjacent frames stacked into one step')
    parser.add_argument('--seed', type=int, default=1234, help='seed of the initial weights and the batches')
    return parser.parse_args(argv)


def check_args(args):
    ''' the mistakes that can be told before anything is read; SystemExit naming the flag '''
    if (args.checkpoint is None) == (args.config is None):
        raise SystemExit('train_recognizer.py: give either -chk or -cfg')
    for what, path in (('checkpoint', args.checkpoint), ('config', args.config), ('training list', args.training_files),
                       ('validation list', args.validation_files)):
        if path is not None and not os.path.isfile(path):
            raise SystemExit(f'train_recognizer.py: no such {what}: {path}')
    if min(args.steps, args.batch_size, args.hidden, args.layers, args.stride) < 1 or not args.learning_rate > 0:
        raise SystemExit(f'train_recognizer.py: -st {args.steps}, -bs {args.batch_size}, -hid {args.hidden}, -ly {args.layers} and '
                         f'-str {args.stride} must be at least 1 and -lr {args.learning_rate} positive')
    out_dir = os.path.dirname(os.path.abspath(args.output))
    if not os.path.isdir(out_dir):
        raise SystemExit(f'train_recognizer.py: no such directory for -o: {out_dir}')


def load_hparams(args):
    from daft_exprt.hparams import HyperParams
    if args.checkpoint is not None:
        import torch
        params = torch.load(args.checkpoint, map_location='cpu', weights_only=False)['config_params']
    else:
        with open(args.config, 'r', encoding='utf-8') as f:
            params = json.load(f)
    return HyperParams(verbose=False, **params)


def main(argv=None):
    args = parse_args(argv)
    logging.basicConfig(format='%(asctime)s [%(levelname)s] %(message)s', datefmt='%Y-%m-%d %H:%M:%S', level=logging.INFO)
    check_args(args)
    from daft_exprt.recognizer import save_recognizer, train_recognizer
    recognizer, report = train_recognizer(load_hparams(args), args.training_files, args.validation_files, steps=args.steps,
                                          batch_size=args.batch_size, lr=args.learning_rate, seed=args.seed, hidden=args.hidden,
                                          layers=args.layers, stride=args.stride)
    save_recognizer(recognizer, args.output)
    _logger.info(f'recogniser saved to {args.output}')
    path = os.path.join(os.path.dirname(os.path.abspath(args.output)), 'recognizer_report.json')
    with open(path, 'w', encoding='utf-8') as f:
        json.dump(report, f, indent=1)
    _logger.info(f'held-out phone error rate {report["phone_error_rate"]} ({report["phone_error_rate_folded"]} with the stress folded), '
                 f'{report["left_out"]} utterances left out, {report["skipped_rows"]} rows skipped; report written to {path}')
    return report


if __name__ == '__main__':
    main()
