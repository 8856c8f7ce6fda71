#!/usr/bin/env python
"""Train the speaker encoder that scores speaker identity, on the corpus's own feature files
    python scripts/train_speaker_encoder.py (-chk CHECKPOINT | -cfg CONFIG_JSON) -tf TRAIN_LIST -vf VALIDATION_LIST -o SPEAKER.pt
                                            [-st 2000] [-bs 32] [-lr 1e-3] [-hid 256] [-ly 3] [-str 2] [-dim 128] [--margin 0.2]
                                            [--scale 30]

  -chk   a training checkpoint, read for its hyper-parameters and speaker statistics only (as `scripts/evaluate.py` reads them);
  -cfg   or a JSON file of the hyper-parameters (`config_params`), when there is no checkpoint yet
  -tf    a `features_dir|feature_file|speaker_id` list to train on, e.g. the training list `scripts/pre_process.py` writes; it must
         name at least two speakers
  -vf    such a list of held-out utterances: the identification error and the equal error rate of the report are measured on it
  -o     where the trained encoder is saved (constructor arguments, weights, speaker ids, centroids, threshold and EER;
         `daft_exprt.speaker.load_speaker_encoder` reads it)
  -st    Adam steps;  -bs utterances per step;  -lr learning rate;  -hid width;  -ly convolutions;  -str frames stacked per step;
  -dim   size of the embedding;  --margin, --scale: the additive-margin softmax

The model (`daft_exprt/speaker.py`: log-mel normalised by one scalar mean and variance per utterance, frames stacked, convolutions,
attentive statistics pooling, unit-length embedding) is trained on the GPU and saved; `speaker_report.json` beside it holds the
report of `train_speaker_encoder` -- the held-out identification error against the speakers' centroids, the equal error rate and its
threshold over all held-out pairs, the trials, the errors per speaker, the utterances left out.  What the encoder's error rates are on
real speech, and how its cosine scores track listeners' judgement of speaker similarity, has not been measured: read the report, and
read a synthesis's scores beside those of the recording (`scripts/evaluate.py -spk`)."""
import argparse
import json
import logging
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'ubisoft-laforge-daft-exprt_amd')
sys.path.insert(0, PKG)

_logger = logging.getLogger('train_speaker_encoder')


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description='Train the speaker encoder of the speaker-identity score on feature files')
    parser.add_argument('-chk', '--checkpoint', default=None, help='training checkpoint: its hyper-parameters and statistics are used')
    parser.add_argument('-cfg', '--config', default=None, help='JSON file of hyper-parameters, instead of a checkpoint')
    parser.add_argument('-tf', '--training_files', required=True, help='list of features_dir|feature_file|speaker_id lines to train on')
    parser.add_argument('-vf', '--validation_files', required=True, help='such a list of held-out utterances')
    parser.add_argument('-o', '--output', required=True, help='file the trained encoder is saved to')
    parser.add_argument('-st', '--steps', type=int, default=2000, help='Adam steps')
    parser.add_argument('-bs', '--batch_size', type=int, default=32, help='utterances per step')
    parser.add_argument('-lr', '--learning_rate', type=float, default=1e-3, help='Adam learning rate')
    parser.add_argument('-hid', '--hidden', type=int, default=256, help='width of the convolutions')
    parser.add_argument('-ly', '--layers', type=int, default=3, help='convolutions')
    parser.add_argument('-str', '--stride', type=int, default=2, help='adjacent frames stacked into one step')
    parser.add_argument('-dim', '--dim', type=int, default=128, help='size of the embedding')
    parser.add_argument('--margin', type=float, default=0.2, help='margin of the additive-margin softmax')
    parser.add_argument('--scale', type=float, default=30.0, help='scale of the additive-margin softmax')
    parser.add_argument('--seed', type=int, default=1234, help='seed of the initial weights and the batches')
    return parser.parse_args(argv)


def check_args(args):
    ''' the mistakes that can be told before anything is read; SystemExit naming the flag '''
    if (args.checkpoint is None) == (args.config is None):
        raise SystemExit('train_speaker_encoder.py: give either -chk or -cfg')
    for what, path in (('checkpoint', args.checkpoint), ('config', args.config), ('training list', args.training_files),
                       ('validation list', args.validation_files)):
        if path is not None and not os.path.isfile(path):
            raise SystemExit(f'train_speaker_encoder.py: no such {what}: {path}')
    if min(args.steps, args.batch_size, args.hidden, args.layers, args.stride, args.dim) < 1 or not args.learning_rate > 0:
        raise SystemExit(f'train_speaker_encoder.py: -st {args.steps}, -bs {args.batch_size}, -hid {args.hidden}, -ly {args.layers}, '
                         f'-str {args.stride} and -dim {args.dim} must be at least 1 and -lr {args.learning_rate} positive')
    if args.margin < 0 or not args.scale > 0:
        raise SystemExit(f'train_speaker_encoder.py: --margin {args.margin} must not be negative and --scale {args.scale} positive')
    out_dir = os.path.dirname(os.path.abspath(args.output))
    if not os.path.isdir(out_dir):
        raise SystemExit(f'train_speaker_encoder.py: no such directory for -o: {out_dir}')


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
    from daft_exprt.speaker import save_speaker_encoder, train_speaker_encoder
    try:
        encoder, report = train_speaker_encoder(load_hparams(args), args.training_files, args.validation_files, steps=args.steps,
                                                batch_size=args.batch_size, lr=args.learning_rate, seed=args.seed, hidden=args.hidden,
                                                layers=args.layers, stride=args.stride, dim=args.dim, scale=args.scale, margin=args.margin)
    except ValueError as e:
        raise SystemExit(f'train_speaker_encoder.py: {e}')
    save_speaker_encoder(encoder, args.output)
    _logger.info(f'speaker encoder saved to {args.output}')
    path = os.path.join(os.path.dirname(os.path.abspath(args.output)), 'speaker_report.json')
    with open(path, 'w', encoding='utf-8') as f:
        json.dump(report, f, indent=1)
    _logger.info(f'held-out identification error {report["identification_error"]}, equal error rate {report["eer"]} at a cosine of '
                 f'{report["threshold"]} over {report["trials"]} trials, {report["left_out"]} utterances left out; report written to {path}')
    return report


if __name__ == '__main__':
    main()
