#!/usr/bin/env python
"""CLI of the training jobs, same flags as the reference `scripts/training.py:131-203` for the `train` and `fine_tune`
sub-commands:
    python scripts/training.py -en EXP -dd DATA_DIR -spks SPK [SPK ...] -lg english train [-chk CKPT] [-nmpd] [-ws N] [-r R] [-m URL] [-rds]
    python scripts/training.py -en EXP -dd DATA_DIR -spks SPK [SPK ...] -lg english fine_tune -chk CKPT
It builds `HyperParams`, writes `<experiment>/config.json` and runs `daft_exprt/train.py` or `daft_exprt/fine_tune.py` in a
sub-process, like the reference (`training.py:101-128`).  `pre_process` is dataset tooling outside the accelerated path
(its markers come from the Montreal Forced Aligner)."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'ubisoft-laforge-daft-exprt_amd')
sys.path.insert(0, PKG)

from daft_exprt.hparams import HyperParams  # noqa: E402


def train(args, hparams, config_file, log_file):
    cmd = [sys.executable, os.path.join(PKG, 'daft_exprt', 'train.py'), '--data_set_dir', args.data_set_dir, '--config_file', config_file,
           '--benchmark_dir', os.path.join(ROOT, 'scripts', 'benchmarks'), '--log_file', log_file, '--world_size', str(args.world_size),
           '--rank', str(args.rank), '--master', args.master]
    if not args.no_multiprocessing_distributed:
        cmd.append('--multiprocessing_distributed')
    return subprocess.call(cmd, env=_env())


def fine_tune_command(args, config_file, log_file):
    ''' the sub-process of `training.py:119-128` '''
    return [sys.executable, os.path.join(PKG, 'daft_exprt', 'fine_tune.py'), '--data_set_dir', args.data_set_dir,
            '--config_file', config_file, '--log_file', log_file]


def _env():
    return dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get('PYTHONPATH', ''))


def experiment_paths(args):
    ''' (output directory, config.json, log file) of the experiment '''
    out_dir = os.path.join(ROOT, 'trainings', args.experiment_name)
    log_name = 'fine_tuning.log' if args.command == 'fine_tune' else 'train.log'
    return out_dir, os.path.join(out_dir, 'config.json'), os.path.join(out_dir, 'logs', log_name)


def build_hparams(args, out_dir):
    features_dir = os.path.join(ROOT, 'datasets', args.language, '22050Hz')
    return HyperParams(training_files=os.path.join(features_dir, f'train_{args.language}.txt'),
                       validation_files=os.path.join(features_dir, f'validation_{args.language}.txt'), output_directory=out_dir,
                       language=args.language, speakers=args.speakers, checkpoint=args.checkpoint,
                       resident_data_set=bool(getattr(args, 'resident_data_set', False)))


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description='script to train Daft-Exprt on MI355X')
    parser.add_argument('-en', '--experiment_name', type=str, required=True)
    parser.add_argument('-dd', '--data_set_dir', type=str, required=True)
    parser.add_argument('-spks', '--speakers', nargs='*', default=[])
    parser.add_argument('-lg', '--language', type=str, default='english')
    sub = parser.add_subparsers(dest='command')
    p_train = sub.add_parser('train')
    p_train.add_argument('-chk', '--checkpoint', type=str, default='')
    p_train.add_argument('-nmpd', '--no_multiprocessing_distributed', action='store_true')
    p_train.add_argument('-ws', '--world_size', type=int, default=1)
    p_train.add_argument('-r', '--rank', type=int, default=0)
    p_train.add_argument('-m', '--master', type=str, default='tcp://localhost:54321')
    # keep the training set in device memory and collate the batches there (daft_exprt/resident_set.py); not in the reference
    p_train.add_argument('-rds', '--resident_data_set', action='store_true')
    p_fine_tune = sub.add_parser('fine_tune')
    p_fine_tune.add_argument('-chk', '--checkpoint', type=str, required=True)
    sub.add_parser('pre_process')
    return parser.parse_args(argv)


if __name__ == '__main__':
    args = parse_args()
    if args.command not in ('train', 'fine_tune'):
        sys.exit(f'"{args.command}" is dataset tooling of the reference (its markers come from MFA); only "train" and "fine_tune" '
                 'are accelerated here')
    out_dir, config_file, log_file = experiment_paths(args)
    hparams = build_hparams(args, out_dir)
    hparams.save_hyper_params(config_file)
    os.makedirs(os.path.dirname(log_file), exist_ok=True)
    if args.command == 'train':
        sys.exit(train(args, hparams, config_file, log_file))
    sys.exit(subprocess.call(fine_tune_command(args, config_file, log_file), env=_env()))
