#!/usr/bin/env python
"""Pre-processing of aligned speaker data sets for training: the reference's `scripts/training.py ... pre_process`
(`training.py:43-98`) without its call of the Montreal Forced Aligner.
    python scripts/pre_process.py -en EXP -dd DATA_DIR -spks SPK [SPK ...] -lg english [-fd FEATURES_DIR] [-pv 0.1] [-nj 6]
DATA_DIR/<speaker>/ holds `wavs/*.wav`, `metadata.csv` and `align/*.markers` + `align/*.lab` as the aligner step of the
reference leaves them.  The features (`daft_exprt.extract_features`, on the GPU) go to FEATURES_DIR; the training / validation
lists and `<experiment>/stats.json` are written where `scripts/training.py ... train` reads them, whatever FEATURES_DIR is (the
list lines carry the path of the features): both scripts take these paths from `training.py`'s `build_hparams`."""
import argparse
import importlib.util
import json
import logging
import os
import sys
import types
from shutil import copyfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'ubisoft-laforge-daft-exprt_amd')
sys.path.insert(0, PKG)

_logger = logging.getLogger(__name__)


def _training_cli():
    ''' scripts/training.py as a module: the experiment directory and the lists' location are defined there, once '''
    spec = importlib.util.spec_from_file_location('daft_exprt_training_cli', os.path.join(ROOT, 'scripts', 'training.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TRAINING = _training_cli()


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description='script to pre-process aligned speakers data sets for Daft-Exprt on MI355X')
    parser.add_argument('-en', '--experiment_name', type=str, required=True)
    parser.add_argument('-dd', '--data_set_dir', type=str, required=True)
    parser.add_argument('-spks', '--speakers', nargs='*', default=[])
    parser.add_argument('-lg', '--language', type=str, default='english')
    parser.add_argument('-fd', '--features_dir', type=str, default=os.path.join(ROOT, 'datasets'))
    parser.add_argument('-pv', '--proportion_validation', type=float, default=0.1)
    parser.add_argument('-nj', '--nb_jobs', type=str, default='6')
    return parser.parse_args(argv)


def list_all_speakers(data_set_dir):
    ''' relative paths of the directories under data_set_dir that hold `wavs/` and `metadata.csv` (`training.py:26-40`) '''
    data_set_dir = os.path.normpath(data_set_dir)
    return [os.path.normpath(os.path.relpath(root, data_set_dir)) for root, directories, files in os.walk(data_set_dir)
            if 'wavs' in directories and 'metadata.csv' in files]


def build_hparams(args, speakers):
    ''' the hyper-parameters `scripts/training.py ... train` builds for this experiment: same output directory, same lists '''
    train_args = types.SimpleNamespace(experiment_name=args.experiment_name, language=args.language, speakers=speakers, checkpoint='',
                                       command='train')
    out_dir, _, _ = TRAINING.experiment_paths(train_args)
    return TRAINING.build_hparams(train_args, out_dir)


def features_directory(args, hparams):
    ''' -fd, or by default the directory of the lists (<ROOT>/datasets/<language>/<rate>Hz) '''
    default = args.features_dir == os.path.join(ROOT, 'datasets')
    return os.path.dirname(hparams.training_files) if default else args.features_dir


def check_data_set(data_set_dir, speakers):
    ''' every speaker needs wavs/, metadata.csv and the aligner's align/ directory '''
    if not speakers:
        sys.exit(f'No speaker found in "{data_set_dir}": a speaker directory holds wavs/ and metadata.csv')
    for speaker in speakers:
        root = os.path.join(data_set_dir, speaker)
        if not os.path.isdir(os.path.join(root, 'align')):
            sys.exit(f'"{os.path.join(root, "align")}" is missing: pre-processing starts from the .markers and .lab files of the '
                     f'aligner (the Montreal Forced Aligner step of the reference is not run here)')
        for path, is_there in ((os.path.join(root, 'wavs'), os.path.isdir), (os.path.join(root, 'metadata.csv'), os.path.isfile)):
            if not is_there(path):
                sys.exit(f'"{path}" is missing')


def pre_process(args):
    from daft_exprt.create_sets import create_sets
    from daft_exprt.extract_features import check_features_config_used, extract_features
    from daft_exprt.features_stats import extract_features_stats
    speakers = args.speakers if args.speakers else list_all_speakers(args.data_set_dir)
    check_data_set(args.data_set_dir, speakers)
    hparams = build_hparams(args, speakers)
    out_dir = hparams.output_directory
    if os.path.isdir(os.path.join(out_dir, 'checkpoints')):
        sys.exit(f'"{out_dir}" has already been used for a previous training experiment\nCannot perform pre-processing\n'
                 f'Please change the "experiment_name" script argument')
    features_dir = features_directory(args, hparams)
    hparams.save_hyper_params(os.path.join(out_dir, 'config.json'))
    log_dir = os.path.join(out_dir, 'logs')
    os.makedirs(log_dir, exist_ok=True)
    logging.basicConfig(handlers=[logging.StreamHandler(), logging.FileHandler(os.path.join(log_dir, 'pre_processing.log'), mode='w')],
                        format='%(asctime)s [%(levelname)s] %(message)s', datefmt='%Y-%m-%d %H:%M:%S', level=logging.INFO)
    if os.path.isdir(features_dir) and not check_features_config_used(features_dir, hparams):
        sys.exit(f'"{features_dir}" contains data that were extracted using a different set of hyper-parameters. '
                 f'Please change the "features_dir" script argument')
    for speaker in speakers:
        os.makedirs(os.path.join(features_dir, speaker), exist_ok=True)
        copyfile(os.path.join(args.data_set_dir, speaker, 'metadata.csv'), os.path.join(features_dir, speaker, 'metadata.csv'))
    nb_jobs = int(args.nb_jobs) if args.nb_jobs != 'max' else 0
    report = extract_features(args.data_set_dir, features_dir, hparams, nb_jobs)
    _logger.info(f'{report["written"]} utterances written, {len(report["skipped"])} skipped, {report["seconds"]:.1f} s')
    create_sets(features_dir, hparams, args.proportion_validation)
    stats = extract_features_stats(hparams, nb_jobs)
    with open(os.path.join(out_dir, 'stats.json'), 'w') as f:
        json.dump(stats, f, indent=4, sort_keys=True)
    return report


if __name__ == '__main__':
    pre_process(parse_args())
