"""Training / validation lists of a features directory (reference: `src/daft_exprt/create_sets.py:8-55`).

One line `<features_dir>/<speaker>|<file>|<speaker_id>` per utterance that has a `.npy`, in the order of the speaker's
`metadata.csv`: the list format `DaftExprtDataLoader` reads.
"""
import logging
import os

_logger = logging.getLogger(__name__)


def create_sets(features_dir, hparams, proportion_validation=0.1):
    ''' writes hparams.training_files and hparams.validation_files.  proportion_validation is a percentage: of every speaker's
        files, each int(100 / proportion_validation)-th goes to the validation list, and the last one does when no other has '''
    for path in (hparams.training_files, hparams.validation_files):
        os.makedirs(os.path.dirname(path), exist_ok=True)
    for line in ('--' * 30, 'CREATING TRAINING AND VALIDATION SETS', '--' * 30):
        _logger.info(line)
    every = int(100 / proportion_validation)
    with open(hparams.training_files, 'w', encoding='utf-8') as training, \
            open(hparams.validation_files, 'w', encoding='utf-8') as validation:
        for speaker, speaker_id in zip(hparams.speakers, hparams.speakers_id):
            _logger.info(f'Speaker: "{speaker}" -- ID: {speaker_id} -- Validation files: {proportion_validation}%')
            spk_features_dir = os.path.join(features_dir, speaker)
            with open(os.path.join(spk_features_dir, 'metadata.csv'), 'r', encoding='utf-8') as f:
                names = [line.strip().split(sep='|')[0].strip() for line in f.readlines()]
            names = [name for name in names if os.path.isfile(os.path.join(spk_features_dir, f'{name}.npy'))]
            in_validation = 0
            for position, name in enumerate(names, start=1):
                held_out = position % every == 0 or (position == len(names) and in_validation == 0)
                (validation if held_out else training).write(f'{spk_features_dir}|{name}|{speaker_id}\n')
                in_validation += held_out
            _logger.info('')
