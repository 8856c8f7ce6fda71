"""CPU checks of training-feature extraction against results recorded from the reference (tests/golden/features_kat.json,
tools/gen_golden_features.py): `update_markers`, the float64 oracle the kernels are held to (tests/feature_oracle.py),
`create_sets`, `extract_features_stats` and the `scripts/pre_process.py` command line."""
import importlib.util
import json
import logging
import os
import types

import numpy as np
import pytest

from tests import feature_oracle as FO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def kat(golden_dir):
    with open(os.path.join(golden_dir, 'features_kat.json'), 'r', encoding='utf-8') as f:
        return json.load(f)


def test_update_markers_reproduces_the_reference(kat, caplog):
    from daft_exprt.extract_features import update_markers
    hp = types.SimpleNamespace(language='english')
    logger = logging.getLogger('test_features_host')
    assert len(kat['markers']) >= 40
    unmatched = 0
    for i, case in enumerate(kat['markers']):
        got = update_markers(f'case{i:02d}', list(case['lines']), case['sentence'], case['sent_begin'], list(case['int_durations']),
                             hp, logger)
        assert got == case['expect'], (i, case['sentence'])
        unmatched += got is None
    assert unmatched == 2
    assert sum('Correspondance issue' in r.getMessage() for r in caplog.records) == 2


def test_update_markers_returns_none_where_the_reference_breaks():
    from daft_exprt.extract_features import update_markers
    hp, logger = types.SimpleNamespace(language='english'), logging.getLogger('test_features_host')
    lines = ['0.1\t0.2\tHH\thi\t0\n', '0.2\t0.3\tSIL\t<sil>\t1\n']
    assert update_markers('f', lines, '...', 0.1, [3, 4], hp, logger) is None              # nothing but punctuation
    assert update_markers('f', lines, 'hi', 0.1, [3, 4], hp, logger) is None               # a marker row is left over
    assert update_markers('f', lines[:1], 'hi there', 0.1, [3], hp, logger) is None        # a word is left over
    with pytest.raises(NotImplementedError):
        update_markers('f', lines, 'hi', 0.1, [3, 4], types.SimpleNamespace(language='french'), logger)


def test_oracle_durations_equal_the_reference(kat):
    cases = kat['durations']
    assert len(cases) >= 300
    by_status = [0, 0, 0, 0]
    single_append = sub_window = 0
    for i, case in enumerate(cases):
        cfg = kat['configs'][case['config']]
        got, status = FO.marker_durations(case['spans'], case['n_samples'], cfg['sampling_rate'], cfg['filter_length'], cfg['hop_length'],
                                          case['centered'])
        assert status == case['status'], (i, status, case['status'])
        assert got == case['durations'], (i, got, case['durations'])
        by_status[status] += 1
        sub_window += case['n_samples'] < cfg['filter_length']
        single_append += status == 3 and len(got) < len(case['spans'])
    print('duration KATs by status', by_status, 'single-append', single_append, 'sub-window', sub_window)
    assert min(by_status) >= 10 and single_append >= 5 and sub_window >= 10


def _parse(lines):
    return np.array([float(line) for line in lines])


def test_oracle_pooling_agrees_with_the_printed_reference(kat):
    kinds = set()
    for case in kat['pooling']:
        energy, pitch = np.float32(case['energy']), np.float32(case['pitch'])
        sym_energy, sym_pitch = FO.symbol_pool(energy, pitch, case['durations'])
        # one unit of the last printed digit: the reference averages in float32, the oracle in float64
        assert np.abs(sym_energy - _parse(case['symbols_energy'])).max() <= 1.001e-3
        assert np.abs(sym_pitch - _parse(case['symbols_pitch'])).max() <= 1.001e-3
        first = np.concatenate(([0], np.cumsum(case['durations'])))
        for row, d in enumerate(case['durations']):
            if d == 0:
                kinds.add('zero row')
                assert sym_energy[row] == 0. and sym_pitch[row] == 0.
            elif not (pitch[first[row]: first[row + 1]] > 0).any():
                kinds.add('unvoiced row')
                assert sym_pitch[row] == 0. and sym_energy[row] > 0.
            if d == 1:
                kinds.add('one-frame row')
                assert sym_energy[row] == float(energy[first[row]])
    assert kinds == {'zero row', 'unvoiced row', 'one-frame row'}


def _write_features_tree(kat, root):
    ''' the fabricated features directory of the golden create_sets / stats case '''
    for speaker, names in kat['metadata'].items():
        os.makedirs(os.path.join(root, speaker))
        with open(os.path.join(root, speaker, 'metadata.csv'), 'w', encoding='utf-8') as f:
            f.writelines(f'{name}|some text\n' for name in names)
    for key, texts in kat['files'].items():
        np.save(os.path.join(root, key) + '.npy', np.zeros((2, 2), dtype=np.float32))
        for ext, text in texts.items():
            with open(os.path.join(root, key) + ext, 'w', encoding='utf-8') as f:
                f.write(text)


def _sets_hparams(kat, tmp_path):
    return types.SimpleNamespace(speakers=kat['speakers'], speakers_id=[0, 1], symbols=kat['symbols'],
                                 training_files=str(tmp_path / 'lists' / 'train.txt'),
                                 validation_files=str(tmp_path / 'lists' / 'validation.txt'))


def test_create_sets_writes_the_golden_lists(kat, tmp_path):
    from daft_exprt.create_sets import create_sets
    features = str(tmp_path / 'features')
    _write_features_tree(kat, features)
    assert len(kat['files']) == 12 and len(kat['speakers']) == 2
    hp = _sets_hparams(kat, tmp_path)
    for proportion in (10, 50):
        create_sets(features, hp, proportion_validation=proportion)
        for key, path in (('training', hp.training_files), ('validation', hp.validation_files)):
            with open(path, 'r', encoding='utf-8') as f:
                got = [line.replace(features + os.sep, '') for line in f.readlines()]
            assert got == kat['sets'][str(proportion)][key], (proportion, key)
    # 7 + 5 files: every 10th -> none, so the last of each speaker; every 2nd -> 3 + 2
    assert len(kat['sets']['10']['validation']) == 2 and len(kat['sets']['50']['validation']) == 5


def test_features_stats_match_the_reference(kat, tmp_path):
    from daft_exprt.create_sets import create_sets
    from daft_exprt.features_stats import extract_features_stats
    features = str(tmp_path / 'features')
    _write_features_tree(kat, features)
    hp = _sets_hparams(kat, tmp_path)
    create_sets(features, hp, proportion_validation=10)
    stats = json.loads(json.dumps(extract_features_stats(hp, 1)))
    ref = kat['stats']
    assert set(stats) == set(ref) == {'spk 0', 'spk 1', 'symbols'}
    for speaker in ('spk 0', 'spk 1'):
        for feature in ('energy', 'pitch'):
            assert set(stats[speaker][feature]) == {'mean', 'std', 'min', 'max'}
            for key, value in ref[speaker][feature].items():
                assert stats[speaker][feature][key] == pytest.approx(value, rel=1e-12, abs=0), (speaker, feature, key)
    assert set(stats['symbols']) == set(ref['symbols'])
    for symbol, values in ref['symbols'].items():
        assert set(stats['symbols'][symbol]) == {'dur_min', 'dur_max', 'dur_mean', 'dur_std'}
        for key, value in values.items():
            assert stats['symbols'][symbol][key] == pytest.approx(value, rel=1e-12, abs=1e-18), (symbol, key)


def test_min_phone_duration_and_config_check(tmp_path):
    from daft_exprt.extract_features import FEATURES_HPARAMS, check_features_config_used, get_min_phone_duration
    from tests.util import make_hparams
    lines = ['0.10\t0.25\tHH\thi\t0\n', '0.25\t0.29\tAY1\thi\t0\n', '0.29\t0.50\tSIL\t<sil>\t1\n']
    assert get_min_phone_duration(lines) == 0.29 - 0.25
    assert get_min_phone_duration(lines, min_phone_dur=0.01) == 0.01
    hp = make_hparams()
    assert check_features_config_used(str(tmp_path), hp)                         # no config yet
    hp.save_hyper_params(str(tmp_path / 'spk' / 'config.json'))
    assert check_features_config_used(str(tmp_path), hp)
    assert 'hop_length' in FEATURES_HPARAMS and 'batch_size' not in FEATURES_HPARAMS
    assert not check_features_config_used(str(tmp_path), make_hparams(hop_length=128, filter_length=512))
    assert check_features_config_used(str(tmp_path), make_hparams(batch_size=4))


def test_batches_respect_the_sample_budget():
    from daft_exprt.extract_features import _plan_batches
    names = [f'u{k}' for k in range(7)]
    assert _plan_batches(names, [10] * 7, 3, 10 ** 9) == [names[0:3], names[3:6], names[6:]]
    assert _plan_batches(names, [10, 10, 1000, 10, 10, 10, 10], 64, 1999) == [names[0:2], names[2:3], names[3:]]
    assert _plan_batches([], [], 64, 100) == []


def _training_cli():
    spec = importlib.util.spec_from_file_location('training_cli', os.path.join(ROOT, 'scripts', 'training.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _pre_process_cli():
    spec = importlib.util.spec_from_file_location('pre_process_cli', os.path.join(ROOT, 'scripts', 'pre_process.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_pre_process_cli_flags_and_missing_align(tmp_path):
    cli = _pre_process_cli()
    args = cli.parse_args(['-en', 'EXP', '-dd', '/data', '-spks', 'A', 'B', '-lg', 'english', '-fd', '/feat', '-pv', '2.5', '-nj', '3'])
    assert (args.experiment_name, args.data_set_dir, args.speakers, args.language) == ('EXP', '/data', ['A', 'B'], 'english')
    assert (args.features_dir, args.proportion_validation, args.nb_jobs) == ('/feat', 2.5, '3')
    hp = cli.build_hparams(args, args.speakers)
    train = _training_cli()
    train_args = train.parse_args(['-en', 'EXP', '-dd', '/data', '-spks', 'A', 'B', '-lg', 'english', 'train'])
    train_hp = train.build_hparams(train_args, train.experiment_paths(train_args)[0])
    # whatever -fd is, the lists and the experiment directory are the ones `training.py ... train` reads
    assert (hp.training_files, hp.validation_files, hp.output_directory) == \
        (train_hp.training_files, train_hp.validation_files, train_hp.output_directory)
    assert hp.output_directory == os.path.join(ROOT, 'trainings', 'EXP') and cli.features_directory(args, hp) == '/feat'
    args = cli.parse_args(['--experiment_name', 'EXP', '--data_set_dir', '/data'])
    assert (args.speakers, args.language, args.proportion_validation, args.nb_jobs) == ([], 'english', 0.1, '6')
    # the default features directory is the directory of the lists
    assert cli.features_directory(args, hp) == os.path.dirname(train_hp.training_files)

    spk = tmp_path / 'data' / 'spkA'
    (spk / 'wavs').mkdir(parents=True)
    (spk / 'metadata.csv').write_text('a0|hello\n', encoding='utf-8')
    assert cli.list_all_speakers(str(tmp_path / 'data')) == ['spkA']
    args = cli.parse_args(['-en', 'never_written_features', '-dd', str(tmp_path / 'data'), '-fd', str(tmp_path / 'features')])
    with pytest.raises(SystemExit) as e:
        cli.pre_process(args)
    assert 'align' in str(e.value) and 'is missing' in str(e.value)
    assert not os.path.exists(os.path.join(ROOT, 'trainings', 'never_written_features'))
    assert not (tmp_path / 'features').exists()
