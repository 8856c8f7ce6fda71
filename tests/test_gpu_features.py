"""GPU checks of training-feature extraction (csrc/features.hip, daft_exprt/extract_features.py): the three kernels against
results recorded from the reference (tests/golden/features_kat.json) and the float64 oracle (tests/feature_oracle.py), and
`extract_features` -> `create_sets` -> `extract_features_stats` -> `DaftExprtDataLoader` on a data set fabricated in tmp_path."""
import json
import logging
import os

import numpy as np
import pytest
import torch

from tests import feature_oracle as FO
from tests import pitch_cases as C
from tests.util import make_hparams

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
FS = 22050


@pytest.fixture(scope='module')
def kat(golden_dir):
    with open(os.path.join(golden_dir, 'features_kat.json'), 'r', encoding='utf-8') as f:
        return json.load(f)


# ---- dx_marker_durations --------------------------------------------------------------------------------------------------------

def _durations_dev(cases, cfg, centered, L):
    ''' one padded launch over `cases`; outputs pre-filled (NaN has no integer form: a value no duration can take) '''
    from daft_exprt import _hip as H
    B = len(cases)
    spans = np.zeros((B, L, 2), dtype=np.float64)
    for b, case in enumerate(cases):
        spans[b, :len(case['spans'])] = case['spans']
    spans = torch.from_numpy(spans).to(DEV)
    n_rows = torch.tensor([len(case['spans']) for case in cases], dtype=torch.int64, device=DEV)
    n_samples = torch.tensor([case['n_samples'] for case in cases], dtype=torch.int64, device=DEV)
    durations = torch.full((B, L), -(2 ** 62), dtype=torch.int64, device=DEV)
    n_out = torch.full((B,), -(2 ** 62), dtype=torch.int64, device=DEV)
    status = torch.full((B,), -77, dtype=torch.int32, device=DEV)
    H.check(H.lib().dx_marker_durations(H.ptr(spans), H.ptr(n_rows), H.ptr(n_samples), H.ptr(durations), H.ptr(n_out), H.ptr(status), B, L,
                                        float(cfg['sampling_rate']), cfg['filter_length'], cfg['hop_length'], int(centered), H.stream()))
    torch.cuda.synchronize()
    return durations.cpu().numpy(), n_out.cpu().numpy(), status.cpu().numpy()


def test_marker_durations_equal_the_reference_bit_for_bit(kat):
    seen = 0
    for c, cfg in enumerate(kat['configs']):
        for centered in (True, False):
            cases = [case for case in kat['durations'] if case['config'] == c and case['centered'] == centered]
            L = max(len(case['spans']) for case in cases)
            assert 1 <= L <= 41 and len(cases) > 0
            durations, n_out, status = _durations_dev(cases, cfg, centered, L)
            solo = [_durations_dev([case], cfg, centered, L) for case in cases]
            for b, case in enumerate(cases):
                want = np.zeros(L, dtype=np.int64)
                want[:len(case['durations'])] = case['durations']
                assert int(status[b]) == case['status'], (c, centered, b, int(status[b]), case['status'])
                np.testing.assert_array_equal(durations[b], want, err_msg=f'config {c} centered {centered} case {b}')
                assert int(n_out[b]) == len(case['durations'])
                np.testing.assert_array_equal(solo[b][0][0], durations[b])           # alone == its row in the batch
                assert int(solo[b][2][0]) == int(status[b]) and int(solo[b][1][0]) == int(n_out[b])
            seen += len(cases)
    assert seen == len(kat['durations']) >= 300


def test_marker_durations_more_rows_than_a_wave():
    ''' 70 - 150 rows: the kernel takes its rows 64 at a time; held to the oracle that the recorded results pin '''
    cfg = dict(sampling_rate=22050, filter_length=1024, hop_length=256)
    rng = np.random.RandomState(9)
    cases, kinds = [], ['plain', 'wav_short', 'wav_long', 'zero_row_late', 'zero_row_unreached', 'plain']
    for i, kind in enumerate(kinds):
        L = [150, 130, 70, 100, 129, 65][i]
        bounds = np.round(np.concatenate(([0.], np.cumsum(rng.uniform(0.03, 0.12, size=L)))), 4)
        spans = [[float(bounds[k]), float(bounds[k + 1])] for k in range(L)]
        n = int(bounds[-1] * cfg['sampling_rate'])
        if kind == 'wav_short':
            n = int(bounds[90] * cfg['sampling_rate'])          # the frames run out in the second chunk of rows
        elif kind == 'wav_long':
            n += 5 * cfg['hop_length']
        elif kind == 'zero_row_late':
            spans[80][1] = spans[80][0]
        elif kind == 'zero_row_unreached':
            spans[120][1] = spans[120][0]
            n = int(bounds[100] * cfg['sampling_rate'])
        cases.append({'spans': spans, 'n_samples': n})
    for centered in (True, False):
        durations, n_out, status = _durations_dev(cases, cfg, centered, 150)
        for b, case in enumerate(cases):
            want, want_status = FO.marker_durations(case['spans'], case['n_samples'], cfg['sampling_rate'], cfg['filter_length'],
                                                    cfg['hop_length'], centered)
            assert int(status[b]) == want_status, (kinds[b], centered, int(status[b]), want_status)
            padded = np.zeros(150, dtype=np.int64)
            padded[:len(want)] = want
            np.testing.assert_array_equal(durations[b], padded, err_msg=f'{kinds[b]} centered {centered}')
            assert int(n_out[b]) == len(want)
            solo = _durations_dev([case], cfg, centered, len(case['spans']))
            np.testing.assert_array_equal(solo[0][0], padded[:len(case['spans'])])
            assert int(solo[2][0]) == want_status
        if centered:
            assert [int(x) for x in status] == [0, 3, 1, 2, 3, 0]


def test_duration_to_integer_wrapper(kat):
    from daft_exprt.extract_features import duration_to_integer
    from types import SimpleNamespace
    raised = {1: IndexError, 2: ValueError}
    picked = {}
    for case in kat['durations']:
        picked.setdefault(case['status'], case)
    assert sorted(picked) == [0, 1, 2, 3]
    for status, case in picked.items():
        hp = SimpleNamespace(centered=case['centered'], **kat['configs'][case['config']])
        if status in raised:
            with pytest.raises(raised[status]):
                duration_to_integer(case['spans'], hp, nb_samples=case['n_samples'])
        else:
            assert duration_to_integer(case['spans'], hp, nb_samples=case['n_samples']) == case['durations']
    # without nb_samples: int(total duration * sampling_rate) samples
    hp = make_hparams()
    spans = [[0., 0.31], [0.31, 0.52], [0.52, 1.004]]
    n = int(sum([(x[1] - x[0]) for x in spans]) * hp.sampling_rate)
    want, status = FO.marker_durations(spans, n, hp.sampling_rate, hp.filter_length, hp.hop_length, hp.centered)
    assert status == FO.OK and duration_to_integer(spans, hp) == want


# ---- dx_symbol_pool -------------------------------------------------------------------------------------------------------------

def _pool_dev(energy, pitch, durations, n_rows):
    ''' the entry point on NaN-filled outputs '''
    from daft_exprt import _hip as H
    B, T = energy.shape
    L = durations.shape[1]
    e, p = torch.from_numpy(energy).to(DEV), torch.from_numpy(pitch).to(DEV)
    d = torch.from_numpy(durations).to(DEV)
    n = torch.tensor(n_rows, dtype=torch.int64, device=DEV)
    sym_e = torch.full((B, L), float('nan'), dtype=torch.float32, device=DEV)
    sym_p = torch.full((B, L), float('nan'), dtype=torch.float32, device=DEV)
    H.check(H.lib().dx_symbol_pool(H.ptr(e), H.ptr(p), e.stride(0), H.ptr(d), H.ptr(n), H.ptr(sym_e), H.ptr(sym_p), B, T, L, H.stream()))
    torch.cuda.synchronize()
    return sym_e.cpu().numpy(), sym_p.cpu().numpy()


def _pool_case(rows, T, rng, unvoiced_rows=()):
    ''' random energies, pitches with 30 % zeros, rows listed in unvoiced_rows [(utterance, row)] without a voiced frame '''
    B, L = len(rows), max(1, max(len(r) for r in rows))
    assert all(sum(r) <= T for r in rows)
    energy = rng.uniform(0.5, 40., size=(B, T)).astype(np.float32)
    pitch = np.where(rng.rand(B, T) < 0.3, 0., rng.uniform(4.2, 5.8, size=(B, T))).astype(np.float32)
    durations = np.zeros((B, L), dtype=np.int64)
    for b, r in enumerate(rows):
        durations[b, :len(r)] = r
    for b, row in unvoiced_rows:
        first = sum(rows[b][:row])
        pitch[b, first: first + rows[b][row]] = 0.
    return energy, pitch, durations, [len(r) for r in rows]


def _check_pool(energy, pitch, durations, n_rows):
    sym_e, sym_p = _pool_dev(energy, pitch, durations, n_rows)
    assert not np.isnan(sym_e).any() and not np.isnan(sym_p).any()                      # every element is written
    worst = 0.
    for b, n in enumerate(n_rows):
        ref_e, ref_p = FO.symbol_pool(energy[b], pitch[b], durations[b, :n])
        # one fp32 rounding of a double-accumulated mean, times 2 for the oracle's own last bit
        for got, ref in ((sym_e[b, :n], ref_e), (sym_p[b, :n], ref_p)):
            err = np.abs(got.astype(np.float64) - ref)
            assert (err <= 2 * 2.0 ** -24 * np.abs(ref)).all(), (b, got, ref)
            worst = max(worst, float((err / np.maximum(np.abs(ref), 1e-30)).max()) if n else 0.)
        assert not sym_e[b, n:].any() and not sym_p[b, n:].any()                          # padding is exactly 0
        solo = _pool_dev(energy[b:b + 1], pitch[b:b + 1], durations[b:b + 1], [n])
        np.testing.assert_array_equal(solo[0][0], sym_e[b])                               # no dependence on the other utterances
        np.testing.assert_array_equal(solo[1][0], sym_p[b])
    print(f'symbol pool: worst relative error {worst:.3g} (bound {2 * 2.0 ** -24:.3g})')
    return sym_e, sym_p


def test_symbol_pool_small_batch():
    rng = np.random.RandomState(5)
    rows = [[1, 5, 0, 3, 7, 0, 0, 2, 4], [40], [0, 0, 6, 1, 1, 1, 10, 0, 2, 3, 0, 5], []]
    energy, pitch, durations, n_rows = _pool_case(rows, 40, rng, unvoiced_rows=[(0, 4), (2, 3)])
    assert durations.shape == (4, 12)
    sym_e, sym_p = _check_pool(energy, pitch, durations, n_rows)
    assert sym_p[0, 4] == 0. and sym_e[0, 4] > 0.                                        # a row of unvoiced frames only
    assert sym_e[0, 0] == energy[0, 0] and sym_e[2, 3] == energy[2, 6] and sym_p[2, 3] == 0.   # one-frame rows
    assert sym_e[0, 2] == 0. and sym_p[0, 2] == 0. and not sym_e[3].any()               # zero rows, an empty utterance


def test_symbol_pool_rows_longer_than_a_wave():
    rng = np.random.RandomState(6)
    energy, pitch, durations, n_rows = _pool_case([[200, 0, 100], [1, 298, 1], [65, 64, 63]], 300, rng, unvoiced_rows=[(2, 1)])
    assert durations.shape == (3, 3)
    _check_pool(energy, pitch, durations, n_rows)


def test_symbol_pool_more_rows_than_a_wave():
    rng = np.random.RandomState(7)
    rows = [list(rng.randint(0, 4, size=150)), list(rng.randint(1, 3, size=64)), list(rng.randint(0, 3, size=65))]
    energy, pitch, durations, n_rows = _pool_case(rows, max(sum(r) for r in rows) + 3, rng)
    _check_pool(energy, pitch, durations, n_rows)


def test_get_symbols_wrappers_print_the_reference_lines(kat):
    from daft_exprt.extract_features import get_symbols_energy, get_symbols_pitch
    for case in kat['pooling']:
        markers = [['0.000', '0.000', str(d), 'AH0', 'w', '0'] for d in case['durations']]
        for got, want in ((get_symbols_energy(np.float32(case['energy']), markers), case['symbols_energy']),
                          (get_symbols_pitch(np.float32(case['pitch']), markers), case['symbols_pitch'])):
            assert len(got) == len(want) and all(line.endswith('\n') for line in got)
            assert np.abs(np.array([float(x) for x in got]) - np.array([float(x) for x in want])).max() <= 1.001e-3


# ---- dx_wav_crop ----------------------------------------------------------------------------------------------------------------

def test_wav_crop():
    from daft_exprt.extract_features import wav_crop_batch
    rng = np.random.RandomState(8)
    x = rng.uniform(-1, 1, size=(3, 50)).astype(np.float32)
    crops = [(0, 20), (30, 20), (10, 0)]                       # from the first sample, up to the last one, empty
    y = wav_crop_batch(torch.from_numpy(x).to(DEV), torch.tensor(crops, dtype=torch.int64, device=DEV), 24)
    torch.cuda.synchronize()
    y = y.cpu().numpy()
    assert y.shape == (3, 24)
    for b, (begin, n) in enumerate(crops):
        np.testing.assert_array_equal(y[b, :n], x[b, begin: begin + n])
        assert not y[b, n:].any()
    # more than one block per row, a width that is no multiple of the block
    x = rng.uniform(-1, 1, size=(2, 5000)).astype(np.float32)
    crops = [(7, 4993), (1500, 2049)]
    y = wav_crop_batch(torch.from_numpy(x).to(DEV), torch.tensor(crops, dtype=torch.int64, device=DEV), 4993).cpu().numpy()
    for b, (begin, n) in enumerate(crops):
        np.testing.assert_array_equal(y[b, :n], x[b, begin: begin + n])
        assert not y[b, n:].any()


# ---- extract_features end to end ------------------------------------------------------------------------------------------------

UTTERANCES = {
    # name: (speaker, sampling rate, seconds between the first and the last marker, sentence, marker words)
    'a0': ('spkA', FS, 1.30, 'Hello world', ['hello', 'world']),
    'a1': ('spkA', 16000, 1.10, 'Good morning, everyone.', ['good', 'morning', 'everyone']),
    'a2': ('spkA', FS, 0.60, 'Too short', ['too', 'short']),                                  # under minimum_wav_duration
    'b0': ('spkB', FS, 1.60, 'Yes, we can', ['yes', '<sil>', 'we', 'can']),
    'b1': ('spkB', FS, 1.20, 'These are other words', ['nothing', 'alike']),                  # cannot be matched
    'b2': ('spkB', FS, 1.00, "That's it!", ['that', 's', 'it']),
}
BAD = {'a2': 'minimum_wav_duration', 'b1': 'does not match'}


def _fabricate(tmp_path, hp):
    ''' data/<speaker>/{wavs, align} and features/<speaker>/metadata.csv: voiced / unvoiced segments, one per marker row '''
    from daft_exprt.audio import write_wav_int16
    rng = np.random.RandomState(11)
    phones = [s for s in hp.symbols if s.isalpha() or s[:-1].isalpha()][:20]
    for name, (speaker, rate, seconds, sentence, words) in UTTERANCES.items():
        data, feat = tmp_path / 'data' / speaker, tmp_path / 'features' / speaker
        for d in (data / 'wavs', data / 'align', feat):
            d.mkdir(parents=True, exist_ok=True)
        rows = [(word, idx) for idx, word in enumerate(words) for _ in range(1 if word == '<sil>' else 2)]
        begin = round(float(rng.uniform(0.05, 0.2)), 4)
        cuts = np.sort(rng.uniform(0.1, 0.9, size=len(rows) - 1)) * seconds
        bounds = np.concatenate(([0.], cuts, [seconds]))
        for k in range(1, len(bounds)):                       # every phone well above half an analysis window
            bounds[k] = max(bounds[k], bounds[k - 1] + 0.05)
        bounds = np.round(bounds * seconds / bounds[-1] + begin, 4)
        lines, pieces = [], [np.zeros(int(round(begin * rate)), dtype=np.float32)]
        for k, (word, idx) in enumerate(rows):
            phone = 'SIL' if word == '<sil>' else phones[int(rng.randint(0, len(phones)))]
            lines.append(f'{bounds[k]}\t{bounds[k + 1]}\t{phone}\t{word}\t{idx}\n')
            span = float(bounds[k + 1] - bounds[k])
            if word == '<sil>':
                pieces.append((0.001 * rng.standard_normal(int(round(span * rate)))).astype(np.float32))
            elif k % 2:
                pieces.append((0.05 * rng.standard_normal(int(round(span * rate)))).astype(np.float32))
            else:
                pieces.append(C.harmonic_tone(float(rng.uniform(100, 260)), rate, span))
        pieces.append(np.zeros(int(0.1 * rate), dtype=np.float32))
        wav = np.concatenate(pieces)
        write_wav_int16(str(data / 'wavs' / f'{name}.wav'), rate, np.clip(np.trunc(wav * 32768.), -32768, 32767).astype(np.int16))
        (data / 'align' / f'{name}.markers').write_text(''.join(lines), encoding='utf-8')
        (data / 'align' / f'{name}.lab').write_text(sentence + '\n', encoding='utf-8')
        with open(feat / 'metadata.csv', 'a', encoding='utf-8') as f:
            f.write(f'{name}|{sentence}\n')
    with open(tmp_path / 'features' / 'spkA' / 'metadata.csv', 'a', encoding='utf-8') as f:
        f.write('a9|no markers for this one\n')


def _solo(path, begin, end, hp):
    ''' the cropped samples of one utterance and the front-end run on them alone '''
    from daft_exprt.audio import crop_range, load_wav
    from daft_exprt.extract_features import mel_spectrogram_batch, pitch_batch
    wav, _ = load_wav(path, sr=FS, device=DEV)
    first, n = crop_range(begin, end, FS, len(wav))
    w = torch.from_numpy(np.ascontiguousarray(wav[first: first + n])).reshape(1, -1).to(DEV)
    n_dev = torch.tensor([n], dtype=torch.int64, device=DEV)
    mel, energy, n_frames = mel_spectrogram_batch(w, n_dev, hp)
    log_pitch, n_pitch = pitch_batch(w, n_dev, hp)
    T = int(n_frames[0])
    assert int(n_pitch[0]) == T
    return n, mel[0, :, :T].cpu().numpy(), energy[0, :T].cpu().numpy(), log_pitch[0, :T].cpu().numpy()


def _text(values):
    return ''.join('%.3f\n' % v for v in np.asarray(values).tolist())


def test_extract_features_end_to_end(tmp_path, caplog):
    from daft_exprt.create_sets import create_sets
    from daft_exprt.data_loader import DaftExprtDataLoader
    from daft_exprt.extract_features import extract_features, update_markers
    from daft_exprt.features_stats import extract_features_stats
    hp = make_hparams(speakers=['spkA', 'spkB'], training_files=str(tmp_path / 'exp' / 'train_english.txt'),
                      validation_files=str(tmp_path / 'exp' / 'validation_english.txt'), output_directory=str(tmp_path / 'out'))
    _fabricate(tmp_path, hp)
    data, features = str(tmp_path / 'data'), str(tmp_path / 'features')
    with caplog.at_level(logging.WARNING):
        report = extract_features(data, features, hp, 2, batch_size=3)
    good = [name for name in UTTERANCES if name not in BAD]
    assert report['written'] == len(good) == 4 and report['already_done'] == 0, report
    assert sorted((spk, name) for spk, name, _ in report['skipped']) == sorted((UTTERANCES[name][0], name) for name in BAD)
    for spk, name, reason in report['skipped']:
        assert BAD[name] in reason
    assert any('audio has length inferior to 1.0s after trimming' in r.getMessage() for r in caplog.records)
    exts = ('.npy', '.markers', '.frames_nrg', '.symbols_nrg', '.frames_f0', '.symbols_f0')
    written = sorted(str(p.relative_to(features)) for p in (tmp_path / 'features').rglob('*') if p.is_file())
    want = sorted([f'{UTTERANCES[name][0]}/{name}{ext}' for name in good for ext in exts] +
                  [f'{spk}/{f}' for spk in hp.speakers for f in ('metadata.csv', 'config.json')])
    assert written == want

    logger = logging.getLogger('test_gpu_features')
    for name in good:
        speaker, rate, seconds, sentence, words = UTTERANCES[name]
        base = os.path.join(features, speaker, name)
        with open(os.path.join(data, speaker, 'align', f'{name}.markers'), 'r', encoding='utf-8') as f:
            lines = f.readlines()
        rows = [line.strip().split('\t') for line in lines]
        begin, end = float(rows[0][0]), float(rows[-1][1])
        n, mel, energy, log_pitch = _solo(os.path.join(data, speaker, 'wavs', f'{name}.wav'), begin, end, hp)
        got_mel = np.load(base + '.npy')
        assert got_mel.dtype == np.float32
        np.testing.assert_array_equal(got_mel, mel, err_msg=name)
        with open(base + '.frames_nrg', 'r', encoding='utf-8') as f:
            assert f.read() == _text(energy), name
        with open(base + '.frames_f0', 'r', encoding='utf-8') as f:
            assert f.read() == _text(log_pitch), name
        assert (log_pitch > 0).any() and (log_pitch == 0).any(), name                     # voiced and unvoiced frames
        spans = [[float(r[0]) - begin, float(r[1]) - begin] for r in rows]
        durations, status = FO.marker_durations(spans, n, hp.sampling_rate, hp.filter_length, hp.hop_length, hp.centered)
        assert status == FO.OK, name
        markers = update_markers(name, lines, sentence, begin, durations, hp, logger)
        with open(base + '.markers', 'r', encoding='utf-8') as f:
            assert f.read() == ''.join('\t'.join(m) + '\n' for m in markers), name
        assert sum(int(m[2]) for m in markers) == mel.shape[1], name
        for ext, frames, is_pitch in (('.symbols_nrg', energy, False), ('.symbols_f0', log_pitch, True)):
            with open(base + ext, 'r', encoding='utf-8') as f:
                got = np.array([float(line) for line in f.readlines()])
            ref = FO.pool_for_markers(frames, markers, is_pitch)
            assert got.shape == ref.shape and np.abs(got - ref).max() <= 1.001e-3, (name, ext)
    b0 = open(os.path.join(features, 'spkB', 'b0.markers'), encoding='utf-8').read().splitlines()
    assert b0[2].split('\t')[3:5] == [',', ','] and int(b0[2].split('\t')[2]) > 0           # the <sil> row became the comma
    b2 = open(os.path.join(features, 'spkB', 'b2.markers'), encoding='utf-8').read().splitlines()
    assert [row.split('\t')[3] for row in b2[-2:]] == ['!', '~']

    # a second call finds everything done
    mtimes = {p: os.stat(os.path.join(features, p)).st_mtime_ns for p in written if not p.endswith('config.json')}
    again = extract_features(data, features, hp, 2)
    assert again['written'] == 0 and again['already_done'] == 4
    assert {r[1] for r in again['skipped']} == set(BAD)
    assert mtimes == {p: os.stat(os.path.join(features, p)).st_mtime_ns for p in mtimes}

    # lists, statistics and the trainer's reader on top
    create_sets(features, hp, proportion_validation=50)
    hp.stats = json.loads(json.dumps(extract_features_stats(hp, 2)))
    assert {'spk 0', 'spk 1', 'symbols'} == set(hp.stats)
    items = 0
    for list_file in (hp.training_files, hp.validation_files):
        loader = DaftExprtDataLoader(list_file, hp, shuffle=False)
        for i in range(len(loader)):
            symbols, dur_float, dur_int, sym_e, sym_p, frames_e, frames_p, mel_spec = loader[i][:8]
            assert len(symbols) == len(dur_float) == len(dur_int) == len(sym_e) == len(sym_p)
            assert int(dur_int.sum()) == mel_spec.shape[1] == len(frames_e) == len(frames_p)
            items += 1
    assert items == 4



def test_pre_process_script_feeds_the_train_command(tmp_path, monkeypatch):
    ''' scripts/pre_process.py with -fd elsewhere, then HyperParams built the way `scripts/training.py ... train` builds them '''
    import importlib.util
    from daft_exprt.data_loader import DaftExprtDataLoader
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('pre_process_cli', os.path.join(root, 'scripts', 'pre_process.py'))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    monkeypatch.setattr(cli.TRAINING, 'ROOT', str(tmp_path / 'repo'))        # experiments and lists under tmp_path
    _fabricate(tmp_path, make_hparams(speakers=['spkA', 'spkB']))
    for spk in ('spkA', 'spkB'):                                             # the data set carries metadata.csv; features/ is the script's
        os.replace(tmp_path / 'features' / spk / 'metadata.csv', tmp_path / 'data' / spk / 'metadata.csv')
    argv = ['-en', 'EXP', '-dd', str(tmp_path / 'data'), '-lg', 'english', '-fd', str(tmp_path / 'elsewhere'), '-pv', '50']
    args = cli.parse_args(argv)
    report = cli.pre_process(args)
    assert report['written'] == 4 and len(report['skipped']) == 2
    out_dir = tmp_path / 'repo' / 'trainings' / 'EXP'
    for name in ('config.json', 'stats.json', os.path.join('logs', 'pre_processing.log')):
        assert (out_dir / name).is_file(), name
    assert (tmp_path / 'elsewhere' / 'spkA' / 'a0.npy').is_file() and (tmp_path / 'elsewhere' / 'spkB' / 'config.json').is_file()
    with open(out_dir / 'stats.json') as f:
        text = f.read()
    assert text == json.dumps(json.loads(text), indent=4, sort_keys=True)

    train = cli.TRAINING
    train_args = train.parse_args(['-en', 'EXP', '-dd', str(tmp_path / 'data'), '-spks', 'spkA', 'spkB', '-lg', 'english', 'train'])
    hp = train.build_hparams(train_args, train.experiment_paths(train_args)[0])
    assert set(hp.stats) == {'spk 0', 'spk 1', 'symbols'}                    # read from the experiment's stats.json
    items = 0
    for list_file in (hp.training_files, hp.validation_files):
        loader = DaftExprtDataLoader(list_file, hp, shuffle=False)
        for i in range(len(loader)):
            item = loader[i]
            assert int(item[2].sum()) == item[7].shape[1] and item[9].startswith(str(tmp_path / 'elsewhere'))
            items += 1
    assert items == 4
    with pytest.raises(SystemExit):                                          # an experiment with checkpoints is refused
        (out_dir / 'checkpoints').mkdir()
        cli.pre_process(args)
