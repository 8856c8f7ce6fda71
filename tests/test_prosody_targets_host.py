"""CPU side of the per-symbol prosody targets: tests/prosody_targets_oracle.py pinned against independent statements of
the same arithmetic -- tests/feature_oracle.py's pooling, the loader's `_standardise`, numpy.mean / numpy.std, cases worked out by
hand -- and the host logic of daft_exprt/clone.py, scripts/clone.py and the `prosody_targets` pass-through of the synthesis driver.
No GPU: nothing here launches a kernel."""
import importlib.util
import inspect
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from daft_exprt.clone import QUANTITIES
from tests import feature_oracle as F
from tests import prosody_targets_oracle as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _curves(T, seed):
    rng = np.random.RandomState(seed)
    energy = rng.uniform(0.1, 5.0, size=T).astype(np.float32)
    pitch = np.where(rng.uniform(size=T) < 0.6, rng.uniform(4.4, 5.6, size=T), 0.).astype(np.float32)
    return energy, pitch


# ---- the oracle's pooling and statistics ----------------------------------------------------------------------------------------------

def test_pooling_with_begin_zero_is_the_feature_oracle():
    for seed, durations in ((0, [3, 0, 5, 1, 2]), (1, [1] * 9), (2, [0, 0, 40]), (3, [7, 13, 0, 0, 1])):
        energy, pitch = _curves(40, seed)
        got = P.pool(energy, pitch, 0, durations, 40)
        want = F.symbol_pool(energy, pitch, durations)
        assert got[0].dtype == np.float32 and got[1].dtype == np.float32
        assert np.array_equal(got[0], want[0].astype(np.float32)) and np.array_equal(got[1], want[1].astype(np.float32))


def test_pooling_with_a_begin_is_the_pooling_of_the_shifted_curves():
    energy, pitch = _curves(60, 4)
    durations = [4, 0, 9, 2, 1]
    for begin in (1, 7, 44):
        got = P.pool(energy, pitch, begin, durations, 60)
        want = F.symbol_pool(energy[begin:], pitch[begin:], durations)
        assert np.array_equal(got[0], want[0].astype(np.float32)) and np.array_equal(got[1], want[1].astype(np.float32))
    assert P.pool(energy, pitch, 44, durations, 60) is not None          # 44 + 16 == 60: the rows end exactly at T
    assert P.pool(energy, pitch, 45, durations, 60) is None and P.pool(energy, pitch, -1, durations, 60) is None
    assert P.pool(energy, pitch, 0, [3, -1], 60) is None
    assert P.pool(energy, pitch, 44, durations, 59) is None               # frames past T are not there, whatever the array holds


def test_pooling_by_hand():
    energy = np.array([9., 1., 2., 3., 4., 5., 6., 9.], dtype=np.float32)
    pitch = np.array([9., 0., 5., 0., 0., 0., 4., 6.], dtype=np.float32)
    e, p = P.pool(energy, pitch, 1, [2, 0, 3, 1], 8)
    assert e.tolist() == [1.5, 0., 4., 6.] and p.tolist() == [5., 0., 0., 4.]      # the all-unvoiced row gives pitch 0


def test_own_statistics_are_numpy_mean_and_population_std():
    rng = np.random.RandomState(5)
    for n in (2, 3, 12, 64):
        v = rng.uniform(0.5, 6.0, size=n).astype(np.float32)
        v[rng.randint(n)] = 0.
        mean, std, count = P.own_stats(v)
        live = v[v != 0].astype(np.float64)
        assert count == len(live) and mean.dtype == np.float32
        assert mean == np.float32(np.mean(live)) and std == np.float32(np.std(live))
    assert P.own_stats(np.zeros(4, dtype=np.float32)) == (0., 0., 0)
    assert P.own_stats(np.array([0., 2.5], dtype=np.float32)) == (2.5, 0., 1)


def test_standardise_is_the_loaders():
    from daft_exprt.data_loader import DaftExprtDataLoader
    rng = np.random.RandomState(6)
    values = rng.uniform(0.2, 7.0, size=50).astype(np.float32)
    values[[3, 17, 49]] = 0.
    mean, std = np.float32(3.1234567), np.float32(0.7654321)
    loader = SimpleNamespace(hparams=SimpleNamespace(stats={'spk 4': {'energy': {'mean': float(mean), 'std': float(std)}}}))
    theirs = DaftExprtDataLoader._standardise(loader, values.copy(), 4, 'energy')
    ours = P.standardise(values, mean, std)
    assert not ours[[3, 17, 49]].any() and not np.asarray(theirs)[[3, 17, 49]].any()
    err = np.abs(np.asarray(theirs, dtype=np.float64) - ours)
    assert (err <= P.standardise_bound(values, mean, std)).all(), err.max()


def test_clone_pool_cases_by_hand():
    energy = np.array([1., 3., 2., 2., 4., 4., 8., 8.], dtype=np.float32)
    pitch = np.array([5., 5., 0., 0., 4., 6., 0., 0.], dtype=np.float32)
    # given statistics: plain standardisation, zeros stay zeros, rows past n_rows are zeros
    out = P.clone_pool(energy, pitch, 0, [2, 2, 2, 2, 9], 4, 8, 6, energy_stats=(2., 2.), pitch_stats=(5., 0.5))
    assert out['status'] == P.OK and out['dropped'] == 0
    assert out['raw_energy'].tolist() == [2., 2., 4., 8., 0., 0.] and out['raw_pitch'].tolist() == [5., 0., 5., 0., 0., 0.]
    assert out['sym_energy'].tolist() == [0., 0., 1., 3., 0., 0.] and out['sym_pitch'].tolist() == [0., 0., 0., 0., 0., 0.]
    assert out['self_stats'].tolist() == [4., np.float32(np.std([2., 2., 4., 8.])), 5., 0.]
    # self statistics: energy over four values; pitch has two equal values: std 0, dropped bit 1
    out = P.clone_pool(energy, pitch, 0, [2, 2, 2, 2], 4, 8, 4)
    assert out['dropped'] == 2 and not out['sym_pitch'].any()
    s = float(np.float32(np.std([2., 2., 4., 8.])))
    assert np.allclose(out['sym_energy'], [(2 - 4) / s, (2 - 4) / s, 0., (8 - 4) / s], rtol=1e-12)
    # a single voiced symbol (bit 1) and constant energy (bit 0)
    out = P.clone_pool(np.full(8, 2.5, dtype=np.float32), pitch, 0, [2, 2, 0, 0], 2, 8, 4)
    assert out['dropped'] == 3 and not out['sym_energy'].any() and not out['sym_pitch'].any()
    assert out['self_stats'].tolist() == [2.5, 0., 5., 0.]
    # given statistics with std 0 cannot be used either
    assert P.clone_pool(energy, pitch, 0, [4, 4], 2, 8, 2, energy_stats=(1., 0.))['dropped'] & 1
    # an overrun: everything zero, status 1
    out = P.clone_pool(energy, pitch, 3, [4, 2], 2, 8, 3)
    assert out['status'] == P.OVERRUN and not out['raw_energy'].any() and not out['sym_energy'].any() and not out['self_stats'].any()
    assert P.clone_pool(energy, pitch, 2, [4, 2, 7], 2, 7, 3)['status'] == P.OVERRUN      # (T rules, not what the array holds)
    assert P.clone_pool(energy, pitch, 2, [4, 2, 7], 2, 8, 3)['status'] == P.OK           # durations behind n_rows are not counted


# ---- the oracle's imposition -----------------------------------------------------------------------------------------------------------

def test_impose_by_hand():
    x = np.array([0.1, 0.2, 0.3, 0.4], dtype=np.float32)
    ones, zeros = [1.] * 4, [0.] * 4
    sec = lambda f: float(P.target_seconds(f, 256, 22050))
    assert sec(1) == float(np.float32(256 / 22050)) and sec(0) == 0.
    # weight 1: the targets themselves; weight 0: the input itself; symbols at or past the length untouched
    d, e, p, exact = P.impose(x, x, x, 3, t_dur=[7, 0, 2, 5], t_energy=[1., 2., 3., 4.], t_pitch=[-1., 0., 1., 2.], w_dur=ones, w_energy=ones,
                              w_pitch=ones)
    assert exact == 1 and d.tolist() == [sec(7), 0., sec(2), float(x[3])]
    assert e.tolist() == [1., 2., 3., float(x[3])] and p.tolist() == [-1., 0., 1., float(x[3])]
    d, e, p, exact = P.impose(x, x, x, 4, t_dur=[7, 0, 2, 5], t_energy=[1., 2., 3., 4.], w_dur=zeros, w_energy=zeros)
    assert exact == 0 and d.tolist() == e.tolist() == p.tolist() == x.astype(np.float64).tolist()
    # in between: x + w (t - x)
    d, e, _, _ = P.impose(x, x, x, 4, t_dur=[4] * 4, t_energy=[2.] * 4, w_dur=[0.5] * 4, w_energy=[0.25] * 4)
    assert np.allclose(d, (x.astype(np.float64) + sec(4)) / 2, rtol=1e-15) and np.allclose(e, 0.75 * x.astype(np.float64) + 0.5, rtol=1e-15)
    # a zero energy / pitch target is a statement: taken over from 0.5 on, ignored below
    _, e, p, _ = P.impose(x, x, x, 4, t_energy=[0.] * 4, t_pitch=[0.] * 4, w_energy=[0.49, 0.5, 1., 0.], w_pitch=[0.5, 0.49, 0., 1.])
    assert e.tolist() == [float(x[0]), 0., 0., float(x[3])] and p.tolist() == [0., float(x[1]), float(x[2]), 0.]
    # frame-exact rows: every symbol below the length has a target, weight 1 and factor 1
    exact = lambda **kw: P.impose(x, x, x, 3, **{**dict(t_dur=[3, 1, 0, -1], w_dur=[1., 1., 1., 0.3]), **kw})[3]
    assert exact() == 1
    assert exact(t_dur=[3, -1, 0, 2]) == 0 and exact(w_dur=[1., 0.999, 1., 1.]) == 0 and exact(dur_factors=[1., 1., 1.25, 1.]) == 0
    assert exact(dur_factors=[1., 1., 1., 7.]) == 1 and exact(t_dur=None, w_dur=None, t_energy=[1.] * 4, w_energy=ones) == 0
    # a weight outside [0, 1] below the length: -1 and nothing touched; behind the length it is not looked at
    d, e, p, flag = P.impose(x, x, x, 3, t_dur=[1, 1, 1, 1], w_dur=[1., 1.5, 1., 1.], t_energy=[9.] * 4, w_energy=ones)
    assert flag == -1 and d.tolist() == e.tolist() == x.astype(np.float64).tolist()
    assert P.impose(x, x, x, 3, t_energy=[9.] * 4, w_energy=[1., 1., 1., float('nan')])[3] == 0
    assert P.impose(x, x, x, 3, t_energy=[9.] * 4, w_energy=[1., float('nan'), 1., 1.])[3] == -1


def test_impose_durations_by_hand():
    dur = np.array([0.05, 0., 0.03, 0.07], dtype=np.float32)
    k16 = np.array([4, 0, 3, 6], dtype=np.int64)
    sec = lambda f: P.target_seconds(f, 256, 22050)
    d, di, total, status = P.impose_durations(1, [2, 1, 0, 9], 3, dur, k16, 13, 1)
    assert di.tolist() == [2, 1, 0, 0] and total == 3 and status == 0 and d.tolist() == [sec(2), sec(1), 0., dur[3]]
    d, di, total, status = P.impose_durations(0, [2, 1, 0, 9], 3, dur, k16, 13, 1)
    assert di.tolist() == k16.tolist() and total == 13 and status == 1 and d.tolist() == dur.tolist()
    assert P.impose_durations(1, [0, 0, 0, 9], 3, dur, k16, 13, 0)[2:] == (0, P.ST_EMPTY)
    assert P.impose_durations(-1, [2, 1, 0, 9], 3, dur, k16, 13, 0)[1:] != () and P.impose_durations(-1, [2, 1, 0, 9], 3, dur, k16, 13, 0)[3] == P.ST_WEIGHT


# ---- daft_exprt/clone.py on the host -----------------------------------------------------------------------------------------------------

def _targets():
    from daft_exprt.clone import ProsodyTargets
    durations = torch.tensor([[3, 1, 0, 2], [5, 5, 0, 0], [1, 2, 3, 4]])
    energy = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    w = torch.tensor([[1., 1., 1., 1.], [0.5, 0.5, 0., 0.], [0., 0., 0., 0.]])
    return ProsodyTargets(durations=durations, energy=energy, w_dur=w, w_energy=0.25)


def test_prosody_targets_hold_what_they_are_given():
    from daft_exprt.clone import ProsodyTargets
    t = _targets()
    assert t.shape == (3, 4) and t.units == 'standardised' and t.pitch is None and t.w_pitch is None
    assert t.durations.dtype == torch.int64 and t.energy.dtype == torch.float32
    assert t.w_energy.shape == (3, 4) and t.w_energy.dtype == torch.float32 and bool((t.w_energy == 0.25).all())
    for kw, word in ((dict(w_dur=1.5), 'w_dur'), (dict(w_energy=float('nan')), 'w_energy'), (dict(units='hz'), 'units'),
                     (dict(w_dur=torch.full((3, 4), -0.1)), 'w_dur'), (dict(w_dur=torch.ones(3, 5)), 'shape')):
        with pytest.raises(ValueError) as e:
            ProsodyTargets(**{**dict(durations=t.durations, energy=t.energy), **kw})
        assert word in str(e.value), (kw, str(e.value))
    with pytest.raises(ValueError):
        ProsodyTargets()
    with pytest.raises(ValueError):
        ProsodyTargets(durations=t.durations, energy=t.energy[:, :3])


def test_prosody_targets_permute_select_mask_and_scale():
    t = _targets()
    p = t.permute([2, 0, 1])
    assert p.durations.tolist() == [[1, 2, 3, 4], [3, 1, 0, 2], [5, 5, 0, 0]] and p.energy[0].tolist() == [8., 9., 10., 11.]
    assert p.w_dur[1].tolist() == [1.] * 4 and p.w_dur[2].tolist() == [0.5, 0.5, 0., 0.] and p.pitch is None and p.units == t.units
    assert t.durations.tolist()[0] == [3, 1, 0, 2]                                           # (a new object: the source is untouched)
    assert t.permute(torch.tensor([0, 1, 2])).energy.tolist() == t.energy.tolist()
    for bad in ([0, 1], [0, 1, 1], [0, 1, 3]):
        with pytest.raises(ValueError):
            t.permute(bad)
    only = t.select(('dur',))
    assert only.energy is None and only.w_energy is None and only.durations.tolist() == t.durations.tolist()
    with pytest.raises(ValueError):
        t.select(('dur', 'loudness'))
    m = t.masked(torch.tensor([True, False, True]))
    assert m.w_dur.tolist() == [[1.] * 4, [0.] * 4, [0.] * 4] and m.w_energy.tolist() == [[0.25] * 4, [0.] * 4, [0.25] * 4]
    s = t.scaled({'energy': 0.5})
    assert bool((s.w_energy == 0.125).all()) and s.w_dur.tolist() == t.w_dur.tolist()
    assert t.narrow(2).durations.tolist() == [[3, 1], [5, 5], [1, 2]] and t.narrow(2).w_dur.shape == (3, 2)


def test_prosody_targets_stack_and_raw_units():
    from daft_exprt.clone import ProsodyTargets
    one = ProsodyTargets(durations=torch.tensor([[4, 2]]), pitch=torch.tensor([[5.0, 0.]]), units='raw')
    two = ProsodyTargets(pitch=torch.tensor([[5.5, 4.5, 5.0]]), w_pitch=0.5, units='raw')
    batch = ProsodyTargets.stack([one, None, two], 3)
    assert batch.shape == (3, 3) and batch.energy is None and batch.units == 'raw'
    assert batch.durations.tolist() == [[4, 2, -1], [-1, -1, -1], [-1, -1, -1]] and batch.w_dur.tolist() == [[1., 1., 0.], [0.] * 3, [0.] * 3]
    assert batch.w_pitch.tolist() == [[1., 1., 0.], [0.] * 3, [0.5] * 3]
    assert ProsodyTargets.stack([None, None], 3) is None
    hp = SimpleNamespace(stats={'spk 2': {'pitch': {'mean': 5.0, 'std': 0.5}}, 'spk 7': {'pitch': {'mean': 4.5, 'std': 0.25}}})
    std = batch.standardised(hp, [2, 2, 7])
    assert std.units == 'standardised' and std.pitch.tolist() == [[0., 0., 0.], [0., 0., 0.], [4., 0., 2.]]     # zeros stay zeros
    assert std.standardised(hp, [2, 2, 7]) is std
    with pytest.raises(KeyError):
        batch.standardised(hp, [2, 3, 7])


def test_report_layout():
    from daft_exprt.align import STATUS
    from daft_exprt.clone import INFO_KEYS, SCORE_KEYS, clone_report, merge_reports
    nan = float('nan')
    host = {'status': [0, 4, 0], 'frames': [55, 0, 40], 'begin': [12, 0, 0], 'moved': [1, 0, 0], 'path_cost': [3.5, nan, 2.5],
            'dropped': [0, 0, 2], 'pool_status': [0, 0, 1], 'usable': [True, False, False], 'frame_exact': [True, False, False], 'mcd_db': [4.0, nan, 6.0], 'f0_rmse_cents': [100., nan, nan],
            'vuv_error': [0.25, nan, 0.75], 'pitch_pcc': [0.5, nan, nan], 'energy_pcc': [0.9, nan, 0.7]}
    report = clone_report(['a', 'b', 'c'], host)
    assert list(report) == ['files', 'summary'] and list(report['files']) == ['a', 'b', 'c']
    for record in report['files'].values():
        assert tuple(record) == ('status', 'frames', 'begin', 'moved', 'path_cost', 'dropped', 'pool_status', 'usable', 'frame_exact', 'scores')
        assert tuple(record['scores']) == SCORE_KEYS
    assert set(INFO_KEYS) < set(report['files']['a'])
    c = report['files']['c']                                      # aligned, yet not cloned: the record says why
    assert (c['status'], c['pool_status'], c['usable'], c['frame_exact']) == (0, 1, False, False)
    b = report['files']['b']
    assert b['status'] == 4 and b['frame_exact'] is False and b['path_cost'] is None and all(v is None for v in b['scores'].values())
    s = report['summary']
    assert s['files'] == 3 and s['frame_exact'] == 1 and s['usable'] == 1 and s['status'] == {str(k): {0: 2, 4: 1}.get(k, 0) for k in sorted(STATUS)}
    assert s['scores']['mcd_db'] == {'mean': 5.0, 'files': 2} and s['scores']['f0_rmse_cents'] == {'mean': 100.0, 'files': 1}
    assert s['scores']['pitch_pcc'] == {'mean': 0.5, 'files': 1}
    json.dumps(report, allow_nan=False)                                                       # NaN never reaches the file
    first = clone_report(['a', 'b'], {k: v[:2] for k, v in host.items()})
    second = clone_report(['c'], {k: v[2:] for k, v in host.items()})
    assert merge_reports([first, second]) == report


# ---- scripts/clone.py --------------------------------------------------------------------------------------------------------------------

def _cli():
    spec = importlib.util.spec_from_file_location('clone_cli', os.path.join(ROOT, 'scripts', 'clone.py'))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def test_clone_cli_flags(tmp_path):
    cli = _cli()
    chk, text, wavs = tmp_path / 'ckpt', tmp_path / 'sentences.txt', tmp_path / 'wavs'
    chk.write_bytes(b'')
    text.write_text('u0|{HH AH0} ~\n', encoding='utf-8')
    wavs.mkdir()
    base = ['-chk', str(chk), '-tf', str(text), '-wd', str(wavs), '-out', str(tmp_path / 'out')]
    args = cli.parse_args(base + ['-spk', '3'])
    assert (args.speakers, args.source_speakers, args.batch_size, args.aligner, args.clone, args.normalise, args.vocoder, args.min_frames,
            args.trim_db) == (['3'], None, 32, None, QUANTITIES, 'self', None, 3, -40.0)
    cli.check_args(args)
    args = cli.parse_args(base + ['-spk', 'spk03', 'spk07', '-bs', '4', '--clone', 'dur,pitch', '--normalise', 'target', '-mf', '2', '-trim',
                                  '-30', '--aligner', str(chk), '-src', '1'])
    assert (args.speakers, args.source_speakers, args.batch_size, args.clone, args.normalise, args.min_frames, args.trim_db, args.aligner) == \
        (['spk03', 'spk07'], ['1'], 4, ('dur', 'pitch'), 'target', 2, -30.0, str(chk))
    cli.check_args(args)
    for bad in (['--clone', 'dur,loudness'], ['--clone', ''], ['--clone', 'dur,dur'], ['--normalise', 'speaker']):
        with pytest.raises(SystemExit):
            cli.parse_args(base + ['-spk', '3'] + bad)
    for bad, word in ((['-mf', '0'], 'at least 1'), (['-trim', '3'], 'at most 0'), (['--aligner', str(tmp_path / 'none')], 'no such aligner'),
                      (['-voc', str(tmp_path / 'none')], 'no such vocoder'), (['-wd', str(tmp_path / 'none')], 'no such recordings')):
        with pytest.raises(SystemExit) as e:
            cli.check_args(cli.parse_args(base + ['-spk', '3'] + bad))
        assert word in str(e.value), (bad, str(e.value))
    hp = SimpleNamespace(speakers=['spk03', 'spk07'], speakers_id=[3, 7])
    assert cli.speaker_ids(['spk07'], 3, hp, '-spk') == [7, 7, 7] and cli.speaker_ids(['3', 'spk07'], 2, hp, '-spk') == [3, 7]
    for bad, word in ((['3', '7'], 'one per sentence'), (['5'], 'knows the speakers'), (['nobody'], 'knows the speakers')):
        with pytest.raises(SystemExit) as e:
            cli.speaker_ids(bad, 3, hp, '-spk')
        assert word in str(e.value)


# ---- the synthesis driver's pass-through -------------------------------------------------------------------------------------------------

class _Reached(Exception):
    pass


def test_generate_without_targets_reaches_the_collate_unchanged(monkeypatch, tmp_path):
    from daft_exprt import generate
    from tests.util import make_hparams
    assert 'prosody_targets' in inspect.signature(generate.generate_mel_specs).parameters
    assert 'prosody_targets' in inspect.signature(generate.generate_batch_mel_specs).parameters
    assert 'prosody_targets' in inspect.signature(__import__('daft_exprt.model', fromlist=['DaftExprt']).DaftExprt.inference).parameters
    seen = []

    def collate(*args, **kwargs):
        seen.append((args, kwargs))
        raise _Reached()

    monkeypatch.setattr(generate, 'collate_tensors', collate)
    hp = make_hparams()
    model = SimpleNamespace(eval=lambda: None)
    sentences = [[['HH', 'AH0'], '~'], [['G', 'UH1', 'D'], '.', '~']]
    refs = [(np.zeros(4), np.zeros(4), np.zeros((80, 4)))] * 2

    def run(**kw):
        with pytest.raises(_Reached):
            generate.generate_mel_specs(model, sentences, ['a', 'b'], [3, 7], refs, str(tmp_path), hp, batch_size=2, **kw)
        return seen.pop()

    plain, with_none = run(), run(prosody_targets=None)
    assert not plain[1] and not with_none[1] and len(plain[0]) == len(with_none[0]) == 9
    for a, b in zip(plain[0], with_none[0]):
        assert a is b or a == b
    assert plain[0][0] == sentences and plain[0][6] == [3, 7] and plain[0][7] == ['a_spk_3_ref_mem0', 'b_spk_7_ref_mem1']
    with pytest.raises(AssertionError):
        generate.generate_mel_specs(model, sentences, ['a', 'b'], [3, 7], refs, str(tmp_path), hp, batch_size=2, prosody_targets=[None])
