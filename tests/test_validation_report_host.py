"""Host side of the validation report (`daft_exprt/validation_report.py`, `train.validate`, `train.generate_benchmark_sentences`):
the oracle's target alignment, the `.npz` round trip, the matplotlib-free path and the exported entry points.  No device."""
import inspect
import os
import sys
import types

import numpy as np

from daft_exprt import _hip as H
from tests.validation_oracle import BINS, alignment_oracle, film_hist_oracle, target_alignment_oracle


def test_target_alignment_of_a_hand_written_case():
    ''' 4 symbols, durations (2, 0, 3, 1): the zero-duration symbol owns nothing and does not move the others '''
    from daft_exprt.validation_report import target_alignment
    want = np.array([[1, 1, 0, 0, 0, 0],
                     [0, 0, 0, 0, 0, 0],
                     [0, 0, 1, 1, 1, 0],
                     [0, 0, 0, 0, 0, 1]], np.float64)
    assert np.array_equal(target_alignment_oracle([2, 0, 3, 1], 4, 6), want)
    assert np.array_equal(target_alignment([2, 0, 3, 1], 6), want)
    # cut at the output length, and symbols at or past the input length own nothing
    assert np.array_equal(target_alignment_oracle([2, 0, 3, 1], 4, 4), want[:, :4])
    assert np.array_equal(target_alignment_oracle([2, 0, 3, 1], 2, 6), want * np.array([[1], [1], [0], [0]]))
    # the scores of a perfect and of a shifted alignment
    frames, hits, mass = alignment_oracle(np.stack([want, np.roll(want, 1, axis=0)]).astype(np.float32), [[2, 0, 3, 1]] * 2, [4, 4], [6, 6])
    assert frames.tolist() == [6, 6] and hits.tolist() == [6, 0] and mass.tolist() == [1., 0.]


def _fabricated_report(nb_blocks=(2, 1, 3), seed=0):
    from daft_exprt.validation_report import MODULES, ValidationReport, histogram_density
    rng = np.random.default_rng(seed)
    films, stats = {}, {}
    for m, nb in zip(MODULES, nb_blocks):
        film = rng.normal(size=(5, nb, 8)).astype(np.float32)
        counts, edges, minmax, finite = film_hist_oracle(film)
        films[m] = {'counts': counts, 'edges': edges, 'density': histogram_density(counts, edges), 'finite': finite, 'minmax': minmax}
        halves = film.astype(np.float64).reshape(5, nb, 2, 4)
        stats[m] = {'mean': halves.mean(axis=(0, 3)), 'std': halves.std(axis=(0, 3))}
    L, T, n_mel = 4, 6, 3
    sample = {'sample_batch': np.int64(0), 'sample_index': np.int64(1), 'sample_durations_int': np.array([2, 0, 3, 1])}
    for key in ('duration', 'energy', 'pitch'):
        sample[f'{key}_target'], sample[f'{key}_pred'] = rng.normal(size=L).astype(np.float32), rng.normal(size=L).astype(np.float32)
    sample['mel_target'], sample['mel_pred'] = rng.normal(size=(n_mel, T)).astype(np.float32), rng.normal(size=(n_mel, T)).astype(np.float32)
    sample['alignment_pred'] = rng.random(size=(L, T)).astype(np.float32)
    sample['alignment_target'] = target_alignment_oracle([2, 0, 3, 1], L, T).astype(np.float32)
    hp = types.SimpleNamespace(seed=1234)
    report = ValidationReport.from_results(hp, 42, films, stats, frames=[6, 0, 4], hits=[3, 0, 4], mass=[0.5, 0., 0.75], sample=sample)
    return report, films, stats, sample


def test_write_round_trips_through_the_npz(tmp_path):
    from daft_exprt.validation_report import MODULES
    report, films, stats, sample = _fabricated_report()
    scalars = report.write(str(tmp_path))
    path = tmp_path / 'iter_0000042.npz'
    assert path.is_file() and report.path(str(tmp_path)) == str(path)
    got = np.load(path)
    assert int(got['iteration']) == 42
    for m, nb in zip(MODULES, (2, 1, 3)):
        assert got[f'film_{m}_counts'].shape == (nb, 2, BINS) and got[f'film_{m}_counts'].dtype == np.int64
        assert got[f'film_{m}_edges'].shape == (nb, 2, BINS + 1) and got[f'film_{m}_edges'].dtype == np.float64
        assert got[f'film_{m}_density'].shape == (nb, 2, BINS) and got[f'film_{m}_finite'].shape == (nb, 2)
        assert got[f'film_{m}_mean'].shape == (nb, 2) and got[f'film_{m}_std'].shape == (nb, 2)
        for key in ('counts', 'edges', 'density', 'finite'):
            assert np.array_equal(got[f'film_{m}_{key}'], films[m][key])
        # density integrates to 1 over the bins, as hist(density=True)
        assert np.allclose((got[f'film_{m}_density'] * np.diff(got[f'film_{m}_edges'], axis=-1)).sum(-1), 1.)
    assert got['alignment_frames'].tolist() == [6, 0, 4] and got['alignment_hits'].tolist() == [3, 0, 4]
    assert got['alignment_frames'].dtype == np.int64 and got['alignment_mass'].dtype == np.float32
    for key, value in sample.items():
        assert np.array_equal(got[key], value), key
    # scalars: utterances without frames do not enter the mean mass; the hit rate is over all frames
    assert scalars['DaftExprt.validation/alignment_mass'] == 0.625
    assert scalars['DaftExprt.validation/alignment_hit_rate'] == 0.7
    for m, nb in zip(MODULES, (2, 1, 3)):
        for blk in range(nb):
            for half, name in enumerate(('gamma', 'beta')):
                assert scalars[f'DaftExprt.film/{m}/block{blk}/{name}_mean'] == float(stats[m]['mean'][blk, half])
                assert scalars[f'DaftExprt.film/{m}/block{blk}/{name}_std'] == float(stats[m]['std'][blk, half])
    assert len(scalars) == 2 + 4 * (2 + 1 + 3)


def test_figures_without_matplotlib_return_none(tmp_path, monkeypatch):
    report, _, _, _ = _fabricated_report()
    monkeypatch.setitem(sys.modules, 'matplotlib', None)        # `import matplotlib` now raises ImportError
    assert report.figures(str(tmp_path)) is None
    assert not list(tmp_path.iterdir())


def test_figures_with_matplotlib_are_pngs(tmp_path):
    try:
        import matplotlib  # noqa: F401
    except ImportError:
        return          # nothing to draw with: the path above is the one in use
    report, _, _, _ = _fabricated_report()
    files = report.figures(str(tmp_path))
    assert len(files) == 11 and all(os.path.getsize(f) > 0 and f.endswith('.png') for f in files)


def test_benchmark_sentences_return_quietly_without_the_phonemised_file(tmp_path, caplog):
    from daft_exprt.train import generate_benchmark_sentences
    hp = types.SimpleNamespace(benchmark_dir=str(tmp_path), language='english', seed=1234, validation_files=str(tmp_path / 'none.txt'))
    with caplog.at_level('INFO', logger='daft_exprt.train'):
        assert generate_benchmark_sentences(None, hp, str(tmp_path / 'out'), 10) is None
    assert not (tmp_path / 'out').exists()
    assert sum('No benchmark sentences generated' in r.getMessage() for r in caplog.records) == 1
    # the file is there but the validation list is not: the same
    os.makedirs(tmp_path / 'english')
    (tmp_path / 'english' / 'sentences_phonemised.txt').write_text('a|{HH AH0} ~\n')
    assert generate_benchmark_sentences(None, hp, str(tmp_path / 'out'), 10) is None
    assert not (tmp_path / 'out').exists()
    # no benchmark directory at all
    assert generate_benchmark_sentences(None, types.SimpleNamespace(language='english', seed=0), str(tmp_path / 'out'), 1) is None


def test_validate_keeps_its_signature():
    from daft_exprt.train import validate
    params = inspect.signature(validate).parameters
    assert list(params) == ['gpu', 'model', 'criterion', 'val_loader', 'hparams', 'report']
    assert params['report'].default is None
    assert all(p.default is inspect.Parameter.empty for name, p in params.items() if name != 'report')


def test_library_exports_the_validation_entry_points():
    if not os.path.exists(H.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = H.lib()
    declared = {name for name, _, _ in H.header_prototypes()}
    for name in ('dx_film_hist_range', 'dx_film_hist_count', 'dx_alignment_score'):
        assert name in declared and hasattr(lib, name), name
    # argument errors are codes, not undefined behaviour
    assert lib.dx_film_hist_range(None, None, None, 1, 1, 2, None) == -1 and b'null' in lib.dx_last_error()
    assert lib.dx_film_hist_count(8, 8, 8, 8, 3, 2, 5, None) == -2 and b'even' in lib.dx_last_error()
    assert lib.dx_alignment_score(8, 8, 8, 8, 8, 8, 8, 1, 10000, 4, None) == -5 and b'LDS' in lib.dx_last_error()
