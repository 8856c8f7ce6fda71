"""`dx_mel_cepstrum`, `dx_dtw_align`, `dx_dtw_path_scores` and what is built on them (daft_exprt/evaluate.py, scripts/evaluate.py)
against the float64 oracle of tests/dtw_oracle.py, which tests/test_dtw_host.py pins against an enumeration of all paths.

Tolerances: TOL_FACTOR (10) times the error the kernels' arithmetic has when restated in NumPy float32, measured on the host over
these same cases (tests/test_dtw_host.py): 5.0e-7 relative on a total, 4.1e-8 relative on an MCD, 9.3e-6 on a cepstral
coefficient, 3.2e-8 relative on an F0 RMSE.  Integer cepstra are exact in float32: totals and whole paths must be equal."""
import functools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import dtw_oracle as O
from tests.util import make_hparams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
TOL_TOTAL, TOL_MCD = O.TOL_FACTOR * O.F32_TOTAL_ERR, O.TOL_FACTOR * O.F32_MCD_ERR
TOL_CEP, TOL_F0 = O.TOL_FACTOR * O.F32_CEP_ERR, O.TOL_FACTOR * O.F32_F0_ERR
VUV_ULP = 2.0 ** -24                    # vuv_error is one float32 rounding of a ratio <= 1


def _pad(rows, extent=None, fill=0.0):
    ''' [(n_b, K)] -> ((B, T, K) fp32 device tensor filled with `fill` behind the rows, (B,) int64 lengths) '''
    T = max(1, max(len(r) for r in rows)) if extent is None else extent
    x = np.full((len(rows), T, rows[0].shape[1]), fill, dtype=np.float32)
    for b, r in enumerate(rows):
        x[b, :len(r)] = r
    return torch.from_numpy(x).to(DEV), torch.tensor([len(r) for r in rows], dtype=torch.int64, device=DEV)


def _align(refs, gens, extents=(None, None), fill=0.0, **kw):
    ''' (total, path, path_len) NumPy of one `dtw_align_batch` call over right-padded rows '''
    from daft_exprt.evaluate import dtw_align_batch
    r, n_r = _pad(refs, extents[0], fill)
    g, n_g = _pad(gens, extents[1], fill)
    out = dtw_align_batch(r, n_r, g, n_g, **kw)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


@functools.lru_cache(maxsize=None)
def _oracle(kind, index):
    name, ref, gen = {'exact': O.exact_cases, 'real': O.real_cases}[kind]()[index] if kind != 'limit' else O.limit_case()
    return (name, ref, gen) + O.dtw(ref, gen)


def _same_rows(a, b, rows_a, rows_b, n_paths):
    ''' bit equality of (total, path, path_len) rows; the path is compared over its written extent of the narrower layout '''
    for ra, rb, n in zip(rows_a, rows_b, n_paths):
        assert a[0][ra].tobytes() == b[0][rb].tobytes() and a[2][ra] == b[2][rb]
        assert np.array_equal(a[1][ra, :n], b[1][rb, :n])


# ---- the DTW --------------------------------------------------------------------------------------------------------------------

def _check_exact(cases, got):
    total, path, path_len = got
    for b, (name, ref, gen, want_total, want_path) in enumerate(cases):
        n = len(want_path)
        print(f'{name}: total {float(total[b]):.0f} (oracle {want_total:.0f}), path_len {int(path_len[b])} (oracle {n})')
        assert float(total[b]) == float(want_total) and float(want_total) < 2 ** 24, name
        assert int(path_len[b]) == n, name
        assert np.array_equal(path[b, :n], want_path), name
        assert (path[b, n:] == -1).all(), name


def test_exact_cases_equal_the_oracle_path_for_path():
    cases = [_oracle('exact', i) for i in range(len(O.EXACT_LENGTHS))]
    assert [(len(c[1]), len(c[2])) for c in cases] == O.EXACT_LENGTHS
    got = _align([c[1] for c in cases], [c[2] for c in cases])
    assert got[1].shape == (len(cases), 2 * O.MAX_LEN - 1, 2)
    _check_exact(cases, got)


def test_the_length_limit():
    from daft_exprt.evaluate import dtw_align_batch, max_dtw_length
    assert max_dtw_length() == O.MAX_LEN
    case = _oracle('limit', 0)
    assert len(case[1]) == len(case[2]) == O.MAX_LEN
    _check_exact([case], _align([case[1]], [case[2]]))
    wide = torch.zeros((1, O.MAX_LEN + 1, 1), dtype=torch.float32, device=DEV)
    n = torch.tensor([8], dtype=torch.int64, device=DEV)
    for r, g in ((wide, wide[:, :64].contiguous()), (wide[:, :64].contiguous(), wide)):
        with pytest.raises(RuntimeError, match='error -5'):
            dtw_align_batch(r, n, g, n)


def test_real_valued_cases_give_a_valid_near_optimal_path():
    cases = [_oracle('real', i) for i in range(len(O.REAL_LENGTHS))]
    total, path, path_len = _align([c[1] for c in cases], [c[2] for c in cases])
    for b, (name, ref, gen, want_total, want_path) in enumerate(cases):
        n = int(path_len[b])
        mine = path[b, :n]
        assert O.is_valid_path(mine, len(ref), len(gen)), name
        assert (path[b, n:] == -1).all(), name
        e_path, e_total = O.rel(O.path_cost64(mine, ref, gen), want_total), O.rel(float(total[b]), want_total)
        print(f'{name}: total error {e_total:.2e}, path cost error {e_path:.2e} (bound {TOL_TOTAL:.1e}), path '
              f'{"equal" if np.array_equal(mine, want_path) else "differs"}')
        assert e_path <= TOL_TOTAL and e_total <= TOL_TOTAL, (name, e_path, e_total)


def _ragged():
    ''' six pairs: exact and real-valued ones cannot share a batch (K differs), so the ragged batch is real-valued '''
    lengths = [(257, 300), (33, 1000), (1, 7), (700, 650), (64, 3), (300, 77)]
    pairs = [O.real_pair(a, b, 5000 + n) for n, (a, b) in enumerate(lengths)]
    return lengths, [p[0] for p in pairs], [p[1] for p in pairs]


def test_a_pair_gives_the_same_bits_whatever_surrounds_it():
    from daft_exprt import config
    from daft_exprt import evaluate as E
    lengths, refs, gens = _ragged()
    n_paths = [a + b - 1 for a, b in lengths]
    rows = list(range(len(lengths)))
    batch = _align(refs, gens)
    for b in rows:                                                                   # alone
        assert O.is_valid_path(batch[1][b, :batch[2][b]], *lengths[b])
        _same_rows(batch, _align([refs[b]], [gens[b]]), [b], [0], [n_paths[b]])
    _same_rows(batch, _align(refs, gens, extents=(1111, 1024)), rows, rows, n_paths)                   # other padded extents
    _same_rows(batch, _align(refs, gens, fill=np.nan), rows, rows, n_paths)                            # NaN in all padding
    _same_rows(batch, _align(refs, gens, max_workspace_bytes=1), rows, rows, n_paths)                  # one-pair sub-batches
    _same_rows(batch, _align(refs, gens), rows, rows, n_paths)                                         # a second call
    order = rows[::-1]                                                                                 # other neighbours
    _same_rows(batch, _align([refs[b] for b in order], [gens[b] for b in order]), order, rows, [n_paths[b] for b in order])
    old = config.POISON
    config.POISON = True
    try:
        E._DTW_WORKSPACE.clear()                                                                       # a fresh workspace, every code invalid
        _same_rows(batch, _align(refs, gens), rows, rows, n_paths)
    finally:
        config.POISON = old


def test_a_zero_length_row_is_nan_and_its_neighbours_are_unchanged():
    lengths, refs, gens = _ragged()
    batch = _align(refs, gens)
    for side in (0, 1):
        r, g = list(refs), list(gens)
        (r if side == 0 else g)[2] = (r if side == 0 else g)[2][:0]
        got = _align(r, g, extents=(700, 1000), fill=np.nan)
        assert np.isnan(got[0][2]) and got[2][2] == 0 and (got[1][2] == -1).all()
        keep = [0, 1, 3, 4, 5]
        _same_rows(batch, got, keep, keep, [sum(lengths[b]) - 1 for b in keep])


def test_non_finite_cepstra_still_give_a_monotone_path():
    ref, gen = O.real_pair(90, 70, 9)
    ref, gen = ref.copy(), gen.copy()
    ref[10:20], gen[33], ref[50, 3] = np.nan, np.inf, -np.inf
    total, path, path_len = _align([ref], [gen])
    assert O.is_valid_path(path[0, :int(path_len[0])], 90, 70) and not np.isfinite(total[0])


# ---- the cepstrum -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n_mel,n_coeffs', O.CEP_SHAPES)
def test_mel_cepstrum_against_the_oracle(n_mel, n_coeffs):
    from daft_exprt.evaluate import mel_cepstrum_batch
    frames = (300, 257, 1, 0)
    mels = [O.mel_case(n_mel, t, 100 * n_mel + t) for t in frames]
    x = np.full((len(frames), n_mel, 333), np.nan, dtype=np.float32)                 # NaN behind every row: nothing there is read
    for b, m in enumerate(mels):
        x[b, :, :m.shape[1]] = m
    n = torch.tensor(frames, dtype=torch.int64, device=DEV)
    cep = mel_cepstrum_batch(torch.from_numpy(x).to(DEV), n, n_coeffs)
    assert cep.shape == (len(frames), 333, n_coeffs) and cep.is_contiguous()
    cep = cep.cpu().numpy()
    worst = 0.0
    for b, m in enumerate(mels):
        t = m.shape[1]
        assert not cep[b, t:].any()                                                 # exact zeros past the length
        if t:
            worst = max(worst, float(np.abs(cep[b, :t] - O.mel_cepstrum(m, n_coeffs)).max()))
    print(f'n_mel {n_mel}, K {n_coeffs}: worst error {worst:.2e} (bound {TOL_CEP:.1e})')
    assert worst <= TOL_CEP
    alone = mel_cepstrum_batch(torch.from_numpy(mels[1][None]).to(DEV), n[1:2], n_coeffs).cpu().numpy()
    assert alone[0].tobytes() == cep[1, :257].tobytes()
    with pytest.raises(ValueError, match='K < n_mel'):
        mel_cepstrum_batch(torch.from_numpy(x).to(DEV), n, n_mel)


# ---- the scores along a path ------------------------------------------------------------------------------------------------------

def _scores(refs, gens, paths, lp_refs=None, lp_gens=None):
    ''' `dtw_path_scores_batch` on given paths (the oracle's own): NumPy (mcd, f0, vuv, voiced, used) '''
    from daft_exprt.evaluate import dtw_path_scores_batch
    r, n_r = _pad(refs)
    g, n_g = _pad(gens)
    P = r.shape[1] + g.shape[1] - 1
    path = np.full((len(refs), P, 2), -1, dtype=np.int32)
    for b, p in enumerate(paths):
        path[b, :len(p)] = p
    path_len = torch.tensor([len(p) for p in paths], dtype=torch.int32, device=DEV)
    lp_r = lp_g = None
    if lp_refs is not None:
        lp_r = _pad([x[:, None] for x in lp_refs], r.shape[1], np.nan)[0][:, :, 0].contiguous()
        lp_g = _pad([x[:, None] for x in lp_gens], g.shape[1], np.nan)[0][:, :, 0].contiguous()
    out = dtw_path_scores_batch(r, n_r, g, n_g, torch.from_numpy(path).to(DEV), path_len, lp_r, lp_g)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def test_path_scores_against_the_oracle_on_its_own_path():
    cases = O.score_cases()
    assert [c[0].split('-')[0] for c in cases] == ['mixed', 'all', 'disjoint', 'mixed']
    paths = [O.dtw(c[1], c[2])[1] for c in cases]
    refs, gens = [c[1] for c in cases], [c[2] for c in cases]
    mcd, f0, vuv, voiced, used = _scores(refs, gens, paths, [c[3] for c in cases], [c[4] for c in cases])
    for b, (name, ref, gen, lp_ref, lp_gen) in enumerate(cases):
        want = O.path_scores(paths[b], ref, gen, lp_ref, lp_gen)
        e_mcd = O.rel(float(mcd[b]), want['mcd_db'])
        print(f'{name}: mcd {float(mcd[b]):.5f} dB (error {e_mcd:.2e}), f0 rmse {float(f0[b]):.3f} cents (oracle {want["f0_rmse_cents"]:.3f}), '
              f'vuv {float(vuv[b]):.4f}, voiced pairs {int(voiced[b])} of {int(used[b])}')
        assert (int(voiced[b]), int(used[b])) == (want['voiced_pairs'], want['path_len']), name
        assert e_mcd <= TOL_MCD and abs(float(vuv[b]) - want['vuv_error']) <= VUV_ULP, name
        if name.startswith('disjoint'):
            assert want['voiced_pairs'] == 0 and math.isnan(f0[b]) and float(vuv[b]) == 1.0            # no doubly voiced pair
        else:
            assert O.rel(float(f0[b]), want['f0_rmse_cents']) <= TOL_F0, name
        if name.startswith('all'):
            assert int(voiced[b]) == len(paths[b]) and float(vuv[b]) == 0.0
    # null pitch pointers: the distortion is unchanged, the pitch outputs are NaN / 0
    plain = _scores(refs, gens, paths)
    assert plain[0].tobytes() == mcd.tobytes() and np.array_equal(plain[4], used)
    assert np.isnan(plain[1]).all() and np.isnan(plain[2]).all() and not plain[3].any()
    # an empty path beside a full one; the full one keeps its bits
    empty = _scores(refs[:2], gens[:2], [paths[0], paths[1][:0]], [c[3] for c in cases[:2]], [c[4] for c in cases[:2]])
    assert np.isnan(empty[0][1]) and np.isnan(empty[1][1]) and np.isnan(empty[2][1]) and empty[3][1] == 0 and empty[4][1] == 0
    assert all(empty[k][0].tobytes() == (mcd, f0, vuv, voiced, used)[k][0].tobytes() for k in range(5))


def test_scores_from_mels_and_the_single_pair_form():
    from daft_exprt.evaluate import DTW_KEYS, dtw_scores_batch, mcd_dtw
    mel_a, mel_b = O.mel_case(80, 120, 1), O.mel_case(80, 95, 2)
    ref, gen = O.mel_cepstrum(mel_a, 13), O.mel_cepstrum(mel_b, 13)
    total, path = O.dtw(ref, gen)
    want = O.path_scores(path, ref, gen)
    x = np.zeros((2, 80, 130), dtype=np.float32)
    x[0, :, :120], x[1, :, :95] = mel_a, mel_b
    x = torch.from_numpy(x).to(DEV)
    n = torch.tensor([120, 95], dtype=torch.int64, device=DEV)
    got = dtw_scores_batch(x[:1], n[:1], x[1:], n[1:])
    assert tuple(got) == DTW_KEYS and all(v.shape == (1,) and v.is_cuda for v in got.values())
    got = {k: v.cpu().tolist()[0] for k, v in got.items()}
    # the float32 cepstra move every d by up to sqrt(K) x F32_CEP_ERR; relative to the mean d that is the bound on the MCD
    slack = O.TOL_FACTOR * math.sqrt(13) * O.F32_CEP_ERR / (want['mcd_db'] / O.MCD_SCALE)
    print(f'mcd {got["mcd_db"]:.5f} dB, oracle {want["mcd_db"]:.5f}, error {O.rel(got["mcd_db"], want["mcd_db"]):.2e} (bound {TOL_MCD + slack:.1e})')
    assert O.rel(got['mcd_db'], want['mcd_db']) <= TOL_MCD + slack
    assert (got['frames_ref'], got['frames_gen'], got['voiced_pairs']) == (120, 95, 0)
    assert max(120, 95) <= got['path_len'] <= 120 + 95 - 1 and math.isnan(got['f0_rmse_cents']) and math.isnan(got['vuv_error'])
    single = mcd_dtw(mel_a.astype(np.float64), mel_b.astype(np.float64))
    assert isinstance(single, float) and single == got['mcd_db']
    assert math.isnan(mcd_dtw(mel_a, mel_b[:, :0]))
    assert mcd_dtw(mel_a, mel_a) == 0.0


# ---- end to end -------------------------------------------------------------------------------------------------------------------

def _tiny_model(golden_dir):
    from daft_exprt.model import DaftExprt
    fx = np.load(os.path.join(golden_dir, 'data_loader.npz'))
    hp = make_hparams(compute_dtype='fp32')
    hp.stats = {f'spk {i}': {'energy': {'mean': float(fx['stats_energy_mean'][i]), 'std': float(fx['stats_energy_std'][i])},
                             'pitch': {'mean': float(fx['stats_pitch_mean'][i]), 'std': float(fx['stats_pitch_std'][i])}} for i in range(11)}
    torch.manual_seed(1234)
    model = DaftExprt(hp)
    with torch.no_grad():   # random duration head: centre it so that the utterances have a sensible length
        model.prosody_predictor.projection.linear_layer.weight[0].mul_(0.05)
        model.prosody_predictor.projection.linear_layer.bias.copy_(torch.tensor([0.08, 0., 0.]))
    return model, hp


def _file_list(golden_dir, tmp_path):
    ''' tests/golden/train_list.txt with absolute feature directories '''
    path = tmp_path / 'validation.txt'
    lines = [line.strip().split('|') for line in open(os.path.join(golden_dir, 'train_list.txt')) if line.strip()]
    path.write_text(''.join(f'{os.path.join(golden_dir, d)}|{f}|{s}\n' for d, f, s in lines))
    return str(path), [f'{os.path.basename(d)}/{f}' for d, f, _ in lines], [int(s) for _, _, s in lines]


def _batch(list_file, hp, count=None):
    from daft_exprt.data_loader import DaftExprtDataCollate, DaftExprtDataLoader
    data = DaftExprtDataLoader(list_file, hp, shuffle=False)
    return DaftExprtDataCollate(hp)([data[i] for i in range(len(data) if count is None else count)])


def test_copy_synthesis_scores(golden_dir, tmp_path):
    from daft_exprt import evaluate as E
    model, hp = _tiny_model(golden_dir)
    model = model.cuda(0)
    list_file, names, _ = _file_list(golden_dir, tmp_path)
    batch = _batch(list_file, hp)
    scores = E.copy_synthesis_scores(model, batch, hp)
    assert tuple(scores) == E.COPY_LEVELS == ('mel', 'audio')
    assert all(tuple(scores[level]) == E.DTW_KEYS and all(v.shape == (5,) and v.is_cuda for v in scores[level].values()) for level in scores)
    inputs, mel, n_frames, wavs, n_samples = E.copy_synthesis(model, batch, hp)
    direct = E.dtw_scores_batch(inputs[8], inputs[9], mel, n_frames)
    host = {level: {k: v.cpu().numpy() for k, v in scores[level].items()} for level in scores}
    assert host['mel']['mcd_db'].tobytes() == direct['mcd_db'].cpu().numpy().tobytes()            # the decoder's mel, nothing else
    recorded, generated = batch[9].numpy(), n_frames.cpu().numpy()
    for level in E.COPY_LEVELS:
        got = host[level]
        assert np.array_equal(got['frames_ref'], recorded) and np.isfinite(got['mcd_db']).all() and (got['mcd_db'] > 0).all()
        assert (got['path_len'] >= np.maximum(got['frames_ref'], got['frames_gen'])).all()
        assert (got['path_len'] <= got['frames_ref'] + got['frames_gen'] - 1).all()
    assert np.array_equal(host['mel']['frames_gen'], generated)
    assert np.isnan(host['mel']['f0_rmse_cents']).all() and np.isnan(host['mel']['vuv_error']).all() and not host['mel']['voiced_pairs'].any()
    # the analysis of the waveform: the front-end's frame count of frames * hop samples (Griffin-Lim keeps that length)
    assert (host['audio']['frames_gen'] <= n_samples.cpu().numpy() // hp.hop_length + 1).all() and (host['audio']['frames_gen'] > 0).all()
    assert (np.abs(host['audio']['frames_gen'] - generated) <= hp.filter_length // hp.hop_length + 1).all()
    assert ((host['audio']['vuv_error'] >= 0) & (host['audio']['vuv_error'] <= 1)).all()
    assert (host['audio']['voiced_pairs'] <= host['audio']['path_len']).all()
    for i in range(5):
        print({level: {k: host[level][k][i].item() for k in E.DTW_KEYS} for level in host})


def _records_equal(entry, api, row):
    for level, scores in api.items():
        for key, values in scores.items():
            want = values[row]
            want = None if isinstance(want, float) and math.isnan(want) else want
            assert entry[level][key] == want, (level, key, entry[level][key], want)


def _check_summary(report, n_files):
    from daft_exprt.evaluate import COPY_LEVELS, DTW_KEYS
    files, summary = report['files'], report['summary']
    assert summary['files'] == n_files == len(files)
    assert sum(s['files'] for s in summary['speakers'].values()) == n_files
    for level in COPY_LEVELS:
        for key in DTW_KEYS:
            finite = [e[level][key] for e in files.values() if e[level][key] is not None]
            s = summary[level][key]
            assert s['count'] == len(finite) == sum(sp[level][key]['count'] for sp in summary['speakers'].values())
            if finite:
                assert s['mean'] == pytest.approx(float(np.mean(finite))) and s['median'] == pytest.approx(float(np.median(finite)))
            else:
                assert s['mean'] is None and s['median'] is None
    for speaker, table in summary['speakers'].items():
        mine = [e for e in files.values() if str(e['speaker_id']) == speaker]
        assert table['files'] == len(mine) and table['mel']['mcd_db']['mean'] == pytest.approx(float(np.mean([e['mel']['mcd_db'] for e in mine])))


def _run_cli(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'evaluate.py'), *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r


def test_evaluate_cli(golden_dir, tmp_path):
    from daft_exprt import evaluate as E
    model, hp = _tiny_model(golden_dir)
    ckpt = str(tmp_path / 'DaftExprt_test')
    torch.save({'iteration': 0, 'state_dict': {f'module.{k}': v for k, v in model.state_dict().items()},
                'config_params': dict(vars(hp))}, ckpt)
    list_file, names, speakers = _file_list(golden_dir, tmp_path)
    out_dir = str(tmp_path / 'out')
    r = _run_cli('-chk', ckpt, '-vf', list_file, '-out', out_dir)
    report = json.load(open(os.path.join(out_dir, 'copy_synthesis.json')))
    assert report['audio'] == 'griffin-lim' and list(report['files']) == names
    assert [report['files'][n]['speaker_id'] for n in names] == speakers and sorted(report['summary']['speakers']) == ['0', '3', '7']
    _check_summary(report, 5)
    assert 'mel mcd_db: mean' in r.stderr and 'audio f0_rmse_cents' in r.stderr
    # the same batch through the API, with the weights the checkpoint holds
    model = model.cuda(0)
    batch = _batch(list_file, hp)
    api = {level: {k: v.cpu().tolist() for k, v in s.items()} for level, s in E.copy_synthesis_scores(model, batch, hp).items()}
    for row, (features_dir, feature_file) in enumerate(zip(batch[11], batch[12])):
        _records_equal(report['files'][f'{os.path.basename(features_dir)}/{feature_file}'], api, row)
    two = str(tmp_path / 'two')
    _run_cli('-chk', ckpt, '-vf', list_file, '-out', two, '-n', '2', '-bs', '1', '-nc', '20')
    report = json.load(open(os.path.join(two, 'copy_synthesis.json')))
    assert list(report['files']) == names[:2]
    _check_summary(report, 2)


def test_evaluate_cli_with_a_vocoder(golden_dir, tmp_path):
    from tests import vocoder_oracle as VO
    from tests.test_gpu_vocoder import SURFACE, _surface_weights
    model, hp = _tiny_model(golden_dir)
    ckpt = str(tmp_path / 'DaftExprt_test')
    torch.save({'iteration': 0, 'state_dict': dict(model.state_dict()), 'config_params': dict(vars(hp))}, ckpt)
    voc_dir = tmp_path / 'hifigan'
    voc_dir.mkdir()
    torch.save({'generator': VO.state_dict(_surface_weights(), 'parametrizations')}, str(voc_dir / 'g_00000001'))
    (voc_dir / 'config.json').write_text(json.dumps(SURFACE))
    list_file, names, _ = _file_list(golden_dir, tmp_path)
    out_dir = str(tmp_path / 'out')
    _run_cli('-chk', ckpt, '-vf', list_file, '-out', out_dir, '-n', '3', '-voc', str(voc_dir / 'g_00000001'))
    report = json.load(open(os.path.join(out_dir, 'copy_synthesis.json')))
    assert report['audio'] == 'hifi-gan' and list(report['files']) == names[:3]
    _check_summary(report, 3)
    for entry in report['files'].values():                                         # the vocoder writes frames * hop samples
        assert entry['audio']['frames_gen'] == entry['mel']['frames_gen'] + 1 and entry['audio']['mcd_db'] > 0
