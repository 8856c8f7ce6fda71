"""Host-side checks of the copy-synthesis scores: the float64 oracle (tests/dtw_oracle.py) pinned against an enumeration of every
monotone path and three cases worked by hand, the error of the kernels' arithmetic restated in float32 -- the figures the GPU
tests' tolerances are built on --, the library's symbols and argument errors, and the command line of scripts/evaluate.py."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import dtw_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('dx_dtw_max_len', 'dx_mel_cepstrum', 'dx_dtw_align', 'dx_dtw_path_scores')


# ---- the oracle, pinned independently of itself ---------------------------------------------------------------------------------

def _all_paths(n_ref, n_gen):
    ''' every monotone path from (0, 0) to (n_ref-1, n_gen-1) with steps (1, 1), (1, 0), (0, 1), as tuples of cells '''
    def walk(i, j):
        if (i, j) == (n_ref - 1, n_gen - 1):
            yield ((i, j),)
            return
        for di, dj in ((1, 1), (1, 0), (0, 1)):
            if i + di < n_ref and j + dj < n_gen:
                for rest in walk(i + di, j + dj):
                    yield ((i, j),) + rest
    return list(walk(0, 0))


def _cost(path, ref, gen):
    return sum(float(np.sqrt(np.sum((ref[i] - gen[j]) ** 2))) for i, j in path)


def _prefix_min(ref, gen):
    ''' D by brute force: for every cell the minimum over all enumerated monotone paths from (0, 0) to it '''
    D = {}
    for i in range(ref.shape[0]):
        for j in range(gen.shape[0]):
            D[i, j] = min(_cost(p, ref, gen) for p in _all_paths(i + 1, j + 1))
    return D


def _selected_path(D, n_ref, n_gen):
    i, j = n_ref - 1, n_gen - 1
    cells = [(i, j)]
    while (i, j) != (0, 0):
        cands = [c for c in ((i - 1, j - 1), (i - 1, j), (i, j - 1)) if c[0] >= 0 and c[1] >= 0]
        best = cands[0]
        for c in cands[1:]:
            if D[c] < D[best]:                                                      # strictly smaller replaces
                best = c
        i, j = best
        cells.append(best)
    return tuple(cells[::-1])


@pytest.mark.parametrize('kind', ['random', 'tied'])
def test_oracle_total_is_the_minimum_over_all_monotone_paths(kind):
    rng = np.random.RandomState(5 if kind == 'random' else 6)
    seen_ties = 0
    for n_ref, n_gen in itertools.product(range(1, 6), repeat=2):
        if kind == 'random':
            ref, gen = rng.standard_normal((n_ref, 3)), rng.standard_normal((n_gen, 3))
        else:                                                                       # integers 0..2, K = 1: every cost exact, ties everywhere
            ref, gen = rng.randint(0, 3, size=(n_ref, 1)).astype(np.float64), rng.randint(0, 3, size=(n_gen, 1)).astype(np.float64)
        paths = _all_paths(n_ref, n_gen)
        costs = [_cost(p, ref, gen) for p in paths]
        total, path = O.dtw(ref, gen)
        assert O.is_valid_path(path, n_ref, n_gen)
        assert tuple(map(tuple, path)) in paths
        if kind == 'tied':
            assert total == min(costs), (n_ref, n_gen)
            assert O.path_cost64(path, ref, gen) == total
            seen_ties += sum(c == min(costs) for c in costs) > 1
            assert tuple(map(tuple, path)) == _selected_path(_prefix_min(ref, gen), n_ref, n_gen), (n_ref, n_gen)
        else:
            assert abs(total - min(costs)) <= 1e-12 * max(1.0, min(costs)), (n_ref, n_gen)
            assert tuple(map(tuple, path)) == paths[int(np.argmin(costs))], (n_ref, n_gen)       # no ties: the one minimal path
    assert kind == 'random' or seen_ties >= 10


def test_three_cases_worked_by_hand():
    col = lambda *v: np.asarray(v, dtype=np.float64)[:, None]
    # 1. ref 0 1 2 against itself: d = |i - j|, the diagonal costs 0
    total, path = O.dtw(col(0, 1, 2), col(0, 1, 2))
    assert total == 0.0 and path.tolist() == [[0, 0], [1, 1], [2, 2]]
    # 2. all-equal sequences, 2 x 3: every path costs 0.  D = 0 everywhere; from (1, 2) the diagonal (0, 1) is taken first, then
    #    row 0 forces (0, 0): the tie rule picks (0,0) (0,1) (1,2), not (0,0) (1,1) (1,2) or any three-step path
    total, path = O.dtw(col(4, 4), col(4, 4, 4))
    assert total == 0.0 and path.tolist() == [[0, 0], [0, 1], [1, 2]]
    # 3. ref 1 3, gen 1 2 3:  d = [[0 1 2] [2 1 0]];  D row 0 = 0 1 3;  D(1,0) = 2;  D(1,1) = 1 + min(0, 1, 2) = 1 via the diagonal;
    #    D(1,2) = 0 + min(D(0,1) = 1, D(0,2) = 3, D(1,1) = 1) = 1: diagonal and left tie at 1, the diagonal comes first
    total, path = O.dtw(col(1, 3), col(1, 2, 3))
    assert total == 1.0 and path.tolist() == [[0, 0], [0, 1], [1, 2]]
    scores = O.path_scores(path, col(1, 3), col(1, 2, 3), lp_ref=[5.0, 0.0], lp_gen=[5.0, 5.0 + np.log(2.0) / 12.0, 0.0])
    # d along the path 0 1 0 -> mean 1/3; pairs (voiced, voiced) 0 cents, (voiced, voiced) 100 cents, (unvoiced, unvoiced)
    assert scores['path_len'] == 3 and scores['voiced_pairs'] == 2 and scores['vuv_error'] == 0.0
    assert abs(scores['mcd_db'] - 10.0 * np.sqrt(2.0) / np.log(10.0) / 3.0) <= 1e-14
    lp = np.float32(5.0 + np.log(2.0) / 12.0)
    assert abs(scores['f0_rmse_cents'] - np.sqrt(0.5) * 1200.0 / np.log(2.0) * (float(lp) - 5.0)) <= 1e-9
    assert abs(scores['f0_rmse_cents'] - np.sqrt(0.5) * 100.0) <= 1e-3
    empty = O.path_scores(np.zeros((0, 2)), col(1), col(1))
    assert empty['path_len'] == 0 and np.isnan(empty['mcd_db']) and np.isnan(O.dtw(col(1)[:0], col(1))[0])


def test_cepstrum_is_the_orthonormal_dct_without_c0():
    table = O.dct_table(8, 7)
    full = np.vstack([np.full((1, 8), np.sqrt(1.0 / 8.0)), table])                  # c0 put back: an orthonormal basis
    assert np.abs(full @ full.T - np.eye(8)).max() <= 1e-14
    mel = O.mel_case(8, 5, 1).astype(np.float64)
    assert np.abs(O.mel_cepstrum(mel + 3.0, 7) - O.mel_cepstrum(mel, 7)).max() <= 1e-12      # the level lives in c0 only


# ---- the float32 restatement: the measured figures the GPU bounds stand on --------------------------------------------------------

def test_float32_restatement_stays_within_the_recorded_errors():
    ''' the bounds of tests/test_gpu_dtw.py are TOL_FACTOR times these four constants '''
    worst = dict(total=0.0, mcd=0.0, cep=0.0, f0=0.0)
    for name, ref, gen in O.real_cases():
        total, path = O.dtw(ref, gen)
        total32, path32 = O.dtw(ref, gen, dtype=np.float32)
        assert np.asarray(total32).dtype == np.float32 and O.is_valid_path(path32, len(ref), len(gen))
        assert abs(O.path_cost64(path, ref, gen) - total) <= 1e-9 * total
        near = O.rel(O.path_cost64(path32, ref, gen), total)                        # a float32 near-tie may go the other way
        worst['total'] = max(worst['total'], O.rel(float(total32), total), near)
        print(f'{name}: total {total:.6f}, float32 error {O.rel(float(total32), total):.2e}, float32 path cost error {near:.2e}, '
              f'paths {"equal" if path32.tolist() == path.tolist() else "differ"}')
    for name, ref, gen, lp_ref, lp_gen in O.score_cases():
        _, path = O.dtw(ref, gen)
        want, got = O.path_scores(path, ref, gen, lp_ref, lp_gen), O.path_scores_f32(path, ref, gen, lp_ref, lp_gen)
        assert (got['voiced_pairs'], got['path_len']) == (want['voiced_pairs'], want['path_len'])
        worst['mcd'] = max(worst['mcd'], O.rel(got['mcd_db'], want['mcd_db']))
        if want['voiced_pairs']:
            worst['f0'] = max(worst['f0'], O.rel(got['f0_rmse_cents'], want['f0_rmse_cents']))
        else:
            assert np.isnan(want['f0_rmse_cents']) and np.isnan(got['f0_rmse_cents'])
    for n_mel, k in O.CEP_SHAPES:
        mel = O.mel_case(n_mel, 300, n_mel)
        worst['cep'] = max(worst['cep'], float(np.abs(O.mel_cepstrum_f32(mel, k) - O.mel_cepstrum(mel, k)).max()))
    print('float32 restatement: ' + ', '.join(f'{k} {v:.3e}' for k, v in worst.items()))
    recorded = dict(total=O.F32_TOTAL_ERR, mcd=O.F32_MCD_ERR, cep=O.F32_CEP_ERR, f0=O.F32_F0_ERR)
    for key, value in worst.items():
        assert value <= recorded[key], (key, value, recorded[key])
        assert value >= recorded[key] / 2, (key, value, recorded[key])              # the measured figures, not slack


def test_exact_cases_are_exact_in_float32():
    ''' what lets the GPU test ask for equality: integer cepstra give the same totals and paths in float32 as in float64 '''
    for name, ref, gen in O.exact_cases():
        total, path = O.dtw(ref, gen)
        total32, path32 = O.dtw(ref, gen, dtype=np.float32)
        assert float(total32) == total and total == round(total) and total < 2 ** 24, name
        assert path32.tolist() == path.tolist(), name


# ---- the library -------------------------------------------------------------------------------------------------------------------

def test_library_exports_the_symbols_and_the_header_declares_them():
    from daft_exprt import _hip as H
    declared = {name for name, _, _ in H.header_prototypes()}
    lib = H.lib()
    for name in SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name
    assert lib.dx_dtw_max_len() == O.MAX_LEN == lib.dx_curve_pcc_max_len()
    assert lib.dx_abi_version() == 13


def test_argument_errors_are_codes_before_any_launch():
    ''' no device is touched: the entry points refuse the arguments first '''
    from daft_exprt import _hip as H
    lib = H.lib()
    big = O.MAX_LEN + 1
    assert lib.dx_mel_cepstrum(None, 80 * 64, 64, 8, 8, 8, 1, 80, 64, 13, None) == -1 and b'null' in lib.dx_last_error()
    assert lib.dx_mel_cepstrum(8, 80 * 64, 64, 8, 8, 8, 1, 80, 64, 80, None) == -2 and b'K < n_mel' in lib.dx_last_error()
    assert lib.dx_mel_cepstrum(8, 80 * 64, 64, 8, 8, 8, 1, 80, 64, 0, None) == -2
    assert lib.dx_dtw_align(8, 8, 8, None, 8, 8, 8, 8, 64 * 16, 1, 64, 64, 13, None) == -1 and b'null' in lib.dx_last_error()
    assert lib.dx_dtw_align(8, 8, 8, 8, 8, 8, 8, 8, big * 16, 1, big, 64, 13, None) == -5 and b'4096' in lib.dx_last_error()
    assert lib.dx_dtw_align(8, 8, 8, 8, 8, 8, 8, 8, big * 16, 1, 64, big, 13, None) == -5
    assert lib.dx_dtw_align(8, 8, 8, 8, 8, 8, 8, 8, 64 * 16 - 1, 1, 64, 64, 13, None) == -2 and b'ws_stride' in lib.dx_last_error()
    assert lib.dx_dtw_path_scores(8, 8, 8, 8, None, 8, None, 0, None, 0, 8, 8, 8, 8, 8, 1, 64, 64, 13, None) == -1
    assert lib.dx_dtw_path_scores(8, 8, 8, 8, 8, 8, None, 0, None, 0, 8, 8, 8, 8, 8, 1, big, 64, 13, None) == -5
    assert lib.dx_dtw_path_scores(8, 8, 8, 8, 8, 8, 8, 63, 8, 64, 8, 8, 8, 8, 8, 2, 64, 64, 13, None) == -2


def test_host_wrappers_refuse_host_tensors():
    import torch
    from daft_exprt import evaluate as E
    assert E.DTW_KEYS == ('mcd_db', 'f0_rmse_cents', 'vuv_error', 'voiced_pairs', 'path_len', 'frames_ref', 'frames_gen')
    assert E.SCORE_KEYS == ('pitch_pcc', 'energy_pcc', 'voiced_ref', 'voiced_gen', 'frames_ref', 'frames_gen')
    n = torch.tensor([4], dtype=torch.int64)
    with pytest.raises(RuntimeError, match='device tensors'):
        E.mel_cepstrum_batch(torch.zeros(1, 80, 4), n)
    with pytest.raises(RuntimeError, match='device tensors'):
        E.dtw_align_batch(torch.zeros(1, 4, 13), n, torch.zeros(1, 4, 13), n)
    with pytest.raises(RuntimeError, match='device tensors'):
        E.dtw_scores_batch(torch.zeros(1, 80, 4), n, torch.zeros(1, 80, 4), n)


# ---- scripts/evaluate.py ---------------------------------------------------------------------------------------------------------

def _cli(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'evaluate.py'), *args], capture_output=True, text=True, timeout=120)


def test_cli_arguments(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    try:
        import evaluate as cli
    finally:
        sys.path.pop(0)
    args = cli.parse_args(['-chk', 'c', '-vf', 'v', '-out', 'o'])
    assert (args.checkpoint, args.validation_files, args.output_dir) == ('c', 'v', 'o')
    assert (args.batch_size, args.vocoder, args.vocoder_config, args.max_utterances, args.n_coeffs) == (50, None, None, None, 13)
    args = cli.parse_args(['-chk', 'c', '-vf', 'v', '-out', 'o', '-bs', '7', '-voc', 'g', '-vcfg', 'j', '-n', '2', '-nc', '20'])
    assert (args.batch_size, args.vocoder, args.vocoder_config, args.max_utterances, args.n_coeffs) == (7, 'g', 'j', 2, 20)
    for missing in (['-vf', 'v', '-out', 'o'], ['-chk', 'c', '-out', 'o'], ['-chk', 'c', '-vf', 'v']):
        with pytest.raises(SystemExit):
            cli.parse_args(missing)


def test_cli_names_a_missing_list_or_checkpoint(tmp_path):
    listing = tmp_path / 'validation.txt'
    listing.write_text('dir|utt|0\n')
    no_ckpt, no_list = str(tmp_path / 'no_such_checkpoint'), str(tmp_path / 'no_such_list.txt')
    r = _cli('-chk', no_ckpt, '-vf', str(listing), '-out', str(tmp_path / 'out'))
    assert r.returncode != 0 and no_ckpt in r.stderr and 'Traceback' not in r.stderr
    ckpt = tmp_path / 'ckpt'
    ckpt.write_bytes(b'')
    r = _cli('-chk', str(ckpt), '-vf', no_list, '-out', str(tmp_path / 'out'))
    assert r.returncode != 0 and no_list in r.stderr and 'Traceback' not in r.stderr
    assert not (tmp_path / 'out').exists()
