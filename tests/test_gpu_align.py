"""`dx_active_span`, `dx_dtw_transfer` (csrc/align.hip) and what daft_exprt/align.py builds on them.

The kernels are integer decisions: they must equal tests/align_oracle.py bit for bit, with poisoned outputs, alone and in a batch,
with the tight and with a larger padded extent.  `transfer_durations` must recover the boundaries of a constructed warp exactly:
a recording made of the synthesis' own frames, each repeated 1 to 3 times, has one zero-cost path (the frames are distinct), so
every symbol must get exactly the repeats of its frames.  `align_batch` and `align_data_set` run on a random-init model and
fabricated recordings: the invariants, determinism, and the round trip through `extract_features`."""
import functools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import align_oracle as A
from tests import dtw_oracle as O
from tests.util import make_hparams

DEV = 'cuda:0'
POISON = -77


# ---- dx_active_span -----------------------------------------------------------------------------------------------------------------

def _span_dev(rows, ns, rel_db, extent=None):
    ''' (begin, end) NumPy of one launch over right-padded rows, the outputs poisoned first '''
    from daft_exprt import _hip as H
    T = max(len(r) for r in rows) if extent is None else extent
    x = np.full((len(rows), T), 3e7, dtype=np.float32)
    for b, r in enumerate(rows):
        x[b, :len(r)] = r
    energy = torch.from_numpy(x).to(DEV)
    n = torch.tensor(ns, dtype=torch.int64, device=DEV)
    begin = torch.full((len(rows),), POISON, dtype=torch.int64, device=DEV)
    end = torch.full((len(rows),), POISON, dtype=torch.int64, device=DEV)
    H.check(H.lib().dx_active_span(H.ptr(energy), energy.stride(0), H.ptr(n), float(rel_db), H.ptr(begin), H.ptr(end), len(rows), T,
                                   H.stream()))
    return begin.cpu().numpy(), end.cpu().numpy()


def test_active_span_equals_the_oracle():
    from daft_exprt.align import active_span_batch
    cases = A.active_span_cases()
    for rel_db in sorted({c[3] for c in cases}):
        mine = [c for c in cases if c[3] == rel_db]
        want = [A.active_span(e, n, rel_db) for _, e, n, _ in mine]
        rows, ns = [c[1] for c in mine], [c[2] for c in mine]
        batch = _span_dev(rows, ns, rel_db)
        wide = _span_dev(rows, ns, rel_db, extent=max(len(r) for r in rows) + 261)
        for b, (name, e, n, _) in enumerate(mine):
            alone = _span_dev([e], [n], rel_db)
            print(f'{name}: {want[b]} batch {(batch[0][b], batch[1][b])} alone {(alone[0][0], alone[1][0])}')
            assert (int(batch[0][b]), int(batch[1][b])) == want[b], name
            assert (int(wide[0][b]), int(wide[1][b])) == want[b], name
            assert (int(alone[0][0]), int(alone[1][0])) == want[b], name
    # the wrapper, on rows longer than one pass of the workgroup
    rng = np.random.RandomState(2)
    x = (rng.uniform(size=(3, 700)) * 1e-3).astype(np.float32)
    x[0, 300:650] += 1.0
    x[1, 699] = 4.0
    x[2, 0] = 2.0
    ns = [700, 700, 513]
    begin, end = active_span_batch(torch.from_numpy(x).to(DEV), torch.tensor(ns, dtype=torch.int64, device=DEV), -40.0)
    assert list(zip(begin.tolist(), end.tolist())) == [A.active_span(x[b], ns[b]) for b in range(3)] == [(300, 650), (699, 700), (0, 1)]


def test_active_span_argument_errors():
    from daft_exprt import _hip as H
    lib = H.lib()
    e = torch.zeros((1, 4), dtype=torch.float32, device=DEV)
    n = torch.tensor([4], dtype=torch.int64, device=DEV)
    out = torch.zeros((2,), dtype=torch.int64, device=DEV)
    assert lib.dx_active_span(None, 4, H.ptr(n), -40.0, H.ptr(out), H.ptr(out[1:]), 1, 4, None) == -1 and b'null' in lib.dx_last_error()
    assert lib.dx_active_span(H.ptr(e), 4, H.ptr(n), -40.0, H.ptr(out), H.ptr(out[1:]), 1, -4, None) == -2
    assert lib.dx_active_span(H.ptr(e), 4, H.ptr(n), 3.0, H.ptr(out), H.ptr(out[1:]), 1, 4, None) == -1 and b'rel_db' in lib.dx_last_error()


# ---- dx_dtw_transfer ------------------------------------------------------------------------------------------------------------------

def _transfer_dev(cases, min_frames, pad=(0, 0, 0)):
    ''' cases: [(path, n_ref, n_gen, durations, n_symbols or None)] -> (rec (B, L), moved, status) NumPy of one launch: the tight
        extents plus `pad` (T_ref, T_gen, L), -1 behind path_len, large durations behind n_symbols, the outputs poisoned first '''
    from daft_exprt import _hip as H
    B = len(cases)
    T_ref = max(1, max(c[1] for c in cases)) + pad[0]
    T_gen = max(1, max(c[2] for c in cases)) + pad[1]
    L = max(1, max(len(c[3]) for c in cases)) + pad[2]
    P = T_ref + T_gen - 1
    path = np.full((B, P, 2), -1, dtype=np.int32)
    path_len = np.zeros((B,), dtype=np.int32)
    dur = np.full((B, L), 1 << 40, dtype=np.int64)
    n_sym = np.zeros((B,), dtype=np.int64)
    for b, (cells, n_ref, n_gen, durations, n_symbols) in enumerate(cases):
        assert len(cells) <= P, (len(cells), P)
        path[b, :len(cells)] = np.asarray(cells, dtype=np.int32).reshape(-1, 2)
        path_len[b] = len(cells)
        dur[b, :len(durations)] = durations
        n_sym[b] = len(durations) if n_symbols is None else n_symbols
    path, path_len, dur, n_sym = (torch.from_numpy(a).to(DEV) for a in (path, path_len, dur, n_sym))
    rec =torch.full((B, L), POISON, dtype=torch.int64, device=DEV)
    moved = torch.full((B,), POISON, dtype=torch.int32, device=DEV)
    status = torch.full((B,), POISON, dtype=torch.int32, device=DEV)
    n_ref = torch.tensor([c[1] for c in cases], dtype=torch.int64, device=DEV)
    n_gen = torch.tensor([c[2] for c in cases], dtype=torch.int64, device=DEV)
    H.check(H.lib().dx_dtw_transfer(H.ptr(path), H.ptr(path_len), H.ptr(n_ref), H.ptr(n_gen), H.ptr(dur), H.ptr(n_sym), H.ptr(rec), H.ptr(moved), H.ptr(status), B, T_ref, T_gen, L, int(min_frames), H.stream()))
    return rec.cpu().numpy(), moved.cpu().numpy(), status.cpu().numpy()


def _check_transfer(names, cases, min_frames):
    ''' the batch, the batch with larger extents and every pair alone against the oracle; every output element is written '''
    want = [A.dtw_transfer(c[0], c[1], c[2], c[3][:len(c[3]) if c[4] is None else c[4]], min_frames) for c in cases]
    batch = _transfer_dev(cases, min_frames)
    wide = _transfer_dev(cases, min_frames, pad=(3, 70, 67))
    for b, (name, c) in enumerate(zip(names, cases)):
        alone = _transfer_dev([c], min_frames)
        n = len(want[b][0])
        print(f'{name} m={min_frames}: oracle {want[b]}, device {batch[0][b].tolist()} moved {batch[1][b]} status {batch[2][b]}')
        for got, row in ((batch, b), (wide, b), (alone, 0)):
            assert got[0][row, :n].tolist() == want[b][0] and not got[0][row, n:].any(), name
            assert (int(got[1][row]), int(got[2][row])) == want[b][1:], name


def test_transfer_hand_built_cases_equal_the_oracle():
    cases = A.transfer_cases()
    for m in sorted({c[5] for c in cases}):
        mine = [c for c in cases if c[5] == m]
        _check_transfer([c[0] for c in mine], [(c[1], c[2], c[3], c[4], None) for c in mine], m)
        for c in mine:                                                  # and the answers worked out by hand
            got = _transfer_dev([(c[1], c[2], c[3], c[4], None)], m)
            assert (got[0][0, :len(c[4])].tolist(), int(got[1][0]), int(got[2][0])) == c[6], c[0]


def test_transfer_symbol_counts_and_row_extents():
    diagonal = [(i, i) for i in range(12)]
    full = [1] * 12
    cases = [(diagonal, 12, 12, full, None),                            # n_symbols == L: the whole row
             (diagonal, 12, 12, full, 0),                               # n_symbols == 0: nothing sounding, status 2
             (diagonal, 12, 12, [3, 9] + [5] * 10, 2),                  # durations behind n_symbols are not read
             (diagonal[:5], 5, 5, [5], None)]
    _check_transfer(['L', '0', 'behind', 'one-symbol'], cases, 1)
    _check_transfer(['L', '0', 'behind', 'one-symbol'], cases, 3)
    # more symbols than a wave holds, more path entries than a wave holds: the scans carry over
    rng = np.random.RandomState(8)
    durations = rng.randint(0, 3, size=150).tolist()
    n_gen = sum(durations)
    ref, gen = O.real_pair(130, n_gen, 91)
    _, path = O.dtw(ref, gen)
    for m in (1, 3):
        _check_transfer(['150-symbols'], [(path.tolist(), 130, n_gen, durations, None)], m)


@functools.lru_cache(maxsize=None)
def _dtw_cases():
    rng = np.random.RandomState(21)
    out = []
    for n, (n_ref, n_gen) in enumerate(((40, 31), (64, 50), (25, 60), (33, 33), (9, 64))):
        ref, gen = O.real_pair(n_ref, n_gen, 5000 + n)
        _, path = O.dtw(ref, gen)
        cuts = rng.randint(0, n_gen + 1, size=int(rng.randint(2, 11)))
        cuts = np.sort(np.concatenate([cuts, cuts[:1]]))                                 # a repeated cut: a silent symbol
        durations = np.diff(np.concatenate([[0], cuts, [n_gen]])).tolist()
        out.append((f'{n_ref}x{n_gen}', path.tolist(), n_ref, n_gen, durations))
    return out


@pytest.mark.parametrize('min_frames', [1, 3])
def test_transfer_over_dtw_paths_equals_the_oracle(min_frames):
    cases = _dtw_cases()
    assert any(0 in c[4] for c in cases)
    _check_transfer([c[0] for c in cases], [(c[1], c[2], c[3], c[4], None) for c in cases], min_frames)


def test_transfer_argument_errors_and_the_wrapper():
    from daft_exprt import _hip as H
    from daft_exprt.align import dtw_transfer_batch
    lib = H.lib()
    t = torch.zeros((8,), dtype=torch.int64, device=DEV)
    p = H.ptr(t)
    assert lib.dx_dtw_transfer(None, p, p, p, p, p, p, p, p, 1, 2, 2, 1, 1, None) == -1 and b'null' in lib.dx_last_error()
    assert lib.dx_dtw_transfer(p, p, p, p, p, p, p, p, p, 1, 2, 2, 0, 1, None) == -2
    assert lib.dx_dtw_transfer(p, p, p, p, p, p, p, p, p, 1, 2, 2, 1, 0, None) == -1 and b'min_frames' in lib.dx_last_error()
    assert lib.dx_dtw_transfer(p, p, p, p, p, p, p, p, p, 1, 4097, 2, 1, 1, None) == -5
    # the wrapper works out extents that hold the rows from the path's own width
    name, cells, n_ref, n_gen, durations, m, want = A.transfer_cases()[3]
    assert name == 'vertical-run-min2'
    path = np.full((1, 20, 2), -1, dtype=np.int32)
    path[0, :len(cells)] = cells
    dev = lambda a, dtype: torch.tensor(a, dtype=dtype, device=DEV)
    rec, moved, status = dtw_transfer_batch(torch.from_numpy(path).to(DEV), dev([len(cells)], torch.int32), dev([n_ref], torch.int64),
                                            dev([n_gen], torch.int64), dev([durations], torch.int64), dev([len(durations)], torch.int64), m)
    assert (rec[0].tolist(), int(moved[0]), int(status[0])) == want


# ---- exact recovery of a constructed warp ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _warps():
    ''' six (mel_gen, durations, repeats): random symbol durations 0..4, every synthesis frame repeated 1..3 times, at most 64
        recording frames '''
    rng = np.random.RandomState(0)
    out = []
    while len(out) < 6:
        durations = rng.randint(0, 5, size=int(rng.randint(1, 12)))
        n = int(durations.sum())
        repeats = rng.randint(1, 4, size=max(n, 1))[:n]
        if n == 0 or repeats.sum() > 64:
            continue
        out.append((O.mel_case(80, n, 100 + len(out)), durations, repeats))
    return out


def _warp_batch(min_frames):
    from daft_exprt.align import transfer_durations
    warps = _warps()
    B, L = len(warps), max(len(w[1]) for w in warps)
    T_gen, T_rec = max(w[0].shape[1] for w in warps), max(int(w[2].sum()) for w in warps)
    mel_gen, mel_rec = np.full((B, 80, T_gen), 9.0, dtype=np.float32), np.full((B, 80, T_rec), -9.0, dtype=np.float32)
    dur = np.full((B, L), 1 << 40, dtype=np.int64)
    for b, (mel, durations, repeats) in enumerate(warps):
        rec = np.repeat(mel, repeats, axis=1)
        mel_gen[b, :, :mel.shape[1]], mel_rec[b, :, :rec.shape[1]], dur[b, :len(durations)] = mel, rec, durations
    ints = lambda values: torch.tensor(values, dtype=torch.int64, device=DEV)
    n_gen, n_rec = ints([w[0].shape[1] for w in warps]), ints([int(w[2].sum()) for w in warps])
    out = transfer_durations(torch.from_numpy(mel_gen).to(DEV), n_gen, torch.from_numpy(dur).to(DEV), ints([len(w[1]) for w in warps]),
                             torch.from_numpy(mel_rec).to(DEV), n_rec, min_frames=min_frames)
    return warps, tuple(t.cpu().numpy() for t in out)


def test_known_boundaries_of_a_constructed_warp_are_recovered_exactly():
    warps, (rec, moved, status, total) = _warp_batch(1)
    for b, (mel, durations, repeats) in enumerate(warps):
        starts = np.concatenate([[0], np.cumsum(durations)])
        want = [int(repeats[starts[s]: starts[s + 1]].sum()) for s in range(len(durations))]
        print(f'pair {b}: durations {durations.tolist()} -> {rec[b].tolist()} (want {want}), moved {moved[b]}, total {total[b]}')
        assert rec[b, :len(want)].tolist() == want and not rec[b, len(want):].any()
        assert moved[b] == 0 and status[b] == 0 and total[b] == 0.0


def test_a_constructed_warp_with_a_minimum_duration_keeps_the_invariants():
    warps, (rec, moved, status, total) = _warp_batch(3)
    seen = set()
    for b, (mel, durations, repeats) in enumerate(warps):
        K, n_rec, n = int((durations > 0).sum()), int(repeats.sum()), len(durations)
        seen.add(int(status[b]))
        assert status[b] == (1 if n_rec < 3 * K else 0) and total[b] == 0.0
        if status[b] == 0:
            assert rec[b].sum() == n_rec and (rec[b, :n][durations > 0] >= 3).all() and not rec[b, :n][durations == 0].any()
            assert not rec[b, n:].any()
        else:
            assert not rec[b].any() and moved[b] == 0
    assert 0 in seen


# ---- a model in the loop ----------------------------------------------------------------------------------------------------------------

FS = 22050
#             name    seconds  silence in front  phonemised sentence                                    .lab sentence
UTTERANCES = (('u0', 1.2, 0.15, '{HH AH0 L OW1} , {W ER1 L D} . ~', 'Hello, world.'),
              ('u1', 0.9, 0.00, '{G UH1 D} {D EY1} ~', 'Good day'),
              ('u2', 1.0, 0.25, '{Y EH1 S} ? {N OW1} ! ~', 'Yes? No!'))


def _wave(seconds, lead, seed):
    ''' silence, a noise burst, a short gap, a second burst, silence: the sounding stretch is at least 0.55 s long '''
    rng = np.random.RandomState(seed)
    n, first = int(seconds * FS), int(lead * FS)
    wav = 1e-4 * rng.standard_normal(n)
    last = n - int(0.1 * FS)
    gap = (first + last) // 2
    wav[first: gap - 600] += 0.2 * rng.standard_normal(gap - 600 - first)
    wav[gap + 600: last] += 0.3 * rng.standard_normal(last - gap - 600)
    return wav.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _model():
    from daft_exprt.model import DaftExprt
    fx = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'data_loader.npz'))
    hp = make_hparams(compute_dtype='fp32', minimum_wav_duration=200)
    hp.stats = {f'spk {i}': {'energy': {'mean': float(fx['stats_energy_mean'][i]), 'std': float(fx['stats_energy_std'][i])},
                             'pitch': {'mean': float(fx['stats_pitch_mean'][i]), 'std': float(fx['stats_pitch_std'][i])}} for i in range(11)}
    torch.manual_seed(1234)
    model = DaftExprt(hp)
    with torch.no_grad():   # random duration head: about 0.06 s for every symbol, so that every symbol has frames
        model.prosody_predictor.projection.linear_layer.weight[0].mul_(0.01)
        model.prosody_predictor.projection.linear_layer.bias.copy_(torch.tensor([0.06, 0., 0.]))
    return model.cuda(0), hp


def _sentences(tmp_path):
    from daft_exprt.generate import read_phonemised_sentences
    path = tmp_path / 'phonemised.txt'
    path.write_text(''.join(f'{name}|{text}\n' for name, _, _, text, _ in UTTERANCES), encoding='utf-8')
    return str(path), read_phonemised_sentences(str(path))[0]


def _run_align_batch(model, hp, sentences):
    from daft_exprt.align import align_batch
    from daft_exprt.generate import _symbol_ids
    ids = [_symbol_ids(s, hp) for s in sentences]
    waves = [_wave(seconds, lead, 40 + k) for k, (_, seconds, lead, _, _) in enumerate(UTTERANCES)]
    symbols = torch.zeros((3, max(len(i) for i in ids)), dtype=torch.int64)
    wavs = torch.zeros((3, max(len(w) for w in waves)), dtype=torch.float32)
    for b in range(3):
        symbols[b, :len(ids[b])], wavs[b, :len(waves[b])] = torch.tensor(ids[b]), torch.from_numpy(waves[b])
    lengths = torch.tensor([len(i) for i in ids], dtype=torch.int64, device=DEV)
    out = align_batch(model, symbols.to(DEV), lengths, wavs.to(DEV), [len(w) for w in waves], torch.tensor([0, 3, 7], device=DEV), hp)
    return ids, waves, {k: v.cpu().numpy() for k, v in out.items()}


def test_align_batch_with_a_random_model(tmp_path):
    from daft_exprt.align import ALIGN_KEYS
    model, hp = _model()
    _, sentences = _sentences(tmp_path)
    ids, waves, out = _run_align_batch(model, hp, sentences)
    assert tuple(out) == ALIGN_KEYS
    for b, (name, seconds, lead, _, _) in enumerate(UTTERANCES):
        n = len(ids[b])
        rec, gen = out['rec_durations'][b], out['gen_durations'][b]
        print(f'{name}: begin {out["begin"][b]}, frames {out["frames"][b]} / {out["frames_gen"][b]}, moved {out["moved"][b]}, '
              f'path cost {out["path_cost"][b]:.3f}, gen {gen[:n].tolist()}, rec {rec[:n].tolist()}')
        assert out['status'][b] == 0 and gen[:n].sum() == out['frames_gen'][b]
        assert rec.sum() == out['frames'][b] and (rec[:n][gen[:n] > 0] >= 3).all() and not rec[:n][gen[:n] == 0].any() and not rec[n:].any()
        assert 0 <= out['moved'][b] <= n and np.isfinite(out['path_cost'][b]) and out['path_cost'][b] > 0
        # the crop: inside the recording, and it starts where the sound does (a frame is hop samples, its window four hops)
        assert (out['begin'][b] + out['frames'][b] - 1) * hp.hop_length <= len(waves[b])
        first = int(lead * FS) / hp.hop_length
        assert first - 2.5 <= out['begin'][b] <= first + 1, (name, out['begin'][b], first)
        assert (out['begin'][b] > 0) == (lead > 0)
    again = _run_align_batch(model, hp, sentences)[2]
    for key in ALIGN_KEYS:
        assert out[key].tobytes() == again[key].tobytes(), key


def test_align_batch_statuses_that_need_no_launch(tmp_path):
    from daft_exprt.align import align_batch
    from daft_exprt.evaluate import max_dtw_length
    model, hp = _model()
    too_long = (max_dtw_length() + 1) * hp.hop_length
    wavs = torch.zeros((2, 8), dtype=torch.float32, device=DEV)            # (the rows are not read: both are decided on the host)
    symbols = torch.ones((2, 3), dtype=torch.int64, device=DEV)
    lengths = torch.tensor([3, 3], dtype=torch.int64, device=DEV)
    out = align_batch(model, symbols, lengths, wavs, [too_long, hp.filter_length // 2], torch.tensor([0, 0], device=DEV), hp)
    assert out['status'].tolist() == [3, 4] and not out['rec_durations'].any() and not out['moved'].any()
    assert torch.isnan(out['path_cost']).all()


def test_align_data_set_round_trip_through_extract_features(tmp_path):
    from daft_exprt.align import align_data_set, flatten_sentence
    from daft_exprt.audio import write_wav_int16
    from daft_exprt.extract_features import extract_features
    model, hp = _model()
    phonemised, sentences = _sentences(tmp_path)
    data, features = tmp_path / 'data', tmp_path / 'features'
    for d in (data / 'spk03' / 'wavs', data / 'spk03' / 'align', features / 'spk03'):
        d.mkdir(parents=True)
    for k, (name, seconds, lead, _, lab) in enumerate(UTTERANCES):
        wav = _wave(seconds, lead, 40 + k)
        write_wav_int16(str(data / 'spk03' / 'wavs' / f'{name}.wav'), FS, np.clip(np.trunc(wav * 32768.), -32768, 32767).astype(np.int16))
        (data / 'spk03' / 'align' / f'{name}.lab').write_text(lab + '\n', encoding='utf-8')
    (features / 'spk03' / 'metadata.csv').write_text(''.join(f'{u[0]}|{u[4]}\n' for u in UTTERANCES), encoding='utf-8')
    (data / 'spk03' / 'align' / 'u1.markers').write_text('kept\n', encoding='utf-8')

    report = align_data_set(str(data), ['spk03'], phonemised, model, hp, batch_size=2)
    assert report['already_done'] == 1 and sorted(report['files']) == ['spk03/u0', 'spk03/u2'] and report['skipped'] == []
    assert (data / 'spk03' / 'align' / 'u1.markers').read_text() == 'kept\n'
    report = align_data_set(str(data), ['spk03'], phonemised, model, hp, batch_size=2, overwrite=True)
    assert report['already_done'] == 0 and report['batches'] == 2 and report['skipped'] == [], report['skipped']
    assert report['summary']['files'] == report['summary']['written'] == 3 and report['summary']['status']['0'] == 3
    with open(data / 'align_report.json', 'r', encoding='utf-8') as f:
        on_disk = json.load(f)
    assert on_disk['files'] == report['files'] and on_disk['summary'] == report['summary']
    for name, record in report['files'].items():
        print(name, record)
        assert record['written'] and record['status'] == 0 and record['frames'] > 0 and record['path_cost'] > 0

    hp_features = make_hparams(speakers=['spk03'], minimum_wav_duration=200)
    done = extract_features(str(data), str(features), hp_features, 1, batch_size=3)
    assert done['written'] == 3 and done['skipped'] == [], done
    for (name, _, _, _, _), sentence in zip(UTTERANCES, sentences):
        for ext in ('.npy', '.markers', '.frames_nrg', '.symbols_nrg', '.frames_f0', '.symbols_f0'):
            assert (features / 'spk03' / f'{name}{ext}').is_file(), (name, ext)
        rows = [line.rstrip('\n').split('\t') for line in (features / 'spk03' / f'{name}.markers').read_text(encoding='utf-8').splitlines()]
        assert [row[3] for row in rows] == [symbol for symbol, _ in flatten_sentence(sentence)], name
        mel = np.load(features / 'spk03' / f'{name}.npy')
        assert sum(int(row[2]) for row in rows) == mel.shape[1]
