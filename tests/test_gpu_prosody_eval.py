"""`dx_curve_pcc` and what is built on it (daft_exprt/evaluate.py, `generate_mel_specs(scores=...)`, scripts/synthesize.py) against
the reference's recorded results (tests/golden/pitch_pcc.npz) and the float64 oracle (tests/curve_oracle.py).

Tolerance: TOL_FACTOR (10) times the error the kernel's direct sums have when restated in NumPy float32, measured on the host
over these same cases (tests/test_prosody_eval_host.py): 1.5e-5 on a correlation, 3.2e-6 on a resampled log-Hz value."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import curve_oracle as O
from tests import pitch_cases as PC
from tests.util import make_hparams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
TOL_PCC, TOL_RS = O.TOL_FACTOR * O.F32_PCC_ERR, O.TOL_FACTOR * O.F32_RESAMPLED_ERR


def _pad(rows, fill=0.0):
    x = np.full((len(rows), max(1, max(len(r) for r in rows))), fill, dtype=np.float32)
    for i, r in enumerate(rows):
        x[i, :len(r)] = r
    return torch.from_numpy(x).to(DEV), torch.tensor([len(r) for r in rows], dtype=torch.int64, device=DEV)


def _run(refs, duts, remove, fill=0.0):
    ''' (pcc, kept_ref, kept_dut, resampled) NumPy of one `curve_pcc_batch` call over right-padded rows '''
    from daft_exprt.evaluate import curve_pcc_batch
    r, n_r = _pad(refs, fill)
    d, n_d = _pad(duts, fill)
    out = curve_pcc_batch(r, n_r, d, n_d, remove_unvoiced=remove, return_resampled=True)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def _check(cases, expected):
    ''' cases [(name, ref, dut, remove)], expected [(pcc, kept_ref, kept_dut, resampled)]: one launch per flag value '''
    worst_pcc = worst_rs = 0.0
    for flag in (False, True):
        idx = [i for i, c in enumerate(cases) if c[3] == flag]
        if not idx:
            continue
        pcc, kept_ref, kept_dut, rs = _run([cases[i][1] for i in idx], [cases[i][2] for i in idx], flag)
        for row, i in enumerate(idx):
            name, (want, kr, kd, y) = cases[i][0], expected[i]
            assert (int(kept_ref[row]), int(kept_dut[row])) == (kr, kd), name
            e_pcc, e_rs = abs(float(pcc[row]) - want), float(np.abs(rs[row, :kr] - y).max())
            print(f'{name}: kept {kr} x {kd}, pcc {want:+.6f}, error {e_pcc:.2e}, resampled error {e_rs:.2e}')
            assert e_pcc <= TOL_PCC and e_rs <= TOL_RS, (name, e_pcc, e_rs)
            assert not rs[row, kr:].any(), name
            worst_pcc, worst_rs = max(worst_pcc, e_pcc), max(worst_rs, e_rs)
    print(f'worst: pcc {worst_pcc:.2e} (bound {TOL_PCC:.1e}), resampled {worst_rs:.2e} (bound {TOL_RS:.1e})')


def test_golden_cases_match_the_reference():
    cases = O.golden_cases()
    z = np.load(O.GOLDEN)
    _check([c[:4] for c in cases], [(c[4], int(z['kept'][i, 0]), int(z['kept'][i, 1]), c[5]) for i, c in enumerate(cases)])


def test_every_branch_of_the_nyquist_rule_and_tiny_curves():
    cases = O.branch_cases()
    assert {(len(c[1]), len(c[2])) for c in cases if not c[3]} == set(O.BRANCH_PAIRS)
    assert any((c[1] < 0).any() and (c[1] == 0).any() and (c[2] < 0).any() for c in cases if c[3])     # values <= 0 are unvoiced
    expected = [O.curve_pcc(ref, dut, remove) for _, ref, dut, remove in cases]
    assert {(e[1], e[2]) for e in expected} == set(O.BRANCH_PAIRS)
    _check(cases, expected)


def test_reference_signature():
    from daft_exprt.evaluate import pcc_on_2_pitch_curve
    _, ref, dut, remove, want, _ = O.golden_cases()[0]
    got = pcc_on_2_pitch_curve(ref.astype(np.float64), dut.astype(np.float64), remove_unvoiced=remove)
    assert isinstance(got, float) and abs(got - want) <= TOL_PCC
    assert math.isnan(pcc_on_2_pitch_curve(ref, np.zeros(0)))
    with pytest.raises(RuntimeError, match='device tensors'):
        from daft_exprt.evaluate import curve_pcc_batch
        n = torch.tensor([4], dtype=torch.int64)
        curve_pcc_batch(torch.ones(1, 4), n, torch.ones(1, 4), n)


def test_undefined_rows_are_nan_not_faults():
    ref, dut = O.voiced_pair(40, 50, 3)
    refs = [np.array([0, -1, 0, -2.5], np.float32), ref, np.full(40, 5.25, np.float32), ref[:0], ref, ref]
    duts = [dut, np.zeros(50, np.float32), dut, dut, dut[:0], dut]
    pcc, kept_ref, kept_dut, rs = _run(refs, duts, True)
    assert np.isnan(pcc[:5]).all()
    assert kept_ref.tolist() == [0, 40, 40, 0, 40, 40] and kept_dut.tolist() == [50, 0, 50, 50, 0, 50]
    assert np.isnan(rs[1, :40]).all() and np.isnan(rs[4, :40]).all()                # nothing to resample
    assert abs(float(pcc[5]) - O.curve_pcc(ref, dut)[0]) <= TOL_PCC                 # the defined row beside them
    pcc, kept_ref, kept_dut, _ = _run(refs, duts, False)                            # the flag off: zeros and negatives are values
    assert kept_ref.tolist() == [4, 40, 40, 0, 40, 40] and kept_dut.tolist() == [50, 50, 50, 50, 0, 50]
    assert np.isnan(pcc[[1, 2, 3, 4]]).all() and abs(float(pcc[0]) - O.curve_pcc(refs[0], duts[0], False)[0]) <= TOL_PCC


def test_ragged_batch_rows_are_independent():
    cases = [c for c in O.branch_cases() if c[3] and c[0].split('-')[0] in ('64x63', '3x2', '200x137', '777x1000', '65x64')]
    assert len(cases) == 5
    refs, duts = [c[1] for c in cases], [c[2] for c in cases]
    batch = _run(refs, duts, True)
    for i in range(5):
        alone = _run([refs[i]], [duts[i]], True)
        kr = int(alone[1][0])
        assert batch[0][i].tobytes() == alone[0][0].tobytes() and batch[1][i] == alone[1][0] and batch[2][i] == alone[2][0], cases[i][0]
        assert batch[3][i, :kr].tobytes() == alone[3][0, :kr].tobytes(), cases[i][0]
    poisoned = _run(refs, duts, True, fill=np.nan)                                  # nothing past n is read
    for a, b in zip(batch, poisoned):
        assert a.tobytes() == b.tobytes()


def test_length_limit():
    from daft_exprt.evaluate import curve_pcc_batch, max_curve_length
    assert max_curve_length() == O.MAX_LEN
    name, ref, dut, remove = O.limit_case()
    assert len(ref) == O.MAX_LEN and (ref > 0).all() and (dut > 0).all()
    _check([(name, ref, dut, remove)], [O.curve_pcc(ref, dut, remove)])
    wide = torch.ones((1, O.MAX_LEN + 1), dtype=torch.float32, device=DEV)
    n = torch.tensor([8], dtype=torch.int64, device=DEV)
    for r, d in ((wide, wide[:, :64]), (wide[:, :64].contiguous(), wide)):
        with pytest.raises(RuntimeError, match='error -5'):
            curve_pcc_batch(r, n, d, n)


# ---- end to end -------------------------------------------------------------------------------------------------------------

SENTENCES = [[['HH', 'AH0', 'L', 'OW1'], ' ', ['W', 'ER1', 'L', 'D'], ',', ['T', 'EH1', 'S', 'T'], '?', '~'],
             [['T', 'EH1', 'S', 'T'], '.', '~'],
             [['AY1'], ' ', ['S', 'IY1'], ' ', ['Y', 'UW1'], '!', '~']]


def _tiny_model(golden_dir):
    from daft_exprt.model import DaftExprt
    st = np.load(os.path.join(golden_dir, 'inference.npz'))
    hp = make_hparams(compute_dtype='fp32')
    hp.stats = {f'spk {i}': {'pitch': {'mean': float(st['stats_pitch_mean'][i]), 'std': float(st['stats_pitch_std'][i])}}
                for i in range(11)}
    torch.manual_seed(1234)
    model = DaftExprt(hp)
    with torch.no_grad():   # random duration head: centre it so that the utterances have a sensible length
        model.prosody_predictor.projection.linear_layer.weight[0].mul_(0.05)
        model.prosody_predictor.projection.linear_layer.bias.copy_(torch.tensor([0.08, 0., 0.]))
    return model, hp


def _style_bank(path, hp):
    ''' two reference recordings made of harmonic tones: a rising glide and a vibrato '''
    from daft_exprt import audio
    os.makedirs(path)
    sr = int(hp.sampling_rate)
    t = np.arange(int(0.8 * sr)) / sr
    for name, f0 in (('glide', 120.0 + 80.0 * t / t[-1]), ('vibrato', 200.0 + 25.0 * np.sin(2 * np.pi * 4.0 * t))):
        tone = PC.harmonic_tone(f0, sr, 0.8)
        audio.write_wav_int16(os.path.join(path, f'{name}.wav'), sr, np.round(tone * 32767.0).astype(np.int16))
    return [os.path.join(path, 'glide.wav'), os.path.join(path, 'vibrato.wav')]


def _read_f64_wav(path):
    raw = open(path, 'rb').read()
    return np.frombuffer(raw[raw.index(b'data') + 8:], dtype='<f8')


def test_scores_of_voiced_audio_are_defined_and_match_the_oracle():
    ''' `prosody_transfer_scores` on waveforms that are voiced for certain (harmonic tones standing in for generated audio)
        against reference curves extracted from other tones: every pitch score is defined '''
    from daft_exprt.evaluate import prosody_transfer_scores
    from daft_exprt.extract_features import mel_spectrogram_batch, pitch_batch
    hp = make_hparams()
    sr = int(hp.sampling_rate)

    def tone(seconds, lo, hi, wobble):
        t = np.arange(int(round(seconds * sr))) / sr
        swell = (0.35 + 0.65 * np.sin(np.pi * t / t[-1]) ** 2).astype(np.float32)   # an envelope: the energy curve varies too
        return swell * PC.harmonic_tone(lo + (hi - lo) * t / t[-1] + wobble * np.sin(2 * np.pi * 3.0 * t), sr, seconds)
    gen = [tone(0.9, 110.0, 190.0, 6.0), tone(0.6, 240.0, 180.0, 10.0), tone(1.1, 150.0, 150.0, 20.0)]
    ref = [tone(0.7, 120.0, 200.0, 5.0), tone(0.8, 250.0, 170.0, 8.0), tone(0.5, 160.0, 160.0, 15.0)]
    x, n = _pad(gen)
    xr, nr = _pad(ref)
    pitch_refs, len_refs = pitch_batch(xr, nr, hp)
    _, energy_refs, _ = mel_spectrogram_batch(xr, nr, hp)
    got = {k: v.cpu().numpy() for k, v in prosody_transfer_scores(x, n, pitch_refs, energy_refs, len_refs, hp).items()}
    pitch, n_pitch = pitch_batch(x, n, hp)
    _, energy, n_frames = mel_spectrogram_batch(x, n, hp)
    pitch, energy, pitch_refs, energy_refs = (t.cpu().numpy() for t in (pitch, energy, pitch_refs, energy_refs))
    for i in range(3):
        tr, tg = int(len_refs[i]), int(n_frames[i])
        p_pcc, v_ref, v_gen, _ = O.curve_pcc(pitch_refs[i, :tr], pitch[i, :int(n_pitch[i])], True)
        e_pcc, f_ref, f_gen, _ = O.curve_pcc(energy_refs[i, :tr], energy[i, :tg], False)
        print(f'row {i}: pitch_pcc {got["pitch_pcc"][i]:+.6f} (oracle {p_pcc:+.6f}), energy_pcc {got["energy_pcc"][i]:+.6f} (oracle {e_pcc:+.6f}), '
              f'voiced {v_ref} / {v_gen} of {f_ref} / {f_gen} frames')
        assert (got['voiced_ref'][i], got['voiced_gen'][i], got['frames_ref'][i], got['frames_gen'][i]) == (v_ref, v_gen, f_ref, f_gen)
        assert v_ref > 1 and v_gen > 1                                              # the tones are voiced
        assert np.isfinite(got['pitch_pcc'][i]) and abs(float(got['pitch_pcc'][i]) - p_pcc) <= TOL_PCC
        assert np.isfinite(got['energy_pcc'][i]) and abs(float(got['energy_pcc'][i]) - e_pcc) <= TOL_PCC


def test_generate_scores_match_the_oracle_and_change_nothing_else(golden_dir, tmp_path):
    from daft_exprt import generate as G
    from daft_exprt.extract_features import mel_spectrogram_batch, pitch_batch
    model, hp = _tiny_model(golden_dir)
    model = model.cuda(0)
    bank = str(tmp_path / 'bank')
    wavs = _style_bank(bank, hp)
    G.extract_reference_parameters_batch(wavs, bank, hp)
    refs = [os.path.join(bank, n) for n in ('glide.npz', 'vibrato.npz', 'glide.npz')]
    spk = [0, 3, 7]
    runs = []
    for out_dir, scores in ((str(tmp_path / 'plain'), None), (str(tmp_path / 'scored'), {})):
        preds = G.generate_mel_specs(model, SENTENCES, ['a', 'b', 'c'], spk, refs, out_dir, hp, batch_size=3, use_griffin_lim=True,
                                     scores=scores)
        runs.append((out_dir, preds, scores))
    (plain_dir, plain, _), (out_dir, preds, scores) = runs
    assert list(scores) == list(preds) and len(preds) == 3
    assert sorted(os.listdir(plain_dir)) == sorted(os.listdir(out_dir))
    for name in preds:                                                              # scoring changes no file and no prediction
        assert open(os.path.join(out_dir, f'{name}.wav'), 'rb').read() == open(os.path.join(plain_dir, f'{name}.wav'), 'rb').read()
        a, b = np.load(os.path.join(out_dir, f'{name}.npz')), np.load(os.path.join(plain_dir, f'{name}.npz'))
        assert a.files == b.files == ['mel_spec'] and a['mel_spec'].tobytes() == b['mel_spec'].tobytes()
        assert all(x.dtype == y.dtype and x.tobytes() == y.tobytes() for x, y in zip(preds[name], plain[name]))
    # the oracle on the same Griffin-Lim output (read back from the preview files) and the reference .npz
    audio = [_read_f64_wav(os.path.join(out_dir, f'{name}.wav')).astype(np.float32) for name in preds]
    x, n = _pad(audio)
    pitch, n_pitch = pitch_batch(x, n, hp)
    _, energy, n_frames = mel_spectrogram_batch(x, n, hp)
    pitch, energy, n_pitch, n_frames = (t.cpu().numpy() for t in (pitch, energy, n_pitch, n_frames))
    for i, name in enumerate(preds):
        ref = np.load(os.path.join(bank, name.split('_ref_')[1] + '.npz'))
        got = scores[name]
        assert list(got) == ['pitch_pcc', 'energy_pcc', 'voiced_ref', 'voiced_gen', 'frames_ref', 'frames_gen']
        assert all(isinstance(got[k], float) for k in ('pitch_pcc', 'energy_pcc')) and all(isinstance(got[k], int) for k in list(got)[2:])
        p_pcc, v_ref, v_gen, _ = O.curve_pcc(ref['pitch'], pitch[i, :int(n_pitch[i])], True)
        e_pcc, f_ref, f_gen, _ = O.curve_pcc(ref['energy'], energy[i, :int(n_frames[i])], False)
        print(f'{name}: pitch_pcc {got["pitch_pcc"]:+.6f} (oracle {p_pcc:+.6f}), energy_pcc {got["energy_pcc"]:+.6f} (oracle {e_pcc:+.6f}), '
              f'voiced {got["voiced_ref"]} / {got["voiced_gen"]}, frames {got["frames_ref"]} / {got["frames_gen"]}')
        assert (got['voiced_ref'], got['voiced_gen'], got['frames_ref'], got['frames_gen']) == (v_ref, v_gen, f_ref, f_gen)
        assert f_ref == len(ref['pitch']) and f_gen == preds[name][4].shape[1] - 2 + hp.filter_length // hp.hop_length + 1
        for mine, want in ((got['pitch_pcc'], p_pcc), (got['energy_pcc'], e_pcc)):
            assert (math.isnan(mine) and math.isnan(want)) or abs(mine - want) <= TOL_PCC, (name, mine, want)
        assert v_ref > 40 and not math.isnan(got['energy_pcc'])                     # the tones are voiced (69 frames); the energy score is defined


def test_synthesize_cli(golden_dir, tmp_path):
    model, hp = _tiny_model(golden_dir)
    ckpt = str(tmp_path / 'DaftExprt_test')
    torch.save({'iteration': 0, 'state_dict': {f'module.{k}': v for k, v in model.state_dict().items()},
                'config_params': dict(vars(hp))}, ckpt)
    bank, out_dir = str(tmp_path / 'bank'), str(tmp_path / 'out')
    _style_bank(bank, hp)
    text = tmp_path / 'sentences_to_generate.txt'
    text.write_text('s.txt_line0|{HH AH0 L OW1} {W ER1 L D} , {T EH1 S T} ? ~\ns.txt_line1|{T EH1 S T} . ~\n'
                    's.txt_line2|{AY1} {S IY1} {Y UW1} ! ~\n', encoding='utf-8')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'synthesize.py'), '-out', out_dir, '-chk', ckpt, '-tf', str(text),
                        '-sb', bank, '-bs', '2'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert sorted(f for f in os.listdir(bank) if f.endswith('.npz')) == ['glide.npz', 'vibrato.npz']
    report = json.load(open(os.path.join(out_dir, 'prosody_transfer.json')))
    files = sorted(os.listdir(out_dir))
    assert len(report['files']) == 3 and report['summary']['files'] == 3
    for idx in range(3):
        assert f'{idx}_ref.wav' in files
        paired = [f for f in files if f.startswith(f'{idx}_s.txt_line{idx}_spk_') and f.endswith('.wav')]
        assert len(paired) == 1
        name = paired[0][len(f'{idx}_'):-len('.wav')]
        assert report['files'][name]['wav'] == paired[0] and f'{name}.npz' in files
        ref_name = name.split('_ref_')[1]
        assert open(os.path.join(out_dir, f'{idx}_ref.wav'), 'rb').read() == open(os.path.join(bank, f'{ref_name}.wav'), 'rb').read()
    for key in ('pitch_pcc', 'energy_pcc'):
        values = [e[key] for e in report['files'].values() if e[key] is not None]
        s = report['summary'][key]
        assert s['undefined'] == 3 - len(values)
        if values:
            assert s['mean'] == pytest.approx(float(np.mean(values))) and s['median'] == pytest.approx(float(np.median(values)))
            assert all(-1.0 - 1e-5 <= v <= 1.0 + 1e-5 for v in values)
        else:
            assert s['mean'] is None and s['median'] is None
    assert report['summary']['energy_pcc']['undefined'] == 0
    assert 'energy_pcc: mean' in r.stderr
