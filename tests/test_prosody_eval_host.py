"""Host-side checks of the prosody-transfer metric: the float64 oracle (tests/curve_oracle.py) against what the reference's
`compare_pitch_curves.pcc_on_2_pitch_curve` returned (tests/golden/pitch_pcc.npz), the error of the kernel's direct sums restated
in float32 -- the figure the GPU tests' tolerance is built on --, and the reader of phonemised sentence files."""
import numpy as np
import pytest

from tests import curve_oracle as O


def test_oracle_reproduces_the_reference_metric():
    cases = O.golden_cases()
    assert len(cases) >= 24
    z = np.load(O.GOLDEN)
    for i, (name, ref, dut, remove, pcc, resampled) in enumerate(cases):
        got, kept_ref, kept_dut, y = O.curve_pcc(ref, dut, remove)
        assert (kept_ref, kept_dut) == tuple(z['kept'][i]), name
        assert abs(got - pcc) <= 1e-12, (name, got, pcc)
        assert y.shape == resampled.shape and np.abs(y - resampled).max() <= 1e-12, name
    assert any(c[3] for c in cases) and not all(c[3] for c in cases)                # the flag on and off
    assert any((np.asarray(c[1]) < 0).any() for c in cases)                         # negative values count as unvoiced


def test_oracle_undefined_rows_are_nan():
    ref, dut = O.voiced_pair(20, 30, 1)
    for r, d, kept in ((np.zeros(5), dut, (0, 30)), (ref, -np.ones(7), (20, 0)), (np.full(9, 5.0), dut, (9, 30)),
                       (ref[:0], dut, (0, 30)), (ref, dut[:0], (20, 0))):
        pcc, kr, kd, _ = O.curve_pcc(r, d, True)
        assert np.isnan(pcc) and (kr, kd) == kept


def test_float32_direct_sums_stay_within_the_recorded_errors():
    ''' the bound of tests/test_gpu_prosody_eval.py is TOL_FACTOR times these two constants '''
    worst_pcc = worst_rs = 0.0
    cases = O.all_cases()
    assert {(len(c[1]), len(c[2])) for c in cases if c[0].endswith('-all')} == set(O.BRANCH_PAIRS)
    for name, ref, dut, remove in cases:
        pcc, kept_ref, kept_dut, y = O.curve_pcc(ref, dut, remove)
        pcc32, y32 = O.direct_f32(ref, dut, remove)
        assert y32.dtype == np.float32 and y32.shape == y.shape
        assert 4.0 < y.min() and y.max() < 6.0, name                               # log-Hz like
        if min(kept_ref, kept_dut) >= 16:                                          # never near-constant (a handful of points may be)
            assert np.std(y) > 0.02 and np.std(O.remove_unvoiced(ref) if remove else ref) > 0.02, name
        worst_pcc, worst_rs = max(worst_pcc, abs(pcc32 - pcc)), max(worst_rs, float(np.abs(y32 - y).max()))
    print(f'float32 direct sums: pcc error {worst_pcc:.3e}, resampled error {worst_rs:.3e}')
    assert worst_pcc <= O.F32_PCC_ERR and worst_rs <= O.F32_RESAMPLED_ERR, (worst_pcc, worst_rs)
    assert worst_pcc >= O.F32_PCC_ERR / 2 and worst_rs >= O.F32_RESAMPLED_ERR / 2    # the constants are the measured figures, not slack


def test_read_phonemised_sentences_round_trip(tmp_path):
    from daft_exprt.generate import read_phonemised_sentences
    from daft_exprt.symbols import eos, symbols_english, whitespace
    sentences = [[['HH', 'AH0', 'L', 'OW1'], whitespace, ['W', 'ER1', 'L', 'D'], ',', ['T', 'EH1', 'S', 'T'], '?', eos],
                 [['T', 'EH1', 'S', 'T'], '.', eos],
                 [['AY1'], whitespace, ['S', 'IY1'], whitespace, ['Y', 'UW1'], '!', eos]]
    names = ['sentences.txt_line0', 'sentences.txt_line1', 'sentences.txt_line2']
    path = tmp_path / 'sentences_to_generate.txt'
    with open(path, 'w', encoding='utf-8') as f:                                    # the writer of `generate.py:483-492`
        for sentence, file_name in zip(sentences, names):
            text = ''
            for item in sentence:
                if isinstance(item, list):
                    item = '{' + ' '.join(item) + '}'
                text = f'{text} {item} '
            f.write(f'{file_name}|{" ".join(text.split())}\n')
    assert open(path).readline() == 'sentences.txt_line0|{HH AH0 L OW1} {W ER1 L D} , {T EH1 S T} ? ~\n'
    got, got_names = read_phonemised_sentences(str(path))
    assert got == sentences and got_names == names
    assert read_phonemised_sentences(str(path), symbols_english) == (sentences, names)

    for bad, what in (('a|{HH AH0} {QQ} . ~', 'QQ'), ('a|{HH AH0} ; ~', ';'), ('a|{HH AH0 . ~', 'brace'), ('no separator', 'file_name')):
        bad_path = tmp_path / 'bad.txt'
        bad_path.write_text('ok|{T EH1 S T} . ~\n' + bad + '\n', encoding='utf-8')
        with pytest.raises(ValueError, match='line 2') as err:
            read_phonemised_sentences(str(bad_path))
        assert what in str(err.value)


def test_scores_need_the_preview_audio():
    from daft_exprt.generate import generate_batch_mel_specs, generate_mel_specs
    with pytest.raises(ValueError, match='use_griffin_lim'):
        generate_mel_specs(None, [], [], [], [], '/nonexistent_daft_exprt_out', None, use_griffin_lim=False, scores={})
    with pytest.raises(ValueError, match='use_griffin_lim'):
        generate_batch_mel_specs(None, [], [], [], [], [], 'add', [], [], '/nonexistent_daft_exprt_out', None, use_griffin_lim=False,
                                 scores={})


def test_length_limit_is_reported_before_any_launch():
    ''' no device is touched: the entry point refuses the shape first '''
    from daft_exprt import _hip as H
    lib = H.lib()
    assert lib.dx_curve_pcc_max_len() == O.MAX_LEN
    rc = lib.dx_curve_pcc(8, O.MAX_LEN + 1, 8, 8, 64, 8, 8, 8, 8, None, 0, 1, O.MAX_LEN + 1, 64, 1, None)
    assert rc == -5 and b'4096' in lib.dx_last_error()
    rc = lib.dx_curve_pcc(8, 64, 8, 8, O.MAX_LEN + 1, 8, 8, 8, 8, None, 0, 1, 64, O.MAX_LEN + 1, 1, None)
    assert rc == -5
    rc = lib.dx_curve_pcc(None, 64, 8, 8, 64, 8, 8, 8, 8, None, 0, 1, 64, 64, 1, None)
    assert rc == -1 and b'null' in lib.dx_last_error()
