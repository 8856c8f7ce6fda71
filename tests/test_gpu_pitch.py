"""GPU checks of the pitch tracker (csrc/pitch.hip) against its float64 oracle (tests/pitch_oracle.py) and against what the
reference's pitch binary recorded (tests/golden/pitch_reaper.npz), and of `extract_reference_parameters` end to end.
The fp32 bounds are derived in tests/pitch_cases.py."""
import os

import numpy as np
import pytest
import torch

from tests import pitch_cases as C
from tests import pitch_oracle as O
from tests.util import make_hparams

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')


@pytest.fixture(scope='module')
def fix():
    return C.Fixture()


@pytest.fixture(scope='module')
def hp(fix):
    hp = make_hparams()
    assert (hp.hop_length, hp.f0_interval, hp.min_f0, hp.max_f0, hp.uv_cost) == (fix.hop, fix.f0_interval, fix.min_f0, fix.max_f0,
                                                                                  fix.uv_cost)
    return hp


def _to_device(xs):
    host = np.zeros((len(xs), max(len(x) for x in xs)), dtype=np.float32)
    for i, x in enumerate(xs):
        host[i, :len(x)] = x
    return torch.from_numpy(host).to(DEV), torch.tensor([len(x) for x in xs], dtype=torch.int64, device=DEV)


def _track_dev(xs, hp, sr):
    from daft_exprt.extract_features import pitch_track_batch
    w, n = _to_device(xs)
    log_pitch, n_frames, hz, (lags, vals) = pitch_track_batch(w, n, hp, sr=sr)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (log_pitch, n_frames, hz, lags, vals))


_CACHE = {}


def _case(fix, hp, sr):
    ''' the ragged batch at `sr`: (utterances, oracle results, device results), computed once '''
    if sr not in _CACHE:
        xs = C.ragged_batch(fix, sr)
        _CACHE[sr] = (xs, [fix.track(x, sr) for x in xs], _track_dev(xs, hp, sr))
    return _CACHE[sr]


@pytest.mark.parametrize('sr', [22050, 16000])
def test_candidates_match_oracle(fix, hp, sr):
    xs, refs, (_, _, _, lags, vals) = _case(fix, hp, sr)
    geo = fix.geometry(sr)
    bound = C.value_bound(geo)
    assert lags.shape[2] == O.K
    for i, ref in enumerate(refs):
        A = ref['lags'].shape[0]
        assert not lags[i, A:].any() and not vals[i, A:].any()
        assert (np.diff(vals[i, :A], axis=1) <= 0).all()                 # in order of value
        problems = C.compare_candidates(lags[i, :A], vals[i, :A], ref['lags'], ref['vals'], bound)
        n = int((ref['lags'] > 0).sum())
        worst = max((abs(float(vals[i, a, k]) - float(ref['vals'][a, k])) for a in range(A) for k in range(O.K)
                     if ref['lags'][a, k] > 0 and abs(lags[i, a, k] - ref['lags'][a, k]) < 1.5), default=0.)
        print(f'{sr} Hz utterance {i}: {A} frames, {n} oracle candidates, worst value error in place {worst:.3g} (bound {bound:.3g})')
        assert problems == [], problems[:5]
    assert (refs[0]['lags'] > 0).sum() > 500 and (refs[1]['lags'] > 0).sum() > 500


@pytest.mark.parametrize('sr', [22050, 16000])
def test_track_matches_oracle(fix, hp, sr):
    xs, refs, (log_pitch, n_frames, hz, _, _) = _case(fix, hp, sr)
    geo = fix.geometry(sr)
    for i, (x, ref) in enumerate(zip(xs, refs)):
        A, T = ref['hz_a'].shape[0], ref['log_pitch'].shape[0]
        bad, flipped, frames = C.compare_tracks(hz[i, :A], ref, C.path_bound(geo, A))
        print(f'{sr} Hz utterance {i}: {bad} bad, {flipped} flipped of {frames} frames')
        assert bad == 0 and flipped <= C.FLIP_CAP * frames
        assert not hz[i, A:].any()
        # the gather to mel frames and the log: exact restatements of what the kernel itself tracked
        assert n_frames[i] == T == 1 + len(x) // fix.hop
        got = hz[i, :A][ref['mel_to_analysis']]
        want = np.where(got > 0, np.log(np.where(got > 0, got, 1.0).astype(np.float64)), 0.0)
        assert np.abs(log_pitch[i, :T] - want).max() <= 1e-5
        assert ((log_pitch[i, :T] > 0) == (got > 0)).all()
        assert not log_pitch[i, T:].any()
    assert (refs[0]['hz_a'] > 0).sum() > 50
    tone = hz[1, :refs[1]['hz_a'].shape[0]]
    inner = tone[8:-8]
    assert (inner > 0).all() and np.abs(inner / 440.0 - 1.0).max() <= 0.01


@pytest.mark.parametrize('sr', [22050, 16000])
def test_ragged_rows_equal_single_runs(fix, hp, sr):
    xs, _, batch = _case(fix, hp, sr)
    for i, x in enumerate(xs):
        single = _track_dev([x], hp, sr)
        for got, want in zip(batch, single):
            cols = want.shape[1] if want.ndim > 1 else None
            row = got[i] if cols is None else got[i, :cols]
            assert np.array_equal(row, want[0])
            if cols is not None:
                assert not got[i, cols:].any()


def test_against_reference_binary(fix, hp):
    ''' pooled over the four recordings of the fixture, each tracked at its own rate: no worse than the oracle's stored counts
        plus one percentage point (the same flip allowance) '''
    got, stored = np.zeros(4), np.zeros(4)
    for sr in (16000, 22050):
        idx = [i for i in range(4) if fix.sr[i] == sr]
        log_pitch, n_frames, _, _, _ = _track_dev([fix.wav(i) for i in idx], hp, sr)
        for row, i in enumerate(idx):
            lp = log_pitch[row, :int(n_frames[row])].astype(np.float64)
            got += np.array(O.errors(np.where(lp > 0, np.exp(lp), 0.0), fix.hz[i]))
            stored += np.array(fix.err[i])
    print(f'voicing decision error {got[0] / got[1]:.4f} (oracle {stored[0] / stored[1]:.4f}), '
          f'gross pitch error {got[2] / got[3]:.4f} (oracle {stored[2] / stored[3]:.4f})')
    assert got[1] == stored[1]
    assert got[0] / got[1] <= stored[0] / stored[1] + 0.01
    assert got[2] / got[3] <= stored[2] / stored[3] + 0.01


def test_extract_pitch_keeps_the_reference_signature(fix, hp):
    from daft_exprt.extract_features import extract_pitch
    i = fix.index_at(22050)
    pitch = extract_pitch(fix.wav(i), 22050, hp)
    assert isinstance(pitch, np.ndarray) and pitch.shape == (1 + len(fix.x[i]) // fix.hop,)
    _, _, (log_pitch, n_frames, _, _, _) = _case(fix, hp, 22050)
    assert np.array_equal(pitch, log_pitch[0, :int(n_frames[0])])


def test_argument_errors():
    from daft_exprt import _hip as H
    lib = H.lib()
    assert lib.dx_pitch_candidates(None, 0, None, None, None, None, 1, 8, 1, 110.25, 331, 44, 552, None) == -1
    assert b'null' in lib.dx_last_error()
    assert lib.dx_pitch_viterbi(None, None, None, None, None, None, None, 1, 8, 1, 1, 22050, 110.25, 256, 552, 0.9, None) == -1
    assert b'null' in lib.dx_last_error()
    w = torch.zeros(1, 64, device=DEV)
    n = torch.tensor([64], dtype=torch.int64, device=DEV)
    hp48 = make_hparams()
    hp48.min_f0 = 20                                                     # 48 kHz / 20 Hz: window + longest lag does not fit
    from daft_exprt.extract_features import pitch_batch
    with pytest.raises(RuntimeError, match='stages'):
        pitch_batch(w, n, hp48, sr=48000)


def test_extract_reference_parameters_end_to_end(fix, hp, tmp_path):
    from daft_exprt import audio
    from daft_exprt import generate as G
    from daft_exprt.extract_features import mel_spectrogram_batch
    from daft_exprt.model import DaftExprt
    from oracle import daft_exprt_cpu as OC
    from oracle.fill import fill_params
    i = fix.index_at(16000)                                              # 16 kHz: the resampler is on the path
    wav_path = str(tmp_path / 'style.wav')
    audio.write_wav_int16(wav_path, 16000, fix.x[i])
    ref_dir = str(tmp_path / 'refs')
    G.extract_reference_parameters(wav_path, ref_dir, hp)
    ref_file = os.path.join(ref_dir, 'style.npz')
    data = np.load(ref_file)
    assert sorted(data.files) == ['energy', 'mel_spec', 'pitch']
    energy, pitch, mel_spec = data['energy'], data['pitch'], data['mel_spec']
    assert energy.shape[0] == pitch.shape[0] == mel_spec.shape[1] and mel_spec.shape[0] == hp.n_mel_channels
    geo = fix.geometry(hp.sampling_rate)                                 # an interpolated lag lies within half a sample of the lag range
    voiced = np.exp(pitch[pitch > 0].astype(np.float64))
    assert voiced.size > 30 and voiced.min() >= hp.sampling_rate / (geo.lag_max + 0.5) * (1 - 1e-6)
    assert voiced.max() <= hp.sampling_rate / (geo.lag_min - 0.5) * (1 + 1e-6)
    y, sr = audio.load_wav(wav_path, sr=hp.sampling_rate)
    w, n = _to_device([y])
    mel, en, nfr = mel_spectrogram_batch(w, n, hp)
    t = int(nfr[0])
    assert t == mel_spec.shape[1] == 1 + len(y) // hp.hop_length
    assert np.array_equal(mel[0, :, :t].cpu().numpy(), mel_spec) and np.array_equal(en[0, :t].cpu().numpy(), energy)
    # a second call leaves the file untouched
    before = (os.stat(ref_file).st_mtime_ns, open(ref_file, 'rb').read())
    G.extract_reference_parameters(wav_path, ref_dir, hp)
    assert (os.stat(ref_file).st_mtime_ns, open(ref_file, 'rb').read()) == before
    # the batched form writes the same arrays, and skips what exists
    batch_dir = str(tmp_path / 'refs_batch')
    wav22 = str(tmp_path / 'other.wav')
    audio.write_wav_int16(wav22, 22050, fix.x[fix.index_at(22050)])
    G.extract_reference_parameters_batch([wav_path, wav22], batch_dir, hp)
    again = np.load(os.path.join(batch_dir, 'style.npz'))
    for key in ('energy', 'pitch', 'mel_spec'):
        assert np.array_equal(again[key], data[key]), key
    other = np.load(os.path.join(batch_dir, 'other.npz'))
    assert other['pitch'].shape[0] == other['energy'].shape[0] == other['mel_spec'].shape[1] == 1 + len(fix.x[fix.index_at(22050)]) // hp.hop_length
    # a .wav reference and the .npz written from it give identical mels
    hpm = make_hparams(compute_dtype='fp32')
    hpm.stats = {f'spk {s}': {'pitch': {'mean': 5.0, 'std': 0.3}} for s in range(11)}
    model = DaftExprt(hpm)
    model.load_state_dict(fill_params(OC.param_shapes(hpm)))
    model = model.cuda(0)
    sentences = [[['UW0', 'IH0'], ' ', ['UH0', 'B'], ',', ['IY2', 'AO2'], '~']]
    outs = []
    for kind, ref in (('wav', wav_path), ('npz', ref_file)):
        names = ['utt']
        preds = G.generate_mel_specs(model, sentences, names, [3], [ref], str(tmp_path / f'out_{kind}'), hpm)
        assert list(preds.keys()) == ['utt_spk_3_ref_style']
        outs.append(preds['utt_spk_3_ref_style'])
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


def test_reference_parameters_of_a_mixed_rate_batch_equal_single_files(fix, hp, tmp_path):
    ''' one `reference_parameters` call on four files: two at 16 kHz of different lengths with the shorter one first (a rate
        group of ragged rows), one at the target rate (no resample), one at 44.1 kHz (a second resample launch).  In file
        order short16, fast44, same22, long16 the rate groups, taken in order of rate, are the rows [0, 3], [2], [1]: the
        16 kHz rows are not adjacent and the groups are not in file order.  Each file's arrays equal, bit for bit, what the
        public pieces give for that file alone on its own one-row tensor. '''
    from daft_exprt import audio
    from daft_exprt import generate as G
    from daft_exprt.extract_features import mel_spectrogram_batch, pitch_batch
    x16, x22 = fix.x[fix.index_at(16000)], fix.x[fix.index_at(22050)]
    files = (('short16', 16000, x16[:2 * len(x16) // 3 + 1]), ('fast44', 44100, x22), ('same22', 22050, x22), ('long16', 16000, x16))
    paths = []
    for name, rate, x in files:
        paths.append(str(tmp_path / f'{name}.wav'))
        audio.write_wav_int16(paths[-1], rate, x)
    assert hp.sampling_rate == 22050
    got = G.reference_parameters(paths, hp)
    assert len(got) == len(paths)
    lengths = set()
    for path, (energy, pitch, mel_spec) in zip(paths, got):
        y, sr = audio.load_wav(path, sr=hp.sampling_rate)
        assert sr == hp.sampling_rate
        w, n = _to_device([y])
        mel, en, nfr = mel_spectrogram_batch(w, n, hp)
        lp, npf = pitch_batch(w, n, hp)
        t = int(nfr[0])
        assert t == int(npf[0]) == 1 + len(y) // hp.hop_length
        assert np.array_equal(en[0, :t].cpu().numpy(), energy), path
        assert np.array_equal(lp[0, :t].cpu().numpy(), pitch), path
        assert np.array_equal(mel[0, :, :t].cpu().numpy(), mel_spec), path
        lengths.add(len(y))
    assert len(lengths) == 4                                             # every row of the batch has a length of its own
