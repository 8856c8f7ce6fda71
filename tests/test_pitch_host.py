"""CPU checks of the pitch tracker's definition (tests/pitch_oracle.py, float64): synthetic signals of known pitch, the
recorded agreement with the reference's own pitch binary (tests/golden/pitch_reaper.npz, tools/gen_golden_pitch.py), the
frame-count contract, and that float32 arithmetic alone keeps the oracle within the allowance the GPU tests grant."""
import numpy as np
import pytest

from tests import pitch_cases as C
from tests import pitch_oracle as O

HOP, F0_INTERVAL, MIN_F0, MAX_F0, UV_COST = 256, 0.005, 40, 500, 0.9
SILENCE_S = 0.2


@pytest.fixture(scope='module')
def fix():
    return C.Fixture()


def _padded(tone, sr):
    z = np.zeros(int(round(SILENCE_S * sr)), dtype=np.float32)
    return np.concatenate([z, tone, z]), z.shape[0], z.shape[0] + tone.shape[0]


def _check(x, begin, end, sr, truth, tolerance):
    ''' truth(sample) -> Hz.  Frames are judged by their centre sample; "further than one window" is the 15 ms correlation
        window, the narrower of the two spans a frame reads. '''
    r = O.track(x, sr, HOP, F0_INTERVAL, MIN_F0, MAX_F0, UV_COST)
    geo = r['geo']
    hz = r['hz_a']
    centres = np.array([geo.centre(a) for a in range(hz.shape[0])])
    silent = (centres < begin - geo.window) | (centres >= end + geo.window)
    inside = (centres >= begin + geo.window) & (centres < end - geo.window)
    assert silent.sum() > 20 and inside.sum() > 20
    assert not (hz[silent] > 0).any(), f'voiced in silence at frames {np.nonzero(silent & (hz > 0))[0]}'
    assert (hz[inside] > 0).all(), f'unvoiced inside the tone at frames {np.nonzero(inside & ~(hz > 0))[0]}'
    rel = np.abs(hz[inside] / truth(centres[inside]) - 1.0)
    assert rel.max() <= tolerance, f'worst relative error {rel.max():.4f} at frame {np.nonzero(inside)[0][rel.argmax()]}'
    return r


@pytest.mark.parametrize('sr', [16000, 22050])
@pytest.mark.parametrize('f0', [60, 110, 220, 440])
def test_oracle_steady_tone(sr, f0):
    # integer-lag resolution alone is 1 / lag = 2 % at 440 Hz / 22.05 kHz: the interpolation has to at least halve it
    x, begin, end = _padded(C.harmonic_tone(float(f0), sr, 0.5), sr)
    _check(x, begin, end, sr, lambda c: np.full(c.shape, float(f0)), 0.01)


@pytest.mark.parametrize('sr', [16000, 22050])
def test_oracle_glide(sr):
    # window + longest lag span about 40 ms: at 200 Hz / s that is about 8 Hz of legitimate smear at 100 - 300 Hz
    n = sr
    f = 100.0 + 200.0 * np.arange(n) / n
    x, begin, end = _padded(C.harmonic_tone(f, sr, 1.0), sr)
    _check(x, begin, end, sr, lambda c: 100.0 + 200.0 * (c - begin) / n, 0.05)


def test_oracle_against_reference_binary(fix):
    ''' the stored counts (voicing decisions that differ, frames, gross errors, frames both voiced) are what the oracle gives now,
        and the generator's bar -- the untuned prototype: 8.1 % voicing, 5.1 % gross, pooled over all 15 recordings -- holds for
        the stored pooled counts '''
    assert len(fix.names) == 4 and sorted(fix.sr) == [16000, 16000, 22050, 22050]
    assert (fix.hop, fix.f0_interval, fix.min_f0, fix.max_f0, fix.uv_cost) == (HOP, F0_INTERVAL, MIN_F0, MAX_F0, UV_COST)
    for i in range(4):
        r = fix.track(fix.wav(i), fix.sr[i])
        assert r['hz'].shape == fix.hz[i].shape
        assert O.errors(r['hz'], fix.hz[i]) == fix.err[i], fix.names[i]
    assert fix.n_pooled == 15
    vde, frames, gross, both = fix.pooled
    print(f'pooled: voicing decision error {vde / frames:.4f}, gross pitch error {gross / both:.4f}')
    assert vde / frames <= 0.081 and gross / both <= 0.051


@pytest.mark.parametrize('hop', [256, 200])
def test_frame_count_contract(hop):
    ''' 1 + n // hop is what `pitch[::hop]` plus the `len % hop == 0` append gives (`extract_features.py:260-264`) '''
    for k in (1, 2, 40):
        for n in (hop * k - 1, hop * k, hop * k + 1):
            per_sample = np.zeros(n)
            frames = per_sample[::hop]
            if n % hop == 0:
                frames = np.append(frames, per_sample[-1])
            assert O.n_mel_frames(n, hop) == len(frames) == 1 + n // hop
    x = C.harmonic_tone(200.0, 16000, (hop * 40 + 1) / 16000)
    for n in (hop * 40 - 1, hop * 40, hop * 40 + 1):
        r = O.track(x[:n], 16000, hop, F0_INTERVAL, MIN_F0, MAX_F0, UV_COST)
        assert r['log_pitch'].shape == (1 + n // hop,)
        assert r['mel_to_analysis'].max() <= r['hz_a'].shape[0] - 1


@pytest.mark.parametrize('sr', [22050, 16000])
def test_float32_oracle_stays_within_the_flip_allowance(fix, sr):
    ''' the inputs of the GPU tests, tracked by the oracle in float32 and compared as the kernels are: no frame disagrees where
        the float64 oracle's two best path costs are further apart than the fp32 bound, and the frames that do disagree stay
        under the cap -- so what the GPU tests allow is enough for fp32 arithmetic as such '''
    geo = fix.geometry(sr)
    for i, x in enumerate(C.ragged_batch(fix, sr)):
        r64, r32 = fix.track(x, sr), fix.track(x, sr, dtype=np.float32)
        assert C.compare_candidates(r32['lags'], r32['vals'], r64['lags'], r64['vals'], C.value_bound(geo)) == []
        bad, flipped, frames = C.compare_tracks(r32['hz_a'], r64, C.path_bound(geo, r64['hz_a'].shape[0]))
        print(f'{sr} Hz utterance {i}: {bad} bad, {flipped} flipped of {frames}')
        assert bad == 0 and flipped <= C.FLIP_CAP * frames
