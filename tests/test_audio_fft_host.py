"""tests/audio_fft_oracle.py, CPU only: pinned to the goldens the reference wrote (tests/golden/mel_frontend.npz, griffin_lim.npz) and
to the older oracles (oracle/mel_frontend_cpu.py over torch.stft, tests/griffin_lim_oracle.py), so that the restatement the GPU file
(tests/test_gpu_audio_fft.py) trusts is not a second unchecked implementation; and the conditions its tolerances stand on, asserted
for every case of the oracle module.  Every float comparison goes through the module's own rule (`bound`) and prints what it measured."""
import os

import numpy as np
import pytest

from tests import audio_fft_oracle as O
from tests import griffin_lim_oracle as GO
from tests.util import make_hparams

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
F64, F32 = np.float64, np.float32


def _within(what, got, o64, o32, factor=8.):
    cost, m, tol = O.bound(o64, o32, factor)
    err = float(np.abs(np.asarray(got, F64) - o64).max()) if np.asarray(o64).size else 0.
    print(f'{what}: err {err:.3g}, fp32 oracle cost {cost:.3g}, m {m:.3g}, bound {tol:.3g}')
    assert err <= tol, (what, err, tol)
    return cost


# ---- front-end -------------------------------------------------------------------------------------------------------------------

def test_mel_frontend_matches_the_reference_fixture_and_the_stft_oracle():
    ''' 1024 / 256 / 80: the float32 outputs of the reference's own mel_spectrogram_HiFi and of oracle.mel_frontend_cpu (torch.stft,
        float32) lie within the rule's bound of the float64 restatement, centred and not '''
    from oracle import mel_frontend_cpu as M
    fx = np.load(os.path.join(GOLDEN, 'mel_frontend.npz'))
    for centred in (1, 0):
        hp = make_hparams(centered=bool(centred))
        for i in range(5):
            k = f'c{centred}_{i}'
            wav = fx[f'{k}_wav']
            (mel64, en64), (mel32, en32) = (O.mel_frontend(wav, len(wav), 1024, 256, 80, centred, dtype=dt) for dt in (F64, F32))
            assert mel64.shape == fx[f'{k}_mel'].shape and mel64.dtype == F64 and mel32.dtype == F32
            _within(f'{k} log-mel vs fixture', fx[f'{k}_mel'], mel64, mel32)
            _within(f'{k} energy vs fixture', fx[f'{k}_energy'], en64, en32)
            stft = M.mel_spectrogram(wav, hp)
            _within(f'{k} log-mel vs torch.stft oracle', stft, mel64, mel32)
            _within(f'{k} energy vs torch.stft oracle', M.frames_energy(stft), en64, en32)


def test_frame_counts():
    assert [O.frame_count(n, 1024, 256, 0) for n in (0, 1023, 1024, 1279, 1280)] == [0, 0, 1, 1, 2]
    assert [O.frame_count(n, 1024, 256, 1) for n in (513, 1023, 1024, 1279, 1280)] == [3, 4, 5, 5, 6]
    for n_fft, hop, centred, n, _ in O.FRONTEND_CASES.values():
        frames = [O.frame_count(k, n_fft, hop, centred) for k in n]
        assert frames == ([3 if hop * 4 == n_fft else 2, 5, 6] if centred else [0, 1, 1, 2]), (n_fft, hop, centred)
        assert n_fft % hop == 0 or hop == n_fft // 4 + 3
        if centred:
            assert n[0] == n_fft // 2 + 1                              # every sample reflected at both ends


@pytest.mark.parametrize('name', list(O.FRONTEND_CASES))
def test_front_end_cases_cost_something(name):
    n_fft, hop, centred, n, wav = O.frontend_inputs(name)
    for n_mel in O.N_MELS:
        for b, k in enumerate(n):
            (mel64, en64), (mel32, en32) = (O.mel_frontend(wav[b], k, n_fft, hop, n_mel, centred, dtype=dt) for dt in (F64, F32))
            if mel64.size == 0:
                continue
            assert _within(f'{name} n_mel {n_mel} b {b} log-mel', mel32, mel64, mel32, factor=1.) > 0.
            assert _within(f'{name} n_mel {n_mel} b {b} energy', en32, en64, en32, factor=1.) > 0.
            assert np.isfinite(mel64).all() and (mel64 > np.log(F32(O.MIN_CLIP))).any()


@pytest.mark.parametrize('n_fft', O.SIZES)
def test_tone_cases_are_what_they_say(n_fft):
    ''' silence: every channel log(max(sum w sqrt(1e-9), min_clip)); the loud tone: no channel clipped but the empty ones; the quiet
        tone: the upper channels all clipped, the lowest quarter never as a whole '''
    hop, n, wav = O.tone_inputs(n_fft)
    floor = np.log(F64(F32(O.MIN_CLIP)))
    for n_mel in O.N_MELS:
        A = O.filterbank(n_fft, n_mel).astype(F64)
        empty = ~(A > 0).any(1)
        silent, loud, quiet = (O.mel_frontend(wav[b], n[b], n_fft, hop, n_mel, 1)[0] for b in range(3))
        want = np.log(np.maximum(A.sum(1) * np.sqrt(1e-9), F64(F32(O.MIN_CLIP))))
        assert silent.shape == (n_mel, 4) and np.abs(silent - want[:, None]).max() <= 1e-12
        assert (loud[~empty] > floor).all() and (loud[empty] == floor).all()
        if n_mel >= 64:
            assert (quiet[-10:] == floor).all() and (quiet[:n_mel // 4].max(0) > floor).all()
    assert int((~(O.filterbank(256, 80) > 0).any(1)).sum()) == 4 and not (~(O.filterbank(1024, 80) > 0).any(1)).any()


# ---- tables ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n_fft', O.SIZES)
def test_tables_are_the_definition(n_fft):
    import torch
    tw, periodic = O.tables(n_fft, False)
    symmetric = O.tables(n_fft, True)[1]
    n = np.arange(n_fft)
    eps = 2 * np.pi * 2. ** -52                                          # the rounding of the angle 2 pi n / n_fft that np.exp is given
    assert np.abs(tw[:, 0] + 1j * tw[:, 1] - np.exp(-2j * np.pi * n / n_fft)).max() <= eps
    assert tw[n_fft // 4, 0] == 0. and tw[n_fft // 2, 1] == 0. and tw[0, 0] == 1. and tw[n_fft // 4, 1] == -1.      # quarter points exact
    assert np.abs(periodic - torch.hann_window(n_fft, periodic=True, dtype=torch.float64).numpy()).max() <= eps
    assert np.abs(symmetric - np.hanning(n_fft)).max() <= eps
    assert periodic[0] == 0. and symmetric[0] == 0. and symmetric[-1] == 0. and periodic[-1] > 0.
    assert np.abs(periodic - symmetric).max() > 1e-4


# ---- NNLS ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n_fft', O.SIZES)
@pytest.mark.parametrize('n_mel', O.NNLS_MELS)
def test_nnls_tables_layout(n_fft, n_mel):
    A, t = O.case_tables(n_fft, n_mel)
    bins = n_fft // 2 + 1
    assert A.shape == (n_mel, bins) and A.dtype == F32 and t['pinv_t'].shape == (n_mel, bins) and t['pinv_t'].dtype == F32
    nz = A > 0
    assert nz.sum(0).max() <= 2                                         # every bin in at most two filters
    for m in range(n_mel):
        lo, hi = int(t['lo'][m]), int(t['hi'][m])
        if nz[m].any():
            assert 0 <= lo < hi <= bins and nz[m, lo:hi].all() and nz[m].sum() == hi - lo       # one contiguous range
        else:
            assert lo == hi                                             # an empty filter
    for k in range(bins):
        ms = [int(m) for m in t['bin_m'][k] if m >= 0]
        assert ms == list(np.nonzero(nz[:, k])[0]) and (t['bin_m'][k, len(ms):] == -1).all()
        assert all(t['bin_w'][k, i] == A[m, k] for i, m in enumerate(ms)) and (t['bin_w'][k, len(ms):] == 0).all()
    assert abs(t['step'] * np.linalg.svd(A.astype(F64), compute_uv=False)[0] ** 2 - 1.) <= 1e-12
    A64 = A.astype(F64)
    P = np.linalg.pinv(A64)
    assert np.abs(A64 @ P @ A64 - A64).max() <= 1e-9 * np.abs(A64).max() and np.array_equal(t['pinv_t'], P.T.astype(F32))
    empty = int((~nz.any(1)).sum())
    print(f'n_fft {n_fft} n_mel {n_mel}: {empty} empty filters, {int((~nz.any(0)).sum())} bins in no filter')
    if n_fft == 256:
        assert empty == {1: 0, 64: 0, 65: 0, 80: 4, 256: 108}[n_mel]
    else:
        assert empty == 0


@pytest.mark.parametrize('n_fft', O.SIZES)
def test_fista_objective_over_50_steps(n_fft):
    ''' 50 steps do not raise the objective of any frame, nor does the first (t = 1: no momentum, a projected gradient step of size
        1 / L).  Step to step FISTA is not monotone -- the momentum overshoots near the minimum, by up to 7.3 x at n_fft 1024 where the
        objective has fallen from 4e-7 to 1e-11 -- so that is printed, not asserted '''
    for n_mel in (80, 256):
        A, t = O.case_tables(n_fft, n_mel)
        _, mel = O.nnls_inputs(n_fft, n_mel, 0)
        trace = []
        O.fista(A, mel[0], 50, t['step'], pinv_t=t['pinv_t'], trace=trace)
        trace = np.stack(trace)
        print(f'n_fft {n_fft} n_mel {n_mel}: objective {trace[0].max():.3g} -> {trace[-1].max():.3g}, '
              f'largest step-to-step ratio {float((trace[1:] / trace[:-1]).max()):.6f}')
        assert (trace[1] <= trace[0]).all() and (trace[50] <= trace[0]).all()


def test_fista_500_steps_meet_the_reference_residuals():
    ''' the rule of tests/test_gpu_griffin_lim.py on the golden frames: per frame || A x - b || / || b || <= reference (1 + 1e-3) + 1e-4 '''
    fx = np.load(os.path.join(GOLDEN, 'griffin_lim.npz'))
    A, t = O.case_tables(1024, 80)
    assert np.array_equal(A, GO.filterbank(make_hparams()))
    for name in ('dec', 'cone', 'noisy', 'edge'):
        b = np.exp(fx[f'nnls_{name}_mel'].astype(F64))
        x = O.fista(A, b, 500, t['step'], pinv_t=t['pinv_t'])
        res, ref = GO.rel_residual(A, x, b), fx[f'nnls_{name}_relres']
        print(f'{name}: largest residual - reference {float((res - ref).max()):.3g}')
        assert (x >= 0).all() and (res <= ref * (1 + 1e-3) + 1e-4).all(), name


@pytest.mark.parametrize('key', list(O.NNLS_CASES))
def test_nnls_cases_cost_something(key):
    n_fft, n_mel = key
    A, t = O.case_tables(n_fft, n_mel)
    sensitivity = O.nnls_log_sensitivity(n_fft, n_mel)
    print(f'{key}: one ulp on exp(mel) moves the start by at most {sensitivity:.3g} m')
    assert (sensitivity <= 2e-6 / 8.) == (key in O.NNLS_LOG_PAIRS)
    for is_log in (0, 1):
        lengths, mel = O.nnls_inputs(n_fft, n_mel, is_log)
        assert lengths == (O.NNLS_T, 1, 0) and np.isfinite(mel).all()
        for iters in O.NNLS_ITERS:
            for b, L in enumerate(lengths[:2]):
                x64, x32 = (O.mel_to_linear(mel[b, :, :L], A, iters, t['step'], is_log, dt, t['pinv_t']) for dt in (F64, F32))
                assert x64.shape == (n_fft // 2 + 1, L) and x64.max() > 0 and (x64 >= 0).all()
                assert _within(f'{key} log {is_log} iters {iters} b {b}', x32, x64, x32, factor=1.) > 0.


# ---- Griffin-Lim -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('T', (3, 24, 64, 100))
def test_griffin_lim_float64_did_not_move(T):
    ''' as tests/test_griffin_lim_host.py::test_oracle_matches_reference_fixture, and the bits of the function it restates '''
    fx = np.load(os.path.join(GOLDEN, 'griffin_lim.npz'))
    hp = make_hparams()
    n_fft, hop = hp.filter_length, hp.hop_length
    mag = GO.harmonic_magnitude(T)[:, :-2]
    S = GO.n_samples(T, n_fft, hop)
    x0 = GO.reference_start(int(fx[f'gl_{T}_seed']), S)
    sigs, proposal = O.griffin_lim(mag, hop, 30, x0, dtype=F64)
    old, old_proposal = GO.griffin_lim(mag, hop, 30, x0)
    assert all(np.array_equal(a, b) for a, b in zip(sigs, old)) and np.array_equal(proposal, old_proposal)
    rel = lambda a, b: float(np.linalg.norm(np.asarray(a, F64) - b) / np.linalg.norm(b))  # noqa: E731
    if f'gl_{T}_sig1' in fx.files:
        assert rel(sigs[0], fx[f'gl_{T}_sig1']) <= 1e-6
    assert rel(sigs[29], fx[f'gl_{T}_sig30']) <= 1e-6
    assert np.abs(sigs[29][-hop:]).max() == 0.
    if f'gl_{T}_norm30' in fx.files:
        norm = O.normalise(sigs[29])
        assert np.abs(norm - fx[f'gl_{T}_norm30']).max() <= 1e-6 and np.abs(norm).max() == 1.
    s32 = O.griffin_lim(mag, hop, 1, x0, dtype=F32)[0][0]
    assert s32.dtype == F32
    _within(f'T {T}: float32 run after 1 iteration', s32, sigs[0], s32, factor=1.)


@pytest.mark.parametrize('name', list(O.GL_CASES))
def test_griffin_lim_cases_are_well_conditioned(name):
    n_fft, hop, lengths, mag, x0 = O.gl_inputs(name)
    assert lengths == (7, 4, 3, 2, 0) and [GO.n_frames(T) for T in lengths] == [5, 2, 1, 0, 0] and n_fft % hop == 0
    assert mag.shape == (5, n_fft // 2 + 1, O.GL_T) and x0.shape == (5, GO.n_samples(O.GL_T, n_fft, hop))
    ratio = O.gl_condition(name, 2)
    print(f'{name}: min |R| / median |R| over two iterations {ratio:.3g}')
    assert ratio >= O.CONDITION
    for iterations in (1, 2):
        o64, o32 = (O.gl_oracle(name, iterations, dt) for dt in (F64, F32))
        for b in range(3):
            assert _within(f'{name} iterations {iterations} b {b}', o32[b], o64[b], o32[b], factor=1.) > 0.
        assert all(o64[b].shape == (n_fft,) and not o64[b].any() for b in (3, 4))
    if hop * 4 == n_fft:
        kw = dict(lengths=O.GL_ZERO_LENGTHS, zero_first=True)
        ratio = O.gl_condition(name, 1, **kw)                       # the utterance beside the silent start
        print(f'{name}, beside x0 = 0: {ratio:.3g}')
        assert ratio >= O.CONDITION
        o64, o32 = (O.gl_oracle(name, 1, dt, **kw) for dt in (F64, F32))
        F, Sb = 3, GO.n_samples(5, n_fft, hop)
        w = np.hanning(n_fft)
        want = np.zeros(Sb)
        for f in range(F):                                            # phase 0 everywhere: the overlap-add of w irfft(S)
            want[f * hop: f * hop + n_fft] += w * np.fft.irfft(mag[0, :, f])
        assert np.abs(o64[0] - want / (n_fft / hop / 2)).max() <= 1e-12 * np.abs(want).max()
        assert _within(f'{name} x0 = 0', o32[0], o64[0], o32[0], factor=1.) > 0.


# ---- noise, normalise ------------------------------------------------------------------------------------------------------------

def test_noise_is_a_standard_normal_of_exact_uniforms():
    n_fft, hop, T, lengths, seeds = O.NOISE_CASE
    S = GO.n_samples(T, n_fft, hop)
    assert GO.n_samples(max(lengths), n_fft, hop) > 256 + 64 and seeds == (0, 1, 2 ** 64 - 1)
    rows = {}
    for seed in seeds:
        for b in range(3):
            v64, v32 = O.noise(seed, b, np.arange(S), F64), O.noise(seed, b, np.arange(S), F32)
            assert _within(f'seed {seed} b {b}', v32, v64, v32, factor=1.) > 0.
            rows[(seed, b)] = v64
    keys = list(rows)
    assert all(not np.array_equal(rows[a], rows[b]) for i, a in enumerate(keys) for b in keys[i + 1:])       # across seeds and b
    v = O.noise(5, 0, np.arange(1 << 18))
    assert len(np.unique(v)) > 0.98 * len(v)                                                                  # across s
    assert abs(v.mean()) < 0.01 and abs(v.std() - 1.) < 0.01 and abs((v > 0).mean() - 0.5) < 0.01
    assert np.array_equal(O.noise(5, 0, [1 << 31]), O.noise(5, 0, [0]))                                       # the counter 2 s wraps at 2^32


@pytest.mark.parametrize('name', list(O.NORMALISE_CASES))
def test_normalise_cases(name):
    n_fft, hop, T, lengths, x = O.normalise_inputs(name)
    sign = O.NORMALISE_CASES[name][4]
    n = [GO.n_samples(L, n_fft, hop) for L in lengths]
    assert x.shape == (4, GO.n_samples(T, n_fft, hop)) and max(n) < x.shape[1] and lengths[3] <= 2
    assert np.abs(x[0, :n[0]]).argmax() == 0 and np.sign(x[0, 0]) == sign
    assert np.abs(x[1, :n[1]]).argmax() == n[1] - 1 and np.sign(x[1, n[1] - 1]) == -sign
    assert not x[2].any() and x[3, :n[3]].any()
    assert all(not x[b, n[b]:].any() for b in range(4))
    assert np.abs(O.normalise(x[1, :n[1]])).max() == 1. and not O.normalise(x[2, :n[2]]).any()
