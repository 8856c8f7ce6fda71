"""K17, the mel / energy front-end (csrc/frontend.hip), and K18, the Griffin-Lim preview path (csrc/griffin_lim.hip: NNLS mel -> linear,
Griffin-Lim, noise, normalise), with the table kernel and the power-of-4 LDS FFT of csrc/dx_fft.h that serve both: every kernel alone,
through the C ABI, against the float64 restatement of tests/audio_fft_oracle.py -- never against the code under test.  The tables the
kernels get are the ORACLE's (rounded to float32), so the kernels and the table builders (dx_mel_tables / dx_gl_tables, `mel_tables`,
`_nnls_tables`) are judged separately.  tests/test_audio_fft_host.py pins the oracle and asserts what the tolerances stand on.

One rule serves every float comparison, per tensor and per utterance, m = max |o64| (`audio_fft_oracle.bound`):
    max |y - o64| <= max(8 x max |o32 - o64|, 2e-6 m),   o32 the float32 CPU run of the same restatement
and every comparison prints err, cost, m, bound and err / bound.  Beside it stand only the 1-ulp checks of the tables and of the
normalised signal.  NaN stands behind every boundary: past n_samples[b] and ldw of every waveform, in the frames of mel / mag at or past
each utterance's, in the padding of every output and all over every output and workspace before the call.

    kernel                          instantiations / paths                        tests
    dx_fft_tables_kernel            periodic, symmetric x 256, 1024, 4096         test_tables_*
    fe_fft_mel_kernel<NFFT>         3 sizes x hop n/4, n/4 + 3 x centred 0, 1     test_front_end[*] (48), test_front_end_tones[*] (12),
                                    x n_mel 1, 64, 65, 80                         test_front_end_wrapper[*]
    gl_nnls_kernel<NFFT>            3 sizes x n_mel 1, 64, 65, 80, 256 x iters    test_mel_to_linear[*] (120), test_nnls_tables_of_the_wrapper[*]
                                    0, 1, 5, 50 x log / linear x 2 layouts
    gl_frames_kernel<NFFT>, ola     3 sizes x hop n/4, n/8, n/2 x 1, 2 iterations test_griffin_lim[*] (18), test_griffin_lim_from_silence[*],
                                                                                  test_griffin_lim_alone_is_bit_equal[*]
    gl_noise_kernel                 seeds 0, 1, 2^64 - 1                          test_noise
    gl_normalise_kernel                                                           test_normalise[*]

Measured on an MI355X (209 tests, 8 s together, the slowest 0.24 s), the largest err / bound per kernel over every comparison it prints:
    fe_fft_mel_kernel     0.31  (485 + 72 + 17 figures; tones 1024, n_mel 80, the loud tone's log-mel: err 3.9e-6, cost 1.6e-6)
    gl_nnls_kernel        0.23  (336 figures; 1024, n_mel 1, 5 steps, linear input: err 3.9e-7, cost 2.1e-7)
    gl_frames / gl_ola    0.20  (75 figures; 1024 / 256, one iteration, the 2-frame utterance: err 2.8e-8, cost 1.3e-8, m 0.069)
    gl_noise_kernel       0.05  (err 2.7e-7 under a cost of 6.8e-7: cospif takes 2 u2 exactly, the restatement rounds 2 pi u2)
    tables, normalise     0 ulp everywhere
The float32 cost (o32 against o64) in that run: one or two Griffin-Lim iterations 1.0 - 2.1e-7 m, FISTA up to 50 steps at most 5.8e-6 m, the
front-end's log-mel and energy at most 6.5e-6 m, the noise 1.5 - 3.7e-7 m.

What the first run on the GPU taught about the restatement's float32 run -- the kernels were right each time (a float32 NumPy emulation
of dx_fft_lds and of the in-order sums reproduces their figures), and the restatement changed, never the rule:
  * A library FFT keeps the symmetry of its input.  The first frame of every centred utterance is even (reflect padding), its
    spectrum real, and NumPy's float32 rfft was then exact to 1e-9 where any float32 butterfly network errs by 1e-7 max |X|: at n_fft 256,
    where a low channel is ONE bin, a bin of 5e-4 max |X| put the kernel 3.2 x past a bound whose cost saw nothing.  The front-end's
    spectrum is now the DFT's definition as a matrix product on the oracle's own table, as tests/spectrogram_oracle.py has it.
  * A blocked sum understates float32.  One filter of n_mel 1 spans 372 bins at 1024 and 1488 at 4096; summed in index order, as
    the kernels do, float32 costs about sqrt(n) ulp there, a BLAS dot a tenth of it (energy of the quiet tone, 4096: 1.4 x past the floor;
    FISTA 1024, n_mel 1, 50 steps: 1.3 x).  The float32 run takes the filterbank products in index order (`in_order`).
  * exp() in front of an ill-conditioned solve.  pinv(A) of (256, 64) and (256, 80) has norm 8e7 and 2e6; the last bit of exp(mel)
    comes out 9 - 37 ulp of max |x| wide, past the rule whatever computes it (1.4 x for the kernel's expf, which is the accurate one: v_exp_f32
    on a split argument).  The log-mel comparison is made at the thirteen pairs where one ulp on b moves the start by less than
    2e-6 m / 8 (`NNLS_LOG_PAIRS`, asserted on the host); linear input runs at all fifteen.
  * `HyperParams` refuses a hop that does not divide filter_length, so the wrapper runs at 256 / 64 and 4096 / 1024, not at hop n / 4 + 3.
  * x0 = 0 runs ONE iteration: its second one's input misses the conditioning threshold at 1024 and 4096 for every seed.

Defects found: none, in the kernels or the wrappers.

Built to fail: one arithmetic-only mutation per kernel, each in a scratch build of the library that is not committed, each run once
against this file (the older tests were not run against them).  Failures of the 209 tests:
    fe_fft_mel_kernel     `+ 1e-9f` dropped from |X|                     11: test_front_end_tones, all but [256-1] (silence there is clipped
                                                                              with or without it); no random signal notices 1e-9
    gl_nnls_kernel        mom = t / tn                                   44: test_mel_to_linear at 5 and 50 steps, every pair but n_mel 1
                                                                              (rank 1: the first step lands on the minimiser)
    gl_nnls_kernel        wa / wb of a bin swapped in A^T r              66: test_mel_to_linear at 1, 5 and 50 steps, every pair but n_mel 1
    gl_frames_kernel      sign of the second frame's imaginary part      21: all 18 test_griffin_lim, 3 test_griffin_lim_from_silence
    gl_ola_kernel         scale n_fft / hop / 4                          21: the same
    gl_noise_kernel       counter constant 0x68E31DA4 -> ...A6           1:  test_noise
    gl_normalise_kernel   maximum over S in place of n_samples[b]        2:  test_normalise (the 1e30 past n_samples enters)
    table kernel          symmetric window by the periodic formula       3:  test_tables_within_one_ulp_of_the_definition
"""
import functools

import numpy as np
import pytest
import torch

from tests import audio_fft_oracle as O
from tests import griffin_lim_oracle as GO
from tests.util import make_hparams

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAN = float('nan')
F64, F32 = np.float64, np.float32


def _H():
    from daft_exprt import _hip as H
    return H


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).to(DEV)


def _check(what, got, o64, o32):
    ''' the module's rule on one tensor of one utterance '''
    got, o64 = np.asarray(got, F64), np.asarray(o64, F64)
    assert got.shape == o64.shape, (what, got.shape, o64.shape)
    assert np.isfinite(got).all(), what
    cost, m, tol = O.bound(o64, o32)
    err = float(np.abs(got - o64).max()) if o64.size else 0.
    print(f'{what}: err {err:.3g}, fp32 oracle cost {cost:.3g}, m {m:.3g}, bound {tol:.3g}, err/bound {err / tol if tol else 0.:.3f}')
    assert err <= tol, (what, err, tol)


def _gather(checks):
    ''' runs every check, so that every tensor is measured before the test fails '''
    missed = []
    for args in checks:
        try:
            _check(*args)
        except AssertionError as e:
            missed.append(e.args[0])
    assert not missed, missed


@functools.lru_cache(maxsize=None)
def _fft_tables(n_fft, symmetric):
    tw, w = O.tables(n_fft, symmetric)
    return _dev(tw.reshape(-1)), _dev(w)


@functools.lru_cache(maxsize=None)
def _mel_tables(n_fft, n_mel):
    A, t = O.case_tables(n_fft, n_mel)
    return dict(fb=_dev(A), lo=_dev(t['lo'], torch.int32), hi=_dev(t['hi'], torch.int32), pinv_t=_dev(t['pinv_t']),
                bin_m=_dev(t['bin_m'].reshape(-1), torch.int32), bin_w=_dev(t['bin_w'].reshape(-1)), step=t['step'])


def _i64(values):
    return torch.tensor(list(values), dtype=torch.int64, device=DEV)


# ---- tables ----------------------------------------------------------------------------------------------------------------------

def _device_tables(n_fft, symmetric):
    H = _H()
    tw = torch.full((2 * n_fft,), NAN, dtype=torch.float32, device=DEV)
    w = torch.full((n_fft,), NAN, dtype=torch.float32, device=DEV)
    with torch.cuda.device(DEV):
        H.check((H.lib().dx_gl_tables if symmetric else H.lib().dx_mel_tables)(H.ptr(tw), H.ptr(w), n_fft, H.stream()))
        torch.cuda.synchronize()
    return tw.cpu().numpy().reshape(n_fft, 2), w.cpu().numpy()


@pytest.mark.parametrize('n_fft', O.SIZES)
def test_tables_within_one_ulp_of_the_definition(n_fft):
    windows = {}
    for symmetric in (False, True):
        tw, w = _device_tables(n_fft, symmetric)
        tw64, w64 = O.tables(n_fft, symmetric)
        u_tw, u_w = O.ulps32(tw, tw64), O.ulps32(w, w64)
        print(f'n_fft {n_fft} symmetric {symmetric}: twiddle {u_tw:.3g} ulp, window {u_w:.3g} ulp')
        assert u_tw <= 1. and u_w <= 1.
        assert w[0] == 0. and tw[0, 0] == 1. and tw[n_fft // 4, 0] == 0. and tw[n_fft // 4, 1] == -1.
        windows[symmetric] = w
    assert windows[True][-1] == 0. and windows[False][-1] > 0.
    assert np.abs(windows[True].astype(F64) - windows[False]).max() > 1e-4        # two windows, not one
    from daft_exprt.audio import fft_tables                                    # the cached pair of the wrappers: the same bits
    for symmetric in (False, True):
        tw, w = fft_tables(n_fft, symmetric, torch.device(DEV))
        assert np.array_equal(w.cpu().numpy(), windows[symmetric]) and np.array_equal(tw.cpu().numpy().reshape(n_fft, 2),
                                                                                       _device_tables(n_fft, symmetric)[0])


# ---- front-end -------------------------------------------------------------------------------------------------------------------

def _front_end(n_fft, hop, centred, n_mel, n, wav, min_clip=O.MIN_CLIP, pad=7, extra=2):
    ''' wav (B, >= max n) on the CPU -> (mel (B, n_mel, T), energy (B, T), n_frames) as NumPy, T = the longest frame count + extra; NaN
        stands past n[b] up to ldw = max n + pad and all over the outputs before the call '''
    H = _H()
    B, frames = len(n), [O.frame_count(k, n_fft, hop, centred) for k in n]
    ldw, T = max(n) + pad, max(frames) + extra
    wd = torch.full((B, ldw), NAN, dtype=torch.float32)
    for b, k in enumerate(n):
        wd[b, :k] = torch.as_tensor(wav[b, :k]).float()
    wd, nd = wd.to(DEV), _i64(n)
    mel = torch.full((B, n_mel, T), NAN, dtype=torch.float32, device=DEV)
    energy = torch.full((B, T), NAN, dtype=torch.float32, device=DEV)
    nfr = torch.full((B,), -1, dtype=torch.int64, device=DEV)
    tw, w = _fft_tables(n_fft, False)
    t = _mel_tables(n_fft, n_mel)
    with torch.cuda.device(DEV):
        H.check(H.lib().dx_mel_spectrogram(H.ptr(wd), ldw, H.ptr(nd), H.ptr(tw), H.ptr(w), H.ptr(t['fb']), H.ptr(t['lo']), H.ptr(t['hi']),
                                           H.ptr(mel), H.ptr(energy), H.ptr(nfr), B, T, n_fft, hop, n_mel, centred, min_clip, H.stream()))
        torch.cuda.synchronize()
    return mel.cpu().numpy(), energy.cpu().numpy(), nfr.cpu().tolist()


def _front_end_checks(what, mel, energy, nfr, oracles, frames):
    checks = []
    assert nfr == frames, (what, nfr, frames)
    for b, f in enumerate(frames):
        assert (mel[b, :, f:] == 0).all() and (energy[b, f:] == 0).all(), (what, b)              # exact zeros over NaN
        (mel64, en64), (mel32, en32) = oracles[b]
        assert mel64.shape[1] == f
        checks += [(f'{what} b {b} log-mel', mel[b, :, :f], mel64, mel32), (f'{what} b {b} energy', energy[b, :f], en64, en32)]
    _gather(checks)


@functools.lru_cache(maxsize=None)
def _front_end_oracles(name, n_mel):
    n_fft, hop, centred, n, wav = O.frontend_inputs(name)
    return [tuple(O.mel_frontend(wav[b], k, n_fft, hop, n_mel, centred, dtype=dt) for dt in (F64, F32)) for b, k in enumerate(n)]


@pytest.mark.parametrize('n_mel', O.N_MELS)
@pytest.mark.parametrize('name', list(O.FRONTEND_CASES))
def test_front_end(name, n_mel):
    n_fft, hop, centred, n, wav = O.frontend_inputs(name)
    frames = [O.frame_count(k, n_fft, hop, centred) for k in n]
    mel, energy, nfr = _front_end(n_fft, hop, centred, n_mel, n, wav)
    _front_end_checks(f'{name} n_mel {n_mel}', mel, energy, nfr, _front_end_oracles(name, n_mel), frames)


@pytest.mark.parametrize('n_mel', O.N_MELS)
@pytest.mark.parametrize('n_fft', O.SIZES)
def test_front_end_tones(n_fft, n_mel):
    ''' silence (|X| = sqrt(1e-9) everywhere), a tone that clips no channel, a quiet one whose upper channels are all clipped '''
    hop, n, wav = O.tone_inputs(n_fft)
    oracles = [tuple(O.mel_frontend(wav[b], k, n_fft, hop, n_mel, 1, dtype=dt) for dt in (F64, F32)) for b, k in enumerate(n)]
    mel, energy, nfr = _front_end(n_fft, hop, 1, n_mel, n, wav)
    _front_end_checks(f'tones {n_fft} n_mel {n_mel}', mel, energy, nfr, oracles, [4, 4, 4])
    A = O.filterbank(n_fft, n_mel).astype(F64)
    want = np.log(np.maximum(A.sum(1) * np.sqrt(1e-9), F64(F32(O.MIN_CLIP))))                   # the closed form of silence
    _check(f'tones {n_fft} n_mel {n_mel} silence, closed form', mel[0, :, :4], np.repeat(want[:, None], 4, 1), oracles[0][1][0])
    if n_mel >= 64:                                                                              # clipped: log(min_clip), the bits of
        assert (mel[2, -10:, :4] == mel[0, -1, 0]).all()                                         # silence's top channel


@pytest.mark.parametrize('name', ['256-64-c1', '256-64-c0', '4096-1024-c1'])
def test_front_end_wrapper(name):
    ''' `mel_spectrogram_batch` at a size that is not the default's, on ITS tables (`fft_tables`, `mel_tables`), beside the direct call
        on the oracle's '''
    from daft_exprt import extract_features as fe
    n_fft, hop, centred, n, wav = O.frontend_inputs(name)
    n_mel = 65
    hp = make_hparams(filter_length=n_fft, hop_length=hop, n_mel_channels=n_mel, centered=bool(centred))
    frames = [O.frame_count(k, n_fft, hop, centred) for k in n]
    wd = torch.zeros((len(n), max(n)), dtype=torch.float32)
    for b, k in enumerate(n):
        wd[b, :k] = torch.as_tensor(wav[b, :k]).float()
        wd[b, k:] = NAN
    with torch.cuda.device(DEV):
        mel, energy, nfr = fe.mel_spectrogram_batch(wd.to(DEV), _i64(n), hp)
        torch.cuda.synchronize()
    mel, energy = mel.cpu().numpy(), energy.cpu().numpy()
    assert mel.shape == (len(n), n_mel, max(1, O.frame_count(max(n), n_fft, hop, centred)))
    oracles = _front_end_oracles(name, n_mel)
    _front_end_checks(f'wrapper {name}', mel, energy, nfr.cpu().tolist(), oracles, frames)
    direct = _front_end(n_fft, hop, centred, n_mel, n, wav)
    for b, f in enumerate(frames):                                            # the two table sets differ by an ulp at the most
        (mel64, en64), (mel32, en32) = oracles[b]
        for what, a, d, o64, o32 in (('log-mel', mel[b, :, :f], direct[0][b, :, :f], mel64, mel32),
                                     ('energy', energy[b, :f], direct[1][b, :f], en64, en32)):
            tol = O.bound(o64, o32)[2]
            diff = float(np.abs(a.astype(F64) - d).max()) if a.size else 0.
            print(f'wrapper {name} b {b} {what}: wrapper - direct {diff:.3g}, bound {tol:.3g}')
            assert diff <= tol
    if centred:
        with pytest.raises(ValueError, match='reflect padding'):
            fe.mel_spectrogram_batch(wd.to(DEV), _i64([n_fft // 2] + list(n[1:])), hp)


# ---- NNLS ------------------------------------------------------------------------------------------------------------------------

def _mel_to_linear(n_fft, n_mel, iters, is_log, lengths, mel, layout):
    ''' -> (linear (B, bins, T) NumPy, the padding of the output: must still be NaN) '''
    H = _H()
    B, T, bins = len(lengths), O.NNLS_T, n_fft // 2 + 1
    md = torch.full((B, n_mel, T), NAN, dtype=torch.float32)
    for b, L in enumerate(lengths):
        md[b, :, :L] = torch.as_tensor(mel[b, :, :L]).float()
    md, ld = md.to(DEV), _i64(lengths)
    if layout == 'frame-major':                                      # (B, T, bins) as the wrapper's, two more frames per utterance
        lin = torch.full((B, T + 2, bins), NAN, dtype=torch.float32, device=DEV)
        strides, live, pad = ((T + 2) * bins, 1, bins), lin[:, :T].transpose(1, 2), lin[:, T:]
    else:                                                            # (B, bins, T), three more rows per utterance
        lin = torch.full((B, bins + 3, T), NAN, dtype=torch.float32, device=DEV)
        strides, live, pad = ((bins + 3) * T, T, 1), lin[:, :bins], lin[:, bins:]
    t = _mel_tables(n_fft, n_mel)
    with torch.cuda.device(DEV):
        H.check(H.lib().dx_mel_to_linear(H.ptr(md), H.ptr(ld), H.ptr(t['fb']), H.ptr(t['lo']), H.ptr(t['hi']), H.ptr(t['pinv_t']),
                                         H.ptr(t['bin_m']), H.ptr(t['bin_w']), H.ptr(lin), *strides, B, T, n_mel, n_fft, iters, t['step'],
                                         is_log, H.stream()))
        torch.cuda.synchronize()
    return live.cpu().numpy(), pad.cpu().numpy()


@pytest.mark.parametrize('iters', O.NNLS_ITERS)
@pytest.mark.parametrize('n_fft,n_mel,is_log', [(*k, 0) for k in O.NNLS_CASES] + [(*k, 1) for k in O.NNLS_LOG_PAIRS])
def test_mel_to_linear(n_fft, n_mel, iters, is_log):
    ''' log-mel input where exp()'s last bit is not amplified past the rule (audio_fft_oracle.NNLS_LOG_PAIRS), linear input at every pair '''
    A, t = O.case_tables(n_fft, n_mel)
    lengths, mel = O.nnls_inputs(n_fft, n_mel, is_log)
    oracles = [tuple(O.mel_to_linear(mel[b, :, :L], A, iters, t['step'], is_log, dt, t['pinv_t']) for dt in (F64, F32))
               for b, L in enumerate(lengths)]
    outs, checks = {}, []
    for layout in ('frame-major', 'bin-major'):
        lin, pad = _mel_to_linear(n_fft, n_mel, iters, is_log, lengths, mel, layout)
        assert pad.size and np.isnan(pad).all(), layout                                          # the padding is not written
        for b, L in enumerate(lengths):
            assert (lin[b, :, L:] == 0).all(), (layout, b)                                       # frames past the utterance: exact zeros
            if L:
                checks.append((f'nnls {n_fft} n_mel {n_mel} iters {iters} log {is_log} {layout} b {b}', lin[b, :, :L], *oracles[b]))
        outs[layout] = lin
    _gather(checks)
    assert np.array_equal(outs['frame-major'], outs['bin-major'])
    assert (outs['bin-major'] >= 0).all()


@pytest.mark.parametrize('n_fft,n_mel', [(256, 80), (1024, 80), (4096, 80), (256, 256), (1024, 1)])
def test_nnls_tables_of_the_wrapper(n_fft, n_mel):
    ''' `mel_tables` and `_nnls_tables` against the oracle's: integers exactly, floats within one ulp '''
    from daft_exprt import griffin_lim as G
    from daft_exprt.extract_features import mel_tables
    hp = make_hparams(filter_length=n_fft, hop_length=n_fft // 4, n_mel_channels=n_mel)
    A, t = O.case_tables(n_fft, n_mel)
    fb, lo, hi = (a.cpu().numpy() for a in mel_tables(hp, torch.device(DEV)))
    pinv_t, bin_m, bin_w, step = G._nnls_tables(hp, torch.device(DEV))
    pinv_t, bin_m, bin_w = pinv_t.cpu().numpy(), bin_m.cpu().numpy(), bin_w.cpu().numpy()
    assert np.array_equal(lo, t['lo']) and np.array_equal(hi, t['hi']) and np.array_equal(bin_m, t['bin_m'])
    assert lo.dtype == np.int32 and hi.dtype == np.int32 and bin_m.dtype == np.int32
    ulps = {'fb': O.ulps32(fb, A), 'pinv_t': O.ulps32(pinv_t, t['pinv_t']), 'bin_w': O.ulps32(bin_w, t['bin_w'])}
    print(f'n_fft {n_fft} n_mel {n_mel}: {ulps}, step {step!r} vs {t["step"]!r}')
    assert fb.shape == A.shape and pinv_t.shape == t['pinv_t'].shape and bin_w.shape == t['bin_w'].shape
    assert max(ulps.values()) <= 1. and abs(step - t['step']) <= np.spacing(t['step'])


# ---- Griffin-Lim -----------------------------------------------------------------------------------------------------------------

def _griffin_lim(n_fft, hop, lengths, mag, x0, iterations, T=O.GL_T, frame_major=False, pad=(5, 11)):
    ''' mag (B, bins, >= T), x0 (B, >= S) on the CPU -> (wav (B, ldw) NumPy, n_samples).  NaN: mag at the frames >= lengths[b] - 2, x0 past
        n_samples[b] up to ldx0 = S + pad[0], all of wav (ldw = S + pad[1]) and of the workspace '''
    H = _H()
    B, bins, S = len(lengths), n_fft // 2 + 1, GO.n_samples(T, n_fft, hop)
    ldx0, ldw = S + pad[0], S + pad[1]
    md = torch.full((B, T, bins) if frame_major else (B, bins, T), NAN, dtype=torch.float32)
    xd = torch.full((B, ldx0), NAN, dtype=torch.float32)
    for b, L in enumerate(lengths):
        F, Sb = GO.n_frames(L), GO.n_samples(L, n_fft, hop)
        live = torch.as_tensor(mag[b, :, :F]).float()
        if frame_major:
            md[b, :F] = live.t()
        else:
            md[b, :, :F] = live
        xd[b, :Sb] = torch.as_tensor(x0[b, :Sb]).float()
    md, xd, ld = md.to(DEV), xd.to(DEV), _i64(lengths)
    strides = (T * bins, 1, bins) if frame_major else (bins * T, T, 1)
    wav = torch.full((B, ldw), NAN, dtype=torch.float32, device=DEV)
    ws = torch.full((max(int(H.lib().dx_gl_ws_floats(B, T, n_fft)), 1),), NAN, dtype=torch.float32, device=DEV)
    n_out = torch.full((B,), -1, dtype=torch.int64, device=DEV)
    tw, w = _fft_tables(n_fft, True)
    with torch.cuda.device(DEV):
        H.check(H.lib().dx_griffin_lim(H.ptr(md), *strides, H.ptr(ld), H.ptr(xd), ldx0, H.ptr(tw), H.ptr(w), H.ptr(wav), ldw, H.ptr(n_out),
                                       H.ptr(ws), B, T, n_fft, hop, iterations, 0, H.stream()))
        torch.cuda.synchronize()
    return wav.cpu().numpy(), n_out.cpu().tolist()


def _griffin_lim_checks(what, wav, n_out, n_fft, hop, lengths, o64, o32, S):
    checks = []
    assert n_out == [GO.n_samples(L, n_fft, hop) for L in lengths], (what, n_out)
    for b, Sb in enumerate(n_out):
        assert (wav[b, Sb:S] == 0).all() and np.isnan(wav[b, S:]).all() and wav.shape[1] > S, (what, b)
        checks.append((f'{what} b {b}', wav[b, :Sb], o64[b], o32[b]))                              # per sample
        if GO.n_frames(lengths[b]) == 0:
            assert (wav[b, :Sb] == 0).all(), (what, b)
    _gather(checks)


@functools.lru_cache(maxsize=None)
def _gl_oracles(name, iterations):
    return O.gl_oracle(name, iterations, F64), O.gl_oracle(name, iterations, F32)


@pytest.mark.parametrize('iterations', (1, 2))
@pytest.mark.parametrize('name', list(O.GL_CASES))
def test_griffin_lim(name, iterations):
    ''' frame counts 5, 2, 1, 0, 0: an odd count's last workgroup has no second frame; the second iteration reads wav in place; the
        magnitude bin-major after one iteration, frame-major (the wrapper's strides) after two '''
    n_fft, hop, lengths, mag, x0 = O.gl_inputs(name)
    wav, n_out = _griffin_lim(n_fft, hop, lengths, mag, x0, iterations, frame_major=iterations == 2)
    _griffin_lim_checks(f'griffin-lim {name} iterations {iterations}', wav, n_out, n_fft, hop, lengths, *_gl_oracles(name, iterations),
                        GO.n_samples(O.GL_T, n_fft, hop))


@pytest.mark.parametrize('n_fft', O.SIZES)
def test_griffin_lim_from_silence(n_fft):
    ''' x0 = 0: R = 0 in every bin, phase 0 as np.angle(0): the overlap-add of w irfft(S) '''
    name, kw = f'{n_fft}-{n_fft // 4}', dict(lengths=O.GL_ZERO_LENGTHS, zero_first=True)
    n_fft, hop, lengths, mag, x0 = O.gl_inputs(name, **kw)
    assert not x0[0].any() and x0[1].any()
    wav, n_out = _griffin_lim(n_fft, hop, lengths, mag, x0, 1)
    _griffin_lim_checks(f'griffin-lim {name} from silence', wav, n_out, n_fft, hop, lengths, O.gl_oracle(name, 1, F64, **kw),
                        O.gl_oracle(name, 1, F32, **kw), GO.n_samples(O.GL_T, n_fft, hop))
    assert np.abs(wav[0, :n_out[0]]).max() > 0.


@pytest.mark.parametrize('name', ['256-64', '4096-1024'])
def test_griffin_lim_alone_is_bit_equal(name):
    ''' an utterance gets the same bits alone, with T, S and both row strides its own '''
    n_fft, hop, lengths, mag, x0 = O.gl_inputs(name)
    wav, n_out = _griffin_lim(n_fft, hop, lengths, mag, x0, 2)
    for b, L in enumerate(lengths):
        if L < 1:
            continue
        alone, n1 = _griffin_lim(n_fft, hop, [L], mag[b:b + 1], x0[b:b + 1], 2, T=L, pad=(0, 0))
        assert n1 == [n_out[b]] and alone.shape == (1, n_out[b]) and np.array_equal(alone[0], wav[b, :n_out[b]]), (name, b)


# ---- noise -----------------------------------------------------------------------------------------------------------------------

def test_noise():
    H = _H()
    n_fft, hop, T, lengths, seeds = O.NOISE_CASE
    B, S = len(lengths), GO.n_samples(T, n_fft, hop)
    ldx, checks, rows, ld = S + 9, [], [], _i64(lengths)
    for seed in seeds:
        x = torch.full((B, ldx), NAN, dtype=torch.float32, device=DEV)
        with torch.cuda.device(DEV):
            H.check(H.lib().dx_gl_noise(H.ptr(x), ldx, H.ptr(ld), B, T, n_fft, hop, seed, H.stream()))
            torch.cuda.synchronize()
        x = x.cpu().numpy()
        for b, L in enumerate(lengths):
            Sb = GO.n_samples(L, n_fft, hop)
            assert (x[b, Sb:S] == 0).all() and np.isnan(x[b, S:]).all(), (seed, b)
            checks.append((f'noise seed {seed} b {b}', x[b, :Sb], O.noise(seed, b, np.arange(Sb), F64), O.noise(seed, b, np.arange(Sb), F32)))
            rows.append(x[b, :n_fft])
    _gather(checks)
    assert all(not np.array_equal(a, b) for i, a in enumerate(rows) for b in rows[i + 1:])


# ---- normalise -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', list(O.NORMALISE_CASES))
def test_normalise(name):
    H = _H()
    n_fft, hop, T, lengths, x = O.normalise_inputs(name)
    B, S = x.shape
    ldw = S + 6
    n = [GO.n_samples(L, n_fft, hop) for L in lengths]
    xd = torch.full((B, ldw), NAN, dtype=torch.float32)
    for b, Sb in enumerate(n):
        xd[b, :Sb] = torch.as_tensor(x[b, :Sb]).float()
        xd[b, Sb:S] = O.HUGE * (-1.) ** b                             # finite: fmaxf would keep it, where it drops a NaN
    assert all(Sb < S for Sb in n)
    xd, ld = xd.to(DEV), _i64(lengths)
    with torch.cuda.device(DEV):
        H.check(H.lib().dx_gl_normalise(H.ptr(xd), ldw, H.ptr(ld), B, T, n_fft, hop, H.stream()))
        torch.cuda.synchronize()
    y = xd.cpu().numpy()
    for b, Sb in enumerate(n):
        assert (y[b, Sb:S] == 0).all() and np.isnan(y[b, S:]).all(), b
        want = O.normalise(x[b, :Sb]) if GO.n_frames(lengths[b]) > 0 else np.zeros(Sb)
        ulp = O.ulps32(y[b, :Sb], want)
        print(f'normalise {name} b {b}: {ulp:.3g} ulp, max |y| {float(np.abs(y[b, :Sb]).max()):.9g}')
        assert np.isfinite(y[b, :Sb]).all() and ulp <= 1., (name, b, ulp)
    assert np.abs(y[0, :n[0]]).max() == 1. == abs(y[0, 0]) and abs(y[1, n[1] - 1]) == 1.
    assert not y[2, :S].any() and not y[3, :S].any()
