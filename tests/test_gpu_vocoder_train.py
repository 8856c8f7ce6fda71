"""Vocoder fine-tuning on the GPU (K33: csrc/vocoder_train.hip, daft_exprt/vocoder_train.py) against tests/vocoder_grad_oracle.py --
float64 autograd through tests/vocoder_oracle.py, pinned in tests/test_vocoder_train_host.py -- and never against the code under test.

Tolerances are the two rules of tests/test_gpu_vocoder.py, applied PER GRADIENT TENSOR, with the floors scaled by m = max |oracle64|
of that tensor (a gradient has no full scale of 1):
    fp32   max |g - o64| <= max(8 x max |o32 - o64|, 2e-6 m), o32 the float32 CPU run of the same oracle
    bf16   max |g - o_rounded| <= max(2 d_round, 2e-3 m), d_round = max |o_rounded - o64|
Every test prints the measured values.  Rows (257, 3, 1): the 257-row utterance needs a second 64-row item and a second 256-row
forward tile; NaN stands at every row at or past n[b] of every operand handed to a kernel."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import vocoder_grad_oracle as G
from tests import vocoder_oracle as O
from tests.test_vocoder_train_host import _write_wav

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = (257, 3, 1)
DTYPES = ['fp32', 'bf16']
T1 = {'resblock': '1', 'upsample_rates': [4, 2], 'upsample_kernel_sizes': [8, 4], 'upsample_initial_channel': 128,
      'resblock_kernel_sizes': [3, 7], 'resblock_dilation_sizes': [[1, 3], [1, 3, 5]], 'num_mels': 80, 'hop_size': 8,
      'sampling_rate': 22050}
T2 = {'resblock': '2', 'upsample_rates': [3, 2], 'upsample_kernel_sizes': [7, 4], 'upsample_initial_channel': 128,
      'resblock_kernel_sizes': [3, 5], 'resblock_dilation_sizes': [[1, 2], [2, 6]], 'num_mels': 80, 'hop_size': 6,
      'sampling_rate': 22050}
CONFIGS = {'T1': T1, 'T2': T2}
LENGTHS = (23, 9, 1)


def _bound(g, o64, o32, orr, dtype, what):
    ''' asserts the module's tolerance rule on one gradient tensor (CPU tensors of one shape) '''
    g, o64 = g.detach().double().cpu(), o64.double()
    assert g.shape == o64.shape, (what, g.shape, o64.shape)
    assert bool(torch.isfinite(g).all()), what
    m = float(o64.abs().max())
    if dtype == 'fp32':
        cost = float((o32.double() - o64).abs().max())
        err, tol = float((g - o64).abs().max()), max(8. * cost, 2e-6 * m)
        print(f'{what} fp32: err {err:.3g}, fp32 oracle cost {cost:.3g}, m {m:.3g}, bound {tol:.3g}')
    else:
        d_round = float((orr.double() - o64).abs().max())
        err, tol = float((g - orr.double()).abs().max()), max(2. * d_round, 2e-3 * m)
        print(f'{what} bf16: err vs rounded oracle {err:.3g}, d_round {d_round:.3g}, m {m:.3g}, bound {tol:.3g}')
    assert err <= tol, (what, dtype, err, tol)


def _three(fn):
    ''' (oracle64, oracle32, oracle_rounded) of fn(dtype, rounding) '''
    return fn(torch.float64, False), fn(torch.float32, False), fn(torch.float64, True)


def _rows_major(x, n, u=1):
    ''' (B, C, T) CPU -> (B, T, C) fp32 on the device, NaN at the rows at or past n[b] * u: they must not be read '''
    x = x.float().transpose(1, 2).contiguous()
    for b, rows in enumerate(n):
        x[b, rows * u:] = float('nan')
    return x.to(DEV)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- the weight gradient, the re-packed data gradient, the gate and the bias gradient of one layer ---------------------------------

def _conv_layer(cin, cout, k, d, rows, dtype, seed, slope=0.1):
    from daft_exprt import vocoder as V
    from daft_exprt import vocoder_train as VT
    B, N, n = len(rows), max(rows), torch.tensor(rows)
    g = _gen(seed)
    x = O.mask_rows(torch.randn((B, cin, N), generator=g), n)
    dy = torch.randn((B, cout, N), generator=g)
    w = torch.randn((cout, cin, k), generator=g) / (cin * k) ** 0.5
    bias = 0.1 * torch.randn((cout,), generator=g)
    (dx64, dw64, db64), (dx32, dw32, db32), (dxr, dwr, dbr) = _three(
        lambda dt, rounding: G.conv_grads(x, w, bias, d, n, dy, slope=slope, rounding=rounding, dtype=dt))
    xd, dyd, nd = _rows_major(x, rows), _rows_major(dy, rows), n.to(DEV)
    what = f'conv {cin}->{cout} k{k} d{d} rows {rows}'
    dw = VT.conv_wgrad(xd, dyd, nd, k, d, slope, dtype)
    assert dw.shape == (k, cout, cin)
    _bound(dw.permute(1, 2, 0), dw64, dw32, dwr, dtype, f'{what}: dW')
    assert torch.equal(dw, VT.conv_wgrad(xd, dyd, nd, k, d, slope, dtype))                      # no atomics: the same bits
    wd = V.pack_conv_dgrad_weight(w.double(), VT._TDT[dtype]).to(DEV)
    pre = VT.conv_forward(dyd, wd, None, nd, cin, k, d, 1., dtype)
    dx = VT._gate(xd, pre, slope)
    dx64, dx32, dxr = (O.mask_rows(t, n) for t in (dx64, dx32, dxr))         # x is a masked layer output: no gradient past its end
    _bound(dx.transpose(1, 2), dx64, dx32, dxr, dtype, f'{what}: dx')
    for b, r in enumerate(rows):
        assert float(dx[b, r:].abs().max() if r < N else 0.) == 0.                               # dead rows: exact zeros, NaN in x or not
    db = VT._bias_grad(dyd, VT._live(nd, N, DEV))
    _bound(db, db64, db32, db64, 'fp32', f'{what}: db')                                         # never rounded


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('cin,cout', [(32, 32), (64, 32), (96, 64)])
def test_conv_gradients_alone(cin, cout, dtype):
    for k in (3, 7, 11):
        for d in (1, 3, 5):
            _conv_layer(cin, cout, k, d, ROWS, dtype, seed=cin * 100 + cout + k * 7 + d)


@pytest.mark.parametrize('dtype', DTYPES)
def test_conv_gradients_with_several_row_chunks(dtype):
    ''' 1100 rows are 18 items of 64: more than one partial tile per output tile and utterance, several items per workgroup '''
    from daft_exprt import _hip as H
    one_part = 4 * 3 * 32 * 32
    assert H.lib().dx_vocoder_wgrad_workspace(2, 1100, 32, 32, 3, 1) >= 2 * 2 * one_part
    _conv_layer(32, 32, 3, 1, (1100, 70), dtype, seed=11)
    _conv_layer(64, 64, 7, 3, (1100, 70), dtype, seed=12)


def _asym_ints(B, N, cin, cout, u=1):
    t, c, o = torch.arange(N), torch.arange(cin), torch.arange(cout)
    x = (((3 * t[None, :] + 5 * c[:, None]) % 7) - 3).double()[None].repeat(B, 1, 1) + torch.arange(B).double()[:, None, None]
    r = torch.arange(N * u)
    dy = (((2 * r[None, :] + 3 * o[:, None]) % 5) - 2).double()[None].repeat(B, 1, 1) - torch.arange(B).double()[:, None, None]
    return x, dy


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('cin,cout,k,d', [(96, 64, 3, 3), (64, 32, 11, 5), (32, 32, 7, 1)])
def test_wgrad_lane_maps_with_asymmetric_integers(cin, cout, k, d, dtype):
    ''' small integers are exact in bf16 and their sums exact in fp32: any lane, tap or channel mix-up changes the result '''
    from daft_exprt import vocoder_train as VT
    B, N, n = len(ROWS), max(ROWS), torch.tensor(ROWS)
    x, dy = _asym_ints(B, N, cin, cout)
    x = O.mask_rows(x, n)
    _, want, _ = G.conv_grads(x, torch.zeros((cout, cin, k)), torch.zeros(cout), d, n, dy, slope=1.)
    dw = VT.conv_wgrad(_rows_major(x, ROWS), _rows_major(dy, ROWS), n.to(DEV), k, d, 1., dtype)
    assert torch.equal(dw.permute(1, 2, 0).double().cpu(), want)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('u,k', [(8, 16), (2, 4), (4, 8), (3, 7)])
def test_upsample_gradients_alone(u, k, dtype):
    from daft_exprt import vocoder as V
    from daft_exprt import vocoder_train as VT
    cin, cout, slope = 64, 32, 0.1
    B, N, n = len(ROWS), max(ROWS), torch.tensor(ROWS)
    g = _gen(u * 1000 + k)
    x = O.mask_rows(torch.randn((B, cin, N), generator=g), n)
    dy = torch.randn((B, cout, N * u), generator=g)
    w = torch.randn((cin, cout, k), generator=g) / (cin * k / u) ** 0.5
    bias = 0.1 * torch.randn((cout,), generator=g)
    (dx64, dw64, db64), (dx32, dw32, db32), (dxr, dwr, _) = _three(
        lambda dt, rounding: G.upsample_grads(x, w, bias, u, n, dy, slope=slope, rounding=rounding, dtype=dt))
    xd, dyd, nd = _rows_major(x, ROWS), _rows_major(dy, ROWS, u), n.to(DEV)
    what = f'upsample {cin}->{cout} u{u} k{k}'
    j, entry = V.upsample_tap_table(k, u)
    raw = VT.upsample_wgrad(xd, dyd, nd, k, u, slope, dtype)
    assert raw.shape == (u, -(-k // u), cout, cin)
    assert float(raw[(j < 0).to(DEV)].abs().max() if bool((j < 0).any()) else 0.) == 0.          # entries whose tap j >= k: zeros
    dw = raw.permute(3, 2, 0, 1).reshape(cin, cout, -1)[:, :, entry.to(DEV)]
    _bound(dw, dw64, dw32, dwr, dtype, f'{what}: dW')
    assert torch.equal(raw, VT.upsample_wgrad(xd, dyd, nd, k, u, slope, dtype))
    pre = VT.upsample_dgrad(dyd, V.pack_upsample_dgrad_weight(w.double(), u, VT._TDT[dtype]).to(DEV), nd, cin, u, dtype)
    dx = VT._gate(xd, pre, slope)
    dx64, dx32, dxr = (O.mask_rows(t, n) for t in (dx64, dx32, dxr))         # x is a masked layer output: no gradient past its end
    _bound(dx.transpose(1, 2), dx64, dx32, dxr, dtype, f'{what}: dx')
    for b, r in enumerate(ROWS):
        assert float(dx[b, r:].abs().max() if r < N else 0.) == 0.
    _bound(VT._bias_grad(dyd, VT._live(nd * u, N * u, DEV)), db64, db32, db64, 'fp32', f'{what}: db')
    # integers: every phase contracts its own rows of dy with its own rows of x
    xi, dyi = _asym_ints(B, N, cin, cout, u)
    xi = O.mask_rows(xi, n)
    _, want, _ = G.upsample_grads(xi, torch.zeros((cin, cout, k)), torch.zeros(cout), u, n, dyi, slope=1.)
    raw = VT.upsample_wgrad(_rows_major(xi, ROWS), _rows_major(dyi, ROWS, u), nd, k, u, 1., dtype)
    assert torch.equal(raw.permute(3, 2, 0, 1).reshape(cin, cout, -1)[:, :, entry.to(DEV)].double().cpu(), want)


def test_unsupported_shapes_are_refused():
    from daft_exprt import vocoder_train as VT
    n = torch.tensor([8], device=DEV)
    x16, x32 = torch.zeros((1, 8, 16), device=DEV), torch.zeros((1, 8, 32), device=DEV)
    with pytest.raises(RuntimeError, match='multiples of 32'):
        VT.conv_wgrad(x16, x16, n, 3, 1, 0.1, 'fp32')
    with pytest.raises(RuntimeError, match='span 70 rows'):
        VT.conv_wgrad(x32, x32, n, 15, 5, 0.1, 'fp32')


# ---- the whole generator ----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _case(name):
    ''' (cfg, mel with random values past the lengths, weight-norm state dict, projection, the three oracles), computed once;
        an oracle is (waveform, {parameter: gradient}, mel gradient) '''
    cfg = CONFIGS[name]
    mel = O.make_mel(cfg, LENGTHS, seed=5)
    sd = O.state_dict(O.make_weights(cfg, mel, LENGTHS, seed=5), 'weight_norm', seed=5)
    proj = torch.randn((len(LENGTHS), max(LENGTHS) * cfg['hop_size']), generator=_gen(6))
    n = torch.tensor(LENGTHS)
    oracles = _three(lambda dt, rounding: G.generator_grads(cfg, sd, mel, n, proj, rounding=rounding, dtype=dt))
    return cfg, mel, sd, proj, oracles


@functools.lru_cache(maxsize=None)
def _generator(name, dtype):
    from daft_exprt.vocoder_train import TrainableGenerator
    cfg, _, sd, _, _ = _case(name)
    return TrainableGenerator(cfg, sd, compute_dtype=dtype).to(DEV)


def _backward(gen, mel, lengths, proj):
    ''' (waveform, {parameter: gradient}, mel gradient) of sum(gen(mel) * proj) '''
    mel = mel.to(DEV).requires_grad_(True)
    wav = gen(mel, torch.tensor(lengths, device=DEV))
    names, params = zip(*gen.named_parameters())
    grads = torch.autograd.grad((wav * proj.to(DEV)).sum(), list(params) + [mel])
    return wav.detach(), dict(zip(names, grads[:-1])), grads[-1]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', list(CONFIGS))
def test_generator_gradients_match_the_oracle(name, dtype):
    ''' the waveform, the gradient of EVERY parameter and of the mel.  Measured on the MI355X: every tensor of T1 and T2 in both modes
        is inside its bound except, on some machines, one -- [T2-fp32] then fails on the scalar d conv_post.weight_g: err 3.06e-05
        against a bound of 1.93e-05 = 2e-6 m (m 9.66).  For a one-element tensor max |o32 - o64| is a single draw of the float32 CPU
        oracle's rounding: 6.8e-08 where it was printed on a GPU machine (the floor decides: missed, four runs), 7.6e-06 on another
        CPU (6.8e-06 .. 2.5e-05 over five other projections), and in the one run of the whole GPU suite the case passed.  The gradient divides the fp32
        forward's error in conv_post's pre-activation (1.1e-06, the float32 oracle's 1.2e-06) by g = 0.18; taking conv_post's sums
        and weight norm in float64 did not move it (2.96e-05 before).  The bound stays as set. '''
    cfg, mel, sd, proj, ((w64, g64, m64), (w32, g32, m32), (wr, gr, mr)) = _case(name)
    wav, grads, dmel = _backward(_generator(name, dtype), mel, LENGTHS, proj)
    _bound(wav, w64, w32, wr, dtype, f'{name} waveform')
    assert sorted(grads) == sorted(sd)
    missed = []
    for key in sd:                                                          # weight_g, weight_v and bias of every layer
        assert grads[key].shape == sd[key].shape
        try:
            _bound(grads[key], g64[key], g32[key], gr[key], dtype, f'{name} d {key}')
        except AssertionError as e:                                         # every tensor is measured before the test fails
            missed.append(e.args[0])
    _bound(dmel, m64, m32, mr, dtype, f'{name} d mel')
    assert not missed, missed
    for b, t in enumerate(LENGTHS):
        assert float(dmel[b, :, t:].abs().max() if t < max(LENGTHS) else 0.) == 0.


@pytest.mark.parametrize('dtype', DTYPES)
def test_backward_is_bit_deterministic_and_batch_independent(dtype):
    cfg, mel, sd, proj, ((_, g64, _), (_, g32, _), _) = _case('T1')
    gen, hop = _generator('T1', dtype), cfg['hop_size']
    _, grads, dmel = _backward(gen, mel, LENGTHS, proj)
    _, again, dmel_again = _backward(gen, mel, LENGTHS, proj)
    assert torch.equal(dmel, dmel_again) and all(torch.equal(grads[k], again[k]) for k in grads)
    alone = []
    for b, t in enumerate(LENGTHS):
        _, g_b, dmel_b = _backward(gen, mel[b:b + 1, :, :t].contiguous(), LENGTHS[b:b + 1], proj[b:b + 1, :t * hop])
        assert torch.equal(dmel_b[0], dmel[b, :, :t]), (b, float((dmel_b[0] - dmel[b, :, :t]).abs().max()))
        alone.append(g_b)
    if dtype == 'fp32':                                                     # the loss is a sum over the utterances
        for key in grads:
            rest = grads[key] - alone[1][key] - alone[2][key]
            cost, m = float((g32[key].double() - g64[key]).abs().max()), float(g64[key].abs().max())
            err, tol = float((rest - alone[0][key]).abs().max()), max(8. * cost, 2e-6 * m)
            print(f'd {key}: alone against batch minus the others {err:.3g}, bound {tol:.3g}')
            assert err <= tol, (key, err, tol)


def test_a_poisoned_workspace_changes_no_bit():
    from daft_exprt import config
    from daft_exprt import vocoder_train as VT
    _, mel, _, proj, _ = _case('T2')
    gen = _generator('T2', 'fp32')
    _, clean, dmel = _backward(gen, mel, LENGTHS, proj)
    dirty = mel.clone()
    for b, t in enumerate(LENGTHS):
        dirty[b, :, t:] = float('nan')
    old = config.POISON
    config.POISON = True
    try:
        VT._WS.clear()                                                      # a fresh, NaN-filled workspace
        _, got, dmel_got = _backward(gen, dirty, LENGTHS, proj)
        torch.cuda.synchronize()
    finally:
        config.POISON = old
    assert all(bool(torch.isfinite(got[k]).all()) and torch.equal(got[k], clean[k]) for k in clean)
    assert torch.equal(dmel_got, dmel)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', list(CONFIGS))
def test_forward_agrees_with_the_inference_path(name, dtype):
    ''' weight norm is folded in float32 here and in float64 there: the rule, not bits '''
    from daft_exprt.vocoder import Vocoder
    cfg, mel, _, _, ((w64, _, _), (w32, _, _), (wr, _, _)) = _case(name)
    gen = _generator(name, dtype)
    n = torch.tensor(LENGTHS, device=DEV)
    with torch.no_grad():
        wav = gen(mel.to(DEV), n)
    ref, n_samples = Vocoder(cfg, gen.state_dict(), compute_dtype=dtype, device=DEV)(mel.to(DEV), n)
    assert n_samples.tolist() == [t * cfg['hop_size'] for t in LENGTHS]
    if dtype == 'fp32':
        err, tol = float((wav - ref).abs().max()), max(8. * float((w32.double() - w64).abs().max()), 2e-6)
    else:
        err, tol = float((wav - ref).abs().max()), max(2. * float((wr - w64).abs().max()), 2e-3)
    print(f'{name} {dtype}: TrainableGenerator against Vocoder {err:.3g}, bound {tol:.3g}')
    assert err <= tol


# ---- the loss mel -------------------------------------------------------------------------------------------------------------------

MEL_CFG = {'n_fft': 1024, 'win_size': 1024, 'hop_size': 256, 'fmin': 0, 'fmax': 8000, 'fmax_for_loss': None, 'num_mels': 80,
           'sampling_rate': 22050}


def _stft_mel(wav):
    ''' HiFi-GAN's training mel by torch.stft on the CPU, in wav's dtype '''
    from daft_exprt.extract_features import mel_filter_bank
    pad = (1024 - 256) // 2
    spec = torch.stft(F.pad(wav[:, None], (pad, pad), 'reflect')[:, 0], 1024, hop_length=256, win_length=1024,
                      window=torch.hann_window(1024, dtype=wav.dtype), center=False, return_complex=True)
    mag = torch.sqrt(spec.real ** 2 + spec.imag ** 2 + 1e-9)
    fb = torch.from_numpy(mel_filter_bank(22050, 1024, 80, 0, None)).to(wav.dtype)
    return torch.log(torch.clamp(fb @ mag, min=1e-5))


def _waveforms():
    g = _gen(9)
    t = torch.arange(8192.) / 22050
    tones = torch.stack([0.4 * torch.sin(2 * np.pi * f0 * t) + 0.2 * torch.sin(2 * np.pi * 3.1 * f0 * t) for f0 in (110., 220., 523.)])
    return tones + 0.05 * torch.randn((3, 8192), generator=g)


def test_loss_mel_against_the_front_end_and_stft():
    from daft_exprt import vocoder_train as VT
    from daft_exprt.extract_features import mel_spectrogram_batch
    wav = _waveforms()
    o64, o32 = _stft_mel(wav.double()), _stft_mel(wav)
    lm = VT.LossMel(MEL_CFG).to(DEV)
    wd = wav.to(DEV).requires_grad_(True)
    got = lm(wd)
    assert got.shape == (3, 80, 32)
    _bound(got, o64, o32, None, 'fp32', 'loss mel against float64 stft')
    pad = (1024 - 256) // 2
    padded = F.pad(wav[:, None], (pad, pad), 'reflect')[:, 0].contiguous().to(DEV)
    hp = VT.front_end(MEL_CFG, centered=False)
    front, _, frames = mel_spectrogram_batch(padded, torch.full((3,), padded.shape[1], dtype=torch.int64, device=DEV), hp)
    assert frames.tolist() == [32] * 3
    cost, m = float((o32.double() - o64).abs().max()), float(o64.abs().max())
    err, tol = float((got.detach() - front[:, :, :32]).abs().max()), max(8. * cost, 2e-6 * m)
    print(f'loss mel against dx_mel_spectrogram: {err:.3g}, fp32 oracle cost {cost:.3g}, m {m:.3g}, bound {tol:.3g}')
    assert err <= tol
    proj = torch.randn((3, 80, 32), generator=_gen(10))

    def grad(dt):
        w = wav.to(dt).requires_grad_(True)
        return torch.autograd.grad((_stft_mel(w) * proj.to(dt)).sum(), w)[0]
    dwav, = torch.autograd.grad((got * proj.to(DEV)).sum(), wd)
    _bound(dwav, grad(torch.float64), grad(torch.float32), None, 'fp32', 'loss mel: waveform gradient')


# ---- training -------------------------------------------------------------------------------------------------------------------

# the smallest generator whose stages are all multiples of 32 channels and whose rates multiply to the front end's hop of 256
TRAIN_CFG = {'resblock': '1', 'upsample_rates': [16, 16], 'upsample_kernel_sizes': [32, 32], 'upsample_initial_channel': 128,
             'resblock_kernel_sizes': [3], 'resblock_dilation_sizes': [[1, 3]], 'num_mels': 80, 'hop_size': 256, 'sampling_rate': 22050,
             'n_fft': 1024, 'win_size': 1024, 'fmin': 0, 'fmax': 8000, 'fmax_for_loss': None}
TRAIN_STEPS, TRAIN_SEED, SEGMENT = 20, 1234, 2048
# `cpu_reference()` below, run on the CPU: the float32 oracle generator with the same discriminators, losses, optimiser, seed and
# segments lowers the mel L1 of the fixed batch from 5.8203 to 1.6419 in TRAIN_STEPS steps
CPU_REFERENCE_DROP = 4.1785


def _device_mel(audio):
    from daft_exprt import vocoder_train as VT
    from daft_exprt.extract_features import mel_spectrogram_batch
    w = torch.from_numpy(audio)[None].to(DEV)
    mel, _, frames = mel_spectrogram_batch(w, torch.tensor([w.shape[1]], device=DEV), VT.front_end(TRAIN_CFG))
    return mel[0, :, :int(frames[0])].cpu().numpy()


def _cpu_mel(audio):
    ''' the front end's centred mel by torch.stft in float64 (for `cpu_reference`, where there is no device) '''
    from daft_exprt.extract_features import mel_filter_bank
    spec = torch.stft(torch.from_numpy(audio).double(), 1024, hop_length=256, win_length=1024,
                      window=torch.hann_window(1024, dtype=torch.float64), center=True, pad_mode='reflect', return_complex=True)
    mag = torch.sqrt(spec.real ** 2 + spec.imag ** 2 + 1e-9)
    fb = torch.from_numpy(mel_filter_bank(22050, 1024, 80, 0, None)).double()
    return torch.log(torch.clamp(fb @ mag, min=1e-5)).float().numpy()


def _fabricate(root, mel_of):
    ''' 8 utterances in `fine_tune`'s layout: a few harmonics with a slow pitch glide, their mels from `mel_of` '''
    os.makedirs(os.path.join(root, 'spk'), exist_ok=True)
    for u in range(8):
        n = 6144 + 512 * u
        t = np.arange(n) / 22050.
        phase = 2 * np.pi * np.cumsum((110. + 30. * u) * (1. + 0.3 * t / t[-1])) / 22050.
        wav = sum(a * np.sin(h * phase) for h, a in ((1, 0.3), (2, 0.15), (3, 0.1), (5, 0.05)))
        pcm = np.round(wav * 32767.).astype(np.int16)
        _write_wav(os.path.join(root, 'spk', f'utt{u}.wav'), pcm)
        np.save(os.path.join(root, 'spk', f'utt{u}.npy'), mel_of(pcm.astype(np.float32) / np.float32(32768.)))
    return root


def _pretrained():
    mel = O.make_mel(TRAIN_CFG, (8,), seed=21)
    return O.state_dict(O.make_weights(TRAIN_CFG, mel, (8,), seed=21), 'weight_norm', seed=21)


def _fixed_batch(root):
    ''' the first segment of the first two training utterances: (mel (2, 80, 8), audio (2, 2048)) '''
    from daft_exprt import vocoder_train as VT
    train, _, _ = VT.read_data_set(root, TRAIN_CFG, SEGMENT, validation_fraction=4)
    return (torch.stack([torch.from_numpy(m[:, :8]) for _, m, _ in train[:2]]),
            torch.stack([torch.from_numpy(a[:SEGMENT]) for _, _, a in train[:2]]))


def _fixed_mel_l1(generate, root, device):
    from daft_exprt import vocoder_train as VT
    mel, audio = (t.to(device) for t in _fixed_batch(root))
    lm = VT.LossMel(TRAIN_CFG).to(device)
    with torch.no_grad():
        return float(VT.mel_l1(lm(audio), lm(generate(mel, torch.full((2,), 8, dtype=torch.int64, device=device)))))


def cpu_reference(steps=TRAIN_STEPS):
    ''' (mel L1 of the fixed batch before, after) `steps` steps of the float32 oracle generator on the CPU; where
        CPU_REFERENCE_DROP comes from:  python -c "import tests.conftest; from tests.test_gpu_vocoder_train import cpu_reference; print(cpu_reference())" '''
    import tempfile
    from daft_exprt import vocoder_train as VT
    with tempfile.TemporaryDirectory() as tmp:
        root = _fabricate(os.path.join(tmp, 'fine_tuning_dataset'), _cpu_mel)
        torch.manual_seed(TRAIN_SEED)
        params = {k: v.clone().float().requires_grad_(True) for k, v in _pretrained().items()}

        def generate(mel, lengths):
            weights = {name: (G.normed(params[f'{name}.weight_g'], params[f'{name}.weight_v']), params[f'{name}.bias'])
                       for name, _, _, _ in O.layer_shapes(TRAIN_CFG)}
            return O.generator(TRAIN_CFG, weights, mel, lengths, dtype=torch.float32)
        mpd, msd = VT.MultiPeriodDiscriminator(), VT.MultiScaleDiscriminator()
        optim_g = torch.optim.AdamW(list(params.values()), VT.LEARNING_RATE, betas=VT.ADAM_BETAS)
        optim_d = torch.optim.AdamW(list(msd.parameters()) + list(mpd.parameters()), VT.LEARNING_RATE, betas=VT.ADAM_BETAS)
        train, _, _ = VT.read_data_set(root, TRAIN_CFG, SEGMENT, validation_fraction=4)
        sampler = VT.SegmentSampler(train, 256, SEGMENT, 'cpu', TRAIN_SEED)
        loss_mel = VT.LossMel(TRAIN_CFG)
        before = _fixed_mel_l1(generate, root, 'cpu')
        for _ in range(steps):
            mel, audio = sampler.draw(2)
            VT.train_step(generate, mpd, msd, optim_g, optim_d, loss_mel, mel, audio)
        return before, _fixed_mel_l1(generate, root, 'cpu')


@pytest.fixture(scope='module')
def corpus(tmp_path_factory):
    ''' (fine-tuning data set, pretrained g_ file, config.json) '''
    base = tmp_path_factory.mktemp('vocoder_train')
    root = _fabricate(str(base / 'fine_tuning_dataset'), _device_mel)
    pre = base / 'pretrained'
    pre.mkdir()
    torch.save({'generator': _pretrained()}, str(pre / 'g_00000000'))
    (pre / 'config.json').write_text(json.dumps(TRAIN_CFG))
    return root, str(pre / 'g_00000000'), str(pre / 'config.json')


def test_training_lowers_the_mel_loss(corpus, tmp_path):
    ''' CPU_REFERENCE_DROP: the float32 CPU oracle lowers the fixed batch's mel L1 by 4.1785 (5.8203 -> 1.6419) in 20 steps; the GPU
        run must lower it by at least half of that '''
    from daft_exprt import vocoder_train as VT
    from daft_exprt.vocoder import Vocoder
    root, g_path, _ = corpus
    out = str(tmp_path / 'out')

    def l1_of(path):
        gen = VT.TrainableGenerator(TRAIN_CFG, torch.load(path, weights_only=False)['generator']).to(DEV)
        return _fixed_mel_l1(gen, root, DEV)
    before = l1_of(g_path)
    with pytest.warns(UserWarning, match='no do_ checkpoint'):
        report = VT.fine_tune_vocoder(TRAIN_CFG, root, g_path, out_dir=out, steps=TRAIN_STEPS, batch_size=2, segment_size=SEGMENT,
                                      checkpoint_interval=TRAIN_STEPS, log_interval=1, validation_fraction=4, seed=TRAIN_SEED, device=DEV)
    assert (report['utterances_used'], report['utterances_skipped'], report['utterances_held_out']) == (6, 0, 2)
    assert [e['step'] for e in report['log']] == list(range(1, TRAIN_STEPS + 1))
    assert all(np.isfinite(e[k]) for e in report['log'] for k in ('disc', 'adv', 'fm', 'mel'))
    assert np.isfinite(report['held_out_mel_l1_start']) and np.isfinite(report['held_out_mel_l1_final'])
    g_new, do_new = os.path.join(out, f'g_{TRAIN_STEPS:08d}'), os.path.join(out, f'do_{TRAIN_STEPS:08d}')
    after = l1_of(g_new)
    print(f'mel L1 of the fixed batch {before:.4f} -> {after:.4f} in {TRAIN_STEPS} steps (CPU oracle: drop {CPU_REFERENCE_DROP}); '
          f'held-out mel L1 {report["held_out_mel_l1_start"]:.4f} -> {report["held_out_mel_l1_final"]:.4f}; '
          f'{report["steps_per_second"]:.2f} steps / s')
    assert before - after >= 0.5 * CPU_REFERENCE_DROP
    voc = Vocoder.from_checkpoint(g_new, compute_dtype='fp32', device=DEV)                      # config.json beside it
    mel, _ = _fixed_batch(root)
    wav, n = voc(mel.to(DEV), torch.full((2,), 8, dtype=torch.int64, device=DEV))
    assert n.tolist() == [SEGMENT] * 2 and bool(torch.isfinite(wav).all()) and float(wav.abs().max()) > 0
    resumed = VT.fine_tune_vocoder(TRAIN_CFG, root, g_new, do_checkpoint=do_new, out_dir=out, steps=1, batch_size=2, segment_size=SEGMENT,
                                   checkpoint_interval=1, validation_fraction=4, seed=TRAIN_SEED, device=DEV)
    assert resumed['first_step'] == TRAIN_STEPS and resumed['steps'] == TRAIN_STEPS + 1
    assert os.path.isfile(os.path.join(out, f'do_{TRAIN_STEPS + 1:08d}'))


def test_train_vocoder_cli(corpus, golden_dir, tmp_path):
    from tests.test_gpu_prosody_eval import _style_bank, _tiny_model
    root, g_path, cfg_path = corpus
    out = str(tmp_path / 'voc')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'train_vocoder.py'), '-ft', root, '-cfg', cfg_path, '-g', g_path,
                        '-o', out, '--steps', '4', '--batch_size', '2', '--segment_size', str(SEGMENT), '--checkpoint_interval', '4'],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert sorted(os.listdir(out)) == ['config.json', 'do_00000004', 'g_00000004', 'vocoder_report.json']
    report = json.load(open(os.path.join(out, 'vocoder_report.json')))
    assert {'utterances_used', 'utterances_skipped', 'utterances_held_out', 'log', 'held_out_mel_l1_start', 'held_out_mel_l1_final',
            'steps_per_second', 'steps', 'generator', 'discriminators'} <= set(report)
    assert set(report['log'][-1]) == {'step', 'disc', 'adv', 'fm', 'mel', 'held_out_mel_l1'} and report['log'][-1]['step'] == 4
    assert report['log'][-1]['held_out_mel_l1'] == report['held_out_mel_l1_final'] and report['steps_per_second'] > 0
    # a data set of another hop: one line, non-zero
    bad_cfg = str(tmp_path / 'config.json')
    json.dump(dict(TRAIN_CFG, upsample_rates=[16, 8], upsample_kernel_sizes=[32, 16], hop_size=128), open(bad_cfg, 'w'))
    bad = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'train_vocoder.py'), '-ft', root, '-cfg', bad_cfg, '-g', g_path,
                          '-o', out, '--steps', '1'], capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0 and 'frames' in bad.stderr.strip().splitlines()[-1]
    # scripts/synthesize.py -voc accepts the fine-tuned generator
    model, hp = _tiny_model(golden_dir)
    ckpt = str(tmp_path / 'DaftExprt_test')
    torch.save({'iteration': 0, 'state_dict': dict(model.state_dict()), 'config_params': dict(vars(hp))}, ckpt)
    bank, syn = str(tmp_path / 'bank'), str(tmp_path / 'syn')
    _style_bank(bank, hp)
    text = tmp_path / 'sentences_to_generate.txt'
    text.write_text('s.txt_line0|{T EH1 S T} . ~\n', encoding='utf-8')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'synthesize.py'), '-out', syn, '-chk', ckpt, '-tf', str(text), '-sb', bank,
                        '-bs', '1', '-voc', os.path.join(out, 'g_00000004')], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert json.load(open(os.path.join(syn, 'prosody_transfer.json')))['audio'] == 'hifi-gan'
