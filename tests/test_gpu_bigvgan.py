"""The BigVGAN vocoder on the GPU -- K34 (csrc/snake.hip: the anti-aliased periodic activation) alone, and whole generators through
daft_exprt/vocoder.py -- against tests/bigvgan_oracle.py, the float64 restatement pinned in tests/test_bigvgan_host.py, and never
against the code under test.

Tolerances are computed at run time from the oracle's own switches:
    the activation alone   max |y - o64| <= max(8 x max |o32 - o64|, 2e-6 x max |o64|), o32 the same oracle in float32
    whole generators       `_bound` of tests/test_gpu_vocoder.py as it stands: its fp32 rule and its bf16 stage rule
Every test prints the measured values.  Rows: with R the kernel's own row tile, n = 1, 2, 3, 5, 6, 11 (both clamps and the 5-row
halo inside one tile), R - 1, R, R + 1 and 2 R + 3 (tile seams), and N itself."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests import bigvgan_oracle as G
from tests import vocoder_oracle as O
from tests.test_gpu_vocoder import _bound, _read_pcm16, _three

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DTYPES = ['fp32', 'bf16']
# asymmetric, twelve distinct values each: a flipped, shifted or swapped tap changes the sums
INT_UP = (3., -1., 4., 1., -5., 9., 2., -6., 5., -3., 7., -2.)
INT_DOWN = (2., 7., -1., 8., -2., -8., 1., -4., 5., 9., -3., 6.)


@functools.lru_cache(maxsize=None)
def _tile():
    from daft_exprt import _hip as H
    return int(H.lib().dx_vocoder_snake_tile_rows())


def _rows():
    r = _tile()
    n_max = 2 * r + 7
    return (1, 2, 3, 5, 6, 11, r - 1, r, r + 1, 2 * r + 3, n_max), n_max


def _snake(x, n, alpha, inv_beta, f_up, f_down, N=None, ld_pad=(4, 8), fill=float('nan')):
    ''' x (B, C, >= max n) CPU -> y (B, N, C) from the kernel; the input rows at or past n[b], both buffers' row padding and all of
        y hold `fill` before the launch; the padding of y must still hold it afterwards '''
    from daft_exprt import _hip as H
    B, C = x.shape[:2]
    N = N or x.shape[2]
    ldx, ldy = C + ld_pad[0], C + ld_pad[1]
    xd = torch.full((B, N, ldx), fill)
    for b, rows in enumerate(n):
        xd[b, :rows, :C] = x[b, :, :rows].t().float()
    xd, y = xd.to(DEV), torch.full((B, N, ldy), fill, device=DEV)
    taps = (ctypes.c_float * 24)(*[float(v) for v in f_up], *[float(v) for v in f_down])
    nd, ad, bd = torch.tensor(n, dtype=torch.int64, device=DEV), alpha.float().to(DEV), inv_beta.float().to(DEV)
    H.check(H.lib().dx_vocoder_snake(H.ptr(xd), ldx, H.ptr(ad), H.ptr(bd), ctypes.addressof(taps), H.ptr(y), ldy, H.ptr(nd), B, N, C,
                                     H.stream()))
    torch.cuda.synchronize()
    pad = y[:, :, C:]
    assert bool(torch.isnan(pad).all()) if fill != fill else bool((pad == fill).all())           # nothing beside the rows is written
    return y[:, :, :C].cpu()


def _oracle(x, n, N, alpha, inv_beta, f_up, f_down, dtype=torch.float64):
    ''' (B, N, C) float64: every utterance alone at its own length, zeros past it '''
    out = torch.zeros((x.shape[0], N, x.shape[1]), dtype=torch.float64)
    taps = [torch.as_tensor(f, dtype=torch.float64).float() for f in (f_up, f_down)]
    for b, rows in enumerate(n):
        if rows:
            out[b, :rows] = G.activation(x[b:b + 1, :, :rows].to(dtype), alpha, inv_beta, *taps)[0].t().double()
    return out


def _params(form, c, seed):
    g = torch.Generator().manual_seed(seed)
    a, b = 0.5 * torch.randn((c,), generator=g), 0.5 * torch.randn((c,), generator=g)
    return G.final_params(a.exp(), None, False) if form == 'snake' else G.final_params(a, b, True)


# ---- the activation alone ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('form', ['snake', 'snakebeta_logscale'])
@pytest.mark.parametrize('c', [32, 8, 96])
def test_snake_alone(c, form):
    n, N = _rows()
    x = torch.randn((len(n), c, N), generator=torch.Generator().manual_seed(c))
    alpha, inv_beta = _params(form, c, c + 1)
    f = G.kaiser_sinc_filter().float()
    y = _snake(x, n, alpha, inv_beta, f, f).double()
    o64, o32 = (_oracle(x, n, N, alpha, inv_beta, f, f, dtype=dt) for dt in (torch.float64, torch.float32))
    assert bool(torch.isfinite(y).all())
    cost, top = float((o32 - o64).abs().max()), float(o64.abs().max())
    err, tol = float((y - o64).abs().max()), max(8. * cost, 2e-6 * top)
    print(f'snake C {c} {form}: err {err:.3g}, fp32 oracle cost {cost:.3g}, max |o64| {top:.3g}, bound {tol:.3g}')
    assert err <= tol, (err, tol)
    for b, rows in enumerate(n):
        assert float(y[b, rows:].abs().max() if rows < N else 0.) == 0.                          # dead rows: exact zeros
    # the periodic term is there and differs per channel: against the same pass without it
    plain = _oracle(x, n, N, alpha, torch.zeros_like(inv_beta), f, f)
    assert float((o64 - plain).abs().max()) > 0.1


@pytest.mark.parametrize('c', [32, 8, 96])
def test_index_maps_with_asymmetric_integers(c):
    ''' alpha = 0 and inv_beta = 0 make the kernel linear; integer taps and integer x make every sum an exactly representable
        integer: bit-equal to the oracle, or a tap, a clamp or a tile seam is wrong '''
    n, N = _rows()
    t, ch, b = torch.arange(N), torch.arange(c), torch.arange(len(n))
    x = (((3 * t[None, None, :] + 5 * ch[None, :, None] + 2 * b[:, None, None]) % 7) - 3).double()
    zero = torch.zeros((c,))
    want = _oracle(x, n, N, zero, zero, INT_UP, INT_DOWN)
    assert float(want.abs().max()) < 2 ** 24 and float(2 * sum(abs(v) for v in INT_UP) * 3 * sum(abs(v) for v in INT_DOWN)) < 2 ** 24
    assert bool((want == want.round()).all()) and float(want.abs().max()) > 100.
    assert len(set(INT_UP)) == len(set(INT_DOWN)) == 12 and INT_UP != INT_UP[::-1] and INT_DOWN != INT_DOWN[::-1]
    y = _snake(x, n, zero, zero, INT_UP, INT_DOWN).double()
    assert torch.equal(y, want), float((y - want).abs().max())


@pytest.mark.parametrize('c', [32, 8])
def test_dead_rows_are_neither_read_nor_left(c):
    n, N = _rows()
    n = n[:-1] + (0,)                                                                            # and an empty utterance
    x = torch.randn((len(n), c, N), generator=torch.Generator().manual_seed(7 + c))
    alpha, inv_beta = _params('snakebeta_logscale', c, 3)
    f = G.kaiser_sinc_filter().float()
    poisoned = _snake(x, n, alpha, inv_beta, f, f)                                               # NaN past n[b] and all over y
    finite = _snake(x, n, alpha, inv_beta, f, f, fill=123.)
    assert bool(torch.isfinite(poisoned).all()) and torch.equal(poisoned, finite)
    for b, rows in enumerate(n):
        assert float(poisoned[b, rows:].abs().max() if rows < N else 0.) == 0.
        if rows:                                                                                 # alone, at its own N and at another
            alone = _snake(x[b:b + 1], (rows,), alpha, inv_beta, f, f, N=rows)
            assert torch.equal(alone[0], poisoned[b, :rows]), (b, rows)
            wider = _snake(x[b:b + 1], (rows,), alpha, inv_beta, f, f, N=rows + _tile() + 1, ld_pad=(0, 0))
            assert torch.equal(wider[0, :rows], poisoned[b, :rows]) and float(wider[0, rows:].abs().max()) == 0.
    order = list(reversed(range(len(n))))                                                        # other neighbours
    swapped = _snake(x[order], tuple(n[b] for b in order), alpha, inv_beta, f, f)
    assert torch.equal(swapped, poisoned[order])


# ---- whole generators --------------------------------------------------------------------------------------------------------

SNAKEBETA = dict(O.SMALL, activation='snakebeta', snake_logscale=True)
CASES = {'snakebeta': (SNAKEBETA, (23, 9, 1), 0.3),
         'snake_resblock2': (dict(O.SMALL, resblock='2', activation='snake'), (23, 9, 1), 0.3),
         'clamp_no_bias': (dict(SNAKEBETA, use_tanh_at_final=False, use_bias_at_final=False), (23, 9, 1), 0.5),
         'padded_channels': (dict(O.SMALL, upsample_initial_channel=96, upsample_rates=[2, 2], upsample_kernel_sizes=[4, 4], hop_size=4,
                                  activation='snakebeta', snake_logscale=True), (9, 4), 0.3)}


@functools.lru_cache(maxsize=None)
def _case(name):
    ''' (cfg, lengths, mel with random values past the lengths, state dict, oracle64, oracle32, oracle_rounded), computed once '''
    cfg, lengths, rms = CASES[name]
    mel = O.make_mel(cfg, lengths, seed=3)
    weights, raw, acts, filters = G.make_weights(cfg, mel, lengths, seed=3, rms=rms)
    o64, o32, orr = _three(lambda dt, rounding: G.generator(cfg, weights, acts, filters, mel, lengths, rounding=rounding, dtype=dt).double())
    return cfg, lengths, mel, G.state_dict(cfg, weights, raw, filters), o64, o32, orr


@functools.lru_cache(maxsize=None)
def _vocoder(name, dtype):
    from daft_exprt.vocoder import Vocoder
    cfg, _, _, sd, _, _, _ = _case(name)
    return Vocoder(cfg, sd, compute_dtype=dtype, device=DEV)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', list(CASES))
def test_generator_matches_the_oracle(name, dtype):
    cfg, lengths, mel, _, o64, o32, orr = _case(name)
    hop = cfg['hop_size']
    if cfg.get('use_tanh_at_final', True):
        assert float((o64.abs() > 0.95).double().mean()) < 0.01                                 # tanh saturation cannot hide an error
    else:
        clamped = float((o64.abs() == 1.).double().mean())
        assert 0. < clamped < 0.1, clamped                                                      # the clamp engages, and hides little
    wavs, n_samples = _vocoder(name, dtype)(mel.to(DEV), torch.tensor(lengths, device=DEV))
    assert wavs.shape == (len(lengths), max(lengths) * hop) and wavs.dtype == torch.float32
    assert n_samples.tolist() == [t * hop for t in lengths]
    _bound(wavs, o64, o32, orr, dtype, f'bigvgan generator {name}')
    for b, t in enumerate(lengths):
        assert float(wavs[b, t * hop:].abs().max() if t < max(lengths) else 0.) == 0.
    assert float(wavs.abs().max()) <= 1.


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', ['snakebeta', 'padded_channels'])
def test_batch_independence_and_poison_bit_for_bit(name, dtype):
    from daft_exprt import config
    cfg, lengths, mel, _, _, _, _ = _case(name)
    hop, voc = cfg['hop_size'], _vocoder(name, dtype)
    mel_d, n = mel.to(DEV), torch.tensor(lengths, device=DEV)
    wavs, _ = voc(mel_d, n)
    again, _ = voc(mel_d, n)
    assert torch.equal(wavs, again)                                                             # a second call
    split, _ = voc(mel_d, n, max_workspace_bytes=1)                                             # one utterance per sub-batch
    assert torch.equal(wavs, split)
    for b, t in enumerate(lengths):
        alone, n_alone = voc(mel_d[b:b + 1, :, :t].contiguous(), n[b:b + 1])
        assert alone.shape == (1, t * hop) and int(n_alone[0]) == t * hop
        assert torch.equal(alone[0], wavs[b, :t * hop]), (b, float((alone[0] - wavs[b, :t * hop]).abs().max()))
    order = list(reversed(range(len(lengths))))                                                  # other neighbours, another padded length
    swapped, _ = voc(torch.cat([mel_d[order], mel_d[order]], dim=2), n[order])
    for row, b in enumerate(order):
        assert torch.equal(swapped[row, :lengths[b] * hop], wavs[b, :lengths[b] * hop])
    dirty = mel.clone()
    for b, t in enumerate(lengths):
        dirty[b, :, t:] = float('nan')
    old = config.POISON
    config.POISON = True
    try:
        voc._ws = None                                                                          # a fresh, NaN-filled workspace
        got, _ = voc(dirty.to(DEV), n)
        torch.cuda.synchronize()
    finally:
        config.POISON = old
    assert bool(torch.isfinite(got).all()) and torch.equal(got, wavs)


# ---- the public surface -----------------------------------------------------------------------------------------------------

SURFACE = {'resblock': '1', 'upsample_rates': [8, 8, 4], 'upsample_kernel_sizes': [16, 16, 8], 'upsample_initial_channel': 256,
           'resblock_kernel_sizes': [3], 'resblock_dilation_sizes': [[1, 3]], 'num_mels': 80, 'hop_size': 256, 'sampling_rate': 22050,
           'activation': 'snakebeta', 'snake_logscale': True, 'use_cuda_kernel': False}


def test_a_checkpoint_as_upstream_writes_it_through_generate_mel_specs(golden_dir, tmp_path):
    from daft_exprt import generate as G_
    from daft_exprt.vocoder import Vocoder, pcm16
    from tests.test_gpu_prosody_eval import SENTENCES, _style_bank, _tiny_model
    model, hp = _tiny_model(golden_dir)
    model = model.cuda(0)
    weights, raw, acts, filters = G.make_weights(SURFACE, O.make_mel(SURFACE, (4,), seed=7), (4,), seed=7)
    voc_dir = tmp_path / 'bigvgan'
    voc_dir.mkdir()
    sd = G.state_dict(SURFACE, weights, raw, filters, form='weight_norm', nested_ups=True)
    assert 'ups.0.0.weight_g' in sd and 'activation_post.downsample.lowpass.filter' in sd and 'ups.0.weight_g' not in sd
    torch.save({'generator': sd}, str(voc_dir / 'bigvgan_generator.pt'))
    (voc_dir / 'config.json').write_text(json.dumps(SURFACE))
    voc = Vocoder.from_checkpoint(str(voc_dir / 'bigvgan_generator.pt'), compute_dtype='fp32', device=DEV)
    assert voc.bigvgan
    bank = str(tmp_path / 'bank')
    G_.extract_reference_parameters_batch(_style_bank(bank, hp), bank, hp)
    refs = [os.path.join(bank, n) for n in ('glide.npz', 'vibrato.npz', 'glide.npz')]
    out_dir = str(tmp_path / 'voc')
    preds = G_.generate_mel_specs(model, SENTENCES, ['a', 'b', 'c'], [0, 3, 7], refs, out_dir, hp, batch_size=3, vocoder=voc)
    assert len(preds) == 3 and sorted(os.listdir(out_dir)) == sorted([f'{name}.npz' for name in preds] + [f'{name}.wav' for name in preds])
    for name in preds:
        mel = torch.from_numpy(preds[name][4])[None]
        t = mel.shape[2]
        want = pcm16(G.generator(SURFACE, weights, acts, filters, mel, [t], dtype=torch.float32)[0]).numpy().astype(np.int64)
        pcm = _read_pcm16(os.path.join(out_dir, f'{name}.wav')).astype(np.int64)
        assert pcm.shape == want.shape == (t * hp.hop_length,)
        print(f'{name}: {t} frames, max |pcm - oracle| {np.abs(pcm - want).max()} LSB, peak {np.abs(pcm).max()}')
        assert np.abs(pcm - want).max() <= 1
        assert np.abs(pcm).max() > 100                                                          # audio, not silence
