"""CPU-side checks of the HiFi-GAN vocoder (K24): the float64 oracle every GPU test compares with is pinned against a direct-sum
NumPy restatement written from the layer formulas; its masks make a batch row equal to the utterance alone, and without them it
does not (so the test shapes can catch a missing mask); weight-norm folding, checkpoint loading and the constructor's validation
in `daft_exprt/vocoder.py`; the library exports the `dx_voc_*` entry points."""
import copy
import json
import os
import types

import numpy as np
import pytest
import torch

from tests import vocoder_oracle as O

LENGTHS = (23, 9, 1)


def _lrelu(x, s):
    return np.where(x > 0, x, x * s)


def _np_conv(x, w, b, d, slope):
    ''' x (C, T), w (Cout, Cin, k): y[o, t] = b[o] + sum_j sum_c w[o, c, j] lrelu(x)[c, t + j d - d (k - 1) / 2], zero outside '''
    a, (cout, _, k), T = _lrelu(x, slope), w.shape, x.shape[1]
    y = np.zeros((cout, T))
    for t in range(T):
        for j in range(k):
            src = t + j * d - d * (k - 1) // 2
            if 0 <= src < T:
                y[:, t] += w[:, :, j] @ a[:, src]
    return y + b[:, None]


def _np_upsample(x, w, b, u, slope):
    ''' x (Cin, T), w (Cin, Cout, k): input i adds w[:, :, j]^T lrelu(x)[:, i] to output i u - (k - u) / 2 + j '''
    a, (_, cout, k), T = _lrelu(x, slope), w.shape, x.shape[1]
    y = np.zeros((cout, T * u))
    for i in range(T):
        for j in range(k):
            o = i * u - (k - u) // 2 + j
            if 0 <= o < T * u:
                y[:, o] += w[:, :, j].T @ a[:, i]
    return y + b[:, None]


def _np_generator(cfg, weights, mel):
    ''' one utterance alone, mel (num_mels, T) float64 -> (T * hop,) '''
    W = {k: (w.double().numpy(), b.double().numpy()) for k, (w, b) in weights.items()}
    nk = len(cfg['resblock_kernel_sizes'])
    x = _np_conv(mel, *W['conv_pre'], 1, 1.)
    for i, u in enumerate(cfg['upsample_rates']):
        x = _np_upsample(x, *W[f'ups.{i}'], u, 0.1)
        total = 0.
        for j, dils in enumerate(cfg['resblock_dilation_sizes']):
            r, name = x, f'resblocks.{i * nk + j}'
            for m, d in enumerate(dils):
                if cfg['resblock'] == '1':
                    t = _np_conv(r, *W[f'{name}.convs1.{m}'], d, 0.1)
                    r = r + _np_conv(t, *W[f'{name}.convs2.{m}'], 1, 0.1)
                else:
                    r = r + _np_conv(r, *W[f'{name}.convs.{m}'], d, 0.1)
            total = total + r
        x = total / nk
    return np.tanh(_np_conv(x, *W['conv_post'], 1, 0.01)[0])


@pytest.fixture(scope='module')
def small():
    mel = O.make_mel(O.SMALL, LENGTHS, seed=1)
    return mel, O.make_weights(O.SMALL, mel, LENGTHS, seed=1)


@pytest.mark.parametrize('resblock', ['1', '2'])
def test_oracle_equals_direct_sums(small, resblock):
    mel, weights = small
    cfg = dict(O.SMALL, resblock=resblock)
    if resblock == '2':
        weights = O.make_weights(cfg, mel, LENGTHS, seed=2)
    for b in (0, 1):
        t = LENGTHS[b]
        got = O.generator(cfg, weights, mel[b:b + 1, :, :t], torch.tensor([t])).numpy()[0]
        want = _np_generator(cfg, weights, mel[b, :, :t].double().numpy())
        assert got.shape == want.shape == (t * cfg['hop_size'],)
        assert np.abs(got - want).max() <= 1e-12, np.abs(got - want).max()


@pytest.mark.parametrize('cfg,lengths', [(O.SMALL, LENGTHS), (O.V1, (12, 5))], ids=['small', 'v1'])
def test_masked_batch_is_each_utterance_alone_and_unmasked_is_not(cfg, lengths):
    mel = O.make_mel(cfg, lengths, seed=1)
    weights = O.make_weights(cfg, mel, lengths, seed=1)
    n, hop = torch.tensor(lengths), cfg['hop_size']
    masked = O.generator(cfg, weights, mel, n)
    unmasked = O.generator(cfg, weights, mel, n, masks=False)
    assert masked.shape == (len(lengths), max(lengths) * hop)
    valid = torch.cat([masked[b, :t * hop] for b, t in enumerate(lengths)])
    assert float((valid.abs() > 0.95).double().mean()) < 0.01          # tanh saturation cannot hide an error
    for b, t in enumerate(lengths):
        alone = O.generator(cfg, weights, mel[b:b + 1, :, :t], n[b:b + 1])[0]
        assert float((masked[b, :t * hop] - alone).abs().max()) <= 1e-12
        assert float(masked[b, t * hop:].abs().max() if t < max(lengths) else 0.) == 0.
        if 1 < t < max(lengths):                                        # the control: these shapes can catch a missing mask
            diff = float((unmasked[b, :t * hop] - alone).abs().max())
            print(f'unmasked vs alone, length {t}: {diff:.3g}')
            assert diff > 1e-2, diff


def test_garbage_past_the_length_does_not_reach_the_oracle(small):
    mel, weights = small
    dirty = mel.clone()
    for b, t in enumerate(LENGTHS):
        dirty[b, :, t:] = float('nan')
    n = torch.tensor(LENGTHS)
    assert torch.equal(O.generator(O.SMALL, weights, mel, n), O.generator(O.SMALL, weights, dirty, n))


# ---- daft_exprt/vocoder.py: folding, loading, validation ---------------------------------------------------------------------

def test_three_key_forms_fold_to_the_same_weights(small):
    from daft_exprt import vocoder as V
    _, weights = small
    folded = {form: V.folded_state(O.SMALL, O.state_dict(weights, form)) for form in O.FORMS}
    for name, (w, b) in weights.items():
        for form in O.FORMS:
            fw, fb = folded[form][name]
            assert fw.dtype == torch.float64 and fw.shape == w.shape
            assert float((fw - w.double()).abs().max()) <= 4e-7 * float(w.abs().max()), (name, form)
            assert torch.equal(fb, b.double())
    assert torch.equal(folded['weight_norm']['ups.0'][0], folded['parametrizations']['ups.0'][0])


def test_transposed_conv_norm_runs_over_axis_0_which_is_cin():
    from daft_exprt import vocoder as V
    g = torch.Generator().manual_seed(5)
    v = torch.randn((6, 4, 8), generator=g)                               # (Cin, Cout, k)
    gain = torch.rand((6, 1, 1), generator=g) + 0.5
    w = V.folded_weight({'ups.0.weight_g': gain, 'ups.0.weight_v': v}, 'ups.0')
    want = gain.double() * v.double() / v.double().pow(2).sum(dim=(1, 2), keepdim=True).sqrt()
    assert float((w - want).abs().max()) <= 1e-15
    other = gain.double().reshape(6, 1, 1) * v.double() / v.double().pow(2).sum(dim=(0, 2), keepdim=True).sqrt()
    assert float((w - other).abs().max()) > 1e-2                          # not the norm over Cout's slices


def test_packed_upsample_weight_holds_every_tap_once():
    from daft_exprt import vocoder as V
    w = torch.arange(2 * 3 * 7, dtype=torch.float64).reshape(2, 3, 7) + 1.     # k 7, u 3: phases of 3, 2 and 2 taps
    p = V.pack_upsample_weight(w, 3, torch.float32)
    assert p.shape == (3, 3, 3, 2)
    seen = []
    for phase in range(3):
        for s in range(3):
            j = (phase + 2) % 3 + 3 * s
            if j < 7:
                assert torch.equal(p[phase, s].double(), w[:, :, j].t())
                seen.append(j)
            else:
                assert float(p[phase, s].abs().max()) == 0.
    assert sorted(seen) == list(range(7))


@pytest.fixture
def V(monkeypatch):
    ''' the module with the upload of the packed weights stubbed out: the constructor then needs no device, and no test below
        launches a kernel '''
    from daft_exprt import vocoder
    monkeypatch.setattr(vocoder.H, 'device', lambda device=None: torch.device('cpu'))
    return vocoder


def test_validation_names_the_offending_key(small, V):
    _, weights = small

    def _bad(cfg, sd, match):
        with pytest.raises(ValueError, match=match):
            V.Vocoder(cfg, sd)
    sd = O.state_dict(weights)
    cfg = copy.deepcopy(O.SMALL)
    _bad(dict(cfg, resblock='3'), sd, 'resblock')
    _bad(dict(cfg, upsample_kernel_sizes=[8]), sd, 'upsample_kernel_sizes')
    _bad(dict(cfg, resblock_dilation_sizes=[[1, 3]]), sd, 'resblock_dilation_sizes')
    _bad(dict(cfg, resblock_kernel_sizes=[3, 4]), sd, 'resblock_kernel_sizes')
    _bad(dict(cfg, upsample_kernel_sizes=[2, 4]), sd, 'upsample_kernel_sizes')          # k < u
    _bad(dict(cfg, upsample_kernel_sizes=[7, 4]), sd, 'upsample_kernel_sizes')          # k - u odd
    _bad(dict(cfg, upsample_initial_channel=66), sd, 'upsample_initial_channel')
    _bad({k: v for k, v in cfg.items() if k != 'num_mels'}, sd, 'num_mels')
    _bad(cfg, {k: v for k, v in sd.items() if k != 'resblocks.1.convs2.0.weight'}, r'resblocks\.1\.convs2\.0')
    _bad(cfg, {k: v for k, v in sd.items() if k != 'ups.1.bias'}, r'ups\.1\.bias')
    _bad(cfg, dict(sd, **{'conv_pre.weight': sd['conv_pre.weight'][:, :40]}), 'conv_pre')
    _bad(dict(cfg, upsample_initial_channel=128), sd, 'conv_pre')                        # shapes no longer match the config


def test_checkpoint_loading_and_check_hparams(tmp_path, small, V):
    ''' a checkpoint written the way HiFi-GAN writes it, `config.json` beside it '''
    _, weights = small
    torch.save({'generator': O.state_dict(weights, 'weight_norm')}, str(tmp_path / 'g_00000001'))
    with open(tmp_path / 'config.json', 'w') as f:
        json.dump(O.SMALL, f)
    voc = V.Vocoder.from_checkpoint(str(tmp_path / 'g_00000001'))
    assert voc.hop == 8 and voc.num_mels == 80 and voc.mel_channels == 96
    w, b, shape, dil = voc._layers['resblocks.1.convs1.2']
    assert w.dtype == torch.bfloat16 and w.shape == (7, 32, 32) and dil == 5
    want = weights['resblocks.1.convs1.2'][0].permute(2, 0, 1)
    assert float((w.float() - want).abs().max()) <= 2 ** -8 * float(want.abs().max())
    voc32 = V.Vocoder(str(tmp_path / 'config.json'), O.state_dict(weights), compute_dtype='fp32')
    assert torch.equal(voc32._layers['resblocks.1.convs1.2'][0], want.contiguous())
    assert voc32._layers['ups.0'][0].shape == (4, 2, 32, 64)
    ok = types.SimpleNamespace(hop_length=8, n_mel_channels=80, sampling_rate=22050)
    voc.check_hparams(ok)
    for key, value, match in (('hop_length', 256, 'hop_length'), ('n_mel_channels', 40, 'num_mels'), ('sampling_rate', 16000, 'sampling_rate')):
        with pytest.raises(ValueError, match=match):
            voc.check_hparams(types.SimpleNamespace(**dict(vars(ok), **{key: value})))
    with pytest.raises(ValueError, match='generator'):
        torch.save({'state_dict': {}}, str(tmp_path / 'other'))
        V.Vocoder.from_checkpoint(str(tmp_path / 'other'))
    with pytest.raises(ValueError, match='compute_dtype'):
        V.Vocoder(O.SMALL, O.state_dict(weights), compute_dtype='fp16')


def test_pcm16_truncates_and_saturates():
    from daft_exprt import vocoder as V
    x = torch.tensor([0., 0.5, -0.5, 1., -1., 0.99999, 1e-5, -1e-5])
    assert V.pcm16(x).tolist() == [0, 16384, -16384, 32767, -32768, 32767, 0, 0]


# ---- ABI --------------------------------------------------------------------------------------------------------------------

def test_library_exports_the_vocoder_entry_points():
    from daft_exprt import _hip as H
    if not os.path.exists(H.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = H.lib()
    declared = [name for name, _, _ in H.header_prototypes() if name.startswith('dx_voc_')]
    assert sorted(declared) == ['dx_voc_conv', 'dx_voc_post', 'dx_voc_upsample']
    for name in declared:
        assert hasattr(lib, name), f'{name} declared in include/daft_exprt_hip.h but not exported'
    assert lib.dx_abi_version() == 13
    rc = lib.dx_voc_conv(None, 32, None, 1, None, None, 32, None, 32, None, 32, 1., 1, None, 1, 1, 32, 32, 3, 1, 0.1, None)
    assert rc == -1 and b'null' in lib.dx_last_error()
    rc = lib.dx_voc_conv(16, 32, 16, 1, None, None, 32, 16, 32, None, 32, 1., 1, 16, 1, 1, 32, 32, 4, 1, 0.1, None)
    assert rc == -2 and b'odd' in lib.dx_last_error()
    rc = lib.dx_voc_conv(20, 32, 16, 1, None, None, 32, 16, 32, None, 32, 1., 1, 16, 1, 1, 32, 32, 3, 1, 0.1, None)
    assert rc == -1 and b'aligned' in lib.dx_last_error()
    rc = lib.dx_voc_upsample(16, 32, 16, 1, None, 16, 32, 16, 1, 1, 32, 32, 7, 4, 0.1, None)
    assert rc == -2 and b'k - u even' in lib.dx_last_error()
    rc = lib.dx_voc_post(None, 32, None, None, None, 8, None, 1, 8, 32, 7, 0.01, None)
    assert rc == -1 and b'null' in lib.dx_last_error()
