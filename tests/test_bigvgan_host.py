"""CPU-side checks of the BigVGAN vocoder (K34): the two statements of the anti-aliased activation in tests/bigvgan_oracle.py --
the replicate-pad / grouped-conv form and the plain index sums of the kernel's contract -- agree; the Kaiser-sinc filter; the key
mapping, parameter transforms, filters, channel padding, workspace accounting and error messages of `daft_exprt/vocoder.py` with
the device upload stubbed out; fine-tuning refuses such a config; a HiFi-GAN config builds what it built before."""
import contextlib
import copy
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import bigvgan_oracle as G
from tests import vocoder_oracle as O

LENGTHS = (23, 9, 1)
BIG = dict(O.SMALL, activation='snakebeta', snake_logscale=True)
# the tail of the 1536-channel models in small: 96 -> 48 -> 24 channels, padded to 96 -> 64 -> 32
PADDED = dict(O.SMALL, upsample_initial_channel=96, upsample_rates=[2, 2], upsample_kernel_sizes=[4, 4], hop_size=4,
              activation='snakebeta', snake_logscale=True)


@pytest.fixture
def V(monkeypatch):
    ''' the module with the upload of the packed weights stubbed out, as in test_vocoder_host.py: no device, no launch '''
    from daft_exprt import vocoder
    monkeypatch.setattr(vocoder.H, 'device', lambda device=None: torch.device('cpu'))
    return vocoder


def _made(cfg, lengths=LENGTHS, seed=1):
    mel = O.make_mel(cfg, lengths, seed=seed)
    return (mel,) + G.make_weights(cfg, mel, lengths, seed=seed)


@pytest.fixture(scope='module')
def big():
    return _made(BIG)


# ---- the oracle --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n', [1, 2, 3, 7, 40])
def test_the_two_statements_of_the_activation_agree(n):
    g = torch.Generator().manual_seed(n)
    c = 5
    x = torch.randn((c, n), generator=g, dtype=torch.float64)
    alpha, inv_beta = torch.randn((c,), generator=g, dtype=torch.float64).exp(), torch.randn((c,), generator=g, dtype=torch.float64).exp()
    for f_up, f_down in ((G.kaiser_sinc_filter(), G.kaiser_sinc_filter()),
                         (torch.randn((12,), generator=g, dtype=torch.float64), torch.randn((12,), generator=g, dtype=torch.float64))):
        conv_form = G.activation(x[None], alpha, inv_beta, f_up, f_down)[0].numpy()
        loops = G.activation_loops(x.numpy(), alpha.numpy(), inv_beta.numpy(), f_up.numpy(), f_down.numpy())
        assert conv_form.shape == loops.shape == (c, n)
        assert np.abs(conv_form - loops).max() <= 1e-12, np.abs(conv_form - loops).max()


def test_filter_taps(V):
    for f in (G.kaiser_sinc_filter(), V.kaiser_sinc_filter()):
        assert f.dtype == torch.float64 and f.shape == (12,)
        assert float((f[:6] - torch.tensor(G.FIRST_TAPS, dtype=torch.float64)).abs().max()) <= 1e-9
        assert float((f - f.flip(0)).abs().max()) <= 1e-15
        assert abs(float(f.sum()) - 1.) <= 1e-15
    assert float((G.kaiser_sinc_filter() - V.kaiser_sinc_filter()).abs().max()) <= 1e-15


@pytest.mark.parametrize('n', [1, 2, 9])
def test_a_constant_stays_constant_without_the_periodic_term(n):
    f = G.kaiser_sinc_filter()
    x = torch.full((1, 3, n), 0.75, dtype=torch.float64)
    y = G.activation(x, torch.ones(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64), f, f)
    assert float((y - 0.75).abs().max()) <= 1e-14


def test_oracle_batch_rows_are_the_utterances_alone(big):
    mel, weights, _, acts, filters = big
    both = G.generator(BIG, weights, acts, filters, mel, LENGTHS)
    assert both.shape == (3, 23 * 8)
    assert float((both.abs() > 0.95).double().mean()) < 0.01
    for b, t in enumerate(LENGTHS):
        alone = G.generator(BIG, weights, acts, filters, mel[b:b + 1, :, :t], [t])
        assert torch.equal(alone[0], both[b, :t * 8]) and float(both[b, t * 8:].abs().sum()) == 0.
    dirty = mel.clone()
    for b, t in enumerate(LENGTHS):
        dirty[b, :, t:] = float('nan')
    assert torch.equal(G.generator(BIG, weights, acts, filters, dirty, LENGTHS), both)


# ---- daft_exprt/vocoder.py ---------------------------------------------------------------------------------------------------

def test_without_the_feature_the_loader_stopped_at_ups_0(big, V):
    ''' `ups.I.0` (upstream's ModuleList) and `ups.I` are both accepted, in every weight form '''
    _, weights, raw, _, filters = big
    built = [V.Vocoder(BIG, G.state_dict(BIG, weights, raw, filters, form=form, nested_ups=nested), compute_dtype='fp32')
             for form in O.FORMS for nested in (True, False)]
    assert all(v.bigvgan for v in built)
    for v in built[1:]:
        for name, (w, b, shape, dil) in built[0]._layers.items():
            assert shape == v._layers[name][2] and dil == v._layers[name][3]
            assert float((w - v._layers[name][0]).abs().max()) <= 4e-7 * float(w.abs().max()), name
            assert torch.equal(b, v._layers[name][1])
    w, _, shape, _ = built[1]._layers['ups.0']                                  # the plain form: exact
    assert shape == (64, 32, 8) and torch.equal(w, V.pack_upsample_weight(weights['ups.0'][0].double(), 4, torch.float32))


@pytest.mark.parametrize('activation', ['snake', 'snakebeta'])
@pytest.mark.parametrize('logscale', [False, True])
def test_parameter_forms(activation, logscale, V):
    cfg = dict(O.SMALL, activation=activation, snake_logscale=logscale)
    _, weights, raw, acts, filters = _made(cfg, seed=2)
    voc = V.Vocoder(cfg, G.state_dict(cfg, weights, raw), compute_dtype='fp32')
    assert list(voc._acts) == [conv for conv, _ in G.fed_convs(cfg)]
    for conv, _ in G.fed_convs(cfg):
        a_raw, b_raw = raw[conv]
        assert (b_raw is None) == (activation == 'snake')
        a = (a_raw.double().exp() if logscale else a_raw.double())
        b = a if b_raw is None else (b_raw.double().exp() if logscale else b_raw.double())
        alpha, inv_beta, taps = voc._acts[conv]
        c = a.numel()
        assert alpha.dtype == inv_beta.dtype == torch.float32
        assert torch.equal(alpha[:c], a.float()) and torch.equal(inv_beta[:c], (1. / (b + 1e-9)).float())
        assert torch.equal(alpha[:c], acts[conv][0]) and torch.equal(inv_beta[:c], acts[conv][1])
        assert bool((alpha[c:] == 1.).all()) and bool((inv_beta[c:] == 0.).all())
        assert alpha.numel() == voc._layers[conv][2][1] and alpha.numel() % 32 == 0
        want = torch.cat([V.kaiser_sinc_filter(), V.kaiser_sinc_filter()]).float()          # no filter in the checkpoint: the formula
        assert torch.equal(torch.tensor(list(taps)), want)
    assert float(voc._acts['conv_post'][0].min()) > 0.


def test_filters_of_the_checkpoint_are_preferred(big, V):
    _, weights, raw, _, _ = big
    f_up, f_down = torch.arange(12.) - 3., torch.arange(12.) * 0.5 + 1.
    voc = V.Vocoder(BIG, G.state_dict(BIG, weights, raw, (f_up, f_down)), compute_dtype='bf16')
    for conv in voc._acts:
        assert list(voc._acts[conv][2]) == f_up.tolist() + f_down.tolist()
    sd = G.state_dict(BIG, weights, raw, (f_up, f_down))
    del sd['activation_post.upsample.filter']                                               # one activation without: only it is computed
    voc = V.Vocoder(BIG, sd, compute_dtype='bf16')
    assert list(voc._acts['conv_post'][2]) == V.kaiser_sinc_filter().float().tolist() + f_down.tolist()
    assert list(voc._acts['resblocks.3.convs2.2'][2]) == f_up.tolist() + f_down.tolist()


def test_errors_name_what_is_wrong(big, V):
    _, weights, raw, _, filters = big
    sd = G.state_dict(BIG, weights, raw, filters)

    def _bad(cfg, state, match):
        with pytest.raises(ValueError, match=match):
            V.Vocoder(cfg, state)
    _bad(dict(BIG, activation='relu'), sd, 'activation.*relu')
    _bad(BIG, {k: v for k, v in sd.items() if k not in ('resblocks.1.activations.2.act.alpha', 'resblocks.2.activations.0.act.alpha')},
         r'resblocks\.1\.activations\.2\.act\.alpha')                                      # the first one missing
    _bad(BIG, {k: v for k, v in sd.items() if k != 'activation_post.act.beta'}, r'activation_post\.act\.beta')
    _bad(BIG, dict(sd, **{'resblocks.0.activations.1.downsample.lowpass.filter': torch.ones((1, 1, 8))}),
         r'resblocks\.0\.activations\.1\.downsample\.lowpass\.filter.*\(1, 1, 8\)')
    _bad(BIG, dict(sd, **{'resblocks.0.activations.1.act.alpha': torch.ones((7,))}), r'resblocks\.0\.activations\.1\.act\.alpha')
    _bad(BIG, {k: v for k, v in sd.items() if not k.startswith('ups.1.')}, r'ups\.1')
    V.Vocoder(dict(BIG, use_cuda_kernel=True), sd)                                         # ignored
    with pytest.raises(ValueError, match='conv_post.bias'):
        V.Vocoder(BIG, {k: v for k, v in sd.items() if k != 'conv_post.bias'})
    no_bias = V.Vocoder(dict(BIG, use_bias_at_final=False, use_tanh_at_final=False), {k: v for k, v in sd.items() if k != 'conv_post.bias'})
    assert float(no_bias._layers['conv_post'][1].abs().max()) == 0. and no_bias._final_clamp
    assert not V.Vocoder(BIG, sd)._final_clamp


def test_padded_packing_puts_zeros_where_it_should(V):
    _, weights, raw, _, filters = _made(PADDED, lengths=(9, 4))
    voc = V.Vocoder(PADDED, G.state_dict(PADDED, weights, raw, filters, form='plain'), compute_dtype='fp32')
    assert voc._chans == [96, 64, 32] and voc.mel_channels == 96
    for name, (w, b, shape, _) in voc._layers.items():
        plain_w, plain_b = weights[name]
        if name == 'conv_pre':
            assert shape == (96, 80, 7) and w.shape == (7, 96, 96)
            assert torch.equal(w[:, :, :80], plain_w.permute(2, 0, 1)) and float(w[:, :, 80:].abs().max()) == 0.
        elif name == 'conv_post':
            assert shape == (1, 32, 7) and w.shape == (7, 32)
            assert torch.equal(w[:, :24], plain_w[0].t()) and float(w[:, 24:].abs().max()) == 0.
            assert torch.equal(b, plain_b)
        elif name.startswith('ups.'):
            cin, cout, k = plain_w.shape
            assert shape == ((96, 64, 4), (64, 32, 4))[int(name[-1])] and w.shape == (2, 2, shape[1], shape[0])
            assert torch.equal(w[:, :, :cout, :cin], V.pack_upsample_weight(plain_w.double(), 2, torch.float32))
            assert float(w[:, :, cout:].abs().max()) == 0. and float(w[:, :, :, cin:].abs().max() if cin < shape[0] else 0.) == 0.
            assert torch.equal(b[:cout], plain_b) and float(b[cout:].abs().max()) == 0.
        else:
            c = plain_w.shape[0]
            cp = 64 if c == 48 else 32
            assert shape == (cp, cp, plain_w.shape[2]) and w.shape == (plain_w.shape[2], cp, cp)
            assert torch.equal(w[:, :c, :c], plain_w.permute(2, 0, 1))
            assert float(w[:, c:].abs().max()) == 0. and float(w[:, :, c:].abs().max()) == 0.
            assert torch.equal(b[:c], plain_b) and float(b[c:].abs().max()) == 0.


def test_workspace_counts_seven_buffers(big, V, monkeypatch):
    _, weights, raw, _, filters = big
    voc = V.Vocoder(BIG, G.state_dict(BIG, weights, raw, filters))
    hifi_weights = O.make_weights(O.SMALL, O.make_mel(O.SMALL, LENGTHS, seed=1), LENGTHS, seed=1)
    hifi = V.Vocoder(O.SMALL, O.state_dict(hifi_weights))
    assert (voc._buffers, hifi._buffers) == (7, 6)
    # SMALL's last stage has 16 channels: BigVGAN runs it padded to 32, HiFi-GAN as it is
    assert voc._elements_per_utterance(10) == (10 * 8 * 32, 10 * 96) and hifi._elements_per_utterance(10) == (10 * 4 * 32, 10 * 96)
    for v, per_utt in ((voc, 7 * 2560 + 960), (hifi, 6 * 1280 + 960)):
        seen = []
        monkeypatch.setattr(v, '_run', lambda mel, lengths, out, T: seen.append(mel.shape[0]))
        monkeypatch.setattr(V.H, 'require_gpu', lambda *tensors: None)
        monkeypatch.setattr(V.torch.cuda, 'device', lambda device: contextlib.nullcontext())
        mel = torch.zeros((3, 80, 10))
        n = torch.tensor([10, 10, 10])
        v(mel, n, max_workspace_bytes=4 * 2 * per_utt)
        assert seen == [2, 1]
        seen.clear()
        v(mel, n, max_workspace_bytes=4 * 2 * per_utt - 1)
        assert seen == [1, 1, 1]


def test_fine_tuning_refuses_a_bigvgan_config(big):
    from daft_exprt import vocoder_train as VT
    _, weights, raw, _, filters = big
    with pytest.raises(ValueError, match='activation.*snakebeta'):
        VT.TrainableGenerator(BIG, G.state_dict(BIG, weights, raw, filters))
    with pytest.raises(ValueError, match='activation'):
        VT.trainable_stages(dict(O.V1, activation='snake'))
    VT.trainable_stages(O.V1)


def test_a_hifigan_config_builds_what_it_built_before(V):
    weights = O.make_weights(O.SMALL, O.make_mel(O.SMALL, LENGTHS, seed=1), LENGTHS, seed=1)
    voc = V.Vocoder(copy.deepcopy(O.SMALL), O.state_dict(weights), compute_dtype='fp32')
    assert not voc.bigvgan and voc._acts == {} and voc._chans == [64, 32, 16]
    assert (voc._slope, voc._post_slope, voc._final_clamp) == (V.LRELU_SLOPE, V.POST_SLOPE, False)
    assert voc.hop == 8 and voc.num_mels == 80 and voc.mel_channels == 96
    assert list(voc._layers) == [name for name, _, _, _ in V.layer_table(O.SMALL)]
    w, b, shape, dil = voc._layers['resblocks.1.convs1.2']
    assert torch.equal(w, weights['resblocks.1.convs1.2'][0].permute(2, 0, 1).contiguous()) and shape == (32, 32, 7) and dil == 5
    assert voc._layers['resblocks.3.convs1.0'][2] == (16, 16, 7)                               # not padded
    assert voc._layers['ups.0'][0].shape == (4, 2, 32, 64)
    assert torch.equal(voc._layers['conv_post'][1], weights['conv_post'][1])


# ---- ABI --------------------------------------------------------------------------------------------------------------------

def test_library_exports_the_activation():
    from daft_exprt import _hip as H
    if not os.path.exists(H.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = H.lib()
    for name in ('dx_vocoder_snake', 'dx_vocoder_snake_tile_rows', 'dx_vocoder_post_clamp'):
        assert name in [n for n, _, _ in H.header_prototypes()] and hasattr(lib, name)
    assert lib.dx_abi_version() == 13
    assert lib.dx_vocoder_snake_tile_rows() >= 12
    taps =(ctypes.c_float * 24)()
    f = ctypes.addressof(taps)
    assert lib.dx_vocoder_snake(None, 32, 16, 16, f, 32, 32, 16, 1, 8, 32, None) == -1 and b'null' in lib.dx_last_error()
    assert lib.dx_vocoder_snake(16, 32, 16, 16, None, 32, 32, 16, 1, 8, 32, None) == -1 and b'null' in lib.dx_last_error()
    assert lib.dx_vocoder_snake(16, 32, 16, 16, f, 32, 32, 16, 1, 0, 32, None) == -2
    assert lib.dx_vocoder_snake(16, 16, 16, 16, f, 32, 32, 16, 1, 8, 32, None) == -2 and b'ldx' in lib.dx_last_error()
    assert lib.dx_vocoder_snake(16, 32, 16, 16, f, 32, 32, 16, 1, 8, 30, None) != 0 and b'multiples of 4' in lib.dx_last_error()
    assert lib.dx_vocoder_snake(16, 32, 16, 16, f, 36, 32, 16, 1, 8, 32, None) == -1 and b'aligned' in lib.dx_last_error()
    assert lib.dx_vocoder_snake(32, 32, 16, 16, f, 32, 32, 16, 1, 8, 32, None) == -1 and b'alias' in lib.dx_last_error()
    assert lib.dx_vocoder_snake(16, 32, 16, 16, f, 32, 32, 16, 60000, 2 ** 31 - 1, 32, None) != 0 and b'grid' in lib.dx_last_error()
    assert lib.dx_vocoder_post_clamp(None, 32, None, None, None, 8, None, 1, 8, 32, 7, 1., None) == -1 and b'null' in lib.dx_last_error()
