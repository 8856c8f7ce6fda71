"""CPU-side checks of BigVGAN fine-tuning (K35, `daft_exprt/bigvgan_train.py`): the two statements of the activation's backward in
tests/bigvgan_grad_oracle.py -- float64 autograd through `bigvgan_oracle.activation` and the plain index sums of the kernel's contract --
agree; the raw-to-final parameter chain against closed forms; the ABI of `dx_vocoder_snake_bwd` and every argument refusal (none of
them launches); `trainable_generator`'s dispatch, `TrainableBigVGAN`'s state dict and its refusal of padded stages, built on the CPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import bigvgan_grad_oracle as BG
from tests import bigvgan_oracle as BO
from tests import vocoder_oracle as O

# asymmetric, and neither filter sums to zero
INT_UP = (1., -2., 3., 1., 2., -1., 3., 2., -3., 1., 2., 1.)
INT_DOWN = (2., 1., -1., 3., -2., 1., 1., 2., 3., -1., 2., -3.)
BIG = dict(O.SMALL, upsample_initial_channel=128, activation='snakebeta', snake_logscale=True)     # stages of 128, 64, 32 channels
LENGTHS = (9, 4)


# ---- the oracle --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n', [1, 2, 3, 5, 6, 11, 40])
def test_the_two_statements_of_the_backward_agree(n):
    g = torch.Generator().manual_seed(100 + n)
    c = 4
    x, dy = (torch.randn((c, n), generator=g, dtype=torch.float64) for _ in range(2))
    alpha, inv_beta = (torch.randn((c,), generator=g, dtype=torch.float64).exp() for _ in range(2))
    kaiser = BO.kaiser_sinc_filter()
    for f_up, f_down in ((torch.tensor(INT_UP, dtype=torch.float64), torch.tensor(INT_DOWN, dtype=torch.float64)), (kaiser, kaiser)):
        auto = BG.snake_grads(x[None], dy[None], alpha, inv_beta, (f_up, f_down))
        loops = BG.snake_grad_loops(x.numpy(), dy.numpy(), alpha.numpy(), inv_beta.numpy(), f_up.numpy(), f_down.numpy())
        for what, a, l in zip(('dx', 'dalpha', 'dinv_beta'), (auto[0][0], auto[1], auto[2]), loops):
            a = a.numpy()
            assert a.shape == l.shape
            rel = np.abs(a - l).max() / np.abs(a).max()
            assert rel <= 1e-12, (what, n, rel)


def test_snake_grads_stop_at_each_utterance_end():
    g = torch.Generator().manual_seed(7)
    x, dy = (torch.randn((2, 3, 9), generator=g, dtype=torch.float64) for _ in range(2))
    alpha, inv_beta = (torch.randn((3,), generator=g, dtype=torch.float64).exp() for _ in range(2))
    taps = (BO.kaiser_sinc_filter(), BO.kaiser_sinc_filter())
    dirty = x.clone()
    dirty[1, :, 4:] = float('nan')
    dx, da, db = BG.snake_grads(dirty, dy, alpha, inv_beta, taps, n=[9, 4])
    assert bool(torch.isfinite(dx).all()) and float(dx[1, :, 4:].abs().max()) == 0.
    one = BG.snake_grads(x[:1], dy[:1], alpha, inv_beta, taps)
    two = BG.snake_grads(x[1:, :, :4], dy[1:, :, :4], alpha, inv_beta, taps)
    assert torch.equal(dx[0], one[0][0]) and torch.equal(dx[1, :, :4], two[0][0])
    assert float((da - one[1] - two[1]).abs().max()) <= 1e-12 * float(da.abs().max())
    assert float((db - one[2] - two[2]).abs().max()) <= 1e-12 * float(db.abs().max())


# ---- raw -> final parameters ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('snakebeta', [False, True])
@pytest.mark.parametrize('logscale', [False, True])
def test_parameter_chain_against_closed_forms(snakebeta, logscale):
    from daft_exprt import bigvgan_train as BT
    g = torch.Generator().manual_seed(3)
    c = 8
    raw_a, raw_b = (0.5 * torch.randn((c,), generator=g) for _ in range(2))
    if not logscale:
        raw_a, raw_b = raw_a.exp(), raw_b.exp()
    ga, gi = (torch.randn((c,), generator=g, dtype=torch.float64) for _ in range(2))         # the gradients the kernel hands back
    a, b = raw_a.clone().requires_grad_(True), (raw_b.clone().requires_grad_(True) if snakebeta else None)
    alpha, inv_beta = BT.final_params(a, b, logscale)
    want = BO.final_params(raw_a, raw_b if snakebeta else None, logscale)
    assert alpha.dtype == inv_beta.dtype == torch.float32
    assert torch.equal(alpha, want[0]) and torch.equal(inv_beta, want[1])                    # the inference path's bits
    (alpha.double() * ga + inv_beta.double() * gi).sum().backward()
    a64, b64 = raw_a.double(), raw_b.double()
    fa = a64.exp() if logscale else a64                                                      # alpha'
    fb = (b64.exp() if logscale else b64) if snakebeta else fa                               # beta'
    d_fa = fa if logscale else torch.ones_like(fa)                                           # d alpha' / d raw alpha
    d_fb = (b64.exp() if logscale else torch.ones_like(b64)) if snakebeta else d_fa
    through_beta = -gi / (fb + 1e-9) ** 2 * d_fb
    if snakebeta:
        want_a, want_b = ga * d_fa, through_beta
        assert float((b.grad.double() - want_b).abs().max()) <= 1e-6 * float(want_b.abs().max())
    else:
        want_a = ga * d_fa + through_beta                                                    # alpha collects both paths
    assert float((a.grad.double() - want_a).abs().max()) <= 1e-6 * float(want_a.abs().max())


# ---- ABI --------------------------------------------------------------------------------------------------------------------

def _lib():
    from daft_exprt import _hip as H
    if not os.path.exists(H.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return H, H.lib()


def test_library_exports_the_backward():
    H, lib = _lib()
    protos = {name: args for name, _, args in H.header_prototypes()}
    for name, arity in (('dx_vocoder_snake_bwd', 18), ('dx_vocoder_snake_bwd_workspace', 3), ('dx_vocoder_snake_bwd_tile_rows', 1)):
        assert name in protos and hasattr(lib, name)
        assert len(protos[name]) == arity, (name, len(protos[name]))
    assert lib.dx_abi_version() == 13
    heights = []
    while lib.dx_vocoder_snake_bwd_tile_rows(len(heights)) > 0:
        heights.append(lib.dx_vocoder_snake_bwd_tile_rows(len(heights)))
    assert len(heights) >= 2 and heights == sorted(set(heights)) and min(heights) >= 12
    assert lib.dx_vocoder_snake_bwd_tile_rows(len(heights)) == 0 and lib.dx_vocoder_snake_bwd_tile_rows(len(heights) + 7) == 0
    assert lib.dx_vocoder_snake_bwd_tile_rows(-1) == 0
    assert lib.dx_vocoder_snake_bwd_workspace(0, 100, 32) == 0
    small, large = lib.dx_vocoder_snake_bwd_workspace(2, 100, 32), lib.dx_vocoder_snake_bwd_workspace(3, 1000, 64)
    assert 0 < small < large
    # one partial per (utterance, tile, channel) and sum, at the smallest height (the most tiles)
    assert small >= 2 * -(-100 // heights[0]) * 32 * 2 * 4


def test_every_refusal_comes_before_a_launch():
    ''' the pointers are made-up addresses: a launch would fault, a refusal returns its code and message '''
    _, lib = _lib()
    taps = (ctypes.c_float * 24)()
    f = ctypes.addressof(taps)
    h0 = lib.dx_vocoder_snake_bwd_tile_rows(0)
    X, DY, A, IB, DX, DA, DB, WS, NR = 0x1000, 0x2000, 0x3000, 0x3100, 0x4000, 0x5000, 0x5100, 0x6000, 0x7000

    def call(x=X, ldx=32, dy=DY, lddy=32, alpha=A, inv_beta=IB, filters=f, dx=DX, lddx=32, da=DA, db=DB, ws=WS, n=NR, B=1, N=8, C=32,
             tile_rows=0):
        rc = lib.dx_vocoder_snake_bwd(x, ldx, dy, lddy, alpha, inv_beta, filters, dx, lddx, da, db, ws, n, B, N, C, tile_rows, None)
        return rc, lib.dx_last_error()
    for name in ('x', 'dy', 'alpha', 'inv_beta', 'filters', 'dx', 'n'):
        rc, msg = call(**{name: None})
        assert rc == -1 and b'null' in msg, (name, rc, msg)
    for kw in (dict(da=None), dict(db=None)):
        rc, msg = call(**kw)
        assert rc == -1 and b'both' in msg, (kw, rc, msg)
    rc, msg = call(ws=None)
    assert rc == -1 and b'workspace' in msg
    for kw in (dict(B=0), dict(N=0), dict(C=0), dict(B=-1)):
        rc, msg = call(**kw)
        assert rc == -2 and b'bad shape' in msg, (kw, rc, msg)
    for name in ('ldx', 'lddy', 'lddx'):
        rc, msg = call(**{name: 16})
        assert rc == -2 and name.encode() in msg, (name, rc, msg)
        rc, msg = call(**{name: 34})
        assert rc != 0 and b'multiples of 4' in msg, (name, rc, msg)
    rc, msg = call(C=30)
    assert rc != 0 and b'multiples of 4' in msg
    for name in ('x', 'dy', 'dx', 'alpha', 'inv_beta', 'ws'):
        rc, msg = call(**{name: 0x8004})
        assert rc == -1 and b'aligned' in msg, (name, rc, msg)
    for kw in (dict(dx=X), dict(dx=DY)):
        rc, msg = call(**kw)
        assert rc == -1 and b'alias' in msg, (kw, rc, msg)
    for bad in (h0 + 1, 7, -32):
        rc, msg = call(tile_rows=bad)
        assert rc != 0 and b'tile_rows' in msg, (bad, rc, msg)
    rc, msg = call(B=60000, N=2 ** 31 - 1)
    assert rc != 0 and b'grid' in msg


# ---- the trainable generator, on the CPU ----------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def made():
    mel = O.make_mel(BIG, LENGTHS, seed=1)
    return BO.make_weights(BIG, mel, LENGTHS, seed=1)


@pytest.fixture
def V(monkeypatch):
    ''' `daft_exprt.vocoder` with the upload stubbed out, as in test_bigvgan_host.py '''
    from daft_exprt import vocoder
    monkeypatch.setattr(vocoder.H, 'device', lambda device=None: torch.device('cpu'))
    return vocoder


def test_dispatch_returns_the_class_of_the_family(made):
    from daft_exprt import bigvgan_train as BT
    from daft_exprt import vocoder_train as VT
    weights, raw, _, filters = made
    big = VT.trainable_generator(BIG, BO.state_dict(BIG, weights, raw, filters, form='weight_norm'))
    assert type(big) is BT.TrainableBigVGAN and big.compute_dtype == 'fp32'
    cfg = dict(O.SMALL, upsample_initial_channel=128)
    hifi_weights = O.make_weights(cfg, O.make_mel(cfg, LENGTHS, seed=1), LENGTHS, seed=1)
    hifi = VT.trainable_generator(cfg, O.state_dict(hifi_weights, 'weight_norm'), compute_dtype='bf16')
    assert type(hifi) is VT.TrainableGenerator and hifi.compute_dtype == 'bf16'
    assert VT.trainable_config(BIG) == 'bigvgan' and VT.trainable_config(cfg) == 'hifi-gan'
    with pytest.raises(ValueError, match='activation'):
        BT.TrainableBigVGAN(cfg, O.state_dict(hifi_weights, 'weight_norm'))
    # a HiFi-GAN generator keeps its parameters
    assert sorted(k for k, _ in hifi.named_parameters()) == sorted(
        f'{name}.{p}' for name, _, _, _ in O.layer_shapes(cfg) for p in ('weight_g', 'weight_v', 'bias'))


@pytest.mark.parametrize('with_filters', [False, True])
@pytest.mark.parametrize('nested', [False, True])
def test_state_dict_is_the_sources(made, nested, with_filters, V):
    from daft_exprt import vocoder_train as VT
    weights, raw, _, _ = made
    filters = (torch.arange(12.) - 3., torch.arange(12.) * 0.5 + 1.) if with_filters else None
    sd = BO.state_dict(BIG, weights, raw, filters, form='weight_norm', nested_ups=nested)
    gen = VT.trainable_generator(BIG, sd)
    out = gen.state_dict()
    assert sorted(out) == sorted(sd)
    assert ('ups.0.0.weight_g' in out) == nested and ('activation_post.upsample.filter' in out) == with_filters
    for key in sd:
        assert out[key].dtype == sd[key].dtype and torch.equal(out[key], sd[key]), key
    names = [k for k, _ in gen.named_parameters()]
    assert 'resblocks.1.activations.3.act.alpha' in names and 'activation_post.act.beta' in names
    assert not any('filter' in k for k in names)                                              # the filters are not trained
    want = (filters[0].tolist() + filters[1].tolist()) if with_filters else torch.cat([V.kaiser_sinc_filter()] * 2).float().tolist()
    assert list(gen.activation_post.taps) == want and list(gen.resblocks[2].activations[1].taps) == want
    voc = V.Vocoder(BIG, out, compute_dtype='fp32')                                           # the inference path loads what is written
    assert voc.bigvgan and list(voc._acts['conv_post'][2]) == want
    gen.load_state_dict(out)
    one_missing = {k: v for k, v in sd.items() if k != 'resblocks.2.activations.0.act.alpha'}
    with pytest.raises(ValueError, match=r'resblocks\.2\.activations\.0\.act\.alpha'):
        VT.trainable_generator(BIG, one_missing)


def test_snake_has_no_beta_and_the_final_stage_follows_the_config(made):
    from daft_exprt import vocoder_train as VT
    weights, raw, _, _ = made
    cfg = dict(BIG, activation='snake', snake_logscale=False, use_tanh_at_final=False, use_bias_at_final=False)
    raw = {conv: (a.exp(), None) for conv, (a, _) in raw.items()}
    sd = BO.state_dict(cfg, weights, raw, None, form='weight_norm')
    assert 'conv_post.bias' not in sd and 'activation_post.act.beta' not in sd
    gen = VT.trainable_generator(cfg, sd)
    assert sorted(gen.state_dict()) == sorted(sd)
    names = [k for k, _ in gen.named_parameters()]
    assert 'conv_post.bias' not in names and not any(k.endswith('.beta') for k in names)
    assert gen.final_clamp and float(gen.conv_post.bias.abs().max()) == 0.


def test_a_48_channel_stage_is_refused_by_name(made):
    from daft_exprt import vocoder_train as VT
    cfg = dict(BIG, upsample_initial_channel=96, upsample_rates=[2, 2], upsample_kernel_sizes=[4, 4], hop_size=4)
    mel = O.make_mel(cfg, LENGTHS, seed=1)
    weights, raw, _, _ = BO.make_weights(cfg, mel, LENGTHS, seed=1)
    with pytest.raises(ValueError, match=r'"ups\.0" has 48 channels'):
        VT.trainable_generator(cfg, BO.state_dict(cfg, weights, raw, None, form='weight_norm'))
    with pytest.raises(ValueError, match=r'"ups\.0" has 48 channels'):
        VT.trainable_config(cfg)
