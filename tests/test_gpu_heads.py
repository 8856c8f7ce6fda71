"""The FiLM head and the speaker classifier as fused launches (`dx_film_head_fwd / _bwd`, `dx_classifier_fwd / _bwd`) against the chain of
small launches they replace (gather_add, linear_small, film_assemble and their backward counterparts, each pinned against the reference
in test_gpu_model / test_gpu_parity_at_size): same forward values bit for bit (same summation order), gradients equal up to the fp32
summation order of the backward reductions.  Reference: model.py:27-54, 276-292 (classifier + gradient reversal), 419-462 (FiLM)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _run(fused, speakers, mode='fp32', B=6):
    from daft_exprt import ops
    from daft_exprt.data_loader import synthetic_batch
    from daft_exprt.model import DaftExprt
    from tests.util import make_hparams, no_dropout
    hp = no_dropout(make_hparams(compute_dtype=mode, batch_size=B, speakers=speakers))
    torch.manual_seed(5)
    model = DaftExprt(hp).to(DEV).train()
    cb = synthetic_batch(hp, B, seed=77, t_max=180, force_first_full=True, l_range=(6, 24))
    inputs, targets, _ = model.parse_batch(DEV, cb)
    old = ops.USE_FUSED_HEADS
    ops.USE_FUSED_HEADS = fused
    try:
        model.zero_grad()
        terms = model.forward_backward(inputs, targets, (1e-2, 1e-3, 1., 1., 1., 1.))
        torch.cuda.synchronize()
    finally:
        ops.USE_FUSED_HEADS = old
    logits, films, _, mel, _ = model.last_outputs
    return terms.clone(), logits.clone(), [f.clone() for f in films], mel.clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters()}


@pytest.mark.parametrize('speakers', [[f'spk{i:02d}' for i in range(11)], ['LJ']])
def test_fused_heads_match_the_separate_launches(speakers):
    t0, l0, f0, m0, g0 = _run(False, speakers)
    t1, l1, f1, m1, g1 = _run(True, speakers)
    assert torch.equal(l0, l1) and all(torch.equal(a, b) for a, b in zip(f0, f1)) and torch.equal(m0, m1)       # forward: bit-identical
    assert torch.allclose(t0, t1, rtol=1e-6, atol=1e-7)
    gmax = max(float(g.abs().max()) for g in g0.values())
    for n in g0:
        err = float((g0[n] - g1[n]).abs().max())
        assert err <= 2e-5 * float(g0[n].abs().max()) + 2e-7 * gmax, (n, err, float(g0[n].abs().max()))
    touched = [n for n in g0 if n.startswith(('speaker_classifier', 'prosody_encoder.gammas', 'prosody_encoder.betas', 'prosody_encoder.spk_embedding',
                                              'prosody_encoder.post_multipliers'))]
    assert len(touched) == 12 and all(float(g1[n].abs().max()) > 0. for n in touched if 'classifier' not in n or len(speakers) > 1)


def test_more_speakers_than_the_fused_classifier_holds():
    ''' n_speakers - 1 > 128 logits do not fit the one-launch classifier's 128-wide tile: the model then takes the
        `linear_small_*` launches instead of raising, and the logits are those of the plain three-layer MLP (model.py:276-292) '''
    speakers = [f'spk{i:03d}' for i in range(140)]
    t1, l1, f1, m1, g1 = _run(True, speakers)
    assert l1.shape == (6, 140) and bool(torch.isfinite(t1).all())
    from daft_exprt.model import DaftExprt
    from tests.util import make_hparams, no_dropout
    hp = no_dropout(make_hparams(compute_dtype='fp32', batch_size=6, speakers=speakers))
    torch.manual_seed(5)
    model = DaftExprt(hp).to(DEV).train()
    assert not model._fused_classifier()
    for n in ('1', '3', '5'):
        assert float(g1[f'speaker_classifier.classifier.{n}.linear_layer.weight'].abs().max()) > 0.


# ---------------------------------------------------------------------------------------------------- the heads alone, against float64
# `dx_film_head_*` and `dx_classifier_*` against tests/pointwise_oracle.py (conventions and bounds in its docstring; each case's purpose
# is held in tests/test_pointwise_host.py).  No literal tolerance: bit for bit, or a bound the oracle returns.  Outputs `ops` allocates
# start as NaN (config.POISON), accumulated outputs start from random values.
import numpy as np

from tests import pointwise_oracle as O

F = np.float32


@pytest.fixture
def poison():
    from daft_exprt import config
    old = config.POISON
    config.POISON = True
    yield
    config.POISON = old


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _host(t):
    return t.detach().cpu().numpy()


def _f(r, *shape):
    return r.standard_normal(shape).astype(F)


def _within(kernel, what, got, ref, bound):
    got = _host(got).astype(np.float64) if torch.is_tensor(got) else np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    bound = np.asarray(bound, dtype=np.float64) + 0. * ref
    assert got.shape == ref.shape and np.isfinite(got).all(), (kernel, what, got.shape, ref.shape)
    err = np.abs(got - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(err == 0, 0., err / bound)
    w = float(ratio.max()) if ratio.size else 0.
    print(f'  RATIO {kernel} | {what}: {w:.3g}')
    assert w <= 1., (kernel, what, w, float(err.max()))


@pytest.mark.parametrize('with_post', [False, True])
@pytest.mark.parametrize('B', O.HEAD_B)
@pytest.mark.parametrize('layout', [O.MODEL_LAYOUT, O.ODD_LAYOUT], ids=['model', 'odd'])
def test_film_head_alone_against_float64(layout, B, with_post, poison):
    ''' speaker ids with a repeat (d_spk_table rows collide) and a table row nobody names; an odd B reaches the tail row of heads_dw_kernel;
        the odd layout the per-lane atomics of dpost and a last workgroup of 48 columns '''
    from daft_exprt import ops
    nb, ch = layout
    W, nblk, V = O.film_width(nb, ch), sum(nb), 7
    r = np.random.default_rng([W, B, 11])
    ids = np.array([3, 0, 3, 5, 3][:B])
    emb, spk = _f(r, B, 128), _f(r, V, 128)
    wg, bg, wb, bb = _f(r, W, 128) / F(11.), _f(r, W), _f(r, W, 128) / F(11.), _f(r, W)
    post = (_f(r, 2, nblk) + np.arange(2 * nblk, dtype=F).reshape(2, nblk)) if with_post else None
    dfilms = [_f(r, B, nb[m], 2 * ch[m]) for m in range(3)]
    tag = f'W {W} B {B} post {with_post}'
    d = {k: _dev(v) for k, v in dict(emb=emb, spk=spk, ids=ids.astype(np.int64), wg=wg, bg=bg, wb=wb, bb=bb, post=post).items()}
    z, g_raw, b_raw, films = ops.film_head_fwd(d['emb'], d['spk'], d['ids'], d['wg'], d['bg'], d['wb'], d['bb'], d['post'], nb, ch)
    fw = O.film_head_fwd(emb, spk, ids, wg, bg, wb, bb, post, nb, ch)
    assert np.array_equal(_host(z), fw.z32)                                     # one correctly rounded addition
    _within('film_head_fwd', 'g_raw ' + tag, g_raw, fw.g_raw, fw.eg)
    _within('film_head_fwd', 'b_raw ' + tag, b_raw, fw.b_raw, fw.eb)
    for m in range(3):
        _within('film_head_fwd', f'film {m} {tag}', films[m], fw.films[m], fw.efilms[m])
    # the source's claim, directly: bit-identical to gather_add + linear_small + film_assemble on the same inputs
    z2 = ops.gather_add_fwd(d['emb'], d['spk'], d['ids'])
    g2, b2 = ops.linear_small_fwd(z2, d['wg'], d['bg']), ops.linear_small_fwd(z2, d['wb'], d['bb'])
    films2 = ops.film_assemble_fwd(g2, b2, d['post'], nb, ch)
    assert torch.equal(z, z2) and torch.equal(g_raw, g2) and torch.equal(b_raw, b2) and all(torch.equal(a, b) for a, b in zip(films, films2))

    g_h, b_h, z_h = _host(g_raw), _host(b_raw), _host(z)
    bw = O.film_head_bwd(g_h, b_h, post, z_h, ids, wg, wb, dfilms, nb, ch, V)
    old = dict(d_emb=_f(r, B, 128), d_spk=_f(r, V, 128), dpost=_f(r, 2, nblk), dwg=_f(r, W, 128), dbg=_f(r, W), dwb=_f(r, W, 128), dbb=_f(r, W))
    o = {k: _dev(v) for k, v in old.items()}
    ops.film_head_bwd(g_raw, b_raw, d['post'], z, d['ids'], d['wg'], d['wb'], [_dev(x) for x in dfilms], o['d_emb'], o['d_spk'], o['dpost'],
                      o['dwg'], o['dbg'], o['dwb'], o['dbb'], nb, ch)
    e_emb, e_spk = O.head_dx_bounds(bw, ids, W, old['d_emb'], old['d_spk'])
    _within('film_head_bwd_dx', 'd_emb ' + tag, o['d_emb'], old['d_emb'] + bw.d_emb, e_emb)
    named = bw.share > 0
    assert named.sum() == len(set(ids)) and not named[1] and (B != 5 or bw.share[3] == 3)
    _within('film_head_bwd_dx', 'd_spk_table ' + tag, _host(o['d_spk'])[named], (old['d_spk'] + bw.d_spk)[named], e_spk[named])
    assert np.array_equal(_host(o['d_spk'])[~named], old['d_spk'][~named])      # rows nobody names keep their bits
    if with_post:
        land, uniform, lanes = O.head_landings(nb, ch, B)
        K = 1 + (6 if uniform else 0) + land
        _within('film_head_bwd_dx', 'dpost ' + tag, o['dpost'], old['dpost'] + bw.dpost, O.gamma(K)[None, :] * (np.abs(old['dpost']) + bw.apost))
    else:
        assert np.array_equal(_host(o['dpost']), old['dpost'])
    Kw = O.heads_dw_chain(B)
    for k, con, mag in (('dwg', bw.dwg, bw.awg), ('dbg', bw.dbg, bw.abg), ('dwb', bw.dwb, bw.awb), ('dbb', bw.dbb, bw.abb)):
        _within('heads_dw (FiLM)', f'{k} {tag}', o[k], old[k] + con, O.acc_bound(Kw, mag, old[k]))


@pytest.mark.parametrize('S', O.CLS_S)
@pytest.mark.parametrize('B', O.CLS_B)
def test_classifier_alone_against_float64(B, S, poison):
    ''' every layer against the oracle fed with the kernel's own previous layer; hidden units that the biases kill are exact zeros, and so
        is their gradient (the rows of dW / db keep their old bits); lambda = 0.25 checks the sign and the scale of the reversal '''
    from daft_exprt import ops
    r = np.random.default_rng([B, S, 12])
    lam = 0.25
    emb = _f(r, B, 128)
    w1, w2, w3 = _f(r, 128, 128) / F(11.), _f(r, 128, 128) / F(11.), _f(r, S, 128) / F(11.)
    b1, b2, b3 = _f(r, 128), _f(r, 128), _f(r, S)
    b1[:9], b2[5:20] = -50., -50.
    dl = _f(r, B, S)
    tag = f'B {B} S {S}'
    d = {k: _dev(v) for k, v in dict(emb=emb, w1=w1, b1=b1, w2=w2, b2=b2, w3=w3, b3=b3, dl=dl).items()}
    logits, h1, h2 = ops.classifier_fwd(d['emb'], d['w1'], d['b1'], d['w2'], d['b2'], d['w3'], d['b3'])
    h1_h, h2_h = _host(h1), _host(h2)
    fw = O.classifier_fwd(emb, w1, b1, w2, b2, w3, b3, h1_in=h1_h, h2_in=h2_h)
    _within('classifier_fwd', 'h1 ' + tag, h1, fw.h1, fw.e1)
    _within('classifier_fwd', 'h2 ' + tag, h2, fw.h2, fw.e2)
    _within('classifier_fwd', 'logits ' + tag, logits, fw.logits, fw.e3)
    assert tuple(logits.shape) == (B, S) and not h1_h[:, :9].any() and not h2_h[:, 5:20].any() and (h1_h >= 0).all() and (h2_h >= 0).all()
    assert (h1_h[:, 9:] > 0).any() and (h2_h[:, 20:] > 0).any()

    bw = O.classifier_bwd(dl, emb, h1_h, h2_h, w1, w2, w3, lam)
    names = ('dw1', 'db1', 'dw2', 'db2', 'dw3', 'db3')
    old = dict(dw1=_f(r, 128, 128), db1=_f(r, 128), dw2=_f(r, 128, 128), db2=_f(r, 128), dw3=_f(r, S, 128), db3=_f(r, S))
    o = {k: _dev(v) for k, v in old.items()}
    d_emb = ops.classifier_bwd(d['dl'], d['emb'], h1, h2, d['w1'], d['w2'], d['w3'], lam, *[o[k] for k in names])
    _within('classifier_bwd_dx', 'd_emb ' + tag, d_emb, bw.d_emb, bw.e_emb)
    plain = (bw.g1 @ w1.astype(np.float64))
    got = _host(d_emb).astype(np.float64)
    assert float((got * plain).sum()) < 0 and np.abs(plain).max() > 0          # MINUS lambda: against the plain gradient
    Kw = O.heads_dw_chain(B)
    for i in range(3):
        (mw, ew), (mb, eb) = bw.adw[i], bw.adb[i]
        kw, kb = names[2 * i], names[2 * i + 1]
        _within('heads_dw (classifier)', f'{kw} {tag}', o[kw], old[kw] + bw.dw[i], O.acc_bound(Kw, mw, old[kw]) + ew)
        _within('heads_dw (classifier)', f'{kb} {tag}', o[kb], old[kb] + bw.db[i], O.acc_bound(Kw, mb, old[kb]) + eb)
    # dead units: g is an exact zero, so `+=` leaves the old bits
    assert np.array_equal(_host(o['dw1'])[:9], old['dw1'][:9]) and np.array_equal(_host(o['db1'])[:9], old['db1'][:9])
    assert np.array_equal(_host(o['dw2'])[5:20], old['dw2'][5:20]) and np.array_equal(_host(o['db2'])[5:20], old['db2'][5:20])


def test_heads_refuse_bad_arguments_before_any_launch():
    from daft_exprt import _hip as H
    L = H.lib()
    whole = torch.full((1 << 16,), -1024., dtype=torch.float32, device=DEV)
    ids = torch.zeros(8, dtype=torch.int64, device=DEV)
    p, i, s = whole.data_ptr(), ids.data_ptr(), H.stream()
    import ctypes
    nb, ch = (ctypes.c_int * 3)(1, 1, 1), (ctypes.c_int * 3)(4, 4, 4)
    UNSUPPORTED = -5                                                              # DX_ERR_UNSUPPORTED
    for S in (0, 129):
        assert L.dx_classifier_fwd(p, p, p, p, p, p, p, p, p, p, 1, 128, S, s) == UNSUPPORTED and b'dx_classifier_fwd' in L.dx_last_error()
        assert L.dx_classifier_bwd(p, p, p, p, p, p, p, p, p, p, 0.25, p, p, p, p, p, p, 1, 128, S, s) == UNSUPPORTED
        assert b'dx_classifier_bwd' in L.dx_last_error()
    assert L.dx_classifier_fwd(p, p, p, p, p, p, p, p, p, p, 1, 64, 4, s) == UNSUPPORTED
    assert L.dx_film_head_fwd(p, p, i, p, p, p, p, None, p, p, p, p, p, p, nb, ch, 1, 64, s) == UNSUPPORTED and b'dx_film_head_fwd' in L.dx_last_error()
    assert L.dx_film_head_bwd(p, p, None, p, i, p, p, p, p, p, p, p, p, p, None, p, p, p, p, nb, ch, 1, 256, s) == UNSUPPORTED
    assert b'dx_film_head_bwd' in L.dx_last_error()
    torch.cuda.synchronize()
    assert bool((whole == -1024.).all())
