"""tests/pointwise_oracle.py held to account on the CPU: every closed formula against float64 autograd of an independent statement
(conv1d with padding 1, embedding, linear, relu, plain indexing) to 1e-12, with values in the padding where the convention says the
padding counts; the restated launch geometry against the constants in csrc/pointwise.hip and csrc/heads.hip, read as text; and for
every case of tests/test_gpu_pointwise.py / test_gpu_heads.py the condition, on the restated geometry, that it reaches the path it
is there for -- a later retuning fails here, not by quietly emptying a GPU case."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from tests import pointwise_oracle as O

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'ubisoft-laforge-daft-exprt_amd', 'csrc')
RTOL = 1e-12


def _rng(seed):
    return np.random.default_rng(seed)


def _f(r, *shape):
    return r.standard_normal(shape).astype(np.float32)


def _t(a, grad=True):
    return torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=grad)


def _same(a, b, what=''):
    a, b = np.asarray(a, dtype=np.float64), b.detach().numpy() if torch.is_tensor(b) else np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = max(float(np.abs(b).max()), 1e-300) if b.size else 1.
    assert float(np.abs(a - b).max()) <= RTOL * scale if b.size else True, (what, float(np.abs(a - b).max()), scale)


def _mask(lengths, B, N):
    return torch.tensor(O.row_mask(lengths, B, N), dtype=torch.float64)


# ---------------------------------------------------------------------------------------------------- oracle against autograd
@pytest.mark.parametrize('taps', [1, 3])
@pytest.mark.parametrize('nfeat', [1, 3])
@pytest.mark.parametrize('lengths', [None, [9, 4, 0]])
def test_scalar_embed_equals_conv1d_autograd(taps, nfeat, lengths):
    ''' the features hold values at and behind the length: row len - 1 sees the feature at len through its third tap, in the
        forward and in dw '''
    r = _rng(taps + 10 * nfeat)
    B, N, C = 3, 9, 128
    feats = [_f(r, B, N) for _ in range(nfeat)]
    ws, bs = [_f(r, C, 1, taps) for _ in range(nfeat)], [_f(r, C) for _ in range(nfeat)]
    base, pos, dout = _f(r, B, N, C), _f(r, N + 3, C), _f(r, B, N, C)
    tw, tb, tbase = [_t(w) for w in ws], [_t(b) for b in bs], _t(base)
    y = tbase + _t(pos, False)[:N]
    for x, w, b in zip(feats, tw, tb):
        y = y + Fn.conv1d(_t(x, False)[:, None, :], w, b, padding=taps // 2).transpose(1, 2)
    y = y * _mask(lengths, B, N)[:, :, None]
    out, bound = O.scalar_embed_fwd(feats, ws, bs, base, pos, lengths)
    _same(out, y, 'out')
    assert (bound >= 0).all() and (lengths is None or not bound[1, 4:].any())
    y.backward(_t(dout, False))
    res = O.scalar_embed_bwd(dout, feats, taps, lengths)
    _same(res.dbase, tbase.grad, 'dbase')
    for f in range(nfeat):
        _same(res.dw[f], tw[f].grad, 'dw'); _same(res.dbias[f], tb[f].grad, 'dbias')
    rows = {(b, n): dout[b, n] for b in range(B) for n in range(N)}
    dw, db, aw, ab, live = O.scalar_embed_bwd_sparse(rows, feats, taps, lengths, B, N)
    for f in range(nfeat):
        _same(dw[f], res.dw[f], 'sparse dw'); _same(db[f], res.dbias[f], 'sparse dbias'); _same(aw[f], res.aw[f], 'sparse aw')
    assert len(live) == (B * N if lengths is None else sum(lengths))


def test_embed_pos_and_gather_add_equal_embedding_autograd():
    r = _rng(3)
    B, N, V, C = 3, 7, 11, 128
    ids = r.integers(0, V, (B, N))
    ids[0, :3], ids[2, 5] = 0, V - 1                        # behind the length of utterance 2
    lengths = [7, 0, 4]
    table, pos, dout = _f(r, V, C), _f(r, N + 2, C), _f(r, B, N, C)
    tt = _t(table)
    y = (Fn.embedding(torch.tensor(ids), tt) + _t(pos, False)[:N]) * _mask(lengths, B, N)[:, :, None]
    _same(O.embed_pos_fwd(ids, table, pos, lengths), y)
    assert np.array_equal(O.embed_pos_fwd32(ids, table, pos, lengths), O.embed_pos_fwd(ids, table, pos, lengths).astype(np.float32))
    y.backward(_t(dout, False))
    con, mag, cnt = O.scatter_rows(ids, dout, V, O.row_mask(lengths, B, N))
    _same(con, tt.grad)
    assert cnt.sum() == 11 and cnt[V - 1] == int((ids[0] == V - 1).sum() + (ids[2, :4] == V - 1).sum()) and (mag >= np.abs(con) - 1e-12).all()
    a, sid = _f(r, 5, C), np.array([2, 0, 2, 2, 4])
    ta, tt = _t(a), _t(table)
    z = ta + tt[torch.tensor(sid)]
    _same(O.gather_add_fwd32(a, table, sid), z.detach().numpy().astype(np.float32))
    z.backward(_t(dout[0, :5], False))
    con, mag, cnt = O.scatter_rows(sid, dout[0, :5], V)
    _same(con, tt.grad)
    assert list(cnt[:5]) == [1, 0, 3, 0, 1]


def test_masked_mean_ignores_the_padding_forward_and_fills_it_backward():
    r = _rng(4)
    B, N, C = 4, 9, 128
    lengths = [9, 0, 1, 5]
    x, dy = _f(r, B, N, C), _f(r, B, C)
    tx = _t(x)
    ln = torch.tensor(lengths, dtype=torch.float64).clamp_min(1.)[:, None]
    y = (tx * _mask(lengths, B, N)[:, :, None]).sum(1) / ln
    out, bound = O.masked_mean_fwd(x, lengths)
    _same(out, y)
    assert not out[1].any() and not bound[1].any()
    x_nan = x.copy()
    for b, n in enumerate(lengths):
        x_nan[b, n:] = np.nan
    assert np.array_equal(O.masked_mean_fwd(x_nan, lengths)[0], out)            # rows at or behind the length are not read
    # backward, as the reference has it: the sum runs over ALL N rows (zero padding), so every row receives dy / len
    tz = _t(x)
    (tz.sum(1) / ln).backward(_t(dy, False))
    want = tz.grad.numpy().copy()
    want[1] = 0.                                                                 # the zero-length utterance: gradient 0 by convention
    _same(O.masked_mean_bwd(dy, lengths, N), want)
    # the fp32 statement is the float64 quotient rounded once (53 >= 2 * 24 + 2 bits: the double rounding of a quotient is innocuous)
    assert np.array_equal(O.masked_mean_bwd32(dy, lengths, N), O.masked_mean_bwd(dy, lengths, N).astype(np.float32))


def _film_torch(g, b, post, nb, ch):
    films, c0, k0 = [], 0, 0
    nblk = sum(nb)
    B = g.shape[0]
    for m in range(3):
        w = nb[m] * ch[m]
        gm, bm = g[:, c0:c0 + w].reshape(B, nb[m], ch[m]), b[:, c0:c0 + w].reshape(B, nb[m], ch[m])
        if post is not None:
            gm = gm * post[0, k0:k0 + nb[m]][None, :, None]
            bm = bm * post[1, k0:k0 + nb[m]][None, :, None]
        films.append(torch.cat([gm + 1., bm], dim=2))
        c0 += w; k0 += nb[m]
    return films


@pytest.mark.parametrize('layout', [O.MODEL_LAYOUT, O.ODD_LAYOUT])
@pytest.mark.parametrize('with_post', [False, True])
def test_film_assembly_equals_autograd(layout, with_post):
    nb, ch = layout
    r = _rng(5)
    B, W, nblk = 3, O.film_width(nb, ch), sum(nb)
    g, b = _f(r, B, W), _f(r, B, W)
    post = _f(r, 2, nblk) if with_post else None
    dfilms = [_f(r, B, nb[m], 2 * ch[m]) for m in range(3)]
    tg, tb, tp = _t(g), _t(b), (_t(post) if with_post else None)
    films = _film_torch(tg, tb, tp, nb, ch)
    got, bounds = O.film_assemble_fwd(g, b, post, nb, ch)
    for m in range(3):
        _same(got[m], films[m]); assert got[m].shape == bounds[m].shape and (bounds[m] >= 0).all()
    sum((f * _t(df, False)).sum() for f, df in zip(films, dfilms)).backward()
    res = O.film_assemble_bwd(g, b, post, dfilms, nb, ch)
    _same(res.dg_raw, tg.grad); _same(res.db_raw, tb.grad)
    if with_post:
        _same(res.dpost, tp.grad)
        f32 = O.film_assemble_fwd32(g, b, post, nb, ch)
        assert all(np.array_equal(f32[m][:, :, ch[m]:], got[m][:, :, ch[m]:].astype(np.float32)) for m in range(3))
    else:
        assert res.dpost is None
        f32 = O.film_assemble_fwd32(g, b, None, nb, ch)
        assert all(np.array_equal(f32[m], got[m].astype(np.float32)) for m in range(3))


@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('lengths', [None, [7, 0, 3, 1]])
def test_masked_linear_equals_autograd(relu, lengths):
    ''' x and dy hold non-zero values on the masked rows: they must reach neither dw nor db nor dx '''
    r = _rng(6)
    B, N, K, Oo = 4, 7, 16, 3
    x, w, bias, dy = _f(r, B, N, K), _f(r, Oo, K), _f(r, Oo), _f(r, B, N, Oo)
    tx, tw, tb = _t(x), _t(w), _t(bias)
    y = Fn.linear(tx, tw, tb)
    y = (Fn.relu(y) if relu else y) * _mask(lengths, B, N)[:, :, None]
    got, bound = O.linear_small_fwd(x, w, bias, relu, lengths, N)
    _same(got, y.reshape(B * N, Oo))
    (-0.5 * (y * _t(dy, False)).sum()).backward()            # dx_scale reaches dx alone; dw and db are unscaled
    res = O.linear_small_bwd(dy, got, x, w, relu, lengths, N, dx_scale=-0.5)
    _same(res.dx, tx.grad.reshape(B * N, K))
    _same(-0.5 * res.dw, tw.grad); _same(-0.5 * res.db, tb.grad)
    if lengths is not None:
        m = O.row_mask(lengths, B, N).reshape(-1)
        assert not got[~m].any() and not bound[~m].any() and not res.dx[~m].any() and np.abs(dy.reshape(B * N, Oo)[~m]).min() > 0


@pytest.mark.parametrize('layout', [O.MODEL_LAYOUT, O.ODD_LAYOUT])
@pytest.mark.parametrize('with_post', [False, True])
def test_film_head_equals_autograd_end_to_end(layout, with_post):
    nb, ch = layout
    r = _rng(7)
    B, V, W, nblk = 5, 6, O.film_width(nb, ch), sum(nb)
    # quarters: z = emb + spk is then exact in fp32, and the oracle (which feeds the projections the ROUNDED z) agrees with float64
    emb, spk = np.round(_f(r, B, 128) * 4) / 4, np.round(_f(r, V, 128) * 4) / 4
    ids = np.array([3, 0, 3, 5, 3])
    wg, bg, wb, bb = _f(r, W, 128), _f(r, W), _f(r, W, 128), _f(r, W)
    post = _f(r, 2, nblk) if with_post else None
    dfilms = [_f(r, B, nb[m], 2 * ch[m]) for m in range(3)]
    t = {k: _t(v) for k, v in dict(emb=emb, spk=spk, wg=wg, bg=bg, wb=wb, bb=bb).items()}
    tp = _t(post) if with_post else None
    z = t['emb'] + Fn.embedding(torch.tensor(ids), t['spk'])
    g, b = Fn.linear(z, t['wg'], t['bg']), Fn.linear(z, t['wb'], t['bb'])
    films = _film_torch(g, b, tp, nb, ch)
    fw = O.film_head_fwd(emb, spk, ids, wg, bg, wb, bb, post, nb, ch)
    _same(fw.z32, z); _same(fw.g_raw, g); _same(fw.b_raw, b)
    for m in range(3):
        _same(fw.films[m], films[m]); assert (fw.efilms[m] > 0).all()
    sum((f * _t(df, False)).sum() for f, df in zip(films, dfilms)).backward()
    bw = O.film_head_bwd(fw.g_raw, fw.b_raw, post, fw.z32, ids, wg, wb, dfilms, nb, ch, V)
    _same(bw.d_emb, t['emb'].grad); _same(bw.d_spk, t['spk'].grad)
    _same(bw.dwg, t['wg'].grad); _same(bw.dbg, t['bg'].grad); _same(bw.dwb, t['wb'].grad); _same(bw.dbb, t['bb'].grad)
    assert list(bw.share) == [1, 0, 0, 3, 0, 1] and not bw.d_spk[1].any() and not bw.a_spk[1].any()
    if with_post:
        _same(bw.dpost, tp.grad)


class _Reverse(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, lam):
        ctx.lam = lam
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return -ctx.lam * g, None


@pytest.mark.parametrize('S', [1, 10, 128])
def test_classifier_equals_autograd_with_gradient_reversal(S):
    r = _rng(8 + S)
    B, lam = 5, 0.25
    emb = _f(r, B, 128)
    w1, w2, w3 = _f(r, 128, 128) / 11, _f(r, 128, 128) / 11, _f(r, S, 128) / 11
    b1, b2, b3 = _f(r, 128), _f(r, 128), _f(r, S)
    b1[:9], b2[5:20] = -50., -50.                            # dead units in both hidden layers
    dl = _f(r, B, S)
    t = {k: _t(v) for k, v in dict(emb=emb, w1=w1, b1=b1, w2=w2, b2=b2, w3=w3, b3=b3).items()}
    h1 = Fn.relu(Fn.linear(_Reverse.apply(t['emb'], lam), t['w1'], t['b1']))
    h2 = Fn.relu(Fn.linear(h1, t['w2'], t['b2']))
    lg = Fn.linear(h2, t['w3'], t['b3'])
    fw = O.classifier_fwd(emb, w1, b1, w2, b2, w3, b3)
    _same(fw.h1, h1); _same(fw.h2, h2); _same(fw.logits, lg)
    assert not fw.h1[:, :9].any() and not fw.h2[:, 5:20].any() and (fw.e2 >= fw.e1.min()).all()
    lg.backward(_t(dl, False))
    bw = O.classifier_bwd(dl, emb, fw.h1, fw.h2, w1, w2, w3, lam)
    _same(bw.d_emb, t['emb'].grad)
    for i, k in enumerate('123'):
        _same(bw.dw[i], t['w' + k].grad); _same(bw.db[i], t['b' + k].grad)
    assert not bw.g1[:, :9].any() and not bw.g2[:, 5:20].any() and not bw.dw[0][:9].any() and not bw.db[1][5:20].any()
    # the sign: with lambda > 0 the embedding's gradient is MINUS lambda times the plain one
    plain = O.classifier_bwd(dl, emb, fw.h1, fw.h2, w1, w2, w3, -1.)
    _same(bw.d_emb, -lam * plain.d_emb)


# ---------------------------------------------------------------------------------------------------- geometry against the source
def _src(name):
    return open(os.path.join(SRC, name)).read()


def _find(text, pattern):
    m = re.search(pattern, text)
    assert m, f'the kernel source no longer states this in the form the test reads: {pattern}'
    return tuple(int(x) for x in m.groups())


def test_restated_geometry_equals_the_kernel_source():
    pw, hd = _src('pointwise.hip'), _src('heads.hip')
    assert _find(pw, r'constexpr int SE_MAX_ROWS = (\d+);') == (O.SE_MAX_ROWS,)
    assert _find(pw, r'int rpb = (\d+);\s*while \(rpb < (\d+) && \(long\)dx_cdiv\(N, rpb\) \* B > (\d+)\) rpb \*= 2;') == (64, O.SE_MAX_ROWS, O.SE_WG_TARGET)
    assert _find(pw, r'__shared__ float red\[(\d+)\]\[3\]\[4\]\[C128\];') == (8,)
    assert _find(pw, r'for \(int n = n0 \+ q; n < n1; n \+= (\d+)\)') == (8,)
    assert _find(pw, r'for \(int n = q; n < n1; n \+= (\d+)\) acc \+= p') == (8,)
    assert _find(pw, r'const bool few_rows = !mask_lengths && M <= (\d+);') == (O.LS_FEW_ROWS,)
    assert _find(pw, r'const int chunks = \(O > (\d+) && M \* K < \(1L << (\d+)\)\) \? dx_cdiv\(O, (\d+)\) : 1;') == (O.LS_DX_OCHUNK, 18, O.LS_DX_OCHUNK)
    assert O.LS_DX_SMALL == 1 << 18
    assert _find(pw, r'int rpc = (\d+);\s*while \(rpc < (\d+) && \(M \+ rpc - 1\) / rpc > (\d+)\) rpc \*= 2;') == (64, O.LS_RPC_MAX, O.LS_CHUNK_TARGET)
    assert _find(pw, r'for \(; m \+ 3 < m1; m \+= (\d+)\)') == (4,)
    assert _find(pw, r'constexpr int LT = (\d+), LR = (\d+);') == (O.LT, O.LR)
    assert _find(pw, r'inline int grid_for\(long total, int block = (\d+), int cap = (\d+)\)') == (256, O.GRID_CAP)
    assert _find(pw, r'int rpb = (\d+);\s*while \(rpb < (\d+) && \(rows \+ rpb - 1\) / rpb > (\d+)\) rpb \*= 2;') == (64, O.COLSUM_RPB_MAX, O.COLSUM_BLOCK_TARGET)
    assert _find(pw, r'constexpr int C128 = (\d+);') == (O.C128,)
    assert _find(hd, r'constexpr int HD = (\d+);') == (O.HD,)
    assert _find(hd, r'film_head_bwd_dx_kernel, dim3\(dx_cdiv\(W, (\d+)\), B\), dim3\((\d+)\)') == (128, 128)
    assert _find(hd, r'for \(; b \+ 1 < a\.B; b \+= (\d+)\)') == (2,)
    # the functions at hand-computed points
    assert [O.se_rows_per_block(*s) for s in ((2, 70), (2, 64), (1, 1), (100, 300), (257, 1025), (48, 700))] == [64, 64, 64, 256, 1024, 256]
    assert O.se_slabs(2, 70) == [(0, 64), (64, 70)] and O.se_slabs(100, 300) == [(0, 256), (256, 300)] and O.se_slabs(257, 1025) == [(0, 1024), (1024, 1025)]
    assert O.ls_chunks(165, 128, 17) == (2, 9) and O.ls_chunks(165, 128, 16) == (1, 16) and O.ls_chunks(48, 128, 1280) == (80, 16)
    assert O.ls_chunks(4096, 64, 17) == (1, 17)
    assert O.ls_rows_per_chunk(165) == 64 and O.ls_rows_per_chunk(256 * 64 + 1) == 128 and O.ls_chunk_seams(165) == [64, 128]
    assert O.colsum_rows_per_block(700) == 64 and O.colsum_rows_per_block(512 * 64 + 1) == 128


def test_model_layout_is_what_the_model_builds():
    from daft_exprt.model import film_layout
    from tests.util import make_hparams
    lay = film_layout(make_hparams())
    assert (tuple(n for n, _ in lay), tuple(c for _, c in lay)) == O.MODEL_LAYOUT


# ---------------------------------------------------------------------------------------------------- each case reaches what it is for
def test_each_scalar_embed_case_reaches_what_it_is_for():
    assert (3 * 7) % 2 == 1                                                         # the last forward workgroup (2 rows) is half empty
    assert O.SE_FWD_SHAPES[(3, 70)] == [70, 33, 0] and 0 in O.SE_FWD_SHAPES[(3, 7)]
    assert O.se_fwd_terms(3, 3, True, True) == 3 * 4 + 2
    assert O.se_rows_per_block(2, 70) == 64 and O.se_slabs(2, 70)[1] == (64, 70)        # a second slab of 6 rows
    assert O.se_slabs(2, 64) == [(0, 64)] and O.se_slabs(1, 1) == [(0, 1)]               # exactly one slab; one row
    assert O.se_rows_per_block(100, 300) == 256 and [b - a for a, b in O.se_slabs(100, 300)] == [256, 44]
    assert O.se_rows_per_block(*O.SE_BWD_BIG) == O.SE_MAX_ROWS and [b - a for a, b in O.se_slabs(*O.SE_BWD_BIG)] == [1024, 1]
    for B, N in O.SE_BWD_SHAPES + [O.SE_BWD_BIG]:
        rag = O.se_lengths(B, N, 'ragged')
        assert len(rag) == B and rag[0] == N and (B < 3 or 0 in rag) and all(0 <= x <= N for x in rag)
        imp = O.se_impulses(B, N)
        slabs = O.se_slabs(B, N)
        whats = {w for _, _, _, w in imp}
        assert {'row 0', 'row N - 1'} <= whats and all(abs(n - j) <= 1 for _, n, j, _ in imp)
        if len(slabs) > 1:           # both sides of every seam: the halo row lies in the NEIGHBOURING slab
            assert any(n == slabs[1][0] and j == n - 1 for _, n, j, _ in imp) and any(n == slabs[0][1] - 1 and j == n + 1 for _, n, j, _ in imp)
    assert O.se_bwd_chain(2, 70) == 8 + 1 + 3 + 4 and O.se_bwd_chain(*O.SE_BWD_BIG) == 128 + 1 + 3 + 2 * 257


def test_each_embedding_and_mean_case_reaches_what_it_is_for():
    assert O.EMBED_SHAPES[(3, 7)] == [7, 0, 4] and (3 * 7) % 2 == 1
    assert set(O.MEAN_N) >= {1, 7, 8, 9} and max(O.MEAN_N) > 64                  # below, at and above the 8 row lanes; 9 trips
    assert O.mean_chain(70) == 9 + 8 + 1 and O.mean_chain(0) == 9 and O.mean_chain(8) == 1 + 9


def test_each_film_case_reaches_what_it_is_for():
    for B in (1, 5):
        land, uniform, lanes = O.film_landings(*O.MODEL_LAYOUT, B)
        assert lanes == 0 and uniform == B * 1280 // 64 and (land == np.array([2] * 4 + [4] + [2] * 4) * B).all()     # wave reductions only
        land, uniform, lanes = O.film_landings(*O.ODD_LAYOUT, B)
        assert lanes > 0 and uniform > 0 and land.sum() == uniform + lanes           # both branches, the per-lane one nothing else runs
        land, uniform, lanes = O.head_landings(*O.ODD_LAYOUT, B)
        assert lanes > 0 and uniform > 0
        assert O.head_landings(*O.MODEL_LAYOUT, B)[2] == 0
    W = O.film_width(*O.ODD_LAYOUT)
    assert W == 560 and W % 64 and W % 128 and W % 256 and all(c % 64 for c in O.ODD_LAYOUT[1][:2])
    key = O.film_keys(*O.ODD_LAYOUT)[3]
    assert len(set(key[:64])) == 2 and key[-1] == 5 and len(set(key)) == 6          # the first wave spans two blocks
    # the last wave of the last utterance of the flat kernel is partly dead (B W % 64 != 0), and so is the heads' last workgroup
    assert (5 * W) % 64 and O.cdiv(W, 128) * 128 - W == 80
    assert O.film_width(*O.MODEL_LAYOUT) == 1280


def test_each_linear_case_reaches_what_it_is_for():
    (B, N, K, Oo), lens = list(O.LS_MASKED.items())[0]
    assert (B, N, K, Oo) == (4, 7, 256, 3) and lens == [7, 0, 3, 1] and not O.ls_few_rows(B * N, True) and O.ls_chunks(B * N, K, Oo)[0] == 1
    for (B, N, K, Oo), lens in list(O.LS_MASKED.items())[1:]:
        M = B * N
        seams = O.ls_chunk_seams(M)
        assert M == 165 and len(seams) == 2 and all(s % N for s in seams)                       # three chunks, seams inside utterances
        assert all(s % N < lens[s // N] for s in seams)                                         # ... and inside their valid part
        assert (M - seams[-1]) == 37 and 37 // 4 == 9 and 37 % 4 == 1                           # 9 quads + 1 tail row
        assert 0 in lens and lens[0] < N                                                        # an utterance seam with a new length inside chunk 0
        assert not O.ls_few_rows(M, True)
    assert O.ls_chunks(165, 128, 17) == (2, 9) and 2 * 9 > 17                                   # chunks == 2; the last chunk is short (the `min`)
    assert O.ls_chunks(165, 128, 1)[0] == 1
    (M1, K1, O1), (M2, K2, O2) = O.LS_PLAIN
    assert M1 == O.LS_FEW_ROWS + 1 and not O.ls_few_rows(M1, False) and O.ls_few_rows(M2, False)     # generic dw kernel, not the LDS-tiled one
    assert M1 % 64 == 1 and O.ls_rows_per_chunk(M1) == 64                                       # a last chunk of one row
    assert M2 == O.LS_FEW_ROWS and K2 % O.LT and O2 % O.LT and K2 > 2 * O.LT and O2 > O.LT and K2 % 4 == 0   # ragged 64-tiles both ways
    assert O.ls_chunks(M2, K2, O2) == (5, 14) and M2 % O.LR == 0
    assert O.ls_dw_chain(M2, False) == 514 and O.ls_dw_chain(M1, False) == 16 + 3 + 1 + 2 + 9


def test_each_layout_helper_case_reaches_what_it_is_for():
    shapes = O.TRANSPOSE_SHAPES
    assert (2, 1, 1) in shapes and any(R % 32 and C % 32 and R > 32 for _, R, C in shapes) and any(R % 32 == 0 and C % 32 == 0 for _, R, C in shapes)
    assert any(R > 64 and C > 64 for _, R, C in shapes)                                          # more than two tiles both ways
    assert set(O.COLSUM_ROWS) >= {1, 64, 65} and O.cdiv(700, O.colsum_rows_per_block(700)) == 11 and 300 in O.COLSUM_C   # two column workgroups
    assert O.FILL_OFFSETS == tuple(range(17)) and set(O.FILL_COUNTS) >= {0, 1, 15, 16, 17, 31} and (max(O.FILL_COUNTS) // 16 + 255) // 256 == 3   # three workgroups


def test_each_heads_case_reaches_what_it_is_for():
    assert any(B % 2 for B in O.HEAD_B if B > 1) and 1 in O.HEAD_B and 2 in O.HEAD_B     # the odd tail row after a pair; alone; no tail
    assert O.heads_dw_chain(5) == 3 + 1 + 2 + 1 and O.heads_dw_chain(1) == 1 + 1 + 2 + 1
    assert O.head_dx_chain(560) == 256 + 2 + 5 and O.head_dx_chain(1280, 3) == 256 + 2 + 30
    assert set(O.CLS_S) == {1, 10, 127, 128} and max(O.CLS_S) == O.HD
