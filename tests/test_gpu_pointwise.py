"""The kernels of csrc/pointwise.hip, each alone, against the float64 oracle of tests/pointwise_oracle.py (its docstring has the
conventions and the derivation of every bound; tests/test_pointwise_host.py holds the oracle against float64 autograd and each case
below to its purpose).  The FiLM head and the classifier of csrc/heads.hip are in tests/test_gpu_heads.py.

There is no literal tolerance in this file: a comparison is either bit for bit (data movement, single correctly rounded operations,
masked rows, rows an atomic kernel does not address) or against a bound the oracle returns.  Every buffer `ops` allocates starts as
NaN (`config.POISON`), every accumulated output starts from random values, and every check prints its error / bound (run with -s).

What runs:
    test_scalar_embed_fwd (18)              (B, N) = (3, 7), (1, 1), (3, 70) x taps 1 / 3 x 1, 2, 3 features; base, positions and
                                            lengths each on and off; rows at or behind the length exact zeros
    test_scalar_embed_bwd (32)              (2, 70), (2, 64), (1, 1), (100, 300) x lengths none / full / ragged / zero x taps;
                                            dbase on and off; dw / dbias onto random values
    test_scalar_embed_bwd_impulses (5)      the four shapes and (257, 1025) (slabs of 1024 + 1): one dout row, the feature non-zero
                                            in one row only -- slab seams (the halo), rows 0 and N - 1, row len - 1 and row len
    test_embed_pos (2), test_gather_add (4), test_masked_mean (5), test_film_assemble (8)
    test_linear_small_masked (6), test_linear_small_unmasked (4)
    test_transpose_last2 (8), test_stack_and_unstack, test_add_inplace, test_colsum (2), test_fill_zero
    test_bad_arguments_are_refused_before_any_launch

Measured on an MI355X: 98 tests here and 21 in test_gpu_heads.py in 4.6 s together, the slowest 0.23 s (it loads the library).  Error /
bound at most 1.0 (gamma = g + 1: one rounding that attains its u), 0.99 / 0.97 for the one- and two-atomic table gradients, 0.87 for
scalar_embed_fwd, between 0.02 and 0.63 for the sums; DESIGN.md §3 has the figure per kernel and the sixteen value-only mutants that
were built to fail, with what each of them fails here.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import pointwise_oracle as O

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SENT = -1024.
F = np.float32


@pytest.fixture(autouse=True)
def _poison():
    from daft_exprt import config
    old = config.POISON
    config.POISON = True
    yield
    config.POISON = old


def _rng(*seed):
    return np.random.default_rng(list(seed))


def _f(r, *shape):
    return r.standard_normal(shape).astype(F)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def _check(kernel, what, got, ref, bound):
    ''' got (device tensor or array) within `bound` of `ref`; prints the worst error / bound (0 / 0 counts as 0) '''
    got = host(got).astype(np.float64) if torch.is_tensor(got) else np.asarray(got, dtype=np.float64)
    ref, bound = np.asarray(ref, dtype=np.float64), np.asarray(bound, dtype=np.float64) + 0. * np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (kernel, what, got.shape, ref.shape)
    assert np.isfinite(got).all(), (kernel, what, 'not finite')
    err = np.abs(got - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(err == 0, 0., err / bound)
    w = float(ratio.max()) if ratio.size else 0.
    print(f'  RATIO {kernel} | {what}: {w:.3g}')
    assert w <= 1., (kernel, what, w, float(err.max()))
    return w


def _bits(kernel, what, got, want):
    got = np.ascontiguousarray(host(got) if torch.is_tensor(got) else got)
    want = np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (kernel, what, got.shape, want.shape, got.dtype, want.dtype)
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8)) or np.array_equal(got, want), (kernel, what, int((got != want).sum()))


# ---------------------------------------------------------------------------------------------------- scalar-feature embedding
@pytest.mark.parametrize('nfeat', [1, 2, 3])
@pytest.mark.parametrize('taps', [1, 3])
@pytest.mark.parametrize('shape', list(O.SE_FWD_SHAPES))
def test_scalar_embed_fwd(shape, taps, nfeat):
    from daft_exprt import ops
    B, N = shape
    r = _rng(B, N, taps, nfeat)
    feats = [_f(r, B, N) * (f + 1) for f in range(nfeat)]           # non-zero everywhere: row len - 1 sees the feature at len
    ws, bs = [_f(r, 128, 1, taps) for _ in range(nfeat)], [_f(r, 128) for _ in range(nfeat)]
    base, pos = _f(r, B, N, 128), _f(r, N + 3, 128)
    for use_base in (False, True):
        for use_pos in (False, True):
            for lengths in (None, O.SE_FWD_SHAPES[shape]):
                args = (base if use_base else None, pos if use_pos else None, lengths)
                out = ops.scalar_embed_fwd([dev(x) for x in feats], [dev(w) for w in ws], [dev(b) for b in bs], dev(args[0]), dev(args[1]),
                                           None if lengths is None else dev(np.array(lengths, dtype=np.int64)))
                ref, bound = O.scalar_embed_fwd(feats, ws, bs, *args)
                _check('scalar_embed_fwd', f'{shape} taps {taps} nfeat {nfeat} base {use_base} pos {use_pos} lengths {lengths}', out, ref, bound)
                if lengths is not None:
                    m = O.row_mask(lengths, B, N)
                    assert not host(out)[~m].any()                   # exact zeros, +0 or -0
                    for b, ln in enumerate(lengths):                 # the third tap of row len - 1 reads the feature at len
                        assert taps == 1 or not 0 < ln < N or all(x[b, ln] != 0 for x in feats)


def _se_bwd_setup(B, N, taps, nfeat, seed):
    r = _rng(B, N, taps, seed)
    feats = [_f(r, B, N) * (f + 1) for f in range(nfeat)]
    old_w, old_b = [_f(r, 128, 1, taps) for _ in range(nfeat)], [_f(r, 128) for _ in range(nfeat)]
    return r, feats, old_w, old_b


@pytest.mark.parametrize('taps', [1, 3])
@pytest.mark.parametrize('kind', ['none', 'full', 'ragged', 'zero'])
@pytest.mark.parametrize('shape', O.SE_BWD_SHAPES)
def test_scalar_embed_bwd(shape, kind, taps):
    from daft_exprt import ops
    B, N = shape
    nfeat = 3 if taps == 3 else 2
    r, feats, old_w, old_b = _se_bwd_setup(B, N, taps, nfeat, 1)
    dout = _f(r, B, N, 128)                                          # non-zero on the masked rows too
    lengths = O.se_lengths(B, N, kind)
    res = O.scalar_embed_bwd(dout, feats, taps, lengths)
    K = O.se_bwd_chain(B, N)
    d_dout, d_feats = dev(dout), [dev(x) for x in feats]
    d_len = None if lengths is None else dev(np.array(lengths, dtype=np.int64))
    for need_dbase in (False, True):
        dws, dbs = [dev(w) for w in old_w], [dev(b) for b in old_b]
        dbase = ops.scalar_embed_bwd(d_dout, d_feats, dws, dbs, d_len, need_dbase=need_dbase)
        if need_dbase:                                               # all N rows are written: dout below the length, zeros up to N
            _bits('scalar_embed_bwd', 'dbase', dbase, res.dbase.astype(F))
        else:
            assert dbase is None
        for f in range(nfeat):
            tag = f'{shape} {kind} taps {taps} dbase {need_dbase} f {f}'
            _check('scalar_embed_bwd', 'dw ' + tag, dws[f], old_w[f].astype(np.float64) + res.dw[f], O.acc_bound(K, res.aw[f], old_w[f]))
            _check('scalar_embed_bwd', 'dbias ' + tag, dbs[f], old_b[f].astype(np.float64) + res.dbias[f], O.acc_bound(K, res.ab[f], old_b[f]))
    assert np.array_equal(host(d_dout), dout)


@pytest.mark.parametrize('shape', O.SE_BWD_SHAPES + [O.SE_BWD_BIG])
def test_scalar_embed_bwd_impulses(shape):
    ''' dout is zero but for ONE row of small integers, and every feature is zero but for ONE row (its own value there: 1, 1.5, 2): dw is
        then a single exact product at exactly one (feature, tap, channel) per channel, and old + product is one rounding -- bit for bit.
        The impulses sit on both sides of every slab seam with the feature in the neighbouring slab (the halo), at rows 0 and N - 1, and
        under a length: at row len - 1 with the feature at len (it counts) and at row len (it does not) '''
    from daft_exprt import ops
    B, N = shape
    r = _rng(B, N, 7)
    old_w, old_b = [_f(r, 128, 1, 3) for _ in range(3)], [_f(r, 128) for _ in range(3)]
    v = r.integers(1, 9, 128).astype(F) * np.where(r.random(128) < .5, -1, 1).astype(F)
    d_dout = torch.zeros(B, N, 128, device=DEV)
    cases = [(None, imp) for imp in O.se_impulses(B, N)]
    if N >= 4:
        ln = N - 2
        lens = [N] * (B - 1) + [ln]
        cases += [(lens, (B - 1, ln - 1, ln, 'row len - 1, feature at len')), (lens, (B - 1, ln, ln - 1, 'row len: masked'))]
    seen = set()
    for lengths, (b, n, j, what) in cases:
        d_dout[b, n] = dev(v)
        feats = [np.zeros((B, N), dtype=F) for _ in range(3)]
        for f in range(3):
            feats[f][b, j] = 1. + .5 * f
            if B > 1:            # the rows next to this utterance in memory: no tap may reach across an utterance's end
                feats[f][b - 1, N - 1], feats[f][(b + 1) % B, 0] = 3., 5.
        d_feats = [dev(x) for x in feats]
        dw, db, aw, ab, live = O.scalar_embed_bwd_sparse({(b, n): v}, feats, 3, lengths, B, N)
        d_len = None if lengths is None else dev(np.array(lengths, dtype=np.int64))
        for need_dbase in (False, True):
            dws, dbs = [dev(w) for w in old_w], [dev(x) for x in old_b]
            dbase = ops.scalar_embed_bwd(d_dout, d_feats, dws, dbs, d_len, need_dbase=need_dbase)
            if need_dbase:
                want = d_dout if live else torch.zeros_like(d_dout)
                assert torch.equal(dbase, want), (what, 'dbase')
            for f in range(3):
                hit = dw[f] != 0
                assert int(hit[:, 0, :].any(0).sum()) == (1 if live else 0) and (not live or hit[:, 0, j - n + 1].all()), (what, f)
                _bits('scalar_embed_bwd', f'{what}: dw[{f}]', dws[f], (old_w[f] + dw[f].astype(F)).astype(F))
                _bits('scalar_embed_bwd', f'{what}: dbias[{f}]', dbs[f], (old_b[f] + db[f].astype(F)).astype(F))
        seen.add(what)
        d_dout[b, n] = 0.
    assert {'row 0', 'row N - 1'} <= seen and (len(O.se_slabs(B, N)) == 1 or {'slab first, halo before', 'slab last, halo behind'} <= seen)


# ---------------------------------------------------------------------------------------------------- embedding + positions, gather-add
@pytest.mark.parametrize('shape', list(O.EMBED_SHAPES))
def test_embed_pos(shape):
    from daft_exprt import ops
    B, N = shape
    lengths = O.EMBED_SHAPES[shape]
    V, unnamed = 11, 5
    r = _rng(B, N, 2)
    ids = r.integers(0, V, (B, N))
    ids[ids == unnamed] = unnamed + 1
    ids[0, 0], ids[0, 1], ids[0, 2], ids[B - 1, 0], ids[B - 1, 1] = 0, V - 1, 0, 0, V - 1     # repeats, the first and the last id
    m = O.row_mask(lengths, B, N)
    if (~m).any():
        ids[~m] = unnamed                                             # named behind the lengths only
    table, pos, dout, old = _f(r, V, 128), _f(r, N + 2, 128), _f(r, B, N, 128), _f(r, V, 128)
    d_ids, d_len = dev(ids.astype(np.int64)), dev(np.array(lengths, dtype=np.int64))
    out = ops.embed_pos_fwd(d_ids, dev(table), dev(pos), d_len)
    _bits('embed_pos_fwd', str(shape), out, O.embed_pos_fwd32(ids, table, pos, lengths))
    dtable = dev(old)
    ops.embed_pos_bwd(d_ids, dev(dout), d_len, dtable)
    con, mag, cnt = O.scatter_rows(ids, dout, V, m)
    assert cnt[unnamed] == 0 and cnt[0] >= 3 and cnt[V - 1] >= 2
    _check('embed_pos_bwd', str(shape), host(dtable)[cnt > 0], (old + con)[cnt > 0], O.scatter_bound(mag, cnt, old)[cnt > 0])
    _bits('embed_pos_bwd', 'rows no valid position names', host(dtable)[cnt == 0], old[cnt == 0])


@pytest.mark.parametrize('C', [128, 130])
@pytest.mark.parametrize('B', [1, 5])
def test_gather_add(B, C):
    from daft_exprt import ops
    V = 6
    r = _rng(B, C, 3)
    ids = np.array([3, 0, 3, 5, 3][:B])
    a, table, dz, old = _f(r, B, C), _f(r, V, C), _f(r, B, C), _f(r, V, C)
    d_ids = dev(ids.astype(np.int64))
    _bits('gather_add_fwd', f'B {B} C {C}', ops.gather_add_fwd(dev(a), dev(table), d_ids), O.gather_add_fwd32(a, table, ids))
    dtable = dev(old)
    ops.gather_add_bwd(dev(dz), d_ids, dtable)
    con, mag, cnt = O.scatter_rows(ids, dz, V)
    _check('gather_add_bwd', f'B {B} C {C}', host(dtable)[cnt > 0], (old + con)[cnt > 0], O.scatter_bound(mag, cnt, old)[cnt > 0])
    _bits('gather_add_bwd', 'rows nobody names', host(dtable)[cnt == 0], old[cnt == 0])


# ---------------------------------------------------------------------------------------------------- masked mean
@pytest.mark.parametrize('N', O.MEAN_N)
def test_masked_mean(N):
    from daft_exprt import ops
    lengths = [0, 1, N, N // 2 + 1, max(N - 1, 0)]
    B = len(lengths)
    r = _rng(N, 4)
    x, dy = _f(r, B, N, 128), _f(r, B, 128)
    x_nan = x.copy()
    for b, ln in enumerate(lengths):
        x_nan[b, ln:] = np.nan                                        # the kernel reads the rows below the length only
    d_x, d_len = dev(x_nan), dev(np.array(lengths, dtype=np.int64))
    out = ops.masked_mean_fwd(d_x, d_len)
    ref, bound = O.masked_mean_fwd(x, lengths)
    _check('masked_mean_fwd', f'N {N}', out, ref, bound)
    assert not host(out)[0].any()                                     # the zero-length utterance: mean 0
    assert torch.equal(out, ops.masked_mean_fwd(d_x, d_len))          # a fixed summation order: bit-identical runs
    dx = ops.masked_mean_bwd(dev(dy), d_len, N)
    _bits('masked_mean_bwd', f'N {N}', dx, O.masked_mean_bwd32(dy, lengths, N))
    assert not host(dx)[0].any()                                      # ... and gradient 0


# ---------------------------------------------------------------------------------------------------- FiLM assembly
@pytest.mark.parametrize('with_post', [False, True])
@pytest.mark.parametrize('B', [1, 5])
@pytest.mark.parametrize('layout', [O.MODEL_LAYOUT, O.ODD_LAYOUT], ids=['model', 'odd'])
def test_film_assemble(layout, B, with_post):
    from daft_exprt import ops
    nb, ch = layout
    W, nblk = O.film_width(nb, ch), sum(nb)
    r = _rng(W, B, 5)
    g, b = _f(r, B, W), _f(r, B, W)
    post = (_f(r, 2, nblk) + np.arange(2 * nblk, dtype=F).reshape(2, nblk)) if with_post else None     # distinct per block and half
    dfilms = [_f(r, B, nb[m], 2 * ch[m]) for m in range(3)]
    old = _f(r, 2, nblk)
    tag = f'W {W} B {B} post {with_post}'
    films = ops.film_assemble_fwd(dev(g), dev(b), dev(post), nb, ch)
    ref, bound = O.film_assemble_fwd(g, b, post, nb, ch)
    ref32 = O.film_assemble_fwd32(g, b, post, nb, ch)
    for m in range(3):
        assert tuple(films[m].shape) == (B, nb[m], 2 * ch[m])
        _check('film_assemble_fwd', f'film {m} {tag}', films[m], ref[m], bound[m])
        _bits('film_assemble_fwd', f'beta {m}', host(films[m])[:, :, ch[m]:], ref32[m][:, :, ch[m]:])
        if not with_post:
            _bits('film_assemble_fwd', f'gamma {m}', host(films[m])[:, :, :ch[m]], ref32[m][:, :, :ch[m]])
    dpost = dev(old)
    dg, db = ops.film_assemble_bwd(dev(g), dev(b), dev(post), [dev(x) for x in dfilms], dpost, nb, ch)
    res = O.film_assemble_bwd(g, b, post, dfilms, nb, ch)
    _bits('film_assemble_bwd', 'dg_raw ' + tag, dg, res.dg_raw.astype(F))          # a product of two fp32 values is exact in float64
    _bits('film_assemble_bwd', 'db_raw ' + tag, db, res.db_raw.astype(F))
    if with_post:
        land, uniform, lanes = O.film_landings(nb, ch, B)
        K = 1 + (6 if uniform else 0) + land
        _check('film_assemble_bwd', 'dpost ' + tag, dpost, old + res.dpost, O.gamma(K)[None, :] * (np.abs(old) + res.apost))
    else:
        _bits('film_assemble_bwd', 'dpost without post-multipliers', dpost, old)


# ---------------------------------------------------------------------------------------------------- exact-fp32 small linear
def _linear_case(M, K, Oo, relu, lengths, N, seed, need_dx_variants=(True, False)):
    from daft_exprt import ops
    r = _rng(M, K, Oo, seed)
    x, w, bias, dy = _f(r, M, K), _f(r, Oo, K) / F(np.sqrt(K)), _f(r, Oo), _f(r, M, Oo)      # x and dy non-zero on the masked rows
    old_w, old_b = _f(r, Oo, K), _f(r, Oo)
    masked = lengths is not None
    d_len = dev(np.array(lengths, dtype=np.int64)) if masked else None
    tag = f'M {M} K {K} O {Oo} relu {relu} masked {masked}'
    d_x, d_w, d_dy = dev(x), dev(w), dev(dy)
    y = ops.linear_small_fwd(d_x, d_w, dev(bias), relu=relu, mask_lengths=d_len, N=N)
    ref, bound = O.linear_small_fwd(x, w, bias, relu, lengths, N)
    _check('linear_small_fwd', tag, y, ref, bound)
    y_host = host(y)
    rows = O.row_mask(lengths, M // N, N).reshape(-1) if masked else np.ones(M, dtype=bool)
    assert not y_host[~rows].any()
    if relu:                                                          # a unit that is dead beyond its bound is an exact zero
        pre, pre_bound = O.linear_small_fwd(x, w, bias, False, lengths, N)
        dead = pre + pre_bound < 0
        assert dead.any() and not y_host[dead].any() and (y_host >= 0).all()
    res = O.linear_small_bwd(dy, y_host, x, w, relu, lengths, N, dx_scale=-0.5)
    for need_dx in need_dx_variants:
        dw, db = dev(old_w), dev(old_b)
        dx = ops.linear_small_bwd(d_dy, y if relu else None, d_x, d_w, dw, db, relu=relu, mask_lengths=d_len, N=N, need_dx=need_dx, dx_scale=-0.5)
        if need_dx:
            _check('linear_small_bwd_dx', tag, dx, res.dx, O.gamma(O.ls_dx_chain(M, K, Oo)) * res.adx)
            assert not host(dx)[~rows].any()
        else:
            assert dx is None
        if O.ls_few_rows(M, masked):                                  # the rows in order, then one atomic: the running bound
            _check('linear_rows_bwd_dw', f'dw {tag} dx {need_dx}', dw, old_w + res.dw, O.rows_dw_bound(res.cw, res.dw, old_w))
            _check('linear_rows_bwd_dw', f'db {tag} dx {need_dx}', db, old_b + res.db, O.rows_dw_bound(res.cb, res.db, old_b))
        else:
            Kc = O.ls_dw_chain(M, masked)
            _check('linear_small_bwd_dw', f'dw {tag} dx {need_dx}', dw, old_w + res.dw, O.acc_bound(Kc, res.aw, old_w))
            _check('linear_small_bwd_dw', f'db {tag} dx {need_dx}', db, old_b + res.db, O.acc_bound(Kc, res.ab, old_b))
    assert np.array_equal(host(d_dy), dy) and np.array_equal(host(d_x), x)


@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('shape', list(O.LS_MASKED))
def test_linear_small_masked(shape, relu):
    B, N, K, Oo = shape
    _linear_case(B * N, K, Oo, relu, O.LS_MASKED[shape], N, 6)


@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('shape', O.LS_PLAIN)
def test_linear_small_unmasked(shape, relu):
    M, K, Oo = shape
    _linear_case(M, K, Oo, relu, None, 1, 7, need_dx_variants=(True,))


# ---------------------------------------------------------------------------------------------------- layout helpers
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('shape', O.TRANSPOSE_SHAPES)
def test_transpose_last2(shape, dtype):
    from daft_exprt import ops
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(*shape, generator=g)
    x.view(-1)[0] = 1. + 2. ** -8                                     # a tie in bf16: to even (1.0), where truncation agrees ...
    x.view(-1)[-1] = 1. + 3. * 2. ** -8                               # ... and a tie that goes up
    y = ops.transpose_last2(x.to(DEV), out_dtype=dtype)
    want = x.transpose(1, 2).contiguous().to(dtype)                   # on the host: bf16 by round to nearest even
    assert y.dtype == dtype and tuple(y.shape) == (shape[0], shape[2], shape[1]) and torch.equal(y.cpu(), want)


def test_stack_and_unstack():
    from daft_exprt import ops
    for K in (1, 2, 3, 4):
        for M in (1, 257):
            y = torch.randn(M, K, generator=torch.Generator().manual_seed(10 * K + M))
            planes = ops.unstack(y.to(DEV), K)
            assert len(planes) == K and all(tuple(p.shape) == (M,) and torch.equal(p.cpu(), y[:, k].contiguous()) for k, p in enumerate(planes))
            back = ops.stack(planes)
            assert tuple(back.shape) == (M, K) and torch.equal(back.cpu(), y)
            mine = [y[:, k].contiguous().to(DEV) for k in range(K)]
            assert torch.equal(ops.stack(mine).cpu(), y)


def test_add_inplace():
    from daft_exprt import ops
    for n in (1, 255, 257):
        g = torch.Generator().manual_seed(n)
        a, b = torch.randn(n + 2, generator=g), torch.randn(n, generator=g)
        want = a.clone()
        want[1:n + 1] += b                                            # one correctly rounded addition per element
        whole = a.clone().to(DEV)
        ops.add_(whole[1:n + 1], b.to(DEV))
        assert torch.equal(whole.cpu(), want)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_colsum(dtype):
    from daft_exprt import ops
    for rows in O.COLSUM_ROWS:
        for C in O.COLSUM_C:
            g = torch.Generator().manual_seed(rows + C)
            x = torch.randn(rows, C, generator=g).to(dtype)
            old = torch.randn(C, generator=g)
            out = old.clone().to(DEV)
            ops.colsum_(x.to(DEV), out)
            s, mag = O.colsum(x.float().numpy())
            _check('colsum', f'rows {rows} C {C} {dtype}', out, old.numpy().astype(np.float64) + s, O.acc_bound(O.colsum_chain(rows), mag, old.numpy()))


def test_fill_zero():
    ''' dx_fill_zero through the library handle on bytes: every start offset 0 .. 16 behind a 16-byte boundary, counts around one 16-byte
        store and beyond one workgroup; the range is zero, every byte outside keeps its 0xA5 '''
    from daft_exprt import _hip as H
    pad = 64
    buf = torch.empty(max(O.FILL_COUNTS) + 2 * pad + 16, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 16 == 0
    for off in O.FILL_OFFSETS:
        for n in O.FILL_COUNTS:
            buf.fill_(0xA5)
            H.check(H.lib().dx_fill_zero(buf.data_ptr() + pad + off, n, H.stream()))
            got = buf.cpu().numpy()
            want = np.full(buf.numel(), 0xA5, dtype=np.uint8)
            want[pad + off:pad + off + n] = 0
            assert np.array_equal(got, want), (off, n, np.flatnonzero(got != want)[:8])


# ---------------------------------------------------------------------------------------------------- argument checks
ARG, SHAPE, DTYPE, UNSUPPORTED = -1, -2, -3, -5       # DX_ERR_* of include/daft_exprt_hip.h


def test_bad_arguments_are_refused_before_any_launch():
    from daft_exprt import _hip as H
    L = H.lib()
    whole = torch.full((4096,), SENT, dtype=torch.float32, device=DEV)
    ids = torch.zeros(64, dtype=torch.int64, device=DEV)
    p, i, s = whole.data_ptr(), ids.data_ptr(), H.stream()
    arr = (ctypes.c_void_p * 4)(p, p, p, p)
    nb, ch = (ctypes.c_int * 3)(1, 1, 1), (ctypes.c_int * 3)(4, 4, 4)
    calls = [
        # the kernels that hold 128 channels only
        ('dx_scalar_embed_fwd', UNSUPPORTED, (None, arr, arr, arr, 1, None, None, p, 1, 2, 64, 3, s)),
        ('dx_scalar_embed_bwd', UNSUPPORTED, (p, arr, 1, None, None, arr, arr, 1, 2, 64, 3, s)),
        ('dx_embed_pos_fwd', UNSUPPORTED, (i, p, p, i, p, 1, 2, 130, s)),
        ('dx_embed_pos_bwd', UNSUPPORTED, (i, p, i, p, 1, 2, 130, s)),
        ('dx_masked_mean_fwd', UNSUPPORTED, (p, i, p, 1, 2, 64, s)),
        ('dx_masked_mean_bwd', UNSUPPORTED, (p, i, p, 1, 2, 256, s)),
        ('dx_scalar_embed_fwd', UNSUPPORTED, (None, arr, arr, arr, 1, None, None, p, 1, 2, 128, 2, s)),              # taps == 2
        ('dx_scalar_embed_bwd', UNSUPPORTED, (p, arr, 1, None, None, arr, arr, 1, 2, 128, 2, s)),
        ('dx_scalar_embed_fwd', ARG, (None, arr, arr, arr, 4, None, None, p, 1, 2, 128, 3, s)),                      # nfeat == 4
        ('dx_scalar_embed_bwd', ARG, (p, arr, 4, None, None, arr, arr, 1, 2, 128, 3, s)),
        ('dx_scalar_embed_bwd', ARG, (p, None, 1, None, None, arr, arr, 1, 2, 128, 3, s)),                           # no pointer arrays
        ('dx_scalar_embed_bwd', ARG, (p, arr, 1, None, None, None, arr, 1, 2, 128, 3, s)),
        ('dx_scalar_embed_bwd', ARG, (p, arr, 1, None, None, arr, (ctypes.c_void_p * 4)(), 1, 2, 128, 3, s)),        # a null entry
        ('dx_scalar_embed_bwd', SHAPE, (p, arr, 1, None, None, arr, arr, 0, 2, 128, 3, s)),
        ('dx_scalar_embed_bwd', SHAPE, (p, arr, 1, None, None, arr, arr, 1, 0, 128, 3, s)),
        ('dx_embed_pos_fwd', SHAPE, (i, p, p, i, p, 0, 2, 128, s)),
        ('dx_embed_pos_bwd', SHAPE, (i, p, i, p, 1, 0, 128, s)),
        ('dx_masked_mean_fwd', SHAPE, (p, i, p, 0, 2, 128, s)),
        ('dx_masked_mean_bwd', SHAPE, (p, i, p, 1, -1, 128, s)),
        ('dx_film_assemble_fwd', SHAPE, (p, p, None, p, p, p, nb, ch, 0, s)),
        ('dx_film_assemble_bwd', SHAPE, (p, p, None, p, p, p, p, p, None, nb, ch, 0, s)),
        ('dx_film_assemble_fwd', SHAPE, (p, p, None, p, p, p, (ctypes.c_int * 3)(0, 0, 0), ch, 1, s)),
        ('dx_linear_small_fwd', SHAPE, (p, p, None, p, None, 1, 2, 6, 1, 0, s)),                                     # K % 4 != 0
        ('dx_linear_small_bwd', SHAPE, (p, None, p, p, p, 1., p, p, None, 1, 0, 4, 1, 0, s)),
        ('dx_linear_small_bwd', SHAPE, (p, None, p, p, p, 1., p, p, None, 1, 2, 0, 1, 0, s)),
        ('dx_linear_small_bwd', SHAPE, (p, None, p, p, p, 1., p, p, None, 1, 2, 4, 0, 0, s)),
        ('dx_linear_small_bwd', SHAPE, (p, None, p, p, p, 1., p, p, i, 0, 2, 4, 1, 0, s)),                           # a mask with N == 0
        ('dx_transpose_last2', DTYPE, (p, p, 7, 1, 2, 2, s)),
        ('dx_stack', ARG, (p, arr, 2, 5, s)),
        ('dx_unstack', ARG, (p, arr, 2, 5, s)),
    ]
    for name, code, args in calls:
        rc = getattr(L, name)(*args)
        assert rc == code and name.encode() in L.dx_last_error(), (name, rc, code, L.dx_last_error())
    torch.cuda.synchronize()
    assert bool((whole == SENT).all()) and not bool(ids.any())
