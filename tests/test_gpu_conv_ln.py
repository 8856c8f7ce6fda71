"""The LayerNorm-fused conv GEMMs -- ops.conv1d_ln (dx_conv1d_ln / dx_conv1d_ln_vres) and ops.conv1d_lnbwd (dx_conv1d_lnbwd) -- on each of
their five kernel paths (dx_conv1d_ln_path: SPLITK = conv_sk_kernel, PLAN_K3 / PLAN_K1 = the LDS-DMA ring of conv_gemm_kernel on
balanced tiles, ROWS64 / ROWS128 = conv_gemm_kernel on fixed tiles), compared element by element with the float64 restatement of
tests/conv_ln_oracle.py under the dropout mask the epilogues draw (tests/dropout_masks.elem_keep, stream 0).

Tolerance, per case, tensor and utterance (y, y_lp, s, mean, rstd, y2 | ds, dx_lp, y2b, dfilm; dgamma and dbeta as a whole), on the
contract rows -- the live rows and the dead rows below the fill end -- computed on the same inputs:
    4 * max|restatement - float64| + 1e-6 * max|float64|                        (absolute)
The restatement is the fp32 one with bf16 rounding where the kernels store or stage bf16 and the contraction added up as an MFMA
chain; tests/test_conv_ln_host.py holds max|restatement - float64| under conv_ln_oracle.CAP of the tensor's largest element, so no
bound can go slack.  The order in which split-K adds its 2 or 4 chains is not matched.  The backward ALONE is handed mean and rstd of
the float64 oracle rounded to fp32, so that an error of the forward cannot cancel; the CHAINED tests feed it the forward's own.

Rows (conv_ln_oracle's docstring has the contract as read from the kernels): y, y_lp, y2, ds, dx_lp are exact zeros on [len, fill end)
on every path; s, mean, rstd there are exact zeros on the plan paths and COMPUTED up to the end of the last live tile on the fixed-tile
paths (zeros behind it) -- each asserted as such.  Every input holds NaN at and past the fill end in every test of this file.

Cases (conv_ln_oracle.CASES; the plan is read back and compared with its Python restatement, the path asserted before every launch):
    T1  B 4, N 128, lens 128 96 33 1, 4 tiles        heights 128 96 33 1: split-K NA 4 3 2 1 (KS 4)
    T2  B 4, N 192, lens 192 161 160 129, 4 tiles    heights 192 161 160 129: NA 6 6 5 5 (KS 2: two channel groups, the j ^ wk exchange)
    T3  B 3, N 256, lens 256 250 193, 3 tiles        two-workgroup tiles 128 + 128, 128 + 122, 128 + 65; the ring's 256-row mapping
    T4  B 3, N 700, lens 700 433 257, 9 tiles        175 x 4, 145 145 143, 129 128: KS 2 and KS 4 in one launch, n0 > 0, grid y = 2
    T5  B 4, N 300, lens 300 252 3 0, default plan   256 tiles of <= 3 rows, fill end 257 < N, an empty utterance, the padding fill
    F1  B 3, N 70, lens 70 33 51, no plan            ROWS64: a partial last tile, residual rows offset by 3
    F2  B 64, N 1001, drawn lens, no plan            ROWS128 (B N > 64000), lens N, 0, 1 among them
SPLITK: T1-T5 at Cin 256, 384 (T2, T4 also 1024); PLAN_K3: T1-T5 at Cin 128, 1024; PLAN_K1 (backward, k = 1): T2, T4, T5 at Cin 384;
ROWS64: F1 at k = 3 (Cin 128, 1024) and k = 1 (Cin 128, 384) for the three operand pairs fp32 / fp32, fp32 x with bf16 w, bf16 / bf16,
and T5 (dead tiles below the fill end); ROWS128: F2, fp32 / fp32 and bf16 / bf16.  Options rotate (conv_ln_oracle.FWD_OPTS, BWD_OPTS).

Measured on an MI355X, kernel error / bound of the fp32-stored tensors and the per-channel sums: the worst ratio per path, operand
pair and direction over the cases, options, tensors and utterances (all seven tests), the median, and the number of figures:
    path      x / w        forward  worst  median    n     backward  worst  median    n
    splitk    bf16 / bf16            0.39    0.08  128                0.63    0.10  140
    plan_k3   bf16 / bf16            0.26    0.11  104                0.45    0.15  114
    plan_k1   bf16 / bf16               -       -    -                0.33    0.13   26
    rows64    fp32 / fp32            0.52    0.13   68                0.48    0.18   72
    rows64    fp32 / bf16            0.25    0.25   68                0.25    0.25   72
    rows64    bf16 / bf16            0.28    0.08   79                0.29    0.10   86
    rows128   fp32 / fp32            0.29    0.22    8                0.42    0.28    8
    rows128   bf16 / bf16            0.17    0.13    8                0.29    0.22    8
The largest ratio anywhere is 0.63 (dbeta of T5 on split-K: 555 rows summed through the atomics of 256 workgroups; it moves with
their order from run to run) and the median of the 989 figures 0.13: the factor 4 stands, and the order of split-K's
partial chains did not have to be matched.  Every bf16-stored tensor (y_lp, dx_lp, both y2: 261 figures) sits at 0.250 exactly -- the
kernel's largest error is the restatement's own, the bf16 rounding of the same element -- and so does every fp32-stored tensor of
fp32 x in front of bf16 weights: there the bf16 rounding of x when it is staged IS the error, and the kernel rounds as the
restatement does.  With fp32 weights the restatement's partial products are the fp32 ones of v_mfma_f32_32x32x2_f32 (K-step 2), not
exact ones: the only place where the rounding model had to follow the path.  Mask readout: the forward's s and the backward's dx_lp
equal elem_keep bit for bit on ROWS64, PLAN_K3 and SPLITK at p = 0.1 and 0.5.  The 246 tests take 19 s together; the slowest are
the six of F2 (1 - 2 s each, the float64 convolution of 64 x 1001 rows on the host), every other test is below 0.3 s but the first
(1 s, it loads the library).  No defect of the kernels or of the wrappers came to light.

Built to fail, in scratch builds that are not committed (failures of this file's 246 tests | of the older
test_splitk_conv_ln_and_lnbwd_match_ring_kernel_and_fp32_reference with its new tall-tile parameters):
  * conv_sk.hip's epilogue alone: `+ xh[e2] * s2` -- 38: every split-K case of test_backward_alone (24) and test_chained (12), the
    split-K test_nothing_dead_is_read and the step-salt test; no ring or fixed-tile test.  The epilogue runs on every tile height, so
    T5 fails with T1-T4 (the older test fails too, all 8: it compares with the ring kernel's copy of the line);
  * the tall-tile split at `n0_tile + blockIdx.y * 96` -- 10, all of them T3 on split-K (4 forward, 4 backward, 2 chained), nothing
    else; the older test passes, its tallest tile has 175 rows;
  * the KS = 2 exchange without its `wave ^ 1` partner -- 30, all of them T2 and T4 on split-K (12 forward, 12 backward, 6 chained),
    nothing else; of the older test only the two new tall-tile parameter sets fail;
  * `fg_h` and `fb_h` swapped in the forward epilogue of conv_gemm_kernel.h -- 65: every FiLM case of test_forward on PLAN_K3, ROWS64
    and ROWS128 (38), every such test_chained (25), test_nothing_dead_is_read on PLAN_K3 and ROWS64; no split-K test;
  * the `cl == 0` guard of the mean / rstd store moved to `cl == 8` -- none, and none can: dx_row16_sum is a symmetric butterfly that
    leaves the same bits in all 16 lanes of a row (csrc/dx_common.h), so lane 1 stores what lane 0 would have.  In its place, the two
    stored values swapped (`mean[rowg] = rstd; rstd[rowg] = mean`) -- 82: every test_forward that saves the statistics and every
    test_chained on PLAN_K3, ROWS64 and ROWS128, and the same two test_nothing_dead_is_read.
"""
import functools

import pytest
import torch

from tests import conv_ln_oracle as K
from tests import layernorm_oracle as L


@pytest.fixture(autouse=True)
def _rows_past_the_fill_end_are_dropped(monkeypatch):
    ''' dead rows are zero-filled only below dx_fill_end (csrc/dx_common.h); the rows past it are unwritten: see the shim '''
    from tests.util import install_unwritten_shim
    install_unwritten_shim(monkeypatch)


pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
F32, BF16 = torch.float32, torch.bfloat16
PLAN_PATHS = (K.SPLITK, K.PLAN_K3, K.PLAN_K1)
ZERO_WHEN_DEAD = ('y', 'y_lp', 'y2', 'ds', 'dx_lp', 'y2b')


def _dev(t):
    return None if t is None else t.to(DEV)


def _wide(t, strided):
    ''' t (B, 256) on the device -- with `strided` as the middle column slice of a (B, 3 * 256) tensor of other values '''
    if t is None:
        return None, None
    if not strided:
        return _dev(t).contiguous(), None
    g = torch.Generator().manual_seed(5)
    wide = torch.randn(t.shape[0], 3 * t.shape[1], generator=g)
    wide[:, t.shape[1]:2 * t.shape[1]] = t
    wide = wide.to(DEV)
    return wide[:, t.shape[1]:2 * t.shape[1]], wide


def _launch_args(c, path, backward):
    ''' packed weights, fragment copy and plan of case c for `path`; asserts that the plan is the restated one and that the
        arguments land on `path` '''
    from daft_exprt import ops
    if backward:
        wp = ops.pack_conv_weight(_dev(c.w_fwd), c.w_dtype, transpose_flip=True)
    else:
        wp = ops.pack_conv_weight(_dev(c.w), c.w_dtype)
    assert tuple(wp.shape) == (c.taps, 128, c.Cin)
    lens = _dev(c.L)
    plan = frag = None
    if path in PLAN_PATHS:
        tiles = K.CASES[c.name][3]
        plan = ops.conv_tile_plan(lens, c.N, tiles=tiles)
        want = K.tile_plan(c.lens, c.N, K.plan_tiles(c.name))
        assert plan[0].cpu().tolist() == [list(e) for e in want], 'the plan is not the restated one'
        if path == K.SPLITK:
            frag = ops.pack_frag_major(wp)
    assert ops.ln_path(c.x_dtype, c.w_dtype, c.taps, c.Cin, c.B, c.N, plan is not None, frag is not None, backward) == path
    return wp, frag, plan, lens


def _forward(c, path, film=None, save=True, lp_copy=True, store_y=True, seed=None, x=None, residual=None):
    from daft_exprt import ops
    wp, frag, plan, lens = _launch_args(c, path, False)
    flm, _ = _wide(c.film, film == 'strided')
    w2 = None if c.w2 is None else ops.pack_conv_weight(_dev(c.w2), BF16)
    vres = None if c.vres is None else tuple(_dev(t).reshape(-1).contiguous() for t in c.vres)
    out = ops.conv1d_ln(_dev(c.x if x is None else x), wp, _dev(c.bias), _dev(c.residual if residual is None else residual), _dev(c.gamma),
                        _dev(c.beta), lens, film=flm, save=save, p_pre=c.p_pre, seed_pre=c.seed_pre if seed is None else seed, lp_copy=lp_copy,
                        plan=plan, w_frag=frag, w2_packed=w2, b2=_dev(c.b2), store_y=store_y, residual_ln=vres)
    got = dict(zip(K.FWD_TENSORS, out))
    assert (got['y'] is not None) == store_y and (got['y_lp'] is not None) == lp_copy and (got['s'] is not None) == save
    assert (got['mean'] is not None) == save and (got['rstd'] is not None) == save
    assert (got.get('y2') is not None) == (c.w2 is not None), 'the split-K path takes the second product into its launch'
    got = {k: v for k, v in got.items() if v is not None}
    for k in ('mean', 'rstd'):
        if k in got:
            got[k] = got[k].view(c.B, c.N)
    for k, v in got.items():
        assert v.dtype == (BF16 if k in K.BF16_STORED else F32), k
    return got


def _backward(c, path, s, mean, rstd, film=None, seed=None, x=None, yin=None):
    ''' one call of ops.conv1d_lnbwd; dgamma, dbeta and dfilm start from c.init (the kernels accumulate) '''
    from daft_exprt import ops
    wp, frag, plan, lens = _launch_args(c, path, True)
    flm, _ = _wide(c.film, False)
    dfilm, wide = _wide(c.init[2] if c.film is not None else None, film == 'strided')
    before = None if wide is None else wide.clone()
    dgamma, dbeta = _dev(c.init[0]).clone(), _dev(c.init[1]).clone()
    y = _dev(c.yin if yin is None else yin).clone()
    w2 = None if c.w2 is None else ops.pack_conv_weight(_dev(c.w2), BF16)
    out = ops.conv1d_lnbwd(_dev(c.x if x is None else x), wp, y, s.contiguous(), mean.reshape(-1).contiguous(), rstd.reshape(-1).contiguous(),
                           _dev(c.gamma), _dev(c.beta), lens, dgamma, dbeta, film=flm, dfilm=dfilm, p_pre=c.p_pre,
                           seed_pre=c.seed_pre if seed is None else seed, plan=plan, w_frag=frag, w2_packed=w2)
    got = {'ds': y, 'dx_lp': out[0] if w2 is not None else out, 'dgamma': dgamma, 'dbeta': dbeta}
    if w2 is not None:
        got['y2b'] = out[1]
    if dfilm is not None:
        got['dfilm'] = dfilm
    if wide is not None:          # the columns beside the slice are not touched
        assert torch.equal(wide[:, :256], before[:, :256]) and torch.equal(wide[:, 512:], before[:, 512:])
    assert got['dx_lp'].dtype == BF16 and got['ds'].dtype == F32
    return got


def _check(c, path, got, ref, low, label):
    ''' every tensor of `got` within its bound of the float64 reference, per utterance, on the contract rows; exact zeros where the
        contract says zero.  Prints the worst error / bound ratio per tensor and asserts after printing '''
    bad, worst = [], {}
    comp = K.computed_rows(c, path)
    for t, g in got.items():
        g = g.detach().double().cpu()
        assert g.shape == ref[t].shape, (t, g.shape, ref[t].shape)
        for b, fe in L.regions(c, t):
            if fe == 0:
                continue
            bnd, _ = L.bound(low, ref, t, b, fe)
            err = float((L.region(g, t, b, fe) - L.region(ref[t], t, b, fe)).abs().max())
            ratio = err / bnd if bnd > 0. else (0. if err == 0. else float('inf'))
            worst[t] = max(worst.get(t, 0.), ratio) if ratio == ratio else float('nan')
            if not err <= bnd:
                bad.append((t, b, fe, err, bnd))
        if g.dim() >= 2 and t != 'dfilm':
            zero = ~c.live if t in ZERO_WHEN_DEAD else ~comp
            for b in range(c.B):
                if bool(g[b, :c.fe[b]][zero[b, :c.fe[b]]].any()):
                    bad.append((t, b, 'rows that must be exactly zero are not'))
    print(f'RATIO {label} {K.PATH_NAME[path]} {c.pair} {c.name}-C{c.Cin}-k{c.taps}:', ' '.join(f'{t} {r:.3f}' for t, r in worst.items()))
    assert not bad, (label, K.PATH_NAME[path], c.name, c.Cin, c.taps, c.pair, bad)


def _rows(cfgs):
    ''' [(cfg, option row)]: F1 takes every row, F2 one, the others two -- neighbours (the two widths of a case) take the other two '''
    out = []
    for k, cfg in enumerate(cfgs):
        rows = range(4) if cfg[1] == 'F1' else ([(0, 2)[k % 2]] if cfg[1] == 'F2' else [k % 4, (k + 2) % 4])
        out += [pytest.param(cfg, o, id=f'{K.config_id(cfg)}-opt{o}') for o in rows]
    return out


@functools.lru_cache(maxsize=2)
def _fwd_problem(cfg, film, p, vres, n2):
    ''' a case, its float64 reference and its restatement, built once for the tests that share them and left unchanged '''
    path, name, cin, taps, pair = cfg
    c = K.make_case(name, cin, taps, pair, False, film=film, p_pre=p, vres=vres, n2=n2)
    return c, K.reference_fwd(c, path), K.restate_fwd(c, path)


@functools.lru_cache(maxsize=2)
def _bwd_problem(cfg, film, p, w2):
    path, name, cin, taps, pair = cfg
    c = K.make_case(name, cin, taps, pair, True, film=film, p_pre=p, n2=128 if w2 else 0)
    return c, K.reference_bwd(c), K.restate_bwd(c)


# ----------------------------------------------------------------------------- 1. forward
@pytest.mark.parametrize('cfg,o', _rows(K.FWD_CONFIGS))
def test_forward(cfg, o):
    film, p, save, lp_copy, store_y, vres, n2 = K.fwd_opts(cfg, o)
    c, ref, low = _fwd_problem(cfg, film is not None, p, vres, n2)
    got = _forward(c, cfg[0], film, save, lp_copy, store_y)
    _check(c, cfg[0], got, ref, low, 'fwd')


# ----------------------------------------------------------------------------- 2. backward alone
@pytest.mark.parametrize('cfg,o', _rows(K.BWD_CONFIGS))
def test_backward_alone(cfg, o):
    film, p, w2 = K.bwd_opts(cfg, o)
    c, ref, low = _bwd_problem(cfg, film is not None, p, w2)
    got = _backward(c, cfg[0], _dev(c.s_in), _dev(c.mean), _dev(c.rstd), film)
    _check(c, cfg[0], got, ref, low, 'bwd' + ('-film' if film else ''))
    keep, scale = K.keep_of(c)
    if keep is not None:          # dx_lp is exactly zero on the dropped elements, ds is not masked
        for b, fe in enumerate(c.fe):
            kb = keep[b, :fe].to(DEV)
            assert not bool(got['dx_lp'][b, :fe][~kb].any()), (b, 'dx_lp of a dropped element must be exactly zero')


# ----------------------------------------------------------------------------- 3. chained
def _nan_past_the_fill_end(c, t):
    t = t.clone()
    for b, fe in enumerate(c.fe):
        t[b, fe:] = float('nan')
    return t


@pytest.mark.parametrize('cfg', [c for c in K.FWD_CONFIGS], ids=[K.config_id(c) for c in K.FWD_CONFIGS])
def test_chained(cfg):
    ''' the forward's own s, mean and rstd feed the backward on the same path, with the same mask, as the model does it '''
    path, name, cin, taps, pair = cfg
    f = K.make_case(name, cin, taps, pair, False, film=True, p_pre=0.1)
    c = K.make_case(name, cin, taps, pair, True, film=True, p_pre=0.1)
    rf, lf = K.reference_fwd(f, path), K.restate_fwd(f, path)
    fwd = _forward(f, path, 'plain')
    _check(f, path, fwd, rf, lf, 'chain')
    s, mean, rstd = (_nan_past_the_fill_end(c, fwd[t]) for t in ('s', 'mean', 'rstd'))
    got = _backward(c, path, s, mean, rstd, 'plain')
    ref = K.reference_bwd(c, (rf['s'], rf['mean'], rf['rstd']))
    low = K.restate_bwd(c, (lf['s'], lf['mean'], lf['rstd']))
    _check(c, path, got, ref, low, 'chain')


# ----------------------------------------------------------------------------- 4. mask readout
@pytest.mark.parametrize('p', [0.1, 0.5])
@pytest.mark.parametrize('path', [K.ROWS64, K.PLAN_K3, K.SPLITK], ids=lambda p: K.PATH_NAME[p])
def test_mask_readout(path, p):
    ''' the mask read out of the forward's s and of the backward's dx_lp on inputs that tell kept from dropped exactly
        (conv_ln_oracle.readout_case): elem_keep's, bit for bit, on every live row '''
    f, c = K.readout_case(False, p), K.readout_case(True, p)
    keep, _ = K.keep_of(f)
    live = f.live[:, :, None].expand_as(keep)
    assert 0 < int((~keep[live]).sum())
    s = _forward(f, path, lp_copy=False)['s'].cpu()
    assert torch.equal((s != 0)[live], keep[live]), ('forward', int(((s != 0) != keep)[live].sum()))
    dx = _backward(c, path, _dev(c.s_in), _dev(c.mean), _dev(c.rstd))['dx_lp'].cpu()
    assert torch.equal((dx != 0)[live], keep[live]), ('backward', int(((dx != 0) != keep)[live].sum()))


# ----------------------------------------------------------------------------- 5. step salt
def test_step_salt_is_added_to_the_seed(monkeypatch):
    ''' with ops.STEP_PTR at a step block of salt t, seed s draws the bits of seed (s + t) mod 2^63 without a block -- in the forward and
        in the backward of the split-K path (the sum passes 2^63) '''
    from daft_exprt import ops
    salt = 0x6F00000012345678
    assert K.SEED_PRE + salt > K.M63
    block = torch.zeros(48, dtype=torch.uint8, device=DEV)
    ops.step_scalars_set(block, salt, 1e-3, (0.9, 0.98), 1, 0.)

    def run(salt_, seed):
        f = K.make_case('T1', 256, 3, 'bf16', False, film=True, p_pre=0.5, salt=salt_)
        c = K.make_case('T1', 256, 3, 'bf16', True, film=True, p_pre=0.5, salt=salt_)
        fwd = _forward(f, K.SPLITK, 'plain', seed=seed)
        bwd = _backward(c, K.SPLITK, _dev(c.s_in), _dev(c.mean), _dev(c.rstd), 'plain', seed=seed)
        return f, c, fwd, bwd
    f, c, want_f, want_b = run(salt, None)
    assert f.seed_pre == (K.SEED_PRE + salt) & K.M63
    _, _, other_f, other_b = run(0, None)
    monkeypatch.setattr(ops, 'STEP_PTR', block.data_ptr())
    _, _, got_f, got_b = run(0, K.SEED_PRE)
    monkeypatch.setattr(ops, 'STEP_PTR', None)
    torch.cuda.synchronize()
    for got, want, other, names in ((got_f, want_f, other_f, ('y', 'y_lp', 's')), (got_b, want_b, other_b, ('ds', 'dx_lp'))):
        for t in names:
            assert all(torch.equal(got[t][b, :fe], want[t][b, :fe]) for b, fe in enumerate(c.fe)), t
            if t != 'ds':          # (ds itself is not masked)
                assert not torch.equal(got[t], other[t]), (t, 'the salt changed nothing')
    _check(f, K.SPLITK, got_f, K.reference_fwd(f, K.SPLITK), K.restate_fwd(f, K.SPLITK), 'salt')
    _check(c, K.SPLITK, got_b, K.reference_bwd(c), K.restate_bwd(c), 'salt')


# ----------------------------------------------------------------------------- 6. nothing dead is read
DEAD = [(K.SPLITK, 256, 3), (K.PLAN_K3, 128, 3), (K.PLAN_K1, 384, 1), (K.ROWS64, 128, 3)]


@pytest.mark.parametrize('path,cin,taps', DEAD, ids=[K.PATH_NAME[p] for p, _, _ in DEAD])
def test_nothing_dead_is_read(path, cin, taps):
    ''' case T5: NaN in every input row at or past the fill end -- x, residual, and in the backward y_inout, s, mean and rstd.  Every
        contract row and every reduction is finite and within its bound, and 7 in place of the NaN changes no bit of a contract row.
        (ROWS128 needs B N > 64000: case F2 carries the same NaN through test_forward, test_backward_alone and test_chained) '''
    c = K.make_case('T5', cin, taps, 'bf16', True, film=True, p_pre=0.1, n2=128 if path == K.SPLITK else 0)
    nanrows = torch.arange(c.N)[None, :] >= torch.tensor(c.fe)[:, None]
    assert int(nanrows.sum()) == 3 * 43
    seven = lambda t: torch.nan_to_num(t.float(), nan=7.).to(t.dtype)
    runs = []
    if path != K.PLAN_K1:
        f = K.make_case('T5', cin, taps, 'bf16', False, film=True, p_pre=0.1, vres=path == K.SPLITK, n2=384 if path == K.SPLITK else 0)
        assert all(bool(torch.isnan(t.float()[nanrows]).all()) for t in (f.x, f.residual))
        a = _forward(f, path, 'plain')
        b_ = _forward(f, path, 'plain', x=seven(f.x), residual=seven(f.residual))
        _check(f, path, a, K.reference_fwd(f, path), K.restate_fwd(f, path), 'dead')
        runs.append((a, b_))
    assert all(bool(torch.isnan(t.float()[nanrows]).all()) for t in (c.x, c.yin, c.s_in, c.mean, c.rstd))
    a = _backward(c, path, _dev(c.s_in), _dev(c.mean), _dev(c.rstd), 'plain')
    b_ = _backward(c, path, _dev(seven(c.s_in)), _dev(seven(c.mean)), _dev(seven(c.rstd)), 'plain', x=seven(c.x), yin=seven(c.yin))
    _check(c, path, a, K.reference_bwd(c), K.restate_bwd(c), 'dead')
    runs.append((a, b_))
    for got, other in runs:
        for t, g in got.items():
            for b, fe in L.regions(c, t):
                assert bool(torch.isfinite(L.region(g, t, b, fe)).all()), (t, b)
            if t not in ('dgamma', 'dbeta', 'dfilm'):          # (the per-channel sums go through atomics: their order is free)
                assert all(torch.equal(g[b, :fe], other[t][b, :fe]) for b, fe in enumerate(c.fe)), t
