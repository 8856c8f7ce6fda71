"""The LayerNorm kernels (csrc/layernorm.hip: ln_fwd_kernel, ln_bwd_kernel, ln_bwd_finish_kernel) called directly through
ops.layernorm_fwd / ops.layernorm_bwd -- all four (x, y) and all five (s, dy, d) storage-type combinations, C = 128, 256, 512, 1024,
with and without FiLM -- and compared element by element with the float64 restatement of tests/layernorm_oracle.py under the
dropout masks that the kernels draw (tests/dropout_masks.elem_keep, stream 0 in front of the LayerNorm, stream 1 behind it).

Tolerance, per case, tensor and utterance (y, y_lp, s, mean, rstd | ds, dx_pre, dx_pre_lp, dfilm; dgamma and dbeta as a whole), on
the contract rows -- the live rows and the dead rows below the fill end, which must be exact zeros -- computed on the same inputs:
    4 * max|restatement - float64| + 1e-6 * max|float64|                        (absolute)
where the restatement is the fp32 one, with bf16 rounding of the tensors that are stored as bf16.  tests/test_layernorm_host.py
holds max|restatement - float64| under 1.2e-5 (fp32) / 7.8e-3 (bf16) of the tensor's largest element, so no bound can go slack.
Summation order is not matched.  The backward ALONE is handed mean and rstd of the float64 oracle rounded to fp32, not the
forward's, so that an error of the forward cannot cancel; the CHAINED tests feed it the forward's own s, mean and rstd.

Cases (tests/layernorm_oracle.CASES):
    A  B 3, N 70, lens 70 33 51          generic: four waves over a slab with a partial last group (70 = 2 * 32 + 6); row offset 3
    B  B 4, N 300, lens 300 252 3 0      fill end 257 < N for three utterances, an empty one and one of three rows; skip_lengths =
                                         lengths, skip_lengths = max(lengths - 2, 0) beside lengths (the grouped step), and
                                         skip_lengths alone (C = 128); rows at or past skip + 2 hold NaN in x, residual, dy, s, mean, rstd
    C  B 30, N 900, C = 128              30 * 29 = 870 > 768 workgroups: rows_per_block = 64, 15 chunks per utterance; 30 lens in 0..900
    D  B 2, N 37, no lengths             row offset 100 with unit spread: a one-pass variance would fail
    E  B 3, N 70, lens 70 33 51          s = relu(randn) with exact zeros and relu_input: gated ds exactly zero, the others compared
A and B at C = 128, 256, 512, 1024; D and E at C = 128 and 1024.

What the kernels may read (their stated contract, test 8): with `skip_lengths` no row at or past skip + 2 is read -- those rows
hold NaN here and every contract row and every reduction stays finite and within its bound.  With `lengths` ALONE the backward
does read the pad rows of s, mean and rstd (their upstream gradient is zeroed, 0 * NaN would reach the per-channel sums), so
the pad rows must be finite then: cases A and E hold no NaN.

Measured on an MI355X, kernel error / bound of the fp32-stored tensors and the per-channel sums: the worst ratio per kernel,
storage types and C over the cases, options, tensors and utterances, and the median over all of them.  `chain` takes in the
chained, step-salt and dead-row tests (forward and backward tensors), `finish` the atomic-free path:
    kernel     types (fwd: x-y, bwd: s-dy-d)   C 128    256    512   1024   median
    fwd        fp32-fp32                        0.17   0.09   0.09   0.26     0.07
    fwd        fp32-bf16                        0.12   0.09   0.10   0.10     0.06
    fwd        bf16-bf16                        0.08   0.06   0.09   0.09     0.06
    fwd        bf16-fp32                        0.10   0.11   0.10   0.10     0.07
    bwd        fp32-fp32-fp32                   0.27   0.10   0.11   0.21     0.08
    bwd        fp32-fp32-bf16                   0.25   0.11   0.09   0.21     0.08
    bwd        fp32-bf16-fp32                   0.23   0.09   0.09   0.22     0.09
    bwd        bf16-bf16-bf16                   0.30   0.15   0.10   0.10     0.07
    bwd        bf16-fp32-bf16                   0.32   0.08   0.06   0.12     0.07
    bwd-film   fp32-fp32-fp32                   0.24   0.10   0.09   0.22     0.08
    bwd-film   fp32-fp32-bf16                   0.38   0.10   0.11   0.22     0.07
    bwd-film   fp32-bf16-fp32                   0.23   0.09   0.11   0.22     0.08
    bwd-film   bf16-bf16-bf16                   0.22   0.08   0.09   0.09     0.07
    bwd-film   bf16-fp32-bf16                   0.41   0.12   0.12   0.12     0.08
    chain      all                              0.23   0.10   0.15   0.11     0.08
    finish     all                              0.15   0.12   0.12   0.10     0.09
The largest ratio anywhere is 0.41 (dbeta of case C, 27 000 rows summed through 450 atomics per channel; the C = 128 column is
where case C runs) and the median of the 1135 figures 0.07; summation order did not have to be matched.  Every bf16-stored tensor
(401 figures) sits at 0.250 exactly: the kernel's largest error is the restatement's own, the bf16 rounding of the same element.
Mask readout: all four masks equal elem_keep bit for bit at p = 0.1, 0.5 and 0.001.  The 366 tests take 8 s together, the slowest
(case B, the first to build a 4 x 300 x 128 dropout mask) half a second.  No defect of the kernels or of the wrappers came to light.
Built to fail, in scratch builds: with the sign of the `xh[j] * m2` term flipped, 204 of the 366 tests fail -- every one that compares
a backward tensor (all of test_backward_alone, test_chained, test_atomic_free_reduction, test_nothing_dead_is_read and the
step-salt test); with `keep_post` dropped from acc_fg, 58: the FiLM cases with p_post > 0 of the same tests; with the two dfilm
slots swapped in the finish kernel, the nine FiLM cases of test_atomic_free_reduction; with the ReLU gate taken on the normalised
value, the twenty case E runs of test_backward_alone.
"""
import functools
import types

import pytest
import torch

from tests import layernorm_oracle as L


@pytest.fixture(autouse=True)
def _rows_past_the_fill_end_are_dropped(monkeypatch):
    ''' dead rows are zero-filled only below dx_fill_end (csrc/dx_common.h); the rows past it are unwritten: see the shim '''
    from tests.util import install_unwritten_shim
    install_unwritten_shim(monkeypatch)


pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
F32, BF16 = torch.float32, torch.bfloat16
NAME = {F32: 'fp32', BF16: 'bf16'}
# neighbours share their inputs' types, hence (with the same options) the case and its float64 reference: see _problem
FWD_PAIRS = [(F32, F32), (F32, BF16), (BF16, BF16), (BF16, F32)]                                              # (x, y)
BWD_TRIPLES = [(F32, F32, F32), (F32, F32, BF16), (F32, BF16, F32), (BF16, BF16, BF16), (BF16, F32, BF16)]      # (s, dy, d)
# (residual, film: None | 'plain' | 'strided' = a column slice of a (B, 3 * 2C) tensor, save, save_s, lp_copy, (p_pre, p_post))
FWD_OPTS = [(True, 'strided', True, True, True, (0.2, 0.3)), (False, None, False, False, False, (0., 0.)),
            (True, None, True, False, True, (0.1, 0.)), (False, 'plain', True, True, False, (0., 0.3))]
# (film, (p_pre, p_post), separate, lp_only); FiLM and no FiLM alternate
BWD_OPTS = [('strided', (0.2, 0.3), False, False), (None, (0., 0.), True, False), ('plain', (0.1, 0.), False, True),
            (None, (0., 0.3), False, False), ('plain', (0., 0.), False, False), (None, (0.2, 0.3), True, False)]
CASE_CONFIGS = [(name, C, variant) for name in L.CASES for C in L.WIDTHS[name] for variant in L.VARIANTS[name]
                if variant != 'skip_only' or C == 128]


@functools.lru_cache(maxsize=3)
def _problem(name, C, variant, x_dtype, dy_dtype, residual, film, pp, s_given):
    ''' a case and its float64 reference, built once for the tests that share them (the next test has the same inputs and options
        and another output type) and left unchanged '''
    c = L.make_case(name, C, variant, x_dtype, dy_dtype, residual=residual, film=film, p_pre=pp[0], p_post=pp[1], s_given=s_given)
    return c, L.reference(c)


def _rotate(items, start, count):
    return [(start + i) % len(items) for i in range(count)]


def _ident(name, C, variant):
    return f'{name}{"-" + variant if variant else ""}-C{C}'


def _dev(t):
    return None if t is None else t.to(DEV)


def _wide(t, strided):
    ''' t (B, 2C) on the device -- with `strided` as the middle column slice of a (B, 3 * 2C) tensor of other values (row stride 6C) '''
    if t is None:
        return None, None
    if not strided:
        return _dev(t).contiguous(), None
    g = torch.Generator().manual_seed(5)
    wide = torch.randn(t.shape[0], 3 * t.shape[1], generator=g)
    wide[:, t.shape[1]:2 * t.shape[1]] = t
    wide = wide.to(DEV)
    return wide[:, t.shape[1]:2 * t.shape[1]], wide


def _forward(c, y_dtype, film=None, save=True, save_s=True, lp_copy=False, seeds=None):
    from daft_exprt import ops
    flm, _ = _wide(c.film, film == 'strided')
    seed_pre, seed_post = seeds if seeds is not None else (c.seed_pre, c.seed_post)
    out = ops.layernorm_fwd(_dev(c.x), _dev(c.gamma), _dev(c.beta), residual=_dev(c.residual), film=flm, lengths=_dev(c.lengths),
                            out_dtype=y_dtype, save=save, save_s=save_s, p_pre=c.p_pre, seed_pre=seed_pre, p_post=c.p_post,
                            seed_post=seed_post, skip_lengths=_dev(c.skip), lp_copy=lp_copy)
    got = dict(zip(('y', 'y_lp', 's', 'mean', 'rstd') if lp_copy else ('y', 's', 'mean', 'rstd'), out))
    assert got['y'].dtype == y_dtype and (not lp_copy or got['y_lp'].dtype == BF16)
    assert (got['s'] is not None) == save_s and (got['mean'] is not None) == save and (got['rstd'] is not None) == save
    got = {k: v for k, v in got.items() if v is not None}
    for k in ('mean', 'rstd'):
        if k in got:
            assert got[k].dtype == F32
            got[k] = got[k].view(c.B, c.N)
    return got


def _backward(c, s, mean, rstd, d_dtype, film=None, separate=False, lp_only=False, seeds=None):
    ''' one call of ops.layernorm_bwd; dgamma, dbeta and dfilm start from c.init (the kernels accumulate).  Returns the tensors by
        name, with `same` = whether dx_pre came back as ds itself '''
    from daft_exprt import ops
    dgamma, dbeta = _dev(c.init[0]).clone(), _dev(c.init[1]).clone()
    flm, _ = _wide(c.film, False)
    dfilm, wide = _wide(c.init[2] if c.film is not None else None, film == 'strided')
    before = None if wide is None else wide.clone()
    seed_pre, seed_post = seeds if seeds is not None else (c.seed_pre, c.seed_post)
    ds, dxp = ops.layernorm_bwd(_dev(c.dy), s, mean.reshape(-1), rstd.reshape(-1), _dev(c.gamma), _dev(c.beta), dgamma, dbeta, film=flm,
                                dfilm=dfilm, lengths=_dev(c.lengths), d_dtype=d_dtype, p_pre=c.p_pre, seed_pre=seed_pre, p_post=c.p_post,
                                seed_post=seed_post, relu_input=c.relu, skip_lengths=_dev(c.skip), lp_only=lp_only, separate=separate)
    assert ds.dtype == d_dtype and dxp.dtype == (BF16 if lp_only else d_dtype)
    got = {'ds': ds, ('dx_pre_lp' if lp_only else 'dx_pre'): dxp, 'dgamma': dgamma, 'dbeta': dbeta}
    if dfilm is not None:
        got['dfilm'] = dfilm
    if wide is not None:          # the columns beside the slice are not touched
        C2 = dfilm.shape[1]
        assert torch.equal(wide[:, :C2], before[:, :C2]) and torch.equal(wide[:, 2 * C2:], before[:, 2 * C2:])
    return got, dxp is ds


def _oracle_stats(c, ref):
    ''' mean and rstd of the float64 oracle rounded to fp32, NaN on the rows the kernel must not read '''
    out = []
    for t in (ref['mean'], ref['rstd']):
        t = t.float()
        t[~c.comp] = float('nan')
        out.append(t)
    return out


def _check(c, got, ref, low, label, types_):
    ''' every tensor of `got` within its bound of the float64 reference, per utterance, on the contract rows; exact zeros where the
        contract says zero.  Prints the worst error / bound ratio per tensor and asserts after printing '''
    bad, worst = [], {}
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
            zero = ~(c.live & c.comp) if t in ('y', 'y_lp') else ~c.comp
            for b in range(c.B):
                if bool(g[b, :c.fe[b]][zero[b, :c.fe[b]]].any()):
                    bad.append((t, b, 'rows that must be exactly zero are not'))
    print(f'RATIO {label} {types_} C{c.C} {c.name}{"-" + c.variant if c.variant else ""}:', ' '.join(f'{t} {r:.3f}' for t, r in worst.items()))
    assert not bad, (label, c.name, c.variant, c.C, types_, bad)


def _same_bits(c, a, b):
    ''' a and b hold the same bits on the contract rows ((B, N, C) tensors) or everywhere (the per-channel sums) '''
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    as_int = torch.int32 if a.dtype == F32 else torch.int16
    if a.dim() == 3:
        return all(torch.equal(a[i, :fe].contiguous().view(as_int), b[i, :fe].contiguous().view(as_int)) for i, fe in enumerate(c.fe))
    return torch.equal(a.contiguous().view(as_int), b.contiguous().view(as_int))


# ----------------------------------------------------------------------------- 1. forward
def _forward_configs():
    out = []
    for k, (name, C, variant) in enumerate(CASE_CONFIGS):
        full = name in ('D', 'E') or (name == 'A' and C in (128, 1024))          # every option row with every pair
        if full:
            picked = [(o, i) for i in range(4) for o in range(4)]
        elif variant in (None, 'same'):                                          # every pair and every option row once
            picked = [((i + k) % 4, i) for i in range(4)]
        else:
            picked = [((i + k + j) % 4, i) for i in _rotate(FWD_PAIRS, k, 2) for j in (0, 2)]
        for o, i in sorted(picked):
            x_dtype, y_dtype = FWD_PAIRS[i]
            out.append(pytest.param(name, C, variant, x_dtype, y_dtype, o, id=f'{_ident(name, C, variant)}-{NAME[x_dtype]}-{NAME[y_dtype]}-opt{o}'))
    return out


@pytest.mark.parametrize('name,C,variant,x_dtype,y_dtype,o', _forward_configs())
def test_forward(name, C, variant, x_dtype, y_dtype, o):
    residual, film, save, save_s, lp_copy, pp = FWD_OPTS[o]
    c, ref = _problem(name, C, variant, x_dtype, F32, residual, film is not None, pp, False)
    low = L.restate(c, y_dtype)
    got = _forward(c, y_dtype, film, save, save_s, lp_copy)
    _check(c, got, ref, low, 'fwd', f'{NAME[x_dtype]}-{NAME[y_dtype]}')


# ----------------------------------------------------------------------------- 2. backward alone
def _backward_configs():
    out = []
    for k, (name, C, variant) in enumerate(CASE_CONFIGS):
        full = name == 'A' and C in (128, 1024)
        triples = range(5) if (name in ('A', 'D', 'E') or variant == 'same') else _rotate(BWD_TRIPLES, 2 * k, 2)
        picked = [(o, i) for i in triples for o in (range(6) if full else _rotate(BWD_OPTS, (0, 0, 1, 2, 3)[i] + k, 1 if name == 'B' else 2))]
        for o, i in sorted(picked):
            out.append(pytest.param(name, C, variant, BWD_TRIPLES[i], o,
                                    id=f'{_ident(name, C, variant)}-{"-".join(NAME[t] for t in BWD_TRIPLES[i])}-opt{o}'))
    return out


def _check_dx_pre_identities(c, got, same, separate, lp_only, d_dtype):
    ''' dx_pre IS ds without pre-dropout (unless a buffer of its own was asked for: then the same bits); with pre-dropout it is exactly
        zero on the dropped elements and ds times the scale on the kept ones (one more rounding of the product in bf16) '''
    if lp_only:
        return
    keep, scale = L.keep_of(c, 0)
    if keep is None:
        assert same == (not separate)
        assert _same_bits(c, got['dx_pre'], got['ds'])
        return
    assert not same
    keep = keep.to(DEV)
    for b, fe in enumerate(c.fe):
        ds, dxp, kb = got['ds'][b, :fe], got['dx_pre'][b, :fe], keep[b, :fe]
        assert not bool(dxp[~kb].any()), (b, 'dx_pre of a dropped element must be exactly zero')
        if d_dtype == F32:
            assert torch.equal(dxp[kb], ds[kb] * scale), b
        else:
            want = ds[kb].double() * scale
            assert bool(((dxp[kb].double() - want).abs() <= 2. ** -7 * (1. + 2. ** -8) * want.abs()).all()), b


@pytest.mark.parametrize('name,C,variant,triple,o', _backward_configs())
def test_backward_alone(name, C, variant, triple, o):
    film, pp, separate, lp_only = BWD_OPTS[o]
    s_dtype, dy_dtype, d_dtype = triple
    c, ref = _problem(name, C, variant, s_dtype, dy_dtype, True, film is not None, pp, True)
    mean, rstd = _oracle_stats(c, ref)
    low = L.restate(c, F32, d_dtype, (mean, rstd))
    got, same = _backward(c, _dev(c.x), _dev(mean), _dev(rstd), d_dtype, film, separate, lp_only)
    _check(c, got, ref, low, 'bwd' + ('-film' if film else ''), '-'.join(NAME[t] for t in triple))
    _check_dx_pre_identities(c, got, same, separate, lp_only, d_dtype)
    if c.relu:
        gated = (c.x.float() <= 0.).to(DEV)
        assert 0.3 < float(gated.float().mean()) < 0.7
        assert not bool(got['ds'][gated].any()), 'ds of an element with s <= 0 must be exactly zero'


# ----------------------------------------------------------------------------- 3. chained
def _chained_configs():
    out = []
    for k, (name, C, variant) in enumerate(CASE_CONFIGS):
        if name == 'E' or variant == 'skip_only' or (variant == 'grouped' and C != 128):
            continue
        i = k % 3                               # the forward's s_out is fp32
        out.append(pytest.param(name, C, variant, BWD_TRIPLES[i], True, id=f'{_ident(name, C, variant)}-{"-".join(NAME[t] for t in BWD_TRIPLES[i])}'))
        if name in ('A', 'D'):                  # bf16 x, no residual, no pre-dropout: s is x itself, as the model's prenet hands it over
            i = 3 + k % 2
            out.append(pytest.param(name, C, variant, BWD_TRIPLES[i], False, id=f'{_ident(name, C, variant)}-{"-".join(NAME[t] for t in BWD_TRIPLES[i])}-raw'))
    return out


@pytest.mark.parametrize('name,C,variant,triple,saved', _chained_configs())
def test_chained(name, C, variant, triple, saved):
    ''' the forward's own s (or the raw bf16 x), mean and rstd feed the backward, as the model does it '''
    s_dtype, dy_dtype, d_dtype = triple
    pp = (0.2, 0.3) if saved else (0., 0.3)
    c = L.make_case(name, C, variant, F32 if saved else BF16, dy_dtype, residual=saved, film=True, p_pre=pp[0], p_post=pp[1])
    ref, low = L.reference(c), L.restate(c, BF16 if not saved else F32, d_dtype)
    fwd = _forward(c, BF16 if not saved else F32, 'plain', True, saved)
    got, _ = _backward(c, fwd['s'] if saved else _dev(c.x), fwd['mean'], fwd['rstd'], d_dtype, 'plain')
    got.update(fwd)
    _check(c, got, ref, low, 'chain', '-'.join(NAME[t] for t in triple))


# ----------------------------------------------------------------------------- 4. atomic-free path
def _chunks(B, N):
    rpb = 32
    while rpb < 1024 and -(-N // rpb) * B > 768:
        rpb *= 2
    return -(-N // rpb), rpb


@pytest.mark.parametrize('film', [None, 'strided'], ids=['plain', 'film'])
@pytest.mark.parametrize('name,C,variant', [p for p in CASE_CONFIGS if p[0] in 'ABC' and p[2] in (None, 'same')],
                         ids=[_ident(*p) for p in CASE_CONFIGS if p[0] in 'ABC' and p[2] in (None, 'same')])
def test_atomic_free_reduction(name, C, variant, film, monkeypatch):
    ''' ops.DETERMINISTIC_LN: per-workgroup partial sums in a workspace and ln_bwd_finish_kernel in place of the atomics '''
    from daft_exprt import _hip as H
    from daft_exprt import ops
    k = [p[:2] for p in CASE_CONFIGS].index((name, C)) + (1 if film else 0)
    triple = BWD_TRIPLES[k % 5]
    s_dtype, dy_dtype, d_dtype = triple
    c = L.make_case(name, C, variant, s_dtype, dy_dtype, film=film is not None, p_pre=0.2, p_post=0.3, s_given=True)
    ref = L.reference(c)
    mean, rstd = _oracle_stats(c, ref)
    low = L.restate(c, F32, d_dtype, (mean, rstd))
    args = (_dev(c.x), _dev(mean), _dev(rstd), d_dtype, film)
    atomics, _ = _backward(c, *args)
    monkeypatch.setattr(ops, 'DETERMINISTIC_LN', True)
    first, _ = _backward(c, *args)
    second, _ = _backward(c, *args)
    chunks, rpb = _chunks(c.B, c.N)
    assert H.lib().dx_layernorm_bwd_ws_floats(c.B, c.N, C) == c.B * chunks * 4 * C
    if name == 'C':
        assert (chunks, rpb) == (15, 64)
    else:
        assert rpb == 32
    _check(c, first, ref, low, 'ws' + ('-film' if film else ''), '-'.join(NAME[t] for t in triple))
    for t in first:
        assert _same_bits(c, first[t], second[t]), (t, 'two runs of the atomic-free path differ')
    for t in ('ds', 'dx_pre'):
        assert _same_bits(c, first[t], atomics[t]), (t, 'the elementwise outputs do not depend on the reduction path')
    for t in [t for t in ('dgamma', 'dbeta', 'dfilm') if t in first]:
        for b, fe in L.regions(c, t):
            bnd, _ = L.bound(low, ref, t, b, fe)
            diff = float((L.region(first[t], t, b, fe).double() - L.region(atomics[t], t, b, fe).double()).abs().max())
            assert diff <= bnd, (t, b, diff, bnd)


# ----------------------------------------------------------------------------- 5. mask readout
def _readout_forward(c, dtype, seeds=None):
    got = _forward(c, dtype, None, False, True, seeds=seeds)
    return got['y'].cpu(), got['s'].cpu()


def _readout_backward(c, dtype, seeds=None):
    ref = L.reference(c)
    got, _ = _backward(c, _dev(c.x), _dev(ref['mean'].float()), _dev(ref['rstd'].float()), dtype, seeds=seeds)
    return got['ds'].cpu(), got['dx_pre'].cpu(), ref['rstd']


@pytest.mark.parametrize('dtype', [F32, BF16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('C', [128, 1024])
@pytest.mark.parametrize('p', [0.1, 0.5, 0.001])
def test_mask_readout(p, C, dtype):
    ''' the four masks -- stream 0 and stream 1, drawn by ln_fwd and regenerated by ln_bwd -- read out of s_out, y, dx_pre and ds
        on inputs that tell kept from dropped exactly (layernorm_oracle.readout_inputs): each is elem_keep's bit for bit.
        p = 0.001 quantises to a threshold of 1 (1 / 256 dropped), not to 0 '''
    from tests import dropout_masks as DM
    for stream in (0, 1):
        keep, scale = DM.elem_keep((L.SEED_PRE, L.SEED_POST)[stream], stream, range(L.READOUT_B), L.READOUT_N, C, p)
        keep = torch.from_numpy(keep)
        assert 0 < int((~keep).sum())
        got = L.decode_forward(stream, *_readout_forward(L.readout_case(C, dtype, p, stream), dtype))
        assert torch.equal(got, keep), ('ln_fwd', stream, int((got != keep).sum()))
        got = L.decode_backward(stream, *_readout_backward(L.readout_case(C, dtype, p, stream, s_given=True), dtype), scale)
        assert torch.equal(got, keep), ('ln_bwd', stream, int((got != keep).sum()))


# ----------------------------------------------------------------------------- 6. step salt
@pytest.mark.parametrize('dtype', [F32, BF16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('C', [128, 1024])
def test_step_salt_is_added_to_both_seeds(C, dtype, monkeypatch):
    ''' with ops.STEP_PTR at a step block of salt t, seed s draws the bits of seed (s + t) mod 2^63 without a block -- in the forward
        and in the backward, for both streams (the sum of SEED_POST and the salt passes 2^63) '''
    from daft_exprt import ops
    salt = 0x6F00000012345678
    assert L.SEED_POST + salt > L.M63
    block = torch.zeros(48, dtype=torch.uint8, device=DEV)
    ops.step_scalars_set(block, salt, 1e-3, (0.9, 0.98), 1, 0.)
    plain = L.make_case('A', C, None, dtype, dtype, p_pre=0.2, p_post=0.3)
    salted = L.make_case('A', C, None, dtype, dtype, p_pre=0.2, p_post=0.3, salt=salt)
    assert (salted.seed_pre, salted.seed_post) == ((L.SEED_PRE + salt) & L.M63, (L.SEED_POST + salt) & L.M63)

    def run(c, seeds):
        fwd = _forward(c, dtype, 'plain', seeds=seeds)
        bwd, _ = _backward(c, fwd['s'], fwd['mean'], fwd['rstd'], F32, 'plain', seeds=seeds)      # (s fp32, dy fp32 or bf16, d fp32)
        return {**fwd, **bwd}
    want, other = run(salted, None), run(plain, None)
    monkeypatch.setattr(ops, 'STEP_PTR', block.data_ptr())
    got = run(plain, (L.SEED_PRE, L.SEED_POST))
    monkeypatch.setattr(ops, 'STEP_PTR', None)
    torch.cuda.synchronize()
    for t in ('y', 's', 'ds', 'dx_pre'):
        assert torch.equal(got[t], want[t]), t
        assert not torch.equal(got[t], other[t]), (t, 'the salt changed nothing')
    ref, low = L.reference(salted), L.restate(salted, dtype, F32)
    _check(salted, got, ref, low, 'salt', NAME[dtype])


# ----------------------------------------------------------------------------- 7. refusals
@pytest.mark.parametrize('C', [64, 384])
def test_unsupported_width_is_refused(C):
    from daft_exprt import ops
    x = torch.randn(2, 5, C, device=DEV)
    v = torch.ones(C, device=DEV)
    with pytest.raises(RuntimeError, match='unsupported'):
        ops.layernorm_fwd(x, v, v)
    stat = torch.ones(10, device=DEV)
    with pytest.raises(RuntimeError, match='unsupported'):
        ops.layernorm_bwd(x, x, stat, stat, v, v, torch.zeros(C, device=DEV), torch.zeros(C, device=DEV))


@pytest.mark.parametrize('triple', [(BF16, F32, F32), (BF16, BF16, F32), (F32, BF16, BF16)], ids=lambda t: '-'.join(NAME[d] for d in t))
def test_unsupported_backward_types_are_refused(triple):
    from daft_exprt import ops
    s_dtype, dy_dtype, d_dtype = triple
    x = torch.randn(2, 5, 128, device=DEV)
    v, stat = torch.ones(128, device=DEV), torch.ones(10, device=DEV)
    with pytest.raises(RuntimeError, match='unsupported dtypes'):
        ops.layernorm_bwd(x.to(dy_dtype), x.to(s_dtype), stat, stat, v, v, torch.zeros(128, device=DEV), torch.zeros(128, device=DEV), d_dtype=d_dtype)


def test_film_without_dfilm_is_refused():
    from daft_exprt import ops
    x = torch.randn(2, 5, 128, device=DEV)
    v, stat = torch.ones(128, device=DEV), torch.ones(10, device=DEV)
    dgamma, dbeta = torch.zeros(128, device=DEV), torch.zeros(128, device=DEV)
    with pytest.raises(RuntimeError, match='film and dfilm come together'):
        ops.layernorm_bwd(x, x, stat, stat, v, v, dgamma, dbeta, film=torch.ones(2, 256, device=DEV))
    with pytest.raises(RuntimeError, match='film and dfilm come together'):
        ops.layernorm_bwd(x, x, stat, stat, v, v, dgamma, dbeta, dfilm=torch.zeros(2, 256, device=DEV))
    assert not bool(dgamma.any()) and not bool(dbeta.any())


# ----------------------------------------------------------------------------- 8. nothing dead is read
@pytest.mark.parametrize('C', [128, 1024])
@pytest.mark.parametrize('variant', ['same', 'grouped'])
def test_nothing_dead_is_read(variant, C):
    ''' case B: NaN in every input row at or past skip + 2 -- x, residual, dy, and in the backward s, mean and rstd.  Every contract
        row and every reduction is finite and within its bound, and 7 in place of the NaN changes no bit of a contract row '''
    c = L.make_case('B', C, variant, p_pre=0.2, p_post=0.3)
    assert all(bool(torch.isnan(t[~c.comp]).all()) and int((~c.comp).sum()) > 500 for t in (c.x, c.residual, c.dy))
    fwd = _forward(c, F32, 'plain', lp_copy=True)
    s, mean, rstd = fwd['s'].clone(), fwd['mean'].clone(), fwd['rstd'].clone()
    dead = (~c.comp).to(DEV)
    s[dead], mean[dead], rstd[dead] = float('nan'), float('nan'), float('nan')
    bwd, _ = _backward(c, s, mean, rstd, F32, 'plain')
    finite = types.SimpleNamespace(**vars(c))
    for t in ('x', 'residual', 'dy'):
        setattr(finite, t, torch.nan_to_num(getattr(c, t), nan=7.))
    fwd2 = _forward(finite, F32, 'plain', lp_copy=True)
    bwd2, _ = _backward(finite, fwd2['s'], fwd2['mean'], fwd2['rstd'], F32, 'plain')
    for got, other in ((fwd, fwd2), (bwd, bwd2)):
        for t, g in got.items():
            if t in ('mean', 'rstd'):
                assert all(torch.equal(g[b, :fe], other[t][b, :fe]) for b, fe in enumerate(c.fe)), t
            elif t not in ('dgamma', 'dbeta', 'dfilm'):
                assert _same_bits(c, g, other[t]), t
            for b, fe in L.regions(c, t):
                assert bool(torch.isfinite(L.region(g, t, b, fe)).all()), (t, b)
    ref, low = L.reference(c), L.restate(c)
    _check(c, {**fwd, **bwd}, ref, low, 'dead', 'fp32')
