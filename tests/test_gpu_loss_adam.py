"""The tail of the training step -- dx_loss_fwd_bwd, dx_sumsq, dx_adam_step, dx_step_scalars_set (csrc/train_ops.hip) and
dx_adam_pack_step (csrc/adam_pack.hip) -- each alone against the float64 oracle of tests/loss_adam_oracle.py (its docstring has the
conventions and the derivation of every bound; tests/test_loss_adam_host.py holds each case to its purpose).

Every tolerance comes from the oracle's bound functions; the one literal is EXP_LOG_ULPS, the measured accuracy of expf / logf.
Every output lives inside a larger buffer of sentinels that must come back unchanged, and every test prints error / bound of what it
compares before it asserts (run with -s to see them).

What runs (127 tests):
    test_loss_terms_and_gradients (28)     the seven shapes of loss_adam_oracle.LOSS_SHAPES in the four forms: plain gradient (atomics),
                                           transposed with the workspace, transposed without it (C API, tpw = MT_TPW), terms only;
                                           d_post accumulated onto random values
    test_loss_with_a_gradient_scale_and_large_logits (9), _without_a_post_multiplier (8), _with_a_post_multiplier_of_zeros (3),
    test_loss_takes_the_speaker_weight_from_the_step_block (4)
    test_loss_impulses (9)                 pred = tgt but for one power of two, 16 positions: a single summand, one non-zero gradient
    test_loss_refuses_an_empty_channel_or_class_axis_before_any_launch
    test_sumsq_against_float64_at_every_alignment (9), test_sumsq_impulses_are_exact (4)
    test_adam_three_steps_on_slices (45)   n x weight decay x clipping, offsets 1 and 3; test_adam_takes_lr_..._from_the_step_block (2);
                                           test_adam_refuses_bad_arguments_before_any_launch
    test_fused_adam_on_a_hand_built_table (4)   bf16 / fp32 copies, by value / from the step block

Measured on an MI355X: 3.5 s for the file, the slowest test 0.46 s (it loads the library).  Error / bound at most 0.99 (p) and 0.95
(d_post): a final rounding just above a power of two attains its u; 0.73 for d_spk, 0.53 for the other gradients, 0.42 for m, 0.29 for
v, 0.28 for terms[7], at most 0.14 for the summed terms and 0.08 for the sums of squares.  expf / logf: 1.16 ulp with all of the error
attributed to them, on the elements of d_spk where they would show; 4 x that is allowed.  No defect of the kernels came to light;
dx_loss_fwd_bwd now refuses n_mel <= 0, n_spk_classes <= 0 and n_post < 0.  DESIGN.md §3 lists the sixteen value-only mutants of
train_ops.hip and adam_pack.hip that were built to fail, and what each of them fails here."""
import math

import numpy as np
import pytest
import torch

from tests import loss_adam_oracle as O

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SENT = -1024.          # exact in bf16 too
GUARD = 64
EXP_LOG_ULPS = 4.64    # 4 x the 1.16 ulp measured on an MI355X: DESIGN.md §3, "The loss, gradient-norm and Adam kernels against float64"
BETAS, EPS, LR = (0.9, 0.98), 1e-9, 1e-3


def _guarded(shape, fill=SENT, dtype=torch.float32):
    ''' (view of `shape`, the whole buffer): GUARD sentinels on both sides of the view '''
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return whole[GUARD:GUARD + n].view(*shape), whole


def _guards_intact(whole, fill=SENT):
    return bool((whole[:GUARD] == fill).all()) and bool((whole[-GUARD:] == fill).all())


def _f64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _worst(name, err, bound):
    ''' largest error / bound (0 / 0 counts as 0), printed; an error where the bound is zero is infinite '''
    err, bound = np.atleast_1d(np.asarray(err, dtype=np.float64)), np.atleast_1d(np.asarray(bound, dtype=np.float64))
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(err == 0, 0., err / bound)
    w = float(ratio.max()) if ratio.size else 0.
    print(f'  {name}: error / bound = {w:.3g}')
    return w


# ---------------------------------------------------------------------------------------------------- dx_loss_fwd_bwd
LOSS_KEYS = ('dur', 'energy', 'pitch', 'dur_t', 'energy_t', 'pitch_t', 'in_len', 'mel', 'mel_t', 'out_len', 'logits', 'ids')


def _run_loss(p, form, weights=O.WEIGHTS, gs=1., post=True, step_ptr=None, old_post=None):
    ''' -> (terms, grads on the host as float64 with d_mel as (B, C, T), old d_post); asserts every guard band '''
    from daft_exprt import _hip as H
    from daft_exprt import ops
    B, L, T, C, S = p['shape']
    d = {k: torch.from_numpy(p[k]).to(DEV) for k in LOSS_KEYS}
    post_t = torch.from_numpy(p['post']).to(DEV) if post else None
    transposed = form in ('tws', 'tnows')
    outs, wholes = {}, {}
    if form != 'terms':
        shapes = {'d_dur': (B, L), 'd_energy': (B, L), 'd_pitch': (B, L), 'd_mel': (B, T, C) if transposed else (B, C, T), 'd_spk': (B, S)}
        for k, shp in shapes.items():
            outs[k], wholes[k] = _guarded(shp)
        if post:
            outs['d_post'], wholes['d_post'] = _guarded((O.N_POST,))
            old_post = np.random.default_rng(3).standard_normal(O.N_POST).astype(np.float32) if old_post is None else old_post
            outs['d_post'].copy_(torch.from_numpy(old_post))
    grads = {k: v for k, v in outs.items() if k != 'd_post'}
    if form == 'tnows':      # the atomics form with a transposed gradient: only the C API reaches it (ops always hands over a workspace)
        terms, wholes['terms'] = _guarded((8,))
        w = [float(x) for x in weights]
        H.check(H.lib().dx_loss_fwd_bwd(*[H.ptr(d[k]) for k in LOSS_KEYS], H.ptr(post_t), *[H.ptr(grads[k]) for k in ('d_dur', 'd_energy', 'd_pitch', 'd_mel', 'd_spk')],
                                        H.ptr(outs.get('d_post')), H.ptr(terms), None, B, L, T, C, S, O.N_POST if post else 0, *w, float(gs), 1,
                                        step_ptr, H.stream()))
    else:
        ops.STEP_PTR = step_ptr
        try:
            terms = ops.loss_fwd_bwd(*[d[k] for k in LOSS_KEYS], post_t, weights, grads=grads or None, d_post_mult=outs.get('d_post'),
                                     grad_scale=gs, d_mel_transposed=transposed)
        finally:
            ops.STEP_PTR = None
    torch.cuda.synchronize()
    for k, whole in wholes.items():
        assert _guards_intact(whole), f'{k}: written outside its shape'
    host = {k: _f64(v) for k, v in outs.items()}
    if transposed:
        host['d_mel'] = host['d_mel'].transpose(0, 2, 1)
    for k in LOSS_KEYS:      # the inputs are inputs
        assert np.array_equal(d[k].cpu().numpy(), p[k]), k
    return _f64(terms), host, old_post


def _check_loss(p, form, weights=O.WEIGHTS, gs=1., post=True, step_ptr=None, oracle_weights=None, old_post=None):
    B, L, T, C, S = p['shape']
    terms, grads, old_post = _run_loss(p, form, weights, gs, post, step_ptr, old_post)
    r = O.loss_terms_and_grads(p, oracle_weights or weights, gs, post)
    K = O.loss_chains(B, L, T, C, O.N_POST if post else 0, form)
    worst = []
    t0_bound, dspk_bound = O.spk_bounds(r.spk, K['ce'], EXP_LOG_ULPS)
    s_t0, s_dspk = O.spk_sensitivity(r.spk)
    b0 = O.spk_bounds(r.spk, K['ce'], 0.)
    if s_t0 >= b0[0] / 4.:
        print(f'  terms[0] error in ulps of expf / logf, all of it attributed to them: {abs(terms[0] - r.terms[0]) / s_t0:.3g}')
    worst.append(_worst('terms[0]', abs(terms[0] - r.terms[0]), t0_bound))
    if post:
        worst.append(_worst('terms[1]', abs(terms[1] - r.terms[1]), O.nonneg_bound(K['post'], O.C_TERM) * r.terms[1]))
    else:
        assert terms[1] == 0.
    for i in (2, 3, 4):
        worst.append(_worst(f'terms[{i}]', abs(terms[i] - r.terms[i]), O.nonneg_bound(K['seq'], O.C_TERM) * r.terms[i]))
    for i in (5, 6):
        worst.append(_worst(f'terms[{i}]', abs(terms[i] - r.terms[i]), O.nonneg_bound(K['mel'], O.C_TERM) * r.terms[i]))
    worst.append(_worst('terms[7]', abs(terms[7] - terms[:7].sum()), 7 * O.U32 * np.abs(terms[:7]).sum()))
    if form != 'terms':
        for k in O.GRAD_ROUNDINGS:
            worst.append(_worst(k, np.abs(grads[k] - r.grads[k]), O.grad_bound(k, r.grads[k])))
        e = np.abs(grads['d_spk'] - r.grads['d_spk'])
        vis = s_dspk >= b0[1] / 4.            # where an ulp of the functions is a quarter of the other roundings or more
        print(f'  d_spk error in ulps of expf / logf, all of it attributed to them, where they would show ({int(vis.sum())} elements): '
              f'{float((e[vis] / s_dspk[vis]).max()) if vis.any() else 0.:.3g}')
        worst.append(_worst('d_spk', e, dspk_bound))
        if post:
            old = old_post.astype(np.float64)
            worst.append(_worst('d_post', np.abs(grads['d_post'] - (old + r.grads['d_post'])), O.post_grad_bound(r.grads['d_post'], old, K['post'])))
    assert max(worst) <= 1., worst
    return terms, grads, r


@pytest.mark.parametrize('form', O.FORMS)
@pytest.mark.parametrize('name', list(O.LOSS_SHAPES))
def test_loss_terms_and_gradients(name, form):
    _check_loss(O.loss_problem(name, seed=1), form)


@pytest.mark.parametrize('form', ['plain', 'tws', 'tnows'])
@pytest.mark.parametrize('name', ['prod', 'wide', 'batch'])
def test_loss_with_a_gradient_scale_and_large_logits(name, form):
    ''' grad_scale != 1 scales every gradient and no term; logits spread over [-80, 80]: only the subtraction of the maximum keeps expf finite '''
    p = O.loss_problem(name, seed=2, logit_scale=80.)
    terms, grads, r = _check_loss(p, form, gs=1. / 48.)
    assert np.isfinite(terms).all() and all(np.isfinite(g).all() for g in grads.values())


@pytest.mark.parametrize('form', O.FORMS)
@pytest.mark.parametrize('name', ['tile1', 'batch'])
def test_loss_without_a_post_multiplier(name, form):
    terms, grads, _ = _check_loss(O.loss_problem(name, seed=3), form, post=False)
    assert terms[1] == 0. and 'd_post' not in grads


@pytest.mark.parametrize('form', ['plain', 'tws', 'tnows'])
def test_loss_with_a_post_multiplier_of_zeros_leaves_its_gradient_alone(form):
    p = O.loss_problem('tile', seed=4)
    p['post'][:] = 0.
    old = np.random.default_rng(8).standard_normal(O.N_POST).astype(np.float32)
    terms, grads, _ = _check_loss(p, form, old_post=old)
    assert terms[1] == 0. and np.array_equal(grads['d_post'], old.astype(np.float64))      # finite and unchanged, bit for bit


@pytest.mark.parametrize('form', ['plain', 'tws', 'tnows', 'terms'])
def test_loss_takes_the_speaker_weight_from_the_step_block(form):
    from daft_exprt import ops
    p = O.loss_problem('prod', seed=5)
    block = torch.zeros(48, dtype=torch.uint8, device=DEV)
    w_block = 0.81
    ops.step_scalars_set(block, 12345, LR, BETAS, 7, w_block)
    assert O.f32(w_block) != O.f32(O.WEIGHTS[0])
    terms, _, r = _check_loss(p, form, step_ptr=block.data_ptr(), oracle_weights=(w_block,) + O.WEIGHTS[1:])
    by_value = O.loss_terms_and_grads(p, O.WEIGHTS).terms[0]
    assert abs(terms[0] - by_value) > 0.5 * abs(r.terms[0] - by_value) > 0.1      # the two weights are far apart: the block's one won


# (kind, f or None, b, c or None, position, impulse): the first and last frame, T - 1 with T % 64 == 1 = the first frame of the second
# tile, the last channel, the last frame of the first tile, the last symbol
IMPULSES = {
    'tile1': [('mel', 0, 0, 0, .5), ('mel', 2, 79, 64, -.5), ('mel', 1, 79, 0, 2.), ('mel', 1, 40, 63, -.25), ('mel', 2, 0, 64, .5),
              ('seq', 0, 0, 0, .5), ('seq', 1, 2, 4, -2.), ('seq', 2, 1, 4, .25)],
    'wide': [('mel', 1, 129, 69, .5), ('mel', 0, 0, 64, -.5), ('mel', 1, 128, 0, 1.), ('seq', 2, 1, 8, .5)],
    'cmax': [('mel', 3, 127, 129, .5), ('mel', 0, 127, 128, -1.), ('seq', 1, 3, 299, .5), ('seq', 0, 2, 256, -.5)],
}


@pytest.mark.parametrize('form', ['plain', 'tws', 'tnows'])
@pytest.mark.parametrize('name', list(IMPULSES))
def test_loss_impulses(name, form):
    ''' pred == tgt but for one power of two: the term is a single summand (K = 0) and the gradient is non-zero at exactly that index '''
    B, L, T, C, S = O.LOSS_SHAPES[name]
    seq_names = ('dur', 'energy', 'pitch')
    for kind, i0, i1, i2, delta in IMPULSES[name]:
        p = O.loss_problem(name, seed=6, grid=True)
        if kind == 'mel':
            b, c, t = i0, i1, i2
            assert b < B and c < C and t < T
            p['mel'][b, c, t] += np.float32(delta)
            assert p['mel'][b, c, t] - p['mel_t'][b, c, t] == delta
            live = {5, 6}
        else:
            f, b, l = i0, i1, i2
            assert b < B and l < L
            p[seq_names[f]][b, l] += np.float32(delta)
            assert p[seq_names[f]][b, l] - p[seq_names[f] + '_t'][b, l] == delta
            live = {2 + f}
        terms, grads, _ = _run_loss(p, form)
        r = O.loss_terms_and_grads(p)
        for i in range(2, 7):
            if i in live:
                assert r.terms[i] > 0 and abs(terms[i] - r.terms[i]) <= O.nonneg_bound(0, O.C_TERM) * r.terms[i], (kind, i0, i1, i2, i)
            else:
                assert terms[i] == 0. == r.terms[i], (kind, i0, i1, i2, i)
        for k in O.GRAD_ROUNDINGS:
            assert np.array_equal(grads[k] != 0, r.grads[k] != 0), (kind, i0, i1, i2, k)
            assert (np.abs(grads[k] - r.grads[k]) <= O.grad_bound(k, r.grads[k])).all(), (kind, i0, i1, i2, k)
        hit = grads['d_mel'][i0, i1, i2] if kind == 'mel' else grads['d_' + seq_names[i0]][i1, i2]
        assert hit != 0 and np.sign(hit) == np.sign(delta)
        assert sum(int((g != 0).sum()) for k, g in grads.items() if k in O.GRAD_ROUNDINGS) == 1


def test_loss_refuses_an_empty_channel_or_class_axis_before_any_launch():
    from daft_exprt import _hip as H
    p = O.loss_problem('one')
    d = {k: torch.from_numpy(p[k]).to(DEV) for k in LOSS_KEYS}
    terms, whole = _guarded((8,))
    for C, S, n_post in ((0, 1, 0), (1, 0, 0), (1, 1, -1)):
        rc = H.lib().dx_loss_fwd_bwd(*[H.ptr(d[k]) for k in LOSS_KEYS], None, None, None, None, None, None, None, H.ptr(terms), None,
                                     2, 1, 1, C, S, n_post, 1., 1., 1., 1., 1., 1., 1., 0, None, H.stream())
        assert rc == -2 and b'dx_loss_fwd_bwd' in H.lib().dx_last_error()          # DX_ERR_SHAPE
    torch.cuda.synchronize()
    assert bool((whole == SENT).all())


# ---------------------------------------------------------------------------------------------------- dx_sumsq
def _sumsq(buf, off, n):
    from daft_exprt import _hip as H
    from daft_exprt import ops
    out = torch.full((1,), 1e30, dtype=torch.float32, device=DEV)       # overwritten, not accumulated
    assert buf.data_ptr() % 16 == 0 and buf.numel() >= n + 16
    if n:
        x = buf[4 + off:4 + off + n]
        assert x.data_ptr() == buf.data_ptr() + 4 * (4 + off) and x.numel() == n
        ops.sumsq(x, out)
    else:          # (an empty view has no pointer to hand over)
        H.check(H.lib().dx_sumsq(buf.data_ptr() + 4 * (4 + off), 0, H.ptr(out), H.stream()))
    return float(out.item())


@pytest.mark.parametrize('n', O.SUMSQ_SMALL + (O.SUMSQ_BIG,))
def test_sumsq_against_float64_at_every_alignment(n):
    g = torch.Generator(device=DEV).manual_seed(n)
    buf = torch.randn(n + 16, generator=g, device=DEV) * 3.
    host = _f64(buf)
    worst = []
    for off in range(4):
        ref = float((host[4 + off:4 + off + n] ** 2).sum())
        got = _sumsq(buf, off, n)
        geo = O.sumsq_geometry(n, off)
        if n == 0:
            assert got == 0.
        worst.append(_worst(f'n = {n}, offset {off} (head {geo["head"]}, tail {geo["tail"]})', abs(got - ref), O.nonneg_bound(geo['K'], O.C_SQ) * ref))
    assert max(worst) <= 1., worst


@pytest.mark.parametrize('n', [5, 1023, 2049, O.SUMSQ_BIG])
def test_sumsq_impulses_are_exact(n):
    ''' zeros but for one small integer, in the head, the first quad, the last quad of the unrolled loop, the remainder loop, the tail
        and at the end: the square comes back bit for bit, and nothing behind the end is read '''
    buf = torch.empty(n + 16, device=DEV)
    seen = set()
    for off in range(4):
        buf.zero_()
        buf[:4 + off] = 7.            # in front of the start and behind the end
        buf[4 + off + n:] = 7.
        for where, i in O.sumsq_positions(n, off).items():
            buf[4 + off + i] = 3.
            got = _sumsq(buf, off, n)
            buf[4 + off + i] = 0.
            assert got == 9., (off, where, i, got)
            seen.add(where)
    assert seen >= {'head', 'first_quad', 'tail', 'last', 'remainder'} and (n != O.SUMSQ_BIG or 'last_unrolled' in seen)


# ---------------------------------------------------------------------------------------------------- dx_adam_step
def _adam_state(n, seed):
    ''' p, m, v and three gradients; from n = 4 on, element 0: all zeros, every step (must stay exactly zero); element 1: m = v = 0 and |g| ~ 1e-10,
        where eps = 1e-9 dominates the denominator; element 2: a zero gradient on a live state '''
    r = np.random.default_rng(seed)
    p = r.standard_normal(n).astype(np.float32)
    m = (r.standard_normal(n) * 1e-2).astype(np.float32)
    v = (r.random(n) * 1e-4).astype(np.float32)
    gs = [(r.standard_normal(n) * 1e-2).astype(np.float32) for _ in range(3)]
    if n >= 4:
        p[0] = m[0] = v[0] = m[1] = v[1] = 0.
        for t, g in enumerate(gs):
            g[0] = g[2] = 0.
            g[1] = (1. + t) * 1e-10 * (-1) ** t
    return p, m, v, gs


def _slice_of(a, off, fill=SENT):
    whole = torch.full((a.size + 8,), fill, dtype=torch.float32, device=DEV)
    whole[off:off + a.size] = torch.from_numpy(a)
    return whole[off:off + a.size], whole


def _outside_intact(whole, off, n, fill=SENT):
    return bool((whole[:off] == fill).all()) and bool((whole[off + n:] == fill).all())


@pytest.mark.parametrize('clip', ['inf', 'loose', 'binding'])
@pytest.mark.parametrize('wd', [0., 1e-6, 0.1])
@pytest.mark.parametrize('n', O.ADAM_SIZES)
def test_adam_three_steps_on_slices(n, wd, clip):
    from daft_exprt import ops
    worst = []
    for off in (1, 3):
        p0, m0, v0, gs = _adam_state(n, 10 * n + off)
        (p, pw), (m, mw), (v, vw) = _slice_of(p0, off), _slice_of(m0, off), _slice_of(v0, off)
        for t, g_host in enumerate(gs, start=1):
            g, gw = _slice_of(g_host, off)
            prev = [_f64(x) for x in (p, m, v)]
            g64 = g_host.astype(np.float64)
            norm = math.sqrt(float((g64 ** 2).sum()))
            thresh = {'inf': math.inf, 'loose': 3. * norm, 'binding': norm / 10.}[clip]
            gn = None
            if clip != 'inf':      # the norm the clipping uses comes from dx_sumsq on the same slice, and is held to float64 on its own
                gn = ops.sumsq(g)
                geo = O.sumsq_geometry(n, off)
                worst.append(_worst('sumsq', abs(float(gn.item()) - norm * norm), O.nonneg_bound(geo['K'], O.C_SQ) * norm * norm))
            accum = torch.full((1,), 5.5, dtype=torch.float32, device=DEV)
            ops.adam_step(p, g, m, v, LR, BETAS, EPS, wd, t, grad_norm_sq=gn, clip_thresh=thresh, norm_accum=accum)
            res = O.adam(*prev[:1], g64, *prev[1:], LR, BETAS, EPS, wd, t, clip=thresh, gnorm_sq=None if gn is None else float(gn.item()))
            assert (res.coef == 1.) == (clip != 'binding') and (clip != 'binding' or 0.09 < res.coef < 0.11)
            for name, dev, ref, bound in (('p', p, res.p, res.ep), ('m', m, res.m, res.em), ('v', v, res.v, res.ev)):
                got = _f64(dev)
                assert np.isfinite(got).all()
                worst.append(_worst(f'{name} (offset {off}, step {t})', np.abs(got - ref), bound))
                assert n < 4 or got[0] == 0., 'the all-zero element moved'
            assert float(accum.item()) >= 5.5
            worst.append(_worst('norm_accum', abs(float(accum.item()) - (5.5 + res.gsq)), O.nonneg_bound(O.adam_chain(n), O.C_SQ) * (5.5 + res.gsq)))
            assert all(_outside_intact(w, off, n) for w in (pw, mw, vw, gw)) and np.array_equal(g.cpu().numpy(), g_host)
    assert max(worst) <= 1., worst


@pytest.mark.parametrize('n', [257, 70001])
def test_adam_takes_lr_and_bias_corrections_from_the_step_block(n, monkeypatch):
    from daft_exprt import ops
    t_block, off, wd = 5, 3, 1e-6
    block = torch.zeros(48, dtype=torch.uint8, device=DEV)
    ops.step_scalars_set(block, 99, LR, BETAS, t_block, 0.3)
    p0, m0, v0, gs = _adam_state(n, n)
    (p, pw), (m, mw), (v, vw), (g, gw) = _slice_of(p0, off), _slice_of(m0, off), _slice_of(v0, off), _slice_of(gs[0], off)
    monkeypatch.setattr(ops, 'STEP_PTR', block.data_ptr())
    ops.adam_step(p, g, m, v, 2. * LR, BETAS, EPS, wd, 1)            # by value: another lr, another step
    monkeypatch.setattr(ops, 'STEP_PTR', None)
    res = O.adam(p0, gs[0], m0, v0, None, BETAS, EPS, wd, None, scalars=O.step_scalars(LR, BETAS, t_block))
    by_value = O.adam(p0, gs[0], m0, v0, 2. * LR, BETAS, EPS, wd, 1)
    worst = [_worst(k, np.abs(_f64(dev) - ref), bound) for k, dev, ref, bound in (('p', p, res.p, res.ep), ('m', m, res.m, res.em), ('v', v, res.v, res.ev))]
    assert max(worst) <= 1., worst
    assert float(np.abs(by_value.p - res.p).max()) > 100 * float(res.ep.max())          # the by-value scalars would have been seen
    assert all(_outside_intact(w, off, n) for w in (pw, mw, vw, gw))


def test_adam_refuses_bad_arguments_before_any_launch():
    from daft_exprt import _hip as H
    x, whole = _guarded((8,))
    for args in ((0, 1), (-1, 1), (8, 0)):
        rc = H.lib().dx_adam_step(H.ptr(x), H.ptr(x), H.ptr(x), H.ptr(x), args[0], LR, 0.9, 0.98, EPS, 0., args[1], None, math.inf, None, None, H.stream())
        assert rc == -1 and b'dx_adam_step' in H.lib().dx_last_error()            # DX_ERR_ARG
    assert H.lib().dx_sumsq(H.ptr(x), -1, H.ptr(x), H.stream()) == -1
    torch.cuda.synchronize()
    assert bool((whole == SENT).all())


# ---------------------------------------------------------------------------------------------------- dx_adam_pack_step
@pytest.mark.parametrize('use_block', [False, True], ids=['by_value', 'step_block'])
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32], ids=['bf16', 'fp32'])
def test_fused_adam_on_a_hand_built_table(dtype, use_block):
    from daft_exprt import ops
    ws, fs, total, live = O.pack_plan()
    wd = 1e-6
    r = np.random.default_rng(17)
    host = {'p': r.standard_normal(total), 'm': r.standard_normal(total) * 1e-2, 'v': r.random(total) * 1e-4}
    dev = {}
    for k, a in host.items():
        a = a.astype(np.float32)
        a[~live] = SENT
        dev[k] = torch.from_numpy(a).to(DEV)
    copies, entries = [], []
    for off, (cout, cin, taps), frag in ws:
        n = cout * cin * taps
        c = {k: _guarded((n,), dtype=dtype) for k in ('fwd', 'tr')}
        if frag and dtype == torch.bfloat16:
            c.update({k: _guarded((n,), dtype=dtype) for k in ('frag_fwd', 'frag_tr')})
            assert all(c[k][0].data_ptr() % 16 == 0 for k in ('frag_fwd', 'frag_tr'))
        copies.append(c)
        entries.append((off, (cout, cin, taps), c['fwd'][0], c['tr'][0], c.get('frag_fwd', (None,))[0], c.get('frag_tr', (None,))[0]))
    table = ops.adam_pack_table(entries, fs, DEV)
    K = O.adam_pack_chain([shp for _, shp, _ in ws], [n for _, n in fs])
    block = torch.zeros(48, dtype=torch.uint8, device=DEV)
    worst = []
    for t in (1, 2):
        g_host = (r.standard_normal(total) * 1e-2).astype(np.float32)
        g_host[~live] = SENT
        g = torch.from_numpy(g_host).to(DEV)
        prev = {k: _f64(x) for k, x in dev.items()}
        accum = torch.full((1,), 5.5, dtype=torch.float32, device=DEV)
        if use_block:      # the block carries step t and LR; by value: step 1 and twice the rate
            ops.step_scalars_set(block, 0, LR, BETAS, t, 0.)
            ops.STEP_PTR = block.data_ptr()
        try:
            ops.adam_pack_step(dev['p'], g, dev['m'], dev['v'], table, dtype, 2. * LR if use_block else LR, BETAS, EPS, wd, 1 if use_block else t,
                               norm_accum=accum)
        finally:
            ops.STEP_PTR = None
        torch.cuda.synchronize()
        res = O.adam(prev['p'][live], g_host[live].astype(np.float64), prev['m'][live], prev['v'][live], LR, BETAS, EPS, wd, t)
        for k, ref, bound in (('p', res.p, res.ep), ('m', res.m, res.em), ('v', res.v, res.ev)):
            got = _f64(dev[k])
            assert np.array_equal(got[~live], np.full(int((~live).sum()), SENT)), f'{k}: a gap between the entries was written'
            worst.append(_worst(f'{k} (step {t})', np.abs(got[live] - ref), bound))
        assert np.array_equal(g.cpu().numpy(), g_host)
        worst.append(_worst('norm_accum', abs(float(accum.item()) - (5.5 + res.gsq)), O.nonneg_bound(K, O.C_SQ) * (5.5 + res.gsq)))
        # every copy is the device's own updated p, cast and gathered through the oracle's statement of the layout
        for (off, (cout, cin, taps), frag), c in zip(ws, copies):
            lay = O.pack_layouts(off, cout, cin, taps)
            assert set(c) == (set(lay) if dtype == torch.bfloat16 else {'fwd', 'tr'})
            for k, (view, whole) in c.items():
                want = dev['p'][torch.from_numpy(lay[k]).to(DEV)].to(dtype)
                assert torch.equal(view, want), f'{k} copy of ({cout}, {cin}, {taps}) at step {t}'
                assert _guards_intact(whole), f'{k} copy of ({cout}, {cin}, {taps}): written outside'
    assert max(worst) <= 1., worst
