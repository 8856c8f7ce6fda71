"""tests/conv_ln_oracle.py checked on the CPU: its forward and its closed-form backward against float64 autograd through torch's own
conv -> dropout -> + residual -> layer_norm -> FiLM -> mask, its convolution against oracle.daft_exprt_cpu.conv1d_cl, its tile plan
against the heights the cases were chosen for, and the two conditions on the INPUTS of tests/test_gpu_conv_ln.py -- the low-precision
restatement stays within the cap (so no bound of that file can go slack), and the mask readout separates kept from dropped."""
import pytest
import torch

from oracle import daft_exprt_cpu as O
from tests import conv_ln_oracle as K
from tests import layernorm_oracle as L

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16


def _close(got, want, rel=1e-11):
    return float((got - want).abs().max()) <= rel * float(want.abs().max())


def _torch_forward(c, x, residual, gamma, beta, film):
    ''' the fused op from torch's own pieces, float64, differentiable '''
    v = O.conv1d_cl(x, c.w.double(), c.bias.double())
    keep, scale = K.keep_of(c)
    if keep is not None:
        v = v * keep.double() * scale
    if c.vres is not None:
        m1, r1, rg, rb = (K._clean(t, F64) for t in c.vres)
        residual = ((residual - m1[:, :, None]) * r1[:, :, None] * rg + rb) * c.live[:, :, None]
    s = v + residual
    t = torch.nn.functional.layer_norm(s, (128,), gamma, beta, eps=1e-5)
    if film is not None:
        t = film[:, None, :128] * t + film[:, None, 128:]
    return t * c.live[:, :, None], s


AUTOGRAD = [(name, taps, o) for name in ('F1', 'T1') for taps in (3, 1) for o in range(4)]


@pytest.mark.parametrize('name,taps,o', AUTOGRAD)
def test_forward_equals_torch_composition(name, taps, o):
    ''' every forward option: FiLM, p_pre 0 / 0.1 / 0.5, the re-derived residual '''
    film, p, _, _, _, vres, n2 = K.FWD_OPTS[o]
    c = K.make_case(name, 128, taps, 'fp32', False, film=film is not None, p_pre=p, vres=vres, n2=n2)
    ref = K.reference_fwd(c, K.SPLITK)
    leaf = lambda t: None if t is None else K._clean(t, F64)
    y, s = _torch_forward(c, leaf(c.x), leaf(c.residual), leaf(c.gamma), leaf(c.beta), leaf(c.film))
    assert _close(ref['y'], y) and _close(ref['s'], s * c.live[:, :, None])
    fixed = K.reference_fwd(c, K.ROWS64)          # fixed tiles: s of the live tiles' dead rows is computed too
    comp = K.computed_rows(c, K.ROWS64)
    assert _close(fixed['s'], s * comp[:, :, None]) and int((comp & ~c.live).sum()) > 0
    if n2:
        want = y.to(BF16).double() @ c.w2.double().T + c.b2.double()
        assert _close(ref['y2'], want * c.live[:, :, None])


@pytest.mark.parametrize('name,taps,o', AUTOGRAD)
def test_closed_form_backward_equals_autograd(name, taps, o):
    ''' u = the conv output that was dropped out in front of the LayerNorm, r the residual: s = keep * scale * u + r, y = mask(FiLM(LN(s))),
        z = conv(y, W) the forward conv 128 -> Cin whose output gradient is the kernel's x; d(sum z * x + sum y * y_inout) / d(r, u, gamma,
        beta, film) = ds, dx, dgamma, dbeta, dfilm -- through the transposed, tap-flipped weight the kernel is handed '''
    film, p, w2 = K.BWD_OPTS[o]
    c = K.make_case(name, 256, taps, 'fp32', True, film=film is not None, p_pre=p, n2=128 if w2 else 0)
    s_in = K._clean(c.s_in, F64)
    mean, rstd = K._stats(s_in)
    ref = K.reference_bwd(c, (s_in, mean, rstd))
    leaf = lambda t: None if t is None else K._clean(t, F64).requires_grad_(True)
    r, u, gamma, beta, flm = leaf(c.s_in), leaf(torch.zeros_like(c.s_in)), leaf(c.gamma), leaf(c.beta), leaf(c.film)
    keep, scale = K.keep_of(c)
    s = (u if keep is None else u * keep.double() * scale) + r
    t = torch.nn.functional.layer_norm(s, (128,), gamma, beta, eps=1e-5)
    if flm is not None:
        t = flm[:, None, :128] * t + flm[:, None, 128:]
    y = t * c.live[:, :, None]
    z = O.conv1d_cl(y, c.w_fwd.double(), torch.zeros(c.Cin, dtype=F64))
    ((z * K._clean(c.x, F64)).sum() + (y * K._clean(c.yin, F64)).sum()).backward()
    live = c.live[:, :, None]
    assert _close(ref['ds'], r.grad * live) and _close(ref['dx_lp'], u.grad * live)
    assert _close(ref['dgamma'] - c.init[0].double(), gamma.grad) and _close(ref['dbeta'] - c.init[1].double(), beta.grad)
    if flm is not None:
        assert _close(ref['dfilm'] - c.init[2].double(), flm.grad)
    if w2:
        assert _close(ref['y2b'], ref['dx_lp'].to(BF16).double() @ c.w2.double().T)
    for t_ in ('ds', 'dx_lp', 'dgamma', 'dbeta'):
        assert float(ref[t_].abs().max()) > 0.1 and bool(torch.isfinite(ref[t_]).all())


@pytest.mark.parametrize('taps', [1, 3])
def test_reference_convolution_equals_conv1d_cl(taps):
    g = torch.Generator().manual_seed(taps)
    x, w, b = torch.randn(3, 70, 48, generator=g, dtype=F64), torch.randn(128, 48, taps, generator=g, dtype=F64), torch.randn(128, generator=g, dtype=F64)
    want = O.conv1d_cl(x, w, b)
    assert _close(K.conv(x, w) + b, want, 1e-13)
    for step, fp32 in ((16, False), (2, True)):            # the chain is the same sum in fp32
        assert float((K.conv_chain(x.float(), w.float(), step, fp32).double() + b - want).abs().max()) <= 1e-5 * float(want.abs().max())


def test_plan_restatement_reaches_every_branch():
    ''' the heights the cases were chosen for, and through them every main-loop variant of conv_sk_kernel: NA 1..6, both KS, tall tiles '''
    seen, tall = set(), 0
    for name, heights in K.HEIGHTS.items():
        B, N, lens, _, _ = K.CASES[name]
        table = K.tile_plan(lens, N, K.plan_tiles(name))
        assert len(table) == K.plan_tiles(name)
        for b in range(B):
            rows = sorted((n0, h) for tb, n0, h, _ in table if tb == b and h > 0)
            assert [h for _, h in rows] == heights[b], (name, b, rows)
            assert [n0 for n0, _ in rows] == [sum(heights[b][:j]) for j in range(len(rows))] and sum(heights[b]) == lens[b]
            for h in heights[b]:
                parts = K.splitk_branches(h)
                tall += len(parts) == 2
                seen.update((na, ks) for _, na, ks in parts)
    assert seen == {(1, 4), (2, 4), (3, 4), (4, 4), (5, 2), (6, 2)}, seen
    assert tall == 3
    assert [K.splitk_branches(h) for h in (256, 250, 193)] == [[(128, 4, 4), (128, 4, 4)], [(128, 4, 4), (122, 4, 4)], [(128, 4, 4), (65, 3, 4)]]
    assert [K.splitk_branches(h)[0][1:] for h in (192, 161, 160, 129)] == [(6, 2), (6, 2), (5, 2), (5, 2)]
    # T5: the default plan, 256 entries of at most 3 rows, an empty utterance without a tile, the padding rows shared out
    table = K.tile_plan(K.CASES['T5'][2], 300, K.plan_tiles('T5'))
    assert len(table) == 256 and max(h for _, _, h, _ in table) == 3 and not any(b == 3 for b, _, h, _ in table if h > 0)
    assert table[0][3] == -(-(0 + 48 + 297 + 300) // 256)
    # fixed tiles: where the computed rows of s end
    assert [K.live_end(l, 70, 64) for l in (70, 33, 51)] == [70, 64, 64] and K.live_end(62, 300, 64) == 64 and K.live_end(63, 300, 64) == 128
    assert K.live_end(0, 1001, 128) == 128 and K.live_end(1001, 1001, 128) == 1001


def _cap_check(c, ref, low, worst):
    for t in ref:
        kind = K.kind_of(c, t)
        for b, fe in L.regions(c, t):
            if fe == 0:
                continue
            assert bool(torch.isfinite(L.region(ref[t], t, b, fe)).all()) and bool(torch.isfinite(L.region(low[t], t, b, fe)).all()), (t, b)
            _, frac = L.bound(low, ref, t, b, fe)
            worst[kind] = max(worst[kind], frac)
            assert frac <= K.CAP[kind], ('restatement too far from float64: change the inputs', K.config_id((0,) + (c.name, c.Cin, c.taps, c.pair)), t, b, frac)


@pytest.mark.parametrize('cfg', K.FWD_CONFIGS, ids=[K.config_id(c) for c in K.FWD_CONFIGS])
def test_forward_restatement_stays_within_the_cap(cfg):
    ''' max|restatement - float64| <= CAP * max|float64| per utterance and tensor, every option row (F2: its first four utterances) '''
    path, name, cin, taps, pair = cfg
    worst = {'fp32': 0., 'mixed': 0., 'bf16': 0.}
    for o in range(4):
        film, p, _, _, _, vres, n2 = K.fwd_opts(cfg, o)
        c = K.make_case(name, cin, taps, pair, False, film=film is not None, p_pre=p, vres=vres, n2=n2, B=4 if name == 'F2' else None)
        _cap_check(c, K.reference_fwd(c, path), K.restate_fwd(c, path), worst)
    print(f'CAP fwd {K.config_id(cfg)}:', ' '.join(f'{k} {v:.2e}' for k, v in worst.items()))


@pytest.mark.parametrize('cfg', K.BWD_CONFIGS, ids=[K.config_id(c) for c in K.BWD_CONFIGS])
def test_backward_restatement_stays_within_the_cap(cfg):
    ''' the backward alone (the float64 statistics rounded to fp32) and chained (each arithmetic's own forward) '''
    path, name, cin, taps, pair = cfg
    worst = {'fp32': 0., 'mixed': 0., 'bf16': 0.}
    for o in range(4):
        film, p, w2 = K.bwd_opts(cfg, o)
        c = K.make_case(name, cin, taps, pair, True, film=film is not None, p_pre=p, n2=128 if w2 else 0, B=4 if name == 'F2' else None)
        _cap_check(c, K.reference_bwd(c), K.restate_bwd(c), worst)
        if o == 0 and path != K.PLAN_K1:
            f = K.make_case(name, cin, taps, pair, False, film=True, p_pre=p, B=4 if name == 'F2' else None)
            rf, lf = K.reference_fwd(f, path), K.restate_fwd(f, path)
            _cap_check(c, K.reference_bwd(c, (rf['s'], rf['mean'], rf['rstd'])), K.restate_bwd(c, (lf['s'], lf['mean'], lf['rstd'])), worst)
    print(f'CAP bwd {K.config_id(cfg)}:', ' '.join(f'{k} {v:.2e}' for k, v in worst.items()))
    assert K.CAP['fp32'] <= 2e-5 and K.CAP['mixed'] <= 8e-3 and K.CAP['bf16'] <= 8e-3


@pytest.mark.parametrize('p', [0.1, 0.5])
def test_mask_readout_separates_kept_from_dropped(p):
    ''' with the restatement standing in for the kernel: s != 0 (forward) and dx_lp != 0 (backward) are elem_keep's bits on the live rows;
        every kept element of the reference is READOUT_MARGIN away from zero and every dropped one exactly zero '''
    for backward in (False, True):
        c = K.readout_case(backward, p)
        keep, _ = K.keep_of(c)
        live = c.live[:, :, None].expand_as(keep)
        assert 0 < int((~keep[live]).sum()) < int(live.sum()) * (p + 0.05)
        if not backward:
            ref, low = K.reference_fwd(c, K.SPLITK)['s'], K.restate_fwd(c, K.SPLITK)['s']
        else:
            ref, low = K.reference_bwd(c)['dx_lp'], K.restate_bwd(c)['dx_lp']
            assert float(K.reference_bwd(c)['ds'][live].abs().min()) >= K.READOUT_MARGIN
        assert torch.equal((low != 0)[live], keep[live])
        assert float(ref[live & keep].abs().min()) >= K.READOUT_MARGIN and not bool(ref[live & ~keep].any())
