"""K28 (csrc/aligner.hip) and daft_exprt/aligner.py on the GPU against tests/aligner_oracle.py.

MAS is an integer decision on fp32 comparisons: on lattices whose fp32 sums are exact it must equal the oracle bit for bit.  The
float kernels are compared with the float64 oracle on the same (fp32-representable) inputs; the tolerance is worked out at run
time as max(2 x the deviation of the float32 restatement from the float64 one, a floor) -- see `_tolerance`.  Every launch gets
its dead inputs as NaN and its outputs and workspaces pre-filled with NaN / garbage, and every utterance is run in the ragged
batch, in the batch with larger padded extents, and alone: the three must agree bit for bit."""
import functools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import align_oracle as AO
from tests import aligner_oracle as O
from tests.util import make_hparams

DEV = 'cuda:0'
EPS = float(np.finfo(np.float32).eps)
# (n_frm, n_sym): the smallest, the forced diagonal, and one and two wave boundaries; then rows without a path and empty rows
SHAPES = ((1, 1), (2, 1), (2, 2), (5, 5), (9, 2), (70, 63), (70, 64), (70, 65), (200, 150))
DEAD = ((3, 5), (0, 4), (6, 0))
TAU, SIGMA = 0.05, 0.4


def _tolerance(hi, lo, scale):
    ''' max(2 x what rounding itself does, a floor).  hi / lo: the float64 oracle and its float32 restatement on the same inputs.
        The floor is 16 eps32 x max(1, scale), `scale` the largest magnitude that enters the quantity (the scores of a softmax row,
        the alpha that are subtracted in an exponent): one fp32 rounding of a value of that
        magnitude is eps x scale / 2, and every output is a handful of such operations (difference, max-shift, exp, log) however
        short the sequence -- 32 half-ulps keeps shapes whose restatement happens to round exactly (one cell, one frame) from
        demanding more than the format holds. '''
    with np.errstate(invalid='ignore'):
        d = np.abs(np.asarray(hi, dtype=np.float64) - np.asarray(lo, dtype=np.float64))
    d = d[np.isfinite(d)]
    return max(2.0 * (float(d.max()) if d.size else 0.0), 16.0 * EPS * max(1.0, float(scale)))


def _sum_tolerance(hi, lo, terms):
    ''' the same rule for dq / dk, which are plain sums of n products taken in order: the floor is 4 eps32 x the largest sum of
        the |terms| of one output element (`_case` works it out in float64).  Adding n numbers one after the other is off by at
        most (n - 1) half-ulps of that sum to first order, and every term carries its own few roundings (a difference, an exp, two
        products): 8 half-ulps is that bound for the shortest sums of these tests and far below it for the long ones, where the
        float32 restatement, which adds in the same order, decides. '''
    d = np.abs(np.asarray(hi, dtype=np.float64) - np.asarray(lo, dtype=np.float64))
    return max(2.0 * float(d.max()), 4.0 * EPS * float(terms))


def _gradient_terms(c, b, nf, ns):
    ''' max over the elements of dq[b] / dk[b] of the sum of |2 tau ds (q - k)| over the axis the element reduces, in float64 '''
    q, k, logp, g = (c[name].astype(np.float64) for name in ('q', 'k', 'logp', 'g'))
    ds = g[b, :nf, :ns] - np.exp(logp[b, :nf, :ns]) * g[b, :nf, :ns].sum(axis=1, keepdims=True)
    over_l = over_t = 0.0
    for a in range(c['A']):
        x = np.abs(ds * (q[b, :nf, a][:, None] - k[b, None, :ns, a]))
        over_l, over_t = max(over_l, float(x.sum(axis=1).max())), max(over_t, float(x.sum(axis=0).max()))
    return 2 * TAU * over_l, 2 * TAU * over_t


def _close(name, got, want, tol):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.array_equal(np.isneginf(got), np.isneginf(want)), name
    assert np.array_equal(np.isnan(got), np.isnan(want)), name
    fin = np.isfinite(want)
    err = float(np.abs(got[fin] - want[fin]).max()) if fin.any() else 0.0
    print(f'{name}: max error {err:.3e}, tolerance {tol:.3e}')
    assert err <= tol, (name, err, tol)


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if dtype is None else torch.tensor(a, dtype=dtype, device=DEV)


def _embed(x, shape, lengths, fill=np.nan):
    ''' x (B, n0, n1) -> `shape`, everything at or past lengths[axis][b] and everything new filled with `fill` '''
    out = np.full(shape, fill, dtype=x.dtype)
    for b in range(x.shape[0]):
        n0, n1 = (int(l[b]) if l is not None else x.shape[1 + i] for i, l in enumerate(lengths))
        out[b, :n0, :n1] = x[b, :n0, :n1]
    return out


@functools.lru_cache(maxsize=None)
def _case(A, shapes=SHAPES + DEAD, seed=0):
    ''' a ragged batch: fp32 inputs, the float64 oracle and the float32 restatement of every quantity, computed once '''
    rng = np.random.RandomState(seed + A)
    B, T, L = len(shapes), max(s[0] for s in shapes), max(s[1] for s in shapes)
    n_frm, n_sym = np.array([s[0] for s in shapes], dtype=np.int64), np.array([s[1] for s in shapes], dtype=np.int64)
    q = (rng.standard_normal((B, T, A)) * (6.0 / np.sqrt(A)) ** 0.5).astype(np.float32)
    k = (rng.standard_normal((B, L, A)) * (6.0 / np.sqrt(A)) ** 0.5).astype(np.float32)
    c = dict(A=A, B=B, T=T, L=L, n_frm=n_frm, n_sym=n_sym, q=q, k=k)
    c['g'] = rng.standard_normal((B, T, L)).astype(np.float32)
    c['w'] = rng.uniform(0.5, 2.0, size=B).astype(np.float32)
    for tag, dt in (('hi', np.float64), ('lo', np.float32)):
        c['logp_' + tag] = O.logprob_fwd(q, k, n_frm, n_sym, TAU, SIGMA, dt)
    c['logp'] = c['logp_hi'].astype(np.float32)                         # the input of the kernels downstream
    c['alpha'] = O.forward_sum(c['logp'], n_frm, n_sym)[0].astype(np.float32)
    for tag, dt in (('hi', np.float64), ('lo', np.float32)):
        c['dq_' + tag], c['dk_' + tag] = O.logprob_bwd(q, k, c['logp'], c['g'], n_frm, n_sym, TAU, dt)
        c['alpha_' + tag], c['loss_' + tag], c['status'] = O.forward_sum(c['logp'], n_frm, n_sym, dt)
        c['dlogp_' + tag] = O.forward_sum_bwd(c['logp'], c['alpha'], c['w'], n_frm, n_sym, dt)
        c['gamma_' + tag] = O.forward_sum_bwd(c['logp'], c['alpha'], c['w'], n_frm, n_sym, dt, return_gamma=True)
    c['scores'] = 1.0 / (2 * SIGMA ** 2) + max(float(np.abs(TAU * ((q[b, :nf, None] - k[b, None, :ns]) ** 2).sum(-1)).max()) for b, (nf, ns) in enumerate(shapes)
                      if nf and ns)
    c['terms'] = [_gradient_terms(c, b, nf, ns) if nf and ns else (0.0, 0.0) for b, (nf, ns) in enumerate(shapes)]
    return c


def _run(c, rows=None, pad=(0, 0)):
    ''' the five entry points on the utterances `rows` of a case (all by default) with the tight extents plus `pad`; dead inputs
        NaN, outputs and workspaces poisoned.  Returns NumPy outputs. '''
    from daft_exprt import _hip as H
    lib = H.lib()
    rows = list(range(c['B'])) if rows is None else rows
    n_frm, n_sym = c['n_frm'][rows], c['n_sym'][rows]
    B, A = len(rows), c['A']
    T, L = max(1, int(n_frm.max())) + pad[0], max(1, int(n_sym.max())) + pad[1]
    q = _dev(_embed(c['q'][rows], (B, T, A), (n_frm, None)))
    k = _dev(_embed(c['k'][rows], (B, L, A), (n_sym, None)))
    logp, g, alpha = (_dev(_embed(c[name][rows], (B, T, L), (n_frm, n_sym))) for name in ('logp', 'g', 'alpha'))
    nf, ns, w = _dev(n_frm), _dev(n_sym), _dev(c['w'][rows])
    nan = lambda *shape: torch.full(shape, float('nan'), dtype=torch.float32, device=DEV)
    junk = lambda *shape: torch.full(shape, -77, dtype=torch.int32, device=DEV)
    o = dict(logp=nan(B, T, L), dq=nan(B, T, A), dk=nan(B, L, A), alpha=nan(B, T, L), loss=nan(B), dlogp=nan(B, T, L), score=nan(B),
             status=junk(B), mas_status=junk(B), path=junk(B, T + L - 1, 2), path_len=junk(B))
    row_ws = nan(B, T)
    words = T * ((L + 63) // 64)
    ws = torch.full((B, words), -1, dtype=torch.int64, device=DEV)           # every direction bit set
    s = H.stream()
    H.check(lib.dx_aln_logprob_fwd(H.ptr(q), H.ptr(k), H.ptr(nf), H.ptr(ns), TAU, SIGMA, H.ptr(o['logp']), B, T, L, A, s))
    H.check(lib.dx_aln_logprob_bwd(H.ptr(q), H.ptr(k), H.ptr(logp), H.ptr(g), H.ptr(nf), H.ptr(ns), TAU, H.ptr(o['dq']), H.ptr(o['dk']),
                                   H.ptr(row_ws), B, T, L, A, s))
    H.check(lib.dx_aln_forward_sum(H.ptr(logp), H.ptr(nf), H.ptr(ns), H.ptr(o['alpha']), H.ptr(o['loss']), H.ptr(o['status']), B, T, L, s))
    H.check(lib.dx_aln_forward_sum_bwd(H.ptr(logp), H.ptr(alpha), H.ptr(w), H.ptr(nf), H.ptr(ns), H.ptr(o['dlogp']), B, T, L, s))
    H.check(lib.dx_aln_mas(H.ptr(logp), H.ptr(nf), H.ptr(ns), H.ptr(o['score']), H.ptr(o['path']), H.ptr(o['path_len']),
                           H.ptr(o['mas_status']), H.ptr(ws), 8 * words, B, T, L, s))
    return {name: t.cpu().numpy() for name, t in o.items()}


def _live(name, out, b, nf, ns):
    ''' the bytes of utterance b's live part of an output, after checking that the rest of the row holds the dead value '''
    x = out[name][b]
    if name in ('logp', 'alpha', 'dlogp'):
        assert not x[nf:].any() and not x[:, ns:].any(), name
        assert not np.signbit(x[nf:]).any() and not np.signbit(x[:, ns:]).any(), name
        return x[:nf, :ns].tobytes()
    if name in ('dq', 'dk'):
        n = nf if name == 'dq' else ns
        assert not x[n:].any(), name
        return x[:n].tobytes()
    if name == 'path':
        n = int(out['path_len'][b])
        assert (x[n:] == -1).all()
        return x[:n].tobytes()
    return x.tobytes()


@pytest.mark.parametrize('A', [1, 32, 80])
def test_kernels_against_float64_alone_in_a_batch_and_padded(A):
    c = _case(A)
    batch, wide, again = _run(c), _run(c, pad=(3, 67)), _run(c)
    for name in batch:                                                       # two runs: bit-equal
        assert batch[name].tobytes() == again[name].tobytes(), name
    assert batch['status'].tolist() == c['status'].tolist() == batch['mas_status'].tolist() == [0] * len(SHAPES) + [1, 2, 2]
    path, path_len, score, _ = O.mas(c['logp'], c['n_frm'], c['n_sym'])
    score32 = O.mas(c['logp'], c['n_frm'], c['n_sym'], np.float32)[2]
    for b, (nf, ns) in enumerate(SHAPES + DEAD):
        alone = _run(c, rows=[b])
        for name in batch:
            assert _live(name, batch, b, nf, ns) == _live(name, wide, b, nf, ns) == _live(name, alone, 0, nf, ns), (name, nf, ns)
        tag = f'A={A} {nf}x{ns} '
        live = (slice(b, b + 1), slice(0, nf), slice(0, ns))
        if c['status'][b] != 0:
            assert np.isnan(batch['loss'][b]) and np.isnan(batch['score'][b]) and batch['path_len'][b] == 0
            assert not batch['alpha'][b].any() and not batch['dlogp'][b].any() and (batch['path'][b] == -1).all()
        if nf == 0 or ns == 0:
            assert not batch['logp'][b].any() and not batch['dq'][b].any() and not batch['dk'][b].any()
            continue
        _close(tag + 'logp', batch['logp'][live], c['logp_hi'][live], _tolerance(c['logp_hi'][live], c['logp_lo'][live], c['scores']))
        assert np.abs(np.exp(batch['logp'][b, :nf, :ns].astype(np.float64)).sum(axis=1) - 1).max() < 64 * EPS
        for name, n, terms in (('dq', nf, c['terms'][b][0]), ('dk', ns, c['terms'][b][1])):
            hi, lo = c[name + '_hi'][b, :n], c[name + '_lo'][b, :n]
            _close(tag + name, batch[name][b, :n], hi, _sum_tolerance(hi, lo, terms))
        if c['status'][b] != 0:
            continue
        big = float(np.abs(c['alpha_hi'][live][np.isfinite(c['alpha_hi'][live])]).max())
        _close(tag + 'alpha', batch['alpha'][live], c['alpha_hi'][live], _tolerance(c['alpha_hi'][live], c['alpha_lo'][live], big))
        _close(tag + 'loss', batch['loss'][b], c['loss_hi'][b], _tolerance(c['loss_hi'][b], c['loss_lo'][b], big))
        tol = _tolerance(c['gamma_hi'][live], c['gamma_lo'][live], big)
        _close(tag + 'dlogp', batch['dlogp'][live], c['dlogp_hi'][live], 2.0 * tol)      # |w| <= 2
        assert not batch['dlogp'][live][c['gamma_hi'][live] == 0].any()                  # cells no path visits: exactly 0
        gamma = -batch['dlogp'][b, :nf, :ns].astype(np.float64) / float(c['w'][b])
        rows = np.abs(gamma.sum(axis=1) - 1).max()
        print(f'{tag}sum_l gamma - 1: {rows:.3e} (tolerance {tol:.3e})')
        assert rows <= tol                                                               # the same tolerance as gamma itself
        # MAS on float values: a monotone path from (0, 0) to the end whose own sum is the reported score
        p = batch['path'][b, :nf]
        assert batch['path_len'][b] == nf and p[:, 0].tolist() == list(range(nf)) and p[0, 1] == 0 and p[-1, 1] == ns - 1
        assert set(np.diff(p[:, 1]).tolist()) <= {0, 1}
        along = np.float32(0)
        for t in range(nf):
            along = np.float32(c['logp'][b, t, p[t, 1]] + along) if t else c['logp'][b, 0, 0]
        assert along == batch['score'][b], (tag, along, batch['score'][b])
        _close(tag + 'score', batch['score'][b], score[b], _tolerance(score[b], score32[b], abs(score[b])))


# ---- MAS: bit-equal on exact lattices -----------------------------------------------------------------------------------------------------

def _exact_lattice(shapes, seed):
    ''' multiples of 1/8 in [-8, 0]: every fp32 sum of up to 4096 of them is exact; drawn from few values, so ties abound '''
    rng = np.random.RandomState(seed)
    B, T, L = len(shapes), max(1, max(s[0] for s in shapes)), max(1, max(s[1] for s in shapes))
    logp = -(rng.randint(0, 5, size=(B, T, L)) * rng.choice([0.125, 1.0, 2.0], size=(B, T, 1))).astype(np.float32)
    return logp, np.array([s[0] for s in shapes], dtype=np.int64), np.array([s[1] for s in shapes], dtype=np.int64)


def _mas_dev(logp, n_frm, n_sym, pad=(0, 0)):
    ''' `dx_aln_mas` alone on a lattice with the tight extents plus `pad`: dead inputs NaN, outputs poisoned, every direction bit
        of the workspace set '''
    from daft_exprt import _hip as H
    B, T, L = len(n_frm), logp.shape[1] + pad[0], logp.shape[2] + pad[1]
    x, nf, ns = _dev(_embed(logp, (B, T, L), (n_frm, n_sym))), _dev(n_frm), _dev(n_sym)
    junk = lambda *shape: torch.full(shape, -77, dtype=torch.int32, device=DEV)
    o = dict(score=torch.full((B,), float('nan'), device=DEV), path=junk(B, T + L - 1, 2), path_len=junk(B), mas_status=junk(B))
    words = T * ((L + 63) // 64)
    ws = torch.full((B, words), -1, dtype=torch.int64, device=DEV)
    H.check(H.lib().dx_aln_mas(H.ptr(x), H.ptr(nf), H.ptr(ns), H.ptr(o['score']), H.ptr(o['path']), H.ptr(o['path_len']),
                               H.ptr(o['mas_status']), H.ptr(ws), 8 * words, B, T, L, H.stream()))
    return {name: t.cpu().numpy() for name, t in o.items()}


@pytest.mark.parametrize('shapes', [SHAPES + DEAD, ((1000, 150),)], ids=['ragged', '1000x150'])
def test_mas_is_bit_equal_to_the_oracle_on_exact_lattices(shapes):
    logp, n_frm, n_sym = _exact_lattice(shapes, 11)
    assert logp.min() >= -8 and np.array_equal(logp * 8, np.round(logp * 8))
    path, path_len, score, status = O.mas(logp, n_frm, n_sym)
    ties = sum(int((np.diff(logp[b, :nf, :ns], axis=1) == 0).sum()) for b, (nf, ns) in enumerate(shapes))
    assert ties > 10
    for pad in ((0, 0), (5, 70)):
        got = _mas_dev(logp, n_frm, n_sym, pad)
        assert got['mas_status'].tolist() == status.tolist() and got['path_len'].tolist() == path_len.tolist()
        assert got['score'].tobytes() == score.astype(np.float32).tobytes()
        for b, (nf, ns) in enumerate(shapes):
            assert np.array_equal(got['path'][b, :nf], path[b, :nf]), (nf, ns, pad)
            assert (got['path'][b, nf if status[b] == 0 else 0:] == -1).all()


def test_float_kernels_on_the_longest_accumulation():
    ''' T = 1000, L = 150, B = 2 (one utterance full, one ragged): where the log-space sums are longest '''
    c = _case(32, shapes=((1000, 150), (731, 97)), seed=3)
    out = _run(c)
    for b, (nf, ns) in enumerate(((1000, 150), (731, 97))):
        live = (slice(b, b + 1), slice(0, nf), slice(0, ns))
        big = float(np.abs(c['alpha_hi'][live][np.isfinite(c['alpha_hi'][live])]).max())
        tag = f'{nf}x{ns} '
        _close(tag + 'logp', out['logp'][live], c['logp_hi'][live], _tolerance(c['logp_hi'][live], c['logp_lo'][live], c['scores']))
        _close(tag + 'alpha', out['alpha'][live], c['alpha_hi'][live], _tolerance(c['alpha_hi'][live], c['alpha_lo'][live], big))
        _close(tag + 'loss', out['loss'][b], c['loss_hi'][b], _tolerance(c['loss_hi'][b], c['loss_lo'][b], big))
        tol = _tolerance(c['gamma_hi'][live], c['gamma_lo'][live], big)
        _close(tag + 'dlogp', out['dlogp'][live], c['dlogp_hi'][live], 2.0 * tol)
        gamma = -out['dlogp'][b, :nf, :ns].astype(np.float64) / float(c['w'][b])
        rows = np.abs(gamma.sum(axis=1) - 1).max()
        print(f'{tag}sum_l gamma - 1: {rows:.3e} (tolerance {tol:.3e})')
        assert rows <= tol
        for name, n, terms in (('dq', nf, c['terms'][b][0]), ('dk', ns, c['terms'][b][1])):
            hi, lo = c[name + '_hi'][b, :n], c[name + '_lo'][b, :n]
            _close(tag + name, out[name][b, :n], hi, _sum_tolerance(hi, lo, terms))


# ---- the wrappers: autograd, the loss, hard durations ---------------------------------------------------------------------------------

def _chain(c, dtype):
    ''' soft alignment -> forward-sum loss (mean per frame over the rows with a path) -> its gradients, restated in `dtype` '''
    n_frm, n_sym, ok = c['n_frm'], c['n_sym'], c['status'] == 0
    logp = O.logprob_fwd(c['q'], c['k'], n_frm, n_sym, TAU, SIGMA, dtype)
    alpha, per, _ = O.forward_sum(logp, n_frm, n_sym, dtype)
    w = np.where(ok, 1.0 / (np.maximum(n_frm, 1) * ok.sum()), 0.0).astype(dtype)
    dlogp = O.forward_sum_bwd(logp, alpha, w, n_frm, n_sym, dtype)
    dq, dk = O.logprob_bwd(c['q'], c['k'], logp, dlogp, n_frm, n_sym, TAU, dtype)
    return dtype((per[ok] / n_frm[ok].astype(dtype)).mean()), dq, dk, logp, dlogp


def test_autograd_functions_and_the_loss():
    ''' the two autograd functions and the mean, end to end, against the same chain restated in float64, with the file's one
        rule: max(2 x the deviation of the chain restated in float32, a floor) -- `_tolerance` on the loss with its own magnitude
        as the scale, `_sum_tolerance` on the gradients with the summed |terms| of the chain's own ds. '''
    from daft_exprt.aligner import forward_sum_loss, soft_alignment
    c = _case(32)
    q, k = _dev(c['q']).requires_grad_(), _dev(c['k']).requires_grad_()
    n_frm, n_sym = _dev(c['n_frm']), _dev(c['n_sym'])
    loss, skipped = forward_sum_loss(soft_alignment(q, k, n_frm, n_sym, TAU, SIGMA), n_frm, n_sym)
    loss.backward()
    hi, lo = _chain(c, np.float64), _chain(c, np.float32)
    assert int(skipped) == 3
    _close('loss', float(loss.detach()), hi[0], _tolerance(hi[0], lo[0], abs(hi[0])))
    inner = dict(c, logp=hi[3], g=hi[4])
    terms = [_gradient_terms(inner, b, nf, ns) for b, (nf, ns) in enumerate(SHAPES + DEAD) if c['status'][b] == 0]
    for i, (name, got) in enumerate((('dq', q.grad), ('dk', k.grad))):
        got = got.cpu().numpy()
        assert np.isfinite(got).all()
        _close(name, got, hi[1 + i], _sum_tolerance(hi[1 + i], lo[1 + i], max(t[i] for t in terms)))


def test_hard_durations_of_a_constructed_lattice():
    from daft_exprt.aligner import hard_durations
    rng = np.random.RandomState(4)
    truth = [rng.randint(1, 6, size=n) for n in (1, 4, 9, 70)]
    B, T, L = len(truth), max(int(d.sum()) for d in truth), max(len(d) for d in truth)
    logp = np.full((B, T, L), -4.0, dtype=np.float32)                       # the unique best path: -1 on the true cells
    for b, d in enumerate(truth):
        logp[b, np.arange(d.sum()), np.repeat(np.arange(len(d)), d)] = -1.0
    n_frm, n_sym = np.array([d.sum() for d in truth], dtype=np.int64), np.array([len(d) for d in truth], dtype=np.int64)
    durations, moved, status, score, mas_status = (t.cpu().numpy() for t in hard_durations(_dev(logp), _dev(n_frm), _dev(n_sym), 1))
    for b, d in enumerate(truth):
        assert durations[b, :len(d)].tolist() == d.tolist() and not durations[b, len(d):].any()
        assert moved[b] == 0 and status[b] == 0 and mas_status[b] == 0 and score[b] == -float(d.sum())
    # min_frames = 3: the repair of K27, as tests/align_oracle.py states it, over the path the MAS oracle gives
    path, path_len, _, _ = O.mas(logp, n_frm, n_sym)
    durations, moved, status, _, _ = (t.cpu().numpy() for t in hard_durations(_dev(logp), _dev(n_frm), _dev(n_sym), 3))
    seen = set()
    for b, d in enumerate(truth):
        want = AO.dtw_transfer(path[b, :path_len[b]].tolist(), int(n_frm[b]), len(d), [1] * len(d), 3)
        print(f'{d.tolist()} -> {durations[b, :len(d)].tolist()} moved {moved[b]} status {status[b]}; oracle {want}')
        assert (durations[b, :len(d)].tolist(), int(moved[b]), int(status[b])) == tuple(want)
        seen.add(int(status[b]))
        if status[b] == 0:
            assert durations[b].sum() == n_frm[b] and (durations[b, :len(d)] >= 3).all()
    assert 0 in seen and moved.max() > 0


# ---- learnability ------------------------------------------------------------------------------------------------------------------------

RESTATEMENT = (0.8720, 0.9393, 0.9089, 0.9486, 0.9430, 0.9351)      # tests/aligner_oracle.py toy_restatement(seed), seeds 0 .. 5
FLOOR = min(RESTATEMENT) - 0.03


def test_the_aligner_learns_the_toy_corpus():
    ''' 64 utterances over 15 symbols with fixed random 80-dimensional templates, 4 to 12 symbols each without immediate repeats,
        2 to 7 frames per symbol, frames = template + 0.5 x Gaussian noise; Aligner(hidden 64, A 32), temperature 0.05, prior sigma
        0.2, 150 Adam steps at 4e-3 with 32 utterances each; MAS with the prior off.  The share of frames given their true symbol
        must reach min(restatement) - 0.03 = 0.842, the restatement being `aligner_oracle.toy_restatement` -- plain torch, float64,
        CPU, the same architecture, data and schedule -- which gave 0.8720, 0.9393, 0.9089, 0.9486, 0.9430, 0.9351 for the seeds
        0 .. 5 (an untrained model gives 0.12 - 0.18). '''
    from daft_exprt.aligner import Aligner, forward_sum_loss, mas_path
    cfg = O.TOY
    utts = O.toy_corpus()
    seed = 0
    torch.manual_seed(seed)
    model = Aligner(cfg['symbols'] + 1, cfg['n_mel'], cfg['hidden'], cfg['att_dim'], cfg['temperature'], cfg['prior_sigma']).to(DEV)
    opt = torch.optim.Adam(model.parameters(), lr=cfg['lr'])

    def batch(idx):
        sym, nl, mel, nt = O.toy_collate([utts[i] for i in idx], torch.float32)
        return sym.to(DEV), nl.to(DEV), mel.transpose(1, 2).contiguous().to(DEV), nt.to(DEV)

    def share():
        with torch.no_grad():
            sym, nl, mel, nt = batch(range(len(utts)))
            path, path_len, _, status = mas_path(model(sym, nl, mel, nt, prior_sigma=0.), nt, nl)
        assert not status.any()
        path, path_len = path.cpu().numpy(), path_len.cpu().numpy()
        return O.frames_correct(utts, [path[b, :path_len[b], 1] for b in range(len(utts))])

    before = share()
    for idx in O.toy_batches(seed):
        sym, nl, mel, nt = batch(idx)
        loss, skipped = forward_sum_loss(model(sym, nl, mel, nt), nt, nl)
        opt.zero_grad()
        loss.backward()
        opt.step()
    after = share()
    print(f'frames given their true symbol: untrained {before:.4f}, trained {after:.4f} (loss {float(loss.detach()):.5f}); floor {FLOOR:.4f}')
    assert int(skipped) == 0 and before < 0.5
    assert after >= FLOOR


# ---- a data set, end to end ---------------------------------------------------------------------------------------------------------------

FS = 22050
UTTERANCES = (('u0', 1.2, 0.15, '{HH AH0 L OW1} , {W ER1 L D} . ~', 'Hello, world.'),
              ('u1', 0.9, 0.00, '{G UH1 D} {D EY1} ~', 'Good day'),
              ('u2', 1.0, 0.25, '{Y EH1 S} ? {N OW1} ! ~', 'Yes? No!'))


def _wave(seconds, lead, seed):
    ''' silence, a noise burst, a short gap, a second burst, silence (as tests/test_gpu_align.py fabricates its recordings) '''
    rng = np.random.RandomState(seed)
    n, first = int(seconds * FS), int(lead * FS)
    wav = 1e-4 * rng.standard_normal(n)
    last = n - int(0.1 * FS)
    gap = (first + last) // 2
    wav[first: gap - 600] += 0.2 * rng.standard_normal(gap - 600 - first)
    wav[gap + 600: last] += 0.3 * rng.standard_normal(last - gap - 600)
    return wav.astype(np.float32)


def test_align_batch_keys_dtypes_and_invariants(tmp_path):
    ''' an untrained Aligner: the dict of `align.align_batch`, the invariants of its rows, the early statuses, determinism '''
    from daft_exprt.align import ALIGN_KEYS
    from daft_exprt.aligner import Aligner
    from daft_exprt.evaluate import max_dtw_length
    from daft_exprt.generate import _symbol_ids, read_phonemised_sentences
    hp = make_hparams(minimum_wav_duration=200)
    phonemised = tmp_path / 'phonemised.txt'
    phonemised.write_text(''.join(f'{name}|{text}\n' for name, _, _, text, _ in UTTERANCES), encoding='utf-8')
    ids = [_symbol_ids(s, hp) for s in read_phonemised_sentences(str(phonemised))[0]]
    waves = [_wave(seconds, lead, 40 + i) for i, (_, seconds, lead, _, _) in enumerate(UTTERANCES)]
    symbols = torch.zeros((3, max(len(i) for i in ids)), dtype=torch.int64)
    wavs = torch.zeros((3, max(len(w) for w in waves)), dtype=torch.float32)
    for b in range(3):
        symbols[b, :len(ids[b])], wavs[b, :len(waves[b])] = torch.tensor(ids[b]), torch.from_numpy(waves[b])
    lengths = torch.tensor([len(i) for i in ids], dtype=torch.int64, device=DEV)
    torch.manual_seed(2)
    aligner = Aligner(len(hp.symbols), hp.n_mel_channels, hidden=32, att_dim=16).to(DEV)
    run = lambda: aligner.align_batch(symbols.to(DEV), lengths, wavs.to(DEV), [len(w) for w in waves], None, hp)
    out = run()
    assert tuple(out) == ALIGN_KEYS
    assert [out[key].dtype for key in ALIGN_KEYS] == [torch.int64, torch.int64, torch.int64, torch.int32, torch.int32, torch.float32,
                                                     torch.int64, torch.int64]
    again = run()
    for key in ALIGN_KEYS:
        assert out[key].cpu().numpy().tobytes() == again[key].cpu().numpy().tobytes(), key
    out = {key: value.cpu().numpy() for key, value in out.items()}
    for b, (name, seconds, lead, _, _) in enumerate(UTTERANCES):
        n, rec = len(ids[b]), out['rec_durations'][b]
        assert out['status'][b] == 0 and out['frames_gen'][b] == n and out['gen_durations'][b].tolist() == [1] * n + [0] * (symbols.shape[1] - n)
        assert rec.sum() == out['frames'][b] and (rec[:n] >= 3).all() and not rec[n:].any() and 0 <= out['moved'][b] <= n
        assert np.isfinite(out['path_cost'][b]) and out['path_cost'][b] > 0
        assert (out['begin'][b] + out['frames'][b] - 1) * hp.hop_length <= len(waves[b]) and (out['begin'][b] > 0) == (lead > 0)
    too_long = (max_dtw_length() + 1) * hp.hop_length
    early = aligner.align_batch(symbols[:2].to(DEV), lengths[:2], torch.zeros((2, 8), device=DEV), [too_long, hp.filter_length // 2], None, hp)
    assert early['status'].tolist() == [3, 4] and not early['rec_durations'].any() and torch.isnan(early['path_cost']).all()


def test_train_align_extract_round_trip(tmp_path):
    from daft_exprt.align import align_data_set, flatten_sentence
    from daft_exprt.aligner import Aligner, load_aligner
    from daft_exprt.audio import write_wav_int16
    from daft_exprt.extract_features import extract_features
    from daft_exprt.generate import read_phonemised_sentences
    hp = make_hparams(speakers=['newspk'], minimum_wav_duration=200)
    phonemised = tmp_path / 'phonemised.txt'
    phonemised.write_text(''.join(f'{name}|{text}\n' for name, _, _, text, _ in UTTERANCES), encoding='utf-8')
    sentences = read_phonemised_sentences(str(phonemised))[0]
    data, features = tmp_path / 'data', tmp_path / 'features'
    for d in (data / 'newspk' / 'wavs', data / 'newspk' / 'align', features / 'newspk'):
        d.mkdir(parents=True)
    for i, (name, seconds, lead, _, lab) in enumerate(UTTERANCES):
        wav = _wave(seconds, lead, 40 + i)
        write_wav_int16(str(data / 'newspk' / 'wavs' / f'{name}.wav'), FS, np.clip(np.trunc(wav * 32768.), -32768, 32767).astype(np.int16))
        (data / 'newspk' / 'align' / f'{name}.lab').write_text(lab + '\n', encoding='utf-8')
    (features / 'newspk' / 'metadata.csv').write_text(''.join(f'{u[0]}|{u[4]}\n' for u in UTTERANCES), encoding='utf-8')

    # through the command line: HyperParams for the speakers, train_aligner, save_aligner, align_data_set
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('train_aligner_cli', os.path.join(root, 'scripts', 'train_aligner.py'))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    cli.main(['-dd', str(data), '-spks', 'newspk', '-tf', str(phonemised), '-o', str(tmp_path / 'aligner.pt'), '-st', '4', '-bs', '2',
              '--seed', '1'])
    aligner = load_aligner(str(tmp_path / 'aligner.pt'))
    assert isinstance(aligner, Aligner) and all(torch.isfinite(p).all() for p in aligner.parameters())
    assert all(p.is_cuda for p in aligner.parameters()) and aligner.args['n_mel'] == hp.n_mel_channels
    with open(data / 'align_report.json', 'r', encoding='utf-8') as f:
        written = json.load(f)
    assert written['skipped'] == [] and written['batches'] == 2 and written['already_done'] == 0, written['skipped']
    # the saved aligner gives the same report again
    report = align_data_set(str(data), ['newspk'], str(phonemised), aligner, hp, batch_size=2, overwrite=True)
    assert report['files'] == written['files'] and report['summary'] == written['summary']
    assert report['summary']['files'] == report['summary']['written'] == 3 and report['summary']['status']['0'] == 3
    with open(data / 'align_report.json', 'r', encoding='utf-8') as f:
        on_disk = json.load(f)
    assert on_disk['files'] == report['files'] and on_disk['summary'] == report['summary']
    for (name, _, _, _, _), sentence in zip(UTTERANCES, sentences):
        record = report['files'][f'newspk/{name}']
        print(name, record)
        assert record['written'] and record['status'] == 0 and record['frames'] > 0 and record['path_cost'] > 0
        assert record['frames_gen'] == record['symbols'] == len(flatten_sentence(sentence))

    done = extract_features(str(data), str(features), hp, 1, batch_size=3)
    assert done['written'] == 3 and done['skipped'] == [], done
    for (name, _, _, _, _), sentence in zip(UTTERANCES, sentences):
        for ext in ('.npy', '.markers', '.frames_nrg', '.symbols_nrg', '.frames_f0', '.symbols_f0'):
            assert (features / 'newspk' / f'{name}{ext}').is_file(), (name, ext)
        rows = [line.rstrip('\n').split('\t') for line in (features / 'newspk' / f'{name}.markers').read_text(encoding='utf-8').splitlines()]
        assert [row[3] for row in rows] == [symbol for symbol, _ in flatten_sentence(sentence)], name
        mel = np.load(features / 'newspk' / f'{name}.npy')
        assert sum(int(row[2]) for row in rows) == mel.shape[1]
