"""`dx_clone_pool`, `dx_prosody_impose`, `dx_prosody_impose_durations` (csrc/prosody_targets.hip) against
tests/prosody_targets_oracle.py, `DaftExprt.inference(..., prosody_targets=...)` against the CPU oracle's own stages on the forced
values, and daft_exprt/clone.py / scripts/clone.py end to end on a random-init model and fabricated recordings.

Bounds, all from the number formats:
  pooled means, statistics, targets at weight 0 and 1, every integer      bit-equal to the oracle
  standardised values   4 * 2^-24 * (|v| + |mean|) / std of float64: the two fp32 roundings of the subtraction and the division
                        (measured: the largest error seen is 0.12 of the bound)
  blended values        2^-23 * (|x| + |t|) of float64: the fp32 roundings of t - x and of the fused multiply-add
                        (measured: 0.27 of the bound)
  forced mel            2e-4 of the tensor's largest magnitude, the bound tests/test_gpu_model.py holds the fp32 inference golden to
                        (measured: 1.4e-6)"""
import functools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import prosody_targets_oracle as P
from tests.util import make_hparams

DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOP, FS = 256, 22050
MEL_TOL = 2e-4                      # tests/test_gpu_model.py TOL['fp32']
ERR_ARG = -1


# ---- dx_clone_pool -------------------------------------------------------------------------------------------------------------------

def _curves(T, seed, constant_energy=False):
    rng = np.random.RandomState(seed)
    energy = np.full(T, 2.5, dtype=np.float32) if constant_energy else rng.uniform(0.1, 5.0, size=T).astype(np.float32)
    pitch = np.where(rng.uniform(size=T) < 0.7, rng.uniform(4.4, 5.6, size=T), 0.).astype(np.float32)
    return energy, pitch


@functools.lru_cache(maxsize=None)
def _pool_cases():
    ''' name -> (energy, pitch, begin, durations, n_rows) '''
    cases = {}
    e, p = _curves(64, 0)
    p[10:15] = 0.                                                       # the symbol that owns frames 10..14 is all unvoiced
    cases['begin 0, a row of 0 frames, an unvoiced symbol'] = (e, p, 0, [4, 6, 5, 0, 9, 1, 2, 11], 8)
    e, p = _curves(80, 1)
    cases['begin > 0, n_rows < L'] = (e, p, 13, [3, 1, 7, 2, 20, 4, 99, 99, 99], 6)
    e, p = _curves(57, 2)
    cases['durations end exactly at T'] = (e, p, 9, [8, 8, 0, 16, 1, 15], 6)             # 9 + 48 == 57
    e, p = _curves(40, 3)
    p[:] = 0.
    p[6:9] = [5.0, 5.1, 5.2]
    cases['a single voiced symbol'] = (e, p, 2, [3, 4, 5, 6], 4)                         # frames 6..8 lie in the second row only
    e, p = _curves(40, 4, constant_energy=True)
    cases['constant energy'] = (e, p, 0, [5, 5, 5, 5, 5], 5)
    e, p = _curves(30, 5)
    cases['overrun'] = (e, p, 20, [5, 200, 5], 3)
    e, p = _curves(57, 2)
    cases['overrun by one frame'] = (e, p, 10, [8, 8, 0, 16, 1, 15], 6)                   # 10 + 48 == 57 + 1
    return cases


def _pool_dev(names, given, pad_t=0, pad_l=0):
    ''' one launch over the named cases, the outputs poisoned first; given: None or {name: ((mean_e, std_e), (mean_p, std_p))} '''
    from daft_exprt import _hip as H
    cases = [_pool_cases()[n] for n in names]
    B = len(cases)
    T = max(len(c[0]) for c in cases)
    ldt, L = T + pad_t, max(len(c[3]) for c in cases) + pad_l
    energy, pitch = np.full((B, ldt), 3e7, dtype=np.float32), np.full((B, ldt), 3e7, dtype=np.float32)
    dur = np.full((B, L), 1 << 40, dtype=np.int64)
    for b, (e, p, _, d, _) in enumerate(cases):
        energy[b, :len(e)], pitch[b, :len(p)], dur[b, :len(d)] = e, p, d
        energy[b, len(e):T], pitch[b, len(p):T] = 0., 0.                                 # frames of the extent the row does not have
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    energy, pitch, dur = to(energy), to(pitch), to(dur)
    begin = to(np.array([c[2] for c in cases], dtype=np.int64))
    n_rows = to(np.array([c[4] for c in cases], dtype=np.int64))
    stats = [None] * 4
    if given is not None:
        stats = [to(np.array([given[n][q][k] for n in names], dtype=np.float32)) for q in (0, 1) for k in (0, 1)]
    outs = [torch.full((B, L), float('nan'), dtype=torch.float32, device=DEV) for _ in range(4)]
    self_stats = torch.full((B, 4), float('nan'), dtype=torch.float32, device=DEV)
    dropped = torch.full((B,), -77, dtype=torch.int32, device=DEV)
    status = torch.full((B,), -77, dtype=torch.int32, device=DEV)
    H.check(H.lib().dx_clone_pool(H.ptr(energy), H.ptr(pitch), ldt, H.ptr(begin), H.ptr(dur), H.ptr(n_rows), *[H.ptr(t) for t in stats],
                                  *[H.ptr(t) for t in outs], H.ptr(self_stats), H.ptr(dropped), H.ptr(status), B, T, L, H.stream()))
    keys = ('sym_energy', 'sym_pitch', 'raw_energy', 'raw_pitch')
    got = {k: t.cpu().numpy() for k, t in zip(keys, outs)}
    got.update(self_stats=self_stats.cpu().numpy(), dropped=dropped.cpu().numpy(), status=status.cpu().numpy(), T=T, L=L)
    return got


GIVEN = ((2.3456789, 1.2345678), (5.0123456, 0.3456789))


def _check_pool_row(got, b, name, own):
    ''' row b of a launch against the oracle run with the launch's own T and L; returns the largest error / bound of its
        standardised values '''
    e, p, begin, durations, n_rows = _pool_cases()[name]
    want = P.clone_pool(e, p, begin, durations + [1 << 40] * (got['L'] - len(durations)), n_rows, got['T'], got['L'],
                        None if own else GIVEN[0], None if own else GIVEN[1])
    assert got['status'][b] == want['status'] and got['dropped'][b] == want['dropped'], name
    assert got['status'][b] == (1 if name.startswith('overrun') else 0), name
    # the pooled means and the utterance's own statistics: the oracle's bits
    for key in ('raw_energy', 'raw_pitch', 'self_stats'):
        assert got[key][b].tobytes() == want[key].tobytes(), (name, key, got[key][b], want[key])
    assert not got['raw_energy'][b, n_rows:].any() and not got['raw_pitch'][b, n_rows:].any(), name
    if want['status'] != 0:                                                              # nothing read, everything written as 0
        assert not got['sym_energy'][b].any() and not got['sym_pitch'][b].any() and not got['self_stats'][b].any(), name
        return 0.
    worst = 0.
    for q, key in enumerate(('sym_energy', 'sym_pitch')):
        raw, mean, std = want[f'raw_{"energy" if q == 0 else "pitch"}'], want['used'][2 * q], want['used'][2 * q + 1]
        v = got[key][b]
        assert np.isfinite(v).all() and not v[raw == 0].any() and not v[n_rows:].any(), (name, key)              # zeros are exactly 0
        if want['dropped'] >> q & 1:
            assert not v.any(), (name, key)
            continue
        err = np.abs(v.astype(np.float64) - want[key])
        bound = P.standardise_bound(raw, mean, std)
        assert (err <= bound).all(), (name, key, err.max())
        worst = max(worst, float((err[raw != 0] / bound[raw != 0]).max()) if (raw != 0).any() else 0.)
    return worst


@pytest.mark.parametrize('own', [False, True], ids=['given statistics', 'self statistics'])
def test_clone_pool_equals_the_oracle(own):
    names = [n for n in _pool_cases() if n != 'overrun by one frame']
    given = None if own else {n: GIVEN for n in names}
    worst = 0.
    for batch in (names[:3], names[3:]):
        got = _pool_dev(batch, given)
        wide = _pool_dev(batch[::-1], given, pad_t=37, pad_l=5)                          # another batch, larger ldt and L
        for b, name in enumerate(batch):
            worst = max(worst, _check_pool_row(got, b, name, own))
            # the same utterance in another batch, at another row, with larger ldt and L: the same bits
            w = len(batch) - 1 - b
            for key in ('sym_energy', 'sym_pitch', 'raw_energy', 'raw_pitch'):
                assert wide[key][w, :got['L']].tobytes() == got[key][b].tobytes() and not wide[key][w, got['L']:].any(), (name, key)
            assert wide['self_stats'][w].tobytes() == got['self_stats'][b].tobytes(), name
            assert (wide['dropped'][w], wide['status'][w]) == (got['dropped'][b], got['status'][b]), name
    print(f'standardised values: largest error / bound = {worst:.3f} (bound 4 * 2^-24 * (|v| + |mean|) / std)')
    if own:
        dropped = {n: int(_pool_dev([n], None)['dropped'][0]) for n in ('a single voiced symbol', 'constant energy')}
        assert dropped == {'a single voiced symbol': 2, 'constant energy': 1}


@pytest.mark.parametrize('own', [False, True], ids=['given statistics', 'self statistics'])
def test_clone_pool_at_the_end_of_the_curves(own):
    ''' the launch's T is the row's own frame count: begin + the durations == T is the last row the kernel may pool (its last frame
        is frame T - 1, with poison behind it in a wider row), begin + the durations == T + 1 is the first it may not '''
    at_end, beyond = 'durations end exactly at T', 'overrun by one frame'
    e, _, begin, durations, n_rows = _pool_cases()[at_end]
    assert begin + sum(durations[:n_rows]) == len(e) == len(_pool_cases()[beyond][0])
    assert _pool_cases()[beyond][2] + sum(durations[:n_rows]) == len(e) + 1
    given = None if own else {n: GIVEN for n in (at_end, beyond)}
    alone = _pool_dev([at_end], given)
    assert alone['T'] == len(e)
    _check_pool_row(alone, 0, at_end, own)
    wide = _pool_dev([at_end], given, pad_t=37, pad_l=5)                                 # ldt > T: 3e7 in the 37 frames behind T
    pair = _pool_dev([beyond, at_end], given, pad_t=3)
    assert wide['T'] == pair['T'] == len(e)
    _check_pool_row(wide, 0, at_end, own)
    _check_pool_row(pair, 0, beyond, own)
    _check_pool_row(pair, 1, at_end, own)
    assert pair['status'].tolist() == [1, 0]
    for key in ('sym_energy', 'sym_pitch', 'raw_energy', 'raw_pitch', 'self_stats'):
        assert wide[key][0, :alone[key].shape[1]].tobytes() == pair[key][1].tobytes() == alone[key][0].tobytes(), key
    # the last row's mean holds the curve's last frame: a kernel that stopped one frame early would not reproduce it
    last = n_rows - 1
    assert alone['raw_energy'][0, last] == np.float32(math.fsum(float(v) for v in e[len(e) - durations[last]:]) / durations[last])


def test_clone_pool_wrapper_and_argument_errors():
    from daft_exprt import _hip as H
    from daft_exprt import ops
    name = 'begin > 0, n_rows < L'
    e, p, begin, durations, n_rows = _pool_cases()[name]
    dev = lambda a, dtype: torch.tensor(np.asarray(a)[None], dtype=dtype, device=DEV)
    out = ops.clone_pool(dev(e, torch.float32), dev(p, torch.float32), torch.tensor([begin], device=DEV), dev(durations, torch.int64),
                         torch.tensor([n_rows], device=DEV), raw=True)
    want = P.clone_pool(e, p, begin, durations, n_rows, len(e), len(durations))
    assert out[5][0].cpu().numpy().tobytes() == want['raw_energy'].tobytes() and out[6][0].cpu().numpy().tobytes() == want['raw_pitch'].tobytes()
    assert out[2][0].cpu().numpy().tobytes() == want['self_stats'].tobytes() and int(out[3][0]) == 0 and int(out[4][0]) == 0
    lib = H.lib()
    t = torch.zeros((16,), dtype=torch.int64, device=DEV)
    q = H.ptr(t)
    assert lib.dx_clone_pool(None, q, 4, q, q, q, None, None, None, None, q, q, None, None, q, q, q, 1, 4, 2, None) == ERR_ARG
    assert b'null' in lib.dx_last_error()
    assert lib.dx_clone_pool(q, q, 4, q, q, q, q, None, None, None, q, q, None, None, q, q, q, 1, 4, 2, None) == ERR_ARG
    assert b'std' in lib.dx_last_error()
    assert lib.dx_clone_pool(q, q, 4, q, q, q, None, None, None, None, q, q, None, None, q, q, q, 1, 4, 0, None) == -2


# ---- dx_prosody_impose / dx_prosody_impose_durations ---------------------------------------------------------------------------------

class _T(object):
    ''' the attributes `ops.prosody_impose` reads '''
    def __init__(self, **kw):
        for key in ('durations', 'energy', 'pitch', 'w_dur', 'w_energy', 'w_pitch'):
            setattr(self, key, kw.get(key))


def _dev(a, dtype):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV).contiguous()


def _impose_dev(x, lengths, t_dur=None, t_energy=None, t_pitch=None, w_dur=None, w_energy=None, w_pitch=None, dur_factors=None, validate=False):
    ''' x: (dur, energy, pitch) NumPy (B, L) -> ((dur, energy, pitch) NumPy, exact NumPy, the device tensors for a second step) '''
    from daft_exprt import ops
    hp = make_hparams()
    f = lambda a: None if a is None else _dev(a, torch.float32)
    dev_x = [_dev(a, torch.float32) for a in x]
    targets = _T(durations=None if t_dur is None else _dev(t_dur, torch.int64), energy=f(t_energy), pitch=f(t_pitch), w_dur=f(w_dur),
                 w_energy=f(w_energy), w_pitch=f(w_pitch))
    n = _dev(lengths, torch.int64)
    exact = ops.prosody_impose(dev_x[0], dev_x[1], dev_x[2], targets, n, f(dur_factors), hp, validate=validate)
    return [t.cpu().numpy() for t in dev_x], exact.cpu().numpy(), (dev_x, targets, n, exact, f(dur_factors), hp)


def _inputs(B=3, L=12, seed=0):
    rng = np.random.RandomState(seed)
    x = [rng.uniform(0.02, 0.12, size=(B, L)).astype(np.float32), rng.standard_normal((B, L)).astype(np.float32),
         rng.standard_normal((B, L)).astype(np.float32)]
    t_dur = rng.randint(0, 9, size=(B, L)).astype(np.int64)
    t_energy, t_pitch = rng.standard_normal((B, L)).astype(np.float32), rng.standard_normal((B, L)).astype(np.float32)
    return x, t_dur, t_energy, t_pitch


def test_impose_weights_zero_one_and_between():
    x, t_dur, t_energy, t_pitch = _inputs()
    lengths = [12, 9, 12]
    w = np.repeat(np.array([[0.], [1.], [0.3]], dtype=np.float32), 12, axis=1)
    got, exact, _ = _impose_dev(x, lengths, t_dur, t_energy, t_pitch, w, w, w)
    assert exact.tolist() == [0, 1, 0]
    seconds = np.array([[P.target_seconds(f, HOP, FS) for f in row] for row in t_dur], dtype=np.float32)
    worst = 0.
    for q, t in enumerate((seconds, t_energy, t_pitch)):
        assert got[q][0].tobytes() == x[q][0].tobytes()                                  # w = 0: the input, bit for bit
        assert got[q][1, :9].tobytes() == t[1, :9].tobytes()                             # w = 1: the target, bit for bit
        assert got[q][1, 9:].tobytes() == x[q][1, 9:].tobytes()                          # at and past the length: untouched
        want = np.array([P.blend(a, b, np.float32(0.3)) for a, b in zip(x[q][2], t[2])])
        bound = np.array([P.blend_bound(a, b) for a, b in zip(x[q][2], t[2])])
        err = np.abs(got[q][2].astype(np.float64) - want)
        assert (err <= bound).all(), (q, err.max())
        worst = max(worst, float((err / bound).max()))
    print(f'w = 0.3: largest error / bound = {worst:.3f} (bound 2^-23 * (|x| + |t|))')
    # and the whole launch against the oracle, row by row
    for b in range(3):
        want = P.impose(x[0][b], x[1][b], x[2][b], lengths[b], t_dur[b], t_energy[b], t_pitch[b], w[b], w[b], w[b])
        assert want[3] == exact[b]
        for q, t in enumerate((seconds, t_energy, t_pitch)):
            bound = np.array([P.blend_bound(a, c) for a, c in zip(x[q][b], t[b])])
            assert (np.abs(got[q][b].astype(np.float64) - want[q]) <= bound).all(), (b, q)


def test_impose_zero_targets_are_statements():
    x, _, _, _ = _inputs(seed=1)
    zeros = np.zeros((3, 12), dtype=np.float32)
    w = np.tile(np.array([0.49, 0.5, 1.0, 0.0], dtype=np.float32), (3, 3))
    got, exact, _ = _impose_dev(x, [12, 12, 12], t_energy=zeros, t_pitch=zeros, w_energy=w, w_pitch=w[:, ::-1].copy())
    assert exact.tolist() == [0, 0, 0] and got[0].tobytes() == x[0].tobytes()            # no duration target: dur untouched
    taken = (w >= 0.5)
    for q, mask in ((1, taken), (2, taken[:, ::-1])):
        assert not got[q][mask].any() and got[q][~mask].tobytes() == x[q][~mask].tobytes()
    # a non-zero target beside them still blends
    t = zeros.copy()
    t[:, ::2] = 1.5
    got, _, _ = _impose_dev(x, [12, 12, 12], t_energy=t, w_energy=np.full((3, 12), 0.49, dtype=np.float32))
    assert got[1][:, 1::2].tobytes() == x[1][:, 1::2].tobytes() and (got[1][:, ::2] != x[1][:, ::2]).all()


def test_exact_flags_and_the_duration_override():
    from daft_exprt import ops
    B, L = 5, 12
    x, t_dur, t_energy, _ = _inputs(B, L, seed=2)
    lengths = [12, 10, 12, 12, 12]
    t_dur[0, :12] = [0, 1, 2, 3, 1, 0, 2, 7, 1, 1, 0, 4]                                 # symbols of 0, 1 and 2 frames
    t_dur[1, 4] = -1                                                                     # one missing target
    t_dur[3, :12] = [1, 0, 1, 1, 1, 1, 0, 0, 1, 1, 1, 1]                                 # nothing K16 keeps: alone it raises IndexError
    w_dur = np.ones((B, L), dtype=np.float32)
    w_dur[4, 7] = 0.999
    factors = np.ones((B, L), dtype=np.float32)
    factors[2, 0] = 1.25
    factors[1, 11] = 3.0                                                                 # (behind the length of row 1: not looked at)
    got, exact, (dev_x, targets, n, exact_dev, f_dev, hp) = _impose_dev(x, lengths, t_dur, t_energy, None, w_dur, np.ones((B, L), dtype=np.float32),
                                                                        None, factors)
    assert exact.tolist() == [1, 0, 0, 1, 0]
    for b in range(B):
        assert P.impose(x[0][b], x[1][b], x[2][b], lengths[b], t_dur[b], t_energy[b], None, w_dur[b], np.ones(L), None, factors[b])[3] == exact[b]
    assert _impose_dev(x, lengths, None, t_energy, None, None, np.ones((B, L), dtype=np.float32))[1].tolist() == [0] * B
    # K16 alone, then K16 and the override
    alone = dev_x[0].clone()
    k16 = [t.cpu().numpy() for t in ops.int_durations(alone, hp, f_dev)]
    dint, totals, status = ops.int_durations(dev_x[0], hp, f_dev)
    ops.prosody_impose_durations(exact_dev, targets, n, dev_x[0], dint, totals, status, hp)
    dint, totals, status, dur = (t.cpu().numpy() for t in (dint, totals, status, dev_x[0]))
    assert k16[2][3] == 1                                                                # (the IndexError row, had K16 had the last word)
    for b in range(B):
        want = P.impose_durations(int(exact[b]), t_dur[b], lengths[b], alone[b].cpu().numpy(), k16[0][b], k16[1][b], k16[2][b], HOP, FS)
        assert dint[b].tolist() == want[1].tolist() and int(totals[b]) == want[2] and int(status[b]) == want[3], b
        assert dur[b].tobytes() == want[0].tobytes(), b
        if exact[b] == 1:
            assert dint[b, :lengths[b]].tolist() == t_dur[b, :lengths[b]].tolist() and not dint[b, lengths[b]:].any()
            assert totals[b] == t_dur[b, :lengths[b]].sum() and status[b] == 0
        else:                                                                            # a non-exact neighbour keeps K16's result
            assert dint[b].tobytes() == k16[0][b].tobytes() and totals[b] == k16[1][b] and status[b] == k16[2][b]
    # a frame-exact row whose targets sum to 0 frames has a status of its own
    zero = np.zeros((1, L), dtype=np.int64)
    _, exact, (dev_x, targets, n, exact_dev, _, hp) = _impose_dev([a[:1] for a in x], [12], zero, w_dur=np.ones((1, L), dtype=np.float32))
    dint, totals, status = ops.int_durations(dev_x[0], hp, None)
    ops.prosody_impose_durations(exact_dev, targets, n, dev_x[0], dint, totals, status, hp)
    assert exact.tolist() == [1] and int(status[0]) == P.ST_EMPTY and int(totals[0]) == 0 and not dint.any()


def test_impose_argument_errors():
    from daft_exprt import _hip as H
    from daft_exprt import ops
    lib = H.lib()
    t = torch.zeros((16,), dtype=torch.int64, device=DEV)
    q = H.ptr(t)
    assert lib.dx_prosody_impose(None, q, q, q, None, None, q, None, None, q, None, q, 1, 2, 256, 22050.0, 0, None) == ERR_ARG
    assert b'null' in lib.dx_last_error()
    assert lib.dx_prosody_impose(q, q, q, q, None, None, None, None, None, q, None, q, 1, 2, 256, 22050.0, 0, None) == ERR_ARG
    assert b'weights' in lib.dx_last_error()
    assert lib.dx_prosody_impose(q, q, q, None, None, None, None, None, None, q, None, q, 1, 0, 256, 22050.0, 0, None) == -2
    assert lib.dx_prosody_impose_durations(None, q, q, q, q, q, q, 1, 2, 256, 22050.0, None) == ERR_ARG and b'null' in lib.dx_last_error()
    # a weight outside [0, 1]: DX_ERR_ARG with a message when the call validates ...
    x, t_dur, t_energy, _ = _inputs(seed=3)
    w = np.ones((3, 12), dtype=np.float32)
    bad = w.copy()
    bad[1, 5] = 1.25
    with pytest.raises(RuntimeError) as e:
        _impose_dev(x, [12, 12, 12], t_dur, t_energy, None, w, bad, validate=True)
    assert 'error -1' in str(e.value) and 'row 1' in str(e.value) and 'outside [0, 1]' in str(e.value)
    bad[1, 5] = float('nan')
    with pytest.raises(RuntimeError):
        _impose_dev(x, [12, 12, 12], t_dur, t_energy, None, bad, w, validate=True)
    got, exact, _ = _impose_dev(x, [12, 12, 12], t_dur, t_energy, None, w, w, validate=True)         # (good weights pass the check)
    assert exact.tolist() == [1, 1, 1] and got[1].tobytes() == t_energy.tobytes()
    # ... and without the read-back: the row is left alone, flagged, and ends as status 4 behind K16
    bad[1, 5] = -0.5
    got, exact, (dev_x, targets, n, exact_dev, _, hp) = _impose_dev(x, [12, 12, 12], t_dur, t_energy, None, bad, w)
    assert exact.tolist() == [1, -1, 1] and all(got[k][1].tobytes() == x[k][1].tobytes() for k in range(3))
    assert got[1][0].tobytes() == t_energy[0].tobytes()
    dint, totals, status = ops.int_durations(dev_x[0], hp, None)
    ops.prosody_impose_durations(exact_dev, targets, n, dev_x[0], dint, totals, status, hp)
    assert status.tolist() == [0, P.ST_WEIGHT, 0]


# ---- the model ---------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _model(mode='fp32'):
    ''' the random-init model of tests/test_gpu_align.py: every symbol lasts about 0.06 s '''
    from daft_exprt.model import DaftExprt
    fx = np.load(os.path.join(ROOT, 'tests', 'golden', 'data_loader.npz'))
    hp = make_hparams(compute_dtype=mode, minimum_wav_duration=200)
    hp.stats = {f'spk {i}': {'energy': {'mean': float(fx['stats_energy_mean'][i]), 'std': float(fx['stats_energy_std'][i])},
                             'pitch': {'mean': float(fx['stats_pitch_mean'][i]), 'std': float(fx['stats_pitch_std'][i])}} for i in range(11)}
    torch.manual_seed(1234)
    model = DaftExprt(hp)
    with torch.no_grad():
        model.prosody_predictor.projection.linear_layer.weight[0].mul_(0.01)
        model.prosody_predictor.projection.linear_layer.bias.copy_(torch.tensor([0.06, 0., 0.]))
    return model.cuda(0).eval(), hp


@functools.lru_cache(maxsize=None)
def _batch(pitch_neutral):
    ''' the 10 inputs of `inference` (CPU tensors): B = 3, L = 12, references of 30 to 44 frames '''
    rng = np.random.RandomState(11)
    lengths = [12, 9, 7]
    symbols = np.zeros((3, 12), dtype=np.int64)
    for b, n in enumerate(lengths):
        symbols[b, :n] = rng.randint(1, 60, size=n)
    ref_lengths = [44, 30, 37]
    energy, pitch, mel = np.zeros((3, 44), dtype=np.float32), np.zeros((3, 44), dtype=np.float32), np.zeros((3, 80, 44), dtype=np.float32)
    for b, n in enumerate(ref_lengths):
        energy[b, :n] = rng.uniform(0.5, 6.0, size=n)
        pitch[b, :n] = np.where(rng.uniform(size=n) < 0.7, rng.uniform(4.5, 5.5, size=n), 0.)
        mel[b, :, :n] = rng.standard_normal((80, n)) - 4.
    ones = torch.ones((3, 12))
    return (torch.from_numpy(symbols), ones.clone(), ones.clone(), torch.full((3, 12), float(pitch_neutral)), torch.tensor(lengths),
            torch.from_numpy(energy), torch.from_numpy(pitch), torch.from_numpy(mel), torch.tensor(ref_lengths), torch.tensor([0, 3, 7]))


@functools.lru_cache(maxsize=None)
def _full_targets():
    ''' durations (with symbols of 0, 1 and 2 frames), energies and pitches (with unvoiced symbols) for the batch, zero past the lengths '''
    rng = np.random.RandomState(12)
    lengths = [12, 9, 7]
    t_dur = np.zeros((3, 12), dtype=np.int64)
    t_energy, t_pitch = np.zeros((3, 12), dtype=np.float32), np.zeros((3, 12), dtype=np.float32)
    for b, n in enumerate(lengths):
        t_dur[b, :n] = rng.randint(0, 8, size=n)
        t_dur[b, :3] = [1, 0, 2]
        t_energy[b, :n] = rng.standard_normal(n)
        t_pitch[b, :n] = np.where(rng.uniform(size=n) < 0.7, rng.standard_normal(n), 0.)
    return torch.from_numpy(t_dur), torch.from_numpy(t_energy), torch.from_numpy(t_pitch)


def _run(model, hp, inputs, transform, targets=None):
    ''' [dur, dur_int, energy, pitch, input_lengths, mel, output_lengths, weights] as NumPy (floats as fp32) '''
    args = (tuple(t.to(DEV) for t in inputs), transform, hp)
    enc, dec, weights = model.inference(*args) if targets is None else model.inference(*args, prosody_targets=targets)
    torch.cuda.synchronize()
    return [(t.float() if t.is_floating_point() else t).cpu().numpy() for t in list(enc) + list(dec) + [weights]]


def _targets_on_device(what=None):
    from daft_exprt.clone import ProsodyTargets
    t_dur, t_energy, t_pitch = _full_targets()
    t = ProsodyTargets(durations=t_dur.to(DEV), energy=t_energy.to(DEV), pitch=t_pitch.to(DEV))
    return t if what is None else t.select(what)


def test_inference_without_targets_is_unchanged():
    model, hp = _model()
    inputs = _batch(0.)
    plain = _run(model, hp, inputs, 'add')
    none = model.inference(tuple(t.to(DEV) for t in inputs), 'add', hp, prosody_targets=None)
    none = [t.cpu().numpy() for t in none[0]] + [t.cpu().numpy() for t in none[1]] + [none[2].cpu().numpy()]
    assert len(plain) == len(none) == 8
    for a, b in zip(plain, none):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_inference_with_full_targets_returns_the_targets():
    ''' The returned pitch can be compared bit for bit only under 'multiply' with factor 0, where `dx_prosody_control` leaves a
        pitch as it is.  Under 'add' every voiced pitch goes through (log(exp(std * p + mean) + shift) - mean) / std, which is not
        the identity in fp32 even at a shift of 0 Hz: that run cannot be bit-exact, and its pitch is held to the tolerance
        tests/test_gpu_model.py holds the inference golden's pitch to.  Integers and energy are exact in both runs. '''
    model, hp = _model()
    t_dur, t_energy, t_pitch = (t.numpy() for t in _full_targets())
    sounding = t_dur > 0
    # 'multiply' with factor 0 leaves the pitch as it is: the floats come back bit for bit (after the zeroing of silent symbols)
    dur, dur_int, energy, pitch, _, mel, out_len, _ = _run(model, hp, _batch(0.), 'multiply', _targets_on_device())
    assert model.last_frame_exact.tolist() == [1, 1, 1]
    assert dur_int.tolist() == t_dur.tolist() and out_len.tolist() == t_dur.sum(axis=1).tolist()
    assert energy.tobytes() == np.where(sounding, t_energy, 0).astype(np.float32).tobytes()
    assert pitch.tobytes() == np.where(sounding, t_pitch, 0).astype(np.float32).tobytes()
    seconds = np.array([[P.target_seconds(f, hp.hop_length, hp.sampling_rate) for f in row] for row in t_dur], dtype=np.float32)
    assert dur.tobytes() == seconds.tobytes()
    # the mel: the CPU oracle's own stages on the forced values
    state = {k: v.detach().float().cpu() for k, v in model.state_dict().items()}
    want_enc, (want_mel, want_len) = P.forced_inference(state, hp, _batch(0.), *_full_targets())
    assert want_len.tolist() == out_len.tolist() and mel.shape == tuple(want_mel.shape)
    rel = float(np.abs(mel - want_mel.numpy()).max() / np.abs(want_mel.numpy()).max())
    print(f'forced mel against the oracle stages: {rel:.2e} of the largest magnitude (bound {MEL_TOL})')
    assert rel <= MEL_TOL
    for b, n in enumerate(out_len):
        assert not mel[b, :, n:].any()
    # 'add' with a shift of 0 Hz: integers and energy as above; the pitch goes through exp and log and comes back within the bound
    # tests/test_gpu_model.py holds the inference golden's pitch to
    _, dur_int, energy, pitch, _, _, out_len, _ = _run(model, hp, _batch(0.), 'add', _targets_on_device())
    assert dur_int.tolist() == t_dur.tolist() and out_len.tolist() == t_dur.sum(axis=1).tolist()
    assert energy.tobytes() == np.where(sounding, t_energy, 0).astype(np.float32).tobytes()
    want = np.where(sounding, t_pitch, 0)
    assert not pitch[want == 0].any() and np.abs(pitch - want).max() <= 5 * MEL_TOL * np.abs(want).max()


def test_partial_cloning_leaves_the_other_predictions_alone():
    model, hp = _model()
    free = _run(model, hp, _batch(0.), 'add')
    cloned = _run(model, hp, _batch(0.), 'add', _targets_on_device(('dur',)))
    t_dur = _full_targets()[0].numpy()
    assert cloned[1].tolist() == t_dur.tolist() and model.last_frame_exact.tolist() == [1, 1, 1]
    both = (free[1] > 0) & (cloned[1] > 0)
    assert both.sum() >= 12
    for q in (2, 3):
        assert cloned[q][both].tobytes() == free[q][both].tobytes()
    # and a row without weight is synthesised as if there were no targets at all
    from daft_exprt.clone import ProsodyTargets
    t = _targets_on_device().masked(torch.tensor([True, False, True]))
    mixed = _run(model, hp, _batch(0.), 'add', t)
    assert model.last_frame_exact.tolist() == [1, 0, 1]
    for q in range(4):
        assert mixed[q][1].tobytes() == free[q][1].tobytes()
    assert mixed[6][1] == free[6][1]
    _run(model, hp, _batch(0.), 'add')
    assert model.last_frame_exact is None                                # the flags are those of the last call, never older ones
    with pytest.raises(ValueError):
        zero = ProsodyTargets(durations=torch.zeros((3, 12), dtype=torch.int64, device=DEV))
        model.inference(tuple(t.to(DEV) for t in _batch(0.)), 'add', hp, prosody_targets=zero)
    with pytest.raises(ValueError):
        raw = ProsodyTargets(pitch=torch.ones((3, 12), device=DEV), units='raw')
        model.inference(tuple(t.to(DEV) for t in _batch(0.)), 'add', hp, prosody_targets=raw)


def test_full_targets_in_bf16():
    model, hp = _model('bf16')
    t_dur = _full_targets()[0].numpy()
    dur, dur_int, energy, pitch, _, mel, out_len, weights = _run(model, hp, _batch(0.), 'add', _targets_on_device())
    assert dur_int.tolist() == t_dur.tolist() and out_len.tolist() == t_dur.sum(axis=1).tolist()
    assert all(np.isfinite(a.astype(np.float32)).all() for a in (dur, energy, pitch, mel, weights))


# ---- end to end --------------------------------------------------------------------------------------------------------------------------

#             name    seconds  silence in front  phonemised sentence   (the recordings and sentences of tests/test_gpu_align.py)
UTTERANCES = (('u0', 1.2, 0.15, '{HH AH0 L OW1} , {W ER1 L D} . ~'),
              ('u1', 0.9, 0.00, '{G UH1 D} {D EY1} ~'),
              ('u2', 1.0, 0.25, '{Y EH1 S} ? {N OW1} ! ~'))
SHORT = ('u3', '{N OW1} ~')                                             # its recording: 400 samples, less than half an analysis window


def _wave(seconds, lead, seed):
    ''' silence, a noise burst, a short gap, a second burst, silence: the sounding stretch is at least 0.55 s long '''
    rng = np.random.RandomState(seed)
    n, first = int(seconds * FS), int(lead * FS)
    wav = 1e-4 * rng.standard_normal(n)
    last = n - int(0.1 * FS)
    gap = (first + last) // 2
    wav[first: gap - 600] += 0.2 * rng.standard_normal(gap - 600 - first)
    wav[gap + 600: last] += 0.3 * rng.standard_normal(last - gap - 600)
    return wav.astype(np.float32)


def _waves(with_short):
    waves = [_wave(seconds, lead, 40 + k) for k, (_, seconds, lead, _) in enumerate(UTTERANCES)]
    return waves + ([(1e-2 * np.random.RandomState(9).standard_normal(400)).astype(np.float32)] if with_short else [])


def _sentences(tmp_path, with_short):
    from daft_exprt.generate import read_phonemised_sentences
    rows = [(u[0], u[3]) for u in UTTERANCES] + ([SHORT] if with_short else [])
    path = tmp_path / 'phonemised.txt'
    path.write_text(''.join(f'{name}|{text}\n' for name, text in rows), encoding='utf-8')
    return str(path), read_phonemised_sentences(str(path))[0], [r[0] for r in rows]


def _clone_inputs(hp, sentences, waves):
    ''' (symbols, lengths, wavs, sample counts, source speakers, target speakers, symbol ids) of `clone_batch` '''
    from daft_exprt.generate import _symbol_ids
    ids = [_symbol_ids(s, hp) for s in sentences]
    B = len(ids)
    symbols = torch.zeros((B, max(len(i) for i in ids)), dtype=torch.int64)
    wavs = torch.zeros((B, max(len(w) for w in waves)), dtype=torch.float32)
    for b in range(B):
        symbols[b, :len(ids[b])], wavs[b, :len(waves[b])] = torch.tensor(ids[b]), torch.from_numpy(waves[b])
    lengths = torch.tensor([len(i) for i in ids], dtype=torch.int64, device=DEV)
    source = torch.tensor([0, 3, 7, 3][:B], device=DEV)
    target = torch.tensor([5, 5, 2, 2][:B], device=DEV)
    return symbols.to(DEV), lengths, wavs.to(DEV), [len(w) for w in waves], source, target, ids


def _clone(model, hp, sentences, waves, **kw):
    from daft_exprt.clone import clone_batch
    *inputs, ids = _clone_inputs(hp, sentences, waves)
    return ids, clone_batch(model, *inputs, hp, **kw)


def _flat(out):
    ''' every tensor of a clone_batch result as bytes '''
    parts = {k: out[k] for k in ('mel', 'n_frames', 'dur', 'dur_int', 'energy', 'pitch', 'frame_exact', 'wavs', 'n_samples')}
    parts.update({f'score {k}': v for k, v in out['scores'].items()})
    parts.update({f'info {k}': v for k, v in out['info'].items()})
    return {k: None if v is None else v.cpu().numpy().tobytes() for k, v in parts.items()}


def test_clone_batch_is_frame_synchronous_with_the_recordings(tmp_path):
    from daft_exprt.clone import SCORE_KEYS
    model, hp = _model()
    _, sentences, _ = _sentences(tmp_path, False)
    ids, out = _clone(model, hp, sentences, _waves(False), use_griffin_lim=True)
    info = {k: v.cpu().numpy() for k, v in out['info'].items()}
    rec = out['targets'].durations.cpu().numpy()
    scores = {k: v.cpu().numpy() for k, v in out['scores'].items()}
    assert tuple(scores) == SCORE_KEYS
    assert info['status'].tolist() == [0, 0, 0] and info['pool_status'].tolist() == [0, 0, 0]         # no row may be left out
    assert out['frame_exact'].tolist() == [True, True, True]
    assert out['n_frames'].tolist() == info['frames'].tolist() == info['n_rec'].tolist()
    assert out['dur_int'].cpu().numpy().tolist() == rec.tolist()
    for b, n in enumerate(len(i) for i in ids):
        print(f'{UTTERANCES[b][0]}: frames {info["frames"][b]}, rec {rec[b, :n].tolist()}, dropped {info["dropped"][b]}, '
              f'scores {({k: float(v[b]) for k, v in scores.items()})}')
        assert rec[b, :n].sum() == info['frames'][b] and not rec[b, n:].any()
        assert np.isfinite(scores['mcd_db'][b]) and scores['mcd_db'][b] > 0
        assert np.isfinite(scores['energy_pcc'][b]) and np.isfinite(scores['vuv_error'][b])
        assert not out['mel'][b, :, int(out['n_frames'][b]):].any()
    again = _clone(model, hp, sentences, _waves(False), use_griffin_lim=True)[1]
    first, second = _flat(out), _flat(again)
    for key in first:
        assert first[key] == second[key], key
    # without audio only the mel is scored; cloning the durations alone is still frame-exact
    _, quiet = _clone(model, hp, sentences, _waves(False), what=('dur',))
    assert quiet['wavs'] is None and quiet['frame_exact'].tolist() == [True] * 3 and quiet['n_frames'].tolist() == info['frames'].tolist()
    assert torch.isfinite(quiet['scores']['mcd_db']).all() and torch.isnan(quiet['scores']['pitch_pcc']).all()
    # without the durations nothing is frame-exact and the frame-against-frame scores are undefined
    _, loose = _clone(model, hp, sentences, _waves(False), what=('energy', 'pitch'))
    assert loose['frame_exact'].tolist() == [False] * 3 and torch.isnan(loose['scores']['mcd_db']).all()


def test_a_recording_that_cannot_be_aligned_is_synthesised_free_running(tmp_path):
    model, hp = _model()
    _, sentences, _ = _sentences(tmp_path, True)
    ids, out = _clone(model, hp, sentences, _waves(True), use_griffin_lim=True)
    assert out['info']['status'].tolist() == [0, 0, 0, 4] and out['frame_exact'].tolist() == [True, True, True, False]
    assert int(out['n_frames'][3]) > 0 and int(out['info']['n_rec'][3]) == 1 + hp.filter_length // hp.hop_length
    for key, v in out['scores'].items():
        assert torch.isnan(v[3]), key
        if key in ('mcd_db', 'energy_pcc', 'vuv_error'):
            assert torch.isfinite(v[:3]).all(), key
    for name in ('w_dur', 'w_energy', 'w_pitch'):
        assert not getattr(out['targets'], name)[3].any()
    # the other rows are what they are without the fourth
    _, three = _clone(model, hp, sentences[:3], _waves(False), use_griffin_lim=True)
    L = three['dur_int'].shape[1]
    assert out['dur_int'][:3, :L].tolist() == three['dur_int'].tolist() and out['n_frames'][:3].tolist() == three['n_frames'].tolist()


def test_the_synthesis_driver_puts_targets_where_the_collate_puts_their_sentences(tmp_path):
    from daft_exprt.clone import ProsodyTargets
    from daft_exprt.generate import _symbol_ids, generate_mel_specs
    model, hp = _model()
    _, sentences, names = _sentences(tmp_path, False)
    counts = [len(_symbol_ids(s, hp)) for s in sentences]
    assert counts == [11, 7, 8]                                          # the collate's order is 0, 2, 1
    inputs = _batch(0.)
    refs = [(inputs[5][b, :n].numpy(), inputs[6][b, :n].numpy(), inputs[7][b, :, :n].numpy()) for b, n in enumerate(inputs[8].tolist())]
    rng = np.random.RandomState(13)
    frames = [rng.randint(0, 7, size=n) for n in counts]
    for f in frames:
        f[:3] = [2, 0, 1]
    targets = [ProsodyTargets(durations=torch.tensor(frames[0][None])), None, ProsodyTargets(durations=torch.tensor(frames[2][None]))]
    run = lambda sub, **kw: generate_mel_specs(model, sentences, list(names), [5, 3, 7], refs, str(tmp_path / sub), hp, batch_size=3, **kw)
    free, cloned = run('free'), run('cloned', prosody_targets=targets)
    assert list(free) == list(cloned) and len(cloned) == 3
    key = lambda b: next(k for k in cloned if k.startswith(f'{names[b]}_spk_'))
    for b in (0, 2):
        assert cloned[key(b)][1].tolist() == frames[b].tolist() and cloned[key(b)][4].shape[1] == frames[b].sum()
    for q in range(4):                                                   # the sentence without targets is synthesised as before
        assert cloned[key(1)][q].tobytes() == free[key(1)][q].tobytes()


def test_clone_cli(tmp_path):
    from daft_exprt.align import STATUS
    from daft_exprt.audio import write_wav_int16
    from daft_exprt.clone import SCORE_KEYS
    model, hp = _model()
    ckpt = str(tmp_path / 'DaftExprt_test')
    torch.save({'iteration': 0, 'state_dict': dict(model.state_dict()), 'config_params': dict(vars(hp))}, ckpt)
    text, _, names = _sentences(tmp_path, True)
    wav_dir, out_dir = tmp_path / 'wavs', tmp_path / 'out'
    wav_dir.mkdir()
    for name, wav in zip(names, _waves(True)):
        write_wav_int16(str(wav_dir / f'{name}.wav'), FS, np.clip(np.trunc(wav * 32768.), -32768, 32767).astype(np.int16))
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'clone.py'), '-chk', ckpt, '-tf', text, '-wd', str(wav_dir), '-spk', 'spk05',
                        '-src', '0', '3', '7', '3', '-out', str(out_dir), '-bs', '3'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    report = json.load(open(out_dir / 'clone_report.json'))
    assert list(report['files']) == names and report['audio'] == 'griffin-lim' and report['what'] == ['dur', 'energy', 'pitch']
    assert report['summary']['files'] == 4 and report['summary']['frame_exact'] == 3
    assert report['summary']['status'] == {str(k): {0: 3, 4: 1}.get(k, 0) for k in sorted(STATUS)}
    assert report['summary']['scores']['mcd_db']['files'] == 3 and report['summary']['scores']['mcd_db']['mean'] > 0
    for name in names:
        record = report['files'][name]
        assert tuple(record) == ('status', 'frames', 'begin', 'moved', 'path_cost', 'dropped', 'pool_status', 'usable', 'frame_exact', 'scores')
        assert tuple(record['scores']) == SCORE_KEYS
        mel = np.load(out_dir / f'{name}.npz')['mel_spec']
        wav = (out_dir / f'{name}.wav').read_bytes()                  # the Griffin-Lim preview: 64-bit float, (frames - 2) hops and a window
        n = (mel.shape[1] - 2) * hp.hop_length + hp.filter_length
        assert wav[:4] == b'RIFF' and wav[8:12] == b'WAVE' and 8 * n < len(wav) <= 8 * n + 64 and mel.shape[0] == 80
        if name == 'u3':
            assert record['status'] == 4 and not record['usable'] and not record['frame_exact'] and all(v is None for v in record['scores'].values())
        else:
            assert record['status'] == 0 and record['pool_status'] == 0 and record['usable'] and record['frame_exact'] and mel.shape[1] == record['frames'] and record['scores']['mcd_db'] > 0
    assert 'u3: status 4, pool_status 0, synthesised free-running' in r.stderr


def test_cloning_through_a_learned_aligner(tmp_path):
    ''' the other source of boundaries: `targets_from_recordings` / `clone_batch` hand the same arguments to `Aligner.align_batch`,
        and `scripts/clone.py --aligner` loads one.  The aligner is random: whatever status a row ends with, a usable row is cloned
        frame-exact with the aligner's own durations and any other row is synthesised free-running. '''
    from daft_exprt.aligner import Aligner, save_aligner
    from daft_exprt.audio import write_wav_int16
    model, hp = _model()
    text, sentences, names = _sentences(tmp_path, True)
    torch.manual_seed(2)
    aligner = Aligner(len(hp.symbols), hp.n_mel_channels, hidden=32, att_dim=16).to(DEV)
    ids, out = _clone(model, hp, sentences, _waves(True), aligner=aligner)
    direct = aligner.align_batch(*_clone_inputs(hp, sentences, _waves(True))[:5], hp)
    info = out['info']
    for key in ('status', 'begin', 'frames', 'moved'):
        assert info[key].tolist() == direct[key].tolist(), key
    assert out['targets'].durations.tolist() == direct['rec_durations'].tolist()
    status, usable, exact = info['status'].tolist(), info['usable'].tolist(), out['frame_exact'].tolist()
    print(f'learned aligner: status {status}, usable {usable}, frames {info["frames"].tolist()} -> {out["n_frames"].tolist()}')
    assert status[3] == 4 and usable == [s == 0 for s in status] == exact
    for b in range(4):
        if usable[b]:
            assert int(out['n_frames'][b]) == int(info['frames'][b]) and out['dur_int'][b].tolist() == direct['rec_durations'][b].tolist()
            assert bool(torch.isfinite(out['scores']['mcd_db'][b]))
        else:
            assert int(out['n_frames'][b]) > 0 and bool(torch.isnan(out['scores']['mcd_db'][b]))
    # and the command line with --aligner
    ckpt, aligner_file = str(tmp_path / 'DaftExprt_test'), str(tmp_path / 'aligner.pt')
    torch.save({'iteration': 0, 'state_dict': dict(model.state_dict()), 'config_params': dict(vars(hp))}, ckpt)
    save_aligner(aligner, aligner_file)
    wav_dir, out_dir = tmp_path / 'wavs', tmp_path / 'out'
    wav_dir.mkdir()
    for name, wav in zip(names, _waves(True)):
        write_wav_int16(str(wav_dir / f'{name}.wav'), FS, np.clip(np.trunc(wav * 32768.), -32768, 32767).astype(np.int16))
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'clone.py'), '-chk', ckpt, '-tf', text, '-wd', str(wav_dir), '-spk', '5',
                        '-out', str(out_dir), '--aligner', aligner_file, '--clone', 'dur'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    report = json.load(open(out_dir / 'clone_report.json'))
    assert report['aligner'] == 'learned' and report['what'] == ['dur'] and list(report['files']) == names
    assert report['files']['u3']['status'] == 4 and report['summary']['usable'] == report['summary']['frame_exact']
