"""The conv weight-gradient kernels of csrc/conv_wgrad.hip -- conv_wgrad_kernel (register-staged), wgrad_ring_body (LDS-DMA ring) and
its pair launch, wgrad_reduce_kernel / wgrad_reduce_multi_kernel, the atomics fallback -- through ops.conv1d_wgrad and
ops.conv1d_wgrad_multi, compared element by element with the float64 oracle of tests/wgrad_oracle.py (its docstring has the contract
as read from the kernels, the cases W1-W8 and why integer operands make the comparison exact; tests/test_wgrad_host.py holds each
case to its purpose).

Kernel families (wgrad_oracle.FAMILIES: dY storage, X storage, compute type): f32 (fp32 fp32 fp32), cast (fp32 fp32 bf16), dy32 (fp32 bf16
bf16), x32 (bf16 fp32 bf16) -- the four on conv_wgrad_kernel -- and ring (all bf16: wgrad_ring_body).  Modes: ws (partial tiles in a
caller-owned workspace of exactly ops.wgrad_ws_floats floats, NaN before the call and with NaN behind it, then the reduce launch) and
atomics (ops.WGRAD_WORKSPACE False, switched with monkeypatch).

What runs (624 tests):
    test_exact (540)                       every family on every (case, channel set) of wgrad_oracle.CASE_SETS: both integer draws in
                                           ws mode, one of them in atomics mode (alternating over families and sets)
    test_exact_on_channel_slices (14)      W2 at (136, 200, 3) and (128, 384, 1), every family in ws mode, f32 and ring also in atomics
                                           mode: operands are channel slices of wider tensors of NaN
    test_exact_without_bias_gradient (10)  db = None, every family and mode, W2 at (128, 256, 3) and (128, 384, 1)
    test_multi_exact (14)                  ops.conv1d_wgrad_multi on W3 and W4: the FFT-block list, the same with the k = 1 pair first,
                                           three k = 1 in a row (a pair and a single), db = None inside the pair and on a k = 3 item;
                                           all-bf16 operands (pair launch), the first and third list also fp32 (multi reduce behind the
                                           staged kernel)
    test_rounded (45)                      Gaussian operands on W2, W3, W4, every family: (128, 256, 3) and (128, 384, 1) in ws mode, one
                                           of them in atomics mode, against the derived bound below
    test_refusals_come_before_any_launch   Cin = 12, row strides of 12, taps = 5, fp32 compute with a bf16 operand
Every exact test asserts torch.equal(dW, initial dW + oracle) and the same for db: no tolerance.  Every ws-mode test also asserts that
the whole workspace was written (no NaN left: the workgroups without items write zero tiles) and nothing behind it.

Measured on an MI355X.  No defect of the kernels or of the wrappers came to light.  The file takes 5.7 s (624 tests); the first test
0.44 s (it loads the library), the multi tests of W4 0.18 s each, every other test 0.1 s or less.
test_rounded, error / bound per element, the worst and the largest median over the cases and sets of a (family, mode):
    family  mode     dW worst  median     db worst  median     n
    f32     ws       1.5e-3    8.0e-5     4.7e-4    6.6e-5     6
    f32     atomics  1.1e-3    8.0e-5     3.3e-4    6.1e-5     3
    cast    ws       4.0e-4    2.4e-5     5.8e-5    8.6e-7     6
    cast    atomics  4.0e-4    2.4e-5     3.9e-5    7.4e-7     3
    dy32    ws       4.0e-4    2.4e-5     5.8e-5    7.3e-7     6
    dy32    atomics  4.0e-4    2.4e-5     3.9e-5    7.3e-7     3
    x32     ws       4.0e-4    2.4e-5     5.8e-5    8.6e-7     6
    x32     atomics  4.0e-4    2.4e-5     3.9e-5    8.6e-7     3
    ring    ws       4.0e-4    2.4e-5     5.8e-5    1.2e-6     6
    ring    atomics  4.0e-4    2.4e-5     3.9e-5    1.1e-6     3
The bound is a worst-case one, linear in the 1168 to 4143 contracted rows, and the errors of a sum grow like its square root: the
ratios are small, and the largest belong to the shortest case (W2).  The four bf16-compute families agree in dW to the printed digits:
they multiply the same rounded operands.  What carries the weight of the file are the exact tests.

Built to fail, in scratch builds that are not committed, each run once (failures of this file's 624 tests | of the four older wgrad
tests of test_gpu_kernels.py).  Every mutation reads fewer rows or swaps two in-range indices:
  (a) staged kernel, X fetch: `n <= flim` -> `n < flim` -- 263: every k = 3 test of the four staged families on W1-W7 (228 test_exact, W8
      has no such row), their slices, no-bias, rounded (20 of 20) and the fp32 FFT list on W3 and W4; no ring test, no k = 1 test (k = 1 never
      meets row flim) | 1 of 4: test_wgrad_matches_autograd_all_dtype_pairs;
  (b) ring kernel, X rows: `n <= xlim` -> `n < xlim` (xlim lowered by one, written so that N = 1 cannot wrap) -- 127, all ring: every ring
      test_exact but the six k = 1 ones of W5 (102: k = 1 meets the dropped row only where an utterance reaches N), every ring slice,
      no-bias, multi (10) and rounded (9) test | 2 of 4: all_dtype_pairs, ring_kernel_ragged_bf16;
  (c) ring k = 3: the `tail0` read one row up -- 68, all ring at k = 3 on W1-W5 and W7 (the items of W6 and W8 have at most 8 rows: the dword behind
      position 63 meets zeros on both sides), 8 multi, 5 rounded | the same 2 of 4;
  (d) wgrad_reduce_kernel: `per = nsplit >> 2` -- 255: every ws-mode single-launch test with nsplit 1, 2 or 6 (W1, W2, W3, W7, W8), all
      five families; none at nsplit 8, 16, 32, where per is unchanged, none in atomics mode, none of the multi tests (they reduce
      in wgrad_reduce_multi_kernel) | 4 of 4 (their shapes have nsplit 1 or 2, where per becomes 0);
  (e) ring: `split = bid / ntiles` kept beside `tile = bid / nsplit` under `by_split` -- 32, all ring on W4, W5, W6 at 2, 3 and 8 tiles
      (24 test_exact in both modes, 5 multi, 3 rounded); in ws mode the unwritten partial tiles show as NaN | 0 of 4: no older test
      reaches `by_split`.
Mutations (a) - (d) also fail older tests: each drops a row per utterance or whole splits, which the 2e-2 / 2e-3 tolerances of those
tests do see on their shapes; what they cannot see is where the rows are, (e), and anything at nsplit > 2.
"""
import pytest
import torch

from tests import wgrad_oracle as W

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
NAN = float('nan')
GUARD = 4096          # floats of NaN behind the caller-owned workspace: they must stay NaN
U = 2. ** -23         # allowed per fp32 addition: twice the unit roundoff (the adds inside an MFMA need not round to nearest)


def _operand(t, dtype, sliced, left):
    ''' t (B, N, C) on the device in `dtype` -- with `sliced` as a channel slice of a wider tensor of NaN '''
    t = t.to(DEV).to(dtype)
    if not sliced:
        return t
    B, N, C = t.shape
    wide = torch.full((B, N, C + left + 8), NAN, dtype=dtype, device=DEV)
    wide[:, :, left:left + C] = t
    return wide[:, :, left:left + C]


def _dw0(p):
    return (p.init_dw if p.taps == 3 else p.init_dw[:, :, 0]).contiguous().to(DEV)


def _poisoned_ws(n):
    buf = torch.full((n + GUARD,), NAN, dtype=torch.float32, device=DEV)
    return buf, buf[:n]


def _check_ws(buf, ws):
    assert bool(torch.isnan(buf[ws.numel():]).all()), 'the kernels wrote past the workspace'
    assert bool(torch.isfinite(ws).all()), 'a partial tile of the workspace was not written (or holds a poisoned row)'


def _run(p, fam, use_ws, monkeypatch, sliced=False, with_db=True):
    ''' one ops.conv1d_wgrad call of family `fam` on the operands of problem p: poisoned rows, poisoned caller-owned workspace of
        exactly wgrad_ws_floats floats (workspace mode), dW and db starting from p.init_* '''
    from daft_exprt import ops
    dyt, xt, cd = W.FAMILIES[fam]
    monkeypatch.setattr(ops, 'WGRAD_WORKSPACE', use_ws)
    dy, x = _operand(p.dy, dyt, sliced, 8), _operand(p.x, xt, sliced, 16)
    assert (dy.stride(1) != p.cout and x.stride(1) != p.cin) == sliced
    dw, db = _dw0(p), (p.init_db.to(DEV) if with_db else None)
    lens = None if p.lens is None else torch.tensor(p.lens, dtype=torch.int64, device=DEV)
    buf = ws = None
    if use_ws:
        n = ops.wgrad_ws_floats(p.B, p.N, p.cin, p.cout, p.taps)
        assert n == p.nsplit * p.tiles * p.taps * W.TILE_FLOATS_PER_TAP
        buf, ws = _poisoned_ws(n)
    ops.conv1d_wgrad(dy, x, dw, db, cd, lens, ws=ws)
    torch.cuda.synchronize()
    if use_ws:
        _check_ws(buf, ws)
    return dw, db


def _assert_exact(p, dw, db, label=''):
    ''' torch.equal with the float64 oracle; the message says how many elements differ and where the first one is '''
    want = p.init_dw.double() + p.dw
    for name, got, want in (('dW', dw, want if p.taps == 3 else want[:, :, 0]), ('db', db, p.init_db.double() + p.db)):
        if got is None:
            continue
        got = got.double().cpu()
        assert got.shape == want.shape
        bad = got != want
        first = tuple(bad.nonzero()[0].tolist()) if bool(bad.any()) else None
        assert torch.equal(got, want), (f'{label}{p.case} {W.set_id(p.chset)} {p.draw} {name}: {int(bad.sum())} of {bad.numel()} elements differ, the first at '
                                        f'{first}: {float(got[first])} for {float(want[first])}')


def _exact_params():
    ''' every family meets every (case, channel set) with both draws in workspace mode and with one draw in atomics mode (the draws
        alternate over the families and the channel sets) '''
    out = []
    for case in W.CASES:
        for k, chset in enumerate(W.CASE_SETS[case]):
            for d, draw in enumerate(W.EXACT_DRAWS):
                out += [(case, chset, draw, fam, 'ws') for fam in W.FAMILIES]
                out += [(case, chset, draw, fam, 'atomics') for j, fam in enumerate(W.FAMILIES) if (j + k) % 2 == d]
    return out


def _id(v):
    return W.set_id(v) if isinstance(v, tuple) else str(v)


# ----------------------------------------------------------------------------- 1. exact
@pytest.mark.parametrize('case,chset,draw,fam,mode', _exact_params(), ids=_id)
def test_exact(case, chset, draw, fam, mode, monkeypatch):
    p = W.problem(case, chset, draw)
    assert p.nsplit == W.expected_nsplit(case, chset)
    dw, db = _run(p, fam, mode == 'ws', monkeypatch)
    _assert_exact(p, dw, db)


SLICED = [('W2', chset, W.EXACT_DRAWS[(j + k) % 2], fam, mode) for k, chset in enumerate(((136, 200, 3), (128, 384, 1)))
          for j, fam in enumerate(W.FAMILIES) for mode in (('ws', 'atomics') if fam in ('ring', 'f32') else ('ws',))]


@pytest.mark.parametrize('case,chset,draw,fam,mode', SLICED, ids=_id)
def test_exact_on_channel_slices(case, chset, draw, fam, mode, monkeypatch):
    ''' every operand a channel slice of a wider tensor that holds NaN around it: lddy != Cout, ldx != Cin '''
    p = W.problem(case, chset, draw)
    dw, db = _run(p, fam, mode == 'ws', monkeypatch, sliced=True)
    _assert_exact(p, dw, db)


@pytest.mark.parametrize('mode', ['ws', 'atomics'])
@pytest.mark.parametrize('fam', list(W.FAMILIES))
def test_exact_without_bias_gradient(fam, mode, monkeypatch):
    ''' db = None: dW is the same, nothing else is written '''
    for chset, draw in (((128, 256, 3), 'dy8'), ((128, 384, 1), 'x8')):
        p = W.problem('W2', chset, draw)
        dw, db = _run(p, fam, mode == 'ws', monkeypatch, with_db=False)
        assert db is None
        _assert_exact(p, dw, None)


# ----------------------------------------------------------------------------- 2. multi and pair
FFT = ((128, 1024, 3), (1024, 128, 3), (128, 384, 1), (128, 128, 1))
LISTS = {
    'fft': (FFT, None),                                                       # two k = 3 launches, then the k = 1 pair
    'pair_first': (FFT[2:] + FFT[:2], None),
    'pair_and_single': (((128, 384, 1), (128, 128, 1), (384, 128, 1)), None),   # three k = 1 in a row: the `paired` flag
    'no_db_in_pair': (FFT, 2),
    'no_db_k3': (FFT, 1),
}
MULTI = [(case, name, W.EXACT_DRAWS[(i + j) % 2], fam) for i, case in enumerate(('W3', 'W4')) for j, name in enumerate(LISTS)
         for fam in (('ring', 'f32') if name in ('fft', 'pair_and_single') else ('ring',))]


@pytest.mark.parametrize('case,name,draw,fam', MULTI, ids=_id)
def test_multi_exact(case, name, draw, fam):
    ''' ops.conv1d_wgrad_multi: the GEMM launches (with all-bf16 operands the k = 1 neighbours go out as conv_wgrad_ring_pair_kernel)
        and ONE wgrad_reduce_multi_kernel launch, every dW and db against the float64 oracle '''
    from daft_exprt import ops
    chsets, no_db = LISTS[name]
    dyt, xt, cd = W.FAMILIES[fam]
    probs = [W.problem(case, chset, draw) for chset in chsets]
    B, N, lens = W.CASES[case]
    assert all(p.nsplit == W.expected_nsplit(case, p.chset) for p in probs)
    items = [(p.dy.to(DEV).to(dyt), p.x.to(DEV).to(xt), _dw0(p), None if i == no_db else p.init_db.to(DEV)) for i, p in enumerate(probs)]
    n = ops.wgrad_multi_ws_floats([(B, N, p.cin, p.cout, p.taps) for p in probs])
    assert n == sum(p.nsplit * p.tiles * p.taps * W.TILE_FLOATS_PER_TAP for p in probs)
    buf, ws = _poisoned_ws(n)
    ops.conv1d_wgrad_multi(items, cd, torch.tensor(lens, dtype=torch.int64, device=DEV), ws=ws)
    torch.cuda.synchronize()
    _check_ws(buf, ws)
    for i, (p, (_, _, dw, db)) in enumerate(zip(probs, items)):
        _assert_exact(p, dw, db, label=f'item {i} of {name}: ')


# ----------------------------------------------------------------------------- 3. rounded
ROUNDED = [(case, chset, fam, mode) for case in ('W2', 'W3', 'W4') for fam in W.FAMILIES
           for chset, mode in (((128, 256, 3), 'ws'), ((128, 384, 1), 'ws'), ((128, 256, 3) if case != 'W3' else (128, 384, 1), 'atomics'))]


@pytest.mark.parametrize('case,chset,fam,mode', ROUNDED, ids=_id)
def test_rounded(case, chset, fam, mode, monkeypatch):
    ''' Gaussian operands: the fp32 -> bf16 cast of the mixed-type staging and ordinary magnitudes.  The oracle contracts the operands
        already rounded to the compute type; each product then enters at most R + S + 2 fp32 additions (R contracted rows, S splits),
        each allowed 2^-23:  |dW - oracle| <= (R + S + 2) 2^-23 A,  |db - oracle| <= (R + 2) 2^-23 Ab, per element.  dW and db start from
        zero '''
    p = W.problem(case, chset, 'gauss', W.FAMILIES[fam][2], True)
    dw, db = _run(p, fam, mode == 'ws', monkeypatch)
    ratios = []
    for got, ref, bound in ((dw, p.dw if p.taps == 3 else p.dw[:, :, 0], (p.R + p.nsplit + 2) * U * (p.A if p.taps == 3 else p.A[:, :, 0])),
                            (db, p.db, (p.R + 2) * U * p.Ab)):
        assert float(bound.min()) > 0.
        r = (got.double().cpu() - ref).abs() / bound
        ratios.append((float(r.max()) if bool(torch.isfinite(r).all()) else float('inf'), float(r.median())))
    print(f'RATIO {fam} {mode} {case} {W.set_id(chset)}: dW worst {ratios[0][0]:.2e} median {ratios[0][1]:.2e}  db worst {ratios[1][0]:.2e} '
          f'median {ratios[1][1]:.2e}')
    assert ratios[0][0] <= 1. and ratios[1][0] <= 1., ratios


# ----------------------------------------------------------------------------- 4. refusals
def test_refusals_come_before_any_launch():
    ''' the error code the source names, and dW / db untouched '''
    from daft_exprt import _hip as H
    lib, B, N = H.lib(), 2, 16
    f32 = lambda *s: torch.ones(*s, device=DEV)
    bf = lambda *s: torch.ones(*s, device=DEV, dtype=torch.bfloat16)

    def call(dy, x, cd, cin, cout, taps):
        dw, db = torch.full((cout, cin, taps), 7., device=DEV), torch.full((cout,), 7., device=DEV)
        rc = lib.dx_conv1d_wgrad(H.ptr(dy), H.dt(dy), dy.stride(1), H.ptr(x), H.dt(x), x.stride(1), H._DT[cd], H.ptr(dw), H.ptr(db), None, None,
                                 B, N, cin, cout, taps, H.stream())
        torch.cuda.synchronize()
        assert bool((dw == 7.).all()) and bool((db == 7.).all())
        return rc
    DX_ERR_SHAPE, DX_ERR_DTYPE, DX_ERR_UNSUPPORTED = -2, -3, -5          # include/daft_exprt_hip.h
    assert call(f32(B, N, 128), f32(B, N, 12), W.F32, 12, 128, 3) == DX_ERR_SHAPE
    assert b'multiples of 8' in lib.dx_last_error()
    assert call(f32(B, N, 128), f32(B, N, 12)[:, :, :8], W.F32, 8, 128, 3) == DX_ERR_SHAPE          # a row stride of 12 (X)
    assert call(bf(B, N, 12)[:, :, :8], bf(B, N, 128), W.BF16, 128, 8, 1) == DX_ERR_SHAPE          # (dY, in front of the ring kernel)
    assert call(f32(B, N, 128), f32(B, N, 128), W.F32, 128, 128, 5) == DX_ERR_UNSUPPORTED
    assert call(bf(B, N, 128), f32(B, N, 128), W.F32, 128, 128, 3) == DX_ERR_DTYPE
    assert call(f32(B, N, 128), bf(B, N, 128), W.F32, 128, 128, 1) == DX_ERR_DTYPE
    assert b'dtype' in lib.dx_last_error()
