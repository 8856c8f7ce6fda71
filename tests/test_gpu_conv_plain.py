"""The plain conv GEMMs -- ops.conv1d on dx_conv1d / dx_conv1d_wfrag, dx_conv1d_relu_bits and dx_conv1d_wide -- on every kernel path
(ops.plain_path: WREG = conv_wreg_kernel, ROWS64 / ROWS128 / ROWS256 = conv_gemm_kernel without a LayerNorm epilogue; and
conv_wide_kernel), compared element by element with the float64 restatement of tests/conv_plain_oracle.py, whose docstring has the
contract as read from the three kernels.

INTEGER TESTS are exact: operands are small integers (two draws per case: 'small' keeps every output an integer of magnitude <= 256,
exact in bf16; 'big' goes through the bf16 rounding), every partial sum stays below 2^24 (tests/test_conv_plain_host.py), and the
kernel's output must `torch.equal` the oracle's on the contract rows -- computed rows, exact zeros on the zero rows, rows at or past
the fill end dropped (tests.util.fill_end) -- with no tolerance.  Every input holds NaN at and past the fill end; every output starts
as NaN (the ones ops allocates through config.POISON, which is set around every launch) or as the old integers under ACCUMULATE,
sliced operands sit in NaN containers that must stay NaN around the slice; a second identical launch must be bit-equal.
ops.plain_path is asserted before every launch, ops.wide_shape_ok and the plan (read back, compared with conv_ln_oracle.tile_plan) for the wide kernel.

Cases (conv_plain_oracle; P4 and the 256-row P5 run in ONE fresh child process under DX_CONV_WIDE_MI=4):
    P1   ROWS64   B 3, N 70, lens 70 33 1; Cin 8 40 128 160; Cout 128 80 8 (vector epilogue) 1 7 33 (scalar)      6 ladders x k 1, 3
    P2   ROWS128  B 2, N 131, lens 131 64; Cin 40 136 (512 with fp32 weights); Cout 136 264 (135: scalar)          6 ladders x k 1, 3
    P3   ROWS128  B 167, N 385 (64295 rows), one channel tile, Cin 8 40, Cout 8 128, k 3; 166 utterances report ROWS64
    P4   ROWS256  B 3, N 300, lens 300 257 5, Cin 512, Cout 256 264 263, forced; P4n: B 512, N 3, Cout 256 reports ROWS256 unforced
    P5   each height: B 4, N 600, lens 600 255 1 0: dead tiles below and past the fill end; ACCUMULATE leaves them untouched
    R1-4 WREG     B 3 N 300 (ngrp 9) | B 8 N 100 (ngrp 8: zmajor) | B 513 N 3 (serial walk, shares cross utterances) | B 4 N 600
                  (dead tiles zeroed and unwritten, idle groups); Cout 256 512; out bf16 fp32; k 1 3; all four ReLU / gate forms per
                  (output, k); with and without the fragment copy; relu_bits written (compared with pack_bits(y > 0)) and read
    W1-4 wide     B 4 N 128 | B 3 N 300 (fill end 257) | B 70 N 40 (second fill block, rotated chunks) | W1 with tiles=4; Cin 256 384
Options rotate (conv_plain_oracle.OPTS): ReLU, gate (fp32 and bf16), mask_lengths, skip_lengths, transposed_out, ACCUMULATE (fp32 and
bf16), bias None, x / out as channel slices (ldx != Cin, ldy != Cout, ldy % 8 != 0).

    kernel path x ladder x k                         tests that run it
    ROWS64  x 6 ladders x k 1, 3                     test_tiled_integer[P1-*] (48), [P5-rows64-*]; test_rounded[G-rows64-*]
    ROWS128 x 6 ladders x k 1, 3                     test_tiled_integer[P2-*] (27), [P3-*] (k 3), [P5-rows128-*]; test_rounded[G-rows128-*]
    ROWS256 x 5 ladders (bf16 weights) x k 3         test_tall_tiles_in_a_child_process (P4-*, P5-rows256-*, G-rows256-*); [P4n-*]
    WREG    x out bf16, fp32 x k 1, 3 x 4 forms      test_wreg_integer[R*] (16 + 8 with bits); test_rounded[G-wreg-*]
    wide    x Cin 256, 384 x Cout 256, 512           test_wide_integer[W*] (16); test_rounded[G-wide-*]

ROUNDED TESTS: Gaussian operands, one case per kernel path, ladder and tap count; bound per utterance, on the contract rows:
    4 * max|restatement - float64| + 1e-6 * max|float64|
Measured on an MI355X, error / bound (the worst utterance of each test; worst and median over the tap counts, number of figures):
    path      x / w / y / gate           worst  median  n        path      x / w / y / gate           worst  median  n
    rows64    f32 f32 f32 f32            0.210   0.210  2        rows128   f32 f32 f32 f32            0.225   0.225  2
    rows64    f32 bf16 f32 f32           0.250   0.250  2        rows128   f32 bf16 f32 f32           0.250   0.250  2
    rows64    f32 bf16 f32 bf16          0.250   0.250  2        rows128   f32 bf16 f32 bf16          0.250   0.250  2
    rows64    f32 bf16 bf16 bf16         0.250   0.250  2        rows128   f32 bf16 bf16 bf16         0.250   0.250  2
    rows64    bf16 bf16 f32 f32          0.149   0.114  2        rows128   bf16 bf16 f32 f32          0.128   0.112  2
    rows64    bf16 bf16 bf16 bf16        0.250   0.250  2        rows128   bf16 bf16 bf16 bf16        0.250   0.250  2
    rows256   f32 bf16 f32 f32           0.250   0.250  1        wreg      bf16 bf16 f32 f32          0.139   0.123  2
    rows256   f32 bf16 bf16 bf16         0.250   0.250  1        wreg      bf16 bf16 bf16 bf16        0.250   0.250  2
    rows256   bf16 bf16 f32 f32          0.191   0.191  1        wide      bf16 bf16 bf16             0.250   0.250  2
    rows256   bf16 bf16 bf16 bf16        0.250   0.250  1
The factor 4 stands on every ladder.  0.250 exactly means that the largest error of the kernel IS the restatement's own: the bf16
rounding of the same element (bf16-stored outputs), or of x when it is staged in front of bf16 weights -- the device rounds to nearest
even as the oracle does.  With exact products (bf16 / bf16 into fp32) and with fp32 weights only the order of the fp32 sums differs
(the tiled kernel walks 32-channel chunks outermost, the restatement taps): 0.08 - 0.23.  The 165 tests take 10 s together; the
slowest are the child process of the tall tiles (2.9 s: a second interpreter and library load) and P3-bf16-C40-O128 / P3-mixb-C8-O128
(1.6 s each: 64295 x 128 outputs, two draws, moved to the device and back), every other test is below 0.25 s.

Defects: none in the kernels.  One in the wrapper: ops.conv1d passed `out.stride(1)` as the row stride, which torch leaves arbitrary
for a one-row dimension: a caller-made (B, 1, N) transposed output of a one-channel conv -- (B, N, 1).transpose(1, 2).contiguous() --
has stride(1) = 1, and every utterance but the first was written to the wrong place.  test_tiled_integer[P1-f32-k3-C40-O1] met it
(its own stride assertion stopped it before the launch); ops.row_stride now takes the stride of a single row from the batch stride,
and test_a_one_row_output_takes_its_row_stride_from_the_batch keeps the call.

Built to fail, in scratch builds that are not committed.  Every mutation reads or writes fewer rows or swaps two in-range indices;
each ran once.  Failures of this file's 165 tests | of the older tests in test_gpu_conv.py and test_gpu_kernels.py (the child process
of the tall tiles stops at its first failing case and counts as one test):
  * tiled main loop, `ci < Cin` of the activation fetch tightened by one 8-chunk (`ci + 8 < Cin`) -- 117: all 90
    test_tiled_integer (every Cin loses its last 8 channels), all 24 tiled test_rounded, the child process, the gate-refusal test's passing
    launch and the one-row test | 40: the kernel header also serves the LayerNorm GEMMs (27 of test_gpu_conv.py, 13 of test_gpu_kernels.py);
  * tiled main loop, the `wm` / `i` row terms of the 256-row mapping swapped (MI = 4 only) -- 1, the child process (P4-bf16-O256 first:
    72494 of 230400 elements); P4n passes, as it must: its N = 3 rows sit in block wm = 0, i = 0, which the swap leaves alone | 1
    (test_conv_tall_tiles);
  * tiled vector epilogue, gate `> 0.f` -> `>= 0.f` -- 15: 12 test_tiled_integer with a gate on the vector path, two test_rounded,
    the child process | 0: no older test draws a gate that holds zeros;
  * tiled vector epilogue, `n >= len` -> `n > len` -- 26: 13 test_tiled_integer, 12 test_rounded (the 128-row cases, all masked), the
    child process | 2 (test_conv_epilogues, test_conv_tall_tiles);
  * tiled scalar epilogue, `n >= len` -> `n > len` -- 12: 11 masked test_tiled_integer on the scalar path, the child process | 1
    (test_conv_epilogues);
  * ACCUMULATE dead tile, `if (accum) return;` removed -- 10: the nine test_tiled_integer that accumulate under skip_lengths (P1, P2, P3
    and the three P5 ones) and the child process | 0.  The first run of this mutant passed EVERY test: the oracle's draw zeroed the old
    output on the dead rows, as it does the inputs, so "untouched" and "zero-filled" were the same bits.  The old output now keeps
    its integers there (tests/test_conv_plain_host.py asserts that they are not all zero) -- a gap of the test, found by its mutant;
  * tiled dead-tile zero fill, first row of each dead tile skipped -- 20: 7 test_tiled_integer, 12 test_rounded, the child process | 6;
  * conv_wreg_kernel, `+ 2` -> `+ 1` in `live_g` -- 3, all R4 (len 255: row 256 starts a tile that lives by the second halo row only) | 1;
  * conv_wreg_kernel, `zero_row = n >= e.len` -> `n > e.len` -- 16 test_wreg_integer (the masked ones) | 10;
  * conv_wreg_kernel, dead-tile zero fill without the first row of each tile -- 16: 12 test_wreg_integer, the 4 wreg test_rounded | 6;
  * conv_wide_kernel, two bias channel blocks swapped (`c ^ 1`) -- 8: the six test_wide_integer that pass a bias, both wide test_rounded | 3;
  * conv_wide_kernel, the last row of every tile not stored (`r0 + row + 1 < h`) -- 18: all 16 test_wide_integer, both test_rounded | 1;
  * conv_wide_kernel, the padding fill stopped after its first 64 utterances -- 4: the four W3 cases, nothing else | 0: no older
    test has more than 6 utterances on this kernel.  The outputs ops allocates start as NaN here (config.POISON); on recycled memory
    this mutant could have passed.
No mutation went uncaught by the new tests in the end; three (the gate's zeros, the ACCUMULATE dead tile, the second fill block) pass
every older test.
"""
import os
import subprocess
import sys

import pytest
import torch

from tests import conv_ln_oracle as K
from tests import conv_plain_oracle as P

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
F32, BF16 = torch.float32, torch.bfloat16
NAN = float('nan')


def _place(t, pad, dev=DEV):
    ''' t on the device -- with pad > 0 as the slice [PAD_LEFT, PAD_LEFT + W) of the last dimension of a NaN container of width W + pad.
        Returns (tensor, container or None) '''
    if not pad:
        return t.to(dev).contiguous(), None
    W = t.shape[-1]
    wide = torch.full(tuple(t.shape[:-1]) + (W + pad,), NAN, dtype=t.dtype)
    wide[..., P.PAD_LEFT:P.PAD_LEFT + W] = t
    wide = wide.to(dev)
    return wide[..., P.PAD_LEFT:P.PAD_LEFT + W], wide


def _around_is_nan(wide, W):
    return bool(torch.isnan(wide[..., :P.PAD_LEFT]).all()) and bool(torch.isnan(wide[..., P.PAD_LEFT + W:]).all())


def _layout(t, c):
    ''' (B, N, Cout) -> the output's layout '''
    return t.transpose(1, 2).contiguous() if c.trans else t


def launch(m):
    ''' one ops.conv1d call of the case under config.POISON, so that every buffer ops allocates -- the output where the case has no old
        value and no row stride of its own, always that of the wide kernel and of relu_bits, and the bit words -- starts as NaN (integers:
        a large negative number), like the outputs this file allocates itself: a row the kernel skips cannot pass for a zero row.
        Returns (y as (B, N, Cout) on the CPU in its stored type, bits or None) '''
    from daft_exprt import config
    old = config.POISON
    config.POISON = True
    try:
        return _launch(m)
    finally:
        config.POISON = old


def _launch(m):
    from daft_exprt import ops
    c = m.c
    x, xw = _place(m.x, c.xpad)
    wp = ops.pack_conv_weight(m.w.to(DEV), m.w_dt)
    assert tuple(wp.shape) == (c.taps, c.Cout, c.Cin)
    bias = None if m.bias is None else m.bias.to(DEV)
    lens = m.L.to(DEV)
    mask = None if m.mask_lens is None else torch.tensor(m.mask_lens, dtype=torch.int64, device=DEV)
    kw = dict(out_dtype=m.y_dt, relu=c.relu, mask_lengths=mask, skip_lengths=lens if c.skip else None)
    if c.path == P.WIDE:
        assert ops.wide_shape_ok(c.Cin, c.Cout)
        plan = ops.conv_tile_plan(lens, c.N, halo=2, round_to=64, tiles=c.tiles)
        T = P.wide_plan_tiles(c)
        assert plan[0].shape[0] == T and plan[0].cpu().tolist() == [list(e) for e in K.tile_plan(m.lens, c.N, T, halo=2)], 'the plan is not the restated one'
        y = ops.conv1d(x, wp, bias, w_frag=ops.pack_frag_major(wp), wide_plan=plan, **kw)
        assert y.dtype == BF16 and tuple(y.shape) == (c.B, c.N, c.Cout)
        assert xw is None or _around_is_nan(xw, c.Cin)
        return y.cpu(), None
    out = ow = None
    if c.accum or c.ypad:
        init = _layout(m.old if c.accum else torch.full((c.B, c.N, c.Cout), NAN, dtype=m.y_dt), c)
        out, ow = _place(init, c.ypad)
    gate = gw = None
    if c.bits == 'in':
        gate = P.pack_bits(torch.nan_to_num(m.gate.float()) > 0).to(DEV)
    elif m.gate is not None:
        gate, gw = _place(_layout(m.gate, c), c.ypad if out is not None else 0)
    frag = ops.pack_frag_major(wp) if c.frag else None
    ldy = ops.row_stride(out) if out is not None else (c.N if c.trans else c.Cout)
    assert ldy == P.ldy_of(c) and x.stride(1) == P.ldx_of(c)
    assert ops.plain_path(m.x_dt, m.w_dt, m.y_dt, c.taps, c.Cin, c.Cout, c.B, c.N, ldx=x.stride(1), ldy=ldy, transposed_out=c.trans,
                          accumulate=c.accum, relu=c.relu) == c.path, 'the case does not land on the path it is named for'
    if c.bits:
        assert ops.relu_bits_ok(x, wp, m.y_dt) and out is None
    y = ops.conv1d(x, wp, bias, relu_gate=gate, transposed_out=c.trans, out=out, accumulate=c.accum, w_frag=frag, relu_bits=c.bits == 'out', **kw)
    bits = None
    if c.bits == 'out':
        y, bits = y
        bits = bits.cpu()
    torch.cuda.synchronize()
    assert y.dtype == m.y_dt and (out is None or y.data_ptr() == out.data_ptr())
    for wide, W in ((xw, c.Cin), (ow, c.N if c.trans else c.Cout), (gw, c.N if c.trans else c.Cout)):
        assert wide is None or _around_is_nan(wide, W), 'a launch wrote (or the test broke) the NaN around a slice'
    y = y.cpu()
    return (y.transpose(1, 2) if c.trans else y), bits


def check_integer(name):
    ''' both draws of an integer case: torch.equal on the contract rows, exact zeros on the zero rows, a second launch bit-equal '''
    c = P.ALL[name]
    for draw in ('small', 'big'):
        m, stored = P.integer_case(name, draw)
        rows = P.contract_rows(m)
        comp = P.computed_rows(m)
        y, bits = launch(m)
        y2, bits2 = launch(m)
        got = y.float().masked_fill(~rows[:, :, None], 0.)
        want = stored.float().masked_fill(~rows[:, :, None], 0.)
        assert got.shape == want.shape
        if not torch.equal(got, want):
            bad = (got != want) | torch.isnan(got)
            idx = bad.nonzero()
            raise AssertionError(f'{name} {draw}: {int(bad.sum())} of {bad.numel()} elements differ; first (b, n, co) {idx[0].tolist()} got '
                                 f'{got[tuple(idx[0])].item()} want {want[tuple(idx[0])].item()}; rows {sorted(set(idx[:, 1].tolist()))[:8]} '
                                 f'channels {sorted(set(idx[:, 2].tolist()))[:8]}')
        if not c.accum:
            z = (rows & ~comp)
            assert not bool(got[z].any()) and not bool(torch.isnan(y.float()[z]).any()), 'rows that must be exactly zero are not'
        assert torch.equal(y.float().masked_fill(~rows[:, :, None], 0.), y2.float().masked_fill(~rows[:, :, None], 0.)), 'two launches differ'
        if c.bits == 'out':                         # the words of the computed rows, in the documented layout; dead tiles leave theirs unwritten
            wb = P.pack_bits(stored.float() > 0)
            sel = comp[:, None, :].expand_as(wb)
            assert torch.equal(bits[sel], wb[sel]) and torch.equal(bits[sel], bits2[sel]), f'{name} {draw}: relu_bits words differ from y > 0'
            assert int((wb[sel] != 0).sum()) > 0


def check_rounded(name):
    m, ref, low = P.gauss_case(name)
    c = m.c
    y, _ = launch(m)
    rows = P.contract_rows(m)
    worst, bad = 0., []
    for b in range(c.B):
        r = rows[b]
        if not bool(r.any()):
            continue
        bound = 4. * float((low[b][r] - ref[b][r]).abs().max()) + 1e-6 * float(ref[b][r].abs().max())
        err = float((y[b].double()[r] - ref[b][r]).abs().max())
        ratio = err / bound if bound > 0. else (0. if err == 0. else float('inf'))
        worst = max(worst, ratio) if ratio == ratio else float('nan')
        if not err <= bound:
            bad.append((b, err, bound))
    print(f'RATIO {P.PATH_NAME[c.path]} {c.ladder} k{c.taps} {name}: {worst:.3f}')
    if c.skip and not c.accum:
        z = (rows & ~P.computed_rows(m))
        assert not bool(y.float()[z].any()), 'rows that must be exactly zero are not'
    assert not bad, (name, bad)


def run_tall():
    ''' the body of the child process: 256-row tiles forced on small problems '''
    assert os.environ.get('DX_CONV_WIDE_MI') == '4'
    for c in P.TALL:
        check_integer(c.name)
    for c in P.ROUNDED_TALL:
        check_rounded(c.name)
    print('tall ok')


@pytest.mark.parametrize('name', [c.name for c in P.TILED])
def test_tiled_integer(name):
    check_integer(name)


@pytest.mark.parametrize('name', [c.name for c in P.WREG_CASES])
def test_wreg_integer(name):
    check_integer(name)


@pytest.mark.parametrize('name', [c.name for c in P.WIDE_CASES])
def test_wide_integer(name):
    check_integer(name)


@pytest.mark.parametrize('name', [c.name for c in P.ROUNDED])
def test_rounded(name):
    check_rounded(name)


def test_a_one_row_output_takes_its_row_stride_from_the_batch():
    ''' a caller-made transposed output of a one-channel conv, (B, N, 1).transpose(1, 2).contiguous(): torch leaves its stride(1) at 1, and
        ops.conv1d used to hand that to the kernel as the row stride -- every utterance but the first landed in the wrong place '''
    from daft_exprt import ops
    m, stored = P.integer_case('P1-f32-k3-C40-O1', 'big')
    c = m.c
    assert c.trans and c.Cout == 1 and not (c.skip or c.accum or c.gate or c.mask or c.relu or c.xpad or c.ypad)
    out = torch.full((c.B, c.N, 1), NAN).transpose(1, 2).contiguous().to(DEV)
    assert out.stride(1) != c.N and ops.row_stride(out) == c.N
    y = ops.conv1d(m.x.to(DEV), ops.pack_conv_weight(m.w.to(DEV), F32), m.bias.to(DEV), transposed_out=True, out=out)
    torch.cuda.synchronize()
    assert torch.equal(y.cpu().transpose(1, 2), stored)


def test_tall_tiles_in_a_child_process():
    ''' P4, the 256-row P5 and the rounded 256-row cases: DX_CONV_WIDE_MI is read once per process, so a fresh child runs them -- the
        same exact comparison, the path asserted there as ROWS256 '''
    code = 'from tests import test_gpu_conv_plain as t; t.run_tall()'
    env = dict(os.environ, DX_CONV_WIDE_MI='4')
    env['PYTHONPATH'] = os.pathsep.join([os.getcwd(), os.path.join(os.getcwd(), 'ubisoft-laforge-daft-exprt_amd'), env.get('PYTHONPATH', '')])
    r = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, cwd=os.getcwd(), timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and 'tall ok' in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


# ----------------------------------------------------------------------------- refusals before any launch
def _buffers():
    from daft_exprt import _hip as H
    z = lambda n, dt: torch.zeros(n, dtype=dt, device=DEV)
    return H, z


def test_dx_conv1d_refuses_before_launching():
    H, z = _buffers()
    x32, xbf, w32, wbf, y32, ybf = z(4096, F32), z(4096, BF16), z(8192, F32), z(8192, BF16), z(4096, F32), z(4096, BF16)
    L = H.lib()

    def call(x, w, y, g=None, Cin=8, ldx=8, taps=1, Cout=8):
        return L.dx_conv1d(H.ptr(x), H.dt(x), ldx, H.ptr(w), H.dt(w), None, H.ptr(y), H.dt(y), Cout, H.ptr(g), H.dt(g) if g is not None else 0,
                           None, None, 1, 4, Cin, Cout, taps, 0, H.stream())
    assert call(x32, w32, y32) == 0                                   # the same call with nothing wrong goes through
    assert call(x32, w32, y32, Cin=12, ldx=16) == -2                  # DX_ERR_SHAPE: Cin % 8
    assert call(x32, w32, y32, ldx=12) == -2                          # ldx % 8
    assert call(x32, w32, y32, taps=5) == -5                          # DX_ERR_UNSUPPORTED
    assert call(xbf, w32, y32) == -3                                  # DX_ERR_DTYPE: bf16 x in front of fp32 weights
    assert call(x32, w32, ybf) == -3                                  # fp32 weights write fp32
    assert call(xbf, wbf, ybf, g=y32) == -3                           # a gate outside the ladder
    assert call(xbf, wbf, y32, g=ybf) == -3
    assert b'dtype' in L.dx_last_error()
    torch.cuda.synchronize()


def test_dx_conv1d_wide_and_relu_bits_refuse_before_launching():
    from daft_exprt import ops
    H, z = _buffers()
    L = H.lib()
    x, wf, y = z(8 * 256, BF16), z(3 * 256 * 256, BF16), z(8 * 256, BF16)
    lens = torch.tensor([8], dtype=torch.int64, device=DEV)
    plan = ops.conv_tile_plan(lens, 8, halo=2, tiles=1)[0]

    def wide(Cin=256, Cout=256, flags=0, tiles=1):
        return L.dx_conv1d_wide(H.ptr(x), Cin, H.ptr(wf), None, H.ptr(y), Cout, H.ptr(lens), H.ptr(plan), tiles, 2, 1, 8, Cin, Cout, flags, H.stream())
    assert wide() == 0
    assert wide(Cin=128) == -5 and wide(Cout=128) == -5 and wide(flags=H.CONV_TRANSPOSED_OUT) == -5 and wide(flags=4) == -5
    assert wide(tiles=0) == -1                                        # DX_ERR_ARG: plan_tiles < B * ceil(N / 256)
    xs, wp, ys, bits = z(8 * 128, BF16), z(3 * 256 * 128, BF16), z(8 * 256, BF16), torch.zeros(8 * 8, dtype=torch.int32, device=DEV)

    def rb(bo, bi):
        return L.dx_conv1d_relu_bits(H.ptr(xs), 128, H.ptr(wp), None, None, H.ptr(ys), 256, H.ptr(bo), H.ptr(bi), None, None, 1, 8, 256, H.stream())
    assert rb(bits, None) == 0 and rb(None, bits) == 0
    assert rb(bits, bits) == -1 and rb(None, None) == -1
    torch.cuda.synchronize()


def test_a_gate_that_does_not_lie_like_the_output_is_refused():
    ''' the kernels read the gate at the output's element offset: ops.conv1d refuses a gate of another row stride, shape or type.  The
        sliced output with a contiguous gate -- the call that would gate with the wrong elements and say nothing -- is the first '''
    from daft_exprt import ops
    B, N, Cin, Cout = 2, 9, 8, 16
    x = torch.ones(B, N, Cin, device=DEV)
    wp = ops.pack_conv_weight(torch.ones(Cout, Cin, 1, device=DEV), F32)
    wide = torch.zeros(B, N, Cout + 16, device=DEV)
    out = wide[:, :, 8:8 + Cout]
    gate = torch.ones(B, N, Cout, device=DEV)
    with pytest.raises(AssertionError, match='relu_gate'):
        ops.conv1d(x, wp, None, relu_gate=gate, out=out)
    assert not bool(wide.any()), 'refused before the launch'
    gwide = torch.ones(B, N, Cout + 16, device=DEV)
    gwide[:, :, 8] = -1.
    y = ops.conv1d(x, wp, None, relu_gate=gwide[:, :, 8:8 + Cout], out=out)       # the same slice geometry goes through, and gates
    torch.cuda.synchronize()
    assert float(y[0, 0, 0]) == 0. and float(y[0, 0, 1]) == Cin
    with pytest.raises(AssertionError, match='relu_gate'):
        ops.conv1d(x, wp, None, relu_gate=gate[:, :, :8])                          # another shape
    with pytest.raises(AssertionError, match='relu_gate'):
        ops.conv1d(x, wp, None, relu_gate=gate.transpose(1, 2).contiguous())      # the transposed layout for a plain output
    with pytest.raises(AssertionError, match='relu_gate'):
        ops.conv1d(x, wp, None, relu_gate=gate, transposed_out=True)              # and the plain layout for a transposed one
    with pytest.raises(AssertionError, match='relu_gate'):
        ops.conv1d(x, wp, None, relu_gate=gate.to(BF16))                          # a bf16 gate of fp32 weights
    xb, wb = x.to(BF16), ops.pack_conv_weight(torch.ones(Cout, Cin, 1, device=DEV), BF16)
    with pytest.raises(AssertionError, match='relu_gate'):
        ops.conv1d(xb, wb, None, out_dtype=BF16, relu_gate=gate)                   # an fp32 gate of a bf16 output
    torch.cuda.synchronize()
