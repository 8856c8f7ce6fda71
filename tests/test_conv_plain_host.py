"""Holds tests/conv_plain_oracle.py to its purpose, on the CPU: the integer draws are exact (every partial sum below 2^24, fp32 and
float64 evaluation bit-equal), the 'small' draw stays within the integers bf16 represents, the operand formulas are symmetric in no
pair of indices, every case reaches the branch it is named for (the kernels' tile and group arithmetic restated in Python, the tile
height from ops.plain_path), and the rounding restatement of the Gaussian cases stays under conv_ln_oracle.CAP of the tensor's
largest element.

Measured here, max|restatement - float64| / max|float64| over the Gaussian cases of each kind (cap): fp32-stored outputs of
fp32 / fp32 and bf16 / bf16 operands 4.4e-7 (2.4e-6); fp32-stored outputs of fp32 x in front of bf16 weights 1.8e-3 (5.5e-3);
bf16-stored outputs 3.2e-3 (7.8e-3).  conv_ln_oracle.CAP holds as it is.
"""
import os

import pytest
import torch
import torch.nn.functional as F

from tests import conv_ln_oracle as K
from tests import conv_plain_oracle as P

INT_CASES = list(P.ALL)
F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope='module', autouse=True)
def _library():
    from daft_exprt import _hip as H
    if not os.path.exists(H.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()


def _abs_bound(m):
    ''' the largest sum of magnitudes any accumulation order can meet: |x| * |w| + |bias| + |old| '''
    v = K.conv(torch.nan_to_num(m.x.double()).abs(), m.w.abs())
    if m.bias is not None:
        v = v + m.bias.double().abs()
    if m.old is not None:
        v = v + torch.nan_to_num(m.old.double()).abs()
    return float(v.max())


@pytest.mark.parametrize('name', INT_CASES)
def test_integer_draws_are_exact_and_small_stays_representable(name):
    c = P.ALL[name]
    for draw in ('small', 'big'):
        m, stored = P.integer_case(name, draw)
        assert _abs_bound(m) < 2 ** 24, (name, draw, _abs_bound(m))
        ref = P.reference(m)
        assert torch.equal(ref, ref.round()) and torch.isfinite(ref).all()
        x32 = torch.nan_to_num(m.x.float())
        v32 = F.conv1d(x32.transpose(1, 2), m.w.float(), None, padding=c.taps // 2).transpose(1, 2)
        assert torch.equal(P._epilogue(m, v32, F32).double(), ref), (name, draw, 'fp32 and float64 evaluation differ')
        if draw == 'small':
            assert float(ref.abs().max()) <= 256, (name, float(ref.abs().max()))
            assert torch.equal(stored.double(), ref)                     # exactly representable in the output's type
        live = ref[P.computed_rows(m)]
        assert float(live.min()) < 0 or c.relu or c.gate or c.bits, name
        assert float(live.abs().max()) > 0
    m, _ = P.integer_case(name, 'big')
    pre = K.conv(torch.nan_to_num(m.x.double()), m.w) + (0 if m.bias is None else m.bias.double())
    rows = P.computed_rows(m)
    assert float(pre[rows].min()) < 0 < float(pre[rows].max()), 'the conv output is signed, so a ReLU acts'
    if m.gate is not None:
        gl = torch.nan_to_num(m.gate.double())[rows]
        assert bool((gl == 0).any()) and bool((gl < 0).any()) and bool((gl > 0).any())


SWAPS = [(1, 0, 2), (2, 1, 0), (0, 2, 1)]


@pytest.mark.parametrize('name', INT_CASES)
def test_operand_formulas_are_symmetric_in_no_pair_of_indices(name):
    c = P.ALL[name]
    m, _ = P.integer_case(name, 'big')
    ref = P.reference(m)
    rows = (P.computed_rows(m) & P.contract_rows(m))[:, :, None]
    for perm in SWAPS:
        x = torch.nan_to_num(P.dress(P.draw_x(c, 'big', c.B, c.N, c.Cin, perm), m.lens, c.N) if c.skip else P.draw_x(c, 'big', c.B, c.N, c.Cin, perm))
        assert not torch.equal(P.reference(m, x=x) * rows, ref * rows), (name, 'x', perm)
        if c.taps == 1 and perm != (1, 0, 2):
            continue                                                   # (one tap: the tap index is always 0, only co <-> ci is a swap)
        w = P.draw_w(c, 'big', c.Cout, c.Cin, c.taps, perm).to(m.w_dt).double()
        assert not torch.equal(P.reference(m, w=w) * rows, ref * rows), (name, 'w', perm)
    for perm in SWAPS:                                                 # the gate and the old output, where the case has them
        if m.gate is not None:
            assert not torch.equal(P.reference(P.make_case(c, 'big', gperm=perm)) * rows, ref * rows), (name, 'gate', perm)
        if m.old is not None:
            allrows = P.contract_rows(m)[:, :, None]
            assert not torch.equal(torch.nan_to_num(P.reference(P.make_case(c, 'big', operm=perm))) * allrows, torch.nan_to_num(ref) * allrows), (name, 'old', perm)


def _natural_path(c):
    from daft_exprt import ops
    x_dt, w_dt, y_dt, _ = P.LADDERS[c.ladder]
    return ops.plain_path(x_dt, w_dt, y_dt, c.taps, c.Cin, c.Cout, c.B, c.N, ldx=P.ldx_of(c), ldy=P.ldy_of(c), transposed_out=c.trans,
                          accumulate=c.accum, relu=c.relu)


@pytest.mark.parametrize('name', INT_CASES + list(P.ALL_ROUNDED))
def test_each_case_reaches_what_it_is_named_for(name):
    from daft_exprt import ops
    c = P.ALL.get(name) or P.ALL_ROUNDED[name]
    lens = P.lengths_of(c)
    assert len(lens) == c.B and max(lens) <= c.N and min(lens) >= 0
    tall = c in P.TALL or c in P.ROUNDED_TALL
    if c.path == P.WIDE:
        assert ops.wide_shape_ok(c.Cin, c.Cout) and c.Cin // 32 in (8, 12) and c.skip
        T = P.wide_plan_tiles(c)
        assert T >= c.B * P.cdiv(c.N, 256)
        if name.startswith('W3'):
            assert c.B > 64 and 0 in lens and c.N in lens and T >= 16          # the second 64-utterance block of the fill; a rotated chunk order
        if name.startswith('W4'):
            assert T == c.B * P.cdiv(c.N, 256)                                # the smallest legal plan
        if name.startswith('W2'):
            assert min(P.fill_end(torch.tensor(lens), c.N).tolist()) < c.N and 0 in lens
        return
    # the tile height is the library's answer; the forced cases report 128-row tiles on their own and are run with DX_CONV_WIDE_MI = 4
    assert not os.environ.get('DX_CONV_WIDE_MI')
    assert _natural_path(c) == (P.ROWS128 if tall else c.path), (name, _natural_path(c))
    if c.path == P.WREG:
        g = P.wreg_geometry(c, lens)
        if name.startswith('R1') or name.startswith('G-wreg'):
            assert g.ngrp == 9 and not g.zmajor and g.ptiles * c.B == 9
            assert not c.skip or g.idle_groups > 0
        if name.startswith('R2'):
            assert g.ngrp == 8 and g.zmajor
        if name.startswith('R3'):
            assert not g.scan and g.zmajor and g.max_share >= 2 and g.crossing > 0 and 0 in lens
        if name.startswith('R4'):
            assert g.dead_zero > 0 and g.dead_unwritten > 0 and g.ngrp > g.total and not g.zmajor and 0 in lens
        return
    BM = P.TILE_ROWS[c.path]
    g = P.tiled_geometry(c, lens, BM)
    assert (g.ztiles == 1) == (c.Cout <= 128)
    if name.startswith('P1'):
        assert g.ztiles == 1 and g.ptiles == 2 and g.partial_chunk == (c.Cin in (8, 40)) and g.vec_out == (c.Cout % 8 == 0 and c.ypad != 12 and not c.trans)
    if name.startswith('P2'):
        assert g.ztiles >= 2 and g.ptiles == 2 and c.Cout % 128 in (7, 8)
    if name.startswith('P3'):
        assert g.ztiles == 1 and c.B * c.N > 64000 and (c.B - 1) * c.N <= 64000 and g.partial_chunk
        x_dt, w_dt, y_dt, _ = P.LADDERS[c.ladder]
        assert ops.plain_path(x_dt, w_dt, y_dt, 3, c.Cin, c.Cout, c.B - 1, c.N, ldx=P.ldx_of(c), ldy=P.ldy_of(c), accumulate=c.accum,
                              relu=c.relu) == P.ROWS64                      # one utterance shorter: 64-row tiles
    if name.startswith('P4n'):
        assert P.cdiv(c.N, 256) * c.B * g.ztiles == 1024
    if name.startswith('P5'):
        assert sum(g.zero) > 0 and (c.trans or sum(g.unwritten) > 0) and c.skip
    if c.accum and c.skip and name.startswith('P5'):           # a dead tile below the fill end holds old integers that are not all zero
        m, _ = P.integer_case(name, 'big')
        dead = (~P.computed_rows(m)) & P.contract_rows(m)
        assert bool(dead.any()) and bool((torch.nan_to_num(m.old.float())[dead] != 0).any())
    if c.skip and not name.startswith(('P3', 'P4n', 'G-')):
        assert sum(g.zero) + sum(g.unwritten) > 0, 'skip_lengths without a dead tile'


def test_the_cases_cover_every_launchable_combination():
    ''' (path x ladder x taps) of conv_plain_launch -- fp32 weights never reach 256-row tiles, k = 1 never does -- and the kernels behind
        try_weight_stationary (output bf16 / fp32, k = 1 / 3, the four ReLU / gate forms, both bit directions) and dx_conv1d_wide '''
    have = {(c.path, c.ladder, c.taps) for c in P.ALL.values()}
    for l in P.LADDERS:
        for taps in (1, 3):
            assert (P.ROWS64, l, taps) in have and (P.ROWS128, l, taps) in have
        if l != 'f32':
            assert (P.ROWS256, l, 3) in have
    forms = {(c.ladder, c.taps, c.relu, c.gate) for c in P.WREG_CASES if not c.bits}
    for l in ('bf16', 'bf32'):
        for taps in (1, 3):
            assert {(r, g) for (ll, t, r, g) in forms if (ll, t) == (l, taps)} == {(False, False), (True, False), (False, True), (True, True)}
    assert {c.bits for c in P.WREG_CASES} == {None, 'out', 'in'} and {c.frag for c in P.WREG_CASES if c.taps == 3} == {True, False}
    assert {(c.Cin, c.Cout, c.relu, c.nobias) for c in P.WIDE_CASES} >= {(256, 256, True, True)} and len({(c.relu, c.nobias) for c in P.WIDE_CASES}) == 4
    opts = ('relu', 'gate', 'mask', 'skip', 'trans', 'accum', 'nobias')
    for path in (P.ROWS64, P.ROWS128, P.ROWS256):
        cs = [c for c in P.ALL.values() if c.path == path]
        for o in opts:
            assert any(getattr(c, o) for c in cs), (P.PATH_NAME[path], o)
        assert any(c.xpad for c in cs) and any(c.ypad == 16 for c in cs) and any(c.ypad == 12 for c in cs)
        assert any(c.Cout % 8 for c in cs) and any(c.accum and P.LADDERS[c.ladder][2] == torch.bfloat16 for c in cs)


@pytest.mark.parametrize('name', list(P.ALL_ROUNDED))
def test_the_rounding_restatement_stays_under_its_cap(name):
    m, ref, low = P.gauss_case(name)
    rows = (P.contract_rows(m))[:, :, None]
    err = float(((low - ref) * rows).abs().max())
    big = float((ref * rows).abs().max())
    kind = P.kind_of(m)
    print(f'CAP {name} {kind}: {err / big:.3e} of {P.CAP[kind]:.1e}')
    assert 0. < big and err <= P.CAP[kind] * big, (name, kind, err / big)
