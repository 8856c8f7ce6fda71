"""Host side of the weight-gradient tests (no GPU): the float64 oracle of tests/wgrad_oracle.py against float64 autograd, its
restatement of wgrad_nsplit against the library's workspace query, the purpose of every case as a condition -- a retuning of
DX_WG_TARGET or of the item size fails HERE instead of quietly emptying tests/test_gpu_wgrad.py -- and the headroom that makes the
integer comparisons exact."""
import pytest
import torch

from tests import wgrad_oracle as W

ALL = [(case, chset) for case in W.CASES for chset in W.CASE_SETS[case]]
IDS = [f'{case}-{W.set_id(chset)}' for case, chset in ALL]


@pytest.mark.parametrize('taps', [1, 3])
@pytest.mark.parametrize('lens', [None, (37, 0, 20, 35, 36)], ids=['nolens', 'lens'])
def test_oracle_equals_float64_autograd(taps, lens):
    ''' dW, db of `contract` == autograd of conv1d (zero padding) under a dY that is zero at n >= nlim_b '''
    B, N, cin, cout = 5, 37, 6, 10
    g = torch.Generator().manual_seed(3 + taps)
    x = torch.randn(B, N, cin, generator=g, dtype=torch.float64)
    dy = torch.randn(B, N, cout, generator=g, dtype=torch.float64)
    nlim = [N] * B if lens is None else [min(N, l + 2) for l in lens]
    assert lens is None or sorted(nlim) == [2, 22, 37, 37, 37]
    w = torch.randn(cout, cin, taps, generator=g, dtype=torch.float64).requires_grad_(True)
    b = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.conv1d(x.transpose(1, 2), w, b, padding=taps // 2).transpose(1, 2)
    mask = torch.arange(N)[None, :, None] < torch.tensor(nlim)[:, None, None]
    (y * dy * mask).sum().backward()
    dw, db, A, Ab, R = W.contract(dy, x, nlim, taps, with_abs=True)
    assert R == sum(nlim)
    assert float((dw - w.grad).abs().max()) <= 1e-12 * float(A.max()) and float((db - b.grad).abs().max()) <= 1e-12 * float(Ab.max())
    assert bool((A >= dw.abs()).all()) and bool((Ab >= db.abs()).all())
    # the rows past nlim are not touched: NaN there changes nothing
    dyp, xp = dy.clone(), x.clone()
    for i, nl in enumerate(nlim):
        dyp[i, nl:] = float('nan')
        xp[i, nl + 1:] = float('nan')
    dwp, dbp, _, _, _ = W.contract(dyp, xp, nlim, taps)
    assert torch.equal(dwp, dw) and torch.equal(dbp, db)


@pytest.mark.parametrize('case,chset', ALL, ids=IDS)
def test_nsplit_restated_equals_the_workspace_query(case, chset):
    from daft_exprt import _hip as H
    B, N, _ = W.CASES[case]
    cin, cout, taps = chset
    floats = H.lib().dx_conv1d_wgrad_ws_floats(B, N, cin, cout, taps)
    per_split = W.tiles(cin, cout) * taps * W.TILE_FLOATS_PER_TAP
    assert floats % per_split == 0
    assert W.nsplit(B, N, cin, cout, taps) == floats // per_split == W.expected_nsplit(case, chset)


def test_every_set_meets_w2_and_w4():
    assert set(W.SETS + W.RAGGED) <= set(W.CASE_SETS['W2']) and set(W.SETS) <= set(W.CASE_SETS['W4'])
    for case in ('W1', 'W2', 'W3'):
        assert set(W.RAGGED) <= set(W.CASE_SETS[case])
    for cin, cout, _ in W.RAGGED:
        assert cin % 8 == 0 and cout % 8 == 0 and (cin % 128 or cout % 128)
    assert all(len(lens) == B for B, _, lens in W.CASES.values() if lens is not None)


def test_each_case_reaches_what_it_is_for():
    ns = lambda case, chset: W.nsplit(W.CASES[case][0], W.CASES[case][1], *chset)
    # W1: one split; the four kinds of utterance end
    assert W.nlims('W1') == [130, 64, 65, 2] and 130 % 64 and [b for b, _ in W.items('W1')] == [0, 0, 0, 1, 2, 2, 3]
    assert W.xlims('W1') == [129, 64, 65, 2]
    # W2: two splits; the second starts inside utterance 0, at row 576, and crosses two utterance ends
    assert len(W.items('W2')) == 19 and W.split_items('W2', 2, 1)[0] == (0, 576)
    assert sorted({b for b, _ in W.split_items('W2', 2, 1)}) == [0, 1, 2] and {b for b, _ in W.split_items('W2', 2, 0)} == {0}
    # W3: uneven shares of the reduce kernels' four groups
    assert all(ns('W3', c) == 6 for c in W.CASE_SETS['W3']) and W.reduce_shares(6) == [2, 2, 2, 0]
    assert W.reduce_shares(2) == [1, 1, 0, 0] and W.reduce_shares(8) == [2, 2, 2, 2] and W.reduce_shares(32) == [8, 8, 8, 8]
    # W4: the split-fastest mapping with 2, 3 and 8 tiles, index order with 1
    lens4 = W.CASES['W4'][2]
    assert lens4[0] == 512 and lens4.count(0) == 1 and len(set(lens4)) > 8
    seen = {W.tiles(c[0], c[1]): W.by_split(ns('W4', c), W.tiles(c[0], c[1]), ring) for c in W.CASE_SETS['W4'] for ring in (False, True)}
    assert seen == {1: False, 2: True, 3: True, 8: True}
    # W5: more splits than items
    assert max(W.CASES['W5'][2]) <= 62 and len(W.items('W5')) == 8 and all(ns('W5', c) == 16 for c in W.CASE_SETS['W5'])
    assert sum(1 for s in range(16) if not W.split_items('W5', 16, s)) == 8
    # W6: the serial walk, with the split-fastest mapping
    B6, N6, lens6 = W.CASES['W6']
    assert B6 > W.SCAN_MAXB and len(W.items('W6')) == B6 and {0, 8} <= set(lens6) and set(W.nlims('W6')) == set(range(2, 9))
    assert all(ns('W6', c) == 32 for c in W.CASE_SETS['W6']) and W.by_split(32, W.tiles(128, 256), True) and W.by_split(32, W.tiles(128, 256), False)
    # W7: the 64-tile weight: tile permutation of the ring kernel, index order in both kernels
    assert W.tiles(1024, 1024) == 64 and ns('W7', (1024, 1024, 3)) == 2 and ns('W7', (1024, 1024, 1)) == 1
    assert not W.by_split(8, 64, True) and W.by_split(8, 64, False)
    assert len(W.items('W7')) == 8 + 2 + 1 + 1
    # W8: one row, no lengths
    assert W.CASES['W8'] == (7, 1, None) and W.nlims('W8') == [1] * 7 and W.xlims('W8') == [0] * 7
    # every k = 3 ring item of >= 64 contracted rows with a live row behind it reads the dword behind position 63
    assert any(n0 + 64 < W.nlims(case)[b] for case in ('W1', 'W2', 'W3', 'W4', 'W7') for b, n0 in W.items(case))


@pytest.mark.parametrize('case,chset', ALL, ids=IDS)
def test_exactness_headroom(case, chset):
    ''' every partial sum of an integer draw is an integer of magnitude <= A (+ 100 from the initial dW): below 2^24, exact in fp32 '''
    for draw in W.EXACT_DRAWS:
        p = W.problem(case, chset, draw, W.F32, True)
        assert float(p.A.max()) + 100 < 2 ** 24 and float(p.Ab.max()) + 100 < 2 ** 24, (draw, float(p.A.max()), float(p.Ab.max()))
        assert p.R == sum(p.nlim) and 127 * 3 * p.R + 100 < 2 ** 24          # (the same, without looking at the draw)
        for t, lim in ((p.dy, 127 if draw == 'dy8' else 3), (p.x, 3 if draw == 'dy8' else 127)):
            v = t[torch.isfinite(t)]
            assert float(v.abs().max()) == lim and bool((v == v.round()).all()) and torch.equal(v.to(torch.bfloat16).float(), v)
        assert bool(torch.isfinite(p.dy).all()) == (p.lens is None)
        for b in range(p.B):          # the poison stands where the contract says, and X row nlim_b is finite
            assert bool(torch.isfinite(p.dy[b, :p.nlim[b]]).all()) and bool(torch.isnan(p.dy[b, p.nlim[b]:]).all())
            xl = W.xlims(case)[b]
            assert bool(torch.isfinite(p.x[b, :xl + 1]).all()) and bool(torch.isnan(p.x[b, xl + 1:]).all()) and xl >= min(p.nlim[b], p.N - 1)
