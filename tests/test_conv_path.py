"""CPU-side check of dx_conv1d_ln_path, the one statement of which kernel a LayerNorm-fused GEMM runs on: literal cases and the paths
the dispatch of csrc/conv_gemm.hip (launch_ln, over the kernel units conv_sk.hip / conv_gemm_ln.hip / conv_gemm_lnbwd.hip) gives them (a host-only query: no GPU here).
The same for dx_conv1d_plain_path, the kernel of dx_conv1d / dx_conv1d_wfrag (launch_taps of csrc/conv_gemm_plain.hip, the shape rule
of csrc/conv_wreg.hip): a literal case on both sides of every condition."""
import os

import pytest

from daft_exprt import _hip as H

SPLITK, PLAN_K3, PLAN_K1, ROWS128, ROWS64 = range(5)   # DX_LN_PATH_* of include/daft_exprt_hip.h
F32, BF16 = H.F32, H.BF16

CASES = [
    # x, w, taps, Cin, B, N, plan, frag, backward -> path
    # bf16, k = 3, plan + fragment-order weights, Cin 1024: split-K while B * N <= 65536 (inclusive), the plan ring above
    (BF16, BF16, 3, 1024, 48, 1000, 1, 1, 0, SPLITK),
    (BF16, BF16, 3, 1024, 64, 1024, 1, 1, 0, SPLITK),
    (BF16, BF16, 3, 1024, 48, 1000, 1, 1, 1, SPLITK),
    (BF16, BF16, 3, 256, 48, 160, 1, 1, 0, SPLITK),
    (BF16, BF16, 3, 1024, 256, 1000, 1, 1, 0, PLAN_K3),
    (BF16, BF16, 3, 1024, 65, 1024, 1, 1, 0, PLAN_K3),
    (BF16, BF16, 3, 1024, 65, 1024, 1, 1, 1, PLAN_K3),
    # Cin below 256 or not a multiple of 128: plan ring
    (BF16, BF16, 3, 128, 48, 1000, 1, 1, 0, PLAN_K3),
    (BF16, BF16, 3, 320, 48, 1000, 1, 1, 0, PLAN_K3),
    (BF16, BF16, 3, 128, 64, 1024, 1, 1, 1, PLAN_K3),
    # without the fragment-order copy: plan ring
    (BF16, BF16, 3, 1024, 48, 1000, 1, 0, 0, PLAN_K3),
    (BF16, BF16, 3, 1024, 64, 1024, 1, 0, 1, PLAN_K3),
    # without a plan, k = 3: 128-row tiles above 64000 rows, 64-row tiles up to there (a copy without a plan changes nothing)
    (BF16, BF16, 3, 1024, 256, 1000, 0, 0, 0, ROWS128),
    (BF16, BF16, 3, 1024, 64, 1001, 0, 0, 0, ROWS128),
    (BF16, BF16, 3, 1024, 64, 1000, 0, 0, 0, ROWS64),
    (BF16, BF16, 3, 1024, 48, 1000, 0, 0, 0, ROWS64),
    (BF16, BF16, 3, 1024, 48, 1000, 0, 1, 0, ROWS64),
    (BF16, BF16, 3, 1024, 256, 1000, 0, 0, 1, ROWS128),
    # fp32 operands (either or both): the same two, whatever plan / frag say
    (F32, F32, 3, 1024, 256, 1000, 1, 1, 0, ROWS128),
    (F32, F32, 3, 1024, 48, 1000, 1, 1, 0, ROWS64),
    (F32, F32, 3, 1024, 48, 1000, 0, 0, 1, ROWS64),
    (F32, BF16, 3, 1024, 256, 1000, 1, 1, 0, ROWS128),
    (F32, BF16, 3, 1024, 48, 1000, 1, 1, 1, ROWS64),
    # k = 1: forward 64-row tiles even with a plan; backward the plan ring with a plan, 64-row tiles without (never 128-row tiles)
    (BF16, BF16, 1, 384, 48, 1000, 1, 0, 0, ROWS64),
    (BF16, BF16, 1, 384, 48, 1000, 1, 1, 0, ROWS64),
    (BF16, BF16, 1, 384, 48, 1000, 1, 0, 1, PLAN_K1),
    (BF16, BF16, 1, 384, 256, 1000, 1, 1, 1, PLAN_K1),
    (BF16, BF16, 1, 128, 48, 160, 1, 0, 1, PLAN_K1),
    (BF16, BF16, 1, 384, 48, 1000, 0, 0, 1, ROWS64),
    (BF16, BF16, 1, 384, 256, 1000, 0, 0, 1, ROWS64),
    (F32, F32, 1, 384, 256, 1000, 1, 0, 1, ROWS64),
]


@pytest.mark.parametrize('case', CASES, ids=lambda c: '-'.join(str(v) for v in c[:-1]))
def test_ln_path_matches_the_dispatch(case):
    if not os.path.exists(H.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    *args, want = case
    assert H.lib().dx_conv1d_ln_path(*args) == want


# ---- dx_conv1d_plain_path: the kernel of dx_conv1d / dx_conv1d_wfrag (launch_taps of csrc/conv_gemm_plain.hip switches on it)
WREG, P64, P128, P256 = range(4)                       # DX_PLAIN_PATH_* of include/daft_exprt_hip.h
RELU, TRANS, ACC = H.CONV_RELU, H.CONV_TRANSPOSED_OUT, 4

PLAIN_CASES = [
    # x, w, y, taps, Cin, Cout, B, N, ldx, ldy, flags -> path
    # register-weights kernel: bf16 x and w, Cin 128, Cout % 256 == 0, fp32 or bf16 output, k = 1 or 3, ReLU allowed
    (BF16, BF16, BF16, 3, 128, 1024, 48, 1000, 128, 1024, 0, WREG),
    (BF16, BF16, F32, 1, 128, 256, 3, 7, 128, 256, RELU, WREG),
    (BF16, BF16, BF16, 3, 128, 256, 1, 1, 136, 264, 0, WREG),                 # strides that are multiples of 8 stay
    # ... and each of the things that turn it off; the tiled kernel then has two or more channel tiles and Cin < 512: 128-row tiles
    (BF16, BF16, BF16, 3, 128, 256, 4, 100, 128, 100, TRANS, P128),
    (BF16, BF16, BF16, 3, 128, 256, 4, 100, 128, 256, ACC, P128),
    (BF16, BF16, BF16, 3, 128, 256, 4, 100, 128, 260, 0, P128),               # ldy % 8 != 0
    (BF16, BF16, BF16, 3, 128, 256, 4, 100, 132, 256, 0, P128),               # ldx % 8 != 0 (the entry point refuses it afterwards)
    (F32, BF16, F32, 3, 128, 256, 4, 100, 128, 256, 0, P128),                 # fp32 x
    (F32, F32, F32, 3, 128, 256, 4, 100, 128, 256, 0, P128),
    (BF16, BF16, BF16, 3, 128, 384, 4, 100, 128, 384, 0, P128),               # Cout % 256 != 0
    (BF16, BF16, BF16, 3, 256, 256, 4, 100, 256, 256, 0, P128),               # Cin != 128
    (BF16, BF16, F32, 3, 128, 256, 1, 1 << 22, 128, 256, 0, P128),            # N * ldy * 4 = 2^32: past 32-bit buffer offsets
    (BF16, BF16, F32, 3, 128, 256, 1, (1 << 22) - 1, 128, 256, 0, WREG),
    # one channel tile (Cout <= 128), k = 3: 128-row tiles above 64000 rows, 64-row tiles up to there
    (BF16, BF16, BF16, 3, 1024, 128, 64, 1000, 1024, 128, 0, P64),
    (BF16, BF16, BF16, 3, 1024, 128, 64, 1001, 1024, 128, 0, P128),
    (F32, F32, F32, 3, 8, 8, 167, 385, 8, 8, 0, P128),                        # 64295 rows
    (F32, F32, F32, 3, 8, 8, 166, 385, 8, 8, 0, P64),                         # 63910 rows
    (BF16, BF16, BF16, 3, 128, 128, 1, 64000, 128, 128, 0, P64),
    (BF16, BF16, BF16, 3, 128, 128, 1, 64001, 128, 128, 0, P128),
    # k = 1: 64-row tiles with one channel tile whatever the row count, 128-row tiles with more (never 256)
    (BF16, BF16, BF16, 1, 1024, 128, 64, 1001, 1024, 128, 0, P64),
    (F32, F32, F32, 1, 384, 80, 256, 1000, 384, 80, 0, P64),
    (BF16, BF16, BF16, 1, 1024, 384, 64, 1001, 1024, 384, 0, P128),
    (BF16, BF16, BF16, 1, 1024, 1024, 256, 1000, 1024, 1024, 0, P128),
    (F32, BF16, F32, 1, 128, 129, 2, 10, 128, 129, 0, P128),                  # Cout 129: two channel tiles
    # several channel tiles, k = 3, bf16 weights: 256-row tiles from Cin 512 on and from 1024 workgroups on
    (BF16, BF16, BF16, 3, 1024, 1024, 48, 1000, 1024, 1024, 0, P256),         # 4 * 48 * 8 = 1536
    (BF16, BF16, BF16, 3, 512, 256, 512, 3, 512, 256, 0, P256),               # 1 * 512 * 2 = 1024
    (BF16, BF16, BF16, 3, 512, 256, 511, 3, 512, 256, 0, P128),               # 1022
    (BF16, BF16, BF16, 3, 512, 256, 256, 257, 512, 256, 0, P256),             # 2 * 256 * 2 = 1024
    (BF16, BF16, BF16, 3, 512, 256, 256, 256, 512, 256, 0, P128),             # 1 * 256 * 2 = 512
    (F32, BF16, F32, 3, 512, 264, 512, 3, 512, 264, 0, P256),                 # fp32 x: the weights' type decides; ceil(264 / 128) = 3
    (BF16, BF16, BF16, 3, 511, 256, 512, 3, 512, 256, 0, P128),               # Cin 511 (the query classifies, the entry point refuses Cin % 8)
    (BF16, BF16, BF16, 3, 504, 256, 512, 3, 504, 256, 0, P128),               # Cin 504: the largest multiple of 8 below 512
    (BF16, BF16, BF16, 3, 512, 1024, 3, 300, 512, 1024, TRANS | RELU, P128),  # 2 * 3 * 8 = 48 workgroups
    # fp32 weights stay on 128-row tiles at any size
    (F32, F32, F32, 3, 1024, 1024, 48, 1000, 1024, 1024, 0, P128),
    (F32, F32, F32, 3, 512, 256, 512, 3, 512, 256, 0, P128),
]


@pytest.mark.parametrize('case', PLAIN_CASES, ids=lambda c: '-'.join(str(v) for v in c[:-1]))
def test_plain_path_matches_the_dispatch(case):
    if not os.path.exists(H.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    if os.environ.get('DX_CONV_WIDE_MI'):
        pytest.fail('DX_CONV_WIDE_MI is set: it overrides the threshold these cases state')
    *args, want = case
    assert H.lib().dx_conv1d_plain_path(*args) == want


def test_plain_path_through_ops_is_the_same_answer():
    import torch
    from daft_exprt import ops
    bf, f32 = torch.bfloat16, torch.float32
    assert (ops.PLAIN_WREG, ops.PLAIN_ROWS64, ops.PLAIN_ROWS128, ops.PLAIN_ROWS256) == (WREG, P64, P128, P256)
    assert ops.plain_path(bf, bf, bf, 3, 128, 1024, 48, 1000) == WREG
    assert ops.plain_path(bf, bf, bf, 3, 128, 1024, 48, 1000, accumulate=True) == P128
    assert ops.plain_path(bf, bf, bf, 3, 128, 256, 4, 100, transposed_out=True) == P128
    assert ops.plain_path(bf, bf, bf, 3, 128, 256, 4, 100, ldy=260) == P128
    assert ops.plain_path(f32, f32, f32, 1, 80, 80, 2, 37, relu=True) == P64
    assert ops.plain_path(bf, bf, bf, 3, 512, 256, 512, 3) == P256
    assert ops.plain_path(bf, bf, bf, 3, 512, 256, 512, 3) == P256           # remembered
