"""CPU-side check of dx_conv1d_ln_path, the one statement of which kernel a LayerNorm-fused GEMM runs on: literal cases and the paths
the dispatch of csrc/conv_gemm.hip (launch_ln, over the kernel units conv_sk.hip / conv_gemm_ln.hip / conv_gemm_lnbwd.hip) gives them (a host-only query: no GPU here)."""
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
