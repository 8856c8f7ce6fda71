// conv_gemm_kernel without a LayerNorm epilogue (LNM 0): the kernel choice of dx_conv1d / dx_conv1d_wfrag (dx_conv1d_plain_path) and
// its dtype ladder.
#include <stdlib.h>

#include <type_traits>

#include "conv_args.h"

namespace {

#include "conv_common.h"
#include "conv_gemm_kernel.h"

template <typename T> constexpr int dtype_of() { return sizeof(T) == 2 ? DX_BF16 : DX_F32; }

template <typename TA, typename TC, typename TO, typename TG>
int launch_taps(const ConvArgs& a, int taps, hipStream_t s) {
  const int path = dx_conv1d_plain_path(dtype_of<TA>(), dtype_of<TC>(), dtype_of<TO>(), taps, a.Cin, a.Cout, a.B, a.N, a.ldx, a.ldy, a.flags);
  if (path == DX_PLAIN_PATH_WREG) {   // weights in registers (conv_wreg.hip)
    if (!conv_wreg_try(a, sizeof(TO) == 2, taps, s)) {
      dx_set_error("dx_conv1d: the register-weights kernel refused a shape dx_conv1d_plain_path gave it");
      return DX_ERR_UNSUPPORTED;
    }
    DX_LAUNCH_CHECK();
    return DX_OK;
  }
  const int mi = path == DX_PLAIN_PATH_ROWS256 ? 4 : (path == DX_PLAIN_PATH_ROWS128 ? 2 : 1);
  const long ptiles = (long)dx_cdiv(a.N, 64 * mi) * a.B;
  dim3 grid((unsigned)(((ptiles + 7) / 8) * 8 * dx_cdiv(a.Cout, BN))), block(NTHREADS);
  if constexpr (sizeof(TC) == 2) {
    if (mi == 4) {
      // (the loader-wave ring at this tile shape measured 918 vs 942 TFLOP/s: the activation stream comes from HBM / Infinity
      // Cache at ~10 B/clk/CU, the pipeline is not the limit)
      hipLaunchKernelGGL((conv_gemm_kernel<TA, TC, TO, TG, 3, 4, 32>), grid, block, 0, s, a);
      DX_LAUNCH_CHECK();
      return DX_OK;
    }
  }
  if (taps == 1 && mi == 1) hipLaunchKernelGGL((conv_gemm_kernel<TA, TC, TO, TG, 1, 1, 32>), grid, block, 0, s, a);
  else if (taps == 1) hipLaunchKernelGGL((conv_gemm_kernel<TA, TC, TO, TG, 1, 2, 32>), grid, block, 0, s, a);
  else if (mi == 1) hipLaunchKernelGGL((conv_gemm_kernel<TA, TC, TO, TG, 3, 1, 32>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((conv_gemm_kernel<TA, TC, TO, TG, 3, 2, 32>), grid, block, 0, s, a);
  DX_LAUNCH_CHECK();
  return DX_OK;
}

}  // namespace

// Narrow-output GEMMs (Cout <= 128, k = 3): 128-row tiles stage the weight chunk once per 128 rows (the LDS write of the
// weight tile is the busiest part of the kernel: 818 vs 609 TFLOP/s on a dense B = 256 problem) but need enough tiles to
// fill the chip; 64-row tiles otherwise.  Measured in the training step: B = 48 equal, B = 128 +2 % for 128 rows.
int conv_narrow_mi(int B, int N) { return (long)B * N > 64000 ? 2 : 1; }

// Which kernel dx_conv1d / dx_conv1d_wfrag runs a GEMM on (public header): launch_taps switches on it and the host side asks it.
// Every condition of that choice is written here (and in conv_wreg_takes, the shape rule of the register-weights kernel) and nowhere else.
extern "C" int dx_conv1d_plain_path(int x_dtype, int w_dtype, int y_dtype, int taps, int Cin, int Cout, int B, int N, long ldx, long ldy,
                                    int flags) {
  (void)y_dtype;   // the register-weights kernel writes fp32 or bf16, the tiled kernel any output of its ladder: no rule reads it today
  if (x_dtype == DX_BF16 && w_dtype == DX_BF16 && conv_wreg_takes(Cin, Cout, N, ldx, ldy, flags)) return DX_PLAIN_PATH_WREG;
  const int ztiles = dx_cdiv(Cout, BN);
  if (ztiles == 1) return taps == 3 && conv_narrow_mi(B, N) == 2 ? DX_PLAIN_PATH_ROWS128 : DX_PLAIN_PATH_ROWS64;
  if (!(taps == 3 && Cin >= 512 && w_dtype == DX_BF16)) return DX_PLAIN_PATH_ROWS128;
  // Wide k = 3 GEMMs with a long contraction (prenet 1024 -> 1024): 256-row tiles (MI = 4, a wave owns 128 x 64) when
  // that still leaves >= 4 workgroups per CU.  The kernel is bound by what a CU can fetch from L2 (~30 B/clk),
  // and a taller tile re-uses the taps x 128-channel weight chunk for twice the positions: 930 vs 810 TFLOP/s.
  // DX_CONV_WIDE_MI (read once) overrides the threshold: 4 = 256-row tiles, 1 = 64-row tiles, anything else = 128-row tiles.
  static const int forced_wide = getenv("DX_CONV_WIDE_MI") ? atoi(getenv("DX_CONV_WIDE_MI")) : 0;
  if (forced_wide) return forced_wide == 4 ? DX_PLAIN_PATH_ROWS256 : (forced_wide == 1 ? DX_PLAIN_PATH_ROWS64 : DX_PLAIN_PATH_ROWS128);
  return (long)dx_cdiv(N, 256) * B * ztiles >= 1024 ? DX_PLAIN_PATH_ROWS256 : DX_PLAIN_PATH_ROWS128;
}

int conv_plain_launch(const ConvArgs& a, int x_dtype, int w_dtype, int y_dtype, int gd, int taps, hipStream_t s) {
  if (w_dtype == DX_BF16) {
    if (x_dtype == DX_F32 && y_dtype == DX_F32 && gd == DX_F32) return launch_taps<float, bf16_t, float, float>(a, taps, s);
    if (x_dtype == DX_F32 && y_dtype == DX_F32 && gd == DX_BF16) return launch_taps<float, bf16_t, float, bf16_t>(a, taps, s);
    if (x_dtype == DX_F32 && y_dtype == DX_BF16 && gd == DX_BF16) return launch_taps<float, bf16_t, bf16_t, bf16_t>(a, taps, s);
    if (x_dtype == DX_BF16 && y_dtype == DX_F32 && gd == DX_F32) return launch_taps<bf16_t, bf16_t, float, float>(a, taps, s);
    if (x_dtype == DX_BF16 && y_dtype == DX_BF16 && gd == DX_BF16) return launch_taps<bf16_t, bf16_t, bf16_t, bf16_t>(a, taps, s);
  } else if (w_dtype == DX_F32) {
    if (x_dtype == DX_F32 && y_dtype == DX_F32 && gd == DX_F32) return launch_taps<float, float, float, float>(a, taps, s);
  }
  dx_set_error("dx_conv1d: unsupported dtype combination x=%d w=%d y=%d gate=%d", x_dtype, w_dtype, y_dtype, gd);
  return DX_ERR_DTYPE;
}
