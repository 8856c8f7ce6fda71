// conv_gemm_kernel with the backward LayerNorm epilogue (LNM 2 with FiLM gradients, 3 without): the dtype ladder of dx_conv1d_lnbwd.
#include <type_traits>

#include "conv_args.h"

namespace {

#include "conv_common.h"
#include "conv_gemm_kernel.h"

}  // namespace

int conv_lnbwd_launch(const ConvArgs& a, int path, int x_dtype, int w_dtype, int taps, hipStream_t s) {
  if (w_dtype == DX_BF16 && x_dtype == DX_BF16) return launch_ln_taps<bf16_t, bf16_t, 2>(a, path, taps, s);
  if (w_dtype == DX_BF16 && x_dtype == DX_F32) return launch_ln_taps<float, bf16_t, 2>(a, path, taps, s);
  if (w_dtype == DX_F32 && x_dtype == DX_F32) return launch_ln_taps<float, float, 2>(a, path, taps, s);
  dx_set_error("dx_conv1d_lnbwd: unsupported dtype combination x=%d w=%d", x_dtype, w_dtype);
  return DX_ERR_DTYPE;
}
