// What the conv GEMM units (conv_gemm*.hip, conv_wreg.hip, conv_sk.hip, conv_wide.hip, conv_plan.hip) share on the host side: the kernel
// argument block, the tile and plan constants, and the host launchers the kernel units export to each other and to the entry points in
// conv_gemm.hip.  Everything else in a unit belongs to that unit's kernel alone.  (Shared device helpers: conv_common.h.)
#pragma once
#include "dx_common.h"

constexpr int BN = 128, NTHREADS = 256;   // output channels of a conv_gemm / conv_sk tile; threads of a four-wave MFMA team

// balanced position tiles (conv_plan.hip): at most DX_PLAN_ROWS rows each, a multiple of DX_NUM_CU of them
constexpr int DX_PLAN_ROWS = 256, DX_NUM_CU = 256;

// LayerNorm epilogue (Cout == 128: a tile holds complete rows): s = dropout(conv) + residual; y = LN(s) [* FiLM] [masked]
// (LN template parameter of conv_gemm_kernel: 0 none, 1 forward LayerNorm, 2 backward LayerNorm)
// Backward (dx_conv1d_lnbwd, the data-gradient GEMM that completes dL/dy of a LayerNorm carries that LayerNorm's
// backward): y = residual gradient in / ds out (in place), y_lp = bf16 dx_pre out, s_out = the saved LayerNorm
// input (read), mean / rstd read, dgamma / dbeta / dfilm accumulated with one atomic per channel per workgroup.
struct LNEpi {
  const float* gamma; const float* beta; const float* residual; const float* film; long ldf;
  float* y; void* y_lp; float* s_out; float* mean; float* rstd;
  float p_pre; uint64_t seed_pre;
  int enabled;
  float* dgamma; float* dbeta; float* dfilm; long lddf;
  const void* w2; void* y2;   // split-K kernel: y2 = y_lp . w2^T (+ b2), a 128 -> n2 k = 1 GEMM on the rows the epilogue has just produced
  const float* b2; int n2;    // (n2 = 128: output-projection data gradient behind the LayerNorm backward; 384: the next block's QKV projection)
  const DxStepScalars* step;  // NULL, or the device-side step block whose salt is added to seed_pre (captured steps)
  // "virtual" residual (split-K forward kernel, dx_conv1d_ln_vres): `residual` is the saved INPUT s of the LayerNorm that produced the
  // residual stream, and the epilogue re-applies that LayerNorm (+ mask) -- its fp32 output then never has to be stored (y = NULL there)
  const float* res_mean; const float* res_rstd; const float* res_gamma; const float* res_beta;
};

struct ConvArgs {
  const void* x; long ldx;
  const void* w; const float* bias;
  void* y; long ldy;
  const void* gate;
  const int64_t* mask_len;
  const int64_t* skip_len;
  int N, Cin, Cout, flags, B;          // flags: DX_CONV_* (public header) in the low byte; conv_wide_kernel: its plan's halo in flags >> 8
  LNEpi ln;
  const int* plan; int plan_tiles;     // balanced position tiles {b, n0, rows, 0} (dx_conv_tile_plan), ring kernels only
  const void* w_frag;                  // the same weights in MFMA-fragment order (dx_pack_frag_major): split-K kernel, or NULL
  uint32_t* relu_bits;                 // conv_wreg_kernel<BITS>: sign bits of the ReLU output, (B, Cout / 32, N) words -- written (RELU) ...
  const uint32_t* gate_bits;           // ... or read as the gate of the data gradient (GATE) instead of the activation itself
};

// ---- host launchers, one kernel unit each; hidden: they are no part of the library's interface
#define DX_HIDDEN __attribute__((visibility("hidden")))
// conv_gemm_plain.hip: conv_gemm_kernel without LayerNorm, every dtype combination of dx_conv1d (DX_ERR_DTYPE otherwise)
// (gd: the gate's dtype, or y_dtype when there is none) on the path dx_conv1d_plain_path names, and the 64- / 128-row tile rule of
// the narrow k = 3 GEMMs (1 / 2), which dx_conv1d_ln_path shares
DX_HIDDEN int conv_plain_launch(const ConvArgs& a, int x_dtype, int w_dtype, int y_dtype, int gd, int taps, hipStream_t s);
DX_HIDDEN int conv_narrow_mi(int B, int N);
// conv_gemm_ln.hip / conv_gemm_lnbwd.hip: conv_gemm_kernel with the forward / backward LayerNorm epilogue on `path`, any value of
// dx_conv1d_ln_path but DX_LN_PATH_SPLITK
DX_HIDDEN int conv_ln_launch(const ConvArgs& a, int path, int x_dtype, int w_dtype, int taps, hipStream_t s);
DX_HIDDEN int conv_lnbwd_launch(const ConvArgs& a, int path, int x_dtype, int w_dtype, int taps, hipStream_t s);
// conv_wreg.hip: bf16 operands, fp32 or bf16 output (and gate); false = shape not taken, nothing launched
DX_HIDDEN bool conv_wreg_try(const ConvArgs& a, bool bf16_out, int taps, hipStream_t s);
// ... and the shape / option rule of that kernel alone (bf16 x and w understood): host-only, what dx_conv1d_plain_path asks
DX_HIDDEN bool conv_wreg_takes(int Cin, int Cout, int N, long ldx, long ldy, int flags);
// conv_sk.hip: DX_LN_PATH_SPLITK, forward or backward by a.ln.enabled
DX_HIDDEN int conv_sk_launch(const ConvArgs& a, hipStream_t s);
// conv_wide.hip
DX_HIDDEN int conv_wide_launch(const ConvArgs& a, hipStream_t s);
