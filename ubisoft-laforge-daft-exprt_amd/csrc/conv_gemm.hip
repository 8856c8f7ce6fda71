// K1 / K3 / K12 -- k-tap conv on channel-last activations as an implicit GEMM on MFMA (gfx950).
//
//   Y[b, n, co] = bias[co] + sum_{tap, ci} X[b, n + tap - taps/2, ci] * W[tap][co][ci]
//
// This file: the C entry points -- argument checks, the kernel argument block (ConvArgs, conv_args.h) -- and the choice of the
// LayerNorm path (dx_conv1d_ln_path).  The kernels live in one unit per family, each behind one or two host launchers (conv_args.h):
//   conv_gemm_kernel.h    conv_gemm_kernel: 64 / 128 / 256-row x 128-channel tiles, register-staged pipeline or LDS-DMA ring with loader
//                         waves; instantiated by conv_gemm_plain.hip (no LayerNorm; the kernel choice of dx_conv1d), conv_gemm_ln.hip
//                         (forward LayerNorm epilogue) and conv_gemm_lnbwd.hip (backward LayerNorm epilogue)
//   conv_wreg.hip         conv_wreg_kernel: weights in registers, K <= 384
//   conv_sk.hip           conv_sk_kernel: split-K inside the workgroup + LayerNorm epilogues
//   conv_wide.hip         conv_wide_kernel: 256 x 256 tiles
//   conv_plan.hip         the balanced position tiles: dx_conv_tile_plan, dx_batch_prep
// The weight gradients live in conv_wgrad.hip, the weight packers in conv_pack.hip, shared device helpers in conv_common.h.
#include "conv_args.h"

namespace {
#include "conv_common.h"   // DX_ZERO_PAGE_EL
}  // namespace

// Which kernel a LayerNorm-fused GEMM (Cout = 128) runs on: launch_ln switches on it, the res_mean / y2 checks of the entry points
// and the Python host side ask it (public header).  Every condition of that choice is written here and nowhere else.
extern "C" int dx_conv1d_ln_path(int x_dtype, int w_dtype, int taps, int Cin, int B, int N, int has_plan, int has_frag, int backward) {
  if (has_plan && x_dtype == DX_BF16 && w_dtype == DX_BF16) {   // balanced tiles (dx_conv_tile_plan) + padding-fill workgroups
    // split-K workgroups, weights in fragment order -- while the batch is ONE round of tiles (B * N <= 256 CUs x 256 rows): measured
    // 0.35 % of the B = 48 step faster than the ring kernel (frame level 46 vs 50 us, phoneme level 27 vs 33 us), 2.5 % of the B = 256
    // step slower (several rounds of 256-row tiles: the ring kernel's two epilogue teams win there).  Its main loop splits the
    // contraction 4 (or 2 x 2 channel groups) ways in steps of 32 channels: whole 128-channel rounds, at least two of them.
    if (taps == 3) return has_frag && Cin >= 256 && Cin % 128 == 0 && (long)B * N <= 256L * 256 ? DX_LN_PATH_SPLITK : DX_LN_PATH_PLAN_K3;
    if (taps == 1 && backward) return DX_LN_PATH_PLAN_K1;   // k = 1 data gradient + LayerNorm backward (QKV projection, K = 384)
  }
  return taps == 3 && conv_narrow_mi(B, N) == 2 ? DX_LN_PATH_ROWS128 : DX_LN_PATH_ROWS64;
}
// a.ln.enabled: 1 forward, 2 backward.  (An operand-type pair no kernel takes is never a plan path: its unit's ladder reports it.)
static int launch_ln(const ConvArgs& a, int x_dtype, int w_dtype, int taps, hipStream_t s) {
  const bool backward = a.ln.enabled == 2;
  const int path = dx_conv1d_ln_path(x_dtype, w_dtype, taps, a.Cin, a.B, a.N, a.plan != nullptr, a.w_frag != nullptr, backward);
  if (path == DX_LN_PATH_SPLITK) return conv_sk_launch(a, s);
  return backward ? conv_lnbwd_launch(a, path, x_dtype, w_dtype, taps, s) : conv_ln_launch(a, path, x_dtype, w_dtype, taps, s);
}
#define DX_SPLITK_ONLY "the split-K path (dx_conv1d_ln_path: bf16, taps = 3, plan + fragment-order weights, Cin %% 128 == 0, B * N <= 65536)"

static int conv1d_impl(const void* x, int x_dtype, long ldx, const void* w_packed, int w_dtype, const float* bias,
                       void* y, int y_dtype, long ldy, const void* relu_gate, int gate_dtype,
                       const int64_t* mask_lengths, const int64_t* skip_lengths, int B, int N, int Cin, int Cout,
                       int taps, int flags, const void* w_frag, void* stream) {
  DX_REQUIRE(x && w_packed && y, DX_ERR_ARG, "dx_conv1d: null pointer");
  DX_REQUIRE(B > 0 && N > 0 && Cin > 0 && Cout > 0, DX_ERR_SHAPE, "dx_conv1d: empty shape B=%d N=%d Cin=%d Cout=%d", B, N, Cin, Cout);
  DX_REQUIRE(Cin % 8 == 0 && ldx % 8 == 0, DX_ERR_SHAPE, "dx_conv1d: Cin (%d) and ldx (%ld) must be multiples of 8", Cin, ldx);
  DX_REQUIRE(taps == 1 || taps == 3, DX_ERR_UNSUPPORTED, "dx_conv1d: taps=%d (only 1 and 3)", taps);
  ConvArgs a{x, ldx, w_packed, bias, y, ldy, relu_gate, mask_lengths, skip_lengths, N, Cin, Cout, flags, B, LNEpi{}};
  a.w_frag = w_frag;
  return conv_plain_launch(a, x_dtype, w_dtype, y_dtype, relu_gate ? gate_dtype : y_dtype, taps, (hipStream_t)stream);
}

extern "C" int dx_conv1d(const void* x, int x_dtype, long ldx, const void* w_packed, int w_dtype, const float* bias,
                         void* y, int y_dtype, long ldy, const void* relu_gate, int gate_dtype,
                         const int64_t* mask_lengths, const int64_t* skip_lengths, int B, int N, int Cin, int Cout,
                         int taps, int flags, void* stream) {
  return conv1d_impl(x, x_dtype, ldx, w_packed, w_dtype, bias, y, y_dtype, ldy, relu_gate, gate_dtype, mask_lengths, skip_lengths, B, N,
                     Cin, Cout, taps, flags, nullptr, stream);
}

extern "C" int dx_conv1d_wfrag(const void* x, int x_dtype, long ldx, const void* w_packed, int w_dtype, const void* w_frag,
                               const float* bias, void* y, int y_dtype, long ldy, const void* relu_gate, int gate_dtype,
                               const int64_t* mask_lengths, const int64_t* skip_lengths, int B, int N, int Cin, int Cout,
                               int taps, int flags, void* stream) {
  DX_REQUIRE(!w_frag || (taps == 3 && w_dtype == DX_BF16 && Cin % 32 == 0 && Cout % 32 == 0), DX_ERR_ARG,
             "dx_conv1d_wfrag: a fragment-order copy goes with bf16 weights, taps = 3, Cin %% 32 == 0 and Cout %% 32 == 0");
  return conv1d_impl(x, x_dtype, ldx, w_packed, w_dtype, bias, y, y_dtype, ldy, relu_gate, gate_dtype, mask_lengths, skip_lengths, B, N,
                     Cin, Cout, taps, flags, w_frag, stream);
}

extern "C" int dx_conv1d_relu_bits(const void* x, long ldx, const void* w_packed, const void* w_frag, const float* bias, void* y, long ldy,
                                   uint32_t* bits_out, const uint32_t* bits_in, const int64_t* mask_lengths, const int64_t* skip_lengths,
                                   int B, int N, int Cout, void* stream) {
  DX_REQUIRE(x && w_packed && y, DX_ERR_ARG, "dx_conv1d_relu_bits: null pointer");
  DX_REQUIRE((bits_out != nullptr) != (bits_in != nullptr), DX_ERR_ARG, "dx_conv1d_relu_bits: exactly one of bits_out (ReLU forward) / bits_in (gated data gradient)");
  DX_REQUIRE(B > 0 && N > 0 && Cout > 0 && Cout % 256 == 0 && ldx % 8 == 0 && ldy % 8 == 0, DX_ERR_SHAPE,
             "dx_conv1d_relu_bits: Cout %% 256 == 0 and row strides multiples of 8 (got B=%d N=%d Cout=%d ldx=%ld ldy=%ld)", B, N, Cout, ldx, ldy);
  ConvArgs a{x, ldx, w_packed, bits_out ? bias : nullptr, y, ldy, nullptr, mask_lengths, skip_lengths, N, 128, Cout, bits_out ? DX_CONV_RELU : 0, B, LNEpi{}};
  a.w_frag = w_frag;
  a.relu_bits = bits_out;
  a.gate_bits = bits_in;
  if (!conv_wreg_try(a, true, 3, (hipStream_t)stream)) {
    dx_set_error("dx_conv1d_relu_bits: shape not taken by the register-weights kernel (N * ld beyond 32-bit buffer offsets?)");
    return DX_ERR_UNSUPPORTED;
  }
  DX_LAUNCH_CHECK();
  return DX_OK;
}

// plan validity for the LayerNorm-fused GEMMs: bf16 operands, k = 3, whole 32-channel chunks
static int plan_check(const char* who, const int* plan, int plan_tiles, const int64_t* lengths, int x_dtype, int w_dtype, long ldx, int Cin,
                      int taps, int B, int N, bool lnbwd = false) {
  if (!plan) return DX_OK;
  DX_REQUIRE(lengths, DX_ERR_ARG, "%s: a tile plan needs lengths", who);
  DX_REQUIRE(x_dtype == DX_BF16 && w_dtype == DX_BF16 && (taps == 3 || (taps == 1 && lnbwd)) && Cin % 32 == 0 && Cin <= DX_ZERO_PAGE_EL && ldx % 8 == 0, DX_ERR_UNSUPPORTED,
             "%s: tile plans are for bf16 operands, taps = 3 (or 1 for the backward variant), Cin %% 32 == 0 (got x=%d w=%d taps=%d Cin=%d)", who, x_dtype, w_dtype, taps, Cin);
  // any tile count the plan kernel accepts (callers may trade tile height against tile count for small batches)
  DX_REQUIRE(plan_tiles >= B * dx_cdiv(N, DX_PLAN_ROWS), DX_ERR_ARG, "%s: plan_tiles=%d < B * ceil(N / 256) = %d", who, plan_tiles,
             B * dx_cdiv(N, DX_PLAN_ROWS));
  return DX_OK;
}

// the argument checks dx_conv1d_ln_vres and dx_conv1d_lnbwd share
static int ln_args_check(const char* who, const void* w_frag, const int* plan, long ldx, int Cin, int taps, int B, int N, float p_pre) {
  DX_REQUIRE(!w_frag || plan, DX_ERR_ARG, "%s: fragment-order weights go with a tile plan", who);
  DX_REQUIRE(B > 0 && N > 0 && Cin > 0, DX_ERR_SHAPE, "%s: empty shape", who);
  DX_REQUIRE(Cin % 8 == 0 && ldx % 8 == 0, DX_ERR_SHAPE, "%s: Cin (%d) and ldx (%ld) must be multiples of 8", who, Cin, ldx);
  DX_REQUIRE(taps == 1 || taps == 3, DX_ERR_UNSUPPORTED, "%s: taps=%d (only 1 and 3)", who, taps);
  DX_REQUIRE(p_pre >= 0.f && p_pre < 1.f, DX_ERR_ARG, "%s: dropout p out of [0,1)", who);
  return DX_OK;
}

extern "C" int dx_conv1d_ln(const void* x, int x_dtype, long ldx, const void* w_packed, int w_dtype, const float* bias,
                            const float* residual, const float* gamma, const float* beta, const float* film, long ldf,
                            const int64_t* lengths, float* y, void* y_lp, float* s_out, float* mean, float* rstd, int B, int N,
                            int Cin, int taps, float p_pre, uint64_t seed_pre, const int* plan, int plan_tiles, const void* w_frag,
                            const void* w2_packed, const float* b2, void* y2, int n2, const DxStepScalars* step, void* stream) {
  return dx_conv1d_ln_vres(x, x_dtype, ldx, w_packed, w_dtype, bias, residual, nullptr, nullptr, nullptr, nullptr, gamma, beta, film, ldf, lengths,
                           y, y_lp, s_out, mean, rstd, B, N, Cin, taps, p_pre, seed_pre, plan, plan_tiles, w_frag, w2_packed, b2, y2, n2, step, stream);
}

extern "C" int dx_conv1d_ln_vres(const void* x, int x_dtype, long ldx, const void* w_packed, int w_dtype, const float* bias,
                                 const float* residual, const float* res_mean, const float* res_rstd, const float* res_gamma, const float* res_beta,
                                 const float* gamma, const float* beta, const float* film, long ldf,
                                 const int64_t* lengths, float* y, void* y_lp, float* s_out, float* mean, float* rstd, int B, int N,
                                 int Cin, int taps, float p_pre, uint64_t seed_pre, const int* plan, int plan_tiles, const void* w_frag,
                                 const void* w2_packed, const float* b2, void* y2, int n2, const DxStepScalars* step, void* stream) {
  const int path = dx_conv1d_ln_path(x_dtype, w_dtype, taps, Cin, B, N, plan != nullptr, w_frag != nullptr, 0);
  DX_REQUIRE(x && w_packed && residual && gamma && beta && (y || y_lp), DX_ERR_ARG, "dx_conv1d_ln: null pointer");
  DX_REQUIRE(y || (x_dtype == DX_BF16 && w_dtype == DX_BF16), DX_ERR_ARG, "dx_conv1d_ln: y = NULL (bf16 copy only) goes with bf16 operands");
  if (res_mean) {
    DX_REQUIRE(res_rstd && res_gamma && res_beta && lengths, DX_ERR_ARG, "dx_conv1d_ln_vres: res_mean / res_rstd / res_gamma / res_beta / lengths come together");
    DX_REQUIRE(path == DX_LN_PATH_SPLITK, DX_ERR_UNSUPPORTED, "dx_conv1d_ln_vres: the re-derived residual needs " DX_SPLITK_ONLY);
  }
  if (int rc = plan_check("dx_conv1d_ln", plan, plan_tiles, lengths, x_dtype, w_dtype, ldx, Cin, taps, B, N)) return rc;
  if (int rc = ln_args_check("dx_conv1d_ln", w_frag, plan, ldx, Cin, taps, B, N, p_pre)) return rc;
  DX_REQUIRE((mean == nullptr) == (rstd == nullptr), DX_ERR_ARG, "dx_conv1d_ln: mean and rstd come together");
  ConvArgs a{x, ldx, w_packed, bias, nullptr, BN, nullptr, lengths, lengths, N, Cin, BN, 0, B,
             LNEpi{gamma, beta, residual, film, ldf, y, y_lp, s_out, mean, rstd, p_pre, seed_pre, 1}};
  a.plan = plan; a.plan_tiles = plan_tiles; a.w_frag = w_frag; a.ln.step = step;
  a.ln.res_mean = res_mean; a.ln.res_rstd = res_rstd; a.ln.res_gamma = res_gamma; a.ln.res_beta = res_beta;
  if (y2) {   // second GEMM in the epilogue (the next block's QKV projection): only the split-K workgroups carry it
    DX_REQUIRE(w2_packed && (n2 == 128 || n2 == 384) && path == DX_LN_PATH_SPLITK, DX_ERR_UNSUPPORTED,
               "dx_conv1d_ln: y2 needs n2 in {128, 384} and " DX_SPLITK_ONLY);
    a.ln.w2 = w2_packed; a.ln.y2 = y2; a.ln.b2 = b2; a.ln.n2 = n2;
  }
  return launch_ln(a, x_dtype, w_dtype, taps, (hipStream_t)stream);
}

extern "C" int dx_conv1d_lnbwd(const void* x, int x_dtype, long ldx, const void* w_packed, int w_dtype, float* y_inout,
                               const float* s_in, const float* mean, const float* rstd, const float* gamma,
                               const float* beta, const float* film, long ldf, const int64_t* lengths, void* dx_pre_lp,
                               float* dgamma, float* dbeta, float* dfilm, long lddf, int B, int N, int Cin, int taps,
                               float p_pre, uint64_t seed_pre, const int* plan, int plan_tiles, const void* w_frag, const void* w2_packed,
                               void* y2, const DxStepScalars* step, void* stream) {
  if (int rc = plan_check("dx_conv1d_lnbwd", plan, plan_tiles, lengths, x_dtype, w_dtype, ldx, Cin, taps, B, N, true)) return rc;
  DX_REQUIRE(x && w_packed && y_inout && s_in && mean && rstd && gamma && beta && lengths && dx_pre_lp && dgamma && dbeta,
             DX_ERR_ARG, "dx_conv1d_lnbwd: null pointer");
  DX_REQUIRE((film == nullptr) == (dfilm == nullptr), DX_ERR_ARG, "dx_conv1d_lnbwd: film and dfilm come together");
  if (int rc = ln_args_check("dx_conv1d_lnbwd", w_frag, plan, ldx, Cin, taps, B, N, p_pre)) return rc;
  ConvArgs a{x, ldx, w_packed, nullptr, y_inout, BN, nullptr, lengths, lengths, N, Cin, BN, 0, B,
             LNEpi{gamma, beta, nullptr, film, ldf, y_inout, dx_pre_lp, const_cast<float*>(s_in), const_cast<float*>(mean),
                   const_cast<float*>(rstd), p_pre, seed_pre, 2, dgamma, dbeta, dfilm, lddf}};
  a.plan = plan; a.plan_tiles = plan_tiles; a.w_frag = w_frag; a.ln.step = step;
  if (y2) {   // second GEMM in the epilogue: only the split-K workgroups carry it
    DX_REQUIRE(w2_packed && dx_conv1d_ln_path(x_dtype, w_dtype, taps, Cin, B, N, plan != nullptr, w_frag != nullptr, 1) == DX_LN_PATH_SPLITK,
               DX_ERR_UNSUPPORTED, "dx_conv1d_lnbwd: y2 needs " DX_SPLITK_ONLY);
    a.ln.w2 = w2_packed; a.ln.y2 = y2; a.ln.b2 = nullptr; a.ln.n2 = BN;
  }
  return launch_ln(a, x_dtype, w_dtype, taps, (hipStream_t)stream);
}

extern "C" int dx_conv1d_wide(const void* x, long ldx, const void* w_frag, const float* bias, void* y, long ldy, const int64_t* lengths,
                              const int* plan, int plan_tiles, int halo, int B, int N, int Cin, int Cout, int flags, void* stream) {
  DX_REQUIRE(x && w_frag && y && lengths && plan, DX_ERR_ARG, "dx_conv1d_wide: null pointer");
  DX_REQUIRE(B > 0 && N > 0, DX_ERR_SHAPE, "dx_conv1d_wide: empty shape");
  DX_REQUIRE(Cin % 128 == 0 && Cin >= 256 && Cin <= DX_ZERO_PAGE_EL && Cout % 256 == 0 && ldx % 8 == 0 && ldy % 8 == 0, DX_ERR_UNSUPPORTED,
             "dx_conv1d_wide: Cin %% 128 == 0 (256..4096), Cout %% 256 == 0, row strides multiples of 8 (got Cin=%d Cout=%d)", Cin, Cout);
  DX_REQUIRE((flags & ~DX_CONV_RELU) == 0 && halo >= 0 && halo <= 8, DX_ERR_UNSUPPORTED, "dx_conv1d_wide: only DX_CONV_RELU is supported (flags=%d), halo 0..8", flags);
  DX_REQUIRE(plan_tiles >= B * dx_cdiv(N, DX_PLAN_ROWS), DX_ERR_ARG, "dx_conv1d_wide: plan_tiles=%d < B * ceil(N / 256)", plan_tiles);
  ConvArgs a{x, ldx, nullptr, bias, y, ldy, nullptr, nullptr, lengths, N, Cin, Cout, flags | (halo << 8), B, LNEpi{}};
  a.w_frag = w_frag; a.plan = plan; a.plan_tiles = plan_tiles;
  return conv_wide_launch(a, (hipStream_t)stream);
}
