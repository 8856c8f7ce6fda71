// K24 -- the HiFi-GAN generator (Kong et al. 2020) as batched inference: mel (B, n_mel, T) -> waveform (B, T * hop).
// Activations are time-major fp32 (rows = samples, channels contiguous); the residual stream and every accumulation are fp32, the
// MFMA operands bf16 or fp32 (the model's switch).  Three entry points:
//   dx_voc_conv      k-tap dilated "same" conv as an implicit GEMM: M = samples, N = Cout, K = taps x Cin.  A workgroup stages 256
//                    output rows + the halo of d (k - 1) / 2 rows per side of ONE 32-channel slice of the input in LDS (leaky-ReLU and
//                    the rounding to the operand type applied once, on the way in); every tap then reads the same image at a row
//                    offset, so the activation is fetched once per Cin slice and not once per tap.  Weights [tap][Cout][Cin] are read
//                    as MFMA B fragments straight from global memory (16 / 32 contiguous bytes per lane, L2 resident).  Epilogue:
//                    bias, residual add, and the running sum over the ResBlocks of a stage (acc = [acc +] scale * result).
//   dx_voc_upsample  ConvTranspose1d(stride u) as u polyphase convs through the SAME kernel: output row t u + p sums the taps
//                    j = j0 + s u, j0 = (p + pad) mod u, of input rows t + (p + pad) div u - s.  Weights [phase][s][Cout][Cin], zero
//                    where j >= k (phases of unequal length, e.g. k 7, u 3).
//   dx_voc_post      leaky-ReLU 0.01, 7-tap conv to one channel, tanh: a reduction on the VALU, fp32 throughout.
//                    dx_vocoder_post_clamp is the same kernel with clamp(-1, 1) in place of tanh (BigVGAN's `use_tanh_at_final` off).
// Sequence ends: rows < 0 or >= n[b] of the input are zeros and are never read; output rows >= n[b] (x u) are written as zeros up
// to the padded extent.  No atomics, no split-K: every output element is one k-ordered chain in one lane, whatever the batch.
// Channel counts that are no multiple of 32 (and taps whose span exceeds the staged halo) run a plain VALU kernel of the same
// contract -- correctness only.
#include "dx_common.h"

namespace {

struct VocArgs {
  const float* x; const void* w; const float* bias; const float* res; float* y; float* acc; const int64_t* n;
  long ldx, ldr, ldy, lda;
  int N, Cin, Cout, taps, dil, ups, u, pad, acc_init;
  float slope, acc_scale;
};

constexpr int VOC_TM = 256;        // output rows (conv) / input rows (one phase of the transposed conv) per workgroup
constexpr int VOC_SPAN = 64;       // staged rows beyond the tile: (taps - 1) * dilation <= 64 (k 11, d 5: 50)
constexpr int VOC_CK = 32;         // input channels per staged slice

template <typename TC> struct VocLd;
template <> struct VocLd<bf16_t> { static constexpr int LD = VOC_CK + 8; };   // 80-byte rows: 16 rows of a ds_read_b128 group on 16 slots
template <> struct VocLd<float> { static constexpr int LD = VOC_CK + 4; };    // 144-byte rows

__device__ __forceinline__ float voc_lrelu(float v, float slope) { return v > 0.f ? v : v * slope; }

__device__ __forceinline__ bf16x8 voc_lds8(const bf16_t* p) { return *reinterpret_cast<const bf16x8*>(p); }
__device__ __forceinline__ f32x8 voc_lds8(const float* p) {
  const f32x4 lo = *reinterpret_cast<const f32x4*>(p), hi = *reinterpret_cast<const f32x4*>(p + 4);
  f32x8 r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return r;
}
__device__ __forceinline__ void voc_put4(bf16_t* p, f32x4 v) {
  bf16x4 r = {(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)v[3]};
  *reinterpret_cast<bf16x4*>(p) = r;
}
__device__ __forceinline__ void voc_put4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

// what one workgroup works on: its utterance, phase and the tap geometry (tap s reads input row m + off0 + s * step)
struct VocGeom { int b, phase, U, off0, step, min_off, n_b; long w_off; };
__device__ __forceinline__ VocGeom voc_geom(const VocArgs& a, int z) {
  VocGeom g;
  g.U = a.ups ? a.u : 1;
  g.b = z / g.U;
  g.phase = z - g.b * g.U;
  if (a.ups) {
    g.off0 = (g.phase + a.pad) / a.u;
    g.step = -1;
    g.w_off = (long)g.phase * a.taps * a.Cout * a.Cin;
  } else {
    g.off0 = -(a.dil * (a.taps - 1)) / 2;
    g.step = a.dil;
    g.w_off = 0;
  }
  g.min_off = g.step > 0 ? g.off0 : g.off0 + (a.taps - 1) * g.step;
  const long n = a.n[g.b];
  g.n_b = n < 0 ? 0 : (n > a.N ? a.N : (int)n);
  return g;
}

// bias, residual, sequence end, the ResBlock sum: one output element
__device__ __forceinline__ void voc_store(const VocArgs& a, const VocGeom& g, int gm, int col, float v) {
  if (gm >= a.N) return;
  const long orow = ((long)g.b * a.N + gm) * g.U + g.phase;
  const bool live = gm < g.n_b;
  if (live) {
    if (a.bias) v += a.bias[col];
    if (a.res) v += a.res[orow * a.ldr + col];
  }
  if (a.y) a.y[orow * a.ldy + col] = live ? v : 0.f;
  if (a.acc) {
    float* p = a.acc + orow * a.lda + col;
    if (live) *p = a.acc_init ? a.acc_scale * v : fmaf(a.acc_scale, v, *p);
    else if (a.acc_init) *p = 0.f;
  }
}

// grid (Cout / (32 NT), ceil(N / 256), B * phases), 4 waves; wave w owns rows 64 w .. 64 w + 63 of the tile and 32 NT output channels
template <typename TC, int NT>
__global__ __launch_bounds__(256) void voc_conv_mfma_kernel(VocArgs a) {
  constexpr int LD = VocLd<TC>::LD;
  __shared__ __attribute__((aligned(16))) TC tile[(VOC_TM + VOC_SPAN) * LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
  const VocGeom g = voc_geom(a, blockIdx.z);
  const int m0 = blockIdx.y * VOC_TM, cout0 = blockIdx.x * 32 * NT;
  f32x16 acc[2][NT];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.f;
  if (m0 < g.n_b) {                                               // a tile past the end: zeros, no loads, no MFMA
    const int rows = VOC_TM + (a.taps - 1) * (g.step > 0 ? g.step : -g.step);
    const float* xb = a.x + (long)g.b * a.N * a.ldx;
    const TC* w = reinterpret_cast<const TC*>(a.w) + g.w_off;
    for (int cin0 = 0; cin0 < a.Cin; cin0 += VOC_CK) {
      if (cin0) __syncthreads();
      for (int i = tid; i < rows * (VOC_CK / 4); i += 256) {
        const int row = i >> 3, q = i & 7, gr = m0 + g.min_off + row;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (gr >= 0 && gr < g.n_b) {
          v = *reinterpret_cast<const f32x4*>(xb + (long)gr * a.ldx + cin0 + 4 * q);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = voc_lrelu(v[e], a.slope);
        }
        voc_put4(tile + row * LD + 4 * q, v);
      }
      __syncthreads();
      for (int s = 0; s < a.taps; ++s) {
        const TC* arow = tile + (wave * 64 + l31 + g.off0 + s * g.step - g.min_off) * LD + 8 * half;
        const TC* wrow = w + ((long)s * a.Cout + cout0 + l31) * a.Cin + cin0 + 8 * half;
#pragma unroll
        for (int ks = 0; ks < VOC_CK / 16; ++ks) {
          const auto a0 = voc_lds8(arow + 16 * ks), a1 = voc_lds8(arow + 32 * LD + 16 * ks);
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) {
            const auto bw = dx_load8<TC, TC>(wrow + (long)nt * 32 * a.Cin + 16 * ks);
            dx_mma(acc[0][nt], a0, bw);
            dx_mma(acc[1][nt], a1, bw);
          }
        }
      }
    }
  }
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        voc_store(a, g, m0 + wave * 64 + mt * 32 + dx_acc_row(r, half), cout0 + nt * 32 + l31, acc[mt][nt][r]);
}

// the same contract on the VALU, any channel count: one thread per output element, taps and channels summed in order
template <typename TC>
__global__ __launch_bounds__(256) void voc_conv_valu_kernel(VocArgs a) {
  const VocGeom g = voc_geom(a, blockIdx.z);
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)a.N * a.Cout) return;
  const int gm = (int)(idx / a.Cout), col = (int)(idx - (long)gm * a.Cout);
  float v = 0.f;
  if (gm < g.n_b) {
    const float* xb = a.x + (long)g.b * a.N * a.ldx;
    const TC* w = reinterpret_cast<const TC*>(a.w) + g.w_off;
    for (int s = 0; s < a.taps; ++s) {
      const int gr = gm + g.off0 + s * g.step;
      if (gr < 0 || gr >= g.n_b) continue;
      const float* xr = xb + (long)gr * a.ldx;
      const TC* wr = w + ((long)s * a.Cout + col) * a.Cin;
      for (int c = 0; c < a.Cin; ++c) v = fmaf((float)(TC)voc_lrelu(xr[c], a.slope), (float)wr[c], v);
    }
  }
  voc_store(a, g, gm, col, v);
}

struct VocPostArgs { const float* x; const float* w; const float* bias; float* y; const int64_t* n; long ldx, ldy; int N, C, taps; float slope; };

// grid (ceil(N / 256), B): one thread per output sample; 16-byte loads when C and ldx are multiples of 4
template <bool CLAMP>
__global__ __launch_bounds__(256) void voc_post_kernel(VocPostArgs a) {
  const int b = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
  if (t >= a.N) return;
  const long n = a.n[b];
  const int n_b = n < 0 ? 0 : (n > a.N ? a.N : (int)n);
  float out = 0.f;
  if (t < n_b) {
    const float* xb = a.x + (long)b * a.N * a.ldx;
    float s = 0.f;
    for (int j = 0; j < a.taps; ++j) {
      const int r = t + j - a.taps / 2;
      if (r < 0 || r >= n_b) continue;
      const float* xr = xb + (long)r * a.ldx;
      const float* wr = a.w + j * a.C;
      if (((a.C | a.ldx) & 3) == 0) {
        for (int c = 0; c < a.C; c += 4) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(xr + c);
#pragma unroll
          for (int e = 0; e < 4; ++e) s = fmaf(voc_lrelu(v[e], a.slope), wr[c + e], s);
        }
      } else {
        for (int c = 0; c < a.C; ++c) s = fmaf(voc_lrelu(xr[c], a.slope), wr[c], s);
      }
    }
    s += a.bias ? a.bias[0] : 0.f;
    out = CLAMP ? fminf(fmaxf(s, -1.f), 1.f) : tanhf(s);
  }
  a.y[(long)b * a.ldy + t] = out;
}

bool voc_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int voc_launch(const VocArgs& a, int w_dtype, int B, void* stream, const char* who) {
  hipStream_t s = (hipStream_t)stream;
  const int U = a.ups ? a.u : 1, span = (a.taps - 1) * (a.ups ? 1 : a.dil);
  const bool mfma = a.Cin % 32 == 0 && a.Cout % 32 == 0 && a.ldx % 4 == 0 && span <= VOC_SPAN;
  DX_REQUIRE((long)B * U <= 65535, DX_ERR_UNSUPPORTED, "%s: B * phases = %ld > 65535 grid slices", who, (long)B * U);
  if (mfma) {
    const int nt = a.Cout % 64 == 0 ? 2 : 1;
    dim3 grid(a.Cout / (32 * nt), dx_cdiv(a.N, VOC_TM), B * U);
    if (w_dtype == DX_BF16) {
      if (nt == 2) hipLaunchKernelGGL((voc_conv_mfma_kernel<bf16_t, 2>), grid, dim3(256), 0, s, a);
      else hipLaunchKernelGGL((voc_conv_mfma_kernel<bf16_t, 1>), grid, dim3(256), 0, s, a);
    } else {
      if (nt == 2) hipLaunchKernelGGL((voc_conv_mfma_kernel<float, 2>), grid, dim3(256), 0, s, a);
      else hipLaunchKernelGGL((voc_conv_mfma_kernel<float, 1>), grid, dim3(256), 0, s, a);
    }
  } else {
    const long blocks = ((long)a.N * a.Cout + 255) / 256;
    DX_REQUIRE(blocks <= 0x7fffffffL, DX_ERR_UNSUPPORTED, "%s: N * Cout = %ld is too large for the VALU kernel", who, (long)a.N * a.Cout);
    dim3 grid((unsigned)blocks, 1, B * U);
    if (w_dtype == DX_BF16) hipLaunchKernelGGL(voc_conv_valu_kernel<bf16_t>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(voc_conv_valu_kernel<float>, grid, dim3(256), 0, s, a);
  }
  DX_LAUNCH_CHECK();
  return DX_OK;
}

template <bool CLAMP>
int voc_post_launch(const float* x, long ldx, const float* w, const float* bias, float* y, long ldy, const int64_t* n_rows, int B, int N,
                    int C, int taps, float in_slope, void* stream, const char* who) {
  DX_REQUIRE(x && w && y && n_rows, DX_ERR_ARG, "%s: null pointer", who);
  DX_REQUIRE(B > 0 && B <= 65535 && N > 0 && C > 0 && taps > 0 && taps % 2 == 1 && ldx >= C && ldy >= N, DX_ERR_SHAPE,
             "%s: bad shape B=%d N=%d C=%d taps=%d ldx=%ld ldy=%ld", who, B, N, C, taps, ldx, ldy);
  DX_REQUIRE(voc_aligned16(x), DX_ERR_ARG, "%s: x must be 16-byte aligned", who);
  VocPostArgs a = {x, w, bias, y, n_rows, ldx, ldy, N, C, taps, in_slope};
  hipLaunchKernelGGL(voc_post_kernel<CLAMP>, dim3(dx_cdiv(N, 256), B), dim3(256), 0, (hipStream_t)stream, a);
  DX_LAUNCH_CHECK();
  return DX_OK;
}

}  // namespace

extern "C" int dx_voc_conv(const float* x, long ldx, const void* w_packed, int w_dtype, const float* bias, const float* residual,
                           long ldr, float* y, long ldy, float* acc, long lda, float acc_scale, int acc_init,
                           const int64_t* n_rows, int B, int N, int Cin, int Cout, int taps, int dilation, float in_slope,
                           void* stream) {
  DX_REQUIRE(x && w_packed && n_rows && (y || acc), DX_ERR_ARG, "dx_voc_conv: null pointer");
  DX_REQUIRE(w_dtype == DX_BF16 || w_dtype == DX_F32, DX_ERR_DTYPE, "dx_voc_conv: w_dtype %d is neither DX_BF16 nor DX_F32", w_dtype);
  DX_REQUIRE(B > 0 && N > 0 && Cin > 0 && Cout > 0 && taps > 0 && taps % 2 == 1 && dilation > 0, DX_ERR_SHAPE,
             "dx_voc_conv: bad shape B=%d N=%d Cin=%d Cout=%d taps=%d (odd) dilation=%d", B, N, Cin, Cout, taps, dilation);
  DX_REQUIRE(ldx >= Cin && (!y || ldy >= Cout) && (!residual || ldr >= Cout) && (!acc || lda >= Cout), DX_ERR_SHAPE,
             "dx_voc_conv: a row stride is shorter than its row (ldx=%ld ldy=%ld ldr=%ld lda=%ld)", ldx, ldy, ldr, lda);
  DX_REQUIRE(voc_aligned16(x) && voc_aligned16(w_packed), DX_ERR_ARG, "dx_voc_conv: x and w_packed must be 16-byte aligned");
  DX_REQUIRE(y != x && acc != x, DX_ERR_ARG, "dx_voc_conv: the output must not alias the input (other workgroups read its halo)");
  VocArgs a = {x, w_packed, bias, residual, y, acc, n_rows, ldx, ldr, ldy, lda, N, Cin, Cout, taps, dilation, 0, 1, 0, acc_init,
               in_slope, acc_scale};
  return voc_launch(a, w_dtype, B, stream, "dx_voc_conv");
}

extern "C" int dx_voc_upsample(const float* x, long ldx, const void* w_packed, int w_dtype, const float* bias, float* y, long ldy,
                               const int64_t* n_rows, int B, int N, int Cin, int Cout, int k, int u, float in_slope, void* stream) {
  DX_REQUIRE(x && w_packed && n_rows && y, DX_ERR_ARG, "dx_voc_upsample: null pointer");
  DX_REQUIRE(w_dtype == DX_BF16 || w_dtype == DX_F32, DX_ERR_DTYPE, "dx_voc_upsample: w_dtype %d is neither DX_BF16 nor DX_F32", w_dtype);
  DX_REQUIRE(B > 0 && N > 0 && Cin > 0 && Cout > 0 && u > 0 && k >= u && (k - u) % 2 == 0, DX_ERR_SHAPE,
             "dx_voc_upsample: bad shape B=%d N=%d Cin=%d Cout=%d k=%d u=%d (k >= u, k - u even)", B, N, Cin, Cout, k, u);
  DX_REQUIRE((long)N * u <= 0x7fffffffL && ldx >= Cin && ldy >= Cout, DX_ERR_SHAPE,
             "dx_voc_upsample: N * u = %ld rows, ldx=%ld, ldy=%ld", (long)N * u, ldx, ldy);
  DX_REQUIRE(voc_aligned16(x) && voc_aligned16(w_packed), DX_ERR_ARG, "dx_voc_upsample: x and w_packed must be 16-byte aligned");
  VocArgs a = {x, w_packed, bias, nullptr, y, nullptr, n_rows, ldx, 0, ldy, 0, N, Cin, Cout, (k + u - 1) / u, 1, 1, u, (k - u) / 2, 0,
               in_slope, 0.f};
  return voc_launch(a, w_dtype, B, stream, "dx_voc_upsample");
}

extern "C" int dx_voc_post(const float* x, long ldx, const float* w, const float* bias, float* y, long ldy, const int64_t* n_rows,
                           int B, int N, int C, int taps, float in_slope, void* stream) {
  return voc_post_launch<false>(x, ldx, w, bias, y, ldy, n_rows, B, N, C, taps, in_slope, stream, "dx_voc_post");
}

extern "C" int dx_vocoder_post_clamp(const float* x, long ldx, const float* w, const float* bias, float* y, long ldy,
                                     const int64_t* n_rows, int B, int N, int C, int taps, float in_slope, void* stream) {
  return voc_post_launch<true>(x, ldx, w, bias, y, ldy, n_rows, B, N, C, taps, in_slope, stream, "dx_vocoder_post_clamp");
}
