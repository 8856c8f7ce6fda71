// K33 -- weight gradients of the HiFi-GAN generator's convolutions (csrc/vocoder.hip, K24), the one kernel family its training adds: the
// forward and both data gradients are dx_voc_conv / dx_voc_upsample launches with weights packed for the purpose.
//   dx_vocoder_wgrad           dW[tap][co][ci] = sum_{b, t < n[b]} rnd(dy[b, t, co]) * rnd(lrelu(x[b, t + (tap - (k - 1) / 2) d, ci]))
//   dx_vocoder_upsample_wgrad  the same kernel for the polyphase transposed conv: dy (B, N u, Cout) is read as (B, N, u Cout), and slot
//                              (p, s) of phase p contracts column block p of dy against x rows t + (p + pad) div u - s
// A GEMM that contracts over positions: M = Cout, N = Cin x taps, K = B x N.  A workgroup (4 waves, 2 x 2 of 32 x 32 MFMA tiles) owns
// 64 (co) x 64 (ci) x up to 4 tap slots of ONE phase and walks its share of the rows in items of 64: the dy tile [64][64] and the
// haloed x tile [64 + span][64] are staged in LDS row-major, activation and operand rounding applied once on the way in (what the
// forward applied to x); every tap slot reads the same x tile at its row offset.  Both MFMA operands want "8 consecutive positions of
// one channel": bf16 takes them with the LDS transpose read (ds_read_b64_tr_b16, gather8), fp32 reads channel-contiguous rows
// directly (A[i = l & 31][k = l >> 5]).  The rows are split over `parts` workgroups per output tile by shapes alone (never by the
// lengths); each writes its partial tile to the workspace in dW order and voc_wgrad_reduce_kernel adds the parts in index order.
// No atomics: two runs give the same bits.  Rows < 0 or >= n[b] of x and dy are zeros and are never read.
#include "dx_common.h"

namespace {

constexpr int VW_P = 64;          // contraction rows per item
constexpr int VW_T = 64;          // output tile: 64 co x 64 ci
constexpr int VW_TG = 4;          // tap slots per workgroup
constexpr int VW_SPAN = 64;       // staged x rows beyond the item: (taps - 1) * dilation <= 64, as in vocoder.hip
constexpr int VW_WG_TARGET = 1024;  // workgroups wanted per launch (4 per CU), while a part keeps >= VW_MIN_ITEMS items
constexpr int VW_MIN_ITEMS = 8;   // a partial tile (64 KiB) costs about two items' operands (36 KiB each)

struct VwArgs {
  const float* x; const float* dy; float* ws; const int64_t* n;
  long ldx, lddy, E;
  int B, N, Cin, Cout, taps, dil, ups, u, pad, k, ngroups, bpp, nchunk, chunk_items;
  float slope;
};

template <typename TC> struct VwLd;
template <> struct VwLd<bf16_t> { static constexpr int LD = VW_T + 8; };   // 144-byte rows (8-byte aligned for the transpose read)
template <> struct VwLd<float> { static constexpr int LD = VW_T + 4; };

__device__ __forceinline__ float vw_lrelu(float v, float slope) { return v > 0.f ? v : v * slope; }
__device__ __forceinline__ void vw_put4(bf16_t* p, f32x4 v) {
  bf16x4 r = {(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)v[3]};
  *reinterpret_cast<bf16x4*>(p) = r;
}
__device__ __forceinline__ void vw_put4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

// grid (tiles_co * tiles_ci, phases * tap groups, parts), 256 threads
template <typename TC>
__global__ __launch_bounds__(256) void voc_wgrad_kernel(VwArgs a) {
  constexpr int LD = VwLd<TC>::LD;
  __shared__ __attribute__((aligned(16))) TC dys[VW_P * LD];
  __shared__ __attribute__((aligned(16))) TC xs[(VW_P + VW_SPAN) * LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 5, l31 = lane & 31;
  const int wm = wave >> 1, wn = wave & 1;
  const int tiles_ci = dx_cdiv(a.Cin, VW_T);
  const int co0 = ((int)blockIdx.x / tiles_ci) * VW_T, ci0 = ((int)blockIdx.x % tiles_ci) * VW_T;
  const int U = a.ups ? a.u : 1;
  const int phase = (int)blockIdx.y / a.ngroups, s0 = ((int)blockIdx.y % a.ngroups) * VW_TG;
  // slot s contracts dy row t with x row t + off0 + s * step; `live` slots carry a tap j < k (the others stay zero)
  int off0, step, live;
  if (a.ups) {
    off0 = (phase + a.pad) / a.u;
    step = -1;
    const int j0 = (phase + a.pad) % a.u;
    live = j0 < a.k ? (a.k - j0 + a.u - 1) / a.u : 0;
  } else {
    off0 = -(a.dil * (a.taps - 1)) / 2;
    step = a.dil;
    live = a.taps;
  }
  const int ng = min(VW_TG, live - s0);                        // slots this workgroup computes (<= 0: none)
  const int o_a = off0 + s0 * step, o_b = off0 + (s0 + (ng > 0 ? ng - 1 : 0)) * step;
  const int min_off = min(o_a, o_b), rows = VW_P + (max(o_a, o_b) - min_off);
  const bool wave_live = co0 + 32 * wm < a.Cout && ci0 + 32 * wn < a.Cin;

  f32x16 acc[VW_TG];
#pragma unroll
  for (int t = 0; t < VW_TG; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  const int bg = (int)blockIdx.z / a.nchunk, chunk = (int)blockIdx.z % a.nchunk;
  const int b_end = min(a.B, (bg + 1) * a.bpp);
  bool first = true;
  if (ng > 0) {
    for (int b = bg * a.bpp; b < b_end; ++b) {
      const long nl = a.n[b];
      const int n_b = nl < 0 ? 0 : (nl > a.N ? a.N : (int)nl);
      const int t_end = min(n_b, (chunk + 1) * a.chunk_items * VW_P);
      const float* dyb = a.dy + (long)b * a.N * U * a.lddy + (long)phase * a.lddy;
      const float* xb = a.x + (long)b * a.N * a.ldx;
      for (int t0 = chunk * a.chunk_items * VW_P; t0 < t_end; t0 += VW_P) {
        if (!first) __syncthreads();
        first = false;
        for (int i = tid; i < VW_P * (VW_T / 4); i += 256) {
          const int row = i >> 4, q = i & 15, t = t0 + row, co = co0 + 4 * q;
          f32x4 v = {0.f, 0.f, 0.f, 0.f};
          if (t < n_b && co < a.Cout) v = *reinterpret_cast<const f32x4*>(dyb + (long)t * U * a.lddy + co);
          vw_put4(dys + row * LD + 4 * q, v);
        }
        for (int i = tid; i < rows * (VW_T / 4); i += 256) {
          const int row = i >> 4, q = i & 15, gr = t0 + min_off + row, ci = ci0 + 4 * q;
          f32x4 v = {0.f, 0.f, 0.f, 0.f};
          if (gr >= 0 && gr < n_b && ci < a.Cin) {
            v = *reinterpret_cast<const f32x4*>(xb + (long)gr * a.ldx + ci);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = vw_lrelu(v[e], a.slope);
          }
          vw_put4(xs + row * LD + 4 * q, v);
        }
        __syncthreads();
        if (wave_live) {
#pragma unroll
          for (int ks = 0; ks < VW_P / 16; ++ks) {
            const int kA = ks * 16 + 8 * g, kB = kA + 4;
            const auto af = gather8<TC, 32>(dys, LD, kA, kB, wm * 32, lane);
#pragma unroll
            for (int t = 0; t < VW_TG; ++t) {
              if (t < ng) {
                const int roff = off0 + (s0 + t) * step - min_off;
                const auto bf = gather8<TC, 32>(xs, LD, kA + roff, kB + roff, wn * 32, lane);
                dx_mma(acc[t], af, bf);
              }
            }
          }
        }
      }
    }
  }
  if (!wave_live) return;
  float* out = a.ws + (long)blockIdx.z * a.E;
  const int ci = ci0 + 32 * wn + l31;
#pragma unroll
  for (int t = 0; t < VW_TG; ++t) {
    if (s0 + t < a.taps) {
      const long slot = (long)phase * a.taps + s0 + t;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = co0 + 32 * wm + dx_acc_row(r, g);
        out[(slot * a.Cout + co) * a.Cin + ci] = acc[t][r];
      }
    }
  }
}

// dW = the parts' tiles added in index order: one thread per 4 consecutive elements
__global__ __launch_bounds__(256) void voc_wgrad_reduce_kernel(const float* __restrict__ ws, float* __restrict__ dw, long E, int parts) {
  const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= E) return;
  f32x4 s = *reinterpret_cast<const f32x4*>(ws + i);
  for (int p = 1; p < parts; ++p) s += *reinterpret_cast<const f32x4*>(ws + (long)p * E + i);
  *reinterpret_cast<f32x4*>(dw + i) = s;
}

struct VwPlan { int ngroups, bpp, nchunk, chunk_items, parts; long E; };

// how the rows are dealt to the workgroups of an output tile: from the shapes alone
VwPlan vw_plan(int B, int N, int Cin, int Cout, int taps, int U) {
  VwPlan p;
  p.ngroups = dx_cdiv(taps, VW_TG);
  p.E = (long)U * taps * Cout * Cin;
  const long tiles = (long)dx_cdiv(Cout, VW_T) * dx_cdiv(Cin, VW_T) * U * p.ngroups;
  const long items = dx_cdiv(N, VW_P), want = tiles >= VW_WG_TARGET ? 1 : VW_WG_TARGET / tiles;
  long per_part = (B * items + want - 1) / want;
  if (per_part < VW_MIN_ITEMS) per_part = VW_MIN_ITEMS;
  if (per_part >= items) {
    p.nchunk = 1;
    p.chunk_items = (int)items;
    const long bpp = per_part / items;
    p.bpp = (int)(bpp > B ? B : bpp);
  } else {
    p.bpp = 1;
    p.nchunk = (int)((items + per_part - 1) / per_part);
    p.chunk_items = (int)((items + p.nchunk - 1) / p.nchunk);
    p.nchunk = (int)((items + p.chunk_items - 1) / p.chunk_items);
  }
  p.parts = dx_cdiv(B, p.bpp) * p.nchunk;
  return p;
}

bool vw_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int vw_launch(VwArgs a, int w_dtype, float* dw, void* stream, const char* who) {
  const int U = a.ups ? a.u : 1, span = (a.taps - 1) * (a.ups ? 1 : a.dil);
  DX_REQUIRE(a.x && a.dy && dw && a.ws && a.n, DX_ERR_ARG, "%s: null pointer", who);
  DX_REQUIRE(w_dtype == DX_BF16 || w_dtype == DX_F32, DX_ERR_DTYPE, "%s: w_dtype %d is neither DX_BF16 nor DX_F32", who, w_dtype);
  DX_REQUIRE(a.Cin % 32 == 0 && a.Cout % 32 == 0, DX_ERR_UNSUPPORTED, "%s: Cin=%d and Cout=%d must be multiples of 32", who, a.Cin, a.Cout);
  DX_REQUIRE(a.N <= (1 << 30), DX_ERR_UNSUPPORTED, "%s: N=%d rows per utterance, at most 2^30", who, a.N);
  DX_REQUIRE(span <= VW_SPAN, DX_ERR_UNSUPPORTED,"%s: the taps span %d rows, at most %d are staged", who, span, VW_SPAN);
  DX_REQUIRE(a.ldx >= a.Cin && a.lddy >= a.Cout && a.ldx % 4 == 0 && a.lddy % 4 == 0, DX_ERR_SHAPE,
             "%s: row strides ldx=%ld lddy=%ld must cover their rows and be multiples of 4", who, a.ldx, a.lddy);
  DX_REQUIRE(vw_aligned16(a.x) && vw_aligned16(a.dy) && vw_aligned16(dw) && vw_aligned16(a.ws), DX_ERR_ARG,
             "%s: x, dy, dw and the workspace must be 16-byte aligned", who);
  const VwPlan p = vw_plan(a.B, a.N, a.Cin, a.Cout, a.taps, U);
  DX_REQUIRE(p.parts <= 65535 && (long)U * p.ngroups <= 65535, DX_ERR_UNSUPPORTED, "%s: %d parts x %ld tap groups exceed the grid", who,
             p.parts, (long)U * p.ngroups);
  a.E = p.E; a.ngroups = p.ngroups; a.bpp = p.bpp; a.nchunk = p.nchunk; a.chunk_items = p.chunk_items;
  hipStream_t s = (hipStream_t)stream;
  dim3 grid(dx_cdiv(a.Cout, VW_T) * dx_cdiv(a.Cin, VW_T), U * p.ngroups, p.parts);
  if (w_dtype == DX_BF16) hipLaunchKernelGGL(voc_wgrad_kernel<bf16_t>, grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL(voc_wgrad_kernel<float>, grid, dim3(256), 0, s, a);
  const long blocks = (p.E / 4 + 255) / 256;
  DX_REQUIRE(blocks <= 0x7fffffffL, DX_ERR_UNSUPPORTED, "%s: %ld weight elements", who, p.E);
  hipLaunchKernelGGL(voc_wgrad_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a.ws, dw, p.E, p.parts);
  DX_LAUNCH_CHECK();
  return DX_OK;
}

}  // namespace

extern "C" long dx_vocoder_wgrad_workspace(int B, int N, int Cin, int Cout, int k, int u) {
  if (B <= 0 || N <= 0 || Cin <= 0 || Cout <= 0 || k <= 0 || u <= 0) return 0;
  const VwPlan p = vw_plan(B, N, Cin, Cout, u > 1 ? (k + u - 1) / u : k, u);
  return (long)p.parts * p.E * (long)sizeof(float);
}

extern "C" int dx_vocoder_wgrad(const float* x, long ldx, const float* dy, long lddy, int w_dtype, float* dw, float* ws,
                            const int64_t* n_rows, int B, int N, int Cin, int Cout, int taps, int dilation, float in_slope,
                            void* stream) {
  DX_REQUIRE(B > 0 && N > 0 && Cin > 0 && Cout > 0 && taps > 0 && taps % 2 == 1 && dilation > 0, DX_ERR_SHAPE,
             "dx_vocoder_wgrad: bad shape B=%d N=%d Cin=%d Cout=%d taps=%d (odd) dilation=%d", B, N, Cin, Cout, taps, dilation);
  VwArgs a = {x, dy, ws, n_rows, ldx, lddy, 0, B, N, Cin, Cout, taps, dilation, 0, 1, 0, taps, 0, 0, 0, 0, in_slope};
  return vw_launch(a, w_dtype, dw, stream, "dx_vocoder_wgrad");
}

extern "C" int dx_vocoder_upsample_wgrad(const float* x, long ldx, const float* dy, long lddy, int w_dtype, float* dw, float* ws,
                                     const int64_t* n_rows, int B, int N, int Cin, int Cout, int k, int u, float in_slope,
                                     void* stream) {
  DX_REQUIRE(B > 0 && N > 0 && Cin > 0 && Cout > 0 && u > 0 && k >= u && (k - u) % 2 == 0, DX_ERR_SHAPE,
             "dx_vocoder_upsample_wgrad: bad shape B=%d N=%d Cin=%d Cout=%d k=%d u=%d (k >= u, k - u even)", B, N, Cin, Cout, k, u);
  DX_REQUIRE((long)N * u <= 0x7fffffffL, DX_ERR_SHAPE, "dx_vocoder_upsample_wgrad: N * u = %ld rows", (long)N * u);
  VwArgs a = {x, dy, ws, n_rows, ldx, lddy, 0, B, N, Cin, Cout, (k + u - 1) / u, 1, 1, u, (k - u) / 2, k, 0, 0, 0, 0, in_slope};
  return vw_launch(a, w_dtype, dw, stream, "dx_vocoder_upsample_wgrad");
}
