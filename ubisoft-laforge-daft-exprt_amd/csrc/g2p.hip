// K30: the hot path of a grapheme-to-phoneme model trained on a pronunciation dictionary -- the CTC loss over the logits of one
// word with its gradient, and greedy CTC decoding.  The contract is the K30 comment of include/daft_exprt_hip.h.
//
// One wave walks one word; a workgroup holds CTC_WAVES words and has no barrier (a dictionary is tens of thousands of short
// words: the launch fills the chip with waves, and the host sorts a batch by length so the waves of a workgroup end together).
// The extended label sequence (blank, l_0, blank, l_1, ... blank: S = 2 n_labels + 1 states) lies over the lanes K states per
// lane, K = 1, 2 or 4 by the padded extent of the launch (S <= 64 / 128 / 256); the states of a lane are consecutive, so the
// s - 1 and s - 2 neighbours are the lane's own registers except at the lane's edge, where they are one DPP move away
// (dx_wave_shr1 / dx_wave_shl1, no LDS).  The arithmetic of a state does not depend on K: a word gives the same bits under any.
// The log-sum-exp of every step is taken first (not a chain: four steps' butterflies in flight at a time) and kept in LDS; the
// chains then gather the K emissions of a lane CTC_PF steps ahead.  The alpha plane lives in an HBM workspace (T x S floats per
// word do not fit the LDS of four words; a lane reads back only what it wrote itself).  The backward chain leaves the
// posteriors gamma(t, .) of a chunk of steps in LDS; the scatter to the class axis is then a gather: the lane that owns class v
// adds the states that carry v in order of s (a per-word list by class, built once), the blank states go through the fixed
// butterfly of dx_wave_sum.  No atomics anywhere.
#include "dx_common.h"

namespace {

constexpr int CTC_MAX_T = 256;         // dx_ctc_max_steps(): the step log-sum-exps (loss) and the arg-max path (greedy) of a word live in LDS
constexpr int CTC_MAX_U = 127;         // dx_ctc_max_labels(): S = 2 U + 1 <= 255 states, at most 4 per lane
constexpr int CTC_MAX_V = 128;         // dx_ctc_max_classes(): a lane owns the classes lane and lane + 64
constexpr int CTC_WAVES = 4;           // words per workgroup
constexpr float CTC_NINF = -__builtin_inff();

// what one lane wrote to LDS, read by another lane of the same wave
__device__ __forceinline__ void ctc_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// log(exp(a) + exp(b) + exp(c)), the terms added in this order; -inf for three -inf, never NaN
__device__ __forceinline__ float ctc_lse3(float a, float b, float c) {
  const float m = fmaxf(fmaxf(a, b), c);
  const float r = m + logf(expf(a - m) + expf(b - m) + expf(c - m));
  return m == CTC_NINF ? m : r;
}

// the log-sum-exp of the steps t0 .. t0 + 3 of a word (x: its logits), four butterflies in flight; lane 0 stores those below nT
__device__ __forceinline__ void ctc_lse4(const float* __restrict__ x, int t0, int nT, int V, int lane, float* __restrict__ s_lse) {
  float xa[4], xb[4], m[4], sum[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const bool in = t0 + j < nT;
    xa[j] = (in && lane < V) ? x[(long)(t0 + j) * V + lane] : CTC_NINF;
    xb[j] = (in && lane + 64 < V) ? x[(long)(t0 + j) * V + lane + 64] : CTC_NINF;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) m[j] = dx_wave_max(fmaxf(xa[j], xb[j]));
#pragma unroll
  for (int j = 0; j < 4; ++j) sum[j] = dx_wave_sum(expf(xa[j] - m[j]) + expf(xb[j] - m[j]));
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (lane == 0 && t0 + j < nT) s_lse[t0 + j] = m[j] + logf(sum[j]);
}

template <int K>
__global__ __launch_bounds__(CTC_WAVES * 64) void ctc_loss_kernel(const float* __restrict__ logits, const int64_t* __restrict__ n_steps,
                                                                  const int64_t* __restrict__ labels,
                                                                  const int64_t* __restrict__ n_labels, const float* __restrict__ w,
                                                                  float* __restrict__ loss, int* __restrict__ status,
                                                                  float* __restrict__ grad, float* __restrict__ ws, int B, int T, int U,
                                                                  int V) {
  constexpr int PF = K == 1 ? 8 : 4;   // steps fetched ahead of the chain (a step of K states is K times as long)
  constexpr int SK = K * 64;           // states the lanes hold
  __shared__ float s_lse[CTC_WAVES][CTC_MAX_T];
  __shared__ float s_gam[CTC_WAVES][PF][SK];
  __shared__ unsigned char s_lab[CTC_WAVES][CTC_MAX_U + 1];     // the labels of the word
  __shared__ unsigned char s_list[CTC_WAVES][CTC_MAX_U + 1];    // the label positions u, grouped by class, ascending inside a class
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int b = blockIdx.x * CTC_WAVES + wave;
  if (b >= B) return;                                           // (a whole wave; the kernel has no workgroup barrier)
  const int nT = (int)dx_clamp_len(n_steps, b, T), nL = (int)dx_clamp_len(n_labels, b, U);
  const int S = 2 * nL + 1, Sld = 2 * U + 1;
  const float* x = logits + (long)b * T * V;
  float* g = grad + (long)b * T * V;
  float* al = ws + (long)b * T * Sld;
  float* lse = s_lse[wave];
  unsigned char* lab = s_lab[wave];
  unsigned char* list = s_list[wave];

  // the labels, their range, and the adjacent equal pairs (each needs a blank between: one more step)
  bool bad = false;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int u = lane + 64 * h;
    const long l = u < nL ? (long)labels[(long)b * U + u] : 1;
    bad = bad || l < 1 || l >= V;
    lab[u] = (unsigned char)((l < 1 || l >= V || u >= nL) ? 0 : l);
  }
  ctc_wave_sync();
  int repeats = 0;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int u = lane + 64 * h;
    repeats += __popcll(__ballot(u >= 1 && u < nL && lab[u] == lab[u - 1]));
  }
  const int st = nT == 0 ? 2 : (__ballot(bad) != 0ull ? 3 : (nT < nL + repeats ? 1 : 0));
  if (st != 0) {                                                // (uniform over the wave)
    for (long i = lane; i < (long)T * V; i += 64) g[i] = 0.f;
    if (lane == 0) { loss[b] = __builtin_nanf(""); status[b] = st; }
    return;
  }

  // the positions of every class: the lane owns the classes lane and lane + 64, counts them, and a scan over the classes in order
  // gives each its stretch of `list`
  int cnt[2] = {0, 0}, start[2];
  for (int u = 0; u < nL; ++u) {
    const int l = lab[u];
    cnt[0] += l == lane;
    cnt[1] += l == lane + 64;
  }
  {
    const int x0 = dx_wave_scan(cnt[0], lane);
    const int x1 = dx_wave_scan(cnt[1], lane) + __shfl(x0, 63, 64);
    start[0] = x0 - cnt[0];
    start[1] = x1 - cnt[1];
    int at0 = start[0], at1 = start[1];
    for (int u = 0; u < nL; ++u) {
      const int l = lab[u];
      if (l == lane) list[at0++] = (unsigned char)u;
      if (l == lane + 64) list[at1++] = (unsigned char)u;
    }
  }
  for (int t0 = 0; t0 < nT; t0 += 4) ctc_lse4(x, t0, nT, V, lane, lse);
  ctc_wave_sync();

  // the lane's states s = K lane + k: the class each emits, and whether s - 2 -> s (forward) and s -> s + 2 (backward) exist
  int ext[K];
  bool live[K], skip[K], skipf[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int s = K * lane + k;
    live[k] = s < S;
    ext[k] = ((s & 1) && s < S) ? lab[(s - 1) >> 1] : 0;
    skip[k] = (s & 1) && s >= 3 && s < S && ext[k] != lab[(s - 3) >> 1];
    skipf[k] = (s & 1) && s + 2 < S && ext[k] != lab[(s + 1) >> 1];
  }

  // ---- alpha ----
  float a[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int s = K * lane + k;
    a[k] = (live[k] && s <= 1) ? x[ext[k]] - lse[0] : CTC_NINF;
    if (live[k]) al[s] = a[k];
  }
  {
    float cur[PF][K], nxt[PF][K];
#pragma unroll
    for (int u = 0; u < PF; ++u)
#pragma unroll
      for (int k = 0; k < K; ++k) cur[u][k] = (live[k] && 1 + u < nT) ? x[(long)(1 + u) * V + ext[k]] : 0.f;
    for (int t0 = 1; t0 < nT; t0 += PF) {
#pragma unroll
      for (int u = 0; u < PF; ++u)
#pragma unroll
        for (int k = 0; k < K; ++k) nxt[u][k] = (live[k] && t0 + PF + u < nT) ? x[(long)(t0 + PF + u) * V + ext[k]] : 0.f;
#pragma unroll
      for (int u = 0; u < PF; ++u) {
        const int t = t0 + u;
        if (t < nT) {                                           // (uniform)
          const float z = lse[t];
          const float up = dx_wave_shr1(a[K - 1], CTC_NINF);    // state K lane - 1
          const float up2 = K >= 2 ? dx_wave_shr1(a[K >= 2 ? K - 2 : 0], CTC_NINF) : dx_wave_shr1(up, CTC_NINF);   // state K lane - 2
          float na[K];
#pragma unroll
          for (int k = 0; k < K; ++k) {
            const float p1 = k > 0 ? a[k > 0 ? k - 1 : 0] : up;
            const float p2 = k > 1 ? a[k > 1 ? k - 2 : 0] : (k == 1 ? up : up2);
            na[k] = live[k] ? (cur[u][k] - z) + ctc_lse3(a[k], p1, skip[k] ? p2 : CTC_NINF) : CTC_NINF;
          }
#pragma unroll
          for (int k = 0; k < K; ++k) {
            a[k] = na[k];
            if (live[k]) al[(long)t * Sld + K * lane + k] = a[k];
          }
        }
      }
#pragma unroll
      for (int u = 0; u < PF; ++u)
#pragma unroll
        for (int k = 0; k < K; ++k) cur[u][k] = nxt[u][k];
    }
  }
  // log p = logaddexp of the last two states of the last step, for every lane
#pragma unroll
  for (int k = 0; k < K; ++k) s_gam[wave][0][K * lane + k] = a[k];
  ctc_wave_sync();
  const float ll = dx_logaddexp(s_gam[wave][0][S - 1], S > 1 ? s_gam[wave][0][S - 2] : CTC_NINF);
  ctc_wave_sync();
  if (lane == 0) { loss[b] = -ll; status[b] = 0; }

  // ---- beta, the posteriors, the gradient ----
  const float wb = w[b];
  float beta[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int s = K * lane + k;
    beta[k] = (s == S - 1 || s == S - 2) ? 0.f : CTC_NINF;
  }
  float ce[PF][K], ca[PF][K], ne[PF][K], na_[PF][K];            // the emissions of step t + 1 and alpha(t, .) of the steps t = t0 - u
#pragma unroll
  for (int u = 0; u < PF; ++u) {
    const int t = nT - 1 - u;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      ce[u][k] = (live[k] && t >= 0 && t + 1 < nT) ? x[(long)(t + 1) * V + ext[k]] : 0.f;
      ca[u][k] = (live[k] && t >= 0) ? al[(long)t * Sld + K * lane + k] : 0.f;
    }
  }
  for (int t0 = nT - 1; t0 >= 0; t0 -= PF) {
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      const int t = t0 - PF - u;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        ne[u][k] = (live[k] && t >= 0) ? x[(long)(t + 1) * V + ext[k]] : 0.f;
        na_[u][k] = (live[k] && t >= 0) ? al[(long)t * Sld + K * lane + k] : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      const int t = t0 - u;
      if (t >= 0) {                                             // (uniform)
        if (t + 1 < nT) {                                       // (uniform)
          const float z = lse[t + 1];
          float c[K];
#pragma unroll
          for (int k = 0; k < K; ++k) c[k] = (ce[u][k] - z) + beta[k];           // dead states: -inf
          const float dn = dx_wave_shl1(c[0], CTC_NINF);        // state K (lane + 1)
          const float dn2 = K >= 2 ? dx_wave_shl1(c[K >= 2 ? 1 : 0], CTC_NINF) : dx_wave_shl1(dn, CTC_NINF);   // state K (lane + 1) + 1
#pragma unroll
          for (int k = 0; k < K; ++k) {
            const float n1 = k < K - 1 ? c[k < K - 1 ? k + 1 : 0] : dn;
            const float n2 = k < K - 2 ? c[k < K - 2 ? k + 2 : 0] : (k == K - 2 ? dn : dn2);
            beta[k] = live[k] ? ctc_lse3(c[k], n1, skipf[k] ? n2 : CTC_NINF) : CTC_NINF;
          }
        }
#pragma unroll
        for (int k = 0; k < K; ++k) s_gam[wave][u][K * lane + k] = live[k] ? expf((ca[u][k] + beta[k]) - ll) : 0.f;
      }
    }
    ctc_wave_sync();
    // the chunk's posteriors to the class axis: blank = the even states, lane i adds the states 2 i and 2 (i + 64), then the butterfly
    float blank[PF];
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      float p = 2 * lane < SK ? s_gam[wave][u][2 * lane < SK ? 2 * lane : 0] : 0.f;
      if (2 * (lane + 64) < SK) p += s_gam[wave][u][2 * (lane + 64) < SK ? 2 * (lane + 64) : 0];
      blank[u] = t0 - u >= 0 ? p : 0.f;
    }
#pragma unroll
    for (int u = 0; u < PF; ++u) blank[u] = dx_wave_sum(blank[u]);
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      const int t = t0 - u;
      if (t >= 0) {                                             // (uniform)
        const float z = lse[t];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int v = lane + 64 * h;
          if (v < V) {
            float post = 0.f;
            if (v == 0) post = blank[u];
            else
              for (int j = 0; j < cnt[h]; ++j) post += s_gam[wave][u][2 * (int)list[start[h] + j] + 1];
            g[(long)t * V + v] = wb * (expf(x[(long)t * V + v] - z) - post);
          }
        }
      }
    }
    ctc_wave_sync();                                            // the next chunk rewrites s_gam
#pragma unroll
    for (int u = 0; u < PF; ++u)
#pragma unroll
      for (int k = 0; k < K; ++k) { ce[u][k] = ne[u][k]; ca[u][k] = na_[u][k]; }
  }
  for (long i = (long)nT * V + lane; i < (long)T * V; i += 64) g[i] = 0.f;
}

__global__ __launch_bounds__(CTC_WAVES * 64) void ctc_greedy_kernel(const float* __restrict__ logits, const int64_t* __restrict__ n_steps,
                                                                    int* __restrict__ ids, int* __restrict__ n_out,
                                                                    float* __restrict__ score, int B, int T, int V) {
  __shared__ unsigned char s_path[CTC_WAVES][CTC_MAX_T];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int b = blockIdx.x * CTC_WAVES + wave;
  if (b >= B) return;
  const int nT = (int)dx_clamp_len(n_steps, b, T);
  const float* x = logits + (long)b * T * V;
  unsigned char* path = s_path[wave];
  float sc = 0.f;
  for (int t0 = 0; t0 < nT; t0 += 4) {
    float xa[4], xb[4], bv[4], m[4], sum[4];
    int bi[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool in = t0 + j < nT;
      xa[j] = (in && lane < V) ? x[(long)(t0 + j) * V + lane] : CTC_NINF;
      xb[j] = (in && lane + 64 < V) ? x[(long)(t0 + j) * V + lane + 64] : CTC_NINF;
      bv[j] = xa[j];
      bi[j] = lane;
      if (xb[j] > bv[j]) { bv[j] = xb[j]; bi[j] = lane + 64; } // the higher class only when strictly greater
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) m[j] = dx_wave_max(bv[j]);
#pragma unroll
    for (int j = 0; j < 4; ++j) bi[j] = dx_wave_min(bv[j] == m[j] ? bi[j] : 0x7fffffff);   // ties: the lowest class
#pragma unroll
    for (int j = 0; j < 4; ++j) sum[j] = dx_wave_sum(expf(xa[j] - m[j]) + expf(xb[j] - m[j]));
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (t0 + j < nT) {                                        // (uniform)
        sc += -logf(sum[j]);                                    // max_v x - lse = -log(sum_v exp(x - max))
        if (lane == 0) path[t0 + j] = (unsigned char)(bi[j] < V ? bi[j] : 0);
      }
  }
  ctc_wave_sync();
  int base = 0;
  for (int c = 0; c * 64 < nT; ++c) {
    const int t = c * 64 + lane;
    const int p = t < nT ? path[t] : 0;
    const int prev = (t > 0 && t < nT) ? path[t - 1] : 0;
    const bool keep = p != 0 && p != prev;                      // a new non-blank symbol (step 0: anything but blank)
    const unsigned long long mask = __ballot(keep);
    if (keep) ids[(long)b * T + base + __popcll(mask & ((1ull << lane) - 1ull))] = p;
    base += __popcll(mask);
  }
  for (int t = base + lane; t < T; t += 64) ids[(long)b * T + t] = 0;
  if (lane == 0) { n_out[b] = base; score[b] = sc; }
}

}  // namespace

extern "C" long dx_ctc_max_steps(void) { return CTC_MAX_T; }
extern "C" long dx_ctc_max_labels(void) { return CTC_MAX_U; }
extern "C" long dx_ctc_max_classes(void) { return CTC_MAX_V; }

extern "C" int dx_ctc_loss(const float* logits, const int64_t* n_steps, const int64_t* labels, const int64_t* n_labels, const float* w,
                           float* loss, int* status, float* grad, float* ws, int B, int T, int U, int V, void* stream) {
  DX_REQUIRE(logits && n_steps && n_labels && w && loss && status && grad && ws && (labels || U == 0), DX_ERR_ARG,
             "dx_ctc_loss: null pointer");
  DX_REQUIRE(B > 0 && T > 0 && U >= 0 && V > 0, DX_ERR_SHAPE, "dx_ctc_loss: bad shape B=%d T=%d U=%d V=%d", B, T, U, V);
  DX_REQUIRE(T <= CTC_MAX_T && U <= CTC_MAX_U && V <= CTC_MAX_V && B <= 65535 * CTC_WAVES, DX_ERR_UNSUPPORTED,
             "dx_ctc_loss: T=%d steps (at most %d), U=%d labels (at most %d), V=%d classes (at most %d) or B=%d > %d", T, CTC_MAX_T, U,
             CTC_MAX_U, V, CTC_MAX_V, B, 65535 * CTC_WAVES);
  const int S = 2 * U + 1;
  const dim3 grid(dx_cdiv(B, CTC_WAVES)), block(CTC_WAVES * 64);
  if (S <= 64)
    hipLaunchKernelGGL(ctc_loss_kernel<1>, grid, block, 0, (hipStream_t)stream, logits, n_steps, labels, n_labels, w, loss, status, grad,
                       ws, B, T, U, V);
  else if (S <= 128)
    hipLaunchKernelGGL(ctc_loss_kernel<2>, grid, block, 0, (hipStream_t)stream, logits, n_steps, labels, n_labels, w, loss, status, grad,
                       ws, B, T, U, V);
  else
    hipLaunchKernelGGL(ctc_loss_kernel<4>, grid, block, 0, (hipStream_t)stream, logits, n_steps, labels, n_labels, w, loss, status, grad,
                       ws, B, T, U, V);
  DX_LAUNCH_CHECK();
  return DX_OK;
}

extern "C" int dx_ctc_greedy(const float* logits, const int64_t* n_steps, int* ids, int* n_out, float* score, int B, int T, int V,
                             void* stream) {
  DX_REQUIRE(logits && n_steps && ids && n_out && score, DX_ERR_ARG, "dx_ctc_greedy: null pointer");
  DX_REQUIRE(B > 0 && T > 0 && V > 0, DX_ERR_SHAPE, "dx_ctc_greedy: bad shape B=%d T=%d V=%d", B, T, V);
  DX_REQUIRE(T <= CTC_MAX_T && V <= CTC_MAX_V && B <= 65535 * CTC_WAVES, DX_ERR_UNSUPPORTED,
             "dx_ctc_greedy: T=%d steps (at most %d), V=%d classes (at most %d) or B=%d > %d", T, CTC_MAX_T, V, CTC_MAX_V, B,
             65535 * CTC_WAVES);
  hipLaunchKernelGGL(ctc_greedy_kernel, dim3(dx_cdiv(B, CTC_WAVES)), dim3(CTC_WAVES * 64), 0, (hipStream_t)stream, logits, n_steps, ids,
                     n_out, score, B, T, V);
  DX_LAUNCH_CHECK();
  return DX_OK;
}
