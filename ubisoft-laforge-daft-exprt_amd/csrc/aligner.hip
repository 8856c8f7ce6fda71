// K28: a learned aligner's hot path -- the soft alignment between frame queries and symbol keys, the forward-sum (monotonic,
// blank-free CTC) loss over it with its gradient, and monotonic alignment search (MAS) for the hard path.  The contract is the K28
// comment of include/daft_exprt_hip.h.
//
// The three lattice kernels (forward sum, its backward, MAS) are dependent chains of n_frm steps.  One workgroup walks one
// utterance, one thread per symbol, the thread's state alpha / beta / V of the previous frame in a register.  The neighbour
// symbol is one DPP move away inside a wave (dx_wave_shr1 / dx_wave_shl1, no LDS); between waves the edge value goes through a
// double-buffered LDS slot and one barrier per frame; a launch whose L fits one wave (<= 64 symbols) is a kernel without any
// barrier.  The rows of logp (and alpha) are fetched ALN_PF frames ahead into registers, so a step waits for arithmetic (an exp
// and a log1p), not for memory.  MAS keeps one direction bit per cell: a wave's 64 decisions of a frame are one ballot, stored as
// one 64-bit word; the backtrack stages 256 frames of words at a time in LDS and one thread walks them.
// The two soft-alignment kernels are not chains: one wave per frame (forward, dq), one workgroup per tile of 8 keys (dk), every
// sum in a fixed order.
#include "dx_common.h"

namespace {

constexpr int ALN_MAX_SYM = 1024;      // dx_aln_max_symbols(): one thread per symbol, one workgroup per utterance
constexpr int ALN_MAX_DIM = 256;       // dx_aln_max_dim()
constexpr int ALN_MAX_WAVES = ALN_MAX_SYM / 64;
constexpr int ALN_PF = 8;              // frames fetched ahead of the chain
constexpr int ALN_ROW_WAVES = 4;       // frames per workgroup of the soft-alignment kernels
constexpr int ALN_KEY_TILE = 8;        // keys per workgroup of the dk kernel (x 32 channels = 256 threads)
constexpr int ALN_MAX_FRAMES = 4096;   // frames whose symbol the MAS backtrack keeps in LDS; the host admits min(this, dx_dtw_max_len())
constexpr int ALN_BT_FRAMES = 256;     // frames of direction words staged per backtrack round: 256 * 16 words = 32 KiB (2 KiB for one wave)
constexpr float ALN_NINF = -__builtin_inff();

__device__ __forceinline__ int aln_status(int nf, int ns) { return (nf == 0 || ns == 0) ? 2 : (nf < ns ? 1 : 0); }

// ---- soft alignment: logp(t, .) = log_softmax_l(-temperature |q_t - k_l|^2 + prior(t, l)) ---------------------------------------------
__global__ __launch_bounds__(ALN_ROW_WAVES * 64) void aln_logprob_fwd_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                            const int64_t* __restrict__ n_frm,
                                                                            const int64_t* __restrict__ n_sym, float* __restrict__ logp,
                                                                            int T, int L, int A, float tau, float inv_2s2) {
  const int b = blockIdx.y, t = blockIdx.x * ALN_ROW_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (t >= T) return;                                           // (a whole wave; the kernel has no barrier)
  const int nf = (int)dx_clamp_len(n_frm, b, T), ns = (int)dx_clamp_len(n_sym, b, L);
  float* out = logp + ((long)b * T + t) * L;
  if (t >= nf || ns == 0) {
    for (int l = lane; l < L; l += 64) out[l] = 0.f;
    return;
  }
  const float* qr = q + ((long)b * T + t) * A;
  const float* kb = k + (long)b * L * A;
  const float ft = ((float)t + 0.5f) / (float)nf;
  float s[ALN_MAX_WAVES];
  float m = ALN_NINF;
#pragma unroll
  for (int c = 0; c < ALN_MAX_WAVES; ++c) {
    s[c] = ALN_NINF;
    const int l = c * 64 + lane;
    if (c * 64 < ns && l < ns) {
      const float* kr = kb + (long)l * A;
      float acc = 0.f;
      for (int a = 0; a < A; ++a) { const float d = qr[a] - kr[a]; acc = fmaf(d, d, acc); }
      float pr = 0.f;
      if (inv_2s2 > 0.f) { const float u = ((float)l + 0.5f) / (float)ns - ft; pr = -(u * u) * inv_2s2; }
      s[c] = fmaf(-tau, acc, pr);
      m = fmaxf(m, s[c]);
    }
  }
  m = dx_wave_max(m);
  float sum = 0.f;
#pragma unroll
  for (int c = 0; c < ALN_MAX_WAVES; ++c)
    if (c * 64 < ns && c * 64 + lane < ns) sum += expf(s[c] - m);
  const float lse = m + logf(dx_wave_sum(sum));
#pragma unroll
  for (int c = 0; c < ALN_MAX_WAVES; ++c) {
    const int l = c * 64 + lane;
    if (c * 64 < L && l < L) out[l] = l < ns ? s[c] - lse : 0.f;
  }
}

// dq and the row sums of g: one wave per frame; ds(t, .) of the frame in the wave's own stretch of LDS
__global__ __launch_bounds__(ALN_ROW_WAVES * 64) void aln_logprob_dq_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                           const float* __restrict__ logp, const float* __restrict__ g,
                                                                           const int64_t* __restrict__ n_frm,
                                                                           const int64_t* __restrict__ n_sym, float* __restrict__ dq,
                                                                           float* __restrict__ gsum, int T, int L, int A, float tau) {
  __shared__ float s_ds[ALN_ROW_WAVES][ALN_MAX_SYM];
  const int b = blockIdx.y, w = threadIdx.x >> 6, t = blockIdx.x * ALN_ROW_WAVES + w, lane = threadIdx.x & 63;
  if (t >= T) return;
  const int nf = (int)dx_clamp_len(n_frm, b, T), ns = (int)dx_clamp_len(n_sym, b, L);
  float* out = dq + ((long)b * T + t) * A;
  if (t >= nf || ns == 0) {
    for (int a = lane; a < A; a += 64) out[a] = 0.f;
    if (lane == 0) gsum[(long)b * T + t] = 0.f;
    return;
  }
  const float* gr = g + ((long)b * T + t) * L;
  const float* lr = logp + ((long)b * T + t) * L;
  float gs = 0.f;
  for (int l = lane; l < ns; l += 64) gs += gr[l];
  gs = dx_wave_sum(gs);
  if (lane == 0) gsum[(long)b * T + t] = gs;
  for (int l = lane; l < ns; l += 64) s_ds[w][l] = gr[l] - expf(lr[l]) * gs;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const float* qr = q + ((long)b * T + t) * A;
  const float* kb = k + (long)b * L * A;
  for (int a = lane; a < A; a += 64) {
    const float qa = qr[a];
    float acc = 0.f;
    for (int l = 0; l < ns; ++l) acc = fmaf(s_ds[w][l], qa - kb[(long)l * A + a], acc);
    out[a] = -2.f * tau * acc;
  }
}

// dk: a workgroup owns 8 keys, a thread one (key, channel) at a time, the frames in order
__global__ __launch_bounds__(ALN_KEY_TILE * 32) void aln_logprob_dk_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                          const float* __restrict__ logp, const float* __restrict__ g,
                                                                          const float* __restrict__ gsum,
                                                                          const int64_t* __restrict__ n_frm,
                                                                          const int64_t* __restrict__ n_sym, float* __restrict__ dk, int T,
                                                                          int L, int A, float tau) {
  const int b = blockIdx.y, l = blockIdx.x * ALN_KEY_TILE + (threadIdx.x >> 5), a0 = threadIdx.x & 31;
  if (l >= L) return;
  const int nf = (int)dx_clamp_len(n_frm, b, T), ns = (int)dx_clamp_len(n_sym, b, L);
  const float* qb = q + (long)b * T * A;
  const float* gb = g + (long)b * T * L + l;
  const float* lb = logp + (long)b * T * L + l;
  const float* sb = gsum + (long)b * T;
  for (int a = a0; a < A; a += 32) {
    float r = 0.f;
    if (l < ns) {
      const float ka = k[((long)b * L + l) * A + a];
      float acc = 0.f;
#pragma unroll 4
      for (int t = 0; t < nf; ++t) {
        const float ds = gb[(long)t * L] - expf(lb[(long)t * L]) * sb[t];
        acc = fmaf(ds, qb[(long)t * A + a] - ka, acc);
      }
      r = 2.f * tau * acc;
    }
    dk[((long)b * L + l) * A + a] = r;
  }
}

// ---- the lattice kernels ------------------------------------------------------------------------------------------------------------------
// rows [t0, t1) of a (T, L) plane of one utterance as zeros, the workgroup's thread l on column l
__device__ __forceinline__ void aln_zero_rows(float* __restrict__ plane, int t0, int t1, int L, int l) {
  if (l < L)
    for (int t = t0; t < t1; ++t) plane[(long)t * L + l] = 0.f;
}

template <bool MULTI>
__global__ __launch_bounds__(MULTI ? ALN_MAX_SYM : 64) void aln_forward_sum_kernel(const float* __restrict__ logp,
                                                                                   const int64_t* __restrict__ n_frm,
                                                                                   const int64_t* __restrict__ n_sym,
                                                                                   float* __restrict__ alpha, float* __restrict__ loss,
                                                                                   int* __restrict__ status, int T, int L) {
  __shared__ float s_edge[2][ALN_MAX_WAVES];
  const int b = blockIdx.x, l = threadIdx.x, lane = l & 63, wave = l >> 6;
  const int nf = (int)dx_clamp_len(n_frm, b, T), ns = (int)dx_clamp_len(n_sym, b, L);
  const int st = aln_status(nf, ns);
  const float* lp = logp + (long)b * T * L;
  float* al = alpha + (long)b * T * L;
  if (st != 0) {                                                // (uniform over the workgroup)
    aln_zero_rows(al, 0, T, L, l);
    if (l == 0) { loss[b] = __builtin_nanf(""); status[b] = st; }
    return;
  }
  const bool live = l < ns, inb = l < L;
  float a = l == 0 ? lp[0] : ALN_NINF;
  if (inb) al[l] = live ? a : 0.f;
  if (MULTI) {
    if (lane == 63) s_edge[0][wave] = a;
    __syncthreads();
  }
  float cur[ALN_PF], nxt[ALN_PF];
#pragma unroll
  for (int u = 0; u < ALN_PF; ++u) cur[u] = (live && 1 + u < nf) ? lp[(long)(1 + u) * L + l] : 0.f;
  for (int t0 = 1; t0 < nf; t0 += ALN_PF) {
#pragma unroll
    for (int u = 0; u < ALN_PF; ++u) nxt[u] = (live && t0 + ALN_PF + u < nf) ? lp[(long)(t0 + ALN_PF + u) * L + l] : 0.f;
#pragma unroll
    for (int u = 0; u < ALN_PF; ++u) {
      const int t = t0 + u;
      if (t < nf) {                                             // (uniform)
        float left = dx_wave_shr1(a, ALN_NINF);
        if (MULTI && lane == 0 && wave > 0) left = s_edge[(t - 1) & 1][wave - 1];
        a = cur[u] + dx_logaddexp(a, left);
        if (MULTI) {
          if (lane == 63) s_edge[t & 1][wave] = a;
          __syncthreads();
        }
        if (inb) al[(long)t * L + l] = live ? a : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < ALN_PF; ++u) cur[u] = nxt[u];
  }
  aln_zero_rows(al, nf, T, L, l);
  if (l == ns - 1) { loss[b] = -a; status[b] = 0; }
}

template <bool MULTI>
__global__ __launch_bounds__(MULTI ? ALN_MAX_SYM : 64) void aln_forward_sum_bwd_kernel(const float* __restrict__ logp,
                                                                                       const float* __restrict__ alpha,
                                                                                       const float* __restrict__ w,
                                                                                       const int64_t* __restrict__ n_frm,
                                                                                       const int64_t* __restrict__ n_sym,
                                                                                       float* __restrict__ dlogp, int T, int L) {
  __shared__ float s_edge[2][ALN_MAX_WAVES + 1];
  const int b = blockIdx.x, l = threadIdx.x, lane = l & 63, wave = l >> 6;
  const int nf = (int)dx_clamp_len(n_frm, b, T), ns = (int)dx_clamp_len(n_sym, b, L);
  const float* lp = logp + (long)b * T * L;
  const float* al = alpha + (long)b * T * L;
  float* out = dlogp + (long)b * T * L;
  if (aln_status(nf, ns) != 0) {
    aln_zero_rows(out, 0, T, L, l);
    return;
  }
  const bool live = l < ns, inb = l < L;
  const int last_wave = (int)(blockDim.x >> 6) - 1;
  const float end = al[(long)(nf - 1) * L + ns - 1], wb = w[b];
  float beta = l == ns - 1 ? 0.f : ALN_NINF;
  if (inb) {
    const float gm = live ? expf(al[(long)(nf - 1) * L + l] + beta - end) : 0.f;
    out[(long)(nf - 1) * L + l] = gm == 0.f ? 0.f : -wb * gm;
  }
  float cl[ALN_PF], ca[ALN_PF], nl[ALN_PF], na[ALN_PF];        // logp(t + 1, l) and alpha(t, l) of the frames t = t0 - u
#pragma unroll
  for (int u = 0; u < ALN_PF; ++u) {
    const int t = nf - 2 - u;
    cl[u] = (live && t >= 0) ? lp[(long)(t + 1) * L + l] : 0.f;
    ca[u] = (live && t >= 0) ? al[(long)t * L + l] : 0.f;
  }
  for (int t0 = nf - 2; t0 >= 0; t0 -= ALN_PF) {
#pragma unroll
    for (int u = 0; u < ALN_PF; ++u) {
      const int t = t0 - ALN_PF - u;
      nl[u] = (live && t >= 0) ? lp[(long)(t + 1) * L + l] : 0.f;
      na[u] = (live && t >= 0) ? al[(long)t * L + l] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < ALN_PF; ++u) {
      const int t = t0 - u;
      if (t >= 0) {                                             // (uniform)
        const float c = cl[u] + beta;
        float right = dx_wave_shl1(c, ALN_NINF);
        if (MULTI) {
          if (lane == 0) s_edge[t & 1][wave] = c;
          __syncthreads();
          if (lane == 63 && wave < last_wave) right = s_edge[t & 1][wave + 1];
        }
        if (l + 1 >= ns) right = ALN_NINF;
        beta = dx_logaddexp(c, right);
        if (inb) {
          const float gm = live ? expf(ca[u] + beta - end) : 0.f;
          out[(long)t * L + l] = gm == 0.f ? 0.f : -wb * gm;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < ALN_PF; ++u) { cl[u] = nl[u]; ca[u] = na[u]; }
  }
  aln_zero_rows(out, nf, T, L, l);
}

template <bool MULTI>
__global__ __launch_bounds__(MULTI ? ALN_MAX_SYM : 64) void aln_mas_kernel(const float* __restrict__ logp, const int64_t* __restrict__ n_frm,
                                                                           const int64_t* __restrict__ n_sym, float* __restrict__ score,
                                                                           int* __restrict__ path, int* __restrict__ path_len,
                                                                           int* __restrict__ status, unsigned long long* ws,
                                                                           long ws_words, int T, int L) {
  __shared__ float s_edge[2][ALN_MAX_WAVES];
  __shared__ unsigned long long s_bits[ALN_BT_FRAMES * (MULTI ? ALN_MAX_WAVES : 1)];   // (one wave: one word per frame)
  __shared__ unsigned short s_lab[ALN_MAX_FRAMES];              // the symbol of every frame
  const int b = blockIdx.x, l = threadIdx.x, lane = l & 63, wave = l >> 6, threads = (int)blockDim.x;
  const int nf = (int)dx_clamp_len(n_frm, b, T), ns = (int)dx_clamp_len(n_sym, b, L);
  const int st = aln_status(nf, ns);
  const int P = T + L - 1;
  int* out = path + (long)b * P * 2;
  if (st != 0) {
    for (int p = l; p < 2 * P; p += threads) out[p] = -1;
    if (l == 0) { score[b] = __builtin_nanf(""); path_len[b] = 0; status[b] = st; }
    return;
  }
  const float* lp = logp + (long)b * T * L;
  unsigned long long* W = ws + (long)b * ws_words;
  const int nw = (ns + 63) >> 6;                                // words per frame: the utterance's own extent, nf * nw <= ws_words
  const bool live = l < ns;
  float v = l == 0 ? lp[0] : ALN_NINF;
  if (MULTI) {
    if (lane == 63) s_edge[0][wave] = v;
    __syncthreads();
  }
  float cur[ALN_PF], nxt[ALN_PF];
#pragma unroll
  for (int u = 0; u < ALN_PF; ++u) cur[u] = (live && 1 + u < nf) ? lp[(long)(1 + u) * L + l] : 0.f;
  for (int t0 = 1; t0 < nf; t0 += ALN_PF) {
#pragma unroll
    for (int u = 0; u < ALN_PF; ++u) nxt[u] = (live && t0 + ALN_PF + u < nf) ? lp[(long)(t0 + ALN_PF + u) * L + l] : 0.f;
#pragma unroll
    for (int u = 0; u < ALN_PF; ++u) {
      const int t = t0 + u;
      if (t < nf) {                                             // (uniform)
        float left = dx_wave_shr1(v, ALN_NINF);
        if (MULTI && lane == 0 && wave > 0) left = s_edge[(t - 1) & 1][wave - 1];
        const bool step = live && left > v;                     // (t - 1, l - 1) only when strictly greater
        const unsigned long long word = __ballot(step);
        if (lane == 0 && wave < nw) W[(long)t * nw + wave] = word;
        v = cur[u] + (step ? left : v);
        if (MULTI) {
          if (lane == 63) s_edge[t & 1][wave] = v;
          __syncthreads();
        }
      }
    }
#pragma unroll
    for (int u = 0; u < ALN_PF; ++u) cur[u] = nxt[u];
  }
  if (l == ns - 1) { score[b] = v; path_len[b] = nf; status[b] = 0; }
  __syncthreads();                                              // the direction words of every wave are written

  // backtrack, 256 frames of words at a time: forced at l = 0 (stay) and at t = l (step), so no word can walk it out of the lattice
  int pos = ns - 1;                                             // (thread 0's)
  for (int thi = nf - 1; thi >= 1; thi -= ALN_BT_FRAMES) {
    const int tlo = max(1, thi - ALN_BT_FRAMES + 1);
    const int n = (thi - tlo + 1) * nw;
    for (int i = l; i < n; i += threads) s_bits[i] = W[(long)tlo * nw + i];
    __syncthreads();
    if (l == 0) {
      for (int t = thi; t >= tlo; --t) {
        s_lab[t] = (unsigned short)pos;
        const unsigned long long word = s_bits[(t - tlo) * nw + (pos >> 6)];
        if (pos > 0 && (t == pos || ((word >> (pos & 63)) & 1ull))) --pos;
      }
    }
    __syncthreads();
  }
  if (l == 0) s_lab[0] = (unsigned short)pos;                   // 0: pos <= t all the way
  __syncthreads();
  for (int p = l; p < P; p += threads) {
    out[2 * p] = p < nf ? p : -1;
    out[2 * p + 1] = p < nf ? (int)s_lab[p] : -1;
  }
}

int aln_check(const char* who, int B, int T, int L, int A) {
  DX_REQUIRE(B > 0 && T > 0 && L > 0 && A > 0, DX_ERR_SHAPE, "%s: bad shape B=%d T=%d L=%d A=%d", who, B, T, L, A);
  const long max_frames = dx_dtw_max_len() < ALN_MAX_FRAMES ? dx_dtw_max_len() : (long)ALN_MAX_FRAMES;
  DX_REQUIRE(T <= max_frames && L <= ALN_MAX_SYM && A <= ALN_MAX_DIM && B <= 65535, DX_ERR_UNSUPPORTED,
             "%s: T=%d frames (at most %ld), L=%d symbols (at most %d), A=%d channels (at most %d) or B=%d > 65535", who, T,
             max_frames, L, ALN_MAX_SYM, A, ALN_MAX_DIM, B);
  return DX_OK;
}

}  // namespace

extern "C" long dx_aln_max_symbols(void) { return ALN_MAX_SYM; }
extern "C" long dx_aln_max_dim(void) { return ALN_MAX_DIM; }

extern "C" int dx_aln_logprob_fwd(const float* q, const float* k, const int64_t* n_frm, const int64_t* n_sym, float temperature,
                                  float prior_sigma, float* logp, int B, int T, int L, int A, void* stream) {
  DX_REQUIRE(q && k && n_frm && n_sym && logp, DX_ERR_ARG, "dx_aln_logprob_fwd: null pointer");
  DX_REQUIRE(temperature > 0.f, DX_ERR_ARG, "dx_aln_logprob_fwd: temperature=%g (must be > 0)", (double)temperature);
  if (int rc = aln_check("dx_aln_logprob_fwd", B, T, L, A)) return rc;
  const float inv_2s2 = prior_sigma > 0.f ? (float)(1.0 / (2.0 * (double)prior_sigma * (double)prior_sigma)) : 0.f;
  hipLaunchKernelGGL(aln_logprob_fwd_kernel, dim3(dx_cdiv(T, ALN_ROW_WAVES), B), dim3(ALN_ROW_WAVES * 64), 0, (hipStream_t)stream, q, k,
                     n_frm, n_sym, logp, T, L, A, temperature, inv_2s2);
  DX_LAUNCH_CHECK();
  return DX_OK;
}

extern "C" int dx_aln_logprob_bwd(const float* q, const float* k, const float* logp, const float* g, const int64_t* n_frm,
                                  const int64_t* n_sym, float temperature, float* dq, float* dk, float* row_ws, int B, int T, int L,
                                  int A, void* stream) {
  DX_REQUIRE(q && k && logp && g && n_frm && n_sym && dq && dk && row_ws, DX_ERR_ARG, "dx_aln_logprob_bwd: null pointer");
  DX_REQUIRE(temperature > 0.f, DX_ERR_ARG, "dx_aln_logprob_bwd: temperature=%g (must be > 0)", (double)temperature);
  if (int rc = aln_check("dx_aln_logprob_bwd", B, T, L, A)) return rc;
  hipLaunchKernelGGL(aln_logprob_dq_kernel, dim3(dx_cdiv(T, ALN_ROW_WAVES), B), dim3(ALN_ROW_WAVES * 64), 0, (hipStream_t)stream, q, k,
                     logp, g, n_frm, n_sym, dq, row_ws, T, L, A, temperature);
  DX_LAUNCH_CHECK();
  hipLaunchKernelGGL(aln_logprob_dk_kernel, dim3(dx_cdiv(L, ALN_KEY_TILE), B), dim3(ALN_KEY_TILE * 32), 0, (hipStream_t)stream, q, k, logp,
                     g, row_ws, n_frm, n_sym, dk, T, L, A, temperature);
  DX_LAUNCH_CHECK();
  return DX_OK;
}

extern "C" int dx_aln_forward_sum(const float* logp, const int64_t* n_frm, const int64_t* n_sym, float* alpha, float* loss, int* status,
                                  int B, int T, int L, void* stream) {
  DX_REQUIRE(logp && n_frm && n_sym && alpha && loss && status, DX_ERR_ARG, "dx_aln_forward_sum: null pointer");
  if (int rc = aln_check("dx_aln_forward_sum", B, T, L, 1)) return rc;
  const int threads = 64 * dx_cdiv(L, 64);
  if (threads == 64)
    hipLaunchKernelGGL(aln_forward_sum_kernel<false>, dim3(B), dim3(64), 0, (hipStream_t)stream, logp, n_frm, n_sym, alpha, loss, status,
                       T, L);
  else
    hipLaunchKernelGGL(aln_forward_sum_kernel<true>, dim3(B), dim3(threads), 0, (hipStream_t)stream, logp, n_frm, n_sym, alpha, loss,
                       status, T, L);
  DX_LAUNCH_CHECK();
  return DX_OK;
}

extern "C" int dx_aln_forward_sum_bwd(const float* logp, const float* alpha, const float* w, const int64_t* n_frm, const int64_t* n_sym,
                                      float* dlogp, int B, int T, int L, void* stream) {
  DX_REQUIRE(logp && alpha && w && n_frm && n_sym && dlogp, DX_ERR_ARG, "dx_aln_forward_sum_bwd: null pointer");
  if (int rc = aln_check("dx_aln_forward_sum_bwd", B, T, L, 1)) return rc;
  const int threads = 64 * dx_cdiv(L, 64);
  if (threads == 64)
    hipLaunchKernelGGL(aln_forward_sum_bwd_kernel<false>, dim3(B), dim3(64), 0, (hipStream_t)stream, logp, alpha, w, n_frm, n_sym, dlogp,
                       T, L);
  else
    hipLaunchKernelGGL(aln_forward_sum_bwd_kernel<true>, dim3(B), dim3(threads), 0, (hipStream_t)stream, logp, alpha, w, n_frm, n_sym,
                       dlogp, T, L);
  DX_LAUNCH_CHECK();
  return DX_OK;
}

extern "C" int dx_aln_mas(const float* logp, const int64_t* n_frm, const int64_t* n_sym, float* score, int* path, int* path_len,
                          int* status, void* ws, long ws_stride, int B, int T, int L, void* stream) {
  DX_REQUIRE(logp && n_frm && n_sym && score && path && path_len && status && ws, DX_ERR_ARG, "dx_aln_mas: null pointer");
  if (int rc = aln_check("dx_aln_mas", B, T, L, 1)) return rc;
  DX_REQUIRE(ws_stride % 8 == 0 && ws_stride >= 8L * T * dx_cdiv(L, 64) && ((uintptr_t)ws & 7) == 0, DX_ERR_SHAPE,
             "dx_aln_mas: ws_stride=%ld bytes per utterance (a multiple of 8, 8 * T * ceil(L / 64) = %ld needed, ws 8-byte aligned)",
             ws_stride, 8L * T * dx_cdiv(L, 64));
  const int threads = 64 * dx_cdiv(L, 64);
  if (threads == 64)
    hipLaunchKernelGGL(aln_mas_kernel<false>, dim3(B), dim3(64), 0, (hipStream_t)stream, logp, n_frm, n_sym, score, path, path_len, status,
                       (unsigned long long*)ws, ws_stride / 8, T, L);
  else
    hipLaunchKernelGGL(aln_mas_kernel<true>, dim3(B), dim3(threads), 0, (hipStream_t)stream, logp, n_frm, n_sym, score, path, path_len,
                       status, (unsigned long long*)ws, ws_stride / 8, T, L);
  DX_LAUNCH_CHECK();
  return DX_OK;
}
