// K11 -- Gaussian upsampling (GaussianUpsamplingModule.forward, model.py:608-662), fp32 throughout
// (the alignment weights lose ~10 % in bf16), integer part exact:
//
//   x'      = enc + conv1->128(energy) + conv1->128(pitch)                          (model.py:618-628)
//   range_l = softplus(w_r . (x'_l + conv1->128(dur_float)_l) + b_r), 1 at pad l    (model.py:633-637)
//   mu_l    = float(d_l)/2 + float(sum_{j<l} d_j)      d = int64 durations          (model.py:641-643)
//   p[l,t]  = exp(-(t+0.5-mu_l)^2 / (2 range_l^2) - log(range_l) - log(sqrt(2 pi))), 0 at pad l
//   w[l,t]  = p[l,t] / (sum_l p[l,t] + 1e-20)                                        (model.py:653-657)
//   x_up[t] = sum_l w[l,t] x'_l                                                      (model.py:659)
//
// The reference materialises a (B, L, 128, T) product (3.4 GB at B=48); here a workgroup owns 32 frames of one
// utterance, keeps the weights of the phonemes that reach those frames in LDS and contracts them against x' from
// L2 -- only w (B,L,T) (it is a model output, "alignments") and x_up ever reach HBM.  The kernel also applies the
// decoder's positional add + mask (model.py:696-701) so the decoder input is produced in the same pass.
// Forward and backward are banded: a Gaussian is exactly 0.f outside its phoneme's reach (gu_reach), so each
// 32-frame tile works on a compacted list of the phonemes that reach it and each phoneme on its own frames.
#include "dx_common.h"

namespace {

constexpr int D = 128;
constexpr float LOG_SQRT_2PI = 0.91893853320467274178f;

// ---------------------------------------------------------------- prepare: x', ranges (one wave per (b,l) row)
struct PrepArgs {
  const float* enc; const float* dur_f; const float* energy; const float* pitch; const int64_t* lengths;
  const float* w_dur; const float* b_dur; const float* w_en; const float* b_en; const float* w_pi; const float* b_pi;
  const float* w_r; const float* b_r;
  float* xp; float* ranges; float* r_pre; float* rin;
  int L; long rows;
};
__device__ __forceinline__ float conv3(const float* ft, int l, int L, const float* w) {
  const float xm = l > 0 ? ft[l - 1] : 0.f, x0 = ft[l], xq = l + 1 < L ? ft[l + 1] : 0.f;
  return w[0] * xm + w[1] * x0 + w[2] * xq;
}
__global__ __launch_bounds__(256) void gu_prepare_kernel(PrepArgs a) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.rows) return;
  const int b = (int)(row / a.L), l = (int)(row - (long)b * a.L);
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int c = lane * 2 + k;
    const float xp = a.enc[row * D + c] + conv3(a.energy + (long)b * a.L, l, a.L, a.w_en + c * 3) + a.b_en[c] +
                     conv3(a.pitch + (long)b * a.L, l, a.L, a.w_pi + c * 3) + a.b_pi[c];
    a.xp[row * D + c] = xp;
    const float rin = xp + conv3(a.dur_f + (long)b * a.L, l, a.L, a.w_dur + c * 3) + a.b_dur[c];
    if (a.rin) a.rin[row * D + c] = rin;
    acc += rin * a.w_r[c];
  }
  acc = dx_wave_sum(acc) + a.b_r[0];
  if (lane == 0) {
    const bool pad = l >= (int)a.lengths[b];
    const float sp = acc > 20.f ? acc : log1pf(expf(acc));  // torch Softplus(beta=1, threshold=20)
    a.ranges[row] = pad ? 1.f : sp;
    if (a.r_pre) a.r_pre[row] = acc;
  }
}

// ---------------------------------------------------------------- means: exact int64 prefix sums (one wave per utterance)
// mu[l] = d[l] / 2 + sum_{k<l} d[k]   (`model.py:632-640`: cumsum of the integer durations, centre of each segment)
__global__ __launch_bounds__(64) void gu_means_kernel(const int64_t* __restrict__ dur_int, float* __restrict__ means,
                                                       int64_t* __restrict__ totals, int B, int L) {
  const int b = blockIdx.x, lane = threadIdx.x;
  long long carry = 0;
  for (int l0 = 0; l0 < L; l0 += 64) {
    const int l = l0 + lane;
    const long long d = l < L ? (long long)dur_int[(long)b * L + l] : 0;
    const long long incl = dx_wave_scan(d, lane);   // exact in int64
    const long long excl = carry + incl - d;
    if (l < L) {
      float mu = (float)d / 2.f;
      if (l > 0) mu += (float)excl;
      means[(long)b * L + l] = mu;
    }
    carry += __shfl(incl, 63, 64);
  }
  if (lane == 0) totals[b] = carry;
}

// ---------------------------------------------------------------- the reach of a phoneme
// p[l,t] = expf(a), a = -(t + .5 - mu)^2 / (2 sd^2) - logf(sd) - LOG_SQRT_2PI, is exactly 0.f wherever a is below expf's underflow
// point.  The smallest fp32 denormal is 2^-149 and anything under 2^-150 = e^-103.97 rounds to 0, so a device expf that keeps
// denormals returns 0 for a < -103.98; one that flushes them returns 0 already below -87.4, which only makes the zero region larger.
// With q = (t + .5 - mu)^2 / (2 sd^2):  q > GU_QZERO - logf(sd)  gives  a < -GU_QZERO - 0.9189 = -106.9, three units under the
// underflow point -- the few ulp of the divide, of logf and of expf's own argument reduction are < 1e-4 of that margin (for a huge q
// the absolute rounding grows with q, but so does the distance).  -logf(sd) > 0 for sd < 1 widens the reach, logf(sd) > 0 narrows
// it; the max with 0 only matters for sd > e^106, which fp32 does not hold.  So p can be non-zero only on the frames
//     |t + .5 - mu| <= sd sqrt(2 (GU_QZERO - logf(sd)))  =: r
// and [lo, hi] = [floor(mu - .5 - r'), ceil(mu - .5 + r')] with r' = 1.001 r + 1 (a frame of slack over the roundings of sqrtf, of
// the products and of mu - .5 -/+ r') contains them all.  sd that is 0, negative, infinite or NaN (and a mean that is not a
// sensible number) gives the whole axis: when in doubt, evaluate.  Forward and backward call this one function, so they agree on
// the band; inside it every pair is evaluated with the expression above, outside it the value is the constant 0.f.
constexpr float GU_QZERO = 106.f;
__device__ __forceinline__ void gu_reach(float mu, float sd, float logsd, int& lo, int& hi) {
  const float r = sd * sqrtf(2.f * fmaxf(GU_QZERO - logsd, 0.f)) * 1.001f + 1.f;
  const float c = mu - 0.5f;
  if (sd > 0.f && r < 1e9f && fabsf(c) < 1e9f) {   // |c -/+ r| < 2e9 < 2^31
    lo = (int)floorf(c - r);
    hi = (int)ceilf(c + r);
  } else {
    lo = -2147483647 - 1;
    hi = 2147483647;
  }
}

constexpr int TT = 32;      // frames per workgroup
constexpr int GU_R = 256;   // phonemes examined per round: one per thread of the workgroup
constexpr int GU_CAP = 128; // (phoneme, 32 frames) rows of Gaussian values a forward workgroup keeps in LDS; later ones go through `weights`

// One round's compacted list: the phonemes of [l0, l0 + GU_R) below `len` whose reach touches frames [t0, t1], in ascending l, with
// their per-phoneme invariants (2 sd^2 and logf(sd): the same values and roundings the per-pair expression used to recompute).
struct GuList {
  int l[GU_R];
  float mu[GU_R], h[GU_R], logsd[GU_R];
  int in[GU_R];     // in[i] != 0: phoneme l0 + i is on the list
  int part[4];
};
// Every thread of the 256-thread workgroup must call it; returns the list's length (<= GU_R: one slot per thread, so no index can
// pass the arrays).  Ends with a barrier; the caller puts another one between its last read of `s` and the next call.
__device__ __forceinline__ int gu_compact(GuList& s, const float* __restrict__ mu, const float* __restrict__ sg, int l0, int len, int t0, int t1) {
  const int tid = threadIdx.x, l = l0 + tid;
  int in = 0;
  float m = 0.f, sd = 1.f, lsd = 0.f;
  if (l < len) {
    m = mu[l]; sd = sg[l]; lsd = logf(sd);
    int lo, hi;
    gu_reach(m, sd, lsd, lo, hi);
    in = (lo <= t1 && hi >= t0) ? 1 : 0;
  }
  s.in[tid] = in;
  int n = 0;
  const int pos = dx_block_scan_step<4>(in, n, s.part);   // exclusive: pos <= tid < GU_R
  if (in) { s.l[pos] = l; s.mu[pos] = m; s.h[pos] = 2.f * sd * sd; s.logsd[pos] = lsd; }
  __syncthreads();
  return n;
}

// ---------------------------------------------------------------- upsample forward
struct UpArgs {
  const float* xp; const float* ranges; const float* means; const int64_t* in_len; const int64_t* out_len;
  const float* pos;   // positional table or null
  float* weights;     // (B, L, T)
  float* out;         // (B, T, D): (x_up + pos) masked by out_len when pos != null, else raw x_up
  int L, T;
};

// A workgroup owns 32 frames of one utterance.  Pass 1 walks the phonemes in rounds of GU_R: compact the ones that reach the tile,
// evaluate each (phoneme, frame) pair of the list ONCE (the value stays in LDS row `slot`, or, past GU_CAP rows, in its own element
// of `weights`, which the same thread reads back) and add it to the frame's partial sum.  Pass 2 divides by the denominators,
// contracts the weights against x' and only then stores: the decoder input, the listed weights and 0 for every other row of the
// tile.  All loads come before all stores because a wave's loads and stores share one in-order counter (vmcnt): a load issued
// behind twenty stores waits for their acknowledgements from HBM.  Every skipped term is an exact 0, and the order of what is left
// is the one the dense form had: partial sums by l mod 8 in ascending l, then k = 0..7; fmaf in ascending l.
// Channels: thread (ft, cg) holds channels 32 v + 4 cg + i (v, i < 4), so that the eight threads of a frame read and write 128
// contiguous bytes per instruction.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(6))) void gu_upsample_fwd_kernel(UpArgs a) {
  __shared__ GuList ls;
  __shared__ float Wt[GU_CAP][TT + 1];
  __shared__ float part[8][TT];
  __shared__ float denom[TT];
  const int tid = threadIdx.x, b = blockIdx.y, t0 = blockIdx.x * TT;
  const int tt = tid & 31, lg = tid >> 5;          // pass 1 / normalisation / weight stores: (frame, l mod 8)
  const int L = a.L, T = a.T;
  const int len = (int)dx_clamp_len(a.in_len, b, L);
  const int t1 = min(t0 + TT, T) - 1;
  const bool tin = t0 + tt < T;
  const float tc = (float)(t0 + tt) + 0.5f;
  const float* mu = a.means + (long)b * L;
  const float* sg = a.ranges + (long)b * L;
  float* wcol = a.weights + (long)b * L * T + t0 + tt;   // + l * T; only dereferenced when tin
  // pass 1
  float s = 0.f;
  int base = 0, n = 0;
  for (int l0 = 0; l0 < len; l0 += GU_R) {
    n = gu_compact(ls, mu, sg, l0, len, t0, t1);
    for (int j = 0; j < n; ++j) {
      const int l = ls.l[j];
      if ((l & 7) == lg) {
        const float dlt = tc - ls.mu[j];
        const float pv = expf(-(dlt * dlt) / ls.h[j] - ls.logsd[j] - LOG_SQRT_2PI);
        s += pv;
        if (base + j < GU_CAP) Wt[base + j][tt] = pv;
        else if (tin) wcol[(long)l * T] = pv;
      }
    }
    base += n;
    __syncthreads();
  }
  part[lg][tt] = s;
  __syncthreads();
  if (tid < TT) {
    float d = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) d += part[k][tid];
    denom[tid] = d + 1e-20f;
  }
  __syncthreads();
  // pass 2
  const int ft = tid >> 3, cg = tid & 7;            // contraction: (frame, channel group)
  f32x4 acc[4];
#pragma unroll
  for (int v = 0; v < 4; ++v) acc[v] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float den = denom[tt];
  const bool one_round = len <= GU_R;               // then `ls` still holds the only list
  const bool valid = a.pos ? t0 + ft < (int)a.out_len[b] : true;
  base = 0;
  for (int l0 = 0; l0 < L; l0 += GU_R) {
    const bool live = l0 < len;                     // a round with phonemes below len: it has a list
    if (live) {
      if (!one_round) n = gu_compact(ls, mu, sg, l0, len, t0, t1);
      for (int j = 0; j < n; ++j) {
        const int l = ls.l[j];
        if ((l & 7) == lg) {
          if (base + j < GU_CAP) Wt[base + j][tt] = Wt[base + j][tt] / den;
          else if (tin) wcol[(long)l * T] = wcol[(long)l * T] / den;
        }
      }
      __syncthreads();
#pragma unroll 2
      for (int j = 0; j < n; ++j) {
        const int l = ls.l[j];
        float w;
        if (base + j < GU_CAP) w = Wt[base + j][ft];
        else w = t0 + ft < T ? a.weights[((long)b * L + l) * T + t0 + ft] : 0.f;   // written by this workgroup before the barrier
        const f32x4* xr = reinterpret_cast<const f32x4*>(a.xp + ((long)b * L + l) * D) + cg;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const f32x4 x = xr[v * 8];
          acc[v][0] = fmaf(w, x[0], acc[v][0]); acc[v][1] = fmaf(w, x[1], acc[v][1]);
          acc[v][2] = fmaf(w, x[2], acc[v][2]); acc[v][3] = fmaf(w, x[3], acc[v][3]);
        }
      }
    }
    if (l0 + GU_R >= L && t0 + ft < T) {            // after the last round's contraction: the decoder input
      const int t = t0 + ft;
      f32x4* o = reinterpret_cast<f32x4*>(a.out + ((long)b * T + t) * D) + cg;
      if (a.pos) {
        const f32x4* pr = reinterpret_cast<const f32x4*>(a.pos + (long)t * D) + cg;
        f32x4 p[4];
#pragma unroll
        for (int v = 0; v < 4; ++v) p[v] = pr[v * 8];
#pragma unroll
        for (int v = 0; v < 4; ++v) o[v * 8] = valid ? acc[v] + p[v] : f32x4{0.f, 0.f, 0.f, 0.f};
      } else {
#pragma unroll
        for (int v = 0; v < 4; ++v) o[v * 8] = acc[v];
      }
    }
    if (tin) {                                      // this round's rows of the weight tile: the listed values, 0 elsewhere
      if (live)
        for (int j = 0; j < n; ++j) {
          const int l = ls.l[j];
          if ((l & 7) == lg && base + j < GU_CAP) wcol[(long)l * T] = Wt[base + j][tt];
        }
      const int lend = min(L, l0 + GU_R);
      for (int l = l0 + lg; l < lend; l += 8)
        if (!(live && ls.in[l - l0])) wcol[(long)l * T] = 0.f;
    }
    if (live) base += n;
    __syncthreads();
  }
}

// ---------------------------------------------------------------- backward, phase 1: dw[l,t] = g[t,:] . x'[l,:], Dsum[t] = sum_l w dw
struct UpBwd1Args {
  const float* g;        // (B, T, D) grad wrt the kernel output (already zero where masked)
  const float* xp; const float* weights; const float* means; const float* ranges; const int64_t* in_len; const int64_t* out_len;
  float* dw;             // (B, L, T), written for the phonemes that reach the tile (dw is only ever used multiplied by w, see bwd2)
  float* dsum;           // (B, T)
  int L, T;
};
__global__ __launch_bounds__(256) void gu_upsample_bwd1_kernel(UpBwd1Args a) {
  __shared__ GuList ls;
  __shared__ float G[TT][D + 1];
  __shared__ float part[8][TT];
  const int tid = threadIdx.x, b = blockIdx.y, t0 = blockIdx.x * TT;
  const int L = a.L, T = a.T, len = (int)dx_clamp_len(a.in_len, b, L);
  const int tvalid = a.out_len ? (int)dx_clamp_len(a.out_len, b, T) : T;
  if (t0 >= tvalid) {   // bwd2 stops at tvalid: nothing of this tile is read but, for tidiness, Dsum
    if (tid < TT && t0 + tid < T) a.dsum[(long)b * T + t0 + tid] = 0.f;
    return;
  }
  for (int i = tid; i < TT * D; i += 256) {
    const int r = i / D, c = i - r * D, t = t0 + r;
    G[r][c] = t < tvalid ? a.g[((long)b * T + t) * D + c] : 0.f;
  }
  const int tt = tid & 31, lg = tid >> 5;
  // the list does not depend on out_len (t1 is the tile's end, not tvalid), so the order of the sums below does not either
  const int t1 = min(t0 + TT, T) - 1;
  float dacc = 0.f;
  for (int l0 = 0; l0 < len; l0 += GU_R) {
    const int n = gu_compact(ls, a.means + (long)b * L, a.ranges + (long)b * L, l0, len, t0, t1);   // its barriers also cover G
    for (int j = lg; j < n; j += 8) {
      const int l = ls.l[j];
      const f32x4* xr = reinterpret_cast<const f32x4*>(a.xp + ((long)b * L + l) * D);
      float dot = 0.f;
      for (int c4 = 0; c4 < D / 4; ++c4) {
        const f32x4 x = xr[c4];
        dot = fmaf(G[tt][c4 * 4 + 0], x[0], dot); dot = fmaf(G[tt][c4 * 4 + 1], x[1], dot);
        dot = fmaf(G[tt][c4 * 4 + 2], x[2], dot); dot = fmaf(G[tt][c4 * 4 + 3], x[3], dot);
      }
      if (t0 + tt < T) {
        const long idx = ((long)b * L + l) * T + t0 + tt;
        a.dw[idx] = dot;
        dacc += a.weights[idx] * dot;
      }
    }
    __syncthreads();
  }
  part[lg][tt] = dacc;
  __syncthreads();
  if (tid < TT && t0 + tid < T) {
    float d = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) d += part[k][tid];
    a.dsum[(long)b * T + t0 + tid] = d;
  }
}

// ---------------------------------------------------------------- backward, phase 2 (one workgroup per (b,l)):
//   dxp[l,:] = sum_t w[l,t] g[t,:];   dsigma[l] = sum_t w[l,t] (dw[l,t] - Dsum[t]) ((t+.5-mu)^2/s^3 - 1/s)
//   dr = dsigma * sigmoid(r_pre);  dxp += dr * w_r;  d(range weight) and d(duration projection) handled by the caller
// t runs over the phoneme's reach clipped to the valid frames.  Eight groups of 32 threads (four channels each) take every eighth
// frame of it, so eight rows of g are in flight at once; the eight partial rows are then added in the fixed order k = 0..7.
struct UpBwd2Args {
  const float* g; const float* weights; const float* dw; const float* dsum; const float* means; const float* ranges;
  const float* r_pre; const float* w_r; const int64_t* in_len; const int64_t* out_len;
  float* dxp;        // (B, L, D) grad wrt x' (upsample path + range path)
  float* drin;       // (B, L, D) grad wrt the range-projection input (= dr * w_r), feeds the duration projection
  float* dr;         // (B, L)
  int L, T;
};
__global__ __launch_bounds__(256) void gu_upsample_bwd2_kernel(UpBwd2Args a) {
  __shared__ float racc[8][D];
  __shared__ float red[4];
  const int tid = threadIdx.x, l = blockIdx.x, b = blockIdx.y;
  const int L = a.L, T = a.T, len = (int)dx_clamp_len(a.in_len, b, L);
  const long row = (long)b * L + l;
  float* dxp = a.dxp + row * D;
  float* drin = a.drin + row * D;
  const int tvalid = a.out_len ? (int)dx_clamp_len(a.out_len, b, T) : T;
  // row < B * L whatever len is: these come back in one round trip with the lengths
  const float mu = a.means[row], sd = a.ranges[row], rp = a.r_pre[row], wr = a.w_r[tid & (D - 1)];
  if (l >= len) {
    if (tid < D) { dxp[tid] = 0.f; drin[tid] = 0.f; }
    if (tid == 0) a.dr[row] = 0.f;
    return;
  }
  const float* w = a.weights + row * T;
  const float* dwr = a.dw + row * T;
  const float* ds = a.dsum + (long)b * T;
  int lo, hi;
  gu_reach(mu, sd, logf(sd), lo, hi);
  const int tfirst = max(lo, 0), tlast = min(hi, tvalid - 1);   // 0 <= t < tvalid <= T inside both loops
  const int fg = tid >> 5, cq = tid & 31;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const float* gb = a.g + (long)b * T * D + cq * 4;
#pragma unroll 2
  for (int t = tfirst + fg; t <= tlast; t += 8) {
    const float wt = w[t];
    const f32x4 gv = *reinterpret_cast<const f32x4*>(gb + (long)t * D);
    acc[0] = fmaf(wt, gv[0], acc[0]); acc[1] = fmaf(wt, gv[1], acc[1]);
    acc[2] = fmaf(wt, gv[2], acc[2]); acc[3] = fmaf(wt, gv[3], acc[3]);
  }
  float dsig = 0.f;
  for (int t = tfirst + tid; t <= tlast; t += 256) {
    const float wt = w[t];
    if (wt != 0.f) {
      const float dlt = (float)t + 0.5f - mu;
      dsig += wt * (dwr[t] - ds[t]) * (dlt * dlt / (sd * sd * sd) - 1.f / sd);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) racc[fg][cq * 4 + i] = acc[i];
  dsig = dx_block_sum<4, false>(dsig, red);   // its barrier also publishes racc
  if (tid < D) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) s += racc[k][tid];
    const float dr = dsig * (rp > 20.f ? 1.f : 1.f / (1.f + expf(-rp)));
    const float dri = dr * wr;
    dxp[tid] = s + dri;
    drin[tid] = dri;
    if (tid == 0) a.dr[row] = dr;
  }
}

}  // namespace

extern "C" int dx_gu_prepare(const float* enc, const float* dur_float, const float* energy, const float* pitch,
                             const int64_t* in_lengths, const float* w_dur, const float* b_dur, const float* w_en,
                             const float* b_en, const float* w_pi, const float* b_pi, const float* w_range,
                             const float* b_range, float* xp, float* ranges, float* r_pre, float* rin, int B, int L,
                             int C, void* stream) {
  DX_REQUIRE(enc && dur_float && energy && pitch && in_lengths && xp && ranges, DX_ERR_ARG, "dx_gu_prepare: null pointer");
  DX_REQUIRE(C == D, DX_ERR_UNSUPPORTED, "dx_gu_prepare: C=%d (only 128)", C);
  DX_REQUIRE(B > 0 && L > 0, DX_ERR_SHAPE, "dx_gu_prepare: empty shape");
  PrepArgs a{enc, dur_float, energy, pitch, in_lengths, w_dur, b_dur, w_en, b_en, w_pi, b_pi, w_range, b_range, xp, ranges, r_pre, rin, L, (long)B * L};
  hipLaunchKernelGGL(gu_prepare_kernel, dim3((unsigned)((a.rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a);
  DX_LAUNCH_CHECK();
  return DX_OK;
}

extern "C" int dx_gu_means(const int64_t* durations_int, float* means, int64_t* totals, int B, int L, void* stream) {
  DX_REQUIRE(durations_int && means && totals, DX_ERR_ARG, "dx_gu_means: null pointer");
  hipLaunchKernelGGL(gu_means_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, durations_int, means, totals, B, L);
  DX_LAUNCH_CHECK();
  return DX_OK;
}

extern "C" int dx_gu_upsample_fwd(const float* xp, const float* ranges, const float* means, const int64_t* in_lengths,
                                  const int64_t* out_lengths, const float* pos_table, float* weights, float* out, int B,
                                  int L, int T, int C, void* stream) {
  DX_REQUIRE(xp && ranges && means && in_lengths && weights && out, DX_ERR_ARG, "dx_gu_upsample_fwd: null pointer");
  DX_REQUIRE(!pos_table || out_lengths, DX_ERR_ARG, "dx_gu_upsample_fwd: pos_table needs out_lengths");
  DX_REQUIRE(C == D, DX_ERR_UNSUPPORTED, "dx_gu_upsample_fwd: C=%d (only 128)", C);
  DX_REQUIRE(B > 0 && L > 0 && T > 0, DX_ERR_SHAPE, "dx_gu_upsample_fwd: empty shape");
  UpArgs a{xp, ranges, means, in_lengths, out_lengths, pos_table, weights, out, L, T};
  hipLaunchKernelGGL(gu_upsample_fwd_kernel, dim3(dx_cdiv(T, TT), B), dim3(256), 0, (hipStream_t)stream, a);
  DX_LAUNCH_CHECK();
  return DX_OK;
}

extern "C" int dx_gu_upsample_bwd(const float* g, const float* xp, const float* weights, const float* means,
                                  const float* ranges, const float* r_pre, const float* w_range,
                                  const int64_t* in_lengths, const int64_t* out_lengths, float* dw_ws, float* dsum_ws,
                                  float* dxp, float* drin, float* dr, int B, int L, int T, int C, void* stream) {
  DX_REQUIRE(g && xp && weights && means && ranges && r_pre && w_range && in_lengths && dw_ws && dsum_ws && dxp && drin && dr,
             DX_ERR_ARG, "dx_gu_upsample_bwd: null pointer");
  DX_REQUIRE(C == D, DX_ERR_UNSUPPORTED, "dx_gu_upsample_bwd: C=%d (only 128)", C);
  hipStream_t s = (hipStream_t)stream;
  UpBwd1Args a1{g, xp, weights, means, ranges, in_lengths, out_lengths, dw_ws, dsum_ws, L, T};
  hipLaunchKernelGGL(gu_upsample_bwd1_kernel, dim3(dx_cdiv(T, TT), B), dim3(256), 0, s, a1);
  UpBwd2Args a2{g, weights, dw_ws, dsum_ws, means, ranges, r_pre, w_range, in_lengths, out_lengths, dxp, drin, dr, L, T};
  hipLaunchKernelGGL(gu_upsample_bwd2_kernel, dim3(L, B), dim3(256), 0, s, a2);
  DX_LAUNCH_CHECK();
  return DX_OK;
}
