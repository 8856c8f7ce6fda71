// K31: the hot path of a CTC phone recogniser that scores intelligibility -- the CTC loss over the logits of one UTTERANCE with its
// gradient, greedy CTC decoding, and the edit distance of a decode to the phones that were asked for.  The contract is the K31 comment
// of include/daft_exprt_hip.h; the mathematics of the first two is K30's (csrc/g2p.hip), stated there once.
//
// K30 gives a wave to a word: a dictionary is tens of thousands of short rows.  An utterance is ~1 000 steps by up to 511 states in
// batches of 16 to 64: there are fewer rows than compute units, and the time goes into the chain over t.  So a row gets a workgroup of
// four waves, and the work is cut along t wherever it is not a chain:
//   1. the step log-sum-exps: all waves, four steps' butterflies in flight per wave, into LDS;
//   2. the chains: wave 0 walks alpha forwards while wave 1 walks beta backwards -- they share nothing but the emissions -- each with
//      K = 1, 2, 4 or 8 consecutive states per lane (neighbours across a lane edge through dx_wave_shr1 / dx_wave_shl1), emissions
//      gathered UC_PF steps ahead, both planes written to the HBM workspace (2 x T x S floats do not fit LDS);
//   3. the gradient: all waves, UC_PF steps per wave at a time: gamma = exp(alpha + beta - log p) into LDS, then K30's gather -- the
//      lane that owns class v adds the states that carry v in order of s, the blank goes through the butterfly of dx_wave_sum.
// The arithmetic of a state depends neither on K nor on which wave or lane holds it: a row gives the same bits under any padded extent.
// No atomics anywhere.
//
// uc_wave_sync, uc_lse3 and uc_lse4 are copies of K30's ctc_wave_sync, ctc_lse3 and ctc_lse4: they stay here, not in dx_common.h,
// so that the device code of g2p.hip is the one its tests pinned.
//
// The edit distance walks the anti-diagonals of the (n_ref + 1) x (n_hyp + 1) lattice with three of them in LDS, one barrier per
// diagonal, as the DTW of dtw_eval.hip does.  A cell carries its substitutions and deletions; with them i and j give the rest
// (matches = i - sub - del, insertions = j - i + del, cost = sub + 2 del + j - i), so no direction is stored and nothing is traced back.
#include "dx_common.h"

namespace {

constexpr int UC_MAX_T = 2048;         // dx_uctc_max_steps(): the step log-sum-exps (loss), the arg-max path and step scores (greedy) live in LDS
constexpr int UC_MAX_U = 255;          // dx_uctc_max_labels(): S = 2 U + 1 <= 511 states, at most 8 per lane
constexpr int UC_MAX_V = 128;          // dx_uctc_max_classes(): a lane owns the classes lane and lane + 64
constexpr int UC_WAVES = 4;
constexpr int UC_THREADS = UC_WAVES * 64;
constexpr int UC_PF = 4;               // steps fetched ahead of a chain, and steps a wave turns into gradient at a time
constexpr int ED_MAX_LEN = 2048;       // dx_edit_max_len(): LDS holds both sequences and 3 diagonals of 2049 cells: 40 972 B
constexpr int ED_THREADS = 256;
constexpr float UC_NINF = -__builtin_inff();

// what one lane wrote to LDS, read by another lane of the same wave
__device__ __forceinline__ void uc_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// log(exp(a) + exp(b) + exp(c)), the terms added in this order; -inf for three -inf, never NaN
__device__ __forceinline__ float uc_lse3(float a, float b, float c) {
  const float m = fmaxf(fmaxf(a, b), c);
  const float r = m + logf(expf(a - m) + expf(b - m) + expf(c - m));
  return m == UC_NINF ? m : r;
}

// the log-sum-exp of the steps t0 .. t0 + 3 of a row (x: its logits), four butterflies in flight; lane 0 stores those below nT
__device__ __forceinline__ void uc_lse4(const float* __restrict__ x, int t0, int nT, int V, int lane, float* __restrict__ s_lse) {
  float xa[4], xb[4], m[4], sum[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const bool in = t0 + j < nT;
    xa[j] = (in && lane < V) ? x[(long)(t0 + j) * V + lane] : UC_NINF;
    xb[j] = (in && lane + 64 < V) ? x[(long)(t0 + j) * V + lane + 64] : UC_NINF;
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
__global__ __launch_bounds__(UC_THREADS) void uctc_loss_kernel(const float* __restrict__ logits, const int64_t* __restrict__ n_steps,
                                                               const int64_t* __restrict__ labels, const int64_t* __restrict__ n_labels,
                                                               const float* __restrict__ w, float* __restrict__ loss,
                                                               int* __restrict__ status, float* __restrict__ grad, float* __restrict__ ws,
                                                               int B, int T, int U, int V) {
  constexpr int SK = K * 64;           // states the lanes hold
  __shared__ float s_lse[UC_MAX_T];
  __shared__ float s_gam[UC_WAVES][UC_PF][SK];
  __shared__ unsigned char s_lab[UC_MAX_U + 1];                 // the labels of the row
  __shared__ unsigned char s_list[UC_MAX_U + 1];                // the label positions u, grouped by class, ascending inside a class
  __shared__ int s_start[UC_MAX_V], s_cnt[UC_MAX_V];            // the stretch of s_list of every class
  __shared__ int s_red[UC_WAVES];
  __shared__ float s_ll;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int b = blockIdx.x;
  const int nT = (int)dx_clamp_len(n_steps, b, T), nL = (int)dx_clamp_len(n_labels, b, U);
  const int S = 2 * nL + 1, Sld = 2 * U + 1;
  const float* x = logits + (long)b * T * V;
  float* g = grad + (long)b * T * V;
  float* al = ws + (long)b * T * Sld;                           // alpha(t, s) at t * Sld + s
  float* be = ws + ((long)B + b) * T * Sld;                     // beta(t, s)

  // the labels (thread u holds label u), their range, and the adjacent equal pairs (each needs a blank between: one more step)
  {
    const long l = tid < nL ? (long)labels[(long)b * U + tid] : 1;
    const bool bad = l < 1 || l >= V;
    s_lab[tid] = (unsigned char)((bad || tid >= nL) ? 0 : l);
    const int n_bad = dx_block_sum<UC_WAVES>(bad ? 1 : 0, s_red);                // (its barriers publish s_lab)
    const int repeats = dx_block_sum<UC_WAVES>((tid >= 1 && tid < nL && s_lab[tid] == s_lab[tid - 1]) ? 1 : 0, s_red);
    const int st = nT == 0 ? 2 : (n_bad != 0 ? 3 : (nT < nL + repeats ? 1 : 0));
    if (st != 0) {                                              // (uniform over the workgroup)
      for (long i = tid; i < (long)T * V; i += UC_THREADS) g[i] = 0.f;
      if (tid == 0) { loss[b] = __builtin_nanf(""); status[b] = st; }
      return;
    }
  }

  // wave 0: the positions of every class -- the lane owns the classes lane and lane + 64, counts them, and a scan over the classes in
  // order gives each its stretch of s_list.  Meanwhile, and then with wave 0 too: the step log-sum-exps
  if (wave == 0) {
    int cnt[2] = {0, 0};
    for (int u = 0; u < nL; ++u) {
      const int l = s_lab[u];
      cnt[0] += l == lane;
      cnt[1] += l == lane + 64;
    }
    const int x0 = dx_wave_scan(cnt[0], lane);
    const int x1 = dx_wave_scan(cnt[1], lane) + __shfl(x0, 63, 64);
    int at0 = x0 - cnt[0], at1 = x1 - cnt[1];
    s_start[lane] = at0; s_start[lane + 64] = at1;
    s_cnt[lane] = cnt[0]; s_cnt[lane + 64] = cnt[1];
    for (int u = 0; u < nL; ++u) {
      const int l = s_lab[u];
      if (l == lane) s_list[at0++] = (unsigned char)u;
      if (l == lane + 64) s_list[at1++] = (unsigned char)u;
    }
  }
  for (int t0 = 4 * wave; t0 < nT; t0 += 4 * UC_WAVES) uc_lse4(x, t0, nT, V, lane, s_lse);
  __syncthreads();

  if (wave < 2) {
    // the lane's states s = K lane + k: the class each emits, and whether s - 2 -> s (forward) and s -> s + 2 (backward) exist
    int ext[K];
    bool live[K], skip[K], skipf[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int s = K * lane + k;
      live[k] = s < S;
      ext[k] = ((s & 1) && s < S) ? s_lab[(s - 1) >> 1] : 0;
      skip[k] = (s & 1) && s >= 3 && s < S && ext[k] != s_lab[(s - 3) >> 1];
      skipf[k] = (s & 1) && s + 2 < S && ext[k] != s_lab[(s + 1) >> 1];
    }
    if (wave == 0) {
      // ---- alpha, forwards ----
      float a[K];
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int s = K * lane + k;
        a[k] = (live[k] && s <= 1) ? x[ext[k]] - s_lse[0] : UC_NINF;
        if (live[k]) al[s] = a[k];
      }
      float cur[UC_PF][K], nxt[UC_PF][K];
#pragma unroll
      for (int u = 0; u < UC_PF; ++u)
#pragma unroll
        for (int k = 0; k < K; ++k) cur[u][k] = (live[k] && 1 + u < nT) ? x[(long)(1 + u) * V + ext[k]] : 0.f;
      for (int t0 = 1; t0 < nT; t0 += UC_PF) {
#pragma unroll
        for (int u = 0; u < UC_PF; ++u)
#pragma unroll
          for (int k = 0; k < K; ++k) nxt[u][k] = (live[k] && t0 + UC_PF + u < nT) ? x[(long)(t0 + UC_PF + u) * V + ext[k]] : 0.f;
#pragma unroll
        for (int u = 0; u < UC_PF; ++u) {
          const int t = t0 + u;
          if (t < nT) {                                         // (uniform)
            const float z = s_lse[t];
            const float up = dx_wave_shr1(a[K - 1], UC_NINF);   // state K lane - 1
            const float up2 = K >= 2 ? dx_wave_shr1(a[K >= 2 ? K - 2 : 0], UC_NINF) : dx_wave_shr1(up, UC_NINF);   // state K lane - 2
            float na[K];
#pragma unroll
            for (int k = 0; k < K; ++k) {
              const float p1 = k > 0 ? a[k > 0 ? k - 1 : 0] : up;
              const float p2 = k > 1 ? a[k > 1 ? k - 2 : 0] : (k == 1 ? up : up2);
              na[k] = live[k] ? (cur[u][k] - z) + uc_lse3(a[k], p1, skip[k] ? p2 : UC_NINF) : UC_NINF;
            }
#pragma unroll
            for (int k = 0; k < K; ++k) {
              a[k] = na[k];
              if (live[k]) al[(long)t * Sld + K * lane + k] = a[k];
            }
          }
        }
#pragma unroll
        for (int u = 0; u < UC_PF; ++u)
#pragma unroll
          for (int k = 0; k < K; ++k) cur[u][k] = nxt[u][k];
      }
      // log p = logaddexp of the last two states of the last step (s_gam is free until the gradient)
#pragma unroll
      for (int k = 0; k < K; ++k) s_gam[0][0][K * lane + k] = a[k];
      uc_wave_sync();
      const float ll = dx_logaddexp(s_gam[0][0][S - 1], S > 1 ? s_gam[0][0][S - 2] : UC_NINF);
      if (lane == 0) { loss[b] = -ll; status[b] = 0; s_ll = ll; }
    } else {
      // ---- beta, backwards ----
      float beta[K];
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int s = K * lane + k;
        beta[k] = (s == S - 1 || s == S - 2) ? 0.f : UC_NINF;
      }
      float ce[UC_PF][K], ne[UC_PF][K];                         // the emissions of step t + 1 for the steps t = t0 - u
#pragma unroll
      for (int u = 0; u < UC_PF; ++u) {
        const int t = nT - 1 - u;
#pragma unroll
        for (int k = 0; k < K; ++k) ce[u][k] = (live[k] && t >= 0 && t + 1 < nT) ? x[(long)(t + 1) * V + ext[k]] : 0.f;
      }
      for (int t0 = nT - 1; t0 >= 0; t0 -= UC_PF) {
#pragma unroll
        for (int u = 0; u < UC_PF; ++u) {
          const int t = t0 - UC_PF - u;
#pragma unroll
          for (int k = 0; k < K; ++k) ne[u][k] = (live[k] && t >= 0) ? x[(long)(t + 1) * V + ext[k]] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < UC_PF; ++u) {
          const int t = t0 - u;
          if (t >= 0) {                                         // (uniform)
            if (t + 1 < nT) {                                   // (uniform)
              const float z = s_lse[t + 1];
              float c[K];
#pragma unroll
              for (int k = 0; k < K; ++k) c[k] = (ce[u][k] - z) + beta[k];       // dead states: -inf
              const float dn = dx_wave_shl1(c[0], UC_NINF);     // state K (lane + 1)
              const float dn2 = K >= 2 ? dx_wave_shl1(c[K >= 2 ? 1 : 0], UC_NINF) : dx_wave_shl1(dn, UC_NINF);   // state K (lane + 1) + 1
#pragma unroll
              for (int k = 0; k < K; ++k) {
                const float n1 = k < K - 1 ? c[k < K - 1 ? k + 1 : 0] : dn;
                const float n2 = k < K - 2 ? c[k < K - 2 ? k + 2 : 0] : (k == K - 2 ? dn : dn2);
                beta[k] = live[k] ? uc_lse3(c[k], n1, skipf[k] ? n2 : UC_NINF) : UC_NINF;
              }
            }
#pragma unroll
            for (int k = 0; k < K; ++k)
              if (live[k]) be[(long)t * Sld + K * lane + k] = beta[k];
          }
        }
#pragma unroll
        for (int u = 0; u < UC_PF; ++u)
#pragma unroll
          for (int k = 0; k < K; ++k) ce[u][k] = ne[u][k];
      }
    }
  }
  __threadfence_block();                                        // the planes, written by two waves, are read by all four
  __syncthreads();

  // ---- the posteriors and the gradient: wave `wave` takes the steps t0 .. t0 + UC_PF - 1 of every UC_WAVES-th chunk ----
  const float ll = s_ll, wb = w[b];
  int cnt[2], start[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) { cnt[h] = s_cnt[lane + 64 * h]; start[h] = s_start[lane + 64 * h]; }
  for (int t0 = UC_PF * wave; t0 < nT; t0 += UC_PF * UC_WAVES) {
#pragma unroll
    for (int u = 0; u < UC_PF; ++u) {
      const int t = t0 + u;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int s = lane + 64 * k;                            // (any assignment of states to lanes: gamma has no neighbours)
        const bool in = t < nT && s < S;
        s_gam[wave][u][s] = in ? expf((al[(long)(in ? t : 0) * Sld + (in ? s : 0)] + be[(long)(in ? t : 0) * Sld + (in ? s : 0)]) - ll) : 0.f;
      }
    }
    uc_wave_sync();
    // the blank = the even states: lane i adds the states 2 i, 2 (i + 64), 2 (i + 128), 2 (i + 192) in this order, then the butterfly
    float blank[UC_PF];
#pragma unroll
    for (int u = 0; u < UC_PF; ++u) {
      float p = 0.f;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int s = 2 * (lane + 64 * q);
        if (q == 0) p = s < SK ? s_gam[wave][u][s < SK ? s : 0] : 0.f;
        else if (s < SK) p += s_gam[wave][u][s < SK ? s : 0];
      }
      blank[u] = p;
    }
#pragma unroll
    for (int u = 0; u < UC_PF; ++u) blank[u] = dx_wave_sum(blank[u]);
#pragma unroll
    for (int u = 0; u < UC_PF; ++u) {
      const int t = t0 + u;
      if (t < nT) {                                             // (uniform)
        const float z = s_lse[t];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int v = lane + 64 * h;
          if (v < V) {
            float post = 0.f;
            if (v == 0) post = blank[u];
            else
              for (int j = 0; j < cnt[h]; ++j) post += s_gam[wave][u][2 * (int)s_list[start[h] + j] + 1];
            g[(long)t * V + v] = wb * (expf(x[(long)t * V + v] - z) - post);
          }
        }
      }
    }
    uc_wave_sync();                                             // the next chunk rewrites s_gam[wave]
  }
  for (long i = (long)nT * V + tid; i < (long)T * V; i += UC_THREADS) g[i] = 0.f;
}

__global__ __launch_bounds__(UC_THREADS) void uctc_greedy_kernel(const float* __restrict__ logits, const int64_t* __restrict__ n_steps,
                                                                 int* __restrict__ ids, int* __restrict__ n_out, float* __restrict__ score,
                                                                 int T, int V) {
  __shared__ unsigned char s_path[UC_MAX_T];
  __shared__ float s_sc[UC_MAX_T];                              // max_v lp(t, v) of every step
  __shared__ int s_base;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int b = blockIdx.x;
  const int nT = (int)dx_clamp_len(n_steps, b, T);
  const float* x = logits + (long)b * T * V;
  for (int t0 = 4 * wave; t0 < nT; t0 += 4 * UC_WAVES) {
    float xa[4], xb[4], bv[4], m[4], sum[4];
    int bi[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool in = t0 + j < nT;
      xa[j] = (in && lane < V) ? x[(long)(t0 + j) * V + lane] : UC_NINF;
      xb[j] = (in && lane + 64 < V) ? x[(long)(t0 + j) * V + lane + 64] : UC_NINF;
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
      if (lane == 0 && t0 + j < nT) {
        s_sc[t0 + j] = -logf(sum[j]);                           // max_v x - lse = -log(sum_v exp(x - max))
        s_path[t0 + j] = (unsigned char)(bi[j] < V ? bi[j] : 0);
      }
  }
  __syncthreads();
  if (wave == 0) {
    float sc = 0.f;
    for (int t = 0; t < nT; ++t) sc += s_sc[t];                 // in order of t (every lane the same sum: an LDS broadcast per step)
    int base = 0;
    for (int c = 0; c * 64 < nT; ++c) {
      const int t = c * 64 + lane;
      const int p = t < nT ? s_path[t] : 0;
      const int prev = (t > 0 && t < nT) ? s_path[t - 1] : 0;
      const bool keep = p != 0 && p != prev;                    // a new non-blank symbol (step 0: anything but blank)
      const unsigned long long mask = __ballot(keep);
      if (keep) ids[(long)b * T + base + __popcll(mask & ((1ull << lane) - 1ull))] = p;
      base += __popcll(mask);
    }
    if (lane == 0) { n_out[b] = base; score[b] = sc; s_base = base; }
  }
  __syncthreads();
  for (int t = s_base + tid; t < T; t += UC_THREADS) ids[(long)b * T + t] = 0;
}

// a cell of the edit lattice: substitutions in the low half, deletions in the high half
__device__ __forceinline__ int ed_cost(unsigned cell, int i, int j) { return (int)(cell & 0xffffu) + 2 * (int)(cell >> 16) + j - i; }

__global__ __launch_bounds__(ED_THREADS) void edit_distance_kernel(const int* __restrict__ ref, const int64_t* __restrict__ n_ref,
                                                                   const int* __restrict__ hyp, const int64_t* __restrict__ n_hyp,
                                                                   int* __restrict__ counts, int R, int H) {
  __shared__ unsigned s_D[3][ED_MAX_LEN + 1];                   // diagonals s, s - 1, s - 2 of the cells (i, s - i), by i
  __shared__ int s_ref[ED_MAX_LEN], s_hyp[ED_MAX_LEN];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int nr = (int)dx_clamp_len(n_ref, b, R), nh = (int)dx_clamp_len(n_hyp, b, H);
  for (int i = tid; i < nr; i += ED_THREADS) s_ref[i] = ref[(long)b * R + i];
  for (int j = tid; j < nh; j += ED_THREADS) s_hyp[j] = hyp[(long)b * H + j];
  __syncthreads();
  for (int s = 0; s <= nr + nh; ++s) {
    unsigned* cur = s_D[s % 3];
    const unsigned* prev1 = s_D[(s + 2) % 3];
    const unsigned* prev2 = s_D[(s + 1) % 3];
    const int ilo = max(0, s - nh), ihi = min(s, nr);
    for (int i = ilo + tid; i <= ihi; i += ED_THREADS) {
      const int j = s - i;
      unsigned best;
      if (j == 0) {
        best = (unsigned)i << 16;                               // i deletions ((0, 0): nothing)
      } else if (i == 0) {
        best = 0u;                                              // j insertions
      } else {
        best = prev2[i - 1] + (s_ref[i - 1] == s_hyp[j - 1] ? 0u : 1u);          // diagonal: a match or a substitution
        int cost = ed_cost(best, i, j);
        const unsigned del = prev1[i - 1] + (1u << 16), ins = prev1[i];          // (i - 1, j) -> (i, j);  (i, j - 1) -> (i, j)
        if (ed_cost(del, i, j) < cost) { best = del; cost = ed_cost(del, i, j); }
        if (ed_cost(ins, i, j) < cost) best = ins;
      }
      cur[i] = best;
    }
    __syncthreads();                                            // diagonal s complete; buffer (s + 1) % 3 free to overwrite
  }
  if (tid == 0) {
    const unsigned cell = s_D[(nr + nh) % 3][nr];
    const int sub = (int)(cell & 0xffffu), del = (int)(cell >> 16);
    counts[4 * b] = sub;
    counts[4 * b + 1] = del;
    counts[4 * b + 2] = nh - nr + del;
    counts[4 * b + 3] = nr - sub - del;
  }
}

}  // namespace

extern "C" long dx_uctc_max_steps(void) { return UC_MAX_T; }
extern "C" long dx_uctc_max_labels(void) { return UC_MAX_U; }
extern "C" long dx_uctc_max_classes(void) { return UC_MAX_V; }
extern "C" long dx_edit_max_len(void) { return ED_MAX_LEN; }

extern "C" int dx_uctc_loss(const float* logits, const int64_t* n_steps, const int64_t* labels, const int64_t* n_labels, const float* w,
                            float* loss, int* status, float* grad, float* ws, int B, int T, int U, int V, void* stream) {
  DX_REQUIRE(logits && n_steps && n_labels && w && loss && status && grad && ws && (labels || U == 0), DX_ERR_ARG,
             "dx_uctc_loss: null pointer");
  DX_REQUIRE(B > 0 && T > 0 && U >= 0 && V > 0, DX_ERR_SHAPE, "dx_uctc_loss: bad shape B=%d T=%d U=%d V=%d", B, T, U, V);
  DX_REQUIRE(T <= UC_MAX_T && U <= UC_MAX_U && V <= UC_MAX_V && B <= 65535, DX_ERR_UNSUPPORTED,
             "dx_uctc_loss: T=%d steps (at most %d), U=%d labels (at most %d), V=%d classes (at most %d) or B=%d > 65535", T, UC_MAX_T, U,
             UC_MAX_U, V, UC_MAX_V, B);
  const int S = 2 * U + 1;
  const dim3 grid(B), block(UC_THREADS);
  if (S <= 64)
    hipLaunchKernelGGL(uctc_loss_kernel<1>, grid, block, 0, (hipStream_t)stream, logits, n_steps, labels, n_labels, w, loss, status, grad,
                       ws, B, T, U, V);
  else if (S <= 128)
    hipLaunchKernelGGL(uctc_loss_kernel<2>, grid, block, 0, (hipStream_t)stream, logits, n_steps, labels, n_labels, w, loss, status, grad,
                       ws, B, T, U, V);
  else if (S <= 256)
    hipLaunchKernelGGL(uctc_loss_kernel<4>, grid, block, 0, (hipStream_t)stream, logits, n_steps, labels, n_labels, w, loss, status, grad,
                       ws, B, T, U, V);
  else
    hipLaunchKernelGGL(uctc_loss_kernel<8>, grid, block, 0, (hipStream_t)stream, logits, n_steps, labels, n_labels, w, loss, status, grad,
                       ws, B, T, U, V);
  DX_LAUNCH_CHECK();
  return DX_OK;
}

extern "C" int dx_uctc_greedy(const float* logits, const int64_t* n_steps, int* ids, int* n_out, float* score, int B, int T, int V,
                              void* stream) {
  DX_REQUIRE(logits && n_steps && ids && n_out && score, DX_ERR_ARG, "dx_uctc_greedy: null pointer");
  DX_REQUIRE(B > 0 && T > 0 && V > 0, DX_ERR_SHAPE, "dx_uctc_greedy: bad shape B=%d T=%d V=%d", B, T, V);
  DX_REQUIRE(T <= UC_MAX_T && V <= UC_MAX_V && B <= 65535, DX_ERR_UNSUPPORTED,
             "dx_uctc_greedy: T=%d steps (at most %d), V=%d classes (at most %d) or B=%d > 65535", T, UC_MAX_T, V, UC_MAX_V, B);
  hipLaunchKernelGGL(uctc_greedy_kernel, dim3(B), dim3(UC_THREADS), 0, (hipStream_t)stream, logits, n_steps, ids, n_out, score, T, V);
  DX_LAUNCH_CHECK();
  return DX_OK;
}

extern "C" int dx_edit_distance(const int* ref, const int64_t* n_ref, const int* hyp, const int64_t* n_hyp, int* counts, int B, int R, int H,
                                void* stream) {
  DX_REQUIRE(n_ref && n_hyp && counts && (ref || R == 0) && (hyp || H == 0), DX_ERR_ARG, "dx_edit_distance: null pointer");
  DX_REQUIRE(B > 0 && R >= 0 && H >= 0, DX_ERR_SHAPE, "dx_edit_distance: bad shape B=%d R=%d H=%d", B, R, H);
  DX_REQUIRE(R <= ED_MAX_LEN && H <= ED_MAX_LEN && B <= 65535, DX_ERR_UNSUPPORTED,
             "dx_edit_distance: sequences of R=%d, H=%d entries (at most %d: three anti-diagonals live in LDS) or B=%d > 65535", R, H,
             ED_MAX_LEN, B);
  hipLaunchKernelGGL(edit_distance_kernel, dim3(B), dim3(ED_THREADS), 0, (hipStream_t)stream, ref, n_ref, hyp, n_hyp, counts, R, H);
  DX_LAUNCH_CHECK();
  return DX_OK;
}
