// K25: copy-synthesis scores -- mel-cepstral distortion, F0 error and voicing error between a recording and a synthesis of the
// same text, after dynamic time warping of their mel cepstra.  Three kernels: the cepstrum (a DCT over the mel axis), the DTW
// itself (one workgroup per pair walks the anti-diagonals of the cost matrix) and the reduction of the scores along the path.
//
// The DTW keeps three anti-diagonals of the accumulated cost D in LDS, indexed by the reference frame i: the cells of diagonal
// s = i + j depend on D(i - 1, j - 1) = diag[s - 2][i - 1], D(i - 1, j) = diag[s - 1][i - 1] and D(i, j - 1) = diag[s - 1][i], so one
// barrier per diagonal orders everything.  The local cost is computed on the fly from the two cepstra (read through L1 / L2);
// the only thing that goes to memory per cell is its 2-bit predecessor code.  Four codes (i, 4 q .. 4 q + 3) share a byte: the byte
// in progress of every row i lives in LDS and is stored when its last cell is done, so no two threads ever write one byte.
// Every sum and every comparison runs in an order fixed by the pair's own lengths: a pair's result does not depend on its batch.
#include "dx_common.h"

namespace {

constexpr int DTW_MAX_LEN = 4096;      // longest sequence; LDS: 3 diagonals of 4096 floats + 4096 code bytes + 4 = 53 252 B: three workgroups per CU
constexpr int DTW_THREADS = 256;
constexpr int DTW_WAVES = DTW_THREADS / 64;
constexpr int CEP_THREADS = 256;
constexpr int CEP_MAX_TABLE = 4096;    // floats of the DCT table staged in LDS (K * n_mel): 16 KiB
constexpr int CEP_KT = 8;              // coefficients accumulated per pass over the mel axis

// d(i, j): the terms in order of k, each one fused multiply-add, one correctly rounded square root
__device__ __forceinline__ float dtw_dist(const float* __restrict__ r, const float* __restrict__ g, int K) {
  float acc = 0.f;
  for (int k = 0; k < K; ++k) { const float t = r[k] - g[k]; acc = fmaf(t, t, acc); }
  return sqrtf(acc);
}

// ---- cepstrum: cep[b, t, k] = sum_m dct[k, m] * mel[b, m, t], t < n[b]; zeros behind ------------------------------------------
__global__ __launch_bounds__(CEP_THREADS) void mel_cepstrum_kernel(const float* __restrict__ mel, long ld_b, long ld_m,
                                                                   const int64_t* __restrict__ n, const float* __restrict__ dct,
                                                                   float* __restrict__ cep, int n_mel, int T, int K) {
  __shared__ float s_dct[CEP_MAX_TABLE];
  const int b = blockIdx.y, t = blockIdx.x * CEP_THREADS + threadIdx.x;
  for (int e = threadIdx.x; e < K * n_mel; e += CEP_THREADS) s_dct[e] = dct[e];
  __syncthreads();
  if (t >= T) return;
  float* out = cep + ((long)b * T + t) * K;
  if (t >= (int)dx_clamp_len(n, b, T)) {
    for (int k = 0; k < K; ++k) out[k] = 0.f;
    return;
  }
  const float* x = mel + (long)b * ld_b + t;
  for (int k0 = 0; k0 < K; k0 += CEP_KT) {
    float acc[CEP_KT];
#pragma unroll
    for (int u = 0; u < CEP_KT; ++u) acc[u] = 0.f;
    for (int m = 0; m < n_mel; ++m) {
      const float v = x[(long)m * ld_m];
#pragma unroll
      for (int u = 0; u < CEP_KT; ++u) acc[u] = fmaf(s_dct[min(k0 + u, K - 1) * n_mel + m], v, acc[u]);
    }
#pragma unroll
    for (int u = 0; u < CEP_KT; ++u) if (k0 + u < K) out[k0 + u] = acc[u];
  }
}

// ---- DTW: forward pass over the anti-diagonals, backtrack, path in forward order ---------------------------------------------
__global__ __launch_bounds__(DTW_THREADS) void dtw_align_kernel(const float* __restrict__ cep_ref, const int64_t* __restrict__ n_ref,
                                                                const float* __restrict__ cep_gen, const int64_t* __restrict__ n_gen,
                                                                float* __restrict__ total, int* __restrict__ path, int* __restrict__ path_len,
                                                                unsigned char* ws, long ws_stride, int T_ref, int T_gen, int K) {
  __shared__ float s_D[3 * DTW_MAX_LEN];                        // diagonals s, s - 1, s - 2 by reference frame; the path afterwards
  __shared__ unsigned char s_code[DTW_MAX_LEN];                 // per reference frame: the code byte in progress
  __shared__ int s_len;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int nr = (int)dx_clamp_len(n_ref, b, T_ref), nd = (int)dx_clamp_len(n_gen, b, T_gen);
  const int P = T_ref + T_gen - 1;
  int* out = path + (long)b * P * 2;
  if (nr == 0 || nd == 0) {                                     // (uniform over the workgroup)
    if (tid == 0) { total[b] = __builtin_nanf(""); path_len[b] = 0; }
    for (int p = tid; p < 2 * P; p += DTW_THREADS) out[p] = -1;
    return;
  }
  const float* R = cep_ref + (long)b * T_ref * K;
  const float* G = cep_gen + (long)b * T_gen * K;
  unsigned char* W = ws + (long)b * ws_stride;
  const int row_bytes = (nd + 3) >> 2;                          // the pair's own extent: nr * row_bytes <= ws_stride

  const int last = nr + nd - 2;
  for (int s = 0; s <= last; ++s) {
    float* cur = s_D + (s % 3) * DTW_MAX_LEN;
    const float* prev1 = s_D + ((s + 2) % 3) * DTW_MAX_LEN;
    const float* prev2 = s_D + ((s + 1) % 3) * DTW_MAX_LEN;
    const int ilo = max(0, s - (nd - 1)), ihi = min(s, nr - 1);
    for (int i = ilo + tid; i <= ihi; i += DTW_THREADS) {
      const int j = s - i;
      const float d = dtw_dist(R + (long)i * K, G + (long)j * K, K);
      float best = 0.f;
      unsigned code = 0u;                                       // 0 diagonal, 1 (i - 1, j), 2 (i, j - 1): the first minimum in that order
      if (i > 0 && j > 0) {
        best = prev2[i - 1];
        const float up = prev1[i - 1], left = prev1[i];
        if (up < best) { best = up; code = 1u; }
        if (left < best) { best = left; code = 2u; }
      } else if (i > 0) {
        best = prev1[i - 1]; code = 1u;
      } else if (j > 0) {
        best = prev1[i]; code = 2u;
      }
      cur[i] = d + best;
      const unsigned c = ((j & 3) ? (unsigned)s_code[i] : 0u) | (code << (2 * (j & 3)));
      s_code[i] = (unsigned char)c;
      if ((j & 3) == 3 || j == nd - 1) W[(long)i * row_bytes + (j >> 2)] = (unsigned char)c;
    }
    __syncthreads();                                            // diagonal s complete; buffer (s + 1) % 3 free to overwrite
  }

  // backtrack: one thread, at most nr + nd - 1 cells; at an edge the move is forced whatever the workspace holds
  const float D_end = s_D[(last % 3) * DTW_MAX_LEN + nr - 1];
  __syncthreads();
  unsigned* s_path = reinterpret_cast<unsigned*>(s_D);          // (i << 16 | j), backwards; 8191 entries at most
  if (tid == 0) {
    total[b] = D_end;
    int i = nr - 1, j = nd - 1, len = 0;
    const int cap = nr + nd - 1;
    for (;;) {
      s_path[len++] = ((unsigned)i << 16) | (unsigned)j;
      if ((i == 0 && j == 0) || len >= cap) break;
      const unsigned code = i == 0 ? 2u : j == 0 ? 1u : ((unsigned)W[(long)i * row_bytes + (j >> 2)] >> (2 * (j & 3))) & 3u;
      if (code == 1u) --i; else if (code == 2u) --j; else { --i; --j; }
    }
    s_len = len;
    path_len[b] = len;
  }
  __syncthreads();
  const int len = s_len;
  for (int p = tid; p < P; p += DTW_THREADS) {
    int pi = -1, pj = -1;
    if (p < len) { const unsigned e = s_path[len - 1 - p]; pi = (int)(e >> 16); pj = (int)(e & 0xffffu); }
    out[2 * p] = pi; out[2 * p + 1] = pj;
  }
}

// ---- scores along a path --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DTW_THREADS) void dtw_path_scores_kernel(const float* __restrict__ cep_ref, const int64_t* __restrict__ n_ref,
                                                                      const float* __restrict__ cep_gen, const int64_t* __restrict__ n_gen,
                                                                      const int* __restrict__ path, const int* __restrict__ path_len,
                                                                      const float* __restrict__ lp_ref, long ld_lpr,
                                                                      const float* __restrict__ lp_gen, long ld_lpg,
                                                                      float* __restrict__ mcd_db, float* __restrict__ f0_rmse_cents,
                                                                      float* __restrict__ vuv_error, int* __restrict__ voiced_pairs,
                                                                      int* __restrict__ used_len, int T_ref, int T_gen, int K) {
  __shared__ double s_red[DTW_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int nr = (int)dx_clamp_len(n_ref, b, T_ref), nd = (int)dx_clamp_len(n_gen, b, T_gen);
  const int P = T_ref + T_gen - 1;
  const int len = min(max(path_len[b], 0), P);
  const int* pp = path + (long)b * P * 2;
  const float* R = cep_ref + (long)b * T_ref * K;
  const float* G = cep_gen + (long)b * T_gen * K;
  const bool pitch = lp_ref != nullptr && lp_gen != nullptr;
  double sd = 0.0, sq = 0.0, cnt = 0.0, both = 0.0, one = 0.0;
  for (int p = tid; p < len; p += DTW_THREADS) {
    const int i = pp[2 * p], j = pp[2 * p + 1];
    if (i < 0 || i >= nr || j < 0 || j >= nd) continue;         // not a cell of this pair: never read, never counted
    cnt += 1.0;
    sd += (double)dtw_dist(R + (long)i * K, G + (long)j * K, K);
    if (pitch) {
      const float a = lp_ref[(long)b * ld_lpr + i], g = lp_gen[(long)b * ld_lpg + j];
      const bool va = a > 0.f, vg = g > 0.f;
      if (va && vg) {
        const double c = (1200.0 / 0.693147180559945309417) * ((double)a - (double)g);
        sq = fma(c, c, sq);
        both += 1.0;
      } else if (va != vg) {
        one += 1.0;
      }
    }
  }
  sd = dx_block_sum<DTW_WAVES>(sd, s_red); cnt = dx_block_sum<DTW_WAVES>(cnt, s_red);
  sq = dx_block_sum<DTW_WAVES>(sq, s_red); both = dx_block_sum<DTW_WAVES>(both, s_red); one = dx_block_sum<DTW_WAVES>(one, s_red);
  if (tid == 0) {
    const float nan = __builtin_nanf("");
    const double scale = 10.0 * 1.41421356237309504880 / 2.30258509299404568402;      // 10 sqrt(2) / ln 10
    used_len[b] = (int)cnt;
    mcd_db[b] = cnt > 0.0 ? (float)(scale * (sd / cnt)) : nan;
    f0_rmse_cents[b] = (pitch && both > 0.0) ? (float)sqrt(sq / both) : nan;
    vuv_error[b] = (pitch && cnt > 0.0) ? (float)(one / cnt) : nan;
    voiced_pairs[b] = (int)both;
  }
}

}  // namespace

extern "C" long dx_dtw_max_len(void) { return DTW_MAX_LEN; }

extern "C" int dx_mel_cepstrum(const float* mel, long ld_b, long ld_m, const int64_t* n, const float* dct, float* cep, int B, int n_mel,
                               int T, int K, void* stream) {
  DX_REQUIRE(mel && n && dct && cep, DX_ERR_ARG, "dx_mel_cepstrum: null pointer");
  DX_REQUIRE(B > 0 && T > 0 && n_mel > 1 && K >= 1 && K < n_mel && ld_m >= T && (B == 1 || ld_b >= ld_m * (n_mel - 1) + T), DX_ERR_SHAPE,
             "dx_mel_cepstrum: bad shape B=%d n_mel=%d T=%d K=%d (1 <= K < n_mel) ld_b=%ld ld_m=%ld", B, n_mel, T, K, ld_b, ld_m);
  DX_REQUIRE((long)K * n_mel <= CEP_MAX_TABLE && B <= 65535, DX_ERR_UNSUPPORTED,
             "dx_mel_cepstrum: K * n_mel = %ld table entries (at most %d are staged in LDS) or B=%d > 65535", (long)K * n_mel,
             CEP_MAX_TABLE, B);
  hipLaunchKernelGGL(mel_cepstrum_kernel, dim3(dx_cdiv(T, CEP_THREADS), B), dim3(CEP_THREADS), 0, (hipStream_t)stream, mel, ld_b, ld_m, n,
                     dct, cep, n_mel, T, K);
  DX_LAUNCH_CHECK();
  return DX_OK;
}

extern "C" int dx_dtw_align(const float* cep_ref, const int64_t* n_ref, const float* cep_gen, const int64_t* n_gen, float* total,
                            int* path, int* path_len, void* ws, long ws_stride, int B, int T_ref, int T_gen, int K, void* stream) {
  DX_REQUIRE(cep_ref && n_ref && cep_gen && n_gen && total && path && path_len && ws, DX_ERR_ARG, "dx_dtw_align: null pointer");
  DX_REQUIRE(B > 0 && T_ref > 0 && T_gen > 0 && K >= 1, DX_ERR_SHAPE, "dx_dtw_align: bad shape B=%d T_ref=%d T_gen=%d K=%d", B, T_ref,
             T_gen, K);
  DX_REQUIRE(T_ref <= DTW_MAX_LEN && T_gen <= DTW_MAX_LEN, DX_ERR_UNSUPPORTED,
             "dx_dtw_align: sequences of T_ref=%d, T_gen=%d frames (at most %d: three anti-diagonals live in LDS)", T_ref, T_gen,
             DTW_MAX_LEN);
  DX_REQUIRE(ws_stride >= (long)T_ref * ((T_gen + 3) / 4), DX_ERR_SHAPE,
             "dx_dtw_align: ws_stride=%ld bytes per pair, T_ref * ceil(T_gen / 4) = %ld needed", ws_stride, (long)T_ref * ((T_gen + 3) / 4));
  hipLaunchKernelGGL(dtw_align_kernel, dim3(B), dim3(DTW_THREADS), 0, (hipStream_t)stream, cep_ref, n_ref, cep_gen, n_gen, total, path,
                     path_len, (unsigned char*)ws, ws_stride, T_ref, T_gen, K);
  DX_LAUNCH_CHECK();
  return DX_OK;
}

extern "C" int dx_dtw_path_scores(const float* cep_ref, const int64_t* n_ref, const float* cep_gen, const int64_t* n_gen, const int* path,
                                  const int* path_len, const float* lp_ref, long ld_lpr, const float* lp_gen, long ld_lpg, float* mcd_db,
                                  float* f0_rmse_cents, float* vuv_error, int* voiced_pairs, int* used_len, int B, int T_ref, int T_gen,
                                  int K, void* stream) {
  DX_REQUIRE(cep_ref && n_ref && cep_gen && n_gen && path && path_len && mcd_db && f0_rmse_cents && vuv_error && voiced_pairs && used_len,
             DX_ERR_ARG, "dx_dtw_path_scores: null pointer");
  DX_REQUIRE(B > 0 && T_ref > 0 && T_gen > 0 && K >= 1 && (!lp_ref || B == 1 || ld_lpr >= T_ref) &&
                 (!lp_gen || B == 1 || ld_lpg >= T_gen),
             DX_ERR_SHAPE,
             "dx_dtw_path_scores: bad shape B=%d T_ref=%d T_gen=%d K=%d ld_lpr=%ld ld_lpg=%ld", B, T_ref, T_gen, K, ld_lpr, ld_lpg);
  DX_REQUIRE(T_ref <= DTW_MAX_LEN && T_gen <= DTW_MAX_LEN, DX_ERR_UNSUPPORTED,
             "dx_dtw_path_scores: sequences of T_ref=%d, T_gen=%d frames (at most %d)", T_ref, T_gen, DTW_MAX_LEN);
  hipLaunchKernelGGL(dtw_path_scores_kernel, dim3(B), dim3(DTW_THREADS), 0, (hipStream_t)stream, cep_ref, n_ref, cep_gen, n_gen, path,
                     path_len, lp_ref, ld_lpr, lp_gen, ld_lpg, mcd_db, f0_rmse_cents, vuv_error, voiced_pairs, used_len, T_ref, T_gen, K);
  DX_LAUNCH_CHECK();
  return DX_OK;
}
