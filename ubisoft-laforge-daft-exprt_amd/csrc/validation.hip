// K23: the numbers behind the validation figures (logger.py:34-157), reduced on the device batch by batch so that only small results
// reach the host: the 50-bin histograms of the FiLM gammas / betas per block (logger.py:100-126 through utils.py:18-36) and, per
// utterance, how closely the Gaussian upsampler's alignment follows the integer durations it was teacher-forced with (the content of
// the "alignments" figure, logger.py:81-98, 154-157).
//
// Histogram bins are decided by comparisons in double against the caller's edge table and counted with integer atomics (LDS per
// workgroup, then one 64-bit global add per bin): the counts depend neither on the launch geometry nor on any floating-point rounding.
#include "dx_common.h"

namespace {

constexpr int VR_THREADS = 256;
constexpr int VR_WAVES = VR_THREADS / 64;
constexpr int VR_BINS = 50;                 // histogram_plot(..., bins=50), utils.py:18
constexpr int VR_MAX_SYMBOLS = 8192;        // alignment score: prefix sums of one utterance in LDS (32 KB + 4 B)

// element i of group (blk, half h) of film (rows, nb_blocks, width): row i / hw, column h * hw + i % hw
__device__ __forceinline__ float film_value(const float* __restrict__ film, long i, int blk, int h, int nb_blocks, int width) {
  const int hw = width / 2;
  const long r = i / hw;
  const int c = (int)(i - r * hw);
  return film[(r * nb_blocks + blk) * (long)width + h * hw + c];
}

// one workgroup per group: min, max and whether every value is finite
__global__ __launch_bounds__(VR_THREADS) void film_range_kernel(const float* __restrict__ film, float* __restrict__ minmax,
                                                                int* __restrict__ finite, long rows, int nb_blocks, int width) {
  __shared__ float s_lo[VR_WAVES], s_hi[VR_WAVES];
  __shared__ int s_bad[VR_WAVES];
  const int g = blockIdx.x, blk = g >> 1, h = g & 1, tid = threadIdx.x;
  const long n = rows * (width / 2);
  float lo = __builtin_inff(), hi = -__builtin_inff();
  int bad = 0;
  for (long i = tid; i < n; i += VR_THREADS) {
    const float x = film_value(film, i, blk, h, nb_blocks, width);
    if (isfinite(x)) { lo = fminf(lo, x); hi = fmaxf(hi, x); } else bad = 1;
  }
  lo = dx_wave_min(lo); hi = dx_wave_max(hi); bad = __ballot(bad) != 0;
  if ((tid & 63) == 0) { s_lo[tid >> 6] = lo; s_hi[tid >> 6] = hi; s_bad[tid >> 6] = bad; }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < VR_WAVES; ++w) { lo = fminf(lo, s_lo[w]); hi = fmaxf(hi, s_hi[w]); bad |= s_bad[w]; }
    minmax[2 * g] = bad ? 0.f : lo;
    minmax[2 * g + 1] = bad ? 0.f : hi;
    finite[g] = !bad;
  }
}

// grid (workgroups per group, G); counts must be zero on entry.  A group whose finite flag is 0 is left at zero.
__global__ __launch_bounds__(VR_THREADS) void film_count_kernel(const float* __restrict__ film, const double* __restrict__ edges,
                                                                const int* __restrict__ finite, unsigned long long* __restrict__ counts,
                                                                long rows, int nb_blocks, int width) {
  __shared__ double s_e[VR_BINS + 1];
  __shared__ unsigned int s_cnt[VR_BINS];
  const int g = blockIdx.y, blk = g >> 1, h = g & 1, tid = threadIdx.x;
  if (!finite[g]) return;                                        // (uniform over the workgroup)
  if (tid <= VR_BINS) s_e[tid] = edges[(long)g * (VR_BINS + 1) + tid];
  if (tid < VR_BINS) s_cnt[tid] = 0u;
  __syncthreads();
  const double e0 = s_e[0], e1 = s_e[VR_BINS];
  const float scale = (float)((double)VR_BINS / (e1 - e0));      // seeds the search only; inf / NaN for a degenerate table is clamped below
  const long n = rows * (width / 2);
  for (long i = (long)blockIdx.x * VR_THREADS + tid; i < n; i += (long)gridDim.x * VR_THREADS) {
    const double x = (double)film_value(film, i, blk, h, nb_blocks, width);
    if (!(x >= e0 && x <= e1)) continue;                         // outside the table (or NaN): numpy.histogram drops it too
    const float est = ((float)x - (float)e0) * scale;
    int k = est > 0.f ? (est < (float)(VR_BINS - 1) ? (int)est : VR_BINS - 1) : 0;
    while (k > 0 && x < s_e[k]) --k;                             // the table decides: e[k] <= x < e[k + 1], the last bin closed
    while (k < VR_BINS - 1 && x >= s_e[k + 1]) ++k;
    atomicAdd(&s_cnt[k], 1u);
  }
  __syncthreads();
  if (tid < VR_BINS && s_cnt[tid]) atomicAdd(&counts[(long)g * VR_BINS + tid], (unsigned long long)s_cnt[tid]);
}

// one workgroup per utterance; dynamic LDS: (L + 1) ints, s_cum[l] = min(sum_{j < l} d_j, T_b) with d_j = 0 for j >= in_lengths[b]
__global__ __launch_bounds__(VR_THREADS) void alignment_score_kernel(const float* __restrict__ weights, const int64_t* __restrict__ durations,
                                                                     const int64_t* __restrict__ in_lengths, const int64_t* __restrict__ out_lengths,
                                                                     int64_t* __restrict__ frames, int64_t* __restrict__ hits,
                                                                     float* __restrict__ mass, int L, int T) {
  extern __shared__ int s_cum[];
  __shared__ long s_part[VR_WAVES];
  __shared__ double s_red[VR_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int Lb = (int)dx_clamp_len(in_lengths, b, L);
  const long Tb = dx_clamp_len(out_lengths, b, T);
  const int64_t* d = durations + (long)b * L;

  // exact prefix sums, a chunk of VR_THREADS symbols at a time; every term is clamped to [0, Tb] first, so a long never overflows
  long carry = 0;
  for (int l0 = 0; l0 < L; l0 += VR_THREADS) {
    const int l = l0 + tid;
    const long before = dx_block_scan_step<VR_WAVES>(l < Lb ? dx_clamp_len(d, l, Tb) : 0L, carry, s_part);
    if (l < L) s_cum[l] = (int)min(before, Tb);
    __syncthreads();
  }
  if (tid == 0) s_cum[L] = (int)min(carry, Tb);
  __syncthreads();
  const int owned = s_cum[L];

  const float* w = weights + (long)b * L * T;
  long hit = 0;
  double sum = 0.0;
  for (int t = tid; t < owned; t += VR_THREADS) {                // lanes walk along T: every load of the l loop is coalesced
    const int lo = dx_locate_item(s_cum, Lb, t);                 // owner: the largest l with s_cum[l] <= t (symbols without frames are skipped)
    float best = w[t], at_owner = best;
    int arg = 0;
    for (int l = 1; l < Lb; ++l) {
      const float v = w[(long)l * T + t];
      if (l == lo) at_owner = v;
      if (v > best) { best = v; arg = l; }                       // strict: the lowest index of equal maxima wins
    }
    hit += arg == lo;
    sum += (double)at_owner;
  }
  const double tot = dx_block_sum<VR_WAVES>(sum, s_red), nhit = dx_block_sum<VR_WAVES>((double)hit, s_red);   // (counts below 2^31 are exact in a double)
  if (tid == 0) {
    frames[b] = owned;
    hits[b] = (int64_t)nhit;
    mass[b] = owned > 0 ? (float)(tot / (double)owned) : 0.f;
  }
}

}  // namespace

extern "C" int dx_film_hist_range(const float* film, float* minmax, int* finite, long rows, int nb_blocks, int width, void* stream) {
  DX_REQUIRE(film && minmax && finite, DX_ERR_ARG, "dx_film_hist_range: null pointer");
  DX_REQUIRE(rows > 0 && nb_blocks > 0 && width >= 2 && width % 2 == 0 && nb_blocks <= 32767, DX_ERR_SHAPE,
             "dx_film_hist_range: bad shape rows=%ld nb_blocks=%d width=%d (width = gammas + betas, even)", rows, nb_blocks, width);
  hipLaunchKernelGGL(film_range_kernel, dim3(2 * nb_blocks), dim3(VR_THREADS), 0, (hipStream_t)stream, film, minmax, finite, rows,
                     nb_blocks, width);
  DX_LAUNCH_CHECK();
  return DX_OK;
}

extern "C" int dx_film_hist_count(const float* film, const double* edges, const int* finite, int64_t* counts, long rows, int nb_blocks,
                                  int width, void* stream) {
  DX_REQUIRE(film && edges && finite && counts, DX_ERR_ARG, "dx_film_hist_count: null pointer");
  DX_REQUIRE(rows > 0 && nb_blocks > 0 && width >= 2 && width % 2 == 0 && nb_blocks <= 32767, DX_ERR_SHAPE,
             "dx_film_hist_count: bad shape rows=%ld nb_blocks=%d width=%d (width = gammas + betas, even)", rows, nb_blocks, width);
  const int G = 2 * nb_blocks;
  if (int rc = dx_fill_zero(counts, (size_t)G * VR_BINS * sizeof(int64_t), stream)) return rc;
  const long n = rows * (width / 2);
  const long per = (n + 8L * VR_THREADS - 1) / (8L * VR_THREADS);            // ~8 values per thread
  hipLaunchKernelGGL(film_count_kernel, dim3((unsigned)(per < 1 ? 1 : (per > 64 ? 64 : per)), G), dim3(VR_THREADS), 0, (hipStream_t)stream,
                     film, edges, finite, reinterpret_cast<unsigned long long*>(counts), rows, nb_blocks, width);
  DX_LAUNCH_CHECK();
  return DX_OK;
}

extern "C" int dx_alignment_score(const float* weights, const int64_t* durations_int, const int64_t* in_lengths,
                                  const int64_t* out_lengths, int64_t* frames, int64_t* hits, float* mass, int B, int L, int T,
                                  void* stream) {
  DX_REQUIRE(weights && durations_int && in_lengths && out_lengths && frames && hits && mass, DX_ERR_ARG,
             "dx_alignment_score: null pointer");
  DX_REQUIRE(B > 0 && L > 0 && T > 0, DX_ERR_SHAPE, "dx_alignment_score: bad shape B=%d L=%d T=%d", B, L, T);
  DX_REQUIRE(L <= VR_MAX_SYMBOLS, DX_ERR_UNSUPPORTED, "dx_alignment_score: L=%d symbols (the prefix sums of at most %d are kept in LDS)",
             L, VR_MAX_SYMBOLS);
  hipLaunchKernelGGL(alignment_score_kernel, dim3(B), dim3(VR_THREADS), (size_t)(L + 1) * sizeof(int), (hipStream_t)stream, weights,
                     durations_int, in_lengths, out_lengths, frames, hits, mass, L, T);
  DX_LAUNCH_CHECK();
  return DX_OK;
}
