// K22: the prosody-transfer metric (scripts/evaluation/compare_pitch_curves.py:5-45): per utterance, drop the unvoiced frames of two
// curves, Fourier-resample the generated one to the reference's length (scipy.signal.resample for real input) and take Pearson's
// correlation.  One workgroup per row; the kept curves, the twiddle table and the weighted spectrum live in LDS.
//
// The curve lengths are arbitrary (the voiced frames of an utterance), so the radix-4 FFT of dx_fft.h does not apply; the DFT and
// its inverse are direct sums, O(Nx * K) and O(num * K) with K = min(num, Nx) / 2 + 1.  The angle of term (k, n) is 2 pi (k n mod N) / N:
// the index k n mod N is advanced in integers and looked up in a table of N entries computed in double, so no float ever sees an
// unreduced angle.  Every sum runs in an order fixed by the row's own lengths: a row's result does not depend on the batch around it.
#include "dx_common.h"

namespace {

constexpr int PCC_MAX_LEN = 4096;      // longest curve (T_ref, T_dut); LDS: 2 curves + 1 float2 table + 2049 bins + scratch = 81 984 B: one workgroup per CU
constexpr int PCC_THREADS = 256;
constexpr int PCC_WAVES = PCC_THREADS / 64;

// stable compaction of src[0, n) into dst (LDS): the elements > 0 in order when `drop`, all of them otherwise.  A ballot gives a
// lane its place inside the wave, the wave totals of a 256-element chunk are combined through LDS.  Returns the kept length.
__device__ __forceinline__ int pcc_compact(const float* __restrict__ src, int n, bool drop, float* dst, int* cnt) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int base = 0;
  for (int i0 = 0; i0 < n; i0 += PCC_THREADS) {
    const int i = i0 + tid;
    const float v = i < n ? src[i] : 0.f;
    const bool keep = i < n && (!drop || v > 0.f);
    const unsigned long long m = __ballot(keep);
    if (lane == 0) cnt[wave] = __popcll(m);
    __syncthreads();
    int off = base, chunk = 0;
#pragma unroll
    for (int w = 0; w < PCC_WAVES; ++w) { const int c = cnt[w]; if (w < wave) off += c; chunk += c; }
    if (keep) dst[off + __popcll(m & ((1ull << lane) - 1ull))] = v;
    base += chunk;
    __syncthreads();
  }
  return base;
}

// tw[i] = (cos, sin)(2 pi i / N), i < N, in double, rounded once
__device__ __forceinline__ void pcc_table(float2* tw, int N) {
  for (int i = threadIdx.x; i < N; i += PCC_THREADS) {
    double s, c;
    sincospi(2.0 * (double)i / (double)N, &s, &c);
    tw[i] = make_float2((float)c, (float)s);
  }
}

__global__ __launch_bounds__(PCC_THREADS) void curve_pcc_kernel(const float* __restrict__ ref, long ld_ref, const int64_t* __restrict__ n_ref,
                                                                const float* __restrict__ dut, long ld_dut, const int64_t* __restrict__ n_dut,
                                                                float* __restrict__ pcc, int* __restrict__ kept_ref, int* __restrict__ kept_dut,
                                                                float* __restrict__ resampled, long ld_rs, int T_ref, int T_dut, int drop) {
  __shared__ float s_ref[PCC_MAX_LEN], s_dut[PCC_MAX_LEN];      // kept curves; s_dut holds the resampled curve from step 4 on
  __shared__ float2 s_tw[PCC_MAX_LEN];                          // twiddles of the length in use
  __shared__ float2 s_X[PCC_MAX_LEN / 2 + 1];                   // w_k / Nx * X[k]
  __shared__ double s_red[PCC_WAVES];
  __shared__ int s_cnt[PCC_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int nr = (int)dx_clamp_len(n_ref, b, T_ref), nd = (int)dx_clamp_len(n_dut, b, T_dut);

  // 1. unvoiced removal
  const int num = pcc_compact(ref + (long)b * ld_ref, nr, drop != 0, s_ref, s_cnt);
  const int Nx = pcc_compact(dut + (long)b * ld_dut, nd, drop != 0, s_dut, s_cnt);
  if (tid == 0) { kept_ref[b] = num; kept_dut[b] = Nx; }
  if (num == 0 || Nx == 0) {                                    // (uniform over the workgroup) nothing to resample, or to resample to
    if (tid == 0) pcc[b] = __builtin_nanf("");
    if (resampled) for (int m = tid; m < num; m += PCC_THREADS) resampled[(long)b * ld_rs + m] = __builtin_nanf("");
    return;
  }

  // 2. centre the curve to resample: the resampling is linear and maps a constant to itself, and the sums then carry the
  //    curve's variation only (a log-Hz curve is 5 +- 0.3)
  double acc = 0.0;
  for (int i = tid; i < Nx; i += PCC_THREADS) acc += (double)s_dut[i];
  const float mean_x = (float)(dx_block_sum<PCC_WAVES>(acc, s_red) / (double)Nx);
  for (int i = tid; i < Nx; i += PCC_THREADS) s_dut[i] -= mean_x;
  pcc_table(s_tw, Nx);
  __syncthreads();

  // 3. X[k] = sum_n x[n] e^{-2 pi i k n / Nx}, k <= N / 2, stored with its weight: 1 for k = 0, 2 otherwise, and for the bin
  //    N / 2 of an even N 2 when downsampling and 1 when not (scipy doubles / halves it before an irfft that counts it once / twice)
  const int N = min(num, Nx), K = N / 2 + 1;
  for (int k = tid; k < K; k += PCC_THREADS) {
    float re[4] = {0.f, 0.f, 0.f, 0.f}, im[4] = {0.f, 0.f, 0.f, 0.f};
    int idx[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) idx[j] = (j * k) % Nx;          // k, j * k < 2^14
    const int step = (4 * k) % Nx;
    for (int n0 = 0; n0 < Nx; n0 += 4) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (n0 + j < Nx) {
          const float x = s_dut[n0 + j];
          const float2 t = s_tw[idx[j]];
          re[j] = fmaf(x, t.x, re[j]);
          im[j] = fmaf(-x, t.y, im[j]);
          idx[j] += step;
          if (idx[j] >= Nx) idx[j] -= Nx;
        }
      }
    }
    float w = k == 0 ? 1.f : 2.f;
    if (k > 0 && 2 * k == N && num >= Nx) w = 1.f;
    w /= (float)Nx;
    s_X[k] = make_float2(w * ((re[0] + re[1]) + (re[2] + re[3])), w * ((im[0] + im[1]) + (im[2] + im[3])));
  }
  __syncthreads();
  pcc_table(s_tw, num);
  __syncthreads();

  // 4. y[m] = mean + sum_k Re(X[k] e^{+2 pi i k m / num})
  float* rs = resampled ? resampled + (long)b * ld_rs : nullptr;
  for (int m = tid; m < num; m += PCC_THREADS) {
    float y[4] = {0.f, 0.f, 0.f, 0.f};
    int idx[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) idx[j] = (j * m) % num;
    const int step = (4 * m) % num;
    for (int k0 = 0; k0 < K; k0 += 4) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (k0 + j < K) {
          const float2 X = s_X[k0 + j];
          const float2 t = s_tw[idx[j]];
          y[j] = fmaf(X.x, t.x, y[j]);
          y[j] = fmaf(-X.y, t.y, y[j]);
          idx[j] += step;
          if (idx[j] >= num) idx[j] -= num;
        }
      }
    }
    const float v = mean_x + ((y[0] + y[1]) + (y[2] + y[3]));
    s_dut[m] = v;                                               // the centred curve is not read any more (barrier above)
    if (rs) rs[m] = v;
  }
  __syncthreads();

  // 5. Pearson in two passes: the means, then the centred sums
  double sr = 0.0, sy = 0.0;
  for (int i = tid; i < num; i += PCC_THREADS) { sr += (double)s_ref[i]; sy += (double)s_dut[i]; }
  const double mr = dx_block_sum<PCC_WAVES>(sr, s_red) / (double)num, my = dx_block_sum<PCC_WAVES>(sy, s_red) / (double)num;
  double srr = 0.0, syy = 0.0, sry = 0.0;
  for (int i = tid; i < num; i += PCC_THREADS) {
    const double dr = (double)s_ref[i] - mr, dy = (double)s_dut[i] - my;
    srr = fma(dr, dr, srr); syy = fma(dy, dy, syy); sry = fma(dr, dy, sry);
  }
  srr = dx_block_sum<PCC_WAVES>(srr, s_red); syy = dx_block_sum<PCC_WAVES>(syy, s_red); sry = dx_block_sum<PCC_WAVES>(sry, s_red);
  if (tid == 0) {
    const double sd_r = sqrt(srr / (double)num), sd_y = sqrt(syy / (double)num);
    pcc[b] = (sd_r > 0.0 && sd_y > 0.0) ? (float)((sry / (double)num) / (sd_y * sd_r)) : __builtin_nanf("");
  }
}

}  // namespace

extern "C" long dx_curve_pcc_max_len(void) { return PCC_MAX_LEN; }

extern "C" int dx_curve_pcc(const float* ref, long ld_ref, const int64_t* n_ref, const float* dut, long ld_dut, const int64_t* n_dut,
                            float* pcc, int* kept_ref, int* kept_dut, float* resampled, long ld_rs, int B, int T_ref, int T_dut,
                            int remove_unvoiced, void* stream) {
  DX_REQUIRE(ref && n_ref && dut && n_dut && pcc && kept_ref && kept_dut, DX_ERR_ARG, "dx_curve_pcc: null pointer");
  DX_REQUIRE(B > 0 && T_ref > 0 && T_dut > 0 && ld_ref >= T_ref && ld_dut >= T_dut && (!resampled || ld_rs >= T_ref), DX_ERR_SHAPE,
             "dx_curve_pcc: bad shape B=%d T_ref=%d T_dut=%d ld_ref=%ld ld_dut=%ld ld_rs=%ld", B, T_ref, T_dut, ld_ref, ld_dut, ld_rs);
  DX_REQUIRE(T_ref <= PCC_MAX_LEN && T_dut <= PCC_MAX_LEN, DX_ERR_UNSUPPORTED,
             "dx_curve_pcc: curves of T_ref=%d, T_dut=%d frames (at most %d are staged in LDS)", T_ref, T_dut, PCC_MAX_LEN);
  hipLaunchKernelGGL(curve_pcc_kernel, dim3(B), dim3(PCC_THREADS), 0, (hipStream_t)stream, ref, ld_ref, n_ref, dut, ld_dut, n_dut, pcc,
                     kept_ref, kept_dut, resampled, ld_rs, T_ref, T_dut, remove_unvoiced);
  DX_LAUNCH_CHECK();
  return DX_OK;
}
