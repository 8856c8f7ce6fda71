// K21: the per-utterance glue of training-feature extraction (extract_features.py:387-494): crop a waveform to its markers' span,
// turn aligner spans into integer frame durations, average frame energy / pitch per symbol.  All three are latency-sized: no
// matrix units, no LDS; one wave per utterance for the two that walk rows.
#include "dx_common.h"

namespace {

// grid (ceil(ldy / 1024), B): y[b, s] = x[b, begin_b + s] for s < len_b, 0 up to ldy.  Samples outside [0, S) read as 0.
__global__ __launch_bounds__(256) void wav_crop_kernel(const float* __restrict__ x, long ldx, const int64_t* __restrict__ crop,
                                                       float* __restrict__ y, long ldy, long S) {
  const int b = blockIdx.y;
  const long begin = crop[2 * b], len = crop[2 * b + 1];
  const long end = min(ldy, (long)(blockIdx.x + 1) * 1024);
  for (long s = (long)blockIdx.x * 1024 + threadIdx.x; s < end; s += 256) {
    const long src = begin + s;
    y[(long)b * ldy + s] = (s < len && src >= 0 && src < S) ? x[(long)b * ldx + src] : 0.f;
  }
}

// One wave per utterance.  The frame count of a row depends on that row's (begin, end) alone, so the rows are counted in
// parallel (lane = row) and the reference's serial `while curr_frame <= nb_frames: pop(0)` becomes a prefix sum: row l is
// popped iff the frames assigned before it are fewer than nb_frames.  Times in fp64, everything else in integers.
__global__ __launch_bounds__(64) void marker_durations_kernel(const double* __restrict__ spans, const int64_t* __restrict__ n_rows,
                                                              const int64_t* __restrict__ n_samples, int64_t* __restrict__ out,
                                                              int64_t* __restrict__ n_out, int* __restrict__ status, int L, double sr,
                                                              int fl, int hop, int centered) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const double* sp = spans + (long)b * L * 2;
  int64_t* o = out + (long)b * L;
  const long rows = dx_clamp_len(n_rows, b, L);
  const long n = n_samples[b];
  const long nb_frames = 1 + (long)((double)(n - fl) / (double)hop);     // int() truncates toward zero, like the cast
  const long half = (long)((double)fl / 2.0);
  const long edge = (long)((double)fl / 2.0 / (double)hop);

  auto count = [&](long l, bool* zero_len) -> long {
    const double bg = sp[2 * l], en = sp[2 * l + 1];
    *zero_len = bg == en;
    return *zero_len ? 0 : dx_span_frames((long)(bg * sr), (long)(en * sr), half, hop, nb_frames);
  };

  // pass 1: how many rows the loop pops (they are a prefix of the rows), and which error ends it
  long assigned = 0, popped = 0;
  int st = 0;
  for (long l0 = 0; l0 < rows && assigned < nb_frames && !st; l0 += 64) {
    const long l = l0 + lane;
    bool zero_len = false;
    const long c = l < rows ? count(l, &zero_len) : 0;
    const long x = dx_wave_scan(c, lane);
    const bool pop = l < rows && assigned + x - c < nb_frames;
    if (__ballot(pop && zero_len)) st = 2;                               // ValueError: a popped row of zero length
    popped += __popcll(__ballot(pop));
    assigned += __shfl(x, 63, 64);
  }
  if (!st && assigned < nb_frames) st = 1;                               // IndexError: pop from an empty list
  if (!st && centered && popped == 0) st = 1;                            // IndexError: int_durations[0] of an empty list
  const bool extra = centered && popped < rows;                          // rows are left: ONE more entry holds the right edge frames
  const long n_list = popped + (extra ? 1 : 0);

  // pass 2: the list itself, left-aligned, zeros behind it; sum and zero test for the caller's asserts
  long total = 0;
  int any_zero = 0;
  for (long l0 = 0; l0 < L; l0 += 64) {
    const long l = l0 + lane;
    if (l >= L) continue;
    long v = 0;
    if (!st) {
      bool zero_len;
      if (l < popped) v = count(l, &zero_len);
      if (centered) {
        if (l == 0) v += edge;
        if (extra ? l == popped : l == popped - 1) v += edge;
      }
      if (l < n_list) { total += v; any_zero |= v == 0; }
    }
    o[l] = v;
  }
  total = dx_wave_sum(total);
  any_zero = __ballot(any_zero) != 0;
  if (!st) {
    const long mel_frames = centered ? 1 + n / hop : (n >= fl ? 1 + (n - fl) / hop : 0);
    if (n_list != rows || total != mel_frames || any_zero) st = 3;       // the asserts of extract_features.py:437-439
  }
  if (lane == 0) {
    status[b] = st;
    if (n_out) n_out[b] = (st == 1 || st == 2) ? 0 : n_list;
  }
}

// One wave per utterance.  Rows are taken 64 at a time: a wave scan gives every row its first frame, then the wave reduces the
// rows one after the other, lane j adding frames j, j + 64, ... of the row in double before a fixed butterfly: the result
// depends on the row's frames alone.
__global__ __launch_bounds__(64) void symbol_pool_kernel(const float* __restrict__ energy, const float* __restrict__ log_pitch, long ldt,
                                                         const int64_t* __restrict__ durations, const int64_t* __restrict__ n_rows,
                                                         float* __restrict__ sym_energy, float* __restrict__ sym_pitch, int T, int L) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const float* e = energy + (long)b * ldt;
  const float* p = log_pitch + (long)b * ldt;
  const int64_t* d = durations + (long)b * L;
  const long rows = dx_clamp_len(n_rows, b, L);
  long first = 0;                                                        // first frame of the chunk's first row
  for (long l0 = 0; l0 < L; l0 += 64) {
    const long l = l0 + lane;
    long dl = l < rows ? (long)d[l] : 0;
    if (dl < 0) dl = 0;
    const long x = dx_wave_scan(dl, lane);
    const long start = first + x - dl;
    first += __shfl(x, 63, 64);
    float out_e = 0.f, out_p = 0.f;
    const int live = (int)min(64L, rows - l0);                           // rows of this chunk that exist (<= 0: none)
    for (int r = 0; r < live; ++r) {
      const long dr = __shfl(dl, r, 64), sr = __shfl(start, r, 64);
      if (dr == 0) continue;                                             // (wave-uniform)
      double se = 0.0, spv = 0.0;
      long voiced = 0;
      for (long f = sr + lane; f < sr + dr && f < T; f += 64) {
        se += (double)e[f];
        const float pv = p[f];
        if (pv > 0.f) { spv += (double)pv; ++voiced; }
      }
      se = dx_wave_sum(se);
      spv = dx_wave_sum(spv);
      voiced = dx_wave_sum(voiced);
      if (lane == r) {
        out_e = (float)(se / (double)dr);
        out_p = voiced ? (float)(spv / (double)voiced) : 0.f;
      }
    }
    if (l < L) { sym_energy[(long)b * L + l] = out_e; sym_pitch[(long)b * L + l] = out_p; }
  }
}

}  // namespace

extern "C" int dx_wav_crop(const float* x, long ldx, const int64_t* crop, float* y, long ldy, int B, long S, void* stream) {
  DX_REQUIRE(x && crop && y, DX_ERR_ARG, "dx_wav_crop: null pointer");
  DX_REQUIRE(B > 0 && B <= 65535 && S > 0 && ldx >= S && ldy > 0, DX_ERR_SHAPE, "dx_wav_crop: bad shape B=%d S=%ld ldx=%ld ldy=%ld", B, S,
             ldx, ldy);
  hipLaunchKernelGGL(wav_crop_kernel, dim3((unsigned)((ldy + 1023) / 1024), B), dim3(256), 0, (hipStream_t)stream, x, ldx, crop, y, ldy, S);
  DX_LAUNCH_CHECK();
  return DX_OK;
}

extern "C" int dx_marker_durations(const double* spans, const int64_t* n_rows, const int64_t* n_samples, int64_t* durations,
                                   int64_t* n_out, int* status, int B, int L, double sampling_rate, int filter_length, int hop_length,
                                   int centered, void* stream) {
  DX_REQUIRE(spans && n_rows && n_samples && durations && status, DX_ERR_ARG, "dx_marker_durations: null pointer");
  DX_REQUIRE(B > 0 && L > 0 && hop_length > 0 && filter_length > 0 && sampling_rate > 0, DX_ERR_SHAPE,
             "dx_marker_durations: bad shape B=%d L=%d filter_length=%d hop_length=%d", B, L, filter_length, hop_length);
  hipLaunchKernelGGL(marker_durations_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, spans, n_rows, n_samples, durations, n_out,
                     status, L, sampling_rate, filter_length, hop_length, centered);
  DX_LAUNCH_CHECK();
  return DX_OK;
}

extern "C" int dx_symbol_pool(const float* energy, const float* log_pitch, long ldt, const int64_t* durations, const int64_t* n_rows,
                              float* sym_energy, float* sym_pitch, int B, int T, int L, void* stream) {
  DX_REQUIRE(energy && log_pitch && durations && n_rows && sym_energy && sym_pitch, DX_ERR_ARG, "dx_symbol_pool: null pointer");
  DX_REQUIRE(B > 0 && T > 0 && L > 0 && ldt >= T, DX_ERR_SHAPE, "dx_symbol_pool: bad shape B=%d T=%d L=%d ldt=%ld", B, T, L, ldt);
  hipLaunchKernelGGL(symbol_pool_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, energy, log_pitch, ldt, durations, n_rows, sym_energy,
                     sym_pitch, T, L);
  DX_LAUNCH_CHECK();
  return DX_OK;
}
