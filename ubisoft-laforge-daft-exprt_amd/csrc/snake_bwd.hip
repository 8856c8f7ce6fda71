// K35 -- the backward of K34 (csrc/snake.hip), BigVGAN's anti-aliased periodic activation, as ONE pass over x and dy: what fine-tuning a
// BigVGAN generator adds to K33.  Nothing is saved by the forward; per utterance b (n = n_rows[b] live rows) and channel c:
//   u[t]   = 2 sum_i f_up[t + 15 - 2 i] x[clamp(i - 5, 0, n - 1)]                        t in [0, 2 n)   (recomputed)
//   ds[t]  = sum_{m in [0, n), k < 12 : clamp(2 m + k - 5, 0, 2 n - 1) = t} f_down[k] dy[m]
//   du[t]  = ds[t] (1 + inv_beta alpha sin(2 alpha u[t]))
//   dx[j]  = 2 sum_{t, i : clamp(i - 5, 0, n - 1) = j, 0 <= t + 15 - 2 i < 12} f_up[t + 15 - 2 i] du[t]
//   dalpha = inv_beta sum_{b, t} ds[t] u[t] sin(2 alpha u[t]),   dinv_beta = 1/2 sum_{b, t} ds[t] (1 - cos(2 alpha u[t]))
// u, ds and du never leave the registers.  A thread owns 4 consecutive channels and walks a tile of `rows` rows exactly as the forward
// does: step m loads x row m + 5 and dy row m + 5, which completes the six rows m .. m + 5 that BOTH new samples t = 2 m + 5 (taps
// 10, 8 .. 0 of either filter) and t = 2 m + 6 (taps 11, 9 .. 1) read -- u from x with the edge ROW replicated, ds from dy with ZEROS
// outside [0, n) -- pushes du of the two into a 12-deep window, and dx[m] is the window under f_up[0 .. 11].  Five steps before the
// tile fill the window (10 samples of halo).  The ends, where the backward differs from the forward:
//   ds[0] also collects the samples t in [-5, -1] (steps m = -5 .. -3 of tile 0), ds[2 n - 1] the samples [2 n, 2 n + 4]: at step
//   m = n - 3 all the dy rows they read (n - 2 and n - 1) are in the window, so the fold is taken there;
//   dx[0] also collects the five virtual rows -5 .. -1 (the window of tile 0's fill steps), dx[n - 1] the rows n .. n + 4: five more
//   shifts of the window with zeros pushed, by the thread that owns row n - 1.
// One chain of fmas per dx[j] in one lane, its order set by the row (and n at the two ends) alone: the same bits alone, in any batch,
// at any N and at any tile height.  The parameter sums: each thread adds the terms of the samples its tile OWNS (t in [2 m0, 2 m0 +
// 2 rows): halo samples are never counted twice) in double, one partial per (utterance, tile, channel) goes to the workspace, and a
// second launch adds the partials in index order in double and rounds once.  No atomics.  The loop is not unrolled (see K34): the
// accurate sincosf with its large-argument reduction is most of a step, eight of them.  64-thread workgroups: at fine-tuning shapes
// (16 x 8192 rows x 32 .. 256 channels) even 32-row tiles are 8 192 .. 32 768 threads, and they are spread over as many CUs as they reach.
#include "dx_common.h"

namespace {

constexpr int SNAKE_BWD_HEIGHTS = 4;
constexpr int SNAKE_BWD_ROWS[SNAKE_BWD_HEIGHTS] = {32, 64, 128, 192};   // dx_vocoder_snake_bwd_tile_rows(i); ascending
constexpr long SNAKE_BWD_FILL = 65536;      // threads of one wave on every SIMD of the 256 CUs: the launcher's rule for tile_rows = 0
constexpr int SNAKE_BWD_SLICES = 16;        // of the reduce launch: 16 outputs x 16 slices of the partials per workgroup

struct SnakeBwdArgs {
  const float* x; const float* dy; const float* alpha; const float* inv_beta; float* dx; double* part; const int64_t* n;
  long ldx, lddy, lddx, threads;
  int N, C, C4, tiles, rows;
  float f_up[12], f_down[12];
};

// one thread per (utterance, tile of a.rows rows, 4 channels), channels fastest; 1-D grid.  At step m slot i of xw / dw holds x / dy row
// m + i and slot j of duw holds du[2 m - 5 + j]
__global__ __launch_bounds__(64) void snake_bwd_kernel(SnakeBwdArgs a) {
  const long idx = (long)blockIdx.x * 64 + threadIdx.x;
  if (idx >= a.threads) return;
  const int cq = (int)(idx % a.C4);
  const long tl = idx / a.C4;
  const int tile = (int)(tl % a.tiles), b = (int)(tl / a.tiles);
  const int n = (int)dx_clamp_len(a.n, b, a.N);
  const int m0 = tile * a.rows, row_end = min(m0 + a.rows, a.N), live_end = min(row_end, n);
  const int own_lo = 2 * m0, own_hi = 2 * (m0 + a.rows);
  const float* xb = a.x + (long)b * a.N * a.ldx + 4 * cq;
  const float* gb = a.dy + (long)b * a.N * a.lddy + 4 * cq;
  float* ob = a.dx + (long)b * a.N * a.lddx + 4 * cq;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  double pa[4] = {0., 0., 0., 0.}, pb[4] = {0., 0., 0., 0.};
  if (m0 < n) {
    const f32x4 al = *reinterpret_cast<const f32x4*>(a.alpha + 4 * cq), ib = *reinterpret_cast<const f32x4*>(a.inv_beta + 4 * cq);
    const f32x4 al2 = 2.f * al, ibal = ib * al;
    // a dy row outside [0, n) is a zero; the load goes to a live row all the same, and its value is dropped
    auto dy_row = [&](int r) -> f32x4 {
      const f32x4 v = *reinterpret_cast<const f32x4*>(gb + (long)min(max(r, 0), n - 1) * a.lddy);
      return r >= 0 && r < n ? v : zero;
    };
    f32x4 xw[6], dw[6], duw[12];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      xw[i] = *reinterpret_cast<const f32x4*>(xb + (long)min(max(m0 - 6 + i, 0), n - 1) * a.ldx);
      dw[i] = dy_row(m0 - 6 + i);
    }
#pragma unroll
    for (int j = 0; j < 12; ++j) duw[j] = zero;
    f32x4 xnext = *reinterpret_cast<const f32x4*>(xb + (long)min(m0, n - 1) * a.ldx), dnext = dy_row(m0);   // rows m + 5, a step ahead
    f32x4 head = zero;          // ds of the samples t < 0, on their way into ds[0]
    f32x4 acc = zero;           // the chain of an edge row: the virtual rows in front of row 0, and row n - 1 until its five are in
#pragma unroll 1
    for (int m = m0 - 5; m < live_end; ++m) {
#pragma unroll
      for (int i = 0; i < 5; ++i) { xw[i] = xw[i + 1]; dw[i] = dw[i + 1]; }
      xw[5] = xnext;
      dw[5] = dnext;
      xnext = *reinterpret_cast<const f32x4*>(xb + (long)min(max(m + 6, 0), n - 1) * a.ldx);
      dnext = dy_row(m + 6);
      f32x4 uo = zero, ue = zero, so = zero, se = zero;
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        uo += a.f_up[10 - 2 * i] * xw[i];                                     // t = 2 m + 5: rows m .. m + 5 under taps 10, 8 .. 0
        ue += a.f_up[11 - 2 * i] * xw[i];                                     // t = 2 m + 6: the same rows under taps 11, 9 .. 1
        so += a.f_down[10 - 2 * i] * dw[i];
        se += a.f_down[11 - 2 * i] * dw[i];
      }
      uo = 2.f * uo;
      ue = 2.f * ue;
      if (m <= -3) {                                                          // tile 0: the samples in front of the utterance
        if (m < -3) { head += so + se; so = zero; se = zero; }
        else { se += head + so; so = zero; }                                  // se is ds[0]
      }
      if (m >= n - 3) {                                                       // so is at or past 2 n - 1, se past it
        if (m == n - 3) {                                                     // dw[1], dw[2]: dy rows n - 2, n - 1 (zeros below row 0)
          so += se;
          so += a.f_down[10] * dw[1];                                         // t = 2 n + 1
          so += a.f_down[8] * dw[2];
          so += a.f_down[11] * dw[1];                                         // 2 n + 2
          so += a.f_down[9] * dw[2];
          so += a.f_down[10] * dw[2];                                         // 2 n + 3
          so += a.f_down[11] * dw[2];                                         // 2 n + 4
        } else {
          so = zero;
        }
        se = zero;
      }
      const int to = 2 * m + 5;
      const float ko = to >= own_lo && to < own_hi ? 1.f : 0.f, ke = to + 1 >= own_lo && to + 1 < own_hi ? 1.f : 0.f;
      f32x4 duo, due;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float sn, cs;
        sincosf(al2[e] * uo[e], &sn, &cs);
        duo[e] = so[e] * fmaf(ibal[e], sn, 1.f);
        pa[e] += (double)(ko * so[e] * (uo[e] * sn));
        pb[e] += (double)(ko * so[e] * (1.f - cs));
        sincosf(al2[e] * ue[e], &sn, &cs);
        due[e] = se[e] * fmaf(ibal[e], sn, 1.f);
        pa[e] += (double)(ke * se[e] * (ue[e] * sn));
        pb[e] += (double)(ke * se[e] * (1.f - cs));
      }
#pragma unroll
      for (int j = 0; j < 10; ++j) duw[j] = duw[j + 2];
      duw[10] = duo;
      duw[11] = due;
      if (m < 0 || m >= m0) {                                                 // (m < 0: tile 0's fill steps, the virtual rows -5 .. -1)
        f32x4 v = m <= 0 ? acc : zero;
#pragma unroll
        for (int j = 0; j < 12; ++j) v += a.f_up[j] * duw[j];
        if (m < 0 || m == n - 1) acc = v;
        else *reinterpret_cast<f32x4*>(ob + (long)m * a.lddx) = 2.f * v;
      }
    }
    if (live_end == n) {                                                      // this thread owns row n - 1: the virtual rows n .. n + 4
#pragma unroll 1
      for (int e = 0; e < 5; ++e) {
#pragma unroll
        for (int j = 0; j < 10; ++j) duw[j] = duw[j + 2];
        duw[10] = zero;
        duw[11] = zero;
#pragma unroll
        for (int j = 0; j < 10; ++j) acc += a.f_up[j] * duw[j];
      }
      *reinterpret_cast<f32x4*>(ob + (long)(n - 1) * a.lddx) = 2.f * acc;
    }
  }
  for (int m = max(m0, live_end); m < row_end; ++m) *reinterpret_cast<f32x4*>(ob + (long)m * a.lddx) = zero;
  if (a.part) {                                                               // a tile without live rows writes its zeros: nothing is preset
    double* p = a.part + ((long)b * a.tiles + tile) * 2 * a.C + 4 * cq;
#pragma unroll
    for (int e = 0; e < 4; ++e) { p[e] = pa[e]; p[a.C + e] = pb[e]; }
  }
}

// part [P][2][C] double -> dalpha, dinv_beta (C): 16 outputs x 16 slices per workgroup; slice s adds the partials s, s + 16, ... in index
// order, then the 16 slice sums are added from left to right -- an order the shapes fix.  The factors the walk left out go on here.
__global__ __launch_bounds__(256) void snake_bwd_reduce_kernel(const double* part, const float* inv_beta, float* dalpha, float* dinv_beta,
                                                               long P, int C) {
  __shared__ double red[SNAKE_BWD_SLICES][17];
  const int o = threadIdx.x & 15, s = threadIdx.x >> 4;
  const int col = blockIdx.x * 16 + o;
  double v = 0.;
  if (col < 2 * C)
    for (long p = s; p < P; p += SNAKE_BWD_SLICES) v += part[p * 2 * C + col];
  red[s][o] = v;
  __syncthreads();
  if (s == 0 && col < 2 * C) {
    double t = red[0][o];
#pragma unroll
    for (int w = 1; w < SNAKE_BWD_SLICES; ++w) t += red[w][o];
    if (col < C) dalpha[col] = (float)(t * (double)inv_beta[col]);
    else dinv_beta[col - C] = (float)(0.5 * t);
  }
}

bool snake_bwd_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

long snake_bwd_tiles(int N, int rows) { return ((long)N + rows - 1) / rows; }

}  // namespace

extern "C" int dx_vocoder_snake_bwd_tile_rows(int index) { return index >= 0 && index < SNAKE_BWD_HEIGHTS ? SNAKE_BWD_ROWS[index] : 0; }

extern "C" long dx_vocoder_snake_bwd_workspace(int B, int N, int C) {
  if (B <= 0 || N <= 0 || C <= 0) return 0;
  return (long)B * snake_bwd_tiles(N, SNAKE_BWD_ROWS[0]) * 2 * C * (long)sizeof(double);      // the smallest height has the most tiles
}

extern "C" int dx_vocoder_snake_bwd(const float* x, long ldx, const float* dy, long lddy, const float* alpha, const float* inv_beta,
                                    const float* filters, float* dx, long lddx, float* dalpha, float* dinv_beta, void* ws,
                                    const int64_t* n_rows, int B, int N, int C, int tile_rows, void* stream) {
  DX_REQUIRE(x && dy && alpha && inv_beta && filters && dx && n_rows, DX_ERR_ARG, "dx_vocoder_snake_bwd: null pointer");
  DX_REQUIRE((dalpha == nullptr) == (dinv_beta == nullptr), DX_ERR_ARG,
             "dx_vocoder_snake_bwd: dalpha and dinv_beta are both given or both null");
  DX_REQUIRE(!dalpha || ws, DX_ERR_ARG, "dx_vocoder_snake_bwd: null workspace (dx_vocoder_snake_bwd_workspace bytes) with dalpha given");
  DX_REQUIRE(B > 0 && N > 0 && C > 0 && ldx >= C && lddy >= C && lddx >= C, DX_ERR_SHAPE,
             "dx_vocoder_snake_bwd: bad shape B=%d N=%d C=%d ldx=%ld lddy=%ld lddx=%ld", B, N, C, ldx, lddy, lddx);
  DX_REQUIRE(C % 4 == 0 && ldx % 4 == 0 && lddy % 4 == 0 && lddx % 4 == 0, DX_ERR_UNSUPPORTED,
             "dx_vocoder_snake_bwd: C=%d, ldx=%ld, lddy=%ld and lddx=%ld must be multiples of 4 (16-byte loads and stores)", C, ldx, lddy, lddx);
  DX_REQUIRE(snake_bwd_aligned16(x) && snake_bwd_aligned16(dy) && snake_bwd_aligned16(dx) && snake_bwd_aligned16(alpha) &&
                 snake_bwd_aligned16(inv_beta) && snake_bwd_aligned16(ws), DX_ERR_ARG,
             "dx_vocoder_snake_bwd: x, dy, dx, alpha, inv_beta and the workspace must be 16-byte aligned");
  DX_REQUIRE(dx != x && dx != dy, DX_ERR_ARG, "dx_vocoder_snake_bwd: dx must not alias x or dy (other threads read their halo)");
  int rows = 0;
  if (tile_rows == 0) {     // the largest height that still fills the machine with one wave per SIMD, else the smallest
    rows = SNAKE_BWD_ROWS[0];
    for (int i = 1; i < SNAKE_BWD_HEIGHTS; ++i)
      if ((long)B * snake_bwd_tiles(N, SNAKE_BWD_ROWS[i]) * (C / 4) >= SNAKE_BWD_FILL) rows = SNAKE_BWD_ROWS[i];
  } else {
    for (int i = 0; i < SNAKE_BWD_HEIGHTS; ++i)
      if (tile_rows == SNAKE_BWD_ROWS[i]) rows = tile_rows;
  }
  DX_REQUIRE(rows > 0, DX_ERR_UNSUPPORTED, "dx_vocoder_snake_bwd: tile_rows=%d is not 0 or one of dx_vocoder_snake_bwd_tile_rows() (%d, %d, %d, %d)",
             tile_rows, SNAKE_BWD_ROWS[0], SNAKE_BWD_ROWS[1], SNAKE_BWD_ROWS[2], SNAKE_BWD_ROWS[3]);
  SnakeBwdArgs a = {x, dy, alpha, inv_beta, dx, dalpha ? (double*)ws : nullptr, n_rows, ldx, lddy, lddx, 0, N, C, C / 4,
                    (int)snake_bwd_tiles(N, rows), rows, {}, {}};
  a.threads = (long)B * a.tiles * a.C4;
  const long blocks = (a.threads + 63) / 64;
  DX_REQUIRE(blocks <= 0x7fffffffL && (long)N + SNAKE_BWD_ROWS[SNAKE_BWD_HEIGHTS - 1] + 8 <= 0x3fffffffL, DX_ERR_UNSUPPORTED,
             "dx_vocoder_snake_bwd: B=%d N=%d C=%d need %ld workgroups: more than grid.x, or more samples than a 32-bit index, holds", B, N,
             C, blocks);
  for (int i = 0; i < 12; ++i) { a.f_up[i] = filters[i]; a.f_down[i] = filters[12 + i]; }
  hipLaunchKernelGGL(snake_bwd_kernel, dim3((unsigned)blocks), dim3(64), 0, (hipStream_t)stream, a);
  DX_LAUNCH_CHECK();
  if (dalpha) {
    hipLaunchKernelGGL(snake_bwd_reduce_kernel, dim3((unsigned)((2 * C + 15) / 16)), dim3(256), 0, (hipStream_t)stream,
                       (const double*)ws, inv_beta, dalpha, dinv_beta, (long)B * a.tiles, C);
    DX_LAUNCH_CHECK();
  }
  return DX_OK;
}
