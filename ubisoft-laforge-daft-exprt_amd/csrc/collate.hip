// K26: batch construction from a training set that is resident in device memory -- the collate of the reference
// (`src/daft_exprt/data_loader.py:146-211`: sort by phoneme count, right-zero-pad to the batch maxima) without a host in the loop.
//
// The store is packed once: the symbol-level arrays of all utterances back to back (symbol ids and integer durations as int32,
// the three float arrays as fp32), the frame-level arrays back to back, and the mels back to back with utterance u laid out as its
// `.npy` file is -- (n_mel, T_u) row-major at mel + n_mel * frm_off[u].  sym_off / frm_off (U + 1) are the int64 prefix sums of
// the L_u / T_u.
//
// Two kernels per batch.  `collate_order_kernel` (one workgroup per micro-batch) ranks the utterances of a micro-batch by phoneme
// count, descending and stable, and writes the per-row index tensors.  `collate_gather_kernel` fills the padded tensors: a
// workgroup owns GATHER_SPAN consecutive positions (frames t, or symbols l) of one output row, one position per lane, and walks
// the channels, so a wave reads 64 consecutive floats of a source row and writes 64 consecutive floats of an output row.
// Source rows start at any multiple of 4 bytes (an odd T_u): every access is one 4- or 8-byte element, nothing wider.
// Nothing here decides a size: L_pad / T_pad come from the host, and an utterance longer than them is cut, never written past.
#include "dx_common.h"

namespace {

constexpr int ORDER_THREADS = 256;
constexpr int ORDER_MAX_B = 1024;      // utterances of one micro-batch: their phoneme counts live in LDS (4 KiB)
constexpr int GATHER_THREADS = 256;
constexpr int GATHER_SPAN = GATHER_THREADS;   // positions (t or l) of one output row per workgroup, one per lane

// utterance index as the kernels use it: inside the store whatever the index tensor holds
__device__ __forceinline__ long store_index(const int64_t* idx, long i, long U) { return min(max((long)idx[i], 0L), U - 1); }

// ---- order: rank of entry b = #{j : L_j > L_b} + #{j < b : L_j == L_b}; row `rank` of the micro-batch takes entry b ------------
__global__ __launch_bounds__(ORDER_THREADS) void collate_order_kernel(
    const int64_t* __restrict__ idx, const int64_t* __restrict__ sym_off, const int64_t* __restrict__ frm_off,
    const int64_t* __restrict__ speaker, long U, const int64_t* __restrict__ pads, int64_t* __restrict__ src_utt,
    int64_t* __restrict__ src_pos, int64_t* __restrict__ input_lengths, int64_t* __restrict__ output_lengths,
    int64_t* __restrict__ speaker_ids, int64_t* __restrict__ skip_in, int64_t* __restrict__ nmax_in, int64_t* __restrict__ skip_out,
    int64_t* __restrict__ nmax_out, int B) {
  __shared__ int s_len[ORDER_MAX_B];
  const int mb = blockIdx.x;
  const long base = (long)mb * B;
  for (int b = threadIdx.x; b < B; b += ORDER_THREADS) {
    const long u = store_index(idx, base + b, U);
    s_len[b] = (int)(sym_off[u + 1] - sym_off[u]);
  }
  __syncthreads();
  const long l_pad = pads[2 * mb], t_pad = pads[2 * mb + 1];
  for (int b = threadIdx.x; b < B; b += ORDER_THREADS) {
    const int mine = s_len[b];
    int rank = 0;
    for (int j = 0; j < B; ++j) {               // (every lane reads the same LDS word: a broadcast)
      const int other = s_len[j];
      rank += (other > mine) || (other == mine && j < b);
    }
    const long u = store_index(idx, base + b, U);
    const long row = base + rank, len_in = mine, len_out = frm_off[u + 1] - frm_off[u];
    src_utt[row] = u;
    src_pos[row] = b;
    input_lengths[row] = len_in;
    output_lengths[row] = len_out;
    speaker_ids[row] = speaker[u];
    if (skip_in) {
      nmax_in[row] = l_pad;
      nmax_out[row] = t_pad;
      skip_in[row] = max(0L, min(len_in, l_pad - 2));
      skip_out[row] = max(0L, min(len_out, t_pad - 2));
    }
  }
}

// ---- gather: blockIdx.y = output row; blockIdx.x < n_frame_chunks: frames [x * SPAN, + SPAN) of the two frame arrays and of every mel
// channel; the other workgroups: symbols [(x - n_frame_chunks) * SPAN, + SPAN) of the five symbol arrays.  Every element of every
// output is written exactly once; positions at or past the utterance's own length get zero.
__global__ __launch_bounds__(GATHER_THREADS) void collate_gather_kernel(
    const int64_t* __restrict__ src_utt, const int64_t* __restrict__ sym_off, const int64_t* __restrict__ frm_off, long U,
    const int* __restrict__ sym, const float* __restrict__ dur_f, const int* __restrict__ dur_i, const float* __restrict__ sym_en,
    const float* __restrict__ sym_pi, const float* __restrict__ frm_en, const float* __restrict__ frm_pi, const float* __restrict__ mel,
    int64_t* __restrict__ o_sym, float* __restrict__ o_dur_f, int64_t* __restrict__ o_dur_i, float* __restrict__ o_sym_en,
    float* __restrict__ o_sym_pi, float* __restrict__ o_frm_en, float* __restrict__ o_frm_pi, float* __restrict__ o_mel, int L_pad,
    int T_pad, int n_mel, int n_frame_chunks) {
  const long row = blockIdx.y;
  const long u = store_index(src_utt, row, U);
  if ((int)blockIdx.x < n_frame_chunks) {
    const int t = blockIdx.x * GATHER_SPAN + threadIdx.x;
    if (t >= T_pad) return;
    const long f0 = frm_off[u];
    const long T_u = min(max(frm_off[u + 1] - f0, 0L), (long)T_pad);
    const bool live = t < T_u;
    o_frm_en[row * T_pad + t] = live ? frm_en[f0 + t] : 0.f;
    o_frm_pi[row * T_pad + t] = live ? frm_pi[f0 + t] : 0.f;
    const long ld_src = frm_off[u + 1] - f0;             // the utterance's own row pitch (not the clamped one)
    const float* s = mel + f0 * n_mel + t;
    float* o = o_mel + row * n_mel * T_pad + t;
    for (int m = 0; m < n_mel; ++m) o[(long)m * T_pad] = live ? s[(long)m * ld_src] : 0.f;
  } else {
    const int l = ((int)blockIdx.x - n_frame_chunks) * GATHER_SPAN + threadIdx.x;
    if (l >= L_pad) return;
    const long s0 = sym_off[u];
    const long L_u = min(max(sym_off[u + 1] - s0, 0L), (long)L_pad);
    const bool live = l < L_u;
    const long o = row * L_pad + l;
    o_sym[o] = live ? (int64_t)sym[s0 + l] : 0;
    o_dur_f[o] = live ? dur_f[s0 + l] : 0.f;
    o_dur_i[o] = live ? (int64_t)dur_i[s0 + l] : 0;
    o_sym_en[o] = live ? sym_en[s0 + l] : 0.f;
    o_sym_pi[o] = live ? sym_pi[s0 + l] : 0.f;
  }
}

}  // namespace

extern "C" long dx_collate_max_batch(void) { return ORDER_MAX_B; }
extern "C" long dx_collate_span(void) { return GATHER_SPAN; }

extern "C" int dx_collate_order(const int64_t* idx, const int64_t* sym_off, const int64_t* frm_off, const int64_t* speaker, long U,
                                const int64_t* pads, int64_t* src_utt, int64_t* src_pos, int64_t* input_lengths,
                                int64_t* output_lengths, int64_t* speaker_ids, int64_t* skip_in, int64_t* nmax_in, int64_t* skip_out,
                                int64_t* nmax_out, int n_micro, int B, void* stream) {
  DX_REQUIRE(idx && sym_off && frm_off && speaker && pads && src_utt && src_pos && input_lengths && output_lengths && speaker_ids,
             DX_ERR_ARG, "dx_collate_order: null pointer");
  const int n_bounds = (skip_in != nullptr) + (nmax_in != nullptr) + (skip_out != nullptr) + (nmax_out != nullptr);
  DX_REQUIRE(n_bounds == 0 || n_bounds == 4, DX_ERR_ARG, "dx_collate_order: null pointer among the four bounds tensors (all or none)");
  DX_REQUIRE(B <= ORDER_MAX_B, DX_ERR_UNSUPPORTED,
             "dx_collate_order: B=%d utterances per micro-batch (at most %d: their phoneme counts live in LDS)", B, ORDER_MAX_B);
  DX_REQUIRE(n_micro > 0 && B > 0 && U > 0, DX_ERR_SHAPE, "dx_collate_order: bad shape n_micro=%d B=%d U=%ld", n_micro, B, U);
  hipLaunchKernelGGL(collate_order_kernel, dim3(n_micro), dim3(ORDER_THREADS), 0, (hipStream_t)stream, idx, sym_off, frm_off, speaker, U,
                     pads, src_utt, src_pos, input_lengths, output_lengths, speaker_ids, skip_in, nmax_in, skip_out, nmax_out, B);
  DX_LAUNCH_CHECK();
  return DX_OK;
}

extern "C" int dx_collate_gather(const int64_t* src_utt, const int64_t* sym_off, const int64_t* frm_off, long U, const int* sym,
                                 const float* dur_f, const int* dur_i, const float* sym_en, const float* sym_pi, const float* frm_en,
                                 const float* frm_pi, const float* mel, int64_t* o_sym, float* o_dur_f, int64_t* o_dur_i,
                                 float* o_sym_en, float* o_sym_pi, float* o_frm_en, float* o_frm_pi, float* o_mel, int B_tot, int L_pad,
                                 int T_pad, int n_mel, void* stream) {
  DX_REQUIRE(src_utt && sym_off && frm_off && sym && dur_f && dur_i && sym_en && sym_pi && frm_en && frm_pi && mel && o_sym && o_dur_f &&
                 o_dur_i && o_sym_en && o_sym_pi && o_frm_en && o_frm_pi && o_mel,
             DX_ERR_ARG, "dx_collate_gather: null pointer");
  DX_REQUIRE(B_tot > 0 && L_pad > 0 && T_pad > 0 && n_mel > 0 && U > 0, DX_ERR_SHAPE,
             "dx_collate_gather: bad shape B_tot=%d L_pad=%d T_pad=%d n_mel=%d U=%ld", B_tot, L_pad, T_pad, n_mel, U);
  DX_REQUIRE(B_tot <= 65535, DX_ERR_UNSUPPORTED, "dx_collate_gather: B_tot=%d rows (at most 65535: one grid row each)", B_tot);
  const int n_frame_chunks = dx_cdiv(T_pad, GATHER_SPAN);
  hipLaunchKernelGGL(collate_gather_kernel, dim3(n_frame_chunks + dx_cdiv(L_pad, GATHER_SPAN), B_tot), dim3(GATHER_THREADS), 0,
                     (hipStream_t)stream, src_utt, sym_off, frm_off, U, sym, dur_f, dur_i, sym_en, sym_pi, frm_en, frm_pi, mel, o_sym,
                     o_dur_f, o_dur_i, o_sym_en, o_sym_pi, o_frm_en, o_frm_pi, o_mel, L_pad, T_pad, n_mel, n_frame_chunks);
  DX_LAUNCH_CHECK();
  return DX_OK;
}
