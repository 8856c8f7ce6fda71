/* daft_exprt_hip.h -- C ABI of libdaftexprt_hip.so, the MI355X (gfx950) kernel library behind the
 * Daft-Exprt acoustic-model hot path.
 *
 * The reference (ubisoft/ubisoft-laforge-daft-exprt) has no native boundary: every device op is an
 * ATen call made from src/daft_exprt/model.py / loss.py / train.py.  Each entry point below replaces
 * the ATen op sequence of the reference lines cited next to it.  The Python binding a maintainer
 * would add on the reference side is shown in INTEGRATION.md (ctypes; no torch types cross this ABI).
 *
 * Conventions
 *   - plain pointers + sizes; all pointers are DEVICE pointers unless stated otherwise;
 *   - the caller owns every buffer (inputs, outputs, workspaces); nothing is allocated or freed here;
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*); no hidden synchronisation;
 *   - activations are channel-last (B, N, C); "lengths" are int64 (B,) device arrays;
 *   - return 0 on success, a negative DX_ERR_* code otherwise; dx_last_error() gives the message
 *     (thread-local).  Argument violations mirror the reference's asserts as errors, never UB.
 *   - dtype codes: DX_F32 / DX_BF16 / DX_I64.
 *   - DEAD ROWS (ABI v11).  Rows of an utterance at or past length + conv halo (`skip_lengths[b] + 2`, or the length of a
 *     masked output) never reach a valid output.  Producers write them as zeros only below
 *         dx_fill_end(len, N) = min(N, roundup(len + 4, 256) + 1)
 *     -- as far as a consumer's last tile (<= 256 rows + 1 halo row, starting below length + 2) can reach; rows at or past
 *     that index are never read by any entry point and are left UNWRITTEN (up to v10 they were written as zeros).  Callers
 *     that inspect whole (B, N, C) intermediate tensors must not look past it.  User-visible outputs -- the transposed
 *     (B, C, N) form of dx_conv1d (the mel), dx_linear_small_*, dx_gu_upsample_fwd -- keep their full zero padding.
 *     A hard sequence end n_max[b] < N (an utterance that belongs to a shorter-padded micro-batch of a grouped step) is
 *     expressed with the same arguments: skip_lengths[b] = min(length, n_max - 2), mask_lengths[b] = n_max.
 */
#ifndef DAFT_EXPRT_HIP_H
#define DAFT_EXPRT_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DX_ABI_VERSION 13

enum { DX_F32 = 0, DX_BF16 = 1, DX_I64 = 2 };
enum { DX_OK = 0, DX_ERR_ARG = -1, DX_ERR_SHAPE = -2, DX_ERR_DTYPE = -3, DX_ERR_LAUNCH = -4, DX_ERR_UNSUPPORTED = -5 };

/* flags of dx_conv1d */
enum { DX_CONV_RELU = 1, DX_CONV_TRANSPOSED_OUT = 2, DX_CONV_ACCUMULATE = 4 /* y += result */ };

int dx_abi_version(void);
const char* dx_last_error(void);

/* ---- the step block: what changes from one optimizer step to the next, in DEVICE memory.
 * The reference's trainer recomputes these on the host every iteration and they reach its kernels as scalar arguments: the
 * learning rate (train.py:139-151, 491-494), Adam's bias corrections (torch.optim.Adam, train.py:299-301), the adversarial
 * loss weight (loss.py:22-28), and -- through torch's Philox offset -- the dropout streams.  A captured step (hipGraph) replays
 * FIXED kernel arguments, so every entry point that consumes one of them takes an optional `const DxStepScalars* step`
 * (NULL = use the by-value arguments, the eager path):
 *   dropout:  effective seed = (seed argument + step->seed_salt) mod 2^63     (dx_conv1d_ln, dx_conv1d_lnbwd, dx_layernorm_fwd / _bwd,
 *             dx_attention_fwd / _bwd) -- the same number the eager path passes by value, hence the same masks bit for bit;
 *   dx_adam_step: lr, bc1 = 1 - beta1^t, bc2_sqrt = sqrt(1 - beta2^t) replace the lr / step arguments;
 *   dx_loss_fwd_bwd: w_speaker replaces w_spk.
 * dx_step_scalars_set fills the block with one single-thread launch (stream-ordered in front of the step that reads it). */
typedef struct DxStepScalars {
  uint64_t seed_salt;
  float lr, bc1, bc2_sqrt, w_speaker;
  int step;
  int reserved[3];
} DxStepScalars;
int dx_step_scalars_set(DxStepScalars* dev, uint64_t seed_salt, float lr, float beta1, float beta2, int step, float w_speaker,
                        void* stream);

/* ---- K1/K3/K12: k-tap (1 or 3) stride-1 "same" conv on channel-last activations as an implicit GEMM
 * on MFMA; also nn.Linear (taps = 1).  Replaces ConvNorm1D.forward (model.py:86-94: transpose, nn.Conv1d,
 * transpose), LinearNorm.forward (model.py:66-72) and the in/out projections of nn.MultiheadAttention
 * (model.py:182-186).
 *   x        (B, N, Cin) rows `ldx` elements apart, dtype x_dtype
 *   w_packed [taps][Cout][Cin], dtype w_dtype = the MFMA operand type (DX_BF16 -> v_mfma_f32_32x32x16_bf16,
 *            DX_F32 -> v_mfma_f32_32x32x2_f32); produced by dx_pack_conv_weight
 *   bias     (Cout) fp32 or NULL
 *   y        (B, N, Cout) rows `ldy` apart -- or (B, Cout, N) rows `ldy` apart with DX_CONV_TRANSPOSED_OUT
 *   relu_gate NULL, or a tensor laid out exactly like y (dtype gate_dtype): y is multiplied by (gate > 0)
 *            (the ReLU derivative when this call is the data-gradient of a conv that fed a ReLU)
 *   mask_lengths NULL, or int64 (B): rows n >= mask_lengths[b] are written as zeros
 *            (masked_fill of model.py:259,262,569,707)
 *   skip_lengths NULL, or int64 (B): padding early-out -- 128-row tiles that start at n0 >= skip_lengths[b] + 2 are
 *            written as zeros without touching the MFMA pipe (rows past length + conv halo never reach a valid
 *            output) -- and not written at all from dx_fill_end on (DEAD ROWS above)
 * Positions outside [0, N) are zero padding (N = the batch's max length).  Cin % 8 == 0.
 */
int dx_conv1d(const void* x, int x_dtype, long ldx, const void* w_packed, int w_dtype, const float* bias,
              void* y, int y_dtype, long ldy, const void* relu_gate, int gate_dtype, const int64_t* mask_lengths,
              const int64_t* skip_lengths, int B, int N, int Cin, int Cout, int taps, int flags, void* stream);

/* dx_conv1d with an optional fragment-order copy of the weights (dx_pack_frag_major(_batched) of w_packed; NULL = dx_conv1d):
 * the register-weights kernel of the Cin = 128, Cout % 256 == 0 GEMMs (FF conv 128 -> 1024 and the data gradient of
 * 1024 -> 128) then loads every MFMA fragment of its weight slice straight into its registers -- one round trip instead of
 * a pass through LDS in front of the first position tile.  Same results bit for bit. */
int dx_conv1d_wfrag(const void* x, int x_dtype, long ldx, const void* w_packed, int w_dtype, const void* w_frag, const float* bias,
                    void* y, int y_dtype, long ldy, const void* relu_gate, int gate_dtype, const int64_t* mask_lengths,
                    const int64_t* skip_lengths, int B, int N, int Cin, int Cout, int taps, int flags, void* stream);

/* The ReLU gate of the FF block as one BIT per element (ABI v12).  The data gradient of PositionWiseConvFF's second conv
 * (model.py:220-237: conv k3 -> ReLU -> conv k3) is gated by `h > 0`, h = the ReLU output of the first conv: a (B, N, Cout) tensor
 * that the gate would re-read in full.  Instead the forward conv leaves `bits` next to h and the data gradient reads those:
 *   bits_out != NULL:  y = relu(conv_k3(x, w) + bias) as dx_conv1d_wfrag with DX_CONV_RELU, and bits_out = (y > 0);
 *   bits_in  != NULL:  y = conv_k3(x, w) where bits_in, 0 elsewhere (the data gradient: w = the transposed / flipped copy, no bias).
 * bf16 x / w / y, Cin = 128, taps = 3, Cout % 256 == 0 (the register-weights kernel); w_frag optional as in dx_conv1d_wfrag.
 * bits: uint32 (B, Cout / 32, N); the bit order inside a word is private to the kernel pair (its own register order) -- only
 * these two calls read or write it.  mask_lengths / skip_lengths as in dx_conv1d; rows at or past mask_lengths have no bit set. */
int dx_conv1d_relu_bits(const void* x, long ldx, const void* w_packed, const void* w_frag, const float* bias, void* y, long ldy,
                        uint32_t* bits_out, const uint32_t* bits_in, const int64_t* mask_lengths, const int64_t* skip_lengths,
                        int B, int N, int Cout, void* stream);

/* dx_conv1d with Cout = 128 and the following LayerNorm fused into its epilogue (a 128-row tile holds complete rows):
 *   s = dropout_pre(conv(x) + bias) + residual;  y = LN(s) * gamma + beta;  y = film[b,:128] * y + film[b,128:];
 *   y = 0 where n >= lengths[b]
 * i.e. the attention out-projection + Dropout + residual + LayerNorm + mask (model.py:186-191, 259) and the second FF conv
 * + Dropout + residual + LayerNorm + FiLM + mask (model.py:226-235, 262) in one launch.  Outputs: y fp32, y_lp optional
 * bf16 copy, s_out / mean / rstd for dx_layernorm_bwd (NULL at inference).  lengths also drives the padding early-out.  * y2 (NULL = off; bf16 (B, N, n2), n2 = 128 or 384) with w2_packed (bf16 [1][n2][128]) and b2 (fp32 (n2) or NULL):
 * y2 = y_lp . w2^T + b2, the k = 1 projection that reads this LayerNorm's output next (the QKV projection of the following FFT
 * block, model.py:165-171), computed by the epilogue from the rows it has just normalised; split-K path only (see dx_conv1d_lnbwd). */
int dx_conv1d_ln(const void* x, int x_dtype, long ldx, const void* w_packed, int w_dtype, const float* bias,
                 const float* residual, const float* gamma, const float* beta, const float* film, long ldf,
                 const int64_t* lengths, float* y, void* y_lp, float* s_out, float* mean, float* rstd, int B, int N,
                 int Cin, int taps, float p_pre, uint64_t seed_pre, const int* plan, int plan_tiles, const void* w_frag,
                 const void* w2_packed, const float* b2, void* y2, int n2, const DxStepScalars* step, void* stream);

/* dx_conv1d_ln whose residual stream is re-derived instead of read (ABI v12).  In an FFT block the residual of the second LayerNorm
 * is the OUTPUT of the first one, a = mask(LN1(s1)) (model.py:186-191 -> 226-235): with res_mean != NULL `residual` is s1 (the saved
 * LayerNorm input of the launch that produced the stream), res_mean / res_rstd its row statistics, res_gamma / res_beta that
 * LayerNorm's parameters, and the epilogue computes  a = (s1 - mean) * rstd * gamma + beta  (0 where n >= lengths[b]) itself -- so
 * the producing launch may pass y = NULL and store only its bf16 copy and s1: 512 bytes per row less to write.  Split-K path only
 * (dx_conv1d_ln_path == DX_LN_PATH_SPLITK: DX_ERR_UNSUPPORTED otherwise); y = NULL is accepted by every path of both entry points
 * as long as y_lp is given.  res_mean = NULL: identical to dx_conv1d_ln. */
int dx_conv1d_ln_vres(const void* x, int x_dtype, long ldx, const void* w_packed, int w_dtype, const float* bias,
                      const float* residual, const float* res_mean, const float* res_rstd, const float* res_gamma, const float* res_beta,
                      const float* gamma, const float* beta, const float* film, long ldf,
                      const int64_t* lengths, float* y, void* y_lp, float* s_out, float* mean, float* rstd, int B, int N,
                      int Cin, int taps, float p_pre, uint64_t seed_pre, const int* plan, int plan_tiles, const void* w_frag,
                      const void* w2_packed, const float* b2, void* y2, int n2, const DxStepScalars* step, void* stream);

/* Data gradient of a conv / linear INTO a 128-channel residual stream, fused with the BACKWARD of the LayerNorm that
 * consumed that stream in the forward pass (autograd of model.py:189-191 resp. 226-235 + 259/262, i.e. what
 * dx_conv1d(..., ACCUMULATE) followed by dx_layernorm_bwd compute in two launches and two extra passes over the tensor):
 *   g  = y_inout + conv(x, w_packed)            (x = gradient of the conv's output, w_packed = transpose_flip packing)
 *   g  = 0 where n >= lengths[b];  FiLM: dfilm[b] += (sum_n g * LN, sum_n g), g *= film_gamma[b]
 *   dgamma += sum g * xhat, dbeta += sum g;  ds = rstd * (g*gamma - mean_c(g*gamma) - xhat * mean_c(g*gamma*xhat))
 *   y_inout <- ds (fp32, the residual gradient that flows on);  dx_pre_lp <- dropout_pre(ds) as bf16 (MFMA operand of the
 *   previous layer's data / weight gradient).   s_in / mean / rstd: saved by dx_conv1d_ln / dx_layernorm_fwd.
 * Cout is 128 by construction.  lengths also drives the padding early-out (rows >= lengths[b] + 2 stay zero).
 * y2 (NULL = off; bf16 (B, N, 128)) with w2_packed (bf16 [1][128][128], forward packing of the map to apply): y2 = dx_pre_lp . w2^T,
 * the 128 -> 128 linear layer whose data gradient consumes dx_pre_lp next (the attention output projection, model.py:182-186),
 * computed by the epilogue from the rows it has just produced instead of by a launch of its own; needs the split-K path
 * (dx_conv1d_ln_path == DX_LN_PATH_SPLITK: DX_ERR_UNSUPPORTED otherwise).  Same values as dx_conv1d on dx_pre_lp. */
int dx_conv1d_lnbwd(const void* x, int x_dtype, long ldx, const void* w_packed, int w_dtype, float* y_inout,
                    const float* s_in, const float* mean, const float* rstd, const float* gamma, const float* beta,
                    const float* film, long ldf, const int64_t* lengths, void* dx_pre_lp, float* dgamma, float* dbeta,
                    float* dfilm, long lddf, int B, int N, int Cin, int taps, float p_pre, uint64_t seed_pre,
                    const int* plan, int plan_tiles, const void* w_frag, const void* w2_packed, void* y2, const DxStepScalars* step,
                    void* stream);

/* Which kernel dx_conv1d_ln / dx_conv1d_ln_vres (backward = 0) or dx_conv1d_lnbwd (backward = 1) runs a GEMM on: the ONE statement
 * of that policy -- the entry points dispatch on it and gate res_mean / y2 with it, the host side asks instead of restating it.
 * Host-only: launches nothing, touches no device.  has_plan / has_frag: whether `plan` / `w_frag` are non-NULL.  It classifies and
 * does not validate: what the entry points reject (a plan with fp32 operands or with taps = 1 forward, ...) they still reject.
 *   DX_LN_PATH_SPLITK   split-K workgroups on the plan's tiles, weights from w_frag; the only path that takes res_mean and y2
 *   DX_LN_PATH_PLAN_K3  loader-wave ring kernel on the plan's tiles, taps = 3
 *   DX_LN_PATH_PLAN_K1  the same, taps = 1 (dx_conv1d_lnbwd only)
 *   DX_LN_PATH_ROWS128 / DX_LN_PATH_ROWS64   fixed 128- / 64-row tiles, no plan */
enum { DX_LN_PATH_SPLITK = 0, DX_LN_PATH_PLAN_K3 = 1, DX_LN_PATH_PLAN_K1 = 2, DX_LN_PATH_ROWS128 = 3, DX_LN_PATH_ROWS64 = 4 };
int dx_conv1d_ln_path(int x_dtype, int w_dtype, int taps, int Cin, int B, int N, int has_plan, int has_frag, int backward);

/* Which kernel dx_conv1d / dx_conv1d_wfrag runs a GEMM on: the ONE statement of that policy, as dx_conv1d_ln_path is for the
 * LayerNorm-fused entry points.  Host-only: launches nothing, touches no device.  It classifies and does not validate (the entry
 * points still reject what they reject).  ldx / ldy / flags as the entry points take them.  Additive (the ABI version stays).
 *   DX_PLAIN_PATH_WREG     conv_wreg_kernel, weights in registers: bf16 x and w, Cin = 128, Cout % 256 == 0, row strides multiples
 *                          of 8, N * ld within 32-bit byte offsets, neither DX_CONV_TRANSPOSED_OUT nor DX_CONV_ACCUMULATE
 *   DX_PLAIN_PATH_ROWS64   conv_gemm_kernel on 64-row tiles: one channel tile (Cout <= 128) with taps = 1, or with B * N <= 64000
 *   DX_PLAIN_PATH_ROWS128  ... on 128-row tiles: one channel tile with taps = 3 and B * N > 64000; every other GEMM with Cout > 128
 *   DX_PLAIN_PATH_ROWS256  ... on 256-row tiles: Cout > 128, taps = 3, Cin >= 512, bf16 weights and
 *                          ceil(N / 256) * B * ceil(Cout / 128) >= 1024 workgroups (the environment variable DX_CONV_WIDE_MI, read once,
 *                          replaces that last condition: 4 = always, 1 = 64-row tiles, any other value = 128-row tiles) */
enum { DX_PLAIN_PATH_WREG = 0, DX_PLAIN_PATH_ROWS64 = 1, DX_PLAIN_PATH_ROWS128 = 2, DX_PLAIN_PATH_ROWS256 = 3 };
int dx_conv1d_plain_path(int x_dtype, int w_dtype, int y_dtype, int taps, int Cin, int Cout, int B, int N, long ldx, long ldy, int flags);

/* The weights of a k = 3 conv in MFMA-fragment order: out[chunk][tap][half][block][lane][8] = w_packed[tap][32 block + (lane & 31)]
 * [32 chunk + 16 half + 8 (lane >> 5) + 0..7], block < Cout / 32; w_packed = the [3][Cout][Cin] bf16 packing of dx_pack_conv_weight
 * (either orientation), Cin and Cout multiples of 32.  A fragment (the B operand of one v_mfma_f32_32x32x16_bf16) is one contiguous
 * KiB, so a wave reads it from L2 straight into registers with one fully coalesced load and the weights never pass through LDS.
 * Users: the optional `w_frag` of dx_conv1d_ln / dx_conv1d_lnbwd (where dx_conv1d_ln_path says DX_LN_PATH_SPLITK: split-K
 * workgroups of 4 waves with 512 registers each, accumulators in AGPRs -- tiles of up to 128 rows: every wave a quarter of the
 * contraction for all 128 channels; 129..192 rows: half of the contraction x 64 channels per wave -- LDS carries the activation
 * tile only, the K slices added through LDS in a fixed order; results differ from the w_frag = NULL path by fp32 summation order
 * only), dx_conv1d_wfrag and dx_conv1d_wide. */
int dx_pack_frag_major(const void* w_packed, void* out, int Cin, int Cout, void* stream);
/* The same for n weights in one launch.  descs_dev: DEVICE array of n records {const void* src; void* dst; int Cin; int Cout;}
 * (dx_frag_desc_size() bytes each); max_elems = the largest Cin * Cout * 3 in the table. */
int dx_frag_desc_size(void);
int dx_pack_frag_major_batched(const void* descs_dev, int n, long max_elems, void* stream);

/* dx_conv1d for the WIDE k = 3 GEMMs (ConvNorm1D with 1024 -> 1024 channels in the prosody encoder's pre-net, model.py:341-363, and its
 * data gradient): bf16 x (B, N, Cin) and y (B, N, Cout), weights in fragment order, Cin % 128 == 0, Cout % 256 == 0, flags = 0 or
 * DX_CONV_RELU, bias fp32 or NULL.  256 rows x 256 channels per 4-wave workgroup (one wave per SIMD, 128 x 128 per wave = 256
 * accumulator registers), activation tile through an LDS-DMA ring, weight fragments from L2 into registers one chunk ahead:
 * 0.25 KB of LDS traffic per MFMA and half the L2 -> CU bytes of 256 x 128 tiles.  Position tiles: `plan` = dx_conv_tile_plan(lengths,
 * ..., n_tiles, table, halo) with ANY n_tiles >= B * ceil(N / 256) -- a multiple of 64 (256 CUs / 4 channel tiles of a 1024-channel output)
 * fills the chip in whole rounds; rows n >= lengths[b] + halo never reach a valid output and are written as zeros. */
int dx_conv1d_wide(const void* x, long ldx, const void* w_frag, const float* bias, void* y, long ldy, const int64_t* lengths,
                   const int* plan, int plan_tiles, int halo, int B, int N, int Cin, int Cout, int flags, void* stream);

/* Balanced position tiles for dx_conv1d_ln / dx_conv1d_lnbwd (optional `plan`; bf16 operands, Cin % 32 == 0, taps = 3 --
 * dx_conv1d_lnbwd also taps = 1).
 * The k = 3 GEMMs into the 128-channel stream are bound by what a compute unit fetches from L2, and every workgroup
 * fetches the whole weight slice whatever the height of its tile; a ragged batch (model.py:21-23 masks, lengths differ
 * 10x inside a batch) cut into fixed 128-row tiles ends a few tiles above a multiple of the 256 CUs.  The plan cuts
 * each utterance into equal pieces of <= 256 rows so that the batch is at most n_tiles pieces with the smallest possible
 * maximum height.  n_tiles: any count >= B * ceil(N / 256); dx_conv_tile_plan_size(B, N) is that bound rounded up to a
 * multiple of the 256 CUs (the default of the Python host side).  table: n_tiles x 4 int32 {b, n0, rows, f}
 * (f = padding rows of the batch each workgroup zero-fills beside its tile),
 * device memory, valid for every GEMM over the same lengths (one plan per batch).  Results are identical to the
 * unplanned call: same rows, same summation order per output; rows >= lengths[b] are written as zeros. */
int dx_conv_tile_plan_size(int B, int N);
int dx_conv_tile_plan(const int64_t* lengths, int B, int N, int n_tiles, int* table, int halo /* rows past the length that still
                      carry work: 0 for the LayerNorm-fused GEMMs (masked), 2 for the pre-net convs of dx_conv1d_wide */, void* stream);
/* One launch for everything a step derives from one lengths tensor: dx_conv_tile_plan(halo 0) into table0 (n_tiles0 entries),
 * dx_conv_tile_plan(halo 2) into table2 (n_tiles2 entries) and dx_length_order into order (B ints); any of the three
 * outputs may be NULL.  Same results as the three separate calls. */
int dx_batch_prep(const int64_t* lengths, int B, int N, int n_tiles0, int* table0, int n_tiles2, int* table2, int* order,
                  void* stream);

/* Pack an fp32 (Cout, Cin, taps) PyTorch conv / (Cout, Cin) linear weight for dx_conv1d.
 *   transpose_flip = 0: out[tap][co][ci] = w[co][ci][tap]                (forward operand)
 *   transpose_flip = 1: out[tap][ci][co] = w[co][ci][taps-1-tap]         (data-gradient operand) */
int dx_pack_conv_weight(const float* w, void* out, int out_dtype, int Cout, int Cin, int taps, int transpose_flip,
                        void* stream);
/* Every GEMM weight of the model in one launch.  descs_dev: DEVICE array of n records
 * {const float* w; void* out; int Cout, Cin, taps, transpose_flip; long begin;} (dx_pack_desc_size() bytes each); a
 * workgroup packs one 32 (Cout) x 32 (Cin) brick of one weight (all taps): begin = running sum of
 * ceil(Cout / 32) * ceil(Cin / 32) over the records before this one, total_bricks = that sum over all records. */
int dx_pack_desc_size(void);
int dx_pack_conv_weights_batched(const void* descs_dev, int n, long total_bricks, int out_dtype, void* stream);

/* Weight / bias gradient of dx_conv1d (and of nn.Linear with taps = 1), accumulated into dw (Cout, Cin, taps)
 * [PyTorch layout, fp32] and db (Cout) [NULL to skip]:
 *   dw[co][ci][tap] += sum_{b,n} dy[b, n, co] * x[b, n + tap - taps/2, ci];   db[co] += sum_{b,n} dy[b, n, co]
 * dy (B, N, Cout) rows lddy apart, x (B, N, Cin) rows ldx apart; compute_dtype = MFMA operand type.
 * lengths (NULL = none): rows n >= lengths[b] + 2 of dy are known to be zero and are skipped (the position axis is
 * split over workgroups by valid rows).  ws: scratch of dx_conv1d_wgrad_ws_floats(...) floats (contents irrelevant, must
 * stay untouched until the call has completed on `stream`): the per-workgroup partial sums go there and a second
 * launch adds them to dw in a fixed order.  ws = NULL: partial sums are added to dw with fp32 atomics instead
 * (slower, summation order varies run to run).  db always uses atomics (Cout values per workgroup). */
long dx_conv1d_wgrad_ws_floats(int B, int N, int Cin, int Cout, int taps);
int dx_conv1d_wgrad(const void* dy, int dy_dtype, long lddy, const void* x, int x_dtype, long ldx,
                    int compute_dtype, float* dw, float* db, const int64_t* lengths, float* ws, int B, int N, int Cin,
                    int Cout, int taps, void* stream);

/* n (<= 8) weight gradients over the SAME batch rows (B, N, lengths) in one call -- e.g. the four of an FFT block's backward pass
 * (model.py:182-186, 226-235: QKV and output projections, the two feed-forward convolutions): the n GEMM launches of dx_conv1d_wgrad,
 * then ONE launch that adds every partial tile to its dw (instead of one reduce launch behind each GEMM; same summation order per
 * element, so the results are those of n dx_conv1d_wgrad calls bit for bit).  descs: HOST array of n records; ws: scratch of
 * dx_conv1d_wgrad_multi_ws_floats(descs, n, B, N) floats (required). */
typedef struct DxWgradDesc {
  const void* dy; const void* x; float* dw; float* db;
  long lddy, ldx;
  int dy_dtype, x_dtype, Cin, Cout, taps, pad;
} DxWgradDesc;
int dx_wgrad_desc_size(void);
long dx_conv1d_wgrad_multi_ws_floats(const DxWgradDesc* descs, int n, int B, int N);
int dx_conv1d_wgrad_multi(const DxWgradDesc* descs, int n, int compute_dtype, const int64_t* lengths, float* ws, int B, int N,
                          void* stream);

/* ---- K5: LayerNorm(C) over channel-last rows fused with its neighbours (C in {128, 256, 1024}):
 *   s = dropout_pre(x) + residual;  y = LN(s) * gamma + beta;  y = dropout_post(y);
 *   y = film[b, :C] * y + film[b, C:];  y = 0 where n >= lengths[b]
 * Replaces nn.LayerNorm + nn.Dropout + residual add + FiLM + masked_fill at model.py:189-191 (attention),
 * 226-235 + 262 (FF block), 346-348/353-355/360-362 (prenet), 533-535/540-542 + 558-566 (predictor).
 * residual / film / lengths / s_out / mean+rstd may be NULL (feature off).  s_out, mean, rstd (fp32) are what
 * dx_layernorm_bwd needs.  Dropout masks are a counter-based hash of (seed, element index), regenerated
 * identically by the backward kernel; p = 0 disables.  skip_lengths (NULL = off): rows n >= skip_lengths[b] + 2 are
 * written as zeros without being read (padding early-out, same rule as dx_conv1d: unwritten from dx_fill_end on).  C in {128, 256, 512, 1024}. */
int dx_layernorm_fwd(const void* x, int x_dtype, const float* residual, const float* gamma, const float* beta,
                     const float* film, long ldf, const int64_t* lengths, const int64_t* skip_lengths, void* y,
                     int y_dtype, void* y_lp /* optional bf16 copy of y */, float* s_out, float* mean, float* rstd, int B, int N, int C, float p_pre,
                     uint64_t seed_pre, float p_post, uint64_t seed_post, const DxStepScalars* step, void* stream);

/* Backward of dx_layernorm_fwd.  dy: grad wrt y.  s_in: s_out of the forward (or x itself when there was no
 * residual / pre-dropout).  Outputs: ds = grad wrt s (equals the residual-branch gradient); dx_pre = grad wrt x
 * through dropout_pre (NULL when p_pre == 0: then it equals ds); dgamma, dbeta (C) and dfilm (B, 2C) are
 * ACCUMULATED with fp32 atomics (zero them first).  relu_input != 0: the normalised tensor was relu(conv) (prenet,
 * predictor); ds is then gated by (s_in > 0) so that it is the gradient of the conv's pre-activation. */
int dx_layernorm_bwd(const void* dy, int dy_dtype, const void* s_in, int s_dtype, const float* mean,
                     const float* rstd, const float* gamma, const float* beta, const float* film, long ldf,
                     const int64_t* lengths, const int64_t* skip_lengths, void* ds, void* dx_pre,
                     void* dx_pre_lp /* optional bf16 copy of dx_pre (of ds when p_pre == 0) */, int d_dtype,
                     float* dgamma, float* dbeta, float* dfilm, long lddf, int B, int N, int C, float p_pre, uint64_t seed_pre,
                     float p_post, uint64_t seed_post, int relu_input,
                     float* ws /* NULL: fp32 atomics; else dx_layernorm_bwd_ws_floats(B,N,C) floats: deterministic two-stage reduction */,
                     const DxStepScalars* step, void* stream);
long dx_layernorm_bwd_ws_floats(int B, int N, int C);

/* ---- K4: multi-head self-attention with key-padding mask, flash-style on MFMA (d_head 16 and 64: the tuned kernels of the
 * published 8- / 2-head configurations; 32 and 128 -- 4 heads / 1 head of a 128-wide model -- run the same templates untuned).
 * Replaces nn.MultiheadAttention's core (model.py:182-186): S = (q/sqrt(d)) k^T, pad keys -> -inf, softmax,
 * dropout on the probabilities, P v -- without materialising (B, H, N, N).
 *   qkv (B, N, 3E) = in-projection output [q | k | v], dtype = MFMA operand type (DX_BF16 or DX_F32)
 *   o   (B, N, E) same dtype;  lse (B, H, N) fp32 log-sum-exp per query (NULL at inference)
 * Queries n >= lengths[b] are not attended (their rows are zeroed by the following masked LayerNorm).
 * order: NULL, or the (B) int32 table of dx_length_order -- workgroups are then launched longest utterance first
 * (same results; a ragged batch finishes sooner). */
int dx_attention_fwd(const void* qkv, int dtype, const int64_t* lengths, const int* order, void* o, float* lse, int B, int N,
                     int H, int E, float p_drop, uint64_t seed, const DxStepScalars* step, void* stream);

/* Backward of dx_attention_fwd (autograd of model.py:182-186): dqkv (B, N, 3E) <- d_o (B, N, E).  delta_ws: (B, H, N) fp32 workspace.
 * algo: DX_ATTN_AUTO picks the fused kernel where it exists (bf16, d_head 16, N <= 1024: one workgroup per (utterance, head)
 * recomputes S / dP once for dQ, dK and dV) and the two-pass pair (dQ kernel, dK/dV kernel) elsewhere; DX_ATTN_TWO_PASS forces the
 * pair; DX_ATTN_FUSED returns DX_ERR_UNSUPPORTED where the fused kernel does not apply.  Both draw the forward's dropout mask.
 * delta_ws: dx_attention_bwd_ws_floats(B, N, H) floats of scratch (delta + the fused kernel's dQ partials); nothing in it has to be
 * initialised or to survive the call, so one grow-only buffer per stream serves every batch shape.
 * counters: dx_attention_bwd_counters(B, H) ints, the arrival counters of the fused kernel (an utterance of more than 512 keys is
 * shared by two workgroups): zero before the FIRST launch, and every launch puts the counters it used back to zero (the second
 * arrival of a pair resets its counter), so the caller zeroes a buffer of max(B * H) ints once per stream and keeps it.  May be
 * NULL when the fused kernel cannot run (fp32 operands, d_head 64, N > 1024, or DX_ATTN_TWO_PASS).  Calls that may run
 * CONCURRENTLY (different streams) must not share either buffer. */
long dx_attention_bwd_ws_floats(int B, int N, int H);
long dx_attention_bwd_counters(int B, int H);
enum { DX_ATTN_AUTO = 0, DX_ATTN_TWO_PASS = 1, DX_ATTN_FUSED = 2 };
int dx_attention_bwd(const void* qkv, const void* o, const void* d_o, int dtype, const float* lse,
                     const int64_t* lengths, const int* order, void* dqkv, float* delta_ws, int* counters, int B, int N, int H, int E,
                     float p_drop, uint64_t seed, const DxStepScalars* step, int algo, void* stream);

/* order[r] = index of the utterance with the r-th largest length (ties: lower index first), B <= 65536.  Host-side
 * analogue: the reference's collate sorts a batch by decreasing phoneme count (data_loader.py:246-250); the attention
 * kernels only use it as a launch order, so any batch order stays valid. */
int dx_length_order(const int64_t* lengths, int B, int* order, void* stream);

/* ---- K6: out = base + sum_f conv1d(1 -> 128, k = taps)(feat_f) + pos_table[n], zero where n >= lengths[b].
 * Energy / pitch embeddings + positional add + mask of the prosody encoder (model.py:400-414); the duration /
 * energy / pitch projections of the upsampler (model.py:618-628).  feats / ws / biases are HOST arrays of
 * nfeat (<= 3) device pointers: feat (B, N), w (128, 1, taps), bias (128).  base, pos_table, lengths may be NULL.
 * taps (ABI v13): 3 (the published conv_kernel) or 1. */
int dx_scalar_embed_fwd(const float* base, const float* const* feats, const float* const* ws,
                        const float* const* biases, int nfeat, const float* pos_table, const int64_t* lengths,
                        float* out, int B, int N, int C, int taps, void* stream);
/* dbase = dout * mask (may be NULL); dws / dbiases are accumulated with atomics. */
int dx_scalar_embed_bwd(const float* dout, const float* const* feats, int nfeat, const int64_t* lengths,
                        float* dbase, float* const* dws, float* const* dbiases, int B, int N, int C, int taps, void* stream);

/* ---- K7/K8: out[b, n] = table[ids[b, n]] + pos_table[n] for n < lengths[b], else 0 (model.py:497-504; the
 * positional gather replaces the host loops of PositionalEncoding.forward, model.py:132-150). */
int dx_embed_pos_fwd(const int64_t* ids, const float* table, const float* pos_table, const int64_t* lengths,
                     float* out, int B, int N, int C, void* stream);
int dx_embed_pos_bwd(const int64_t* ids, const float* dout, const int64_t* lengths, float* dtable, int B, int N, int C,
                     void* stream);

/* ---- K9: out[b] = sum_n x[b, n] / lengths[b] (model.py:419) and its backward dx[b, n] = dy[b] / lengths[b] for all N rows.
 * An utterance of length 0 has mean 0 and gradient 0. */
int dx_masked_mean_fwd(const float* x, const int64_t* lengths, float* out, int B, int N, int C, void* stream);
int dx_masked_mean_bwd(const float* dy, const int64_t* lengths, float* dx, int B, int N, int C, void* stream);

/* ---- K9: FiLM assembly (model.py:430-462).  g_raw / b_raw (B, W) are the gammas / betas projections, W = sum_m
 * nb[m] * ch[m] over the 3 FiLM-ed modules (encoder, predictor, decoder; nb / ch are HOST int[3]); post (2, sum nb)
 * or NULL.  film_m (B, nb[m], 2 ch[m]) = [post_g * g + 1 | post_b * b]. */
int dx_film_assemble_fwd(const float* g_raw, const float* b_raw, const float* post, float* film_enc, float* film_pp,
                         float* film_dec, const int* nb, const int* ch, int B, void* stream);
int dx_film_assemble_bwd(const float* g_raw, const float* b_raw, const float* post, const float* dfilm_enc,
                         const float* dfilm_pp, const float* dfilm_dec, float* dg_raw, float* db_raw, float* dpost,
                         const int* nb, const int* ch, int B, void* stream);

/* ---- K10/K14: exact-fp32 nn.Linear for the small heads (VALU, no operand rounding): FiLM projections
 * (model.py:427-428), speaker classifier (276-283), prosody projection 256 -> 3 (568-569), range projection
 * (634).  x (M, K), w (O, K), y (M, O); rows with (m % N) >= mask_lengths[m / N] are zero when mask_lengths != NULL.
 * Backward: dx = (dy * relu'(y)) W * dx_scale (NULL to skip; dx_scale = -lambda implements the gradient
 * reversal of model.py:34-38); dw / db accumulated with atomics. */
int dx_linear_small_fwd(const float* x, const float* w, const float* bias, float* y, const int64_t* mask_lengths,
                        int N, long M, int K, int O, int relu, void* stream);
int dx_linear_small_bwd(const float* dy, const float* y, const float* x, const float* w, float* dx, float dx_scale,
                        float* dw, float* db, const int64_t* mask_lengths, int N, long M, int K, int O, int relu,
                        void* stream);

/* out[b] = a[b] + table[ids[b]] (speaker-embedding add, model.py:423-424); backward scatter-adds dz into dtable. */
int dx_gather_add_fwd(const float* a, const float* table, const int64_t* ids, float* out, int B, int C, void* stream);
int dx_gather_add_bwd(const float* dz, const int64_t* ids, float* dtable, int B, int C, void* stream);

/* The two per-utterance heads behind the prosody embedding as single launches (C = 128).
 * dx_film_head_fwd = dx_gather_add_fwd + 2 x dx_linear_small_fwd + dx_film_assemble_fwd (model.py:419-462): z = emb + spk_table[ids]
 * (B, C), g_raw / b_raw = z W^T + bias (B, W), the three FiLM tensors assembled; bit-identical to the separate launches.
 * dx_film_head_bwd: from dfilm_* -- (dg_raw, db_raw) into the two (B, W) scratch buffers, dpost +=, d_emb += dz and d_spk_table[ids] += dz
 * (fp32 atomics), then the weight / bias gradients of both projections (+=, one thread per element: deterministic).
 * dx_classifier_fwd / _bwd (model.py:27-54, 276-292): three linear layers with ReLU; the backward WRITES d_emb = -lambda * (...) (the
 * gradient reversal), stores the gated gradients of layers 1 / 2 in two (B, C) scratch buffers and accumulates the six parameter
 * gradients.  S = number of logits (<= 128). */
int dx_film_head_fwd(const float* emb, const float* spk_table, const int64_t* spk_ids, const float* wg, const float* bg, const float* wb,
                     const float* bb, const float* post, float* z, float* g_raw, float* b_raw, float* film_enc, float* film_pp,
                     float* film_dec, const int* nb, const int* ch, int B, int C, void* stream);
int dx_film_head_bwd(const float* g_raw, const float* b_raw, const float* post, const float* z, const int64_t* spk_ids, const float* wg,
                     const float* wb, const float* dfilm_enc, const float* dfilm_pp, const float* dfilm_dec, float* dg_raw_ws,
                     float* db_raw_ws, float* d_emb, float* d_spk_table, float* dpost, float* dwg, float* dbg, float* dwb, float* dbb,
                     const int* nb, const int* ch, int B, int C, void* stream);
int dx_classifier_fwd(const float* emb, const float* w1, const float* b1, const float* w2, const float* b2, const float* w3,
                      const float* b3, float* h1, float* h2, float* logits, int B, int C, int S, void* stream);
int dx_classifier_bwd(const float* d_logits, const float* emb, const float* h1, const float* h2, const float* w1, const float* w2,
                      const float* w3, float* g1_ws, float* g2_ws, float* d_emb, float lambda, float* dw1, float* db1, float* dw2,
                      float* db2, float* dw3, float* db3, int B, int C, int S, void* stream);
int dx_add_inplace(float* dst, const float* src, long n, void* stream);           /* dst += src */
int dx_colsum(const void* x, int dtype, float* out, long rows, int C, void* stream); /* out[c] += sum_r x[r][c] (bias grads) */
int dx_scale(float* x, long n, float s, void* stream);
/* Layout helpers (the reference gets these from ATen views / copies around its modules):
 *   dx_transpose_last2: fp32 (B, R, C) -> (B, C, R) in y_dtype (DX_F32, or DX_BF16 = the rounding the first pre-net GEMM applies
 *   at operand load) -- the mel batch arrives as (B, n_mel, T) (model.py:744), kernels want rows;
 *   dx_unstack / dx_stack: y (M, K) interleaved <-> K planes of M floats, K <= 4 -- the duration / energy / pitch heads share one
 *   projection (model.py:567-575);  planes = host array of K device pointers;
 *   dx_fill_zero: stream-ordered memset of a device buffer. */
int dx_transpose_last2(const float* x, void* y, int y_dtype, int B, int R, int C, void* stream);
int dx_unstack(const float* y, float* const* planes, long M, int K, void* stream);
int dx_stack(float* y, const float* const* planes, long M, int K, void* stream);
int dx_fill_zero(void* p, size_t bytes, void* stream);
/* an empty single-thread launch: inside a stream capture, the first node recorded behind a fork decides which branch the graph
 * executor keeps on the forking node's queue -- the capturing trainer records one on the launch stream right behind every fork to
 * the weight-gradient stream (train.CapturedStep) */
int dx_anchor(void* stream);
/* one wave that occupies its hardware queue for `microseconds` (<= 100 000): HIP maps streams onto a few hardware queues
 * (GPU_MAX_HW_QUEUES, 4 by default) and two streams on the SAME queue run in submission order -- the weight-gradient stream, the
 * optimizer stream and RCCL's stream only overlap with the launch stream when they sit on other queues.  daft_exprt.streams probes
 * that with this kernel and picks streams that do (no reference counterpart: torch / DDP leave it to chance). */
int dx_spin(int microseconds, void* stream);

/* ---- K11: Gaussian upsampling (GaussianUpsamplingModule.forward, model.py:608-662), fp32, integer prefix sums exact.
 * dx_gu_prepare : xp = enc + conv(energy) + conv(pitch); rin = xp + conv(dur_float); r_pre = w_range . rin + b_range;
 *                 ranges = softplus(r_pre), 1 at l >= in_lengths[b].  r_pre / rin may be NULL (inference).
 * dx_gu_means   : means[l] = float(d[l]) / 2 + float(sum_{j<l} d[j]) from int64 durations; totals[b] = sum_l d.
 * dx_gu_upsample_fwd : weights (B, L, T) and out (B, T, 128).  With pos_table != NULL the decoder's positional add +
 *                 mask (model.py:696-701) is applied: out = (x_up + pos) where t < out_lengths[b], else 0. */
int dx_gu_prepare(const float* enc, const float* dur_float, const float* energy, const float* pitch,
                  const int64_t* in_lengths, const float* w_dur, const float* b_dur, const float* w_en,
                  const float* b_en, const float* w_pi, const float* b_pi, const float* w_range,
                  const float* b_range, float* xp, float* ranges, float* r_pre, float* rin, int B, int L,
                  int C, void* stream);
int dx_gu_means(const int64_t* durations_int, float* means, int64_t* totals, int B, int L, void* stream);
int dx_gu_upsample_fwd(const float* xp, const float* ranges, const float* means, const int64_t* in_lengths,
                       const int64_t* out_lengths, const float* pos_table, float* weights, float* out, int B,
                       int L, int T, int C, void* stream);
/* g = grad wrt `out`.  Outputs: dxp (grad wrt xp incl. the range path), drin (grad wrt rin), dr (B, L) grad wrt r_pre.
 * dw_ws (B, L, T) and dsum_ws (B, T) are fp32 workspaces. */
int dx_gu_upsample_bwd(const float* g, const float* xp, const float* weights, const float* means,
                       const float* ranges, const float* r_pre, const float* w_range,
                       const int64_t* in_lengths, const int64_t* out_lengths, float* dw_ws, float* dsum_ws,
                       float* dxp, float* drin, float* dr, int B, int L, int T, int C, void* stream);

/* ---- K13: the 7-term training loss and its gradients in one pass (DaftExprtLoss.forward, loss.py:54-99).
 * terms (8 floats, device): speaker, post_mult, duration, energy, pitch, mel_l1, mel_l2 (weighted), total.
 * mel / mel_t are (B, n_mel, T).  Gradient outputs (NULL to skip) are d(total * grad_scale)/d(pred);
 * d_post_mult is ACCUMULATED.  w_spk is the ramped adversarial weight (loss.py:22-28).
 * ws: NULL, or dx_loss_ws_floats(B, T) floats of scratch (no initialisation): with it (and the transposed mel gradient) the
 * per-workgroup terms are added in a fixed order by the last of THREE launches -- run-to-run identical loss terms, no same-address
 * atomics; without it four launches and fp32 atomics on terms[2..6].  With n_mel > 128 (the transposed-tile kernel's limit) ws is
 * ignored.  B, L, T, n_mel and n_spk_classes must be positive and n_post >= 0 (DX_ERR_SHAPE); every length >= 1. */
long dx_loss_ws_floats(int B, int T);
int dx_loss_fwd_bwd(const float* dur, const float* energy, const float* pitch, const float* dur_t,
                    const float* energy_t, const float* pitch_t, const int64_t* in_lengths, const float* mel,
                    const float* mel_t, const int64_t* out_lengths, const float* spk_logits,
                    const int64_t* spk_ids, const float* post_mult, float* d_dur, float* d_energy,
                    float* d_pitch, float* d_mel, float* d_spk_logits, float* d_post_mult, float* terms, float* ws,
                    int B, int L, int T, int n_mel, int n_spk_classes, int n_post, float w_spk, float w_post,
                    float w_dur, float w_energy, float w_pitch, float w_mel, float grad_scale,
                    int d_mel_transposed /* write d_mel as (B, T, n_mel) */,
                    const DxStepScalars* step /* NULL, or the step block: its w_speaker replaces w_spk */, void* stream);

/* ---- K15: torch.optim.Adam as configured at train.py:299-301 (coupled L2, bias correction, amsgrad off) over a
 * flat fp32 buffer; clip_grad_norm_ (train.py:399) folded in: grad_norm_sq (device scalar from dx_sumsq) and
 * clip_thresh (INFINITY = log only). */
int dx_sumsq(const float* x, long n, float* out, void* stream);
int dx_adam_step(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2,
                 float eps, float weight_decay, int step, const float* grad_norm_sq, float clip_thresh,
                 float* grad_norm_sq_accum /* NULL, or a device scalar that receives += sum(g^2) of this slice: the norm the
                 trainer logs (train.py:399 with an infinite threshold) without a pass of its own; per-section calls add up */,
                 const DxStepScalars* scalars /* NULL, or the step block: its lr / bias corrections replace `lr` and `step` */,
                 void* stream);

/* dx_adam_step over the whole flat buffer FUSED with the refresh of the MFMA operand copies of the GEMM weights (what
 * dx_pack_conv_weights_batched + dx_pack_frag_major_batched do after every optimizer step): one launch, the weights are read once.
 * bricks_dev: DEVICE array of n_weights records {long off; void* fwd; void* tr; void* frag_fwd; void* frag_tr; int Cout, Cin, taps,
 * pad; long begin;} (dx_adam_pack_desc_size() bytes): off = offset of the fp32 weight (Cout, Cin, taps) in p / g / m / v; fwd =
 * [taps][Cout][Cin], tr = [taps][Cin][Cout] with flipped taps (dx_pack_conv_weight layouts), frag_* = dx_pack_frag_major of those
 * (bf16, taps = 3, Cout and Cin multiples of 32), any of them NULL; begin = running count of 32 x 32 bricks, total_bricks their sum.
 * flats_dev: DEVICE array of n_flats records {long off, n, begin;} (dx_adam_flat_desc_size() bytes) covering every parameter that is
 * not a GEMM weight; begin = running count of dx_adam_flat_block()-element blocks, total_flat_blocks their sum.  out_dtype = dtype of
 * the copies (DX_BF16 / DX_F32).  Same arithmetic per element as dx_adam_step with an infinite clipping threshold; grad_norm_sq_accum
 * and scalars as there. */
int dx_adam_pack_desc_size(void);
int dx_adam_flat_desc_size(void);
int dx_adam_flat_block(void);
int dx_adam_pack_step(float* p, const float* g, float* m, float* v, const void* bricks_dev, int n_weights, long total_bricks,
                      const void* flats_dev, int n_flats, long total_flat_blocks, int out_dtype, float lr, float beta1, float beta2,
                      float eps, float weight_decay, int step, float* grad_norm_sq_accum, const DxStepScalars* scalars, void* stream);

/* ---- K16: float -> integer frame durations on the device (DaftExprt.get_int_durations model.py:789-812 +
 * duration_to_integer extract_features.py:69-111): optional dur_factors multiply (model.py:891), in-place
 * thresholding at filter_length / sampling_rate / 2, fp64 cumulative times, sample/frame counting in integers.
 * status[b]: 0 ok, 1 = the reference would raise IndexError (utterance shorter than one analysis window),
 * 2 = the reference's scatter would fail (symbol / duration count mismatch). */
int dx_int_durations(float* duration_preds, const float* dur_factors, int64_t* durations_int, int64_t* totals, int* status, int B, int L,
                     double sampling_rate, int filter_length, int hop_length, int centered, void* stream);

/* Inference-time prosody control (model.py:895-905, pitch_shift 814-834, pitch_multiply 836-864), in place.
 * mode 0 = 'add', 1 = 'multiply'. */
int dx_prosody_control(float* energy, float* pitch, const float* energy_factors, const float* pitch_factors,
                       const int64_t* durations_int, const int64_t* speaker_ids, const float* spk_pitch_mean,
                       const float* spk_pitch_std, int mode, int B, int L, void* stream);

/* ---- K17: mel / energy front-end of the synthesis path (extract_features.py:330-359 `mel_spectrogram_HiFi`,
 * 299-304 `extract_energy` as applied at generate.py:457 and extract_features.py:465-466).
 *   mel[b, m, f]   = log(max(sum_k fb[m, k] * sqrt(re^2 + im^2 + 1e-9), min_clip)),  X = STFT(wav[b], n_fft, hop, Hann,
 *                    center / reflect padding as torch.stft)            frames past the utterance: zeros
 *   energy[b, f]   = || exp(mel[b, :, f]) ||_2;      n_frames[b] = centered ? 1 + n / hop : 1 + (n - n_fft) / hop
 * wav (B, ldw) fp32, n_samples (B) int64.  twiddle (2 * n_fft floats) / window (n_fft floats): device tables filled
 * once by dx_mel_tables.  fb (n_mel, n_fft/2 + 1) dense filterbank with the non-zero bin range [fb_lo[m], fb_hi[m]) of
 * every filter.  mel (B, n_mel, T), energy (B, T).  T >= max n_frames.  n_fft in {256, 1024, 4096} (radix-4 FFT in LDS,
 * one workgroup per frame). */
int dx_mel_tables(float* twiddle, float* window, int n_fft, void* stream);
int dx_mel_spectrogram(const float* wav, long ldw, const int64_t* n_samples, const float* twiddle, const float* window,
                       const float* fb, const int* fb_lo, const int* fb_hi, float* mel, float* energy,
                       int64_t* n_frames, int B, int T, int n_fft, int hop, int n_mel, int centered, float min_clip,
                       void* stream);

/* ---- K18: Griffin-Lim preview audio (griffin_lim.py:63-198 as called from generate.py:130-137, 311-314).
 * n_fft in {256, 1024, 4096} and (dx_griffin_lim / dx_gl_normalise) a multiple of hop: DX_ERR_UNSUPPORTED otherwise.
 *
 * dx_gl_tables: twiddle (2 * n_fft floats) = exp(-2 pi i t / n_fft), window (n_fft floats) = SYMMETRIC Hann np.hanning(n_fft)
 * (griffin_lim.py:144), not the periodic window of dx_mel_tables.  Both computed in double, stored fp32.
 *
 * dx_mel_to_linear (replaces griffin_lim.py:63-114 `nnls` / `mel_to_linear`): per frame f < lengths[b],
 *   linear[:, f] ~ argmin_{x >= 0} 1/2 || A x - m ||^2,  m = input_is_log ? exp(mel[b, :, f]) : mel[b, :, f]
 * started like the reference at clip(pinv(A) m, 0), then `iters` FISTA steps of size `step` (1 / ||A||_2^2).  A = fb
 * (n_mel, n_fft/2 + 1) with the non-zero bin range [fb_lo[m], fb_hi[m]) of every filter; pinv_t (n_mel, n_fft/2 + 1) =
 * pinv(A)^T; bin_m / bin_w (n_fft/2 + 1, 2): the (at most two) filters of every bin and their weights (filter -1,
 * weight 0 where absent).  mel (B, n_mel, T); linear[b, k, f] at b * ld_lb + k * ld_lk + f * ld_lt, zero for
 * f >= lengths[b].  n_mel <= 256. */
int dx_gl_tables(float* twiddle, float* window, int n_fft, void* stream);
int dx_mel_to_linear(const float* mel, const int64_t* lengths, const float* fb, const int* fb_lo, const int* fb_hi,
                     const float* pinv_t, const int* bin_m, const float* bin_w, float* linear, long ld_lb, long ld_lk,
                     long ld_lt, int B, int T, int n_mel, int n_fft, int iters, float step, int input_is_log,
                     void* stream);
/* dx_griffin_lim (replaces griffin_lim.py:117-173 as called at 194 on linear_spec[:, :-2]): utterance b uses
 * F_b = max(lengths[b] - 2, 0) frames of mag (b * ld_mb + k * ld_mk + f * ld_mt, k < n_fft/2 + 1) and has
 * n_samples[b] = F_b * hop + n_fft samples (the reference's trailing hop of zeros included); frames start at
 * 0, hop, ..., (F_b - 1) * hop.  `iters` >= 1 iterations of: window, rFFT, keep the phase (R / |R|, 1 where R = 0),
 * swap in mag, irFFT, window, overlap-add in frame order (deterministic), divide by n_fft / hop / 2.  Start: x0 (B, ldx0)
 * when given, else standard normal noise hashed on the device from (seed, b, sample).  wav (B, ldw), ldw >= S =
 * max(T - 2, 0) * hop + n_fft, holds the result (unnormalised), zeros past n_samples[b].  ws: dx_gl_ws_floats(B, T, n_fft)
 * floats of scratch (NULL allowed when that is 0). */
long dx_gl_ws_floats(int B, int T, int n_fft);
int dx_griffin_lim(const float* mag, long ld_mb, long ld_mk, long ld_mt, const int64_t* lengths, const float* x0,
                   long ldx0, const float* twiddle, const float* window, float* wav, long ldw, int64_t* n_samples,
                   float* ws, int B, int T, int n_fft, int hop, int iters, uint64_t seed, void* stream);
/* dx_gl_noise: the start signal dx_griffin_lim draws when x0 is NULL (replaces griffin_lim.py:142, np.random.randn): x (B, ldx),
 * ldx >= S, standard normal from a counter-based hash of (seed, b, sample) and Box-Muller, zeros past n_samples[b]. */
int dx_gl_noise(float* x, long ldx, const int64_t* lengths, int B, int T, int n_fft, int hop, uint64_t seed, void* stream);
/* dx_gl_normalise (griffin_lim.py:196, waveform / max|waveform|) in place over the first n_samples of every row; an utterance
 * with lengths[b] <= 2 or all zeros gives zeros (the reference divides 0 by 0 there). */
int dx_gl_normalise(float* wav, long ldw, const int64_t* lengths, int B, int T, int n_fft, int hop, void* stream);

/* ---- K19: audio of the vocoder fine-tuning data set (fine_tune.py:91-115).
 *
 * dx_resample (replaces fine_tune.py:92, `librosa.load(wav_file, sr=hparams.sampling_rate)` when the file's rate differs:
 * librosa 0.8.1 `resample(res_type='kaiser_best')` -> resampy): x (B, ldx) fp32 with n_in[b] <= S_in samples per row ->
 * y (B, ldy), S_out = ceil(S_in * sr_out / sr_in) <= ldy, n_out[b] = ceil(n_in[b] * sr_out / sr_in) (librosa's length; may be
 * NULL).  With g = gcd(sr_in, sr_out), P = sr_out / g, Q = sr_in / g, output t < floor(n_in[b] * P / Q) is
 *     y[b, t] = sum_{j < taps} bank[j * P + t mod P] * x[b, floor(t Q / P) - (left - 1) + j]     (x = 0 outside [0, n_in[b]))
 * summed in fp32 in tap order; outputs from floor(n_in[b] * P / Q) on are 0 (librosa's fix_length pads the ceiling sample).
 * bank: (taps, P) fp32, tap-major, built on the host (daft_exprt/audio.py `resample_bank`) from the windowed-sinc table;
 * `left` taps sit at or before floor(t Q / P).  Equal rates copy x (bank may be NULL), as librosa skips resampling.
 * P * taps > dx_resample_max_weights() or a ratio whose 512-output run stages more than 16384 input samples:
 * DX_ERR_UNSUPPORTED (every rate pair among 8, 16, 22.05, 24, 32, 44.1 and 48 kHz fits). */
long dx_resample_max_weights(void);
int dx_resample(const float* x, long ldx, const int64_t* n_in, const float* bank, float* y, long ldy, int64_t* n_out,
                int B, long S_in, long S_out, int sr_in, int sr_out, int taps, int left, void* stream);
/* dx_ft_pack (replaces fine_tune.py:75-109: mel_spec_preds.cpu(), mel_spec_pred[:, :output_length], wav[begin:end],
 * (wav * 32768.0).astype('int16')): mel (b * ld_mb + m * ld_mk + f) fp32 (B, n_mel, T) -> mel_out, utterance b as a
 * contiguous (n_mel, T_b) block, T_b = min(lengths[b], T), blocks back to back in batch order (offset n_mel * sum_{i<b} T_i).
 * wav (B, ldw) fp32, crop (B, 2) int64 = (begin_b, len_b) with 0 <= begin_b, begin_b + len_b <= S -> wav_out int16, utterance b
 * at offset sum_{i<b} len_i: trunc(wav[b, begin_b + s] * 32768) for s < len_b.  Values outside the int16 range saturate to
 * -32768 / 32767 and NaN gives 0 (the reference's cast is undefined there); samples outside [0, S) are written as 0. */
int dx_ft_pack(const float* mel, long ld_mb, long ld_mk, const int64_t* lengths, int B, int n_mel, int T, const float* wav,
               long ldw, const int64_t* crop, long S, float* mel_out, int16_t* wav_out, void* stream);

/* ---- K20: pitch tracking (stands in for extract_features.py:222-269, which runs a prebuilt REAPER binary; not a port of it:
 * tests/pitch_oracle.py defines the arithmetic, DESIGN 9d the algorithm and its constants).  Additive entry points.
 *
 * dx_pitch_candidates: wav (B, ldw) fp32 with n_samples[b] <= S samples per row.  Analysis frame a < A_b = 1 + floor(n_b / step)
 * (step = sr * f0_interval samples, a double) is centred on sample floor(a * step + 0.5); its normalised cross-correlation
 *     r(k) = sum_{i < window} x[s + i] x[s + k + i] / (sqrt(e(0) e(k)) + floor),   s = centre - window / 2,  x = 0 outside [0, n_b)
 * over lags lag_min - 1 .. lag_max + 1 has its cross term summed in fp32 in tap order, e(k) = the energy of the lagged window
 * (from one running sum of squares, in double) and floor = window * (1e-2 * mean(x^2) + 1e-10).  cand_lag / cand_val (B, A, K),
 * K = dx_pitch_num_candidates(): the up to K largest local maxima above 0.3 at lags lag_min .. lag_max, lag and value
 * interpolated through their neighbours, in order of value (then of lag); empty slots and frames a >= A_b are 0.
 * mean_sq: B doubles of scratch.  A >= 1 + floor(S / step); window + lag_max + 1 > 2048: DX_ERR_UNSUPPORTED.
 *
 * dx_pitch_viterbi: the cheapest path per utterance over the K candidates and one unvoiced state per analysis frame.
 * back ((B, A, K + 1) bytes) and hz ((B, A) floats: sr / lag along the path, 0 where unvoiced or a >= A_b) are scratch and
 * by-product; log_pitch (B, T), T >= 1 + S / hop: mel frame t < n_frames[b] = 1 + n_b / hop takes analysis frame
 * min(floor(t * hop / step + 0.5), A_b - 1) and holds log(Hz), 0 where unvoiced and for t >= n_frames[b].  uv_cost scales the
 * cost of the unvoiced state (hparams.uv_cost). */
int dx_pitch_num_candidates(void);
int dx_pitch_candidates(const float* wav, long ldw, const int64_t* n_samples, double* mean_sq, float* cand_lag,
                        float* cand_val, int B, long S, int A, double step, int window, int lag_min, int lag_max,
                        void* stream);
int dx_pitch_viterbi(const float* cand_lag, const float* cand_val, const int64_t* n_samples, unsigned char* back, float* hz,
                     float* log_pitch, int64_t* n_frames, int B, long S, int A, int T, int sr, double step, int hop,
                     int lag_max, float uv_cost, void* stream);

/* ---- K21: per-utterance glue of training-feature extraction (extract_features.py:387-494, one utterance per process there).
 * Additive entry points.
 *
 * dx_wav_crop (replaces extract_features.py:426, `wav[int(sent_begin * fs): int(sent_end * fs)]`): x (B, ldx) fp32 with S <= ldx
 * valid columns, crop (B, 2) int64 = (begin_b, len_b) -> y (B, ldy): y[b, s] = x[b, begin_b + s] for s < len_b, 0 for
 * len_b <= s < ldy.  The mel front-end reflects at the edges of its row, so the crop becomes a row of its own.  Samples outside
 * [0, S) read as 0.
 *
 * dx_marker_durations (replaces extract_features.py:69-111, `duration_to_integer(float_durations, hparams, nb_samples=len(wav))`,
 * with its int() truncations and order of operations; K16 is the nb_samples=None form fed from predicted durations): spans
 * (B, L, 2) fp64 = the aligner rows' (begin, end) in seconds relative to the sentence begin, n_rows (B) of them per utterance,
 * n_samples (B) = length of the cropped waveform.  durations (B, L): the list the reference returns, left-aligned, zeros behind
 * it (all zeros on status 1 / 2); n_out (B, may be NULL): its length.  Times in fp64, counting in integers.  status (B):
 *   0 ok;  1 the reference raises IndexError (the rows run out before the frames do, or there is no frame at all);
 *   2 it raises ValueError (a row of zero length is reached);
 *   3 one of the asserts at extract_features.py:437-439 fails: the list is not n_rows long, or its sum is not the mel's frame
 *     count (centered ? 1 + n / hop : 1 + (n - filter_length) / hop, 0 below one window), or it holds a 0.
 *
 * dx_symbol_pool (replaces extract_features.py:272-296 `get_symbols_pitch` and 307-327 `get_symbols_energy`): energy / log_pitch
 * (B, ldt) fp32 with T <= ldt frames, durations (B, L) int64, n_rows (B).  Row l < n_rows[b] with duration d > 0 owns the next d
 * frames; a row with d == 0 gives 0 and owns nothing.  sym_energy[b, l] = mean of the row's frames; sym_pitch[b, l] = mean of
 * the row's frames that are > 0, 0 when there is none.  Sums in fp64 in an order fixed by the row alone, one rounding to fp32.
 * Rows l >= n_rows[b] are written as 0.  The durations of an utterance must not add up to more than T (frames past T are not
 * read). */
int dx_wav_crop(const float* x, long ldx, const int64_t* crop, float* y, long ldy, int B, long S, void* stream);
int dx_marker_durations(const double* spans, const int64_t* n_rows, const int64_t* n_samples, int64_t* durations, int64_t* n_out,
                        int* status, int B, int L, double sampling_rate, int filter_length, int hop_length, int centered,
                        void* stream);
int dx_symbol_pool(const float* energy, const float* log_pitch, long ldt, const int64_t* durations, const int64_t* n_rows,
                   float* sym_energy, float* sym_pitch, int B, int T, int L, void* stream);

/* ---- K22: the prosody-transfer metric (scripts/evaluation/compare_pitch_curves.py:5-45, `pcc_on_2_pitch_curve` with `_remove_unvoiced`,
 * `scipy.signal.resample` and `_pcc`).  Additive entry points.
 *
 * dx_curve_pcc: ref (B, ld_ref) fp32 with n_ref[b] <= T_ref values per row, dut (B, ld_dut) fp32 with n_dut[b] <= T_dut; nothing at or
 * past n_ref[b] / n_dut[b] is read.  Per row, independently of the other rows:
 *   1. with remove_unvoiced the values > 0 of each curve are kept, in order (NaN and values <= 0 count as unvoiced); without it all
 *      n values.  kept_ref[b] = num, kept_dut[b] = Nx: the lengths left.
 *   2. the kept dut is resampled to num values as scipy.signal.resample does for real input: with N = min(num, Nx),
 *        X[k] = sum_n x[n] e^{-2 pi i k n / Nx}, k = 0 .. N / 2;     y[m] = 1 / Nx * sum_k w_k Re(X[k] e^{+2 pi i k m / num}),
 *      w_0 = 1, w_k = 2, and for the bin N / 2 of an even N w = 2 when num < Nx and w = 1 when num >= Nx.  Direct sums in fp32 over
 *      the curve centred on its mean (added back to y); the angle index k n mod N is advanced in integers and looked up in a table
 *      computed in double.  resampled (B, ld_rs), ld_rs >= T_ref, may be NULL: y in [0, num), the rest of the row is not written.
 *   3. pcc[b] = mean((ref - mean ref) (y - mean y)) / (std ref * std y), means first, then the centred sums, in double.
 *   4. pcc[b] = NaN when num = 0 or Nx = 0 (the reference returns NaN for an empty ref and raises ValueError for an empty dut; NaN
 *      for both is an extension) or when a standard deviation is 0; `resampled` is NaN in [0, num) when Nx = 0.
 * One workgroup per row with both curves, one twiddle table and the spectrum in LDS: T_ref, T_dut > dx_curve_pcc_max_len() = 4096
 * (81 984 B of LDS, one workgroup per CU; 47 s of frames at hop 256, 22.05 kHz) returns DX_ERR_UNSUPPORTED before any launch. */
long dx_curve_pcc_max_len(void);
int dx_curve_pcc(const float* ref, long ld_ref, const int64_t* n_ref, const float* dut, long ld_dut, const int64_t* n_dut,
                 float* pcc, int* kept_ref, int* kept_dut, float* resampled, long ld_rs, int B, int T_ref, int T_dut,
                 int remove_unvoiced, void* stream);

/* ---- K23: the numbers behind the validation figures (logger.py:34-157), reduced on the device.  Additive entry points.
 *
 * dx_film_hist_range / dx_film_hist_count (replace `histogram_plot(..., bins=50)` over the FiLM tensors, logger.py:100-126 through
 * utils.py:18-36, i.e. numpy.histogram per block of gammas and of betas): film (rows, nb_blocks, width) fp32, rows = the utterances
 * of the validation set; the first width / 2 values of a block are its gammas, the rest its betas (logger.py:118-125).  Group
 * g = 2 * block + (0 gammas | 1 betas) holds rows * width / 2 values; G = 2 * nb_blocks groups.
 *   range: minmax (G, 2) fp32 = the group's (min, max), finite (G) int = 1 when every value of the group is finite; a group with a
 *          NaN or an infinity gets finite = 0 and minmax = (0, 0) (numpy raises there; a diagnostic must not stop a training run).
 *   count: edges (G, 51) fp64, ascending, built by the HOST from minmax as numpy.histogram does (numpy.linspace(lo, hi, 51) in
 *          double, lo - 0.5 .. hi + 0.5 when lo == hi); counts (G, 50) int64, cleared here.  Value x counts in bin i with
 *          edges[i] <= x < edges[i + 1], the last bin closed, values outside the table in none; the comparison runs in double
 *          against the table (an fp32 estimate only seeds the search), the counts are integer atomics: the result depends on
 *          neither the launch geometry nor any rounding and equals numpy.histogram(values as float64, bins=50)[0].  Groups with
 *          finite = 0 keep zero counts.
 *
 * dx_alignment_score (new; the numeric content of the "alignments" figure, logger.py:81-98 and 154-157): weights (B, L, T) fp32 as
 * dx_gu_upsample_fwd returns them, durations_int (B, L) int64, in_lengths / out_lengths (B) int64.  Symbol l < in_lengths[b] owns
 * the frames [c_l, c_l + d_l), c_l = sum_{j < l} d_j (exact integers), cut at out_lengths[b]; symbols at or past in_lengths[b]
 * own nothing.  Per utterance:
 *   frames[b] = min(sum_l d_l, out_lengths[b]), the owned frames;
 *   hits[b]   = the owned frames t whose argmax_{l < in_lengths[b]} weights[b, l, t] is the owner (lowest l among equal maxima);
 *   mass[b]   = the mean over the owned frames of weights[b, owner(t), t], summed in double, 0 when frames[b] == 0.
 * The target alignment comes from the batch's own durations_int -- the integers the upsampler was teacher-forced with -- where the
 * reference's figure re-derives integers from the FLOAT duration targets through duration_to_integer (logger.py:81-91): the score
 * compares the alignment with what actually drove it.  L > 8192: DX_ERR_UNSUPPORTED (one utterance's prefix sums live in LDS). */
int dx_film_hist_range(const float* film, float* minmax, int* finite, long rows, int nb_blocks, int width, void* stream);
int dx_film_hist_count(const float* film, const double* edges, const int* finite, int64_t* counts, long rows, int nb_blocks,
                       int width, void* stream);
int dx_alignment_score(const float* weights, const int64_t* durations_int, const int64_t* in_lengths, const int64_t* out_lengths,
                       int64_t* frames, int64_t* hits, float* mass, int B, int L, int T, void* stream);

/* ---- K24: the HiFi-GAN generator (Kong et al. 2020, `models.py` of jik876/hifi-gan) as batched inference -- the vocoder the
 * fine-tuning data set of K19 exists to train.  Additive entry points.  Activations are TIME-MAJOR fp32: (B, N, C) with rows
 * (samples) ld* floats apart and utterance b at row b * N; n_rows (B) int64 = the live rows of each utterance.  Rows < 0 or
 * >= n_rows[b] of an input are zeros and are NEVER READ; an output's rows >= n_rows[b] are written as zeros up to N, so an utterance
 * gets the same bits alone, in any batch, in any sub-batch.  No atomics, no split-K.  x, w_packed 16-byte aligned.
 *
 * dx_voc_conv: v = Conv1d(Cin, Cout, taps, dilation, padding dilation (taps - 1) / 2)(leaky_relu(x, in_slope)) + bias [+ residual]
 * (in_slope = 1: no activation).  w_packed [tap][Cout][Cin] in w_dtype = the operand type: DX_BF16 (v_mfma_f32_32x32x16_bf16, the
 * post-activation input rounded to bf16 at operand load) or DX_F32 (v_mfma_f32_32x32x2_f32, exact); accumulation fp32.
 *   y   NULL or (B, N, Cout): y = v;       residual NULL or laid out like y (may be y itself, never x);
 *   acc NULL or (B, N, Cout): acc = acc_scale * v when acc_init, acc += acc_scale * v otherwise -- the mean over the ResBlocks of
 *       a stage costs no launch of its own.
 * An input tile with its halo is staged in LDS once per 32-channel slice and read by every tap.  Cin and Cout multiples of 32 and
 * (taps - 1) * dilation <= 64 run on MFMA; anything else runs a plain VALU kernel of the same contract (correctness only).
 *
 * dx_voc_upsample: y (B, N * u, Cout) = ConvTranspose1d(Cin, Cout, k, stride u, padding (k - u) / 2)(leaky_relu(x, in_slope)) + bias,
 * x (B, N, Cin), as u polyphase convs through the same kernels: output row t u + p sums the taps j = j0 + s u, j0 = (p + pad) mod u,
 * of input rows t + (p + pad) div u - s.  w_packed [u][ceil(k / u)][Cout][Cin], entry (p, s) = weight[:, :, j]^T, zeros where j >= k.
 * k >= u, k - u even.  n_rows counts INPUT rows; output rows >= n_rows[b] * u are zeros.
 *
 * dx_voc_post: y (B, ldy) fp32, y[b, t] = tanh(Conv1d(C, 1, taps)(leaky_relu(x, in_slope))[t] + bias) for t < n_rows[b], 0 up to N.
 * w [tap][C] fp32, bias one float or NULL.  A VALU reduction, fp32 throughout. */
int dx_voc_conv(const float* x, long ldx, const void* w_packed, int w_dtype, const float* bias, const float* residual, long ldr,
                float* y, long ldy, float* acc, long lda, float acc_scale, int acc_init, const int64_t* n_rows, int B, int N,
                int Cin, int Cout, int taps, int dilation, float in_slope, void* stream);
int dx_voc_upsample(const float* x, long ldx, const void* w_packed, int w_dtype, const float* bias, float* y, long ldy,
                    const int64_t* n_rows, int B, int N, int Cin, int Cout, int k, int u, float in_slope, void* stream);
int dx_voc_post(const float* x, long ldx, const float* w, const float* bias, float* y, long ldy, const int64_t* n_rows, int B, int N,
                int C, int taps, float in_slope, void* stream);

/* ---- K25: copy-synthesis scores -- mel-cepstral distortion, F0 error and voicing error between a recording and a synthesis of
 * the same text, along the path of a dynamic time warping of their mel cepstra.  Additive entry points (the ABI version stays).
 * Per pair, independently of the other pairs: nothing at or past n_ref[b] / n_gen[b] is read, and a pair gives the same bits alone,
 * in any batch, with any padded extent and whatever the workspace held.  No atomics.
 *
 * dx_mel_cepstrum: mel (B, n_mel, T) fp32 (natural-log mel; utterances ld_b, channels ld_m floats apart) with n[b] <= T frames ->
 * cep (B, T, K) fp32, time-major, contiguous: cep[b, t, k] = sum_m dct[k, m] * mel[b, m, t] for t < n[b], zeros for n[b] <= t < T.
 * dct (K, n_mel) fp32 is the caller's table: rows 1 .. K of the orthonormal DCT-II, sqrt(2 / n_mel) cos(pi (m + 1/2) k / n_mel),
 * computed in double and rounded once (c0, the level, is dropped).  1 <= K < n_mel: DX_ERR_SHAPE otherwise; K * n_mel > 4096 (the
 * table is staged in LDS): DX_ERR_UNSUPPORTED.  The sum runs in order of m, fused multiply-adds in fp32.
 *
 * dx_dtw_align: the unconstrained DTW (no band, no slope weight) of cep_ref[b, :n_ref[b]] against cep_gen[b, :n_gen[b]], both
 * (B, T, K) fp32 contiguous, with
 *   d(i, j) = sqrt(sum_k (ref[i, k] - gen[j, k])^2)   in fp32, terms in order of k, computed on the fly (no cost matrix in memory),
 *   D(i, j) = d(i, j) + min(D(i - 1, j - 1), D(i - 1, j), D(i, j - 1)),  D(0, 0) = d(0, 0),
 * the predecessor being the FIRST minimum in the order diagonal, (i - 1, j), (i, j - 1): a later candidate replaces an earlier one
 * only when strictly smaller.  total[b] = D(n_ref - 1, n_gen - 1); path (B, T_ref + T_gen - 1, 2) int32: the cells (i, j) from
 * (0, 0) to (n_ref - 1, n_gen - 1), entries at or past path_len[b] are -1.  n_ref[b] == 0 or n_gen[b] == 0: path_len 0, total NaN.
 * ws: ws_stride bytes per pair of scratch, ws_stride >= T_ref * ceil(T_gen / 4) (2 bits per cell: 4 MiB per pair at the limit);
 * nothing in it has to be initialised or to survive the call.  The backtrack takes at most n_ref + n_gen - 1 steps and its move is
 * forced at i = 0 and at j = 0, so no workspace content and no non-finite cepstrum can walk it out of the matrix or make it loop
 * (non-finite values inside the live region are the caller's error: the path stays monotone, the totals are non-finite).
 * One workgroup per pair, three anti-diagonals of D in LDS (53 252 B with the code bytes in progress): T_ref, T_gen >
 * dx_dtw_max_len() = 4096 returns DX_ERR_UNSUPPORTED before any launch.
 *
 * dx_dtw_path_scores: per pair, over the entries p < path_len[b] of `path` (laid out as dx_dtw_align writes it for the same
 * T_ref, T_gen; an entry that is no cell of the pair is skipped and not counted), sums in double in an order fixed by path_len:
 *   mcd_db[b]        = (10 sqrt(2) / ln 10) * mean d(i, j)                                   NaN for an empty path
 *   f0_rmse_cents[b] = sqrt(mean((1200 / ln 2 * (lp_ref[b, i] - lp_gen[b, j]))^2)) over the entries with both values > 0 (log Hz,
 *                      <= 0 is unvoiced); NaN when there is none
 *   vuv_error[b]     = the share of entries where exactly one side is voiced;              NaN for an empty path
 *   voiced_pairs[b]  = the entries with both sides voiced;   used_len[b] = the entries counted.
 * lp_ref (B, ld_lpr) / lp_gen (B, ld_lpg) fp32 may both be NULL: f0_rmse_cents and vuv_error are then NaN, voiced_pairs 0. */
long dx_dtw_max_len(void);
int dx_mel_cepstrum(const float* mel, long ld_b, long ld_m, const int64_t* n, const float* dct, float* cep, int B, int n_mel,
                    int T, int K, void* stream);
int dx_dtw_align(const float* cep_ref, const int64_t* n_ref, const float* cep_gen, const int64_t* n_gen, float* total,
                 int* path, int* path_len, void* ws, long ws_stride, int B, int T_ref, int T_gen, int K, void* stream);
int dx_dtw_path_scores(const float* cep_ref, const int64_t* n_ref, const float* cep_gen, const int64_t* n_gen, const int* path,
                       const int* path_len, const float* lp_ref, long ld_lpr, const float* lp_gen, long ld_lpg, float* mcd_db,
                       float* f0_rmse_cents, float* vuv_error, int* voiced_pairs, int* used_len, int B, int T_ref, int T_gen,
                       int K, void* stream);

/* ---- K26: batches collated on the device from a training set that is resident there.  Replaces DaftExprtDataCollate.__call__
 * (data_loader.py:146-211: sort by phoneme count, right-zero-pad to the batch maxima) and the per-step H2D copy of its result.
 * Additive entry points (the ABI version stays).
 *
 * The store, packed once by the caller (U utterances, utterance u with L_u symbols and T_u frames):
 *   sym_off, frm_off (U + 1) int64: prefix sums of the L_u / T_u;   speaker (U) int64;
 *   sym, dur_i (sum L) int32, dur_f, sym_en, sym_pi (sum L) fp32: symbol ids, durations_int, durations_float, symbols_energy,
 *   symbols_pitch, utterance u at sym_off[u];
 *   frm_en, frm_pi (sum T) fp32: frames_energy / frames_pitch, utterance u at frm_off[u];
 *   mel (n_mel * sum T) fp32: utterance u at n_mel * frm_off[u], laid out as its .npy file is, (n_mel, T_u) row-major.
 * Rows of the store are 4-byte aligned only; the kernels assume no more.  An index outside [0, U) is clamped into it.
 *
 * dx_collate_order (data_loader.py:158-166, 190-205): idx (n_micro * B) int64 = the utterances of n_micro micro-batches of B each, in
 * the sampler's order (the same utterance may appear twice).  Each micro-batch is ordered on its own by L, descending and STABLE:
 * entry b goes to row  #{j : L_j > L_b} + #{j < b : L_j == L_b}  of its micro-batch.  For every output row (n_micro * B, int64 each):
 *   src_utt = the utterance, src_pos = its position b in the sampler's micro-batch, input_lengths = L, output_lengths = T,
 *   speaker_ids;
 * and, when the four bounds pointers are given (all or none), the `bounds` of a grouped step, with pads (n_micro, 2) int64 on the
 * device = (L_pad, T_pad) of each micro-batch as the HOST computed them:
 *   nmax_in / nmax_out = L_pad / T_pad of the row's own micro-batch,  skip_* = max(0, min(length, nmax - 2)).
 * pads is never NULL (n_micro pairs; read only with bounds).  One workgroup per micro-batch, the B phoneme counts in LDS:
 * B > dx_collate_max_batch() = 1024 returns DX_ERR_UNSUPPORTED before any launch.
 *
 * dx_collate_gather (data_loader.py:168-205): fills the padded batch of the rows src_utt (B_tot), in parse_batch's layout and dtypes:
 *   o_sym, o_dur_i int64 (B_tot, L_pad);  o_dur_f, o_sym_en, o_sym_pi fp32 (B_tot, L_pad);
 *   o_frm_en, o_frm_pi fp32 (B_tot, T_pad);  o_mel fp32 (B_tot, n_mel, T_pad).
 * EVERY element of every output is written, padding as zero: the buffers need no memset.  L_pad / T_pad are the caller's (the
 * allocation is); an utterance longer than them is cut.  A workgroup owns dx_collate_span() = 256 consecutive t (or l) of one row,
 * one per lane, so reads and writes are both coalesced; a long row is split over ceil(T_pad / span) + ceil(L_pad / span) workgroups.
 * B_tot > 65535: DX_ERR_UNSUPPORTED.  Neither entry point synchronises, allocates, or reads anything back. */
long dx_collate_max_batch(void);
long dx_collate_span(void);
int dx_collate_order(const int64_t* idx, const int64_t* sym_off, const int64_t* frm_off, const int64_t* speaker, long U,
                     const int64_t* pads, int64_t* src_utt, int64_t* src_pos, int64_t* input_lengths, int64_t* output_lengths,
                     int64_t* speaker_ids, int64_t* skip_in, int64_t* nmax_in, int64_t* skip_out, int64_t* nmax_out, int n_micro,
                     int B, void* stream);
int dx_collate_gather(const int64_t* src_utt, const int64_t* sym_off, const int64_t* frm_off, long U, const int* sym,
                      const float* dur_f, const int* dur_i, const float* sym_en, const float* sym_pi, const float* frm_en,
                      const float* frm_pi, const float* mel, int64_t* o_sym, float* o_dur_f, int64_t* o_dur_i, float* o_sym_en,
                      float* o_sym_pi, float* o_frm_en, float* o_frm_pi, float* o_mel, int B_tot, int L_pad, int T_pad, int n_mel,
                      void* stream);

/* ---- K27: synthesis-based forced alignment -- from a recording and the model's own synthesis of the same text to the frames each
 * symbol takes in the recording (daft_exprt/align.py; the reference starts from the .markers of an external aligner instead).
 * Additive entry points (the ABI version stays).  Per row / pair, independently of the others: nothing at or past the row's own
 * lengths is read, every output element is written, and the same bits come out alone, in any batch and with any padded extent.
 *
 * dx_active_span: energy (B, T) fp32, rows ld floats apart, with n_frames[b] <= T frames; rel_db <= 0 (DX_ERR_ARG otherwise).
 *   peak = max(energy[b, :n]),  thr = peak * f in fp32, f = 10^(rel_db / 20) computed in double on the host and rounded once,
 *   begin[b] = the first frame with energy >= thr,  end[b] = one past the last such frame           (int64 each).
 * n == 0, or a peak that is not > 0, gives (0, 0).  One workgroup per row, workgroup reductions, no atomics.
 *
 * dx_dtw_transfer: path (B, T_ref + T_gen - 1, 2) int32 / path_len (B) int32 exactly as dx_dtw_align writes them, the i axis being
 * the recording (n_ref[b] frames) and the j axis the synthesis (n_gen[b] frames); gen_durations (B, L) int64, the frames the model
 * gave each symbol of its synthesis, n_symbols[b] <= L of them; min_frames >= 1 (DX_ERR_ARG otherwise).
 *   A symbol s < n_symbols[b] with d_s > 0 is SOUNDING; its first synthesis frame is g_s = sum_{r < s} d_r.
 *   raw start      a_s = min{ i : (i, g_s) is an entry of the path }       (entries that are no cell of the pair are skipped)
 *   with the K sounding symbols in order, k = 0 .. K - 1:
 *     forward      a_k = max(a_k, a_{k-1} + min_frames)                    k = 1 .. K - 1
 *     then         a_k = min(a_k, n_ref - min_frames * (K - k))            k = 0 .. K - 1
 *   rec_durations[b, s] = a_{k+1} - a_k, the last sounding symbol n_ref - a_k;  0 for silent symbols and for l >= n_symbols[b]
 *   moved[b]  = how many starts the repair changed (int32): large where the synthesis and the recording disagree
 *   status[b] = 0  ok: every sounding symbol has >= min_frames frames and the row sums to n_ref - a_0, which is n_ref for every
 *                  path that starts in recording frame 0, as those of dx_dtw_align do
 *               2  nothing to transfer: path_len 0, K == 0, a negative d_s, sum d != n_gen, or a g_s the path never visits
 *               1  otherwise, n_ref < min_frames * K
 *   (2 is decided before 1.)  With status != 0 all durations and moved are 0.
 * Everything is integer.  One wave per pair: the per-frame minima in LDS (an integer minimum, whatever order the path entries
 * arrive in), the symbols 64 at a time with wave scans, the repair serially over K <= n_gen values in LDS.
 * T_ref, T_gen > dx_dtw_max_len() returns DX_ERR_UNSUPPORTED before any launch. */
int dx_active_span(const float* energy, long ld, const int64_t* n_frames, float rel_db, int64_t* begin, int64_t* end, int B, int T,
                   void* stream);
int dx_dtw_transfer(const int* path, const int* path_len, const int64_t* n_ref, const int64_t* n_gen, const int64_t* gen_durations,
                    const int64_t* n_symbols, int64_t* rec_durations, int* moved, int* status, int B, int T_ref, int T_gen, int L,
                    int min_frames, void* stream);

/* ---- K28: a learned aligner -- soft alignment between frame queries and symbol keys, the forward-sum (monotonic, blank-free CTC)
 * loss over it, and monotonic alignment search (MAS) for the hard path (daft_exprt/aligner.py; RAD-TTS / "One TTS Alignment to Rule
 * Them All", Glow-TTS; the reference starts from the .markers of an external aligner instead).  Additive entry points (the ABI
 * version stays).
 *
 * Common to the five entry points.  Utterance b has n_frm[b] <= T frames and n_sym[b] <= L symbols (int64, clamped into [0, T] /
 * [0, L]); every tensor is contiguous in the shape given.  Utterances are independent of each other; nothing at or past n_frm[b] /
 * n_sym[b] is read; EVERY output element is written (dead cells 0, -1 for the path); an utterance gives the same bits alone, in
 * any batch, with any padded extent T / L and whatever the outputs and workspaces held before.  No atomics: two runs are bit-equal.
 * T > dx_dtw_max_len() = 4096, L > dx_aln_max_symbols() = 1024 (one thread per symbol, one workgroup per utterance) or
 * A > dx_aln_max_dim() = 256 returns DX_ERR_UNSUPPORTED before any launch, as does B > 65535.  All arithmetic is fp32.
 * status[b] (forward sum and MAS): 2 when n_sym[b] == 0 or n_frm[b] == 0; otherwise 1 when n_frm[b] < n_sym[b] (no monotone path
 * with one frame per symbol exists); otherwise 0.
 *
 * dx_aln_logprob_fwd: q (B, T, A), k (B, L, A), temperature > 0 (DX_ERR_ARG otherwise) -> logp (B, T, L).  For t < n_frm, l < n_sym:
 *   d(t, l)     = sum_a (q[t, a] - k[l, a])^2          the difference form; a = 0 .. A - 1 in order, each term one fused multiply-add
 *   prior(t, l) = -u^2 * c,  u = (l + 1/2) / n_sym - (t + 1/2) / n_frm,  c = 1 / (2 prior_sigma^2) computed in double on the host
 *                 and rounded once;  0 when prior_sigma <= 0
 *   s(t, l)     = fma(-temperature, d, prior)
 *   logp(t, l)  = s(t, l) - (m + log(sum_l' exp(s(t, l') - m))),  m = max_l' s(t, l')
 * One wave per frame; lane i holds the symbols l = i, i + 64, ...: it sums its exp terms in order of l, then the 64 lane sums go
 * through the xor butterfly of dx_wave_sum (pairs at distance 32, 16, ... 1).  The order depends on l alone.
 *
 * dx_aln_logprob_bwd: q, k, logp as above and g = dLoss/dlogp (B, T, L) -> dq (B, T, A), dk (B, L, A); dead rows 0.
 *   G(t)     = sum_l g(t, l)                           per lane in order of l = i, i + 64, ..., then the butterfly
 *   ds(t, l) = g(t, l) - exp(logp(t, l)) * G(t)
 *   dq[t, a] = -2 temperature * sum_l ds(t, l) (q[t, a] - k[l, a])        l = 0 .. n_sym - 1 in order, fused multiply-adds
 *   dk[l, a] = +2 temperature * sum_t ds(t, l) (q[t, a] - k[l, a])        t = 0 .. n_frm - 1 in order, fused multiply-adds
 * Two launches: one wave per frame (dq and G), then one workgroup per tile of 8 keys, one thread per (key, channel), which walks
 * the frames itself: the sum over t is one thread's, hence deterministic.  row_ws: B * T floats of scratch (G).
 *
 * dx_aln_forward_sum: logp (B, T, L) -> alpha (B, T, L), loss (B), status (B) int32.
 *   alpha(0, 0) = logp(0, 0),  alpha(0, l > 0) = -inf
 *   alpha(t, l) = logp(t, l) + logaddexp(alpha(t - 1, l), alpha(t - 1, l - 1)),   alpha(t - 1, -1) = -inf
 *   logaddexp(x, y) = max + log1p(exp(min - max));  -inf for two -inf, never NaN
 *   loss[b] = -alpha(n_frm - 1, n_sym - 1)
 * Live cells of alpha that no path from (0, 0) reaches hold -inf.  status != 0: loss NaN, alpha all 0.
 *
 * dx_aln_forward_sum_bwd: logp, alpha as dx_aln_forward_sum wrote it, w (B) = dLoss/dloss[b] -> dlogp (B, T, L).
 *   beta(n_frm - 1, n_sym - 1) = 0, -inf for the other symbols of the last frame
 *   beta(t, l)  = logaddexp(logp(t + 1, l) + beta(t + 1, l), logp(t + 1, l + 1) + beta(t + 1, l + 1)),   the second -inf at l + 1 = n_sym
 *   gamma(t, l) = exp(alpha(t, l) + beta(t, l) - alpha(n_frm - 1, n_sym - 1))
 *   dlogp(t, l) = -w[b] * gamma(t, l),  and exactly +0 where gamma is 0 (every cell no path visits)
 * status != 0 (recomputed from the lengths): the row is all 0.
 *
 * dx_aln_mas: logp -> score (B) fp32, path (B, T + L - 1, 2) int32, path_len (B) int32, status (B) int32.
 *   V(0, 0) = logp(0, 0),  V(0, l > 0) = -inf,  V(t, l) = logp(t, l) + max(V(t - 1, l), V(t - 1, l - 1))
 * The predecessor of (t, l) is (t - 1, l); it is (t - 1, l - 1) only when that one is STRICTLY greater (the first-minimum rule of
 * dx_dtw_align, mirrored).  score[b] = V(n_frm - 1, n_sym - 1).  path / path_len are laid out exactly as dx_dtw_align writes them for
 * T_ref = T, T_gen = L, so dx_dtw_transfer reads them directly: the cells (t, l) from (0, 0) to (n_frm - 1, n_sym - 1), one entry per
 * frame (path_len = n_frm), entries at or past path_len -1.  status != 0: path_len 0, score NaN, the path all -1.
 * ws: ws_stride bytes of scratch per utterance, 8-byte aligned, ws_stride a multiple of 8 and >= 8 * T * ceil(L / 64) (DX_ERR_SHAPE
 * otherwise): one direction bit per cell, frame t of utterance b in the 64-bit words ws[b][t * ceil(n_sym[b] / 64) ...], bit l & 63
 * of word l >> 6.  Nothing in it has to be initialised or to survive the call, and its content is not trusted: the backtrack takes
 * exactly n_frm - 1 moves and is forced at l = 0 (stay) and at t = l (step), so no workspace content can walk it out of the lattice.
 *
 * The three lattice kernels: one workgroup per utterance, thread l owns symbol l and keeps its value of the previous frame in a
 * register; the l - 1 (l + 1) neighbour comes by one DPP move inside a wave, through a double-buffered LDS slot and one barrier per
 * frame between waves; L <= 64 launches a one-wave kernel without barriers.  Rows are fetched 8 frames ahead. */
long dx_aln_max_symbols(void);
long dx_aln_max_dim(void);
int dx_aln_logprob_fwd(const float* q, const float* k, const int64_t* n_frm, const int64_t* n_sym, float temperature,
                       float prior_sigma, float* logp, int B, int T, int L, int A, void* stream);
int dx_aln_logprob_bwd(const float* q, const float* k, const float* logp, const float* g, const int64_t* n_frm,
                       const int64_t* n_sym, float temperature, float* dq, float* dk, float* row_ws, int B, int T, int L, int A,
                       void* stream);
int dx_aln_forward_sum(const float* logp, const int64_t* n_frm, const int64_t* n_sym, float* alpha, float* loss, int* status, int B,
                       int T, int L, void* stream);
int dx_aln_forward_sum_bwd(const float* logp, const float* alpha, const float* w, const int64_t* n_frm, const int64_t* n_sym,
                           float* dlogp, int B, int T, int L, void* stream);
int dx_aln_mas(const float* logp, const int64_t* n_frm, const int64_t* n_sym, float* score, int* path, int* path_len, int* status,
               void* ws, long ws_stride, int B, int T, int L, void* stream);

/* ---- K29: per-symbol prosody targets -- a recording's timing, loudness and intonation, symbol by symbol, imposed on the prosody
 * predictor's outputs at synthesis time (daft_exprt/clone.py; the reference only scales the predictions by factors).  Additive entry
 * points (the ABI version stays).  Per utterance, independently of the others: one wave each, fp64 sums in an order fixed by the row
 * alone, no atomics, and the same bits alone, in any batch and with any padded extent.
 *
 * dx_clone_pool: energy / log_pitch (B, ldt) fp32 frame curves of the WHOLE recording with T <= ldt frames (pitch in natural-log Hz,
 * 0 = unvoiced, as K20 / K17 give them), begin (B) int64 = the first frame of the sounding stretch, durations (B, L) int64 and n_rows
 * (B) int64 as dx_symbol_pool takes them.  Row l < n_rows[b] with duration d > 0 owns the next d frames, the first row starting at
 * begin[b]; pooling is dx_symbol_pool's: the mean of the row's frames, for pitch over the frames > 0 only and 0 when there is none,
 * 0 for a row of duration 0, the sum in fp64, one rounding to fp32.  raw_energy / raw_pitch (B, L), each may be NULL: these means.
 *   self_stats (B, 4) fp32 = (mean, std) of the utterance's own non-zero pooled energies, then of its non-zero pooled pitches: the
 *     mean and the POPULATION std (as features_stats) of the fp32 means, two passes in fp64, rounded once; (0, 0) without a value.
 *   sym_energy / sym_pitch (B, L): v != 0 ? (v - mean) / std : 0 in fp32 (data_loader._standardise: zeros stay exactly 0), with
 *     mean_e / std_e and mean_p / std_p (B) fp32 when the pair is given, with the row's self_stats when the pair is NULL (a mean
 *     without its std is DX_ERR_ARG).
 *   dropped (B) int32: bit 0 (energy) / bit 1 (pitch) is set, and that quantity's outputs are all 0, when its statistics cannot
 *     be used: self statistics of fewer than two non-zero values or with a std that is not > 0; a given std that is not > 0.
 *   status (B) int32: 0, or 1 when begin[b] < 0, a duration is negative or begin[b] + sum of the durations > T: nothing is read
 *     for such a row and all its outputs are 0.  Frames at or past T are never read.
 * Every element of every output is written, rows l >= n_rows[b] as 0.
 *
 * dx_prosody_impose: in place on the predictor's dur (seconds), energy, pitch (B, L) fp32, for l < lengths[b] (the rest of a row is
 * left alone).  t_dur_frames (B, L) int64 or NULL, an entry < 0 meaning "no target for this symbol"; t_energy / t_pitch (B, L) fp32
 * or NULL; w_dur / w_energy / w_pitch (B, L) fp32 in [0, 1], each needed only with its target; dur_factors (B, L) fp32 or NULL (= 1).
 *   x = w == 0 ? x : w == 1 ? t : fmaf(w, t - x, x)     w = 0 leaves x and w = 1 yields t, bit for bit
 *   t_dur = frames * hop_length / sampling_rate, product and quotient in fp64, rounded once to fp32
 *   a ZERO energy / pitch target is a statement (silent / unvoiced), not a number: x = 0 when w >= 0.5, x unchanged otherwise
 *   exact[b] (B) int32 = 1 iff t_dur_frames is given and every l < lengths[b] has a target >= 0, w_dur == 1 and dur_factors == 1.0;
 *     0 otherwise; -1 when a weight of the row that would be used is outside [0, 1] or NaN: such a row is left untouched.
 * validate != 0: the weights are checked first and the call returns DX_ERR_ARG, naming the row, when one is outside [0, 1] -- this
 * reads B ints back and synchronises the stream.  validate == 0 never synchronises; the bad row surfaces as status 4 below.
 *
 * dx_prosody_impose_durations runs after K16 (dx_int_durations), on its outputs: for a row with exact[b] == 1
 *   durations_int[b, l] = t_dur_frames[b, l] for l < lengths[b] and 0 behind it,  totals[b] = their sum,
 *   dur[b, l] = the target in seconds again for l < lengths[b] (K16 zeroes what is shorter than filter_length / sampling_rate / 2,
 *   2 frames at the default settings; the integers of a recording hold symbols of 0, 1 and 2 frames, which K16 cannot return),
 *   status[b] = 0, or 3 when the targets sum to 0 (the host raises: there is nothing to synthesise).
 * A row with exact[b] == 0 keeps K16's result; one with exact[b] == -1 gets status 4 (the host raises). */
int dx_clone_pool(const float* energy, const float* log_pitch, long ldt, const int64_t* begin, const int64_t* durations,
                  const int64_t* n_rows, const float* mean_e, const float* std_e, const float* mean_p, const float* std_p,
                  float* sym_energy, float* sym_pitch, float* raw_energy, float* raw_pitch, float* self_stats, int* dropped, int* status,
                  int B, int T, int L, void* stream);
int dx_prosody_impose(float* dur, float* energy, float* pitch, const int64_t* t_dur_frames, const float* t_energy, const float* t_pitch,
                      const float* w_dur, const float* w_energy, const float* w_pitch, const int64_t* lengths, const float* dur_factors,
                      int* exact, int B, int L, int hop_length, double sampling_rate, int validate, void* stream);
int dx_prosody_impose_durations(const int* exact, const int64_t* t_dur_frames, const int64_t* lengths, float* dur,
                                int64_t* durations_int, int64_t* totals, int* status, int B, int L, int hop_length, double sampling_rate,
                                void* stream);

/* ---- K30: a grapheme-to-phoneme model learned from a pronunciation dictionary -- the CTC loss of a word with its gradient, and greedy
 * CTC decoding (daft_exprt/g2p.py; the reference runs `mfa g2p` on the words its dictionary lacks, generate.py:84-105).  Additive
 * entry points (the ABI version stays).
 *
 * Common to both.  logits (B, T, V) fp32, contiguous; word b has n_steps[b] <= T output steps (int64, clamped into [0, T]); class 0
 * is the blank.  Words are independent of each other; nothing at or past n_steps[b] / n_labels[b] is read; EVERY output element is
 * written; a word gives the same bits alone, in any batch, with any padded extent T / U / B and whatever the outputs and the
 * workspace held before.  No atomics: two runs are bit-equal.  T > dx_ctc_max_steps() = 256, U > dx_ctc_max_labels() = 127,
 * V > dx_ctc_max_classes() = 128 or B > 262140 returns DX_ERR_UNSUPPORTED before any launch.  All arithmetic is fp32.
 *   z(t)      = m + log(sum_v exp(x(t, v) - m)),  m = max_v x(t, v): lane i adds exp(x(t, i) - m) + exp(x(t, i + 64) - m) (a class at
 *               or past V counts 0), then the 64 lane sums go through the xor butterfly of dx_wave_sum
 *   lp(t, v)  = x(t, v) - z(t)
 *
 * dx_ctc_loss (generate.py:84-105): labels (B, U) int64 in [1, V - 1], n_labels[b] <= U of them (U = 0: labels may be NULL), w (B) fp32
 * -> loss (B) fp32 = -log p(labels | logits), status (B) int32, grad (B, T, V) fp32 = w[b] * dloss[b] / dlogits, in ONE launch.
 *   states s = 0 .. S - 1, S = 2 n_labels + 1: e(s) = blank for even s, labels[(s - 1) / 2] for odd s
 *   skip(s) = s odd, s >= 3 and e(s) != e(s - 2)
 *   lse3(a, b, c) = m + log(exp(a - m) + exp(b - m) + exp(c - m)), m = max(a, b, c), the terms added in this order; -inf for three -inf
 *   alpha(0, 0) = lp(0, blank),  alpha(0, 1) = lp(0, e(1)),  alpha(0, s > 1) = -inf
 *   alpha(t, s) = lp(t, e(s)) + lse3(alpha(t - 1, s), alpha(t - 1, s - 1), skip(s) ? alpha(t - 1, s - 2) : -inf)
 *   log p       = logaddexp(alpha(n_steps - 1, S - 1), alpha(n_steps - 1, S - 2))     (K28's logaddexp; the second -inf when S = 1)
 *   beta(n_steps - 1, s) = 0 for s = S - 1 and s = S - 2, -inf otherwise
 *   c(t + 1, s) = lp(t + 1, e(s)) + beta(t + 1, s)
 *   beta(t, s)  = lse3(c(t + 1, s), c(t + 1, s + 1), skip(s + 2) ? c(t + 1, s + 2) : -inf)      states at or past S count -inf
 *   gamma(t, s) = exp((alpha(t, s) + beta(t, s)) - log p)
 *   post(t, v)  = sum of gamma(t, s) over the states with e(s) = v: for a label class in order of s, starting from 0; for the blank
 *                 lane i adds gamma(t, 2 i) + gamma(t, 2 (i + 64)) (a state at or past S counts 0), then the butterfly of dx_wave_sum
 *   grad(t, v)  = w[b] * (exp(x(t, v) - z(t)) - post(t, v))   for t < n_steps;  0 for t >= n_steps
 * status[b]: 2 when n_steps[b] == 0; otherwise 3 when one of the word's labels is outside [1, V - 1]; otherwise 1 when
 * n_steps[b] < n_labels[b] + (number of u >= 1 with labels[u] == labels[u - 1]) (no path: equal neighbours need a blank between);
 * otherwise 0.  n_labels[b] == 0 is a valid word (the all-blank path).  status != 0: loss NaN, the word's grad all 0.
 * ws: B * T * (2 U + 1) floats of scratch (the alpha plane: T x S floats per word do not fit LDS beside the other words of a
 * workgroup).  Nothing in it has to be initialised or to survive the call; a lane reads back only cells it wrote in this call.
 *
 * dx_ctc_greedy (generate.py:84-105): -> ids (B, T) int32, n_out (B) int32, score (B) fp32.
 *   best(t)  = the class of the largest x(t, .), the LOWEST class among equal ones
 *   ids[b]   = best(0 .. n_steps - 1) with runs of one class collapsed to one entry, then the blanks dropped; n_out[b] entries,
 *              0 behind them up to T
 *   score[b] = sum over t, in order, of -log(sum_v exp(x(t, v) - max_v x(t, v)))  = sum_t max_v lp(t, v);  0 for n_steps = 0
 *
 * Both kernels: one wave per word, four words per workgroup, no barrier.  The loss kernel holds K = 1, 2 or 4 consecutive states per
 * lane (2 U + 1 <= 64 / 128 / 256); s - 1 and s - 2 are the lane's own registers or one DPP move away; emissions are gathered 8 (K = 1)
 * or 4 steps ahead of the chain.  Sort a batch by n_steps so the waves of a workgroup end together. */
long dx_ctc_max_steps(void);
long dx_ctc_max_labels(void);
long dx_ctc_max_classes(void);
int dx_ctc_loss(const float* logits, const int64_t* n_steps, const int64_t* labels, const int64_t* n_labels, const float* w, float* loss,
                int* status, float* grad, float* ws, int B, int T, int U, int V, void* stream);
int dx_ctc_greedy(const float* logits, const int64_t* n_steps, int* ids, int* n_out, float* score, int B, int T, int V, void* stream);

/* ---- K31: a CTC phone recogniser trained on the corpus's own feature files, to score the intelligibility of a synthesis -- the CTC
 * loss at utterance length with its gradient, greedy decoding, and the edit distance of the decode to the phones that were asked for
 * (daft_exprt/recognizer.py; the reference has no counterpart).  Additive entry points (the ABI version stays).
 *
 * dx_uctc_loss / dx_uctc_greedy: arguments, outputs, status codes and mathematics are EXACTLY those of dx_ctc_loss / dx_ctc_greedy in
 * the K30 comment above (z, lp, states, skip, lse3, alpha, log p, beta, c, gamma, post, grad, status; best, ids, score), with the same
 * guarantees: words are independent; nothing at or past n_steps[b] / n_labels[b] is read; EVERY output element is written; a row gives
 * the same bits alone, in any batch, with any padded extent T / U / B and whatever the outputs and the workspace held before; no
 * atomics, two runs are bit-equal; all arithmetic is fp32.  What differs:
 *   limits    T <= dx_uctc_max_steps() = 2048, U <= dx_uctc_max_labels() = 255 (S = 2 U + 1 <= 511), V <= dx_uctc_max_classes() = 128,
 *             B <= 65535; beyond any of them DX_ERR_UNSUPPORTED before any launch
 *   post      the blank's lane sum has four terms: lane i adds gamma(t, 2 i) + gamma(t, 2 (i + 64)) + gamma(t, 2 (i + 128)) +
 *             gamma(t, 2 (i + 192)) in this order (a state at or past S counts 0), then the butterfly of dx_wave_sum.  For S <= 255
 *             that is K30's sum; K31 is nevertheless only promised to agree with K30 within rounding, not bit for bit
 *   ws        2 * B * T * (2 U + 1) floats of scratch: the alpha planes of all rows, then the beta planes.  Nothing in it has to be
 *             initialised or to survive the call; the kernel reads back only cells it wrote in this call
 *   layout    ONE WORKGROUP of four waves per row -- at ~1 000 steps the chain over t is the cost, not the number of rows.  (1) all
 *             waves take the step log-sum-exps, four steps in flight per wave; (2) wave 0 runs the alpha chain forwards WHILE wave 1
 *             runs the beta chain backwards (they are independent; K30 runs them in turn), K = 1, 2, 4 or 8 consecutive states per
 *             lane (2 U + 1 <= 64 / 128 / 256 / 512), lane-edge neighbours one DPP move away, both planes to ws; (3) all waves turn
 *             alpha + beta into the gradient, four steps per wave at a time, the scatter to classes being K30's gather over a per-row
 *             list of label positions by class.  The greedy kernel: all waves take the arg-max and the step scores, one wave adds
 *             the scores in order of t and collapses the path.
 *
 * dx_edit_distance: ref (B, R) / hyp (B, H) int32 with n_ref / n_hyp (B) int64 clamped into [0, R] / [0, H] (R = 0 or H = 0: the pointer
 * may be NULL) -> counts (B, 4) int32 = substitutions, deletions, insertions, matches of one canonical cheapest alignment of
 * ref[b, :n_ref[b]] with hyp[b, :n_hyp[b]].  Cell (i, j) aligns the first i reference entries with the first j of the hypothesis:
 *   (i, 0) is i deletions, (0, j) is j insertions; otherwise the cheapest, at unit costs, of
 *     diagonal   (i - 1, j - 1) -> (i, j): a match when ref[i - 1] == hyp[j - 1], else a substitution (a match costs 0)
 *     deletion   (i - 1, j) -> (i, j)
 *     insertion  (i, j - 1) -> (i, j)
 *   among equal costs the diagonal wins, then the deletion, then the insertion.  The counts ride along with the cell, so there is no
 *   back-trace: a cell stores its substitutions and deletions, and i and j give the rest (matches = i - sub - del, insertions =
 *   j - i + del, cost = sub + del + insertions); counts[b] is cell (n_ref, n_hyp).
 * All-integer, every element written, nothing at or past the lengths read, rows independent of their batch.  One workgroup per pair walks
 * the anti-diagonals with three of them in LDS (as dx_dtw_align does).  R or H > dx_edit_max_len() = 2048 or B > 65535 returns
 * DX_ERR_UNSUPPORTED before any launch. */
long dx_uctc_max_steps(void);
long dx_uctc_max_labels(void);
long dx_uctc_max_classes(void);
long dx_edit_max_len(void);
int dx_uctc_loss(const float* logits, const int64_t* n_steps, const int64_t* labels, const int64_t* n_labels, const float* w, float* loss,
                 int* status, float* grad, float* ws, int B, int T, int U, int V, void* stream);
int dx_uctc_greedy(const float* logits, const int64_t* n_steps, int* ids, int* n_out, float* score, int B, int T, int V, void* stream);
int dx_edit_distance(const int* ref, const int64_t* n_ref, const int* hyp, const int64_t* n_hyp, int* counts, int B, int R, int H,
                     void* stream);

/* ---- K32: a speaker encoder trained on the corpus's own feature files, to score WHOSE voice a synthesis has -- attentive statistics
 * pooling over the live steps of an utterance with its backward, and the score histograms of all verification trials of a set
 * (daft_exprt/speaker.py; the reference has no counterpart).  Additive entry points (the ABI version stays).
 *
 * dx_attn_stat_pool_fwd: h (B, T, C) fp32 time-major, a (B, T) fp32 attention logits, n_steps (B) int64 -> out (B, 2 C) fp32 and
 * stat (B, 2) fp32.  Per row b with n = clamp(n_steps[b], 0, T):
 *   m      = max_{t < n} a[t]                      l = sum_{t < n} exp(a[t] - m)                 stat[b] = (m, l)
 *   w[t]   = exp(a[t] - m) / l                     (the softmax of a over the live steps)
 *   mu[c]  = sum_{t < n} w[t] h[t, c]
 *   var[c] = sum_{t < n} w[t] (h[t, c] - mu[c])^2  -- about the mean, in a second pass over the row; never sum w h^2 - mu^2
 *   sd[c]  = sqrt(var[c] + 1e-5)                   out[b] = [mu, sd]
 *   n = 0: out[b] = 0 and stat[b] = (0, 0).
 * dx_attn_stat_pool_bwd: the same h, a, n_steps, the out and stat of the forward and g_out (B, 2 C) = [g_mu, g_sd] -> g_h (B, T, C),
 * g_a (B, T), with d[t, c] = h[t, c] - mu[c]:
 *   g_h[t, c] = w[t] (g_mu[c] + g_sd[c] d[t, c] / sd[c])
 *   q[t]      = sum_c (g_mu[c] d[t, c] + g_sd[c] d[t, c]^2 / (2 sd[c]))      (the g_mu term centred: sum_t w[t] d[t, c] = 0)
 *   g_a[t]    = w[t] (q[t] - sum_{s < n} w[s] q[s])
 *   +0 at and past n, and everywhere in a row with n = 0.
 *   ws: B * ceil(C / 64) * T floats of scratch (the partial q of every 64-channel block); nothing in it has to be initialised.
 * Guarantees of both: nothing of h or a at or past n is read; EVERY element of every output is written; all arithmetic is fp32; no
 * atomics, two runs are bit-equal; a row gives the same bits alone, in any batch and with any padded extent T / B.
 *   layout    one workgroup of four waves per (row, 64-channel block): the lanes along C (64 lanes x 4 B are one 256-B segment of a
 *             step), the waves split t and combine through LDS in the order of the waves; the softmax weights of the row live in LDS.
 *             The backward's q needs all channels: every block writes its partial q to ws and a second launch (one workgroup per
 *             row) adds the blocks in order and forms g_a.
 *   limits    1 <= C <= dx_spk_pool_max_channels() = 1024, 1 <= T <= dx_spk_pool_max_steps() = 4096, 1 <= B <= 65535; beyond them
 *             DX_ERR_SHAPE / DX_ERR_UNSUPPORTED before any launch; a NULL pointer returns DX_ERR_ARG.
 *
 * dx_trial_counts: E (N, D) fp32, rows of unit length (not normalised here), spk (N) int32 -> counts (2, 4096) int64, zeroed by the
 * entry point.  For every unordered pair i < j:
 *   s   = sum_d E[i, d] E[j, d]                    (fp32, the exact-fp32 MFMA v_mfma_f32_32x32x2f32, d ascending in two interleaved
 *                                                  halves of every 16)
 *   bin = clamp(floor((s + 1) * 2048), 0, 4095)    (a NaN score counts in bin 0)
 *   counts[spk[i] == spk[j] ? 0 : 1][bin] += 1     -- row 0 the target trials, row 1 the non-target trials
 *   layout    the upper triangle of the N x N scores in 128 x 128 tiles, i < j masked on the diagonal tiles; a fixed number of
 *             persistent workgroups loop over the tiles, count into two LDS histograms and flush their nonzero bins ONCE with
 *             64-bit INTEGER global atomics -- order-independent, so two runs are bit-equal.
 *   limits    1 <= D <= dx_trial_max_dim() = 1024 (any D: the tail of the last 16 is zero-filled), 1 <= N <= dx_trial_max_rows() =
 *             65536; beyond them DX_ERR_SHAPE / DX_ERR_UNSUPPORTED before any launch; a NULL pointer returns DX_ERR_ARG. */
long dx_spk_pool_max_channels(void);
long dx_spk_pool_max_steps(void);
long dx_trial_max_dim(void);
long dx_trial_max_rows(void);
int dx_attn_stat_pool_fwd(const float* h, const float* a, const int64_t* n_steps, float* out, float* stat, int B, int T, int C,
                          void* stream);
int dx_attn_stat_pool_bwd(const float* h, const float* a, const int64_t* n_steps, const float* out, const float* stat,
                          const float* g_out, float* g_h, float* g_a, float* ws, int B, int T, int C, void* stream);
int dx_trial_counts(const float* E, const int* spk, int64_t* counts, int N, int D, void* stream);

/* ---- K33: weight gradients of the HiFi-GAN generator's convolutions (K24) -- what fine-tuning the vocoder adds; the forward and
 * both data gradients are K24 launches with re-packed weights.  Additive entry points (the ABI version stays).  Layout and contract
 * are K24's: x (B, N, Cin) and dy time-major fp32, rows ld* floats apart, n_rows (B) int64 = the live rows of x; rows < 0 or
 * >= n_rows[b] of x and of dy count as zeros and are NEVER READ.  w_dtype = the operand type: DX_BF16 rounds dy and
 * leaky_relu(x, in_slope) to bf16 when they are staged (v_mfma_f32_32x32x16_bf16), DX_F32 is exact (v_mfma_f32_32x32x2_f32);
 * accumulation fp32.  in_slope = the slope the forward applied to x (1: none).
 *
 * dx_vocoder_wgrad: dy (B, N, Cout);  dw [tap][Cout][Cin] fp32, the forward's packed order:
 *     dw[tap][co][ci] = sum_{b, t < n_rows[b]} dy[b, t, co] * leaky_relu(x[b, t + (tap - (taps - 1) / 2) * dilation, ci])
 * dx_vocoder_upsample_wgrad: dy (B, N * u, Cout), read as (B, N, u * Cout);  dw [u][ceil(k / u)][Cout][Cin] fp32, the order of the
 *     forward's w_packed: entry (p, s) contracts dy rows t u + p with x rows t + (p + pad) div u - s; entries whose tap
 *     j = (p + pad) mod u + s u >= k are written as zeros.
 * The contraction over the rows is split by the shapes alone (never by n_rows) over workgroups that write partial tiles to ws; a
 * second launch adds them in index order into dw, every element of which is written.  No atomics: two calls give the same bits.
 * ws: dx_vocoder_wgrad_workspace(B, N, Cin, Cout, k, u) bytes (u = 1 for dx_vocoder_wgrad, k = taps), 16-byte aligned; nothing in it has to
 * be initialised.  x, dy, dw 16-byte aligned, ldx and lddy multiples of 4.
 * Cin or Cout no multiple of 32, or (taps - 1) * dilation > 64: DX_ERR_UNSUPPORTED before any launch (conv_pre comes in with its
 * input channels zero-padded to a multiple of 32, as in the forward). */
long dx_vocoder_wgrad_workspace(int B, int N, int Cin, int Cout, int k, int u);
int dx_vocoder_wgrad(const float* x, long ldx, const float* dy, long lddy, int w_dtype, float* dw, float* ws, const int64_t* n_rows,
                 int B, int N, int Cin, int Cout, int taps, int dilation, float in_slope, void* stream);
int dx_vocoder_upsample_wgrad(const float* x, long ldx, const float* dy, long lddy, int w_dtype, float* dw, float* ws,
                          const int64_t* n_rows, int B, int N, int Cin, int Cout, int k, int u, float in_slope, void* stream);

/* ---- K34: the anti-aliased periodic activation of the BigVGAN generator (Lee et al. 2023: `Activation1d` with ratio 2 and
 * 12-tap filters around `Snake` / `SnakeBeta`), the one operation that generator adds to K24's.  Additive entry points (the ABI
 * version stays).  Layout is K24's: x, y (B, N, C) time-major fp32, rows ld* floats apart, n_rows (B) int64.
 *
 * dx_vocoder_snake: per utterance b with n = n_rows[b] live rows and per channel c, clamp(i, lo, hi) clamping the index,
 *     u[t] = 2 * sum_i f_up[t + 15 - 2 i] * x[clamp(i - 5, 0, n - 1)]       t in [0, 2 n), over the i with 0 <= t + 15 - 2 i < 12
 *     s[t] = u[t] + inv_beta[c] * sin(alpha[c] * u[t])^2
 *     y[m] = sum_{k < 12} f_down[k] * s[clamp(2 m + k - 5, 0, 2 n - 1)]     m in [0, n)
 * i.e. replicate-pad (5, 5), transposed conv of stride 2, crop [15 : -15], the activation, replicate-pad (5, 6), conv of stride 2.
 * The first clamp replicates the edge ROW of x, the second the edge VALUE of s (u is not continued past the edge).
 *   alpha, inv_beta  (C) fp32 on the device, in their final form: the host applies exp() for `snake_logscale` and computes
 *                    inv_beta = 1 / (beta + 1e-9) (beta = alpha for `snake`) in float64;
 *   filters          a HOST pointer to 24 floats, f_up[12] then f_down[12]; they travel in the kernel's argument block.
 * Sequence ends, K24's contract in its strict form: rows >= n_rows[b] of x are NEVER READ -- the edge row is replicated, the one place
 * where a dead row is not a zero; rows >= n_rows[b] of y are written as zeros up to N; n_rows[b] = 0 writes zeros only.  No atomics,
 * no LDS: u and s live in registers, every s is computed once per tile of dx_vocoder_snake_tile_rows() rows (plus 11 of halo), and
 * an utterance gets the same bits alone, in any batch, at any N, whatever the buffers held.  fp32 throughout, the accurate sinf.
 * y must not alias x.  x, y, alpha, inv_beta 16-byte aligned; C, ldx, ldy multiples of 4 (DX_ERR_UNSUPPORTED otherwise), more
 * workgroups than grid.x holds likewise -- all before any launch.
 *
 * dx_vocoder_post_clamp: dx_voc_post (arguments, contract and kernel) with clamp(v, -1, 1) in place of tanh(v): what the
 * generator ends in when its config says `use_tanh_at_final: false`. */
int dx_vocoder_snake_tile_rows(void);
int dx_vocoder_snake(const float* x, long ldx, const float* alpha, const float* inv_beta, const float* filters, float* y, long ldy,
                     const int64_t* n_rows, int B, int N, int C, void* stream);
int dx_vocoder_post_clamp(const float* x, long ldx, const float* w, const float* bias, float* y, long ldy, const int64_t* n_rows,
                          int B, int N, int C, int taps, float in_slope, void* stream);

/* ---- K35: the backward of K34 -- what fine-tuning a BigVGAN generator adds to K33.  Additive entry points (the ABI version stays).
 * Layout and notation are dx_vocoder_snake's: x, dy, dx (B, N, C) time-major fp32, rows ld* floats apart, n_rows (B) int64, alpha and
 * inv_beta (C) fp32 on the device in their final form, filters a HOST pointer to f_up[12] then f_down[12].
 *
 * dx_vocoder_snake_bwd: nothing is saved by the forward.  Per utterance b with n = n_rows[b] live rows and per channel c:
 *     u[t]   = 2 * sum_i f_up[t + 15 - 2 i] * x[clamp(i - 5, 0, n - 1)]                  t in [0, 2 n)   (recomputed, as in the forward)
 *     ds[t]  = sum_{m in [0, n), k in [0, 12) : clamp(2 m + k - 5, 0, 2 n - 1) = t} f_down[k] * dy[m]
 *     w[t]   = 2 * alpha[c] * u[t]
 *     du[t]  = ds[t] * (1 + inv_beta[c] * alpha[c] * sin(w[t]))
 *     dx[j]  = 2 * sum_{t in [0, 2 n), i : clamp(i - 5, 0, n - 1) = j, 0 <= t + 15 - 2 i < 12} f_up[t + 15 - 2 i] * du[t]
 *     dalpha[c]    = sum_b sum_t ds[t] * inv_beta[c] * u[t] * sin(w[t])
 *     dinv_beta[c] = sum_b sum_t ds[t] * (1 - cos(w[t])) / 2
 * The forward's first clamp replicates x's edge row, so dx[0] and dx[n - 1] also collect the five virtual rows on their side; its second
 * clamp replicates s's edge value, so ds[0] and ds[2 n - 1] also collect the samples t in [-5, -1] and [2 n, 2 n + 4]; dy outside
 * [0, n) counts as zero (it is not replicated); at n = 1 everything folds onto one row.  One accurate sincosf per sample, fp32 throughout.
 *   x and dy rows >= n_rows[b] are NEVER READ; dx rows n_rows[b] .. N are written as zeros; dx aliases neither input.
 *   Every dx[j] is one chain of fmas in one lane whose order depends on the row (and, at the two edge rows, on n) alone: an utterance gets
 *   the same bits alone, in any batch, at any N and at any tile height.  x and dy are read once, dx written once; u, ds, du stay in registers.
 *   tile_rows  rows per thread: 0 = the launcher's choice, otherwise one of dx_vocoder_snake_bwd_tile_rows(0), (1), ... (ascending; 0
 *              past the end).  The rule for 0: the LARGEST supported height at which B * ceil(N / height) * C / 4 threads are still
 *              >= 65536 (one wave on every SIMD of the 256 CUs), and the smallest height when none is.
 *   dalpha, dinv_beta  (C) fp32, both given or both null (null: the sums and the second launch are skipped; ws may be null then).
 *              No atomics: a thread sums, in double, the terms of the samples its tile owns (t in [2 m0, 2 m0 + 2 tile_rows)), writes one
 *              partial per (utterance, tile, channel) to ws, and a second launch adds the partials in index order in double and rounds
 *              once: two calls give the same bits.
 *   ws         dx_vocoder_snake_bwd_workspace(B, N, C) bytes (0 for B = 0), 16-byte aligned; nothing in it has to be initialised.
 * x, dy, dx, alpha, inv_beta 16-byte aligned; C and the leading dimensions multiples of 4 (DX_ERR_UNSUPPORTED otherwise), an unsupported
 * tile_rows and more workgroups than grid.x holds likewise -- all before any launch. */
int dx_vocoder_snake_bwd_tile_rows(int index);
long dx_vocoder_snake_bwd_workspace(int B, int N, int C);
int dx_vocoder_snake_bwd(const float* x, long ldx, const float* dy, long lddy, const float* alpha, const float* inv_beta,
                         const float* filters, float* dx, long lddx, float* dalpha, float* dinv_beta, void* ws, const int64_t* n_rows,
                         int B, int N, int C, int tile_rows, void* stream);

/* ---- K36: the magnitude spectrogram of a waveform and its gradient back to the waveform -- the one operation BigVGAN's
 * multi-resolution discriminator (Lee et al. 2023, section 3) adds to fine-tuning (csrc/spectrogram.hip).  Additive entry points (the ABI
 * version stays).  wav (B, S) fp32, rows ldw floats apart; n_samples (B) int64 on the device; window (n_fft) fp32 on the device, ANY
 * table (ones on [l, l + win), l = (n_fft - win) div 2, zeros elsewhere is torch.stft's window=None; a Hann table gives a Hann
 * spectrogram); twiddle (2 n_fft) fp32 from dx_spectrogram_tables (exp(-2 pi i t / n_fft) computed in double).
 *
 * dx_spectrogram: per utterance b with n = n_samples[b] and the resolution (n_fft, hop):
 *     p          = (n_fft - hop) div 2
 *     x~[s]      = x[r(s - p)],  s in [0, n + 2 p),   r(i) = -i (i < 0), 2 (n - 1) - i (i >= n), i otherwise        (torch's 'reflect')
 *     F_b        = 1 + (n + 2 p - n_fft) div hop
 *     X[f, k]    = sum_j window[j] * x~[f hop + j] * exp(-2 pi i j k / n_fft),   k in [0, n_fft / 2]
 *     mag[b,k,f] = sqrt(re^2 + im^2)                                (no epsilon: torch.norm of torch.stft(center=False))
 *   mag (B, n_fft / 2 + 1, T) fp32, contiguous; frames F_b .. T are written as zeros; wav samples at or past n_samples[b] are NEVER READ.
 * dx_spectrogram_bwd: nothing is saved by the forward, X is recomputed.  dmag (B, n_fft / 2 + 1, T) fp32, contiguous:
 *     G[f, k]    = dmag[b,k,f] * X[f, k] / |X[f, k]|,   0 where |X| = 0                  (torch's norm backward: never NaN)
 *     dy_f[j]    = window[j] * Re sum_{k = 0}^{n_fft / 2} G[f, k] * exp(+2 pi i j k / n_fft)    (the one-sided sum: bins are not doubled)
 *     dx~[s]     = sum_{f in [0, F_b) : 0 <= s - f hop < n_fft} dy_f[s - f hop]
 *     dx[i]      = dx~[i + p]  +  (1 <= i <= p ? dx~[p - i] : 0)  +  (n - 1 - p <= i <= n - 2 ? dx~[p + 2 (n - 1) - i] : 0)
 *   dwav (B, S) fp32, rows lddw floats apart; samples n_samples[b] .. S are written as zeros; dmag frames at or past F_b and wav samples at
 *   or past n_samples[b] are NEVER READ.  No atomics: one launch writes every live frame's dy_f to ws, a second gathers each sample's at
 *   most ceil(n_fft / hop) frames in ascending frame order and then the two folds in the order written above -- two calls give the same
 *   bits, and an utterance gets the same bits alone, in any batch and at any T.
 *   ws         dx_spectrogram_bwd_workspace(B, T, n_fft) bytes (0 for a non-positive argument), 4-byte aligned; nothing in it has to be
 *              initialised.
 * n_samples_host: a HOST array of the same B values as n_samples, which the launcher checks before any launch: n <= p or n + 2 p < n_fft
 * (torch refuses the same padding) returns DX_ERR_UNSUPPORTED naming the utterance, as do an n_fft outside {256, 512, 1024, 2048, 4096} and
 * a hop outside [1, n_fft]; n > S, F_b > T, ldw or lddw < S, B > 65535 or a non-positive B, S, T return DX_ERR_SHAPE; a NULL pointer
 * DX_ERR_ARG.  The kernels read the device copy and give an utterance that fails these conditions there no frame (mag and dwav zeros), so
 * no index leaves a buffer whatever n_samples holds.  fp32 throughout; one workgroup of n_fft / 4 threads and 16 n_fft bytes of LDS per
 * frame (the radix-4 Stockham loop of the audio kernels closed by one radix-2 stage for 512 and 2048). */
int dx_spectrogram_tables(float* twiddle, int n_fft, void* stream);
int dx_spectrogram(const float* wav, long ldw, const int64_t* n_samples, const int64_t* n_samples_host, const float* twiddle,
                   const float* window, float* mag, int B, int S, int T, int n_fft, int hop, void* stream);
long dx_spectrogram_bwd_workspace(int B, int T, int n_fft);
int dx_spectrogram_bwd(const float* wav, long ldw, const int64_t* n_samples, const int64_t* n_samples_host, const float* twiddle,
                       const float* window, const float* dmag, float* dwav, long lddw, void* ws, int B, int S, int T, int n_fft, int hop,
                       void* stream);

/* ---- K37: one scale of a multi-scale mel loss -- the log10-mel of a waveform, and the L1 between it and a target's with its gradient
 * back to the waveform (csrc/mel_loss.hip): the reconstruction term of BigVGAN-v2's fine-tuning.  Per scale it replaces what
 * `vocoder_train.LossMel` + `mel_l1` are for the single HiFi-GAN mel: a dense (n_fft, 2 bins) DFT matmul, a filter-bank matmul, the
 * log / clamp / abs torch ops and the autograd graph over them.  Additive entry points (the ABI version stays).
 * wav (B, S) fp32, rows ldw floats apart; n_samples (B) int64 on the device and n_samples_host, the same B values on the host, as K36;
 * window (n_fft) fp32 on the device, any table; twiddle (2 n_fft) fp32 from dx_mel_loss_tables (computed in double); fb (M, n_fft / 2 + 1)
 * fp32 on the device, non-negative, filter m non-zero only on the bins [fb_lo[m], fb_hi[m]) (an empty filter: lo = hi); pad = p >= 0, the
 * reflect padding per side (n_fft / 2 is torch.stft(center=True, pad_mode='reflect'), (n_fft - hop) / 2 HiFi-GAN's framing).
 *     x~[s]     = x[r(s - p)],  s in [0, n + 2 p)                                    (torch's 'reflect', n = n_samples[b])
 *     F_b       = 1 + (n + 2 p - n_fft) div hop
 *     X[f, k]   = sum_j window[j] x~[f hop + j] exp(-2 pi i j k / n_fft),  k in [0, n_fft / 2];   mag = sqrt(re^2 + im^2)
 *     mel[f, m] = sum_k fb[m, k] mag[f, k];   L[f, m] = log10(max(mel[f, m], eps))
 * dx_mel_loss_log_mel writes L as log_mel (B, T, M) fp32, frame-major; frames F_b .. T are zeros.
 * dx_mel_loss takes the generated waveform, target (B, T, M) from dx_mel_loss_log_mel and writes
 *     loss[b]   = sum_{f < F_b, m} |target[b, f, m] - L[b, f, m]|                                                      (B) fp32
 *     g[f, m]   = -sign(target - L) (mel >= eps ? 1 : 0) / (mel ln 10)         (sign(0) = 0: torch.abs's and torch.clamp's gradients)
 *     dmag[f,k] = sum_m fb[m, k] g[f, m]        over [bin_lo[k], bin_hi[k]), a run of filters that holds every m with fb[m, k] != 0
 *     G[f, k]   = dmag X / |X| (0 where |X| = 0);   dy_f[j] = window[j] Re sum_{k <= n_fft / 2} G[f, k] exp(+2 pi i j k / n_fft)
 *     dx~[s]    = sum_{f : 0 <= s - f hop < n_fft} dy_f[s - f hop]
 *     dwav[i]   = scale ( dx~[i + p] + (1 <= i <= p ? dx~[p - i] : 0) + (n - 1 - p <= i <= n - 2 ? dx~[p + 2 (n - 1) - i] : 0) )
 *   dwav (B, S) fp32, rows lddw floats apart, zeros at and past n_samples[b]; log_mel, if not NULL, gets the generated waveform's L as
 *   dx_mel_loss_log_mel writes it.  Samples at or past n_samples[b] and target frames at or past F_b are NEVER READ.  No atomics: frame
 *   terms and windowed gradients go to ws -- dx_mel_loss_workspace(B, T, M, n_fft) bytes (0 for a non-positive argument), nothing in it has
 *   to be initialised -- and are summed in an order the indices and n alone fix: two calls give the same bits, and an utterance gets the
 *   same bits alone, in any batch and at any T.
 * Checked on the host copy before any launch: n <= p or n + 2 p < n_fft (named by utterance), an n_fft outside {32, 64, 128, 256, 512,
 * 1024, 2048}, a hop outside [1, n_fft], M < 1 and eps <= 0 return DX_ERR_UNSUPPORTED; n > S, F_b > T, ldw or lddw < S, B > 65535 or a
 * non-positive B, S, T DX_ERR_SHAPE; a NULL pointer or a negative pad DX_ERR_ARG.  The kernels read the device copy and give an utterance
 * that fails these conditions no frame at all.  fp32 throughout; n_fft / 4 threads per frame, 256 / (n_fft / 4) frames per workgroup below
 * 1024 points. */
int dx_mel_loss_tables(float* twiddle, int n_fft, void* stream);
int dx_mel_loss_log_mel(const float* wav, long ldw, const int64_t* n_samples, const int64_t* n_samples_host, const float* twiddle,
                        const float* window, const float* fb, const int* fb_lo, const int* fb_hi, float* log_mel, int B, int S, int T,
                        int M, int n_fft, int hop, int pad, float eps, void* stream);
long dx_mel_loss_workspace(int B, int T, int M, int n_fft);
int dx_mel_loss(const float* wav, long ldw, const int64_t* n_samples, const int64_t* n_samples_host, const float* twiddle,
                const float* window, const float* fb, const int* fb_lo, const int* fb_hi, const int* bin_lo, const int* bin_hi,
                const float* target, float scale, float* loss, float* dwav, long lddw, float* log_mel, void* ws, int B, int S, int T, int M,
                int n_fft, int hop, int pad, float eps, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DAFT_EXPRT_HIP_H */
