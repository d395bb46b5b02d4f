/*
 * kosmosx_hip.h — C ABI of libkosmosx_hip.so: the MI355X (gfx950) hot path behind
 * kosmosx.model.Kosmos.forward / KosmosLanguage.forward.
 *
 * The reference (kyegomez/Kosmos-X) has no FFI of its own: its hot path is Python glue
 * (/root/reference/kosmosx/model.py:208-253, :310-320) over four third-party torch modules.
 * Each entry point below therefore cites the reference call site (or the third-party module
 * behind it) whose arithmetic it replaces.  INTEGRATION.md shows the ctypes
 * binding a reference maintainer would add.
 *
 * Conventions (all entry points):
 *   - return 0 on success, non-zero kx_status on failure; message via kx_last_error()
 *     (thread-local).  No C++ exception crosses the boundary.
 *   - every pointer is a caller-owned DEVICE pointer unless the parameter says "host";
 *     the library never allocates or frees user-visible memory.  Scratch is passed in with an
 *     explicit byte size (query with kx_*_workspace_bytes).
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *     launches are asynchronous on it, the library never synchronises, so every call is
 *     capturable into a hipGraph.
 *   - activations are row-major; "rows" are tokens.  Linear weights are [out, in] row-major
 *     (PyTorch convention) and are consumed as the K-contiguous B^T operand.
 *   - precision KX_PREC_BF16: GEMM/attention operands bf16 (MFMA 16x16x32 bf16), residual
 *     stream, LayerNorm statistics, softmax, GELU and all accumulators fp32.
 *     precision KX_PREC_F32: operands fp32 on the exact-f32 MFMA (16x16x4 f32).
 */
#ifndef KOSMOSX_HIP_H
#define KOSMOSX_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KX_ABI_VERSION 7

typedef enum {
  KX_OK = 0,
  KX_ERR_INVALID_ARG = 1,   /* shape / alignment / null pointer */
  KX_ERR_WORKSPACE = 2,     /* workspace too small */
  KX_ERR_LAUNCH = 3,        /* hipGetLastError() after a launch */
  KX_ERR_UNSUPPORTED = 4
} kx_status;

/* KX_PREC_BF16X3 (stage-level entry points only): bf16 MFMA arithmetic on split operands.  Every GEMM operand value v
 * travels as hi = bf16(v), lo = bf16(v - hi); an activation row is stored as [hi(K) | hi(K) | lo(K)] (dtype
 * KX_BF16X3, 3K bf16 per row) and the matching weight row as [hi | lo | hi], so an ordinary bf16 GEMM over 3K
 * accumulates a_hi*w_hi + a_hi*w_lo + a_lo*w_hi in fp32 — 16 mantissa bits per operand at 3x the bf16 MFMA work.
 * Attention and the residual stream stay fp32.  ~1e-4 parity with the fp32 reference (bf16: ~4e-2, fp32: ~1e-5).
 *
 * KX_PREC_F16C ("fp16, compensated"): the cheapest arithmetic that holds the north star's 1e-3 on the logits (measured
 * 1.4e-4; tools/precision_study.py).  One fp16 product carries the values; the two first-order rounding corrections
 * a_hi*dw + da*w_hi — each 2^-12 of the result, so 4 bits of them suffice — run on the block-scaled fp8 (e4m3) MFMA at
 * twice the fp16 rate: 2x the bf16 MFMA time instead of bf16x3's 3x.  Operand rows (dtype KX_F16C), K values = 4K bytes:
 *   activation row  [ h = fp16(a) (2K B) | e = fp8(a) (K B)                 | r = fp8((a - h) * 2^11) (K B) ]
 *   weight row      [ h = fp16(w) (2K B) | r = fp8((w - h) * 2^(s+11)) (K B) | e = fp8(w * 2^s) (K B)        ]
 * with one exponent s per weight ROW (|w| * 2^s <= 128), handed to the scaled MFMA as the E8M0 byte 127 - s; the
 * activation-side scale is the constant 2^-11.  A packed weight matrix is N such rows followed by the N scale bytes
 * (kx_gemm_args.w_scale).  fp8 conversions saturate at +-448; values must fit fp16 (|a| < 65504).  K % 128 == 0.
 * Attention takes fp32 q/k/v and multiplies fp16 (hi, lo) pairs: three products per score / output, P split the same
 * way.  The residual stream, statistics and accumulators stay fp32.
 *
 * KX_PREC_F16: plain fp16 operands (dtype KX_F16, 2 bytes per value) on the fp16 MFMA — the bf16 pipeline with three
 * more mantissa bits at the same speed.  On its own it leaves 4.6e-3 on the logits, but the error budget is very uneven
 * (tools/precision_study.py --budget fp16): the whole CLIP tower in plain fp16 moves the logits by 2.5e-4, every decoder
 * GEMM family by 1.4-2.7e-3.  The model-level mode "mixed" therefore runs the tower in KX_PREC_F16 and the Perceiver and
 * decoder in KX_PREC_F16C.  Values must fit fp16 (|x| < 65504). */
/* KX_PREC_F32W24 (kx_decoder_decode_step / kx_decoder_workspace_bytes only): KX_PREC_F32 arithmetic whose STREAMING copies
 * (kx_decoder_layer.w*_t, kx_decoder_weights.wout_t) are 24-bit weight planes (kx_gemm_args.w_tiled = 2); the row-major fp32
 * operands beside them hold the same values (low mantissa byte zero).  The decode step of f16c / mixed: 3 bytes per weight. */
/* KX_PREC_F32W16: the same with block-scaled 16-bit streaming copies (kx_gemm_args.w_tiled = 3): 2.125 bytes per weight. */
typedef enum { KX_PREC_BF16 = 0, KX_PREC_F32 = 1, KX_PREC_BF16X3 = 2, KX_PREC_F16C = 3, KX_PREC_F16 = 4, KX_PREC_F32W24 = 5,
               KX_PREC_F32W16 = 6, KX_PREC_F16CHL = 7 /* kx_attention only: KX_PREC_F16C on KX_F16HL q / k / v rows */ } kx_precision;
/* kx_gemm_args.f16c_corr: the fp8 correction products of a KX_PREC_F16C launch (ABI 7) */
typedef enum { KX_CORR_BOTH = 0, KX_CORR_WEIGHT = 1, KX_CORR_ACT = 2, KX_CORR_NONE = 3 } kx_f16c_corr;
/* KX_F16P (weight-streaming decode step only): fp32-pitched rows of fp16 PIECE pairs, value = hi + lo with hi = fp16(x) toward
 * zero and lo = fp16(x - hi) — per 32 values 128 bytes: [hi pieces, 64 B][lo pieces, 64 B], each as four 16-byte chunks g =
 * 0..3 holding values 4g..4g+3 then 16+4g..16+4g+3 of the 32 (the fragment order of kx_gemm_args.w_tiled = 3's fp16-pieces
 * kernel).  Written by kx_gemm(tile 16) / kx_attention_decode as `cdt` / `odt`, read by kx_gemm(tile 16, w_tiled = 4). */
/* KX_F16HL (round 5): an fp32-PITCHED row of 64-value head slots, each slot (256 bytes) = [64 fp16 hi | 64 fp16 lo] of
 * 2^8 x: hi = fp16(2^8 x) (saturating), lo = fp16(2^8 x - hi) — the operand pieces the KX_PREC_F16C attention kernel
 * multiplies, written ONCE by the qkv GEMM's epilogue instead of being re-derived from fp32 q / k / v by every workgroup
 * that loads a tile (kx_gemm: KX_PREC_F16C operands, XPos epilogue, N % 64 == 0; kx_attention: prec KX_PREC_F16CHL). */
typedef enum { KX_F32 = 0, KX_BF16 = 1, KX_BF16X3 = 2, KX_F16C = 3, KX_F16 = 4, KX_F16P = 5, KX_F16HL = 6 } kx_dtype;
/* KX_ACT_RELU / KX_ACT_SWISH (x * sigmoid(x)): the other two names torchscale's get_activation_fn knows
 * (`KosmosLanguage(activation_fn=...)`, /root/reference/tests/test_kosmos_lang.py:17-66).  Off the reference's default path:
 * offered by the generic 128 x 128 tile kernel of every precision (kx_gemm takes that kernel whatever `tile` says), not by
 * the weight-streaming decode kernels (tile 16).  Values 3 and 4 are internal variants of GELU. */
typedef enum { KX_ACT_NONE = 0, KX_ACT_GELU = 1, KX_ACT_QUICK_GELU = 2, KX_ACT_RELU = 5, KX_ACT_SWISH = 6 } kx_act;
typedef enum { KX_ATTN_FULL = 0, KX_ATTN_CAUSAL = 1 } kx_attn_mask;

int kx_version(void);
/* copies the calling thread's last error message (NUL-terminated) into buf; returns its length */
int kx_last_error(char* buf, size_t n);

/* ------------------------------------------------------------------------------------------
 * Primitive ops (exported so each kernel is parity-tested on its own)
 * ---------------------------------------------------------------------------------------- */

/* Row LayerNorm, y = LN(x [+ pre_add]) * gamma + beta, statistics in fp32.
 * Replaces torch.nn.LayerNorm / apex FusedLayerNorm as reached from torchscale
 * (self_attn_layer_norm, inner_attn_ln, final_layer_norm, ffn_layernorm, decoder.layer_norm),
 * HF CLIP (pre_layrnorm, layer_norm1/2) and flamingo (norm_media, norm_latents, FeedForward[0],
 * norm) — SURVEY.md §2.2 row "layer_norm".
 * x: [rows, cols] fp32.  y: dtype ydt.  cols % 4 == 0, cols <= 8192.
 * Output row remap (used to assemble the Perceiver's cat(media, latents) key/value input,
 * flamingo PerceiverAttention.forward `torch.cat((x, latents), dim=-2)`):
 *   out_row = (row / rows_per_group) * out_group_stride + out_row_offset + row % rows_per_group
 * pass rows_per_group = rows, out_group_stride = 0, out_row_offset = 0 for the identity map.
 * pre_add: optional [cols] fp32 vector added to every row before the statistics
 * (flamingo `x + media_pos_emb[:times]`). */
int kx_layernorm(const float* x, const float* pre_add, const float* gamma, const float* beta,
                 void* y, kx_dtype ydt, int64_t rows, int64_t cols, float eps,
                 int64_t rows_per_group, int64_t out_group_stride, int64_t out_row_offset,
                 void* stream);

/* C = epilogue(A · Wᵀ).  Replaces every nn.Linear on the path (cuBLAS GEMM + bias,
 * SURVEY.md §2.2) with the elementwise work that follows it fused into the epilogue.
 *   A [M,K] (lda), W [N,K] (ldw): dtype of `prec`.  K % 64 == 0 (bf16) / K % 32 == 0 (f32),
 *   lda/ldw multiples of 8 (bf16) / 4 (f32) elements, 16-byte aligned bases.
 *   epilogue, in order:  v = acc + bias[n];  v *= qscale for n < qcols;
 *     XPos rotation/scale for n < 2*xpos_dim when xpos tables are given
 *     (torchscale XPOS.forward + apply_rotary_pos_emb; q columns [0,xpos_dim) use the q tables,
 *      k columns [xpos_dim,2*xpos_dim) the k tables; position = row % xpos_T; head_dim 64);
 *     v = act(v);  v += residual[m,n] (fp32, may alias C);  store as cdt. */
typedef struct {
  const void* A; int64_t lda;
  const void* W; int64_t ldw;
  void* C; int64_t ldc; int32_t cdt;          /* kx_dtype */
  const float* bias;                          /* [N] or NULL */
  const float* residual; int64_t ldr;         /* [M,N] fp32 or NULL */
  int64_t M, N, K;
  int32_t act;                                /* kx_act */
  float qscale; int64_t qcols;                /* 1.0f / 0 to disable */
  const float* xq_cs; const float* xq_ss;     /* [xpos_T, 32] fp32: cos*scale, sin*scale for q */
  const float* xk_cs; const float* xk_ss;     /* same for k (downscale) */
  int64_t xpos_T; int64_t xpos_dim;           /* 0 to disable */
  int32_t prec;                               /* kx_precision */
  int32_t tile;                               /* 0 = auto; kernel variant override for tests/bench */
  /* Folded sub-LayerNorm (Magneto sub-LN: inner_attn_ln before out_proj, ffn_layernorm before fc2).
   * Consumer side: with row_stats [M,2] = (mean, rstd) of each A row and colsum [N] = Σ_k W[n,k], and W holding
   * γ ⊙ W_original, the epilogue starts with v = rstd·(acc − mean·colsum[n]); pass β·W_originalᵀ + b as `bias`.
   * Then y = LN(A)·Wᵀ + b without a LayerNorm pass over A.
   * Producer side: stats_out [M, N/64, 2] receives, per row and 64-column segment, (sum, Σ(x − segment mean)²)
   * of act(acc + bias) (N % 64 == 0; combines with bias and activation only) — kx_row_stats_finalize(seg_size 64)
   * turns them into (mean, rstd). */
  const float* row_stats; const float* colsum;
  float* stats_out;
  /* Optional split-K scratch for skinny problems (the 64x64 variant): when given, K is sliced over up to 16
   * workgroup rows so that the weights are streamed by ~512 workgroups instead of N/64; partial sums
   * [splits, M, N] fp32 are combined in slice order (deterministic) by a reduce kernel that owns the epilogue.
   * splitk: 0 = automatic, 1 = off, n = force n slices (tests). */
  void* splitk_ws; size_t splitk_ws_bytes; int32_t splitk;
  /* Weight-streaming variant, tile = 16 (bf16 or fp32 operands, M <= 16: incremental decoding, one token per sequence;
   * the fp32 form — exact-f32 MFMA, 4 bytes per weight — is the decode step of every precision that holds the north
   * star's tolerance: fp32 itself, and f16c / mixed, whose caches are fp32 already).  One launch
   * per GEMM: a workgroup owns 16 output columns, its waves split K and stream their weight rows straight into
   * MFMA fragments, the partial sums meet in LDS (fixed order) and wave 0 runs the epilogue above.  It takes three
   * extra inputs that remove the small kernels around a decode-step GEMM (all optional, this variant only):
   *   ln_gamma/ln_beta/ln_eps : A is then the raw fp32 rows [M,K] (lda in floats) and LayerNorm(A)*gamma+beta, rounded
   *       to bf16 exactly as kx_layernorm does (kept in fp32 for fp32 operands), is the operand (M*(K*es+16) <= 144 KB);
   *   stats_partials [M, stats_in_nseg, 2] + stats_in_seg + stats_eps : the consumer side of the folded sub-LayerNorm
   *       takes the producer's partial statistics directly (what kx_row_stats_finalize would turn into row_stats);
   *   stats_out_seg : the producer side emits its statistics per 16-column segment ([M, N/16, 2]; must be 16 here,
   *       0 or 64 for every other variant). */
  /* The TILE kernels take stats_partials TOGETHER WITH row_stats_scratch (+ colsum; ABI 7: the explicit, non-const field at the
   * end of this struct — until ABI 6 the const `row_stats` doubled as that output): row_stats_scratch [M, 2] is where
   * kx_gemm puts the finalised (mean, rstd) — it runs kx_row_stats_finalize itself before the launch — and `row_stats` must be
   * NULL.  The scratch is OVERWRITTEN; its contents after the call are unspecified: with tuning key 15 & 32 the pair split of
   * the 256 x 256 kernel with the accumulator-level residual epilogue finalises the partials inside the launch instead (each
   * workgroup the rows it finishes, while it waits for its partner; the same arithmetic bit for bit, stats_in_nseg <= 128) and
   * leaves the scratch untouched: one launch fewer per folded sub-LayerNorm, and measured 1 % SLOWER on the headline step (two
   * steps in flight hide the 5 us finalize launches; the in-launch walk sits on the hand-off) — opt-in, A/B. */
  const float* ln_gamma; const float* ln_beta; float ln_eps;
  const float* stats_partials; int64_t stats_in_nseg; int64_t stats_in_seg; float stats_eps;
  int32_t stats_out_seg;
  /* Row-owning split-K reduce (skinny problems, N <= 8192, N % 4 == 0): when ln_out is given, the reduce kernel — one
   * workgroup per output row — also writes LayerNorm(C[m, :]) * ln_out_gamma + ln_out_beta to ln_out [M, N] (dtype
   * ln_out_dt), i.e. the LayerNorm that would follow this GEMM costs no launch; with stats_partials it also takes the
   * folded-LN statistics straight from the producer's partials.  Only valid when the call will be split
   * (kx_gemm fails otherwise; the stage-level entry points check with the same rule before asking). */
  void* ln_out; int32_t ln_out_dt; const float* ln_out_gamma; const float* ln_out_beta; float ln_out_eps;
  /* KX_PREC_F16C only: [N] E8M0 scale bytes of the weight rows (see kx_precision).  A, W are KX_F16C rows: lda/ldw (and
   * ldc for a KX_F16C output) count 2-byte units (>= 2K, >= 2N), K is the number of values per row (K % 128 == 0). */
  const uint8_t* w_scale;
  /* Folded PRE-LayerNorm, producer side (the residual GEMMs out_proj / fc2: fp32 C with `residual`, N % 64 == 0, a tile
   * kernel of 128 rows or more, no split-K): besides C = x_new the epilogue writes x_new a second time as the operand
   * rows of the GEMM that follows the next LayerNorm (ln_operand_dt = KX_BF16 / KX_F16 / KX_F16C, dense [M, N]) and the
   * partial statistics (sum, M2 about the segment mean) of every 64-column segment to ln_operand_stats [M, N/64, 2].
   * kx_row_stats_finalize(seg_size 64) turns them into the (mean, rstd) the consumer takes as `row_stats` together with
   * gamma-folded weights, `colsum` and bias' = W·beta + b — torchscale's self_attn_layer_norm / final_layer_norm /
   * decoder.layer_norm and CLIP's layer_norm1/2 then cost no pass over the residual stream. */
  void* ln_operand_out; int32_t ln_operand_dt; float* ln_operand_stats;
  /* tile 16 (weight streaming) only: W is stored [ceil(N/16)][K/32][64][8] bf16 — block (p, c) holds rows 16p..16p+15,
   * columns 32c..32c+31 as 64 pieces of 16 bytes, piece l = row 16p + (l & 15), columns 32c + 8(l >> 4) .. +7 (the MFMA
   * fragment a lane loads), rows past N zero.  fp32 operands: [ceil(N/16)][K/16][64][4], piece l = row 16p + (l & 15),
   * columns 16c + 4(l >> 4) .. +3.  K % 32 == 0; ldw is ignored.
   * w_tiled = 2 (fp32 operands only): 24-BIT weights — each value is an fp32 number whose low mantissa byte is zero (round
   * the weight to 16 significant bits), stored as its top three bytes: [ceil(N/16)][K/32][1536 B], a block = rows 16p..16p+15
   * x columns 32c..32c+31 as 64 pieces of 16 B (piece l: the bf16 halves of row 16p + (l & 15), columns 32c + 4(l >> 4) .. +3
   * then 32c + 16 + 4(l >> 4) .. +3) followed by 64 pieces of 8 B (the third bytes of the same eight values).  The kernel
   * rebuilds the fp32 values in registers and multiplies on the exact-f32 MFMA: 3 bytes streamed per weight.
   * w_tiled = 3 (fp32 operands only): BLOCK-SCALED 16-BIT weights — [ceil(N/16)][K/32][1088 B]: 64 pieces of 16 B of int16
   * values q (the piece order of w_tiled = 2's halves) followed by the fp32 scales of the block's 16 rows (64 B);
   * w = (float)q * scale with scale = max|w| over the row's 32 columns / 32767 (1 for an all-zero run).  2.125 bytes per
   * weight; the row-major fp32 operand beside it holds exactly (float)q * scale.  Launches the VALU form does not take
   * (three rows and more; two rows of K = 8192) multiply fp16 PIECES on the fp16 MFMA: q = 1024 (q >> 10) + (q & 1023), the
   * activation as fp16 hi + lo (21-22 significant bits, absolute floor 2^-25); exact products, the block's scale applied to
   * each 32-k partial sum: within 2^-20 sum|a||w| of the exact-f32 form (tuning key 8 = 5).
   * w_tiled = 4: w_tiled = 3's planes, and A holds KX_F16P piece rows (lda in fp32 units, as for fp32 rows) that a producer
   * (this kernel with cdt = KX_F16P, kx_attention_decode with odt = KX_F16P) wrote: the fp16-pieces kernel then takes its
   * activation fragments as they are — the same bits it would make of the fp32 rows.  No ln_gamma; refused where the launch
   * would not be the fp16-pieces form (M <= 2 on the VALU, tuning key 8 = 4 / 5). */
  int32_t w_tiled;
  /* tile 16 (weight streaming) only — the residual stream of a decode step as a PAIR (x = xa + xb, always summed in that
   * order).  A residual GEMM with few columns (out_proj / fc2: N = 2048 -> 128 workgroups for 256 CUs) is launched with its
   * K extent cut into `ksplit` (1 or 2) parts, one workgroup per (16 columns, part): part 0 writes
   * C = (residual + residual2) + bias + its partial product, part 1 writes its partial product to C2 [M, N] fp32 (ldc) —
   * no cross-workgroup reduction, no atomics, bit-reproducible.  Needs an fp32 C, no activation / statistics producer / XPos /
   * ln_gamma, N % 16 == 0, K % (64 * ksplit) == 0.  residual2 (optional, with `residual`): second addend of the residual.
   * a_add (optional, with ln_gamma): second addend of the raw rows, LayerNorm(A + a_add) is the operand. */
  int32_t ksplit; void* C2; const float* residual2; const float* a_add;
  /* ABI 6 — scratch for the PAIR split of the 256x256 tile kernel (optional; 16-bit operand precisions).  A problem whose
   * 256x256 tiles fill about half of the chip's CUs (the decoder's out_proj / fc2 at M = 32 x 114: 15 x 8 = 120 tiles for 256
   * CUs) is launched as 2 x tiles workgroups: the two workgroups of a pair take one half of the K extent each, exchange half
   * of their fp32 accumulators through this scratch (write-through stores + an agent-scope flag hand-off: correct under any
   * workgroup placement) and each runs the epilogue of half of the tile's rows — the 256x256 main loop instead of the
   * 256x128 one, every CU busy, and half an epilogue per CU.  a + b == b + a: the result does not depend on which workgroup
   * finishes a row; it differs from the unsplit kernels by fp32 summation order only (two partial sums per element).
   * Layout: bytes [0, 4096) are the hand-off words — zero when the call is issued, zero again when it has completed (the
   * stage-level entry points clear them once per call); then one 128 KB slab per workgroup.  kx_gemm takes the split when
   * pair_ws_bytes >= 4096 + 2 * tiles * 131072, tiles % 8 == 0, 0.85 * CUs <= 2 * tiles <= CUs, K-tiles even, and the
   * epilogue has no activation / produced statistics (tile = 0: automatic; tile = 1024 asks for it and fails otherwise).
   * CONTRACT: (i) a workgroup spins on its partner's flag, so both must be RESIDENT — the rule 2 * tiles <= CUs with
   * one workgroup per CU (128 KB of LDS each) and in-order dispatch gives that; it is the dispatcher's guarantee, not the code's,
   * which is why the automatic rule never oversubscribes and the spin has no fallback; (ii) ONE scratch serves ONE stream at a
   * time: launches in flight on two streams need two scratches (the library's stage entry points and the trainer key theirs by
   * stream); a scratch shared across streams can clobber a flag.  (iii) The poll is BOUNDED: a workgroup gives up after 1 s of
   * the device's wall clock (a legitimate wait is the partner's K loop, < 1 ms), records 1 + its index in a sticky device word
   * and finishes with wrong rows — kx_pair_split_errors() reports it; a broken contract is an error code, not a hung GPU. */
  void* pair_ws; size_t pair_ws_bytes;
  /* ABI 7.  row_stats_scratch: see stats_partials above (tile kernels only; NULL otherwise).
   * f16c_corr (KX_PREC_F16C operands only; kx_f16c_corr): which of the two fp8 correction products a launch contracts.
   * A KX_F16C product is h_a.h_w + 2^-(s+11) (e_a.r_w + r_a.e_w); each correction term is half an fp16 pass of matrix time
   * and a quarter of the row's bytes.  KX_CORR_BOTH (0, default) is the arithmetic every parity statement of this library is
   * made for; KX_CORR_WEIGHT keeps e_a.r_w only (the weights stay 14-15 bits wide, the activations count as fp16: 1.5x the bf16
   * matrix time instead of 2x, the operand rows' r plane is never read); KX_CORR_ACT keeps r_a.e_w only; KX_CORR_NONE is plain
   * fp16 on KX_F16C rows.  The rows themselves do not change, so one packed weight matrix and one producer serve every value.
   * The stage-level entry points take their per-family assignment from tuning key 16 (DESIGN.md §5 has the measured table). */
  float* row_stats_scratch;
  int32_t f16c_corr;
  /* ABI 7 — IN-LAUNCH split-K reduction (optional; batch-1-sized problems: the 64 x 64 split-K launches with N <= 8192,
   * N % 4 == 0, 16-byte aligned rows, M <= workgroups <= 2 per CU).  splitk_flags = 2 x CUs 4-byte words (2 KB on MI355X), one
   * per workgroup, owned by ONE stream at a time like the scratch itself; cleared once when allocated (any later contents are
   * fine: every launch has its own epoch value).  The (tile, K slice) workgroups then store their partial tiles write-through,
   * each stores the launch's epoch into its own word, and the last M workgroups in dispatch order wait until every word shows
   * it and each reduces ONE whole output row — slices in slice order, the fused epilogue, folded-LN statistics from the
   * producer's partials, the LayerNorm that follows (ln_out): the row-owning reduce kernel's arithmetic bit for bit, one launch
   * instead of two.  NULL (or a problem that does not qualify, or tuning key 17 = 2): the separate reduce launch.  MEASURED on
   * MI355X (tools/coop_bench.py, profiles/r06_d_*): not faster than the two launches on any batch-1 shape — the write-through
   * partials and the arrival poll cost what the launch boundary they replace costs; kept as an opt-in, tested form.  The poll is
   * bounded like the pair split's (kx_pair_split_errors reports 0x80000000 | (1 + workgroup)). */
  uint32_t* splitk_flags;
} kx_gemm_args;
int kx_gemm(const kx_gemm_args* args, void* stream);
/* What kx_gemm would launch for `args`, as text — nothing is launched and no operand pointer is dereferenced (only their
 * alignment is looked at), so it runs on a machine without a GPU.  kx_gemm takes one snapshot of the tuning table, plans the
 * whole call from (args, snapshot, CU count) in one pure host function, and executes the plan; this entry point prints the same
 * plan.  One line per launch, in launch order: "kx_row_stats_finalize" (when the call finalises stats_partials first), then the
 * main kernel as "template<arguments> grid=XxY block=B" — gemm_kernel<T, BM, BN, ACT, EPI, NST, COOP>,
 * gemm_kernel_p3<T, ACT, PHASED> or gemm_kernel_p5<T, ACT, BM, EPI, KS2, BAL>, grid in workgroups; "gemv_fused" for
 * tile 16, whose launcher keeps its own variant choice — then the split-K reduce (splitk_reduce_kernel<ACT> or
 * splitk_reduce_rows_kernel<ACT, NJ>) when there is one; last, one line "plan tile=... kind=... ..." with the resolved tile, the
 * profile kind (kx_prof_kind) and the host flags.  cu_count <= 0: the current device's CU count (256 without a device).
 * A call kx_gemm would refuse returns the same code and leaves the same message; out_bytes too small is KX_ERR_INVALID_ARG
 * (4096 bytes always suffice).  A function-only addition: no struct changed, kx_version() stays 7. */
int kx_gemm_describe(const kx_gemm_args* args, int cu_count, char* out, size_t out_bytes);
/* Diagnostics of the pair split's bounded hand-off: *word_out = 0 when every poll since the last call met its partner, else
 * 1 + the index of the last workgroup that gave up (the word is then cleared).  SYNCHRONISES the device — call it after a
 * batch of steps, never inside the step. */
int kx_pair_split_errors(unsigned* word_out);

/* Fused softmax(Q·Kᵀ [+causal mask])·V, head_dim 64, flash-style (no T×T tensor in HBM).
 * Replaces torchscale MultiheadAttention's bmm/nan_to_num/+mask/softmax(fp32)/bmm chain,
 * HF eager_attention_forward, and flamingo PerceiverAttention's einsum/amax/softmax/einsum.
 * Q is expected pre-scaled (and XPos-rotated) by the producing GEMM epilogue.
 * nan_to_num (torchscale applies torch.nan_to_num to the scores before the mask; HF CLIP and flamingo do not): reproduced
 * where it can matter — KX_ATTN_CAUSAL launches (the decoder's self-attention) and kx_attention_decode in KX_PREC_F32, whose
 * operands span the fp32 range: NaN -> 0, +-inf -> +-FLT_MAX, then mask and softmax (tests/test_xpos_kat_gpu.py pins it for
 * kx_attention on an overflowing score row against the torch statement, tests/test_attention_decode_gpu.py for
 * kx_attention_decode against the float64 reference of tests/decode_ref.py).  KX_PREC_F16 / KX_PREC_F16C operands saturate at
 * +-65504, so a score cannot leave the fp32 range from finite inputs (|s| <= 64 * 65504^2); kx_attention_decode in
 * KX_PREC_F16C reads the fp32 cache and clamps like KX_PREC_F32.  DIVERGENCE: KX_PREC_BF16 operands do span
 * the fp32 range and that kernel does not clamp — an overflowing bf16 score row yields NaN where the reference yields a
 * one-hot row (bf16 is the throughput mode outside the north star's tolerance; the parity modes are fp32 / f16c / mixed).
 * DIVERGENCE: the same holds for kx_attention_decode on the bf16 cache (KX_PREC_BF16): no nan_to_num, an overflowing or NaN
 * score gives a NaN output row for that head.
 *   q: [B, Tq, H, 64] with element strides (q_batch_stride, q_row_stride), head h at +h*64.
 *   k, v: [B, Tk, H, 64] with (kv_batch_stride, kv_row_stride).   dtype of `prec`.
 *   out: [B, Tq, H*64] contiguous rows of out_row_stride elements, dtype odt. */
typedef struct {
  const void* q; int64_t q_batch_stride; int64_t q_row_stride;
  const void* k; const void* v; int64_t kv_batch_stride; int64_t kv_row_stride;
  void* out; int64_t out_batch_stride; int64_t out_row_stride; int32_t odt;
  int64_t B, H, Tq, Tk;
  int32_t mask;                               /* kx_attn_mask */
  int32_t prec;
  float* stats_out;                           /* optional [B*Tq, H, 2]: per row and head (sum, M2 about the head's mean)
                                                 of the 64 output values, for the folded inner_attn_ln */
  float* lse_out;                             /* optional [B,H,Tq] fp32: log-sum-exp of each query's scores: what
                                                 kx_attention_backward needs to rebuild P */
  /* ABI 4, training only (torchscale MultiheadAttention's dropout_module on the probabilities; the reference trains with
   * attention_dropout = 0.1, kosmosx/model.py:177): dropout_p > 0 keeps probability (b,h,q,k) iff Philox4x32-10(seed;
   * ((b*H + h)*Tq + q)*Tk + k, site) says so and scales it by 1/(1-p); the softmax normaliser stays un-dropped.  fp32
   * q/k/v (the wave-per-query kernel), or KX_PREC_BF16 q/k/v (the matrix-core kernel: one Philox block per query and four
   * keys, two when Tk % 4 != 0); fp32 output, no stats_out; zero = off. */
  float dropout_p; int32_t dropout_site; uint64_t dropout_seed;
} kx_attn_args;
int kx_attention(const kx_attn_args* args, void* stream);

/* (mean, rstd) per row from partial statistics: partials [rows, nseg, 2] = (sum, M2 about the segment mean) over
 * segments of seg_size values each; combined with Chan's parallel-variance formula (what a two-pass LayerNorm
 * computes, to fp32 rounding).  out [rows, 2] = (mean, 1/sqrt(var + eps)), var biased as in torch LayerNorm. */
int kx_row_stats_finalize(const float* partials, int64_t rows, int64_t nseg, int64_t seg_size, float eps,
                          float* out, void* stream);

/* Decoder input assembly (a6-a8): token gather + learned positions (fairseq offset 2) +
 * image-token splice + second position add.
 * Replaces Decoder.forward_embedding(text_tokens)[1] → torch.cat([x[:, :2], images, x[:, 2:]])
 * → Decoder.forward_embedding(model_input, token_embedding=model_input)[0]
 * (/root/reference/kosmosx/model.py:238-244).
 *   tokens [B,Tt] int64; embed [vocab,d] fp32; pos [max_pos,d] fp32; img [B,n_img,d] fp32 or
 *   NULL with n_img = 0 (KosmosLanguage path, model.py:319: single position add);
 *   out [B, Tt+n_img, d] fp32.  The n_img rows of img are spliced in after the first `splice_at`
 *   text rows (2 on the Kosmos path: "<s> <image>" | image features | "</image> text").
 *   Tt = 0, splice_at = 0 adds positions to an already-embedded sequence
 *   (forward_embedding(x, token_embedding=x)).  u1_alias: 1 = first forward_embedding's [1] return
 *   already contains positions (in-place `x += positions`), so text rows get positions
 *   twice.  Returns KX_ERR_INVALID_ARG ("position ... out of range") when Tt+n_img+2 > max_pos —
 *   the condition under which the reference's F.embedding raises IndexError.
 *   Token ids are clamped to [0, vocab) for memory safety.  pos_offset shifts every position index (0 on the
 *   forward path; the number of cached tokens when embedding the next token of an incremental decode). */
int kx_embed_splice(const int64_t* tokens, const float* embed, const float* pos, const float* img,
                    float* out, int64_t B, int64_t Tt, int64_t n_img, int64_t d, int64_t vocab,
                    int64_t max_pos, int64_t splice_at, int32_t u1_alias, int64_t pos_offset, void* stream);

/* (min, max) of n int64 token ids -> out2[0], out2[1] (device).  The kernels clamp ids for memory safety only; the
 * Python boundary calls this first and raises IndexError for ids outside [0, vocab), as torch.nn.functional.embedding
 * does on the reference's CPU path (/root/reference/kosmosx/model.py:238 -> Decoder.forward_embedding). */
int kx_token_range(const int64_t* tokens, int64_t n, int64_t* out2, void* stream);


/* ------------------------------------------------------------------------------------------
 * Token sampling on the device — the end of a decode step (added within ABI 7: one struct, two functions and one
 * kx_struct_id value are appended; no existing layout moves, so kx_version() stays 7).
 *
 * kx_sample_logits: one launch, one workgroup per row of fp32 logits [B, V] (leading dimension ld >= V; any V >= 1, rows
 * need no alignment).  Per row b, in the order of the `transformers` logits processors:
 *   1. repetition penalty r (1 = off): every id in history[b, 0:hist_len], once per distinct id: l > 0 ? l / r : l * r;
 *   2. temperature T: x = l / T.  T == 0 or do_sample == 0: GREEDY — arg max of the penalised logits, lowest index among
 *      exact ties, no filter, no random numbers;
 *   3. top-k (k <= 0 or k >= V = off): keep x_i >= the k-th largest value (ties at the threshold are all kept);
 *   4. top-p (p >= 1 = off): with the softmax renormalised over what top-k kept, keep token i iff the probability mass of
 *      tokens with STRICTLY greater x is < p.  A value threshold: always keeps the arg max, independent of any sort order;
 *   5. draw: arg max over the kept set of x_i - log(-log(u_i)) (Gumbel-max), lowest index on exact ties,
 *      u_i = (2 (w >> 9) + 1) 2^-24 with w = word (i & 3) of Philox4x32-10(counter = (position, sequence id, i >> 2, 0),
 *      key = seed): position = args.position (the absolute position of the token being generated), sequence id =
 *      sequence_ids[b] (its low 32 bits; NULL = the row index b).  A sequence's draws depend on (seed, its id, the position,
 *      its logits) only — not on the batch row it occupies, the batch size, or the launch geometry;
 *   6. -inf and NaN logits are never selected; a row with no candidate emits pad_id and is marked finished;
 *   7. finished [B] uint8 (in/out, may be NULL): a finished row emits pad_id; a row that draws eos_id (< 0 = none) emits it
 *      and becomes finished;
 *   8. outputs: next_token [B] int64 (required: what kx_embed_step reads in the next step); optional out_tokens[b * out_ld +
 *      out_col], history[b * hist_ld + hist_len] (append: hist_ld > hist_len), kept_count [B] int32 and keep_mask [B, V]
 *      uint8 (the kept set; under greedy: the candidates).
 * Bit-for-bit reproducible: thresholds come from integer histograms (counts; exp(x - max) in 2^-40 fixed point), maxima from
 * (value, index) pairs — no floating-point sum whose order the hardware chooses.  x, the penalty and 1/T are IEEE fp32.
 * x saturates as fp32 does: where l / T overflows, negative logits become -inf and drop out of the candidate set, positive ones
 * become +inf and tie at the maximum (exp(inf - inf) counts as 1); the draw is then among those ties.
 * Limits (KX_ERR_UNSUPPORTED): V <= 2^23; with a repetition penalty V <= 327680 (the history bitmap is kept in LDS).
 * Argument errors name the argument and are reported before any launch.  Never allocates, never synchronises. */
typedef struct {
  uint32_t struct_bytes;                      /* = sizeof(kx_sample_args) of the caller ("stale binding" otherwise) */
  int32_t do_sample;                          /* 0 = greedy */
  const float* logits; int64_t ld; int64_t B; int64_t V;
  float temperature; int32_t top_k; float top_p; float repetition_penalty;
  uint64_t seed; int64_t position;
  const int64_t* sequence_ids;                /* [B] or NULL */
  int64_t* history; int64_t hist_ld; int64_t hist_len;
  uint8_t* finished;
  int64_t eos_id; int64_t pad_id;
  int64_t* next_token;
  int64_t* out_tokens; int64_t out_ld; int64_t out_col;
  int32_t* kept_count; uint8_t* keep_mask;
} kx_sample_args;
int kx_sample_logits(const kx_sample_args* args, void* stream);

/* Embedding of one generated token per sequence: out[b] = embed[tokens[b]] + pos[2 + pos_a] (+ pos[2 + pos_b] when
 * pos_b >= 0), tokens [B] int64 ON THE DEVICE (kx_sample_logits' next_token), out [B, d] fp32.  The row kx_embed_splice
 * writes for a text token, additions in the same order: KosmosLanguage / u1_alias = 0: pos_a = the token's position,
 * pos_b = -1; the multimodal prompt with u1_alias = 1: pos_a = its text index, pos_b = its spliced index (text index +
 * n_img).  Ids are clamped to [0, vocab) for memory safety; either position beyond the table returns KX_ERR_INVALID_ARG
 * ("position ... out of range"), as kx_embed_splice does. */
int kx_embed_step(const int64_t* tokens, const float* embed, const float* pos, float* out, int64_t B, int64_t d,
                  int64_t vocab, int64_t max_pos, int64_t pos_a, int64_t pos_b, void* stream);

/* ------------------------------------------------------------------------------------------
 * Stage-level entry points (what kosmosx.model calls).  Weight structs hold device pointers
 * to tensors packed by the Python side from the reference's state_dict key namespace
 * (SURVEY.md §8b); `w*` GEMM operands are in the dtype of `prec`, everything else fp32.
 *
 * Binding safety (ABI 5).  The structs below grow at the end from one ABI version to the next, and the per-layer structs
 * are walked as ARRAYS: a binding written against an older header would make the library index `layer[i]` with the wrong
 * stride and read pointers out of the neighbouring element (round 2's INTEGRATION.md example did exactly that).  Every
 * weights struct therefore starts with the two sizes the CALLER's declaration has — struct_bytes = sizeof(kx_*_weights),
 * layer_bytes = sizeof(kx_*_layer) — and every stage entry point returns KX_ERR_INVALID_ARG ("stale binding") before
 * touching anything else when they differ from the library's own.  kx_struct_bytes() reports the library's sizes so a
 * binding can assert its mirrors at import time.
 * ---------------------------------------------------------------------------------------- */
typedef enum {
  KX_STRUCT_GEMM_ARGS = 0, KX_STRUCT_ATTN_ARGS = 1, KX_STRUCT_VIT_LAYER = 2, KX_STRUCT_VIT_WEIGHTS = 3,
  KX_STRUCT_PERCEIVER_LAYER = 4, KX_STRUCT_PERCEIVER_WEIGHTS = 5, KX_STRUCT_DECODER_LAYER = 6,
  KX_STRUCT_DECODER_WEIGHTS = 7, KX_STRUCT_RESAMPLE_PLAN = 8, KX_STRUCT_PROF_RECORD = 9, KX_STRUCT_SAMPLE_ARGS = 10,
  KX_STRUCT_BEAM_ARGS = 11, KX_STRUCT_CONSTRAIN_ARGS = 12, KX_STRUCT_COUNT = 13
} kx_struct_id;
/* sizeof() of the struct as this library was compiled; 0 for an unknown id.  Pure host arithmetic. */
size_t kx_struct_bytes(int32_t id);
typedef struct {
  const float *ln1_g, *ln1_b;                 /* layer_norm1 */
  const void* wqkv; const float* bqkv;        /* cat(q_proj,k_proj,v_proj) [3d,d] */
  const void* wo;   const float* bo;          /* out_proj */
  const float *ln2_g, *ln2_b;                 /* layer_norm2 */
  const void* w1;   const float* b1;          /* mlp.fc1 */
  const void* w2;   const float* b2;          /* mlp.fc2 */
  /* Optional (all NULL = off): layer_norm1 / layer_norm2 FOLDED into the GEMMs that consume them, packed like the
   * decoder's sub-LNs below — w := gamma ⊙ W, b := W·beta + b, colsum[n] := Σ_k w[n,k].  With them (and 64 | dim,
   * a batch large enough for the tile kernels) the residual GEMMs emit the operand rows + statistics themselves
   * (kx_gemm_args.ln_operand_out) and no LayerNorm kernel runs between the layers. */
  const void* wqkv_f; const float* bqkv_f; const float* wqkv_colsum;
  const void* w1_f;   const float* b1_f;   const float* w1_colsum;
} kx_vit_layer;

typedef struct {
  uint32_t struct_bytes, layer_bytes;         /* = sizeof(kx_vit_weights), sizeof(kx_vit_layer) AS THE CALLER DECLARES THEM (below) */
  int32_t image, patch, dim, heads, ffn, layers, act; float eps;
  int32_t kpad;                               /* padded im2col K (multiple of 64) */
  const void* wpatch;                         /* [dim, kpad]  (conv weight flattened c,ky,kx, zero padded) */
  const float* cls;                           /* embeddings.class_embedding [dim] */
  const float* pos;                           /* embeddings.position_embedding.weight [tokens, dim] */
  const float *pre_g, *pre_b;                 /* pre_layrnorm */
  const kx_vit_layer* layer;                  /* host array [layers] */
} kx_vit_weights;

/* CLIP ViT-L/14 vision tower: clip_model(pixel_values=images)["last_hidden_state"]
 * (/root/reference/kosmosx/model.py:230; HF CLIPVisionTransformer.forward).
 * pixels [B,3,image,image] fp32 -> out [B, tokens, dim] fp32. */
size_t kx_vit_workspace_bytes(const kx_vit_weights* w, int64_t B, int32_t prec);
int kx_vit_forward(const kx_vit_weights* w, const float* pixels, int64_t B, float* out,
                   void* workspace, size_t workspace_bytes, int32_t prec, void* stream);

typedef struct {
  const float *nm_g, *nm_b, *nl_g, *nl_b;     /* norm_media, norm_latents */
  const void *wq, *wkv, *wout;                /* to_q [inner,dim], to_kv [2*inner,dim], to_out [dim,inner] */
  const float *ff_g, *ff_b;                   /* layers.i.1.0 (LayerNorm) */
  const void *w1, *w2;                        /* layers.i.1.1 [dim*mult,dim], layers.i.1.3 [dim,dim*mult] */
} kx_perceiver_layer;

typedef struct {
  uint32_t struct_bytes, layer_bytes;         /* = sizeof(kx_perceiver_weights), sizeof(kx_perceiver_layer) of the caller */
  int32_t dim, depth, heads, latents, ff_mult, out_dim; float eps;
  const float* latents_p;                     /* perceive.latents [latents, dim] */
  const float* media_pos;                     /* perceive.media_pos_emb[0,0,:] [dim] */
  const kx_perceiver_layer* layer;            /* host array [depth] */
  const float *norm_g, *norm_b;               /* perceive.norm */
  const void* wproj;                          /* image_proj.weight [out_dim, dim] */
} kx_perceiver_weights;

/* PerceiverResampler + image_proj: self.image_proj(self.perceive(images).squeeze(1))
 * (/root/reference/kosmosx/model.py:231-232).  x [B, m, dim] fp32 -> out [B, latents, out_dim] fp32.
 * lat_out (optional, may be NULL): the resampler output before image_proj [B, latents, dim] fp32.
 * out may be NULL (and wproj NULL) when only lat_out is wanted (standalone PerceiverResampler call). */
size_t kx_perceiver_workspace_bytes(const kx_perceiver_weights* w, int64_t B, int64_t m, int32_t prec);
int kx_perceiver_forward(const kx_perceiver_weights* w, const float* x, int64_t B, int64_t m,
                         float* out, float* lat_out, void* workspace, size_t workspace_bytes,
                         int32_t prec, void* stream);

/* With subln != 0 the two sub-LayerNorms are FOLDED into the GEMMs that consume them (no LayerNorm pass, no fp32
 * intermediate): the caller packs, with γ/β = the sub-LN's weight/bias and W/b = the following Linear,
 *     w  := γ ⊙ W (column k scaled by γ_k, then cast to the operand dtype),
 *     b  := W·β + b  (fp32),        w*_colsum[n] := Σ_k w[n,k]  (fp32 sum of the cast values)
 * for (inner_attn_ln, out_proj) -> wo/bo/wo_colsum and (ffn_layernorm, fc2) -> w2/b2/w2_colsum.
 * With subln == 0 wo/bo/w2/b2 are the plain weights and the colsum pointers are unused. */
typedef struct {
  const float *sa_g, *sa_b;                   /* self_attn_layer_norm.A */
  const void* wqkv; const float* bqkv;        /* cat(q,k,v)_proj.A [3d,d] */
  const void* wo;   const float* bo;          /* self_attn.out_proj.A (sub-LN folded, see above) */
  const float* wo_colsum;
  const float *fl_g, *fl_b;                   /* final_layer_norm.A */
  const void* w1;   const float* b1;          /* ffn.A.fc1 */
  const void* w2;   const float* b2;          /* ffn.A.fc2 (sub-LN folded) */
  const float* w2_colsum;
  /* Optional (all NULL = off): self_attn_layer_norm folded into qkv, final_layer_norm into fc1 (same packing rule) */
  const void* wqkv_f; const float* bqkv_f; const float* wqkv_colsum;
  const void* w1_f;   const float* b1_f;   const float* w1_colsum;
  /* Optional (NULL = off), decode step only (bf16 and fp32 operands): wqkv / wo / w1 / w2 once more in the STREAMING layout of
   * kx_gemm_args.w_tiled — the weight-streaming kernels then read one contiguous 1 KB block per wave instruction instead of
   * 16 row segments of 64 B (4.2-5.0 vs 3.2-3.7 TB/s, profiles/r02_gemv_stream_probe.log). */
  const void *wqkv_t, *wo_t, *w1_t, *w2_t;
} kx_decoder_layer;

typedef struct {
  uint32_t struct_bytes, layer_bytes;         /* = sizeof(kx_decoder_weights), sizeof(kx_decoder_layer) of the caller */
  int32_t layers, dim, heads, ffn, vocab, act, subln, xpos; float eps;
  const kx_decoder_layer* layer;              /* host array [layers] */
  const float *ln_g, *ln_b;                   /* decoder.layer_norm */
  const void* wout;                           /* output_projection.weight [vocab, dim] */
  /* Optional: decoder.layer_norm folded into the output projection (bout_f = Wout·beta, [vocab]) */
  const void* wout_f; const float* bout_f; const float* wout_colsum;
  const void* wout_t;                         /* optional: wout in the streaming layout (vocab padded to a multiple of 16 rows) */
} kx_decoder_weights;

/* Decoder.forward(x, passed_x=x)[0] (/root/reference/kosmosx/model.py:250, :320; torchscale
 * Decoder.forward with the README.md:179-193 patch): `layers` × DecoderLayer, final LayerNorm,
 * output_projection.   x [B,T,dim] fp32 (overwritten: it is the residual stream),
 * XPos tables [T,32] fp32 for this T (xq_*: q, xk_*: k/downscale; may be NULL when xpos == 0),
 * logits [B,T,vocab] dtype ldt. */
size_t kx_decoder_workspace_bytes(const kx_decoder_weights* w, int64_t B, int64_t T, int32_t prec);
int kx_decoder_forward(const kx_decoder_weights* w, float* x, int64_t B, int64_t T,
                       const float* xq_cs, const float* xq_ss, const float* xk_cs, const float* xk_ss,
                       void* logits, int32_t ldt, void* workspace, size_t workspace_bytes,
                       int32_t prec, void* stream);

/* ------------------------------------------------------------------------------------------
 * Incremental decoding (torchscale Decoder.forward(..., incremental_state=...),
 * MultiheadAttention's prev_key / prev_value path).  Not exercised by the reference's own call
 * (/root/reference/kosmosx/model.py:250 passes no incremental_state); built as the next row after the forward.
 *
 * Caches: kcache / vcache, layers x B x Tmax x dim values in the operand dtype of `prec`, opaque to the caller (written
 * by the prefill and the steps, read by the steps; per layer and sequence [heads][Tmax][64]: a head's keys are contiguous).
 * Keys are stored AFTER the XPos
 * rotation/scale (torchscale stores them before and re-rotates the whole cache every step; the score only depends
 * on i − m and the centring constant cancels), so the tables passed to the prefill and to every
 * decode step must share ONE centring: build [Tmax, 32] tables once with min_pos of the prefill length.
 *
 * kx_decoder_prefill  = kx_decoder_forward that also fills rows [0, T) of the caches.
 * kx_decoder_decode_step: x [B, 1, dim] fp32 = embedding of the ONE new token at position t (consumed);
 *   xq_*, xk_* point at ROW t of the tables ([32] floats each); appends row t to the caches, attends over rows
 *   [0, t], returns logits [B, 1, vocab].  Workspace: kx_decoder_workspace_bytes(w, B, 1, prec).
 * kx_attention_decode: the single-query attention + cache append used by the step (qkv [B, 3*dim] rows of the new
 *   token; stats_out [B, H, 2] optional, as kx_attn_args.stats_out). */
int kx_decoder_prefill(const kx_decoder_weights* w, float* x, int64_t B, int64_t T,
                       const float* xq_cs, const float* xq_ss, const float* xk_cs, const float* xk_ss,
                       void* logits, int32_t ldt, void* kcache, void* vcache, int64_t Tmax,
                       void* workspace, size_t workspace_bytes, int32_t prec, void* stream);
int kx_decoder_decode_step(const kx_decoder_weights* w, float* x, int64_t B, int64_t t,
                           const float* xq_cs, const float* xq_ss, const float* xk_cs, const float* xk_ss,
                           void* kcache, void* vcache, int64_t Tmax, void* logits, int32_t ldt,
                           void* workspace, size_t workspace_bytes, int32_t prec, void* stream);
int kx_attention_decode(const void* qkv, void* kcache, void* vcache, void* out, int32_t odt, float* stats_out,
                        int64_t B, int64_t H, int64_t t, int64_t Tmax, int32_t prec, void* stream);

/* ------------------------------------------------------------------------------------------
 * Ragged batches: every sequence at its own position, held ON THE DEVICE (added within ABI 7: functions only, no struct and
 * no existing signature changes, so kx_version() stays 7).
 *
 * positions [B] int32 (device): positions[b] = the number of tokens sequence b has in the cache = the absolute position of
 * the token its next step appends.  A step's launch arguments are then the same for every token: what changes from one
 * token to the next is device memory only (kx_sample_logits_ragged advances the array).
 *
 * Positions cannot be validated by the host per step, so the kernels check them: a row whose position is outside the cache
 * or the tables reads and writes nothing for that row and ORs a bit into the sticky *error_word (int32, device, zeroed by
 * the caller once; read it whenever the host synchronises anyway — kosmosx.generation: at the stop poll and after the loop).
 *
 * kx_attention_decode_ragged: kx_attention_decode with t = positions[b] per sequence; appends the new k / v to cache row
 *   positions[b].  Same slots, key order and arithmetic: where all positions equal t, the bits of kx_attention_decode at t.
 * kx_step_prepare: the start of a ragged step, one launch.  Per sequence b with t = positions[b]:
 *   x[b] = embed[tokens[b]] + pos[2 + t]                           (pos_shift == 0; kx_embed_step(pos_a = t, pos_b = -1))
 *   x[b] = embed[tokens[b]] + pos[2 + t - pos_shift] + pos[2 + t]  (pos_shift  > 0; kx_embed_step(t - pos_shift, t))
 *   with kx_embed_step's order of additions, and xpos_rows[k][b][0:32] = row t of table k (k = 0..3: xq_cs, xq_ss, xk_cs,
 *   xk_ss, each [xpos_len, 32] fp32) — the [B, 32] tables a qkv GEMM over the M = B rows of the step reads with xpos_T = B.
 *   The four tables and xpos_rows [4, B, 32] may all be NULL (no XPos).  KX_RAGGED_ERR_TABLE: t < pos_shift, t + 2 >= max_pos
 *   or t >= xpos_len; that row of x and of xpos_rows is not written, so the caller initialises both buffers once (zeros):
 *   what a rejected row then computes until the error word is read is finite and deterministic.
 * kx_sample_logits_ragged: kx_sample_logits with the Philox position of row b = positions[b] + advance (args->position is
 *   ignored).  advance != 0: one lane of the row's workgroup stores that value back after the draw, finished rows included —
 *   so the first call after a prefill runs with advance = 0 and every later one with advance = 1, and no other launch or
 *   host scalar moves the positions.  Everything else as kx_sample_logits.
 * kx_decoder_decode_step_ragged: kx_step_prepare + kx_decoder_decode_step with per-sequence positions.  tokens [B] int64
 *   (device), embed [vocab, dim], pos [max_pos, dim]; x [B, 1, dim] fp32 scratch (the step's residual stream); xq_*, xk_*
 *   the FULL [Tmax, 32] tables (one centring, as for the prefill); xpos_rows [4, B, 32] fp32 scratch.  x and xpos_rows
 *   are zeroed by the caller before the first step (see kx_step_prepare).  Both step paths
 *   (weight streaming up to 16 sequences, tile GEMMs above) run their qkv launch with xpos_T = B on xpos_rows. */
typedef enum { KX_RAGGED_ERR_TABLE = 1, KX_RAGGED_ERR_CACHE = 2, KX_RAGGED_ERR_GATHER = 4 /* kx_kv_cache_gather */,
               KX_RAGGED_ERR_COMMIT = 8 /* kx_kv_cache_commit */ } kx_ragged_error;
int kx_attention_decode_ragged(const void* qkv, void* kcache, void* vcache, void* out, int32_t odt, float* stats_out,
                               int64_t B, int64_t H, const int32_t* positions, int64_t Tmax, int32_t prec,
                               int32_t* error_word, void* stream);
int kx_step_prepare(const int64_t* tokens, const float* embed, const float* pos, const int32_t* positions,
                    const float* xq_cs, const float* xq_ss, const float* xk_cs, const float* xk_ss, float* x,
                    float* xpos_rows, int64_t B, int64_t d, int64_t vocab, int64_t max_pos, int64_t pos_shift,
                    int64_t xpos_len, int32_t* error_word, void* stream);
int kx_sample_logits_ragged(const kx_sample_args* args, int32_t* positions, int64_t advance, void* stream);
int kx_decoder_decode_step_ragged(const kx_decoder_weights* w, const int64_t* tokens, const float* embed, const float* pos,
                                  int64_t vocab, int64_t max_pos, int64_t pos_shift, float* x, int64_t B,
                                  const int32_t* positions, const float* xq_cs, const float* xq_ss, const float* xk_cs,
                                  const float* xk_ss, float* xpos_rows, void* kcache, void* vcache, int64_t Tmax,
                                  void* logits, int32_t ldt, void* workspace, size_t workspace_bytes, int32_t prec,
                                  int32_t* error_word, void* stream);

/* ------------------------------------------------------------------------------------------
 * Beam search on the device (added within ABI 7: one struct, three functions, one kx_struct_id value and one kx_ragged_error bit
 * are appended; no existing layout moves, so kx_version() stays 7).
 *
 * State per batch row b: W live beams, each with an fp32 cumulative score s_j; a pool of at most W finished hypotheses
 * (score, end step, parent beam); a `done` byte.
 *
 * kx_beam_step — step g (0-based, args->step) ranks Win input beams per batch row: Win = 1 at g = 0 (the prefill ran once per batch
 * row, not W times), Win = W afterwards.  For input beam j with logits row x = logits[(b * Win + j) * ld + 0:V]:
 *   - on load: NaN and -inf are never candidates, +inf is clamped to FLT_MAX, -0 is read as +0;
 *   - m = max x; Z = sum exp(x - m) accumulated as 64-bit integers in 2^-40 fixed point (the sampler's mass: integer adds
 *     commute, so Z does not depend on execution order); lse = m + logf((float)Z * 2^-40);
 *   - candidate (j, v) has c = fl(s_j + fl(x_v - lse)), single fp32 operations; a candidate needs c > -inf (a beam whose score
 *     is -inf offers none);
 *   - candidates are ranked by c descending, exact ties to the lower flat index j * V + v; the best 2W are walked in rank order.
 * Walking: a candidate with v == eos_id at rank < W (0-based) enters the pool with score c / (g + 1)^alpha (fp32; alpha =
 * length_penalty), end step g and parent beam j — a full pool replaces its worst entry (lowest score, the later slot among equal
 * ones) only if the new score is strictly better; at rank >= W it is skipped.  Any other candidate becomes the next live beam
 * until W are filled (at most one EOS candidate exists per input beam, so 2W candidates always hold W others when enough finite
 * candidates exist).  An unfilled slot i gets score -inf, token pad_id and parent i (0 when i >= Win).
 * Outputs per row b * W + i: next_token int64 (what kx_embed_step reads), parent int32 = j (with next_token: the backpointers of
 * step g), src_row int32 = b * Win + j (what kx_kv_cache_gather reads), scores_out = s_i.
 * Done: after the walk row b becomes done when its pool holds W hypotheses and (early_stopping, or worst pool score >= best live
 * c / (g + 1)^alpha; no live beam counts as -inf).  A done row is frozen from the next step on: its pool never changes, its live
 * beams keep their scores, their tokens are pad_id and their parents the identity.
 *
 * Two launches, no workgroup waits on another: one 1024-thread workgroup per input beam row computes m, Z, lse and writes the
 * row's own best 2W (key(c), v) pairs to `scratch` (B * Win * 2W uint64; the best 2W of a batch row lie inside the union of these
 * sets) by 2W exact arg-max passes over (key, ~index) pairs — 2 + 2W reads of the row, consecutive lanes on consecutive logits,
 * 16-byte loads where the row is 16-byte aligned; one workgroup per batch row then ranks the <= W * 2W <= 512 pairs by counting,
 * walks them and writes the outputs.  scores_in [B * Win] and scores_out [B * W] may be the same buffer only when Win == W.
 * Limits: 1 <= W <= 16, Win in {1, W}, V >= 2W, V <= 2^23.  Never allocates, never synchronises.
 *
 * kx_beam_finalize — after the last of n steps: every row that is not done offers its live beams (score > -inf) to the pool at
 * s_i / n^alpha (end step n, parent i) under the same replacement rule; then the R best pool entries per row (score descending,
 * the earlier slot among equal ones) are backtracked through parent / token ([n, trace_ld] arrays, row g = step g's outputs,
 * trace_ld >= B * W) into out_tokens [B, R, out_ld] (out_ld >= n; columns 0:n are written: the hypothesis, its EOS, then pad_id)
 * and out_scores [B, R].  A slot with no hypothesis is all pad_id with score -inf.  One thread per hypothesis.
 *
 * kx_kv_cache_gather — dst[l, r, h, 0:t, :] = src[l, src_row[r], h, 0:t, :] for both caches ([L, B, heads, Tmax, 64], elem_bytes
 * = 4 for the fp32 / f16c cache, 2 for the bf16 cache; 16-byte aligned), src_row [B_dst] int32 ON THE DEVICE.  Rows at and after t
 * of dst are not written.  Under tuning key 9 = 1 the caches are [L, B, Tmax, heads, 64] and the copy is dst[l, r, 0:t, :, :] =
 * src[l, src_row[r], 0:t, :, :]: the first t rows of heads * 64 elements per (layer, sequence); the key is read at the call, like
 * the prefill and the steps read it.  src and dst must not overlap (KX_ERR_INVALID_ARG, nothing launched).  A src_row entry outside
 * [0, B_src) makes that row copy nothing and ORs KX_RAGGED_ERR_GATHER into the sticky *error_word (see "Ragged batches"). */
typedef struct {
  uint32_t struct_bytes;                      /* = sizeof(kx_beam_args) of the caller ("stale binding" otherwise) */
  int32_t early_stopping;
  const float* logits; int64_t ld; int64_t B; int64_t Win; int64_t W; int64_t V;
  int64_t step; float length_penalty;
  int64_t eos_id; int64_t pad_id;             /* eos_id < 0 = none */
  const float* scores_in;                     /* [B * Win] */
  float* scores_out;                          /* [B * W] */
  int64_t* next_token;                        /* [B * W] */
  int32_t* parent;                            /* [B * W] */
  int32_t* src_row;                           /* [B * W] */
  float* pool_score; int32_t* pool_end; int32_t* pool_parent;   /* [B * W] each */
  int32_t* pool_count;                        /* [B], zeroed by the caller before step 0 */
  uint8_t* done;                              /* [B], zeroed by the caller before step 0 */
  uint64_t* scratch;                          /* [B * Win * 2W] */
} kx_beam_args;
int kx_beam_step(const kx_beam_args* args, void* stream);
int kx_beam_finalize(const float* scores_live, const uint8_t* done, float* pool_score, int32_t* pool_end, int32_t* pool_parent,
                     int32_t* pool_count, const int32_t* parent, const int64_t* token, int64_t trace_ld, int64_t B, int64_t W,
                     int64_t R, int64_t n, float length_penalty, int64_t eos_id, int64_t pad_id, int64_t* out_tokens,
                     int64_t out_ld, float* out_scores, void* stream);
int kx_kv_cache_gather(const void* src_k, const void* src_v, void* dst_k, void* dst_v, int64_t L, int64_t B_src, int64_t B_dst,
                       int64_t heads, int64_t Tmax, int64_t t, int32_t elem_bytes, const int32_t* src_row, int32_t* error_word,
                       void* stream);

/* ------------------------------------------------------------------------------------------
 * Constraints on what may be emitted and when a row stops (added within ABI 7: one struct, one function and one kx_struct_id
 * value are appended; no existing layout moves, so kx_version() stays 7).
 *
 * kx_constrain_logits: one launch, one 256-thread workgroup per row, issued BEFORE kx_sample_logits or kx_beam_step on the fp32
 * rows logits [B, V] (any ld >= V) that launch is about to read.  It edits the rows in place: a banned id's logit becomes -inf and
 * nothing else is written.  The sampler never selects -inf (its rule 6) and to kx_beam_step -inf is never a candidate, so neither
 * kernel changes.  Bans commute with the repetition penalty (-inf * r == -inf == -inf / r), so constrain-then-sample is the
 * `transformers` order (processors, then warpers).  A row whose every logit is banned falls under the sampler's rule 6: it emits
 * pad_id and is finished.
 *
 * Row b's LOGICAL token sequence s (length n) is read from history [B, hist_ld] int64, the buffer kx_sample_logits appends to, of
 * which hist_len physical columns are in use: columns [0, hist_len) when prompt_lens is NULL; otherwise (the ragged batch) columns
 * [0, prompt_lens[b]) followed by [prompt_width, hist_len) — the columns in between are right padding (copies of the row's first
 * token) and take part in no match.  history may be NULL with hist_len = 0 (n = 0: the history-free constraints only, as under
 * beam search).  g = new_tokens is the number of tokens already generated, a host scalar common to all rows.  Per row, in order:
 *   1. a row with finished[b] != 0 is left untouched;
 *   2. stop: if g >= 1 and some stop sequence is a suffix of s, finished[b] = 1 and the row gets no bans (the sampler that follows
 *      emits pad_id: the output keeps the stop sequence and is padded after it, as after an EOS).  The sequence may begin inside
 *      the prompt; g >= 1 makes its last token a generated one;
 *   3. no-repeat n-gram (ngram = N >= 1; 0 = off): for every i with i + N - 1 < n and s[i : i+N-1] == s[n-N+1 : n], ban s[i+N-1];
 *      nothing when n + 1 < N; N = 1 bans every id of s (NoRepeatNGramLogitsProcessor);
 *   4. bad words: a sequence w of m ids bans w[0] when m == 1, else w[m-1] when n >= m - 1 and s[n-m+1 : n] == w[0 : m-1]
 *      (NoBadWordsLogitsProcessor);
 *   5. minimum length: g < min_new and eos_id >= 0 bans eos_id (MinNewTokensLengthLogitsProcessor);
 *   6. range: an id outside [0, V) — in the history or in a sequence — is compared as a value and never used as an index, and a
 *      prompt_lens[b] outside [0, prompt_width] is clamped into it: memory safety does not depend on the device data.
 * Bad and stop sequences are CSR tables on the device: ids int64 and offsets int32 [n + 1].  The offsets are ALSO passed as a host
 * array (*_off_host, the same n + 1 values) so that the limits are checked before the launch; the kernel skips any device entry
 * that disagrees with them (a length outside 1..64 or an offset outside [0, off_host[n]]).
 * The workgroup stages the last 64 ids of s in LDS (what a 64-id suffix, a 63-id n-gram prefix or bad-word prefix can need); threads
 * stride over the n-gram start positions and over the sequences.  Several threads may store the same -inf to one address.
 * Limits (KX_ERR_UNSUPPORTED, before any launch): ngram <= 64; every bad or stop sequence 1..64 ids long.  Argument errors name the
 * argument.  Never allocates, never synchronises. */
typedef struct {
  uint32_t struct_bytes;                      /* = sizeof(kx_constrain_args) of the caller ("stale binding" otherwise) */
  int32_t ngram;                              /* 0 = off */
  float* logits; int64_t ld; int64_t B; int64_t V;
  const int64_t* history; int64_t hist_ld; int64_t hist_len;    /* hist_ld > hist_len: the sampler appends after this launch */
  int64_t prompt_width; const int32_t* prompt_lens;             /* [B] device or NULL */
  int64_t new_tokens;
  const int64_t* bad_ids; const int32_t* bad_off; const int32_t* bad_off_host; int64_t n_bad;
  const int64_t* stop_ids; const int32_t* stop_off; const int32_t* stop_off_host; int64_t n_stop;
  int64_t min_new; int64_t eos_id;            /* eos_id < 0 = none */
  uint8_t* finished;                          /* [B] in/out, may be NULL */
} kx_constrain_args;
int kx_constrain_logits(const kx_constrain_args* args, void* stream);

/* ------------------------------------------------------------------------------------------
 * Speculative decoding by prompt lookup (added within ABI 7: one struct and three functions are appended; no existing layout moves
 * and the kx_struct_id list is unchanged — kx_spec_args carries its own struct_bytes, which kx_spec_accept checks — so kx_version()
 * stays 7).
 *
 * A verify step feeds K = D + 1 rows per sequence in one pass over the weights: row 0 is the last confirmed token, rows 1..D are
 * guesses ("drafts") for the tokens after it, at consecutive positions base .. base + D.  Row j's greedy pick is the model's
 * token after rows 0..j, so draft j + 1 is right exactly when it equals row j's pick; the picks up to and including the first
 * wrong draft's row are what plain greedy decoding would emit, one token per pass.  Exact for greedy decoding.
 *
 * kx_attention_decode_block: kx_attention_decode_ragged over M = B * K rows of which row r = b * K + j belongs to cache sequence b
 *   (caches [B, ...], not [M, ...]).  positions [B * K] int32 (device): row r sits at t = positions[r] and its sequence's base is
 *   t0 = positions[b * K]; the row must have t == t0 + j.  It attends over cache keys 0 .. t0 - 1 of sequence b and over keys
 *   t0 + i, i = 0..j, read from qkv row b * K + i, and appends its own k / v to cache row t of sequence b.  Same slots, key order
 *   and arithmetic as kx_attention_decode_ragged: ONE launch gives, bit for bit, the outputs, stats_out and cache rows of K
 *   successive kx_attention_decode_ragged launches on the sequence (launch j: the rows j of every sequence at positions t0 + j),
 *   in every output form and under both cache layouts.  A row with t outside [0, Tmax), t0 < 0 or t != t0 + j writes nothing
 *   (no output, no cache row) and ORs KX_RAGGED_ERR_CACHE into *error_word; the other rows are unaffected.  K in 2..16.
 * kx_decoder_decode_step_block: kx_decoder_decode_step_ragged with M = B * K rows and B cache sequences: kx_step_prepare on the
 *   B * K tokens and positions (pos_shift as there), the qkv launch with xpos_T = B * K, kx_attention_decode_block in place of the
 *   ragged attention, everything else row-wise.  x [B * K, 1, dim] and xpos_rows [4, B * K, 32] scratch zeroed once by the caller;
 *   caches [L, B, heads, Tmax, 64]; logits [B * K, vocab]; workspace = kx_decoder_workspace_bytes(w, B * K, 1, prec).
 *
 * kx_spec_accept — one launch per verify step, after kx_sample_logits (greedy, no history, no finished) has left picked [B * Kin]
 * for the step's logits block; one 256-thread workgroup per sequence, integer work only (exact, order-free).  Kin = 1 at step 0
 * (the block is the prefill's last row) and K afterwards.  Per sequence b, with fed = fed[b * Kin ..], picked = picked[b * Kin ..]:
 *   Accept.  a = the largest value with fed[j] == picked[j - 1] for all 1 <= j <= a (a <= Kin - 1; a = 0 when Kin = 1, fed unused).
 *     The candidates are picked[0..a].
 *   Emit.  A row with finished[b] != 0 on entry emits nothing and moves nothing (emitted[b, step] = 0).  Otherwise
 *     e = min(a + 1, max_new - n_out[b]) candidates, cut after the first eos_id (inclusive; eos_id < 0 = none), are appended to
 *     out_tokens[b, n_out[b] ..] and history[b, hist_len[b] ..]; out_src[b, n_out[b] + j] = step * K + j (the logits row token j was
 *     picked from, counted in [step][row of the sequence]) and emitted[b, step] = e when those are given.  n_out[b], hist_len[b]
 *     and the K positions of the sequence advance by e; at Kin = 1 the positions are initialised instead: positions[b * K + j] =
 *     prefill_len - 1 + e + j (the first emitted token is fed at position prefill_len).  The row becomes finished when it emitted
 *     eos_id or n_out[b] reached max_new.  out_tokens is filled with pad_id by the caller, so slots after a cut stay pad_id.
 *   Draft the next block into next_tokens[b * K ..].  A finished row gets pad_id in all K rows (it keeps stepping at its frozen
 *     positions, rewriting its own spare cache rows).  Otherwise row 0 = the last emitted token `last`, and rows 1..K-1:
 *     - draft_from [B, draft_ld] given: row m = draft_from[b, n_out[b] + m - 1] (the draft for output slot n_out[b] + m - 1, n_out
 *       after the append), `last` where that slot is outside [0, draft_ld);
 *     - else the lookup in s = history[b, 0:len], len = hist_len[b] after the append: for n = min(ngram_max, len - 1) down to 1 take
 *       the LARGEST i <= len - n - 1 with s[i : i + n] == s[len - n : len] (the suffix never matches itself); the first n that has
 *       one wins, and row m = s[i + n + ((m - 1) mod p)], p = len - (i + n): the continuation of the match, wrapping at the
 *       sequence's end.  No n matches: every draft = `last`.  Any draft is correct — a wrong one is only rejected.
 *   Guards.  Ids are compared and copied as values and never used as an index.  n_out[b] outside [0, max_new], hist_len[b] outside
 *     [0, hist_ld - (max_new - n_out[b])] (no room for what may still be appended) or, at Kin = K, positions[b * K] < 0 make the row
 *     finished with nothing emitted: memory safety does not depend on the device data.
 * Host checks (KX_ERR_INVALID_ARG, nothing launched): null pointers, struct_bytes, K outside 2..16, Kin not in {1, K}, B < 1,
 * ngram_max outside 1..64, out_ld < max_new, max_new < 1, fed missing with Kin = K.  Never allocates, never synchronises. */
typedef struct {
  uint32_t struct_bytes;                      /* = sizeof(kx_spec_args) of the caller ("stale binding" otherwise) */
  int32_t ngram_max;                          /* 1..64: the longest suffix n-gram looked up */
  int64_t B; int64_t K; int64_t Kin;
  const int64_t* fed;                         /* [B * Kin]: the tokens the block's rows were fed (NULL when Kin = 1) */
  const int64_t* picked;                      /* [B * Kin]: kx_sample_logits' greedy picks */
  int32_t* positions;                         /* [B * K] in/out */
  int64_t prefill_len;                        /* read when Kin = 1 */
  int64_t* history; int64_t hist_ld; int32_t* hist_len;          /* [B, hist_ld], [B] in/out */
  int64_t* out_tokens; int64_t out_ld; int32_t* n_out;           /* [B, out_ld], [B] in/out (zeroed before step 0) */
  uint8_t* finished;                          /* [B] in/out (zeroed before step 0) */
  int64_t max_new; int64_t eos_id; int64_t pad_id;               /* eos_id < 0 = none */
  int64_t step;                               /* the verify step's index, 0 = the prefill's */
  int32_t* out_src;                           /* [B, out_ld] or NULL */
  int32_t* emitted; int64_t emitted_ld;       /* [B, emitted_ld] (step < emitted_ld) or NULL */
  const int64_t* draft_from; int64_t draft_ld;                   /* [B, draft_ld] or NULL */
  int64_t* next_tokens;                       /* [B * K] out: the next block's tokens */
} kx_spec_args;
int kx_spec_accept(const kx_spec_args* args, void* stream);
int kx_attention_decode_block(const void* qkv, void* kcache, void* vcache, void* out, int32_t odt, float* stats_out,
                              int64_t B, int64_t K, int64_t H, const int32_t* positions, int64_t Tmax, int32_t prec,
                              int32_t* error_word, void* stream);
int kx_decoder_decode_step_block(const kx_decoder_weights* w, const int64_t* tokens, const float* embed, const float* pos,
                                 int64_t vocab, int64_t max_pos, int64_t pos_shift, float* x, int64_t B, int64_t K,
                                 const int32_t* positions, const float* xq_cs, const float* xq_ss, const float* xk_cs,
                                 const float* xk_ss, float* xpos_rows, void* kcache, void* vcache, int64_t Tmax,
                                 void* logits, int32_t ldt, void* workspace, size_t workspace_bytes, int32_t prec,
                                 int32_t* error_word, void* stream);

/* ------------------------------------------------------------------------------------------
 * Scoring candidates over a shared prompt cache (added within ABI 7: three functions are appended; no struct, no existing layout
 * moves and the kx_struct_id list is unchanged, so kx_version() stays 7).
 *
 * C candidate continuations of K fed rows each are scored in one pass over the weights against the KV cache a prefill of Bc
 * prompts left: several candidates read the same cache sequence and nobody appends to it.
 *
 * kx_attention_decode_shared: kx_attention_decode_block's rows and addressing — M = C * K rows, row r = c * K + j the j-th row of
 *   candidate c, positions [C * K] int32 (device) with t = positions[r], t0 = positions[c * K] and t == t0 + j required — with
 *   candidate c reading cache sequence cache_seq[c] (cache_seq [C] int32, device; caches [Bc, ...]; any mapping: repeated,
 *   unordered, unused sequences).  Row r attends over cache keys 0 .. t0 - 1 of that sequence and over keys t0 + i, i = 0..j, read
 *   from qkv row c * K + i.  It APPENDS NOTHING: the caches are const and bitwise unchanged by the launch, rows >= t0 of a cache
 *   sequence are never read.  Same slots, key order and arithmetic: one launch gives, bit for bit, the outputs and stats_out of
 *   kx_attention_decode_block run on a cache replicated per candidate (sequence c of the replica = sequence cache_seq[c]), and for
 *   K = 1 those of kx_attention_decode_ragged on that replica; every output form (KX_F32, KX_BF16, KX_F16C, KX_F16P), both cache
 *   layouts (tuning key 9).  cache_seq[c] is requested together with the two position words: one scalar round trip before the
 *   one vector round trip, as in the block form.  A row with cache_seq[c] outside [0, Bc), t outside [0, Tmax), t0 < 0 or
 *   t != t0 + j writes nothing and ORs KX_RAGGED_ERR_CACHE into *error_word; the other rows are unaffected.  K in 1..16,
 *   C * K <= 65535.
 * kx_decoder_score_step: kx_decoder_decode_step_block with C candidates of K rows, Bc cache sequences and cache_seq: kx_step_prepare
 *   on the C * K tokens and positions (pos_shift as there), the qkv launch with xpos_T = C * K, kx_attention_decode_shared in place
 *   of the block attention — the caches [L, Bc, heads, Tmax, 64] are const and stay untouched — everything else row-wise.  Up to 16
 *   rows the step streams the weights, above that it runs the tile GEMMs.  x [C * K, 1, dim] and xpos_rows [4, C * K, 32] scratch
 *   zeroed once by the caller; logits [C * K, vocab]; workspace = kx_decoder_workspace_bytes(w, C * K, 1, prec).
 * kx_token_logprob: one launch, one 256-thread workgroup per output row r = 0 .. rows - 1:
 *     out[r] = x[target[r]] - logsumexp(x),  x = logits[row_index[r] * ld + 0 .. V)   (fp32; ld >= V elements between rows)
 *   row_index [rows] int32 (device) may repeat and reorder rows of the [rows_available, ld] logits buffer — one logits row serves
 *   many outputs without a copy; NULL means row_index[r] = r.  The arithmetic is kx_cross_entropy's (the same device code):
 *   (x[target] - max) - log(sum exp(x - max)), one pass for the max and one for the sum, no softmax materialised; deterministic.
 *   target[r] outside [0, V) or row_index[r] outside [0, rows_available): out[r] = 0.0 exactly, nothing is read through the bad
 *   index.  A -inf logit at the target gives -inf (the row's maximum being finite); a NaN anywhere in the row gives NaN.
 *   Host checks (KX_ERR_INVALID_ARG, nothing launched): null logits / target / out, rows < 1, rows_available < 1, V < 1, ld < V.
 * None of the three allocates or synchronises.
 * ------------------------------------------------------------------------------------------ */
int kx_attention_decode_shared(const void* qkv, const void* kcache, const void* vcache, void* out, int32_t odt, float* stats_out,
                               int64_t C, int64_t K, int64_t H, const int32_t* positions, const int32_t* cache_seq, int64_t Bc,
                               int64_t Tmax, int32_t prec, int32_t* error_word, void* stream);
int kx_decoder_score_step(const kx_decoder_weights* w, const int64_t* tokens, const float* embed, const float* pos,
                          int64_t vocab, int64_t max_pos, int64_t pos_shift, float* x, int64_t C, int64_t K,
                          const int32_t* positions, const int32_t* cache_seq, int64_t Bc, const float* xq_cs, const float* xq_ss,
                          const float* xk_cs, const float* xk_ss, float* xpos_rows, const void* kcache, const void* vcache,
                          int64_t Tmax, void* logits, int32_t ldt, void* workspace, size_t workspace_bytes, int32_t prec,
                          int32_t* error_word, void* stream);
int kx_token_logprob(const float* logits, int64_t rows_available, int64_t V, int64_t ld, const int32_t* row_index,
                     const int64_t* target, float* out, int64_t rows, void* stream);

/* ------------------------------------------------------------------------------------------
 * Per-token log-probs of a generation step (added within ABI 7: one function is appended; no struct, no existing layout moves and
 * the kx_struct_id list is unchanged, so kx_version() stays 7).
 *
 * kx_step_logprobs: one launch, one 256-thread workgroup per row b = 0 .. B - 1 of the fp32 logits (x = logits[b * ld + 0 .. V),
 *   any V >= 1, ld >= V, no alignment asked of a row), after the sampler has left the row's token in token[b] (device):
 *     token_logprob[b, out_col] = (x[t] - max) - log(sum exp(x - max)),  t = token[b]
 *   kx_token_logprob's device code, so the same bits.  t outside [0, V): 0.0 exactly, nothing read through t.
 *   With top_n > 0 also the row's top_n entries by value descending, the lowest id first among exactly equal values (-0 == +0):
 *     top_id[b, out_col, j] = the j-th entry's id,  top_logprob[b, out_col, j] = (x[id] - max) - log(sum)   — the same formula,
 *   so slot j holds what kx_token_logprob gives for that id.  -inf entries sort last and give -inf; with V < top_n the trailing slots
 *   hold id -1 and -inf.  A NaN in the row: the log-probs are NaN as in kx_token_logprob, the ids unspecified but in [-1, V).
 *   token_logprob is [B, out_ld] fp32, top_logprob / top_id are [B, out_ld, top_n] fp32 / int64; the launch writes column out_col
 *   of them and nothing else.  skip [B] uint8 (device) or NULL: a row with skip[b] != 0 reads nothing of its logits and gets exact
 *   zeros — token_logprob 0.0, every top_logprob slot 0.0, every top_id slot -1 — what score() leaves at padded slots.
 *   The ids are selected by integer comparisons on (value, id) alone and the sums run in kx_token_logprob's fixed order: the result
 *   does not depend on B, on the row's index or on how threads split the row; two calls give identical bits.  top_n == 0 runs
 *   kx_token_logprob's two passes and no selection.
 *   Host checks (KX_ERR_INVALID_ARG, nothing launched): null logits / token / token_logprob, B < 1, V < 1, ld < V, out_col outside
 *   [0, out_ld), top_n outside 0..16, top_n > 0 with a null top_logprob or top_id.  Does not allocate or synchronise.
 * ------------------------------------------------------------------------------------------ */
int kx_step_logprobs(const float* logits, int64_t ld, int64_t B, int64_t V, const int64_t* token, const uint8_t* skip,
                     float* token_logprob, int64_t out_ld, int64_t out_col, int32_t top_n, float* top_logprob, int64_t* top_id,
                     void* stream);

/* ------------------------------------------------------------------------------------------
 * Decoding rows over a shared, read-only prefix cache plus a private tail cache (added within ABI 7: two functions are appended; no
 * struct, no existing layout moves and the kx_struct_id list is unchanged, so kx_version() stays 7).
 *
 * M rows — the n sampled continuations of each of Bp prompts, say — decode one token each.  A row's first keys are rows of a prefix
 * cache that a prefill of Bp sequences left and that nobody writes; the keys it produced itself live in a small tail cache of its own.
 *
 * kx_attention_decode_prefix: kx_attention_decode_ragged's rows — one query per (row, head) — with three int32 device words per
 *   row r: t = positions[r] (the number of keys before the new one), c = prefix_seq[r] and P = prefix_len[r].  Row r attends over
 *   keys 0 .. t: keys 0 .. P - 1 are rows 0 .. P - 1 of sequence c of the prefix caches [Bp, heads, Tmax, 64] (const: the launch has no
 *   store to them, they are bitwise unchanged), keys P .. t - 1 are rows 0 .. t - P - 1 of sequence r of the tail caches
 *   [M, heads, Ttail, 64], key t is the new token's, read from the qkv row.  The launch appends the new k / v to tail row t - P of
 *   sequence r and writes no other tail row.  Several rows may name the same c, with the same or different P; P = 0 reads the tail
 *   alone.  Same slots, key order and arithmetic on t, only the address a key is loaded from differs: one launch gives, bit for
 *   bit, the outputs and stats_out of kx_attention_decode_ragged on a private cache whose rows 0 .. P - 1 are the prefix rows and
 *   rows P .. t - 1 the tail rows, and the appended tail row is that launch's cache row t; every output form (KX_F32, KX_BF16,
 *   KX_F16C, KX_F16P), both cache dtypes, both layouts (tuning key 9, applied to both caches).  The three words are requested
 *   together: one scalar round trip before the one vector round trip.  A row with c outside [0, Bp), P < 0, P > Tmax, t < P or
 *   t - P >= Ttail writes nothing (no output, no statistics, no tail row) and ORs KX_RAGGED_ERR_CACHE into *error_word; the other
 *   rows are unaffected.  Host checks (KX_ERR_INVALID_ARG, nothing launched): null pointers, M or H empty or over the grid limits
 *   (65535), Bp / Tmax / Ttail outside 1 .. 2^31 - 1, the precision / output-form pairs of kx_attention_decode.
 * kx_decoder_decode_step_prefix: kx_decoder_decode_step_ragged with M rows, the const prefix caches [L, Bp, heads, Tmax, 64] and the
 *   tail caches [L, M, heads, Ttail, 64]: kx_step_prepare on the M tokens and positions (pos_shift as there; the XPos tables
 *   [Tmax, 32] and max_pos keep their own row counts), the qkv launch with xpos_T = M, kx_attention_decode_prefix in place of the
 *   ragged attention, everything else row-wise.  Up to 16 rows the step streams the weights, above that it runs the tile GEMMs.
 *   x [M, 1, dim] and xpos_rows [4, M, 32] scratch zeroed once by the caller; logits [M, vocab]; workspace =
 *   kx_decoder_workspace_bytes(w, M, 1, prec).
 * Neither allocates or synchronises.
 * ------------------------------------------------------------------------------------------ */
int kx_attention_decode_prefix(const void* qkv, const void* kprefix, const void* vprefix, void* ktail, void* vtail, void* out,
                               int32_t odt, float* stats_out, int64_t M, int64_t H, const int32_t* positions,
                               const int32_t* prefix_seq, const int32_t* prefix_len, int64_t Bp, int64_t Tmax, int64_t Ttail,
                               int32_t prec, int32_t* error_word, void* stream);
int kx_decoder_decode_step_prefix(const kx_decoder_weights* w, const int64_t* tokens, const float* embed, const float* pos,
                                  int64_t vocab, int64_t max_pos, int64_t pos_shift, float* x, int64_t M,
                                  const int32_t* positions, const int32_t* prefix_seq, const int32_t* prefix_len, int64_t Bp,
                                  const float* xq_cs, const float* xq_ss, const float* xk_cs, const float* xk_ss, float* xpos_rows,
                                  const void* kprefix, const void* vprefix, int64_t Tmax, void* ktail, void* vtail, int64_t Ttail,
                                  void* logits, int32_t ldt, void* workspace, size_t workspace_bytes, int32_t prec,
                                  int32_t* error_word, void* stream);

/* ------------------------------------------------------------------------------------------
 * Chunked prefill: append MANY rows to filled caches in one pass over the forward's tile GEMMs and flash attention (added
 * within ABI 7: functions only).  P is a host scalar, the number of rows every sequence already has in the caches; P = 0 is allowed.
 *
 * kx_attention_extend: qkv [B * Tn, 3 * H * 64], row b * Tn + i = sequence b's i-th new token, q pre-scaled and XPos-rotated
 *   and k rotated as the qkv GEMM's epilogue writes them.  Cache dtype and layout as kx_attention_decode: bf16 for KX_PREC_BF16,
 *   fp32 for KX_PREC_F32 and KX_PREC_F16C; per sequence [H][Tmax][64], or [Tmax][H * 64] under tuning key 9 = 1.
 *   Appends the rows' k and v to cache rows P .. P + Tn - 1 (a launch of its own), then query i attends cache rows 0 .. P + i
 *   — the causal mask with its diagonal shifted by P — reading keys from the caches only: rows at and after P + Tn are never
 *   read, whatever they hold.  nan_to_num as kx_attention applies it to causal launches (the fp32 kernel: every score; the
 *   16-bit kernels: not reachable, plain bf16 the documented divergence).  out [B * Tn, H * 64] as kx_attention writes it for the
 *   precision: fp32, or bf16 (KX_PREC_BF16, KX_PREC_F32) / KX_F16C rows (KX_PREC_F16C); stats_out [B * Tn, H, 2] optional, as
 *   kx_attn_args.stats_out.  Per query the key tiles, their order and every sum are those of kx_attention's causal launch over the
 *   P + Tn rows: rows P .. P + Tn - 1 of that launch, bit for bit with KX_PREC_F32 and KX_PREC_F16C.  KX_PREC_BF16 may differ in the
 *   last bit: that kernel's rescale factor for an unchanged running maximum is exp2 of a rounding residue (1 +- 1 ulp), applied
 *   once more to a query whose wave still has work in a tile the query itself has none in — and which queries share a wave
 *   depends on P.
 *   KX_ERR_INVALID_ARG and nothing launched: null pointers, Tn < 1, P < 0, P + Tn > Tmax, a precision or output form outside the
 *   above, pointers not 16-byte aligned, KX_PREC_F32 under tuning key 2 = 1 (the first-version kernel has no cache form).
 *   The launch has H x ceil(ceil(Tn / 128) / 2) x B workgroups (KX_PREC_F32: ceil(Tn / 64) x H x B), each walking the whole key
 *   stream below its diagonal: with P much larger than Tn that is few workgroups on long streams; there is no split over keys.
 * kx_decoder_extend: kx_decoder_prefill with the T rows at positions P .. P + T - 1 of caches that hold P rows.  xq_*, xk_*
 *   are the FULL [Tmax, 32] tables of the caches' one centring (as the ragged step takes them); the qkv GEMM reads them from row
 *   P.  x [B, T, dim] fp32 (consumed).  P = 0 is kx_decoder_prefill, launch for launch.  logits [B, T, vocab], or NULL: the call then
 *   ends after the last layer — no decoder.layer_norm, no output projection — and only the caches were its purpose.
 *   Workspace: kx_decoder_workspace_bytes(w, B, T, prec).  Precisions: those of the prefill with a cache (bf16, fp32, f16c).
 * ------------------------------------------------------------------------------------------ */
int kx_attention_extend(const void* qkv, void* kcache, void* vcache, void* out, int32_t odt, float* stats_out,
                        int64_t B, int64_t H, int64_t Tn, int64_t P, int64_t Tmax, int32_t prec, void* stream);
int kx_decoder_extend(const kx_decoder_weights* w, float* x, int64_t B, int64_t T, int64_t P,
                      const float* xq_cs, const float* xq_ss, const float* xk_cs, const float* xk_ss,
                      void* logits, int32_t ldt, void* kcache, void* vcache, int64_t Tmax,
                      void* workspace, size_t workspace_bytes, int32_t prec, void* stream);

/* ------------------------------------------------------------------------------------------
 * Ragged extend: the chunked prefill above with a per-sequence P on the DEVICE (added within ABI 7: functions only).  positions
 * int32 [B]: sequence b already holds positions[b] = P_b cache rows; its Tn new rows are positions P_b .. P_b + Tn - 1.  Tn is one
 * host value for the whole batch.  Nothing is read back to the host.
 *
 * kx_attention_extend_ragged: kx_attention_extend's operands, append and launch (same grid, same tiles, same order of sums), with P
 *   and Tk = P + Tn loaded once per workgroup from positions[b].  Sequence b of the launch gives, bit for bit in all three
 *   precisions, what a B = 1 kx_attention_extend launch at P = P_b gives: outputs, statistics and cache rows.
 *   Guard (as kx_attention_decode_block): a sequence with P_b < 0 or P_b + Tn > Tmax writes nothing — no output row, no statistics,
 *   no cache row, in the append or in the attention — and ORs KX_RAGGED_ERR_CACHE into *error_word (int32, device, sticky; the
 *   caller clears it).  The other sequences are unaffected.
 *   KX_ERR_INVALID_ARG and nothing launched: kx_attention_extend's refusals (with Tn > Tmax for the range), null positions or
 *   error_word.  Both cache layouts (tuning key 9).
 * kx_decoder_extend_ragged: kx_decoder_extend for rows that are still token ids.  Row (b, i) is embedded as kx_step_prepare embeds a
 *   row at position positions[b] + i (pos_shift as there) into x [B, T, dim] fp32 (workspace of the caller, consumed), and its
 *   four XPos rows are gathered from the FULL [Tmax, 32] tables into xpos_rows [4, B * T, 32] (caller scratch; the qkv GEMM reads
 *   them with xpos_T = B * T); then the layers, with kx_attention_extend_ragged.  A row whose position leaves the position table
 *   or the XPos tables sets KX_RAGGED_ERR_TABLE and is not embedded, a sequence that leaves the cache KX_RAGGED_ERR_CACHE: its
 *   logits rows are then undefined, the other sequences' are not touched by it.  logits [B, T, vocab], or NULL: the call ends
 *   after the last layer.  Workspace: kx_decoder_workspace_bytes(w, B, T, prec).  Precisions: bf16, fp32, f16c.
 * ------------------------------------------------------------------------------------------ */
int kx_attention_extend_ragged(const void* qkv, void* kcache, void* vcache, void* out, int32_t odt, float* stats_out,
                               int64_t B, int64_t H, int64_t Tn, const int32_t* positions, int64_t Tmax, int32_t prec,
                               int32_t* error_word, void* stream);
int kx_decoder_extend_ragged(const kx_decoder_weights* w, const int64_t* tokens, const float* embed, const float* pos,
                             int64_t vocab, int64_t max_pos, int64_t pos_shift, float* x, int64_t B, int64_t T,
                             const int32_t* positions, const float* xq_cs, const float* xq_ss, const float* xk_cs,
                             const float* xk_ss, float* xpos_rows, void* logits, int32_t ldt, void* kcache, void* vcache,
                             int64_t Tmax, void* workspace, size_t workspace_bytes, int32_t prec, int32_t* error_word,
                             void* stream);

/* ------------------------------------------------------------------------------------------
 * Host pre-processing, tensor half: what KosmosTokenizer does to images and token ids before
 * Kosmos.forward, on the device.  Integer / byte work; results are bit-identical to the HF processor.
 * ------------------------------------------------------------------------------------------ */

/* Resampling plan of one source size (H, W): Pillow ImagingResample's precomputed taps for the centre-crop window
 * only.  All arrays are DEVICE pointers to int32; built by the host binding (kosmosx/preprocess.py) in Pillow's
 * double arithmetic and fixed-point rounding (22 fractional bits).
 *   hbounds [crop][2]  (first source column, tap count) of output column left+xo;  hcoef [crop][hk] its taps
 *   vbounds [crop][2]  (first source row,    tap count) of output row    top+yo;   vcoef [crop][vk]
 *   y_first, rows_needed : union of the vertical windows  (source rows the horizontal pass must produce)
 *   x_first, span_px     : union of the horizontal windows (source columns staged per row) */
typedef struct {
  int32_t crop, hk, vk;
  int32_t y_first, rows_needed, x_first, span_px;
  const int32_t *hbounds, *hcoef, *vbounds, *vcoef;
} kx_resample_plan;

/* KosmosTokenizer.tokenize_images (/root/reference/kosmosx/model.py:88-104) -> HF CLIPProcessor(images=...)
 * .pixel_values: resize(shortest edge = crop, PIL BICUBIC) -> center_crop(crop) -> rescale(1/255) -> normalize.
 * src: B packed-RGB uint8 images of one size [B][H][W][3] (row_pitch / img_stride in bytes, 16-byte aligned base);
 * lut [3][256] float = rescale+normalize of every byte value per channel; out [B,3,crop,crop] float32;
 * out_u8 (optional, may be NULL) [B,crop,crop,3]: the uint8 image after resize + crop (the processor's
 * intermediate, for parity tests).  workspace: kx_clip_preprocess_workspace_bytes(B, plan->rows_needed, crop). */
size_t kx_clip_preprocess_workspace_bytes(int64_t B, int32_t rows_needed, int32_t crop);
int kx_clip_preprocess(const uint8_t* src, int64_t B, int32_t H, int32_t W, int64_t img_stride, int64_t row_pitch,
                       const kx_resample_plan* plan, const float* lut, float* out, uint8_t* out_u8,
                       void* workspace, size_t workspace_bytes, void* stream);

/* KosmosTokenizer.tokenize_texts / tokenize, tensor half (/root/reference/kosmosx/model.py:72-82, 114-127):
 * texts [B,L] int64 (tokenizer output, column 0 = <s>) -> tokens [B,L+2] = [<s>, im_idx, im_end_idx, texts[:,1:]],
 * mask [B, n_img+L+2] float32 = [ones(n_img) | tokens != pad_id]. */
int kx_token_splice(const int64_t* texts, int64_t B, int64_t L, int64_t im_idx, int64_t im_end_idx, int64_t pad_id,
                    int64_t n_img, int64_t* tokens, float* mask, void* stream);

/* ------------------------------------------------------------------------------------------
 * Training step, first slice (/root/reference/train.py:642-656: loss, backward,
 * clip_grad_norm_(1.0), AdamW step).  fp32 activations / gradients; the matrix products of the backward pass are
 * kx_gemm on transposed operands (dX = kx_gemm(dY, W^T), dW = kx_gemm(dY^T, X^T)).  Deterministic reductions.
 * The step itself is orchestrated by kosmosx/training.py over these entry points.
 * ------------------------------------------------------------------------------------------ */
/* dst[c][r] = src[r][c]; dt = KX_F32 or KX_BF16 */
int kx_transpose(const void* src, void* dst, int64_t rows, int64_t cols, int64_t ld_src, int64_t ld_dst, int32_t dt,
                 void* stream);
/* fp32 matrix [rows, cols] -> bf16 GEMM operand: O = transpose ? src^T : src, its K (column) dimension zero-padded to kp
 * (a multiple of 8; use 64 for kx_gemm), format fmt: 1 = bf16 rows [kp]; 2 / 3 = bf16x3 activation rows [hi|hi|lo] /
 * weight rows [hi|lo|hi], each 3*kp wide (kx_precision doc).  Mixed-precision training: fp32 master weights,
 * activations and gradients become operands right before each product. */
int kx_to_operand(const float* src, void* dst, int64_t rows, int64_t cols, int64_t ld_src, int64_t kp, int32_t transpose,
                  int32_t fmt, void* stream);
/* One pass over an fp32 matrix producing the bf16 operand rows dst [rows, kp] and/or the transposed operand rows
 * dst_t [cols, kpt] (kp >= cols, kpt >= rows, multiples of 8, padding zero; either output may be NULL) and, when
 * `colsum` is not NULL, colsum[c] = sum_r src[r][c] (a bias gradient; deterministic: one partial row per 64-row slice in
 * `workspace`, summed in slice order).  A gradient matrix is consumed all three ways, a weight forward and backward. */
size_t kx_to_operand_pair_workspace_bytes(int64_t rows, int64_t cols);
int kx_to_operand_pair(const float* src, void* dst, void* dst_t, int64_t rows, int64_t cols, int64_t ld_src, int64_t kp,
                       int64_t kpt, float* colsum, void* workspace, size_t workspace_bytes, void* stream);
/* The same pass over dpre = dg * gelu'(pre) (erf GELU; `pre` = the saved pre-activation, shape and pitch of dg): the GELU
 * backward of the training step's FFN folded into the operand conversion — outputs and column sums (fc1's bias gradient)
 * as kx_to_operand_pair's, the fp32 dpre is never written (torchscale FeedForwardNetwork: fc1 -> gelu -> ffn_layernorm ->
 * fc2; /root/reference/kosmosx/model.py:170-183 selects it). */
int kx_gelu_backward_operand_pair(const float* dg, const float* pre, void* dst, void* dst_t, int64_t rows, int64_t cols,
                                  int64_t ld_src, int64_t kp, int64_t kpt, float* colsum, void* workspace,
                                  size_t workspace_bytes, void* stream);
/* out[c] (+)= sum_r x[r][c] (bias gradients) */
size_t kx_colsum_workspace_bytes(int64_t rows, int64_t cols);
int kx_colsum(const float* x, int64_t rows, int64_t cols, int64_t ld, float* out, int32_t accumulate, void* workspace,
              size_t workspace_bytes, void* stream);
/* torch.nn.LayerNorm backward: dx = rstd*(g - mean(g) - xhat*mean(g*xhat)) (+ dres, the residual branch's gradient,
 * may be NULL), g = dy*gamma; dgamma = sum_r dy*xhat, dbeta = sum_r dy (both NULL to skip). */
size_t kx_layernorm_backward_workspace_bytes(int64_t rows, int64_t cols);
int kx_layernorm_backward(const float* x, const float* gamma, const float* dy, const float* dres, float* dx,
                          float* dgamma, float* dbeta, int64_t rows, int64_t cols, float eps, void* workspace,
                          size_t workspace_bytes, void* stream);
/* LayerNorm(gelu(pre)) and its backward with the activation rebuilt on load: torchscale's FeedForwardNetwork runs fc1 -> gelu ->
 * ffn_layernorm -> fc2 (subln; /root/reference/kosmosx/model.py:170-183), the training step keeps the pre-activation only and
 * never writes the activation.  kx_gelu_layernorm: y (KX_F32 or KX_BF16 rows) = LN(gelu(pre)) * gamma + beta, cols % 4 == 0,
 * cols <= 8192.  kx_gelu_layernorm_backward: kx_layernorm_backward with x = gelu(pre); dx is the gradient at the activation
 * (kx_gelu_backward_operand_pair continues from it); one-pass shapes only — kx_gelu_layernorm_backward_supported(cols) != 0:
 * cols a multiple of 1024 up to 4096, 6144 or 8192; workspace as kx_layernorm_backward_workspace_bytes. */
int kx_gelu_layernorm(const float* pre, const float* gamma, const float* beta, void* y, kx_dtype ydt, int64_t rows,
                      int64_t cols, float eps, void* stream);
int kx_gelu_layernorm_backward_supported(int64_t cols);
int kx_gelu_layernorm_backward(const float* pre, const float* gamma, const float* dy, const float* dres, float* dx,
                               float* dgamma, float* dbeta, int64_t rows, int64_t cols, float eps, void* workspace,
                               size_t workspace_bytes, void* stream);
/* exact (erf) GELU forward on a kept pre-activation, and its backward: dpre = dg * (Phi(pre) + pre*phi(pre)) */
int kx_gelu_forward(const float* pre, float* out, int64_t n, void* stream);
int kx_gelu_backward(const float* pre, const float* dg, float* dpre, int64_t n, void* stream);
/* HF QuickGELUActivation (CLIP's MLP, modeling_clip.py: x * sigmoid(1.702 x)) on a kept pre-activation, and its backward */
int kx_quick_gelu_forward(const float* pre, float* out, int64_t n, void* stream);
int kx_quick_gelu_backward(const float* pre, const float* dg, float* dpre, int64_t n, void* stream);
/* out[r][c] = x[r][c] + vec[c]: flamingo PerceiverResampler's `x + media_pos_emb[:times]` kept as a tensor (the
 * backward of norm_media needs it); cols % 4 == 0, 16-byte aligned buffers */
int kx_add_rowvec(const float* x, const float* vec, float* out, int64_t rows, int64_t cols, void* stream);
/* The vision tower's embeddings as stand-alone steps for the op-by-op training forward (HF CLIPVisionEmbeddings):
 * kx_patchify: pixels [B,3,image,image] fp32 -> patch rows [B*(image/patch)^2, kpad] (fp32 for KX_PREC_F32, bf16 for
 * KX_PREC_BF16), columns (channel, dy, dx) as nn.Conv2d's weight.flatten(1), zero padded to kpad;
 * kx_vit_assemble: x[b] = cat(class_embedding, patch_out[b]) + position_embedding, [B, tokens, dim] fp32;
 * dim % 4 == 0, 16-byte aligned buffers (rows move as 16-byte vectors). */
int kx_patchify(const float* pixels, void* patches, int64_t B, int32_t image, int32_t patch, int32_t kpad, int32_t prec,
                void* stream);
int kx_vit_assemble(const float* patch_out, const float* cls, const float* pos, float* x, int64_t B, int32_t tokens,
                    int32_t dim, void* stream);
/* F.cross_entropy rows: loss_rows[r] = logsumexp(logits[r]) - logits[r][target[r]] (0 for targets outside [0,V):
 * ignore_index); dlogits (optional) = (softmax - onehot) * scale. */
int kx_cross_entropy(const float* logits, int64_t rows, int64_t V, int64_t ld, const int64_t* target, float scale,
                     float* loss_rows, float* dlogits, int64_t ldd, void* stream);
/* out[0] (+)= sum x[i] (squares != 0: sum x[i]^2 — the gradient norm); workspace >= 4 KB */
int kx_reduce_sum(const float* x, int64_t n, int32_t squares, float* out, int32_t accumulate, void* workspace,
                  size_t workspace_bytes, void* stream);
/* backward of the qkv epilogue (q *= qscale, XPos rotate/scale of q and k), in place on the fused [M,3D] gradient */
int kx_xpos_backward(float* dqkv, int64_t M, int64_t D, int64_t T, const float* xq_cs, const float* xq_ss,
                     const float* xk_cs, const float* xk_ss, float qscale, void* stream);
/* dembed[v] = sum of dx rows whose token is v (overwrites all vocab rows); dpos[2+pos_offset+t] = sum_b dx[b,t] */
int kx_embed_backward(const int64_t* tokens, const float* dx, int64_t B, int64_t T, int64_t d, int64_t vocab,
                      int64_t pos_offset, float* dembed, float* dpos, void* stream);
/* torch.optim.AdamW step on one flat fp32 tensor; grad_norm_sq (optional, device scalar) + max_norm apply
 * clip_grad_norm_'s factor min(1, max_norm / (norm + 1e-6)) to the gradient on the fly. */
int kx_adamw(float* param, const float* grad, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
             float weight_decay, int64_t step, const float* grad_norm_sq, float max_norm, void* stream);
/* lion_pytorch.Lion step (the optimizer the reference's train.py:547-556 selects) on one flat fp32 tensor:
 * p *= 1 - lr*wd;  p -= lr * sign(beta1*m + (1-beta1)*g);  m = beta2*m + (1-beta2)*g;  optional clip factor as kx_adamw. */
int kx_lion(float* param, const float* grad, float* m, int64_t n, float lr, float beta1, float beta2, float weight_decay,
            const float* grad_norm_sq, float max_norm, void* stream);
/* Attention backward (head_dim 64): q/k/v/dq/dk/dv are column blocks of fused [B*T, 3D] buffers (row / batch strides in
 * elements, the same for the inputs and the fp32 gradients), out/dout [B,T,D] fp32; lse [B,H,T] from kx_attention
 * (lse_out); delta [B,H,T] scratch.  qkv_dt: dtype of q/k/v (KX_F32, or KX_BF16 with bf16 products).
 * prec: KX_PREC_F32 = exact-f32 MFMA; KX_PREC_BF16 = bf16 MFMA products (fp32 inputs are rounded on the way in,
 * statistics and accumulators stay fp32) for mixed-precision training. */
int kx_attention_backward(const void* q, const void* k, const void* v, int32_t qkv_dt, const float* out, const float* dout,
                          const float* lse, float* dq, float* dk, float* dv, float* delta, int64_t B, int64_t H, int64_t T,
                          int64_t qkv_row_stride, int64_t qkv_batch_stride, int64_t out_row_stride,
                          int64_t out_batch_stride, int32_t mask, int32_t prec, void* stream);

/* kx_attention_backward for a forward that ran with kx_attn_args.dropout_p > 0 (same seed / site; fp32 q/k/v) */
int kx_attention_backward_dropout(const float* q, const float* k, const float* v, const float* out, const float* dout,
                                  const float* lse, float* dq, float* dk, float* dv, float* delta, int64_t B, int64_t H,
                                  int64_t T, int64_t qkv_row_stride, int64_t qkv_batch_stride, int64_t out_row_stride,
                                  int64_t out_batch_stride, int32_t mask, float dropout_p, uint64_t seed, int32_t site,
                                  void* stream);
/* The same on the matrix-core passes with bf16 products (q/k/v: KX_F32 rounded on the way in, or KX_BF16 as stored — what
 * kx_attention_backward takes with KX_PREC_BF16), for a KX_PREC_BF16 forward that ran with dropout_p > 0 (reference:
 * attention_dropout = 0.1 under model.train(), /root/reference/kosmosx/model.py:177, /root/reference/train.py:642). */
int kx_attention_backward_dropout_bf16(const void* q, const void* k, const void* v, int32_t qkv_dt, const float* out,
                                       const float* dout, const float* lse, float* dq, float* dk, float* dv, float* delta,
                                       int64_t B, int64_t H, int64_t T, int64_t qkv_row_stride, int64_t qkv_batch_stride,
                                       int64_t out_row_stride, int64_t out_batch_stride, int32_t mask, float dropout_p,
                                       uint64_t seed, int32_t site, void* stream);
/* Inverted dropout of the training step (torchscale dropout_module after the embedding, after out_proj and after fc2,
 * reference dropout = 0.1, kosmosx/model.py:175): y = (residual +) keep(i) * x / (1 - p), keep = Philox4x32-10(seed; i, site).
 * Applied to a gradient it is its own backward.  kx_dropout_mask exports the keep bytes (what the CPU autograd reference
 * multiplies by — test infrastructure). */
int kx_dropout(const float* x, const float* residual, float* y, int64_t n, float p, uint64_t seed, int32_t site, void* stream);
int kx_dropout_mask(uint8_t* keep, int64_t n, float p, uint64_t seed, int32_t site, void* stream);

/* Kernel-variant selection for in-process A/B measurement (tools/gemm_bench.py, tools/ln_bench.py).  Defaults (all 0) are the
 * shipped configuration.  key 0: LayerNorm variant (0 wave-per-row, 1 workgroup-per-row);
 * key 1: GEMM tile override used by the stage-level entry points (0 auto, else as kx_gemm_args.tile);
 * key 2: attention variant (0 = bf16 v2: 32 queries/wave, transpose-read V, prefetched tiles / fp32 on the matrix
 *        cores; 1 = the first versions: bf16 v1 / fp32 wave-per-query VALU kernel; 4 = KX_PREC_F16C attention with P and V as
 *        plain fp16 — one product for O += P V instead of three; A/B only: 1.5e-3 on the logits, outside the tolerance; 5 = unmasked bf16 / fp16
 *        launches fold a last query block of <= 32 queries into a fifth wave — bit-identical, 0.8 % slower in situ;
 *        6 / 7 = KX_PREC_F16C causal attention with ONE cross term of O += P V dropped (6: P plain, V split; 7: P split, V plain:
 *        two products instead of three; A/B); 8 = causal KX_PREC_F16C launches keep 32 consecutive queries per wave
 *        instead of two 16-query blocks 64 rows apart (bit-identical, A/B));
 * key 3: 256x256 GEMM start stagger per phase group in 10 ns ticks (0 = none; measured useless, kept for A/B);
 * key 4: GEMM epilogue (0 auto: lean bf16 tile store where it applies, prefetching store loop for residual / statistics /
 *        XPos operands; 1 rolled per-pass loop everywhere, no lean epilogue; 2 prefetching loop everywhere; 10 = the row-owning
 *        split-K reduce keeps its unspecialised form (eight column groups per thread, operands loaded where they are used; A/B));
 * key 5: phased GEMM kernels skip the MFMAs of waves whose rows are all beyond M (0 on, 1 off);
 * key 6: kx_clip_preprocess reads its taps from global memory instead of the LDS-staged row (0 auto, 1 force);
 * key 7: the 256-column GEMM kernel is launched persistently, each workgroup walking its own tiles (0 = one workgroup
 *        per CU, n > 0 = n workgroups, -1 = one workgroup per tile);
 * key 8: tile-16 weight-streaming kernel (0 = second form: small loads first, counted waits, one-barrier LayerNorm
 *        prologue, 16 KB per wave in flight for K slices of 512; 1 = the first form; 2 = second form without the
 *        16 KB variant; 3 = second form whose 5..8-row LayerNorm prologue walks its row three times instead of
 *        keeping it in registers; 4 = fp32 operands with one or two rows multiply on the matrix pipe instead of the VALU;
 *        5 = block-scaled 16-bit planes (w_tiled = 3) keep the exact-f32 MFMA where the default multiplies fp16 pieces;
 *        7 = LayerNorm-prologue launches of 9..16 rows keep eight waves and the three-walk prologue (default: sixteen
 *        waves, one row per wave in registers); 10 + n = the VALU form takes up to n rows (default 2));
 * key 9: KV-cache layout per layer and sequence (0 = [heads][Tmax][64]; 1 = the first layout [Tmax][heads*64]; set it
 *        before a prefill and keep it for that cache's steps).
 * key 10: 1 = the fp32 decode step keeps the split-K tile kernels instead of the fp32 weight-streaming kernel (A/B).
 * key 11: 1 = the streamed decode step keeps ONE workgroup per 16 columns in its residual GEMMs (no kx_gemm_args.ksplit pair).
 * key 12: 1 = the fp16-pieces decode step keeps fp32 rows between its kernels (each consumer splits them itself) instead of
 *         KX_F16P rows written by the producers (A/B).
 * key 13: 1 = never take the pair split of the 256x256 kernel (kx_gemm_args.pair_ws) automatically (A/B); 2 = FAULT INJECTION
 *         (tests of the bounded hand-off): the odd workgroup of every pair never publishes its flag and the poll's bound is 2 ms
 *         — the launch must complete and kx_pair_split_errors must report it.
 * key 14: K loop of the 256-column kernel (0 = the balanced form: the LDS-DMA of a K-tile issued in two halves, one per read
 *         phase, counted vmcnt waits; 1 = the first form: whole tile issued in the first read phase, vmcnt(0) in the second.
 *         The two are bit-identical).
 * key 15: bit mask that switches automatic kernel-choice rules of round 5 OFF (A/B): 1 = 16-bit lean-store GEMMs whose padded
 *         256 x 256 rounds cover <= 1.5x the problem take the 256-column kernel (the ViT's qkv / fc1); 2 = residual GEMMs
 *         with a ragged last 160-row tile take 192 x 256 tiles (the ViT's fc2 / out_proj at M = 32 * 257); 4 = the f16c decoder's
 *         qkv GEMM writes KX_F16HL pieces for the attention kernel at T >= 512.  Bit 8 switches one rule ON: plain fp16 GELU outputs of
 *         the 256-column kernel's lean epilogue use the transcendental-free polynomial of the bf16 outputs (A/B: +0.6 %, not shipped).
 *         16 = fp32-with-residual outputs of the 256-column kernel keep the generic store loop (lean_store_f32_res off);
         64 = one-round problems that fill >= 0.8 of the CUs with 192 x 256 tiles keep the 128 / 160-row kernels (the Perceiver's
         to_kv; the rule never applies to launches with produced statistics, ln_operand_out, KX_F16C / KX_BF16X3 outputs or residual +
         16-bit output, which were not measured on these tiles); Bit 32 switches one rule ON:
 *         folded sub-LayerNorm statistics given as row_stats_scratch + stats_partials are finalised inside the pair-split launch (slower).
 * key 18: SCHEDULING OBJECTIVE of the automatic kernel choice.  0 (default) = latency: every launch is chosen to finish soonest
 *         ALONE on the chip (rounds x tile time) — one step at a time, batch 1, decode, training.  1 = throughput: for a caller
 *         that keeps two or more steps in flight on separate streams (bench.py's headline loop, a serving loop), where a launch's
 *         idle CUs are filled by the other steps' kernels and what counts is its CU-microseconds: 256-row tiles wherever 192-row
 *         ones were chosen to save nothing but padding.  Same results bit for bit (the tile height does not change an element's
 *         summation order); measured +2.7 % with two steps in flight, -3 % with one.
 *         key 15 & 256 is the same rule as an A/B bit (15 & 1024 / 2048 exclude the XPos launches / all the others from it); key 15 & 128 = whole 256 x 256 tiles on half the chip instead of the pair
 *         split (+0.2 % on top with two steps in flight, -10 % with one: A/B only).
 * key 17: in-launch split-K reduction (kx_gemm_args.splitk_flags).  0 = kx_gemm honours the field, the stage entry points do not
 *         pass it (MEASURED: 0.4-4 us slower per batch-1 GEMM than the reduce launch it replaces, batch-1 forward 4.52 vs 3.85 ms);
 *         1 = the stage entry points hand every split-K launch their flag words (A/B); 2 = kx_gemm ignores the field.
 * key 16: per-family fp8-correction assignment of the KX_PREC_F16C stage entry points, two bits (a kx_f16c_corr value) per GEMM
 *         family: bits 0-1 decoder qkv, 2-3 out_proj, 4-5 fc1, 6-7 fc2, 8-9 output projection, 10-11 every Perceiver GEMM.
 *         0 = both corrections everywhere.  -1 = the library's shipped default. */
int kx_set_tuning(int key, int value);

/* ------------------------------------------------------------------------------------------
 * Token-automaton constrained decoding (added within ABI 7: one struct and one function are appended; no existing layout moves
 * and the kx_struct_id list is unchanged — kx_automaton_args carries its own struct_bytes, which kx_automaton_step checks, as
 * kx_spec_args does — so kx_version() stays 7).
 *
 * Where kx_constrain_logits bans ids by the row's history, kx_automaton_step bans them by the row's STATE in an automaton over
 * token ids that the caller compiled (a set of answers, a whitelist, a regular expression or a schema over ids).  The state lives
 * on the device and advances from the token kx_sample_logits or kx_beam_step just left there.  One launch, issued BEFORE the
 * sampler or the beam step (after the step's kx_constrain_logits launch, if any) on the fp32 rows logits [B, V] (any ld >= V) that
 * kernel is about to read; a banned id's logit becomes -inf and nothing else is written, so neither kernel changes and the mask
 * commutes with the other bans and with the repetition penalty.  The logits are never read.
 *
 * The automaton is four device tables in CSR form, uploaded once per generate() call; S states and E edges are host scalars:
 *   edge_off     int32 [S + 1]   state s owns edges [edge_off[s], edge_off[s + 1])
 *   edge_tok     int32 [E]       the id an edge is taken on, strictly ascending within a state
 *   edge_next    int32 [E]       the next state, or -1: this id is banned here
 *   default_next int32 [S]       where an id the state does not list leads, or -1: every unlisted id is banned
 * (sparse-allow states: default -1 and a few edges; sparse-deny states: a default and a few -1 edges; no S x V table.)
 * state_in int32 [B_in], state_out int32 [B] (must not overlap: KX_ERR_INVALID_ARG, nothing launched — a loop alternates two
 * buffers, which is what lets several workgroups work on one row), src_row int32 [B] or NULL (beams: kx_beam_step's src_row, the row
 * of state_in each row descends from; NULL needs B_in == B), last_token int64 [B] or NULL (NULL at step 0), finished uint8 [B] or
 * NULL (read only).  Per row b, in order:
 *   1. s = state_in[src_row ? src_row[b] : b]; a src_row entry outside [0, B_in) or an s outside [0, S) is the dead state -1;
 *   2. finished[b] != 0: state_out[b] = s and the row is left untouched;
 *   3. last_token != NULL and s >= 0: advance on t = last_token[b] — a listed edge gives s = its edge_next (maybe -1), an unlisted
 *      t in [0, V) gives s = default_next[s], a t outside [0, V) gives -1;
 *   4. state_out[b] = s;
 *   5. mask: in the dead state the whole row becomes -inf; otherwise id v is allowed iff it is listed with next >= 0, or unlisted
 *      with default_next[s] >= 0.  Allowed entries keep their bit pattern, NaN included;
 *   6. range: offsets are clamped into [0, E] and a state whose offsets are out of order has no edges; an edge_tok outside [0, V)
 *      is skipped; an edge_next or default_next outside [-1, S) is read as -1; ids are compared as values and never used as an index
 *      without the range check: memory safety does not depend on the device data.
 * A row in which every id is banned falls under the sampler's rule 6: it emits pad_id and becomes finished — a state with no way
 * out is how a grammar without an EOS ends a row.  Under beams such a state only kills the beam: a hypothesis ends by eos_id alone.
 * 256-thread workgroups, one per (row, slice of 4096 ids): each repeats the row's advance (a binary search over the state's
 * edges), the row's first writes state_out[b]; the slice's allowed set is a 512-byte bitmap in LDS filled from the default and
 * edited per edge with LDS atomics, then consecutive lanes store -inf to consecutive banned ids.
 * Limits (KX_ERR_UNSUPPORTED, before any launch): V <= 2^23 (kx_sample_logits' own limit; the bitmap covers a slice, not the row);
 * 1 <= S < 2^31, E < 2^31; B x ceil(V / 4096) < 2^31 workgroups.  Argument errors name the argument.  Never allocates, never
 * synchronises. */
typedef struct {
  uint32_t struct_bytes;                      /* = sizeof(kx_automaton_args) of the caller ("stale binding" otherwise) */
  int32_t reserved;
  float* logits; int64_t ld; int64_t B; int64_t V;
  const int32_t* edge_off; const int32_t* edge_tok; const int32_t* edge_next; const int32_t* default_next;
  int64_t S; int64_t E;
  const int32_t* state_in; int64_t B_in;
  int32_t* state_out;
  const int32_t* src_row;                     /* [B] or NULL */
  const int64_t* last_token;                  /* [B] or NULL */
  const uint8_t* finished;                    /* [B] or NULL, read only */
} kx_automaton_args;
int kx_automaton_step(const kx_automaton_args* args, void* stream);

/* ------------------------------------------------------------------------------------------
 * Logit shaping: logit bias, presence / frequency penalties and min-p (added within ABI 7: one struct and two functions are
 * appended; no existing layout moves and the kx_struct_id list is unchanged — kx_shape_args carries its own struct_bytes, which
 * kx_shape_logits checks, as kx_automaton_args does; kx_sample_args is untouched — so kx_version() stays 7).
 *
 * Order per row and step: kx_constrain_logits' bans, kx_automaton_step's bans, kx_shape_logits, then the sampler; inside the
 * sampler min-p comes after top-p.
 *
 * kx_shape_logits: one launch on the fp32 rows logits [B, V] (any ld >= V) the sampler is about to read, edited in place.
 *   bias_off  int32 [B + 1] or NULL   row b owns the bias entries [bias_off[b], bias_off[b + 1]) (CSR; n_bias entries in all)
 *   bias_ids  int32 [n_bias]          the ids, strictly ascending within a row
 *   bias_val  fp32  [n_bias]          finite, or -inf: a ban
 *   counts    int32 [B, V] in/out, or NULL when both penalties are 0: c_i = how often THIS call has emitted id i for the row so
 *             far — the caller zeroes it once before the first step; the prompt does not count
 *   frequency f, presence p           finite host floats, negative allowed
 *   last_token int64 [B] or NULL      the sampler's next_token of the previous step (NULL at step 0)
 *   finished  uint8 [B] or NULL       read only
 * Per row b, in order:
 *   1. finished[b] != 0: the row is left alone, its logits and its counts (the pads of a finished row do not count);
 *   2. count: counts[b, last_token[b]] += 1; a last_token outside [0, V) is ignored;
 *   3. bias: every listed id gets l = l + value, one IEEE fp32 add;
 *   4. penalty: where c_i > 0, l = (l - f * (float)c_i) - p — three separate IEEE fp32 operations, never contracted into an FMA,
 *      so a numpy float32 restatement matches bit for bit; where c_i == 0 the logit is untouched;
 *   5. a logit that is -inf or NaN when step 3 or step 4 meets it keeps its bit pattern: a bias never revives a banned id;
 *   6. range: offsets are clamped into [0, n_bias] and a row whose offsets are out of order has no entries; a bias id outside
 *      [0, V) is skipped; ids and the last token are compared as values and never used as an index without the range check: a
 *      malformed table changes what is shaped, never what is addressed.
 * The shaping comes before the sampler's own repetition penalty (its rule 1).
 * 256-thread workgroups, one per (row, slice of 4096 ids), with no hand-off between workgroups: the thread that owns element i is
 * the only one that reads or writes counts[b, i] and logits[b, i] — the count is c = stored + (i == last), stored back by that
 * owner; the bias entries are applied by the workgroup that owns their slice, before a barrier and the penalty pass.
 * Limits (KX_ERR_UNSUPPORTED, before any launch): V <= 2^23 (kx_sample_logits' own limit), n_bias < 2^31, B x ceil(V / 4096) <
 * 2^31 workgroups.  Argument errors (a non-finite penalty, a penalty without counts, neither a bias table nor counts) name the
 * argument.  Never allocates, never synchronises. */
typedef struct {
  uint32_t struct_bytes;                      /* = sizeof(kx_shape_args) of the caller ("stale binding" otherwise) */
  int32_t reserved;
  float* logits; int64_t ld; int64_t B; int64_t V;
  const int32_t* bias_off;                    /* [B + 1] or NULL */
  const int32_t* bias_ids; const float* bias_val; int64_t n_bias;
  int32_t* counts;                            /* [B, V] in/out, or NULL */
  float frequency; float presence;
  const int64_t* last_token;                  /* [B] or NULL */
  const uint8_t* finished;                    /* [B] or NULL, read only */
} kx_shape_args;
int kx_shape_logits(const kx_shape_args* args, void* stream);

/* kx_sample_logits_min_p: kx_sample_logits (positions == NULL; advance is unused) or kx_sample_logits_ragged (positions != NULL)
 * with one more filter, min_p = m in [0, 1] (0 = off: the launch of the other two entry points).  The `transformers` order —
 * temperature -> top-k -> top-p -> min-p: after top-k and top-p have fixed their threshold on x = penalised logit / T, the kept
 * set is additionally restricted to x_i >= x_max + lm, one fp32 add and a compare, with lm = (float)log((double)m) computed once
 * on the host: p_i >= m p_max.  Top-p's mass stays renormalised over what top-k kept, not over what min-p keeps.  The arg max is
 * always kept; m = 1 keeps exactly the ties at the maximum.  Under greedy it is ignored, as top-k is.  kx_sample_args is unchanged.
 * An m outside [0, 1] (NaN included): KX_ERR_INVALID_ARG naming min_p, before any launch. */
int kx_sample_logits_min_p(const kx_sample_args* args, int32_t* positions, int64_t advance, float min_p, void* stream);

/* ------------------------------------------------------------------------------------------
 * Truncation sampling: typical-p, epsilon and eta (added within ABI 7: one struct and one function are appended; no existing
 * layout moves and the kx_struct_id list is unchanged — kx_truncate_args carries its own struct_bytes, which
 * kx_sample_logits_truncate checks, as kx_shape_args does; kx_sample_args is untouched — so kx_version() stays 7).
 *
 * kx_sample_logits_truncate: kx_sample_logits_min_p (positions == NULL: the uniform form, advance unused; positions != NULL: the
 * ragged form) with up to three more filters behind min-p, the `transformers` warper order — temperature -> top-k -> top-p ->
 * min-p -> typical-p -> epsilon -> eta.  Each stage takes its probabilities renormalised over what the stage before it kept.
 * With typical_p == 1, epsilon_cutoff == 0 and eta_cutoff == 0 it IS kx_sample_logits_min_p(args, positions, advance, min_p):
 * the same launches.  Otherwise one launch of one more instantiation of the sampler's kernel, min-p inside it.
 *
 * Notation: x_i = the sampler's penalised logit / T (its rules 1-2), m = the row maximum, w_i = exp(x_i - m) in 2^-40 fixed
 * point, truncated (x_i == m gives exactly 2^40, also when both are +inf) — the mass top-p already sums; S0 = the set the
 * sampler's rules 1-4 and min-p keep.  Three properties hold for everything below:
 *   (a) every sum is a 64-bit INTEGER sum (V <= 2^23 elements of at most 2^40 keep it below 2^63);
 *   (b) every per-element quantity is a stated sequence of single IEEE operations;
 *   (c) no result depends on the order in which lanes, waves or LDS atomics run: a row's outputs do not depend on B or on its
 *       row index, and two calls give identical bits.
 * Over a set S: Z(S) = sum of w_i; E(S) = sum of e_i with e_i = (uint64)((double)w_i * (double)(m - x_i)), m - x_i one fp32
 * subtraction, and e_i = 0 where x_i == m or w_i == 0 (the +inf ties; w (m - x) <= 2^40 / e per element);
 * mu(S) = (float)((double)E / (double)Z): the expected surprise minus (lse - m).
 *
 * typical_p = t in (0, 1], 1 = off.  With mu = mu(S0): d_i = fabsf(s_i - mu), s_i = m - x_i (0 where x_i == m) — two fp32
 * operations and an absolute value; the lse cancels out of |-log p_i - H|, no logarithm is taken.  i in S0 stays iff the mass of
 * {j in S0 : d_j < d_i} (STRICTLY smaller) is < ceil((double)t * Z(S0)) — the integer form top-p uses, found by the same radix
 * select over the order-preserving key of d, ascending.  Ties in d stay or go together.  This is TypicalLogitsWarper: it always
 * keeps the tokens of least d — not necessarily the arg max.  S1 = what stays.
 * epsilon_cutoff = e in [0, 1), 0 = off.  i in S1 stays iff w_i >= ceil((double)e * Z(S1)), or x_i is the maximum of S1
 * (min_tokens_to_keep = 1; exact ties at that maximum all stay).  S2 = what stays.
 * eta_cutoff = e in [0, 1), 0 = off.  With H2 = log(Z(S2) 2^-40) + mu(S2), the entropy of S2's distribution, the cut-off is
 * min(e, sqrt(e) exp(-H2)); it is applied as the integer compare w_i >= ceil(c), c = min((double)e * Z(S2),
 * sqrt((double)e) * exp(-(double)mu(S2)) * 2^40) computed once per row in double by one thread, or x_i is the maximum of S2
 * (which is the maximum of S1).
 * A stage whose Z is 0 keeps what it was given.  (S0 always holds the arg max, and a stage never drops all mass it was handed, so
 * this is a guard and not a reachable state; the nearest reachable row — everything but the maximum underflows 2^-40 relative to
 * m — is handled by the rules as written: e_i = 0 there, mu = 0, and the maximum alone has d = 0.)
 * The Gumbel draw runs over the conjunction of all stage predicates; keep_mask / kept_count report that final set.  Under greedy
 * all three are ignored, as top-k and min-p are.  Finished rows and rows without a candidate behave as in kx_sample_logits.
 * Passes over the row (it stays in L2): typical-p 1 + 3, epsilon 1, eta 1; no LDS beyond the sampler's own.
 * Argument errors (KX_ERR_INVALID_ARG, nothing launched, the message names the argument): a null trunc, a stale struct_bytes,
 * min_p outside [0, 1], typical_p outside (0, 1], epsilon_cutoff or eta_cutoff outside [0, 1) (NaN included), a negative
 * advance; then kx_sample_logits' own.  Never allocates, never synchronises. */
typedef struct {
  uint32_t struct_bytes;                      /* = sizeof(kx_truncate_args) of the caller ("stale binding" otherwise) */
  float min_p;                                /* [0, 1], 0 = off: kx_sample_logits_min_p's argument */
  float typical_p;                            /* (0, 1], 1 = off */
  float epsilon_cutoff;                       /* [0, 1), 0 = off */
  float eta_cutoff;                           /* [0, 1), 0 = off */
  int32_t reserved;
} kx_truncate_args;
int kx_sample_logits_truncate(const kx_sample_args* args, int32_t* positions, int64_t advance, const kx_truncate_args* trunc, void* stream);

/* ------------------------------------------------------------------------------------------
 * Classifier-free guidance (added within ABI 7: one struct and one function are appended; no existing layout moves and the
 * kx_struct_id list is unchanged — kx_guidance_args carries its own struct_bytes, which kx_guidance_logits checks, as
 * kx_shape_args does — so kx_version() stays 7).
 *
 * generate(guidance_scale = s) runs every sequence as two rows of one ragged batch: row b reads the prompt (the conditional row),
 * row B + b a negative prompt or a negative image (the unconditional row); both are fed the same sampled token.  Order per step:
 * kx_guidance_logits, then kx_constrain_logits' bans, kx_automaton_step's bans, kx_shape_logits, then the sampler — bans and
 * biases apply to the guided row, the `transformers` order.
 *
 * kx_guidance_logits: one launch on B pairs of raw fp32 rows.
 *   cond, ld_cond      fp32 [B, V]   the conditional rows
 *   uncond, ld_uncond  fp32 [B, V]   the unconditional rows
 *   out, ld_out        fp32 [B, V]   the guided rows; out may be cond with ld_out == ld_cond (in place), and overlaps neither input
 *                                    otherwise
 *   Any ld >= V; no alignment is asked of a row.
 *   scale s            a finite host float; 1 reproduces the conditional log-softmax, 0 the unconditional one
 *   finished  uint8 [B] or NULL      read only
 *   positions int32 [B] or NULL      in/out: the unconditional rows' device positions
 *   advance   0 or 1
 * Per pair b, in order:
 *   1. log-probs: lc_i = (c_i - max c) - log(sum exp(c - max c)), likewise lu_i from the unconditional row — the arithmetic and
 *      the summation order of kx_token_logprob, bit for bit what it returns for that row and id;
 *   2. combine: out_i = lu_i + s * (lc_i - lu_i) — a subtract, a multiply and an add in IEEE fp32, never contracted into an FMA, so
 *      a numpy float32 restatement over the device's own log-probs matches bit for bit;
 *   3. a result that is not finite (either input -inf or NaN at i, a NaN anywhere in a row — its sum is NaN —, a row of -inf
 *      alone, overflow) is written as -inf: such an id is never a candidate, and a row of nothing but -inf makes the sampler emit
 *      a pad and finish the row (its rule 6);
 *   4. finished[b] != 0: out row b is not written and neither input row is read;
 *   5. positions != NULL and advance != 0: one lane stores positions[b] + advance, finished rows included — the rule
 *      kx_sample_logits_ragged follows for the conditional rows, so an unconditional row moves exactly when its partner does.
 * One 256-thread workgroup per pair with no hand-off between workgroups: results do not depend on B or on the pair's index, and
 * two calls give identical bits.
 * Limits (KX_ERR_UNSUPPORTED, before any launch): V <= 2^23 (kx_sample_logits' own limit).  Argument errors (KX_ERR_INVALID_ARG,
 * nothing launched, the message names the argument): a null cond, uncond or out, B < 1, V < 1, an ld < V, a non-finite scale, an
 * advance outside {0, 1}, out overlapping uncond, out overlapping cond without being cond.  Never allocates, never synchronises. */
typedef struct {
  uint32_t struct_bytes;                      /* = sizeof(kx_guidance_args) of the caller ("stale binding" otherwise) */
  int32_t reserved;
  const float* cond; int64_t ld_cond;
  const float* uncond; int64_t ld_uncond;
  float* out; int64_t ld_out;
  int64_t B; int64_t V;
  float scale; int32_t reserved2;
  const uint8_t* finished;                    /* [B] or NULL, read only */
  int32_t* positions;                         /* [B] or NULL, in/out */
  int64_t advance;
} kx_guidance_args;
int kx_guidance_logits(const kx_guidance_args* args, void* stream);

/* ------------------------------------------------------------------------------------------
 * Per-row sampling options: a batch of unlike requests in one launch (added within ABI 7: two structs and three functions are
 * appended; no existing layout moves and the kx_struct_id list is unchanged — kx_sample_rows_args carries its own struct_bytes,
 * which kx_sample_logits_rows checks, as kx_truncate_args does; kx_sample_args and kx_shape_args are untouched — so kx_version()
 * stays 7).
 *
 * kx_sample_row: what one row of the batch asked of the sampler — everything kx_sample_args and kx_truncate_args carry once per
 * launch.  56 bytes, 8-byte aligned; the table of a launch is B of them, consecutive.
 *
 * kx_sample_rows_pack: `in` [B] host records -> `out` [B] host records ready for upload, and the launch summary in *flags_out.
 * Host only and pure: it touches no device and makes no runtime call.  Every record is validated with the rules of
 * kx_sample_logits, kx_sample_logits_min_p and kx_sample_logits_truncate — temperature >= 0, top_p > 0, repetition_penalty > 0,
 * min_p in [0, 1], typical_p in (0, 1], epsilon_cutoff and eta_cutoff in [0, 1) (NaN refused everywhere), max_new >= 0 — else
 * KX_ERR_INVALID_ARG with a message that names the row and the field, and *flags_out is not written.  out[b] is in[b] with
 * log_min_p = (float)log((double)min_p), the expression kx_sample_logits_min_p evaluates (0 where min_p == 0: off), and the
 * reserved word 0.  Flags: KX_SAMPLE_ROWS_PENALTY (bit 0) some row has repetition_penalty != 1; KX_SAMPLE_ROWS_BUDGET (bit 1)
 * some row has max_new > 0.  in == out is allowed; B >= 1, V >= 1 (the vocabulary the table is meant for).
 *
 * kx_sample_logits_rows: kx_sample_logits_truncate (positions == NULL: the uniform form, advance unused; positions != NULL: the
 * ragged form) with row b sampled under rows->table[b] instead of the launch's scalars: greedy or not (do_sample == 0 or
 * temperature == 0: greedy, every filter ignored), repetition penalty, temperature, top-k, top-p, min-p through log_min_p,
 * typical-p, epsilon, eta — the same stages in the same order over the same passes, LDS and 1024-thread workgroup — and seed as
 * the row's Philox key; the counter stays (position, sequence id, i >> 2, 0).  Row b's outputs are bit for bit those of a one-row
 * launch of the scalar entry points with the record's values.  One more instantiation of the sampler's kernel per form; its
 * workgroup reads its record through a workgroup-uniform address, so every branch on a record value is uniform.
 *   rows->table   DEVICE memory, B records as kx_sample_rows_pack wrote them; rows->flags: the pack's.
 *   The scalar sampling fields of args (do_sample, temperature, top_k, top_p, repetition_penalty, seed) are ignored — not read,
 *   not validated.  Everything else in args means what it means in kx_sample_logits.
 * Rules:
 *   1. the launch carries the history bitmap in LDS iff flag bit 0 is set, history != NULL and hist_len > 0; then V <= 327680
 *      (KX_ERR_UNSUPPORTED), as for kx_sample_logits with a penalty;
 *   2. a record with repetition_penalty != 1 in a launch without the bitmap is read as 1; in a launch with it a record of exactly 1
 *      divides and multiplies by 1 (exact).  No record value ever decides whether LDS is addressed;
 *   3. flag bit 1 with finished == NULL is KX_ERR_INVALID_ARG; with flag bit 1 clear every max_new is read as 0;
 *   4. a row with max_new > 0 becomes finished by the launch in which out_col + 1 >= max_new (out_col counts the launches of the
 *      call whether or not out_tokens is given).  The token of that launch is emitted normally; from the next launch on the row
 *      emits pad_id, as a row that drew the EOS does;
 *   5. record values are compared and used in arithmetic only, never as an index; top_k outside (0, V) is off.  A malformed table
 *      changes what is sampled, never what is addressed;
 *   6. all of kx_sample_logits' guarantees carry over: a row's outputs do not depend on B, on its row index or on execution
 *      order, and two calls give identical bits.  Finished rows and rows without a candidate behave as in kx_sample_logits.
 * Argument errors (KX_ERR_INVALID_ARG, nothing launched): a null rows, a stale struct_bytes, a null table, flags beyond the two
 * bits, a negative advance; then kx_sample_logits' own.  Never allocates, never synchronises. */
typedef struct {
  int32_t do_sample;                          /* 0: greedy */
  float temperature;                          /* >= 0; 0: greedy */
  int32_t top_k;                              /* outside (0, V): off */
  float top_p;                                /* > 0; >= 1: off */
  float repetition_penalty;                   /* > 0; 1: off */
  float min_p;                                /* [0, 1], 0 = off */
  float log_min_p;                            /* filled by kx_sample_rows_pack */
  float typical_p;                            /* (0, 1], 1 = off */
  float epsilon_cutoff;                       /* [0, 1), 0 = off */
  float eta_cutoff;                           /* [0, 1), 0 = off */
  int32_t max_new;                            /* the row's token budget, 0 = none */
  int32_t reserved;
  uint64_t seed;                              /* the row's Philox key */
} kx_sample_row;
#define KX_SAMPLE_ROWS_PENALTY 1u
#define KX_SAMPLE_ROWS_BUDGET 2u
typedef struct {
  uint32_t struct_bytes;                      /* = sizeof(kx_sample_rows_args) of the caller ("stale binding" otherwise) */
  uint32_t flags;                             /* kx_sample_rows_pack's flags_out */
  const kx_sample_row* table;                 /* [B], device memory */
} kx_sample_rows_args;
int kx_sample_rows_pack(const kx_sample_row* in, int64_t B, int64_t V, kx_sample_row* out, uint32_t* flags_out);
int kx_sample_logits_rows(const kx_sample_args* args, int32_t* positions, int64_t advance, const kx_sample_rows_args* rows, void* stream);

/* kx_shape_logits_rows: kx_shape_logits with row b's penalties read from two device fp32 [B] arrays: f = frequency_rows[b] and
 * p = presence_rows[b] in the same three single fp32 operations (its rule 4), never contracted.  Either array may be NULL: the
 * scalar of args for every row; with both NULL it IS kx_shape_logits(args, stream).  counts is required when an array is given
 * (KX_ERR_INVALID_ARG naming counts); the values of an array are used in arithmetic only — the caller passes finite ones, as it
 * passes finite scalars.  Nothing else about the launch, its ownership rules or its limits changes. */
int kx_shape_logits_rows(const kx_shape_args* args, const float* frequency_rows, const float* presence_rows, void* stream);

/* ------------------------------------------------------------------------------------------
 * Contrastive search on the device (added within ABI 7: six functions are appended; no struct, no existing layout moves and the
 * kx_struct_id list is unchanged, so kx_version() stays 7 and KX_STRUCT_COUNT 13).
 *
 * A step of contrastive search takes the k <= 16 most likely next tokens of each of B sequences, runs them as M = B * k rows of
 * kx_decoder_decode_step_prefix (prefix = the sequence so far, prefix_seq[r] = r / k, prefix_len == positions == P_b repeated k times,
 * tail caches [L, M, heads, 1, 64]) and keeps, per sequence, the candidate j with the largest
 *     score_j = one_minus_alpha * p_j - alpha * max over i < P_b of dot(u_j, history[b, i]),
 * u being unit vectors of the hidden states.  Row b * k + j is candidate j of sequence b everywhere below.
 *
 * kx_contrast_candidates: sequence b's current logits row is row b * k_prev + chosen[b] of logits [rows, V] (row pitch ld), or row b
 *   with chosen == NULL (k_prev = 1): addressed, not copied.  One launch writes its k ids of largest value, the lowest id first among
 *   equal values — bit for bit the top_id of kx_step_logprobs with top_n = k, whose device code it shares — to step_tokens[b * k + j]
 *   (the next step's tokens), prob[b * k + j] = expf(that launch's top_logprob) and, when cand_id / cand_prob are given, the same to
 *   slot ((b * out_ld + out_col) * k + j) of both.  A sequence with finished[b] != 0 (finished may be NULL), or whose chosen[b] is
 *   outside [0, k_prev), writes nothing (kx_kv_cache_commit reports the latter).  Host checks: null pointers, k outside 1..16 or above
 *   V, k_prev outside 1..16, rows < B * k_prev, ld < V, out_col outside [0, out_ld).
 * kx_contrast_hidden: out row = u = h / ||h||_2 in fp32, h = decoder.layer_norm (w->ln_g, w->ln_b, w->eps) of a row of the final
 *   residual stream — what the output projection multiplies.  step != 0: x [B, dim] is the x of a decode step of B rows (T == 1) that
 *   has just run with `workspace` and `prec`; the residual is x alone, or x + xb of the workspace where that step ran its
 *   two-workgroup residual form — decided by the very helper the step asks, from w, B, prec and the tuning keys.  step == 0:
 *   x [B, T, dim] holds rows as they are (kx_decoder_prefill leaves the final residual in its x), workspace and prec are unused.
 *   Row (b, t) goes to out + b * out_ld + t * dim (out_ld in floats, >= T * dim); with lengths (int32 [B], device) rows t >=
 *   lengths[b] are not written.  residual_out (optional, fp32 [B * T, dim]): the rows v the kernel normalised, x or the summed pair,
 *   for a caller that wants to restate the result.  The arithmetic, every operation a single fp32 one: v_i = x_i + xb_i (the pair only);
 *   mean = (sum v_i) / dim; c_i = v_i - mean; var = (sum c_i * c_i) / dim; r = 1 / sqrtf(var + eps); h_i = (c_i * r) * g_i + b_i
 *   (two products and one sum, not contracted); n = sqrtf(sum h_i * h_i); u_i = h_i / n.  Each sum: 256 threads over elements
 *   tid, tid + 256, ... in ascending order, a butterfly over the 64 lanes, then (w0 + w1) + (w2 + w3) — a function of dim alone.
 * kx_contrast_select: u [B * k, D] (kx_contrast_hidden's rows), prob [B * k], history [B, cap, D] fp32, P_b = hist_rows[b * p_stride]
 *   (int32, device).  Two launches.  The first splits the history along i, CS = 32 rows per workgroup, grid (ceil(cap / 32), B):
 *   a workgroup stages its sequence's k candidate vectors once (k * D * 4 <= 128 KB of LDS), reads the history 16 bytes per lane and
 *   writes k partial maxima to scratch (kx_contrast_scratch_bytes(B, k, cap) bytes).  Every dot product is summed in one order that
 *   depends on D alone: lane l takes the 4-element vectors l, l + 64, ... ascending with acc = fma(h3, c3, fma(h2, c2, fma(h1, c1,
 *   fma(h0, c0, acc)))), then a butterfly over the 64 lanes (xor 32 .. 1) — the chunking, the grid, B, k and the place of a row or a
 *   candidate do not enter, and the maximum over i is exact in any order.  No workgroup waits on another; no atomics on floats.  The
 *   second, one workgroup per sequence, takes penalty_j = the maximum of the partial maxima, score_j = (one_minus_alpha * p_j) -
 *   (alpha * penalty_j) as two products and one difference each rounded once (one_minus_alpha is the caller's fp32), chooses the
 *   largest score, the lowest j among equal ones, a NaN score losing to every number, and writes next_token[b] = step_tokens[b * k + j],
 *   chosen[b] = j, history[b, P_b] = u[b * k + j] (bitwise), hist_len[b] = P_b + 1, finished[b] = 1 when the token is eos_id (eos_id
 *   < 0: none) and, where given, out_tokens[b * out_ld + out_col], chosen_trace[b * out_ld + out_col] and cand_penalty[(b * out_ld +
 *   out_col) * k + j'] for every j'.  A row that enters finished writes pad_id to next_token[b] and out_tokens and nothing else.  A row
 *   with P_b < 1 or P_b >= cap writes nothing and ORs KX_RAGGED_ERR_CACHE into *error_word.  Host checks: null pointers, k outside
 *   1..16, B outside 1..65535, D % 4, k * D * 4 > 128 KB, cap < 2, alpha or one_minus_alpha outside [0, 1], out_col outside
 *   [0, out_ld), u / history not 16-byte aligned or overlapping, scratch_bytes too small.
 * kx_kv_cache_commit: for every layer and head, tail row 0 of row b * k + chosen[b] of the tail caches [L, B * k, heads, Ttail, 64]
 *   goes to row P_b = positions[b * k] of sequence b of the caches [L, B, heads, Tmax, 64], k and v, 16 bytes per thread; then
 *   positions[b * k .. b * k + k - 1] = P_b + 1.  Both cache dtypes (elem_bytes 2 or 4) and both layouts (tuning key 9, applied to the
 *   caches and the tails).  A row with finished[b] != 0 (finished may be NULL) is skipped.  chosen[b] outside [0, k) or P_b outside
 *   [0, Tmax) writes nothing, leaves the positions and ORs KX_RAGGED_ERR_COMMIT into the sticky *error_word.  Host checks as for
 *   kx_kv_cache_gather: null pointers, elem_bytes, shape ranges, k outside 1..16, 16-byte alignment, overlap of tails and caches.
 * None of them allocates or synchronises.
 * ------------------------------------------------------------------------------------------ */
int kx_contrast_candidates(const float* logits, int64_t ld, int64_t rows, int64_t B, int64_t V, int32_t k, const int32_t* chosen,
                           int64_t k_prev, const uint8_t* finished, int64_t* step_tokens, float* prob, int64_t* cand_id,
                           float* cand_prob, int64_t out_ld, int64_t out_col, void* stream);
int kx_contrast_hidden(const kx_decoder_weights* w, const float* x, void* workspace, int64_t B, int64_t T, int32_t prec, int32_t step,
                       const int32_t* lengths, float* out, int64_t out_ld, float* residual_out, void* stream);
size_t kx_contrast_scratch_bytes(int64_t B, int32_t k, int64_t cap);
int kx_contrast_select(const float* u, const float* prob, float* history, int64_t B, int32_t k, int64_t D, int64_t cap,
                       const int32_t* hist_rows, int64_t p_stride, int32_t* hist_len, float alpha, float one_minus_alpha,
                       const int64_t* step_tokens, uint8_t* finished, int64_t eos_id, int64_t pad_id, int64_t* next_token,
                       int32_t* chosen, int64_t* out_tokens, int64_t out_ld, int64_t out_col, float* cand_penalty,
                       int32_t* chosen_trace, float* scratch, size_t scratch_bytes, int32_t* error_word, void* stream);
int kx_kv_cache_commit(const void* ktail, const void* vtail, void* kcache, void* vcache, int64_t L, int64_t B, int32_t k,
                       int64_t heads, int64_t Tmax, int64_t Ttail, int32_t elem_bytes, const int32_t* chosen, int32_t* positions,
                       const uint8_t* finished, int32_t* error_word, void* stream);

/* ------------------------------------------------------------------------------------------
 * In-process kernel timing (bench.py's roofline leg; the reference's own ad-hoc equivalents are the
 * wall-clock fences of /root/reference/tests/test_benchmarking.py:68-95,192-196).
 * When enabled, every kernel launch made through this library is bracketed by hipEventRecord on
 * the launch stream.  kx_prof_collect synchronises the recorded events and returns one record
 * per launch, in launch order.  Not for use under hipGraph capture.
 * ---------------------------------------------------------------------------------------- */
typedef enum {
  KX_K_GEMM_BF16_128 = 0, KX_K_GEMM_BF16_64 = 1, KX_K_GEMM_F32_128 = 2, KX_K_GEMM_F32_64 = 3,
  KX_K_LAYERNORM = 4, KX_K_ATTN_BF16 = 5, KX_K_ATTN_F32 = 6, KX_K_EMBED = 7, KX_K_MISC = 8,
  KX_K_GEMM_BF16_160 = 9, KX_K_GEMM_BF16_256X128 = 10, KX_K_GEMM_BF16_256X256 = 11,
  /* the same tile kernels on KX_PREC_F16C rows (fp16 MFMA + two fp8 correction MFMAs: 2x the matrix time per algorithmic
   * flop) and on plain KX_PREC_F16 rows — named for what they multiply, so a reader of a kernel table never sees an f16c
   * kernel under a bf16 label (round 4) */
  KX_K_GEMM_F16C_128 = 12, KX_K_GEMM_F16C_64 = 13, KX_K_GEMM_F16C_160 = 14, KX_K_GEMM_F16C_256X128 = 15,
  KX_K_GEMM_F16C_256X256 = 16,
  KX_K_GEMM_F16_128 = 17, KX_K_GEMM_F16_64 = 18, KX_K_GEMM_F16_160 = 19, KX_K_GEMM_F16_256X128 = 20,
  KX_K_GEMM_F16_256X256 = 21,
  KX_K_ATTN_F16 = 22,      /* the v2 flash kernel on fp16 MFMAs (KX_PREC_F16) */
  KX_K_ATTN_F16S = 23      /* split-fp16 (hi, lo) flash kernel of KX_PREC_F16C: three MFMAs per product */
} kx_kernel_kind;
typedef struct {
  int32_t kind;      /* kx_kernel_kind */
  int32_t reserved;
  int64_t a, b, c;   /* GEMM: M,N,K.  LayerNorm: rows, cols, HBM bytes per value (fp32 in + pre_add + the output format's
                        bytes; 0 / 1: not reported).  Attention: B*H, Tq, Tk.  else rows, cols, 0 */
  float ms;          /* device time of the launch */
  float reserved2;
} kx_prof_record;
int kx_prof_enable(int on);                               /* on != 0: clear records and start recording */
int kx_prof_collect(kx_prof_record* out, int max_records); /* returns the number of records written */

#ifdef __cplusplus
}
#endif
#endif /* KOSMOSX_HIP_H */
