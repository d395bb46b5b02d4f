// The launch plan of kx_gemm: every host-side decision of one call — argument checks, epilogue class, tile, pair split /
// split-K, the exact kernel instantiation of each launch — as ONE pure function of (kx_gemm_args, a snapshot of the tuning
// table, the CU count).  No HIP call, no global state, no operand pointer is dereferenced: a plain host compiler builds this
// header, kx_gemm_describe prints its result, and tests pin it on a machine without a GPU.  kx_gemm itself is
// snapshot -> plan -> copy into GemmParams -> execute (kx_gemm.hip).
#pragma once
#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "../../include/kosmosx_hip.h"

// ---- runtime tuning knobs (kx_set_tuning) ----
enum { KX_TUNE_LN_VARIANT = 0, KX_TUNE_GEMM_TILE = 1, KX_TUNE_ATTN_VARIANT = 2, KX_TUNE_GEMM_STAGGER = 3, KX_TUNE_GEMM_EPILOGUE = 4, KX_TUNE_GEMM_IDLE_SKIP = 5, KX_TUNE_PREPROCESS_NO_LDS = 6, KX_TUNE_GEMM_PERSISTENT = 7, KX_TUNE_GEMV_VARIANT = 8, KX_TUNE_CACHE_LAYOUT = 9, KX_TUNE_DECODE_STREAM_F32 = 10, KX_TUNE_DECODE_KSPLIT = 11, KX_TUNE_DECODE_PIECES = 12, KX_TUNE_GEMM_PAIRK = 13, KX_TUNE_GEMM_KLOOP = 14, KX_TUNE_GEMM_RULES = 15, KX_TUNE_F16C_CORR = 16, KX_TUNE_SPLITK_COOP = 17, KX_TUNE_OBJECTIVE = 18, KX_TUNE_COUNT = 19 };
// A by-value snapshot of the tuning table.  kx_gemm takes one on entry and everything below it reads the snapshot, never the
// global table: a kx_set_tuning from another thread cannot give one call an inconsistent plan.
struct KxTuning { int v[KX_TUNE_COUNT]; };

#define KX_ACT_GELU_FAST 3  /* internal: chosen by kx_gemm for KX_ACT_GELU when prec == bf16 */
#define KX_ACT_GELU_POLY 4  /* internal: gemm_kernel_p5's lean epilogues, bf16 operands and bf16 output (see kx_common.h) */

// kernel family of the main launch, and the element type its template is instantiated with
enum { KX_FAM_TILE = 0 /* gemm_kernel */, KX_FAM_P3 = 1 /* gemm_kernel_p3 */, KX_FAM_P5 = 2 /* gemm_kernel_p5 */, KX_FAM_TILE16 = 3 /* weight streaming */ };
enum { KX_ELEM_BF16 = 0, KX_ELEM_F16C = 1 /* KX_PREC_F16C and plain KX_PREC_F16 rows */, KX_ELEM_F32 = 2 };
enum { KX_REDUCE_NONE = 0, KX_REDUCE_PLAIN = 1 /* splitk_reduce_kernel */, KX_REDUCE_ROWS = 2 /* splitk_reduce_rows_kernel */ };

struct KxGemmPlan {
  int tile;                 // resolved: 16 / 64 / 128 / 160 / 256 / 257 / 384 / 512
  int kind;                 // profile kind (KX_K_GEMM_*)
  // launch 0 (optional): kx_row_stats_finalize of the producer's partials into row_stats_scratch.  fin_in_launch: the pair
  // split finalises them itself instead (tuning key 15 & 32) and the call keeps its stats_partials.
  int fin_first, fin_in_launch;
  // launch 1: the main kernel
  int family, elem, BM, BN, ACT, EPI, NST, KS2, BAL, COOP, PHASED;
  unsigned grid_x, grid_y, block;   // (no dynamic LDS: the tile kernels keep theirs static, tile 16 sizes its own in the launcher)
  // launch 2 (optional): the split-K reduce
  int reduce, reduce_act, reduce_nj;
  unsigned reduce_grid;
  // every host-computed scalar of GemmParams (same names; the pointers come from the arguments)
  long long lda_b, ldw_b;
  int c_bf16, c_x3, c_f16, c_f16c, c_hilo, c_pieces;
  int nk_main, kskip, K, act;
  int tiles_m, tiles_n;
  int vec_ok, vec8_ok, vec2_ok;
  int stats_nseg, splitk, stagger_ticks;
  int fast_epilogue, lean_epilogue, lean_xpos, lean_res, lean_f16c;
  int w_tiled, ring, gelu_poly, persistent, skip_idle_waves, bal;
  int pairk, pk_fault; unsigned pk_spin_ticks;
  int coop;
  int gsplit, kfull, no_rowreg, a_pieces;
  int take_ln_g, take_stats_partials, take_pair_extras;   // which optional argument groups GemmParams takes (tile 16 / row reduce)
  char msg[640];            // refusal text (moves into kx_set_error)
};

namespace kx_plan_detail {

inline int refuse(KxGemmPlan* pl, int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(pl->msg, sizeof(pl->msg), fmt, ap);
  va_end(ap);
  return code;
}
#define KXP_REQUIRE(cond, ...) \
  do { if (!(cond)) return kx_plan_detail::refuse(pl, KX_ERR_INVALID_ARG, __VA_ARGS__); } while (0)
#define KXP_TRY(expr) \
  do { const int rc__ = (expr); if (rc__ != KX_OK) return rc__; } while (0)

inline long long cdiv(long long x, long long y) { return (x + y - 1) / y; }

// what the phases hand to each other besides the plan
struct Ctx {
  const kx_gemm_args* a;     // the call, seen as a row_stats call when it came with row_stats_scratch (see validate_stats_form)
  kx_gemm_args a_copy;
  const KxTuning* tn;
  int cus;
  bool f16c, f16; int es, bk;
  int64_t fin_nseg;
  int t(int key) const { return tn->v[key]; }
};

}  // namespace kx_plan_detail

// K slices for a 64x64-tile launch: ~512 workgroups streaming the weights, at most 16 slices, at least two K-tiles per
// slice, partials [slices, M, N] fp32 within the scratch.  `forced` > 0 overrides the count (tests), < 0 is a minimum.
inline long long kx_splitk_slices(const KxTuning& tn, int64_t M, int64_t N, int64_t K, int bk, size_t ws_bytes, int forced, bool f16c_rows = false) {
  const long long tiles = ((M + 63) / 64) * ((N + 63) / 64);
  const long long nk_all = K / bk;
  // the ring kernel keeps 64 KB of LDS per workgroup = two workgroups per CU = 512 resident: never more slices than fit in
  // ONE round (a 640-workgroup grid ran 1.25 rounds = twice the time); A/B: tuning key 4 = 6 restores the r1 rule
  // (KX_F16C rows keep the r1 rule and the two-stage kernel: twice the K-tiles per slice, measured 7 % slower on the ring)
  const bool ring = tn.v[KX_TUNE_GEMM_EPILOGUE] != 6 && !f16c_rows;
  long long sp = forced > 0 ? forced : ring ? (tiles >= 256 ? 1 : 512 / tiles) : (tiles >= 384 ? 1 : (512 + tiles - 1) / tiles);
  if (forced < 0 && sp < -forced) sp = -forced;   // callers whose epilogue lives in the reduce kernel (statistics producer)
  if (sp > 16) sp = 16;
  if (sp > nk_all / 2) sp = nk_all / 2;
  while (sp > 1 && (size_t)sp * M * N * 4 > ws_bytes) --sp;
  if (sp > 1) {
    const long long kchunk = (nk_all + sp - 1) / sp;
    sp = (nk_all + kchunk - 1) / kchunk;          // no empty slices
  }
  return sp < 1 ? 1 : sp;
}

// number of K slices the automatic choice gives an (M, N, K) problem with `ws_bytes` of split-K scratch (1 = no split): the
// rule the planner applies, for callers that must know before they ask for the row-owning reduce
inline int kx_gemm_auto_splits_with(const KxTuning& tn, int64_t M, int64_t N, int64_t K, int prec, size_t ws_bytes) {
  using kx_plan_detail::cdiv;
  if (!ws_bytes || cdiv(M, 128) * cdiv(N, 128) >= 192) return 1;       // the automatic tile choice is not 64x64
  if (prec == KX_PREC_F16C) return (int)kx_splitk_slices(tn, M, N, 2 * K, 64, ws_bytes, 0, true);   // 4K-byte rows = 2K 2-byte units
  return (int)kx_splitk_slices(tn, M, N, K, (prec == KX_PREC_BF16 || prec == KX_PREC_F16) ? 64 : 32, ws_bytes, 0);
}

namespace kx_plan_detail {

// ---- phase 1: the argument checks that do not depend on the tile, and the scalars read off the arguments ----
// row_stats_scratch AND stats_partials (tile kernels; ABI 7): the partials are what the producer wrote, the scratch is where
// their finalised (mean, rstd) go when this launch does not finalise them itself: kx_gemm runs kx_row_stats_finalize first.  The pair split
// with the lean residual epilogue CAN finalise them in the launch (each workgroup the 128 rows it finishes, while it waits for
// its partner's flag: kx_row_stats_finalize's arithmetic, wave per row; row_stats untouched) — opt-in, tuning key 15 & 32:
// measured SLOWER on the headline (25.14 vs 24.90 ms same-box alternating: with two steps in flight the 5 us finalize launches
// hide under the other stream, the in-launch walk sits on the hand-off).  Below this point the call looks like a row_stats
// call; the plan remembers that the partials are to be finalised (fin_first / fin_in_launch).
inline int validate_stats_form(Ctx& c, const kx_gemm_args* a_in, KxGemmPlan* pl) {
  c.a = a_in;
  c.fin_nseg = 0;
  KXP_REQUIRE(!(a_in->row_stats && a_in->stats_partials && a_in->tile != 16),
              "kx_gemm: row_stats together with stats_partials was the ABI 6 form; ABI 7 takes the output scratch as row_stats_scratch");
  KXP_REQUIRE(!a_in->row_stats_scratch || (a_in->stats_partials && !a_in->row_stats && a_in->tile != 16),
              "kx_gemm: row_stats_scratch goes with stats_partials on the tile kernels (row_stats NULL)");
  if (a_in->row_stats_scratch) {
    KXP_REQUIRE(a_in->stats_in_nseg > 0 && a_in->stats_in_seg > 0 && !a_in->ln_out,
                "kx_gemm: row_stats_scratch + stats_partials needs nseg, seg size (and no ln_out: that is the row-owning reduce's form)");
    pl->fin_first = 1;
    c.fin_nseg = a_in->stats_in_nseg;
    c.a_copy = *a_in; c.a_copy.stats_partials = nullptr; c.a_copy.stats_in_nseg = 0; c.a_copy.stats_in_seg = 0;
    c.a_copy.row_stats = a_in->row_stats_scratch; c.a_copy.row_stats_scratch = nullptr;     // below this point: a row_stats call
    c.a = &c.a_copy;
  }
  return KX_OK;
}

inline int validate(Ctx& c, KxGemmPlan* pl) {
  const kx_gemm_args* a = c.a;
  KXP_REQUIRE(a->A && a->W && a->C, "kx_gemm: null operand pointer");
  KXP_REQUIRE(a->M > 0 && a->N > 0 && a->K > 0, "kx_gemm: empty problem M=%lld N=%lld K=%lld", (long long)a->M,
              (long long)a->N, (long long)a->K);
  KXP_REQUIRE(a->M < (1ll << 31) && a->N < (1ll << 31) && a->K < (1ll << 31), "kx_gemm: dimension overflow");
  const bool f16c = c.f16c = a->prec == KX_PREC_F16C;
  const bool f16 = c.f16 = a->prec == KX_PREC_F16;                    // plain fp16 rows on the KX_F16C kernels, no correction tiles
  const int es = c.es = (a->prec == KX_PREC_BF16 || f16c || f16) ? 2 : 4;   // KX_F16C rows: lda/ldw/ldc count 2-byte units
  const int bk = c.bk = f16c ? 128 : 128 / es;
  KXP_REQUIRE(a->prec == KX_PREC_BF16 || a->prec == KX_PREC_F32 || f16c || f16, "kx_gemm: bad precision %d", a->prec);
  KXP_REQUIRE(!f16 || (a->tile != 16 && a->tile != 257), "kx_gemm: KX_PREC_F16 runs the tile kernels 64/128/160/256/384/512");
  KXP_REQUIRE(a->cdt != KX_F16 || f16 || f16c, "kx_gemm: KX_F16 outputs come from the fp16 kernels (KX_PREC_F16 / KX_PREC_F16C)");
  KXP_REQUIRE(a->cdt != KX_BF16 || !f16, "kx_gemm: KX_PREC_F16 writes KX_F16 or fp32");
  KXP_REQUIRE(a->K % bk == 0, "kx_gemm: K=%lld must be a multiple of %d", (long long)a->K, bk);
  KXP_REQUIRE(!f16c || (a->w_scale && a->lda >= 2 * a->K && a->ldw >= 2 * a->K && a->tile != 16 && a->tile != 257),
              "kx_gemm: KX_PREC_F16C needs w_scale, lda/ldw >= 2K (2-byte units) and a tile kernel (not 16 / 257)");
  KXP_REQUIRE((a->lda * es) % 16 == 0 && (a->ldw * es) % 16 == 0, "kx_gemm: lda/ldw must give 16-byte row pitch");
  KXP_REQUIRE(((uintptr_t)a->A & 15) == 0 && ((uintptr_t)a->W & 15) == 0, "kx_gemm: A/W must be 16-byte aligned");
  KXP_REQUIRE(a->lda >= a->K && a->ldw >= a->K && a->ldc >= a->N, "kx_gemm: leading dimension too small");
  KXP_REQUIRE(a->qcols % 4 == 0, "kx_gemm: qcols must be a multiple of 4");
  if (a->xpos_dim) {
    KXP_REQUIRE(a->xq_cs && a->xq_ss && a->xk_cs && a->xk_ss && a->xpos_T > 0, "kx_gemm: xpos tables missing");
    KXP_REQUIRE(a->xpos_dim % 64 == 0 && 2 * a->xpos_dim <= a->N, "kx_gemm: xpos_dim must be heads*64 and <= N/2");
  }
  pl->lda_b = a->lda * es; pl->ldw_b = a->ldw * es;
  pl->c_bf16 = a->cdt == KX_BF16 || a->cdt == KX_BF16X3 || a->cdt == KX_F16C || a->cdt == KX_F16;
  pl->c_x3 = a->cdt == KX_BF16X3; pl->c_f16c = a->cdt == KX_F16C; pl->c_f16 = a->cdt == KX_F16;
  pl->c_pieces = a->cdt == KX_F16P;
  pl->c_hilo = a->cdt == KX_F16HL;
  KXP_REQUIRE(!pl->c_hilo || (f16c && a->xpos_dim > 0 && a->N % 64 == 0 && a->ldc % 4 == 0 && ((uintptr_t)a->C & 15) == 0 &&
                              !a->residual && !a->stats_out && !a->row_stats && a->act == KX_ACT_NONE && a->tile != 16 &&
                              !a->ln_operand_out && c.t(KX_TUNE_GEMM_EPILOGUE) != 1),
              "kx_gemm: a KX_F16HL output comes from KX_PREC_F16C operands with the XPos epilogue (the prefetching store loop), "
              "N %% 64 == 0, 16-byte aligned fp32-pitched rows, no residual / statistics / activation");
  KXP_REQUIRE(a->cdt != KX_F16P || (a->tile == 16 && a->prec == KX_PREC_F32 && a->N % 32 == 0 && a->ldc % 32 == 0 &&
                                    ((uintptr_t)a->C & 15) == 0 && !a->residual && a->ksplit <= 1),
              "kx_gemm: KX_F16P rows come from tile 16 on fp32 operands, N %% 32 == 0, ldc %% 32 == 0, no residual / ksplit");
  pl->nk_main = f16c ? (int)(a->K / 64) : 0x7fffffff; pl->kskip = 0;
  KXP_REQUIRE(a->f16c_corr >= KX_CORR_BOTH && a->f16c_corr <= KX_CORR_NONE && (f16c || a->f16c_corr == KX_CORR_BOTH),
              "kx_gemm: f16c_corr is a kx_f16c_corr value and belongs to KX_PREC_F16C operands");
  KXP_REQUIRE(a->cdt != KX_F16C || (a->N % 8 == 0 && a->ldc >= 2 * a->N && a->ldc % 8 == 0 && a->tile != 16 &&
                                     ((uintptr_t)a->C & 15) == 0),
              "kx_gemm: a KX_F16C output needs N %% 8 == 0, ldc >= 2N (2-byte units), ldc %% 8 == 0 (and is not offered by tile 16)");
  KXP_REQUIRE(a->cdt != KX_BF16X3 || (a->N % 8 == 0 && a->ldc >= 3 * a->N && a->ldc % 8 == 0 && a->tile != 16 &&
                                       ((uintptr_t)a->C & 15) == 0),
              "kx_gemm: a KX_BF16X3 output needs N %% 8 == 0, ldc >= 3N, ldc %% 8 == 0 (and is not offered by tile 16)");
  pl->K = (int)(f16c ? 2 * a->K : a->K);   // f16c: 2-byte units of the 4K-byte row
  if (f16c && a->f16c_corr != KX_CORR_BOTH) {
    // one correction product (K / 128 fp8 tiles after the K / 64 fp16 tiles) or none: the loop is shorter, the rows are not
    pl->K = (int)(a->f16c_corr == KX_CORR_NONE ? a->K : a->K + a->K / 2);
    if (a->f16c_corr == KX_CORR_ACT) pl->kskip = (int)(a->K / 128);            // ... and its fp8 tiles are the rows' second region
  }
  pl->act = (a->act == KX_ACT_GELU && (a->prec == KX_PREC_BF16 || f16c || f16)) ? KX_ACT_GELU_FAST : a->act;
  pl->stats_nseg = (int)(a->N / 64);
  KXP_REQUIRE((!a->row_stats && !a->stats_partials) == !a->colsum, "kx_gemm: row_stats and colsum must be given together");
  KXP_REQUIRE(!a->colsum || ((uintptr_t)a->colsum & 15) == 0, "kx_gemm: colsum must be 16-byte aligned");
  KXP_REQUIRE(!a->stats_out || a->stats_out_seg == 16 || a->N % 64 == 0, "kx_gemm: stats_out needs N %% 64 == 0 (N=%lld)",
              (long long)a->N);
  KXP_REQUIRE(!a->stats_out || (a->qcols == 0 && a->xpos_dim == 0),
              "kx_gemm: stats_out combines with the folded-LN consume, bias and activation only");
  KXP_REQUIRE(!a->stats_out || !a->residual, "kx_gemm: stats_out is taken before the residual add; pass one of them");
  pl->vec_ok = (a->ldc % 4 == 0) && (!a->residual || a->ldr % 4 == 0) &&
               (((uintptr_t)a->C & 15) == 0) && (!a->residual || ((uintptr_t)a->residual & 15) == 0);
  pl->vec8_ok = pl->vec_ok && (a->ldc % 8 == 0) && (a->N % 8 == 0);
  pl->vec2_ok = a->cdt == KX_F32 && (a->ldc % 2 == 0) && (((uintptr_t)a->C & 7) == 0);
  KXP_REQUIRE(!a->bias || ((uintptr_t)a->bias & 15) == 0, "kx_gemm: bias must be 16-byte aligned");
  pl->splitk = 1;
  KXP_REQUIRE(!a->ln_operand_out == !a->ln_operand_stats, "kx_gemm: ln_operand_out and ln_operand_stats go together");
  KXP_REQUIRE(!a->ln_operand_out ||
                  (a->residual && a->cdt == KX_F32 && a->N % 64 == 0 && pl->vec_ok && !a->stats_out && !a->ln_out &&
                   (a->ln_operand_dt == KX_BF16 || a->ln_operand_dt == KX_F16 || a->ln_operand_dt == KX_F16C) &&
                   ((uintptr_t)a->ln_operand_out & 15) == 0 && c.t(KX_TUNE_GEMM_EPILOGUE) != 1),
              "kx_gemm: ln_operand_out needs an fp32 output with residual, N %% 64 == 0, aligned rows, a 2-byte / KX_F16C "
              "operand dtype and the prefetching store loop");
  pl->pk_spin_ticks = 100000000u;
  pl->gsplit = 1; pl->kfull = pl->K;
  pl->no_rowreg = c.t(KX_TUNE_GEMV_VARIANT) == 3;
  return KX_OK;
}

// ---- phase 2: the epilogue class (which store loop / accumulator-level epilogue the call is eligible for) ----
inline void epilogue_class(const Ctx& c, KxGemmPlan* pl) {
  const kx_gemm_args* a = c.a;
  const bool f16c = c.f16c, f16 = c.f16;
  // The prefetching store loop pays where the epilogue has per-row global operands to wait for (residual, folded-LN
  // statistics, XPos tables); bias-only bf16 epilogues measured ~5 % faster on the plain rolled loop.
  const int mode = c.t(KX_TUNE_GEMM_EPILOGUE);   // 0 auto, 1 never, 2 always (A/B)
  pl->skip_idle_waves = c.t(KX_TUNE_GEMM_IDLE_SKIP) != 1;   // A/B: 1 = off
  // K loop of the 256-column kernel (tuning key 14: 0 = balanced, 1 = the first form, A/B).  tools/kloop_bench.py,
  // profiles/r05_c_kloop_bench.jsonl: +5...13 % on every shape of the forward at K >= 2048 (f16c, bf16, fp16), +3...7 % at
  // K = 1024, bit-identical
  pl->bal = c.t(KX_TUNE_GEMM_KLOOP) != 1;
  {   // one persistent workgroup per CU unless told otherwise (key 7: -1 = one workgroup per tile, n > 0 = n workgroups)
    const int pv = c.t(KX_TUNE_GEMM_PERSISTENT);
    pl->persistent = pv < 0 ? 0 : pv > 0 ? pv : c.cus;
  }
  // the lean epilogue covers bf16 outputs (not bf16x3) without residual / folded-LN consume / XPos on
  // 16-byte-aligned rows; the 256-column kernel also asks for N % 256 == 0.  Everything else keeps the generic loops.
  pl->lean_epilogue = mode != 1 && pl->c_bf16 && !pl->c_x3 && !pl->c_f16c &&
                      ((f16 || f16c) ? pl->c_f16 : !pl->c_f16) && pl->vec8_ok && !a->residual &&
                      !a->row_stats && !a->xpos_dim && a->qcols % 64 == 0 && !(a->stats_out && a->qcols);
  // the decoder's qkv GEMM in bf16: bias + q-scale + XPos, no folded-LN consume / residual / statistics, whole heads per wave
  // A/B only (tuning key 4 = 3): measured SLOWER than the row-major store loop it was meant to replace — C3 qkv 36.5 ms
  // (1084 TFLOP/s) on the generic loop, 49.3 ms with the tables read from global in accumulator layout, 44.5 ms with
  // them staged through LDS (the 256-row variant pushes half of its rotated accumulators through scratch).
  // KX_F16C output (the decoder's fc1 in f16c / mixed) without residual / XPos / q-scale split inside a tile: the 256-column
  // kernel's three-plane lean store (tuning key 4 = 8: generic loops, A/B)
  pl->lean_f16c = mode != 1 && mode != 8 && pl->c_f16c && f16c &&
                  !a->residual && !a->xpos_dim && a->qcols % 64 == 0 && a->N % 16 == 0 && (a->ldc * 2) % 16 == 0 &&
                  !a->ln_operand_out;
  // bias + q-scale + XPos at accumulator level (tables through LDS) and a whole-row tile store: bf16 operands -> bf16
  // rows, f16c operands -> the fp32 q / k / v the split attention reads.  Eligible = 1 (taken on the 192-row
  // tiles), 2 = asked for on any tile (tuning key 4 = 3, A/B); tuning key 4 = 1 / 8 keep the generic loops.
  {
    const int k4 = mode;
    const bool shape_ok = a->xpos_dim > 0 && !a->residual && !a->row_stats && !a->stats_out && a->act == KX_ACT_NONE &&
                          a->qcols % 256 == 0 && a->xpos_dim % 256 == 0 && !a->ln_operand_out;
    const bool bf = a->prec == KX_PREC_BF16 && a->cdt == KX_BF16 && pl->vec8_ok;
    const bool fc = f16c && (a->cdt == KX_F32 || a->cdt == KX_F16HL) && pl->vec_ok && a->N % 4 == 0;
    pl->lean_xpos = (shape_ok && (bf || fc) && k4 != 1 && k4 != 8 && k4 != 9) ? ((k4 == 3 && bf) ? 2 : 1) : 0;   // (9: only this one off, A/B)
  }
  // fp32 output with residual on whole 256-column tiles (the decoder's out_proj / fc2; pair split or not): bias + folded-LN
  // consume at accumulator level, residual rows requested before the tile is parked (tuning key 15 & 16: generic loops, A/B)
  pl->lean_res = mode != 1 && !(c.t(KX_TUNE_GEMM_RULES) & 16) && a->cdt == KX_F32 && a->residual && pl->vec_ok &&
                 a->act == KX_ACT_NONE && !a->xpos_dim && !a->stats_out && !a->ln_operand_out && a->qcols % 64 == 0 &&
                 a->N % 256 == 0 && !a->ln_out;
  pl->ring = mode != 6 && !f16c;
  // A/B: tuning key 4 = 4 keeps the A&S erf in the lean epilogues
  // For plain fp16 rows out of plain fp16 operands (the tower in mixed mode) it is OPT-IN (tuning key 15 & 8): measured +0.6 %
  // on the headline step (1268 -> 1275 samples/s alternating, all model-level parity tests green), but the polynomial's 5.5e-5
  // is a ninth of fp16's rounding step at 1.0 and flips 23 % of the roundings, which breaks the kernel-level contract
  // "fp16 output == rounded fp32 output" (tests/test_f16c_gpu.py::test_gemm_f16_plain) — not worth it
  pl->gelu_poly = mode != 4 && a->act == KX_ACT_GELU &&
                  ((a->prec == KX_PREC_BF16 && a->cdt == KX_BF16) ||
                   (f16 && a->cdt == KX_F16 && (c.t(KX_TUNE_GEMM_RULES) & 8)));
  pl->fast_epilogue = mode == 2 || (mode != 1 && (a->residual || a->row_stats || a->xpos_dim > 0));
}

// Pair split of the 256x256 kernel (kx_gemm_args.pair_ws): half a round of 256x256 tiles becomes a full round of
// (tile, K half) workgroups.  Measured on the decoder's N = 2048 GEMMs at M = 3648 (tools/gemm_bench.py, HISTORY §4.1).
inline bool pair_ok(const Ctx& c, const KxGemmPlan* pl, int tile) {
  const kx_gemm_args* a = c.a;
  if (!(a->prec == KX_PREC_BF16 || c.f16c || c.f16) || !a->pair_ws || ((uintptr_t)a->pair_ws & 255)) return false;
  const long long t = ((a->M + 255) / 256) * ((a->N + 255) / 256);
  const long long nkt = pl->K / (128 / c.es);
  const int cus = c.cus;
  // (automatic choice: >= 64 K-tiles — half a K extent of 16 tiles does not amortise the exchange: bf16 / fp16 K = 2048
  //  measured 0.93-0.95x, K = 8192 1.16x; f16c rows hold twice the K-tiles: K = 2048 1.11x, K = 8192 1.25x)
  return t % 8 == 0 && 2 * t <= cus && 2 * t >= (85 * cus) / 100 && nkt % 2 == 0 && nkt >= (tile == 1024 ? 8 : 64) && a->act == KX_ACT_NONE &&
         !a->stats_out && !a->ln_out && !a->stats_partials && a->pair_ws_bytes >= 4096 + (size_t)(2 * t) * 131072;
}

// ---- phase 3: the tile ----
// Kernel-variant choice (measured on MI355X with tools/gemm_bench.py and in situ with bench.py):
//   64x64    when 128x128 tiles would leave most of the 256 CUs idle (batch-1 shapes);
//   256x256 phased (one workgroup per CU, 128x64 per wave) when its grid fills the chip — C3, decoder fc1;
//   256x128 phased/pipelined (one workgroup per CU) when K is long enough to amortise its prologue and its grid
//            fills the chip evenly — the decoder's M = B*114 GEMMs;
//   160x128  when it removes a nearly empty trailing wave of 128x128 tiles — the ViT's M = B*257 = 64.25 x 128
//            GEMMs (520 tiles on 512 slots) — estimated with the cost model below;
//   128x128  otherwise.
inline int choose_tile(const Ctx& c, KxGemmPlan* pl) {
  const kx_gemm_args* a = c.a;
  const bool f16c = c.f16c, f16 = c.f16;
  const int es = c.es;
  const int rules = c.t(KX_TUNE_GEMM_RULES);
  int tile = a->tile;
  const bool rare_act = a->act == KX_ACT_RELU || a->act == KX_ACT_SWISH;    // see kx_act: the generic 128 x 128 kernel, unsplit
  KXP_REQUIRE(!rare_act || tile != 16, "kx_gemm: relu / swish are not offered by the weight-streaming kernel (tile 16)");
  KXP_REQUIRE(a->act == KX_ACT_NONE || a->act == KX_ACT_GELU || a->act == KX_ACT_QUICK_GELU || rare_act, "kx_gemm: unknown activation %d", a->act);
  if (rare_act) tile = 128;
  if (tile == 1024) {
    KXP_REQUIRE(pair_ok(c, pl, tile), "kx_gemm: tile 1024 (pair split of the 256x256 kernel) needs pair_ws, 16-bit operands, tiles %% 8 == 0 with "
                "0.85 CUs <= 2 tiles <= CUs, an even number of K-tiles, no activation / statistics (M=%lld N=%lld K=%lld)",
                (long long)a->M, (long long)a->N, (long long)a->K);
    pl->pairk = 1; tile = 512;
  } else if (tile == 0 && c.t(KX_TUNE_GEMM_PAIRK) != 1 && !(rules & 128) && pair_ok(c, pl, tile)) {
    pl->pairk = 1; tile = 512;
  } else if (tile == 0 && (rules & 128) && pair_ok(c, pl, tile)) {
    // A/B (tuning key 15 & 128, "CU-time" experiment of round 6): what the pair split would take runs as HALF a round of whole
    // 256 x 256 tiles instead — longer per launch, fewer CU-microseconds, the other CUs left to the second stream in flight
    tile = 512;
  }
  if (pl->pairk && c.t(KX_TUNE_GEMM_PAIRK) == 2) { pl->pk_fault = 1; pl->pk_spin_ticks = 200000u; }   // fault injection (tests): 2 ms
  if (tile == 0) {
    const long long t128 = cdiv(a->M, 128) * cdiv(a->N, 128);
    if (t128 < 192) {
      tile = 64;
    } else if (a->prec == KX_PREC_F32) {
      tile = 128;
    } else {
      const long long t256 = cdiv(a->M, 256) * cdiv(a->N, 128);
      const double eff256 = (double)t256 / (double)(cdiv(t256, 256) * 256);
      auto cost = [&](int bm) {  // tile-time units: full waves of 512 resident tiles, cheaper trailing wave if <= 1 tile/CU
        const long long t = cdiv(a->M, bm) * cdiv(a->N, 128);
        const long long full = t / 512, rem = t % 512;
        return bm * ((double)full + (rem == 0 ? 0.0 : (rem <= 256 ? 0.62 : 1.0)));
      };
      const long long t512 = cdiv(a->M, 256) * cdiv(a->N, 256);
      const double eff512 = (double)t512 / (double)(cdiv(t512, 256) * 256);
      // 256x256 (128x64 per wave) is the fastest main loop (1.37 vs 1.09 PFLOP/s at 8192^3: 512 vs 768 B of LDS
      // traffic per MFMA) but needs >= ~0.85 of a 256-CU wave of tiles to pay: C3-sized problems, decoder fc1
      if (a->K >= 1024 && eff512 >= 0.85) tile = 512;
      // ... and, for outputs that take its lean 16-bit tile store, already when the padded rounds cover <= 1.5x the problem:
      // the ViT's qkv / fc1 at M = 32 * 257 (396 / 528 tiles = 2 / 3 rounds, the third one 16 tiles of 32 live rows) measured
      // 63.7 / 95.4 us against 69.7 / 101.5 on the 160-row kernel in bf16 and 79 / 111 there in fp16 (tools/epi_probe.py)
      else if (!(rules & 1) && a->K >= 1024 && pl->lean_epilogue && !a->stats_out && a->N % 256 == 0 &&
               (double)(cdiv(t512, 256) * 256) * 65536.0 <= 1.5 * (double)a->M * (double)a->N) tile = 512;
      else if (a->K >= 2048 && eff256 >= 0.85 && a->N <= 16384) tile = 256;
      else tile = cost(160) <= cost(128) ? 160 : 128;
      // 192x256 (96x64 per wave, same kernel): M = 32*114 = 19 x 192 exactly, and the decoder qkv GEMM (N = 6144)
      // then needs 456 tiles = 2 rounds instead of 360 256x256 tiles (also 2 rounds, each 1/0.83 longer) or 720
      // 256x128 tiles (3 rounds).  Relative round times measured with tools/gemm_bench.py: 1.0 / 0.83 / 0.6.
      if ((tile == 512 || tile == 256) && a->K >= 1024) {
        const long long t384 = cdiv(a->M, 192) * cdiv(a->N, 256);
        const double c384 = 0.83 * (double)cdiv(t384, 256);
        const double cur = tile == 512 ? (double)cdiv(t512, 256) : 0.6 * (double)cdiv(t256, 256);
        if (c384 < 0.97 * cur) tile = 384;
      }
      // The ViT's residual GEMMs (fc2, out_proj: N = 1024, fp32 residual epilogue) at M = 32 * 257: 43 x 4 tiles of 192 x 256 on
      // the 256-column kernel measured 91.6 / 38.3 us against 101.4 / 40.2 on the 160-row kernel (fp16, tools/epi_probe.py tower)
      if (!(rules & 2) && tile == 160 && (f16 || f16c || a->prec == KX_PREC_BF16) && a->residual &&
          a->N % 256 == 0 && a->K >= 1024 && cdiv(a->M, 192) * cdiv(a->N, 256) <= c.cus &&
          cdiv(a->M, 192) * cdiv(a->N, 256) >= c.cus / 2)
        tile = 384;
      // ... and any N % 256 == 0 problem whose 192 x 256 tiles make one round that fills >= 0.8 of the CUs (the Perceiver's to_kv at
      // B = 32: 10272 x 1024 x 1024 = 54 x 4 tiles: 55.8 us against 75.3 on 128 x 128, tools/tile_probe.py, profiles/r05_k_*)
      // (measured with f16c rows -> fp32 rows + bias, the to_kv launch itself; the rule excludes the epilogue classes
      //  nobody measured on these tiles — produced statistics, ln_operand_out, KX_F16C / KX_BF16X3 outputs, residual + 16-bit
      //  output — and has its own off bit, tuning key 15 & 64)
      if (!(rules & (2 | 64)) && (tile == 160 || tile == 128) && (f16 || f16c || a->prec == KX_PREC_BF16) &&
          !a->stats_out && !a->ln_operand_out && !pl->c_f16c && !pl->c_x3 && !(a->residual && pl->c_bf16) &&
          a->N % 256 == 0 && a->K >= 1024 && cdiv(a->M, 192) * cdiv(a->N, 256) <= c.cus &&
          cdiv(a->M, 192) * cdiv(a->N, 256) >= (4 * c.cus) / 5)
        tile = 384;
      // A/B: tuning key 4 = 6 keeps the 128 / 160-row kernels for fp16 rows where bf16 takes the 256x128 ring
      if ((f16c || f16) && tile == 256 && c.t(KX_TUNE_GEMM_EPILOGUE) == 6) tile = cost(160) <= cost(128) ? 160 : 128;
    }
  }
  // THROUGHPUT objective (tuning key 18 = 1; A/B alone: key 15 & 256): 256-row tiles wherever the rules above chose 192-row ones.
  // The rules above minimise the time of ONE launch alone on the chip (rounds x tile time).  A caller that keeps two steps in
  // flight on two streams fills a launch's idle CUs with the other step's kernels, and what counts then is the launch's
  // CU-microseconds = tiles x tile time: since the balanced K loop a K-tile costs the same at both heights (2436 vs 2450 cycles),
  // so 19 x 24 tiles of 192 rows (decoder qkv at M = 3648) are 27 % more CU time than 15 x 24 of 256 — for the same two rounds.
  // Measured, same box, alternating (tools/cutime_ab.sh, profiles/r06_h_*): two steps in flight 1280 -> 1314 samples/s (+2.7 %,
  // two boxes); ONE step at a time 27.7 -> 28.5 ms (-3 %: there the rounds are what counts) — hence an objective, not a default.
  // (The other CU-time candidate — whole 256 x 256 tiles on half the chip instead of the pair split, key 15 & 128 — measured
  // +1.3 % alone, +0.2 % on top of this rule, and -10 % with one step at a time: A/B only.)
  if (tile == 384 && a->tile == 0 && ((rules & 256) || c.t(KX_TUNE_OBJECTIVE) == 1) &&
      !((rules & 1024) && a->xpos_dim) && !((rules & 2048) && !a->xpos_dim))
    tile = 512;                          // (A/B bits 15 & 1024 / 2048: the XPos launches / all the others keep their 192-row tiles)
  // A 64x64 wave owns 32 columns only: the statistics producer needs the split-K reduce kernel (whose threads walk whole
  // 64-column segments) — when the call will not actually be split, take 128x128 instead (its waves own 64 columns).
  if (tile == 64 && a->ln_operand_out) tile = 128;        // the producer lives in the 64-column store loops
  if (tile == 64 && a->stats_out &&
      !(a->splitk_ws && kx_splitk_slices(*c.tn, a->M, a->N, pl->K, 128 / es, a->splitk_ws_bytes, a->splitk ? a->splitk : (a->stats_out && !f16c ? -2 : 0), f16c) > 1))
    tile = 128;
  pl->tile = tile;
  return KX_OK;
}

// ---- phase 3b: what belongs to tile 16 (weight streaming) and what is refused everywhere else ----
inline int tile16_or_not(const Ctx& c, KxGemmPlan* pl) {
  const kx_gemm_args* a = c.a;
  const int es = c.es;
  if (pl->tile == 16) {
    KXP_REQUIRE((a->prec == KX_PREC_BF16 || a->prec == KX_PREC_F32) && a->M <= 16,
                "kx_gemm: tile 16 (weight streaming) takes bf16 or fp32 operands, M <= 16 only");
    KXP_REQUIRE(!a->w_tiled || a->K % 32 == 0, "kx_gemm: the streaming weight layout needs K %% 32 == 0");
    KXP_REQUIRE(a->w_tiled >= 0 && a->w_tiled <= 4 && (a->w_tiled < 2 || (a->prec == KX_PREC_F32 && a->K % 32 == 0)),
                "kx_gemm: w_tiled is 0, 1 or (fp32 operands, K %% 32 == 0) 2 = 24-bit planes / 3 = block-scaled 16-bit weights / 4 = 3 with KX_F16P rows in A");
    KXP_REQUIRE(a->w_tiled != 4 || (!a->ln_gamma && a->lda % 32 == 0), "kx_gemm: w_tiled = 4 takes KX_F16P rows (lda %% 32 == 0), no ln_gamma");
    pl->w_tiled = a->w_tiled == 4 ? 3 : a->w_tiled;
    pl->a_pieces = a->w_tiled == 4;
    KXP_REQUIRE(!a->ln_gamma || (a->ln_beta && (size_t)a->M * (a->K * es + 16) <= 144 * 1024 && a->K % 4 == 0),     // (+ 16 KB of accumulators: 160)
                "kx_gemm: LayerNorm prologue needs beta and M*(K*%d+16) <= 144 KB", es);
    KXP_REQUIRE(!a->ln_operand_out, "kx_gemm: tile 16 does not produce ln_operand_out");
    KXP_REQUIRE(!a->residual2 || a->residual, "kx_gemm: residual2 is the second addend of `residual`");
    KXP_REQUIRE(!a->a_add || a->ln_gamma, "kx_gemm: a_add is the second addend of the LayerNorm-prologue rows (ln_gamma)");
    KXP_REQUIRE(!(a->residual2 || a->ksplit > 1) || (pl->vec_ok && a->N % 16 == 0 && !a->xpos_dim && !(a->row_stats && !a->stats_partials)),
                "kx_gemm: residual2 / ksplit need N %% 16 == 0, 16-byte aligned rows, no XPos, statistics as partials");
    KXP_REQUIRE(c.t(KX_TUNE_GEMV_VARIANT) != 1 || !(a->residual2 || a->a_add || a->ksplit > 1),
                "kx_gemm: the pair form of the residual stream needs the second form of the streaming kernel (tuning key 8 != 1)");
    pl->take_pair_extras = 1;
    if (a->ksplit > 1) {
      KXP_REQUIRE(a->ksplit == 2 && a->C2 && a->cdt == KX_F32 && a->act == KX_ACT_NONE && !a->stats_out && !a->ln_gamma &&
                      a->K % (64 * a->ksplit) == 0 && ((uintptr_t)a->C2 & 15) == 0,
                  "kx_gemm: ksplit = 2 needs C2, an fp32 C, no activation / statistics producer / ln_gamma, K %% 128 == 0");
      pl->gsplit = a->ksplit; pl->kfull = pl->K; pl->K = pl->K / a->ksplit;
    }
    KXP_REQUIRE(!a->stats_partials || (a->colsum && !a->row_stats && a->stats_in_nseg > 0 && a->stats_in_seg > 0),
                "kx_gemm: stats_partials needs colsum, nseg, seg size and excludes row_stats");
    KXP_REQUIRE(!a->stats_out || (a->stats_out_seg == 16 && a->N % 16 == 0 && !a->residual),
                "kx_gemm: tile 16 emits statistics per 16-column segment (stats_out_seg = 16, N %% 16 == 0, no residual)");
    pl->take_ln_g = 1;
    if (a->ln_gamma) pl->lda_b = a->lda * 4;              // A holds fp32 rows in this mode
    pl->take_stats_partials = 1;
    if (a->stats_out) pl->stats_nseg = (int)(a->N / 16);
  } else {
    KXP_REQUIRE(!(a->ln_gamma || (a->stats_out_seg != 0 && a->stats_out_seg != 64)),
                "kx_gemm: ln_gamma / stats_out_seg = 16 belong to tile 16 (weight streaming)");
    KXP_REQUIRE(a->ksplit <= 1 && !a->C2 && !a->residual2 && !a->a_add, "kx_gemm: ksplit / C2 / residual2 / a_add belong to tile 16");
    if (a->stats_partials) {                            // consumed by the row-owning split-K reduce (checked below)
      KXP_REQUIRE(a->colsum && !a->row_stats && a->stats_in_nseg > 0 && a->stats_in_seg > 0,
                  "kx_gemm: stats_partials needs colsum, nseg, seg size and excludes row_stats");
      pl->take_stats_partials = 1;
    }
  }
  return KX_OK;
}

// ---- phase 4: split-K of the 64x64 launches, the row-owning reduce's preconditions, the finalize launch ----
inline int split_k(const Ctx& c, KxGemmPlan* pl) {
  const kx_gemm_args* a = c.a;
  const bool f16c = c.f16c, f16 = c.f16;
  const int es = c.es, tile = pl->tile;
  if (tile == 64 && a->splitk_ws) {
    // Skinny problems (batch-1 shapes: M = 114 / 257 / 64) are weight-streaming bound and a 64x64 grid of N/64 x 2
    // workgroups leaves most CUs idle while each one walks all of K serially.  Slice K so that ~512 workgroups
    // stream the weights concurrently; partials are small ([splits][M][N] fp32, L2/MALL resident).
    long long sp = kx_splitk_slices(*c.tn, a->M, a->N, pl->K, 128 / es, a->splitk_ws_bytes, a->splitk ? a->splitk : (a->stats_out && !f16c ? -2 : 0), f16c);
    // ... unless the tiles alone nearly fill the chip (the batch-1 qkv GEMMs: 192 / 240 tiles) and nothing needs the reduce
    // kernel: then ONE workgroup per tile walks all of K on the 8-stage ring (six K-tiles in flight instead of three) and
    // the reduce launch with its dirty-L2 boundary disappears.  Tuning key 4 = 7 keeps the split.
    const long long tiles64 = ((a->M + 63) / 64) * ((a->N + 63) / 64);
    if (sp == 2 && !a->splitk && pl->ring && es == 2 && !f16 && tiles64 >= 160 && tiles64 <= c.cus && !a->stats_out &&
        !a->ln_out && !a->stats_partials && c.t(KX_TUNE_GEMM_EPILOGUE) != 7 && pl->K / 64 >= 8) {
      sp = 1;
      pl->ring = 8;
    }
    if (sp > 1 && pl->c_hilo) sp = 1;                      // the reduce kernel's epilogue does not write KX_F16HL rows
    if (sp > 1) {
      pl->splitk = (int)sp;
      // in-launch reduction (GemmParams.coop; the caller asks for it by passing splitk_flags — the stage entry points only with
      // tuning key 17 = 1: MEASURED no faster than the reduce launch it replaces, profiles/r06_d_*): every workgroup resident
      // (64 KB of LDS / 256 threads: two per CU), the row-owning reduce's preconditions, and a kernel that exists in this form
      // (the ring for bf16 / fp16 / fp32 rows, two stages for KX_F16C)
      pl->coop = a->splitk_flags && c.t(KX_TUNE_SPLITK_COOP) != 2 && a->N <= 8192 && a->N % 4 == 0 && pl->vec_ok &&
                 tiles64 * sp <= 2ll * c.cus && a->M <= tiles64 * sp && (pl->ring == 1 || f16c) && !pl->c_hilo && !pl->c_pieces;
    }
  }
  // row-owning reduce (LayerNorm of the output row as a second output; folded-LN statistics from partials)
  if (a->ln_out || (a->stats_partials && tile != 16)) {
    KXP_REQUIRE(pl->splitk > 1 && a->N <= 8192 && a->N % 4 == 0 && pl->vec_ok,
                "kx_gemm: ln_out / stats_partials need the split-K row reduce (skinny problem with scratch, N <= 8192, "
                "N %% 4 == 0, aligned C): M=%lld N=%lld K=%lld splits=%d", (long long)a->M, (long long)a->N, (long long)a->K,
                pl->splitk);
    KXP_REQUIRE(!a->ln_out || (a->ln_out_gamma && a->ln_out_beta && (((uintptr_t)a->ln_out | (uintptr_t)a->ln_out_gamma |
                                                                    (uintptr_t)a->ln_out_beta) & 15) == 0),
                "kx_gemm: ln_out needs 16-byte aligned gamma / beta / output");
    KXP_REQUIRE(!a->stats_out, "kx_gemm: the row reduce does not produce statistics");
  }
  if (pl->fin_first && pl->pairk && pl->lean_res && c.fin_nseg <= 128 && (c.t(KX_TUNE_GEMM_RULES) & 32)) {   // opt-in: measured slower (see validate_stats_form)
    pl->fin_first = 0; pl->fin_in_launch = 1;
  }
  if (tile == 512 || tile == 384) {
    const int st = c.t(KX_TUNE_GEMM_STAGGER);
    if (st >= 200000) { if (a->residual) pl->stagger_ticks = st - 200000; }   // A/B: only the in-place residual epilogues
    else if (st > 0) pl->stagger_ticks = st;
  }
  return KX_OK;
}

// ---- phase 5: the instantiation of every launch ----
inline bool act4(int act) { return act == KX_ACT_NONE || act == KX_ACT_GELU || act == KX_ACT_GELU_FAST || act == KX_ACT_QUICK_GELU; }

// gemm_kernel<T, BM, BN, ACT, EPI, NST, COOP> (+ the split-K reduce)
inline int instantiate_tile(const Ctx& c, KxGemmPlan* pl, int BM, int BN) {
  const kx_gemm_args* a = c.a;
  pl->family = KX_FAM_TILE; pl->BM = BM; pl->BN = BN; pl->NST = 2;
  pl->tiles_m = (int)cdiv(a->M, BM); pl->tiles_n = (int)cdiv(a->N, BN);
  pl->grid_x = (unsigned)(pl->tiles_m * pl->tiles_n); pl->grid_y = (unsigned)pl->splitk; pl->block = 256;
  const bool t64 = BM == 64 && BN == 64, two_byte = pl->elem != KX_ELEM_F32;
  pl->ACT = pl->act;
  if (pl->splitk > 1) {
    // skinny problem: the tile kernels only produce partials (activation-free), the reduce kernel owns the epilogue
    if (t64 && pl->coop) {                      // ... or the launch reduces them itself (GemmParams.coop)
      if (!act4(pl->act)) return refuse(pl, KX_ERR_INVALID_ARG, "kx_gemm: unknown activation %d", pl->act);
      if (pl->ring) pl->NST = 4;
      else if (pl->elem != KX_ELEM_F16C)
        return refuse(pl, KX_ERR_UNSUPPORTED, "kx_gemm: the in-launch split-K reduction of this precision needs the ring kernel");
      pl->COOP = 1;
      return KX_OK;
    }
    pl->ACT = KX_ACT_NONE;
    if (t64 && pl->ring) pl->NST = 4;
    if (!act4(pl->act)) return refuse(pl, KX_ERR_INVALID_ARG, "kx_gemm: unknown activation %d", pl->act);
    pl->reduce_act = pl->act;
    if (a->ln_out || (pl->take_stats_partials && a->stats_partials && !(pl->take_ln_g && a->ln_gamma))) {   // row-owning reduce with its fusions
      // 16-byte column groups per thread: 2 (N <= 2048: operands prefetched, see splitk_reduce_row) or 8; tuning key 4 = 10: always 8 (A/B)
      pl->reduce = KX_REDUCE_ROWS;
      pl->reduce_nj = (a->N <= 2048 && c.t(KX_TUNE_GEMM_EPILOGUE) != 10) ? 2 : 8;
      pl->reduce_grid = (unsigned)a->M;
    } else {
      pl->reduce = KX_REDUCE_PLAIN;
      const long long work = (long long)a->M * ((a->N + 3) / 4);
      pl->reduce_grid = (unsigned)((work + 255) / 256);
    }
    return KX_OK;
  }
  // the ViT's bf16 / fp16-output GEMMs (qkv, fc1) on the 160-row kernel: lean epilogue
  if (BM == 160 && two_byte && pl->lean_epilogue && !a->stats_out && a->N % BN == 0 &&
      (pl->act == KX_ACT_NONE || pl->act == KX_ACT_QUICK_GELU || pl->act == KX_ACT_GELU_FAST)) {
    pl->EPI = 1;
    return KX_OK;
  }
  // unsplit skinny launch whose tiles fit one per CU: the 8-stage ring (128 KB of LDS, six K-tiles in flight) walks all of
  // K in one workgroup — no partials, no reduce launch (the batch-1 qkv GEMMs: 192 / 240 tiles)
  if (t64 && pl->elem == KX_ELEM_BF16 && pl->ring == 8) {
    if (!(pl->act == KX_ACT_NONE || pl->act == KX_ACT_GELU_FAST || pl->act == KX_ACT_QUICK_GELU))
      return refuse(pl, KX_ERR_INVALID_ARG, "kx_gemm: unknown activation %d", pl->act);
    pl->NST = 8;
    return KX_OK;
  }
  if (t64 && pl->ring) {
    if (!act4(pl->act)) return refuse(pl, KX_ERR_INVALID_ARG, "kx_gemm: unknown activation %d", pl->act);
    pl->NST = 4;
    return KX_OK;
  }
  // the activation is a compile-time property of the kernel: a runtime switch costs ~4 scalar branches per value
  if (pl->act == KX_ACT_RELU || pl->act == KX_ACT_SWISH) {            // relu / swish: the 128 x 128 kernel only (choose_tile routes them here)
    if (!(BM == 128 && BN == 128))
      return refuse(pl, KX_ERR_UNSUPPORTED, "kx_gemm: %s is offered by the 128 x 128 tile kernel only", pl->act == KX_ACT_RELU ? "relu" : "swish");
    return KX_OK;
  }
  if (!act4(pl->act)) return refuse(pl, KX_ERR_INVALID_ARG, "kx_gemm: unknown activation %d", pl->act);
  return KX_OK;
}

// gemm_kernel_p3<T, ACT, PHASED>: the 256x128 ring kernel
inline int instantiate_p3(const Ctx& c, KxGemmPlan* pl, bool phased) {
  const kx_gemm_args* a = c.a;
  pl->family = KX_FAM_P3; pl->BM = 256; pl->BN = 128; pl->PHASED = phased;
  pl->tiles_m = (int)cdiv(a->M, 256); pl->tiles_n = (int)cdiv(a->N, 128);
  pl->grid_x = (unsigned)(pl->tiles_m * pl->tiles_n); pl->grid_y = 1; pl->block = 512;
  if (!act4(pl->act)) return refuse(pl, KX_ERR_INVALID_ARG, "kx_gemm: unknown activation %d", pl->act);
  pl->ACT = pl->act;
  return KX_OK;
}

// gemm_kernel_p5<T, ACT, BM, EPI, KS2, BAL>: the 256-column kernel on 256- or 192-row tiles.  EPI: 0 generic store loops, 1 lean
// 16-bit tile store, 4 the same with produced statistics, 5 bf16 XPos rows, 6 / 7 KX_F16C three-plane store without / with
// statistics, 8 fp32 XPos rows, 9 fp32 rows with residual.  The lean variants exist for the activations the forward uses them
// with; a (class, activation) pair without a kernel takes EPI 0 — decided here, never discovered by the launcher.
inline int instantiate_p5(const Ctx& c, KxGemmPlan* pl, int BM) {
  const kx_gemm_args* a = c.a;
  const bool is16c = pl->elem == KX_ELEM_F16C;
  pl->family = KX_FAM_P5; pl->BM = BM; pl->BN = 256; pl->BAL = pl->bal;
  pl->tiles_m = (int)cdiv(a->M, BM); pl->tiles_n = (int)cdiv(a->N, 256);
  pl->grid_y = 1; pl->block = 512;
  const int nwg = pl->tiles_m * pl->tiles_n;
  if (BM == 256 && pl->pairk) {                // K split over workgroup pairs (pair_ok: no activation / statistics, even nk, tiles % 8 == 0)
    pl->grid_x = (unsigned)(2 * nwg);
    pl->ACT = KX_ACT_NONE; pl->EPI = pl->lean_res ? 9 : 0; pl->KS2 = 1;
    return KX_OK;
  }
  pl->grid_x = (unsigned)(pl->persistent > 0 ? (nwg < pl->persistent ? nwg : pl->persistent) : nwg);
  // lean_xpos: 2 = asked for (tuning key 4 = 3), 1 = eligible — taken on the 192-row tiles, where the rotated accumulators fit
  // the registers (bf16 qkv at M = 3648: 109.6 -> 93.8 us, bit-identical; the 256-row form spills 352 B / lane and measured slower)
  const bool lx = pl->lean_xpos == 2 || (pl->lean_xpos == 1 && BM == 192);
  const bool n256 = a->N % 256 == 0;
  int epi = 0;
  if (pl->lean_res) epi = 9;
  else if (is16c) {
    // KX_F16C output on whole 256-column tiles, no residual / XPos: the three-plane lean store (else the generic loops)
    if (BM == 256 && pl->lean_f16c && n256) epi = a->stats_out ? 7 : 6;
    else if (BM == 192 && lx && !pl->c_bf16 && n256) epi = 8;      // fp32 q / k / v of the f16c qkv GEMM
    // plain fp16 rows out of fp16 / f16c operands (the CLIP tower's qkv and fc1 in mixed mode): the lean tile store, as for bf16 —
    // these launches took the generic store loops until round 5 (+16 k cycles per tile: tools/epi_probe.py, profiles/r05_f_*)
    else if (pl->lean_epilogue && pl->c_f16 && !a->stats_out && n256) epi = 1;
  }
  else if (lx && pl->c_bf16 && n256) epi = 5;
  else if (pl->lean_epilogue && n256) epi = a->stats_out ? 4 : 1;
  const int act = pl->act;
  pl->ACT = act;
  if (epi == 9) { pl->ACT = KX_ACT_NONE; pl->EPI = 9; return KX_OK; }      // fp32 output with residual, bias + folded-LN consume at accumulator level (no activation)
  if (epi == 8) {                                                          // fp32 output, bias + q-scale + XPos at accumulator level (no activation)
    if (act == KX_ACT_NONE) { pl->EPI = 8; return KX_OK; }
    epi = 0;
  }
  if (epi == 6 || epi == 7) {     // KX_F16C output (BM = 256): plain and GELU, with (7) or without (6) produced statistics
    if (act == KX_ACT_NONE) { pl->EPI = epi; return KX_OK; }
    // (GELU without statistics spills 248 B / lane in this form: it keeps the generic loops)
    if (epi == 7 && act == KX_ACT_GELU_FAST) { pl->EPI = 7; return KX_OK; }
    epi = 0;
  }
  for (;;) {                      // epi is 0, 1, 4 or 5 here; one fallback to 0 at most
    if (act == KX_ACT_NONE && epi != 4) { pl->EPI = epi; return KX_OK; }
    if (epi == 5) { epi = 0; continue; }
    if (act == KX_ACT_GELU_FAST) {
      // plain bf16 in, plain bf16 out, accumulator-level epilogue: the transcendental-free packed GELU (KX_ACT_GELU_POLY); round 5:
      // plain fp16 in / out too (EPI 1: the CLIP tower's fc1 in mixed mode — gelu_poly is set for those launches only)
      const bool poly_exists = is16c ? epi == 1 : epi != 0;
      if (poly_exists && pl->gelu_poly) pl->ACT = KX_ACT_GELU_POLY;
      pl->EPI = epi; return KX_OK;
    }
    if (act == KX_ACT_QUICK_GELU && (epi == 0 || epi == 1)) { pl->EPI = epi; return KX_OK; }
    if (epi != 0) { epi = 0; continue; }
    if (act == KX_ACT_GELU) { pl->EPI = 0; return KX_OK; }
    return refuse(pl, KX_ERR_INVALID_ARG, "kx_gemm: unknown activation %d", act);
  }
}

inline int instantiate(const Ctx& c, KxGemmPlan* pl) {
  const kx_gemm_args* a = c.a;
  const int tile = pl->tile;
  // 16-bit tile kernels: [bf16 | f16c | f16] x [128, 64, 160, 256x128, 256x256]
  static const int kinds16[3][5] = {
      {KX_K_GEMM_BF16_128, KX_K_GEMM_BF16_64, KX_K_GEMM_BF16_160, KX_K_GEMM_BF16_256X128, KX_K_GEMM_BF16_256X256},
      {KX_K_GEMM_F16C_128, KX_K_GEMM_F16C_64, KX_K_GEMM_F16C_160, KX_K_GEMM_F16C_256X128, KX_K_GEMM_F16C_256X256},
      {KX_K_GEMM_F16_128, KX_K_GEMM_F16_64, KX_K_GEMM_F16_160, KX_K_GEMM_F16_256X128, KX_K_GEMM_F16_256X256}};
  const int tsel = (tile == 64 || tile == 16) ? 1 : tile == 160 ? 2 : (tile == 256 || tile == 257) ? 3 : (tile == 512 || tile == 384) ? 4 : 0;
  pl->kind = a->prec == KX_PREC_F32 ? (tile == 64 || tile == 16 ? KX_K_GEMM_F32_64 : KX_K_GEMM_F32_128)
                                    : kinds16[c.f16c ? 1 : c.f16 ? 2 : 0][tsel];
  pl->elem = a->prec == KX_PREC_BF16 ? KX_ELEM_BF16 : a->prec == KX_PREC_F32 ? KX_ELEM_F32 : KX_ELEM_F16C;
  const int e = pl->elem;
  if (tile == 16 && e != KX_ELEM_F16C) {      // the weight-streaming launcher keeps its own variant choice
    pl->family = KX_FAM_TILE16; pl->ACT = pl->act;
    return KX_OK;
  }
  if (tile == 128) return instantiate_tile(c, pl, 128, 128);
  if (tile == 64) return instantiate_tile(c, pl, 64, 64);
  if (tile == 160 && e != KX_ELEM_F32) return instantiate_tile(c, pl, 160, 128);
  if (tile == 256 && e != KX_ELEM_F32) return instantiate_p3(c, pl, true);     // 256x128 ring, phased
  if (tile == 257 && e == KX_ELEM_BF16) return instantiate_p3(c, pl, false);   // A/B: same tile and ring, unphased
  if (tile == 512 && e != KX_ELEM_F32) return instantiate_p5(c, pl, 256);      // 256x256, 128x64 per wave
  if (tile == 384 && e != KX_ELEM_F32) return instantiate_p5(c, pl, 192);      // 192x256,  96x64 per wave
  return refuse(pl, KX_ERR_UNSUPPORTED, "kx_gemm: unknown tile variant %d", tile);
}

}  // namespace kx_plan_detail

// The whole decision.  Returns KX_OK and a complete plan, or the refusal's code with its text in plan->msg.
inline int kx_gemm_plan(const kx_gemm_args& args, const KxTuning& tn, int cu_count, KxGemmPlan* pl) {
  using namespace kx_plan_detail;
  memset(pl, 0, sizeof(*pl));
  Ctx c;
  c.tn = &tn; c.cus = cu_count;
  KXP_TRY(validate_stats_form(c, &args, pl));
  KXP_TRY(validate(c, pl));
  epilogue_class(c, pl);
  KXP_TRY(choose_tile(c, pl));
  KXP_TRY(tile16_or_not(c, pl));
  KXP_TRY(split_k(c, pl));
  return instantiate(c, pl);
}
#undef KXP_REQUIRE
#undef KXP_TRY
