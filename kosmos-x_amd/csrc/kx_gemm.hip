// C = epilogue(A · Wᵀ) for gfx950 — the GEMM behind every nn.Linear on the Kosmos-X forward path.
//
// Layout decisions (MI355X-first):
//  * Both operands are K-contiguous (activations [M,K], PyTorch weights [N,K]), so A and B MFMA
//    fragments are plain 16-byte reads.  The WEIGHT tile is the MFMA "A" operand and the
//    ACTIVATION tile the "B" operand: the accumulator of v_mfma_f32_16x16x{32 bf16,4 f32} then
//    holds 4 consecutive output COLUMNS (n) per lane for one row (m) — 16-byte epilogue stores,
//    float4 bias/residual reads, and the XPos (2j,2j+1) pairs are lane-local.
//  * Tiles are staged HBM→LDS with global_load_lds_dwordx4 (no VGPR round trip).  The LDS image is
//    lane-linear, so the bank-conflict swizzle (16-B chunk ^= row&7 inside each 128-B tile row) is
//    applied to the per-lane SOURCE address and again on the ds_read_b128 (guide rule 21).
//  * A tile row is always 128 bytes (64 bf16 or 32 f32), so one kernel template serves the bf16
//    MFMA path and the exact-f32 MFMA path (fp32 parity mode).
//  * blockIdx → tile map is XCD-aware (bijective remap so each XCD's L2 sees a contiguous run of
//    tiles) and grouped 8 tile-rows deep so neighbouring blocks share operand panels.
#include "kx_gemm_impl.h"


// CUs of the current device, cached per device ordinal (relaxed atomics: racing first calls store the same value)
int kx_cu_count() {
  static std::atomic<int> cus[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  int n = cus[dev].load(std::memory_order_relaxed);
  if (n == 0) {
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cus[dev].store(n, std::memory_order_relaxed);
  }
  return n;
}

// the planner's own split rule (kx_gemm_plan.h) under the current tuning table
int kx_gemm_auto_splits(int64_t M, int64_t N, int64_t K, int prec, size_t ws_bytes) {
  return kx_gemm_auto_splits_with(kx_tuning_snapshot(), M, N, K, prec, ws_bytes);
}

// Sticky device word of the pair split's bounded hand-off (GemmParams.pk_err): 0, or 1 + the index of the last workgroup that
// gave up waiting for its partner's flag.  One word per process and device context; kx_pair_split_errors reads and clears it.
__device__ unsigned g_kx_pair_err;
static unsigned* pair_err_word() {          // the CURRENT device's copy of the word (cached per device ordinal, like kx_cu_count)
  static std::atomic<unsigned*> ptr[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
  unsigned* w = ptr[dev].load(std::memory_order_relaxed);
  if (!w) {
    void* q = nullptr;
    if (hipGetSymbolAddress(&q, HIP_SYMBOL(g_kx_pair_err)) != hipSuccess) return nullptr;
    w = (unsigned*)q;
    ptr[dev].store(w, std::memory_order_relaxed);
  }
  return w;
}
extern "C" int kx_pair_split_errors(unsigned* word_out) {
  KX_REQUIRE(word_out != nullptr, "kx_pair_split_errors: null output");
  unsigned* w = pair_err_word();
  KX_REQUIRE(w != nullptr, "kx_pair_split_errors: device word unavailable");
  unsigned v = 0, zero = 0;
  if (hipMemcpy(&v, w, sizeof v, hipMemcpyDeviceToHost) != hipSuccess ||        // synchronises the device: diagnostics, not the hot path
      (v && hipMemcpy(w, &zero, sizeof zero, hipMemcpyHostToDevice) != hipSuccess)) {
    kx_set_error("kx_pair_split_errors: reading the device word failed");
    return KX_ERR_LAUNCH;
  }
  *word_out = v;
  return KX_OK;
}

extern "C" int kx_row_stats_finalize(const float* partials, int64_t rows, int64_t nseg, int64_t seg_size, float eps, float* out,
                                    void* stream);
// snapshot -> plan (kx_gemm_plan.h: every check, rule and instantiation) -> GemmParams -> launches
extern "C" int kx_gemm(const kx_gemm_args* a, void* stream) {
  KX_REQUIRE(a != nullptr, "kx_gemm: null args");
  const KxTuning tn = kx_tuning_snapshot();
  KxGemmPlan k;
  const int rc = kx_gemm_plan(*a, tn, kx_cu_count(), &k);
  if (rc != KX_OK) { kx_set_error("%s", k.msg); return rc; }
  // a call with row_stats_scratch consumes (mean, rstd) from the scratch: finalised by the launch below, or by the pair split itself
  const bool scratch = a->row_stats_scratch != nullptr;
  GemmParams p;
  p.A = (const char*)a->A; p.W = (const char*)a->W; p.lda_b = k.lda_b; p.ldw_b = k.ldw_b;
  p.C = a->C; p.ldc = a->ldc; p.c_bf16 = k.c_bf16; p.c_x3 = k.c_x3; p.c_f16 = k.c_f16; p.c_f16c = k.c_f16c; p.c_hilo = k.c_hilo;
  p.nk_main = k.nk_main; p.wscale = a->w_scale; p.kskip = k.kskip;
  p.bias = a->bias; p.residual = a->residual; p.ldr = a->ldr;
  p.M = (int)a->M; p.N = (int)a->N; p.K = k.K;
  p.act = k.act; p.qscale = a->qscale; p.qcols = (int)a->qcols;
  p.xq_cs = a->xq_cs; p.xq_ss = a->xq_ss; p.xk_cs = a->xk_cs; p.xk_ss = a->xk_ss;
  p.xpos_T = (int)a->xpos_T; p.xpos_dim = (int)a->xpos_dim;
  p.tiles_m = k.tiles_m; p.tiles_n = k.tiles_n;
  p.vec_ok = k.vec_ok; p.vec8_ok = k.vec8_ok; p.vec2_ok = k.vec2_ok;
  p.row_stats = scratch ? a->row_stats_scratch : a->row_stats; p.colsum = a->colsum;
  p.stats_out = a->stats_out; p.stats_nseg = k.stats_nseg;
  p.lnop_out = a->ln_operand_out; p.lnop_dt = a->ln_operand_dt; p.lnop_stats = a->ln_operand_stats;
  p.splitk = k.splitk; p.partial = k.splitk > 1 ? (float*)a->splitk_ws : nullptr;
  p.stagger_ticks = k.stagger_ticks;
  p.fast_epilogue = k.fast_epilogue; p.lean_epilogue = k.lean_epilogue; p.lean_xpos = k.lean_xpos; p.lean_res = k.lean_res;
  p.lean_f16c = k.lean_f16c; p.w_tiled = k.w_tiled; p.ring = k.ring; p.gelu_poly = k.gelu_poly; p.persistent = k.persistent;
  p.skip_idle_waves = k.skip_idle_waves; p.bal = k.bal;
  p.pairk = k.pairk; p.pk_slab = nullptr; p.pk_flag = nullptr; p.pk_epoch = 0;
  p.pk_err = nullptr; p.pk_spin_ticks = k.pk_spin_ticks; p.pk_fault = k.pk_fault;
  p.coop = k.coop; p.coop_flags = nullptr;
  p.ln_g = k.take_ln_g ? a->ln_gamma : nullptr; p.ln_b = k.take_ln_g ? a->ln_beta : nullptr; p.ln_eps = k.take_ln_g ? a->ln_eps : 0.f;
  // folded-LN statistics as partials: tile 16 and the row-owning reduce take the caller's; the scratch form only when the pair split finalises them
  const bool partials = scratch ? k.fin_in_launch != 0 : k.take_stats_partials != 0;
  p.stats_partials = partials ? a->stats_partials : nullptr; p.stats_in_nseg = partials ? (int)a->stats_in_nseg : 0;
  p.stats_in_seg = partials ? (float)a->stats_in_seg : 0.f; p.stats_eps = partials ? a->stats_eps : 0.f;
  p.gsplit = k.gsplit; p.kfull = k.kfull; p.C2 = k.gsplit > 1 ? a->C2 : nullptr;
  p.residual2 = k.take_pair_extras ? a->residual2 : nullptr; p.a_add = k.take_pair_extras ? a->a_add : nullptr;
  p.no_rowreg = k.no_rowreg; p.valu = 0; p.gb_staged = 0; p.c_pieces = k.c_pieces; p.a_pieces = k.a_pieces; p.hp = 0;
  p.ln_out = a->ln_out; p.ln_out_dt = a->ln_out_dt; p.ln_out_g = a->ln_out_gamma; p.ln_out_b = a->ln_out_beta; p.ln_out_eps = a->ln_out_eps;
  // what needs the device: the hand-offs' epoch and error word
  if (k.pairk) {
    static std::atomic<unsigned> epoch{0};
    p.pk_flag = (unsigned*)a->pair_ws;
    p.pk_slab = (float*)((char*)a->pair_ws + 4096);
    p.pk_epoch = epoch.fetch_add(1, std::memory_order_relaxed) % 0xfffffff0u + 1u;   // never 0 (= consumed / not yet published)
    p.pk_err = pair_err_word();
    KX_REQUIRE(p.pk_err != nullptr, "kx_gemm: the pair split's error word is unavailable");
  }
  if (k.coop) {
    static std::atomic<unsigned> coop_epoch{0};
    p.coop_flags = a->splitk_flags;
    p.pk_epoch = coop_epoch.fetch_add(1, std::memory_order_relaxed) % 0xfffffff0u + 1u;     // never 0: a cleared word is "not arrived"
    p.pk_err = pair_err_word();
    KX_REQUIRE(p.pk_err != nullptr, "kx_gemm: the hand-off error word is unavailable");
  }
  if (k.fin_first)
    KX_TRY(kx_row_stats_finalize(a->stats_partials, a->M, a->stats_in_nseg, a->stats_in_seg, a->stats_eps, a->row_stats_scratch, stream));
  hipStream_t s = (hipStream_t)stream;
  KxProfScope prof(k.kind, a->M, a->N, a->K, s);
  if (k.elem == KX_ELEM_BF16) return k.family == KX_FAM_P3 || k.family == KX_FAM_P5 ? kx_gemm_launch_phased_bf16(p, k, s) : kx_gemm_launch_tiles_bf16(p, k, tn, s);
  if (k.elem == KX_ELEM_F16C) return kx_gemm_launch_f16c(p, k, s);
  return kx_gemm_launch_f32(p, k, tn, s);
}

// What kx_gemm would launch for these arguments, as text (nothing is launched, no operand pointer is read): one line per launch —
// kernel template, template arguments, grid, block (none takes dynamic LDS from the planner) — then one line with the resolved tile and the host flags.
static const char* elem_name(int e) { return e == KX_ELEM_BF16 ? "bf16_t" : e == KX_ELEM_F16C ? "f16c_t" : "float"; }
extern "C" int kx_gemm_describe(const kx_gemm_args* a, int cu_count, char* out, size_t out_bytes) {
  KX_REQUIRE(a != nullptr, "kx_gemm: null args");
  KX_REQUIRE(out != nullptr && out_bytes > 0, "kx_gemm_describe: no output buffer");
  const KxTuning tn = kx_tuning_snapshot();
  KxGemmPlan k;
  const int rc = kx_gemm_plan(*a, tn, cu_count > 0 ? cu_count : kx_cu_count(), &k);
  if (rc != KX_OK) { kx_set_error("%s", k.msg); return rc; }
  size_t n = 0;
  auto put = [&](const char* fmt, auto... v) {
    if (n < out_bytes) { const int w = snprintf(out + n, out_bytes - n, fmt, v...); n += w > 0 ? (size_t)w : 0; }
  };
  const char* tf[2] = {"false", "true"};
  if (k.fin_first) put("%s\n", "kx_row_stats_finalize");
  switch (k.family) {
    case KX_FAM_TILE16: put("%s\n", "gemv_fused"); break;
    case KX_FAM_TILE:
      put("gemm_kernel<%s, %d, %d, %d, %d, %d, %s> grid=%ux%u block=%u\n", elem_name(k.elem), k.BM, k.BN, k.ACT, k.EPI, k.NST,
          tf[k.COOP != 0], k.grid_x, k.grid_y, k.block);
      break;
    case KX_FAM_P3:
      put("gemm_kernel_p3<%s, %d, %s> grid=%ux%u block=%u\n", elem_name(k.elem), k.ACT, tf[k.PHASED != 0], k.grid_x, k.grid_y,
          k.block);
      break;
    default:
      put("gemm_kernel_p5<%s, %d, %d, %d, %s, %s> grid=%ux%u block=%u\n", elem_name(k.elem), k.ACT, k.BM, k.EPI, tf[k.KS2 != 0],
          tf[k.BAL != 0], k.grid_x, k.grid_y, k.block);
  }
  if (k.reduce == KX_REDUCE_ROWS) put("splitk_reduce_rows_kernel<%d, %d> grid=%ux1 block=256\n", k.reduce_act, k.reduce_nj, k.reduce_grid);
  else if (k.reduce == KX_REDUCE_PLAIN) put("splitk_reduce_kernel<%d> grid=%ux1 block=256\n", k.reduce_act, k.reduce_grid);
  put("plan tile=%d kind=%d K=%d act=%d splitk=%d pairk=%d coop=%d ring=%d bal=%d persistent=%d fast_epilogue=%d lean_epilogue=%d lean_xpos=%d "
      "lean_res=%d lean_f16c=%d gelu_poly=%d skip_idle_waves=%d stagger_ticks=%d fin_in_launch=%d pk_fault=%d\n",
      k.tile, k.kind, k.K, k.act, k.splitk, k.pairk, k.coop, k.ring, k.bal, k.persistent, k.fast_epilogue, k.lean_epilogue, k.lean_xpos,
      k.lean_res, k.lean_f16c, k.gelu_poly, k.skip_idle_waves, k.stagger_ticks, k.fin_in_launch, k.pk_fault);
  KX_REQUIRE(n < out_bytes, "kx_gemm_describe: the description needs %zu bytes, %zu given", n + 1, out_bytes);
  return KX_OK;
}
