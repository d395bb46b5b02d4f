// Beam search on the device: the beam step (kx_beam_step), the finalisation (kx_beam_finalize) and the KV-cache reorder
// (kx_kv_cache_gather).  Contract: include/kosmosx_hip.h, "Beam search on the device".
//
// As in kx_sample.hip, everything that decides a result is an exact integer operation or a per-element fp32 expression: maxima
// are taken over (key, ~index) pairs, the softmax mass is a 64-bit fixed-point sum, ranks come from counting.  No result depends
// on the order in which lanes, waves or atomics run, and no workgroup waits on another.
//
// The step is two launches.  rank_kernel: one 1024-thread workgroup per input beam row finds m, Z, lse and then the row's own best
// K = 2W candidates by K arg-max passes, each taking the largest (key(c), ~v) pair below the previous one: 2 + K reads of a row that
// stays in L2 (V * 4 bytes), no histogram and no LDS atomics — the candidates' keys crowd into a few top-digit bins, which is
// where a radix select over 2W <= 32 elements would spend its time.  merge_kernel: one workgroup per batch row ranks the
// Win * K <= 512 pairs by counting how many beat each, and one lane walks the best K.
#include "kx_common.h"
#include "kx_select.h"

#include <cfloat>

namespace {

constexpr int BEAM_MAX_W = 16;
constexpr int MERGE_T = 2 * BEAM_MAX_W * BEAM_MAX_W;   // 512: one thread per (input beam, candidate) pair
constexpr long long KX_BEAM_MAX_V = 1ll << 23;         // 2^23 masses of at most 2^40 each stay below 2^63

struct BeamParams {
  const float* logits; long long ld; int B, Win, W, V, K, step, early;
  float alpha; long long eos, pad;
  const float* s_in; float* s_out; long long* next; int* parent; int* src_row;
  float* pool_score; int* pool_end; int* pool_parent; int* pool_count; unsigned char* done;
  unsigned long long* scratch;
};

// NaN and -inf come back as -inf (never a candidate), +inf as FLT_MAX, -0 as +0 (one key per value)
__device__ __forceinline__ float beam_x(float l) {
  if (!(l > -__builtin_inff())) l = -__builtin_inff();
  if (l > FLT_MAX) l = FLT_MAX;
  if (l == 0.f) l = 0.f;
  return l;
}

// f(i, row[i]) for every i < V: consecutive lanes on consecutive 16-byte vectors where the row allows, scalars otherwise
template <typename F>
__device__ __forceinline__ void scan_row(const float* __restrict__ row, int V, bool vec, F&& f) {
  const int tid = threadIdx.x;
  int done = 0;
  if (vec) {
    const float4* __restrict__ r4 = reinterpret_cast<const float4*>(row);
    const int n4 = V >> 2;
#pragma unroll 2
    for (int q = tid; q < n4; q += SB) {
      const float4 v = r4[q];
      f(4 * q, v.x); f(4 * q + 1, v.y); f(4 * q + 2, v.z); f(4 * q + 3, v.w);
    }
    done = n4 << 2;
  }
  for (int i = done + tid; i < V; i += SB) f(i, row[i]);
}

__global__ __launch_bounds__(SB) void rank_kernel(const BeamParams a) {
  __shared__ unsigned long long red[SW];
  const long long r = blockIdx.x;                     // input beam row b * Win + j
  const int tid = threadIdx.x;
  const float* __restrict__ row = a.logits + r * a.ld;
  const bool vec = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
  unsigned long long* out = a.scratch + r * a.K;
  const float s = a.s_in[r];
  const bool live = !a.done[r / a.Win] && s > -__builtin_inff();   // (uniform)

  unsigned long long best = 0;
  if (live) scan_row(row, a.V, vec, [&](int i, float l) {
    const unsigned long long pk = ((unsigned long long)f2key(beam_x(l)) << 32) | (0xffffffffu - (unsigned)i);
    best = pk > best ? pk : best;
  });
  best = block_max_u64(best, red);
  const unsigned kmax = (unsigned)(best >> 32);
  if (!live || kmax < KEY_MIN_VALID) {                // a frozen row, a dead beam, or no finite logit: no candidate
    for (int k = tid; k < a.K; k += SB) out[k] = 0;
    return;
  }
  const float m = key2f(kmax);
  unsigned long long z = 0;
  scan_row(row, a.V, vec, [&](int, float l) {
    const float x = beam_x(l);
    if (x > -__builtin_inff()) z += mass_fix(x, m);
  });
  z = block_sum_u64(z, red);
  const float lse = m + logf((float)z * 9.094947017729282e-13f);   // 2^-40

  unsigned long long prev = ~0ull;
#pragma unroll 1
  for (int k = 0; k < a.K; ++k) {
    unsigned long long cur = 0;
    scan_row(row, a.V, vec, [&](int i, float l) {
      const float x = beam_x(l);
      float c = s + (x - lse);                        // -inf for x = -inf
      if (c == 0.f) c = 0.f;
      const unsigned long long pk = ((unsigned long long)f2key(c) << 32) | (0xffffffffu - (unsigned)i);
      if (pk < prev && pk > cur) cur = pk;
    });
    cur = block_max_u64(cur, red);
    if ((unsigned)(cur >> 32) < KEY_MIN_VALID) cur = 0;            // what is left is at -inf
    if (tid == 0) out[k] = cur ? ((cur & 0xffffffff00000000ull) | (0xffffffffu - (unsigned)cur)) : 0ull;
    if (cur == 0) {
      for (int q = k + 1 + tid; q < a.K; q += SB) out[q] = 0;
      break;
    }
    prev = cur;
  }
}

// pool insertion under the replacement rule; returns nothing, the pool is per batch row and owned by one lane
__device__ void pool_offer(float* ps, int* pe, int* pp, int& count, int W, float score, int end, int parent) {
  if (count < W) {
    ps[count] = score; pe[count] = end; pp[count] = parent;
    ++count;
    return;
  }
  int worst = 0;
  for (int k = 1; k < W; ++k) if (ps[k] <= ps[worst]) worst = k;   // the later slot among equal ones
  if (score > ps[worst]) { ps[worst] = score; pe[worst] = end; pp[worst] = parent; }
}

__global__ __launch_bounds__(MERGE_T) void merge_kernel(const BeamParams a) {
  __shared__ unsigned long long ent[MERGE_T];
  __shared__ unsigned long long top[2 * BEAM_MAX_W];
  __shared__ int topj[2 * BEAM_MAX_W];
  const int tid = threadIdx.x, b = blockIdx.x, W = a.W, K = a.K;
  const long long o = (long long)b * W;
  if (a.done[b]) {                                    // frozen: scores kept, pad, identity
    if (tid < W) {
      const int p = tid < a.Win ? tid : 0;
      a.s_out[o + tid] = a.s_in[(long long)b * a.Win + p];
      a.next[o + tid] = a.pad;
      a.parent[o + tid] = p;
      a.src_row[o + tid] = b * a.Win + p;
    }
    return;
  }
  const int n = a.Win * K;
  const unsigned long long e = tid < n ? a.scratch[(long long)b * n + tid] : 0ull;
  ent[tid] = e;
  if (tid < 2 * BEAM_MAX_W) top[tid] = 0;
  __syncthreads();
  if (e) {                                            // rank = how many pairs beat this one (key, then the lower j * V + v)
    const int j = tid / K;
    const unsigned key = (unsigned)(e >> 32);
    const long long flat = (long long)j * a.V + (unsigned)e;
    int rank = 0, u = 0;
    for (int ju = 0; ju < a.Win; ++ju)
      for (int k = 0; k < K; ++k, ++u) {
        const unsigned long long eu = ent[u];
        const unsigned ku = (unsigned)(eu >> 32);
        rank += eu != 0 && (ku > key || (ku == key && (long long)ju * a.V + (unsigned)eu < flat));
      }
    if (rank < K) { top[rank] = e; topj[rank] = j; }
  }
  __syncthreads();
  if (tid != 0) return;
  const float pen = powf((float)(a.step + 1), a.alpha);
  float* ps = a.pool_score + o;
  int* pe = a.pool_end + o;
  int* pp = a.pool_parent + o;
  int count = a.pool_count[b], filled = 0;
  float best_live = -__builtin_inff();
  for (int k = 0; k < K && filled < W; ++k) {
    const unsigned long long t = top[k];
    if (!t) break;
    const float c = key2f((unsigned)(t >> 32));
    const long long v = (unsigned)t;
    if (a.eos >= 0 && v == a.eos) {
      if (k < W) pool_offer(ps, pe, pp, count, W, c / pen, a.step, topj[k]);
      continue;
    }
    if (filled == 0) best_live = c;
    a.s_out[o + filled] = c;
    a.next[o + filled] = v;
    a.parent[o + filled] = topj[k];
    a.src_row[o + filled] = b * a.Win + topj[k];
    ++filled;
  }
  for (int i = filled; i < W; ++i) {
    const int p = i < a.Win ? i : 0;
    a.s_out[o + i] = -__builtin_inff();
    a.next[o + i] = a.pad;
    a.parent[o + i] = p;
    a.src_row[o + i] = b * a.Win + p;
  }
  a.pool_count[b] = count;
  if (count == W) {
    float worst = ps[0];
    for (int k = 1; k < W; ++k) worst = ps[k] < worst ? ps[k] : worst;
    if (a.early || worst >= best_live / pen) a.done[b] = 1;
  }
}

__global__ __launch_bounds__(64) void finalize_kernel(const float* __restrict__ s_live, const unsigned char* __restrict__ done,
                                                      float* pool_score, int* pool_end, int* pool_parent, int* pool_count,
                                                      const int* __restrict__ parent, const long long* __restrict__ token,
                                                      long long trace_ld, int W, int R, int n, float alpha, long long eos,
                                                      long long pad, long long* out_tokens, long long out_ld, float* out_scores) {
  __shared__ int order[BEAM_MAX_W];
  const int b = blockIdx.x, tid = threadIdx.x;
  const long long o = (long long)b * W;
  float* ps = pool_score + o;
  int* pe = pool_end + o;
  int* pp = pool_parent + o;
  if (tid == 0) {
    int count = pool_count[b];
    if (!done[b]) {
      const float pen = powf((float)n, alpha);
      for (int i = 0; i < W; ++i)
        if (s_live[o + i] > -__builtin_inff()) pool_offer(ps, pe, pp, count, W, s_live[o + i] / pen, n, i);
      pool_count[b] = count;
    }
    unsigned used = 0;                                // the R best: score descending, the earlier slot among equal ones
    for (int r = 0; r < R; ++r) {
      int pick = -1;
      for (int k = 0; k < count; ++k)
        if (!((used >> k) & 1u) && (pick < 0 || ps[k] > ps[pick])) pick = k;
      if (pick >= 0) used |= 1u << pick;
      order[r] = pick;
    }
  }
  __syncthreads();
  if (tid >= R) return;
  long long* out = out_tokens + ((long long)b * R + tid) * out_ld;
  for (int g = 0; g < n; ++g) out[g] = pad;
  const int k = order[tid];
  out_scores[(long long)b * R + tid] = k < 0 ? -__builtin_inff() : ps[k];
  if (k < 0) return;
  int end = pe[k], slot = pp[k];
  end = end < 0 ? 0 : (end > n ? n : end);            // memory safety only
  if (end < n) out[end] = eos;
  for (int g = end - 1; g >= 0; --g) {
    slot = slot < 0 ? 0 : (slot >= W ? W - 1 : slot);
    out[g] = token[g * trace_ld + o + slot];
    slot = parent[g * trace_ld + o + slot];
  }
}

// one 16-byte vector per thread and iteration; a (layer, row, head) chunk of copy_vecs vectors is contiguous on both sides
// (`heads` = chunks per (layer, row): 1 under the row-major cache layout, whose chunk is the first t rows of every head)
__global__ __launch_bounds__(256) void kv_gather_kernel(const uint4* __restrict__ sk, const uint4* __restrict__ sv,
                                                        uint4* __restrict__ dk, uint4* __restrict__ dv,
                                                        const int* __restrict__ src_row, int B_src, int B_dst, int heads,
                                                        long long row_vecs, long long copy_vecs, long long total, int* err) {
  const long long stride = (long long)gridDim.x * 256;
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += stride) {
    const long long chunk = idx / copy_vecs, off = idx - chunk * copy_vecs;
    const int h = (int)(chunk % heads);
    const long long lr = chunk / heads;
    const int r = (int)(lr % B_dst);
    const long long l = lr / B_dst;
    const int s = src_row[r];
    if (s < 0 || s >= B_src) {                        // the caller's error: nothing of this row is read or written
      if (off == 0 && h == 0 && l == 0) atomicOr(err, KX_RAGGED_ERR_GATHER);
      continue;
    }
    const long long si = ((l * B_src + s) * heads + h) * row_vecs + off;
    const long long di = ((l * B_dst + r) * heads + h) * row_vecs + off;
    dk[di] = sk[si];
    dv[di] = sv[si];
  }
}

bool ranges_overlap(const void* a, size_t an, const void* b, size_t bn) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + bn && y < x + an;
}

}  // namespace

extern "C" int kx_beam_step(const kx_beam_args* args, void* stream) {
  KX_REQUIRE(args != nullptr, "kx_beam_step: null args");
  KX_REQUIRE(args->struct_bytes == sizeof(kx_beam_args),
             "kx_beam_step: stale binding — caller declares kx_beam_args as %u bytes, this library (ABI %d) as %zu",
             (unsigned)args->struct_bytes, KX_ABI_VERSION, sizeof(kx_beam_args));
  KX_REQUIRE(args->logits && args->scores_in && args->scores_out && args->next_token && args->parent && args->src_row,
             "kx_beam_step: null logits / scores_in / scores_out / next_token / parent / src_row");
  KX_REQUIRE(args->pool_score && args->pool_end && args->pool_parent && args->pool_count && args->done && args->scratch,
             "kx_beam_step: null pool_score / pool_end / pool_parent / pool_count / done / scratch");
  KX_REQUIRE(args->W >= 1 && args->W <= BEAM_MAX_W, "kx_beam_step: W=%lld outside [1, %d]", (long long)args->W, BEAM_MAX_W);
  KX_REQUIRE(args->Win == 1 || args->Win == args->W, "kx_beam_step: Win=%lld must be 1 or W=%lld", (long long)args->Win,
             (long long)args->W);
  KX_REQUIRE(args->B >= 1 && args->B * args->W <= 0x7fffffffll, "kx_beam_step: B=%lld must be >= 1", (long long)args->B);
  KX_REQUIRE(args->V >= 2 * args->W, "kx_beam_step: V=%lld is smaller than 2W=%lld", (long long)args->V, (long long)(2 * args->W));
  KX_REQUIRE(args->ld >= args->V, "kx_beam_step: ld=%lld is smaller than V=%lld", (long long)args->ld, (long long)args->V);
  KX_REQUIRE(args->step >= 0 && args->step < 0x7fffffffll, "kx_beam_step: step=%lld must be >= 0", (long long)args->step);
  KX_REQUIRE(args->length_penalty >= 0.0f, "kx_beam_step: length_penalty=%g must be >= 0", (double)args->length_penalty);
  KX_REQUIRE(args->Win == args->W || (const void*)args->scores_in != (const void*)args->scores_out,
             "kx_beam_step: scores_in and scores_out may be one buffer only when Win == W");
  if (args->V > KX_BEAM_MAX_V) {
    kx_set_error("kx_beam_step: V=%lld exceeds %lld (64-bit fixed-point mass)", (long long)args->V, KX_BEAM_MAX_V);
    return KX_ERR_UNSUPPORTED;
  }
  BeamParams p;
  p.logits = args->logits; p.ld = args->ld; p.B = (int)args->B; p.Win = (int)args->Win; p.W = (int)args->W; p.V = (int)args->V;
  p.K = 2 * p.W; p.step = (int)args->step; p.early = args->early_stopping ? 1 : 0;
  p.alpha = args->length_penalty; p.eos = args->eos_id; p.pad = args->pad_id;
  p.s_in = args->scores_in; p.s_out = args->scores_out; p.next = (long long*)args->next_token; p.parent = args->parent;
  p.src_row = args->src_row;
  p.pool_score = args->pool_score; p.pool_end = args->pool_end; p.pool_parent = args->pool_parent;
  p.pool_count = args->pool_count; p.done = args->done; p.scratch = (unsigned long long*)args->scratch;
  KxProfScope prof(KX_K_MISC, args->B * args->Win, args->V, args->W, (hipStream_t)stream);
  hipLaunchKernelGGL(rank_kernel, dim3((unsigned)(p.B * p.Win)), dim3(SB), 0, (hipStream_t)stream, p);
  KX_CHECK_LAUNCH("kx_beam_step (rank)");
  hipLaunchKernelGGL(merge_kernel, dim3((unsigned)p.B), dim3(MERGE_T), 0, (hipStream_t)stream, p);
  KX_CHECK_LAUNCH("kx_beam_step (merge)");
  return KX_OK;
}

extern "C" int kx_beam_finalize(const float* scores_live, const uint8_t* done, float* pool_score, int32_t* pool_end,
                                int32_t* pool_parent, int32_t* pool_count, const int32_t* parent, const int64_t* token,
                                int64_t trace_ld, int64_t B, int64_t W, int64_t R, int64_t n, float length_penalty, int64_t eos_id,
                                int64_t pad_id, int64_t* out_tokens, int64_t out_ld, float* out_scores, void* stream) {
  KX_REQUIRE(scores_live && done && pool_score && pool_end && pool_parent && pool_count && parent && token && out_tokens &&
             out_scores, "kx_beam_finalize: null pointer");
  KX_REQUIRE(W >= 1 && W <= BEAM_MAX_W, "kx_beam_finalize: W=%lld outside [1, %d]", (long long)W, BEAM_MAX_W);
  KX_REQUIRE(R >= 1 && R <= W, "kx_beam_finalize: R=%lld outside [1, W=%lld]", (long long)R, (long long)W);
  KX_REQUIRE(B >= 1 && B * W <= 0x7fffffffll, "kx_beam_finalize: B=%lld must be >= 1", (long long)B);
  KX_REQUIRE(n >= 1 && n <= 0x7fffffffll && out_ld >= n, "kx_beam_finalize: n=%lld must be in [1, out_ld=%lld]", (long long)n,
             (long long)out_ld);
  KX_REQUIRE(trace_ld >= B * W, "kx_beam_finalize: trace_ld=%lld is smaller than B*W=%lld", (long long)trace_ld,
             (long long)(B * W));
  KX_REQUIRE(length_penalty >= 0.0f, "kx_beam_finalize: length_penalty=%g must be >= 0", (double)length_penalty);
  KxProfScope prof(KX_K_MISC, B, W, R, (hipStream_t)stream);
  hipLaunchKernelGGL(finalize_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, scores_live, done, pool_score, pool_end,
                     pool_parent, pool_count, parent, (const long long*)token, (long long)trace_ld, (int)W, (int)R, (int)n,
                     length_penalty, (long long)eos_id, (long long)pad_id, (long long*)out_tokens, (long long)out_ld, out_scores);
  KX_CHECK_LAUNCH("kx_beam_finalize");
  return KX_OK;
}

extern "C" int kx_kv_cache_gather(const void* src_k, const void* src_v, void* dst_k, void* dst_v, int64_t L, int64_t B_src,
                                  int64_t B_dst, int64_t heads, int64_t Tmax, int64_t t, int32_t elem_bytes,
                                  const int32_t* src_row, int32_t* error_word, void* stream) {
  KX_REQUIRE(src_k && src_v && dst_k && dst_v && src_row && error_word, "kx_kv_cache_gather: null pointer");
  KX_REQUIRE(elem_bytes == 2 || elem_bytes == 4, "kx_kv_cache_gather: elem_bytes=%d must be 2 or 4", (int)elem_bytes);
  KX_REQUIRE(L >= 1 && B_src >= 1 && B_dst >= 1 && heads >= 1 && Tmax >= 1 && B_src <= 0x7fffffffll && B_dst <= 0x7fffffffll &&
             heads <= 0x7fffffffll, "kx_kv_cache_gather: bad shape L=%lld B_src=%lld B_dst=%lld heads=%lld Tmax=%lld", (long long)L,
             (long long)B_src, (long long)B_dst, (long long)heads, (long long)Tmax);
  KX_REQUIRE(t >= 0 && t <= Tmax, "kx_kv_cache_gather: t=%lld outside [0, Tmax=%lld]", (long long)t, (long long)Tmax);
  KX_REQUIRE((((uintptr_t)src_k | (uintptr_t)src_v | (uintptr_t)dst_k | (uintptr_t)dst_v) & 15) == 0,
             "kx_kv_cache_gather: pointers must be 16-byte aligned");
  const size_t pos_bytes = (size_t)64 * elem_bytes;
  const size_t sn = (size_t)L * B_src * heads * Tmax * pos_bytes, dn = (size_t)L * B_dst * heads * Tmax * pos_bytes;
  KX_REQUIRE(!ranges_overlap(src_k, sn, dst_k, dn) && !ranges_overlap(src_k, sn, dst_v, dn) &&
             !ranges_overlap(src_v, sn, dst_k, dn) && !ranges_overlap(src_v, sn, dst_v, dn) && !ranges_overlap(dst_k, dn, dst_v, dn),
             "kx_kv_cache_gather: src and dst caches overlap (the gather is not an in-place permutation)");
  if (t == 0) return KX_OK;
  // head-major [heads][Tmax][64]: one chunk per (layer, sequence, head); tuning key 9 = 1, [Tmax][heads*64]: the first t rows
  // of heads*64 elements are ONE contiguous chunk per (layer, sequence)
  const bool head_major = kx_tuning_get(KX_TUNE_CACHE_LAYOUT) != 1;
  const long long chunks = head_major ? heads : 1;
  const long long vpp = (long long)(pos_bytes / 16) * (head_major ? 1 : heads);
  const long long row_vecs = Tmax * vpp, copy_vecs = t * vpp, total = L * B_dst * chunks * copy_vecs;
  const long long blocks = (total + 255) / 256;
  KxProfScope prof(KX_K_MISC, L * B_dst * heads, t, elem_bytes, (hipStream_t)stream);
  hipLaunchKernelGGL(kv_gather_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, (hipStream_t)stream,
                     (const uint4*)src_k, (const uint4*)src_v, (uint4*)dst_k, (uint4*)dst_v, (const int*)src_row, (int)B_src,
                     (int)B_dst, (int)chunks, row_vecs, copy_vecs, total, (int*)error_word);
  KX_CHECK_LAUNCH("kx_kv_cache_gather");
  return KX_OK;
}
