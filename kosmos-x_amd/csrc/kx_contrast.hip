// Contrastive search on the device: the degeneration penalty and the choice (kx_contrast_select) and the commit of the chosen
// candidate's K/V row (kx_kv_cache_commit).  Contract: include/kosmosx_hip.h, "Contrastive search on the device".
// (kx_contrast_candidates shares kx_step_logprobs' selection and lives next to it in kx_rowops.hip; kx_contrast_hidden reads the
// decode step's workspace plan and lives next to the step in kx_forward.hip.)
#include "kx_common.h"

namespace {

constexpr int CS_THREADS = 512;                   // 8 waves per workgroup
constexpr int CS_WAVES = CS_THREADS / 64;
constexpr int CS_CHUNK = 32;                      // history rows per workgroup: 4 per wave (a row is D * 4 bytes: 8 KB at D = 2048)

// Partial maxima.  Workgroup (c, b) owns history rows [c * CS_CHUNK, min((c + 1) * CS_CHUNK, P_b)) of sequence b.  It stages the
// sequence's k candidate vectors once (k * D * 4 bytes of LDS: 128 KB at k = 16, D = 2048, one workgroup per CU; 32 KB at k = 4, five),
// then every wave walks its rows: a lane reads 16 bytes of the row per iteration (vector v = lane, lane + 64, ...) and the same
// vector of each candidate from LDS (lane-consecutive 16-byte reads: conflict-free) and keeps k accumulators
//   acc_j = fma(h.w, c.w, fma(h.z, c.z, fma(h.y, c.y, fma(h.x, c.x, acc_j))))   over its vectors in ascending order,
// then the 64 lanes' sums are combined by a butterfly (xor 32, 16, 8, 4, 2, 1): the order of every addition is a function of D
// alone — not of the chunk, the grid, B, k, or where the row or the candidate sits.  The maximum over rows is exact in any order.
// No workgroup waits on another; nothing is atomic.
template <int KC>
__global__ __launch_bounds__(CS_THREADS) void contrast_partial_kernel(const float* __restrict__ u, const float* __restrict__ history,
                                                                      const int* __restrict__ hist_rows, long long p_stride,
                                                                      const unsigned char* __restrict__ finished, int k, int D,
                                                                      long long cap, int chunks_ld, float* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) float cand[];           // [k][D]
  __shared__ float wmax[CS_WAVES][KC];
  const int tid = threadIdx.x, b = blockIdx.y, c = blockIdx.x;
  if (finished && finished[b]) return;                                    // (uniform over the workgroup: nobody reaches a barrier)
  const long long p = hist_rows[(long long)b * p_stride];
  if (p < 1 || p >= cap) return;                                          // the choosing launch reports it
  const long long r0 = (long long)c * CS_CHUNK;
  if (r0 >= p) return;
  const long long r1 = r0 + CS_CHUNK < p ? r0 + CS_CHUNK : p;
  const int D4 = D >> 2;
  const float4* us = reinterpret_cast<const float4*>(u + (size_t)b * k * D);
  float4* cs = reinterpret_cast<float4*>(cand);
  for (int i = tid; i < k * D4; i += CS_THREADS) cs[i] = us[i];
  __syncthreads();
  const int wave = tid >> 6, lane = tid & 63;
  float m[KC];
#pragma unroll
  for (int j = 0; j < KC; ++j) m[j] = -INFINITY;
  for (long long r = r0 + wave; r < r1; r += CS_WAVES) {
    const float4* h = reinterpret_cast<const float4*>(history + ((size_t)b * cap + r) * D);
    float acc[KC];
#pragma unroll
    for (int j = 0; j < KC; ++j) acc[j] = 0.f;
    for (int v = lane; v < D4; v += 64) {
      const float4 hv = h[v];
#pragma unroll
      for (int j = 0; j < KC; ++j) {
        if (j < k) {
          const float4 cv = cs[j * D4 + v];
          acc[j] = fmaf(hv.w, cv.w, fmaf(hv.z, cv.z, fmaf(hv.y, cv.y, fmaf(hv.x, cv.x, acc[j]))));
        }
      }
    }
#pragma unroll
    for (int j = 0; j < KC; ++j) {
      float a = acc[j];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
      m[j] = a > m[j] ? a : m[j];                                         // (a NaN dot product never becomes the maximum)
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < KC; ++j) wmax[wave][j] = m[j];
  }
  __syncthreads();
  if (tid < k) {
    float best = wmax[0][tid];
#pragma unroll
    for (int w = 1; w < CS_WAVES; ++w) best = wmax[w][tid] > best ? wmax[w][tid] : best;
    partial[((size_t)b * chunks_ld + c) * k + tid] = best;
  }
}

// The choice: one workgroup per sequence.  penalty_j = the maximum of the sequence's ceil(P / CS_CHUNK) partial maxima,
// score_j = one_minus_alpha * p_j - alpha * penalty_j as two products and one difference, each rounded on its own; the largest
// score wins, the lowest j among equal ones, a NaN loses to every number.  Then the chosen unit vector is appended to the history.
__global__ __launch_bounds__(256) void contrast_choose_kernel(const float* __restrict__ u, const float* __restrict__ prob,
                                                              float* __restrict__ history, const int* __restrict__ hist_rows,
                                                              long long p_stride, int* __restrict__ hist_len, int k, int D, long long cap,
                                                              int chunks_ld, const float* __restrict__ partial, float alpha,
                                                              float one_minus_alpha, const long long* __restrict__ step_tokens,
                                                              unsigned char* __restrict__ finished, long long eos, long long pad,
                                                              long long* __restrict__ next_token, int* __restrict__ chosen,
                                                              long long* __restrict__ out_tokens, long long out_ld, long long out_col,
                                                              float* __restrict__ cand_penalty, int* __restrict__ chosen_trace,
                                                              int* __restrict__ err) {
  __shared__ float pen[16], score[16];
  __shared__ int pick;
  const int tid = threadIdx.x;
  const long long b = blockIdx.x;
  if (finished[b]) {                                                      // a finished row emits the pad token and nothing else
    if (tid == 0) {
      next_token[b] = pad;
      if (out_tokens) out_tokens[b * out_ld + out_col] = pad;
    }
    return;
  }
  const long long p = hist_rows[b * p_stride];
  if (p < 1 || p >= cap) {                                                // no history to compare with, or no row to append to
    if (tid == 0) atomicOr(err, KX_RAGGED_ERR_CACHE);
    return;
  }
  if (tid < k) {
    const int nch = (int)((p + CS_CHUNK - 1) / CS_CHUNK);
    float m = -INFINITY;
    for (int c = 0; c < nch; ++c) {
      const float v = partial[((size_t)b * chunks_ld + c) * k + tid];
      m = v > m ? v : m;
    }
    pen[tid] = m;
    score[tid] = __fsub_rn(__fmul_rn(one_minus_alpha, prob[b * k + tid]), __fmul_rn(alpha, m));
  }
  __syncthreads();
  if (tid == 0) {
    int best = 0;
    float bs = score[0];
    for (int j = 1; j < k; ++j) {
      const float s = score[j];
      if ((s == s) && (!(bs == bs) || s > bs)) { best = j; bs = s; }
    }
    pick = best;
  }
  __syncthreads();
  const int j = pick;
  const float4* src = reinterpret_cast<const float4*>(u + ((size_t)b * k + j) * D);
  float4* dst = reinterpret_cast<float4*>(history + ((size_t)b * cap + p) * D);
  for (int v = tid; v < (D >> 2); v += 256) dst[v] = src[v];
  if (tid < k && cand_penalty) cand_penalty[(b * out_ld + out_col) * k + tid] = pen[tid];
  if (tid == 0) {
    const long long tok = step_tokens[b * k + j];
    next_token[b] = tok;
    chosen[b] = j;
    hist_len[b] = (int)p + 1;
    if (out_tokens) out_tokens[b * out_ld + out_col] = tok;
    if (chosen_trace) chosen_trace[b * out_ld + out_col] = j;
    if (eos >= 0 && tok == eos) finished[b] = 1;
  }
}

// Commit: one workgroup per sequence copies tail row 0 of row b * k + chosen[b] to cache row P_b, every layer and head, both caches,
// one 16-byte vector per thread and iteration; every thread has read P_b before the barrier behind which thread 0 moves it on
// (all k copies: the step reads positions[b * k + j]).
__global__ __launch_bounds__(1024) void kv_commit_kernel(const uint4* __restrict__ kt, const uint4* __restrict__ vt, uint4* __restrict__ kc,
                                                         uint4* __restrict__ vc, int L, int B, int k, int heads, long long Tmax,
                                                         long long Ttail, int vp, int head_major, const int* __restrict__ chosen,
                                                         int* __restrict__ positions, const unsigned char* __restrict__ finished,
                                                         int* __restrict__ err) {
  const int b = blockIdx.x, tid = threadIdx.x;
  if (finished && finished[b]) return;
  const int j = chosen[b];
  const long long p = positions[(long long)b * k];
  if (j < 0 || j >= k || p < 0 || p >= Tmax) {                            // the caller's error: nothing is read or written
    if (tid == 0) atomicOr(err, KX_RAGGED_ERR_COMMIT);
    return;
  }
  const long long M = (long long)B * k, r = (long long)b * k + j;
  const int per_layer = heads * vp;
  for (int idx = tid; idx < L * per_layer; idx += 1024) {
    const int l = idx / per_layer, rem = idx - l * per_layer, h = rem / vp, o = rem - h * vp;
    long long si, di;
    if (head_major) {
      si = ((l * M + r) * heads + h) * Ttail * vp + o;
      di = (((long long)l * B + b) * heads + h) * Tmax * vp + p * vp + o;
    } else {
      si = (l * M + r) * Ttail * per_layer + rem;
      di = (((long long)l * B + b) * Tmax + p) * per_layer + rem;
    }
    kc[di] = kt[si];
    vc[di] = vt[si];
  }
  __syncthreads();
  if (tid < k) positions[(long long)b * k + tid] = (int)p + 1;
}

bool spans_overlap(const void* a, size_t an, const void* b, size_t bn) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + bn && y < x + an;
}

}  // namespace

extern "C" size_t kx_contrast_scratch_bytes(int64_t B, int32_t k, int64_t cap) {
  if (B < 1 || k < 1 || cap < 1) return 0;
  return (size_t)B * (size_t)((cap + CS_CHUNK - 1) / CS_CHUNK) * (size_t)k * sizeof(float);
}

extern "C" int kx_contrast_select(const float* u, const float* prob, float* history, int64_t B, int32_t k, int64_t D, int64_t cap,
                                  const int32_t* hist_rows, int64_t p_stride, int32_t* hist_len, float alpha, float one_minus_alpha,
                                  const int64_t* step_tokens, uint8_t* finished, int64_t eos_id, int64_t pad_id, int64_t* next_token,
                                  int32_t* chosen, int64_t* out_tokens, int64_t out_ld, int64_t out_col, float* cand_penalty,
                                  int32_t* chosen_trace, float* scratch, size_t scratch_bytes, int32_t* error_word, void* stream) {
  KX_REQUIRE(u && prob && history, "kx_contrast_select: null u / prob / history");
  KX_REQUIRE(hist_rows && hist_len, "kx_contrast_select: null hist_rows / hist_len");
  KX_REQUIRE(step_tokens && finished && next_token && chosen, "kx_contrast_select: null step_tokens / finished / next_token / chosen");
  KX_REQUIRE(scratch && error_word, "kx_contrast_select: null scratch / error_word");
  KX_REQUIRE(k >= 1 && k <= 16, "kx_contrast_select: k=%d outside 1..16", (int)k);
  KX_REQUIRE(B >= 1 && B <= 65535, "kx_contrast_select: B=%lld outside 1..65535", (long long)B);
  KX_REQUIRE(D >= 4 && D % 4 == 0 && D <= 0x7fffffffll / 16 && (size_t)k * D * 4 <= 128 * 1024,
             "kx_contrast_select: D=%lld must be a multiple of 4 with k * D * 4 <= 128 KB of LDS (k=%d)", (long long)D, (int)k);
  KX_REQUIRE(cap >= 2 && cap <= 0x7fffffffll, "kx_contrast_select: cap=%lld outside 2..2^31-1 history rows", (long long)cap);
  KX_REQUIRE(p_stride >= 1, "kx_contrast_select: p_stride=%lld must be >= 1", (long long)p_stride);
  KX_REQUIRE(alpha >= 0.f && alpha <= 1.f && one_minus_alpha >= 0.f && one_minus_alpha <= 1.f,
             "kx_contrast_select: alpha=%g / one_minus_alpha=%g outside [0, 1]", (double)alpha, (double)one_minus_alpha);
  KX_REQUIRE(!(out_tokens || cand_penalty || chosen_trace) || (out_col >= 0 && out_col < out_ld),
             "kx_contrast_select: out_col=%lld outside [0, out_ld=%lld)", (long long)out_col, (long long)out_ld);
  KX_REQUIRE((((uintptr_t)u | (uintptr_t)history) & 15) == 0, "kx_contrast_select: u and history must be 16-byte aligned");
  KX_REQUIRE(!spans_overlap(u, (size_t)B * k * D * 4, history, (size_t)B * cap * D * 4), "kx_contrast_select: u and history overlap");
  const size_t need = kx_contrast_scratch_bytes(B, k, cap);
  KX_REQUIRE(scratch_bytes >= need, "kx_contrast_select: scratch of %zu bytes is smaller than kx_contrast_scratch_bytes = %zu", scratch_bytes,
             need);
  hipStream_t s = (hipStream_t)stream;
  const int chunks = (int)((cap + CS_CHUNK - 1) / CS_CHUNK);
  KX_REQUIRE(chunks <= 0x7fffffff / 16, "kx_contrast_select: cap=%lld has too many chunks", (long long)cap);
  const size_t lds = (size_t)k * D * 4;
  static bool lds_raised = false;                     // (more than 64 KB of dynamic LDS must be asked for once per kernel)
  if (!lds_raised) {
    (void)hipFuncSetAttribute((const void*)contrast_partial_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
    (void)hipFuncSetAttribute((const void*)contrast_partial_kernel<8>, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
    (void)hipFuncSetAttribute((const void*)contrast_partial_kernel<16>, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
    lds_raised = true;
  }
  {
    KxProfScope prof(KX_K_MISC, B * k, cap, D, s);
    const dim3 grid((unsigned)chunks, (unsigned)B), block(CS_THREADS);
#define KX_CONTRAST_PARTIAL(KC)                                                                                              \
  hipLaunchKernelGGL(contrast_partial_kernel<KC>, grid, block, lds, s, u, (const float*)history, (const int*)hist_rows,       \
                     (long long)p_stride, (const unsigned char*)finished, (int)k, (int)D, (long long)cap, chunks, scratch)
    if (k <= 4) KX_CONTRAST_PARTIAL(4);
    else if (k <= 8) KX_CONTRAST_PARTIAL(8);
    else KX_CONTRAST_PARTIAL(16);
#undef KX_CONTRAST_PARTIAL
    KX_CHECK_LAUNCH("kx_contrast_select (partial maxima)");
  }
  KxProfScope prof(KX_K_MISC, B, k, D, s);
  hipLaunchKernelGGL(contrast_choose_kernel, dim3((unsigned)B), dim3(256), 0, s, u, prob, history, (const int*)hist_rows,
                     (long long)p_stride, (int*)hist_len, (int)k, (int)D, (long long)cap, chunks, (const float*)scratch, alpha,
                     one_minus_alpha, (const long long*)step_tokens, finished, (long long)eos_id, (long long)pad_id,
                     (long long*)next_token, (int*)chosen, (long long*)out_tokens, (long long)out_ld, (long long)out_col, cand_penalty,
                     (int*)chosen_trace, (int*)error_word);
  KX_CHECK_LAUNCH("kx_contrast_select (choice)");
  return KX_OK;
}

extern "C" int kx_kv_cache_commit(const void* ktail, const void* vtail, void* kcache, void* vcache, int64_t L, int64_t B, int32_t k,
                                  int64_t heads, int64_t Tmax, int64_t Ttail, int32_t elem_bytes, const int32_t* chosen,
                                  int32_t* positions, const uint8_t* finished, int32_t* error_word, void* stream) {
  KX_REQUIRE(ktail && vtail && kcache && vcache, "kx_kv_cache_commit: null ktail / vtail / kcache / vcache");
  KX_REQUIRE(chosen && positions && error_word, "kx_kv_cache_commit: null chosen / positions / error_word");
  KX_REQUIRE(elem_bytes == 2 || elem_bytes == 4, "kx_kv_cache_commit: elem_bytes=%d must be 2 or 4", (int)elem_bytes);
  KX_REQUIRE(k >= 1 && k <= 16, "kx_kv_cache_commit: k=%d outside 1..16", (int)k);
  KX_REQUIRE(L >= 1 && B >= 1 && heads >= 1 && Tmax >= 1 && Ttail >= 1 && B <= 65535 && Tmax <= 0x7fffffffll && Ttail <= 0x7fffffffll &&
             L * heads * 16 <= 0x7fffffffll, "kx_kv_cache_commit: bad shape L=%lld B=%lld heads=%lld Tmax=%lld Ttail=%lld", (long long)L,
             (long long)B, (long long)heads, (long long)Tmax, (long long)Ttail);
  KX_REQUIRE((((uintptr_t)ktail | (uintptr_t)vtail | (uintptr_t)kcache | (uintptr_t)vcache) & 15) == 0,
             "kx_kv_cache_commit: pointers must be 16-byte aligned");
  const size_t pos_bytes = (size_t)64 * elem_bytes;
  const size_t tn = (size_t)L * B * k * heads * Ttail * pos_bytes, cn = (size_t)L * B * heads * Tmax * pos_bytes;
  KX_REQUIRE(!spans_overlap(ktail, tn, kcache, cn) && !spans_overlap(ktail, tn, vcache, cn) && !spans_overlap(vtail, tn, kcache, cn) &&
             !spans_overlap(vtail, tn, vcache, cn) && !spans_overlap(kcache, cn, vcache, cn) && !spans_overlap(ktail, tn, vtail, tn),
             "kx_kv_cache_commit: the tail caches and the caches overlap");
  const bool head_major = kx_tuning_get(KX_TUNE_CACHE_LAYOUT) != 1;      // per sequence [heads][T][64]; tuning key 9 = 1: [T][heads * 64]
  KxProfScope prof(KX_K_MISC, L * B * heads, 1, elem_bytes, (hipStream_t)stream);
  hipLaunchKernelGGL(kv_commit_kernel, dim3((unsigned)B), dim3(1024), 0, (hipStream_t)stream, (const uint4*)ktail, (const uint4*)vtail,
                     (uint4*)kcache, (uint4*)vcache, (int)L, (int)B, (int)k, (int)heads, (long long)Tmax, (long long)Ttail,
                     (int)(pos_bytes / 16), head_major ? 1 : 0, (const int*)chosen, (int*)positions, finished, (int*)error_word);
  KX_CHECK_LAUNCH("kx_kv_cache_commit");
  return KX_OK;
}
