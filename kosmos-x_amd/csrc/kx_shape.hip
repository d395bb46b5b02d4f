// Logit shaping (kx_shape_logits): the request fields a completion API passes straight through — a per-id logit bias and the
// presence / frequency penalties over the tokens THIS call emitted — applied in place to the fp32 logits row the sampler is about
// to read, after the constraint and automaton launches.  Contract: include/kosmosx_hip.h.
//
// One launch, 256-thread workgroups, one per (row, slice of SLICE ids), and no hand-off between workgroups: the thread that owns
// element i is the only one that reads or writes counts[b, i] and logits[b, i].  Every workgroup of a row reads the row's last token
// (one uniform load); the count of id i as this launch sees it is c = stored + (i == last), stored back by the owner of i alone.
// The bias entries of the row that fall into the slice (two lower bounds over the row's ascending ids find them) are applied one per
// thread, then — behind a barrier, because a bias entry's thread is not its element's penalty-pass thread — consecutive lanes walk
// consecutive ids for the penalty.  Every operation on a logit is a single IEEE fp32 add, multiply or subtract (contraction is off
// in this file's kernel), so a numpy float32 restatement matches bit for bit.  Every value read from device memory that becomes an
// index (last_token, bias ids, offsets) is range-checked first: a malformed table changes what is shaped, never what is addressed.
#include "kx_common.h"

namespace {

constexpr int HB = 256;                  // threads per workgroup
constexpr int SLICE = 4096;              // ids per workgroup: 16 elements per thread in the penalty pass
constexpr long long KX_SHAPE_MAX_V = 1ll << 23;   // kx_sample_logits' own limit: the kernel that reads the row next

struct ShapeParams {
  float* logits; long long ld; int V;
  const int* bias_off; const int* bias_ids; const float* bias_val; int E;
  int* counts; float f, p;
  const float* f_rows; const float* p_rows;             // kx_shape_logits_rows: row b's own f / p (NULL: the scalar)
  const long long* last_token; const unsigned char* finished;
  int slices;
};

// first k in [lo, hi) with ids[k] >= v (hi if none); stays inside [lo, hi) whatever the array holds
__device__ __forceinline__ int lower_bound(const int* __restrict__ ids, int lo, int hi, int v) {
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (ids[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(HB) void shape_kernel(const ShapeParams a) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x;
  const int b = blockIdx.x / a.slices;                  // (B * slices < 2^31: checked on the host)
  const int slice = blockIdx.x - b * a.slices;
  if (a.finished && a.finished[b]) return;              // (uniform: one byte, read by every thread) logits and counts stay as they are
  const int v0 = slice * SLICE;
  const int n = min(a.V - v0, SLICE);                   // ids of this slice (>= 1)
  float* __restrict__ row = a.logits + (long long)b * a.ld + v0;
  const float ninf = -__builtin_inff();

  // 1. the bias entries of this slice: l = l + value; a logit that is -inf or NaN stays what it is, bit for bit
  if (a.bias_off) {
    int lo = min(max(a.bias_off[b], 0), a.E);           // offsets clamped into [0, E], out of order = none
    int hi = min(max(a.bias_off[b + 1], 0), a.E);
    if (hi < lo) hi = lo;
    const int k0 = lower_bound(a.bias_ids, lo, hi, v0);
    const int k1 = lower_bound(a.bias_ids, k0, hi, v0 + n);
    for (int k = k0 + tid; k < k1; k += HB) {
      const int i = a.bias_ids[k] - v0;
      if (i < 0 || i >= n) continue;                    // (an id outside the slice or the vocabulary: compared, never an index)
      const float l = row[i];
      if (l > ninf) row[i] = l + a.bias_val[k];
    }
  }
  if (!a.counts) return;
  __syncthreads();

  // 2. the counts of the tokens this call emitted, then the penalty where the count is positive
  int last = -1;                                        // the slice-local index of the token the last sampler launch emitted
  if (a.last_token) {
    const long long t = a.last_token[b];
    if (t >= v0 && t < v0 + n) last = (int)(t - v0);
  }
  int* __restrict__ cnt = a.counts + (long long)b * a.V + v0;
  const float f = a.f_rows ? a.f_rows[b] : a.f;         // (uniform: one word per array, read by every thread)
  const float p = a.p_rows ? a.p_rows[b] : a.p;
  for (int i = tid; i < n; i += HB) {
    int c = cnt[i];
    if (i == last) { c += 1; cnt[i] = c; }
    if (c > 0) {
      const float l = row[i];
      if (l > ninf) {
        const float t = f * (float)c;
        const float u = l - t;
        row[i] = u - p;
      }
    }
  }
}

}  // namespace

static int shape_impl(const kx_shape_args* args, const float* frequency_rows, const float* presence_rows, void* stream) {
  KX_REQUIRE(args != nullptr, "kx_shape_logits: null args");
  KX_REQUIRE(args->struct_bytes == sizeof(kx_shape_args),
             "kx_shape_logits: stale binding — caller declares kx_shape_args as %u bytes, this library (ABI %d) as %zu",
             (unsigned)args->struct_bytes, KX_ABI_VERSION, sizeof(kx_shape_args));
  KX_REQUIRE(args->logits != nullptr, "kx_shape_logits: null logits");
  KX_REQUIRE(args->B >= 1 && args->B <= 0x7fffffffll, "kx_shape_logits: B=%lld must be >= 1", (long long)args->B);
  KX_REQUIRE(args->V >= 1, "kx_shape_logits: V=%lld must be >= 1", (long long)args->V);
  KX_REQUIRE(args->ld >= args->V, "kx_shape_logits: ld=%lld is smaller than V=%lld", (long long)args->ld, (long long)args->V);
  if (args->V > KX_SHAPE_MAX_V) {
    kx_set_error("kx_shape_logits: V=%lld exceeds %lld (the limit of kx_sample_logits, which reads the row next)",
                 (long long)args->V, KX_SHAPE_MAX_V);
    return KX_ERR_UNSUPPORTED;
  }
  const long long slices = (args->V + SLICE - 1) / SLICE;
  if (args->B * slices > 0x7fffffffll) {
    kx_set_error("kx_shape_logits: B=%lld rows x %lld slices of %d ids exceed one launch's 2^31 - 1 workgroups", (long long)args->B,
                 slices, SLICE);
    return KX_ERR_UNSUPPORTED;
  }
  KX_REQUIRE(args->n_bias >= 0, "kx_shape_logits: n_bias=%lld must be >= 0", (long long)args->n_bias);
  if (args->n_bias > 0x7fffffffll) {
    kx_set_error("kx_shape_logits: n_bias=%lld must be below 2^31", (long long)args->n_bias);
    return KX_ERR_UNSUPPORTED;
  }
  KX_REQUIRE(args->bias_off != nullptr || args->n_bias == 0, "kx_shape_logits: null bias_off with n_bias=%lld", (long long)args->n_bias);
  KX_REQUIRE(args->n_bias == 0 || args->bias_ids != nullptr, "kx_shape_logits: null bias_ids with n_bias=%lld", (long long)args->n_bias);
  KX_REQUIRE(args->n_bias == 0 || args->bias_val != nullptr, "kx_shape_logits: null bias_val with n_bias=%lld", (long long)args->n_bias);
  // (x - x == 0 holds for finite values only)
  KX_REQUIRE(args->frequency - args->frequency == 0.0f, "kx_shape_logits: frequency=%g must be finite", (double)args->frequency);
  KX_REQUIRE(args->presence - args->presence == 0.0f, "kx_shape_logits: presence=%g must be finite", (double)args->presence);
  KX_REQUIRE(args->counts != nullptr || (args->frequency == 0.0f && args->presence == 0.0f),
             "kx_shape_logits: null counts with frequency=%g, presence=%g", (double)args->frequency, (double)args->presence);
  KX_REQUIRE(args->counts != nullptr || (frequency_rows == nullptr && presence_rows == nullptr),
             "kx_shape_logits_rows: null counts with per-row penalties");
  KX_REQUIRE(args->counts != nullptr || args->bias_off != nullptr, "kx_shape_logits: neither bias_off nor counts: nothing to shape");
  ShapeParams p;
  p.logits = args->logits; p.ld = args->ld; p.V = (int)args->V;
  p.bias_off = args->bias_off; p.bias_ids = args->bias_ids; p.bias_val = args->bias_val; p.E = (int)args->n_bias;
  p.counts = args->counts; p.f = args->frequency; p.p = args->presence;
  p.f_rows = frequency_rows; p.p_rows = presence_rows;
  p.last_token = (const long long*)args->last_token; p.finished = args->finished;
  p.slices = (int)slices;
  KxProfScope prof(KX_K_MISC, args->B, args->V, 4, (hipStream_t)stream);
  hipLaunchKernelGGL(shape_kernel, dim3((unsigned)(args->B * slices)), dim3(HB), 0, (hipStream_t)stream, p);
  KX_CHECK_LAUNCH("kx_shape_logits");
  return KX_OK;
}

extern "C" int kx_shape_logits(const kx_shape_args* args, void* stream) { return shape_impl(args, nullptr, nullptr, stream); }

// Row b's f / p from the arrays (either may be NULL: the scalar); both NULL: kx_shape_logits' launch.
extern "C" int kx_shape_logits_rows(const kx_shape_args* args, const float* frequency_rows, const float* presence_rows, void* stream) {
  return shape_impl(args, frequency_rows, presence_rows, stream);
}
