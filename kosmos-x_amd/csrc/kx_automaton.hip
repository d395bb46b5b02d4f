// Token-automaton constrained decoding (kx_automaton_step): every row carries a state of a caller-compiled automaton over token ids;
// one launch advances the state on the token the sampler (or the beam step) just left on the device and bans, in the fp32 logits row
// that kernel is about to read, every id the new state does not allow.  Contract: include/kosmosx_hip.h.
//
// A banned id's logit becomes -inf and nothing else is written, as in kx_constrain_logits: the sampler never selects -inf (its rule
// 6), to the beam step -inf is never a candidate, and a row with every id banned emits pad and is finished.  The logits are never read.
//
// One launch, 256-thread workgroups, one per (row, slice of SLICE ids).  Every workgroup of a row repeats the row's advance — a few
// uniform loads and one binary search over the state's sorted edges — and workgroup 0 of the row writes state_out[b]; state_in and
// state_out do not overlap (checked on the host), so nobody reads what another workgroup writes.  The slice's allowed set is a bitmap
// in LDS: filled from the state's default, then threads stride over the state's edges that fall into the slice (two lower bounds find
// them) and set or clear their bits with LDS atomics; after the barrier consecutive lanes store -inf to consecutive banned ids.
// Every value read from device memory (states, src_row, offsets, edge ids, next states) is range-checked before it is used as an
// index: a malformed table changes what is banned, never what is addressed.
#include "kx_common.h"

namespace {

constexpr int AB = 256;                  // threads per workgroup
constexpr int SLICE = 4096;              // ids per workgroup: 128 bitmap words, 16 stores per thread when the whole slice is banned
constexpr long long KX_AUTOMATON_MAX_V = 1ll << 23;   // kx_sample_logits' own limit: the kernel that reads the row next

struct AutomatonParams {
  float* logits; long long ld; int V;
  const int* edge_off; const int* edge_tok; const int* edge_next; const int* default_next;
  int S, E;
  const int* state_in; int B_in; int* state_out;
  const int* src_row; const long long* last_token; const unsigned char* finished;
  int slices;
};

// first k in [lo, hi) with tok[k] >= v (hi if none); stays inside [lo, hi) whatever the array holds
__device__ __forceinline__ int lower_bound(const int* __restrict__ tok, int lo, int hi, int v) {
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (tok[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(AB) void automaton_kernel(const AutomatonParams a) {
  __shared__ unsigned bits[SLICE / 32];
  const int tid = threadIdx.x;
  const int b = blockIdx.x / a.slices;                  // (B * slices < 2^31: checked on the host)
  const int slice = blockIdx.x - b * a.slices;

  // 1. the state the row comes from; anything out of range is the dead state
  int from = a.src_row ? a.src_row[b] : b;
  int s = (from >= 0 && from < a.B_in) ? a.state_in[from] : -1;
  if (s < 0 || s >= a.S) s = -1;
  // 2. a finished row carries its state over and keeps its logits
  if (a.finished && a.finished[b]) {                    // (uniform: one byte, read by every thread)
    if (slice == 0 && tid == 0) a.state_out[b] = s;
    return;
  }
  // the state's edges [lo, hi): offsets clamped into [0, E], out of order = none
  int lo = 0, hi = 0;
  if (s >= 0) {
    lo = min(max(a.edge_off[s], 0), a.E);
    hi = min(max(a.edge_off[s + 1], 0), a.E);
    if (hi < lo) hi = lo;
  }
  // 3. advance on the token just emitted (uniform over the workgroup, repeated by every workgroup of the row)
  if (a.last_token && s >= 0) {
    const long long t = a.last_token[b];
    int nx = -1;
    if (t >= 0 && t < a.V) {
      const int k = lower_bound(a.edge_tok, lo, hi, (int)t);
      nx = (k < hi && a.edge_tok[k] == (int)t) ? a.edge_next[k] : a.default_next[s];
    }
    s = (nx >= 0 && nx < a.S) ? nx : -1;
    lo = hi = 0;
    if (s >= 0) {
      lo = min(max(a.edge_off[s], 0), a.E);
      hi = min(max(a.edge_off[s + 1], 0), a.E);
      if (hi < lo) hi = lo;
    }
  }
  // 4.
  if (slice == 0 && tid == 0) a.state_out[b] = s;

  // 5. the slice's allowed set, then -inf on what it lacks
  const int v0 = slice * SLICE;
  const int n = min(a.V - v0, SLICE);                   // ids of this slice (>= 1)
  float* __restrict__ row = a.logits + (long long)b * a.ld + v0;
  const float ninf = -__builtin_inff();
  if (s < 0) {
    for (int i = tid; i < n; i += AB) row[i] = ninf;
    return;
  }
  const int d = a.default_next[s];
  const unsigned fill = (d >= 0 && d < a.S) ? 0xffffffffu : 0u;
  for (int w = tid; w < SLICE / 32; w += AB) bits[w] = fill;
  __syncthreads();
  const int k0 = lower_bound(a.edge_tok, lo, hi, v0);
  const int k1 = lower_bound(a.edge_tok, k0, hi, v0 + n);
  for (int k = k0 + tid; k < k1; k += AB) {
    const int i = a.edge_tok[k] - v0;
    if (i < 0 || i >= n) continue;                      // (an id outside the slice or the vocabulary: compared, never an index)
    const int nx = a.edge_next[k];
    if (nx >= 0 && nx < a.S) atomicOr(&bits[i >> 5], 1u << (i & 31));
    else atomicAnd(&bits[i >> 5], ~(1u << (i & 31)));
  }
  __syncthreads();
  for (int i = tid; i < n; i += AB)
    if (!((bits[i >> 5] >> (i & 31)) & 1u)) row[i] = ninf;
}

bool overlap(const void* p, long long pb, const void* q, long long qb) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a < b + (uintptr_t)qb && b < a + (uintptr_t)pb;
}

}  // namespace

extern "C" int kx_automaton_step(const kx_automaton_args* args, void* stream) {
  KX_REQUIRE(args != nullptr, "kx_automaton_step: null args");
  KX_REQUIRE(args->struct_bytes == sizeof(kx_automaton_args),
             "kx_automaton_step: stale binding — caller declares kx_automaton_args as %u bytes, this library (ABI %d) as %zu",
             (unsigned)args->struct_bytes, KX_ABI_VERSION, sizeof(kx_automaton_args));
  KX_REQUIRE(args->logits != nullptr, "kx_automaton_step: null logits");
  KX_REQUIRE(args->B >= 1 && args->B <= 0x7fffffffll, "kx_automaton_step: B=%lld must be >= 1", (long long)args->B);
  KX_REQUIRE(args->V >= 1, "kx_automaton_step: V=%lld must be >= 1", (long long)args->V);
  KX_REQUIRE(args->ld >= args->V, "kx_automaton_step: ld=%lld is smaller than V=%lld", (long long)args->ld, (long long)args->V);
  KX_REQUIRE(args->E >= 0, "kx_automaton_step: E=%lld must be >= 0", (long long)args->E);
  if (args->V > KX_AUTOMATON_MAX_V) {
    kx_set_error("kx_automaton_step: V=%lld exceeds %lld (the limit of kx_sample_logits, which reads the row next)",
                 (long long)args->V, KX_AUTOMATON_MAX_V);
    return KX_ERR_UNSUPPORTED;
  }
  if (args->S < 1 || args->S > 0x7fffffffll || args->E > 0x7fffffffll) {
    kx_set_error("kx_automaton_step: S=%lld must be in [1, 2^31) and E=%lld below 2^31", (long long)args->S, (long long)args->E);
    return KX_ERR_UNSUPPORTED;
  }
  const long long slices = (args->V + SLICE - 1) / SLICE;
  if (args->B * slices > 0x7fffffffll) {
    kx_set_error("kx_automaton_step: B=%lld rows x %lld slices of %d ids exceed one launch's 2^31 - 1 workgroups", (long long)args->B,
                 slices, SLICE);
    return KX_ERR_UNSUPPORTED;
  }
  KX_REQUIRE(args->edge_off != nullptr, "kx_automaton_step: null edge_off");
  KX_REQUIRE(args->default_next != nullptr, "kx_automaton_step: null default_next");
  KX_REQUIRE(args->E == 0 || args->edge_tok != nullptr, "kx_automaton_step: null edge_tok with E=%lld", (long long)args->E);
  KX_REQUIRE(args->E == 0 || args->edge_next != nullptr, "kx_automaton_step: null edge_next with E=%lld", (long long)args->E);
  KX_REQUIRE(args->state_in != nullptr, "kx_automaton_step: null state_in");
  KX_REQUIRE(args->state_out != nullptr, "kx_automaton_step: null state_out");
  KX_REQUIRE(args->B_in >= 1 && args->B_in <= 0x7fffffffll, "kx_automaton_step: B_in=%lld must be >= 1", (long long)args->B_in);
  KX_REQUIRE(args->src_row != nullptr || args->B_in == args->B,
             "kx_automaton_step: B_in=%lld differs from B=%lld without a src_row", (long long)args->B_in, (long long)args->B);
  KX_REQUIRE(!overlap(args->state_in, 4 * (long long)args->B_in, args->state_out, 4 * (long long)args->B),
             "kx_automaton_step: state_in [%lld] and state_out [%lld] overlap (the loops alternate two buffers)",
             (long long)args->B_in, (long long)args->B);
  AutomatonParams p;
  p.logits = args->logits; p.ld = args->ld; p.V = (int)args->V;
  p.edge_off = args->edge_off; p.edge_tok = args->edge_tok; p.edge_next = args->edge_next; p.default_next = args->default_next;
  p.S = (int)args->S; p.E = (int)args->E;
  p.state_in = args->state_in; p.B_in = (int)args->B_in; p.state_out = args->state_out;
  p.src_row = args->src_row; p.last_token = (const long long*)args->last_token; p.finished = args->finished;
  p.slices = (int)slices;
  KxProfScope prof(KX_K_MISC, args->B, args->V, 4, (hipStream_t)stream);
  hipLaunchKernelGGL(automaton_kernel, dim3((unsigned)(args->B * slices)), dim3(AB), 0, (hipStream_t)stream, p);
  KX_CHECK_LAUNCH("kx_automaton_step");
  return KX_OK;
}
