// Constraints on the next token (kx_constrain_logits): no-repeat n-gram, bad words, minimum length and stop sequences, applied to
// the fp32 logits rows in place before kx_sample_logits or kx_beam_step reads them.  Contract: include/kosmosx_hip.h.
//
// A banned id's logit becomes -inf and nothing else is written: the sampler never selects -inf (its rule 6) and to the beam step
// -inf is never a candidate, so neither kernel knows about constraints.  Bans commute with the repetition penalty
// (-inf * r == -inf / r == -inf): constrain-then-sample is the `transformers` processor order.  A row with every logit banned
// falls under the sampler's own rule: it emits pad and is finished.
//
// One launch, one 256-thread workgroup per row, nothing shared between workgroups.  The work is latency-bound (a few KB per row):
// the last 64 ids of the row's logical sequence are staged once in LDS, translated from logical to physical history columns (the
// ragged batch's right padding takes part in no match); threads stride over the start positions of the n-gram scan, reading the
// history with an early exit at the first mismatch, and over the bad and stop sequences.  Every value read from device memory
// (ids, CSR offsets, prompt_lens) is range-checked before it is used as an index.  The -inf stores are plain stores; several
// threads may store the same value to one address.
#include "kx_common.h"

namespace {

constexpr int CB = 256;        // threads per row
constexpr int TAIL = 64;       // staged suffix: a 64-id stop sequence, a 63-id n-gram or bad-word prefix
constexpr int MAX_SEQ = 64;    // ids per bad / stop sequence, and the largest ngram

struct ConstrainParams {
  float* logits; long long ld, V;
  const long long* history; long long hist_ld; int hist_len;
  int prompt_width; const int* prompt_lens;
  int new_tokens, ngram;
  const long long* bad_ids; const int* bad_off; int n_bad, bad_total;
  const long long* stop_ids; const int* stop_off; int n_stop, stop_total;
  int ban_eos; long long eos;
  unsigned char* finished;
};

// Sequence k of a CSR table as (first id, length); length 0 when the device offsets leave [0, total] or the limits.
__device__ __forceinline__ int csr_entry(const int* __restrict__ off, int k, int total, int& begin) {
  const int a = off[k], e = off[k + 1];
  begin = a;
  if (a < 0 || e > total || e <= a || e - a > MAX_SEQ) return 0;
  return e - a;
}

__global__ __launch_bounds__(CB) void constrain_kernel(const ConstrainParams a) {
  __shared__ long long tail[TAIL];
  __shared__ int stop_hit;
  const int tid = threadIdx.x;
  const long long b = blockIdx.x;
  if (a.finished && a.finished[b]) return;            // (uniform: one byte, read by every thread)
  float* __restrict__ row = a.logits + b * a.ld;
  const long long* __restrict__ hist = a.history + b * a.hist_ld;
  const float ninf = -__builtin_inff();

  // logical index j -> physical column: j < pl ? j : pw + (j - pl); n = pl + (hist_len - pw)
  int pw = a.hist_len, pl = a.hist_len;
  if (a.prompt_lens) {
    pw = a.prompt_width;                                // (0 <= prompt_width <= hist_len: checked on the host)
    const int l = a.prompt_lens[b];
    pl = l < 0 ? 0 : (l > pw ? pw : l);
  }
  const int gap = pw - pl;
  const int n = a.hist_len - gap;
  const int tl = n < TAIL ? n : TAIL;                  // tail[j] = s[n - tl + j]
  if (tid < tl) {
    const int j = n - tl + tid;
    tail[tid] = hist[j < pl ? j : j + gap];
  }
  if (tid == 0) stop_hit = 0;
  __syncthreads();

  if (a.n_stop > 0 && a.new_tokens >= 1) {
    for (int k = tid; k < a.n_stop; k += CB) {
      int w0;
      const int m = csr_entry(a.stop_off, k, a.stop_total, w0);
      if (m == 0 || m > n) continue;
      bool eq = true;
      for (int j = 0; j < m && eq; ++j) eq = a.stop_ids[w0 + j] == tail[tl - m + j];
      if (eq) stop_hit = 1;
    }
    __syncthreads();
    if (stop_hit) {                                     // (uniform)
      if (tid == 0 && a.finished) a.finished[b] = 1;
      return;
    }
  }

  const int N = a.ngram;
  if (N >= 1 && n + 1 >= N) {
    const long long* pre = tail + (tl - (N - 1));      // s[n-N+1 : n]  (N - 1 <= 63 <= tl whenever N - 1 <= n)
    for (int i = tid; i + N - 1 < n; i += CB) {
      bool eq = true;
      for (int j = 0; j < N - 1 && eq; ++j) {
        const int q = i + j;
        eq = hist[q < pl ? q : q + gap] == pre[j];
      }
      if (eq) {
        const int q = i + N - 1;
        const long long id = hist[q < pl ? q : q + gap];
        if (id >= 0 && id < a.V) row[id] = ninf;
      }
    }
  }

  for (int k = tid; k < a.n_bad; k += CB) {
    int w0;
    const int m = csr_entry(a.bad_off, k, a.bad_total, w0);
    if (m == 0 || m - 1 > n) continue;
    bool eq = true;
    for (int j = 0; j < m - 1 && eq; ++j) eq = a.bad_ids[w0 + j] == tail[tl - (m - 1) + j];
    if (eq) {
      const long long id = a.bad_ids[w0 + m - 1];
      if (id >= 0 && id < a.V) row[id] = ninf;
    }
  }

  if (tid == 0 && a.ban_eos) row[a.eos] = ninf;         // (ban_eos: g < min_new and 0 <= eos < V, decided on the host)
}

// The host copy of a CSR table's offsets: the limits, before any launch.
int check_table(const char* what, const int64_t* ids, const int32_t* off, const int32_t* off_host, int64_t n, int* total) {
  *total = 0;
  KX_REQUIRE(n >= 0 && n <= 0x7fffffffll, "kx_constrain_logits: n_%s=%lld must be >= 0", what, (long long)n);
  if (n == 0) return KX_OK;
  KX_REQUIRE(ids != nullptr, "kx_constrain_logits: null %s_ids with n_%s=%lld", what, what, (long long)n);
  KX_REQUIRE(off != nullptr, "kx_constrain_logits: null %s_off with n_%s=%lld", what, what, (long long)n);
  KX_REQUIRE(off_host != nullptr, "kx_constrain_logits: null %s_off_host with n_%s=%lld", what, what, (long long)n);
  KX_REQUIRE(off_host[0] == 0, "kx_constrain_logits: %s_off_host[0]=%d must be 0", what, (int)off_host[0]);
  for (int64_t k = 0; k < n; ++k) {
    const long long m = (long long)off_host[k + 1] - (long long)off_host[k];
    if (m < 1 || m > MAX_SEQ) {
      kx_set_error("kx_constrain_logits: %s sequence %lld has %lld ids (%s_off_host); a sequence holds 1 to %d ids", what,
                   (long long)k, m, what, MAX_SEQ);
      return KX_ERR_UNSUPPORTED;
    }
  }
  *total = (int)off_host[n];
  return KX_OK;
}

}  // namespace

extern "C" int kx_constrain_logits(const kx_constrain_args* args, void* stream) {
  KX_REQUIRE(args != nullptr, "kx_constrain_logits: null args");
  KX_REQUIRE(args->struct_bytes == sizeof(kx_constrain_args),
             "kx_constrain_logits: stale binding — caller declares kx_constrain_args as %u bytes, this library (ABI %d) as %zu",
             (unsigned)args->struct_bytes, KX_ABI_VERSION, sizeof(kx_constrain_args));
  KX_REQUIRE(args->logits != nullptr, "kx_constrain_logits: null logits");
  KX_REQUIRE(args->B >= 1 && args->B <= 0x7fffffffll, "kx_constrain_logits: B=%lld must be >= 1", (long long)args->B);
  KX_REQUIRE(args->V >= 1, "kx_constrain_logits: V=%lld must be >= 1", (long long)args->V);
  KX_REQUIRE(args->ld >= args->V, "kx_constrain_logits: ld=%lld is smaller than V=%lld", (long long)args->ld, (long long)args->V);
  KX_REQUIRE(args->hist_len >= 0 && args->hist_len <= 0x7fffffffll, "kx_constrain_logits: hist_len=%lld must be >= 0",
             (long long)args->hist_len);
  KX_REQUIRE(args->history != nullptr || args->hist_len == 0, "kx_constrain_logits: null history with hist_len=%lld",
             (long long)args->hist_len);
  KX_REQUIRE(args->history == nullptr || args->hist_ld > args->hist_len,
             "kx_constrain_logits: hist_ld=%lld leaves no room to append after hist_len=%lld", (long long)args->hist_ld,
             (long long)args->hist_len);
  KX_REQUIRE(args->prompt_lens == nullptr || (args->prompt_width >= 0 && args->prompt_width <= args->hist_len),
             "kx_constrain_logits: prompt_width=%lld outside [0, hist_len=%lld]", (long long)args->prompt_width,
             (long long)args->hist_len);
  KX_REQUIRE(args->new_tokens >= 0 && args->new_tokens <= 0x7fffffffll, "kx_constrain_logits: new_tokens=%lld must be >= 0",
             (long long)args->new_tokens);
  KX_REQUIRE(args->min_new >= 0, "kx_constrain_logits: min_new=%lld must be >= 0", (long long)args->min_new);
  KX_REQUIRE(args->ngram >= 0, "kx_constrain_logits: ngram=%d must be >= 0", (int)args->ngram);
  if (args->ngram > MAX_SEQ) {
    kx_set_error("kx_constrain_logits: ngram=%d exceeds %d (the n-gram's prefix is staged in LDS)", (int)args->ngram, MAX_SEQ);
    return KX_ERR_UNSUPPORTED;
  }
  ConstrainParams p;
  KX_TRY(check_table("bad", args->bad_ids, args->bad_off, args->bad_off_host, args->n_bad, &p.bad_total));
  KX_TRY(check_table("stop", args->stop_ids, args->stop_off, args->stop_off_host, args->n_stop, &p.stop_total));
  p.logits = args->logits; p.ld = args->ld; p.V = args->V;
  p.history = (const long long*)args->history; p.hist_ld = args->hist_ld; p.hist_len = (int)args->hist_len;
  p.prompt_width = (int)args->prompt_width; p.prompt_lens = (const int*)args->prompt_lens;
  p.new_tokens = (int)args->new_tokens; p.ngram = (int)args->ngram;
  p.bad_ids = (const long long*)args->bad_ids; p.bad_off = (const int*)args->bad_off; p.n_bad = (int)args->n_bad;
  p.stop_ids = (const long long*)args->stop_ids; p.stop_off = (const int*)args->stop_off; p.n_stop = (int)args->n_stop;
  p.eos = args->eos_id;
  p.ban_eos = (args->new_tokens < args->min_new && args->eos_id >= 0 && args->eos_id < args->V) ? 1 : 0;
  p.finished = args->finished;
  KxProfScope prof(KX_K_MISC, args->B, args->V, 4, (hipStream_t)stream);
  hipLaunchKernelGGL(constrain_kernel, dim3((unsigned)args->B), dim3(CB), 0, (hipStream_t)stream, p);
  KX_CHECK_LAUNCH("kx_constrain_logits");
  return KX_OK;
}
