// Speculative decoding by prompt lookup: the per-step accept-and-draft launch (kx_spec_accept).  Contract: include/kosmosx_hip.h,
// "Speculative decoding by prompt lookup"; restated in plain Python in tests/spec_ref.py.
//
// One launch per verify step, one 256-thread workgroup per sequence, nothing shared between workgroups.  Integer work only: the
// result does not depend on execution order.  Lane 0 compares the at most 16 fed tokens with the picks and decides how many are
// emitted; the first lanes append them; then either the drafts are copied from draft_from, or the workgroup looks the sequence's
// last n-gram up in its own history: the last 64 ids are staged in LDS, threads stride over the start positions with an early
// exit at the first mismatch (the scan of kx_constrain.hip) and the largest matching start wins through an LDS atomicMax.
// Every id is compared or copied as a value and never indexes anything; every length and position read from device memory is
// checked before it does.  All stores are plain vector stores.
#include "kx_common.h"

namespace {

constexpr int SB = 256;        // threads per sequence
constexpr int TAIL = 64;       // staged suffix = the longest n-gram
constexpr int MAXK = 16;

struct SpecParams {
  int B, K, Kin, ngram_max;
  const long long* fed; const long long* picked;
  int* positions; int prefill_len;
  long long* history; long long hist_ld; int* hist_len;
  long long* out_tokens; long long out_ld; int* n_out;
  unsigned char* finished;
  int max_new; long long eos, pad;
  int step;
  int* out_src; int* emitted; long long emitted_ld;
  const long long* draft_from; long long draft_ld;
  long long* next_tokens;
};

__global__ __launch_bounds__(SB) void spec_accept_kernel(const SpecParams a) {
  __shared__ long long tail[TAIL];
  __shared__ long long cand[MAXK];
  __shared__ int best[TAIL + 1];
  __shared__ int sh_e, sh_fin, sh_nout, sh_hl, sh_base;
  const int tid = threadIdx.x;
  const long long b = blockIdx.x;
  const int K = a.K, Kin = a.Kin;
  long long* __restrict__ hist = a.history + b * a.hist_ld;

  if (tid == 0) {
    int fin = a.finished[b] != 0;
    const int nout = a.n_out[b], hl = a.hist_len[b];
    const int base = Kin == 1 ? a.prefill_len - 1 : a.positions[b * K];
    int e = 0;
    if (!fin) {
      const bool ok = nout >= 0 && nout <= a.max_new && hl >= 0 && (long long)hl + (a.max_new - nout) <= a.hist_ld &&
                      base >= 0 && base <= 0x7fffffff - 4 * MAXK;
      if (!ok) fin = 1;                                     // (the guards: finished, nothing emitted)
      else {
        const long long* f = a.fed + b * Kin;               // (not read when Kin == 1)
        const long long* p = a.picked + b * Kin;
        int acc = 0;
        while (acc + 1 < Kin && f[acc + 1] == p[acc]) ++acc;
        e = min(acc + 1, a.max_new - nout);
        for (int j = 0; j < e; ++j) {
          const long long v = p[j];
          cand[j] = v;
          if (a.eos >= 0 && v == a.eos) { e = j + 1; fin = 1; break; }
        }
        if (nout + e >= a.max_new) fin = 1;
      }
    }
    sh_e = e; sh_fin = fin; sh_nout = nout; sh_hl = hl; sh_base = base;
  }
  if (tid <= TAIL) best[tid] = -1;
  __syncthreads();
  const int e = sh_e, fin = sh_fin, nout = sh_nout, hl = sh_hl;

  if (tid < e) {                                            // append (e <= max_new - nout: inside out_ld and hist_ld, see the guards)
    a.out_tokens[b * a.out_ld + nout + tid] = cand[tid];
    hist[hl + tid] = cand[tid];
    if (a.out_src) a.out_src[b * a.out_ld + nout + tid] = a.step * K + tid;
  }
  if (tid == 0) {
    if (a.emitted) a.emitted[b * a.emitted_ld + a.step] = e;
    if (e > 0) { a.n_out[b] = nout + e; a.hist_len[b] = hl + e; }
    if (fin) a.finished[b] = 1;
  }
  if (tid < K && (e > 0 || Kin == 1)) a.positions[b * K + tid] = sh_base + e + tid;
  long long* __restrict__ next = a.next_tokens + b * K;
  if (fin) {                                                // (uniform) finished rows step on pad_id at their frozen positions
    if (tid < K) next[tid] = a.pad;
    return;
  }
  const long long last = cand[e - 1];                      // (not finished: e >= 1)
  if (tid == 0) next[0] = last;
  if (a.draft_from) {
    if (tid >= 1 && tid < K) {
      const long long slot = (long long)nout + e + tid - 1;
      next[tid] = slot < a.draft_ld ? a.draft_from[b * a.draft_ld + slot] : last;
    }
    return;
  }

  // the lookup in s = hist[0:len]
  const int len = hl + e;
  const int tl = len < TAIL ? len : TAIL;                   // tail[j] = s[len - tl + j]
  __syncthreads();                                          // the appended ids are in memory for every thread of the workgroup
  if (tid < tl) tail[tid] = hist[len - tl + tid];
  __syncthreads();
  int n = a.ngram_max < len - 1 ? a.ngram_max : len - 1, at = -1;
  for (; n >= 1; --n) {                                     // (uniform: `at` comes from LDS after a barrier)
    const long long* suf = tail + (tl - n);                 // s[len - n : len]
    int mine = -1;
    for (int i = tid; i <= len - n - 1; i += SB) {
      bool eq = true;
      for (int j = 0; j < n && eq; ++j) eq = hist[i + j] == suf[j];
      if (eq) mine = i;                                     // (i grows: the thread's largest)
    }
    if (mine >= 0) atomicMax(&best[n], mine);
    __syncthreads();
    at = best[n];
    if (at >= 0) break;
  }
  if (tid >= 1 && tid < K) {
    if (at >= 0) {
      const int from = at + n, p = len - from;              // 1 <= p: the match ends before the sequence does
      next[tid] = hist[from + (tid - 1) % p];
    } else next[tid] = last;
  }
}

}  // namespace

extern "C" int kx_spec_accept(const kx_spec_args* args, void* stream) {
  KX_REQUIRE(args != nullptr, "kx_spec_accept: null args");
  KX_REQUIRE(args->struct_bytes == sizeof(kx_spec_args),
             "kx_spec_accept: stale binding — caller declares kx_spec_args as %u bytes, this library (ABI %d) as %zu",
             (unsigned)args->struct_bytes, KX_ABI_VERSION, sizeof(kx_spec_args));
  KX_REQUIRE(args->K >= 2 && args->K <= MAXK, "kx_spec_accept: K=%lld outside 2..16 rows per sequence", (long long)args->K);
  KX_REQUIRE(args->Kin == 1 || args->Kin == args->K, "kx_spec_accept: Kin=%lld must be 1 (the prefill's row) or K=%lld",
             (long long)args->Kin, (long long)args->K);
  KX_REQUIRE(args->B >= 1 && args->B <= 0x7fffffffll / MAXK, "kx_spec_accept: B=%lld must be >= 1", (long long)args->B);
  KX_REQUIRE(args->ngram_max >= 1 && args->ngram_max <= TAIL, "kx_spec_accept: ngram_max=%d outside 1..%d", (int)args->ngram_max, TAIL);
  KX_REQUIRE(args->picked && args->positions && args->history && args->hist_len && args->out_tokens && args->n_out &&
             args->finished && args->next_tokens, "kx_spec_accept: null pointer (picked, positions, history, hist_len, out_tokens, "
             "n_out, finished and next_tokens are required)");
  KX_REQUIRE(args->fed != nullptr || args->Kin == 1, "kx_spec_accept: null fed with Kin=%lld", (long long)args->Kin);
  KX_REQUIRE(args->max_new >= 1 && args->max_new <= 0x7fffffffll - 4 * MAXK, "kx_spec_accept: max_new=%lld must be >= 1",
             (long long)args->max_new);
  KX_REQUIRE(args->out_ld >= args->max_new, "kx_spec_accept: out_ld=%lld is smaller than max_new=%lld", (long long)args->out_ld,
             (long long)args->max_new);
  KX_REQUIRE(args->hist_ld >= args->max_new, "kx_spec_accept: hist_ld=%lld leaves no room for max_new=%lld ids",
             (long long)args->hist_ld, (long long)args->max_new);
  KX_REQUIRE(args->Kin != 1 || (args->prefill_len >= 1 && args->prefill_len <= 0x7fffffffll - 4 * MAXK),
             "kx_spec_accept: prefill_len=%lld must be >= 1", (long long)args->prefill_len);
  KX_REQUIRE(args->step >= 0 && args->step <= 0x7fffffffll / MAXK, "kx_spec_accept: step=%lld must be >= 0", (long long)args->step);
  KX_REQUIRE(args->emitted == nullptr || args->step < args->emitted_ld, "kx_spec_accept: step=%lld outside emitted_ld=%lld",
             (long long)args->step, (long long)args->emitted_ld);
  KX_REQUIRE(args->draft_from == nullptr || args->draft_ld >= 0, "kx_spec_accept: draft_ld=%lld must be >= 0", (long long)args->draft_ld);
  SpecParams p;
  p.B = (int)args->B; p.K = (int)args->K; p.Kin = (int)args->Kin; p.ngram_max = (int)args->ngram_max;
  p.fed = (const long long*)args->fed; p.picked = (const long long*)args->picked;
  p.positions = args->positions; p.prefill_len = (int)args->prefill_len;
  p.history = (long long*)args->history; p.hist_ld = args->hist_ld; p.hist_len = args->hist_len;
  p.out_tokens = (long long*)args->out_tokens; p.out_ld = args->out_ld; p.n_out = args->n_out;
  p.finished = args->finished;
  p.max_new = (int)args->max_new; p.eos = args->eos_id; p.pad = args->pad_id;
  p.step = (int)args->step;
  p.out_src = args->out_src; p.emitted = args->emitted; p.emitted_ld = args->emitted_ld;
  p.draft_from = (const long long*)args->draft_from; p.draft_ld = args->draft_ld;
  p.next_tokens = (long long*)args->next_tokens;
  KxProfScope prof(KX_K_MISC, args->B, args->K, 8, (hipStream_t)stream);
  hipLaunchKernelGGL(spec_accept_kernel, dim3((unsigned)args->B), dim3(SB), 0, (hipStream_t)stream, p);
  KX_CHECK_LAUNCH("kx_spec_accept");
  return KX_OK;
}
