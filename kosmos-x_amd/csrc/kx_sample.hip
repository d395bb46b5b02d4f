// Token sampling on the device (kx_sample_logits) and the one-row embedding launch that feeds a sampled token back into
// the decoder (kx_embed_step): the last piece of autoregressive decoding.  Contract: include/kosmosx_hip.h.
//
// One launch per decode step, one 1024-thread workgroup per sequence, nothing shared between workgroups.  Everything that
// decides a result is either an exact integer operation or a per-element fp32 expression, so a row's outputs do not depend
// on the order in which lanes, waves or atomics happen to run:
//   * x_i (penalised logit / T) is mapped to an order-preserving 32-bit key; maxima are taken over (key, ~index) pairs;
//   * the k-th largest value and the top-p threshold are found by radix select on that key (11 + 11 + 10 bits) over a
//     2048-bin LDS histogram of 64-bit INTEGER sums: element counts for top-k, exp(x_i - max) in 2^-40 fixed point for top-p
//     (integer adds commute, so the LDS atomics may land in any order);
//   * typical-p / epsilon / eta (kx_sample_logits_truncate) add 64-bit integer sums of the same masses and of
//     (uint64)((double)w_i * (double)(m - x_i)), one mean per row taken from two such sums, and one more radix select, over the key
//     of |(m - x_i) - mean| ascending;
//   * the draw is a Gumbel arg max with Philox4x32-10 addressed by (seed, sequence id, position, element index).
// Every loop has a trip count fixed by V, the histogram size or the wave width; there is no waiting on other threads
// beyond __syncthreads().
#include "kx_common.h"
#include "kx_select.h"   // f2key / key2f / mass_fix / block reductions, shared with kx_beam.hip

namespace {

constexpr int BINS = 2048;
constexpr long long KX_SAMPLE_MAX_V = 1ll << 23;  // 2^23 values of at most 2^40 each stay below 2^63
constexpr long long KX_SAMPLE_MAX_V_PENALTY = 40960ll * 8;   // the history bitmap lives in LDS next to the histogram

struct SampleParams {
  const float* logits; long long ld; int V;
  float T, p, r; int k, greedy, pen;
  unsigned long long seed; unsigned position;
  const long long* seq;
  long long* history; long long hist_ld; int hist_len;
  unsigned char* finished; long long eos, pad;
  long long* next; long long* out_tokens; long long out_ld, out_col;
  int* kept_count; unsigned char* keep_mask;
};

// x_i: repetition penalty (ids in the row's history, once per distinct id), then temperature; both IEEE fp32 divisions.
// NaN and -inf come back as -inf (never a candidate), -0 as +0 (one key per value).
__device__ __forceinline__ float load_x(const SampleParams& a, const float* __restrict__ row, const unsigned* bitmap, int i) {
  float l = row[i];
  if (a.pen && ((bitmap[i >> 5] >> (i & 31)) & 1u)) l = l > 0.f ? l / a.r : l * a.r;
  if (!a.greedy) l = l / a.T;
  if (!(l > -__builtin_inff())) l = -__builtin_inff();
  if (l == 0.f) l = 0.f;
  return l;
}

// What radix_select orders the row by: KEY(x, key) says whether x takes part and gives its 32-bit key (larger = selected first).
//   XKey: the value itself, among the candidates with key(x) >= limit (top-k, top-p);
//   DistKey: typical-p — among the same candidates, the distance d = |(m - x) - mu| ASCENDING: the key is ~key(d), two fp32
//            subtractions and an absolute value (x == m gives m - x = 0, also when both are +inf).
struct XKey {
  unsigned limit;
  __device__ __forceinline__ bool operator()(float x, unsigned& key) const { key = f2key(x); return key >= limit; }
};
__device__ __forceinline__ unsigned dist_key(float x, float m, float mu) {
  const float s = x == m ? 0.f : m - x;
  return ~f2key(fabsf(s - mu));
}
struct DistKey {
  unsigned limit; float m, mu;
  __device__ __forceinline__ bool operator()(float x, unsigned& key) const { key = dist_key(x, m, mu); return f2key(x) >= limit; }
};

// The largest key K (among the elements KEY admits) whose weight at or above it reaches `target`:
//   MASS = false: weight = element count  -> K = the target-th largest key;
//   MASS = true : weight = mass_fix       -> K = the smallest key whose strictly-greater mass is still below target.
// Three histogram passes fix the key's digits from the top; `carry` is the weight strictly above the chosen bin.
// Returns false (key untouched) when the whole weight stays below target.
// (OWNER: one instantiation per kernel that calls it, so that each stays a single-caller function the compiler folds into its
// kernel exactly as it did when there was one kernel)
template <bool MASS, typename OWNER, typename KEY>
__device__ bool radix_select(const SampleParams& a, const float* __restrict__ row, const unsigned* bitmap, float m,
                             const KEY admit, unsigned long long target, unsigned long long* hist,
                             unsigned long long* gsum, unsigned long long* sel, unsigned& key_out) {
  const int tid = threadIdx.x;
  unsigned prefix = 0, pmask = 0;
  unsigned long long carry = 0;
#pragma unroll 1
  for (int level = 0; level < 3; ++level) {
    const int shift = level == 0 ? 21 : (level == 1 ? 10 : 0);
    const unsigned dmask = level == 2 ? 1023u : 2047u;
    for (int j = tid; j < BINS; j += SB) hist[j] = 0;
    __syncthreads();
#pragma unroll 4
    for (int i = tid; i < a.V; i += SB) {            // consecutive lanes read consecutive logits
      const float x = load_x(a, row, bitmap, i);
      unsigned key;
      if (admit(x, key) && (key & pmask) == prefix) {
        const unsigned long long inc = MASS ? mass_fix(x, m) : 1ull;
        if (inc) atomicAdd(&hist[(key >> shift) & dmask], inc);
      }
    }
    __syncthreads();
    // Scan from the top in two steps, every LDS read with consecutive lanes on consecutive bins: the 32 sums of 64-bin
    // groups (two per wave), then wave 0 picks the group and the bin inside it.
    for (int g = (tid >> 6) * 2; g < (tid >> 6) * 2 + 2; ++g) {
      unsigned long long v = hist[g * 64 + (tid & 63)];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      if ((tid & 63) == 0) gsum[g] = v;
    }
    __syncthreads();
    if (tid < 64) {
      const unsigned long long gs = tid < 32 ? gsum[31 - tid] : 0ull;         // lane 0 = the top group
      unsigned long long incl = gs;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long t = __shfl_up(incl, o, 64);
        if (tid >= o) incl += t;
      }
      const unsigned long long hit = __ballot(tid < 32 && carry + incl >= target);
      if (hit == 0) {
        if (tid == 0) sel[0] = ~0ull;
      } else {
        const int fl = __ffsll((long long)hit) - 1;
        const int G = 31 - fl;
        const unsigned long long above = __shfl(carry + incl - gs, fl, 64);   // weight strictly above group G
        const unsigned long long h = hist[G * 64 + 63 - tid];                 // lane 0 = the group's top bin
        unsigned long long incl2 = h;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const unsigned long long t = __shfl_up(incl2, o, 64);
          if (tid >= o) incl2 += t;
        }
        const unsigned long long hit2 = __ballot(above + incl2 >= target);    // non-empty: the group's total reaches target
        if (tid == __ffsll((long long)hit2) - 1) {
          sel[0] = (unsigned long long)(G * 64 + 63 - tid);
          sel[1] = above + incl2 - h;
        }
      }
    }
    __syncthreads();
    const unsigned long long bin = sel[0];
    if (bin == ~0ull) { __syncthreads(); return false; }
    carry = sel[1];
    prefix |= (unsigned)bin << shift;
    pmask |= dmask << shift;
  }
  __syncthreads();
  key_out = prefix;
  return true;
}

// RAGGED: the Philox position of row b is positions[b] + advance (device memory, one word per row) instead of a.position, and
// with advance != 0 thread 0 stores it back after the draw — the same launch moves the row on.  Nothing else differs.
// The ragged launch passes one more kernel argument (R = RaggedPos); the uniform launch has an empty pack, i.e. the signature and
// kernel-argument layout it always had.
// MINP (kx_sample_logits_min_p): one more kernel argument behind it (MinP: lm = log(min_p), taken on the host) and one more
// threshold after top-p, x_i >= x_max + lm.  The empty and the RaggedPos-only pack stay the kernels they always were.
// TRUNC (kx_sample_logits_truncate): one more kernel argument, last of the pack (Trunc: min-p's lm with its on/off flag, and the
// three cut-offs as the ABI carries them) and up to three more stages after min-p — typical-p, epsilon, eta — each over what the
// stage before it kept.  The kept set stays a conjunction of per-element predicates (Kept), so every pass recomputes membership
// from x alone and nothing per element is stored.
// ROWS (kx_sample_logits_rows): one more kernel argument, last of the pack (Rows: the device table of one kx_sample_row per row and
// whether the launch honours the budgets).  The workgroup reads its row's record through a workgroup-uniform address and runs the
// stages of the Trunc instantiation with the record's values in place of the launch's scalars — greedy or not, r, T, k, p, min-p's
// lm, the three cut-offs, the seed — so every branch on a record value is uniform across the workgroup and no barrier sits in
// divergent code.  Whether the bitmap is built and read stays the launch's own a.pen: a record only supplies the r it is used with.
struct RaggedPos { int* positions; int advance; };
struct MinP { float lm; };
struct Trunc { float lm, typical, epsilon, eta; int minp; };
struct Rows { const kx_sample_row* table; int budget; };
template <bool SECOND, typename T> __device__ __forceinline__ const T& pick(const T& a, const T& b) {
  if constexpr (SECOND) return b; else return a;
}
struct Kept {
  unsigned tau;                  // rules 1-4 and min-p: key(x) >= tau
  int typ; float mu; unsigned dkey;        // typical-p (typ != 0): dist_key(x) >= dkey
  unsigned long long wmin; unsigned ktop;  // epsilon / eta (wmin != 0): mass_fix(x) >= wmin, or key(x) == ktop (the stage's arg max)
};
__device__ __forceinline__ bool kept_in(const Kept& s, float x, float m) {
  const unsigned k = f2key(x);
  bool in = k >= s.tau;
  if (s.typ) in = in && dist_key(x, m, s.mu) >= s.dkey;
  if (s.wmin) in = in && (mass_fix(x, m) >= s.wmin || k == s.ktop);
  return in;
}
// Over the kept set: Z = sum of w_i, E = sum of (uint64)((double)w_i * (double)(m - x_i)) (0 where x_i == m or w_i == 0), both
// 64-bit integer sums, and the largest key(x).  One pass over the row, three block reductions.
__device__ __forceinline__ void kept_stats(const SampleParams& a, const float* __restrict__ row, const unsigned* bitmap, float m,
                                           const Kept& s, unsigned long long* red, unsigned long long& Z, unsigned long long& E,
                                           unsigned& ktop) {
  unsigned long long z = 0, e = 0, top = 0;
#pragma unroll 2
  for (int i = threadIdx.x; i < a.V; i += SB) {
    const float x = load_x(a, row, bitmap, i);
    if (kept_in(s, x, m)) {
      const unsigned long long w = mass_fix(x, m);
      z += w;
      if (w != 0 && x != m) e += (unsigned long long)((double)w * (double)(m - x));
      const unsigned long long k = f2key(x);
      top = k > top ? k : top;
    }
  }
  Z = block_sum_u64(z, red);
  E = block_sum_u64(e, red);
  ktop = (unsigned)block_max_u64(top, red);
}
template <typename A, typename... Rest> __device__ __forceinline__ const A& first_arg(const A& a, const Rest&...) { return a; }
template <typename A, typename... Rest> __device__ __forceinline__ const auto& last_arg(const A& a, const Rest&... rest) {
  if constexpr (sizeof...(Rest) == 0) return a; else return last_arg(rest...);
}
template <typename T, typename... R> constexpr bool pack_has = (std::is_same_v<T, R> || ...);

template <typename... R>
__global__ __launch_bounds__(SB) void sample_kernel(const SampleParams a0, const R... r) {
  constexpr bool RAGGED = pack_has<RaggedPos, R...>;    // (first of the pack)
  constexpr bool MINP = pack_has<MinP, R...>;           // (last of the pack)
  constexpr bool ROWS = pack_has<Rows, R...>;           // (last of the pack)
  constexpr bool TRUNC = pack_has<Trunc, R...> || ROWS; // (last of the pack; ROWS: the record's cut-offs)
  using Owner = void(R...);
  // ROWS: the launch's parameters with the row's record over the scalar sampling fields; otherwise `a` IS the kernel argument
  [[maybe_unused]] SampleParams ar;
  [[maybe_unused]] Trunc tr;
  [[maybe_unused]] int budget = 0;
  if constexpr (ROWS) {
    const Rows& rw = last_arg(r...);
    const kx_sample_row rec = rw.table[blockIdx.x];     // (uniform: one record, read by every thread)
    ar = a0;
    ar.greedy = (!rec.do_sample || rec.temperature == 0.0f) ? 1 : 0;
    ar.T = rec.temperature; ar.k = rec.top_k; ar.p = rec.top_p; ar.seed = rec.seed;
    ar.r = a0.pen ? rec.repetition_penalty : 1.0f;      // (a launch without the bitmap reads every r as 1)
    tr.minp = rec.min_p != 0.0f;
    tr.lm = rec.log_min_p; tr.typical = rec.typical_p; tr.epsilon = rec.epsilon_cutoff; tr.eta = rec.eta_cutoff;
    budget = rw.budget ? rec.max_new : 0;
  }
  const SampleParams& a = pick<ROWS>(a0, ar);
  __shared__ unsigned long long hist[BINS];
  __shared__ unsigned long long red[SW];
  __shared__ unsigned long long gsum[BINS / 64];
  __shared__ unsigned long long sel[2];
  extern __shared__ unsigned bitmap[];
  const int tid = threadIdx.x;
  const long long b = blockIdx.x;
  const float* __restrict__ row = a.logits + b * a.ld;
  unsigned char* mask = a.keep_mask ? a.keep_mask + b * a.V : nullptr;

  long long tok = a.pad;
  int fin = 0, kept = 0;
  if (a.finished && a.finished[b]) {                  // (uniform: one byte, read by every thread)
    if (mask) for (int i = tid; i < a.V; i += SB) mask[i] = 0;
  } else {
    if (a.pen) {
      const int words = (a.V + 31) >> 5;
      for (int j = tid; j < words; j += SB) bitmap[j] = 0;
      __syncthreads();
      for (int j = tid; j < a.hist_len; j += SB) {
        const long long id = a.history[b * a.hist_ld + j];
        if (id >= 0 && id < a.V) atomicOr(&bitmap[id >> 5], 1u << (id & 31));
      }
      __syncthreads();
    }
    // arg max of x, lowest index among exact ties: max over (key << 32 | ~index)
    unsigned long long best = 0;
#pragma unroll 4
    for (int i = tid; i < a.V; i += SB) {
      const unsigned long long pk = ((unsigned long long)f2key(load_x(a, row, bitmap, i)) << 32) | (0xffffffffu - (unsigned)i);
      best = pk > best ? pk : best;
    }
    best = block_max_u64(best, red);
    const unsigned kmax = (unsigned)(best >> 32);
    if (kmax < KEY_MIN_VALID) {                       // no candidate: pad, and the row is finished
      fin = 1;
      if (mask) for (int i = tid; i < a.V; i += SB) mask[i] = 0;
    } else if (a.greedy) {
      tok = 0xffffffffu - (unsigned)best;
      if (mask || a.kept_count) {                     // greedy applies no filter: the debug outputs report the candidates
        unsigned long long c = 0;
        for (int i = tid; i < a.V; i += SB) {
          const bool v = f2key(load_x(a, row, bitmap, i)) >= KEY_MIN_VALID;
          if (mask) mask[i] = v;
          c += v;
        }
        kept = (int)block_sum_u64(c, red);
      }
    } else {
      const float m = key2f(kmax);
      unsigned tau = KEY_MIN_VALID;
      if (a.k > 0 && a.k < a.V) {
        unsigned kk;
        if (radix_select<false, Owner>(a, row, bitmap, m, XKey{tau}, (unsigned long long)a.k, hist, gsum, sel, kk)) tau = kk;
      }
      if (a.p < 1.0f) {
        unsigned long long z = 0;                     // mass of what top-k kept
#pragma unroll 4
        for (int i = tid; i < a.V; i += SB) {
          const float x = load_x(a, row, bitmap, i);
          if (f2key(x) >= tau) z += mass_fix(x, m);
        }
        z = block_sum_u64(z, red);
        // keep iff (mass strictly above) < p Z; the masses are integers, so "< p Z" is "< ceil(p Z)"
        const unsigned long long target = (unsigned long long)ceil((double)a.p * (double)z);
        unsigned kp;
        if (radix_select<true, Owner>(a, row, bitmap, m, XKey{tau}, target > 0 ? target : 1ull, hist, gsum, sel, kp)) tau = kp;
      }
      if constexpr (MINP) {                             // min-p, after top-p: x_i >= x_max + lm (keys order as the values do)
        const unsigned km = f2key(m + last_arg(r...).lm);
        tau = km > tau ? km : tau;
      }
      [[maybe_unused]] Kept s{tau, 0, 0.f, 0u, 0ull, kmax};
      if constexpr (TRUNC) {
        const Trunc& t = [&]() -> const Trunc& { if constexpr (ROWS) return tr; else return last_arg(r...); }();
        if (t.minp) {                                   // min-p, as above
          const unsigned km = f2key(m + t.lm);
          s.tau = km > tau ? km : tau;
        }
        unsigned long long Z, E;
        unsigned top;
        if (t.typical < 1.0f) {                         // typical-p: the band of least |(m - x) - mu| whose mass reaches typical * Z
          kept_stats(a, row, bitmap, m, s, red, Z, E, top);
          if (Z) {                                      // (a stage without mass keeps what it was given)
            const float mu = (float)((double)E / (double)Z);
            const unsigned long long target = (unsigned long long)ceil((double)t.typical * (double)Z);
            unsigned dk;
            if (radix_select<true, Owner>(a, row, bitmap, m, DistKey{s.tau, m, mu}, target > 0 ? target : 1ull, hist, gsum, sel, dk)) {
              s.typ = 1; s.mu = mu; s.dkey = dk;
            }
          }
        }
        if (t.epsilon > 0.f || t.eta > 0.f) {
          kept_stats(a, row, bitmap, m, s, red, Z, E, top);
          s.ktop = top;                                 // the arg max of what typical-p left; epsilon keeps it, so it is eta's too
          if (t.epsilon > 0.f) {                        // epsilon: w_i >= epsilon * Z
            s.wmin = (unsigned long long)ceil((double)t.epsilon * (double)Z);
            if (t.eta > 0.f) kept_stats(a, row, bitmap, m, s, red, Z, E, top);
          }
          if (t.eta > 0.f && Z) {                       // eta: w_i >= min(eta, sqrt(eta) exp(-H)) * Z, H = log(Z 2^-40) + mu2
            if (tid == 0) {
              const float mu2 = (float)((double)E / (double)Z);
              const double cut = fmin((double)t.eta * (double)Z, sqrt((double)t.eta) * exp(-(double)mu2) * 1099511627776.0);
              sel[0] = (unsigned long long)ceil(cut);
            }
            __syncthreads();
            const unsigned long long w2 = sel[0];
            __syncthreads();
            s.wmin = w2 > s.wmin ? w2 : s.wmin;
          }
        }
      }
      // Gumbel arg max over the kept set {key >= tau}; Philox block `base / 4` serves elements base .. base + 3, so here
      // (and only here) a thread owns four consecutive elements
      // (RAGGED: thread 0 stores the advanced position below, behind the barriers of the two reductions that follow this read)
      unsigned position = a.position;
      if constexpr (RAGGED) position = (unsigned)(first_arg(r...).positions[b] + first_arg(r...).advance);
      const unsigned long long ctr = ((unsigned long long)(unsigned)(a.seq ? a.seq[b] : b) << 32) | position;
      unsigned long long gbest = 0, c = 0;
      for (int base = tid * 4; base < a.V; base += SB * 4) {
        float xs[4];
        bool kp[4], any = false;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int i = base + e;
          kp[e] = false;
          xs[e] = 0.f;
          if (i < a.V) {
            xs[e] = load_x(a, row, bitmap, i);
            if constexpr (TRUNC) kp[e] = kept_in(s, xs[e], m);
            else kp[e] = f2key(xs[e]) >= tau;
            if (mask) mask[i] = kp[e];
          }
          any |= kp[e];
        }
        if (any) {
          unsigned w[4];
          philox4x32_10(ctr, (unsigned)(base >> 2), a.seed, w);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            if (kp[e]) {
              const float u = (float)(2u * (w[e] >> 9) + 1u) * 5.9604644775390625e-8f;      // odd / 2^24: exact, inside (0, 1)
              const float score = xs[e] - logf(-logf(u));
              const unsigned long long pk = ((unsigned long long)f2key(score) << 32) | (0xffffffffu - (unsigned)(base + e));
              gbest = pk > gbest ? pk : gbest;
              ++c;
            }
          }
        }
      }
      gbest = block_max_u64(gbest, red);
      kept = (int)block_sum_u64(c, red);
      tok = 0xffffffffu - (unsigned)gbest;
    }
    if (!fin && a.eos >= 0 && tok == a.eos) fin = 1;
    if constexpr (ROWS) {                               // the row's budget: this launch wrote its max_new-th token
      if (budget > 0 && a.out_col + 1 >= (long long)budget) fin = 1;
    }
  }
  if (tid == 0) {
    a.next[b] = tok;
    if (a.out_tokens) a.out_tokens[b * a.out_ld + a.out_col] = tok;
    if (a.history) a.history[b * a.hist_ld + a.hist_len] = tok;
    if (a.finished && fin) a.finished[b] = 1;
    if (a.kept_count) a.kept_count[b] = kept;
    if constexpr (RAGGED) {
      const RaggedPos& rp = first_arg(r...);
      if (rp.advance) rp.positions[b] = rp.positions[b] + rp.advance;
    }
  }
}

// The start of a ragged decode step: embed_step_kernel with the row's own position rows, read from positions[b], and the
// gather of the row's four XPos table rows into [B, 32] tables (see kx_step_prepare in include/kosmosx_hip.h).
// R = SpanRows (kx_decoder_extend_ragged): the launch's B rows are sequences of `span` consecutive rows, row b = (b / span, b % span)
// at position positions[b / span] + b % span.  The empty pack is the launch it always was.
struct SpanRows { int span; };
template <typename... R>
__global__ __launch_bounds__(256) void step_prepare_kernel(const long long* __restrict__ tokens, const float* __restrict__ embed,
                                                           const float* __restrict__ pos, const int* __restrict__ positions,
                                                           const float* __restrict__ t0, const float* __restrict__ t1,
                                                           const float* __restrict__ t2, const float* __restrict__ t3,
                                                           float* __restrict__ out, float* __restrict__ xrows, int B, int d,
                                                           long long vocab, long long max_pos, int pos_shift, long long xpos_len,
                                                           int* err, const R... r) {
  const long long b = blockIdx.x;
  long long t;
  if constexpr (sizeof...(R) != 0) {
    const int span = first_arg(r...).span;
    t = (long long)positions[b / span] + b % span;
  } else t = positions[b];
  if (t < pos_shift || t + 2 >= max_pos || (xrows && t >= xpos_len)) {   // the caller's error: nothing of this row is read or written
    if (threadIdx.x == 0) atomicOr(err, KX_RAGGED_ERR_TABLE);
    return;
  }
  long long id = tokens[b];
  id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);   // memory safety only
  const float4* src = reinterpret_cast<const float4*>(embed + id * d);
  const float4* pa = reinterpret_cast<const float4*>(pos + (2 + t - pos_shift) * d);
  const float4* pb = pos_shift ? reinterpret_cast<const float4*>(pos + (2 + t) * d) : nullptr;
  float4* o = reinterpret_cast<float4*>(out + b * d);
  for (int c = threadIdx.x; c < (d >> 2); c += 256) {
    float4 v = src[c];
    const float4 a1 = pa[c];
    v.x += a1.x; v.y += a1.y; v.z += a1.z; v.w += a1.w;
    if (pb) { const float4 a2 = pb[c]; v.x += a2.x; v.y += a2.y; v.z += a2.z; v.w += a2.w; }
    o[c] = v;
  }
  if (xrows && threadIdx.x < 128) {                   // 4 tables x 32 values
    const int k = threadIdx.x >> 5, j = threadIdx.x & 31;
    const float* tb = k == 0 ? t0 : k == 1 ? t1 : k == 2 ? t2 : t3;
    xrows[((long long)k * B + b) * 32 + j] = tb[t * 32 + j];
  }
}

// out[b] = embed[tokens[b]] + pos[2 + pos_a] (+ pos[2 + pos_b]): the row embed_splice_kernel writes for a text token whose
// first / second position rows are pos_a / pos_b, in the same order of additions.
__global__ __launch_bounds__(256) void embed_step_kernel(const long long* __restrict__ tokens, const float* __restrict__ embed,
                                                         const float* __restrict__ pos, float* __restrict__ out, int d,
                                                         long long vocab, long long pos_a, long long pos_b) {
  const long long b = blockIdx.x;
  long long id = tokens[b];
  id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);   // memory safety only
  const float4* src = reinterpret_cast<const float4*>(embed + id * d);
  const float4* pa = reinterpret_cast<const float4*>(pos + (2 + pos_a) * d);
  const float4* pb = pos_b >= 0 ? reinterpret_cast<const float4*>(pos + (2 + pos_b) * d) : nullptr;
  float4* o = reinterpret_cast<float4*>(out + b * d);
  for (int c = threadIdx.x; c < (d >> 2); c += 256) {
    float4 v = src[c];
    const float4 a1 = pa[c];
    v.x += a1.x; v.y += a1.y; v.z += a1.z; v.w += a1.w;
    if (pb) { const float4 a2 = pb[c]; v.x += a2.x; v.y += a2.y; v.z += a2.z; v.w += a2.w; }
    o[c] = v;
  }
}

}  // namespace

static int sample_impl(const kx_sample_args* args, int32_t* positions, int64_t advance, void* stream, const float* log_min_p = nullptr,
                       const Trunc* trunc = nullptr, const kx_sample_rows_args* rows = nullptr) {
  KX_REQUIRE(args != nullptr, "kx_sample_logits: null args");
  KX_REQUIRE(args->struct_bytes == sizeof(kx_sample_args),
             "kx_sample_logits: stale binding — caller declares kx_sample_args as %u bytes, this library (ABI %d) as %zu",
             (unsigned)args->struct_bytes, KX_ABI_VERSION, sizeof(kx_sample_args));
  KX_REQUIRE(args->logits != nullptr, "kx_sample_logits: null logits");
  KX_REQUIRE(args->next_token != nullptr, "kx_sample_logits: null next_token");
  KX_REQUIRE(args->B >= 1 && args->B <= 0x7fffffffll, "kx_sample_logits: B=%lld must be >= 1", (long long)args->B);
  KX_REQUIRE(args->V >= 1, "kx_sample_logits: V=%lld must be >= 1", (long long)args->V);
  KX_REQUIRE(args->ld >= args->V, "kx_sample_logits: ld=%lld is smaller than V=%lld", (long long)args->ld, (long long)args->V);
  // (rows: the scalar sampling fields are ignored — the table's records were validated by kx_sample_rows_pack)
  KX_REQUIRE(rows || args->temperature >= 0.0f, "kx_sample_logits: temperature=%g must be >= 0", (double)args->temperature);
  KX_REQUIRE(rows || args->top_p > 0.0f, "kx_sample_logits: top_p=%g must be > 0", (double)args->top_p);
  KX_REQUIRE(rows || args->repetition_penalty > 0.0f, "kx_sample_logits: repetition_penalty=%g must be > 0",
             (double)args->repetition_penalty);
  KX_REQUIRE(!rows || !(rows->flags & KX_SAMPLE_ROWS_BUDGET) || args->finished != nullptr,
             "kx_sample_logits_rows: null finished with a row budget in the table (flags bit 1)");
  KX_REQUIRE(args->hist_len >= 0 && args->hist_len <= 0x7fffffffll, "kx_sample_logits: hist_len=%lld must be >= 0",
             (long long)args->hist_len);
  KX_REQUIRE(args->history == nullptr || args->hist_ld > args->hist_len,
             "kx_sample_logits: hist_ld=%lld leaves no room to append after hist_len=%lld", (long long)args->hist_ld,
             (long long)args->hist_len);
  KX_REQUIRE(args->out_tokens == nullptr || (args->out_col >= 0 && args->out_col < args->out_ld),
             "kx_sample_logits: out_col=%lld outside [0, out_ld=%lld)", (long long)args->out_col, (long long)args->out_ld);
  KX_REQUIRE(positions || (args->position >= 0 && args->position <= 0xffffffffll), "kx_sample_logits: position=%lld outside [0, 2^32)",
             (long long)args->position);
  if (args->V > KX_SAMPLE_MAX_V) {
    kx_set_error("kx_sample_logits: V=%lld exceeds %lld (64-bit fixed-point mass)", (long long)args->V, KX_SAMPLE_MAX_V);
    return KX_ERR_UNSUPPORTED;
  }
  SampleParams p;
  p.logits = args->logits; p.ld = args->ld; p.V = (int)args->V;
  p.greedy = (!args->do_sample || args->temperature == 0.0f) ? 1 : 0;
  p.T = args->temperature; p.p = args->top_p; p.r = args->repetition_penalty; p.k = args->top_k;
  const bool penalty = rows ? (rows->flags & KX_SAMPLE_ROWS_PENALTY) != 0 : args->repetition_penalty != 1.0f;
  p.pen = (penalty && args->history != nullptr && args->hist_len > 0) ? 1 : 0;
  if (p.pen && args->V > KX_SAMPLE_MAX_V_PENALTY) {
    kx_set_error("kx_sample_logits: repetition_penalty with V=%lld exceeds %lld (the history bitmap is kept in LDS)",
                 (long long)args->V, KX_SAMPLE_MAX_V_PENALTY);
    return KX_ERR_UNSUPPORTED;
  }
  p.seed = args->seed; p.position = positions ? 0u : (unsigned)args->position;
  p.seq = (const long long*)args->sequence_ids;
  p.history = (long long*)args->history; p.hist_ld = args->hist_ld; p.hist_len = (int)args->hist_len;
  p.finished = args->finished; p.eos = args->eos_id; p.pad = args->pad_id;
  p.next = (long long*)args->next_token; p.out_tokens = (long long*)args->out_tokens;
  p.out_ld = args->out_ld; p.out_col = args->out_col;
  p.kept_count = args->kept_count; p.keep_mask = args->keep_mask;
  const size_t lds = p.pen ? (size_t)((args->V + 31) / 32) * 4 : 0;
  KxProfScope prof(KX_K_MISC, args->B, args->V, 0, (hipStream_t)stream);
  if (rows && positions)
    hipLaunchKernelGGL((sample_kernel<RaggedPos, Rows>), dim3((unsigned)args->B), dim3(SB), lds, (hipStream_t)stream, p,
                       RaggedPos{(int*)positions, (int)advance}, Rows{rows->table, (rows->flags & KX_SAMPLE_ROWS_BUDGET) ? 1 : 0});
  else if (rows)
    hipLaunchKernelGGL(sample_kernel<Rows>, dim3((unsigned)args->B), dim3(SB), lds, (hipStream_t)stream, p,
                       Rows{rows->table, (rows->flags & KX_SAMPLE_ROWS_BUDGET) ? 1 : 0});
  else if (trunc && positions)
    hipLaunchKernelGGL((sample_kernel<RaggedPos, Trunc>), dim3((unsigned)args->B), dim3(SB), lds, (hipStream_t)stream, p,
                       RaggedPos{(int*)positions, (int)advance}, *trunc);
  else if (trunc) hipLaunchKernelGGL(sample_kernel<Trunc>, dim3((unsigned)args->B), dim3(SB), lds, (hipStream_t)stream, p, *trunc);
  else if (log_min_p && positions)
    hipLaunchKernelGGL((sample_kernel<RaggedPos, MinP>), dim3((unsigned)args->B), dim3(SB), lds, (hipStream_t)stream, p,
                       RaggedPos{(int*)positions, (int)advance}, MinP{*log_min_p});
  else if (log_min_p) hipLaunchKernelGGL(sample_kernel<MinP>, dim3((unsigned)args->B), dim3(SB), lds, (hipStream_t)stream, p, MinP{*log_min_p});
  else if (positions) hipLaunchKernelGGL(sample_kernel<RaggedPos>, dim3((unsigned)args->B), dim3(SB), lds, (hipStream_t)stream, p,
                                    RaggedPos{(int*)positions, (int)advance});
  else hipLaunchKernelGGL(sample_kernel<>, dim3((unsigned)args->B), dim3(SB), lds, (hipStream_t)stream, p);
  KX_CHECK_LAUNCH("kx_sample_logits");
  return KX_OK;
}

extern "C" int kx_sample_logits(const kx_sample_args* args, void* stream) { return sample_impl(args, nullptr, 0, stream); }

extern "C" int kx_sample_logits_ragged(const kx_sample_args* args, int32_t* positions, int64_t advance, void* stream) {
  KX_REQUIRE(positions != nullptr, "kx_sample_logits_ragged: null positions");
  KX_REQUIRE(advance >= 0 && advance <= 0x7fffffffll, "kx_sample_logits_ragged: advance=%lld must be >= 0", (long long)advance);
  return sample_impl(args, positions, advance, stream);
}

// min_p == 0: the launches of the two entry points above.  Otherwise lm = log(min_p) in double, rounded once to fp32 (m = 1: +0).
extern "C" int kx_sample_logits_min_p(const kx_sample_args* args, int32_t* positions, int64_t advance, float min_p, void* stream) {
  KX_REQUIRE(min_p >= 0.0f && min_p <= 1.0f, "kx_sample_logits_min_p: min_p=%g must be in [0, 1]", (double)min_p);
  KX_REQUIRE(positions == nullptr || (advance >= 0 && advance <= 0x7fffffffll), "kx_sample_logits_min_p: advance=%lld must be >= 0",
             (long long)advance);
  if (min_p == 0.0f) return sample_impl(args, positions, positions ? advance : 0, stream);
  const float lm = (float)log((double)min_p);
  return sample_impl(args, positions, positions ? advance : 0, stream, &lm);
}

// The three cut-offs at their defaults: kx_sample_logits_min_p's launches.  Otherwise one launch of the Trunc instantiation, min-p inside it.
extern "C" int kx_sample_logits_truncate(const kx_sample_args* args, int32_t* positions, int64_t advance, const kx_truncate_args* trunc,
                                         void* stream) {
  KX_REQUIRE(trunc != nullptr, "kx_sample_logits_truncate: null trunc");
  KX_REQUIRE(trunc->struct_bytes == sizeof(kx_truncate_args),
             "kx_sample_logits_truncate: stale binding — caller declares kx_truncate_args as %u bytes, this library (ABI %d) as %zu",
             (unsigned)trunc->struct_bytes, KX_ABI_VERSION, sizeof(kx_truncate_args));
  KX_REQUIRE(trunc->min_p >= 0.0f && trunc->min_p <= 1.0f, "kx_sample_logits_truncate: min_p=%g must be in [0, 1]", (double)trunc->min_p);
  KX_REQUIRE(trunc->typical_p > 0.0f && trunc->typical_p <= 1.0f, "kx_sample_logits_truncate: typical_p=%g must be in (0, 1]",
             (double)trunc->typical_p);
  KX_REQUIRE(trunc->epsilon_cutoff >= 0.0f && trunc->epsilon_cutoff < 1.0f, "kx_sample_logits_truncate: epsilon_cutoff=%g must be in [0, 1)",
             (double)trunc->epsilon_cutoff);
  KX_REQUIRE(trunc->eta_cutoff >= 0.0f && trunc->eta_cutoff < 1.0f, "kx_sample_logits_truncate: eta_cutoff=%g must be in [0, 1)",
             (double)trunc->eta_cutoff);
  KX_REQUIRE(positions == nullptr || (advance >= 0 && advance <= 0x7fffffffll), "kx_sample_logits_truncate: advance=%lld must be >= 0",
             (long long)advance);
  if (trunc->typical_p == 1.0f && trunc->epsilon_cutoff == 0.0f && trunc->eta_cutoff == 0.0f)
    return kx_sample_logits_min_p(args, positions, advance, trunc->min_p, stream);
  Trunc t;
  t.minp = trunc->min_p != 0.0f;
  t.lm = t.minp ? (float)log((double)trunc->min_p) : 0.0f;
  t.typical = trunc->typical_p; t.epsilon = trunc->epsilon_cutoff; t.eta = trunc->eta_cutoff;
  return sample_impl(args, positions, positions ? advance : 0, stream, nullptr, &t);
}

// One launch of the Rows instantiation (either form), whatever the records hold; the pack function lives in kx_sample_rows.hip.
extern "C" int kx_sample_logits_rows(const kx_sample_args* args, int32_t* positions, int64_t advance, const kx_sample_rows_args* rows,
                                     void* stream) {
  KX_REQUIRE(rows != nullptr, "kx_sample_logits_rows: null rows");
  KX_REQUIRE(rows->struct_bytes == sizeof(kx_sample_rows_args),
             "kx_sample_logits_rows: stale binding — caller declares kx_sample_rows_args as %u bytes, this library (ABI %d) as %zu",
             (unsigned)rows->struct_bytes, KX_ABI_VERSION, sizeof(kx_sample_rows_args));
  KX_REQUIRE(rows->table != nullptr, "kx_sample_logits_rows: null table");
  KX_REQUIRE((rows->flags & ~(KX_SAMPLE_ROWS_PENALTY | KX_SAMPLE_ROWS_BUDGET)) == 0, "kx_sample_logits_rows: flags=%#x beyond bits 0 and 1",
             (unsigned)rows->flags);
  KX_REQUIRE(positions == nullptr || (advance >= 0 && advance <= 0x7fffffffll), "kx_sample_logits_rows: advance=%lld must be >= 0",
             (long long)advance);
  return sample_impl(args, positions, positions ? advance : 0, stream, nullptr, nullptr, rows);
}

// span == 1: kx_step_prepare's launch.  span > 1: B counts the rows, `span` consecutive ones per entry of positions (see the kernel).
int kx_launch_step_prepare(const int64_t* tokens, const float* embed, const float* pos, const int32_t* positions,
                           const float* xq_cs, const float* xq_ss, const float* xk_cs, const float* xk_ss, float* x,
                           float* xpos_rows, int64_t B, int64_t span, int64_t d, int64_t vocab, int64_t max_pos, int64_t pos_shift,
                           int64_t xpos_len, int32_t* error_word, void* stream) {
  KX_REQUIRE(tokens && embed && pos && positions && x && error_word, "kx_step_prepare: null pointer");
  KX_REQUIRE(B > 0 && B <= 0x7fffffffll && d > 0 && d % 4 == 0 && d <= 0x7fffffffll && vocab > 0,
             "kx_step_prepare: bad shape B=%lld d=%lld vocab=%lld", (long long)B, (long long)d, (long long)vocab);
  KX_REQUIRE((((uintptr_t)embed | (uintptr_t)pos | (uintptr_t)x) & 15) == 0, "kx_step_prepare: pointers must be 16-byte aligned");
  KX_REQUIRE(max_pos > 2 && pos_shift >= 0 && pos_shift <= 0x7fffffffll, "kx_step_prepare: bad max_pos=%lld / pos_shift=%lld",
             (long long)max_pos, (long long)pos_shift);
  const bool tabs = xq_cs || xq_ss || xk_cs || xk_ss || xpos_rows;
  KX_REQUIRE(!tabs || (xq_cs && xq_ss && xk_cs && xk_ss && xpos_rows && xpos_len > 0),
             "kx_step_prepare: the four XPos tables, xpos_rows and xpos_len > 0 are given together or not at all");
  KX_REQUIRE(span >= 1 && span <= 0x7fffffffll && B % span == 0, "kx_step_prepare: %lld rows are no multiple of %lld per sequence",
             (long long)B, (long long)span);
  KxProfScope prof(KX_K_EMBED, B, d, 1, (hipStream_t)stream);
  if (span > 1)
    hipLaunchKernelGGL(step_prepare_kernel<SpanRows>, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, (const long long*)tokens, embed,
                       pos, (const int*)positions, xq_cs, xq_ss, xk_cs, xk_ss, x, xpos_rows, (int)B, (int)d, (long long)vocab,
                       (long long)max_pos, (int)pos_shift, (long long)xpos_len, (int*)error_word, SpanRows{(int)span});
  else
    hipLaunchKernelGGL(step_prepare_kernel<>, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, (const long long*)tokens, embed,
                       pos, (const int*)positions, xq_cs, xq_ss, xk_cs, xk_ss, x, xpos_rows, (int)B, (int)d, (long long)vocab,
                       (long long)max_pos, (int)pos_shift, (long long)xpos_len, (int*)error_word);
  KX_CHECK_LAUNCH("kx_step_prepare");
  return KX_OK;
}

extern "C" int kx_step_prepare(const int64_t* tokens, const float* embed, const float* pos, const int32_t* positions,
                               const float* xq_cs, const float* xq_ss, const float* xk_cs, const float* xk_ss, float* x,
                               float* xpos_rows, int64_t B, int64_t d, int64_t vocab, int64_t max_pos, int64_t pos_shift,
                               int64_t xpos_len, int32_t* error_word, void* stream) {
  return kx_launch_step_prepare(tokens, embed, pos, positions, xq_cs, xq_ss, xk_cs, xk_ss, x, xpos_rows, B, 1, d, vocab, max_pos, pos_shift,
                                xpos_len, error_word, stream);
}

extern "C" int kx_embed_step(const int64_t* tokens, const float* embed, const float* pos, float* out, int64_t B,
                             int64_t d, int64_t vocab, int64_t max_pos, int64_t pos_a, int64_t pos_b, void* stream) {
  KX_REQUIRE(tokens && embed && pos && out, "kx_embed_step: null pointer");
  KX_REQUIRE(B > 0 && B <= 0x7fffffffll && d > 0 && d % 4 == 0 && vocab > 0, "kx_embed_step: bad shape B=%lld d=%lld vocab=%lld",
             (long long)B, (long long)d, (long long)vocab);
  KX_REQUIRE((((uintptr_t)embed | (uintptr_t)pos | (uintptr_t)out) & 15) == 0, "kx_embed_step: pointers must be 16-byte aligned");
  // the same condition and wording as kx_embed_splice (the Python boundary turns it into the reference's IndexError)
  KX_REQUIRE(pos_a >= 0 && pos_a + 2 < max_pos, "kx_embed_step: position %lld out of range for a %lld-row table",
             (long long)(pos_a + 2), (long long)max_pos);
  KX_REQUIRE(pos_b < 0 || pos_b + 2 < max_pos, "kx_embed_step: position %lld out of range for a %lld-row table",
             (long long)(pos_b + 2), (long long)max_pos);
  KxProfScope prof(KX_K_EMBED, B, d, 0, (hipStream_t)stream);
  hipLaunchKernelGGL(embed_step_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, (const long long*)tokens,
                     embed, pos, out, (int)d, (long long)vocab, (long long)pos_a, (long long)pos_b);
  KX_CHECK_LAUNCH("kx_embed_step");
  return KX_OK;
}
