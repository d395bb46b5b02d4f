// Classifier-free guidance (kx_guidance_logits): two raw fp32 logits rows per sequence — the conditional one and the unconditional
// one, rows b and B + b of the 2B-row ragged batch generate() runs under guidance — combined into the guided row
// out = lu + s * (lc - lu) over their log-softmaxes, in front of the constraint, automaton and shaping launches and the sampler.
// Contract: include/kosmosx_hip.h.
//
// One launch, one 256-thread workgroup per pair, no hand-off between workgroups.  Both log-sum-exps come from block_max_sumexp's
// two halves (kx_common.h), so lc_i and lu_i are bit for bit what kx_token_logprob gives for the row and id i; the combine is a subtract, a
// multiply and an add in IEEE fp32 (contraction is off in this file's kernel), so a numpy float32 restatement over the device's own
// log-probs matches bit for bit.  Every read of cond[i] happens in the thread that later writes out[i], and both reductions end
// behind barriers before the first write: out may be cond.  Nothing read from device memory becomes an index.
#include "kx_common.h"

namespace {

constexpr int HB = 256;                  // threads per workgroup: what block_max_sumexp is written for
constexpr long long KX_GUIDANCE_MAX_V = 1ll << 23;   // kx_sample_logits' own limit: the kernel that reads the row in the end

struct GuidanceParams {
  const float* cond; long long ld_cond;
  const float* uncond; long long ld_uncond;
  float* out; long long ld_out;
  int V; float scale;
  const unsigned char* finished;
  int* positions; int advance;
};

__global__ __launch_bounds__(HB) void guidance_kernel(const GuidanceParams a) {
#pragma clang fp contract(off)
  __shared__ float red[4];
  const long long b = blockIdx.x;
  // the unconditional row moves exactly when its partner does: kx_sample_logits_ragged's rule, finished rows included
  if (a.positions && a.advance && threadIdx.x == 0) a.positions[b] = a.positions[b] + a.advance;
  if (a.finished && a.finished[b]) return;              // (uniform: one byte, read by every thread) nothing read, nothing written
  const float* c = a.cond + b * a.ld_cond;              // (no __restrict__: out may be cond)
  const float* u = a.uncond + b * a.ld_uncond;
  float* o = a.out + b * a.ld_out;
  const int V = a.V;
  // block_max_sumexp of both rows, taken through its two halves (kx_common.h): the maxima of the two rows in ONE pass with sixteen
  // loads in flight — a maximum is exact in any order — then block_sumexp per row, whose summation order is the shared one.  A
  // single workgroup walks 2 x 256 KB at V = 64007: what it waits for is load latency, not bandwidth.
  float mc = -INFINITY, mu = -INFINITY;
  int i = threadIdx.x;
  for (; i < V - 7 * HB; i += 8 * HB) {
    float x[8], y[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) x[k] = c[i + k * HB];
#pragma unroll
    for (int k = 0; k < 8; ++k) y[k] = u[i + k * HB];
#pragma unroll
    for (int k = 0; k < 8; ++k) { mc = fmaxf(mc, x[k]); mu = fmaxf(mu, y[k]); }
  }
  for (; i < V; i += HB) { mc = fmaxf(mc, c[i]); mu = fmaxf(mu, u[i]); }
  mc = block_max_finish(mc, red);
  mu = block_max_finish(mu, red);
  const float sc = block_sumexp(c, V, red, mc);
  __syncthreads();                                      // (block_sumexp ends on a read of `red`)
  const float su = block_sumexp(u, V, red, mu);
  const float lsc = logf(sc), lsu = logf(su);
  const float ninf = -__builtin_inff();
  auto guided = [&](float ci, float ui) {
    const float lc = (ci - mc) - lsc;                   // kx_token_logprob's expression
    const float lu = (ui - mu) - lsu;
    const float d = lc - lu;
    const float t = a.scale * d;
    const float g = lu + t;
    return (g - g == 0.0f) ? g : ninf;                  // (x - x == 0 holds for finite values only) never a candidate otherwise
  };
  i = threadIdx.x;                                      // the thread that writes out[i] is the one that read cond[i]: out may be cond
  for (; i < V - 7 * HB; i += 8 * HB) {
    float x[8], y[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) x[k] = c[i + k * HB];
#pragma unroll
    for (int k = 0; k < 8; ++k) y[k] = u[i + k * HB];
#pragma unroll
    for (int k = 0; k < 8; ++k) o[i + k * HB] = guided(x[k], y[k]);
  }
  for (; i < V; i += HB) o[i] = guided(c[i], u[i]);
}

// [p, p + (B - 1) * ld + V) of two fp32 row sets share an element
bool rows_overlap(const float* p, long long ldp, const float* q, long long ldq, long long B, long long V) {
  const uintptr_t p0 = (uintptr_t)p, p1 = p0 + (uintptr_t)(((B - 1) * ldp + V) * 4);
  const uintptr_t q0 = (uintptr_t)q, q1 = q0 + (uintptr_t)(((B - 1) * ldq + V) * 4);
  return p0 < q1 && q0 < p1;
}

}  // namespace

extern "C" int kx_guidance_logits(const kx_guidance_args* args, void* stream) {
  KX_REQUIRE(args != nullptr, "kx_guidance_logits: null args");
  KX_REQUIRE(args->struct_bytes == sizeof(kx_guidance_args),
             "kx_guidance_logits: stale binding — caller declares kx_guidance_args as %u bytes, this library (ABI %d) as %zu",
             (unsigned)args->struct_bytes, KX_ABI_VERSION, sizeof(kx_guidance_args));
  KX_REQUIRE(args->cond != nullptr, "kx_guidance_logits: null cond");
  KX_REQUIRE(args->uncond != nullptr, "kx_guidance_logits: null uncond");
  KX_REQUIRE(args->out != nullptr, "kx_guidance_logits: null out");
  KX_REQUIRE(args->B >= 1 && args->B <= 0x7fffffffll, "kx_guidance_logits: B=%lld must be >= 1", (long long)args->B);
  KX_REQUIRE(args->V >= 1, "kx_guidance_logits: V=%lld must be >= 1", (long long)args->V);
  if (args->V > KX_GUIDANCE_MAX_V) {
    kx_set_error("kx_guidance_logits: V=%lld exceeds %lld (the limit of kx_sample_logits, which reads the row in the end)",
                 (long long)args->V, KX_GUIDANCE_MAX_V);
    return KX_ERR_UNSUPPORTED;
  }
  KX_REQUIRE(args->ld_cond >= args->V, "kx_guidance_logits: ld_cond=%lld is smaller than V=%lld", (long long)args->ld_cond,
             (long long)args->V);
  KX_REQUIRE(args->ld_uncond >= args->V, "kx_guidance_logits: ld_uncond=%lld is smaller than V=%lld", (long long)args->ld_uncond,
             (long long)args->V);
  KX_REQUIRE(args->ld_out >= args->V, "kx_guidance_logits: ld_out=%lld is smaller than V=%lld", (long long)args->ld_out,
             (long long)args->V);
  KX_REQUIRE(args->scale - args->scale == 0.0f, "kx_guidance_logits: scale=%g must be finite", (double)args->scale);
  KX_REQUIRE(args->advance == 0 || args->advance == 1, "kx_guidance_logits: advance=%lld must be 0 or 1", (long long)args->advance);
  KX_REQUIRE(!rows_overlap(args->out, args->ld_out, args->uncond, args->ld_uncond, args->B, args->V),
             "kx_guidance_logits: out overlaps uncond (out may be cond, never uncond)");
  KX_REQUIRE((args->out == args->cond && args->ld_out == args->ld_cond) ||
                 !rows_overlap(args->out, args->ld_out, args->cond, args->ld_cond, args->B, args->V),
             "kx_guidance_logits: out overlaps cond without being cond (in place means the same pointer and the same ld)");
  GuidanceParams p;
  p.cond = args->cond; p.ld_cond = args->ld_cond; p.uncond = args->uncond; p.ld_uncond = args->ld_uncond;
  p.out = args->out; p.ld_out = args->ld_out; p.V = (int)args->V; p.scale = args->scale;
  p.finished = args->finished; p.positions = args->positions; p.advance = (int)args->advance;
  KxProfScope prof(KX_K_MISC, args->B, args->V, 33, (hipStream_t)stream);
  hipLaunchKernelGGL(guidance_kernel, dim3((unsigned)args->B), dim3(HB), 0, (hipStream_t)stream, p);
  KX_CHECK_LAUNCH("kx_guidance_logits");
  return KX_OK;
}
