// kx_sample_rows_pack: the host half of the per-row sampling table (kx_sample_logits_rows; contract: include/kosmosx_hip.h).
// Host only and pure — no device, no runtime call — so it is callable on a machine without a GPU, and this file holds nothing else:
// it can be compiled alone, next to a main of its own, under a host sanitizer.
#include <math.h>
#include "kx_common.h"

// The rules of kx_sample_logits, kx_sample_logits_min_p and kx_sample_logits_truncate, per record; a NaN fails every compare.
extern "C" int kx_sample_rows_pack(const kx_sample_row* in, int64_t B, int64_t V, kx_sample_row* out, uint32_t* flags_out) {
  KX_REQUIRE(in != nullptr, "kx_sample_rows_pack: null in");
  KX_REQUIRE(out != nullptr, "kx_sample_rows_pack: null out");
  KX_REQUIRE(flags_out != nullptr, "kx_sample_rows_pack: null flags_out");
  KX_REQUIRE(B >= 1 && B <= 0x7fffffffll, "kx_sample_rows_pack: B=%lld must be >= 1", (long long)B);
  KX_REQUIRE(V >= 1, "kx_sample_rows_pack: V=%lld must be >= 1", (long long)V);
  for (int64_t b = 0; b < B; ++b) {
    const kx_sample_row& r = in[b];
    const long long row = (long long)b;
    KX_REQUIRE(r.temperature >= 0.0f, "kx_sample_rows_pack: row %lld: temperature=%g must be >= 0", row, (double)r.temperature);
    KX_REQUIRE(r.top_p > 0.0f, "kx_sample_rows_pack: row %lld: top_p=%g must be > 0", row, (double)r.top_p);
    KX_REQUIRE(r.repetition_penalty > 0.0f, "kx_sample_rows_pack: row %lld: repetition_penalty=%g must be > 0", row,
               (double)r.repetition_penalty);
    KX_REQUIRE(r.min_p >= 0.0f && r.min_p <= 1.0f, "kx_sample_rows_pack: row %lld: min_p=%g must be in [0, 1]", row, (double)r.min_p);
    KX_REQUIRE(r.typical_p > 0.0f && r.typical_p <= 1.0f, "kx_sample_rows_pack: row %lld: typical_p=%g must be in (0, 1]", row,
               (double)r.typical_p);
    KX_REQUIRE(r.epsilon_cutoff >= 0.0f && r.epsilon_cutoff < 1.0f, "kx_sample_rows_pack: row %lld: epsilon_cutoff=%g must be in [0, 1)",
               row, (double)r.epsilon_cutoff);
    KX_REQUIRE(r.eta_cutoff >= 0.0f && r.eta_cutoff < 1.0f, "kx_sample_rows_pack: row %lld: eta_cutoff=%g must be in [0, 1)", row,
               (double)r.eta_cutoff);
    KX_REQUIRE(r.max_new >= 0, "kx_sample_rows_pack: row %lld: max_new=%d must be >= 0 (0 = no budget)", row, (int)r.max_new);
  }
  uint32_t flags = 0;
  for (int64_t b = 0; b < B; ++b) {                     // (every record is valid: nothing is written before that is known)
    kx_sample_row r = in[b];                            // a copy: in == out is allowed
    r.log_min_p = r.min_p != 0.0f ? (float)log((double)r.min_p) : 0.0f;
    r.reserved = 0;
    if (r.repetition_penalty != 1.0f) flags |= KX_SAMPLE_ROWS_PENALTY;
    if (r.max_new > 0) flags |= KX_SAMPLE_ROWS_BUDGET;
    out[b] = r;
  }
  *flags_out = flags;
  return KX_OK;
}
