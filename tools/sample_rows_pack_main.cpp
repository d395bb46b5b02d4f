// kx_sample_rows_pack on its own, for host sanitizers: good tables (out-of-place, in place, one record, many), every refusal, and
// the edges of the ranges; prints one line per case and exits non-zero when a result is not the expected one.  No device, no Python:
//   hipcc --offload-arch=gfx950 -std=c++17 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//     kosmos-x_amd/csrc/kx_sample_rows.hip -x hip tools/sample_rows_pack_main.cpp -o sample_rows_pack_main && ./sample_rows_pack_main
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../include/kosmosx_hip.h"

static char g_error[512];
void kx_set_error(const char* fmt, ...) {   // the library's error plumbing, here a plain buffer
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_error, sizeof(g_error), fmt, ap);
  va_end(ap);
}

static kx_sample_row off() {
  kx_sample_row r;
  memset(&r, 0, sizeof(r));
  r.temperature = 1.0f; r.top_p = 1.0f; r.repetition_penalty = 1.0f; r.typical_p = 1.0f;
  return r;
}

static int failures = 0;
static void expect(bool ok, const char* what) {
  printf("%s %s\n", ok ? "ok  " : "FAIL", what);
  failures += !ok;
}

int main() {
  // good tables of 1 .. 1000 records, packed into a second array of exactly B records and then in place
  for (int B : {1, 2, 7, 1000}) {
    std::vector<kx_sample_row> in(B), out(B);
    for (int b = 0; b < B; ++b) {
      in[b] = off();
      in[b].do_sample = b & 1;
      in[b].min_p = b % 3 == 0 ? 0.0f : 1.0f / (float)(b + 1);
      in[b].repetition_penalty = b == B - 1 ? 1.25f : 1.0f;
      in[b].max_new = b == 0 ? 3 : 0;
      in[b].seed = 0xffffffffffffffffull - (uint64_t)b;
      in[b].log_min_p = 123.0f; in[b].reserved = 77;          // what the caller left there does not matter
    }
    uint32_t flags = 0xdeadu;
    int rc = kx_sample_rows_pack(in.data(), B, 64007, out.data(), &flags);
    bool ok = rc == KX_OK && flags == (KX_SAMPLE_ROWS_PENALTY | KX_SAMPLE_ROWS_BUDGET);
    for (int b = 0; b < B && ok; ++b) {
      const float lm = in[b].min_p != 0.0f ? (float)log((double)in[b].min_p) : 0.0f;
      ok = memcmp(&out[b].log_min_p, &lm, 4) == 0 && out[b].reserved == 0 && out[b].seed == in[b].seed && in[b].log_min_p == 123.0f;
    }
    expect(ok, "a good table, out of place");
    flags = 0;
    rc = kx_sample_rows_pack(in.data(), B, 64007, in.data(), &flags);
    expect(rc == KX_OK && memcmp(in.data(), out.data(), sizeof(kx_sample_row) * (size_t)B) == 0, "the same table in place");
  }
  // the edges of the ranges are accepted
  {
    kx_sample_row r = off();
    r.temperature = 0.0f; r.top_p = 1e-30f; r.min_p = 1.0f; r.typical_p = 1e-30f; r.epsilon_cutoff = 0.99999994f; r.eta_cutoff = 0.0f;
    r.max_new = 0x7fffffff;
    uint32_t flags = 0;
    expect(kx_sample_rows_pack(&r, 1, 1, &r, &flags) == KX_OK && r.log_min_p == 0.0f && flags == KX_SAMPLE_ROWS_BUDGET, "the edges of the ranges");
  }
  // every refusal names the row and the field and writes nothing
  struct Bad { const char* field; size_t offset; float value; };
  const float nan = nanf("");
  const Bad bad[] = {{"temperature", offsetof(kx_sample_row, temperature), -1.0f}, {"temperature", offsetof(kx_sample_row, temperature), nan},
                     {"top_p", offsetof(kx_sample_row, top_p), 0.0f}, {"top_p", offsetof(kx_sample_row, top_p), nan},
                     {"repetition_penalty", offsetof(kx_sample_row, repetition_penalty), 0.0f},
                     {"repetition_penalty", offsetof(kx_sample_row, repetition_penalty), nan},
                     {"min_p", offsetof(kx_sample_row, min_p), -0.5f}, {"min_p", offsetof(kx_sample_row, min_p), 1.5f},
                     {"min_p", offsetof(kx_sample_row, min_p), nan}, {"typical_p", offsetof(kx_sample_row, typical_p), 0.0f},
                     {"typical_p", offsetof(kx_sample_row, typical_p), 2.0f}, {"typical_p", offsetof(kx_sample_row, typical_p), nan},
                     {"epsilon_cutoff", offsetof(kx_sample_row, epsilon_cutoff), 1.0f}, {"epsilon_cutoff", offsetof(kx_sample_row, epsilon_cutoff), nan},
                     {"eta_cutoff", offsetof(kx_sample_row, eta_cutoff), -1e-3f}, {"eta_cutoff", offsetof(kx_sample_row, eta_cutoff), nan}};
  for (const Bad& c : bad) {
    for (int at : {0, 4}) {
      kx_sample_row in[5], out[5];
      for (auto& r : in) r = off();
      memset(out, 0x5a, sizeof(out));
      memcpy((char*)&in[at] + c.offset, &c.value, 4);
      uint32_t flags = 0xdeadu;
      g_error[0] = 0;
      const int rc = kx_sample_rows_pack(in, 5, 100, out, &flags);
      char want[64];
      snprintf(want, sizeof(want), "row %d: %s", at, c.field);
      bool untouched = flags == 0xdeadu;
      for (size_t i = 0; i < sizeof(out); ++i) untouched = untouched && ((unsigned char*)out)[i] == 0x5a;
      char what[128];
      snprintf(what, sizeof(what), "refused: %s", g_error);
      expect(rc == KX_ERR_INVALID_ARG && strstr(g_error, want) != nullptr && untouched, what);
    }
  }
  {
    kx_sample_row r = off();
    r.max_new = -1;
    uint32_t flags = 0;
    expect(kx_sample_rows_pack(&r, 1, 10, &r, &flags) == KX_ERR_INVALID_ARG && strstr(g_error, "row 0: max_new"), "a negative budget");
    r = off();
    expect(kx_sample_rows_pack(nullptr, 1, 10, &r, &flags) == KX_ERR_INVALID_ARG, "null in");
    expect(kx_sample_rows_pack(&r, 1, 10, nullptr, &flags) == KX_ERR_INVALID_ARG, "null out");
    expect(kx_sample_rows_pack(&r, 1, 10, &r, nullptr) == KX_ERR_INVALID_ARG, "null flags_out");
    expect(kx_sample_rows_pack(&r, 0, 10, &r, &flags) == KX_ERR_INVALID_ARG, "B = 0");
    expect(kx_sample_rows_pack(&r, -3, 10, &r, &flags) == KX_ERR_INVALID_ARG, "B < 0");
    expect(kx_sample_rows_pack(&r, 1, 0, &r, &flags) == KX_ERR_INVALID_ARG, "V = 0");
  }
  printf("%d failures\n", failures);
  return failures ? 1 : 0;
}
