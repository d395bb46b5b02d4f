// The GEMM planner on its own, for host sanitizers: plans every case of the golden table's argument list (written by
// `python tools/gemm_plan_golden.py --args-out args.txt`: name|cus|key=value,...|word:hex ... with the non-zero 32-bit words of
// kx_gemm_args) and prints one line per case.  No HIP, no Python:
//   clang++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/gemm_plan_main.cpp -o gemm_plan_main
//   ./gemm_plan_main args.txt
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "../kosmos-x_amd/csrc/kx_gemm_plan.h"

int main(int argc, char** argv) {
  if (argc < 2) { std::cerr << "usage: gemm_plan_main <gemm_plan_args.txt>\n"; return 2; }
  std::ifstream in(argv[1]);
  if (!in) { std::cerr << "cannot read " << argv[1] << "\n"; return 2; }
  std::string line;
  int cases = 0, refused = 0;
  while (std::getline(in, line)) {
    if (line.empty()) continue;
    std::vector<std::string> f;
    std::stringstream ls(line);
    for (std::string part; std::getline(ls, part, '|');) f.push_back(part);
    if (f.size() < 3) { std::cerr << "malformed line: " << line << "\n"; return 2; }
    if (f.size() < 4) f.push_back("");
    KxTuning tn;
    memset(&tn, 0, sizeof(tn));
    std::stringstream ts(f[2]);
    for (std::string kv; std::getline(ts, kv, ',');) {
      const size_t eq = kv.find('=');
      const int key = std::stoi(kv.substr(0, eq));
      if (key < 0 || key >= KX_TUNE_COUNT) { std::cerr << "bad tuning key in: " << line << "\n"; return 2; }
      tn.v[key] = std::stoi(kv.substr(eq + 1));
    }
    uint32_t words[sizeof(kx_gemm_args) / 4 + 1] = {0};
    std::stringstream ws(f[3]);
    for (std::string iw; ws >> iw;) {
      const size_t colon = iw.find(':');
      const size_t idx = std::stoul(iw.substr(0, colon));
      if (idx >= sizeof(kx_gemm_args) / 4) { std::cerr << "word index out of range in: " << line << "\n"; return 2; }
      words[idx] = (uint32_t)std::stoul(iw.substr(colon + 1), nullptr, 16);
    }
    kx_gemm_args a;
    memcpy(&a, words, sizeof(a));
    KxGemmPlan pl;
    const int rc = kx_gemm_plan(a, tn, std::stoi(f[1]), &pl);
    ++cases;
    if (rc != KX_OK) { ++refused; std::cout << f[0] << " refused " << rc << " " << pl.msg << "\n"; continue; }
    std::cout << f[0] << " tile=" << pl.tile << " kind=" << pl.kind << " family=" << pl.family << " elem=" << pl.elem << " " << pl.BM << "x" << pl.BN
              << " ACT=" << pl.ACT << " EPI=" << pl.EPI << " NST=" << pl.NST << " KS2=" << pl.KS2 << " BAL=" << pl.BAL << " COOP=" << pl.COOP
              << " grid=" << pl.grid_x << "x" << pl.grid_y << " reduce=" << pl.reduce << "\n";
  }
  std::cerr << cases << " cases planned, " << refused << " refused\n";
  return cases > 0 ? 0 : 1;
}
