// Host harness for the HIP-free part of the episode monitor (csrc/host_tables.cpp monitor_layout and check_monitor_apply): what
// trex_batch_set_monitor and trex_batch_monitor_apply check before any HIP call, and the layout of the monitor's state. Built by
// tests/test_monitor_tables_host.py from host_tables.cpp + model.cpp with g++ -fsanitize=address,undefined; no HIP, no stubs.
//
//   monitor_harness <numbers file>
//
// The numbers file holds white-space separated numbers:
//   n window cols_a cols_b env_offset block, then optionally the apply's arguments:
//   reward(0/1) reward_stride done(0/1) done_stride block_a(0/1) stride_a block_b(0/1) stride_b.
// Output: one line per part, "name value value ...", or the single line "REFUSED <code> <message>" (exit code 0: a refusal is an
// answer). The layout line is layout_check.hpp's, over the members the layout lists itself. Exit code 2: bad usage.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "layout_check.hpp"

int main(int argc, char **argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: monitor_harness <numbers file>\n"); return 2; }
  std::vector<double> in;
  {
    std::ifstream f(argv[1]);
    std::string tok;
    while (f >> tok) in.push_back(std::strtod(tok.c_str(), nullptr));
  }
  if (in.size() != 6 && in.size() != 14) { std::fprintf(stderr, "numbers file: 6 or 14 numbers\n"); return 2; }
  try {
    const int n = (int)in[0], window = (int)in[1], cols_a = (int)in[2], cols_b = (int)in[3], block = (int)in[5];
    const uint32_t env_offset = (uint32_t)in[4];
    const trex::MonitorLayout m = trex::monitor_layout(n, window, cols_a, cols_b, env_offset, block);
    if (in.size() == 14)
      trex::check_monitor_apply(m, in[6] != 0, (int)in[7], in[8] != 0, (int)in[9], in[10] != 0, (int)in[11], in[12] != 0, (int)in[13]);
    std::printf("shape %d %d %d %d %d %d\n", m.window, m.cols_a, m.cols_b, m.cols, m.team, m.groups);
    check_layout("layout", m);
  } catch (const trex::Refusal &r) {
    std::printf("REFUSED %d %s\n", r.code, r.what());
  }
  return 0;
}
