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
// answer). With the layout the harness makes the allocation on the host, writes every member's first and last byte and checks that
// no two members share one: an overlap or an overrun is the sanitizer's to report. Exit code 2: bad usage.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "../../trex-gym_amd/csrc/host_tables.hpp"

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
    const size_t N = (size_t)n, C = (size_t)m.cols, W = (size_t)m.window;
    struct Member { const char *name; size_t at, bytes, align; };
    const std::vector<Member> members = {
        {"ret", m.ret, N * 8, 8}, {"col", m.col, N * C * 8, 8}, {"total", m.total, 8, 8}, {"by_reason", m.by_reason, 32, 8},
        {"len", m.len, N * 4, 4}, {"episodes", m.episodes, N * 4, 4}, {"fin", m.fin, N * 4, 4},
        {"last_return", m.last_return, N * 4, 4}, {"last_length", m.last_length, N * 4, 4}, {"last_reason", m.last_reason, N * 4, 4},
        {"last_t", m.last_t, N * 4, 4}, {"last_cols", m.last_cols, N * C * 4, 4}, {"t", m.t, 4, 4},
        {"ring_return", m.ring_return, W * 4, 4}, {"ring_length", m.ring_length, W * 4, 4}, {"ring_reason", m.ring_reason, W * 4, 4},
        {"ring_env", m.ring_env, W * 4, 4}, {"ring_t", m.ring_t, W * 4, 4}, {"ring_cols", m.ring_cols, W * C * 4, 4},
        {"counts", m.counts, (size_t)m.groups * 4, 4}};
    std::vector<unsigned char> state(m.bytes, 0);
    long long clashes = 0, misaligned = 0;
    if (m.window > 0) {
      for (const Member &k : members) {
        if (k.at % k.align) misaligned++;
        for (size_t i = 0; i < k.bytes; i++) {
          if (state.at(k.at + i)) clashes++;
          state[k.at + i] = 1;
        }
      }
    }
    long long unused = 0;
    for (unsigned char c : state) unused += c ? 0 : 1;
    std::printf("layout %lld %lld %lld %lld\n", (long long)m.bytes, clashes, misaligned, unused);
  } catch (const trex::Refusal &r) {
    std::printf("REFUSED %d %s\n", r.code, r.what());
  }
  return 0;
}
