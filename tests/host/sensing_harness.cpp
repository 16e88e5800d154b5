// Host harness for the group table of the sensor model (csrc/host_tables.cpp build_sense_table, check_sense_delay): what the
// sensing kernel reads. Built by tests/test_sensing_tables_host.py from host_tables.cpp + model.cpp with
// g++ -fsanitize=address,undefined; no HIP, no stubs.
//
//   sensing_harness <numbers file>
//
// The numbers file holds white-space separated numbers ("nan" and "inf" included). Either
//   0 obs_dim G, then G x (col0 width noise_kind noise bias quantum delay_min delay_max); or
//   1 delay_min delay_max   (the range check of trex_batch_set_action_delay).
// Output: one line per part, "name value value ..." (floats with 9 digits: every f32 exactly), or the single line
// "REFUSED <code> <message>" (exit code 0: a refusal is an answer). Exit code 2: bad usage.
//
//   sensing_harness layout <numbers file>
//
// The numbers file holds n G delayed action_delay(0/1) action_cols: the layouts of the groups' counters and history and of the
// action delay's (sense_counter_layout, sense_hist_layout), a line each as layout_check.hpp prints it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "layout_check.hpp"

namespace {

template <class T> void ints(const char *name, const std::vector<T> &v) {
  std::printf("%s", name);
  for (const T &x : v) std::printf(" %lld", (long long)x);
  std::printf("\n");
}
void floats(const char *name, const std::vector<float> &v) {
  std::printf("%s", name);
  for (float x : v) std::printf(" %.9g", (double)x);
  std::printf("\n");
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: sensing_harness <numbers file>\n"); return 2; }
  const bool layout = argc > 2 && std::string(argv[1]) == "layout";
  std::vector<double> in;
  {
    std::ifstream f(argv[layout ? 2 : 1]);
    std::string tok;
    while (f >> tok) in.push_back(std::strtod(tok.c_str(), nullptr));
  }
  if (layout) {
    if (in.size() != 5) { std::fprintf(stderr, "numbers file: n G delayed action_delay(0/1) action_cols\n"); return 2; }
    const int n = (int)in[0], on = in[3] != 0.0;
    check_layout("counters", trex::sense_counter_layout(n, (int)in[1]));
    check_layout("hist", trex::sense_hist_layout(n, (int)in[2]));
    check_layout("act_counters", trex::sense_counter_layout(n, on ? 1 : 0));   // (what trex_batch_set_action_delay asks for)
    check_layout("act_hist", trex::sense_hist_layout(n, on ? (int)in[4] : 0));
    return 0;
  }
  try {
    if (in.size() >= 3 && in[0] == 0.0) {
      const int D = (int)in[1], G = (int)in[2];
      const bool count_ok = G >= 0 && G <= TREX_SENSE_MAXGROUPS;   // (a count the builder refuses before it reads: no values needed)
      if (count_ok && in.size() != 3 + 8 * (size_t)G) { std::fprintf(stderr, "numbers file: 0 obs_dim G, then G x 8 values\n"); return 2; }
      std::vector<TrexSenseGroup> groups(count_ok ? (size_t)G : 0);
      for (size_t g = 0; g < groups.size(); g++) {
        const double *x = in.data() + 3 + 8 * g;
        groups[g].col0 = (int32_t)x[0]; groups[g].width = (int32_t)x[1]; groups[g].noise_kind = (int32_t)x[2];
        groups[g].noise = (float)x[3]; groups[g].bias = (float)x[4]; groups[g].quantum = (float)x[5];
        groups[g].delay_min = (int32_t)x[6]; groups[g].delay_max = (int32_t)x[7];
      }
      TrexSenseGroup none{};
      const trex::SenseTable t = trex::build_sense_table(D, count_ok ? (groups.empty() ? &none : groups.data()) : &none, G);
      ints("scalars", std::vector<long long>{t.groups, t.obs_dim, t.delayed, (long long)t.o_col_group, (long long)t.o_col_hist, (long long)t.blob.size()});
      ints("col_group", t.col_group); ints("col_hist", t.col_hist);
      std::vector<long long> col0, width, kind, dmin, dmax;
      std::vector<float> noise, bias, quantum, inv;
      for (const TrexSenseGrp &o : t.group) {
        col0.push_back(o.col0); width.push_back(o.width); kind.push_back(o.kind); dmin.push_back(o.delay_min); dmax.push_back(o.delay_max);
        noise.push_back(o.noise); bias.push_back(o.bias); quantum.push_back(o.quantum); inv.push_back(o.inv_quantum);
      }
      ints("col0", col0); ints("width", width); ints("kind", kind); ints("delay_min", dmin); ints("delay_max", dmax);
      floats("noise", noise); floats("bias", bias); floats("quantum", quantum); floats("inv_quantum", inv);
      // the blob is the three parts, byte for byte
      bool same = t.blob.size() == t.o_col_hist + t.col_hist.size() * sizeof(int16_t);
      if (same && t.groups > 0)
        same = !std::memcmp(t.blob.data(), t.group.data(), t.o_col_group) &&
               !std::memcmp(t.blob.data() + t.o_col_group, t.col_group.data(), t.col_group.size() * sizeof(int16_t)) &&
               !std::memcmp(t.blob.data() + t.o_col_hist, t.col_hist.data(), t.col_hist.size() * sizeof(int16_t));
      ints("blob_is_parts", std::vector<int>{same ? 1 : 0});
    } else if (in.size() == 3 && in[0] == 1.0) {
      trex::check_sense_delay("trex_batch_set_action_delay: ", (int)in[1], (int)in[2]);
      ints("ok", std::vector<int>{1});
    } else {
      std::fprintf(stderr, "numbers file: mode 0 (table) or 1 (delay range), see the header of this file\n");
      return 2;
    }
  } catch (const trex::Refusal &r) {
    std::printf("REFUSED %d %s\n", r.code, r.what());
  }
  return 0;
}
