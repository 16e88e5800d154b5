// Host harness for the term table of the start-state randomisation (csrc/host_tables.cpp build_start_table, check_start_apply,
// start_state_layout): what trex_batch_set_start_state and trex_batch_apply_start_state check and what the start-state kernel
// reads. Built by tests/test_start_state_tables_host.py from host_tables.cpp + model.cpp with g++ -fsanitize=address,undefined; no
// HIP, no stubs.
//
//   start_state_harness <numbers file>
//
// The numbers file holds white-space separated numbers ("nan" and "inf" included):
//   nj n env_offset T, then T x (kind mask index shared lo hi).
// Output: one line per part, "name value value ..." (floats with 9 digits: every f32 exactly), or the single line
// "REFUSED <code> <message>" (exit code 0: a refusal is an answer). Exit code 2: bad usage.
//
//   start_state_harness layout <numbers file>      n T: the layout of the state (start_state_layout), as layout_check.hpp prints it
//   start_state_harness apply <numbers file>       num_terms done done_stride rows row_stride nj pen_in_rows: check_start_apply
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "layout_check.hpp"

namespace {

void ints(const char *name, const std::vector<long long> &v) {
  std::printf("%s", name);
  for (long long x : v) std::printf(" %lld", x);
  std::printf("\n");
}
void floats(const char *name, const std::vector<float> &v) {
  std::printf("%s", name);
  for (float x : v) std::printf(" %.9g", (double)x);
  std::printf("\n");
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: start_state_harness [layout|apply] <numbers file>\n"); return 2; }
  const std::string mode = argc > 2 ? argv[1] : "";
  std::vector<double> in;
  {
    std::ifstream f(argv[argc > 2 ? 2 : 1]);
    std::string tok;
    while (f >> tok) in.push_back(std::strtod(tok.c_str(), nullptr));
  }
  if (mode == "layout") {
    if (in.size() != 2) { std::fprintf(stderr, "numbers file: n T\n"); return 2; }
    check_layout("layout", trex::start_state_layout((int)in[0], (int)in[1]));
    return 0;
  }
  try {
    if (mode == "apply") {
      if (in.size() != 7) { std::fprintf(stderr, "numbers file: num_terms done done_stride rows row_stride nj pen_in_rows\n"); return 2; }
      trex::check_start_apply((int)in[0], in[1] != 0.0, (int)in[2], in[3] != 0.0, (int)in[4], (int)in[5], in[6] != 0.0);
      std::printf("OK\n");
      return 0;
    }
    if (in.size() < 4) { std::fprintf(stderr, "numbers file: nj n env_offset T, then T x 6 values\n"); return 2; }
    const int nj = (int)in[0], n = (int)in[1], T = (int)in[3];
    const bool count_ok = T >= 0 && T <= TREX_START_MAXTERMS;   // (a count the builder refuses before it reads: no values needed)
    if (count_ok && in.size() != 4 + 6 * (size_t)T) { std::fprintf(stderr, "numbers file: nj n env_offset T, then T x 6 values\n"); return 2; }
    std::vector<TrexStartTerm> terms(count_ok ? (size_t)T : 0);
    for (size_t t = 0; t < terms.size(); t++) {
      const double *x = in.data() + 4 + 6 * t;
      terms[t].kind = (int32_t)x[0]; terms[t].mask = (uint32_t)x[1]; terms[t].index = (int32_t)x[2]; terms[t].shared = (int32_t)x[3];
      terms[t].lo = (float)x[4]; terms[t].hi = (float)x[5];
    }
    trex::check_env_offset("trex_batch_set_start_state: ", (uint32_t)in[2], n);   // (what the C entry checks first)
    TrexStartTerm none{};
    const TrexStartTable t = trex::build_start_table(nj, terms.empty() ? &none : terms.data(), T);
    ints("scalars", {t.num_terms, t.rotate, t.clearance_term, (long long)sizeof(TrexStartTerm), (long long)sizeof(TrexStartTable)});
    std::vector<long long> kind, mask, index, shared;
    std::vector<float> lo, hi;
    for (int i = 0; i < t.num_terms; i++) {
      const TrexStartTerm &o = t.term[i];
      kind.push_back(o.kind); mask.push_back(o.mask); index.push_back(o.index); shared.push_back(o.shared);
      lo.push_back(o.lo); hi.push_back(o.hi);
    }
    ints("kind", kind); ints("mask", mask); ints("index", index); ints("shared", shared);
    floats("lo", lo); floats("hi", hi);
  } catch (const trex::Refusal &r) {
    std::printf("REFUSED %d %s\n", r.code, r.what());
  }
  return 0;
}
