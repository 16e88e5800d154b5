// Host harness for the term table of the episode randomisation (csrc/host_tables.cpp build_random_table): what
// trex_batch_set_randomization checks and what the randomize kernel reads. Built by tests/test_randomize_tables_host.py from
// host_tables.cpp + model.cpp with g++ -fsanitize=address,undefined; no HIP, no stubs.
//
//   randomize_harness <numbers file>
//
// The numbers file holds white-space separated numbers ("nan" and "inf" included):
//   nb nj stiffness T, then T x (kind mask index shared lo hi interval duration probability).
// Output: one line per part, "name value value ..." (floats with 9 digits: every f32 exactly), or the single line
// "REFUSED <code> <message>" (exit code 0: a refusal is an answer). Exit code 2: bad usage.
//
//   randomize_harness layout <numbers file>
//
// The numbers file holds n T P: the layout of the state (rand_state_layout), as layout_check.hpp prints it.
#include <cstdio>
#include <cstdlib>
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
  if (argc < 2) { std::fprintf(stderr, "usage: randomize_harness <numbers file>\n"); return 2; }
  const bool layout = argc > 2 && std::string(argv[1]) == "layout";
  std::vector<double> in;
  {
    std::ifstream f(argv[layout ? 2 : 1]);
    std::string tok;
    while (f >> tok) in.push_back(std::strtod(tok.c_str(), nullptr));
  }
  if (layout) {
    if (in.size() != 3) { std::fprintf(stderr, "numbers file: n T P\n"); return 2; }
    check_layout("layout", trex::rand_state_layout((int)in[0], (int)in[1], (int)in[2]));
    return 0;
  }
  if (in.size() < 4) { std::fprintf(stderr, "numbers file: nb nj stiffness T, then T x 9 values\n"); return 2; }
  try {
    const int nb = (int)in[0], nj = (int)in[1], T = (int)in[3];
    const bool stiffness = in[2] != 0.0;
    const bool count_ok = T >= 0 && T <= TREX_RAND_MAXTERMS;   // (a count the builder refuses before it reads: no values needed)
    if (count_ok && in.size() != 4 + 9 * (size_t)T) { std::fprintf(stderr, "numbers file: nb nj stiffness T, then T x 9 values\n"); return 2; }
    std::vector<TrexRandomTerm> terms(count_ok ? (size_t)T : 0);
    for (size_t t = 0; t < terms.size(); t++) {
      const double *x = in.data() + 4 + 9 * t;
      terms[t].kind = (int32_t)x[0]; terms[t].mask = (uint32_t)x[1]; terms[t].index = (int32_t)x[2]; terms[t].shared = (int32_t)x[3];
      terms[t].lo = (float)x[4]; terms[t].hi = (float)x[5]; terms[t].interval = (int32_t)x[6]; terms[t].duration = (int32_t)x[7];
      terms[t].probability = (float)x[8];
    }
    TrexRandomTerm none{};
    const trex::RandTable t = trex::build_random_table(nb, nj, stiffness, terms.empty() ? &none : terms.data(), T);
    ints("scalars", std::vector<long long>{t.terms, t.pushes, t.mass, t.friction, t.gains, t.command, (long long)sizeof(TrexRandomTerm)});
    std::vector<long long> kind, mask, index, shared, interval, duration, slot(t.push_slot, t.push_slot + TREX_RAND_MAXTERMS);
    std::vector<float> lo, hi, probability;
    for (const TrexRandomTerm &o : t.term) {
      kind.push_back(o.kind); mask.push_back(o.mask); index.push_back(o.index); shared.push_back(o.shared);
      interval.push_back(o.interval); duration.push_back(o.duration);
      lo.push_back(o.lo); hi.push_back(o.hi); probability.push_back(o.probability);
    }
    ints("kind", kind); ints("mask", mask); ints("index", index); ints("shared", shared); ints("interval", interval);
    ints("duration", duration); ints("push_slot", slot);
    floats("lo", lo); floats("hi", hi); floats("probability", probability);
  } catch (const trex::Refusal &r) {
    std::printf("REFUSED %d %s\n", r.code, r.what());
  }
  return 0;
}
