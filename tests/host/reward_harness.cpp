// Host harness for the term table of the reward terms (csrc/host_tables.cpp build_reward_table): what the reward kernel reads. Built
// by tests/test_reward_tables_host.py from host_tables.cpp + model.cpp with g++ -fsanitize=address,undefined; no HIP, no stubs.
//
//   reward_harness <file.urdf> <numbers file>
//
// The numbers file holds white-space separated numbers ("nan" and "inf" included): action_cols, T, then T x (kind link mask x y z
// weight p0 p1). Output: one line per part of the table, "name value value ..." (floats with 9 digits: every f32 exactly), or the
// single line "REFUSED <code> <message>" (exit code 0: a refusal is an answer). Exit code 2: bad usage, or the model does not load.
//
//   reward_harness layout <numbers file>
//
// The numbers file holds n A J T: the layout of the terms' history (reward_hist_layout), as layout_check.hpp prints it.
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
  if (argc < 3) { std::fprintf(stderr, "usage: reward_harness <urdf> <numbers file>\n"); return 2; }
  std::vector<double> in;
  {
    std::ifstream f(argv[2]);
    std::string tok;
    while (f >> tok) in.push_back(std::strtod(tok.c_str(), nullptr));
  }
  if (std::string(argv[1]) == "layout") {
    if (in.size() != 4) { std::fprintf(stderr, "numbers file: n A J T\n"); return 2; }
    check_layout("layout", trex::reward_hist_layout((int)in[0], (int)in[1], (int)in[2], (int)in[3]));
    return 0;
  }
  if (in.size() < 2 || in.size() != 2 + 9 * (size_t)in[1]) { std::fprintf(stderr, "numbers file: action_cols, T, T x 9 numbers\n"); return 2; }
  trex::HostModel h;
  try {
    int code = 0;
    h = trex::load_model(argv[1], nullptr, &code);
  } catch (const std::exception &e) {
    std::fprintf(stderr, "model: %s\n", e.what());
    return 2;
  }
  trex::Links links;
  links.body = h.link_body; links.tf = h.link_tf;
  const int action_cols = (int)in[0], T = (int)in[1];
  std::vector<TrexRewardTerm> term((size_t)T);
  for (int k = 0; k < T; k++) {
    const double *x = in.data() + 2 + 9 * (size_t)k;
    term[k].kind = (int32_t)x[0]; term[k].link = (int32_t)x[1]; term[k].mask = (uint32_t)x[2];
    for (int c = 0; c < 3; c++) term[k].local_xyz[c] = (float)x[3 + c];
    term[k].weight = (float)x[6]; term[k].p0 = (float)x[7]; term[k].p1 = (float)x[8];
  }
  try {
    const trex::RewTable t = trex::build_reward_table(links, h.obs_order, h.nb, action_cols, term.data(), T);
    ints("scalars", std::vector<long long>{t.terms, t.action_cols, t.contact, t.actions, t.command, (long long)t.body_mask,
                                           (long long)t.o_joint, (long long)t.blob.size()});
    const TrexRewTerm *e = (const TrexRewTerm *)t.blob.data();   // (a vector's storage: aligned for the struct)
    std::vector<long long> kind, body, mask;
    std::vector<float> tf, point, weight, p0, p1;
    for (int k = 0; k < t.terms; k++) {
      kind.push_back(e[k].kind); body.push_back(e[k].body); mask.push_back(e[k].mask);
      tf.insert(tf.end(), e[k].tf, e[k].tf + 12);
      point.insert(point.end(), e[k].point, e[k].point + 3);
      weight.push_back(e[k].weight); p0.push_back(e[k].p0); p1.push_back(e[k].p1);
    }
    ints("kind", kind); ints("body", body); ints("mask", mask);
    floats("tf", tf); floats("point", point); floats("weight", weight); floats("p0", p0); floats("p1", p1);
    if (t.terms > 0) {
      const int32_t *jb = (const int32_t *)(t.blob.data() + t.o_joint);
      ints("joint_body", std::vector<int32_t>(jb, jb + TREX_TL));
    }
  } catch (const trex::Refusal &r) {
    std::printf("REFUSED %d %s\n", r.code, r.what());
  }
  return 0;
}
