// Host harness for the clip table and the term list of the motion clip (csrc/host_tables.cpp build_motion_table,
// build_motion_terms): what the motion kernels read. Built by tests/test_motion_tables_host.py from host_tables.cpp + model.cpp with
// g++ -fsanitize=address,undefined; no HIP, no stubs.
//
//   motion_harness <file.urdf> <numbers file>
//
// The numbers file holds white-space separated numbers ("nan" and "inf" included). Either
//   0 F frame_dt loop has_velocities, then F x (7 + J) frame values, then - has_velocities - F x (6 + J) velocity values; or
//   1 has_probes step_weight T, then T x (kind mask weight scale aux).
// Output: one line per part, "name value value ..." (floats with 9 digits: every f32 exactly), or the single line
// "REFUSED <code> <message>" (exit code 0: a refusal is an answer). Exit code 2: bad usage, or the model does not load.
//
//   motion_harness layout <numbers file>
//
// The numbers file holds n T: the layouts of the clocks (motion_clock_layout) and of the terms' held values (motion_held_layout),
// a line each as layout_check.hpp prints it.
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
  if (argc < 3) { std::fprintf(stderr, "usage: motion_harness <urdf> <numbers file>\n"); return 2; }
  std::vector<double> in;
  {
    std::ifstream f(argv[2]);
    std::string tok;
    while (f >> tok) in.push_back(std::strtod(tok.c_str(), nullptr));
  }
  if (std::string(argv[1]) == "layout") {
    if (in.size() != 2) { std::fprintf(stderr, "numbers file: n T\n"); return 2; }
    check_layout("clock", trex::motion_clock_layout((int)in[0]));
    check_layout("held", trex::motion_held_layout((int)in[0], (int)in[1]));
    return 0;
  }
  trex::HostModel h;
  try {
    int code = 0;
    h = trex::load_model(argv[1], nullptr, &code);
  } catch (const std::exception &e) {
    std::fprintf(stderr, "model: %s\n", e.what());
    return 2;
  }
  const int J = h.nb - 1;
  try {
    if (in.size() >= 5 && in[0] == 0.0) {
      const int F = (int)in[1], has_vel = (int)in[4];
      const bool count_ok = F >= 0 && F <= TREX_MOT_MAXFRAMES;   // (a count the builder refuses before it reads: no values needed)
      const size_t nf = count_ok ? (size_t)F * (7 + J) : 0, nv = has_vel && count_ok ? (size_t)F * (6 + J) : 0;
      if (count_ok && in.size() != 5 + nf + nv) { std::fprintf(stderr, "numbers file: 0 F frame_dt loop has_velocities, frames, velocities\n"); return 2; }
      const double *frames = in.data() + 5, *vel = has_vel ? frames + nf : nullptr;
      const trex::MotionTable t = trex::build_motion_table(h.q_lower, h.q_upper, h.obs_order, frames, vel, F, in[2], (int)in[3]);
      ints("scalars", std::vector<long long>{t.frames, t.nj, t.stride, t.loop, (long long)t.rows.size()});
      floats("constants", std::vector<float>{t.frame_dt, t.inv_dt, t.duration, t.inv_duration, t.disp[0], t.disp[1]});
      floats("rows", t.rows);
    } else if (in.size() >= 4 && in[0] == 1.0 && in.size() == 4 + 5 * (size_t)in[3]) {
      const int T = (int)in[3];
      std::vector<TrexMotionTerm> term((size_t)T);
      for (int k = 0; k < T; k++) {
        const double *x = in.data() + 4 + 5 * (size_t)k;
        term[k].kind = (int32_t)x[0]; term[k].mask = (uint32_t)x[1];
        term[k].weight = (float)x[2]; term[k].scale = (float)x[3]; term[k].aux = (float)x[4];
      }
      const std::vector<TrexMotTerm> out = trex::build_motion_terms(J, in[1] != 0.0, term.data(), T, (float)in[2]);
      std::vector<long long> kind, mask;
      std::vector<float> weight, scale, aux;
      for (const TrexMotTerm &o : out) {
        kind.push_back(o.kind); mask.push_back(o.mask);
        weight.push_back(o.weight); scale.push_back(o.scale); aux.push_back(o.aux);
      }
      ints("kind", kind); ints("mask", mask);
      floats("weight", weight); floats("scale", scale); floats("aux", aux);
    } else {
      std::fprintf(stderr, "numbers file: mode 0 (table) or 1 (terms), see the header of this file\n");
      return 2;
    }
  } catch (const trex::Refusal &r) {
    std::printf("REFUSED %d %s\n", r.code, r.what());
  }
  return 0;
}
