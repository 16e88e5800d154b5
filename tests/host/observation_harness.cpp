// Host harness for the channel table of the observation channels (csrc/host_tables.cpp build_obs_table): what the compose kernel
// reads. Built by tests/test_observation_tables_host.py from host_tables.cpp + model.cpp with g++ -fsanitize=address,undefined; no
// HIP, no stubs.
//
//   observation_harness <file.urdf> <numbers file>
//
// The numbers file holds white-space separated numbers ("nan" and "inf" included): action_cols, C, then C x (kind link x y z scale).
// Output: one line per part of the table, "name value value ..." (floats with 9 digits: every f32 exactly), or the single line
// "REFUSED <code> <message>" (exit code 0: a refusal is an answer). Exit code 2: bad usage, or the model does not load.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "../../trex-gym_amd/csrc/host_tables.hpp"

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
  if (argc < 3) { std::fprintf(stderr, "usage: observation_harness <urdf> <numbers file>\n"); return 2; }
  std::vector<double> in;
  {
    std::ifstream f(argv[2]);
    std::string tok;
    while (f >> tok) in.push_back(std::strtod(tok.c_str(), nullptr));
  }
  if (in.size() < 2 || in.size() != 2 + 6 * (size_t)in[1]) { std::fprintf(stderr, "numbers file: action_cols, C, C x 6 numbers\n"); return 2; }
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
  const int action_cols = (int)in[0], C = (int)in[1];
  std::vector<TrexObsChannel> ch((size_t)C);
  for (int k = 0; k < C; k++) {
    const double *x = in.data() + 2 + 6 * (size_t)k;
    ch[k].kind = (int32_t)x[0]; ch[k].link = (int32_t)x[1];
    for (int c = 0; c < 3; c++) ch[k].local_xyz[c] = (float)x[2 + c];
    ch[k].scale = (float)x[5];
  }
  try {
    const trex::ObsTable t = trex::build_obs_table(links, h.nb - 1, action_cols, ch.data(), C);
    ints("scalars", std::vector<long long>{t.channels, t.extra, t.extern_cols, t.action_cols, t.contact, t.actions, (long long)t.body_mask,
                                           (long long)t.o_col, (long long)t.blob.size()});
    const TrexObsChan *chan = (const TrexObsChan *)t.blob.data();   // (a vector's storage: aligned for the struct)
    std::vector<int32_t> kind, body, col0, width;
    std::vector<float> tf, point, scale;
    for (int k = 0; k < t.channels; k++) {
      kind.push_back(chan[k].kind); body.push_back(chan[k].body); col0.push_back(chan[k].col0); width.push_back(chan[k].width);
      tf.insert(tf.end(), chan[k].tf, chan[k].tf + 12);
      point.insert(point.end(), chan[k].point, chan[k].point + 3);
      scale.push_back(chan[k].scale);
    }
    ints("kind", kind); ints("body", body); ints("col0", col0); ints("width", width);
    floats("tf", tf); floats("point", point); floats("scale", scale);
    const uint8_t *cc = (const uint8_t *)t.blob.data() + t.o_col;
    ints("col_chan", std::vector<int>(cc, cc + t.extra));
  } catch (const trex::Refusal &r) {
    std::printf("REFUSED %d %s\n", r.code, r.what());
  }
  return 0;
}
