// Host harness for the HIP-free part of the mirror maps (csrc/host_tables.cpp: build_model_mirror, build_mirror_row_table, the action
// and command tables, build_mirror_words, check_mirror_rows, check_mirror_augment). Built by tests/test_symmetry_tables_host.py from
// host_tables.cpp + model.cpp with g++ -fsanitize=address,undefined; no HIP, no stubs.
//
//   symmetry_harness <mode> <numbers file> [file.urdf]
//
// The numbers file holds white-space separated numbers. By mode:
//   model    lateral tol_pos action_cols tail C, C x (kind link x y z scale), X, X x extern_src, X x extern_sign    (needs the urdf)
//   words    W, W x src, W x sign
//   rows     table_width in_offset in_stride out_offset out_stride n width      (offsets in floats into one imagined buffer; -1: null)
//   augment  obs_width act_width critic_width has_critic_table buffers obs_v num_samples D A Dv
// Output: one line per part, "name value value ...", or the single line "REFUSED <code> <message>" (exit code 0: a refusal is an
// answer). Exit code 2: bad usage, or the model does not load.
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

}  // namespace

int main(int argc, char **argv) {
  if (argc < 3) { std::fprintf(stderr, "usage: symmetry_harness <mode> <numbers file> [urdf]\n"); return 2; }
  const std::string mode = argv[1];
  std::vector<double> in;
  {
    std::ifstream f(argv[2]);
    std::string tok;
    while (f >> tok) in.push_back(std::strtod(tok.c_str(), nullptr));
  }
  size_t at = 0;
  auto next = [&]() -> double {
    if (at >= in.size()) { std::fprintf(stderr, "numbers file too short\n"); std::exit(2); }
    return in[at++];
  };
  try {
    if (mode == "model") {
      if (argc < 4) { std::fprintf(stderr, "model mode needs the urdf\n"); return 2; }
      trex::HostModel h;
      try {
        int code = 0;
        h = trex::load_model(argv[3], nullptr, &code);
      } catch (const std::exception &e) {
        std::fprintf(stderr, "model: %s\n", e.what());
        return 2;
      }
      const int lateral = (int)next();
      const double tol = next();
      const int action_cols = (int)next(), tail = (int)next(), C = (int)next();
      std::vector<TrexObsChannel> ch((size_t)C);
      for (auto &c : ch) {
        c.kind = (int32_t)next(); c.link = (int32_t)next();
        for (float &v : c.local_xyz) v = (float)next();
        c.scale = (float)next();
      }
      const int X = (int)next();
      std::vector<int32_t> es((size_t)X);
      std::vector<int8_t> eg((size_t)X);
      for (auto &v : es) v = (int32_t)next();
      for (auto &v : eg) v = (int8_t)next();
      const trex::ModelMirror m = trex::build_model_mirror(h, lateral, tol);
      std::printf("lateral %d\n", m.lateral);
      ints("pair", m.pair); ints("sign", m.sign); ints("body_pair", m.body_pair);
      std::printf("residual");
      for (double r : m.residual) std::printf(" %.17g", r);
      std::printf("\n");
      const int nj = h.nb - 1;
      for (int stiff = 0; stiff < 2; stiff++) {
        std::vector<int32_t> s((size_t)nj * (1 + stiff));
        std::vector<int8_t> g(s.size());
        trex::build_mirror_action_table(m.pair.data(), m.sign.data(), nj, stiff != 0, s.data(), g.data());
        ints(stiff ? "action2_src" : "action_src", s); ints(stiff ? "action2_sign" : "action_sign", g);
      }
      std::vector<int32_t> cs(3);
      std::vector<int8_t> cg(3);
      trex::build_mirror_command_table(m.lateral, cs.data(), cg.data());
      ints("command_src", cs); ints("command_sign", cg);
      const trex::RowMirror r = trex::build_mirror_row_table(h, m, tol, ch.data(), C, action_cols, tail, X ? es.data() : nullptr, X ? eg.data() : nullptr);
      ints("row_src", r.src); ints("row_sign", r.sign);
    } else if (mode == "words") {
      const int W = (int)next();
      const size_t count = W > 0 && W < 100000 ? (size_t)W : 0;
      std::vector<int32_t> src(count + 1);          // (one spare element: a width of 0 still hands over arrays that exist)
      std::vector<int8_t> sign(count + 1);
      for (size_t c = 0; c < count; c++) src[c] = (int32_t)next();
      for (size_t c = 0; c < count; c++) sign[c] = (int8_t)next();
      const trex::MirrorWords t = trex::build_mirror_words(src.data(), sign.data(), W);
      ints("word", t.word);
      std::printf("involution %d\n", t.involution ? 1 : 0);
    } else if (mode == "rows") {
      static float buffer[1 << 16];
      const int tw = (int)next();
      const long in_off = (long)next();
      const int in_stride = (int)next();
      const long out_off = (long)next();
      const int out_stride = (int)next(), n = (int)next(), width = (int)next();
      trex::check_mirror_rows(tw, in_off < 0 ? nullptr : buffer + in_off, in_stride, out_off < 0 ? nullptr : buffer + out_off, out_stride, n, width);
      std::printf("ok 1\n");
    } else if (mode == "augment") {
      const int ow = (int)next(), aw = (int)next(), cw = (int)next();
      const bool has = next() != 0, buffers = next() != 0, obs_v = next() != 0;
      const int64_t N = (int64_t)next();
      const int D = (int)next(), A = (int)next(), Dv = (int)next();
      trex::check_mirror_augment(ow, aw, cw, has, buffers, obs_v, N, D, A, Dv);
      std::printf("ok 1\n");
    } else {
      std::fprintf(stderr, "unknown mode %s\n", mode.c_str());
      return 2;
    }
  } catch (const trex::Refusal &r) {
    std::printf("REFUSED %d %s\n", r.code, r.what());
  }
  return 0;
}
