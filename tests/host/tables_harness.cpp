// Host harness for the table builders of the C-ABI (csrc/host_tables.cpp): the arithmetic that decides what every kernel reads.
// Built by tests/test_host_tables.py from host_tables.cpp + model.cpp with g++ -fsanitize=address,undefined; no HIP, no stubs.
//
//   tables_harness <file.urdf> <builder> [<numbers file>]
//
// The numbers file holds the builder's arguments as white-space separated numbers ("nan" and "inf" included):
//   model    (none)                                                    fill_device_model
//   probes   K, then K x (link x y z)                                   build_probe_table
//   prox     C, then C x (body p0 xyz p1 xyz radius), P, then P x (A B)  build_prox_table
//   ik       K, K links, K modes, joint_mask, with_params (0 / 1), iterations damping gain max_step tol_pos tol_ori   build_ik_task
//   camera   distance yaw pitch fov near far target xyz width height    camera_basis
//   rows     n stride width                                             row_block_bytes
//   overlap  a na b nb (two byte ranges, the addresses as numbers)       ranges_overlap
// Output: one line per table, "name value value ..." (floats with 9 digits: every f32 exactly), or the single line
// "REFUSED <code> <message>" (exit code 0: a refusal is an answer). Exit code 2: bad usage, or the model does not load.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../../trex-gym_amd/csrc/host_tables.hpp"

namespace {

template <class T> void ints(const char *name, const T *v, size_t n) {
  std::printf("%s", name);
  for (size_t i = 0; i < n; i++) std::printf(" %lld", (long long)v[i]);
  std::printf("\n");
}
void floats(const char *name, const float *v, size_t n) {
  std::printf("%s", name);
  for (size_t i = 0; i < n; i++) std::printf(" %.9g", (double)v[i]);
  std::printf("\n");
}

struct Numbers {
  std::vector<double> v;
  size_t at = 0;
  double next() {
    if (at >= v.size()) { std::fprintf(stderr, "numbers file too short\n"); std::exit(2); }
    return v[at++];
  }
  int next_int() { return (int)next(); }
};

}  // namespace

int main(int argc, char **argv) {
  if (argc < 3) { std::fprintf(stderr, "usage: tables_harness <urdf> <builder> [<numbers file>]\n"); return 2; }
  const std::string what = argv[2];
  Numbers in;
  if (argc > 3) {
    std::ifstream f(argv[3]);
    std::string tok;
    while (f >> tok) in.v.push_back(std::strtod(tok.c_str(), nullptr));
  }
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
  try {
    if (what == "model") {
      TrexDeviceModel d;
      trex::fill_device_model(h, d);
      const int sc[] = {d.nb, d.maxdepth, d.head_body, d.nv, d.nchunk};
      ints("scalars", sc, 5);
      ints("parent", d.parent, TREX_TL); ints("depth", d.depth, TREX_TL); ints("obs_slot", d.obs_slot, TREX_TL);
      ints("anc", &d.anc[0][0], TREX_MAXD * TREX_TL); ints("child", &d.child[0][0], TREX_MAXCH * TREX_TL);
      ints("desc_mask", d.desc_mask, TREX_TL); ints("hull_start", d.hull_start, TREX_TL + 1); ints("cm_pack", d.cm_pack, TREX_TL);
      floats("sphere", &d.sphere[0][0], 4 * TREX_TL); floats("box_half", &d.box_half[0][0], 3 * TREX_TL);
      ints("chunk_body", d.chunk_body, TREX_TL); ints("chunk_v0", d.chunk_v0, TREX_TL); ints("chunk_v1", d.chunk_v1, TREX_TL);
      floats("chunk_c", &d.chunk_c[0][0], 3 * TREX_TL); floats("chunk_h", &d.chunk_h[0][0], 3 * TREX_TL);
    } else if (what == "probes") {
      const int K = in.next_int();
      std::vector<int32_t> link((size_t)K);
      std::vector<double> xyz((size_t)K * 3);
      for (int k = 0; k < K; k++) {
        link[k] = in.next_int();
        for (int c = 0; c < 3; c++) xyz[3 * (size_t)k + c] = in.next();
      }
      const trex::ProbeTable t = trex::build_probe_table(links, link.data(), xyz.data(), K);
      ints("body", t.body.data(), t.body.size());
      floats("tf", t.tf.data(), t.tf.size());
    } else if (what == "prox") {
      const int C = in.next_int();
      std::vector<int32_t> body((size_t)C);
      std::vector<double> cap((size_t)C * 7);
      for (int c = 0; c < C; c++) {
        body[c] = in.next_int();
        for (int k = 0; k < 7; k++) cap[7 * (size_t)c + k] = in.next();
      }
      const int P = in.next_int();
      std::vector<int32_t> pair((size_t)P * 2);
      for (auto &x : pair) x = in.next_int();
      const trex::ProxTable t = trex::build_prox_table(h.nb, body.data(), cap.data(), C, pair.data(), P);
      const long long sc[] = {t.caps, t.pairs, t.tests, (long long)t.o_body, (long long)t.o_test, (long long)t.o_first, (long long)t.blob.size()};
      ints("scalars", sc, 7);
      const char *b = t.blob.data();   // (the parts start at multiples of 16 bytes: aligned for their types)
      floats("cap", (const float *)b, (size_t)t.caps * 8);
      ints("cap_body", (const int32_t *)(b + t.o_body), (size_t)t.caps);
      ints("test", (const uint32_t *)(b + t.o_test), (size_t)t.tests);
      ints("pair_first", (const int32_t *)(b + t.o_first), (size_t)t.pairs);
    } else if (what == "ik") {
      const int K = in.next_int();
      if (K < 0 || K > TREX_IK_MAXPROBES) { std::fprintf(stderr, "ik: at most %d probes\n", TREX_IK_MAXPROBES); return 2; }
      std::vector<int32_t> probe_body, mode;
      for (int k = 0; k < K; k++) probe_body.push_back(links.body.at((size_t)in.next_int()));
      for (int k = 0; k < K; k++) mode.push_back(in.next_int());
      const uint32_t joint_mask = (uint32_t)in.next();
      const bool with_params = in.next_int() != 0;
      TrexIkParams p = TREX_IK_DEFAULTS;
      if (with_params) {
        p.iterations = in.next_int();
        p.damping = (float)in.next(); p.gain = (float)in.next(); p.max_step = (float)in.next();
        p.tol_pos = (float)in.next(); p.tol_ori = (float)in.next();
      }
      const trex::IkTask t = trex::build_ik_task(probe_body, h.parent, h.obs_order, mode.data(), joint_mask, with_params ? &p : nullptr);
      ints("body", t.body, (size_t)K); ints("mode", t.mode, (size_t)K); ints("row0", t.row0, (size_t)K); ints("chain", t.chain, (size_t)K);
      const long long sc[] = {t.rows, (long long)t.move_mask, t.iterations};
      ints("scalars", sc, 3);
      const float par[] = {t.damping2, t.gain, t.max_step, t.tol_pos, t.tol_ori};
      floats("params", par, 5);
    } else if (what == "camera") {
      TrexCamera cam{};
      cam.distance = (float)in.next(); cam.yaw_deg = (float)in.next(); cam.pitch_deg = (float)in.next(); cam.fov_deg = (float)in.next();
      cam.near_z = (float)in.next(); cam.far_z = (float)in.next();
      for (float &x : cam.target) x = (float)in.next();
      const int width = in.next_int(), height = in.next_int();
      const trex::CameraBasis b = trex::camera_basis(cam, width, height);
      floats("offset", b.offset, 3); floats("fwd", b.fwd, 3); floats("right", b.right, 3); floats("up", b.up, 3);
      const float tn[] = {b.tan_x, b.tan_y};
      floats("tan", tn, 2);
    } else if (what == "rows") {
      const size_t n = (size_t)in.next();
      const int stride = in.next_int(), width = in.next_int();
      const long long bytes[] = {(long long)trex::row_block_bytes(n, stride, width)};
      ints("bytes", bytes, 1);
    } else if (what == "overlap") {   // (addresses as numbers: the predicate compares, it never reads)
      const uintptr_t a = (uintptr_t)in.next();
      const size_t na = (size_t)in.next();
      const uintptr_t b = (uintptr_t)in.next();
      const size_t nb = (size_t)in.next();
      const int share[] = {trex::ranges_overlap((const void *)a, na, (const void *)b, nb) ? 1 : 0};
      ints("overlap", share, 1);
    } else {
      std::fprintf(stderr, "unknown builder '%s'\n", what.c_str());
      return 2;
    }
  } catch (const trex::Refusal &r) {
    std::printf("REFUSED %d %s\n", r.code, r.what());
  }
  return 0;
}
