// Host harness for the HIP-free part of the trainer (csrc/host_tables.cpp check_policy_* and csrc/policy_limits.h make_layout): what
// the C-ABI of include/trex_policy.h, trex_policy_critic.h and trex_policy_distill.h refuses before any HIP call, and the layout of
// the parameter vector. Built by tests/test_policy_checks_host.py from host_tables.cpp + model.cpp with
// g++ -fsanitize=address,undefined; no HIP, no stubs.
//
//   policy_harness <words file>
//
// The words file holds white-space separated words: the call, then its numbers. A policy is the three numbers D A Dv (D < 0: a
// null policy; its env count is 33); a pointer is 0 (null) or 1.
//   layout D A Dv
//   create num_envs obs_dim act_dim hidden
//   set_critic D A Dv critic_dim
//   critic_stats D A Dv host                      (trex_policy_critic_get_stats)
//   observe D A Dv rows row_stride with_reward
//   critic_observe D A Dv rows_v stride_v
//   act | critic_act D A Dv theta rows rows_v noise actions value_out obs_v_out row_stride stride_v value_only
//   gae D A Dv buffers T
//   minibatch_stats D A Dv buffers num_minibatches mb num_samples
//   minibatch <who> D A Dv distill critic buffers mb first num_samples kind teacher_logstd teacher_value vf_coef
// Output: "layout <the 13 offsets> <count>" or "OK", or the single line "REFUSED <code> <message>" (exit code 0: a refusal is an
// answer). Exit code 2: bad usage.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "../../trex-gym_amd/csrc/host_tables.hpp"

int main(int argc, char **argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: policy_harness <words file>\n"); return 2; }
  std::vector<std::string> w;
  {
    std::ifstream f(argv[1]);
    std::string tok;
    while (f >> tok) w.push_back(tok);
  }
  if (w.empty()) { std::fprintf(stderr, "words file: empty\n"); return 2; }
  const std::string call = w[0];
  size_t at = 1;
  std::string who;
  if (call == "minibatch") who = w.at(at++);
  std::vector<double> in;
  for (; at < w.size(); at++) in.push_back(std::strtod(w[at].c_str(), nullptr));
  const auto need = [&](size_t n) { if (in.size() != n) { std::fprintf(stderr, "%s: %zu numbers\n", call.c_str(), n); std::exit(2); } };
  const auto I = [&](size_t k) { return (int)in[k]; };
  const auto B = [&](size_t k) { return in[k] != 0; };
  trex::PolicyShape shape;
  const trex::PolicyShape *p = nullptr;
  if (call != "create") {
    if (in.size() < 3) { std::fprintf(stderr, "%s: a policy is D A Dv\n", call.c_str()); return 2; }
    shape.n = 33; shape.D = I(0); shape.A = I(1); shape.Dv = I(2);
    shape.lay = trex_policy::make_layout(shape.D, shape.A, shape.Dv);
    if (shape.D >= 0) p = &shape;
  }
  try {
    if (call == "layout") {
      need(3);
      const trex_policy::PolicyLayout &l = shape.lay;
      std::printf("layout %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", l.pW1, l.pb1, l.pW2, l.pb2, l.pW3, l.pb3, l.vW1, l.vb1, l.vW2, l.vb2,
                  l.vW3, l.vb3, l.logstd, l.count);
      return 0;
    } else if (call == "create") {
      need(4);
      trex::check_policy_create(I(0), I(1), I(2), I(3));
    } else if (call == "set_critic") {
      need(4);
      trex::check_policy_set_critic(p, I(3));
    } else if (call == "critic_stats") {
      need(4);
      trex::check_policy_has_critic("trex_policy_critic_get_stats", p, B(3));
    } else if (call == "observe") {
      need(6);
      trex::check_policy_observe(p, B(3), I(4), B(5));
    } else if (call == "critic_observe") {
      need(5);
      trex::check_policy_critic_observe(p, B(3), I(4));
    } else if (call == "act" || call == "critic_act") {
      need(13);
      const trex::PolicyActCall c{B(3), B(4), B(5), B(6), B(7), B(8), B(9), I(10), I(11), B(12)};
      if (call == "act") trex::check_policy_act(p, c);
      else trex::check_policy_critic_act(p, c);
    } else if (call == "gae") {
      need(5);
      trex::check_policy_gae(p, B(3), I(4));
    } else if (call == "minibatch_stats") {
      need(7);
      trex::check_policy_minibatch_stats(p, B(3), I(4), I(5), (int64_t)in[6]);
    } else if (call == "minibatch") {
      need(13);
      const trex::PolicyMinibatchCall c{who.c_str(), B(3), B(4), B(5), I(6), I(7), (int64_t)in[8], I(9), B(10), B(11), (float)in[12]};
      trex::check_policy_minibatch(p, c);
    } else {
      std::fprintf(stderr, "unknown call %s\n", call.c_str());
      return 2;
    }
    std::printf("OK\n");
  } catch (const trex::Refusal &r) {
    std::printf("REFUSED %d %s\n", r.code, r.what());
  }
  return 0;
}
