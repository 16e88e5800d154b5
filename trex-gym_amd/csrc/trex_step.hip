// The step kernels without the actuator model, the launch shape and the one step launcher (trex_step_body.h: the step body, the
// feature variants and the variant table; trex_step_act.hip: the ACT half).
#include "trex_step_body.h"

// the kernels without a feature, under the names the profiles, bench.py and the scripts know them by
template <bool RESET, bool DEBUG>
__global__ __launch_bounds__(64, 4) void trex_step_kernel(TrexStepArgs args) { trex_step_body<RESET, DEBUG, false>(args, (int)blockIdx.x); }
// two envs per workgroup with split roles between the barriers of a substep (PAIR above): even batches of at most 4096 envs
__global__ __launch_bounds__(128, 4) void trex_step_pair_kernel(TrexStepArgs args) { trex_step_body<false, false, false, true>(args, (int)blockIdx.x); }
// S env-steps per launch (trex_batch_step_many)
__global__ __launch_bounds__(64, 4) void trex_step_many_kernel(TrexStepArgs args) { trex_step_body<false, false, true>(args, (int)blockIdx.x); }

// ---------------------------------------------------------------- host launchers (called by capi.cpp)
extern "C" {

// THE decision of a launch's form, for the launch and for trex_batch_launch_info alike: the pair form (two envs per workgroup) for
// the step launch of an even batch that is resident at once - where the build has it (TREX_PAIR_LAUNCH, TREX_PAIR_MAX) and it exists
// for these features: a warm batch with actuators steps through the single-env form (trex_step_variant_exists)
TrexStepShape trex_step_launch_shape(TrexStepKind kind, int n, unsigned features) {
  const bool pair = kind == TREX_KIND_STEP && TREX_PAIR_LAUNCH && (n & 1) == 0 && n <= TREX_PAIR_MAX &&
                    trex_step_variant_exists(FORM_PAIR, features);
  const int epw = pair ? 2 : 1;
  const size_t lds = (pair ? 2 * sizeof(WaveLds) + sizeof(CgLds) : sizeof(WaveLds)) +
                     ((features & TREX_FEAT_WARM) ? epw * MAXC * sizeof(float4) : 0);   // (WARM: the record of every env, Wrec)
  return {epw, (n + epw - 1) / epw, 64 * epw, (int)lds};   // one wavefront per env
}

// Every step launch: the kernel is the table's for the form - the kind's, or the pair form - and the features the arguments carry.
hipError_t trex_launch_step(const TrexStepArgs *args, TrexStepKind kind, hipStream_t stream) {
  TrexStepArgs a = *args;
  const unsigned features = trex_step_features(a);
  // The stamped diagnostic build runs the PRODUCT instantiation, stamped and balanced, for a diagnostics step too (the dump of
  // <false, true> would change its code, and it reports the env of every wave); else a diagnostics step keeps env k in workgroup k.
  if (TREX_STAMPS && kind == TREX_KIND_STEP_DEBUG) kind = TREX_KIND_STEP;
  if (kind == TREX_KIND_STEP_DEBUG) a.bal = nullptr;
  const TrexStepShape shape = trex_step_launch_shape(kind, a.n_envs, features);
  const int form = shape.envs_per_workgroup == 2 ? (int)FORM_PAIR : (int)kind;
  const TrexStepKernel kernel = (features & TREX_FEAT_ACT) ? trex_step_act_variant(form, features) : trex_step_variant<false>(form, features);
  if (!kernel) return hipErrorInvalidValue;   // (capi.cpp refuses what does not exist - a diagnostics step of a batch with a feature -
                                              // before it gets here)
  hipLaunchKernelGGL(kernel, dim3(shape.grid), dim3(shape.block), 0, stream, a);
  return hipGetLastError();
}

}  // extern "C"
