// The product step launches with the actuator model (ACT, trex_step_body.h), with and without WARM, EXT and SENS: the ACT half of
// the variant table, compiled in a translation unit of its own next to trex_step.hip.
#include "trex_step_body.h"

extern "C" TrexStepKernel trex_step_act_variant(int form, unsigned features) { return trex_step_variant<true>(form, features); }
