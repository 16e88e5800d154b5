// The ACT instantiations of the step kernel (trex_step.hip: the actuator model) and their launchers, as a translation unit of
// their own: they double the product kernels, and the two files compile side by side.
#define TREX_ACT_TU 1
#include "trex_step.hip"
