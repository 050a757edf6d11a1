// Translation unit of the one-lane multi-objective adjoint kernel
// (csrc/mk_sens_multi_lane.h; the parallel product build of __graft_entry__.build).
#define PCK_KERNEL_TU 1
#include "mk_sens_multi_lane.h"
