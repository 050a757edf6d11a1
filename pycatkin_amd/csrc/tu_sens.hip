// Translation unit of the analytic-DRC kernels (csrc/mk_sens.h; the parallel
// product build of __graft_entry__.build).
#define PCK_KERNEL_TU 1
#include "mk_sens.h"
namespace pck {
#define PCK_X(GG) PCK_DO_SENS(, GG)
PCK_INST_SENS(PCK_X)
#undef PCK_X
}  // namespace pck
