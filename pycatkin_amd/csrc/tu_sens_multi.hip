// Translation unit of the multi-objective analytic-DRC kernels
// (csrc/mk_sens_multi.h; the parallel product build of __graft_entry__.build).
#define PCK_KERNEL_TU 1
#include "mk_sens_multi.h"
namespace pck {
#define PCK_X(GG) PCK_DO_MULTI(, GG)
PCK_INST_MULTI(PCK_X)
#undef PCK_X
}  // namespace pck
