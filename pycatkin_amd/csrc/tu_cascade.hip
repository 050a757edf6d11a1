// Translation unit of the reactor-cascade kernels (csrc/mk_cascade.h,
// csrc/mk_inst.h; the parallel product build of __graft_entry__.build).
#define PCK_KERNEL_TU 1
#include "mk_inst.h"
namespace pck {
#define PCK_X(N) PCK_DO_CASCADE_RT(, N)
PCK_INST_LANE_RT(PCK_X)
#undef PCK_X
#define PCK_X(id, T) PCK_DO_CASCADE_CT(, id, T)
PCK_INST_CASCADE_CT(PCK_X)
#undef PCK_X
}  // namespace pck
