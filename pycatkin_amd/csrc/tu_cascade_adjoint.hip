// Translation unit of the bed DRC kernel
// (csrc/mk_cascade_adjoint.h; the parallel product build of __graft_entry__.build).
#define PCK_KERNEL_TU 1
#include "mk_cascade_adjoint.h"
