// Implicit-GEMM conv: the LDS-halo stride-1 3x3 fwd / dgrad kernel (conv_halo.inc).
#include "conv_plan.h"
#include "conv_lds.h"
namespace md2 {
#include "conv_halo.inc"
}  // namespace md2
