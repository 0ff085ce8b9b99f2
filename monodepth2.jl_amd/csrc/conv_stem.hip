// Implicit-GEMM conv: the ResNet stem forward on the space-to-depth grid (conv_stem.inc).
#include "conv_kernel.h"
#include "conv_lds.h"
namespace md2 {
#include "conv_stem.inc"
}  // namespace md2
