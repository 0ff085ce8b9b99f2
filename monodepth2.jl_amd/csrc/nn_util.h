// Host helpers shared by the translation units behind nn.h (internal: include after nn.h).
#pragma once
#include "nn.h"

namespace md2 {

// Element index helpers: every activation here is < 2^31 elements (checked on the host), so
// indices are 32-bit and divisions by runtime extents use magic numbers (FastDiv).
static inline FastDiv fd(long d) { return make_fastdiv((uint32_t)d); }
static inline int check_u31(long n) {
  MD2_CHECK_ARG(n >= 0 && n < (1L << 31), "tensor larger than 2^31 elements");
  return MD2_OK;
}

// device-side form of a SkipAdd (range already checked against the tensor: < 2^31)
static inline SkipSrc skip_src(const SkipAdd& sk) {
  SkipSrc pd{};
  pd.skip = sk.skip;
  pd.skip_lo = (uint32_t)sk.lo;
  pd.skip_hi = (uint32_t)sk.hi;
  return pd;
}

}  // namespace md2
