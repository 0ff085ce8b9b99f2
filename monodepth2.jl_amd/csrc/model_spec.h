// Architecture specification: every layer's shape and its offsets into the flat parameter vector
// (model_spec.cpp); the executor (model_impl.h) is built from it.
#pragma once
#include "model.h"

namespace md2 {

struct PConv {
  int cin = 0, cout = 0, k = 1, stride = 1, pad = 0, reflect = 0;
  bool bias = false;
  long w = -1, b = -1;
};
struct PBN {
  int c = 0;
  long g = -1, b = -1;
};
struct BlockSpec {
  std::vector<PConv> convs;
  std::vector<PBN> bns;
  bool down = false;
  PConv dconv;
  PBN dbn;
  int cin = 0, cout = 0, stride = 1;
};
struct BranchSpec {
  int bid = 0;
  PConv c1, c2;
  int cin = 0, cout = 0, cskip = 0;
  int head = -1;          // index into heads when a DecoderBlock head follows this branch
};
struct ArchSpec {
  std::vector<ParamEntry> table;
  long total = 0;
  PConv stem;
  PBN stem_bn;
  std::vector<std::vector<BlockSpec>> stages;
  int enc_ch[5];
  std::vector<BranchSpec> branches;
  std::vector<PConv> heads;
  std::vector<int> head_level;
  PConv squeezer, p1, p2, p3;
  long stage_begin[5];    // flat offsets: [0] stem, [1..4] layer1..4
  long depth_begin = 0;
};

ArchSpec build_spec(const ArchCfg& a);

inline int out_dim(int in, int k, int s, int p) { return (in + 2 * p - k) / s + 1; }
// a BatchNorm's gamma entry of the parameter table (one per BatchNorm, in make_bn order)
inline bool is_gamma(const ParamEntry& e) {
  return e.name.size() > 6 && e.name.compare(e.name.size() - 6, 6, ".gamma") == 0;
}

}  // namespace md2
