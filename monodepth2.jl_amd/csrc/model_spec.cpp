// The architecture's layers and flat parameter table (model_spec.h), in the order of
// oracle/md2_oracle.py param_spec.
#include "model_spec.h"

namespace md2 {

ArchSpec build_spec(const ArchCfg& a) {
  ArchSpec S;
  auto add = [&](const std::string& name, std::initializer_list<int> shape) -> long {
    ParamEntry e;
    e.name = name;
    e.ndim = (int)shape.size();
    long n = 1;
    int i = 0;
    for (int s : shape) {
      e.shape[i++] = s;
      n *= s;
    }
    for (; i < 4; ++i) e.shape[i] = 1;
    e.offset = S.total;
    e.numel = n;
    S.total += n;
    S.table.push_back(e);
    return e.offset;
  };
  auto conv = [&](const std::string& name, int cin, int cout, int k, int stride, int pad,
                  int reflect, bool bias) {
    PConv c;
    c.cin = cin; c.cout = cout; c.k = k; c.stride = stride; c.pad = pad; c.reflect = reflect;
    c.bias = bias;
    c.w = add(name + ".weight", {cout, cin, k, k});
    if (bias) c.b = add(name + ".bias", {cout});
    return c;
  };
  auto bn = [&](const std::string& name, int c) {
    PBN b;
    b.c = c;
    b.g = add(name + ".gamma", {c});
    b.b = add(name + ".beta", {c});
    return b;
  };
  const bool bottleneck = a.arch >= 50;
  const int* layers;
  static const int L18[4] = {2, 2, 2, 2}, L34[4] = {3, 4, 6, 3};
  layers = (a.arch == 18) ? L18 : L34;
  const int exp = bottleneck ? 4 : 1;
  S.stage_begin[0] = 0;
  S.stem = conv("encoder.stem.conv", a.in_ch, 64, 7, 2, 3, 0, false);
  S.stem_bn = bn("encoder.stem.bn", 64);
  int cin = 64;
  const int widths[4] = {64, 128, 256, 512};
  S.stages.resize(4);
  for (int si = 0; si < 4; ++si) {
    S.stage_begin[si + 1] = S.total;
    for (int bi = 0; bi < layers[si]; ++bi) {
      const int stride = (bi == 0 && si > 0) ? 2 : 1;
      const std::string p = "encoder.layer" + std::to_string(si + 1) + "." + std::to_string(bi);
      const int width = widths[si], cout = width * exp;
      BlockSpec B;
      B.cin = cin;
      B.cout = cout;
      B.stride = stride;
      if (bottleneck) {
        B.convs.push_back(conv(p + ".conv1", cin, width, 1, 1, 0, 0, false));
        B.bns.push_back(bn(p + ".bn1", width));
        B.convs.push_back(conv(p + ".conv2", width, width, 3, stride, 1, 0, false));
        B.bns.push_back(bn(p + ".bn2", width));
        B.convs.push_back(conv(p + ".conv3", width, cout, 1, 1, 0, 0, false));
        B.bns.push_back(bn(p + ".bn3", cout));
      } else {
        B.convs.push_back(conv(p + ".conv1", cin, width, 3, stride, 1, 0, false));
        B.bns.push_back(bn(p + ".bn1", width));
        B.convs.push_back(conv(p + ".conv2", width, width, 3, 1, 1, 0, false));
        B.bns.push_back(bn(p + ".bn2", width));
      }
      if (stride != 1 || cin != cout) {
        B.down = true;
        B.dconv = conv(p + ".down", cin, cout, 1, stride, 0, 0, false);
        B.dbn = bn(p + ".down_bn", cout);
      }
      S.stages[si].push_back(B);
      cin = cout;
    }
  }
  const int enc18[5] = {64, 64, 128, 256, 512}, enc50[5] = {64, 256, 512, 1024, 2048};
  for (int i = 0; i < 5; ++i) S.enc_ch[i] = bottleneck ? enc50[i] : enc18[i];
  // DepthDecoder(; encoder_channels, scale_levels, embedding_levels=0) src/depth_decoder.jl:26-50
  S.depth_begin = S.total;
  const int dec[5] = {256, 128, 64, 32, 16};
  int encr[5];   // + embedding_levels in MPI mode (src/depth_decoder.jl:32)
  for (int i = 0; i < 5; ++i) encr[i] = S.enc_ch[4 - i] + a.emb;
  const int in_ch[5] = {encr[0], dec[0], dec[1], dec[2], dec[3]};
  const int skip[5] = {encr[1], encr[2], encr[3], encr[4], 0};
  int bstart = 1;
  for (int li = 0; li < a.nlevels; ++li) {
    const int slevel = a.levels[li];
    for (int bid = bstart; bid <= slevel; ++bid) {
      const int b = bid - 1;
      BranchSpec br;
      br.bid = bid;
      br.cin = in_ch[b];
      br.cout = dec[b];
      br.cskip = skip[b];
      br.c1 = conv("depth.branch" + std::to_string(bid) + ".c1", in_ch[b], dec[b], 3, 1, 1, 1, true);
      br.c2 = conv("depth.branch" + std::to_string(bid) + ".c2", dec[b] + skip[b], dec[b], 3, 1, 1, 1, true);
      S.branches.push_back(br);
    }
    S.heads.push_back(conv("depth.head" + std::to_string(slevel), dec[slevel - 1], 1, 3, 1, 1, 1, true));
    S.head_level.push_back(slevel);
    S.branches.back().head = (int)S.heads.size() - 1;
    bstart = slevel + 1;
  }
  // PoseDecoder(encoder_out_channels) src/pose_decoder.jl:13-21
  S.squeezer = conv("pose.squeezer", S.enc_ch[4], 256, 1, 1, 0, 0, true);
  S.p1 = conv("pose.conv1", 512, 256, 3, 1, 1, 0, true);
  S.p2 = conv("pose.conv2", 256, 256, 3, 1, 1, 0, true);
  S.p3 = conv("pose.conv3", 256, 6, 1, 1, 0, 0, true);
  return S;
}

std::vector<ParamEntry> build_param_table(const ArchCfg& a) { return build_spec(a).table; }

// BatchNorm running statistics as model state (testmode.h): their count and flat length
int arch_bn_stat_count(const ArchCfg& a, long* n_bn, long* n_elems) {
  long nb = 0, ne = 0;
  for (const ParamEntry& e : build_param_table(a))
    if (is_gamma(e)) {
      ++nb;
      ne += 2 * e.numel;
    }
  if (n_bn) *n_bn = nb;
  if (n_elems) *n_elems = ne;
  return MD2_OK;
}

// DepthDecoder(; scale_levels) (src/depth_decoder.jl:26-50): at most 5 levels in 1:5 (the
// reference's own error); levels that do not strictly increase are MD2_ENOTSUP (the reference
// then builds empty branches: a duplicate head for a repeated level, a channel mismatch at run
// time for a decreasing one)
int check_scale_levels(const ArchCfg& a) {
  MD2_CHECK_ARG(a.nlevels >= 1 && a.nlevels <= MAX_SCALES,
                "`scale_levels` should be at most of length 5 and have values in [1, 5] range.");
  for (int i = 0; i < a.nlevels; ++i)
    MD2_CHECK_ARG(a.levels[i] >= 1 && a.levels[i] <= 5,
                  "`scale_levels` should be at most of length 5 and have values in [1, 5] range.");
  for (int i = 1; i < a.nlevels; ++i)
    if (a.levels[i] <= a.levels[i - 1]) {
      set_error("scale_levels must be strictly increasing (repeated / decreasing levels: not supported)");
      return MD2_ENOTSUP;
    }
  return MD2_OK;
}

}  // namespace md2
