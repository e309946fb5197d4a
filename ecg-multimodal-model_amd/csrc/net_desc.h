// The two encoder networks and the CRNN front end described once: per-block channel counts, strides, parameter- /
// buffer-table indices and geometry.  Every launch plan (plan_resnet18.hip, plan_resnet1d.hip, plan_crnn.hip,
// plan_infer.hip) walks these records.
// A record is built in two steps: *_static() fills what the weights depend on (dtype, table indices, channel counts,
// strides) and *_shape() adds what depends on N and the input size.  Both take the message prefix of the calling plan;
// what else a plan validates (out_dim, bn_eps, ...) stays with that plan's entry points.
#pragma once
#include "ops.h"

// what a BatchNorm call needs to know of the descriptor
struct BnCfg {
  int dtype, training;
  float momentum, eps;
};

inline int desc_dtype_ok(int dtype, const char* who) {
  if (dtype != ECGMM_BF16 && dtype != ECGMM_F32) ECG_FAIL(ECGMM_ERR_DTYPE, "%s: bad dtype %d", who, dtype);
  return 0;
}

// ================================================================================================
// ResNet18.  Parameter table order (62 entries, == named_parameters() order of the Python module):
//   conv1.weight, bn1.weight, bn1.bias,
//   layer{1..4}.{0,1}.{conv1.weight, bn1.weight, bn1.bias, conv2.weight, bn2.weight, bn2.bias,
//                      [downsample.0.weight, downsample.1.weight, downsample.1.bias]},
//   fc.weight, fc.bias
// Buffer table order (60 entries): per BatchNorm in the same walk: running_mean, running_var,
//   num_batches_tracked (int64).
// ================================================================================================
struct Blk18 {
  int cin, cout, stride, hin, win, hout, wout;
  bool down;
  int p_conv1, p_bn1, p_conv2, p_bn2, p_dconv, p_dbn;  // param indices (weight; bn bias = +1)
  int b_bn1, b_bn2, b_dbn;                              // buffer indices (rm; rv = +1; nbt = +2)
  ConvGeom conv1_geom(int N) const { return make_geom(N, hin, win, cin, cout, 3, 3, stride, 1, 1); }
  ConvGeom conv2_geom(int N) const { return make_geom(N, hout, wout, cout, cout, 3, 3, 1, 1, 1); }
  ConvGeom down_geom(int N) const { return make_geom(N, hin, win, cin, cout, 1, 1, stride, 0, 0); }
};

struct Net18 {
  ecgmm_resnet18_desc d;
  BnCfg bn;
  int H1, W1, H2, W2;
  Blk18 blk[8];
  int p_fc;
  size_t max_act;  // largest block-level activation (elements)
};

inline int net18_static(const ecgmm_resnet18_desc* d, Net18& r, const char* who) {
  if (!d) ECG_FAIL(ECGMM_ERR_SHAPE, "%s: null desc", who);
  ECG_TRY(desc_dtype_ok(d->dtype, who));
  r.d = *d;
  r.bn = {d->dtype, d->training, d->bn_momentum, d->bn_eps};
  int pi = 3, bi = 3, cin = 64;
  for (int L = 0; L < 4; ++L) {
    const int cout = 64 << L;
    for (int b = 0; b < 2; ++b) {
      Blk18& k = r.blk[L * 2 + b];
      k.cin = cin; k.cout = cout; k.stride = (b == 0 && L > 0) ? 2 : 1;
      k.down = (k.stride != 1 || cin != cout);
      k.p_conv1 = pi; k.p_bn1 = pi + 1; k.p_conv2 = pi + 3; k.p_bn2 = pi + 4; pi += 6;
      k.b_bn1 = bi; k.b_bn2 = bi + 3; bi += 6;
      if (k.down) {
        k.p_dconv = pi; k.p_dbn = pi + 1; pi += 3;
        k.b_dbn = bi; bi += 3;
      } else {
        k.p_dconv = k.p_dbn = k.b_dbn = -1;
      }
      cin = cout;
    }
  }
  r.p_fc = pi;
  if (pi + 2 != ECGMM_RESNET18_NPARAMS || bi != ECGMM_RESNET18_NBUFFERS)
    ECG_FAIL(ECGMM_ERR_SHAPE, "%s: internal table mismatch %d %d", who, pi + 2, bi);
  return 0;
}

inline int net18_shape(Net18& r, const char* who) {
  const ecgmm_resnet18_desc& d = r.d;
  if (d.N < 1 || d.H < 32 || d.W < 32) ECG_FAIL(ECGMM_ERR_SHAPE, "%s: bad input %dx%dx%d", who, d.N, d.H, d.W);
  r.H1 = (d.H + 6 - 7) / 2 + 1;
  r.W1 = (d.W + 6 - 7) / 2 + 1;
  r.H2 = (r.H1 + 2 - 3) / 2 + 1;
  r.W2 = (r.W1 + 2 - 3) / 2 + 1;
  int h = r.H2, w = r.W2;
  r.max_act = (size_t)d.N * h * w * 64;  // (the pool output = block 0's input; every other block input is a block output)
  for (int i = 0; i < 8; ++i) {
    Blk18& k = r.blk[i];
    k.hin = h; k.win = w;
    k.hout = (h + 2 - 3) / k.stride + 1;
    k.wout = (w + 2 - 3) / k.stride + 1;
    const size_t a = (size_t)d.N * k.hout * k.wout * k.cout;
    if (a > r.max_act) r.max_act = a;
    h = k.hout; w = k.wout;
  }
  return 0;
}

// ================================================================================================
// ResNet1D_SE.  Parameter table (52): initial.0.{weight,bias}, initial.1.{weight,bias}, then per layer
//   conv1.{w,b}, bn1.{w,b}, conv2.{w,b}, bn2.{w,b}, se.fc.0.{w,b}, se.fc.2.{w,b},
//   [downsample.0.{w,b}, downsample.1.{w,b}] (layers 2,3), then classifier.1.{w,b}, classifier.4.{w,b}.
// Buffer table (27): running_mean, running_var, num_batches_tracked per BatchNorm in the same walk.
// ================================================================================================
// offsets from a block's first parameter (Blk1::p0); a BatchNorm's bias is its weight + 1
enum {
  T1_CONV1_W, T1_CONV1_B, T1_BN1, T1_CONV2_W = T1_BN1 + 2, T1_CONV2_B, T1_BN2,
  T1_SE_W1 = T1_BN2 + 2, T1_SE_B1, T1_SE_W2, T1_SE_B2, T1_NPARAMS,
  T1_DOWN_W = T1_NPARAMS, T1_DOWN_B, T1_DBN, T1_NPARAMS_DOWN = T1_DBN + 2
};
// offsets from a block's first buffer (Blk1::b0): running_mean; running_var = +1; num_batches_tracked = +2
enum { T1B_BN1 = 0, T1B_BN2 = T1B_BN1 + 3, T1B_NBUFFERS = T1B_BN2 + 3, T1B_DBN = T1B_NBUFFERS, T1B_NBUFFERS_DOWN = T1B_DBN + 3 };
// offsets from the classifier's first parameter (Net1D::p_cls)
enum { T1_CLS_W1, T1_CLS_B1, T1_CLS_W2, T1_CLS_B2, T1_NCLS };
static_assert(T1_NPARAMS == 12 && T1_NPARAMS_DOWN == 16 && T1B_NBUFFERS == 6 && T1B_NBUFFERS_DOWN == 9 && T1_NCLS == 4,
              "ResNet1D_SE table walk");

struct Blk1 {
  int cin, cout, stride, lin, lout, cr;
  bool down;
  int p0;  // first param index
  int b0;  // first buffer index
  ConvGeom conv1_geom(int N) const { return make_geom(N, 1, lin, cin, cout, 1, 3, stride, 0, 1); }
  ConvGeom conv2_geom(int N) const { return make_geom(N, 1, lout, cout, cout, 1, 3, 1, 0, 1); }
  ConvGeom down_geom(int N) const { return make_geom(N, 1, lin, cin, cout, 1, 1, stride, 0, 0); }
};

struct Net1D {
  ecgmm_resnet1d_desc d;
  BnCfg bn;
  int L1, L2;
  Blk1 blk[3];
  int p_cls;
  size_t max_act;
};

inline int net1d_static(const ecgmm_resnet1d_desc* d, Net1D& r, const char* who) {
  if (!d) ECG_FAIL(ECGMM_ERR_SHAPE, "%s: null desc", who);
  ECG_TRY(desc_dtype_ok(d->dtype, who));
  r.d = *d;
  r.bn = {d->dtype, d->training, d->bn_momentum, d->bn_eps};
  int pi = 4, bi = 3, cin = 64;
  for (int i = 0; i < 3; ++i) {
    Blk1& k = r.blk[i];
    k.cin = cin; k.cout = 64 << i; k.stride = i == 0 ? 1 : 2;
    k.cr = k.cout / 16;
    k.down = (k.stride != 1 || k.cin != k.cout);
    k.p0 = pi; k.b0 = bi;
    pi += k.down ? T1_NPARAMS_DOWN : T1_NPARAMS;
    bi += k.down ? T1B_NBUFFERS_DOWN : T1B_NBUFFERS;
    cin = k.cout;
  }
  r.p_cls = pi;
  if (pi + T1_NCLS != ECGMM_RESNET1D_NPARAMS || bi != ECGMM_RESNET1D_NBUFFERS)
    ECG_FAIL(ECGMM_ERR_SHAPE, "%s: internal table mismatch %d %d", who, pi + T1_NCLS, bi);
  return 0;
}

inline int net1d_shape(Net1D& r, const char* who) {
  const ecgmm_resnet1d_desc& d = r.d;
  if (d.N < 1 || d.L < 64 || d.cin < 1 || d.cin > 24)
    ECG_FAIL(ECGMM_ERR_SHAPE, "%s: bad input N=%d cin=%d L=%d", who, d.N, d.cin, d.L);
  r.L1 = (d.L + 6 - 7) / 2 + 1;
  r.L2 = (r.L1 + 2 - 3) / 2 + 1;
  int l = r.L2;
  r.max_act = (size_t)d.N * r.L2 * 64;
  for (int i = 0; i < 3; ++i) {
    Blk1& k = r.blk[i];
    k.lin = l; k.lout = (l + 2 - 3) / k.stride + 1;
    const size_t a = (size_t)d.N * k.lout * k.cout;
    if (a > r.max_act) r.max_act = a;
    l = k.lout;
  }
  return 0;
}

// ================================================================================================
// CRNN front end (train_physionet2.py:55-65, 87-93): three blocks Conv2d(k = 5, pad = 2, bias) -> BatchNorm2d -> ReLU ->
// MaxPool2d(2).  Parameter table (12): per block conv weight, conv bias, bn weight, bn bias; buffer table (9): per block
// running_mean, running_var, num_batches_tracked.  Walked by plan_crnn.hip (training plan) and plan_infer.hip.
// ================================================================================================
struct BlkC {
  int cin, cout, h, w, ph, pw;   // conv input = output extent (h, w), pooled extent (ph, pw)
  int p0, b0;
  long pixels(int B) const { return (long)B * h * w; }
  long pooled(int B) const { return (long)B * ph * pw; }
  ConvGeom geom(int B) const { return make_geom(B, h, w, cin, cout, 5, 5, 1, 2, 2); }
};
struct NetC {
  ecgmm_crnn_front_desc d;
  BnCfg bn;
  BlkC blk[3];
};

inline int netc_static(const ecgmm_crnn_front_desc* d, NetC& r, const char* who) {
  if (!d) ECG_FAIL(ECGMM_ERR_SHAPE, "%s: null desc", who);
  ECG_TRY(desc_dtype_ok(d->dtype, who));
  r.d = *d;
  r.bn = {d->dtype, d->training, d->bn_momentum, d->bn_eps};
  int cin = 1;
  for (int i = 0; i < 3; ++i) {
    BlkC& k = r.blk[i];
    k.cin = cin; k.cout = 32 << i; k.p0 = 4 * i; k.b0 = 3 * i;
    k.h = k.w = k.ph = k.pw = 0;
    cin = k.cout;
  }
  return 0;
}

inline int netc_shape(NetC& r, const char* who) {
  const ecgmm_crnn_front_desc& d = r.d;
  if (d.B < 1) ECG_FAIL(ECGMM_ERR_SHAPE, "%s: B = %d", who, d.B);
  if (d.F < 8) ECG_FAIL(ECGMM_ERR_SHAPE, "%s: F = %d (three 2x2 pools need F >= 8)", who, d.F);
  if (d.T < 8) ECG_FAIL(ECGMM_ERR_SHAPE, "%s: T = %d (three 2x2 pools need T >= 8)", who, d.T);
  if ((long)d.B * d.F * d.T > 0x7fffffffL / 32) ECG_FAIL(ECGMM_ERR_SHAPE, "%s: input too large", who);
  int h = d.F, w = d.T;
  for (int i = 0; i < 3; ++i) {
    BlkC& k = r.blk[i];
    k.h = h; k.w = w; k.ph = h / 2; k.pw = w / 2;
    h = k.ph; w = k.pw;
  }
  return 0;
}

inline int netc_build(const ecgmm_crnn_front_desc* d, NetC& r, const char* who) {
  ECG_TRY(netc_static(d, r, who));
  return netc_shape(r, who);
}
