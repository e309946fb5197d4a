// Host-side helpers the launch plans share (plan_resnet18.hip, plan_resnet1d.hip, plan_infer.hip).
#pragma once
#include "net_desc.h"

inline const float* P(const void* const* params, int i) { return (const float*)params[i]; }
inline float* G(void* const* grads, int i) { return grads ? (float*)grads[i] : nullptr; }

// a caller-owned workspace / blob must be there and large enough
#define ECG_NEED(ptr, have, need, what)                                                                       \
  do {                                                                                                        \
    if (!(ptr) || (have) < (need)) ECG_FAIL(ECGMM_ERR_WORKSPACE, "%s %zu < %zu", what, (size_t)(have), (size_t)(need)); \
  } while (0)

// BN statistics of a fresh conv output -> coefficients (train: batch stats + running update; eval: running stats)
inline int bn_coef(const BnCfg& c, const float* stats, int rows, int C, long count, const void* const* params, int p_bn,
                   void* const* buffers, int b_bn, float* coef, hipStream_t s) {
  if (c.training)
    return ecg_bn_finalize(stats, rows, C, (double)count, P(params, p_bn), P(params, p_bn + 1), (float*)buffers[b_bn],
                           (float*)buffers[b_bn + 1], (long long*)buffers[b_bn + 2], c.momentum, c.eps, coef, s);
  return ecg_bn_eval_coef(C, P(params, p_bn), P(params, p_bn + 1), (const float*)buffers[b_bn],
                          (const float*)buffers[b_bn + 1], c.eps, coef, s);
}

// BatchNorm backward of either forward mode (operands as ecg_bn_bwd): the training form (batch statistics: reduce + apply)
// or, behind an eval-mode forward, the one-pass affine form (bn_eval_bwd.hip).  The training call is exactly the one the
// plans always made.  (mask_bits: the eval forward writes none, its backward re-reads maskref)
inline int bn_bwd_mode(const BnCfg& c, const void* dout, const void* maskref, const float* gate, const float* addc, int rps,
                       const void* y, const float* coef, const float* gamma, float* dgamma, float* dbeta, void* dy,
                       void* dz_out, float* dbias, long M, int C, float* scratch, hipStream_t s,
                       const unsigned char* mask_bits = nullptr) {
  if (c.training)
    return ecg_bn_bwd(c.dtype, dout, maskref, gate, addc, rps, y, coef, gamma, dgamma, dbeta, dy, dz_out, dbias, M, C,
                      scratch, s, mask_bits);
  return ecg_bn_eval_bwd(c.dtype, dout, maskref, gate, addc, rps, y, coef, dgamma, dbeta, dy, dz_out, dbias, M, C, scratch,
                         s);
}

// The stem convolution (R = 7: 7x7 / 2 / 3; R = 1: 1x7 / 2 / 3 with H = 1) and the number of statistics rows it writes.
// (bf16: statistics rows per workgroup -- sums kept in registers across the workgroup's tiles -- instead of per tile)
inline int stem_forward(int dt, const float* x, const void* wpk, const float* bias, void* y, float* stats, int N, int Cin,
                        int H, int W, int R, hipStream_t s) {
  if (dt == ECGMM_BF16) return ecg_stem_fwd_wgrows(dt, x, wpk, bias, y, stats, N, Cin, H, W, R, s);
  return ecg_stem_fwd(dt, x, wpk, bias, y, stats, N, Cin, H, W, R, s);
}
inline int stem_forward_rows(int dt, int N, int Cin, int H, int W, int R) {
  return dt == ECGMM_BF16 ? ecg_stem_wg_stats_rows(N, Cin, H, W, R) : ecg_stem_stats_rows(N, Cin, H, W, R);
}

// squeeze-excite MLP: g = sigmoid(w2 relu(w1 m + b1) + b2), one launch where head_fused.hip can serve the sizes
inline int se_mlp_forward(const float* m, const float* w1, const float* b1, const float* w2, const float* b2, float* h,
                          float* g, int N, int C, int CR, hipStream_t s) {
  if (ecg_se_mlp_fused_ok(C, CR)) return ecg_se_mlp_fwd(m, w1, b1, w2, b2, h, g, N, C, CR, s);
  ECG_TRY(ecg_linear_fwd(m, w1, b1, h, N, C, CR, ECGMM_ACT_RELU, nullptr, s));
  return ecg_linear_fwd(h, w2, b2, g, N, CR, C, ECGMM_ACT_SIGMOID, nullptr, s);
}

// What one residual block of either training plan keeps for its backward.  (bits: the ReLU mask of `out`, one bit per
// element -- ResNet18 bf16 plans; m h g: the squeeze-excite vectors -- ResNet1D_SE; the downsample set: blocks that have one;
// null otherwise)
struct BlockWs {
  void *w1f, *w1d, *w2f, *w2d, *wdf, *wdd;
  void *y1, *a1, *y2, *yd, *out;
  unsigned char* bits;
  float *coef1, *coef2, *coefd, *m, *h, *g;
};
// The block's part of a forward workspace: N samples of `pix` output pixels, cin -> cout channels, `taps`-tap convolutions,
// es bytes per element; cr: the squeeze-excite bottleneck width (0: no SE vectors).
inline void layout_block(Arena& a, BlockWs& b, int N, size_t pix, int cin, int cout, int taps, bool down, size_t es,
                         bool want_bits, int cr) {
  const size_t osz = (size_t)N * pix * cout, w1 = (size_t)cout * cin * taps * es, w2 = (size_t)cout * cout * taps * es;
  b = BlockWs{};
  b.w1f = a.take_bytes(w1, "w1f");
  b.w1d = a.take_bytes(w1, "w1d");
  b.w2f = a.take_bytes(w2, "w2f");
  b.w2d = a.take_bytes(w2, "w2d");
  b.y1 = a.take_bytes(osz * es, "y1");
  b.a1 = a.take_bytes(osz * es, "a1");
  b.y2 = a.take_bytes(osz * es, "y2");
  b.out = a.take_bytes(osz * es, "out");
  // bn2's backward reads these 1/16-size bytes instead of `out`
  if (want_bits) b.bits = a.take<unsigned char>(osz / 8, "bits");
  b.coef1 = a.take<float>(4 * cout, "coef1");
  b.coef2 = a.take<float>(4 * cout, "coef2");
  if (cr) {
    b.m = a.take<float>((size_t)N * cout, "m");
    b.h = a.take<float>((size_t)N * cr, "h");
    b.g = a.take<float>((size_t)N * cout, "g");
  }
  if (down) {
    b.wdf = a.take_bytes((size_t)cout * cin * es, "wdf");
    b.wdd = a.take_bytes((size_t)cout * cin * es, "wdd");
    b.yd = a.take_bytes(osz * es, "yd");
    b.coefd = a.take<float>(4 * cout, "coefd");
  }
}

// Workspace views (ecgmm_resnet18_ws_view / ecgmm_resnet1d_ws_view): where a named tensor lies inside a plan's workspace,
// for tests and debugging.  A plan runs its own layout_fwd / layout_bwd with a null base and a WsTable attached to the Arena
// (ops.h): every take made with a name is recorded as (name, index, offset, bytes), and the pair is looked up here.  A
// tensor this descriptor does not have was never taken, so it is not in the table.
inline int ws_view_find(const char* who, const WsTable& t, const char* name, int index, size_t ws_bytes, size_t* offset,
                        size_t* bytes) {
  if (t.overflow) ECG_FAIL(ECGMM_ERR_SHAPE, "%s: more named tensors than the view table holds", who);
  for (int i = 0; i < t.n; ++i) {
    const WsTable::Entry& e = t.e[i];
    if (e.index != index || strcmp(e.name, name) != 0) continue;
    if (e.off + e.bytes > ws_bytes) ECG_FAIL(ECGMM_ERR_WORKSPACE, "%s: '%s' ends past the workspace", who, name);
    *offset = e.off;
    *bytes = e.bytes;
    return 0;
  }
  ECG_FAIL(ECGMM_ERR_SHAPE, "%s: no tensor '%s' (index %d) for this descriptor", who, name, index);
}
