// Launch plan of the CRNN convolutional front end (train_physionet2.py:55-65, 87-93): conv1..conv3 of `CRNN`, each
// Conv2d(k = 5, pad = 2, bias) -> BatchNorm2d -> ReLU -> MaxPool2d(2), then permute(0,3,1,2) + Flatten(2): one call per
// direction, spectrogram [B,1,F,T] fp32 in, seq [B, T/8, 128 * (F/8)] fp32 out.  Kernels: crnn_front.hip (Cin = 1
// convolution, 5x5 weight gradients, pooling) and conv_igemm.hip at R = S = 5 (forward / input gradient of blocks 2, 3).
#include "plan_common.h"

namespace {

// The three blocks are described once, in net_desc.h (NetC, BlkC, netc_build): the inference plan walks the same record.

int stats_rows_of(const NetC& n, int i) {
  const BlkC& k = n.blk[i];
  return i == 0 ? ecg_conv5_in1_stats_rows(n.d.B, k.h, k.w) : ecg_conv_stats_rows(k.pixels(n.d.B));
}

struct FwdC {
  void* y[3];            // raw conv outputs [B][h][w][cout], compute dtype
  float* coef[3];        // [4][cout]
  unsigned char* idx[3]; // pool winners
  void* pool[2];         // pooled outputs of blocks 1, 2 = inputs of blocks 2, 3
  void* wf[3];           // packed weights of blocks 2, 3 (index 1, 2): forward, dgrad
  void* wd[3];
  float* stats;
  size_t bytes;
};
FwdC fwd_carve(const NetC& n, void* ws) {
  FwdC f;
  memset(&f, 0, sizeof(f));
  Arena a(ws);
  const size_t esz = dtype_size(n.d.dtype);
  int rows = 0;
  for (int i = 0; i < 3; ++i) {
    const BlkC& k = n.blk[i];
    f.y[i] = a.take_bytes((size_t)k.pixels(n.d.B) * k.cout * esz);
    f.coef[i] = a.take<float>(4 * k.cout);
    f.idx[i] = a.take<unsigned char>((size_t)k.pooled(n.d.B) * k.cout);
    if (i < 2) f.pool[i] = a.take_bytes((size_t)k.pooled(n.d.B) * k.cout * esz);
    if (i > 0) {
      f.wf[i] = a.take_bytes((size_t)k.cout * k.cin * 25 * esz);
      f.wd[i] = a.take_bytes((size_t)k.cout * k.cin * 25 * esz);
    }
    if (stats_rows_of(n, i) > rows) rows = stats_rows_of(n, i);
  }
  f.stats = a.take<float>((size_t)(rows + ECG_TAIL_ROWS) * 2 * 128);
  f.bytes = align_up(a.off, 256);
  return f;
}

struct BwdC {
  void* dy[3];     // gradient of the raw conv outputs
  void* dx[3];     // input gradient of blocks 2, 3 (index 1, 2) = pooled gradient of blocks 1, 2
  void* pool_ws; size_t pool_bytes;
  void* wg_ws; size_t wg_bytes;
  size_t bytes;
};
BwdC bwd_carve(const NetC& n, void* ws) {
  BwdC b;
  memset(&b, 0, sizeof(b));
  Arena a(ws);
  const size_t esz = dtype_size(n.d.dtype);
  for (int i = 0; i < 3; ++i) {
    const BlkC& k = n.blk[i];
    b.dy[i] = a.take_bytes((size_t)k.pixels(n.d.B) * k.cout * esz);
    if (i > 0) b.dx[i] = a.take_bytes((size_t)k.pixels(n.d.B) * k.cin * esz);
    const size_t pw = ecg_pool2_bn_bwd_workspace(n.d.B, k.h, k.w, k.cout);
    if (pw > b.pool_bytes) b.pool_bytes = pw;
    const size_t ww = i == 0 ? ecg_conv5_in1_wgrad_workspace(n.d.B, k.h, k.w) : ecg_conv5_wgrad_workspace(n.d.dtype, k.geom(n.d.B));
    if (ww > b.wg_bytes) b.wg_bytes = ww;
  }
  b.pool_ws = a.take_bytes(b.pool_bytes);
  b.wg_ws = a.take_bytes(b.wg_bytes);
  b.bytes = align_up(a.off, 256);
  return b;
}

}  // namespace

extern "C" {

size_t ecgmm_crnn_front_fwd_workspace(const ecgmm_crnn_front_desc* d) {
  NetC n;
  if (netc_build(d, n, "crnn_front_fwd_workspace") != 0) return 0;
  return fwd_carve(n, nullptr).bytes;
}
size_t ecgmm_crnn_front_bwd_workspace(const ecgmm_crnn_front_desc* d) {
  NetC n;
  if (netc_build(d, n, "crnn_front_bwd_workspace") != 0) return 0;
  return bwd_carve(n, nullptr).bytes;
}

int ecgmm_crnn_front_forward(const ecgmm_crnn_front_desc* d, const float* spec, const void* const* params,
                             void* const* buffers, float* seq_out, void* ws, size_t ws_bytes, void* stream) {
  NetC n;
  ECG_TRY(netc_build(d, n, "crnn_front_forward"));
  if (!spec || !params || !buffers || !seq_out) ECG_FAIL(ECGMM_ERR_SHAPE, "crnn_front_forward: null operand");
  for (int i = 0; i < 12; ++i)
    if (!params[i]) ECG_FAIL(ECGMM_ERR_SHAPE, "crnn_front_forward: null parameter %d", i);
  const FwdC f = fwd_carve(n, ws);
  ECG_NEED(ws, ws_bytes, f.bytes, "crnn_front_forward: workspace");
  hipStream_t s = (hipStream_t)stream;
  const int B = n.d.B, dt = n.d.dtype;
  for (int i = 0; i < 3; ++i) {
    const BlkC& k = n.blk[i];
    int rows = stats_rows_of(n, i);
    if (i == 0) {
      ECG_TRY(ecg_conv5_in1_fwd(dt, spec, P(params, k.p0), P(params, k.p0 + 1), f.y[0], f.stats, B, k.h, k.w, s));
    } else {
      ECG_TRY(ecg_pack_weight(dt, P(params, k.p0), f.wf[i], f.wd[i], k.cout, k.cin, 25, s));
      ConvEpi e = {};
      e.wg_rows = 1;
      ECG_TRY(ecg_conv_igemm(dt, 0, k.geom(B), f.pool[i - 1], f.wf[i], f.y[i], P(params, k.p0 + 1), nullptr, f.stats, 0, s, &e));
      if (e.stats_rows > 0) rows = e.stats_rows;
    }
    ECG_TRY(bn_coef(n.bn, f.stats, rows, k.cout, k.pixels(B), params, k.p0 + 2, buffers, k.b0, f.coef[i], s));
    ECG_TRY(ecg_bnrelu_maxpool2(dt, f.y[i], f.coef[i], i < 2 ? f.pool[i] : (void*)seq_out, f.idx[i], B, k.h, k.w, k.cout,
                                i == 2, s));
  }
  return 0;
}

int ecgmm_crnn_front_backward_dx(const ecgmm_crnn_front_desc* d, const float* spec, const float* dseq,
                                 const void* const* params, void* const* grads, void* ws_fwd, void* ws_bwd,
                                 size_t ws_bwd_bytes, float* dspec, void* stream) {
  NetC n;
  ECG_TRY(netc_build(d, n, "crnn_front_backward"));
  if (!spec || !dseq || !params || !ws_fwd) ECG_FAIL(ECGMM_ERR_SHAPE, "crnn_front_backward: null operand");
  if (dspec && !params[0]) ECG_FAIL(ECGMM_ERR_SHAPE, "crnn_front_backward: null parameter 0 (the input gradient reads conv1's weight)");
  const FwdC f = fwd_carve(n, ws_fwd);
  const BwdC b = bwd_carve(n, ws_bwd);
  ECG_NEED(ws_bwd, ws_bwd_bytes, b.bytes, "crnn_front_backward: workspace");
  hipStream_t s = (hipStream_t)stream;
  const int B = n.d.B, dt = n.d.dtype;
  for (int i = 2; i >= 0; --i) {
    const BlkC& k = n.blk[i];
    const void* dp = i == 2 ? (const void*)dseq : b.dx[i + 1];
    ECG_TRY(ecg_pool2_bn_bwd(dt, dp, f.idx[i], f.y[i], f.coef[i], n.d.training, G(grads, k.p0 + 2), G(grads, k.p0 + 3), b.dy[i],
                             G(grads, k.p0 + 1), B, k.h, k.w, k.cout, i == 2, b.pool_ws, b.pool_bytes, s));
    if (i == 0) {
      if (G(grads, 0) || G(grads, 1))   // (dbias was written above; the weight gradient alone here)
        ECG_TRY(ecg_conv5_in1_wgrad(dt, spec, b.dy[0], G(grads, 0), nullptr, 0, b.wg_ws, b.wg_bytes, B, k.h, k.w, s));
      if (dspec) ECG_TRY(ecg_conv5_in1_dgrad(dt, b.dy[0], P(params, 0), dspec, B, k.h, k.w, s));
      break;
    }
    ECG_TRY(ecg_conv_igemm(dt, 1, k.geom(B), b.dy[i], f.wd[i], b.dx[i], nullptr, nullptr, nullptr, 0, s));
    if (G(grads, k.p0))
      ECG_TRY(ecg_conv5_wgrad(dt, k.geom(B), f.pool[i - 1], b.dy[i], G(grads, k.p0), 0, b.wg_ws, b.wg_bytes, s));
  }
  return 0;
}

int ecgmm_crnn_front_backward(const ecgmm_crnn_front_desc* d, const float* spec, const float* dseq, const void* const* params,
                              void* const* grads, void* ws_fwd, void* ws_bwd, size_t ws_bwd_bytes, void* stream) {
  return ecgmm_crnn_front_backward_dx(d, spec, dseq, params, grads, ws_fwd, ws_bwd, ws_bwd_bytes, nullptr, stream);
}

}  // extern "C"
