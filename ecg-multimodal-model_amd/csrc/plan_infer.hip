// Inference plans of both encoders and of the CRNN front end (gfx950): eval-mode forwards with every BatchNorm folded into the convolution in front
// of it and bias / residual / ReLU applied in the convolution's epilogue.  Opt-in beside the training plans
// (plan_resnet18.hip, plan_resnet1d.hip), which stay what `model.eval()` runs and what a backward or Grad-CAM needs.
//
// Two calls per encoder:
//   prepare : parameters + BatchNorm buffers -> a *prepared blob* (folded packed weights in the compute dtype, folded fp32
//             biases, fp32 copies of the dense-tail weights), ONE batched launch (infer_fold.hip).  Done once per set of
//             weights; the blob depends on dtype, out_dim / num_classes (and cin), eps -- not on the batch or the input size.
//   infer   : input + blob -> features.  Reads nothing but the blob: parameters may change afterwards (the optimizer
//             writes them through raw pointers) without the answer changing until the blob is prepared again.
//
// ResNet18 block (2-3 launches instead of 5-7):   a1 = relu(conv1'(x) + b1');  [yd = convd'(x) + bd'];
//                                                 out = relu(conv2'(a1) + b2' + (yd | x))
// ResNet1D_SE block: a1 as above; y2 = conv2'(a1) + b2'; gate = SE(mean_L y2); [yd]; out = relu(y2 * gate + (yd | x)) in
//   place.  The squeeze needs the whole y2 of a sample, so that last pass cannot be a convolution epilogue.
// Stem: stem_fwd(w', b') -> relu_maxpool (no coefficients, no argmax bytes).
// CRNN front end (behind the encoders): three folded 5x5 blocks, conv + max(0, 2x2 max-pool), block 1 as one kernel.
// ECGTransformer1D (at the end of this file): four launches per encoder layer on the fused tails of transformer_infer.hip.
//
// Workspace: the stem output, the pooled tensor and a fixed set of rotating block buffers of the largest block activation
// instead of one saved set per block; the rotating buffers alias the stem output, which is dead once the max-pool has read it.
#include "plan_common.h"
#include "side_stream.h"

namespace {

// rotating block buffers: `cur` holds the block's input, take() hands out one of the others
struct Rot {
  void* buf[4];
  int cur;
  unsigned used;
  void* take() {
    for (int i = 0; i < 4; ++i)
      if (i != cur && !(used & (1u << i))) { used |= 1u << i; return buf[i]; }
    return nullptr;
  }
  void advance(void* out) {
    for (int i = 0; i < 4; ++i)
      if (buf[i] == out) cur = i;
    used = 0;
  }
};

// The convolutions of one residual block in a prepared blob, either encoder: folded packed weight + folded fp32 bias.
struct BlobConvs { void *w1, *w2, *wd; float *b1, *b2, *bd; };
void layout_blob_convs(Arena& a, BlobConvs& b, int cin, int cout, int taps, bool down, size_t es) {
  b.w1 = a.take_bytes((size_t)cout * cin * taps * es);
  b.b1 = a.take<float>(cout);
  b.w2 = a.take_bytes((size_t)cout * cout * taps * es);
  b.b2 = a.take<float>(cout);
  b.wd = down ? a.take_bytes((size_t)cout * cin * es) : nullptr;
  b.bd = down ? a.take<float>(cout) : nullptr;
}

// Buffers, either encoder: region A holds the stem conv output (y0_bytes) and, once the max-pool has consumed it, three
// rotating block buffers (act_bytes each); B0 (the max-pool's output = block 0's input) is the fourth.  A ResNet18 block with
// a downsample branch has four live tensors (x, a1, yd, out), the others three; ResNet1D_SE: x, a1, y2 (becomes out in
// place), yd.
struct RotWs {
  void* y0;
  void* rot[4];
};
void layout_rot(Arena& a, RotWs& w, size_t y0_bytes, size_t act_bytes) {
  const size_t act = align_up(act_bytes, 256);
  unsigned char* A = (unsigned char*)a.take_bytes(y0_bytes > 3 * act ? y0_bytes : 3 * act);
  w.y0 = A;
  w.rot[0] = a.take_bytes(act);
  for (int i = 0; i < 3; ++i) w.rot[1 + i] = A ? A + i * act : nullptr;
}

// ================================================================================================
// ResNet18
// ================================================================================================
// The network description is net_desc.h's; the blob depends on the weight-only part of it (net18_static) and, beyond what
// the training plans validate, on out_dim and eps.
int build18_static(const ecgmm_resnet18_desc* d, Net18& r) {
  ECG_TRY(net18_static(d, r, "resnet18 infer"));
  if (d->out_dim < 1) ECG_FAIL(ECGMM_ERR_SHAPE, "resnet18 infer: out_dim %d", d->out_dim);
  if (!(d->bn_eps >= 0.f)) ECG_FAIL(ECGMM_ERR_SHAPE, "resnet18 infer: bn_eps %g", (double)d->bn_eps);
  return 0;
}
int build18(const ecgmm_resnet18_desc* d, Net18& r) {
  ECG_TRY(build18_static(d, r));
  return net18_shape(r, "resnet18 infer");
}

struct Blob18 {
  void* wstem; float* bstem;
  BlobConvs b[8];
  float *fcw, *fcb;
  size_t bytes;
};
void layout_blob18(const Net18& r, void* base, Blob18& q) {
  Arena a(base);
  const size_t es = dtype_size(r.d.dtype);
  q.wstem = a.take_bytes(ecg_stem_packed_elems(3, 7) * es);
  q.bstem = a.take<float>(64);
  for (int i = 0; i < 8; ++i) {
    const Blk18& k = r.blk[i];
    layout_blob_convs(a, q.b[i], k.cin, k.cout, 9, k.down, es);
  }
  q.fcw = a.take<float>((size_t)r.d.out_dim * 512);
  q.fcb = a.take<float>(r.d.out_dim);
  q.bytes = align_up(a.off, 256);
}

struct Ws18 : RotWs {
  float* pooled;
  size_t bytes;
};
void layout_ws18(const Net18& r, void* base, Ws18& w) {
  Arena a(base);
  const size_t es = dtype_size(r.d.dtype);
  layout_rot(a, w, (size_t)r.d.N * r.H1 * r.W1 * 64 * es, r.max_act * es);
  w.pooled = a.take<float>((size_t)r.d.N * 512);
  w.bytes = align_up(a.off, 256);
}

// The downsample convolution on a library-owned side stream beside conv1 (as the training forward does), or in line.
// DEFAULT in line: see DESIGN.md (inference plans) for the same-call measurement.
SideStream g_side_inf;
bool down_side_on() { return sw::INFER_DOWN_SIDE.get() != 0; }

// ================================================================================================
// ResNet1D_SE
// ================================================================================================
int build1d_static(const ecgmm_resnet1d_desc* d, Net1D& r) {
  ECG_TRY(net1d_static(d, r, "resnet1d infer"));
  if (d->cin < 1 || d->cin > 24) ECG_FAIL(ECGMM_ERR_SHAPE, "resnet1d infer: cin %d (1..24)", d->cin);
  if (d->num_classes < 1) ECG_FAIL(ECGMM_ERR_SHAPE, "resnet1d infer: num_classes %d", d->num_classes);
  if (!(d->bn_eps >= 0.f)) ECG_FAIL(ECGMM_ERR_SHAPE, "resnet1d infer: bn_eps %g", (double)d->bn_eps);
  return 0;
}
int build1d(const ecgmm_resnet1d_desc* d, Net1D& r) {
  ECG_TRY(build1d_static(d, r));
  return net1d_shape(r, "resnet1d infer");
}

struct Blob1D {
  void* wstem; float* bstem;
  struct B : BlobConvs { float *sw1, *sb1, *sw2, *sb2; } b[3];
  float *cw1, *cb1, *cw2, *cb2;
  size_t bytes;
};
void layout_blob1d(const Net1D& r, void* base, Blob1D& q) {
  Arena a(base);
  const size_t es = dtype_size(r.d.dtype);
  q.wstem = a.take_bytes(ecg_stem_packed_elems(r.d.cin, 1) * es);
  q.bstem = a.take<float>(64);
  for (int i = 0; i < 3; ++i) {
    const Blk1& k = r.blk[i];
    Blob1D::B& b = q.b[i];
    layout_blob_convs(a, b, k.cin, k.cout, 3, k.down, es);
    b.sw1 = a.take<float>((size_t)k.cr * k.cout);
    b.sb1 = a.take<float>(k.cr);
    b.sw2 = a.take<float>((size_t)k.cout * k.cr);
    b.sb2 = a.take<float>(k.cout);
  }
  q.cw1 = a.take<float>(64 * 256);
  q.cb1 = a.take<float>(64);
  q.cw2 = a.take<float>((size_t)r.d.num_classes * 64);
  q.cb2 = a.take<float>(r.d.num_classes);
  q.bytes = align_up(a.off, 256);
}

struct Ws1D : RotWs {
  float *m, *h, *g, *pooled, *h1;
  size_t bytes;
};
void layout_ws1d(const Net1D& r, void* base, Ws1D& w) {
  Arena a(base);
  const size_t es = dtype_size(r.d.dtype);
  layout_rot(a, w, (size_t)r.d.N * r.L1 * 64 * es, r.max_act * es);
  w.m = a.take<float>((size_t)r.d.N * 256);
  w.h = a.take<float>((size_t)r.d.N * 16);
  w.g = a.take<float>((size_t)r.d.N * 256);
  w.pooled = a.take<float>((size_t)r.d.N * 256);
  w.h1 = a.take<float>((size_t)r.d.N * 64);
  w.bytes = align_up(a.off, 256);
}

int check_table(const void* const* table, int n, const char* what, const char* who) {
  if (!table) ECG_FAIL(ECGMM_ERR_SHAPE, "%s: null %s table", who, what);
  for (int i = 0; i < n; ++i)
    if (!table[i]) ECG_FAIL(ECGMM_ERR_SHAPE, "%s: %s %d is null", who, what, i);
  return 0;
}
int check_tables(const void* const* params, int np, const void* const* buffers, int nb, const char* who) {
  ECG_TRY(check_table(params, np, "parameter", who));
  return check_table(buffers, nb, "buffer", who);
}

EcgFoldItem conv_item(int kind, const void* const* params, int p_w, const float* conv_bias, int p_bn,
                      const void* const* buffers, int b_bn, void* wout, float* bout, int Cout, int Cin, int RS) {
  EcgFoldItem it = {};
  it.kind = kind;
  it.w = P(params, p_w); it.conv_bias = conv_bias;
  it.gamma = P(params, p_bn); it.beta = P(params, p_bn + 1);
  it.rm = P(buffers, b_bn); it.rv = P(buffers, b_bn + 1);
  it.wout = wout; it.bout = bout; it.Cout = Cout; it.Cin = Cin; it.RS = RS;
  return it;
}
EcgFoldItem copy_item(const float* src, float* dst, int rows, int cols) {
  EcgFoldItem it = {};
  it.kind = ECG_FOLD_COPY; it.w = src; it.wout = dst; it.Cout = rows; it.Cin = cols; it.RS = 1;
  return it;
}

}  // namespace

// ---- ResNet18 ------------------------------------------------------------------------------------------------------
extern "C" size_t ecgmm_resnet18_infer_prepared_bytes(const ecgmm_resnet18_desc* d) {
  Net18 r;
  if (build18_static(d, r)) return 0;
  Blob18 q;
  layout_blob18(r, nullptr, q);
  return q.bytes;
}

extern "C" int ecgmm_resnet18_infer_prepare(const ecgmm_resnet18_desc* d, const void* const* params,
                                            const void* const* buffers, void* blob, size_t blob_bytes, void* stream_) {
  Net18 r;
  ECG_TRY(build18_static(d, r));
  ECG_TRY(check_tables(params, ECGMM_RESNET18_NPARAMS, buffers, ECGMM_RESNET18_NBUFFERS, "resnet18 infer prepare"));
  Blob18 q;
  layout_blob18(r, blob, q);
  ECG_NEED(blob, blob_bytes, q.bytes, "resnet18 infer prepare: blob");
  EcgFoldItem items[ECG_FOLD_MAX];
  int n = 0;
  items[n++] = conv_item(ECG_FOLD_STEM, params, 0, nullptr, 1, buffers, 0, q.wstem, q.bstem, 64, 3, 7);
  for (int i = 0; i < 8; ++i) {
    const Blk18& k = r.blk[i];
    const BlobConvs& b = q.b[i];
    items[n++] = conv_item(ECG_FOLD_CONV, params, k.p_conv1, nullptr, k.p_bn1, buffers, k.b_bn1, b.w1, b.b1, k.cout, k.cin, 9);
    items[n++] = conv_item(ECG_FOLD_CONV, params, k.p_conv2, nullptr, k.p_bn2, buffers, k.b_bn2, b.w2, b.b2, k.cout, k.cout, 9);
    if (k.down)
      items[n++] = conv_item(ECG_FOLD_CONV, params, k.p_dconv, nullptr, k.p_dbn, buffers, k.b_dbn, b.wd, b.bd, k.cout, k.cin, 1);
  }
  items[n++] = copy_item(P(params, r.p_fc), q.fcw, r.d.out_dim, 512);
  items[n++] = copy_item(P(params, r.p_fc + 1), q.fcb, r.d.out_dim, 1);
  return ecg_fold_batch(r.d.dtype, items, n, r.d.bn_eps, (hipStream_t)stream_);
}

extern "C" size_t ecgmm_resnet18_infer_workspace(const ecgmm_resnet18_desc* d) {
  Net18 r;
  if (build18(d, r)) return 0;
  Ws18 w;
  layout_ws18(r, nullptr, w);
  return w.bytes;
}

extern "C" int ecgmm_resnet18_infer(const ecgmm_resnet18_desc* d, const float* image, const void* blob, size_t blob_bytes,
                                    float* feat_out, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t s = (hipStream_t)stream_;
  Net18 r;
  ECG_TRY(build18(d, r));
  if (!image || !feat_out) ECG_FAIL(ECGMM_ERR_SHAPE, "resnet18 infer: null image / output");
  Blob18 q;
  layout_blob18(r, const_cast<void*>(blob), q);
  ECG_NEED(blob, blob_bytes, q.bytes, "resnet18 infer: blob");
  Ws18 w;
  layout_ws18(r, ws, w);
  ECG_NEED(ws, ws_bytes, w.bytes, "resnet18 infer: workspace");
  const int dt = r.d.dtype, N = r.d.N;
  const bool side = down_side_on();
  if (side) ECG_TRY(g_side_inf.init());

  // (bf16: the instantiation the eval forward of the training plan runs)
  ECG_TRY(stem_forward(dt, image, q.wstem, q.bstem, w.y0, nullptr, N, 3, r.d.H, r.d.W, 7, s));
  ECG_TRY(ecg_relu_maxpool(dt, w.y0, w.rot[0], N, r.H1, r.W1, 64, s));

  Rot rot = {{w.rot[0], w.rot[1], w.rot[2], w.rot[3]}, 0, 0u};
  for (int i = 0; i < 8; ++i) {
    const Blk18& k = r.blk[i];
    const BlobConvs& b = q.b[i];
    const void* cur = rot.buf[rot.cur];
    void* a1 = rot.take();
    void* yd = k.down ? rot.take() : nullptr;
    void* out = rot.take();
    const ConvGeom g1 = k.conv1_geom(N);
    const ConvGeom g2 = k.conv2_geom(N);
    const ConvGeom gd = k.down_geom(N);
    hipEvent_t down_done = nullptr;
    if (k.down && side) {
      g_side_inf.fork(s);
      ECG_TRY(ecg_conv_igemm(dt, 0, gd, cur, b.wd, yd, b.bd, nullptr, nullptr, 0, g_side_inf.s));
      down_done = g_side_inf.mark();
    }
    ECG_TRY(ecg_conv_igemm(dt, 0, g1, cur, b.w1, a1, b.b1, nullptr, nullptr, 1, s));
    if (k.down && !side) ECG_TRY(ecg_conv_igemm(dt, 0, gd, cur, b.wd, yd, b.bd, nullptr, nullptr, 0, s));
    if (down_done) main_wait(s, down_done);
    ECG_TRY(ecg_conv_igemm(dt, 0, g2, a1, b.w2, out, b.b2, k.down ? yd : cur, nullptr, 1, s));
    rot.advance(out);
  }
  const Blk18& last = r.blk[7];
  ECG_TRY(ecg_avgpool(dt, rot.buf[rot.cur], w.pooled, N, last.hout * last.wout, 512, nullptr, s));
  return ecg_linear_fwd(w.pooled, q.fcw, q.fcb, feat_out, N, 512, r.d.out_dim, 0, nullptr, s);
}

// ---- ResNet1D_SE ---------------------------------------------------------------------------------------------------
extern "C" size_t ecgmm_resnet1d_infer_prepared_bytes(const ecgmm_resnet1d_desc* d) {
  Net1D r;
  if (build1d_static(d, r)) return 0;
  Blob1D q;
  layout_blob1d(r, nullptr, q);
  return q.bytes;
}

extern "C" int ecgmm_resnet1d_infer_prepare(const ecgmm_resnet1d_desc* d, const void* const* params,
                                            const void* const* buffers, void* blob, size_t blob_bytes, void* stream_) {
  Net1D r;
  ECG_TRY(build1d_static(d, r));
  ECG_TRY(check_tables(params, ECGMM_RESNET1D_NPARAMS, buffers, ECGMM_RESNET1D_NBUFFERS, "resnet1d infer prepare"));
  Blob1D q;
  layout_blob1d(r, blob, q);
  ECG_NEED(blob, blob_bytes, q.bytes, "resnet1d infer prepare: blob");
  EcgFoldItem items[ECG_FOLD_MAX];
  int n = 0;
  items[n++] = conv_item(ECG_FOLD_STEM, params, 0, P(params, 1), 2, buffers, 0, q.wstem, q.bstem, 64, r.d.cin, 1);
  for (int i = 0; i < 3; ++i) {
    const Blk1& k = r.blk[i];
    const Blob1D::B& b = q.b[i];
    const int p = k.p0, bb = k.b0;
    items[n++] = conv_item(ECG_FOLD_CONV, params, p + T1_CONV1_W, P(params, p + T1_CONV1_B), p + T1_BN1, buffers, bb + T1B_BN1,
                           b.w1, b.b1, k.cout, k.cin, 3);
    items[n++] = conv_item(ECG_FOLD_CONV, params, p + T1_CONV2_W, P(params, p + T1_CONV2_B), p + T1_BN2, buffers, bb + T1B_BN2,
                           b.w2, b.b2, k.cout, k.cout, 3);
    items[n++] = copy_item(P(params, p + T1_SE_W1), b.sw1, k.cr, k.cout);
    items[n++] = copy_item(P(params, p + T1_SE_B1), b.sb1, k.cr, 1);
    items[n++] = copy_item(P(params, p + T1_SE_W2), b.sw2, k.cout, k.cr);
    items[n++] = copy_item(P(params, p + T1_SE_B2), b.sb2, k.cout, 1);
    if (k.down)
      items[n++] = conv_item(ECG_FOLD_CONV, params, p + T1_DOWN_W, P(params, p + T1_DOWN_B), p + T1_DBN, buffers, bb + T1B_DBN,
                             b.wd, b.bd, k.cout, k.cin, 1);
  }
  const int pc = r.p_cls;
  items[n++] = copy_item(P(params, pc + T1_CLS_W1), q.cw1, 64, 256);
  items[n++] = copy_item(P(params, pc + T1_CLS_B1), q.cb1, 64, 1);
  items[n++] = copy_item(P(params, pc + T1_CLS_W2), q.cw2, r.d.num_classes, 64);
  items[n++] = copy_item(P(params, pc + T1_CLS_B2), q.cb2, r.d.num_classes, 1);
  return ecg_fold_batch(r.d.dtype, items, n, r.d.bn_eps, (hipStream_t)stream_);
}

extern "C" size_t ecgmm_resnet1d_infer_workspace(const ecgmm_resnet1d_desc* d) {
  Net1D r;
  if (build1d(d, r)) return 0;
  Ws1D w;
  layout_ws1d(r, nullptr, w);
  return w.bytes;
}

extern "C" int ecgmm_resnet1d_infer(const ecgmm_resnet1d_desc* d, const float* signal, const void* blob, size_t blob_bytes,
                                    float* feat_out, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t s = (hipStream_t)stream_;
  Net1D r;
  ECG_TRY(build1d(d, r));
  if (!signal || !feat_out) ECG_FAIL(ECGMM_ERR_SHAPE, "resnet1d infer: null signal / output");
  Blob1D q;
  layout_blob1d(r, const_cast<void*>(blob), q);
  ECG_NEED(blob, blob_bytes, q.bytes, "resnet1d infer: blob");
  Ws1D w;
  layout_ws1d(r, ws, w);
  ECG_NEED(ws, ws_bytes, w.bytes, "resnet1d infer: workspace");
  const int dt = r.d.dtype, N = r.d.N, cin = r.d.cin;

  ECG_TRY(stem_forward(dt, signal, q.wstem, q.bstem, w.y0, nullptr, N, cin, 1, r.d.L, 1, s));
  ECG_TRY(ecg_relu_maxpool(dt, w.y0, w.rot[0], N, 1, r.L1, 64, s));

  Rot rot = {{w.rot[0], w.rot[1], w.rot[2], w.rot[3]}, 0, 0u};
  for (int i = 0; i < 3; ++i) {
    const Blk1& k = r.blk[i];
    const Blob1D::B& b = q.b[i];
    const void* cur = rot.buf[rot.cur];
    void* a1 = rot.take();
    void* y2 = rot.take();
    void* yd = k.down ? rot.take() : nullptr;
    const long M = (long)N * k.lout;
    const ConvGeom g1 = k.conv1_geom(N);
    const ConvGeom g2 = k.conv2_geom(N);
    ECG_TRY(ecg_conv_igemm(dt, 0, g1, cur, b.w1, a1, b.b1, nullptr, nullptr, 1, s));
    ECG_TRY(ecg_conv_igemm(dt, 0, g2, a1, b.w2, y2, b.b2, nullptr, nullptr, 0, s));
    // squeeze-excite gate from mean_L(y2): y2 already IS bn2(conv2(a1))
    ECG_TRY(ecg_avgpool(dt, y2, w.m, N, k.lout, k.cout, nullptr, s));
    ECG_TRY(se_mlp_forward(w.m, b.sw1, b.sb1, b.sw2, b.sb2, w.h, w.g, N, k.cout, k.cr, s));
    if (k.down) {
      const ConvGeom gd = k.down_geom(N);
      ECG_TRY(ecg_conv_igemm(dt, 0, gd, cur, b.wd, yd, b.bd, nullptr, nullptr, 0, s));
    }
    ECG_TRY(ecg_gate_res_relu(dt, y2, w.g, k.down ? yd : cur, y2, M, k.cout, k.lout, s));
    rot.advance(y2);
  }
  ECG_TRY(ecg_avgpool(dt, rot.buf[rot.cur], w.pooled, N, r.blk[2].lout, 256, nullptr, s));
  ECG_TRY(ecg_linear_fwd(w.pooled, q.cw1, q.cb1, w.h1, N, 256, 64, ECGMM_ACT_RELU, nullptr, s));
  return ecg_linear_fwd(w.h1, q.cw2, q.cb2, feat_out, N, 64, r.d.num_classes, 0, nullptr, s);
}

// ---- CRNN front end ------------------------------------------------------------------------------------------------
// conv1..conv3 of `CRNN` (train_physionet2.py:55-65, 87-93) with the BatchNorms folded: each block is one convolution
// followed by max(0, max over the 2x2 window).  Five launches: block 1 as ONE kernel (crnn_front.hip: the [B,F,T,32]
// tensor, the largest of the model, is never written), then conv_igemm (bias epilogue, no statistics) + relu_maxpool2 for
// blocks 2 and 3, the last one straight into the LSTM's layout.  The training plan's eval mode (plan_crnn.hip) stays what
// a backward needs.
namespace {

int buildc_static(const ecgmm_crnn_front_desc* d, NetC& r) {
  ECG_TRY(netc_static(d, r, "crnn_front infer"));
  if (!(d->bn_eps >= 0.f)) ECG_FAIL(ECGMM_ERR_SHAPE, "crnn_front infer: bn_eps %g", (double)d->bn_eps);
  return 0;
}
int buildc(const ecgmm_crnn_front_desc* d, NetC& r) {
  ECG_TRY(buildc_static(d, r));
  return netc_shape(r, "crnn_front infer");
}

// folded weights: block 1 fp32 OIHW (its kernel rounds the operands itself), blocks 2, 3 the forward pack; fp32 biases
struct BlobC {
  void* w[3];
  float* b[3];
  size_t bytes;
};
void layout_blobc(const NetC& r, void* base, BlobC& q) {
  Arena a(base);
  const size_t es = dtype_size(r.d.dtype);
  for (int i = 0; i < 3; ++i) {
    const BlkC& k = r.blk[i];
    q.w[i] = a.take_bytes((size_t)k.cout * k.cin * 25 * (i == 0 ? sizeof(float) : es));
    q.b[i] = a.take<float>(k.cout);
  }
  q.bytes = align_up(a.off, 256);
}

// pooled outputs of blocks 1, 2 and raw conv outputs of blocks 2, 3; nothing else
struct WsC {
  void* pool[2];
  void* y[3];
  size_t bytes;
};
void layout_wsc(const NetC& r, void* base, WsC& w) {
  Arena a(base);
  const size_t es = dtype_size(r.d.dtype);
  w.y[0] = nullptr;
  for (int i = 0; i < 3; ++i) {
    const BlkC& k = r.blk[i];
    if (i > 0) w.y[i] = a.take_bytes((size_t)k.pixels(r.d.B) * k.cout * es);
    if (i < 2) w.pool[i] = a.take_bytes((size_t)k.pooled(r.d.B) * k.cout * es);
  }
  w.bytes = align_up(a.off, 256);
}

}  // namespace

extern "C" size_t ecgmm_crnn_front_infer_prepared_bytes(const ecgmm_crnn_front_desc* d) {
  NetC r;
  if (buildc_static(d, r)) return 0;
  BlobC q;
  layout_blobc(r, nullptr, q);
  return q.bytes;
}

extern "C" int ecgmm_crnn_front_infer_prepare(const ecgmm_crnn_front_desc* d, const void* const* params,
                                              const void* const* buffers, void* blob, size_t blob_bytes, void* stream_) {
  NetC r;
  ECG_TRY(buildc_static(d, r));
  ECG_TRY(check_tables(params, 12, buffers, 9, "crnn_front infer prepare"));
  BlobC q;
  layout_blobc(r, blob, q);
  ECG_NEED(blob, blob_bytes, q.bytes, "crnn_front infer prepare: blob");
  EcgFoldItem items[3];
  for (int i = 0; i < 3; ++i) {
    const BlkC& k = r.blk[i];
    items[i] = conv_item(i == 0 ? ECG_FOLD_OIHW : ECG_FOLD_CONV, params, k.p0, P(params, k.p0 + 1), k.p0 + 2, buffers, k.b0,
                         q.w[i], q.b[i], k.cout, k.cin, 25);
  }
  return ecg_fold_batch(r.d.dtype, items, 3, r.d.bn_eps, (hipStream_t)stream_);
}

extern "C" size_t ecgmm_crnn_front_infer_workspace(const ecgmm_crnn_front_desc* d) {
  NetC r;
  if (buildc(d, r)) return 0;
  WsC w;
  layout_wsc(r, nullptr, w);
  return w.bytes;
}

extern "C" int ecgmm_crnn_front_infer(const ecgmm_crnn_front_desc* d, const float* spec, const void* blob, size_t blob_bytes,
                                      float* seq_out, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t s = (hipStream_t)stream_;
  NetC r;
  ECG_TRY(buildc(d, r));
  if (!spec || !seq_out) ECG_FAIL(ECGMM_ERR_SHAPE, "crnn_front infer: null spectrogram / output");
  BlobC q;
  layout_blobc(r, const_cast<void*>(blob), q);
  ECG_NEED(blob, blob_bytes, q.bytes, "crnn_front infer: blob");
  WsC w;
  layout_wsc(r, ws, w);
  ECG_NEED(ws, ws_bytes, w.bytes, "crnn_front infer: workspace");
  const int dt = r.d.dtype, B = r.d.B;
  ECG_TRY(ecg_conv5_in1_relu_pool2(dt, spec, (const float*)q.w[0], q.b[0], w.pool[0], B, r.blk[0].h, r.blk[0].w, s));
  for (int i = 1; i < 3; ++i) {
    const BlkC& k = r.blk[i];
    ECG_TRY(ecg_conv_igemm(dt, 0, k.geom(B), w.pool[i - 1], q.w[i], w.y[i], q.b[i], nullptr, nullptr, 0, s));
    ECG_TRY(ecg_relu_maxpool2(dt, w.y[i], i < 2 ? w.pool[i] : (void*)seq_out, B, k.h, k.w, k.cout, i == 2, s));
  }
  return 0;
}

// ---- ECGTransformer1D ----------------------------------------------------------------------------------------------
// The eval forward of `ECGTransformer1D` (train_physionet.py:211-240): embed, then per layer FOUR launches -- in_proj,
// attention, out_proj + residual + norm1 (ecg_linear_res_ln), feed-forward + residual + norm2 (ecg_ffn_res_ln) -- where the
// training composition of ecgmm.hip.nn.TransformerEncoderLayer takes nine, then the mean over the positions and the
// Linear-ReLU-Linear classifier.  Nothing is kept for a backward: three [R, E] buffers rotate through all layers (x, the
// attention output, the next x), qkv and lse are reused by every layer and the [R, ff] hidden activation never exists.
namespace {

constexpr int TFM_HIDDEN = 64;        // the classifier's hidden width (train_physionet.py:227)
constexpr int TFM_LAYER_PARAMS = 12;
constexpr int TFM_MAX_LAYERS = 64;

int buildt_static(const ecgmm_transformer_infer_desc* d, const char* who) {
  if (!d) ECG_FAIL(ECGMM_ERR_SHAPE, "%s: null descriptor", who);
  if (d->layers < 1 || d->layers > TFM_MAX_LAYERS) ECG_FAIL(ECGMM_ERR_SHAPE, "%s: layers=%d (needs 1 <= layers <= 64)", who, d->layers);
  if (d->classes < 1 || d->classes > 4096) ECG_FAIL(ECGMM_ERR_SHAPE, "%s: classes=%d (needs 1 <= classes <= 4096)", who, d->classes);
  if (d->input_dim < 1 || d->input_dim > 12)
    ECG_FAIL(ECGMM_ERR_SHAPE, "%s: input_dim=%d (needs 1 <= input_dim <= 12)", who, d->input_dim);
  if (d->E < 16 || d->E > 256 || d->E % 16)
    ECG_FAIL(ECGMM_ERR_SHAPE, "%s: E=%d (needs a multiple of 16 with 16 <= E <= 256)", who, d->E);
  if (d->ff < 16 || d->ff > 4096 || d->ff % 16)
    ECG_FAIL(ECGMM_ERR_SHAPE, "%s: ff=%d (needs a multiple of 16 with 16 <= ff <= 4096)", who, d->ff);
  if (d->heads < 1 || d->E % d->heads || (d->E / d->heads != 16 && d->E / d->heads != 32))
    ECG_FAIL(ECGMM_ERR_SHAPE, "%s: heads=%d with E=%d (E / heads must be 16 or 32)", who, d->heads, d->E);
  if (d->batch_first != 0 && d->batch_first != 1) ECG_FAIL(ECGMM_ERR_SHAPE, "%s: batch_first=%d (0 or 1)", who, d->batch_first);
  if (!(d->eps >= 0.f)) ECG_FAIL(ECGMM_ERR_SHAPE, "%s: eps %g (needs eps >= 0)", who, (double)d->eps);
  if (d->L < 1 || d->L > (1 << 24)) ECG_FAIL(ECGMM_ERR_SHAPE, "%s: L=%d (needs 1 <= L <= 2^24)", who, d->L);
  return 0;
}
int buildt(const ecgmm_transformer_infer_desc* d, const char* who) {
  ECG_TRY(buildt_static(d, who));
  if (d->B < 1 || d->B > 65535) ECG_FAIL(ECGMM_ERR_SHAPE, "%s: B=%d (needs 1 <= B <= 65535)", who, d->B);
  if ((double)d->B * d->L * 3.0 * d->E > 2147483647.0)
    ECG_FAIL(ECGMM_ERR_SHAPE, "%s: B * L * 3E = %.0f elements is too large", who, (double)d->B * d->L * 3.0 * d->E);
  return 0;
}

struct BlobT {
  struct Layer { float *in_w, *in_b, *out_w, *out_b, *w1, *b1, *w2, *b2, *g1, *be1, *g2, *be2; };
  float *conv_w, *conv_b, *cw1, *cb1, *cw2, *cb2, *pos;
  Layer layer[TFM_MAX_LAYERS];   // filled for d.layers
  size_t bytes;
};
// entry i of the parameter table <-> (destination, floats), in the table's order; the positional table is the blob's LAST
// entry, so every other offset is independent of L.  The ONE walk of the blob: sizes, copy items and every pointer.
struct CopyT { float* dst; size_t n; };
int layout_blobt(const ecgmm_transformer_infer_desc& d, void* base, BlobT& q, CopyT* items) {
  Arena a(base);
  const size_t E = d.E, ff = d.ff;
  int n = 0;
  auto take = [&](size_t count, int slot) {
    float* p = a.take<float>(count);
    if (items) items[slot] = {p, count};
    return p;
  };
  q.conv_w = take(E * d.input_dim * 3, 0);
  q.conv_b = take(E, 1);
  n = 3;
  for (int l = 0; l < d.layers; ++l) {
    BlobT::Layer& k = q.layer[l];
    k.in_w = take(3 * E * E, n++); k.in_b = take(3 * E, n++);
    k.out_w = take(E * E, n++);    k.out_b = take(E, n++);
    k.w1 = take(ff * E, n++);      k.b1 = take(ff, n++);
    k.w2 = take(E * ff, n++);      k.b2 = take(E, n++);
    k.g1 = take(E, n++);           k.be1 = take(E, n++);
    k.g2 = take(E, n++);           k.be2 = take(E, n++);
  }
  q.cw1 = take(TFM_HIDDEN * E, n++);
  q.cb1 = take(TFM_HIDDEN, n++);
  q.cw2 = take((size_t)d.classes * TFM_HIDDEN, n++);
  q.cb2 = take(d.classes, n++);
  q.pos = take((size_t)d.L * E, 2);
  q.bytes = align_up(a.off, 256);
  return n;
}

// x / nxt / att: [R, E] each (att first holds the zero-padded copy of the raw input: input_dim <= 12 < E); qkv [R, 3E];
// lse [R heads]; the tail's [B, E], [B, 64] and [B] int32.  Nothing here depends on layers or on ff.
struct WsT {
  float *x, *nxt, *att, *qkv, *lse, *pooled, *h1;
  int* lens;
  size_t bytes;
};
void layout_wst(const ecgmm_transformer_infer_desc& d, void* base, WsT& w) {
  Arena a(base);
  const size_t R = (size_t)d.B * d.L, E = d.E;
  w.x = a.take<float>(R * E);
  w.nxt = a.take<float>(R * E);
  w.att = a.take<float>(R * E);
  w.qkv = a.take<float>(R * 3 * E);
  w.lse = a.take<float>(R * d.heads);
  w.pooled = a.take<float>((size_t)d.B * E);
  w.h1 = a.take<float>((size_t)d.B * TFM_HIDDEN);
  w.lens = a.take<int>(d.B);
  w.bytes = align_up(a.off, 256);
}
inline bool avgpool_width_ok(int C) { return C % 4 == 0 && 256 % (C / 4) == 0; }   // the widths ecg_avgpool takes in fp32

}  // namespace

extern "C" size_t ecgmm_transformer_infer_prepared_bytes(const ecgmm_transformer_infer_desc* d) {
  if (buildt_static(d, "transformer infer")) return 0;
  BlobT q;
  layout_blobt(*d, nullptr, q, nullptr);
  return q.bytes;
}

extern "C" int ecgmm_transformer_infer_prepare(const ecgmm_transformer_infer_desc* d, const void* const* params, void* blob,
                                               size_t blob_bytes, void* stream_) {
  ECG_TRY(buildt_static(d, "transformer infer prepare"));
  const int np = 3 + TFM_LAYER_PARAMS * d->layers + 4;
  ECG_TRY(check_table(params, np, "parameter", "transformer infer prepare"));
  BlobT q;
  CopyT items[3 + TFM_LAYER_PARAMS * TFM_MAX_LAYERS + 4];
  layout_blobt(*d, blob, q, items);
  ECG_NEED(blob, blob_bytes, q.bytes, "transformer infer prepare: blob");
  for (int i = 0; i < np; ++i) {
    hipError_t e = hipMemcpyAsync(items[i].dst, params[i], items[i].n * sizeof(float), hipMemcpyDeviceToDevice,
                                  (hipStream_t)stream_);
    if (e != hipSuccess) ECG_FAIL(ECGMM_ERR_LAUNCH, "transformer infer prepare: copy of parameter %d: %s", i, hipGetErrorString(e));
  }
  return 0;
}

extern "C" size_t ecgmm_transformer_infer_workspace(const ecgmm_transformer_infer_desc* d) {
  if (buildt(d, "transformer infer")) return 0;
  WsT w;
  layout_wst(*d, nullptr, w);
  return w.bytes;
}

extern "C" int ecgmm_transformer_infer(const ecgmm_transformer_infer_desc* d, const float* x, const int32_t* lengths,
                                       const void* blob, size_t blob_bytes, float* logits, void* ws, size_t ws_bytes,
                                       void* stream_) {
  hipStream_t s = (hipStream_t)stream_;
  ECG_TRY(buildt(d, "transformer infer"));
  if (!x || !logits) ECG_FAIL(ECGMM_ERR_SHAPE, "transformer infer: null input / output");
  if (lengths && !d->batch_first)
    ECG_FAIL(ECGMM_ERR_SHAPE, "transformer infer: lengths need batch_first = 1 (attention across the batch has no per-record length)");
  BlobT q;
  layout_blobt(*d, const_cast<void*>(blob), q, nullptr);
  ECG_NEED(blob, blob_bytes, q.bytes, "transformer infer: blob");
  WsT w;
  layout_wst(*d, ws, w);
  ECG_NEED(ws, ws_bytes, w.bytes, "transformer infer: workspace");
  const int B = d->B, L = d->L, E = d->E;
  const long R = (long)B * L;

  if (lengths) {   // the conv's right tap at a record's last live position reads the first padded sample
    ECG_TRY(ecg_mask_pad_rows(x, lengths, w.att, B, d->input_dim, L, s));
    x = w.att;
  }
  ECG_TRY(ecgmm_embed1d_fwd(x, q.conv_w, q.conv_b, q.pos, w.x, B, d->input_dim, L, E, stream_));
  ecgmm_mha_desc m = {};
  m.S = d->batch_first ? L : B;
  m.N = d->batch_first ? B : L;
  m.heads = d->heads; m.head_dim = E / d->heads; m.batch_first = d->batch_first; m.p_drop = 0.f;
  for (int l = 0; l < d->layers; ++l) {
    const BlobT::Layer& k = q.layer[l];
    ECG_TRY(ecg_linear_fwd(w.x, k.in_w, k.in_b, w.qkv, (int)R, E, 3 * E, 0, nullptr, s));
    if (lengths) ECG_TRY(ecgmm_mha_forward_varlen(&m, w.qkv, lengths, w.att, w.lse, 0, 0, stream_));
    else ECG_TRY(ecgmm_mha_forward(&m, w.qkv, w.att, w.lse, 0, 0, stream_));
    ECG_TRY(ecg_linear_res_ln(w.att, k.out_w, k.out_b, w.x, k.g1, k.be1, w.nxt, R, E, E, d->eps, s));
    ECG_TRY(ecg_ffn_res_ln(w.nxt, k.w1, k.b1, k.w2, k.b2, k.g2, k.be2, w.x, R, E, d->ff, d->eps, s));
  }
  if (lengths) {
    ECG_TRY(ecg_seq_mean_varlen_fwd(w.x, lengths, w.pooled, B, L, E, s));
  } else if (avgpool_width_ok(E)) {
    ECG_TRY(ecg_avgpool(ECGMM_F32, w.x, w.pooled, B, L, E, nullptr, s));
  } else {   // a width the pooling kernel does not take: the masked mean over every record's full length
    ECG_TRY(ecg_fill_i32(w.lens, L, B, s));
    ECG_TRY(ecg_seq_mean_varlen_fwd(w.x, w.lens, w.pooled, B, L, E, s));
  }
  ECG_TRY(ecg_linear_fwd(w.pooled, q.cw1, q.cb1, w.h1, B, E, TFM_HIDDEN, ECGMM_ACT_RELU, nullptr, s));
  return ecg_linear_fwd(w.h1, q.cw2, q.cb2, logits, B, TFM_HIDDEN, d->classes, 0, nullptr, s);
}
