// Inference plans of both encoders (gfx950): eval-mode forwards with every BatchNorm folded into the convolution in front
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
//
// Workspace: the stem output, the pooled tensor and a fixed set of rotating block buffers of the largest block activation
// instead of one saved set per block; the rotating buffers alias the stem output, which is dead once the max-pool has read it.
#include <stdlib.h>

#include "ops.h"
#include "side_stream.h"

namespace {

int check_dtype(int dtype, const char* who) {
  if (dtype != ECGMM_BF16 && dtype != ECGMM_F32) ECG_FAIL(ECGMM_ERR_DTYPE, "%s: bad dtype %d", who, dtype);
  return 0;
}

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

// ================================================================================================
// ResNet18
// ================================================================================================
struct Blk18 {
  int cin, cout, stride, hin, win, hout, wout;
  bool down;
  int p_conv1, p_bn1, p_conv2, p_bn2, p_dconv, p_dbn;  // parameter indices (weight; bn bias = +1)
  int b_bn1, b_bn2, b_dbn;                              // buffer indices (rm; rv = +1)
};
struct I18 {
  ecgmm_resnet18_desc d;
  int H1, W1, H2, W2;
  Blk18 blk[8];
  int p_fc;
  size_t max_act;
};

// the weight-only part of the description (what the blob depends on)
int build18_static(const ecgmm_resnet18_desc* d, I18& r) {
  if (!d) ECG_FAIL(ECGMM_ERR_SHAPE, "resnet18 infer: null desc");
  ECG_TRY(check_dtype(d->dtype, "resnet18 infer"));
  if (d->out_dim < 1) ECG_FAIL(ECGMM_ERR_SHAPE, "resnet18 infer: out_dim %d", d->out_dim);
  if (!(d->bn_eps >= 0.f)) ECG_FAIL(ECGMM_ERR_SHAPE, "resnet18 infer: bn_eps %g", (double)d->bn_eps);
  r.d = *d;
  int pi = 3, bi = 3, cin = 64;
  for (int L = 0; L < 4; ++L) {
    const int cout = 64 << L;
    for (int b = 0; b < 2; ++b) {
      Blk18& k = r.blk[L * 2 + b];
      k.cin = cin; k.cout = cout; k.stride = (b == 0 && L > 0) ? 2 : 1;
      k.down = (k.stride != 1 || cin != cout);
      k.p_conv1 = pi; k.p_bn1 = pi + 1; k.p_conv2 = pi + 3; k.p_bn2 = pi + 4; pi += 6;
      k.b_bn1 = bi; k.b_bn2 = bi + 3; bi += 6;
      if (k.down) { k.p_dconv = pi; k.p_dbn = pi + 1; pi += 3; k.b_dbn = bi; bi += 3; }
      else k.p_dconv = k.p_dbn = k.b_dbn = -1;
      cin = cout;
    }
  }
  r.p_fc = pi;
  if (pi + 2 != ECGMM_RESNET18_NPARAMS || bi != ECGMM_RESNET18_NBUFFERS)
    ECG_FAIL(ECGMM_ERR_SHAPE, "resnet18 infer: internal table mismatch %d %d", pi + 2, bi);
  return 0;
}
int build18(const ecgmm_resnet18_desc* d, I18& r) {
  ECG_TRY(build18_static(d, r));
  if (d->N < 1 || d->H < 32 || d->W < 32) ECG_FAIL(ECGMM_ERR_SHAPE, "resnet18 infer: bad input %dx%dx%d", d->N, d->H, d->W);
  r.H1 = (d->H + 6 - 7) / 2 + 1;
  r.W1 = (d->W + 6 - 7) / 2 + 1;
  r.H2 = (r.H1 + 2 - 3) / 2 + 1;
  r.W2 = (r.W1 + 2 - 3) / 2 + 1;
  int h = r.H2, w = r.W2;
  r.max_act = (size_t)d->N * h * w * 64;
  for (int i = 0; i < 8; ++i) {
    Blk18& k = r.blk[i];
    k.hin = h; k.win = w;
    k.hout = (h + 2 - 3) / k.stride + 1;
    k.wout = (w + 2 - 3) / k.stride + 1;
    const size_t a = (size_t)d->N * k.hout * k.wout * k.cout;
    if (a > r.max_act) r.max_act = a;
    h = k.hout; w = k.wout;
  }
  return 0;
}

struct Blob18 {
  void* wstem; float* bstem;
  struct B { void *w1, *w2, *wd; float *b1, *b2, *bd; } b[8];
  float *fcw, *fcb;
  size_t bytes;
};
void layout_blob18(const I18& r, void* base, Blob18& q) {
  Arena a(base);
  const size_t es = dtype_size(r.d.dtype);
  q.wstem = a.take_bytes(ecg_stem_packed_elems(3, 7) * es);
  q.bstem = a.take<float>(64);
  for (int i = 0; i < 8; ++i) {
    const Blk18& k = r.blk[i];
    Blob18::B& b = q.b[i];
    b.w1 = a.take_bytes((size_t)k.cout * k.cin * 9 * es);
    b.b1 = a.take<float>(k.cout);
    b.w2 = a.take_bytes((size_t)k.cout * k.cout * 9 * es);
    b.b2 = a.take<float>(k.cout);
    b.wd = k.down ? a.take_bytes((size_t)k.cout * k.cin * es) : nullptr;
    b.bd = k.down ? a.take<float>(k.cout) : nullptr;
  }
  q.fcw = a.take<float>((size_t)r.d.out_dim * 512);
  q.fcb = a.take<float>(r.d.out_dim);
  q.bytes = align_up(a.off, 256);
}

// Buffers: region A holds the stem conv output and, once the max-pool has consumed it, three rotating block buffers;
// B0 (the max-pool's output = block 0's input) is the fourth.  A block with a downsample branch has four live tensors
// (x, a1, yd, out), the others three.
struct Ws18 {
  void* y0;
  void* rot[4];
  float* pooled;
  size_t bytes;
};
void layout_ws18(const I18& r, void* base, Ws18& w) {
  Arena a(base);
  const size_t es = dtype_size(r.d.dtype);
  const size_t act = align_up(r.max_act * es, 256), y0 = (size_t)r.d.N * r.H1 * r.W1 * 64 * es;
  unsigned char* A = (unsigned char*)a.take_bytes(y0 > 3 * act ? y0 : 3 * act);
  w.y0 = A;
  w.rot[0] = a.take_bytes(act);
  for (int i = 0; i < 3; ++i) w.rot[1 + i] = A ? A + i * act : nullptr;
  w.pooled = a.take<float>((size_t)r.d.N * 512);
  w.bytes = align_up(a.off, 256);
}

// The downsample convolution on a library-owned side stream beside conv1 (as the training forward does), or in line.
// DEFAULT in line: see DESIGN.md (inference plans) for the same-call measurement.
SideStream g_side_inf;
int g_down_side = -1;
bool down_side_on() {
  if (g_down_side < 0) { const char* e = getenv("ECGMM_INFER_DOWN_SIDE"); g_down_side = (e && e[0] == '1'); }
  return g_down_side != 0;
}

inline const float* P(const void* const* t, int i) { return (const float*)t[i]; }

// ================================================================================================
// ResNet1D_SE
// ================================================================================================
struct Blk1 {
  int cin, cout, stride, lin, lout, cr;
  bool down;
  int p0, b0;
};
struct I1D {
  ecgmm_resnet1d_desc d;
  int L1, L2;
  Blk1 blk[3];
  int p_cls;
  size_t max_act;
};
int build1d_static(const ecgmm_resnet1d_desc* d, I1D& r) {
  if (!d) ECG_FAIL(ECGMM_ERR_SHAPE, "resnet1d infer: null desc");
  ECG_TRY(check_dtype(d->dtype, "resnet1d infer"));
  if (d->cin < 1 || d->cin > 24) ECG_FAIL(ECGMM_ERR_SHAPE, "resnet1d infer: cin %d (1..24)", d->cin);
  if (d->num_classes < 1) ECG_FAIL(ECGMM_ERR_SHAPE, "resnet1d infer: num_classes %d", d->num_classes);
  if (!(d->bn_eps >= 0.f)) ECG_FAIL(ECGMM_ERR_SHAPE, "resnet1d infer: bn_eps %g", (double)d->bn_eps);
  r.d = *d;
  int pi = 4, bi = 3, cin = 64;
  for (int i = 0; i < 3; ++i) {
    Blk1& k = r.blk[i];
    k.cin = cin; k.cout = 64 << i; k.stride = i == 0 ? 1 : 2;
    k.cr = k.cout / 16;
    k.down = (k.stride != 1 || k.cin != k.cout);
    k.p0 = pi; k.b0 = bi;
    pi += k.down ? 16 : 12;
    bi += k.down ? 9 : 6;
    cin = k.cout;
  }
  r.p_cls = pi;
  if (pi + 4 != ECGMM_RESNET1D_NPARAMS || bi != ECGMM_RESNET1D_NBUFFERS)
    ECG_FAIL(ECGMM_ERR_SHAPE, "resnet1d infer: internal table mismatch %d %d", pi + 4, bi);
  return 0;
}
int build1d(const ecgmm_resnet1d_desc* d, I1D& r) {
  ECG_TRY(build1d_static(d, r));
  if (d->N < 1 || d->L < 64) ECG_FAIL(ECGMM_ERR_SHAPE, "resnet1d infer: bad input N=%d L=%d", d->N, d->L);
  r.L1 = (d->L + 6 - 7) / 2 + 1;
  r.L2 = (r.L1 + 2 - 3) / 2 + 1;
  int l = r.L2;
  r.max_act = (size_t)d->N * r.L2 * 64;
  for (int i = 0; i < 3; ++i) {
    Blk1& k = r.blk[i];
    k.lin = l; k.lout = (l + 2 - 3) / k.stride + 1;
    const size_t a = (size_t)d->N * k.lout * k.cout;
    if (a > r.max_act) r.max_act = a;
    l = k.lout;
  }
  return 0;
}

struct Blob1D {
  void* wstem; float* bstem;
  struct B { void *w1, *w2, *wd; float *b1, *b2, *bd, *sw1, *sb1, *sw2, *sb2; } b[3];
  float *cw1, *cb1, *cw2, *cb2;
  size_t bytes;
};
void layout_blob1d(const I1D& r, void* base, Blob1D& q) {
  Arena a(base);
  const size_t es = dtype_size(r.d.dtype);
  q.wstem = a.take_bytes(ecg_stem_packed_elems(r.d.cin, 1) * es);
  q.bstem = a.take<float>(64);
  for (int i = 0; i < 3; ++i) {
    const Blk1& k = r.blk[i];
    Blob1D::B& b = q.b[i];
    b.w1 = a.take_bytes((size_t)k.cout * k.cin * 3 * es);
    b.b1 = a.take<float>(k.cout);
    b.w2 = a.take_bytes((size_t)k.cout * k.cout * 3 * es);
    b.b2 = a.take<float>(k.cout);
    b.wd = k.down ? a.take_bytes((size_t)k.cout * k.cin * es) : nullptr;
    b.bd = k.down ? a.take<float>(k.cout) : nullptr;
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

struct Ws1D {
  void* y0;
  void* rot[4];   // x, a1, y2 (becomes out in place), yd
  float *m, *h, *g, *pooled, *h1;
  size_t bytes;
};
void layout_ws1d(const I1D& r, void* base, Ws1D& w) {
  Arena a(base);
  const size_t es = dtype_size(r.d.dtype);
  const size_t act = align_up(r.max_act * es, 256), y0 = (size_t)r.d.N * r.L1 * 64 * es;
  unsigned char* A = (unsigned char*)a.take_bytes(y0 > 3 * act ? y0 : 3 * act);
  w.y0 = A;
  w.rot[0] = a.take_bytes(act);
  for (int i = 0; i < 3; ++i) w.rot[1 + i] = A ? A + i * act : nullptr;
  w.m = a.take<float>((size_t)r.d.N * 256);
  w.h = a.take<float>((size_t)r.d.N * 16);
  w.g = a.take<float>((size_t)r.d.N * 256);
  w.pooled = a.take<float>((size_t)r.d.N * 256);
  w.h1 = a.take<float>((size_t)r.d.N * 64);
  w.bytes = align_up(a.off, 256);
}

int check_tables(const void* const* params, int np, const void* const* buffers, int nb, const char* who) {
  if (!params || !buffers) ECG_FAIL(ECGMM_ERR_SHAPE, "%s: null parameter / buffer table", who);
  for (int i = 0; i < np; ++i)
    if (!params[i]) ECG_FAIL(ECGMM_ERR_SHAPE, "%s: parameter %d is null", who, i);
  for (int i = 0; i < nb; ++i)
    if (!buffers[i]) ECG_FAIL(ECGMM_ERR_SHAPE, "%s: buffer %d is null", who, i);
  return 0;
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
  I18 r;
  if (build18_static(d, r)) return 0;
  Blob18 q;
  layout_blob18(r, nullptr, q);
  return q.bytes;
}

extern "C" int ecgmm_resnet18_infer_prepare(const ecgmm_resnet18_desc* d, const void* const* params,
                                            const void* const* buffers, void* blob, size_t blob_bytes, void* stream_) {
  I18 r;
  ECG_TRY(build18_static(d, r));
  ECG_TRY(check_tables(params, ECGMM_RESNET18_NPARAMS, buffers, ECGMM_RESNET18_NBUFFERS, "resnet18 infer prepare"));
  Blob18 q;
  layout_blob18(r, blob, q);
  if (!blob || blob_bytes < q.bytes) ECG_FAIL(ECGMM_ERR_WORKSPACE, "resnet18 infer prepare: blob %zu < %zu", blob_bytes, q.bytes);
  EcgFoldItem items[ECG_FOLD_MAX];
  int n = 0;
  items[n++] = conv_item(ECG_FOLD_STEM, params, 0, nullptr, 1, buffers, 0, q.wstem, q.bstem, 64, 3, 7);
  for (int i = 0; i < 8; ++i) {
    const Blk18& k = r.blk[i];
    const Blob18::B& b = q.b[i];
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
  I18 r;
  if (build18(d, r)) return 0;
  Ws18 w;
  layout_ws18(r, nullptr, w);
  return w.bytes;
}

extern "C" int ecgmm_infer_down_side(int on) {
  g_down_side = on != 0;
  return 0;
}

extern "C" int ecgmm_resnet18_infer(const ecgmm_resnet18_desc* d, const float* image, const void* blob, size_t blob_bytes,
                                    float* feat_out, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t s = (hipStream_t)stream_;
  I18 r;
  ECG_TRY(build18(d, r));
  if (!image || !feat_out) ECG_FAIL(ECGMM_ERR_SHAPE, "resnet18 infer: null image / output");
  Blob18 q;
  layout_blob18(r, const_cast<void*>(blob), q);
  if (!blob || blob_bytes < q.bytes) ECG_FAIL(ECGMM_ERR_WORKSPACE, "resnet18 infer: blob %zu < %zu", blob_bytes, q.bytes);
  Ws18 w;
  layout_ws18(r, ws, w);
  if (!ws || ws_bytes < w.bytes) ECG_FAIL(ECGMM_ERR_WORKSPACE, "resnet18 infer: workspace %zu < %zu", ws_bytes, w.bytes);
  const int dt = r.d.dtype, N = r.d.N;
  const bool side = down_side_on();
  if (side) ECG_TRY(g_side_inf.init());

  // (bf16: the instantiation the eval forward of the training plan runs)
  if (dt == ECGMM_BF16) ECG_TRY(ecg_stem_fwd_wgrows(dt, image, q.wstem, q.bstem, w.y0, nullptr, N, 3, r.d.H, r.d.W, 7, s));
  else ECG_TRY(ecg_stem_fwd(dt, image, q.wstem, q.bstem, w.y0, nullptr, N, 3, r.d.H, r.d.W, 7, s));
  ECG_TRY(ecg_relu_maxpool(dt, w.y0, w.rot[0], N, r.H1, r.W1, 64, s));

  Rot rot = {{w.rot[0], w.rot[1], w.rot[2], w.rot[3]}, 0, 0u};
  for (int i = 0; i < 8; ++i) {
    const Blk18& k = r.blk[i];
    const Blob18::B& b = q.b[i];
    const void* cur = rot.buf[rot.cur];
    void* a1 = rot.take();
    void* yd = k.down ? rot.take() : nullptr;
    void* out = rot.take();
    const ConvGeom g1 = make_geom(N, k.hin, k.win, k.cin, k.cout, 3, 3, k.stride, 1, 1);
    const ConvGeom g2 = make_geom(N, k.hout, k.wout, k.cout, k.cout, 3, 3, 1, 1, 1);
    const ConvGeom gd = make_geom(N, k.hin, k.win, k.cin, k.cout, 1, 1, k.stride, 0, 0);
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
  I1D r;
  if (build1d_static(d, r)) return 0;
  Blob1D q;
  layout_blob1d(r, nullptr, q);
  return q.bytes;
}

extern "C" int ecgmm_resnet1d_infer_prepare(const ecgmm_resnet1d_desc* d, const void* const* params,
                                            const void* const* buffers, void* blob, size_t blob_bytes, void* stream_) {
  I1D r;
  ECG_TRY(build1d_static(d, r));
  ECG_TRY(check_tables(params, ECGMM_RESNET1D_NPARAMS, buffers, ECGMM_RESNET1D_NBUFFERS, "resnet1d infer prepare"));
  Blob1D q;
  layout_blob1d(r, blob, q);
  if (!blob || blob_bytes < q.bytes) ECG_FAIL(ECGMM_ERR_WORKSPACE, "resnet1d infer prepare: blob %zu < %zu", blob_bytes, q.bytes);
  EcgFoldItem items[ECG_FOLD_MAX];
  int n = 0;
  items[n++] = conv_item(ECG_FOLD_STEM, params, 0, P(params, 1), 2, buffers, 0, q.wstem, q.bstem, 64, r.d.cin, 1);
  for (int i = 0; i < 3; ++i) {
    const Blk1& k = r.blk[i];
    const Blob1D::B& b = q.b[i];
    const int p = k.p0, bb = k.b0;
    items[n++] = conv_item(ECG_FOLD_CONV, params, p, P(params, p + 1), p + 2, buffers, bb, b.w1, b.b1, k.cout, k.cin, 3);
    items[n++] = conv_item(ECG_FOLD_CONV, params, p + 4, P(params, p + 5), p + 6, buffers, bb + 3, b.w2, b.b2, k.cout, k.cout, 3);
    items[n++] = copy_item(P(params, p + 8), b.sw1, k.cr, k.cout);
    items[n++] = copy_item(P(params, p + 9), b.sb1, k.cr, 1);
    items[n++] = copy_item(P(params, p + 10), b.sw2, k.cout, k.cr);
    items[n++] = copy_item(P(params, p + 11), b.sb2, k.cout, 1);
    if (k.down)
      items[n++] = conv_item(ECG_FOLD_CONV, params, p + 12, P(params, p + 13), p + 14, buffers, bb + 6, b.wd, b.bd, k.cout, k.cin, 1);
  }
  const int pc = r.p_cls;
  items[n++] = copy_item(P(params, pc), q.cw1, 64, 256);
  items[n++] = copy_item(P(params, pc + 1), q.cb1, 64, 1);
  items[n++] = copy_item(P(params, pc + 2), q.cw2, r.d.num_classes, 64);
  items[n++] = copy_item(P(params, pc + 3), q.cb2, r.d.num_classes, 1);
  return ecg_fold_batch(r.d.dtype, items, n, r.d.bn_eps, (hipStream_t)stream_);
}

extern "C" size_t ecgmm_resnet1d_infer_workspace(const ecgmm_resnet1d_desc* d) {
  I1D r;
  if (build1d(d, r)) return 0;
  Ws1D w;
  layout_ws1d(r, nullptr, w);
  return w.bytes;
}

extern "C" int ecgmm_resnet1d_infer(const ecgmm_resnet1d_desc* d, const float* signal, const void* blob, size_t blob_bytes,
                                    float* feat_out, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t s = (hipStream_t)stream_;
  I1D r;
  ECG_TRY(build1d(d, r));
  if (!signal || !feat_out) ECG_FAIL(ECGMM_ERR_SHAPE, "resnet1d infer: null signal / output");
  Blob1D q;
  layout_blob1d(r, const_cast<void*>(blob), q);
  if (!blob || blob_bytes < q.bytes) ECG_FAIL(ECGMM_ERR_WORKSPACE, "resnet1d infer: blob %zu < %zu", blob_bytes, q.bytes);
  Ws1D w;
  layout_ws1d(r, ws, w);
  if (!ws || ws_bytes < w.bytes) ECG_FAIL(ECGMM_ERR_WORKSPACE, "resnet1d infer: workspace %zu < %zu", ws_bytes, w.bytes);
  const int dt = r.d.dtype, N = r.d.N, cin = r.d.cin;

  if (dt == ECGMM_BF16) ECG_TRY(ecg_stem_fwd_wgrows(dt, signal, q.wstem, q.bstem, w.y0, nullptr, N, cin, 1, r.d.L, 1, s));
  else ECG_TRY(ecg_stem_fwd(dt, signal, q.wstem, q.bstem, w.y0, nullptr, N, cin, 1, r.d.L, 1, s));
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
    const ConvGeom g1 = make_geom(N, 1, k.lin, k.cin, k.cout, 1, 3, k.stride, 0, 1);
    const ConvGeom g2 = make_geom(N, 1, k.lout, k.cout, k.cout, 1, 3, 1, 0, 1);
    ECG_TRY(ecg_conv_igemm(dt, 0, g1, cur, b.w1, a1, b.b1, nullptr, nullptr, 1, s));
    ECG_TRY(ecg_conv_igemm(dt, 0, g2, a1, b.w2, y2, b.b2, nullptr, nullptr, 0, s));
    // squeeze-excite gate from mean_L(y2): y2 already IS bn2(conv2(a1))
    ECG_TRY(ecg_avgpool(dt, y2, w.m, N, k.lout, k.cout, nullptr, s));
    if (ecg_se_mlp_fused_ok(k.cout, k.cr)) {
      ECG_TRY(ecg_se_mlp_fwd(w.m, b.sw1, b.sb1, b.sw2, b.sb2, w.h, w.g, N, k.cout, k.cr, s));
    } else {
      ECG_TRY(ecg_linear_fwd(w.m, b.sw1, b.sb1, w.h, N, k.cout, k.cr, ECGMM_ACT_RELU, nullptr, s));
      ECG_TRY(ecg_linear_fwd(w.h, b.sw2, b.sb2, w.g, N, k.cr, k.cout, ECGMM_ACT_SIGMOID, nullptr, s));
    }
    if (k.down) {
      const ConvGeom gd = make_geom(N, 1, k.lin, k.cin, k.cout, 1, 1, k.stride, 0, 0);
      ECG_TRY(ecg_conv_igemm(dt, 0, gd, cur, b.wd, yd, b.bd, nullptr, nullptr, 0, s));
    }
    ECG_TRY(ecg_gate_res_relu(dt, y2, w.g, k.down ? yd : cur, y2, M, k.cout, k.lout, s));
    rot.advance(y2);
  }
  ECG_TRY(ecg_avgpool(dt, rot.buf[rot.cur], w.pooled, N, r.blk[2].lout, 256, nullptr, s));
  ECG_TRY(ecg_linear_fwd(w.pooled, q.cw1, q.cb1, w.h1, N, 256, 64, ECGMM_ACT_RELU, nullptr, s));
  return ecg_linear_fwd(w.h1, q.cw2, q.cb2, feat_out, N, 64, r.d.num_classes, 0, nullptr, s);
}
