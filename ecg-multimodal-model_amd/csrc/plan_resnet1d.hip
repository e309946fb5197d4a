// ResNet1D_SE signal encoder as a native launch plan (forward + backward), gfx950.
// Mirrors multimodal_paper_modal_balance.py:49-125 (== signal_model.py:12-88):
//   Conv1d(cin,64,7,2,3)+BN+ReLU+MaxPool1d(3,2,1) -> 3 x BasicBlock1D(conv3+BN+ReLU, conv3+BN, SE,
//   +identity / conv1 s2 + BN, ReLU) -> global avgpool -> Linear(256,64)+ReLU+Dropout -> Linear(64,n)
// Conv1d layers keep their bias in front of BN, as the reference does.  Activations are [N, L, C]
// channels-last in the compute dtype; the signal enters as [N, cin, L] fp32.
//
// The network description (block table, parameter / buffer table order and the named T1_* offsets, geometry): net_desc.h.
#include "plan_common.h"
#include "side_stream.h"

namespace {

int build(const ecgmm_resnet1d_desc* d, Net1D& r) {
  ECG_TRY(net1d_static(d, r, "resnet1d"));
  return net1d_shape(r, "resnet1d");
}

struct Fwd1 {
  void* wstem; void* y0; float* coef0; void* p0; unsigned char* idx0;
  BlockWs b[3];
  float *pooled, *h1, *hd;
  unsigned char* dmask;
  float* stats;
  size_t bytes;
};

// (views: a WsTable the named takes are recorded in, see ws_view_find)
void layout_fwd(const Net1D& r, void* base, Fwd1& w, WsTable* views = nullptr) {
  Arena a(base, views);
  const size_t es = dtype_size(r.d.dtype);
  const int N = r.d.N;
  w.wstem = a.take_bytes(ecg_stem_packed_elems(r.d.cin, 1) * es, "wstem");
  w.y0 = a.take_bytes((size_t)N * r.L1 * 64 * es, "y0");
  w.coef0 = a.take<float>(4 * 64, "coef0");
  w.p0 = a.take_bytes((size_t)N * r.L2 * 64 * es, "p0");
  w.idx0 = a.take<unsigned char>((size_t)N * r.L2 * 64, "idx0");
  size_t max_rows_c = (size_t)ecg_stem_stats_rows(N, r.d.cin, 1, r.d.L, 1) * 2 * 64;
  max_rows_c += (size_t)ECG_TAIL_ROWS * 2 * 64;
  for (int i = 0; i < 3; ++i) {
    const Blk1& k = r.blk[i];
    a.index = i;
    layout_block(a, w.b[i], N, (size_t)k.lout, k.cin, k.cout, 3, k.down, es, false, k.cr);
    size_t rows_c = (size_t)(ecg_conv_stats_rows((long)N * k.lout) + ECG_TAIL_ROWS) * 2 * k.cout;
    if (rows_c > max_rows_c) max_rows_c = rows_c;
  }
  a.index = 0;
  w.pooled = a.take<float>((size_t)N * 256, "pooled");
  w.h1 = a.take<float>((size_t)N * 64, "h1");
  w.hd = a.take<float>((size_t)N * 64, "hd");
  w.dmask = a.take<unsigned char>((size_t)N * 64, "dmask");
  w.stats = a.take<float>(max_rows_c);
  w.bytes = align_up(a.off, 256);
}

struct Bwd1 {
  void* X[2]; void *dz, *dy, *dy1, *dyd, *da, *dtmp, *big0, *big1;
  float *dpooled, *dh1, *dfeat_h, *dg, *ds, *dh, *dm, *dbias_scratch;
  float *sa1, *sa2, *sa3, *se_rows;   // per-sample sums of the merged SE / BatchNorm backward pass, and its reduction row
  float* bn_scratch;
  void* wg_ws; size_t wg_bytes;
  void* stem_ws; size_t stem_bytes;
  void* lin_ws; size_t lin_bytes;
  size_t bytes;
};

void layout_bwd(const Net1D& r, void* base, Bwd1& w, WsTable* views = nullptr) {
  Arena a(base, views);
  const size_t es = dtype_size(r.d.dtype);
  const int N = r.d.N;
  for (a.index = 0; a.index < 2; ++a.index) w.X[a.index] = a.take_bytes(r.max_act * es, "X");
  a.index = 0;
  w.dz = a.take_bytes(r.max_act * es, "dz");
  w.dy = a.take_bytes(r.max_act * es, "dy");
  w.dy1 = a.take_bytes(r.max_act * es, "dy1");  // own buffers for the three wgrad operands: the side stream still reads one
  w.dyd = a.take_bytes(r.max_act * es, "dyd");  // while the main stream's BatchNorm backward writes the next
  w.da = a.take_bytes(r.max_act * es, "da");
  w.dtmp = a.take_bytes(r.max_act * es, "dtmp");
  size_t big = (size_t)N * r.L1 * 64;
  w.big0 = a.take_bytes(big * es, "big0");
  w.big1 = a.take_bytes(big * es, "big1");
  w.dpooled = a.take<float>((size_t)N * 256, "dpooled");
  w.dh1 = a.take<float>((size_t)N * 64, "dh1");
  w.dfeat_h = a.take<float>((size_t)N * 64, "dfeat_h");
  w.dg = a.take<float>((size_t)N * 256, "dg");
  w.ds = a.take<float>((size_t)N * 256, "ds");
  w.dh = a.take<float>((size_t)N * 16, "dh");
  w.dm = a.take<float>((size_t)N * 256, "dm");
  w.dbias_scratch = a.take<float>(256);
  w.sa1 = a.take<float>((size_t)N * 256, "sa1");   // (named: only the merged form writes these four, which is how a test
  w.sa2 = a.take<float>((size_t)N * 256, "sa2");   //  started with ECGMM_SE_MERGE=0 sees that the two-pass form ran)
  w.sa3 = a.take<float>((size_t)N * 256, "sa3");
  w.se_rows = a.take<float>((size_t)ecg_se_bn_nrows() * 2 * 256, "se_rows");
  size_t bn = ecg_bn_bwd_scratch(r.d.dtype, (long)N * r.L1, 64);
  size_t wg = 0;
  size_t lin = ecg_linear_bwd_scratch(N, 256, 64);
  size_t l2 = ecg_linear_bwd_scratch(N, 64, r.d.num_classes);
  if (l2 > lin) lin = l2;
  for (int i = 0; i < 3; ++i) {
    const Blk1& k = r.blk[i];
    size_t s = ecg_bn_bwd_scratch(r.d.dtype, (long)N * k.lout, k.cout);
    if (s > bn) bn = s;
    size_t g1 = ecg_conv_wgrad_workspace(r.d.dtype, k.conv1_geom(N));
    size_t g2 = ecg_conv_wgrad_workspace(r.d.dtype, k.conv2_geom(N));
    if (g1 > wg) wg = g1;
    if (g2 > wg) wg = g2;
    if (k.down) {
      size_t g3 = ecg_conv_wgrad_workspace(r.d.dtype, k.down_geom(N));
      if (g3 > wg) wg = g3;
    }
    size_t la = ecg_linear_bwd_scratch(N, k.cr, k.cout), lb = ecg_linear_bwd_scratch(N, k.cout, k.cr);
    if (la > lin) lin = la;
    if (lb > lin) lin = lb;
  }
  w.bn_scratch = (float*)a.take_bytes(bn);
  w.wg_ws = a.take_bytes(wg);
  w.wg_bytes = wg;
  w.stem_bytes = ecg_stem_wgrad_workspace(N, r.d.cin, 1, r.d.L, 1);
  w.stem_ws = a.take_bytes(w.stem_bytes);
  w.lin_ws = a.take_bytes(lin);
  w.lin_bytes = lin;
  w.bytes = align_up(a.off, 256);
}

// stage 0 up to the pooled features: d loss / d pooled [N][256] (+ the classifier's parameter gradients)
int classifier_bwd(const Net1D& r, const Fwd1& w, const Bwd1& q, const float* dfeat, const void* const* params,
                   void* const* grads, hipStream_t s) {
  const int pc = r.p_cls, N = r.d.N;
  const bool drop = r.d.training && r.d.dropout_p > 0.f;   // (as the forward: no dropout in eval mode)
  ECG_TRY(ecg_linear_bwd(dfeat, drop ? w.hd : w.h1, P(params, pc + T1_CLS_W2), q.dfeat_h, G(grads, pc + T1_CLS_W2),
                         G(grads, pc + T1_CLS_B2), N, 64, r.d.num_classes, q.lin_ws, q.lin_bytes, s));
  if (drop) ECG_TRY(ecg_dropout_bwd(q.dfeat_h, w.dmask, q.dfeat_h, (long)N * 64, r.d.dropout_p, s));
  ECG_TRY(ecg_act_bwd(q.dfeat_h, w.h1, q.dh1, (long)N * 64, ECGMM_ACT_RELU, s));
  return ecg_linear_bwd(q.dh1, w.pooled, P(params, pc + T1_CLS_W1), q.dpooled, G(grads, pc + T1_CLS_W1),
                        G(grads, pc + T1_CLS_B1), N, 256, 64, q.lin_ws, q.lin_bytes, s);
}

}  // namespace

// weight-gradient side stream of this plan (side_stream.h); its own instance, see there
static SideStream g_side1;
int ecg_resnet1d_side_enable(int on) {
  ECG_TRY(g_side1.init());
  g_side1.enabled = on != 0;
  return 0;
}
// The ResNet1D_SE plan's own switch.  Beside the image encoder (multimodal model: the signal encoder already runs on a
// side stream of the host's) its weight gradients stay on the encoder's stream: HIP maps streams onto four hardware
// queues, and a fifth busy stream -- with data parallelism the process group's stream is one more -- shares a queue with
// another, whose event waits then serialise both (same-call A/B: 7.15 -> 7.09 ms/step, and the one-rank rehearsal of the
// data-parallel path 7.52 -> 7.17).  Alone (12-lead configuration) the side stream is worth 3 %.
// (a hint ANDed with the global switch ecgmm_side_wgrad / ECGMM_SIDE_WGRAD, so profiling runs that turn every side
// stream off stay serialized)
static bool g_side1_alone = true;
extern "C" int ecgmm_resnet1d_side_wgrad(int on) {
  g_side1_alone = on != 0;
  return 0;
}

extern "C" size_t ecgmm_resnet1d_fwd_workspace(const ecgmm_resnet1d_desc* d) {
  Net1D r;
  if (build(d, r)) return 0;
  Fwd1 w;
  layout_fwd(r, nullptr, w);
  return w.bytes;
}
extern "C" size_t ecgmm_resnet1d_bwd_workspace(const ecgmm_resnet1d_desc* d) {
  Net1D r;
  if (build(d, r)) return 0;
  Bwd1 w;
  layout_bwd(r, nullptr, w);
  return w.bytes;
}

// Offset and size of a named tensor of the forward (backward = 0) or backward workspace (see ecgmm_resnet18_ws_view).
// index: the block (0..2) for per-block tensors, 0 / 1 for X, else 0.
extern "C" int ecgmm_resnet1d_ws_view(const ecgmm_resnet1d_desc* d, int backward, const char* name, int index,
                                      size_t* offset, size_t* bytes) {
  Net1D r;
  ECG_TRY(build(d, r));
  if (!name || !offset || !bytes) ECG_FAIL(ECGMM_ERR_SHAPE, "resnet1d ws_view: null argument");
  WsTable t;
  Fwd1 w;
  Bwd1 q;
  if (backward) layout_bwd(r, nullptr, q, &t);
  else layout_fwd(r, nullptr, w, &t);
  return ws_view_find(backward ? "resnet1d ws_view (backward)" : "resnet1d ws_view (forward)", t, name, index,
                      backward ? q.bytes : w.bytes, offset, bytes);
}

extern "C" int ecgmm_resnet1d_forward(const ecgmm_resnet1d_desc* d, const float* signal, const void* const* params,
                                      void* const* buffers, float* feat_out, void* ws, size_t ws_bytes,
                                      void* stream_) {
  hipStream_t s = (hipStream_t)stream_;
  Net1D r;
  ECG_TRY(build(d, r));
  Fwd1 w;
  layout_fwd(r, ws, w);
  ECG_NEED(ws, ws_bytes, w.bytes, "resnet1d fwd: workspace");
  const int dt = r.d.dtype, N = r.d.N, cin = r.d.cin;
  float* st = r.d.training ? w.stats : nullptr;

  {  // every conv weight -> compute-dtype operand layouts, one launch
    EcgPackItem items[ECG_PACK_MAX];
    int n = 0;
    for (int i = 0; i < 3; ++i) {
      const Blk1& k = r.blk[i];
      BlockWs& b = w.b[i];
      items[n++] = {P(params, k.p0 + T1_CONV1_W), b.w1f, b.w1d, k.cout, k.cin, 3};
      items[n++] = {P(params, k.p0 + T1_CONV2_W), b.w2f, b.w2d, k.cout, k.cout, 3};
      if (k.down) items[n++] = {P(params, k.p0 + T1_DOWN_W), b.wdf, b.wdd, k.cout, k.cin, 1};
    }
    ECG_TRY(ecg_pack_weight_batch(dt, items, n, s));
  }
  ECG_TRY(ecg_stem_pack(dt, P(params, 0), w.wstem, cin, 1, s));
  ECG_TRY(stem_forward(dt, signal, w.wstem, P(params, 1), w.y0, st, N, cin, 1, r.d.L, 1, s));
  ECG_TRY(bn_coef(r.bn, w.stats, stem_forward_rows(dt, N, cin, 1, r.d.L, 1), 64, (long)N * r.L1, params, 2, buffers, 0,
                  w.coef0, s));
  ECG_TRY(ecg_bnrelu_maxpool(dt, w.y0, w.coef0, w.p0, w.idx0, N, 1, r.L1, 64, s));

  const void* cur = w.p0;
  for (int i = 0; i < 3; ++i) {
    const Blk1& k = r.blk[i];
    BlockWs& b = w.b[i];
    const int p = k.p0, bb = k.b0;
    const long M = (long)N * k.lout;
    const int rows = ecg_conv_stats_rows(M);
    ConvGeom g1 = k.conv1_geom(N);
    ConvGeom g2 = k.conv2_geom(N);
    ECG_TRY(ecg_conv_igemm(dt, 0, g1, cur, b.w1f, b.y1, P(params, p + T1_CONV1_B), nullptr, st, 0, s));
    ECG_TRY(bn_coef(r.bn, w.stats, rows, k.cout, M, params, p + T1_BN1, buffers, bb + T1B_BN1, b.coef1, s));
    ECG_TRY(ecg_bn_act(dt, b.y1, b.coef1, nullptr, nullptr, nullptr, 1, 1, b.a1, M, k.cout, s));
    ECG_TRY(ecg_conv_igemm(dt, 0, g2, b.a1, b.w2f, b.y2, P(params, p + T1_CONV2_B), nullptr, st, 0, s));
    ECG_TRY(bn_coef(r.bn, w.stats, rows, k.cout, M, params, p + T1_BN2, buffers, bb + T1B_BN2, b.coef2, s));
    // squeeze-excite gate from mean_L(bn2(y2))
    ECG_TRY(ecg_avgpool(dt, b.y2, b.m, N, k.lout, k.cout, b.coef2, s));
    ECG_TRY(se_mlp_forward(b.m, P(params, p + T1_SE_W1), P(params, p + T1_SE_B1), P(params, p + T1_SE_W2),
                           P(params, p + T1_SE_B2), b.h, b.g, N, k.cout, k.cr, s));
    if (k.down) {
      ConvGeom gd = k.down_geom(N);
      ECG_TRY(ecg_conv_igemm(dt, 0, gd, cur, b.wdf, b.yd, P(params, p + T1_DOWN_B), nullptr, st, 0, s));
      ECG_TRY(bn_coef(r.bn, w.stats, rows, k.cout, M, params, p + T1_DBN, buffers, bb + T1B_DBN, b.coefd, s));
      ECG_TRY(ecg_bn_act(dt, b.y2, b.coef2, b.yd, b.coefd, b.g, k.lout, 1, b.out, M, k.cout, s));
    } else {
      ECG_TRY(ecg_bn_act(dt, b.y2, b.coef2, cur, nullptr, b.g, k.lout, 1, b.out, M, k.cout, s));
    }
    cur = b.out;
  }
  const int pc = r.p_cls;
  ECG_TRY(ecg_avgpool(dt, cur, w.pooled, N, r.blk[2].lout, 256, nullptr, s));
  ECG_TRY(ecg_linear_fwd(w.pooled, P(params, pc + T1_CLS_W1), P(params, pc + T1_CLS_B1), w.h1, N, 256, 64, ECGMM_ACT_RELU,
                         nullptr, s));
  const float* hin = w.h1;
  if (r.d.training && r.d.dropout_p > 0.f) {
    ECG_TRY(ecg_dropout_fwd(w.h1, w.hd, w.dmask, (long)N * 64, r.d.dropout_p, r.d.seed, r.d.offset, s));
    hin = w.hd;
  }
  ECG_TRY(ecg_linear_fwd(hin, P(params, pc + T1_CLS_W2), P(params, pc + T1_CLS_B2), feat_out, N, 64, r.d.num_classes, 0,
                         nullptr, s));
  return 0;
}

// stages: 0 = classifier + avgpool, 1..3 = blocks 2..0, 4 = stem
// dsignal (nullable): the input gradient [N][cin][L] fp32, written by the last stage.  Behind an eval-mode forward every
// BatchNorm backward is the affine form (two-pass SE route); nothing in the forward workspace is written in either mode.
static int r1d_backward(const ecgmm_resnet1d_desc* d, const float* signal, const float* dfeat, const void* const* params,
                        void* const* grads, void* ws_fwd, void* ws_bwd, size_t ws_bwd_bytes, int stage_begin, int stage_end,
                        float* dsignal, hipStream_t s) {
  Net1D r;
  ECG_TRY(build(d, r));
  const bool train = r.d.training != 0;
  Fwd1 w;
  layout_fwd(r, ws_fwd, w);
  Bwd1 q;
  layout_bwd(r, ws_bwd, q);
  ECG_NEED(ws_fwd && ws_bwd, ws_bwd_bytes, q.bytes, "resnet1d bwd: workspace");
  const int dt = r.d.dtype, N = r.d.N, cin = r.d.cin;
  ECG_TRY(g_side1.init());
  const bool side = g_side1.enabled && g_side1_alone;
  // weight gradients of this call run beside the dgrad chain: narrow launches (conv_wgrad.hip, pick_nsplit)
  ecg_conv_wgrad_narrow(side);
  struct NarrowOff { ~NarrowOff() { ecg_conv_wgrad_narrow(false); } } narrow_off;
  hipStream_t wst = side ? g_side1.s : s;  // stream of the weight-gradient kernels

  for (int st = stage_begin; st < stage_end; ++st) {
    if (st == 0) {
      g_side1.doneA = g_side1.doneB = g_side1.doneC = nullptr;
      ECG_TRY(classifier_bwd(r, w, q, dfeat, params, grads, s));
      const int R = r.blk[2].lout;
      ECG_TRY(ecg_bcast_rows(dt, q.dpooled, q.X[0], N, R, 256, 1.f / (float)R, s));
    } else if (st <= 3) {
      const int i = 3 - st;
      const Blk1& k = r.blk[i];
      BlockWs& b = w.b[i];
      const int p = k.p0;
      const void* in = i == 0 ? w.p0 : w.b[i - 1].out;
      const void* dcur = q.X[(st - 1) & 1];
      void* din = q.X[st & 1];
      const long M = (long)N * k.lout;
      ConvGeom g1 = k.conv1_geom(N);
      ConvGeom g2 = k.conv2_geom(N);
      // out = relu(bn2(y2) * g + identity); gate gradient first.  Merged form (default): this pass also stores the masked
      // gradient dz and the per-sample sums the BatchNorm-backward reduction needs, so bn2's backward below is finalize +
      // apply only -- one read of (dcur, out, y2) less per block.  ECGMM_SE_MERGE=0: the two-pass form.
      const bool se_merge = sw::SE_MERGE.get() && train;   // (the merged pass feeds the training form's reduction)
      if (se_merge) {
        ECG_TRY(ecg_se_gate_bn(dt, dcur, b.out, b.y2, b.coef2, q.dz, q.dg, q.sa1, q.sa2, q.sa3, N, k.lout, k.cout, s));
      } else {
        ECG_TRY(ecg_se_gate_grad(dt, dcur, b.out, b.y2, b.coef2, q.dg, N, k.lout, k.cout, s));
      }
      if (ecg_se_mlp_fused_ok(k.cout, k.cr)) {   // the SE MLP's backward in two launches (head_fused.hip)
        ECG_TRY(ecg_se_mlp_bwd(q.dg, b.g, b.h, b.m, P(params, p + T1_SE_W1), P(params, p + T1_SE_W2), q.ds, q.dh, q.dm,
                               G(grads, p + T1_SE_W1), G(grads, p + T1_SE_B1), G(grads, p + T1_SE_W2), G(grads, p + T1_SE_B2),
                               N, k.cout, k.cr, 1.f / (float)k.lout, s));
      } else {
        ECG_TRY(ecg_act_bwd(q.dg, b.g, q.ds, (long)N * k.cout, ECGMM_ACT_SIGMOID, s));
        ECG_TRY(ecg_linear_bwd(q.ds, b.h, P(params, p + T1_SE_W2), q.dh, G(grads, p + T1_SE_W2), G(grads, p + T1_SE_B2), N,
                               k.cr, k.cout, q.lin_ws, q.lin_bytes, s));
        ECG_TRY(ecg_act_bwd(q.dh, b.h, q.dh, (long)N * k.cr, ECGMM_ACT_RELU, s));
        ECG_TRY(ecg_linear_bwd(q.dh, b.m, P(params, p + T1_SE_W1), q.dm, G(grads, p + T1_SE_W1), G(grads, p + T1_SE_B1), N,
                               k.cout, k.cr, q.lin_ws, q.lin_bytes, s));
        ECG_TRY(ecg_axpby(1.f / (float)k.lout, q.dm, 0.f, q.dm, (long)N * k.cout, s));
      }
      main_wait(s, g_side1.doneA);  // the previous block's wgrad2 has finished reading q.dy
      if (se_merge) {
        ECG_TRY(ecg_se_bn_rows(q.sa1, q.sa2, q.sa3, b.g, q.dm, N, k.lout, k.cout, q.se_rows, s));
        ECG_TRY(ecg_bn_bwd_tail(dt, q.dz, nullptr, b.y2, b.coef2, P(params, p + T1_BN2), G(grads, p + T1_BN2),
                                G(grads, p + T1_BN2 + 1), q.dy, q.se_rows, ecg_se_bn_nrows(), M, k.cout, q.bn_scratch, s, b.g,
                                q.dm, k.lout, G(grads, p + T1_CONV2_B)));
      } else {
        ECG_TRY(bn_bwd_mode(r.bn, dcur, b.out, b.g, q.dm, k.lout, b.y2, b.coef2, P(params, p + T1_BN2), G(grads, p + T1_BN2),
                            G(grads, p + T1_BN2 + 1), q.dy, q.dz, G(grads, p + T1_CONV2_B), M, k.cout, q.bn_scratch, s));
      }
      if (G(grads, p + T1_CONV2_W)) {
        if (side) g_side1.fork(s);
        ECG_TRY(ecg_conv_wgrad(dt, g2, b.a1, q.dy, G(grads, p + T1_CONV2_W), 0, q.wg_ws, q.wg_bytes, wst));
        if (side) g_side1.doneA = g_side1.mark();
      }
      ECG_TRY(ecg_conv_igemm(dt, 1, g2, q.dy, b.w2d, q.da, nullptr, nullptr, nullptr, 0, s));
      main_wait(s, g_side1.doneB);
      ECG_TRY(bn_bwd_mode(r.bn, q.da, b.y1 /* mask recomputed from y1 */, nullptr, nullptr, 1, b.y1, b.coef1,
                          P(params, p + T1_BN1), G(grads, p + T1_BN1), G(grads, p + T1_BN1 + 1), q.dy1, nullptr,
                          G(grads, p + T1_CONV1_B), M, k.cout, q.bn_scratch, s));
      if (G(grads, p + T1_CONV1_W)) {
        if (side) g_side1.fork(s);
        ECG_TRY(ecg_conv_wgrad(dt, g1, in, q.dy1, G(grads, p + T1_CONV1_W), 0, q.wg_ws, q.wg_bytes, wst));
        if (side) g_side1.doneB = g_side1.mark();
      }
      if (k.down) {
        ConvGeom gd = k.down_geom(N);
        main_wait(s, g_side1.doneC);
        ECG_TRY(bn_bwd_mode(r.bn, q.dz, nullptr, nullptr, nullptr, 1, b.yd, b.coefd, P(params, p + T1_DBN),
                            G(grads, p + T1_DBN), G(grads, p + T1_DBN + 1), q.dyd, nullptr, G(grads, p + T1_DOWN_B), M, k.cout,
                            q.bn_scratch, s));
        if (G(grads, p + T1_DOWN_W)) {
          if (side) g_side1.fork(s);
          ECG_TRY(ecg_conv_wgrad(dt, gd, in, q.dyd, G(grads, p + T1_DOWN_W), 0, q.wg_ws, q.wg_bytes, wst));
          if (side) g_side1.doneC = g_side1.mark();
        }
        ConvEpi ed = {};   // downsample branch folded into the stride-2 dgrad (see plan_resnet18.hip)
        if (sw::DOWN_FOLD.get()) { ed.src2 = q.dyd; ed.wpk2 = b.wdd; }
        if (ed.src2) ECG_TRY(ecg_conv_igemm(dt, 1, g1, q.dy1, b.w1d, din, nullptr, nullptr, nullptr, 0, s, &ed));
        if (!ed.src2_done) {
          ECG_TRY(ecg_conv_igemm(dt, 1, gd, q.dyd, b.wdd, q.dtmp, nullptr, nullptr, nullptr, 0, s));
          ECG_TRY(ecg_conv_igemm(dt, 1, g1, q.dy1, b.w1d, din, nullptr, q.dtmp, nullptr, 0, s));
        }
      } else {
        ECG_TRY(ecg_conv_igemm(dt, 1, g1, q.dy1, b.w1d, din, nullptr, q.dz, nullptr, 0, s));
      }
    } else if (st == 4) {
      const void* dp0 = q.X[3 & 1];
      if (train && ecg_stem_fuse_on()) {
        ECG_TRY(ecg_pool_bn_bwd(dt, dp0, w.p0, w.idx0, w.y0, w.coef0, P(params, 2), G(grads, 2), G(grads, 3), q.big1,
                                G(grads, 1), N, 1, r.L1, 64, q.bn_scratch, s));
      } else {
        ECG_TRY(ecg_maxpool_relu_bwd(dt, dp0, w.p0, w.idx0, q.big0, N, 1, r.L1, 64, s));
        ECG_TRY(bn_bwd_mode(r.bn, q.big0, nullptr, nullptr, nullptr, 1, w.y0, w.coef0, P(params, 2), G(grads, 2), G(grads, 3),
                            q.big1, nullptr, G(grads, 1), (long)N * r.L1, 64, q.bn_scratch, s));
      }
      if (G(grads, 0))  // last kernel: stays on the caller's stream (own slab buffer), see plan_resnet18.hip
        ECG_TRY(ecg_stem_wgrad(dt, signal, q.big1, G(grads, 0), 0, q.stem_ws, q.stem_bytes, N, cin, 1, r.d.L, 1, s));
      // the input gradient: the transposed stem convolution of the same dy0 (conv_stem_dgrad.hip)
      if (dsignal) ECG_TRY(ecg_stem_dgrad(dt, q.big1, P(params, 0), dsignal, N, cin, 1, r.d.L, 1, s));
    } else {
      ECG_FAIL(ECGMM_ERR_SHAPE, "resnet1d bwd: stage %d out of range", st);
    }
  }
  if (side) ECG_TRY(g_side1.wait_on(s));  // join: everything the side stream did is ordered before the caller's next work
  return 0;
}

extern "C" int ecgmm_resnet1d_backward(const ecgmm_resnet1d_desc* d, const float* signal, const float* dfeat,
                                       const void* const* params, void* const* grads, void* ws_fwd, void* ws_bwd,
                                       size_t ws_bwd_bytes, int stage_begin, int stage_end, void* stream_) {
  return r1d_backward(d, signal, dfeat, params, grads, ws_fwd, ws_bwd, ws_bwd_bytes, stage_begin, stage_end, nullptr,
                      (hipStream_t)stream_);
}

// The same backward with the input gradient as one more output of the last stage (dsignal may be null).
extern "C" int ecgmm_resnet1d_backward_dx(const ecgmm_resnet1d_desc* d, const float* signal, const float* dfeat,
                                          const void* const* params, void* const* grads, void* ws_fwd, void* ws_bwd,
                                          size_t ws_bwd_bytes, int stage_begin, int stage_end, float* dsignal,
                                          void* stream_) {
  return r1d_backward(d, signal, dfeat, params, grads, ws_fwd, ws_bwd, ws_bwd_bytes, stage_begin, stage_end, dsignal,
                      (hipStream_t)stream_);
}

// Grad-CAM of the last block's output for the logits whose gradient w.r.t. the encoder output is dfeat [N][num_classes]
// (see ecgmm_resnet18_gradcam).  cam: [N][L] fp32 in [0, 1].
extern "C" int ecgmm_resnet1d_gradcam(const ecgmm_resnet1d_desc* d, const float* dfeat, const void* const* params,
                                      void* ws_fwd, void* ws_bwd, size_t ws_bwd_bytes, float* cam, void* stream_) {
  hipStream_t s = (hipStream_t)stream_;
  Net1D r;
  ECG_TRY(build(d, r));
  Fwd1 w;
  layout_fwd(r, ws_fwd, w);
  Bwd1 q;
  layout_bwd(r, ws_bwd, q);
  ECG_NEED(ws_fwd && ws_bwd, ws_bwd_bytes, q.bytes, "resnet1d gradcam: workspace");
  if (!dfeat || !cam) ECG_FAIL(ECGMM_ERR_SHAPE, "resnet1d gradcam: null operand");
  ECG_TRY(classifier_bwd(r, w, q, dfeat, params, nullptr, s));
  // (q.X[0] holds max_act elements >= N x lout x 256: room for the N x lout fp32 map)
  return ecg_gradcam(r.d.dtype, w.b[2].out, q.dpooled, (float*)q.X[0], cam, r.d.N, 1, r.blk[2].lout, 256, 1, r.d.L, s);
}
