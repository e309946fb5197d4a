// ResNet18 image encoder as a native launch plan (forward + backward), gfx950.
// Mirrors torchvision.models.resnet18() as instantiated by the reference at
// multimodal_paper_modal_balance.py:210,221 and train_image_only.py:92-99:
//   conv7x7/2 -> BN -> ReLU -> maxpool3/2 -> 4 stages x 2 BasicBlocks -> global avgpool -> fc
// Activations live channels-last in the compute dtype inside a caller-owned workspace; the image
// enters as NCHW fp32 exactly as the reference's DataLoader hands it over.
//
// The network description (block table, parameter / buffer table order, geometry): net_desc.h.
#include "plan_common.h"
#include "side_stream.h"

namespace {
// The 2-D stem by recompute (conv_stem_fused.hip), ECGMM_STEM_RECOMPUTE / ecgmm_stem_recompute.  DEFAULT OFF: measured in the step
// (same-call A/B, batch 256, round 3) it removes 1.6 GB of fabric traffic per step and is 0.2 ms SLOWER (7.12 -> 7.32 ms):
// its kernels are VALU-issue-bound (~2600 instructions per 128-pixel tile for 96 MFMAs), not byte-bound -- stand-alone
// forward 418 -> 396 us, backward 401 -> 584 us.  Kept as a tested option (memory: -1.2 GB of workspace at batch 256).
bool stem_recompute(int dtype) {
  return sw::STEM_RECOMPUTE.get() && ecg_stem_fused_ok(dtype, 3, 7);
}
// bn2's backward takes the block's ReLU mask from one bit per element written by the forward activation pass instead of re-reading
// the activated tensor (ECGMM_RELU_BITS=0: re-read it).  Read once per process: forward and backward must agree.
bool relu_bits_on() { return sw::RELU_BITS.get() != 0; }

int build(const ecgmm_resnet18_desc* d, Net18& r) {
  ECG_TRY(net18_static(d, r, "resnet18"));
  return net18_shape(r, "resnet18");
}

// saved-for-backward workspace
struct FwdWs {
  void* wstem;
  void* y0; float* coef0; void* p0; unsigned char* idx0;
  BlockWs b[8];
  float* pooled;
  float* stats;  // transient partial-sum rows (largest layer)
  float* stats_d;  // the same for the downsample convolutions (they run on the side stream beside conv1 / conv2)
  size_t bytes;
};

// (views: a WsTable the named takes are recorded in, see ws_view_find)
void layout_fwd(const Net18& r, void* base, FwdWs& w, WsTable* views = nullptr) {
  Arena a(base, views);
  const size_t es = dtype_size(r.d.dtype);
  const int N = r.d.N;
  w.wstem = a.take_bytes(ecg_stem_packed_elems(3, 7) * es, "wstem");
  // (the recomputing stem never materialises the conv output)
  w.y0 = stem_recompute(r.d.dtype) ? nullptr : a.take_bytes((size_t)N * r.H1 * r.W1 * 64 * es, "y0");
  w.coef0 = a.take<float>(4 * 64, "coef0");
  w.p0 = a.take_bytes((size_t)N * r.H2 * r.W2 * 64 * es, "p0");
  w.idx0 = a.take<unsigned char>((size_t)N * r.H2 * r.W2 * 64, "idx0");
  size_t max_rows_c = (size_t)(stem_recompute(r.d.dtype) ? ecg_stem_stats_only_rows(N, 3, r.d.H, r.d.W, 7)
                                                          : ecg_stem_stats_rows(N, 3, r.d.H, r.d.W, 7)) * 2 * 64;
  max_rows_c += (size_t)ECG_TAIL_ROWS * 2 * 64;
  size_t max_rows_d = 64;
  for (int i = 0; i < 8; ++i) {
    const Blk18& k = r.blk[i];
    a.index = i;
    // (ReLU mask of `out` as bits: bf16 plans)
    layout_block(a, w.b[i], N, (size_t)k.hout * k.wout, k.cin, k.cout, 9, k.down, es, es == 2, 0);
    size_t rows_c = (size_t)(ecg_conv_stats_rows((long)N * k.hout * k.wout) + ECG_TAIL_ROWS) * 2 * k.cout;
    if (rows_c > max_rows_c) max_rows_c = rows_c;
    if (k.down && rows_c > max_rows_d) max_rows_d = rows_c;
  }
  a.index = 0;
  w.pooled = a.take<float>((size_t)N * 512, "pooled");
  w.stats = a.take<float>(max_rows_c);
  w.stats_d = a.take<float>(max_rows_d);
  w.bytes = align_up(a.off, 256);
}

struct BwdWs {
  void* X[2];   // gradient w.r.t. block outputs (ping-pong)
  void* dz;     // masked residual-branch gradient
  // operands of the side-stream weight-gradient kernels, two of each (blocks alternate): the main stream's next
  // BatchNorm backward then never has to wait for the previous block's wgrad to finish reading, only for the one
  // two blocks back (an exposed cross-stream wait costs 35-140 us here, and the side stream does run behind)
  void* dy[2];   // gradient w.r.t. conv2's raw output
  void* dy1[2];  // gradient w.r.t. conv1's raw output
  void* dyd[2];  // gradient w.r.t. the downsample conv's raw output
  void* da;     // gradient w.r.t. a1
  void* dtmp;   // downsample-path input gradient
  void* big0;   // stem: dz0
  void* big1;   // stem: dy0
  float* dpooled;
  float* bn_scratch;
  float *red1, *red2;  // partial rows of BatchNorm-backward reductions fused into dgrad epilogues (ConvEpi): bn1 / bn2
  void* wg_ws; size_t wg_bytes;
  void* stem_ws; size_t stem_bytes;  // the stem's slab buffer (it runs on the caller's stream, concurrently with side-stream wgrads)
  void* lin_ws; size_t lin_bytes;
  size_t bytes;
};

constexpr size_t RED_ROWS_FLOATS = (size_t)512 * 2 * 512;   // red1, red2: up to 512 rows of [2][512 channels]

void layout_bwd(const Net18& r, void* base, BwdWs& w, WsTable* views = nullptr) {
  Arena a(base, views);
  const size_t es = dtype_size(r.d.dtype);
  const int N = r.d.N;
  for (a.index = 0; a.index < 2; ++a.index) w.X[a.index] = a.take_bytes(r.max_act * es, "X");
  a.index = 0;
  w.dz = a.take_bytes(r.max_act * es, "dz");
  for (a.index = 0; a.index < 2; ++a.index) {
    w.dy[a.index] = a.take_bytes(r.max_act * es, "dy");
    w.dy1[a.index] = a.take_bytes(r.max_act * es, "dy1");
    w.dyd[a.index] = a.take_bytes(r.max_act * es, "dyd");
  }
  a.index = 0;
  w.da = a.take_bytes(r.max_act * es, "da");
  w.dtmp = a.take_bytes(r.max_act * es, "dtmp");
  const bool recompute = stem_recompute(r.d.dtype);
  size_t big = recompute ? 0 : (size_t)N * r.H1 * r.W1 * 64;   // (recomputing stem: neither dz0 nor dy0 exist)
  w.big0 = a.take_bytes(big * es, "big0");
  w.big1 = a.take_bytes(big * es, "big1");
  w.dpooled = a.take<float>((size_t)N * 512, "dpooled");
  size_t bn = ecg_bn_bwd_scratch(r.d.dtype, (long)N * r.H1 * r.W1, 64);
  size_t wg = 0;
  for (int i = 0; i < 8; ++i) {
    const Blk18& k = r.blk[i];
    size_t s = ecg_bn_bwd_scratch(r.d.dtype, (long)N * k.hout * k.wout, k.cout);
    if (s > bn) bn = s;
    size_t g1 = ecg_conv_wgrad_workspace(r.d.dtype, k.conv1_geom(N));
    size_t g2 = ecg_conv_wgrad_workspace(r.d.dtype, k.conv2_geom(N));
    if (g1 > wg) wg = g1;
    if (g2 > wg) wg = g2;
    if (k.down) {
      size_t g3 = ecg_conv_wgrad_workspace(r.d.dtype, k.down_geom(N));
      if (g3 > wg) wg = g3;
    }
  }
  w.bn_scratch = (float*)a.take_bytes(bn);
  w.red1 = a.take<float>(RED_ROWS_FLOATS);
  w.red2 = a.take<float>(RED_ROWS_FLOATS);
  w.wg_ws = a.take_bytes(wg);
  w.wg_bytes = wg;
  w.stem_bytes = recompute ? ecg_stem_pool_bwd_workspace(N, 3, r.d.H, r.d.W) : ecg_stem_wgrad_workspace(N, 3, r.d.H, r.d.W, 7);
  w.stem_ws = a.take_bytes(w.stem_bytes);
  w.lin_bytes = ecg_linear_bwd_scratch(N, 512, r.d.out_dim);
  w.lin_ws = a.take_bytes(w.lin_bytes);
  w.bytes = align_up(a.off, 256);
}

// ---- side stream for the weight-gradient kernels (side_stream.h) ----------------------------------
SideStream g_side;
int side_init() { return g_side.init(); }
inline hipEvent_t side_next_ev() { return g_side.next_ev(); }
inline void side_fork(hipStream_t main) { g_side.fork(main); }
inline hipEvent_t side_mark() { return g_side.mark(); }

// BatchNorm (training statistics from a conv's partial rows, or running statistics in eval mode) + activation pass.
// Where the rows are few enough the finalize is folded into the activation pass itself (ecg_bn_act_fold: one dependent
// ~5 us launch less on the forward's critical path, 16 times per forward).
int bn_then_act(const Net18& r, const float* stats, int rows, int C, long count, const void* const* params, int p_bn,
                void* const* buffers, int b_bn, float* coef, const void* y, const void* res, const float* rcoef, void* out,
                hipStream_t s, unsigned char* relu_bits = nullptr) {
  const int dt = r.d.dtype;
  if (r.d.training && ecg_bn_fold_ok(C, rows)) {
    EcgBnFold f = {stats, rows, (double)count, P(params, p_bn), P(params, p_bn + 1), (float*)buffers[b_bn],
                   (float*)buffers[b_bn + 1], (long long*)buffers[b_bn + 2], r.d.bn_momentum, r.d.bn_eps};
    return ecg_bn_act_fold(dt, y, coef, f, res, rcoef, nullptr, 1, 1, out, count, C, s, relu_bits);
  }
  ECG_TRY(bn_coef(r.bn, stats, rows, C, count, params, p_bn, buffers, b_bn, coef, s));
  return ecg_bn_act(dt, y, coef, res, rcoef, nullptr, 1, 1, out, count, C, s, relu_bits);
}

// stage 0 up to the pooled features: d loss / d pooled [N][512] (+ the fc parameter gradients)
int fc_bwd(const Net18& r, const FwdWs& w, const BwdWs& q, const float* dfeat, const void* const* params, void* const* grads,
           hipStream_t s) {
  return ecg_linear_bwd(dfeat, w.pooled, P(params, r.p_fc), q.dpooled, G(grads, r.p_fc), G(grads, r.p_fc + 1), r.d.N, 512,
                        r.d.out_dim, q.lin_ws, q.lin_bytes, s);
}

}  // namespace

// Runtime switch for the side-stream weight-gradient overlap (default on; ECGMM_SIDE_WGRAD=0 disables it
// at start-up).  bench.py turns it off for its serialized kernel-timing pass.
extern "C" int ecgmm_side_wgrad(int on) {
  ECG_TRY(side_init());
  g_side.enabled = on != 0;
  return ecg_resnet1d_side_enable(on);
}

// Data-parallel overlap: with defer = 1 a backward call returns WITHOUT joining the side stream to the caller's
// stream (the dgrad chain of the next stage group then keeps overlapping this group's weight-gradient tail); the
// caller orders its consumer (the all-reduce stream) after the weight gradients with ecgmm_side_wait() and must
// run the last stage group with defer = 0, whose join covers everything.
extern "C" int ecgmm_side_defer_join(int defer) {
  ECG_TRY(side_init());
  g_side.defer_join = defer != 0;
  return 0;
}

// Everything the side stream has been given so far happens-before later work on `stream`.
extern "C" int ecgmm_side_wait(void* stream) {
  ECG_TRY(side_init());
  if (!g_side.enabled) return 0;
  return g_side.wait_on((hipStream_t)stream);
}

// The library's weight-gradient side stream (NULL when it is switched off), and "fork": everything enqueued on `stream`
// so far happens-before later work on the side stream.  A data-parallel host issues its early all-reduces from the side
// stream's context (after a fork) instead of from a stream of its own: a fifth busy HIP stream oversubscribes the four
// hardware queues (GPU_MAX_HW_QUEUES), and two streams that share a queue serialise each other's event waits.
extern "C" void* ecgmm_side_stream(void) {
  if (side_init() != 0 || !g_side.enabled) return nullptr;
  return (void*)g_side.s;
}
extern "C" int ecgmm_side_fork(void* stream) {
  ECG_TRY(side_init());
  if (g_side.enabled) g_side.fork((hipStream_t)stream);
  return 0;
}

extern "C" size_t ecgmm_resnet18_fwd_workspace(const ecgmm_resnet18_desc* d) {
  Net18 r;
  if (build(d, r)) return 0;
  FwdWs w;
  layout_fwd(r, nullptr, w);
  return w.bytes;
}

extern "C" size_t ecgmm_resnet18_bwd_workspace(const ecgmm_resnet18_desc* d) {
  Net18 r;
  if (build(d, r)) return 0;
  BwdWs w;
  layout_bwd(r, nullptr, w);
  return w.bytes;
}

// Offset and size of a named tensor of the forward (backward = 0) or backward workspace: a test and debugging aid that
// launches nothing.  index: the block (0..7) for per-block tensors, 0 / 1 for X, dy, dy1, dyd, else 0.
extern "C" int ecgmm_resnet18_ws_view(const ecgmm_resnet18_desc* d, int backward, const char* name, int index,
                                      size_t* offset, size_t* bytes) {
  Net18 r;
  ECG_TRY(build(d, r));
  if (!name || !offset || !bytes) ECG_FAIL(ECGMM_ERR_SHAPE, "resnet18 ws_view: null argument");
  WsTable t;
  FwdWs w;
  BwdWs q;
  if (backward) layout_bwd(r, nullptr, q, &t);
  else layout_fwd(r, nullptr, w, &t);
  return ws_view_find(backward ? "resnet18 ws_view (backward)" : "resnet18 ws_view (forward)", t, name, index,
                      backward ? q.bytes : w.bytes, offset, bytes);
}

extern "C" int ecgmm_resnet18_forward(const ecgmm_resnet18_desc* d, const float* image, const void* const* params,
                                      void* const* buffers, float* feat_out, void* ws, size_t ws_bytes,
                                      void* stream_) {
  hipStream_t s = (hipStream_t)stream_;
  Net18 r;
  ECG_TRY(build(d, r));
  FwdWs w;
  layout_fwd(r, ws, w);
  ECG_NEED(ws, ws_bytes, w.bytes, "resnet18 fwd: workspace");
  const int dt = r.d.dtype, N = r.d.N;
  const int stats_rows = r.d.training ? 1 : 0;
  ECG_TRY(side_init());
  const bool side_fwd = g_side.enabled && sw::DOWN_SIDE.get();

  ecg_tl_mark(100, s);
  // ---- every conv weight -> compute-dtype operand layouts, one launch.  (Running it on the side stream underneath
  // the stem convolution was measured: no gain -- a cross-stream event wait costs 35-140 us of GPU-side latency on
  // this platform, more than the 0.1 ms pack hides.)
  {
    EcgPackItem items[ECG_PACK_MAX];
    int n = 0;
    for (int i = 0; i < 8; ++i) {
      const Blk18& k = r.blk[i];
      BlockWs& b = w.b[i];
      items[n++] = {P(params, k.p_conv1), b.w1f, b.w1d, k.cout, k.cin, 9};
      items[n++] = {P(params, k.p_conv2), b.w2f, b.w2d, k.cout, k.cout, 9};
      if (k.down) items[n++] = {P(params, k.p_dconv), b.wdf, b.wdd, k.cout, k.cin, 1};
    }
    ECG_TRY(ecg_pack_weight_batch(dt, items, n, s));
  }
  // ---- stem
  ECG_TRY(ecg_stem_pack(dt, P(params, 0), w.wstem, 3, 7, s));
  if (stem_recompute(dt)) {
    // pass 1: statistics only; pass 2: conv recomputed -> bn -> relu -> max-pool.  The 64 x H1 x W1 conv output (411 MB at
    // batch 256) is never written: 154 + 154 MB read, 154 MB written instead of 154 + 411 + 411 read/written + 154
    if (stats_rows) ECG_TRY(ecg_stem_stats_only(dt, image, w.wstem, nullptr, w.stats, N, 3, r.d.H, r.d.W, 7, s));
    ECG_TRY(bn_coef(r.bn, w.stats, ecg_stem_stats_only_rows(N, 3, r.d.H, r.d.W, 7), 64, (long)N * r.H1 * r.W1, params, 1,
                    buffers, 0, w.coef0, s));
    ECG_TRY(ecg_stem_pool_fwd(image, w.wstem, w.coef0, w.p0, w.idx0, N, 3, r.d.H, r.d.W, s));
  } else {
    ECG_TRY(stem_forward(dt, image, w.wstem, nullptr, w.y0, stats_rows ? w.stats : nullptr, N, 3, r.d.H, r.d.W, 7, s));
    ECG_TRY(bn_coef(r.bn, w.stats, stem_forward_rows(dt, N, 3, r.d.H, r.d.W, 7), 64, (long)N * r.H1 * r.W1, params, 1,
                    buffers, 0, w.coef0, s));
    ECG_TRY(ecg_bnrelu_maxpool(dt, w.y0, w.coef0, w.p0, w.idx0, N, r.H1, r.W1, 64, s));
  }

  ecg_tl_mark(101, s);
  const void* cur = w.p0;
  for (int i = 0; i < 8; ++i) {
    const Blk18& k = r.blk[i];
    BlockWs& b = w.b[i];
    const long M = (long)N * k.hout * k.wout;
    const int rows = ecg_conv_stats_rows(M);
    ConvGeom g1 = k.conv1_geom(N);
    ConvGeom g2 = k.conv2_geom(N);
    // (ConvEpi.wg_rows: the halo kernel writes one partial-sum row per workgroup instead of one per 64 pixels)
    ConvEpi e1 = {}, e2 = {};
    e1.wg_rows = e2.wg_rows = 1;
    // the downsample branch (1x1 stride-2 conv + its BatchNorm statistics) only meets the main branch at the block's
    // last pass: it runs on the weight-gradient side stream (idle in the forward) beside conv1 -> bn1 -> conv2
    hipEvent_t down_done = nullptr;
    const bool down_side = k.down && side_fwd;
    if (down_side) {
      ConvGeom gd = k.down_geom(N);
      side_fork(s);
      ECG_TRY(ecg_conv_igemm(dt, 0, gd, cur, b.wdf, b.yd, nullptr, nullptr, stats_rows ? w.stats_d : nullptr, 0, g_side.s));
      ECG_TRY(bn_coef(r.bn, w.stats_d, rows, k.cout, M, params, k.p_dbn, buffers, k.b_dbn, b.coefd, g_side.s));
      down_done = side_mark();
    }
    ECG_TRY(ecg_conv_igemm(dt, 0, g1, cur, b.w1f, b.y1, nullptr, nullptr, stats_rows ? w.stats : nullptr, 0, s, &e1));
    ECG_TRY(bn_then_act(r, w.stats, e1.stats_rows, k.cout, M, params, k.p_bn1, buffers, k.b_bn1, b.coef1, b.y1, nullptr,
                        nullptr, b.a1, s));
    ECG_TRY(ecg_conv_igemm(dt, 0, g2, b.a1, b.w2f, b.y2, nullptr, nullptr, stats_rows ? w.stats : nullptr, 0, s, &e2));
    if (k.down) {
      if (down_side) {
        main_wait(s, down_done);
      } else {
        ConvGeom gd = k.down_geom(N);
        // (own row buffer: bn2's rows in w.stats are still unread -- their finalize is folded into the pass below)
        ECG_TRY(ecg_conv_igemm(dt, 0, gd, cur, b.wdf, b.yd, nullptr, nullptr, stats_rows ? w.stats_d : nullptr, 0, s));
        ECG_TRY(bn_coef(r.bn, w.stats_d, rows, k.cout, M, params, k.p_dbn, buffers, k.b_dbn, b.coefd, s));
      }
      ECG_TRY(bn_then_act(r, w.stats, e2.stats_rows, k.cout, M, params, k.p_bn2, buffers, k.b_bn2, b.coef2, b.y2, b.yd,
                          b.coefd, b.out, s, r.d.training && relu_bits_on() ? b.bits : nullptr));
    } else {
      ECG_TRY(bn_then_act(r, w.stats, e2.stats_rows, k.cout, M, params, k.p_bn2, buffers, k.b_bn2, b.coef2, b.y2, cur,
                          nullptr, b.out, s, r.d.training && relu_bits_on() ? b.bits : nullptr));
    }
    cur = b.out;
    ecg_tl_mark(102 + i, s);
  }
  const Blk18& last = r.blk[7];
  ECG_TRY(ecg_avgpool(dt, cur, w.pooled, N, last.hout * last.wout, 512, nullptr, s));
  ECG_TRY(ecg_linear_fwd(w.pooled, P(params, r.p_fc), P(params, r.p_fc + 1), feat_out, N, 512, r.d.out_dim, 0, nullptr,
                         s));
  ecg_tl_mark(110, s);
  return 0;
}

// stages: 0 = fc + avgpool, 1..8 = blocks 7..0, 9 = stem.  Run [stage_begin, stage_end).
// dimage (nullable): the input gradient [N][3][H][W] fp32, written by the last stage.  Behind an eval-mode forward
// (training = 0) every BatchNorm backward is the affine form; nothing in the forward workspace is written in either mode.
static int r18_backward(const ecgmm_resnet18_desc* d, const float* image, const float* dfeat, const void* const* params,
                        void* const* grads, void* ws_fwd, void* ws_bwd, size_t ws_bwd_bytes, int stage_begin, int stage_end,
                        float* dimage, hipStream_t s) {
  Net18 r;
  ECG_TRY(build(d, r));
  const bool train = r.d.training != 0;
  if (stem_recompute(r.d.dtype) && (dimage || !train))
    ECG_FAIL(ECGMM_ERR_SHAPE, "resnet18 bwd: %s needs the stored stem conv output; switch ecgmm_stem_recompute(0) "
             "(ECGMM_STEM_RECOMPUTE) off", dimage ? "the input gradient" : "an eval-mode backward");
  FwdWs w;
  layout_fwd(r, ws_fwd, w);
  BwdWs q;
  layout_bwd(r, ws_bwd, q);
  ECG_NEED(ws_fwd && ws_bwd, ws_bwd_bytes, q.bytes, "resnet18 bwd: workspace");
  const int dt = r.d.dtype, N = r.d.N;
  ECG_TRY(side_init());
  const bool side = g_side.enabled;
  // weight gradients of this call run beside the dgrad chain: narrow launches (conv_wgrad.hip, pick_nsplit)
  ecg_conv_wgrad_narrow(side, N >= 192 ? 192 : 256);
  struct NarrowOff { ~NarrowOff() { ecg_conv_wgrad_narrow(false); } } narrow_off;
  hipStream_t ws = side ? g_side.s : s;  // stream of the weight-gradient kernels
  // (capping the persistent input-gradient kernels of this call to the CUs the side stream leaves free -- 160 / 192 / 224 of 256 --
  //  measured 6.57-6.60 / 6.62-6.63 / 6.53-6.55 ms against 6.54-6.56 uncapped: the weight gradients hold their CUs only part of the time)

  if (stage_begin == 0) ecg_tl_mark(200, s);
  for (int st = stage_begin; st < stage_end; ++st) {
    if (st > 0) ecg_tl_mark(200 + st, s);   // (mark 200 + st = stage st - 1 enqueued behind it: fc = 201, blocks 7..0 = 202..209)
    if (st == 0) {
      g_side.doneA = g_side.doneB = g_side.doneC = nullptr;
      for (int a = 0; a < 3; ++a) g_side.done2[a][0] = g_side.done2[a][1] = nullptr;
      const Blk18& last = r.blk[7];
      ECG_TRY(fc_bwd(r, w, q, dfeat, params, grads, s));
      const int R = last.hout * last.wout;
      ECG_TRY(ecg_bcast_rows(dt, q.dpooled, q.X[0], N, R, 512, 1.f / (float)R, s));
    } else if (st <= 8) {
      const int i = 8 - st;
      const Blk18& k = r.blk[i];
      BlockWs& b = w.b[i];
      const void* in = i == 0 ? w.p0 : w.b[i - 1].out;
      const void* dcur = q.X[(st - 1) & 1];
      void* din = q.X[st & 1];
      const long M = (long)N * k.hout * k.wout;
      ConvGeom g1 = k.conv1_geom(N);
      ConvGeom g2 = k.conv2_geom(N);
      const int pp = st & 1;  // which of the two dy / dy1 / dyd buffers (and their reader events) this block uses
      void *dyb = q.dy[pp], *dy1b = q.dy1[pp], *dydb = q.dyd[pp];
      // The REDUCTION pass of a BatchNorm backward is fused into the epilogue of the dgrad that produces its input,
      // wherever that dgrad runs on the halo kernel (ConvEpi): bn1's into this block's conv2 dgrad; bn2's into the conv1
      // dgrad of the NEXT block (processed one stage earlier), which then also stores the gradient already masked by
      // this block's ReLU -- that buffer IS dz.  Pure function of the geometry, so stage ranges may be split across calls.
      bool fused2 = false;
      int fused2_rows = 0;
      // (ECGMM_BN_FUSE=0: always the separate reduction pass -- A/B switch; same results up to fp32 summation order)
      // Round 2 fused it where it paid then (serialized trace, profiles/r02_*_v1): on the 56x56 tensors the reduction pass
      // it replaces cost more HBM time (52 us) than the epilogue added (20-30 us); from 28x28 down the epilogue's exposed
      // load latency (one persistent workgroup per CU, 3-4 tiles each) costs MORE than the 10-30 us pass.
      // Round 3: DEFAULT OFF everywhere.  The fused epilogue is ~500 VALU per wave and tile (137 us per layer-1 launch), the
      // stream form of the same input gradient without it takes 82 us (101 with the residual addend) + the 50 us pass:
      // same-call A/B of the whole step, fused on layer 1 / never fused = 6.84, 6.88 / 6.75, 6.75 ms.
      // ECGMM_BN_FUSE_MIN_M (ecgmm_bn_fuse_min_pixels) sets the pixel-count threshold: 400000 = round 2's choice (layer 1 at
      // batch 256), 0 = fuse wherever possible.
      const bool fuse_here = train && sw::BN_FUSE.get() && M >= sw::BN_FUSE_MIN_M.get();   // (the fused reductions are the training form's)
      if (fuse_here && i + 1 < 8 && !r.blk[i + 1].down) {
        const Blk18& kn = r.blk[i + 1];
        const ConvGeom gn = kn.conv1_geom(N);
        fused2 = ecg_conv_halo_ok(dt, 1, gn);
        fused2_rows = fused2 ? ecg_conv_halo_rows(1, gn) : 0;
      }
      // out = relu(bn2(y2) + identity)
      main_wait(s, g_side.done2[0][pp]);  // the wgrad2 of two blocks ago has finished reading this dy buffer
      const void* dzp = q.dz;
      // Downsample block: bn2 and the shortcut BatchNorm differentiate the same dz -- one reduce + one apply pass for both
      // (ecg_bn_bwd_dual: dz read once instead of three times, two launches instead of four; same bits).  It writes dyd
      // here already, so the wait for that buffer's reader of two blocks ago moves up with it.  The downsample weight
      // gradient still forks where it did, behind conv1's: an earlier fork would only add slack to the side stream.
      // The shortcut BatchNorm's rows and coefficients go to red2: the rows of a fused bn2 reduction are not in use here
      // (!fused2; a downsample block's own conv1 dgrad fuses none), and the workspace keeps its size.
      const bool dual = k.down && train && !fused2 && ecg_bn_dual_on() &&
                        ecg_bn_bwd_scratch(dt, M, k.cout) <= RED_ROWS_FLOATS * sizeof(float);
      if (dual) {
        main_wait(s, g_side.done2[2][pp]);
        ECG_TRY(ecg_bn_bwd_dual(dt, dcur, b.out, relu_bits_on() ? b.bits : nullptr, nullptr, nullptr, b.y2, b.coef2,
                                P(params, k.p_bn2), G(grads, k.p_bn2), G(grads, k.p_bn2 + 1), dyb, b.yd, b.coefd,
                                P(params, k.p_dbn), G(grads, k.p_dbn), G(grads, k.p_dbn + 1), dydb, q.dz, nullptr, M, k.cout,
                                q.bn_scratch, q.red2, s));
      } else if (fused2) {
        dzp = dcur;
        ECG_TRY(ecg_bn_bwd_tail(dt, dcur, nullptr, b.y2, b.coef2, P(params, k.p_bn2), G(grads, k.p_bn2),
                                G(grads, k.p_bn2 + 1), dyb, q.red2, fused2_rows, M, k.cout, q.bn_scratch, s));
      } else {
        // (the eval forward writes no mask bits: its backward re-reads `out`)
        ECG_TRY(bn_bwd_mode(r.bn, dcur, b.out, nullptr, nullptr, 1, b.y2, b.coef2, P(params, k.p_bn2), G(grads, k.p_bn2),
                            G(grads, k.p_bn2 + 1), dyb, q.dz, nullptr, M, k.cout, q.bn_scratch, s,
                            train && relu_bits_on() ? b.bits : nullptr));
      }
      if (G(grads, k.p_conv2)) {
        if (side) side_fork(s);
        ECG_TRY(ecg_conv_wgrad(dt, g2, b.a1, dyb, G(grads, k.p_conv2), 0, q.wg_ws, q.wg_bytes, ws));
        if (side) g_side.done2[0][pp] = side_mark();
      }
      // a1 = relu(bn1(y1)); the mask is recomputed from y1
      ConvEpi ea = {};
      if (fuse_here) { ea.wg_rows = 1; ea.red_y = b.y1; ea.red_mask = b.y1; ea.red_coef = b.coef1; ea.red_rows = q.red1; }
      ECG_TRY(ecg_conv_igemm(dt, 1, g2, dyb, b.w2d, q.da, nullptr, nullptr, nullptr, 0, s, &ea));
      main_wait(s, g_side.done2[1][pp]);
      if (ea.red_done) {
        ECG_TRY(ecg_bn_bwd_tail(dt, q.da, b.y1, b.y1, b.coef1, P(params, k.p_bn1), G(grads, k.p_bn1),
                                G(grads, k.p_bn1 + 1), dy1b, q.red1, ea.red_rows_n, M, k.cout, q.bn_scratch, s));
      } else {
        ECG_TRY(bn_bwd_mode(r.bn, q.da, b.y1, nullptr, nullptr, 1, b.y1, b.coef1, P(params, k.p_bn1), G(grads, k.p_bn1),
                            G(grads, k.p_bn1 + 1), dy1b, nullptr, nullptr, M, k.cout, q.bn_scratch, s));
      }
      if (G(grads, k.p_conv1)) {
        if (side) side_fork(s);
        ECG_TRY(ecg_conv_wgrad(dt, g1, in, dy1b, G(grads, k.p_conv1), 0, q.wg_ws, q.wg_bytes, ws));
        if (side) g_side.done2[1][pp] = side_mark();
      }
      if (k.down) {
        ConvGeom gd = k.down_geom(N);
        if (!dual) {
          main_wait(s, g_side.done2[2][pp]);
          ECG_TRY(bn_bwd_mode(r.bn, dzp, nullptr, nullptr, nullptr, 1, b.yd, b.coefd, P(params, k.p_dbn), G(grads, k.p_dbn),
                              G(grads, k.p_dbn + 1), dydb, nullptr, nullptr, M, k.cout, q.bn_scratch, s));
        }
        if (G(grads, k.p_dconv)) {
          if (side) side_fork(s);
          ECG_TRY(ecg_conv_wgrad(dt, gd, in, dydb, G(grads, k.p_dconv), 0, q.wg_ws, q.wg_bytes, ws));
          if (side) g_side.done2[2][pp] = side_mark();
        }
        // the downsample branch's input gradient is one more tap of the stride-2 dgrad's parity class (0,0): one launch,
        // no [N][H][W][Cin] temporary written and re-read as addend
        ConvEpi ed = {};
        ed.src2 = dydb; ed.wpk2 = b.wdd;
        if (!sw::DOWN_FOLD.get()) ed.src2 = nullptr;
        if (ed.src2) {
          ECG_TRY(ecg_conv_igemm(dt, 1, g1, dy1b, b.w1d, din, nullptr, nullptr, nullptr, 0, s, &ed));
        }
        if (!ed.src2_done) {
          ECG_TRY(ecg_conv_igemm(dt, 1, gd, dydb, b.wdd, q.dtmp, nullptr, nullptr, nullptr, 0, s));
          ECG_TRY(ecg_conv_igemm(dt, 1, g1, dy1b, b.w1d, din, nullptr, q.dtmp, nullptr, 0, s));
        }
      } else {
        // this conv1 dgrad produces the previous block's output gradient: fuse that block's bn2 reduction (see above)
        ConvEpi eb = {};
        if (fuse_here && i > 0 && ecg_conv_halo_ok(dt, 1, g1)) {
          const BlockWs& pb = w.b[i - 1];
          eb.wg_rows = 1; eb.red_y = pb.y2; eb.red_mask = pb.out; eb.red_coef = pb.coef2; eb.red_rows = q.red2;
        }
        ECG_TRY(ecg_conv_igemm(dt, 1, g1, dy1b, b.w1d, din, nullptr, dzp, nullptr, 0, s, &eb));
      }
    } else if (st == 9) {
      const void* dp0 = q.X[8 & 1];
      if (stem_recompute(dt)) {
        // BatchNorm-backward reduction over the pooled tensors, then ONE kernel: conv recomputed per tile, max-pool backward
        // gathered, BatchNorm backward applied, weight-gradient products taken -- neither y0 nor dy0 exist.  On the
        // caller's stream like the stem wgrad it replaces (see below); own workspace q.stem_ws.
        ECG_TRY(ecg_stem_pool_bwd(image, w.wstem, w.coef0, P(params, 1), dp0, w.p0, w.idx0, G(grads, 1), G(grads, 2),
                                  G(grads, 0), q.stem_ws, q.stem_bytes, N, 3, r.d.H, r.d.W, s));
        continue;
      }
      if (train && ecg_stem_fuse_on()) {
        ECG_TRY(ecg_pool_bn_bwd(dt, dp0, w.p0, w.idx0, w.y0, w.coef0, P(params, 1), G(grads, 1), G(grads, 2), q.big1,
                                nullptr, N, r.H1, r.W1, 64, q.bn_scratch, s));
      } else {
        // (eval: always the plain two passes -- max-pool + ReLU backward, then the affine BatchNorm backward)
        ECG_TRY(ecg_maxpool_relu_bwd(dt, dp0, w.p0, w.idx0, q.big0, N, r.H1, r.W1, 64, s));
        ECG_TRY(bn_bwd_mode(r.bn, q.big0, nullptr, nullptr, nullptr, 1, w.y0, w.coef0, P(params, 1), G(grads, 1), G(grads, 2),
                            q.big1, nullptr, nullptr, (long)N * r.H1 * r.W1, 64, q.bn_scratch, s));
      }
      if (G(grads, 0)) {
        // the last kernel of the backward stays on the caller's stream: nothing is left there to overlap it with, it
        // overlaps the side stream's remaining wgrads instead, and the join below then waits for an event that has
        // usually fired already (an exposed cross-stream wait costs 35-140 us here).  Own slab buffer: q.stem_ws.
        ECG_TRY(ecg_stem_wgrad(dt, image, q.big1, G(grads, 0), 0, q.stem_ws, q.stem_bytes, N, 3, r.d.H, r.d.W, 7, s));
      }
      // the input gradient: the transposed stem convolution of the same dy0 (conv_stem_dgrad.hip)
      if (dimage) ECG_TRY(ecg_stem_dgrad(dt, q.big1, P(params, 0), dimage, N, 3, r.d.H, r.d.W, 7, s));
    } else {
      ECG_FAIL(ECGMM_ERR_SHAPE, "resnet18 bwd: stage %d out of range", st);
    }
  }
  if (stage_end == 10) ecg_tl_mark(210, s);
  if (side && !g_side.defer_join) {  // join: everything the side stream did is ordered before whatever the caller enqueues next
    hipEvent_t e = side_next_ev();
    (void)hipEventRecord(e, g_side.s);
    (void)hipStreamWaitEvent(s, e, 0);
  }
  if (stage_end == 10) ecg_tl_mark(211, s);
  return 0;
}

extern "C" int ecgmm_resnet18_backward(const ecgmm_resnet18_desc* d, const float* image, const float* dfeat,
                                       const void* const* params, void* const* grads, void* ws_fwd, void* ws_bwd,
                                       size_t ws_bwd_bytes, int stage_begin, int stage_end, void* stream_) {
  return r18_backward(d, image, dfeat, params, grads, ws_fwd, ws_bwd, ws_bwd_bytes, stage_begin, stage_end, nullptr,
                      (hipStream_t)stream_);
}

// The same backward with the input gradient as one more output of the last stage (dimage may be null).
extern "C" int ecgmm_resnet18_backward_dx(const ecgmm_resnet18_desc* d, const float* image, const float* dfeat,
                                          const void* const* params, void* const* grads, void* ws_fwd, void* ws_bwd,
                                          size_t ws_bwd_bytes, int stage_begin, int stage_end, float* dimage,
                                          void* stream_) {
  return r18_backward(d, image, dfeat, params, grads, ws_fwd, ws_bwd, ws_bwd_bytes, stage_begin, stage_end, dimage,
                      (hipStream_t)stream_);
}

// Grad-CAM of layer4's output for the logits whose gradient w.r.t. the encoder output is dfeat [N][out_dim]: the fc
// backward gives d / d pooled, the map kernels (gradcam.hip) do the rest.  cam: [N][H][W] fp32 in [0, 1].
extern "C" int ecgmm_resnet18_gradcam(const ecgmm_resnet18_desc* d, const float* dfeat, const void* const* params,
                                      void* ws_fwd, void* ws_bwd, size_t ws_bwd_bytes, float* cam, void* stream_) {
  hipStream_t s = (hipStream_t)stream_;
  Net18 r;
  ECG_TRY(build(d, r));
  FwdWs w;
  layout_fwd(r, ws_fwd, w);
  BwdWs q;
  layout_bwd(r, ws_bwd, q);
  ECG_NEED(ws_fwd && ws_bwd, ws_bwd_bytes, q.bytes, "resnet18 gradcam: workspace");
  if (!dfeat || !cam) ECG_FAIL(ECGMM_ERR_SHAPE, "resnet18 gradcam: null operand");
  ECG_TRY(fc_bwd(r, w, q, dfeat, params, nullptr, s));
  const Blk18& last = r.blk[7];
  // (q.X[0] holds max_act elements of the compute dtype >= N x hout x wout x 512: room for the N x hout x wout fp32 map)
  return ecg_gradcam(r.d.dtype, w.b[7].out, q.dpooled, (float*)q.X[0], cam, r.d.N, last.hout, last.wout, 512, r.d.H, r.d.W,
                     s);
}

