/* libecgmm_hip.so -- C ABI of the MI355X (gfx950) multimodal ECG hot path.
 *
 * The reference (hyeeiin/ECG-Multimodal-Model) is pure PyTorch and has no FFI; the boundary this
 * library sits behind is the torch.nn.Module / autograd contract of its model classes.  Each entry
 * point below therefore names the reference torch call it replaces (paths relative to the reference
 * tree; "PMB" = multimodal_paper_modal_balance.py).  The Python host (ecg-multimodal-model_amd/)
 * binds these with ctypes; INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; the caller (PyTorch) owns ALL memory.  No entry point
 *     allocates, frees, synchronises or retains a pointer after it returns.
 *   - every function enqueues on the hipStream_t passed as `stream` (void*; 0 = default stream).
 *   - return 0 on success, an ECGMM_ERR_* code otherwise; ecgmm_last_error() gives the message
 *     (thread-local).  The Python wrapper raises RuntimeError.
 *   - activations are channels-last ([N,H,W,C] / [N,L,C]) in the compute dtype (ECGMM_BF16 or
 *     ECGMM_F32); parameters, statistics, gradients and the dense tails are fp32.
 */
#ifndef ECGMM_H
#define ECGMM_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ECGMM_VERSION 100

enum { ECGMM_F32 = 0, ECGMM_BF16 = 1 };
enum { ECGMM_ACT_NONE = 0, ECGMM_ACT_RELU = 1, ECGMM_ACT_SIGMOID = 2 };
enum {
  ECGMM_OK = 0,
  ECGMM_ERR_SHAPE = 1,
  ECGMM_ERR_DTYPE = 2,
  ECGMM_ERR_WORKSPACE = 3,
  ECGMM_ERR_LAUNCH = 4
};

int ecgmm_version(void);
const char* ecgmm_last_error(void);

/* The ECGMM_* environment switches the library reads (one table: csrc/switches.h; list: INTEGRATION.md section 5), by
 * name.  ecgmm_switch_name(i): the i-th switch's environment variable name, NULL past the end.  ecgmm_switch_get: the
 * value in effect (reads the environment if nothing has yet).  ecgmm_switch_set: what the named setter below does, with
 * the same clamp; ECGMM_ERR_SHAPE for an unknown name and for a switch that is read once at start-up.  ECGMM_SIDE_WGRAD
 * is refused too: after start-up it is each plan's own state, switched with ecgmm_side_wgrad(), which initialises the GPU. */
const char* ecgmm_switch_name(int i);
int ecgmm_switch_get(const char* env_name, int64_t* value);
int ecgmm_switch_set(const char* env_name, int64_t value);

/* ---------------------------------------------------------------------------------------------
 * Encoder plans (the product path: one call = one encoder forward / backward)
 * ------------------------------------------------------------------------------------------- */
#define ECGMM_RESNET18_NPARAMS 62
#define ECGMM_RESNET18_NBUFFERS 60
typedef struct {
  int N, H, W;      /* image batch, NCHW fp32 */
  int out_dim;      /* fc out_features (PMB:221 -> image_dim; train_image_only.py:96 -> num_classes) */
  int dtype;        /* trunk compute dtype */
  int training;     /* BatchNorm batch statistics + running-stat update (model.train(), train.py:57) */
  float bn_momentum, bn_eps;
} ecgmm_resnet18_desc;

/* replaces self.image_encoder(image) -- torchvision resnet18 instantiated at PMB:210, called PMB:325;
 * ImageOnlyClassifier.forward, train_image_only.py:98 */
size_t ecgmm_resnet18_fwd_workspace(const ecgmm_resnet18_desc* d);
size_t ecgmm_resnet18_bwd_workspace(const ecgmm_resnet18_desc* d);
int ecgmm_resnet18_forward(const ecgmm_resnet18_desc* d, const float* image, const void* const* params,
                           void* const* buffers, float* feat_out, void* ws, size_t ws_bytes, void* stream);
/* replaces the image-encoder part of total_loss.backward() (train.py:80, train_image_only.py:131).
 * grads[i] == NULL skips that parameter (requires_grad=False, train.py:35-40). Gradients are WRITTEN
 * (not accumulated).  stages [begin,end): 0 = fc+avgpool, 1..8 = blocks 7..0, 9 = stem -- the split
 * lets the host launch a gradient all-reduce bucket between stages. */
int ecgmm_resnet18_backward(const ecgmm_resnet18_desc* d, const float* image, const float* dfeat,
                            const void* const* params, void* const* grads, void* ws_fwd, void* ws_bwd,
                            size_t ws_bwd_bytes, int stage_begin, int stage_end, void* stream);
/* The same backward with the input gradient as one more output: dimage [N,3,H,W] fp32 (nullable) is written, in full, by
 * the last stage (9) -- image.requires_grad_(True) upstream of self.image_encoder(image), PMB:325.  Both entry points
 * also run behind a forward with training = 0 (torch: net.eval(); net(x).backward()): every BatchNorm backward is then
 * the affine form over the running statistics, parameter gradients are produced for every non-null entry of grads as in
 * training mode, and the forward workspace is only read, so one eval forward serves any number of backward calls.
 * With ecgmm_stem_recompute(1) (no stored stem conv output) the input gradient and the eval backward are refused. */
int ecgmm_resnet18_backward_dx(const ecgmm_resnet18_desc* d, const float* image, const float* dfeat,
                               const void* const* params, void* const* grads, void* ws_fwd, void* ws_bwd,
                               size_t ws_bwd_bytes, int stage_begin, int stage_end, float* dimage, void* stream);
/* Grad-CAM of layer4's output (the overlays of the reference's gpt/ pictures): dfeat [N,out_dim] = d logit / d encoder
 * output (from the head's backward); ws_fwd = the workspace of the forward, ws_bwd as for ecgmm_resnet18_backward.
 * cam [N,H,W] fp32 = upsample_bilinear(relu(sum_c a_c A_c) / max), a_c = d logit / d pooled_c / (H'W'); all zero where
 * the maximum is 0; align_corners=False. */
int ecgmm_resnet18_gradcam(const ecgmm_resnet18_desc* d, const float* dfeat, const void* const* params, void* ws_fwd,
                           void* ws_bwd, size_t ws_bwd_bytes, float* cam, void* stream);
/* Debugging and test aid: where a named tensor lies inside the forward (backward = 0) or backward (backward = 1) workspace
 * of this descriptor -- *offset bytes from the workspace base, *bytes long.  Computed by the plan's own layout code; launches
 * nothing and needs no GPU.  Forward names: wstem y0 coef0 p0 idx0 pooled (index 0) and, per block (index 0..7), w1f w1d w2f
 * w2d wdf wdd y1 a1 y2 yd out bits coef1 coef2 coefd.  Backward names: X dy dy1 dyd (index 0 / 1), dz da dtmp big0 big1
 * dpooled (index 0).  Activations are channels-last in the compute dtype, coef* are [4][C] fp32 (scale, shift, mean,
 * invstd), bits one bit per element of out, idx0 one byte per pooled element.  ECGMM_ERR_SHAPE with a message for an
 * unknown name or index and for a tensor this descriptor does not have (yd / wdf / wdd / coefd of a block without a
 * downsample, bits in fp32, y0 / big0 / big1 under ecgmm_stem_recompute(1)). */
int ecgmm_resnet18_ws_view(const ecgmm_resnet18_desc* d, int backward, const char* name, int index, size_t* offset,
                           size_t* bytes);

/* The ResNet18 backward runs its weight-gradient kernels on a library-owned side stream (forked from /
 * joined to `stream` with events inside each call).  0 = keep everything on the caller's stream. */
int ecgmm_side_wgrad(int on);
/* Data-parallel overlap (parallel.py): defer = 1 makes ecgmm_resnet18_backward return without joining the side
 * stream; ecgmm_side_wait(stream) orders `stream` (the all-reduce stream) after the weight gradients issued so
 * far.  The last stage group of a backward must run with defer = 0. */
int ecgmm_side_defer_join(int defer);
/* the same switch for the ResNet1D_SE plan alone (ecgmm_side_wgrad sets both): a host that already runs the signal encoder
 * on a side stream of its own beside the image encoder turns it off -- more than four busy HIP streams share hardware queues */
int ecgmm_resnet1d_side_wgrad(int on);
int ecgmm_side_wait(void* stream);
/* The side stream itself (a hipStream_t, NULL when switched off) and "fork" (work enqueued on `stream` so far happens-before
 * later work on the side stream): a data-parallel host can issue its overlapped all-reduces from the side stream's
 * context instead of a stream of its own -- a fifth busy stream oversubscribes the four hardware queues. */
void* ecgmm_side_stream(void);
int ecgmm_side_fork(void* stream);

#define ECGMM_RESNET1D_NPARAMS 52
#define ECGMM_RESNET1D_NBUFFERS 27
typedef struct {
  int N, cin, L;        /* signal batch [N, cin, L] fp32 (ecg_signal.unsqueeze(1), PMB:328) */
  int num_classes;      /* classifier[4] out_features (PMB:226 -> signal_dim) */
  int dtype;
  int training;
  float bn_momentum, bn_eps;
  float dropout_p;      /* classifier[3] = Dropout(0.3), PMB:115; applied only when training */
  uint64_t seed, offset;
} ecgmm_resnet1d_desc;

/* replaces ResNet1D_SE.forward (PMB:119-125; signal_model.py:82-88; train_signal_12_af.py:204-210) */
size_t ecgmm_resnet1d_fwd_workspace(const ecgmm_resnet1d_desc* d);
size_t ecgmm_resnet1d_bwd_workspace(const ecgmm_resnet1d_desc* d);
int ecgmm_resnet1d_forward(const ecgmm_resnet1d_desc* d, const float* signal, const void* const* params,
                           void* const* buffers, float* feat_out, void* ws, size_t ws_bytes, void* stream);
/* stages: 0 = classifier+avgpool, 1..3 = layer3..layer1, 4 = stem */
int ecgmm_resnet1d_backward(const ecgmm_resnet1d_desc* d, const float* signal, const float* dfeat,
                            const void* const* params, void* const* grads, void* ws_fwd, void* ws_bwd,
                            size_t ws_bwd_bytes, int stage_begin, int stage_end, void* stream);
/* as ecgmm_resnet18_backward_dx: dsignal [N,cin,L] fp32 (nullable) written by the last stage (4); eval-mode forwards
 * (training = 0) are differentiated through the running statistics by both entry points */
int ecgmm_resnet1d_backward_dx(const ecgmm_resnet1d_desc* d, const float* signal, const float* dfeat,
                               const void* const* params, void* const* grads, void* ws_fwd, void* ws_bwd,
                               size_t ws_bwd_bytes, int stage_begin, int stage_end, float* dsignal, void* stream);
/* Grad-CAM of layer3's output along the signal: cam [N,L] fp32 (see ecgmm_resnet18_gradcam) */
int ecgmm_resnet1d_gradcam(const ecgmm_resnet1d_desc* d, const float* dfeat, const void* const* params, void* ws_fwd,
                           void* ws_bwd, size_t ws_bwd_bytes, float* cam, void* stream);
/* as ecgmm_resnet18_ws_view.  Forward names: wstem y0 coef0 p0 idx0 pooled h1 hd dmask (index 0) and, per block (index
 * 0..2), w1f w1d w2f w2d wdf wdd y1 a1 y2 yd out coef1 coef2 coefd m h g.  Backward names: X (index 0 / 1), dz dy dy1 dyd
 * da dtmp big0 big1 dpooled dh1 dfeat_h dg ds dh dm (index 0); dg ds dh dm are sized for the widest block. */
int ecgmm_resnet1d_ws_view(const ecgmm_resnet1d_desc* d, int backward, const char* name, int index, size_t* offset,
                           size_t* bytes);

/* ---------------------------------------------------------------------------------------------
 * Inference plans (opt-in): the eval-mode forward of either encoder with every BatchNorm folded into the convolution in
 * front of it and bias / residual / ReLU in the convolution's epilogue.  They replace self.image_encoder(image) /
 * self.signal_encoder(ecg_signal) under model.eval() + torch.no_grad(): the validation pass (train.py:92-95,
 * train_kfold.py:72-74, train_image_only.py:142-144, signal_model.py:174-176), the test pass (train.py:175-182,
 * train_kfold.py:118-121, train_image_only.py:180-185) and the embedding extraction of shap_fusion_modal_balance.py:54-59.
 * The training plans above, their eval mode, the eval-mode backward and Grad-CAM are unchanged; an inference forward keeps
 * nothing a backward could use.
 *
 * prepare: params / buffers (the tables of ecgmm_resnet18_forward / ecgmm_resnet1d_forward) -> a prepared blob of
 *   *_infer_prepared_bytes(d) bytes, one launch.  Of the descriptor only dtype, out_dim / num_classes, cin and bn_eps are
 *   read: one blob serves any batch and any input size.  Do it again after the weights changed.
 * infer: input + blob -> feat_out [N, out_dim] fp32.  Reads no parameter, no buffer, writes nothing but feat_out and ws
 *   (*_infer_workspace(d) bytes: the stem output + a fixed set of rotating block buffers).  `training`, `bn_momentum`,
 *   `dropout_p`, `seed`, `offset` of the descriptors are ignored: there is no dropout and no statistics update. */
size_t ecgmm_resnet18_infer_prepared_bytes(const ecgmm_resnet18_desc* d);
int ecgmm_resnet18_infer_prepare(const ecgmm_resnet18_desc* d, const void* const* params, const void* const* buffers,
                                 void* blob, size_t blob_bytes, void* stream);
size_t ecgmm_resnet18_infer_workspace(const ecgmm_resnet18_desc* d);
int ecgmm_resnet18_infer(const ecgmm_resnet18_desc* d, const float* image, const void* blob, size_t blob_bytes,
                         float* feat_out, void* ws, size_t ws_bytes, void* stream);
size_t ecgmm_resnet1d_infer_prepared_bytes(const ecgmm_resnet1d_desc* d);
int ecgmm_resnet1d_infer_prepare(const ecgmm_resnet1d_desc* d, const void* const* params, const void* const* buffers,
                                 void* blob, size_t blob_bytes, void* stream);
size_t ecgmm_resnet1d_infer_workspace(const ecgmm_resnet1d_desc* d);
int ecgmm_resnet1d_infer(const ecgmm_resnet1d_desc* d, const float* signal, const void* blob, size_t blob_bytes,
                         float* feat_out, void* ws, size_t ws_bytes, void* stream);
/* ResNet18 inference plan: the downsample convolution of a block on a library-owned side stream beside conv1 (1) or in
 * line on the caller's stream (0, default).  Start-up value: ECGMM_INFER_DOWN_SIDE. */
int ecgmm_infer_down_side(int on);

/* The multimodal head: everything ECGMultimodalModel.forward does after the three encoders, as ONE call per
 * direction (PMB:326-354 / multimodal.py:440-469: three LayerNorms, three branch Linear heads, AttentionFusion,
 * fusion_classifier = Linear-ReLU-Dropout-Linear, var_loss).  Same kernels as the per-op entry points below.
 * params (19, fp32): image_norm.{weight,bias}, signal_norm.{..}, clinical_norm.{..}, image_classifier.{weight,bias},
 * signal_classifier.{..}, clinical_classifier.{..}, attention_fusion.weights, attention_fusion.norm.{weight,bias},
 * fusion_classifier.0.{weight,bias}, fusion_classifier.3.{weight,bias}.
 * raw[3]: encoder outputs [B, dim[m]];  logits[4]: image / signal / clinical / fusion logits [B, num_classes];
 * var_loss: scalar;  soft_w: softmax of the 3 fusion weights. */
#define ECGMM_HEAD_NPARAMS 19
typedef struct {
  int B;
  int dim[3];        /* image_dim, signal_dim, clinical_dim (PMB:203-206: 256 each; multimodal.py:340-342: 512/128/32) */
  int hidden;        /* fusion_classifier.0 out_features (128, PMB:284) */
  int num_classes;
  int training;      /* Dropout active (model.train()) */
  float ln_eps;
  float dropout_p;   /* fusion_classifier.2 = Dropout(0.3), PMB:287 */
  uint64_t seed, offset;
} ecgmm_head_desc;
size_t ecgmm_head_fwd_workspace(const ecgmm_head_desc* d);
size_t ecgmm_head_bwd_workspace(const ecgmm_head_desc* d);
int ecgmm_head_forward(const ecgmm_head_desc* d, const float* const* raw, const void* const* params,
                       float* const* logits, float* var_loss, float* soft_w, void* ws, size_t ws_bytes, void* stream);
/* replaces the head part of total_loss.backward() (train.py:80).  dlogits[k] / dvar NULL = that output is not in the
 * loss (train.py:78 uses only fusion_logits and var_loss): the branch is skipped, its grads[] entries are left
 * untouched.  grads[i] NULL skips a parameter; draw[m] NULL = encoder m is frozen (train.py:35-40).  Gradients are
 * WRITTEN, not accumulated. */
int ecgmm_head_backward(const ecgmm_head_desc* d, const float* const* raw, const void* const* params,
                        void* const* grads, const float* const* dlogits, const float* dvar, float* const* draw,
                        void* ws_fwd, void* ws_bwd, size_t ws_bwd_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Per-op entry points (building blocks of the plans; also what the parity tests call one by one)
 * ------------------------------------------------------------------------------------------- */
typedef struct {
  int N, H, W, Cin, Cout, R, S, stride, pad_h, pad_w;
} ecgmm_conv_desc;

/* layout helpers (the reference's tensors are NCHW / OIHW) */
int ecgmm_nchw_to_nhwc(int dtype, const float* src, void* dst, int N, int C, int64_t HW, void* stream);
int ecgmm_nhwc_to_nchw(int dtype, const void* src, float* dst, int N, int C, int64_t HW, void* stream);
int ecgmm_cast(int dtype, const float* src, void* dst, int64_t n, void* stream);
int ecgmm_uncast(int dtype, const void* src, float* dst, int64_t n, void* stream);
/* OIHW fp32 -> forward pack [Cout][R*S][Cin] and/or dgrad pack [Cin][R*S][Cout] (either may be NULL) */
int ecgmm_pack_conv_weight(int dtype, const float* w_oihw, void* fwd, void* dgrad, int Cout, int Cin, int RS,
                           void* stream);

/* nn.Conv2d / nn.Conv1d forward (F.conv2d inside torchvision BasicBlock; PMB:71,74,81 Conv1d).
 * stats (nullable): partial BatchNorm sums, ecgmm_conv_stats_rows(N*OH*OW) rows of [2][Cout]. */
int ecgmm_conv_stats_rows(int64_t out_pixels);
/* Stride-1 3x3 (pad 1) and 1x3 (pad 1) bf16 convolutions over whole 256-pixel tiles are served by the halo-resident
 * kernel (csrc/conv_halo.hip) instead of the general implicit-GEMM one: mode 0 = never, 1 = for the shapes it is
 * faster on (default), 2 = wherever it is applicable (A/B timing, tests).  Start-up value: ECGMM_CONV_HALO=0|1|2. */
int ecgmm_conv_halo_enable(int on);
/* Cap on the CUs (one persistent workgroup each) a halo-kernel launch occupies; 0 = all of them (default).  The partial-row
 * counts of its fused BatchNorm reductions follow the cap.  Start-up value: ECGMM_HALO_CUS. */
int ecgmm_conv_halo_cus(int cus);
/* 64 -> 64 channel 3x3 convolutions (ResNet18 layer 1) on 4-wave workgroups, two per CU, instead of one 8-wave
 * workgroup per CU: 0 = off (default: faster stand-alone, slower inside the overlapped step), 1 = on.
 * Start-up value: ECGMM_HALO_W4. */
int ecgmm_conv_halo_w4(int on);
/* Halo conv kernel: waves 4-7 of the 8-wave workgroup run each step's first MFMA block behind the step's barrier instead of
 * in front of it, so the two waves of a SIMD alternate between the matrix pipe and the LDS / fill issue instead of meeting
 * there: 1 = on (default), 0 = lock step.  Pure scheduling (bit-identical results).  Start-up value: ECGMM_HALO_STAGGER. */
int ecgmm_conv_halo_stagger(int on);
/* Halo conv kernel, 64 -> 64 channel 3x3 tiles (ResNet18 layer 1): STREAM form -- the K loop runs on across tile boundaries
 * (weight ring, next tile's halo and step-0 fragments already in flight) and a tile's epilogue runs inside the next tile's
 * first K steps: 1 = on (default), 0 = one tile at a time.  Bit-identical results.  Start-up value: ECGMM_HALO_STREAM. */
int ecgmm_conv_halo_stream(int on);
/* Halo conv kernel, 128-channel tiles: ping-pong K loop (each K step as four read | MFMA phases, waves 4-7 one barrier behind
 * waves 0-3, so one wave of every SIMD feeds the matrix pipe while its partner reads LDS / issues fills): 1 = on (default),
 * 0 = the lock-step loop.  Bit-identical results.  Start-up value: ECGMM_HALO_PP. */
int ecgmm_conv_halo_pingpong(int on);
/* Ring weight-gradient kernel (3x3, two 4-wave groups per workgroup): the groups run half a K step apart (a second barrier
 * in the middle of the step, one barrier of offset), so one group's MFMA-only half pairs with the other's fill issue /
 * fragment-address head: 1 = on, 0 = lock step (default: measured 1 % slower with it).  Bit-identical results.
 * Start-up value: ECGMM_WGRAD_PP. */
int ecgmm_conv_wgrad_pingpong(int on);
/* Weight gradients of the same stride-1 3x3 / 1x3 bf16 convolutions keep their x operand in an LDS ring of pixel rows
 * (wgrad_ring_kernel, csrc/conv_wgrad.hip) instead of one gathered tile per filter tap: 0 = never, 1 = for the shapes
 * it is faster on (default), 2 = wherever applicable (A/B, tests).  Start-up value: ECGMM_WGRAD_RING=0|1|2. */
int ecgmm_conv_wgrad_ring_enable(int on);
int ecgmm_conv_fwd(int dtype, const ecgmm_conv_desc* c, const void* x, const void* w_fwd, const float* bias, void* y,
                   float* stats, int act, void* stream);
/* the same with the BatchNorm partial sums as ONE row per workgroup where the halo-resident kernel serves the shape (*nrows
 * rows of [2][Cout], at most 512; otherwise the per-64-pixel rows above and their count): what the encoder plans call.
 * stats: room for ecgmm_conv_stats_rows(N*OH*OW) + ECGMM_BN_TAIL_ROWS rows. */
int ecgmm_conv_fwd_wgrows(int dtype, const ecgmm_conv_desc* c, const void* x, const void* w_fwd, const float* bias, void* y,
                          float* stats, int* nrows, int act, void* stream);
/* autograd of the above: input gradient (addend, nullable, is added to dx) and weight gradient */
int ecgmm_conv_bwd_data(int dtype, const ecgmm_conv_desc* c, const void* dy, const void* w_dgrad, const void* addend,
                        void* dx, void* stream);
size_t ecgmm_conv_bwd_weight_workspace(int dtype, const ecgmm_conv_desc* c);
int ecgmm_conv_bwd_weight(int dtype, const ecgmm_conv_desc* c, const void* x, const void* dy, float* dw_oihw,
                          int accumulate, void* ws, size_t ws_bytes, void* stream);

/* stem convolutions straight from NCHW / NCL fp32 input: resnet18.conv1 (R = 7) and
 * ResNet1D_SE.initial[0] (R = 1, H = 1; PMB:100) */
size_t ecgmm_stem_packed_elems(int Cin, int R);
int ecgmm_stem_stats_rows(int N, int Cin, int H, int W, int R);
int ecgmm_stem_pack(int dtype, const float* w_oihw, void* packed, int Cin, int R, void* stream);
int ecgmm_stem_fwd(int dtype, const float* x, const void* packed, const float* bias, void* y, float* stats, int N,
                   int Cin, int H, int W, int R, void* stream);
/* bf16 form of ecgmm_stem_fwd whose BatchNorm partial sums stay in registers across a workgroup's tiles: 4 rows per
 * workgroup (ecgmm_stem_wg_stats_rows) instead of 4 per tile -- what the encoder plans call */
int ecgmm_stem_wg_stats_rows(int N, int Cin, int H, int W, int R);
int ecgmm_stem_fwd_wgrows(int dtype, const float* x, const void* packed, const float* bias, void* y, float* stats, int N,
                          int Cin, int H, int W, int R, void* stream);
size_t ecgmm_stem_bwd_weight_workspace(int N, int Cin, int H, int W, int R);
int ecgmm_stem_bwd_weight(int dtype, const float* x, const void* dy, float* dw_oihw, int accumulate, void* ws,
                          size_t ws_bytes, int N, int Cin, int H, int W, int R, void* stream);
/* input gradient of the same two convolutions == autograd of F.conv2d(x, w, stride=2, padding=3) (R = 7) /
 * F.conv1d(x, w, stride=2, padding=3) (R = 1, H = 1) w.r.t. x: dy [N,OH,OW,64] compute dtype channels-last (as
 * ecgmm_stem_fwd stores y), w_oihw the fp32 master weights [64,Cin,R,7] (rounded to the compute dtype inside),
 * dx [N,Cin,H,W] fp32, every element written once (no memset, no atomics); fp32 accumulation.  Cin <= 9 (R = 7) / 24. */
int ecgmm_stem_bwd_data(int dtype, const void* dy, const float* w_oihw, float* dx, int N, int Cin, int H, int W, int R,
                        void* stream);

/* The 2-D stem BY RECOMPUTE (csrc/conv_stem_fused.hip; bf16, 7x7 stride 2, Cin <= 3): conv1 -> bn1 -> relu -> maxpool of
 * torchvision's resnet18 (the reference's image encoder, multimodal_paper_modal_balance.py:210) without the
 * full-resolution conv output ever reaching HBM.
 *   stem_stats_only   image -> BatchNorm partial sums ([rows][2][64], rows = ecgmm_stem_stats_only_rows; finalize with
 *                     ecgmm_bn_finalize over N*OH*OW values)
 *   stem_pool_fwd     image -> conv -> bn(coef) -> relu -> MaxPool(3,2,1): pooled [N,PH,PW,64] bf16 + arg-max bytes; the
 *                     same values as ecgmm_stem_fwd + ecgmm_bnrelu_maxpool
 *   stem_pool_bwd     gradient w.r.t. pooled -> dgamma, dbeta of bn1 and (dw_oihw non-null) the conv weight gradient: the
 *                     conv is recomputed per tile, the max-pool backward gathered, the BatchNorm backward applied and the
 *                     weight-gradient products taken without writing y or dy.  Same results as ecgmm_pool_bn_bwd +
 *                     ecgmm_stem_bwd_weight up to fp32 summation order. */
int ecgmm_stem_stats_only_rows(int N, int Cin, int H, int W, int R);
int ecgmm_stem_stats_only(int dtype, const float* x, const void* packed, const float* bias, float* stats, int N, int Cin,
                          int H, int W, int R, void* stream);
int ecgmm_stem_pool_fwd(const float* x, const void* packed, const float* coef, void* pooled, uint8_t* idx, int N, int Cin,
                        int H, int W, void* stream);
size_t ecgmm_stem_pool_bwd_workspace(int N, int Cin, int H, int W);
int ecgmm_stem_pool_bwd(const float* x, const void* packed, const float* coef, const float* gamma, const void* dp,
                        const void* pooled, const uint8_t* idx, float* dgamma, float* dbeta, float* dw_oihw, void* ws,
                        size_t ws_bytes, int N, int Cin, int H, int W, void* stream);

/* nn.BatchNorm{1,2}d (train: batch mean / biased var, running update with unbiased var; eval: running
 * stats).  coef = [4][C]: scale, shift, mean, invstd.
 * Partial-sum buffers ([rows][2][C] floats, written by conv_fwd / stem_fwd / col_stats) must be
 * allocated with ECGMM_BN_TAIL_ROWS spare rows after `rows`: bn_finalize folds long buffers into
 * that tail before the final reduction. */
#define ECGMM_BN_TAIL_ROWS 64
int ecgmm_col_stats_rows(int dtype, int64_t M, int C);
int ecgmm_col_stats(int dtype, const void* x, int64_t M, int C, float* partial, void* stream);
int ecgmm_bn_finalize(const float* partial, int rows, int C, double count, const float* gamma, const float* beta,
                      float* running_mean, float* running_var, int64_t* num_batches_tracked, float momentum, float eps,
                      float* coef, void* stream);
int ecgmm_bn_eval_coef(int C, const float* gamma, const float* beta, const float* running_mean,
                       const float* running_var, float eps, float* coef, void* stream);
/* out = relu?( bn(y) * gate[n][c] + residual ), residual = res or res*rcoef.scale + rcoef.shift
 * (BasicBlock tail; BasicBlock1D tail with the SE gate, PMB:88-93) */
int ecgmm_bn_act(int dtype, const void* y, const float* coef, const void* res, const float* rcoef, const float* gate,
                 int rows_per_sample, int relu, void* out, int64_t M, int C, void* stream);
/* ecgmm_bn_finalize + ecgmm_bn_act as ONE launch: every workgroup of the activation pass folds the (<= 512) partial rows
 * itself -- no dependent finalize launch in between; workgroup 0 writes coef_out [4][C] (for the backward) and updates the
 * running statistics.  More rows / unsupported widths fall back to the two launches.  Same values. */
int ecgmm_bn_act_from_rows(int dtype, const void* y, const float* partial, int rows, double count, const float* gamma,
                           const float* beta, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                           float momentum, float eps, float* coef_out, const void* res, const float* rcoef,
                           const float* gate, int rows_per_sample, int relu, void* out, int64_t M, int C, void* stream);
/* BatchNorm backward with the ReLU mask / SE gate folded in:
 *   dz = [maskref > 0] * dout * gate[n][c] + addc[n][c];  dy, dgamma, dbeta; dz_out = masked dout;
 *   (maskref == y: the mask is recomputed as bn(y) > 0, saving the read of the activated tensor)
 *   dbias (nullable) = column sum of dy (Conv1d bias gradient). scratch: ecgmm_bn_bwd_scratch bytes */
size_t ecgmm_bn_bwd_scratch(int dtype, int64_t M, int C);
int ecgmm_bn_bwd(int dtype, const void* dout, const void* maskref, const float* gate, const float* addc,
                 int rows_per_sample, const void* y, const float* coef, const float* gamma, float* dgamma,
                 float* dbeta, void* dy, void* dz_out, float* dbias, int64_t M, int C, void* scratch, void* stream);
/* backward of a BatchNorm whose forward ran in eval mode (net.eval(): running statistics, a constant per-channel affine
 * map -- torch differentiates it the same way): one pass, operands as ecgmm_bn_bwd,
 *   g = [maskref > 0] * dout * [gate] + [addc],  dy = g * scale_c,  dbeta = sum g,  dgamma = sum g * (y - running_mean) * rstd,
 *   dbias = sum dy.  scratch (ecgmm_bn_bwd_scratch bytes) is needed only when one of the three sums is asked for. */
int ecgmm_bn_eval_bwd(int dtype, const void* dout, const void* maskref, const float* gate, const float* addc,
                      int rows_per_sample, const void* y, const float* coef, float* dgamma, float* dbeta, void* dy,
                      void* dz_out, float* dbias, int64_t M, int C, float* scratch, void* stream);

/* The same backward with its reduction pass fused into the convolution that PRODUCES dout (autograd of
 * conv -> BatchNorm -> ReLU chains: torchvision BasicBlock, multimodal_paper_modal_balance.py:210; train.py:80):
 * ecgmm_conv_bwd_data_bnred is ecgmm_conv_bwd_data that also accumulates, in its epilogue, the partial rows
 * (sum g, sum g * (bn_y - mean)) of g = [mask] * dx over the pixels, bn_mask == bn_y (or NULL): mask = (bn(bn_y) > 0)
 * and dx is stored unmasked; otherwise mask = (bn_mask > 0) and dx is stored MASKED.  rows: room for 512 x [2][Cin]
 * floats.  *nrows = rows written, or 0 when this geometry is not served by the fused kernel (dx is then the plain
 * gradient and the caller runs ecgmm_bn_bwd).  ecgmm_bn_bwd_from_rows finishes the backward from such rows
 * (finalize + apply; maskref as in ecgmm_bn_bwd, NULL for an already masked dout). */
int ecgmm_conv_bwd_data_bnred(int dtype, const ecgmm_conv_desc* c, const void* dy, const void* w_dgrad,
                              const void* addend, void* dx, const void* bn_y, const void* bn_mask, const float* bn_coef,
                              float* rows, int* nrows, void* stream);
/* rows a launch of ecgmm_conv_bwd_data_bnred writes for this geometry under the current settings (0: the fused form does
 * not apply and *nrows will be 0) -- for callers whose consumer runs in another call; follows ecgmm_conv_halo_cus */
int ecgmm_conv_bwd_data_bnred_rows(int dtype, const ecgmm_conv_desc* c);
/* Input gradient of a ResNet stage-entry block's two stride-2 branches in one launch (torchvision BasicBlock with
 * downsample; BasicBlock1D, multimodal_paper_modal_balance.py:71-93):  dx = dgrad(conv c, dy) + dgrad(1x1 stride-2 pad-0
 * conv of the same input, dy_down).  The 1x1 branch is one more tap of the stride-2 kernel's parity class (0,0); no
 * temporary is written.  c describes the main convolution (3x3 or 1x3, stride 2, pad <= 1); both gradients are
 * [N][OH][OW][Cout], w_down_dgrad is the 1x1 weight packed for dgrad.  tmp (same size as dx) is only used for geometries
 * the folded form does not serve; NULL is accepted when c has stride 2 and pad <= 1. */
int ecgmm_conv_bwd_data_with_downsample(int dtype, const ecgmm_conv_desc* c, const void* dy, const void* w_dgrad,
                                        const void* dy_down, const void* w_down_dgrad, void* dx, void* tmp,
                                        void* stream);
int ecgmm_bn_bwd_from_rows(int dtype, const void* dout, const void* maskref, const void* y, const float* coef,
                           const float* gamma, float* dgamma, float* dbeta, void* dy, const float* rows, int nrows,
                           int64_t M, int C, void* scratch, void* stream);

/* ResNet18 plan: a BatchNorm-backward reduction is fused into the producing dgrad's epilogue only for layers with at
 * least this many output pixels.  Default (and any negative m): never -- since round 3 the stream form of the layer-1 input
 * gradient plus the separate reduction pass is faster than the fused epilogue; 400000 = the 56x56 stage at batch >= 128
 * (round 2's default), 0 = wherever the halo kernel runs.  Start-up value: ECGMM_BN_FUSE_MIN_M.  Results differ by fp32
 * summation order only. */
int ecgmm_bn_fuse_min_pixels(int64_t m);
/* BatchNorm finalize folded into its consumer pass (every workgroup of bn_act / the backward's apply pass folds the <= 512
 * partial rows itself instead of a separate ~5 us launch in between; csrc/elementwise.hip): 1 = on (default), 0 = separate
 * launches.  Start-up value: ECGMM_BN_FOLD.  Same values up to the fp64 summation grouping of the partial rows. */
int ecgmm_bn_fold(int on);
/* Channel-sliced launch of those folded passes for C >= 256: a workgroup is a (pixel chunk, 128-channel slice) pair, folds
 * only its own 128 channels of the partial rows (one group instead of C / 128, one after the other) and walks 128-channel
 * row segments; at most 256 workgroups as before.  1 = on (default), 0 = every workgroup walks whole rows and folds all C
 * channels.  Start-up value: ECGMM_BN_FOLD_SLICE.  Bit-identical results (same fp64 summation order per channel). */
int ecgmm_bn_fold_slice(int on);
/* ecgmm_bn_act_from_rows that also writes the ReLU mask as bits (bf16 and relu != 0; relu_bits nullable): [M][C / 8] bytes,
 * bit j of byte [row][k] = (out[row][8 k + j] > 0), 1/16 of the activated tensor's bytes; and ecgmm_bn_bwd reading that
 * mask (bf16 only) instead of a mask tensor -- the pair the ResNet18 plan runs around each residual block's bn2. */
int ecgmm_bn_act_from_rows_bits(int dtype, const void* y, const float* partial, int rows, double count, const float* gamma,
                                const float* beta, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                                float momentum, float eps, float* coef_out, const void* res, const float* rcoef,
                                const float* gate, int rows_per_sample, int relu, void* out, uint8_t* relu_bits, int64_t M,
                                int C, void* stream);
int ecgmm_bn_bwd_bits(int dtype, const void* dout, const uint8_t* mask_bits, const float* gate, const float* addc,
                      int rows_per_sample, const void* y, const float* coef, const float* gamma, float* dgamma,
                      float* dbeta, void* dy, void* dz_out, float* dbias, int64_t M, int C, void* scratch, void* stream);
/* Two BatchNorm backwards of ONE masked gradient dz = [mask] * dout in one reduce + one apply pass -- bn2 (y_a, ...) and the
 * shortcut BatchNorm (y_b, ...) of a ResNet18 downsample block: dz is stored once and read once, two launches instead of
 * four.  Mask: mask_bits (bf16) or maskref > 0 (a tensor of its own, not y_a / y_b); one of them is required.  Bit-identical to
 *   ecgmm_bn_bwd(_bits)(dout, mask, ..., y_a, ..., dy_a, dz_out = dz)  followed by  ecgmm_bn_bwd(dz, no mask, ..., y_b, ..., dy_b).
 * gate, addc and dbias are not supported: ECGMM_ERR_SHAPE unless null.  scratch_a, scratch_b: one buffer per BatchNorm of
 * ecgmm_bn_bwd_scratch(dtype, M, C) bytes each (partial rows as ecgmm_bn_bwd leaves them in its scratch). */
int ecgmm_bn_bwd_dual(int dtype, const void* dout, const void* maskref, const uint8_t* mask_bits, const float* gate,
                      const float* addc, const void* y_a, const float* coef_a, const float* gamma_a, float* dgamma_a,
                      float* dbeta_a, void* dy_a, const void* y_b, const float* coef_b, const float* gamma_b,
                      float* dgamma_b, float* dbeta_b, void* dy_b, void* dz, float* dbias, int64_t M, int C, void* scratch_a,
                      void* scratch_b, void* stream);
/* ResNet18 plan, training backward of the downsample blocks: 1 = that dual pass pair (default), 0 = the two separate
 * BatchNorm backwards.  Run time only (no environment variable).  Bit-identical results. */
int ecgmm_bn_dual(int on);
/* ResNet18 plan: run the stem by recompute (ecgmm_stem_stats_only / stem_pool_fwd / stem_pool_bwd; bf16 only): 1 = on,
 * 0 = the two-pass route that keeps the full-resolution conv output (default: 0.2 ms per step faster at batch 256 although
 * it moves 1.6 GB more -- the recomputing kernels are instruction-bound).  Start-up value: ECGMM_STEM_RECOMPUTE.
 * It changes the plan's workspace layout: switch between steps, never between a forward and its backward. */
int ecgmm_stem_recompute(int on);

/* relu(bn(y)) -> MaxPool(3,2,1) (resnet18.maxpool; ResNet1D_SE.initial[3], PMB:103) and its backward */
int ecgmm_bnrelu_maxpool(int dtype, const void* y, const float* coef, void* out, uint8_t* idx, int N, int H, int W,
                         int C, void* stream);
int ecgmm_maxpool_relu_bwd(int dtype, const void* dp, const void* pooled, const uint8_t* idx, void* dz, int N, int H,
                           int W, int C, void* stream);
/* Backward of [BatchNorm -> ReLU -> MaxPool(3,2,1)] in one call, without the full-resolution pooled-gradient tensor: the
 * BatchNorm reduction runs over the pooled tensors (dp, pooled), the apply pass gathers the max-pool backward on the fly.
 * Same results as ecgmm_maxpool_relu_bwd + ecgmm_bn_bwd up to the rounding of `pooled` (header of the kernels in
 * csrc/elementwise.hip).  scratch: ecgmm_bn_bwd_scratch(dtype, N*H*W, C) bytes.  dbias nullable (sum of dy). */
int ecgmm_pool_bn_bwd(int dtype, const void* dp, const void* pooled, const uint8_t* idx, const void* y, const float* coef,
                      const float* gamma, float* dgamma, float* dbeta, void* dy, float* dbias, int N, int H, int W, int C,
                      void* scratch, void* stream);
/* AdaptiveAvgPool(1) (+ optional per-channel affine of the mean) and its broadcast backward */
int ecgmm_avgpool(int dtype, const void* x, float* out, int N, int R, int C, const float* coef, void* stream);
int ecgmm_bcast_rows(int dtype, const float* v, void* out, int N, int R, int C, float scale, void* stream);
int ecgmm_se_gate_grad(int dtype, const void* dout, const void* maskref, const void* y, const float* coef, float* dg,
                       int N, int R, int C, void* stream);
/* the first pass of the merged SE / BatchNorm backward the ResNet1D_SE plan runs, per op: ONE read of dout, maskref and y
 * [N][R][C] gives dz = [maskref > 0] * dout (stored, [N][R][C]), dg [N][C] (the sum of ecgmm_se_gate_grad) and the per-sample
 * sums a1 = sum_r dz, a2 = sum_r dz * (y - mean), a3 = sum_r (y - mean), each [N][C] fp32; coef [4][C] as ecgmm_bn_finalize
 * writes it. */
int ecgmm_se_gate_bn(int dtype, const void* dout, const void* maskref, const void* y, const float* coef, void* dz, float* dg,
                     float* a1, float* a2, float* a3, int N, int R, int C, void* stream);
/* SEBlock.fc (PMB:35-46) on the pooled means m [N][C], fp32, one kernel forward and two backward (the kernels the ResNet1D_SE
 * and inference plans use, whatever ECGMM_SE_MLP_FUSED says): h [N][CR] = relu(m W1^T + b1), g [N][C] = sigmoid(h W2^T + b2),
 * w1 [CR][C], w2 [C][CR].  Backward: ds [N][C] = dg * g * (1 - g) and dh [N][CR] = (ds W2) * [h > 0] are caller-provided
 * scratch that is written, dm [N][C] = (dh W1) * scale (scale = 1 / L: the mean over L), dw2 = ds^T h, db2 = sum_n ds,
 * dw1 = dh^T m, db1 = sum_n dh; each of dw1 / db1 / dw2 / db2 may be NULL (skipped).
 * ECGMM_ERR_SHAPE unless N >= 1, 1 <= C <= 1024, 1 <= CR <= 64. */
int ecgmm_se_mlp_fwd(const float* m, const float* w1, const float* b1, const float* w2, const float* b2, float* h, float* g,
                     int N, int C, int CR, void* stream);
int ecgmm_se_mlp_bwd(const float* dg, const float* g, const float* h, const float* m, const float* w1, const float* w2,
                     float* ds, float* dh, float* dm, float* dw1, float* db1, float* dw2, float* db2, int N, int C, int CR,
                     float scale, void* stream);

/* nn.Linear (+bias, +ReLU/Sigmoid) fp32: MFMA (exact f32) when the shape allows, VALU otherwise.
 * (clinical_encoder PMB:256-262, fusion_classifier PMB:283-289, branch heads PMB:269-271, SE fc PMB:53-58) */
int ecgmm_linear_fwd(const float* x, const float* w, const float* bias, float* y, int B, int In, int Out, int act,
                     void* stream);
size_t ecgmm_linear_bwd_scratch(int B, int In, int Out);
int ecgmm_linear_bwd(const float* dz, const float* x, const float* w, float* dx, float* dw, float* db, int B, int In,
                     int Out, void* scratch, size_t scratch_bytes, void* stream);
int ecgmm_act_bwd(const float* dy, const float* y, float* dz, int64_t n, int act, void* stream);

/* nn.LayerNorm (PMB:223,239,263) and AttentionFusion (PMB:31-46): softmax(weights) * feats -> cat ->
 * LayerNorm, one row kernel.  nseg = 1 (plain LN, fusion_w = NULL) or 3 (fusion). stat = [B][2]. */
int ecgmm_layernorm_fwd(const float* const* seg, const int* dims, int nseg, const float* fusion_w, const float* gamma,
                        const float* beta, float* out, float* stat, float* soft_w, int B, float eps, void* stream);
size_t ecgmm_layernorm_bwd_scratch(int B, int D);
int ecgmm_layernorm_bwd(const float* const* seg, const int* dims, int nseg, const float* fusion_w, const float* gamma,
                        const float* stat, const float* dout, float* const* dseg, int dseg_accumulate, float* dgamma,
                        float* dbeta, float* dfusion_w, int B, void* scratch, void* stream);

/* var_loss (PMB:349-352). scratch = (3*B + 4) floats, kept for the backward */
int ecgmm_varloss_fwd(const float* f0, const float* f1, const float* f2, int B, int D0, int D1, int D2, float* loss,
                      float* scratch, void* stream);
int ecgmm_varloss_bwd(const float* f, int B, int D, const float* gout, const float* scratch, int which, float* df,
                      int accumulate, void* stream);

/* nn.CrossEntropyLoss() (train.py:31) / FocalLoss (signal_model.py:91-106), mean reduction.
 * dcoef = [B] floats kept for the backward; labels are int64 */
int ecgmm_ce_fwd(const float* logits, const int64_t* labels, int B, int C, int focal, float alpha, float gamma,
                 float* loss, float* dcoef, void* stream);
int ecgmm_ce_bwd(const float* logits, const int64_t* labels, int B, int C, const float* dcoef, const float* gout,
                 float* dlogits, void* stream);
/* the step loss of train.py:69-78 in one launch per direction: loss = CrossEntropy(logits, labels) + extra_w * extra[0]
 * (extra = var_loss, extra_w = 0.1); backward: dlogits and dextra[0] = gout * extra_w */
int ecgmm_ce_plus_fwd(const float* logits, const int64_t* labels, int B, int C, const float* extra, float extra_w,
                      float* loss, float* dcoef, void* stream);
int ecgmm_ce_plus_bwd(const float* logits, const int64_t* labels, int B, int C, const float* dcoef, const float* gout,
                      float* dlogits, float* dextra, float extra_w, void* stream);

/* nn.Dropout (PMB:115,260,287): Philox4x32-10, keep-mask bytes saved for the backward */
int ecgmm_dropout_fwd(const float* x, float* y, uint8_t* mask, int64_t n, float p, uint64_t seed, uint64_t offset,
                      void* stream);
int ecgmm_dropout_bwd(const float* dy, const uint8_t* mask, float* dx, int64_t n, float p, void* stream);

/* torch.optim.Adam.step (train.py:43,81; betas/eps defaults; beta1 varies under OneCycleLR,
 * train_signal_12_af.py:250-252) over one contiguous fp32 run; gscale multiplies the gradient
 * (1/world_size after a summed all-reduce) */
int ecgmm_adam(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
               float weight_decay, int64_t step, float gscale, void* stream);
int ecgmm_axpby(float a, const float* x, float b, float* y, int64_t n, void* stream);

/* SURVEY 8(f1) -- the step in front of the hot path, on device: per-signal StandardScaler (optional,
 * per time column) -> moving-average baseline removal (np.convolve(x, ones(w)/w, 'same')) -> IIR
 * low-pass applied forward-backward exactly as scipy.signal.filtfilt(b, a, x) (odd padding 3*(order+1),
 * lfilter_zi initial conditions `zi`).  Replaces preprocess_signal: dataset.py:81-95,
 * train_signal_12_af.py:19-34.  x/out: [S][L] fp32 (S = batch * leads); fp64 arithmetic inside. */
size_t ecgmm_signal_preprocess_workspace(int S, int L, int order);
int ecgmm_signal_preprocess(const float* x, float* out, int S, int L, const float* sc_mean, const float* sc_scale,
                            int window, const double* b, const double* a, const double* zi, int order, void* ws,
                            size_t ws_bytes, void* stream);
/* The same pipeline straight from WFDB format-16 frames, one launch (replaces wfdb.rdsamp(path, channels) -> [::2] ->
 * remove_baseline_drift -> lowpass_filter -> crop or zero-pad, train_signal_only_ptb.py:40-53, per sample per epoch on CPU
 * workers).  raw: the .dat payload of R records, int16 [R][T][nsig] as on disk; chan: nc <= 16 channel numbers (host
 * memory, each < nsig); gain double [R][nc] and baseline int [R][nc] on the device.  Row (r, c) of out [R][nc][out_len]
 * fp32: sample t = frame t*step of channel chan[c], Lf = ceil(T / step) samples, decoded as wfdb's p_signal
 * (d - baseline) / gain in float64 with -32768 (the format's invalid-sample code) -> NaN, which poisons its own row only;
 * then the moving average and filtfilt of ecgmm_signal_preprocess; out[:min(Lf, out_len)] is the result and out[Lf:] is
 * exactly 0.0f.  One row stays resident in one CU's LDS, (2 Lf + 6 (order+1) + 576) * 8 bytes < 160 KiB (Lf <= 9933 at
 * order 5); a longer row is refused with ECGMM_ERR_SHAPE, there is no workspace route.  Everything is checked on the host
 * before the launch (chan[i] < nsig, Lf >= window, Lf > 3*(order+1), a[0] == 1, out_len >= 1). */
int ecgmm_signal_preprocess_i16(const int16_t* raw, int R, int T, int nsig, const int* chan, int nc, const double* gain,
                                const int* baseline, int step, float* out, int out_len, int window, const double* b,
                                const double* a, const double* zi, int order, void* stream);

/* PhysioNet-2017 single-lead path.  filtfilt + z-score of a whole [S][L] fp32 matrix in one launch: exactly
 * scipy.signal.filtfilt(b, a, x) (odd padding 3*(order+1), lfilter_zi initial conditions `zi`) for a general transfer
 * function b[0..order], a[0..order] (a[0] = 1, 1 <= order <= 8: the 4th-order Butterworth band-pass is order 8), then, when
 * `zscore` is set, (y - mean(y)) / (std(y) + eps) with the population standard deviation over the L samples.  fp64
 * arithmetic, fp32 result.  Replaces bandpass_filter + z_score_normalize = preprocess_signal, train_physionet.py:23-45,
 * train_physionet_multi.py:20-42.  One record stays resident in one CU's LDS: L <= 19904 - 6*(order+1) (19850 at
 * order 8), longer records are refused. */
int ecgmm_signal_filter_zscore(const float* x, float* out, int S, int L, const double* b, const double* a,
                               const double* zi, int order, int zscore, double eps, void* stream);
/* Accuracy contract of the three filtfilt entry points above (ecgmm_signal_preprocess, _i16, ecgmm_signal_filter_zscore): for
 * any order and cutoff the float64 arithmetic adds at most one fp32 half-ulp at the row's scale to scipy's sequential float64
 * filtfilt, wherever that itself is this accurate.  The kernels cut a record into chunks that run on nl lanes and chain the
 * chunk states; the chain loses digits for a narrow-band, high-order design, so nl = 64, 32, 16, 8, 4, 2 or 1 (the sequential
 * pass) is chosen on the host from (a, L) alone.  This returns the nl those entry points use for a record of L samples
 * (needs no GPU); 0 with the message set for a null a, a[0] != 1, an order outside 1..8 or L < 1. */
int ecgmm_signal_filter_lanes(const double* a, int order, int L);
/* resample_signal (train_physionet.py:35-39, train_physionet_multi.py:32-36) = scipy.signal.resample(x, num), the Fourier
 * method, for a whole [S][L] fp32 matrix (csrc/resample.hip): with X = rfft(x), m = min(N, num), K = m / 2 + 1,
 *   y[j] = (X[0] + sum_{1 <= k < K} w_k 2 Re(X[k] e^{2 pi i k j / num})) / N,
 * w_k = 1 except at k = m / 2 with m even, where the term is 2 Re X[k] (-1)^j (num < N) or Re X[k] cos(2 pi k j / num)
 * (num > N).  Two direct sums in fp64 through the workspace X [S][min(L, T_out) / 2 + 1] complex doubles, fp32 result; every
 * sum in a fixed order, no atomics: two calls give the same bits, and a row's bits depend on that row alone (not on S, its
 * neighbours or L).  num == N copies the row bit for bit.  Accuracy: tests/resample_bounds.py.
 *   without lengths  every row goes L -> num (1 <= num <= T_out); ratio is ignored; out_lengths must be null
 *   with lengths     device int32 [S], clamped to [0, L] on the device: row s is resampled over its first N_s = lengths[s]
 *                    samples to num_s = (int)((double)N_s * ratio) samples, ratio = target_fs / orig_fs as a double, which
 *                    is Python's int(len * (target_fs / orig_fs)); num must be 0 and T_out >= (int)(L * ratio);
 *                    out_lengths (nullable, device int32 [S]) receives num_s; x at and beyond N_s is never read (NaN allowed)
 * out [S][T_out] is exactly 0 from num_s on; a row with N_s = 0 or num_s = 0 is all zeros.  With all lengths equal to L the
 * bits are those of the call without lengths and num = (int)(L * ratio).
 * Needs S >= 1 and 1 <= L, T_out <= 65536, a 16-byte aligned workspace of ecgmm_signal_resample_workspace bytes (no GPU
 * needed; 0 with the message set when refused), a finite ratio > 0 with lengths; anything else (null x / out / ws included)
 * is ECGMM_ERR_SHAPE before any launch, and nothing is written.
 * ecgmm_signal_resample_len (no GPU needed): (int)((double)n * ratio), the length of the resampled record; -1 with the
 * message set for n < 0, a ratio that is not finite and > 0, or a result beyond an int. */
/* train_physionet.py:35-39: num = int(len(signal) * (target_fs / orig_fs)) */
int ecgmm_signal_resample_len(int n, double ratio);
/* train_physionet.py:35-39 */
size_t ecgmm_signal_resample_workspace(int S, int L, int T_out);
/* train_physionet.py:35-39: resample(signal, num) */
int ecgmm_signal_resample(const float* x, int S, int L, const int32_t* lengths, int num, double ratio, float* out, int T_out,
                          int32_t* out_lengths, void* ws, size_t ws_bytes, void* stream);
/* The per-step batch gather fused with augment_signal (train_physionet.py:47-60): out[i][:] = augment(src[index[i]][:]),
 * src [n][L] fp32, index int64 [B], out [B][L] fp32.  augment = 0: the plain gather.  augment = 1, per row i: three
 * Bernoulli(p) decisions in the reference's order -- add N(0, sigma^2) noise per sample point; multiply by a uniform on
 * [scale_lo, scale_hi); circular roll out[(t + shift) mod L] = v[t] by an integer uniform on [shift_lo, shift_hi).
 * Philox4x32-10 keyed by `seed`; the counter is (offset, i, element group), so row i's result does not depend on B, on
 * the launch geometry or on the other rows; the caller advances `offset` by one per call.
 * decisions (nullable) [B][4] fp32: noise flag, scale (1 when not drawn), shift (0 when not drawn), the three decisions as
 * bits (1 noise, 2 scale, 4 roll).  A row whose index is outside [0, n) is filled with NaN and never addresses memory. */
int ecgmm_signal_gather_augment(const float* src, int64_t n, int L, const int64_t* index, int B, float* out,
                                float* decisions, int augment, float p, float sigma, float scale_lo, float scale_hi,
                                int shift_lo, int shift_hi, uint64_t seed, uint64_t offset, void* stream);
/* WeightedRandomSampler(weights, count, replacement=True) = torch.multinomial with replacement
 * (train_signal_only_ptb.py:230-235,241), one launch per epoch.  cdf: the inclusive prefix sum of the n weights in float64
 * (device); out int64 [count]; u_out (nullable) double [count], the uniform each draw used.  Draw i takes Philox4x32-10 keyed
 * by `seed` at counter (offset, i, 0xFFFFFFFD), u = ((w0 >> 5) * 2^26 + (w1 >> 6)) * 2^-53, and returns the first j with
 * cdf[j] > u * cdf[n-1] (binary search); where rounding leaves no such j it returns last_positive, the last index of positive
 * weight.  An index of weight 0 is never returned, and draw i depends on (seed, offset, i) alone.  The caller advances
 * `offset` by one per call.  torch's own random stream is not reproduced. */
int ecgmm_weighted_sample(const double* cdf, int64_t n, int64_t last_positive, int64_t* out, double* u_out, int64_t count,
                          uint64_t seed, uint64_t offset, void* stream);

/* SURVEY 8(f3) -- the TabNet clinical encoder of multimodal.py:109-148 (pytorch_tabnet.tab_network.TabNetNoEmbeddings:
 * third-party, source and version absent from the reference; restated from its published algorithm).  Row kernels,
 * fp32: GLU gate out = z[:, :D] * sigmoid(z[:, D:]) of a [N, 2D] tensor; sparsemax along rows of [N, D], D <= 64;
 * elementwise helpers of the mask / prior recurrence; mean_n sum_d M log(M + eps). */
enum { ECGMM_EW_MUL = 0, ECGMM_EW_ADD_SCALE = 1, ECGMM_EW_PRIOR = 2, ECGMM_EW_RELU = 3, ECGMM_EW_RELU_BWD = 4,
       ECGMM_EW_SCALE = 5, ECGMM_EW_NEG_MUL = 6, ECGMM_EW_ADD = 7, ECGMM_EW_RSUB = 8 };
int ecgmm_glu_fwd(const float* z, float* out, int64_t N, int D, void* stream);
int ecgmm_glu_bwd(const float* z, const float* dout, float* dz, int64_t N, int D, void* stream);
int ecgmm_sparsemax_fwd(const float* x, float* p, int64_t N, int D, void* stream);
int ecgmm_sparsemax_bwd(const float* p, const float* dp, float* dx, int64_t N, int D, void* stream);
int ecgmm_ew(int op, const float* a, const float* b, float* out, int64_t n, float s, void* stream);
/* x [N, D] -> d = x[:, :nd] (through ReLU when relu != 0), a = x[:, nd:]; bwd merges (gd / ga may be NULL = zero) */
int ecgmm_split_cols(const float* x, float* d, float* a, int64_t N, int D, int nd, int relu, void* stream);
int ecgmm_split_cols_bwd(const float* d, const float* gd, const float* ga, float* gx, int64_t N, int D, int nd, int relu,
                         void* stream);
/* BatchNorm1d over the rows of a small [N, C] fp32 matrix, any C (one block per channel): the 2- / 64- / 128-wide
 * (ghost) batch norms of TabNet.  save = [2][C] mean, invstd.  accumulate != 0 adds into dgamma / dbeta.
 * gamma / beta NULL = 1 / 0.  training != 0: batch statistics; rm / rv (both or neither) take the momentum update with the
 * unbiased variance and *nbt (nullable) goes up by one with it; N == 1 is refused with ECGMM_ERR_SHAPE as torch refuses one
 * value per channel (nothing is written).  training == 0 needs rm / rv and changes neither them nor *nbt. */
int ecgmm_bn_small_fwd(const float* x, const float* gamma, const float* beta, float* rm, float* rv, long long* nbt,
                       float* y, float* save, int N, int C, int training, float momentum, float eps, void* stream);
int ecgmm_bn_small_bwd(const float* x, const float* dy, const float* gamma, const float* save, float* dx, float* dgamma,
                       float* dbeta, int N, int C, int accumulate, void* stream);
/* the same behind an eval-mode forward (save = running mean, invstd): dx = dy * gamma * invstd (dx may be NULL) */
int ecgmm_bn_small_eval_bwd(const float* x, const float* dy, const float* gamma, const float* save, float* dx,
                            float* dgamma, float* dbeta, int N, int C, int accumulate, void* stream);
int ecgmm_entropy_fwd(const float* M, float* out, int64_t N, int D, float eps, void* stream);
int ecgmm_entropy_bwd(const float* M, const float* g, float* dM, int64_t N, int D, float eps, void* stream);

/* SURVEY 8(f1), image half: Resize((OH, OW)) -> ToTensor -> Normalize(mean, std) of decoded RGB pictures
 * (dataset.py:61,119-123; train_image_only.py:58-62; dataset_image.py:67-70 when OH==H && OW==W).
 * torchvision hands a PIL picture to Pillow's antialiased BILINEAR resample (8 bpc, two passes, 22-bit
 * fixed-point coefficients, uint8 intermediate); the result is bit-identical to Pillow followed by
 * float32 x/255 and (x-mean)/std.  img: uint8 [B][H][W][3] on the device; out: fp32 [B][3][OH][OW].
 * The coefficient table is built on the host (tables_bytes / tables) and copied to the device by the
 * caller once per (H, W, OH, OW); it is not needed (may be NULL) when no resize takes place. */
size_t ecgmm_image_resize_tables_bytes(int H, int W, int OH, int OW);
int ecgmm_image_resize_tables(int H, int W, int OH, int OW, void* host_tables, size_t bytes);
int ecgmm_image_transform(const void* img, float* out, int B, int H, int W, int OH, int OW, const void* dev_tables,
                          size_t table_bytes, const float* mean3, const float* std3, void* stream);

/* Measurement only (no reference counterpart): HIP-event timing of the conv kernels on their launch
 * stream.  kinds: 0 igemm fwd, 1 igemm dgrad, 2 wgrad, 3 stem fwd, 4 stem wgrad, 5 / 6 igemm fwd / dgrad of the exact-fp32
 * instantiation.  collect()
 * synchronises the recorded events and returns per-kind total ms / algorithmic FLOPs / algorithmic
 * HBM bytes / launches.  enable(1) times every kind, enable(2) only kinds 0 and 1, enable(3) only kinds 5 and 6, enable(0) switches it off. */
int ecgmm_prof_enable(int on);
/* pause(1) suspends the bracketing, pause(0) resumes it; recorded launches are kept (bench.py samples steps). */
int ecgmm_prof_pause(int paused);
int ecgmm_prof_collect(int nkinds, double* ms, double* flops, double* bytes, int64_t* count);
/* Diagnostic step timeline: with ecgmm_tl_enable(1) the ResNet18 plan records a timestamped event on the caller's stream at
 * every phase boundary (ids 100.. forward: 100 start, 101 stem, 102..109 blocks, 110 end; 200.. backward: 200 start, 201 fc,
 * 202..209 blocks 7..0, 210 stem, 211 joined); ecgmm_tl_mark adds the host's own marks; ecgmm_tl_collect returns ids and
 * milliseconds since the first mark and clears the list. */
int ecgmm_tl_enable(int on);
int ecgmm_tl_mark(int id, void* stream);
int ecgmm_tl_collect(int cap, int* ids, float* ms);

/* ---- per-op pieces of the inference plans ----
 * F.relu(F.conv2d(x, w, bias) + addend) as ONE launch -- what torchvision's BasicBlock does in three modules (conv2, bn2
 * folded into w / bias, `out += identity; out = self.relu(out)`) and PMB:84-93 in the 1-D blocks.  bias [Cout] fp32 and
 * addend (the shape and dtype of y) are nullable; act = ECGMM_ACT_NONE or ECGMM_ACT_RELU; no statistics. */
int ecgmm_conv_fwd_fused(int dtype, const ecgmm_conv_desc* c, const void* x, const void* w_fwd, const float* bias,
                         const void* addend, void* y, int act, void* stream);
/* nn.BatchNorm2d / nn.BatchNorm1d in eval mode behind a convolution (torchvision BasicBlock bn1 / bn2 / downsample.1,
 * PMB:72,75,82,100) folded into it: scale = gamma / sqrt(running_var + eps); w_out = w * scale[cout] (fp32 product, rounded
 * once to dtype), packed as layout 0 = the forward pack of ecgmm_pack_conv_weight ([Cout][RS][Cin]) or 1 = ecgmm_stem_pack
 * (Cout = 64, RS = kernel rows 1 or 7); b_out = beta + (conv_bias - running_mean) * scale, fp32.  conv_bias and scale_out
 * (the scale the kernel used, [Cout] fp32) are nullable. */
int ecgmm_fold_conv_bn(int dtype, int layout, const float* w, const float* conv_bias, const float* gamma, const float* beta,
                       const float* running_mean, const float* running_var, float eps, void* w_out, float* b_out,
                       float* scale_out, int Cout, int Cin, int RS, void* stream);
/* nn.ReLU + nn.MaxPool2d(3, 2, 1) (torchvision resnet stem) / nn.MaxPool1d(3, 2, 1) (PMB:103, H = 1) of a channels-last
 * tensor: ecgmm_bnrelu_maxpool without coefficients and without the argmax bytes.  C: any multiple of 8 (bf16) / 4 (fp32). */
int ecgmm_relu_maxpool(int dtype, const void* y, void* out, int N, int H, int W, int C, void* stream);
/* out = relu(y * gate[row / rows_per_sample][c] + res): `out = self.se(out); out += identity; out = self.relu(out)`,
 * PMB:88-92, with bn2 already folded into y.  out may be y. */
int ecgmm_gate_res_relu(int dtype, const void* y, const float* gate, const void* res, void* out, int64_t M, int C,
                        int rows_per_sample, void* stream);

/* ---------------------------------------------------------------------------------------------
 * nn.LSTM(In, H, num_layers, batch_first, bidirectional) with bias, fp32 (train_physionet2.py:75-76,94: the CRNN's
 * nn.LSTM(512, 200, num_layers=3, batch_first=True, bidirectional=True)).  Gate order i, f, g, o; the reverse direction
 * walks t = T-1 .. 0; the output is [fwd | rev] along features; layer l > 0 reads the D*H wide output of layer l-1.
 * H <= 384 (the LDS budget of the recurrence kernels), layers <= 8.
 *   x [B,T,In] (batch_first = 1) or [T,B,In] (0: rows are indexed t*B + b, no transposing copy); y likewise, D*H wide.
 *   params / grads: torch's _flat_weights order -- per layer, per direction: w_ih [4H,In_l], w_hh [4H,H], b_ih, b_hh [4H].
 *   h0, c0, hn, cn, dhn, dcn, dh0, dc0: [layers*D, B, H]; h0 / c0 null = zeros; hn / cn nullable.
 * save_for_backward = 1 keeps the activated gates, c_t and h_{t-1} of every layer and direction in the forward
 * workspace, which ecgmm_lstm_backward only READS; 0 keeps nothing beyond the layer outputs (smaller workspace).
 * Backward: dy, dhn, dcn each nullable (zero cotangent); dx, dh0, dc0 and every grads entry nullable (not computed);
 * gradients are WRITTEN, reductions in a fixed order.  The workspace queries need no GPU and return 0 on a bad
 * descriptor (ecgmm_last_error() says why). */
typedef struct {
  int B, T, In, H, layers, bidirectional, batch_first, save_for_backward;
} ecgmm_lstm_desc;
/* train_physionet2.py:75-76,94 */
size_t ecgmm_lstm_fwd_workspace(const ecgmm_lstm_desc* d);
/* train_physionet2.py:75-76,94 (its loss.backward()) */
size_t ecgmm_lstm_bwd_workspace(const ecgmm_lstm_desc* d);
/* train_physionet2.py:75-76,94: x, (h_n, c_n) = self.lstm(x) */
int ecgmm_lstm_forward(const ecgmm_lstm_desc* d, const float* x, const float* const* params, const float* h0,
                       const float* c0, float* y, float* hn, float* cn, void* ws, size_t ws_bytes, void* stream);
/* train_physionet2.py:75-76,94: the nn.LSTM part of loss.backward() */
int ecgmm_lstm_backward(const ecgmm_lstm_desc* d, const float* x, const float* const* params, const float* h0,
                        const float* c0, const float* dy, const float* dhn, const float* dcn, const void* ws, float* dx,
                        float* const* grads, float* dh0, float* dc0, void* scratch, size_t scratch_bytes, void* stream);
/* Variable-length form: x stays padded ([B,T,In] or [T,B,In]) and lengths [B] (device int32) says where each row ends.
 * It equals pad_packed_sequence(lstm(pack_padded_sequence(x, lengths, enforce_sorted=False), hx), total_length=T) for
 * every layer and direction, as a masked hold: at step t row b is live iff t < lengths[b], in both directions.
 *   live row            the cell of ecgmm_lstm_forward.
 *   dead row, forward   h and c keep their values and y[b,t] = 0.  The reverse direction so carries h0 / c0 untouched down
 *                       to t = lengths[b]-1 and starts there; hn / cn are the states after the row's last live step
 *                       (t = lengths[b]-1 forward, t = 0 reverse).
 *   dead row, backward  gate gradients are exact zeros, the dh / dc carries pass through, dy there is ignored: dx is exactly
 *                       zero at padded positions and no parameter gradient sees them.
 * lengths are clamped to [0, T] on the device (no host sync).  A length-0 row gives y = 0, hn = h0, cn = c0, dx = 0,
 * dh0 = dhn, dc0 = dcn.  lengths = null is exactly ecgmm_lstm_forward / ecgmm_lstm_backward, bit for bit (the same
 * kernels); so is, in value, lengths all equal to T.  The backward takes the lengths the forward ran with.
 * A slice of 16 consecutive batch rows runs only max(lengths of the slice) recurrence steps.  Rows ordered by length so save
 * CU time (short slices retire early), NOT latency while every slice has a CU of its own: a layer lasts as long as its
 * longest slice, and at B = 256 no gain was measured; latency only beyond 2048 rows per direction pair or with
 * other work on the idle CUs.  The projection and gradient GEMMs stay over all B*T rows, where padded x is multiplied by exact
 * zeros: PADDED x MUST BE FINITE (dy at padded positions is never read into arithmetic and may be anything).
 * Workspace and scratch sizes are those of ecgmm_lstm_fwd_workspace / ecgmm_lstm_bwd_workspace. */
/* train_physionet2.py:94-95: x, (h_n, c_n) = self.lstm(x) on records of unequal length */
int ecgmm_lstm_forward_varlen(const ecgmm_lstm_desc* d, const float* x, const int32_t* lengths, const float* const* params,
                              const float* h0, const float* c0, float* y, float* hn, float* cn, void* ws, size_t ws_bytes,
                              void* stream);
/* train_physionet2.py:94-95: the nn.LSTM part of loss.backward() on records of unequal length */
int ecgmm_lstm_backward_varlen(const ecgmm_lstm_desc* d, const float* x, const int32_t* lengths, const float* const* params,
                               const float* h0, const float* c0, const float* dy, const float* dhn, const float* dcn,
                               const void* ws, float* dx, float* const* grads, float* dh0, float* dc0, void* scratch,
                               size_t scratch_bytes, void* stream);
/* The same four calls with a compute dtype for the RECURRENT products; lengths nullable (null: the fixed-length kernels).
 * ECGMM_F32 runs exactly the code behind the entry points above: the same bits and the same workspace sizes.
 * ECGMM_BF16 changes only the recurrent products, which run on v_mfma_f32_16x16x32_bf16 with W_hh held on chip (registers
 * and LDS) for all T steps where it fits (H <= 208; above that part of it streams from a bf16 copy in the workspace):
 *   forward   pre_t = P_t + b_hh + bf(h_{t-1}) bf(W_hh)^T, P_t = x_t W_ih^T + b_ih the exact-fp32 projection as above.
 *             bf() is round-to-nearest-even to bf16; h0 is rounded as an operand the same way.  The products are exact, the
 *             sums fp32 in the MFMA accumulator in the kernel's fixed order (K-steps of 32 ascending; K zero-padded).  The
 *             gate functions, c_t, h_t, y, hn, cn are fp32 as above; y and the saved h_{t-1} are the UNROUNDED h; c is
 *             never rounded.
 *   backward  dh_{t-1} = dy_{t-1} + bf(dgates_t) bf(W_hh); the cell arithmetic is that of the fp32 kernel; the stored dgates
 *             are the unrounded fp32 values, and dW_ih, dW_hh, dx, db are the exact-fp32 GEMMs / row sums over them, the
 *             layer input and the saved h_{t-1}, as above (db_ih and db_hh bit-identical to each other).
 *   lengths   the masked hold described above, unchanged: exact zeros in the padding, hn / cn after the row's last own
 *             step, padded x finite.
 * Two identical calls give identical bits.  The bf16 workspaces are larger than the fp32 ones by the packed bf(W_hh)
 * (written by every call from the fp32 parameters; nothing is cached between calls).  A dtype other than the two, like H
 * above 384, is ECGMM_ERR_SHAPE (the workspace queries return 0) with ecgmm_last_error() set. */
size_t ecgmm_lstm_fwd_workspace_dt(const ecgmm_lstm_desc* d, int dtype);
size_t ecgmm_lstm_bwd_workspace_dt(const ecgmm_lstm_desc* d, int dtype);
/* train_physionet2.py:94-95: x, (h_n, c_n) = self.lstm(x), recurrence in `dtype` */
int ecgmm_lstm_forward_dt(const ecgmm_lstm_desc* d, int dtype, const float* x, const int32_t* lengths,
                          const float* const* params, const float* h0, const float* c0, float* y, float* hn, float* cn,
                          void* ws, size_t ws_bytes, void* stream);
/* train_physionet2.py:94-95: the nn.LSTM part of loss.backward(), recurrence in `dtype` (that of the forward) */
int ecgmm_lstm_backward_dt(const ecgmm_lstm_desc* d, int dtype, const float* x, const int32_t* lengths,
                           const float* const* params, const float* h0, const float* c0, const float* dy, const float* dhn,
                           const float* dcn, const void* ws, float* dx, float* const* grads, float* dh0, float* dc0,
                           void* scratch, size_t scratch_bytes, void* stream);
/* Where a saved tensor lies (needs no GPU; for tests).  which = "gates" (activated gates [B T][4H]), "c" (c_t [B T][H]),
 * "hprev" (h_{t-1} [B T][H]), "out" (output of layer < layers-1, [B T][D H], both directions): byte offset and size inside
 * the forward workspace of a save_for_backward = 1 descriptor; "dgates" ([B T][4H] of `direction`): inside the backward
 * scratch, holding the LAST layer processed (layer 0), so meaningful for single-layer calls.  Rows are ordered as x. */
int ecgmm_lstm_ws_view(const ecgmm_lstm_desc* d, int dtype, const char* which, int layer, int direction, size_t* offset,
                       size_t* bytes);
/* train_physionet2.py:94-95: x.mean(dim=1) over each row's own steps: out[b,c] = sum_{t < len_b} x[b,t,c] / len_b, x [B,T,C]
 * fp32, lengths [B] device int32 clamped to [0, T]; len_b = 0 gives 0.  Any C >= 1; the sum runs t = 0, 1, ... in order. */
int ecgmm_seq_mean_varlen_fwd(const float* x, const int32_t* lengths, float* out, int B, int T, int C, void* stream);
/* train_physionet2.py:94-95 (its loss.backward()): dx[b,t,c] = t < len_b ? dy[b,c] / len_b : 0 (exact zeros). */
int ecgmm_seq_mean_varlen_bwd(const float* dy, const int32_t* lengths, float* dx, int B, int T, int C, void* stream);

/* ---------------------------------------------------------------------------------------------
 * CRNN convolutional front end, per-op (train_physionet2.py:55-65, 87-93): three ConvBlocks
 * Conv2d(k = 5, pad = 2, bias) -> BatchNorm2d -> ReLU -> MaxPool2d(2) on a log-spectrogram [B, 1, F, T].  Activations are
 * channels-last with H = frequency, W = time.  Forward and input gradient of the 32 -> 64 and 64 -> 128 convolutions are
 * ecgmm_conv_fwd / ecgmm_conv_fwd_wgrows / ecgmm_conv_bwd_data at R = S = 5, pad 2 (weights from ecgmm_pack_conv_weight,
 * RS = 25); the entry points below are the pieces those do not cover.  ecgmm_conv_bwd_weight goes on refusing 25 taps.
 * Every split reduction is a fixed-order second pass (no float atomics): results are run-to-run identical.
 * ------------------------------------------------------------------------------------------- */
/* train_physionet2.py:59 with in_channels = 1 (line 70): x [N,H,W] fp32 (Cin = 1: NCHW == NHWC), w_oihw [32,1,5,5] fp32,
 * bias [32] (nullable) -> y [N,H,W,32] compute dtype.  ECGMM_BF16 rounds x and w to bf16; products and sums are fp32.
 * stats (nullable): ecgmm_conv5_in1_stats_rows(N,H,W) BatchNorm partial rows [2][32] (+ ECGMM_BN_TAIL_ROWS spare rows). */
int ecgmm_conv5_in1_stats_rows(int N, int H, int W);
int ecgmm_conv5_in1_fwd(int dtype, const float* x, const float* w_oihw, const float* bias, void* y, float* stats, int N, int H,
                        int W, void* stream);
/* train_physionet2.py:59, 70 (its loss.backward()): dw_oihw [32,1,5,5] and dbias [32] fp32 (either nullable) from x and
 * dy [N,H,W,32] (compute dtype).  accumulate != 0 adds into both.  The input gradient is ecgmm_conv5_in1_bwd_data. */
size_t ecgmm_conv5_in1_bwd_weight_workspace(int N, int H, int W);
int ecgmm_conv5_in1_bwd_weight(int dtype, const float* x, const void* dy, float* dw_oihw, float* dbias, int accumulate, void* ws,
                               size_t ws_bytes, int N, int H, int W, void* stream);
/* train_physionet2.py:59, 70 (what spectrogram.requires_grad_() gives there): the input gradient
 *   dx[n][h][w] = sum_{co < 32} sum_{r,s < 5} dy[n][h+2-r][w+2-s][co] * w[co][0][r][s],   taps outside the image dropped.
 * dy [N,H,W,32] compute dtype (16-byte aligned), w_oihw [32,1,5,5] fp32 (rounded to bf16 under ECGMM_BF16, as the forward
 * rounds it), dx [N,H,W] fp32 (Cin = 1: NCHW == NHWC, the spectrogram's own layout).  Products and sums are fp32 in a
 * fixed order, no atomics; every element of dx is written.  Refused like ecgmm_conv5_in1_fwd: dtype, bad input, null.
 * ecgmm_conv5_in1_bwd_data_tile: the kernel's tiling at height H (each nullable): columns of a strip, rows of a trip, rows
 * of a workgroup -- for tests and tools that want shapes across its boundaries; needs no GPU. */
int ecgmm_conv5_in1_bwd_data(int dtype, const void* dy, const float* w_oihw, float* dx, int N, int H, int W, void* stream);
void ecgmm_conv5_in1_bwd_data_tile(int H, int* strip, int* row_step, int* rows);
/* train_physionet2.py:59, 71-72 (their loss.backward()): weight gradient of a 5x5, stride 1, pad 2 convolution with Cin and
 * Cout multiples of 32: dw_oihw [Cout,Cin,5,5] fp32 from x [N,H,W,Cin] and dy [N,H,W,Cout] (compute dtype).  accumulate as
 * in ecgmm_conv_bwd_weight.  The workspace query needs no GPU and returns 0 on a descriptor it does not serve. */
size_t ecgmm_conv5_bwd_weight_workspace(int dtype, const ecgmm_conv_desc* c);
int ecgmm_conv5_bwd_weight(int dtype, const ecgmm_conv_desc* c, const void* x, const void* dy, float* dw_oihw, int accumulate,
                           void* ws, size_t ws_bytes, void* stream);
/* train_physionet2.py:60-62: relu(bn(y)) -> MaxPool2d(2), floor semantics (the last row / column of an odd extent is
 * dropped); ties go to the first element of the window in row-major order, as torch.  y [N,H,W,C] compute dtype, coef [4][C]
 * (ecgmm_bn_finalize / ecgmm_bn_eval_coef), C = 32, 64, 128 or 256.  out [N,H/2,W/2,C] compute dtype, or with
 * seq_layout != 0 the LSTM's input seq[n][w][c * (H/2) + h] fp32 (permute(0,3,1,2) + Flatten(2), train_physionet2.py:92-93).
 * idx [N,H/2,W/2,C] (nullable): position of the winner in its window, 2 * row + column. */
int ecgmm_bnrelu_maxpool2(int dtype, const void* y, const float* coef, void* out, uint8_t* idx, int N, int H, int W, int C,
                          int seq_layout, void* stream);
/* train_physionet2.py:60-62 (their loss.backward()): backward of [BatchNorm -> ReLU -> MaxPool2d(2)].  dp = gradient of the
 * pooled output in the layout ecgmm_bnrelu_maxpool2 wrote it (seq_layout: fp32).  training != 0: batch-statistics form, the
 * reductions run over all N H W conv outputs (rows / columns the floor dropped receive no pooled gradient but count);
 * training == 0: the affine form behind an eval-mode forward (as ecgmm_bn_eval_bwd).  dgamma, dbeta [C], dy [N,H,W,C]
 * (compute dtype) and dbias [C] (= column sum of dy: the convolution's bias gradient) are each nullable. */
size_t ecgmm_pool2_bn_bwd_workspace(int N, int H, int W, int C);
int ecgmm_pool2_bn_bwd(int dtype, const void* dp, const uint8_t* idx, const void* y, const float* coef, int training,
                       float* dgamma, float* dbeta, void* dy, float* dbias, int N, int H, int W, int C, int seq_layout,
                       void* ws, size_t ws_bytes, void* stream);

/* The three blocks as ONE call per direction (train_physionet2.py:55-65, 87-93: conv1..conv3 of CRNN, permute, Flatten).
 * spec [B,1,F,T] fp32; params (12): per block conv weight [cout,cin,5,5], conv bias, bn weight, bn bias (cout = 32, 64,
 * 128); buffers (9): per block running_mean, running_var, num_batches_tracked (int64); seq_out [B, T/8, 128 * (F/8)] fp32.
 * training = 0 uses the running statistics; a backward behind it is the affine form.  grads[i] == NULL skips a parameter;
 * gradients are WRITTEN.  The forward workspace is only read by the backward.  F < 8, T < 8, an unknown dtype or a short
 * workspace are refused with a message; the workspace queries need no GPU and return 0 on a bad descriptor. */
typedef struct {
  int B, F, T, dtype, training;
  float bn_momentum, bn_eps;
} ecgmm_crnn_front_desc;
/* train_physionet2.py:55-65, 87-93 */
size_t ecgmm_crnn_front_fwd_workspace(const ecgmm_crnn_front_desc* d);
size_t ecgmm_crnn_front_bwd_workspace(const ecgmm_crnn_front_desc* d);
int ecgmm_crnn_front_forward(const ecgmm_crnn_front_desc* d, const float* spec, const void* const* params,
                             void* const* buffers, float* seq_out, void* ws, size_t ws_bytes, void* stream);
/* train_physionet2.py:55-65, 87-93 (their loss.backward()); the spectrogram's own gradient: ecgmm_crnn_front_backward_dx */
int ecgmm_crnn_front_backward(const ecgmm_crnn_front_desc* d, const float* spec, const float* dseq, const void* const* params,
                              void* const* grads, void* ws_fwd, void* ws_bwd, size_t ws_bwd_bytes, void* stream);
/* The same with the input gradient (train_physionet2.py:55-65, 87-93 with spectrogram.requires_grad_()): dspec [B,1,F,T]
 * fp32, written whole.  dspec == NULL is ecgmm_crnn_front_backward: same launches, same bits.  Works behind a training-mode
 * and an eval-mode forward; the workspace and its query are ecgmm_crnn_front_bwd_workspace's.  With every grads[i] NULL (or
 * grads NULL) no weight-gradient kernel runs: the chain of input gradients alone. */
int ecgmm_crnn_front_backward_dx(const ecgmm_crnn_front_desc* d, const float* spec, const float* dseq,
                                 const void* const* params, void* const* grads, void* ws_fwd, void* ws_bwd,
                                 size_t ws_bwd_bytes, float* dspec, void* stream);

/* ---- inference forms of the CRNN front end: every BatchNorm folded into its convolution (eval mode, no backward) ----
 * nn.ReLU + nn.MaxPool2d(2) (train_physionet2.py:61-62) behind a convolution that already carries its BatchNorm:
 * ecgmm_bnrelu_maxpool2 without coefficients and without argmax bytes, out = max(0, max of the 2x2 window), floor
 * semantics.  y [N,H,W,C] compute dtype; out [N,H/2,W/2,C] compute dtype or, with seq_layout != 0, the fp32 LSTM layout
 * seq[n][w][c * (H/2) + h].  C: any multiple of 8 (bf16) / 4 (fp32); y (and a channels-last out) 16-byte aligned.
 * A bad dtype, H < 2, W < 2 and null operands are refused with a message. */
int ecgmm_relu_maxpool2(int dtype, const void* y, void* out, int N, int H, int W, int C, int seq_layout, void* stream);
/* train_physionet2.py:57-62 of the first block, BatchNorm folded into w / bias: Conv2d(1, 32, 5, pad 2) + bias + ReLU +
 * MaxPool2d(2) as ONE kernel.  x [N,H,W] fp32, w_oihw [32,1,5,5] fp32 (rounded to bf16 under ECGMM_BF16, as
 * ecgmm_conv5_in1_fwd rounds it), bias [32] fp32 (nullable), out [N,H/2,W/2,32] compute dtype (16-byte aligned).  Bit for
 * bit ecgmm_conv5_in1_fwd(stats = NULL) followed by ecgmm_relu_maxpool2 (for finite weights), without the [N,H,W,32]
 * tensor: no conv output of a row / column the floor drops is computed.  H, W >= 2. */
int ecgmm_conv5_in1_relu_pool2(int dtype, const float* x, const float* w_oihw, const float* bias, void* out, int N, int H,
                               int W, void* stream);
/* ecgmm_fold_conv_bn for a 5x5 convolution (25 taps): layout 0 = the forward pack [Cout][25][Cin] in the compute dtype
 * (what ecgmm_conv_fwd_fused reads), layout 1 = OIHW fp32 whatever the dtype (what ecgmm_conv5_in1_* read: those kernels
 * round their operands themselves, so that stays the single rounding).  Same formulas, same nullable operands. */
int ecgmm_fold_conv5_bn(int dtype, int layout, const float* w, const float* conv_bias, const float* gamma, const float* beta,
                        const float* running_mean, const float* running_var, float eps, void* w_out, float* b_out,
                        float* scale_out, int Cout, int Cin, void* stream);
/* The three blocks as an inference plan, in the shape of ecgmm_resnet1d_infer*: prepare folds the 12 parameters and 9
 * buffers of ecgmm_crnn_front_forward into a blob (one launch; the blob depends on dtype and bn_eps, not on B, F, T: fp32
 * folded conv1 weight, packed folded weights of blocks 2 and 3 in the compute dtype, three fp32 biases); infer reads the
 * blob and the spectrogram alone and writes seq_out [B, T/8, 128 * (F/8)] fp32 in 5 launches.  The workspace holds the two
 * pooled tensors and the conv outputs of blocks 2 and 3 -- no [B,F,T,32] tensor, no argmax bytes, no statistics rows.
 * desc.training and desc.bn_momentum are ignored.  F < 8, T < 8, an unknown dtype, null operands, a short blob or
 * workspace are refused with a message; the size queries need no GPU and return 0 on a bad descriptor. */
size_t ecgmm_crnn_front_infer_prepared_bytes(const ecgmm_crnn_front_desc* d);
int ecgmm_crnn_front_infer_prepare(const ecgmm_crnn_front_desc* d, const void* const* params, const void* const* buffers,
                                   void* blob, size_t blob_bytes, void* stream);
size_t ecgmm_crnn_front_infer_workspace(const ecgmm_crnn_front_desc* d);
int ecgmm_crnn_front_infer(const ecgmm_crnn_front_desc* d, const float* spec, const void* blob, size_t blob_bytes,
                           float* seq_out, void* ws, size_t ws_bytes, void* stream);

/* Grad-CAM of the CRNN's last ConvBlock on the spectrogram (csrc/gradcam.hip).  There is no global average pool in front of
 * the CRNN's head, so the gradient varies over space and is an operand: seq, dseq [B][Tp][C*Fp] fp32 are the front end's
 * output and the gradient of the chosen logit w.r.t. it, feature index c*Fp + f (permute(0,3,1,2) + Flatten(2) of the
 * activation A[b][c][f][t], train_physionet2.py:92-93).
 *   a[b][c]    = (1 / (Tp*Fp)) * sum_{t,f} dseq[b][t][c*Fp+f]                  (fixed order)
 *   m[b][f][t] = relu(sum_c a[b][c] * seq[b][t][c*Fp+f]),  m[b] /= max m[b]     (a true division: the maximum becomes
 *                exactly 1; all zero when the maximum is 0)
 *   cam [B][F][T] = bilinear upsample of m from (Fp, Tp) to (F, T), align_corners=False
 * steps (nullable, int32 [B], 1..Tp): the live steps of each record; only t < steps[b] is read from either operand (the
 * variable-length LSTM leaves exact zeros behind it, so the sums are the same, and padded NaN is never touched) and m is
 * exactly 0 behind it.  frames (nullable, int32 [B], 1..T): the live spectrogram frames; columns t >= frames[b] of cam are
 * set to exactly 0.  Neither is range-checked on the device: values outside their range are the caller's error.
 * ws: ecgmm_crnn_gradcam_workspace bytes (needs no GPU; 0 with the message set for extents < 1).  Refused with a message:
 * null seq / dseq / cam, an extent < 1, a short workspace. */
size_t ecgmm_crnn_gradcam_workspace(int B, int Tp, int Fp, int C);
int ecgmm_crnn_gradcam(const float* seq, const float* dseq, const int32_t* steps, const int32_t* frames, void* ws,
                       size_t ws_bytes, float* cam, int B, int Tp, int C, int Fp, int F, int T, void* stream);

/* The map kernels behind ecgmm_resnet18_gradcam / ecgmm_resnet1d_gradcam on their own (csrc/gradcam.hip), for callers that
 * hold the last activation and d logit / d pooled themselves, and for the tests:
 *   s[n][r]  = relu((1 / (Hs*Ws)) * sum_c dpooled[n][c] * act[n][r][c]),  s[n] *= 1 / max_r s[n][r]  (the reciprocal form: the
 *              maximum becomes 1 or 1 - 2^-24; all zero when the maximum is 0)
 *   out [N][H][W] fp32 = bilinear upsample of s from (Hs, Ws) to (H, W), align_corners=False
 * act [N][Hs*Ws][C] channels-last in `dtype` (ECGMM_BF16 / ECGMM_F32), dpooled [N][C] fp32, small [N][Hs*Ws] fp32 scratch that
 * holds the normalised coarse map afterwards; every element of small and out is written.  Refused with a message: a null
 * operand, an extent < 1, an unknown dtype, Hs*Ws or H*W beyond 2^31 - 1. */
int ecgmm_gradcam(int dtype, const void* act, const float* dpooled, float* small, float* out, int N, int Hs, int Ws, int C,
                  int H, int W, void* stream);

/* The log-spectrogram in front of the CRNN (train_physionet2.py:30-34): np.log1p(np.abs(scipy.signal.stft(x, fs, window,
 * nperseg=64, noverlap = 64 - hop)[2])) with scipy's defaults (boundary='zeros', padded=True, one-sided, scaling='spectrum',
 * no detrend) for a whole [S][L] fp32 matrix in one launch.  Frame t covers samples [hop*t - 32, hop*t + 32) of the record,
 * zeros outside [0, L); T = ceil(L / hop) + 1 frames (ecgmm_log_spectrogram_frames: no GPU needed, 0 with the message set
 * for a refused shape).  table [33][64][2] fp32 on the device: w[j] / sum(w) * (cos, -sin)(2 pi j k / 64) for the window
 * coefficients w, built by the caller (ecgmm/spectrogram.py) -- the kernel evaluates no sin / cos.  out [S][33][T] fp32 =
 * the [S,1,33,T] memory ecgmm_crnn_front_forward reads; every element is written, an all-zero frame gives exactly 0, so a
 * record zero-padded to the longest one gives its own spectrogram followed by zeros.  fp32 accumulation in a fixed order,
 * no atomics: a row's bits do not depend on S.  Refused with a message: nperseg != 64, hop outside 1..64, L < nperseg
 * ("length"), T != the query's value ("frames"), null operands, S < 1.  L is not bounded by LDS. */
int ecgmm_log_spectrogram_frames(int L, int nperseg, int hop);
int ecgmm_log_spectrogram(const float* x, int S, int L, const float* table, int nperseg, int hop, float* out, int T,
                          void* stream);

/* LIME tabular of the fusion head (lime_fusion_modal_balance.py:118-160; lime 0.2.x with the defaults that call hits),
 * csrc/lime.hip.  All pointers are device pointers.  Every entry refuses a bad shape with ECGMM_ERR_SHAPE and then writes
 * nothing; a table or column index read on the device is range-checked before it addresses memory.
 *
 * ecgmm_lime_perturb -- the data_inverse of explain_instance (:158-160) for B rows at once.  x [B][D] fp32.  The quartile
 * discretiser's table, S = the widest feature's bin count (<= 16): nbins [D]; qts [D][S] float64, the first nbins - 1 of a
 * row are np.unique(np.percentile(...)); cdf [D][S] float64, the inclusive cumulative bin frequencies; stats [4][D][S]
 * float64 = mean, std, min, max of each bin; lim [2][D][S] fp32 = min, max rounded to fp32 (the clamp).
 * Outputs: Z uint8 [B][N][D] (drawn bin == bin of x), inverse fp32 [B][N][D], d2 int32 [B][N] (the zeros of a Z row),
 * u_out (nullable) double [B][N][D][2], the two uniforms of each element.  Row n = 0 is the instance: Z = 1, inverse = x.
 * Element (b, n, f) takes ONE Philox4x32-10 block keyed by `seed` at counter
 *     (offset low, offset high, n, 0x40000000 | (b0 + b) << 12 | f)
 * u_bin = ((w0 >> 5) * 2^26 + (w1 >> 6)) * 2^-53, u_val likewise from w2, w3: it depends on (seed, offset, b0 + b, n, f)
 * alone (b0: the index of the call's first row in the caller's batch, so chunked calls reproduce one call).  The bin is the
 * first j with cdf[j] > u_bin * cdf[nbins - 1] (the rule of ecgmm_weighted_sample: a bin of zero frequency is never drawn);
 * the value is mean + std * Phi^-1(Phi(a) + u_val (Phi(b) - Phi(a))), a, b = (min, max - mean) / std, in fp64 (mirrored for
 * a > 0), rounded to fp32 and clamped to lim; it is mean where std is the bare 1e-11 offset and the common point where a == b.
 * Needs 1 <= D <= 4096, b0 + B <= 2^18, B * N < 2^31.  The caller advances `offset` by one per explanation batch. */
int ecgmm_lime_perturb(const float* x, const double* qts, const double* cdf, const double* stats, const float* lim,
                       const int* nbins, int S, int B, int b0, int N, int D, uint64_t seed, uint64_t offset, uint8_t* Z,
                       float* inverse, int* d2, double* u_out, void* stream);
/* ecgmm_lime_ridge -- the weighted ridge of explain_instance_with_data (:158-161): per sample b and label l
 *     w_n = sqrt(exp(-d2_n / kernel_width^2)),  (Zc^T W Zc + alpha I) beta = Zc^T W yc  with w-weighted centring,
 * over the K kept columns cols [B][K] int32 (nullable: all D columns, K == D).  Z [B][N][D] uint8 (0 / nonzero),
 * d2 [B][N], y [B][L][N] fp32.  Outputs: coef [B][L][K], intercept [B][L]; nullable w [B][N], score [B][L] (the weighted
 * R^2), local_pred [B][L] = intercept + sum_k coef.  The Gram runs on the exact-fp32 MFMA with fp32 accumulation, the
 * centring is a rank-one correction in fp64, the factorisation a blocked fp32 Cholesky shared by the L right-hand sides.
 * A column whose entries are all equal gets the coefficient 0 exactly; a column index outside [0, D) is never addressed
 * and its coefficient is NaN.  Needs 1 <= K <= D <= 4096, K <= 1024, 1 <= L <= 8, B <= 65535, kernel_width, alpha > 0.
 * ecgmm_lime_ridge_workspace(B, N, D), 1 <= D <= 4096: bytes for any K <= min(D, 1024) and L <= 8 (no GPU needed; 0 with
 * the message set when refused); too small a workspace is ECGMM_ERR_WORKSPACE. */
size_t ecgmm_lime_ridge_workspace(int B, int N, int D);
int ecgmm_lime_ridge(const uint8_t* Z, const int* d2, const float* y, const int* cols, int B, int N, int D, int K, int L,
                     double kernel_width, double alpha, float* coef, float* intercept, float* w, float* score,
                     float* local_pred, void* ws, size_t ws_bytes, void* stream);
/* predict_fn's torch.softmax(outputs, dim=1)[:, label] (:126-131): out[m * out_stride] = softmax(logits[m])[label],
 * logits [M][C] fp32. */
int ecgmm_lime_prob(const float* logits, int64_t M, int C, int label, float* out, int64_t out_stride, void* stream);

/* SHAP of the fusion head, csrc/shap.hip: the two estimators the reference asks shap for, restricted to the network they are
 * applied to, Linear(D, H) -> ReLU -> Dropout(eval) -> Linear(H, C).  All pointers are device pointers and fp32 unless said
 * otherwise: x [B][D], bg [N][D], W1 [H][D], b1 [H], W2 [C][H], phi [B][D][C].  Per sample b and pair k with background row r:
 *     z = W1 p + b1,  s_c = W2[c, :] * gate(z),  G_c = W1^T s_c,  phi[b, :, c] = mean_k G_c * (x_b - bg_r).
 * Both GEMMs run on the exact-fp32 MFMA; the sums over pairs (and of the squares) are fp64 in a fixed order that depends on
 * k alone, stored as fp32: one call with B samples equals B calls with one, bit for bit.  No floating-point atomics.
 * Needs B, N >= 1, 1 <= K <= 4096, 1 <= D <= 4096, 1 <= H <= 256, 1 <= C <= 8; anything else is ECGMM_ERR_SHAPE, too small
 * a workspace ECGMM_ERR_WORKSPACE, and a refused call writes nothing.
 * ecgmm_shap_mlp_workspace(B, K, D, H, C): bytes for either entry (K = N for ecgmm_shap_deep); needs no GPU; 0 with the
 * message set when refused.
 *
 * ecgmm_shap_gradient -- shap.GradientExplainer(...).shap_values (shap_fusion_modal_balance.py:122-160; the PyTorch back
 * end with local_smoothing = 0).  ridx int32 [B][K] and t [B][K] are the caller's draws: pair (b, k) uses r = ridx[b][k] and
 * the point p = t x_b + (1 - t) bg_r evaluated in fp32 in exactly that form (t = 1 gives x_b, t = 0 gives bg_r bit for
 * bit); gate = 1[z > 0].  var (nullable) [B][D][C] is shap's return_variances: the population variance over k divided by
 * sqrt(K).  z (nullable) [B][K][H] receives the pre-activations.  A ridx outside [0, N) is never used as an address and
 * makes that sample's phi and var NaN.
 *
 * ecgmm_shap_deep -- shap.DeepExplainer(...).shap_values (shap_fusion.py:62, shap_fusion_paper.py:71; the PyTorch back end:
 * rescale rule on ReLU, plain gradient through Linear, Dropout passed through).  The pairs are all (b, n), K = N;
 * gate = (relu(zx) - relu(zb)) / (zx - zb), and 1[zb > 0] where |zx - zb| < 1e-6 (shap's constant).  zx [B][H] and zb [N][H]
 * (both nullable) receive the pre-activations of the rows, computed once per row by the instruction sequence that computes
 * z of ecgmm_shap_gradient: a pair with t = 1 / t = 0 there has bit-equal z. */
size_t ecgmm_shap_mlp_workspace(int B, int K, int D, int H, int C);
int ecgmm_shap_gradient(const float* x, const float* bg, const int* ridx, const float* t, const float* W1, const float* b1,
                        const float* W2, int B, int N, int K, int D, int H, int C, float* phi, float* var, float* z,
                        void* ws, size_t ws_bytes, void* stream);
int ecgmm_shap_deep(const float* x, const float* bg, const float* W1, const float* b1, const float* W2, int B, int N, int D,
                    int H, int C, float* phi, float* zx, float* zb, void* ws, size_t ws_bytes, void* stream);

/* Multi-head self-attention of nn.TransformerEncoderLayer, csrc/attention.hip: softmax(Q K^T / sqrt(head_dim)) V per
 * (n, head), fp32, products on the exact-fp32 MFMA.  S is the sequence length and N the attention batch AS TORCH SEES
 * THEM: train_physionet.py:219 builds the layer with batch_first = False and :236 feeds it [B, L, E], so there S = B and
 * N = L; multimodal_paper_modal_balance.py:135 uses batch_first = True.  All pointers are device pointers, 16-byte aligned:
 *   qkv  [rows][3E], E = heads * head_dim, as linear(x, in_proj_weight, in_proj_bias) leaves it; row(s, n) = s * N + n
 *        (batch_first = 0) or n * S + s (batch_first = 1); read by stride, never copied or transposed
 *   out  [rows][E], heads concatenated: the input of out_proj;  lse [N][heads][S]: log-sum-exp of each scaled score row
 *   dout [rows][E];  dqkv [rows][3E]: every element WRITTEN (dQ, dK, dV), each reduced in a fixed order, no atomics
 * No S x S tensor is formed: online softmax over 16-key tiles forward; the backward recomputes the probabilities from lse
 * and needs one float per (n, head, query) of workspace (ecgmm_mha_bwd_workspace: no GPU needed, 0 with the message set on
 * a bad descriptor).  Two identical calls give identical bits.
 * p_drop > 0: dropout on the normalised probabilities, kept ones scaled by 1 / (1 - p_drop).  The decision for
 * (n, head, query i, key j) is word j % 4 of the Philox4x32-10 block keyed by `seed` at counter
 *     (offset low, offset high, n * heads + head, 0xC0000000 | i * ceil(S / 4) + j / 4),  keep iff (word >> 8) * 2^-24 >= p_drop;
 * the backward regenerates it from the same (seed, offset), nothing is stored.  ecgmm_mha_keep_mask writes the decisions
 * as bytes [N][heads][S][S] (tests and small shapes).  The caller advances `offset` by one per forward call.
 * Needs S, N, heads >= 1, head_dim 16 or 32, batch_first 0 or 1, 0 <= p_drop < 1, S <= 32768 when p_drop > 0; anything
 * else is ECGMM_ERR_SHAPE and writes nothing.  No attention mask and no causal mask; a key-padding mask only in the form
 * of one length per attention-batch element (the _varlen entry points below). */
typedef struct {
  int S, N, heads, head_dim, batch_first;
  float p_drop;
} ecgmm_mha_desc;
/* train_physionet.py:219-220, 236 (its loss.backward()) */
size_t ecgmm_mha_bwd_workspace(const ecgmm_mha_desc* d);
/* train_physionet.py:219-220, 236: self_attn of each encoder layer */
int ecgmm_mha_forward(const ecgmm_mha_desc* d, const float* qkv, float* out, float* lse, uint64_t seed, uint64_t offset,
                      void* stream);
/* train_physionet.py:219-220, 236: the self_attn part of loss.backward() */
int ecgmm_mha_backward(const ecgmm_mha_desc* d, const float* qkv, const float* out, const float* lse, const float* dout,
                       float* dqkv, void* ws, size_t ws_bytes, uint64_t seed, uint64_t offset, void* stream);
/* train_physionet.py:219 (dropout = 0.1 of the layer, applied to the attention weights) */
int ecgmm_mha_keep_mask(const ecgmm_mha_desc* d, uint8_t* mask, uint64_t seed, uint64_t offset, void* stream);
/* Variable-length form: qkv, out, dout and dqkv stay padded ([rows][..] of the padded S) and lengths [N] (device int32) says
 * how many positions of attention-batch element n are live, s < lengths[n], the same in every head.  It equals torch's
 * key_padding_mask[n][s] = s >= lengths[n] on the live rows, plus exact zeros in the padding:
 *   live query     softmax over the live keys only; the arithmetic and the order of the 16-key tiles are those of
 *                  ecgmm_mha_forward on that element alone with S = lengths[n] (at S > 8 and lengths[n] > 8: the same bits)
 *   padded query   its out row is exactly 0, its lse 0, its dQ row exactly 0
 *   padded key     its dK and dV rows are exactly 0
 * lengths are clamped to [0, S] on the device (no host sync); lengths[n] = 0 makes everything of n zero.  Every element of
 * out, lse and dqkv is WRITTEN, as without lengths.  Padded rows of qkv and dout are never read into arithmetic that reaches
 * an output (empty tile slots read position lengths[n] - 1 instead): THEY MAY HOLD ANYTHING, NaN included.
 * Work follows the lengths: the key loop of the forward and dQ kernels and the query loop of the dK / dV kernel run
 * ceil(lengths[n] / 16) tiles, and a unit whose own 16 rows are all padding only stores its zeros.
 * Dropout: the decision stays the function of (seed, offset, n, head, query, key) above with ceil(S / 4) of the PADDED S as the
 * stride, so ecgmm_mha_keep_mask of the same descriptor describes the launch (its entries at padded positions are unused).
 * The packed form (S <= 8) takes lengths too.  lengths = null is exactly ecgmm_mha_forward / ecgmm_mha_backward, bit for bit
 * (the same kernel instantiations); so is lengths all equal to S.  The backward takes the lengths the forward ran with and
 * the workspace of ecgmm_mha_bwd_workspace.  No atomics: two identical calls give identical bits. */
/* multimodal_paper_modal_balance.py:133-140, 145 (batch_first = True: attention over the positions) on records of unequal
 * length */
int ecgmm_mha_forward_varlen(const ecgmm_mha_desc* d, const float* qkv, const int32_t* lengths, float* out, float* lse,
                             uint64_t seed, uint64_t offset, void* stream);
/* multimodal_paper_modal_balance.py:133-140, 145 (its loss.backward()) */
int ecgmm_mha_backward_varlen(const ecgmm_mha_desc* d, const float* qkv, const int32_t* lengths, const float* out,
                              const float* lse, const float* dout, float* dqkv, void* ws, size_t ws_bytes, uint64_t seed,
                              uint64_t offset, void* stream);
/* Attention maps and attention rollout, from the qkv the forward read and the lse it wrote (the backward's own recomputation):
 *     p[n,h,i,j] = exp(scale q_i . k_j - lse[n,h,i]),  the normalised probabilities BEFORE dropout.
 * p_drop of the descriptor is validated and then ignored: in eval mode and at dropout 0 these are torch's attention weights;
 * in training mode torch returns the dropped, rescaled weights and these stay the undropped ones.
 * ecgmm_mha_weights: weights [N][heads][S][S] (per_head = 1) or the head average [N][S][S] (per_head = 0, torch's
 *   average_attn_weights = True): the heads h = 0, 1, .. summed in that order in fp32, then ONE multiplication by the fp32
 *   1 / heads.  The layout is always (query row, key column), whatever batch_first says of qkv.  Every element is WRITTEN.
 * ecgmm_mha_rollout_step: v_in, v_out [N][S] fp32 (v_out != v_in),
 *     v_out[n][j] = residual v_in[n][j] + (1 - residual) (1 / heads) sum_h sum_i v_in[n][i] p[n,h,i,j],   0 <= residual < 1:
 *   one step of attention rollout (Abnar & Zuidema 2020) of a ROW vector through a I + (1 - a) mean_h P, without the S x S
 *   matrix and without a workspace.  residual outside [0, 1) is ECGMM_ERR_SHAPE.
 * lengths (nullable, device int32 [N], clamped to [0, S], the lengths the forward ran with): a live query row holds the
 * softmax over the live keys; padded query rows and padded key columns of the weights are exact 0 (torch's padded QUERY rows
 * still attend to the live keys: here they do not exist); padded v_in is never read and padded v_out is exact 0; padded rows
 * of qkv are never read; a tile wholly in the padding loads nothing, and the loops run ceil(lengths[n] / 16) tiles.  At
 * S > 8 and lengths[n] > 8 element n has the bits of the same element alone with S = lengths[n]; lengths = null equals
 * lengths all S bit for bit.  Any S >= 1 (S <= 8 runs as one partial tile per n).  Each output element is written by one
 * lane, every sum runs in a fixed order, no atomics: two identical calls give identical bits.  A refused call writes nothing. */
/* train_physionet.py:219-220, 236; multimodal_paper_modal_balance.py:133-140: the attention weights of each self_attn */
int ecgmm_mha_weights(const ecgmm_mha_desc* d, const float* qkv, const float* lse, const int32_t* lengths, float* weights,
                      int per_head, void* stream);
/* train_physionet.py:219-220, 236; multimodal_paper_modal_balance.py:133-140: the rollout of the mean-pooled output */
int ecgmm_mha_rollout_step(const ecgmm_mha_desc* d, const float* qkv, const float* lse, const int32_t* lengths,
                           const float* v_in, float* v_out, float residual, void* stream);

/* The front of ECGTransformer1D (train_physionet.py:216-217, 233-235) as one launch: Conv1d(Cin, Dm, 3, padding = 1) + bias
 * written straight as [B][L][Dm] with pos[l][c] added.  x [B][Cin][L], w [Dm][Cin][3], bias [Dm], pos [>= L][Dm], fp32.
 * Backward: dy [B][L][Dm]; dw [Dm][Cin][3], db [Dm], dpos [pos_len][Dm] (rows >= L are written as zero) and dx [B][Cin][L]
 * are each nullable (not computed) and otherwise WRITTEN, sums in a fixed order.  dw / db need the workspace
 * (ecgmm_embed1d_bwd_workspace: no GPU needed, 0 with the message set when refused).
 * Needs B, L >= 1, 1 <= Cin <= 12, 1 <= Dm <= 4096, pos_len >= L; else ECGMM_ERR_SHAPE and nothing is written. */
int ecgmm_embed1d_fwd(const float* x, const float* w, const float* bias, const float* pos, float* y, int B, int Cin, int L,
                      int Dm, void* stream);
/* train_physionet.py:216-217, 233-235 (its loss.backward()) */
size_t ecgmm_embed1d_bwd_workspace(int B, int Cin, int L, int Dm);
int ecgmm_embed1d_bwd(const float* x, const float* w, const float* dy, float* dw, float* db, float* dpos, float* dx, int B,
                      int Cin, int L, int Dm, int pos_len, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Forward-only tails of a post-norm TransformerEncoderLayer and the inference plan of ECGTransformer1D
 * (csrc/transformer_infer.hip, csrc/plan_infer.hip; ecgmm.inference.Predictor).  Exact fp32 on v_mfma_f32_16x16x4_f32.
 *
 * ecgmm_linear_res_ln: out[r, :] = LayerNorm(res[r, :] + a[r, :] W^T + bias; gamma, beta, eps).  a [R, K], W [E, K] (torch's
 *   layout), res and out [R, E], bias / gamma / beta [E]: out_proj + residual + norm1 of a layer as ONE launch; the pre-norm
 *   sum is never stored.
 * ecgmm_ffn_res_ln:    out[r, :] = LayerNorm(x[r, :] + relu(x[r, :] W1^T + b1) W2^T + b2; gamma, beta, eps).  x and out [R, E],
 *   W1 [ff, E], b1 [ff], W2 [E, ff], b2 / gamma / beta [E]: the feed-forward block + residual + norm2 as ONE launch; the
 *   hidden activation lives in registers, 16 units at a time, and never exists in memory.  No workspace.
 * The variance is the biased one over the E values of a row (two passes over the registers: mean, then the centred sum of
 * squares).  A wave owns whole rows; a row's bits depend on that row and the weights alone -- not on R, not on the row's place
 * in a tile -- the summation order is fixed, there are no atomics, two identical calls give identical bits.
 * Needs R >= 1; E a multiple of 16 with 16 <= E <= 256; K / ff a multiple of 16 with 16 <= K, ff <= 4096; eps >= 0; every
 * operand non-null and 16-byte aligned; out must NOT alias res, a or x (equal pointers are refused: in place is not
 * supported).  Anything else is ECGMM_ERR_SHAPE with the limit in the message, and nothing is written. */
/* train_physionet.py:219-220, 236 in eval mode: out_proj, the residual add and norm1 of each encoder layer */
int ecgmm_linear_res_ln(const float* a, const float* w, const float* bias, const float* res, const float* gamma,
                        const float* beta, float* out, int64_t R, int K, int E, float eps, void* stream);
/* train_physionet.py:219-220, 236 in eval mode: linear1, ReLU, linear2, the residual add and norm2 of each encoder layer */
int ecgmm_ffn_res_ln(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, const float* gamma,
                     const float* beta, float* out, int64_t R, int E, int ff, float eps, void* stream);

/* The whole eval forward of ECGTransformer1D (train_physionet.py:211-240) as an inference plan, in the shape of
 * ecgmm_crnn_front_infer*.  E = d_model, ff = dim_feedforward, classes = num_classes; the classifier's hidden width is the
 * model's 64.  batch_first = 0 is the reference's attention ACROSS THE BATCH (S = B, N = L), 1 attends along each record's
 * positions (S = L, N = B).
 * prepare: params[3 + 12 * layers + 4] fp32 device pointers -- conv.weight [E, input_dim, 3], conv.bias [E], pos_embedding
 *   [L, E] (L of THIS descriptor = the rows of the embedding to keep, the model's seq_len), then per layer in_proj_weight
 *   [3E, E], in_proj_bias, out_proj.weight [E, E], out_proj.bias, linear1.weight [ff, E], linear1.bias, linear2.weight [E, ff],
 *   linear2.bias, norm1.weight, norm1.bias, norm2.weight, norm2.bias, then classifier.1.weight [64, E], .bias,
 *   classifier.4.weight [classes, 64], .bias -- are copied into one blob (B is not looked at).  The positional table is
 *   the blob's last entry, so a run at any L' <= L reads the same blob.
 * infer: x [B, input_dim, L] fp32 -> logits [B, classes] fp32 on the given stream, reading the blob alone:
 *   embed (ecgmm_embed1d_fwd), per layer 4 launches -- in_proj (ecgmm_linear_fwd), ecgmm_mha_forward(_varlen),
 *   ecgmm_linear_res_ln, ecgmm_ffn_res_ln -- then the mean over the positions and Linear-ReLU-Linear.  Bit for bit that
 *   sequence of per-op calls.  lengths (nullable, device int32 [B], only with batch_first = 1, clamped to [0, L] on the
 *   device): positions at or behind a record's length are never keys and do not enter the mean, and the record's raw samples
 *   there are replaced by zeros before the convolution (one more launch), so its logits depend on its own live samples
 *   alone; a length 0 gives the classifier of a zero vector.
 * workspace: rotating buffers that depend neither on layers nor on ff -- x, next x and the attention output [B L, E] each,
 *   qkv [B L, 3E], lse [B L heads], and [B, E] + [B, 64] + [B] for the tail: at most
 *   4 B L (6E + heads) + 4 B (E + 64 + classes) bytes + 256 per buffer.
 * Needs B, L, layers, classes >= 1, 1 <= input_dim <= 12, E and ff as the two ops above, E / heads 16 or 32, eps >= 0,
 * B <= 65535; else ECGMM_ERR_SHAPE (the size queries: 0) with the limit in the message; a short blob or workspace is
 * ECGMM_ERR_WORKSPACE.  The size queries need no GPU. */
typedef struct {
  int B, L, input_dim, E, heads, ff, layers, classes, batch_first;
  float eps;
} ecgmm_transformer_infer_desc;
/* train_physionet.py:211-240 */
size_t ecgmm_transformer_infer_prepared_bytes(const ecgmm_transformer_infer_desc* d);
/* train_physionet.py:211-240 (a snapshot of every parameter) */
int ecgmm_transformer_infer_prepare(const ecgmm_transformer_infer_desc* d, const void* const* params, void* blob,
                                    size_t blob_bytes, void* stream);
/* train_physionet.py:233-240 */
size_t ecgmm_transformer_infer_workspace(const ecgmm_transformer_infer_desc* d);
/* train_physionet.py:233-240 under model.eval() and torch.no_grad() (:352-358) */
int ecgmm_transformer_infer(const ecgmm_transformer_infer_desc* d, const float* x, const int32_t* lengths, const void* blob,
                            size_t blob_bytes, float* logits, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The eval forward of TabNetNoEmbeddings (ecgmm/tabnet.py; pytorch_tabnet as multimodal.py:113-123 instantiates it) as an
 * inference plan (csrc/tabnet_infer.hip; ecgmm.inference.Predictor, TabNetEncoder.forward_masks).  Exact fp32 on
 * v_mfma_f32_16x16x4_f32; ONE launch per prepare and ONE per forward, whatever the depth.
 *
 * prepare: params[4 + 5 (n_steps + 1) (n_shared + n_independent) + 5 n_steps + 1] fp32 device pointers, IN state_dict ORDER
 *   with every num_batches_tracked left out: encoder.initial_bn {weight, bias, running_mean, running_var}; then for the
 *   FeatTransformers initial_splitter, feat_transformers.0 .. n_steps-1, for their GLU layers shared.glu_layers.* then
 *   specifics.glu_layers.*: {fc.weight [2 (n_d + n_a), K], bn.bn.weight, .bias, .running_mean, .running_var} (K = input_dim
 *   for a FeatTransformer's first layer, n_d + n_a otherwise; a shared fc.weight appears once per FeatTransformer, as it does
 *   in the state_dict, each time next to THAT FeatTransformer's BatchNorm); then for att_transformers.0 .. n_steps-1:
 *   {fc.weight [input_dim, n_a], bn.bn.weight, .bias, .running_mean, .running_var}; then final_mapping.weight [out_dim, n_d].
 *   Every BatchNorm is folded into the bias-free fc in front of it: s_j = gamma_j / sqrt(rv_j + bn_eps),
 *   W'[j, k] = s_j W[j, k], b'_j = beta_j - rm_j s_j (one fused multiply-add); gamma_j = 0 gives a row of exact zeros.
 *   initial_bn becomes a (scale, shift) pair and is NOT folded into the first layer: the masks multiply the normalised
 *   input.  K and the attentive output width are zero-padded to multiples of 16; every byte of the blob is written.
 *   Blob layout, in floats, every piece at a multiple of 64 (Dp = input_dim rounded up to 16, W = n_d + n_a, pad64 rounds up
 *   to 64): scale[64] shift[64] | for each FeatTransformer, for each layer: W' [2W, K] row-major (K = Dp for the first layer,
 *   W otherwise), b' [pad64(2W)] | for each step: attentive W' [Dp, n_a], b' [64] | final_mapping [out_dim, n_d].
 * infer: x [B, input_dim] -> out [B, out_dim] = final_mapping(sum_step relu(d_step)).  Optional outputs, not written when null
 *   (out has the same bits whichever are requested): m_explain [B, input_dim] = sum_step M_step * sum_j relu(d_step)_j
 *   (pytorch_tabnet's forward_masks with the identity group matrix), masks [n_steps, B, input_dim] (each row on the simplex;
 *   an entry outside the support is exactly 0.0), row_entropy [B] = sum_step sum_d M log(M + epsilon) (its mean over B,
 *   divided by n_steps, is the module's M_loss).  The sparsemax is Michelot's fixed point on the row minus its maximum (no
 *   sort).  A row's bits depend on that row and the blob alone -- not on B, not on its place in a tile; no atomics; two
 *   identical calls give identical bits.
 * Needs 1 <= input_dim <= 64; n_d and n_a multiples of 16 with n_d + n_a <= 128; 1 <= n_steps <= 8; n_shared,
 * n_independent >= 0 with 1 <= n_shared + n_independent <= 8; out_dim a multiple of 16 with 16 <= out_dim <= 128 (a ragged
 * out_dim is refused, not padded); 0 <= gamma <= 1e6; epsilon, bn_eps in [0, 1]; 1 <= B < 2^31 - 64; a 16-byte aligned blob.
 * Anything else is ECGMM_ERR_SHAPE (the size query: 0) with the limit in the message and nothing is written; a short blob is
 * ECGMM_ERR_WORKSPACE.  There is no workspace.  The size query needs no GPU. */
typedef struct {
  int input_dim, n_d, n_a, n_steps, n_shared, n_independent, out_dim;
  float gamma, epsilon, bn_eps;
} ecgmm_tabnet_infer_desc;
/* multimodal.py:113-123 */
size_t ecgmm_tabnet_infer_prepared_bytes(const ecgmm_tabnet_infer_desc* d);
/* multimodal.py:113-123 in eval mode (a folded snapshot of every parameter and running statistic) */
int ecgmm_tabnet_infer_prepare(const ecgmm_tabnet_infer_desc* d, const void* const* params, void* blob, size_t blob_bytes,
                               void* stream);
/* multimodal.py:141-148 under model.eval() and torch.no_grad(); the masks are what :170-240 plots */
int ecgmm_tabnet_infer(const ecgmm_tabnet_infer_desc* d, const float* x, int64_t B, const void* blob, size_t blob_bytes,
                       float* out, float* m_explain, float* masks, float* row_entropy, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ECGMM_H */
