// Internal (C++) launch interface between the kernel files, the encoder plans and the C-ABI layer.
#pragma once
#include "common.h"
#include "switches.h"

// preprocess.hip: how many lanes of the chunked filtfilt kernels (preprocess.hip, physionet.hip) run the recurrences, from the
// denominator a[0..order] (a[0] = 1) and the padded record length E alone: 64, 32, 16, 8, 4, 2 or 1 (sequential)
int ecg_iir_lanes(const double* a, int order, int E);

// conv_igemm.hip
int ecg_conv_stats_rows(long M);
// Optional epilogue extras of a convolution launch (the encoder plans use them; the C ABI passes none).
struct ConvEpi {
  // in -- dgrad only: fuse the REDUCTION pass of the BatchNorm backward that consumes this gradient into the epilogue
  // (done by the halo kernel only: check red_done).  g = [mask] * dst as stored; rows of (sum g, sum g * (y - mean)).
  const void* red_y;      // raw conv output that BatchNorm normalised (same [pixels][channels] layout as dst), or null
  const void* red_mask;   // null / == red_y: mask = (bn(y) > 0), dst stored unmasked; else mask = (red_mask > 0), dst stored MASKED
  const float* red_coef;  // that BatchNorm's forward coefficients [4][C]
  float* red_rows;        // [>= 512 rows][2][C] (one row per workgroup of a channel tile; 64-channel tiles run two workgroups per CU)
  int wg_rows;            // in: 1 = the launch may write ONE partial row per workgroup instead of one per 64 pixels
  // in -- stride-2 dgrad only: fold the input gradient of a 1x1 stride-2 pad-0 convolution of the same input (ResNet
  // downsample branch) into this launch: src2 = that branch's output gradient (same shape as src), wpk2 = its dgrad pack.
  // Done by the parity-class kernel only: check src2_done (0 = run it as its own launch and pass the result as addend).
  const void* src2;
  const void* wpk2;
  // out
  int src2_done;
  int stats_rows;         // rows of `stats` the forward launch wrote
  int red_done;           // 1 = red_rows holds red_rows_n rows; 0 = the caller runs the separate reduction pass
  int red_rows_n;
};
int ecg_conv_igemm(int dtype, int mode, const ConvGeom& g, const void* src, const void* wpk, void* dst,
                   const float* bias, const void* addend, float* stats, int act, hipStream_t stream,
                   ConvEpi* epi = nullptr);
// conv_halo.hip: stride-1 "same" 3x3 / 1x3 convolutions with a halo-resident activation tile (bf16, whole 256-pixel tiles)
bool ecg_conv_halo_ok(int dtype, int mode, const ConvGeom& g);
int ecg_conv_halo_rows(int mode, const ConvGeom& g);
int ecg_conv_halo(int mode, const ConvGeom& g, const void* src, const void* wpk, void* dst, const float* bias,
                  const void* addend, float* stats, int act, ConvEpi* epi, hipStream_t stream);
// conv_wgrad.hip
size_t ecg_conv_wgrad_workspace(int dtype, const ConvGeom& g);
void ecg_conv_wgrad_narrow(bool narrow, int slots = 256);   // slots: four-wave slots of a narrow launch (conv_wgrad.hip, pick_nsplit)
int ecg_conv_wgrad(int dtype, const ConvGeom& g, const void* x, const void* dy, float* grad_oihw, int accumulate,
                   void* workspace, size_t workspace_bytes, hipStream_t stream);
// conv_stem.hip
size_t ecg_stem_packed_elems(int Cin, int R);
int ecg_stem_stats_rows(int N, int Cin, int H, int W, int R);
int ecg_stem_pack(int dtype, const float* w, void* out, int Cin, int R, hipStream_t stream);
int ecg_stem_fwd(int dtype, const float* x, const void* wpk, const float* bias, void* y, float* stats, int N, int Cin,
                 int H, int W, int R, hipStream_t stream);
size_t ecg_stem_wgrad_workspace(int N, int Cin, int H, int W, int R);
int ecg_stem_wgrad(int dtype, const float* x, const void* dy, float* grad, int accumulate, void* workspace,
                   size_t workspace_bytes, int N, int Cin, int H, int W, int R, hipStream_t stream);
int ecg_stem_stats_only_rows(int N, int Cin, int H, int W, int R);
int ecg_stem_wg_stats_rows(int N, int Cin, int H, int W, int R);
int ecg_stem_fwd_wgrows(int dtype, const float* x, const void* wpk, const float* bias, void* y, float* stats, int N, int Cin,
                        int H, int W, int R, hipStream_t stream);   // bf16: statistics rows per workgroup (4 x grid) instead of per tile
int ecg_stem_stats_only(int dtype, const float* x, const void* wpk, const float* bias, float* stats, int N, int Cin, int H,
                        int W, int R, hipStream_t stream);
int ecg_stem_wgrad_reduce(const float* slab, float* grad, int rows, int NG, int accumulate, hipStream_t stream);
// conv_stem_dgrad.hip: input gradient of the stem convolutions (R = 7: 7x7 / 2 / 3; R = 1: 1x7 / 2 / 3 with H = 1); dy is the
// [N][OH][OW][64] gradient of the conv output in the compute dtype, w the fp32 OIHW master weights, dx [N][Cin][H][W] fp32
int ecg_stem_dgrad(int dtype, const void* dy, const float* w, float* dx, int N, int Cin, int H, int W, int R,
                   hipStream_t stream);
// conv_stem_fused.hip: the 2-D stem by recompute (bf16, R = 7, Cin <= 3): conv -> bn -> relu -> max-pool, no full-resolution tensor
bool ecg_stem_fused_ok(int dtype, int Cin, int R);
int ecg_stem_pool_fwd(const float* x, const void* wpk, const float* coef, void* pooled, unsigned char* idx, int N, int Cin,
                      int H, int W, hipStream_t stream);
size_t ecg_stem_pool_bwd_workspace(int N, int Cin, int H, int W);
int ecg_stem_pool_bwd(const float* x, const void* wpk, const float* coef, const float* gamma, const void* dp, const void* pooled,
                      const unsigned char* idx, float* dgamma, float* dbeta, float* dw, void* ws, size_t ws_bytes, int N,
                      int Cin, int H, int W, hipStream_t stream);
// elementwise.hip
int ecg_pool_bn_bwd_reduce(int dtype, const void* dp, const void* pooled, const float* coef, const float* gamma, float* dgamma,
                           float* dbeta, int N, int H, int W, int C, float* scratch, const float** bcoef_out,
                           hipStream_t stream);
int ecg_bn_rows(int dtype, long M, int C);
int ecg_bn_finalize(const float* partial, int rows, int C, double count, const float* gamma, const float* beta,
                    float* rm, float* rv, long long* nbt, float momentum, float eps, float* coef, hipStream_t stream);
int ecg_bn_eval_coef(int C, const float* gamma, const float* beta, const float* rm, const float* rv, float eps,
                     float* coef, hipStream_t stream);
int ecg_col_stats(int dtype, const void* x, long M, int C, float* partial, int* rows_out, hipStream_t stream);
// finalize folded into the consumer (elementwise.hip): the producer's partial rows + what bn_finalize needs
struct EcgBnFold {
  const float* partial; int rows; double count;
  const float* gamma; const float* beta;
  float* rm; float* rv; long long* nbt;   // running statistics (nullable)
  float momentum, eps;
};
bool ecg_bn_fold_ok(int C, int rows);
int ecg_bn_act_fold(int dtype, const void* y, float* coef, const EcgBnFold& f, const void* res, const float* rcoef,
                    const float* gate, int rows_per_sample, int relu, void* out, long M, int C, hipStream_t stream,
                    unsigned char* relu_bits = nullptr);
// relu_bits (nullable; bf16 + relu only): [M][C / 8] bytes, bit j of byte [row][k] = (out[row][8 k + j] > 0) -- the ReLU mask
// for ecg_bn_bwd's mask_bits, 1/16 of the bytes of the activated tensor it would otherwise re-read
int ecg_bn_act(int dtype, const void* y, const float* coef, const void* res, const float* rcoef, const float* gate,
               int rows_per_sample, int relu, void* out, long M, int C, hipStream_t stream, unsigned char* relu_bits = nullptr);
size_t ecg_bn_bwd_scratch(int dtype, long M, int C);
int ecg_bn_bwd(int dtype, const void* dout, const void* maskref, const float* gate, const float* addc,
               int rows_per_sample, const void* y, const float* coef, const float* gamma, float* dgamma, float* dbeta,
               void* dy, void* dz_out, float* dbias, long M, int C, float* scratch, hipStream_t stream,
               const unsigned char* mask_bits = nullptr);
// Two BatchNorm backwards of the same masked gradient dz = [mask] * dout (bn2 and the shortcut BatchNorm of a downsample
// block) in one reduce + one apply pass; results bit-identical to ecg_bn_bwd(dout, mask, ..., y_a, ..., dy_a, dz) followed by
// ecg_bn_bwd(dz, no mask, ..., y_b, ..., dy_b).  gate / addc / dbias must be null.  scratch_a, scratch_b: ecg_bn_bwd_scratch bytes each.
int ecg_bn_bwd_dual(int dtype, const void* dout, const void* maskref, const unsigned char* mask_bits, const float* gate,
                    const float* addc, const void* y_a, const float* coef_a, const float* gamma_a, float* dgamma_a,
                    float* dbeta_a, void* dy_a, const void* y_b, const float* coef_b, const float* gamma_b, float* dgamma_b,
                    float* dbeta_b, void* dy_b, void* dz, float* dbias, long M, int C, float* scratch_a, float* scratch_b,
                    hipStream_t stream);
void ecg_bn_dual_set(int on);   // plans: the dual form where it applies (default on) / the separate calls
bool ecg_bn_dual_on();
int ecg_bn_bwd_tail(int dtype, const void* dout, const void* maskref, const void* y, const float* coef,
                    const float* gamma, float* dgamma, float* dbeta, void* dy, const float* partial, int rows, long M,
                    int C, float* scratch, hipStream_t stream, const float* gate = nullptr, const float* addc = nullptr,
                    int rows_per_sample = 1, float* dbias = nullptr);
// bn_eval_bwd.hip: backward of a BatchNorm whose forward used the running statistics (one pass; operands as ecg_bn_bwd;
// scratch of ecg_bn_bwd_scratch(dtype, M, C) bytes, needed only when a parameter gradient is asked for)
int ecg_bn_eval_bwd(int dtype, const void* dout, const void* maskref, const float* gate, const float* addc,
                    int rows_per_sample, const void* y, const float* coef, float* dgamma, float* dbeta, void* dy,
                    void* dz_out, float* dbias, long M, int C, float* scratch, hipStream_t stream);
int ecg_bn_small_eval_bwd(const float* x, const float* dy, const float* gamma, const float* save, float* dx, float* dgamma,
                          float* dbeta, int N, int C, int accumulate, hipStream_t stream);
// gradcam.hip: relu(channel-weighted sum) / per-sample max, bilinear upsample (align_corners=False) to [N][H][W]
int ecg_gradcam(int dtype, const void* act, const float* dpooled, float* small, float* out, int N, int Hs, int Ws, int C,
                int H, int W, hipStream_t stream);
// the same map from a gradient that varies over space (no global average pool in front of the head): the CRNN's
// sequence layout seq / dseq [B][Tp][C * Fp]; ws = channel weights [B][C] | coarse map [B][Fp][Tp]
size_t ecg_crnn_gradcam_workspace(int B, int Tp, int Fp, int C);
int ecg_crnn_gradcam(const float* seq, const float* dseq, const int* steps, const int* frames, void* ws, size_t ws_bytes,
                     float* cam, int B, int Tp, int C, int Fp, int F, int T, hipStream_t stream);
int ecg_se_gate_bn(int dtype, const void* dout, const void* maskref, const void* y, const float* coef, void* dz,
                   float* dg, float* a1, float* a2, float* a3, int N, int R, int C, hipStream_t stream);
int ecg_se_bn_nrows();   // rows ecg_se_bn_rows writes ([rows][2][C])
int ecg_se_bn_rows(const float* a1, const float* a2, const float* a3, const float* gate, const float* addc, int N, int R,
                   int C, float* rows, hipStream_t stream);
int ecg_rows_sum(const float* partial, int rows, int C, float* out, int accumulate, hipStream_t stream);
int ecg_bnrelu_maxpool(int dtype, const void* y, const float* coef, void* out, unsigned char* idx, int N, int H, int W,
                       int C, hipStream_t stream);
int ecg_maxpool_relu_bwd(int dtype, const void* dp, const void* pooled, const unsigned char* idx, void* dz, int N,
                         int H, int W, int C, hipStream_t stream);
int ecg_pool_bn_bwd(int dtype, const void* dp, const void* pooled, const unsigned char* idx, const void* y,
                    const float* coef, const float* gamma, float* dgamma, float* dbeta, void* dy, float* dbias, int N,
                    int H, int W, int C, float* scratch, hipStream_t stream);
bool ecg_stem_fuse_on();
int ecg_avgpool(int dtype, const void* x, float* out, int N, int R, int C, const float* coef, hipStream_t stream);
int ecg_bcast_rows(int dtype, const float* v, void* out, int N, int R, int C, float scale, hipStream_t stream);
int ecg_se_gate_grad(int dtype, const void* dout, const void* maskref, const void* y, const float* coef, float* dg,
                     int N, int R, int C, hipStream_t stream);
constexpr int ECG_PACK_MAX = 24;
struct EcgPackItem {
  const float* w;  // OIHW / OIL fp32 master weight
  void* fwd;       // [Cout][RS][Cin] compute dtype (nullable)
  void* dgrad;     // [Cin][RS][Cout] compute dtype (nullable)
  int Cout, Cin, RS;
};
int ecg_pack_weight_batch(int dtype, const EcgPackItem* items, int n, hipStream_t stream);
// infer_fold.hip: inference-only kernels.  Fold an eval-mode BatchNorm into the convolution in front of it
// (scale = gamma / sqrt(rv + eps); w' = w * scale[cout] rounded once to the compute dtype; b' = beta + (conv_bias - rm) * scale)
constexpr int ECG_FOLD_MAX = 32;
enum { ECG_FOLD_CONV = 0,    // OIHW / OIL fp32 -> forward pack [Cout][RS][Cin] (the layout of ecg_pack_weight)
       ECG_FOLD_STEM = 1,    // [64][Cin][R][7] fp32 -> stem pack (ecg_stem_pack); RS = R (1 or 7)
       ECG_FOLD_COPY = 2,    // plain fp32 copy of Cout x Cin floats (dense-tail weights kept beside the folded ones)
       ECG_FOLD_OIHW = 3 };  // OIHW fp32 -> OIHW fp32 whatever the dtype: the weight of a kernel that rounds its operands
                             // itself (the CRNN's Cin = 1 convolution), so that rounding stays the only one
struct EcgFoldItem {
  int kind;
  const float* w;
  const float* conv_bias;                 // nullable
  const float *gamma, *beta, *rm, *rv;    // the BatchNorm (unused by ECG_FOLD_COPY)
  void* wout;                             // compute dtype (fp32 for ECG_FOLD_COPY and ECG_FOLD_OIHW)
  float* bout;                            // [Cout] fp32
  float* scale_out;                       // nullable: the scale the kernel used, [Cout] fp32
  int Cout, Cin, RS;
};
int ecg_fold_batch(int dtype, const EcgFoldItem* items, int n, float eps, hipStream_t stream);
// max(0, 3x3 / 2 / 1 max-pool) of a [N][H][W][C] tensor (H = 1: the 1-D 3 / 2 / 1 pool)
int ecg_relu_maxpool(int dtype, const void* y, void* out, int N, int H, int W, int C, hipStream_t stream);
// out = relu(y * gate[row / rows_per_sample][c] + res); out may be y
int ecg_gate_res_relu(int dtype, const void* y, const float* gate, const void* res, void* out, long M, int C,
                      int rows_per_sample, hipStream_t stream);
// plan_resnet1d.hip: switches the ResNet1D_SE backward's weight-gradient side stream (ecgmm_side_wgrad toggles both plans)
int ecg_resnet1d_side_enable(int on);
int ecg_pack_weight(int dtype, const float* w_oihw, void* fwd, void* dgrad, int Cout, int Cin, int RS,
                    hipStream_t stream);
int ecg_nchw_to_nhwc(int dtype, const float* src, void* dst, int N, int C, long HW, hipStream_t stream);
int ecg_nhwc_to_nchw(int dtype, const void* src, float* dst, int N, int C, long HW, hipStream_t stream);
int ecg_cast(int dtype, const float* src, void* dst, long n, hipStream_t stream);
int ecg_uncast(int dtype, const void* src, float* dst, long n, hipStream_t stream);
// head.hip
int ecg_linear_fwd_valu(const float* x, const float* w, const float* bias, float* y, int B, int In, int Out, int act,
                        hipStream_t s);
int ecg_linear_dgrad_valu(const float* dy, const float* w, float* dx, int B, int In, int Out, int accumulate,
                          hipStream_t s);
int ecg_linear_wgrad_valu(const float* dy, const float* x, float* dw, float* db, int B, int In, int Out,
                          int accumulate, hipStream_t s);
int ecg_act_bwd(const float* dy, const float* y, float* dz, long n, int act, hipStream_t s);
int ecg_axpby(float a, const float* x, float b, float* y, long n, hipStream_t s);
int ecg_layernorm_fwd(const float* const* seg, const int* dims, int nseg, const float* fusion_w, const float* gamma,
                      const float* beta, float* out, float* stat, float* soft_w, int B, float eps, hipStream_t s);
size_t ecg_layernorm_bwd_scratch(int B, int D);
int ecg_layernorm_bwd(const float* const* seg, const int* dims, int nseg, const float* fusion_w, const float* gamma,
                      const float* stat, const float* dout, float* const* dseg, int dseg_accumulate, float* dgamma,
                      float* dbeta, float* dfusion_w, int B, float* scratch, hipStream_t s);
// head_fused.hip: the head's row-local work as one kernel per direction + one-wave-per-tile dense kernels
bool ecg_head_fused_ok(const int* dim, int B, int hidden, int num_classes);
int ecg_head_partial_floats(const int* dim, int num_classes);
int ecg_head_bwd_blocks(int B);
int ecg_head_rows_fwd(const float* const* raw, const float* const* ln_g, const float* const* ln_b,
                      const float* const* cls_w, const float* const* cls_b, const float* aw, const float* fg,
                      const float* fb, float* const* feat, float* const* stat, float* const* logits, float* rowvar,
                      float* fused, float* statf, float* soft_w, const int* dim, int B, int NC, float eps,
                      hipStream_t s);
int ecg_head_rows_bwd(const float* const* raw, const float* const* ln_g, const float* const* cls_w, const float* aw,
                      const float* fg, const float* const* feat, const float* const* stat, const float* statf,
                      const float* dfused, const float* const* dlog, const float* dvar, const float* gs,
                      float* const* draw, const int* have, float* partial, const int* dim, int B, int NC,
                      hipStream_t s);
int ecg_head_finalize(const float* partial, int rows, const int* dim, int NC, float* const* g_ln, float* const* g_cls,
                      float* g_aw, float* g_fg, float* g_fb, const float* aw, const int* have, const int* have_cls,
                      int have_fusion, const float* dz, int B, int H, float* fc0_db, hipStream_t s);
bool ecg_se_mlp_fused_ok(int C, int CR);
int ecg_se_mlp_fwd(const float* m, const float* w1, const float* b1, const float* w2, const float* b2, float* h, float* g,
                   int N, int C, int CR, hipStream_t s);
int ecg_se_mlp_bwd(const float* dg, const float* g, const float* h, const float* m, const float* w1, const float* w2,
                   float* ds, float* dh, float* dm, float* dw1, float* db1, float* dw2, float* db2, int N, int C, int CR,
                   float scale, hipStream_t s);
bool ecg_dense16_ok(const void* a, const void* b, const void* c, int B, int In, int Out);
int ecg_dense16_fwd(const float* x, const float* w, const float* bias, float* y, int B, int In, int Out, int act,
                    hipStream_t s);
int ecg_dense16_dgrad(const float* dy, const float* w, float* dx, int B, int In, int Out, hipStream_t s);
int ecg_dense16_wgrad(const float* dy, const float* x, float* dw, int B, int In, int Out, hipStream_t s);
int ecg_fc_dgrad_drop_relu(const float* dlog, const float* w, const unsigned char* mask, const float* hact, float* dz,
                           int B, int H, int NC, float dropout_p, hipStream_t s);
int ecg_varloss_finish(float* scratch, int B, float* loss, hipStream_t s);
int ecg_varloss_fwd(const float* f0, const float* f1, const float* f2, int B, int D0, int D1, int D2, float* loss,
                    float* scratch, hipStream_t s);
int ecg_varloss_bwd(const float* f, int B, int D, const float* gout, const float* scratch, int m, float* df,
                    int accumulate, hipStream_t s);
int ecg_ce_fwd(const float* logits, const long long* labels, int B, int C, int focal, float alpha, float gamma,
               float* loss, float* dcoef, const float* extra, float extra_w, hipStream_t s);
int ecg_ce_bwd(const float* logits, const long long* labels, int B, int C, const float* dcoef, const float* gout,
               float* dlogits, float* dextra, float extra_w, hipStream_t s);
int ecg_dropout_fwd(const float* x, float* y, unsigned char* mask, long n, float p, unsigned long long seed,
                    unsigned long long offset, hipStream_t s);
int ecg_dropout_bwd(const float* dy, const unsigned char* mask, float* dx, long n, float p, hipStream_t s);
int ecg_adam(float* p, const float* g, float* m, float* v, long n, float lr, float b1, float b2, float eps, float wd,
             long step, float gscale, hipStream_t s);

// linear.hip: fp32 Linear that picks the MFMA kernels when the shape allows, the VALU kernels otherwise
size_t ecg_linear_bwd_scratch(int B, int In, int Out);
int ecg_linear_fwd(const float* x, const float* w, const float* bias, float* y, int B, int In, int Out, int act,
                   float* stats, hipStream_t s);
// dz is the gradient w.r.t. the pre-activation output; dx / dw / db may be null
int ecg_linear_bwd(const float* dz, const float* x, const float* w, float* dx, float* dw, float* db, int B, int In,
                   int Out, void* scratch, size_t scratch_bytes, hipStream_t s);

// lstm.hip: nn.LSTM plans (projection GEMMs through ecg_linear_*, the recurrence on lstm_seq_fwd / lstm_seq_bwd kernels)
// dtype: ECGMM_F32 (the exact-fp32 recurrence) or ECGMM_BF16 (recurrent products on bf16 operands, W_hh held on chip)
size_t ecg_lstm_fwd_workspace(const ecgmm_lstm_desc* d, int dtype);
size_t ecg_lstm_bwd_workspace(const ecgmm_lstm_desc* d, int dtype);
int ecg_lstm_ws_view(const ecgmm_lstm_desc* d, int dtype, const char* which, int layer, int direction, size_t* offset,
                     size_t* bytes);
// lengths: device int32 [B] or null (null: the fixed-length kernels, the code of before there were lengths)
int ecg_lstm_forward(const ecgmm_lstm_desc* d, int dtype, const float* x, const int* lengths, const float* const* params,
                     const float* h0, const float* c0, float* y, float* hn, float* cn, void* ws, size_t ws_bytes,
                     hipStream_t s);
int ecg_lstm_backward(const ecgmm_lstm_desc* d, int dtype, const float* x, const int* lengths, const float* const* params,
                      const float* h0, const float* c0, const float* dy, const float* dhn, const float* dcn, const void* ws,
                      float* dx, float* const* grads, float* dh0, float* dc0, void* scratch, size_t scratch_bytes,
                      hipStream_t s);
// mean over each row's own steps of x [B][T][C] and its backward (fixed summation order; len 0 gives 0)
int ecg_seq_mean_varlen_fwd(const float* x, const int* lengths, float* out, int B, int T, int C, hipStream_t s);
int ecg_seq_mean_varlen_bwd(const float* dy, const int* lengths, float* dx, int B, int T, int C, hipStream_t s);

// crnn_front.hip: the CRNN front end's own kernels (train_physionet2.py:55-65, 87-93).  Conv2d(1, 32, 5, pad 2) straight from
// the [N][H][W] fp32 spectrogram; the 5x5 weight gradient (Cin, Cout multiples of 32); [BatchNorm -> ReLU -> MaxPool2d(2)]
int ecg_conv5_in1_stats_rows(int N, int H, int W);
int ecg_conv5_in1_fwd(int dtype, const float* x, const float* w, const float* bias, void* y, float* stats, int N, int H,
                      int W, hipStream_t s);
size_t ecg_conv5_in1_wgrad_workspace(int N, int H, int W);
int ecg_conv5_in1_wgrad(int dtype, const float* x, const void* dy, float* dw, float* db, int accumulate, void* ws,
                        size_t ws_bytes, int N, int H, int W, hipStream_t s);
// dx [N][H][W] fp32 from dy [N][H][W][32] (compute dtype, 16-byte aligned) and w [32][1][5][5]; every element written
int ecg_conv5_in1_dgrad(int dtype, const void* dy, const float* w, float* dx, int N, int H, int W, hipStream_t s);
void ecg_conv5_in1_dgrad_tile(int H, int* strip, int* row_step, int* rows);
size_t ecg_conv5_wgrad_workspace(int dtype, const ConvGeom& g);
int ecg_conv5_wgrad(int dtype, const ConvGeom& g, const void* x, const void* dy, float* dw, int accumulate, void* ws,
                    size_t ws_bytes, hipStream_t s);
int ecg_bnrelu_maxpool2(int dtype, const void* y, const float* coef, void* out, unsigned char* idx, int N, int H, int W, int C,
                        int seq_layout, hipStream_t s);
// inference forms (BatchNorm folded into the convolution): max(0, MaxPool2d(2)) without coefficients / argmax bytes, C a
// multiple of 8 (bf16) / 4 (fp32), same output layouts as ecg_bnrelu_maxpool2; and block 1 as one kernel,
// [N][H][W] fp32 -> [N][H/2][W/2][32], the bits of ecg_conv5_in1_fwd(stats = null) + ecg_relu_maxpool2
int ecg_relu_maxpool2(int dtype, const void* y, void* out, int N, int H, int W, int C, int seq_layout, hipStream_t s);
int ecg_conv5_in1_relu_pool2(int dtype, const float* x, const float* w, const float* bias, void* out, int N, int H, int W,
                             hipStream_t s);
size_t ecg_pool2_bn_bwd_workspace(int N, int H, int W, int C);
int ecg_pool2_bn_bwd(int dtype, const void* dp, const unsigned char* idx, const void* y, const float* coef, int training,
                     float* dgamma, float* dbeta, void* dy, float* dbias, int N, int H, int W, int C, int seq_layout, void* ws,
                     size_t ws_bytes, hipStream_t s);

// transformer_infer.hip: the forward-only tails of a post-norm encoder layer (exact-fp32 MFMA, a wave owns 16 whole rows):
// out = LayerNorm(res + a W^T + bias) and out = LayerNorm(x + relu(x W1^T + b1) W2^T + b2); 16 <= E <= 256, K / FF <= 4096,
// all multiples of 16; every operand 16-byte aligned; out must not alias an input
int ecg_linear_res_ln(const float* a, const float* w, const float* bias, const float* res, const float* gamma,
                      const float* beta, float* out, long R, int K, int E, float eps, hipStream_t s);
int ecg_ffn_res_ln(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, const float* gamma,
                   const float* beta, float* out, long R, int E, int FF, float eps, hipStream_t s);
// out[b][ci][l] = l < lengths[b] ? x[b][ci][l] : 0; and a constant int32 vector
int ecg_mask_pad_rows(const float* x, const int* lengths, float* out, int B, int Cin, int L, hipStream_t s);
int ecg_fill_i32(int* out, int v, int n, hipStream_t s);

// prof.hip
enum { ECG_PROF_IGEMM_FWD = 0, ECG_PROF_IGEMM_DGRAD = 1, ECG_PROF_WGRAD = 2, ECG_PROF_STEM_FWD = 3, ECG_PROF_STEM_WGRAD = 4,
       ECG_PROF_IGEMM_F32_FWD = 5, ECG_PROF_IGEMM_F32_DGRAD = 6 };  // exact-fp32 instantiation (other MFMA peak): own kinds
void ecg_prof_begin(int kind, double flops, double bytes, hipStream_t s);
void ecg_prof_end(hipStream_t s);
void ecg_tl_mark(int id, hipStream_t s);   // diagnostic step timeline (prof.hip); ids: 100 + k forward, 200 + k backward

// What an Arena handed out under a name: a fixed-capacity table on the caller's stack (the workspace views, plan_common.h).
struct WsTable {
  struct Entry { const char* name; int index; size_t off, bytes; };
  Entry e[128];   // (the ResNet18 forward workspace names up to 126 tensors)
  int n = 0;
  bool overflow = false;
};

// bump allocator over a caller-owned workspace (base == nullptr: measure only).  With a table attached, a take made with a
// name (and more than zero bytes) is also recorded there as (name, index, offset, bytes); a layout loop sets `index`.
struct Arena {
  unsigned char* base;
  size_t off;
  WsTable* table;
  int index;
  explicit Arena(void* b, WsTable* t = nullptr) : base((unsigned char*)b), off(0), table(t), index(0) {}
  template <typename T> T* take(size_t count, const char* name = nullptr) {
    off = align_up(off, 256);
    if (table && name && count) {
      if (table->n < (int)(sizeof(table->e) / sizeof(table->e[0]))) table->e[table->n++] = {name, index, off, count * sizeof(T)};
      else table->overflow = true;
    }
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += count * sizeof(T);
    return p;
  }
  void* take_bytes(size_t bytes, const char* name = nullptr) { return take<unsigned char>(bytes, name); }
};
