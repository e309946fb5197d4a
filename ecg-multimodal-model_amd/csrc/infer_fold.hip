// Inference-only kernels (gfx950): BatchNorm folded into the packed conv weights, ReLU + max-pool, SE gate + residual + ReLU.
//
// An eval-mode BatchNorm is a per-channel affine map of the convolution in front of it, so the pair is ONE convolution:
//   scale = gamma / sqrt(running_var + eps)
//   w'    = w * scale[cout]                                  (multiplied in fp32, rounded ONCE to the compute dtype)
//   b'    = beta + (conv_bias - running_mean) * scale        (fp32)
// Nothing is commuted past a ReLU, so negative and zero gamma fold like any other value.  The fold runs once per set of
// weights (ecgmm_*_infer_prepare), not once per forward: all tensors of an encoder go through one batched launch.
#include "ops.h"

namespace {

__device__ __forceinline__ u32x4 ld16(const void* p) { return *reinterpret_cast<const u32x4*>(p); }
__device__ __forceinline__ void st16(void* p, const u32x4& v) { *reinterpret_cast<u32x4*>(p) = v; }

// ------------------------------------------------------------------------------------------------
// batched fold-and-pack
// ------------------------------------------------------------------------------------------------
struct FoldBatch {
  const float* w[ECG_FOLD_MAX];
  const float* cbias[ECG_FOLD_MAX];
  const float* gamma[ECG_FOLD_MAX];
  const float* beta[ECG_FOLD_MAX];
  const float* rm[ECG_FOLD_MAX];
  const float* rv[ECG_FOLD_MAX];
  void* wout[ECG_FOLD_MAX];
  float* bout[ECG_FOLD_MAX];
  float* sout[ECG_FOLD_MAX];
  int kind[ECG_FOLD_MAX], cout[ECG_FOLD_MAX], cin[ECG_FOLD_MAX], rs[ECG_FOLD_MAX];
  int blk0[ECG_FOLD_MAX + 1];  // first block of each item
  int n;
  float eps;
};

constexpr int FOLD_T = 32, FOLD_RS_MAX = 25, FOLD_COPY_PER_BLOCK = 2048;
// the staging tile of a ECG_FOLD_CONV block: FOLD_T output channels of up to 9 taps (every 3x3 / 1x3 / 1x1 convolution), or
// FOLD_CO_WIDE output channels of up to FOLD_RS_MAX taps (the CRNN's 5x5 blocks), FOLD_T input channels each, rows padded by 1
constexpr int FOLD_RS_NARROW = 9, FOLD_CO_WIDE = 8;
constexpr int FOLD_TILE = FOLD_T * (FOLD_T * FOLD_RS_NARROW + 1);
static_assert(FOLD_CO_WIDE * (FOLD_T * FOLD_RS_MAX + 1) <= FOLD_TILE, "the wide tile must fit the staging buffer");
__host__ __device__ inline int fold_co_rows(int RS) { return RS <= FOLD_RS_NARROW ? FOLD_T : FOLD_CO_WIDE; }
__host__ __device__ inline int fold_row_stride(int RS) { return FOLD_T * (RS <= FOLD_RS_NARROW ? FOLD_RS_NARROW : FOLD_RS_MAX) + 1; }

__device__ __forceinline__ float fold_scale(const FoldBatch& b, int t, int co) {
  return b.gamma[t][co] / sqrtf(b.rv[t][co] + b.eps);
}
__device__ __forceinline__ void fold_bias(const FoldBatch& b, int t, int co, float sc) {
  const float cb = b.cbias[t] ? b.cbias[t][co] : 0.f;
  b.bout[t][co] = b.beta[t][co] + (cb - b.rm[t][co]) * sc;
  if (b.sout[t]) b.sout[t][co] = sc;
}

// kind ECG_FOLD_CONV: one block = a 32 (co) x 32 (ci) tile of one tensor with all its taps (8 x 32 above 9 taps), staged
// through LDS as in pack_weight_batch_kernel (elementwise.hip): OIHW rows read in contiguous runs, [co][tap][ci] written
// 32 ci at a time.
// kind ECG_FOLD_STEM: one block = one output channel of the stem layout [64][KP], k = (c * R + r) * 8 + s (conv_stem.hip).
// kind ECG_FOLD_COPY: fp32 copy of a dense tensor (the fc / SE / classifier weights an inference plan reads from its blob).
// kind ECG_FOLD_OIHW: w * scale[cout] in the layout it came in, fp32 out (FOLD_COPY_PER_BLOCK elements per block; the first
//                     block writes the biases).
template <typename T>
__global__ __launch_bounds__(256) void fold_batch_kernel(FoldBatch b) {
  __shared__ float tile[FOLD_TILE];
  __shared__ float s_scale[FOLD_T];
  int t = 0;
  while (t + 1 < b.n && (int)blockIdx.x >= b.blk0[t + 1]) ++t;
  const int lb = blockIdx.x - b.blk0[t];
  const int kind = b.kind[t];
  if (kind == ECG_FOLD_COPY) {
    const long n = (long)b.cout[t] * b.cin[t];
    float* out = (float*)b.wout[t];
    for (long i = (long)lb * FOLD_COPY_PER_BLOCK + threadIdx.x; i < n && i < (long)(lb + 1) * FOLD_COPY_PER_BLOCK; i += 256)
      out[i] = b.w[t][i];
    return;
  }
  if (kind == ECG_FOLD_OIHW) {
    const int per = b.cin[t] * b.rs[t];   // elements per output channel
    const long n = (long)b.cout[t] * per;
    float* out = (float*)b.wout[t];
    for (long i = (long)lb * FOLD_COPY_PER_BLOCK + threadIdx.x; i < n && i < (long)(lb + 1) * FOLD_COPY_PER_BLOCK; i += 256)
      out[i] = b.w[t][i] * fold_scale(b, t, (int)(i / per));
    if (lb == 0)
      for (int co = threadIdx.x; co < b.cout[t]; co += 256) fold_bias(b, t, co, fold_scale(b, t, co));
    return;
  }
  if (kind == ECG_FOLD_STEM) {
    const int NG = b.cin[t] * b.rs[t], KP = ((NG + 3) / 4) * 32, co = lb;   // cin = channels, rs = kernel rows (1 or 7)
    const float sc = fold_scale(b, t, co);
    T* out = (T*)b.wout[t];
    for (int k = threadIdx.x; k < KP; k += 256) {
      const int G = k >> 3, s = k & 7;
      const float v = (G < NG && s < 7) ? b.w[t][((size_t)co * NG + G) * 7 + s] * sc : 0.f;
      Elem<T>::st(out + (size_t)co * KP + k, v);
    }
    if (threadIdx.x == 0) fold_bias(b, t, co, sc);
    return;
  }
  const int Cout = b.cout[t], Cin = b.cin[t], RS = b.rs[t];
  const float* __restrict__ w = b.w[t];
  T* __restrict__ fwd = (T*)b.wout[t];
  const int ci_tiles = (Cin + FOLD_T - 1) / FOLD_T;
  const int co_rows = fold_co_rows(RS), stride = fold_row_stride(RS);
  const int co0 = (lb / ci_tiles) * co_rows, ci0 = (lb % ci_tiles) * FOLD_T;
  const int nci = min(FOLD_T, Cin - ci0), nco = min(co_rows, Cout - co0);
  const int run = nci * RS;
  if (threadIdx.x < nco) {
    const float sc = fold_scale(b, t, co0 + threadIdx.x);
    s_scale[threadIdx.x] = sc;
    if (ci0 == 0) fold_bias(b, t, co0 + threadIdx.x, sc);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nco * run; i += 256) {
    const int co = i / run, k = i - co * run;
    tile[co * stride + k] = w[((size_t)(co0 + co) * Cin + ci0) * RS + k] * s_scale[co];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nco * RS * FOLD_T; i += 256) {
    const int ci = i % FOLD_T, ct = i / FOLD_T, tap = ct % RS, co = ct / RS;
    if (ci < nci) Elem<T>::st(fwd + ((size_t)(co0 + co) * RS + tap) * Cin + ci0 + ci, tile[co * stride + ci * RS + tap]);
  }
}

// ------------------------------------------------------------------------------------------------
// ReLU + 3x3 / stride 2 / pad 1 max-pool (H may be 1: the 1-D 3 / 2 / 1 pool): max(0, max over the window).
// No coefficients and no argmax bytes: an inference forward has no backward to feed.
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void relu_maxpool_kernel(const T* __restrict__ y, T* __restrict__ out, int N, int H, int W,
                                                           int C, int OH, int OW) {
  constexpr int VEC = Elem<T>::VEC;
  const int cpr = C / VEC;
  const long total = (long)N * OH * OW * cpr;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int chunk = (int)(i % cpr);
    const long pix = i / cpr;
    const int ow = (int)(pix % OW);
    const long t = pix / OW;
    const int oh = (int)(t % OH), n = (int)(t / OH);
    const int c0 = chunk * VEC;
    float best[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) best[j] = 0.f;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      const int h = oh * 2 - 1 + kh;
      if ((unsigned)h >= (unsigned)H) continue;
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int w = ow * 2 - 1 + kw;
        if ((unsigned)w >= (unsigned)W) continue;
        float f[VEC];
        unpack16<T>(ld16(y + (((size_t)n * H + h) * W + w) * C + c0), f);
#pragma unroll
        for (int j = 0; j < VEC; ++j) best[j] = f[j] > best[j] ? f[j] : best[j];   // (a NaN input never wins, -0 never wins)
      }
    }
    st16(out + pix * C + c0, pack16<T>(best));
  }
}

// ------------------------------------------------------------------------------------------------
// out = relu(y * gate[n][c] + res): the last pass of a squeeze-excite block whose BatchNorms are folded.  The gate is a
// function of the mean of the WHOLE y over the sample, so this pass cannot move into the convolution's epilogue.
// Each thread keeps a fixed 16-byte channel chunk and walks rows (as bn_act_kernel, elementwise.hip).
// ------------------------------------------------------------------------------------------------
constexpr int GATE_THREADS = 1024;
template <typename T>
__global__ __launch_bounds__(GATE_THREADS) void gate_res_relu_kernel(const T* y, const float* __restrict__ gate,
                                                                     const T* __restrict__ res, T* out, long M,   // (out may be y)
                                                                     int C, int rows_per_sample) {
  constexpr int VEC = Elem<T>::VEC;
  const int cpr = C / VEC, rpi = GATE_THREADS / cpr;
  const int chunk = threadIdx.x % cpr, r0 = threadIdx.x / cpr;
  const int c0 = chunk * VEC;
  for (long r = (long)blockIdx.x * rpi + r0; r < M; r += (long)gridDim.x * rpi) {
    float f[VEC], g[VEC];
    unpack16<T>(ld16(y + r * C + c0), f);
    unpack16<T>(ld16(res + r * C + c0), g);
    const float* gp = gate + (size_t)((unsigned)r / (unsigned)rows_per_sample) * C + c0;   // (rows < 2^31: 32-bit divide)
#pragma unroll
    for (int j = 0; j < VEC; ++j) f[j] = fmaxf(f[j] * gp[j] + g[j], 0.f);
    st16(out + r * C + c0, pack16<T>(f));
  }
}

// rows of whole 16-byte chunks: all relu_maxpool_kernel needs (it finds chunk and pixel of every element by division)
inline bool vec_ok(int C, int dtype) {
  const int vec = dtype == ECGMM_BF16 ? 8 : 4;
  return C >= vec && C % vec == 0;
}
// ... and a workgroup that is whole rows of them: gate_res_relu_kernel's threads keep one chunk each (rpi = threads / cpr)
inline bool chunk_ok(int C, int dtype, int threads) {
  if (!vec_ok(C, dtype)) return false;
  const int cpr = C / (dtype == ECGMM_BF16 ? 8 : 4);
  return cpr <= threads && threads % cpr == 0;
}

}  // namespace

int ecg_fold_batch(int dtype, const EcgFoldItem* items, int n, float eps, hipStream_t stream) {
  if (dtype != ECGMM_BF16 && dtype != ECGMM_F32) ECG_FAIL(ECGMM_ERR_DTYPE, "fold: bad dtype %d", dtype);
  if (n < 1 || n > ECG_FOLD_MAX) ECG_FAIL(ECGMM_ERR_SHAPE, "fold: %d items (1..%d)", n, ECG_FOLD_MAX);
  if (!(eps >= 0.f)) ECG_FAIL(ECGMM_ERR_SHAPE, "fold: eps %g", (double)eps);
  FoldBatch b;
  memset(&b, 0, sizeof(b));
  b.n = n;
  b.eps = eps;
  int blocks = 0;
  for (int i = 0; i < n; ++i) {
    const EcgFoldItem& it = items[i];
    if (!it.w || !it.wout) ECG_FAIL(ECGMM_ERR_SHAPE, "fold: item %d has a null weight pointer", i);
    if (it.Cout < 1 || it.Cin < 1) ECG_FAIL(ECGMM_ERR_SHAPE, "fold: item %d has shape %d x %d", i, it.Cout, it.Cin);
    b.blk0[i] = blocks;
    if (it.kind == ECG_FOLD_COPY) {
      blocks += ceil_div((long)it.Cout * it.Cin, FOLD_COPY_PER_BLOCK);
    } else {
      if (!it.gamma || !it.beta || !it.rm || !it.rv || !it.bout)
        ECG_FAIL(ECGMM_ERR_SHAPE, "fold: item %d lacks a BatchNorm tensor or the bias output", i);
      if (it.kind == ECG_FOLD_STEM) {
        if (it.Cout != 64 || (it.RS != 1 && it.RS != 7))
          ECG_FAIL(ECGMM_ERR_SHAPE, "fold: stem item %d needs 64 output channels and 1 or 7 kernel rows", i);
        blocks += 64;
      } else if (it.kind == ECG_FOLD_CONV) {
        if (it.RS < 1 || it.RS > FOLD_RS_MAX) ECG_FAIL(ECGMM_ERR_SHAPE, "fold: %d taps unsupported (1..%d)", it.RS, FOLD_RS_MAX);
        blocks += ceil_div(it.Cout, fold_co_rows(it.RS)) * ceil_div(it.Cin, FOLD_T);
      } else if (it.kind == ECG_FOLD_OIHW) {
        if (it.RS < 1 || (long)it.Cout * it.Cin * it.RS > 0x7fffffffL) ECG_FAIL(ECGMM_ERR_SHAPE, "fold: item %d has %d taps", i, it.RS);
        blocks += ceil_div((long)it.Cout * it.Cin * it.RS, FOLD_COPY_PER_BLOCK);
      } else {
        ECG_FAIL(ECGMM_ERR_SHAPE, "fold: item %d has kind %d", i, it.kind);
      }
    }
    b.w[i] = it.w; b.cbias[i] = it.conv_bias; b.gamma[i] = it.gamma; b.beta[i] = it.beta; b.rm[i] = it.rm; b.rv[i] = it.rv;
    b.wout[i] = it.wout; b.bout[i] = it.bout; b.sout[i] = it.scale_out;
    b.kind[i] = it.kind; b.cout[i] = it.Cout; b.cin[i] = it.Cin; b.rs[i] = it.RS;
  }
  b.blk0[n] = blocks;
  if (dtype == ECGMM_BF16) hipLaunchKernelGGL(fold_batch_kernel<bf16_t>, dim3(blocks), dim3(256), 0, stream, b);
  else hipLaunchKernelGGL(fold_batch_kernel<float>, dim3(blocks), dim3(256), 0, stream, b);
  ECG_CHECK_LAUNCH("fold_batch");
  return 0;
}

int ecg_relu_maxpool(int dtype, const void* y, void* out, int N, int H, int W, int C, hipStream_t stream) {
  if (dtype != ECGMM_BF16 && dtype != ECGMM_F32) ECG_FAIL(ECGMM_ERR_DTYPE, "relu_maxpool: bad dtype %d", dtype);
  if (!y || !out) ECG_FAIL(ECGMM_ERR_SHAPE, "relu_maxpool: null operand");
  if (N < 1 || H < 1 || W < 1) ECG_FAIL(ECGMM_ERR_SHAPE, "relu_maxpool: bad shape %d x %d x %d", N, H, W);
  if (!vec_ok(C, dtype)) ECG_FAIL(ECGMM_ERR_SHAPE, "relu_maxpool: C=%d unsupported", C);
  const int OH = (H + 2 - 3) / 2 + 1, OW = (W + 2 - 3) / 2 + 1;
  const int vec = dtype == ECGMM_BF16 ? 8 : 4;
  long blocks = ((long)N * OH * OW * (C / vec) + 255) / 256;
  const int grid = (int)(blocks > 4096 ? 4096 : blocks);
  if (dtype == ECGMM_BF16)
    hipLaunchKernelGGL(relu_maxpool_kernel<bf16_t>, dim3(grid), dim3(256), 0, stream, (const bf16_t*)y, (bf16_t*)out, N, H, W,
                       C, OH, OW);
  else
    hipLaunchKernelGGL(relu_maxpool_kernel<float>, dim3(grid), dim3(256), 0, stream, (const float*)y, (float*)out, N, H, W, C,
                       OH, OW);
  ECG_CHECK_LAUNCH("relu_maxpool");
  return 0;
}

int ecg_gate_res_relu(int dtype, const void* y, const float* gate, const void* res, void* out, long M, int C,
                      int rows_per_sample, hipStream_t stream) {
  if (dtype != ECGMM_BF16 && dtype != ECGMM_F32) ECG_FAIL(ECGMM_ERR_DTYPE, "gate_res_relu: bad dtype %d", dtype);
  if (!y || !gate || !res || !out) ECG_FAIL(ECGMM_ERR_SHAPE, "gate_res_relu: null operand");
  if (M < 1 || M > 0x7fffffffL || rows_per_sample < 1 || M % rows_per_sample) ECG_FAIL(ECGMM_ERR_SHAPE, "gate_res_relu: %ld rows / %d per sample", M, rows_per_sample);
  if (!chunk_ok(C, dtype, GATE_THREADS)) ECG_FAIL(ECGMM_ERR_SHAPE, "gate_res_relu: C=%d unsupported", C);
  const int vec = dtype == ECGMM_BF16 ? 8 : 4, rpi = GATE_THREADS / (C / vec);
  long blocks = (M + (long)rpi * 4 - 1) / ((long)rpi * 4);
  const int grid = (int)(blocks > 2048 ? 2048 : blocks);
  if (dtype == ECGMM_BF16)
    hipLaunchKernelGGL(gate_res_relu_kernel<bf16_t>, dim3(grid), dim3(GATE_THREADS), 0, stream, (const bf16_t*)y, gate,
                       (const bf16_t*)res, (bf16_t*)out, M, C, rows_per_sample);
  else
    hipLaunchKernelGGL(gate_res_relu_kernel<float>, dim3(grid), dim3(GATE_THREADS), 0, stream, (const float*)y, gate,
                       (const float*)res, (float*)out, M, C, rows_per_sample);
  ECG_CHECK_LAUNCH("gate_res_relu");
  return 0;
}
