// Forward-only tails of a post-norm TransformerEncoderLayer (train_physionet.py:219) for the inference plan of
// ECGTransformer1D (plan_infer.hip), exact fp32 on v_mfma_f32_16x16x4_f32:
//   ecg_linear_res_ln : out = LayerNorm(res + a W^T + b)                       (out_proj + residual + norm1, one launch)
//   ecg_ffn_res_ln    : out = LayerNorm(x + relu(x W1^T + b1) W2^T + b2)       (feed-forward + residual + norm2, one launch)
//   ecg_mask_pad_rows / ecg_fill_i32 : plumbing of the plan (raw padding -> 0; a constant lengths vector)
//
// Layout.  A wave owns 16 rows and ALL E output features of them; a workgroup is four such waves (64 rows) that share
// nothing but the L1 hits on the weights, so there is no LDS and no barrier.  Every product is computed TRANSPOSED:
// the weight tile is the A operand (16 output features x 4 k), the activation tile the B operand (4 k x 16 rows), so in the
// result lane l holds, of data row l & 15, the four features 4 (l >> 4) + reg of each 16-feature tile:
//   * a row's E values sit in the registers of the four lanes {c, c + 16, c + 32, c + 48}: its mean and its centred sum of
//     squares are a sum over own registers and two cross-lane exchanges (xor 16, xor 32), nothing leaves the wave;
//   * the contraction index of an MFMA is a free permutation, so the hidden tile relu(x W1^T + b1)^T feeds the second
//     product as it stands: register `reg` is the B operand of the k-step whose A operand is W2[i][16 c + 4 (l >> 4) + reg],
//     which is one float4 load of W2's row.  The hidden activation never leaves the registers;
//   * the same permutation makes every operand load a float4: lane l reads [row][16 kb + 4 (l >> 4) .. + 3].
// The x tile of ecg_ffn_res_ln doubles as the residual: xb[t][reg] IS x[row][16 t + 4 (l >> 4) + reg].
// A row's arithmetic touches its own column of every MFMA and the weights alone, in a fixed order: its bits depend neither
// on R nor on where in a tile it sits, and there are no atomics.
// NT = compile-time feature-tile capacity (E <= 16 NT); E / 16 tiles are live, tested with wave-uniform guards that fold away
// in the FULL instantiations (E == 16 NT: 16, 32, 64, 128, 256).
#include "ops.h"

namespace {

constexpr int TI_WAVES = 4;               // waves per workgroup
constexpr int TI_ROWS = 16 * TI_WAVES;    // rows per workgroup

__device__ __forceinline__ f32x4 mfma4(const float4& a, const float4& b, f32x4 c) {
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, c, 0, 0, 0);
  return c;
}
__device__ __forceinline__ f32x4 mfma4(const float4& a, const f32x4& b, f32x4 c) {
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b[0], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b[1], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b[2], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b[3], c, 0, 0, 0);
  return c;
}
__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// the sum over the four lanes that hold one row; every one of them ends with the same bits (float addition commutes)
__device__ __forceinline__ float row4_sum(float v) {
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}

// z[t][reg] = the pre-norm value of feature 16 t + 4 g + reg of this lane's row -> normalised, scaled, shifted, stored
template <int NT>
__device__ __forceinline__ void ln_store(float (&z)[NT][4], int nt, int E, int g, const float* gamma, const float* beta,
                                         float eps, float* orow, bool live) {
  float s = 0.f;
#pragma unroll
  for (int t = 0; t < NT; ++t)
    if (t < nt) s += (z[t][0] + z[t][1]) + (z[t][2] + z[t][3]);
  const float mean = row4_sum(s) / (float)E;
  float q = 0.f;
#pragma unroll
  for (int t = 0; t < NT; ++t)
    if (t < nt) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        z[t][i] -= mean;
        q = fmaf(z[t][i], z[t][i], q);
      }
    }
  const float rstd = rsqrtf(row4_sum(q) / (float)E + eps);
#pragma unroll
  for (int t = 0; t < NT; ++t)
    if (t < nt) {
      const float4 ga = ld4(gamma + 16 * t + 4 * g), be = ld4(beta + 16 * t + 4 * g);
      float4 y;
      y.x = fmaf(z[t][0] * rstd, ga.x, be.x);
      y.y = fmaf(z[t][1] * rstd, ga.y, be.y);
      y.z = fmaf(z[t][2] * rstd, ga.z, be.z);
      y.w = fmaf(z[t][3] * rstd, ga.w, be.w);
      if (live) *reinterpret_cast<float4*>(orow + 16 * t + 4 * g) = y;
    }
}

template <int NT, bool FULL>
__global__ __launch_bounds__(64 * TI_WAVES) void linear_res_ln_kernel(const float* __restrict__ a, const float* __restrict__ W,
                                                                      const float* __restrict__ bias, const float* __restrict__ res,
                                                                      const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                      float* __restrict__ out, long R, int K, int E, float eps) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = lane & 15, g = lane >> 4;
  const long row0 = ((long)blockIdx.x * TI_WAVES + wave) * 16;
  if (row0 >= R) return;                         // wave-uniform; the kernel has no barrier
  const long r = row0 + c;
  const bool live = r < R;
  const long rl = live ? r : R - 1;              // a dead lane re-reads the last row and stores nothing
  const int nt = FULL ? NT : E >> 4;   // FULL: E == 16 NT, every guard folds away
  f32x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float* ap = a + (size_t)rl * K + 4 * g;
  const float* wp = W + (size_t)c * K + 4 * g;
#pragma unroll 1
  for (int k0 = 0; k0 < K; k0 += 16) {
    const float4 b4 = ld4(ap + k0);
    float4 w4[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
      if (t < nt) w4[t] = ld4(wp + (size_t)t * 16 * K + k0);
#pragma unroll
    for (int t = 0; t < NT; ++t)
      if (t < nt) acc[t] = mfma4(w4[t], b4, acc[t]);
  }
  float z[NT][4];
#pragma unroll
  for (int t = 0; t < NT; ++t)
    if (t < nt) {
      const float4 bi = ld4(bias + 16 * t + 4 * g), re = ld4(res + (size_t)rl * E + 16 * t + 4 * g);
      z[t][0] = (acc[t][0] + bi.x) + re.x;
      z[t][1] = (acc[t][1] + bi.y) + re.y;
      z[t][2] = (acc[t][2] + bi.z) + re.z;
      z[t][3] = (acc[t][3] + bi.w) + re.w;
    }
  ln_store<NT>(z, nt, E, g, gamma, beta, eps, out + (size_t)rl * E, live);
}

template <int NT, bool FULL>
__global__ __launch_bounds__(64 * TI_WAVES) void ffn_res_ln_kernel(const float* __restrict__ x, const float* __restrict__ W1,
                                                                   const float* __restrict__ b1, const float* __restrict__ W2,
                                                                   const float* __restrict__ b2, const float* __restrict__ gamma,
                                                                   const float* __restrict__ beta, float* __restrict__ out, long R,
                                                                   int E, int FF, float eps) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = lane & 15, g = lane >> 4;
  const long row0 = ((long)blockIdx.x * TI_WAVES + wave) * 16;
  if (row0 >= R) return;
  const long r = row0 + c;
  const bool live = r < R;
  const long rl = live ? r : R - 1;
  const int nt = FULL ? NT : E >> 4, nc = FF >> 4;
  float4 xb[NT];
  f32x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    xb[t] = t < nt ? ld4(x + (size_t)rl * E + 16 * t + 4 * g) : float4{0.f, 0.f, 0.f, 0.f};
  }
  // two 16-unit chunks of the hidden layer per trip: two independent accumulator chains in the first product; the second
  // product adds them to acc in chunk order, so the pairing does not show in the bits
#pragma unroll 1
  for (int cc = 0; cc < nc; cc += 2) {
    const bool two = cc + 1 < nc;
    f32x4 h0 = {0.f, 0.f, 0.f, 0.f}, h1 = {0.f, 0.f, 0.f, 0.f};
    const float* w1p = W1 + (size_t)(16 * cc + c) * E + 4 * g;
#pragma unroll
    for (int t = 0; t < NT; ++t)
      if (t < nt) {
        h0 = mfma4(ld4(w1p + 16 * t), xb[t], h0);
        if (two) h1 = mfma4(ld4(w1p + (size_t)16 * E + 16 * t), xb[t], h1);
      }
    const float4 ba = ld4(b1 + 16 * cc + 4 * g);
    h0[0] = fmaxf(h0[0] + ba.x, 0.f); h0[1] = fmaxf(h0[1] + ba.y, 0.f);
    h0[2] = fmaxf(h0[2] + ba.z, 0.f); h0[3] = fmaxf(h0[3] + ba.w, 0.f);
    if (two) {
      const float4 bb = ld4(b1 + 16 * cc + 16 + 4 * g);
      h1[0] = fmaxf(h1[0] + bb.x, 0.f); h1[1] = fmaxf(h1[1] + bb.y, 0.f);
      h1[2] = fmaxf(h1[2] + bb.z, 0.f); h1[3] = fmaxf(h1[3] + bb.w, 0.f);
    }
    const float* w2p = W2 + (size_t)c * FF + 16 * cc + 4 * g;
#pragma unroll
    for (int t = 0; t < NT; ++t)
      if (t < nt) {
        acc[t] = mfma4(ld4(w2p + (size_t)t * 16 * FF), h0, acc[t]);
        if (two) acc[t] = mfma4(ld4(w2p + (size_t)t * 16 * FF + 16), h1, acc[t]);
      }
  }
  float z[NT][4];
#pragma unroll
  for (int t = 0; t < NT; ++t)
    if (t < nt) {
      const float4 bi = ld4(b2 + 16 * t + 4 * g);
      z[t][0] = (acc[t][0] + bi.x) + xb[t].x;
      z[t][1] = (acc[t][1] + bi.y) + xb[t].y;
      z[t][2] = (acc[t][2] + bi.z) + xb[t].z;
      z[t][3] = (acc[t][3] + bi.w) + xb[t].w;
    }
  ln_store<NT>(z, nt, E, g, gamma, beta, eps, out + (size_t)rl * E, live);
}

// out[b][ci][l] = l < clamp(lengths[b], 0, L) ? x[b][ci][l] : 0   (what ECGTransformer1D.forward's masked_fill does)
__global__ __launch_bounds__(256) void mask_pad_rows_kernel(const float* __restrict__ x, const int* __restrict__ lengths,
                                                            float* __restrict__ out, int Cin, int L, long total) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long row = i / L;
    const int l = (int)(i - row * L);
    out[i] = l < lengths[row / Cin] ? x[i] : 0.f;
  }
}
__global__ __launch_bounds__(256) void fill_i32_kernel(int* __restrict__ out, int v, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = v;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int tail_shape(const char* what, long R, int E, const char* kname, int K) {
  if (R < 1) ECG_FAIL(ECGMM_ERR_SHAPE, "%s: R=%ld rows (needs R >= 1)", what, R);
  if (E < 16 || E > 256 || E % 16)
    ECG_FAIL(ECGMM_ERR_SHAPE, "%s: E=%d (needs a multiple of 16 with 16 <= E <= 256)", what, E);
  if (K < 16 || K > 4096 || K % 16)
    ECG_FAIL(ECGMM_ERR_SHAPE, "%s: %s=%d (needs a multiple of 16 with 16 <= %s <= 4096)", what, kname, K, kname);
  if (R > ((long)1 << 31) / TI_ROWS * TI_ROWS) ECG_FAIL(ECGMM_ERR_SHAPE, "%s: R=%ld rows is too large", what, R);
  return 0;
}

}  // namespace

#define TI_LAUNCH(KERNEL, N, ...)                                                                                  \
  do {                                                                                                             \
    if (E == 16 * N) hipLaunchKernelGGL((KERNEL<N, true>), grid_, block_, 0, s, __VA_ARGS__);                      \
    else hipLaunchKernelGGL((KERNEL<N, false>), grid_, block_, 0, s, __VA_ARGS__);                                 \
  } while (0)
#define TI_DISPATCH(KERNEL, ...)                                                                                   \
  do {                                                                                                             \
    const dim3 grid_((unsigned)((R + TI_ROWS - 1) / TI_ROWS)), block_(64 * TI_WAVES);                              \
    if (E <= 16) TI_LAUNCH(KERNEL, 1, __VA_ARGS__);                                                                \
    else if (E <= 32) TI_LAUNCH(KERNEL, 2, __VA_ARGS__);                                                           \
    else if (E <= 64) TI_LAUNCH(KERNEL, 4, __VA_ARGS__);                                                           \
    else if (E <= 128) TI_LAUNCH(KERNEL, 8, __VA_ARGS__);                                                          \
    else TI_LAUNCH(KERNEL, 16, __VA_ARGS__);                                                                       \
  } while (0)

int ecg_linear_res_ln(const float* a, const float* w, const float* bias, const float* res, const float* gamma,
                      const float* beta, float* out, long R, int K, int E, float eps, hipStream_t s) {
  ECG_TRY(tail_shape("linear_res_ln", R, E, "K", K));
  if (!(eps >= 0.f)) ECG_FAIL(ECGMM_ERR_SHAPE, "linear_res_ln: eps %g (needs eps >= 0)", (double)eps);
  if (!a || !w || !bias || !res || !gamma || !beta || !out) ECG_FAIL(ECGMM_ERR_SHAPE, "linear_res_ln: null operand");
  if (out == res || out == a)
    ECG_FAIL(ECGMM_ERR_SHAPE, "linear_res_ln: out must not alias res or a (in-place operation is not supported)");
  if (!aligned16(a) || !aligned16(w) || !aligned16(bias) || !aligned16(res) || !aligned16(gamma) || !aligned16(beta) ||
      !aligned16(out))
    ECG_FAIL(ECGMM_ERR_SHAPE, "linear_res_ln: every operand must be 16-byte aligned");
  TI_DISPATCH(linear_res_ln_kernel, a, w, bias, res, gamma, beta, out, R, K, E, eps);
  ECG_CHECK_LAUNCH("linear_res_ln");
  return 0;
}

int ecg_ffn_res_ln(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, const float* gamma,
                   const float* beta, float* out, long R, int E, int FF, float eps, hipStream_t s) {
  ECG_TRY(tail_shape("ffn_res_ln", R, E, "ff", FF));
  if (!(eps >= 0.f)) ECG_FAIL(ECGMM_ERR_SHAPE, "ffn_res_ln: eps %g (needs eps >= 0)", (double)eps);
  if (!x || !w1 || !b1 || !w2 || !b2 || !gamma || !beta || !out) ECG_FAIL(ECGMM_ERR_SHAPE, "ffn_res_ln: null operand");
  if (out == x) ECG_FAIL(ECGMM_ERR_SHAPE, "ffn_res_ln: out must not alias x (in-place operation is not supported)");
  if (!aligned16(x) || !aligned16(w1) || !aligned16(b1) || !aligned16(w2) || !aligned16(b2) || !aligned16(gamma) ||
      !aligned16(beta) || !aligned16(out))
    ECG_FAIL(ECGMM_ERR_SHAPE, "ffn_res_ln: every operand must be 16-byte aligned");
  TI_DISPATCH(ffn_res_ln_kernel, x, w1, b1, w2, b2, gamma, beta, out, R, E, FF, eps);
  ECG_CHECK_LAUNCH("ffn_res_ln");
  return 0;
}

int ecg_mask_pad_rows(const float* x, const int* lengths, float* out, int B, int Cin, int L, hipStream_t s) {
  if (!x || !lengths || !out || B < 1 || Cin < 1 || L < 1) ECG_FAIL(ECGMM_ERR_SHAPE, "mask_pad_rows: null operand or empty shape");
  const long total = (long)B * Cin * L;
  const long blocks = (total + 255) / 256;
  hipLaunchKernelGGL(mask_pad_rows_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, s, x, lengths, out,
                     Cin, L, total);
  ECG_CHECK_LAUNCH("mask_pad_rows");
  return 0;
}

int ecg_fill_i32(int* out, int v, int n, hipStream_t s) {
  if (!out || n < 1) ECG_FAIL(ECGMM_ERR_SHAPE, "fill_i32: null operand or empty shape");
  hipLaunchKernelGGL(fill_i32_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, s, out, v, n);
  ECG_CHECK_LAUNCH("fill_i32");
  return 0;
}

/* train_physionet.py:219-220, 236 in eval mode: out_proj + residual + norm1 of each encoder layer */
extern "C" int ecgmm_linear_res_ln(const float* a, const float* w, const float* bias, const float* res, const float* gamma,
                                   const float* beta, float* out, int64_t R, int K, int E, float eps, void* stream) {
  return ecg_linear_res_ln(a, w, bias, res, gamma, beta, out, (long)R, K, E, eps, (hipStream_t)stream);
}

/* train_physionet.py:219-220, 236 in eval mode: linear1 + ReLU + linear2 + residual + norm2 of each encoder layer */
extern "C" int ecgmm_ffn_res_ln(const float* x, const float* w1, const float* b1, const float* w2, const float* b2,
                                const float* gamma, const float* beta, float* out, int64_t R, int E, int ff, float eps,
                                void* stream) {
  return ecg_ffn_res_ln(x, w1, b1, w2, b2, gamma, beta, out, (long)R, E, ff, eps, (hipStream_t)stream);
}
