// BatchNorm backward through an EVAL-mode forward (running statistics), gfx950.
// In eval mode nn.BatchNorm{1,2}d is a per-channel affine map with constant coefficients, y_bn = y * scale_c + shift_c
// (scale_c = gamma_c * rstd_c from the running variance), so its backward has no batch-mean correction terms:
//     g      = [maskref > 0] * dout * [gate[n][c]] + [addc[n][c]]          (each factor optional, as ecg_bn_bwd)
//     dy     = g * scale_c
//     dbeta  = sum g,   dgamma = sum g * (y - running_mean) * rstd,   dbias = sum dy (a Conv1d bias in front of the BN)
// One pass over (dout, [maskref], y) instead of the training backward's reduce + apply; the per-channel sums are only
// taken when a parameter gradient is asked for (an attribution pass asks for none: the pass is then a masked scale).
// Same operand conventions as ecg_bn_bwd (elementwise.hip) so that the encoder plans swap one call for the other.
#include "ops.h"

namespace {

constexpr int EB_THREADS = 256;

struct BnEvalBwdParams {
  const void* dout;
  const void* maskref;   // nullable; == y: mask = (bn(y) > 0), recomputed through the affine
  const float* gate;     // nullable [N][C]
  const float* addc;     // nullable [N][C]
  const void* y;
  const float* coef;     // forward coef [4][C]: scale, shift, mean, invstd
  void* dy;
  void* dz_out;          // nullable: the masked gradient before gate / addc (the residual branch's gradient)
  float* partial;        // nullable [grid][3][C]: sum g, sum g * xhat, sum dy
  long M;
  int C, rows_per_sample;
};

template <typename T>
__global__ __launch_bounds__(EB_THREADS) void bn_eval_bwd_kernel(BnEvalBwdParams p) {
  constexpr int VEC = Elem<T>::VEC;
  extern __shared__ float eb_shm[];   // [EB_THREADS][3 * VEC + 1] (sums only)
  const int cpr = p.C / VEC, rpi = EB_THREADS / cpr;
  const int chunk = threadIdx.x % cpr, r0 = threadIdx.x / cpr;
  const int c0 = chunk * VEC;
  float sc[VEC], sh[VEC], mean[VEC], inv[VEC], a1[VEC], a2[VEC], a3[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    sc[j] = p.coef[c0 + j];
    sh[j] = p.coef[p.C + c0 + j];
    mean[j] = p.coef[2 * p.C + c0 + j];
    inv[j] = p.coef[3 * p.C + c0 + j];
    a1[j] = a2[j] = a3[j] = 0.f;
  }
  const T* dout = (const T*)p.dout;
  const T* mref = (const T*)p.maskref;
  const T* y = (const T*)p.y;
  const bool need_y = p.partial != nullptr || mref == y;
  for (long r = (long)blockIdx.x * rpi + r0; r < p.M; r += (long)gridDim.x * rpi) {
    float d[VEC], m[VEC], v[VEC];
    unpack16<T>(*reinterpret_cast<const u32x4*>(dout + r * p.C + c0), d);
    if (need_y) unpack16<T>(*reinterpret_cast<const u32x4*>(y + r * p.C + c0), v);
    if (mref == y) {
#pragma unroll
      for (int j = 0; j < VEC; ++j) d[j] = (v[j] * sc[j] + sh[j]) > 0.f ? d[j] : 0.f;
    } else if (mref) {
      unpack16<T>(*reinterpret_cast<const u32x4*>(mref + r * p.C + c0), m);
#pragma unroll
      for (int j = 0; j < VEC; ++j) d[j] = m[j] > 0.f ? d[j] : 0.f;
    }
    if (p.dz_out) *reinterpret_cast<u32x4*>((T*)p.dz_out + r * p.C + c0) = pack16<T>(d);
    if (p.gate) {
      const float* gp = p.gate + (r / p.rows_per_sample) * p.C + c0;
#pragma unroll
      for (int j = 0; j < VEC; ++j) d[j] *= gp[j];
    }
    if (p.addc) {
      const float* ap = p.addc + (r / p.rows_per_sample) * p.C + c0;
#pragma unroll
      for (int j = 0; j < VEC; ++j) d[j] += ap[j];
    }
    float o[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) o[j] = d[j] * sc[j];
    const u32x4 pk = pack16<T>(o);
    *reinterpret_cast<u32x4*>((T*)p.dy + r * p.C + c0) = pk;
    if (p.partial) {
      float back[VEC];
      unpack16<T>(pk, back);   // the bias gradient sums what was actually stored, as the training backward does
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        a1[j] += d[j];
        a2[j] += d[j] * ((v[j] - mean[j]) * inv[j]);
        a3[j] += back[j];
      }
    }
  }
  if (p.partial) {
    constexpr int SW = 3 * VEC + 1;
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      eb_shm[threadIdx.x * SW + j] = a1[j];
      eb_shm[threadIdx.x * SW + VEC + j] = a2[j];
      eb_shm[threadIdx.x * SW + 2 * VEC + j] = a3[j];
    }
    __syncthreads();
    for (int o = threadIdx.x; o < 3 * p.C; o += EB_THREADS) {
      const int which = o / p.C, c = o % p.C;
      const int ck = c / VEC, j = c % VEC;
      float s = 0.f;
      for (int k = 0; k < rpi; ++k) s += eb_shm[(k * cpr + ck) * SW + which * VEC + j];
      p.partial[(size_t)blockIdx.x * 3 * p.C + o] = s;
    }
  }
}

// rows of [rows][3][C] -> dbeta, dgamma, dbias (each nullable), summed in double in a fixed order
__global__ __launch_bounds__(256) void bn_eval_bwd_finalize_kernel(const float* __restrict__ partial, int rows, int C,
                                                                   float* dgamma, float* dbeta, float* dbias) {
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= 3 * C) return;
  const int which = o / C, c = o % C;
  float* out = which == 0 ? dbeta : which == 1 ? dgamma : dbias;
  if (!out) return;
  double s = 0.0;
  for (int r = 0; r < rows; ++r) s += (double)partial[(size_t)r * 3 * C + o];
  out[c] = (float)s;
}

// small [N][C] fp32 matrices of any C (the clinical branches: one workgroup per channel, as bn_small_* of tabnet.hip):
// save = [2][C] running mean, invstd as the eval forward stored them
__global__ __launch_bounds__(256) void bn_small_eval_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                const float* __restrict__ gamma,
                                                                const float* __restrict__ save, float* __restrict__ dx,
                                                                float* dgamma, float* dbeta, int N, int C, int accumulate) {
  __shared__ double sh[2][256];
  const int c = blockIdx.x, tid = threadIdx.x;
  const float mean = save[c], invstd = save[C + c];
  const float sc = (gamma ? gamma[c] : 1.f) * invstd;
  double s1 = 0.0, s2 = 0.0;
  for (int n = tid; n < N; n += 256) {
    const float g = dy[(size_t)n * C + c];
    if (dx) dx[(size_t)n * C + c] = g * sc;
    s1 += (double)g;
    s2 += (double)(g * ((x[(size_t)n * C + c] - mean) * invstd));
  }
  if (!dgamma && !dbeta) return;
  sh[0][tid] = s1;
  sh[1][tid] = s2;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      sh[0][tid] += sh[0][tid + o];
      sh[1][tid] += sh[1][tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    if (dbeta) dbeta[c] = (accumulate ? dbeta[c] : 0.f) + (float)sh[0][0];
    if (dgamma) dgamma[c] = (accumulate ? dgamma[c] : 0.f) + (float)sh[1][0];
  }
}

}  // namespace

int ecg_bn_small_eval_bwd(const float* x, const float* dy, const float* gamma, const float* save, float* dx, float* dgamma,
                          float* dbeta, int N, int C, int accumulate, hipStream_t stream) {
  if (N < 1 || C < 1) ECG_FAIL(ECGMM_ERR_SHAPE, "bn_small_eval_bwd: empty input");
  if (!x || !dy || !save) ECG_FAIL(ECGMM_ERR_SHAPE, "bn_small_eval_bwd: null operand");
  hipLaunchKernelGGL(bn_small_eval_bwd_kernel, dim3(C), dim3(256), 0, stream, x, dy, gamma, save, dx, dgamma, dbeta, N, C,
                     accumulate);
  ECG_CHECK_LAUNCH("bn_small_eval_bwd");
  return 0;
}

// scratch: what ecg_bn_bwd_scratch(dtype, M, C) returns is enough (the plans share one buffer between the two modes)
int ecg_bn_eval_bwd(int dtype, const void* dout, const void* maskref, const float* gate, const float* addc,
                    int rows_per_sample, const void* y, const float* coef, float* dgamma, float* dbeta, void* dy,
                    void* dz_out, float* dbias, long M, int C, float* scratch, hipStream_t stream) {
  const int vec = dtype == ECGMM_BF16 ? 8 : 4;
  if (dtype != ECGMM_BF16 && dtype != ECGMM_F32) ECG_FAIL(ECGMM_ERR_DTYPE, "bn_eval_bwd: bad dtype %d", dtype);
  if (C < vec || C % vec != 0 || EB_THREADS % (C / vec) != 0 || C > 512)
    ECG_FAIL(ECGMM_ERR_SHAPE, "bn_eval_bwd: C=%d unsupported", C);
  if (!dout || !y || !coef || !dy || M < 1) ECG_FAIL(ECGMM_ERR_SHAPE, "bn_eval_bwd: null operand");
  const bool sums = dgamma || dbeta || dbias;
  if (sums && !scratch) ECG_FAIL(ECGMM_ERR_WORKSPACE, "bn_eval_bwd: parameter gradients need the scratch buffer");
  const int rpi = EB_THREADS / (C / vec);
  long grid = (M + (long)rpi * 8 - 1) / ((long)rpi * 8);
  if (grid > 1024) grid = 1024;
  if (sums) {
    const long cap = (long)(ecg_bn_bwd_scratch(dtype, M, C) / sizeof(float)) / (3L * C);
    if (grid > cap) grid = cap;
  }
  if (grid < 1) grid = 1;
  BnEvalBwdParams p;
  memset(&p, 0, sizeof(p));
  p.dout = dout; p.maskref = maskref; p.gate = gate; p.addc = addc; p.y = y; p.coef = coef; p.dy = dy; p.dz_out = dz_out;
  p.partial = sums ? scratch : nullptr;
  p.M = M; p.C = C; p.rows_per_sample = rows_per_sample > 0 ? rows_per_sample : 1;
  const size_t lds = sums ? (size_t)EB_THREADS * (3 * vec + 1) * sizeof(float) : 0;
  if (dtype == ECGMM_BF16)
    hipLaunchKernelGGL(bn_eval_bwd_kernel<bf16_t>, dim3((unsigned)grid), dim3(EB_THREADS), lds, stream, p);
  else
    hipLaunchKernelGGL(bn_eval_bwd_kernel<float>, dim3((unsigned)grid), dim3(EB_THREADS), lds, stream, p);
  ECG_CHECK_LAUNCH("bn_eval_bwd");
  if (sums) {
    hipLaunchKernelGGL(bn_eval_bwd_finalize_kernel, dim3(ceil_div(3 * C, 256)), dim3(256), 0, stream,
                       (const float*)scratch, (int)grid, C, dgamma, dbeta, dbias);
    ECG_CHECK_LAUNCH("bn_eval_bwd_finalize");
  }
  return 0;
}
