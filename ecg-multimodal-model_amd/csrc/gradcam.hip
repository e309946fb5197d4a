// Grad-CAM map of an encoder's last activation (gfx950).  After a global average pool the gradient of any logit w.r.t. the
// last activation map A [N][R = H' x W'][C] is constant over space, d logit / d A[n][r][c] = dpooled[n][c] / R, so the
// channel weights are known from the head's backward alone:
//     cam[n][r] = relu( sum_c (dpooled[n][c] / R) * A[n][r][c] ),   cam[n] /= max_r cam[n][r]  (all zero if the maximum is 0)
// followed by a bilinear upsample to the input size with align_corners=False semantics (F.interpolate).
#include "ops.h"

namespace {

// one wave per position: lanes stride the channels
template <typename T>
__global__ __launch_bounds__(256) void cam_weighted_sum_kernel(const T* __restrict__ act, const float* __restrict__ dpooled,
                                                               float* __restrict__ cam, long NR, int R, int C, float scale) {
  const long pos = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pos >= NR) return;
  const int lane = threadIdx.x & 63;
  const long n = pos / R;
  const T* a = act + pos * C;
  const float* wt = dpooled + n * C;
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += wt[c] * Elem<T>::ld(a + c);
  s = wave_sum(s) * scale;
  if (lane == 0) cam[pos] = fmaxf(s, 0.f);
}

// one workgroup per sample: maximum over the R positions, then divide
__global__ __launch_bounds__(256) void cam_normalise_kernel(float* __restrict__ cam, int R) {
  __shared__ float sh[4];
  float* c = cam + (size_t)blockIdx.x * R;
  float m = 0.f;
  for (int r = threadIdx.x; r < R; r += 256) m = fmaxf(m, c[r]);
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
  __syncthreads();
  m = fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
  const float inv = m > 0.f ? 1.f / m : 0.f;
  for (int r = threadIdx.x; r < R; r += 256) c[r] = m > 0.f ? c[r] * inv : 0.f;
}

__device__ __forceinline__ void bilinear_src(int dst, float scale, int in, int& i0, int& i1, float& lam) {
  float src = ((float)dst + 0.5f) * scale - 0.5f;
  src = src < 0.f ? 0.f : src;
  i0 = (int)src;
  if (i0 > in - 1) i0 = in - 1;
  i1 = i0 + 1 < in ? i0 + 1 : in - 1;
  lam = src - (float)i0;
}

__global__ __launch_bounds__(256) void cam_upsample_kernel(const float* __restrict__ cam, float* __restrict__ out, int N,
                                                           int Hs, int Ws, int H, int W) {
  const long total = (long)N * H * W;
  const float sh = (float)Hs / (float)H, sw = (float)Ws / (float)W;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int w = (int)(i % W), h = (int)((i / W) % H);
    const long n = i / ((long)W * H);
    int h0, h1, w0, w1;
    float lh, lw;
    bilinear_src(h, sh, Hs, h0, h1, lh);
    bilinear_src(w, sw, Ws, w0, w1, lw);
    const float* c = cam + n * Hs * Ws;
    const float top = c[h0 * Ws + w0] * (1.f - lw) + c[h0 * Ws + w1] * lw;
    const float bot = c[h1 * Ws + w0] * (1.f - lw) + c[h1 * Ws + w1] * lw;
    out[i] = top * (1.f - lh) + bot * lh;
  }
}

}  // namespace

// act [N][Hs*Ws][C] (compute dtype), dpooled [N][C], small [N][Hs*Ws] scratch, out [N][H][W]
int ecg_gradcam(int dtype, const void* act, const float* dpooled, float* small, float* out, int N, int Hs, int Ws, int C,
                int H, int W, hipStream_t stream) {
  if (!act || !dpooled || !small || !out) ECG_FAIL(ECGMM_ERR_SHAPE, "gradcam: null operand");
  if (N < 1 || Hs < 1 || Ws < 1 || C < 1 || H < 1 || W < 1) ECG_FAIL(ECGMM_ERR_SHAPE, "gradcam: bad shape");
  const int R = Hs * Ws;
  const long NR = (long)N * R;
  const float scale = 1.f / (float)R;
  if (dtype == ECGMM_BF16)
    hipLaunchKernelGGL(cam_weighted_sum_kernel<bf16_t>, dim3(ceil_div(NR, 4)), dim3(256), 0, stream, (const bf16_t*)act,
                       dpooled, small, NR, R, C, scale);
  else if (dtype == ECGMM_F32)
    hipLaunchKernelGGL(cam_weighted_sum_kernel<float>, dim3(ceil_div(NR, 4)), dim3(256), 0, stream, (const float*)act,
                       dpooled, small, NR, R, C, scale);
  else
    ECG_FAIL(ECGMM_ERR_DTYPE, "gradcam: bad dtype %d", dtype);
  ECG_CHECK_LAUNCH("gradcam_sum");
  hipLaunchKernelGGL(cam_normalise_kernel, dim3(N), dim3(256), 0, stream, small, R);
  ECG_CHECK_LAUNCH("gradcam_normalise");
  long blocks = ((long)N * H * W + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(cam_upsample_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, (const float*)small, out, N, Hs, Ws,
                     H, W);
  ECG_CHECK_LAUNCH("gradcam_upsample");
  return 0;
}
