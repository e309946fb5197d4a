// Grad-CAM map of an encoder's last activation (gfx950).  After a global average pool the gradient of any logit w.r.t. the
// last activation map A [N][R = H' x W'][C] is constant over space, d logit / d A[n][r][c] = dpooled[n][c] / R, so the
// channel weights are known from the head's backward alone:
//     cam[n][r] = relu( sum_c (dpooled[n][c] / R) * A[n][r][c] ),   cam[n] /= max_r cam[n][r]  (all zero if the maximum is 0)
// followed by a bilinear upsample to the input size with align_corners=False semantics (F.interpolate).
// The spectrogram CRNN has no pool in front of its head: ecg_crnn_gradcam takes the gradient itself, means it per channel
// and forms the weighted sum in the front end's sequence layout; normalisation and upsample are the kernels above.
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

// one workgroup per sample: maximum over the R positions, then divide.  EXACT: a true division, so that the maximum itself
// becomes exactly 1 (m * (1 / m) may round to 1 - 2^-24); the encoders' maps keep the reciprocal they have always used.
template <bool EXACT> __global__ __launch_bounds__(256) void cam_normalise_kernel(float* __restrict__ cam, int R) {
  __shared__ float sh[4];
  float* c = cam + (size_t)blockIdx.x * R;
  float m = 0.f;
  for (int r = threadIdx.x; r < R; r += 256) m = fmaxf(m, c[r]);
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
  __syncthreads();
  m = fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
  const float inv = m > 0.f ? 1.f / m : 0.f;
  for (int r = threadIdx.x; r < R; r += 256) c[r] = m > 0.f ? (EXACT ? c[r] / m : c[r] * inv) : 0.f;
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

// ---- the CRNN: no pool in front of the head, the gradient varies over space and is read ----
// a[b][c] = mean over (t, f) of dseq[b][t][c * Fp + f]; one wave per (b, c), lanes stride the live (t, f) pairs
__global__ __launch_bounds__(256) void crnn_cam_weights_kernel(const float* __restrict__ dseq, const int* __restrict__ steps,
                                                               float* __restrict__ a, long BC, int Tp, int C, int Fp,
                                                               float scale) {
  const long bc = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (bc >= BC) return;
  const int lane = threadIdx.x & 63, c = (int)(bc % C);
  const long b = bc / C;
  const int live = steps ? min(max(steps[b], 0), Tp) : Tp;   // (clamped: a bad length must not read past the record)
  const float* g = dseq + b * Tp * (long)C * Fp + (long)c * Fp;
  float s = 0.f;
  for (int i = lane; i < live * Fp; i += 64) s += g[(long)(i / Fp) * C * Fp + i % Fp];
  s = wave_sum(s) * scale;
  if (lane == 0) a[bc] = s;
}

// m[b][f][t] = relu(sum_c a[b][c] * seq[b][t][c * Fp + f]) for live t, 0 behind; one wave per (b, f, t), lanes stride c
__global__ __launch_bounds__(256) void crnn_cam_map_kernel(const float* __restrict__ seq, const float* __restrict__ a,
                                                           const int* __restrict__ steps, float* __restrict__ m, long total,
                                                           int Tp, int C, int Fp) {
  const long pos = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pos >= total) return;
  const int lane = threadIdx.x & 63, t = (int)(pos % Tp), f = (int)((pos / Tp) % Fp);
  const long b = pos / ((long)Tp * Fp);
  if (steps && t >= steps[b]) {   // (wave-uniform)
    if (lane == 0) m[pos] = 0.f;
    return;
  }
  const float* x = seq + (b * Tp + t) * (long)C * Fp + f;
  const float* wt = a + b * C;
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += wt[c] * x[(long)c * Fp];
  s = wave_sum(s);
  if (lane == 0) m[pos] = fmaxf(s, 0.f);
}

// columns t >= frames[b] of cam [B][F][T] := 0
__global__ __launch_bounds__(256) void crnn_cam_mask_kernel(float* __restrict__ cam, const int* __restrict__ frames, long total,
                                                            int F, int T) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256)
    if ((int)(i % T) >= frames[i / ((long)F * T)]) cam[i] = 0.f;
}

}  // namespace

size_t ecg_crnn_gradcam_workspace(int B, int Tp, int Fp, int C) {
  if (B < 1 || Tp < 1 || Fp < 1 || C < 1) {
    ecg_set_error("crnn_gradcam_workspace: bad shape B=%d Tp=%d Fp=%d C=%d", B, Tp, Fp, C);
    return 0;
  }
  return align_up(((size_t)B * C + (size_t)B * Fp * Tp) * sizeof(float), 256);
}

int ecg_crnn_gradcam(const float* seq, const float* dseq, const int* steps, const int* frames, void* ws, size_t ws_bytes,
                     float* cam, int B, int Tp, int C, int Fp, int F, int T, hipStream_t stream) {
  if (!seq || !dseq || !cam) ECG_FAIL(ECGMM_ERR_SHAPE, "crnn_gradcam: null operand");
  if (B < 1 || Tp < 1 || C < 1 || Fp < 1 || F < 1 || T < 1)
    ECG_FAIL(ECGMM_ERR_SHAPE, "crnn_gradcam: bad shape B=%d Tp=%d C=%d Fp=%d F=%d T=%d", B, Tp, C, Fp, F, T);
  if ((long)Tp * Fp > 0x7fffffffL || (long)C * Fp > 0x7fffffffL) ECG_FAIL(ECGMM_ERR_SHAPE, "crnn_gradcam: map too large");
  const size_t need = ecg_crnn_gradcam_workspace(B, Tp, Fp, C);
  if (!ws || ws_bytes < need) ECG_FAIL(ECGMM_ERR_WORKSPACE, "crnn_gradcam: workspace %zu bytes, need %zu", ws_bytes, need);
  float* a = (float*)ws;
  float* m = a + (size_t)B * C;
  const long BC = (long)B * C, R = (long)Fp * Tp, total = (long)B * R;
  hipLaunchKernelGGL(crnn_cam_weights_kernel, dim3(ceil_div(BC, 4)), dim3(256), 0, stream, dseq, steps, a, BC, Tp, C, Fp,
                     1.f / (float)R);
  ECG_CHECK_LAUNCH("crnn_gradcam_weights");
  hipLaunchKernelGGL(crnn_cam_map_kernel, dim3(ceil_div(total, 4)), dim3(256), 0, stream, seq, (const float*)a, steps, m, total,
                     Tp, C, Fp);
  ECG_CHECK_LAUNCH("crnn_gradcam_map");
  hipLaunchKernelGGL(cam_normalise_kernel<true>, dim3(B), dim3(256), 0, stream, m, (int)R);
  ECG_CHECK_LAUNCH("crnn_gradcam_normalise");
  const long out = (long)B * F * T;
  const unsigned blocks = (out + 255) / 256 > 4096 ? 4096u : (unsigned)((out + 255) / 256);
  hipLaunchKernelGGL(cam_upsample_kernel, dim3(blocks), dim3(256), 0, stream, (const float*)m, cam, B, Fp, Tp, F, T);
  ECG_CHECK_LAUNCH("crnn_gradcam_upsample");
  if (frames) {
    hipLaunchKernelGGL(crnn_cam_mask_kernel, dim3(blocks), dim3(256), 0, stream, cam, frames, out, F, T);
    ECG_CHECK_LAUNCH("crnn_gradcam_mask");
  }
  return 0;
}

// act [N][Hs*Ws][C] (compute dtype), dpooled [N][C], small [N][Hs*Ws] scratch, out [N][H][W]
int ecg_gradcam(int dtype, const void* act, const float* dpooled, float* small, float* out, int N, int Hs, int Ws, int C,
                int H, int W, hipStream_t stream) {
  if (!act || !dpooled || !small || !out) ECG_FAIL(ECGMM_ERR_SHAPE, "gradcam: null operand");
  if (N < 1 || Hs < 1 || Ws < 1 || C < 1 || H < 1 || W < 1)
    ECG_FAIL(ECGMM_ERR_SHAPE, "gradcam: bad shape N=%d Hs=%d Ws=%d C=%d H=%d W=%d", N, Hs, Ws, C, H, W);
  // (the kernels index the coarse map and one output plane with int)
  if ((long)Hs * Ws > 0x7fffffffL || (long)H * W > 0x7fffffffL) ECG_FAIL(ECGMM_ERR_SHAPE, "gradcam: map too large");
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
  hipLaunchKernelGGL(cam_normalise_kernel<false>, dim3(N), dim3(256), 0, stream, small, R);
  ECG_CHECK_LAUNCH("gradcam_normalise");
  long blocks = ((long)N * H * W + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(cam_upsample_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, (const float*)small, out, N, Hs, Ws,
                     H, W);
  ECG_CHECK_LAUNCH("gradcam_upsample");
  return 0;
}
