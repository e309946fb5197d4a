// SHAP of the fusion head on the device (reference: shap_fusion_modal_balance.py:122-160 shap.GradientExplainer, and
// shap_fusion.py:62 / shap_fusion_paper.py:71 shap.DeepExplainer), for the one network they are applied to:
// Linear(D, H) -> ReLU -> Dropout(eval) -> Linear(H, C).  For sample b and pair k (background row r):
//     z   = W1 p + b1                    p = t x_b + (1 - t) bg_r (expected gradients) / x_b and bg_r themselves (DeepLIFT)
//     s_c = W2[c, :] * gate(z)           gate = 1[z > 0]  /  (relu(zx) - relu(zb)) / (zx - zb), 1[zb > 0] where |zx - zb| < 1e-6
//     G_c = W1^T s_c
//     phi[b, :, c] = mean_k G_c * (x_b - bg_r)
//
//   shap_tile_kernel<MODE, CT>: one workgroup (four waves) per (sample, tile of 64 pairs).
//     phase 1 (MODE_GRAD, MODE_Z): the points of the tile are built in LDS 32 columns of D at a time beside the same columns of
//       W1, and z [64][Hp] accumulates on v_mfma_f32_16x16x4_f32 (exact fp32: an fmaf chain over d = 0 .. D - 1 from 0, then
//       + b1).  Wave w owns the column tiles w, w + 4, .. of H for all four row tiles.  MODE_Z stops here and stores z: it
//       gives zx / zb of the DeepLIFT entry once per ROW, with the very instruction sequence of the per-pair z, so a pair at
//       t = 1 / t = 0 has bit-equal z.  MODE_DEEP has no phase 1: its gates come from the stored zx, zb.
//     phase 2: the gates sit in LDS; per 32 columns of D, G_c [64][32] = (gate * W2[c]) W1 on the same MFMA (wave w owns row
//       tile w, both column tiles, every class: 2 CT independent accumulators), multiplied in fp32 by the re-gathered
//       x_b - bg_r and column-summed in fp64 (four rows per lane, xor-16 / xor-32 butterflies, then the four waves in order).
//       The sums and the sums of squares of the tile go to the workspace: the points, G and the products never touch memory.
//   shap_combine_kernel: tiles added in order, mean and shap's variance (population variance / sqrt(K)) in fp64, stored fp32.
//   The reduction order is a function of k alone: sample b's result depends on its own rows and the shared tensors only.
//   Rows past K, columns past D / H and classes past C are zero-filled in LDS and never addressed; a ridx outside [0, N) is
//   never used as an address and makes its sample's phi / var NaN.
#include "ops.h"

#include <math.h>

namespace {

constexpr int SH_MAX_D = 4096, SH_MAX_H = 256, SH_MAX_C = 8, SH_MAX_K = 4096;
constexpr int SH_TP = 64;   // pairs per tile
constexpr int SH_DC = 32;   // columns of D per chunk
constexpr int SH_CS = 36;   // row stride of the chunk images in LDS: 36 i + g, i < 16, g < 4 covers 64 distinct banks
enum { MODE_GRAD = 0, MODE_DEEP = 1, MODE_Z = 2 };

struct ShapParams {
  const float* x;      // [B][D]
  const float* bg;     // [N][D]
  const int* ridx;     // [B][K] (MODE_GRAD)
  const float* t;      // [B][K] (MODE_GRAD)
  const float* W1;     // [H][D]
  const float* b1;     // [H]
  const float* W2;     // [C][H]
  const float* zx;     // [B][H] (MODE_DEEP)
  const float* zb;     // [N][H] (MODE_DEEP)
  const float* src;    // [rows][D] (MODE_Z)
  float* zout;         // MODE_GRAD: [B][K][H] or null; MODE_Z: [rows][H]
  double* part;        // [B][T][2][C][D]: sums, sums of squares
  int* flag;           // [B][T]: 1 = the tile met a ridx outside [0, N)
  float* phi;          // [B][D][C]
  float* var;          // [B][D][C] or null
  int B, N, K, D, H, C, Hp, T, rows;
};

// CT: the classes the instantiation carries.  69 KB at Hp = 128, CT = 2: two workgroups per CU
static size_t tile_lds_bytes(int Hp, int CT) {
  return (size_t)2 * 4 * 2 * CT * 16 * sizeof(double) +
         ((size_t)SH_TP * (Hp + 4) + (size_t)Hp * SH_CS + (size_t)SH_TP * SH_CS + (size_t)SH_MAX_C * Hp + Hp + 2 * SH_TP) *
             sizeof(float);
}

template <int MODE, int CT>
__global__ __launch_bounds__(256) void shap_tile_kernel(ShapParams p) {
  extern __shared__ double shap_lds[];
  const int D = p.D, H = p.H, Hp = p.Hp, K = p.K, GS = Hp + 4;
  double* red = shap_lds;                            // [2][4 waves][2 column tiles][CT][16]
  float* gate = (float*)(red + 2 * 4 * 2 * CT * 16); // [64][GS]
  float* w1s = gate + SH_TP * GS;                    // [Hp][36]
  float* ps = w1s + Hp * SH_CS;                      // [64][36] points (phase 1)
  float* dfs = ps;                                   // [64][36] x_b - bg_r (phase 2: the points are consumed by then)
  float* w2s = ps + SH_TP * SH_CS;                   // [8][Hp]
  float* b1s = w2s + SH_MAX_C * Hp;                  // [Hp]
  int* rid = (int*)(b1s + Hp);                       // [64]: the background row of a pair, -1 = no such pair
  float* ts = (float*)(rid + SH_TP);                 // [64]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i16 = lane & 15, g4 = lane >> 4;
  const int lc = tid & 31, lr = tid >> 5;
  const int b = MODE == MODE_Z ? 0 : (int)(blockIdx.x / (unsigned)p.T);
  const int tile = MODE == MODE_Z ? (int)blockIdx.x : (int)(blockIdx.x - (unsigned)b * (unsigned)p.T);
  const int k0 = tile * SH_TP;
  const int nrow = MODE == MODE_Z ? p.rows : K;
  const float* xb = MODE == MODE_Z ? nullptr : p.x + (size_t)b * D;

  if (tid < SH_TP) {
    const int k = k0 + tid;
    int r = -1, bad = 0;
    float tv = 0.f;
    if (k < nrow) {
      if (MODE == MODE_GRAD) {
        r = p.ridx[(size_t)b * K + k];
        tv = p.t[(size_t)b * K + k];
        if (r < 0 || r >= p.N) { r = -1; bad = 1; }
      } else {
        r = k;
      }
    }
    rid[tid] = r;
    ts[tid] = tv;
    if (MODE == MODE_GRAD) {
      bad = __any(bad);   // tid < 64: wave 0, whole
      if (tid == 0) p.flag[(size_t)b * p.T + tile] = bad;
    } else if (MODE == MODE_DEEP) {
      if (tid == 0) p.flag[(size_t)b * p.T + tile] = 0;
    }
  }
  for (int e = tid; e < SH_MAX_C * Hp; e += 256) {
    const int c = e / Hp, h = e - c * Hp;
    w2s[e] = (MODE != MODE_Z && c < p.C && h < H) ? p.W2[(size_t)c * H + h] : 0.f;
  }
  for (int h = tid; h < Hp; h += 256) b1s[h] = h < H ? p.b1[h] : 0.f;
  __syncthreads();

  // One chunk (32 columns of D) of W1 and of the tile's background rows travels through registers: it is fetched while the
  // MFMAs of the chunk before it run, and stored to LDS between the two barriers at the top of the next iteration.
  const float* rows = MODE == MODE_Z ? p.src : p.bg;
  float wreg[SH_MAX_H / 8], breg[8], xreg = 0.f;
  bool fok = false;
  auto fetch = [&](int d0) {
    const int d = d0 + lc;
    fok = d < D;
#pragma unroll
    for (int q = 0; q < SH_MAX_H / 8; ++q) {
      const int h = lr + 8 * q;
      if (8 * q < Hp) wreg[q] = (fok && h < H) ? p.W1[(size_t)h * D + d] : 0.f;   // Hp is a multiple of 16: uniform
    }
    xreg = (MODE != MODE_Z && fok) ? xb[d] : 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int r = rid[lr + 8 * q];
      breg[q] = (fok && r >= 0) ? rows[(size_t)r * D + d] : 0.f;
    }
  };
  auto store_w1 = [&]() {
#pragma unroll
    for (int q = 0; q < SH_MAX_H / 8; ++q)
      if (8 * q < Hp) w1s[(lr + 8 * q) * SH_CS + lc] = wreg[q];
  };

  // ---- phase 1: z = W1 p + b1 ------------------------------------------------------------------------------
  if (MODE != MODE_DEEP) {
    f32x4 acc[4][4];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[rt][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    fetch(0);
    for (int d0 = 0; d0 < D; d0 += SH_DC) {
      __syncthreads();
      store_w1();
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int row = lr + 8 * q;
        float pv = breg[q];   // MODE_Z: the row itself; 0 where there is no such row or column
        if (MODE == MODE_GRAD) {
          const float tv = ts[row];
          pv = (fok && rid[row] >= 0) ? __fadd_rn(__fmul_rn(tv, xreg), __fmul_rn(__fsub_rn(1.f, tv), breg[q])) : 0.f;
        }
        ps[row * SH_CS + lc] = pv;
      }
      __syncthreads();
      if (d0 + SH_DC < D) fetch(d0 + SH_DC);
#pragma unroll
      for (int kk = 0; kk < SH_DC; kk += 4) {
        float a[4];
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) a[rt] = ps[(rt * 16 + i16) * SH_CS + kk + g4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int ct = wave + 4 * j;
          if (ct * 16 < Hp) {   // uniform over the wave
            const float bv = w1s[(ct * 16 + i16) * SH_CS + kk + g4];
#pragma unroll
            for (int rt = 0; rt < 4; ++rt) acc[rt][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[rt], bv, acc[rt][j], 0, 0, 0);
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int ct = wave + 4 * j;
      if (ct * 16 < Hp) {
        const int h = ct * 16 + i16;
        const float bias = b1s[h];
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = rt * 16 + g4 * 4 + r, k = k0 + row;
            const float zv = __fadd_rn(acc[rt][j][r], bias);
            if (MODE == MODE_GRAD) gate[row * GS + h] = (rid[row] >= 0 && h < H && zv > 0.f) ? 1.f : 0.f;
            if (p.zout && k < nrow && h < H) p.zout[((size_t)b * nrow + k) * H + h] = zv;
          }
      }
    }
    if (MODE == MODE_Z) return;
  } else {
    const float* zx = p.zx + (size_t)b * H;
    for (int e = tid; e < SH_TP * Hp; e += 256) {
      const int row = e / Hp, h = e - row * Hp, r = rid[row];
      float g = 0.f;
      if (r >= 0 && h < H) {
        const float a = zx[h], c = p.zb[(size_t)r * H + h];
        const float dz = __fsub_rn(a, c);
        g = fabsf(dz) < 1e-6f ? (c > 0.f ? 1.f : 0.f) : __fdiv_rn(__fsub_rn(fmaxf(a, 0.f), fmaxf(c, 0.f)), dz);
      }
      gate[row * GS + h] = g;
    }
  }

  // ---- phase 2: G_c = W1^T (gate * W2[c]), products with x_b - bg_r, fp64 column sums ---------------------------
  double* part = p.part + ((size_t)b * p.T + tile) * 2 * p.C * D;
  fetch(0);
  for (int d0 = 0; d0 < D; d0 += SH_DC) {
    const int d = d0 + lc;
    const bool dok = d < D;
    __syncthreads();
    store_w1();
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int row = lr + 8 * q;
      dfs[row * SH_CS + lc] = (fok && rid[row] >= 0) ? __fsub_rn(xreg, breg[q]) : 0.f;
    }
    __syncthreads();
    if (d0 + SH_DC < D) fetch(d0 + SH_DC);
    f32x4 acc[2][CT];
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int c = 0; c < CT; ++c) acc[ct][c] = f32x4{0.f, 0.f, 0.f, 0.f};
    // four k-steps at a time (Hp is a multiple of 16): their LDS reads are issued ahead of their MFMAs
    for (int k16 = 0; k16 < Hp; k16 += 16) {
      float g[4], v0[4], v1[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int h = k16 + 4 * u + g4;
        g[u] = gate[(wave * 16 + i16) * GS + h];
        v0[u] = w1s[h * SH_CS + i16];
        v1[u] = w1s[h * SH_CS + 16 + i16];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int c = 0; c < CT; ++c) {
          const float a = __fmul_rn(g[u], w2s[c * Hp + k16 + 4 * u + g4]);
          acc[0][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, v0[u], acc[0][c], 0, 0, 0);
          acc[1][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, v1[u], acc[1][c], 0, 0, 0);
        }
    }
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
      float df[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) df[r] = dfs[(wave * 16 + g4 * 4 + r) * SH_CS + ct * 16 + i16];
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        double s = 0.0, q = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const double pr = (double)__fmul_rn(acc[ct][c][r], df[r]);
          s += pr;
          q += pr * pr;
        }
        s += __shfl_xor(s, 16, 64);
        s += __shfl_xor(s, 32, 64);
        q += __shfl_xor(q, 16, 64);
        q += __shfl_xor(q, 32, 64);
        if (g4 == 0) {
          red[(((0 * 4 + wave) * 2 + ct) * CT + c) * 16 + i16] = s;
          red[(((1 * 4 + wave) * 2 + ct) * CT + c) * 16 + i16] = q;
        }
      }
    }
    __syncthreads();
    if (tid < 32 * CT) {
      const int c = tid >> 5, ct = lc >> 4, i = lc & 15;
      if (c < p.C && dok) {
#pragma unroll
        for (int m = 0; m < 2; ++m) {
          double s = red[(((m * 4 + 0) * 2 + ct) * CT + c) * 16 + i];
#pragma unroll
          for (int w = 1; w < 4; ++w) s += red[(((m * 4 + w) * 2 + ct) * CT + c) * 16 + i];
          part[((size_t)m * p.C + c) * D + d] = s;
        }
      }
    }
  }
}

__global__ __launch_bounds__(256) void shap_combine_kernel(ShapParams p) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  const int D = p.D, C = p.C, T = p.T;
  if (e >= (long long)p.B * D * C) return;
  const int b = (int)(e / ((long long)D * C));
  const int rem = (int)(e - (long long)b * D * C), d = rem / C, c = rem - d * C;
  const double* part = p.part + (size_t)b * T * 2 * C * D;
  double s = 0.0, q = 0.0;
  int bad = 0;
  for (int tile = 0; tile < T; ++tile) {
    s += part[((size_t)tile * 2 * C + c) * D + d];
    q += part[((size_t)tile * 2 * C + C + c) * D + d];
    bad |= p.flag[(size_t)b * T + tile];
  }
  const double mean = s / (double)p.K;
  const float nanv = __builtin_nanf("");
  p.phi[e] = bad ? nanv : (float)mean;
  if (p.var) p.var[e] = bad ? nanv : (float)((q / (double)p.K - mean * mean) / sqrt((double)p.K));
}

struct ShapWs {
  size_t zx, zb, part, flag, total;
};

static ShapWs shap_ws(size_t B, size_t K, size_t D, size_t H, size_t C) {
  const size_t T = (K + SH_TP - 1) / SH_TP;
  ShapWs o;
  size_t off = 0;
  o.zx = off;   off = align_up(off + B * H * sizeof(float), 256);
  o.zb = off;   off = align_up(off + K * H * sizeof(float), 256);
  o.part = off; off = align_up(off + B * T * 2 * C * D * sizeof(double), 256);
  o.flag = off; off = align_up(off + B * T * sizeof(int), 256);
  o.total = off;
  return o;
}

static bool shap_shape_ok(int B, int K, int D, int H, int C) {
  return B >= 1 && K >= 1 && K <= SH_MAX_K && D >= 1 && D <= SH_MAX_D && H >= 1 && H <= SH_MAX_H && C >= 1 &&
         C <= SH_MAX_C && (long long)B * ceil_div(K, SH_TP) <= 0x7fffffffLL;
}

template <int MODE>
static int launch_tiles(const ShapParams& p, unsigned grid, hipStream_t st, const char* what) {
#define SHAP_LAUNCH(CTV)                                                                                               \
  do {                                                                                                                 \
    const size_t lds = tile_lds_bytes(p.Hp, CTV);                                                                      \
    (void)hipFuncSetAttribute((const void*)shap_tile_kernel<MODE, CTV>, hipFuncAttributeMaxDynamicSharedMemorySize,    \
                              160 * 1024);                                                                             \
    hipLaunchKernelGGL((shap_tile_kernel<MODE, CTV>), dim3(grid), dim3(256), lds, st, p);                              \
  } while (0)
  if (MODE == MODE_Z || p.C <= 1) SHAP_LAUNCH(1);
  else if (p.C <= 2) SHAP_LAUNCH(2);
  else if (p.C <= 4) SHAP_LAUNCH(4);
  else SHAP_LAUNCH(8);
#undef SHAP_LAUNCH
  ECG_CHECK_LAUNCH(what);
  return 0;
}

static int launch_combine(const ShapParams& p, hipStream_t st) {
  const long long n = (long long)p.B * p.D * p.C;
  hipLaunchKernelGGL(shap_combine_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p);
  ECG_CHECK_LAUNCH("shap combine");
  return 0;
}

}  // namespace

extern "C" size_t ecgmm_shap_mlp_workspace(int B, int K, int D, int H, int C) {
  if (!shap_shape_ok(B, K, D, H, C)) {
    ecg_set_error("shap_mlp_workspace: need B >= 1, 1 <= K <= %d, 1 <= D <= %d, 1 <= H <= %d, 1 <= C <= %d "
                  "(B=%d K=%d D=%d H=%d C=%d)", SH_MAX_K, SH_MAX_D, SH_MAX_H, SH_MAX_C, B, K, D, H, C);
    return 0;
  }
  return shap_ws((size_t)B, (size_t)K, (size_t)D, (size_t)H, (size_t)C).total;
}

extern "C" int ecgmm_shap_gradient(const float* x, const float* bg, const int* ridx, const float* t, const float* W1,
                                   const float* b1, const float* W2, int B, int N, int K, int D, int H, int C, float* phi,
                                   float* var, float* z, void* ws, size_t ws_bytes, void* stream) {
  if (!x || !bg || !ridx || !t || !W1 || !b1 || !W2 || !phi || !ws) ECG_FAIL(ECGMM_ERR_SHAPE, "shap_gradient: null operand");
  if (!shap_shape_ok(B, K, D, H, C) || N < 1)
    ECG_FAIL(ECGMM_ERR_SHAPE,
             "shap_gradient: need B, N >= 1, 1 <= K <= %d, 1 <= D <= %d, 1 <= H <= %d, 1 <= C <= %d "
             "(B=%d N=%d K=%d D=%d H=%d C=%d)", SH_MAX_K, SH_MAX_D, SH_MAX_H, SH_MAX_C, B, N, K, D, H, C);
  const ShapWs o = shap_ws((size_t)B, (size_t)K, (size_t)D, (size_t)H, (size_t)C);
  if (ws_bytes < o.total) ECG_FAIL(ECGMM_ERR_WORKSPACE, "shap_gradient: workspace of %zu bytes, %zu needed", ws_bytes, o.total);
  char* base = (char*)ws;
  ShapParams p;
  memset(&p, 0, sizeof(p));
  p.x = x; p.bg = bg; p.ridx = ridx; p.t = t; p.W1 = W1; p.b1 = b1; p.W2 = W2;
  p.zout = z; p.part = (double*)(base + o.part); p.flag = (int*)(base + o.flag); p.phi = phi; p.var = var;
  p.B = B; p.N = N; p.K = K; p.D = D; p.H = H; p.C = C; p.Hp = (int)align_up((size_t)H, 16); p.T = ceil_div(K, SH_TP);
  hipStream_t st = (hipStream_t)stream;
  ECG_TRY(launch_tiles<MODE_GRAD>(p, (unsigned)((long long)B * p.T), st, "shap_gradient tiles"));
  return launch_combine(p, st);
}

extern "C" int ecgmm_shap_deep(const float* x, const float* bg, const float* W1, const float* b1, const float* W2, int B,
                               int N, int D, int H, int C, float* phi, float* zx, float* zb, void* ws, size_t ws_bytes,
                               void* stream) {
  if (!x || !bg || !W1 || !b1 || !W2 || !phi || !ws) ECG_FAIL(ECGMM_ERR_SHAPE, "shap_deep: null operand");
  if (!shap_shape_ok(B, N, D, H, C))
    ECG_FAIL(ECGMM_ERR_SHAPE,
             "shap_deep: need B >= 1, 1 <= N <= %d, 1 <= D <= %d, 1 <= H <= %d, 1 <= C <= %d (B=%d N=%d D=%d H=%d C=%d)",
             SH_MAX_K, SH_MAX_D, SH_MAX_H, SH_MAX_C, B, N, D, H, C);
  const ShapWs o = shap_ws((size_t)B, (size_t)N, (size_t)D, (size_t)H, (size_t)C);
  if (ws_bytes < o.total) ECG_FAIL(ECGMM_ERR_WORKSPACE, "shap_deep: workspace of %zu bytes, %zu needed", ws_bytes, o.total);
  char* base = (char*)ws;
  hipStream_t st = (hipStream_t)stream;
  ShapParams p;
  memset(&p, 0, sizeof(p));
  p.W1 = W1; p.b1 = b1; p.W2 = W2;
  p.B = B; p.N = N; p.K = N; p.D = D; p.H = H; p.C = C; p.Hp = (int)align_up((size_t)H, 16); p.T = ceil_div(N, SH_TP);
  float* zx_ = zx ? zx : (float*)(base + o.zx);
  float* zb_ = zb ? zb : (float*)(base + o.zb);
  // zx, zb once per row
  ShapParams q = p;
  q.src = x; q.rows = B; q.zout = zx_;
  ECG_TRY(launch_tiles<MODE_Z>(q, (unsigned)ceil_div(B, SH_TP), st, "shap_deep zx"));
  q.src = bg; q.rows = N; q.zout = zb_;
  ECG_TRY(launch_tiles<MODE_Z>(q, (unsigned)ceil_div(N, SH_TP), st, "shap_deep zb"));
  p.x = x; p.bg = bg; p.zx = zx_; p.zb = zb_;
  p.part = (double*)(base + o.part); p.flag = (int*)(base + o.flag); p.phi = phi;
  ECG_TRY(launch_tiles<MODE_DEEP>(p, (unsigned)((long long)B * p.T), st, "shap_deep tiles"));
  return launch_combine(p, st);
}
