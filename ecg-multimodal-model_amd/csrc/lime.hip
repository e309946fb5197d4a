// LIME tabular on the device (reference: lime_fusion_modal_balance.py:118-160, the work inside
// LimeTabularExplainer.explain_instance): the perturbation sampler, the weighted ridge fit and the class-probability column.
//
//   lime_perturb_kernel : one workgroup per (sample b, perturbation n), one thread per feature f (strided).  Per element two
//     53-bit uniforms from ONE Philox4x32-10 block (the generator of head.hip / physionet.hip), counter
//         c0, c1 = the call's 64-bit offset;  c2 = n;  c3 = 0x40000000 | (b0 + b) << 12 | f      (f < 2^12, b0 + b < 2^18)
//     so an element depends on (seed, offset, b0 + b, n, f) alone: neither on B, nor on how the caller chunks the batch, nor
//     on the launch geometry.  c3 is neither 0 (dropout), nor 0x8....... (augmentation noise), nor 0xFFFFFFFD..F (row
//     decisions, weighted_sample).  Words 0, 1 -> u_bin, words 2, 3 -> u_val.  The bin is the first j with
//     cdf[j] > u_bin * cdf[last] (weighted_sample's rule: a bin of zero frequency is never drawn), the value the inverse-CDF
//     truncated normal in fp64 rounded to fp32 and clamped to the table's fp32 [min, max].
//   ridge: (Zc^T W Zc + alpha I) beta = Zc^T W yc with w-weighted centring, per sample:
//     lime_w_kernel        w_n = exp(-d2_n / (2 kw^2)) in fp64, stored fp32 (= sqrt(exp(-d2 / kw^2)))
//     lime_moments_kernel  fp64 column sums s_i = sum_n w_n z_ni, the counts of ones, r_il = sum_n w_n z_ni y_ln, W = sum w,
//                          ybar_l; right-hand side b_il = r_il - s_i ybar_l rounded to fp32
//     lime_gram_kernel     G_ij = sum_n (w_n z_ni) z_nj on v_mfma_f32_16x16x4_f32: Z is 0/1, so every product is exact and
//                          the only error is the fp32 accumulation over N.  Lower-triangle 64 x 64 tiles, ragged N and K
//                          zero-filled in LDS.  The centring is a rank-one correction AFTER the Gram, in fp64:
//                          A_ij = fl32(G_ij - s_i s_j / W + alpha [i == j]).  A column of equal entries (count 0 or N) has
//                          an exactly zero centred column: its row and column of A are alpha e_i and its b_i is 0, which
//                          makes its coefficient exactly 0.  Rows K .. Kp (Kp = K rounded up to 32) are identity.
//     lime_chol_solve_kernel  one workgroup per sample: right-looking blocked Cholesky (block 32) of the lower triangle in
//                          place.  The 32 x 32 diagonal block is factored in the registers of one wave (row per lane,
//                          v_readlane broadcasts), the panel below it is solved a row per thread and kept in LDS, and the
//                          trailing update A_ij -= sum_p L_ip L_jp runs 16 x 16 tiles on the f32 MFMA from that LDS panel.
//                          Then the two triangular solves for all L right-hand sides, which share the factor.
//     lime_fit_stats_kernel   intercept, local_pred and the weighted R^2 in fp64 from the stored fp32 coefficients
//   lime_prob_kernel : one column of the row softmax.
#include "ops.h"

#include <math.h>

namespace {

constexpr int LIME_MAX_BINS = 16;
constexpr int LIME_MAX_D = 4096;         // f takes 12 bits of the Philox counter
constexpr int LIME_MAX_B = 1 << 18;      // b0 + b takes 18 bits
constexpr int LIME_MAX_L = 8;
constexpr int LIME_MAX_K = 1024;         // the panel of the Cholesky stays in one CU's LDS
constexpr int LIME_NB = 32;
constexpr int LIME_DS = 33;              // row stride of the diagonal block in LDS
constexpr int LIME_PS = 36;              // row stride of the panel in LDS: 36 i + g, i < 16, g < 4 covers 64 distinct banks
constexpr int LIME_CHOL_THREADS = 512;
constexpr int LIME_GS = 80;              // row stride of the Gram operand tiles: 80 r + i, r < 4, i < 16 likewise

// Philox4x32-10 exactly as in physionet.hip
__device__ __forceinline__ void philox4(unsigned long long seed, unsigned c0, unsigned c1, unsigned c2, unsigned c3,
                                        unsigned* r) {
  const unsigned M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
  unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const unsigned hi0 = __umulhi(M0, c0), lo0 = M0 * c0;
    const unsigned hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
    const unsigned n0 = hi1 ^ c1 ^ k0, n1 = lo1, n2 = hi0 ^ c3 ^ k1, n3 = lo0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}

// the 53-bit uniform of weighted_sample_kernel: [0, 1)
__device__ __forceinline__ double u53(unsigned a, unsigned b) {
  return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6)) * (1.0 / 9007199254740992.0);
}

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ------------------------------------------------------------------------------------------------
// perturbation
// ------------------------------------------------------------------------------------------------
struct PerturbParams {
  const float* x;        // [B][D]
  const double* qts;     // [D][S]: the first nbins[f] - 1 entries of a row are the feature's distinct quantiles
  const double* cdf;     // [D][S]: inclusive cumulative bin frequencies, the first nbins[f] entries
  const double* stats;   // [4][D][S]: mean, std, min, max of each bin
  const float* lim;      // [2][D][S]: the fp32 clamp limits of each bin
  const int* nbins;      // [D]
  unsigned char* Z;      // [B][N][D]
  float* inverse;        // [B][N][D]
  int* d2;               // [B][N]
  double* u_out;         // [B][N][D][2] or null
  int S, B, b0, N, D;
  unsigned long long seed, offset;
};

__global__ __launch_bounds__(256) void lime_perturb_kernel(PerturbParams p) {
  __shared__ int part[4];
  const int N = p.N, D = p.D, S = p.S;
  const int b = blockIdx.x / N, n = blockIdx.x - b * N;
  const unsigned o_lo = (unsigned)p.offset, o_hi = (unsigned)(p.offset >> 32);
  const size_t DS = (size_t)D * S;
  int zeros = 0;
  for (int f = threadIdx.x; f < D; f += 256) {
    const size_t e = ((size_t)b * N + n) * D + f;
    unsigned r[4];
    philox4(p.seed, o_lo, o_hi, (unsigned)n, 0x40000000u | ((unsigned)(p.b0 + b) << 12) | (unsigned)f, r);
    const double ub = u53(r[0], r[1]), uv = u53(r[2], r[3]);
    if (p.u_out) {
      p.u_out[2 * e] = ub;
      p.u_out[2 * e + 1] = uv;
    }
    int nb = p.nbins[f];
    nb = nb < 1 ? 1 : (nb > S ? S : nb);   // every table index below lies in [0, S)
    const double* qt = p.qts + (size_t)f * S;
    const double* cdf = p.cdf + (size_t)f * S;
    const float xv = p.x[(size_t)b * D + f];
    int xb = 0;   // np.searchsorted(qts, x), left side: the number of quantiles below x
#pragma unroll 1
    for (int j = 0; j + 1 < nb; ++j) xb += (double)xv > qt[j] ? 1 : 0;
    unsigned char z = 1;
    float val = xv;
    if (n > 0) {
      const double t = ub * cdf[nb - 1];
      int jb = -1;
#pragma unroll 1
      for (int j = 0; j < nb; ++j)
        if (jb < 0 && cdf[j] > t) jb = j;
      if (jb < 0) {   // the product rounded up to the total: the last bin of positive frequency
        jb = 0;
#pragma unroll 1
        for (int j = 0; j < nb; ++j)
          if (cdf[j] > (j ? cdf[j - 1] : 0.0)) jb = j;
      }
      z = jb == xb ? 1 : 0;
      const size_t k = (size_t)f * S + jb;
      const double mean = p.stats[k], sd = p.stats[DS + k], lo = p.stats[2 * DS + k], hi = p.stats[3 * DS + k];
      double v = mean;
      if (sd > 1e-11) {   // a bin whose std is the bare offset yields its mean
        double a = (lo - mean) / sd, c = (hi - mean) / sd;
        if (a == c) {
          v = mean + sd * a;
        } else if (a > 0.0) {   // upper tail: draw from the mirrored interval, where Phi keeps its relative accuracy
          const double pa = normcdf(-c), pc = normcdf(-a);
          v = mean - sd * normcdfinv(pc - uv * (pc - pa));
        } else {
          const double pa = normcdf(a), pc = normcdf(c);
          v = mean + sd * normcdfinv(pa + uv * (pc - pa));
        }
      }
      val = fminf(fmaxf((float)v, p.lim[k]), p.lim[DS + k]);
    }
    zeros += z ? 0 : 1;
    p.Z[e] = z;
    p.inverse[e] = val;
  }
  zeros = wave_sum_int(zeros);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = zeros;
  __syncthreads();
  if (threadIdx.x == 0) p.d2[(size_t)b * N + n] = part[0] + part[1] + part[2] + part[3];
}

// ------------------------------------------------------------------------------------------------
// ridge
// ------------------------------------------------------------------------------------------------
struct RidgeWs {
  size_t w, A, rhs, s, flag, scal, total;
};

static RidgeWs ridge_ws(size_t B, size_t N, size_t K) {
  const size_t Kp = align_up(K, LIME_NB);
  RidgeWs o;
  size_t off = 0;
  o.w = off;    off = align_up(off + B * N * sizeof(float), 256);
  o.A = off;    off = align_up(off + B * Kp * Kp * sizeof(float), 256);
  o.rhs = off;  off = align_up(off + B * LIME_MAX_L * Kp * sizeof(float), 256);
  o.s = off;    off = align_up(off + B * Kp * sizeof(double), 256);
  o.flag = off; off = align_up(off + B * Kp * sizeof(int), 256);
  o.scal = off; off = align_up(off + B * (1 + LIME_MAX_L) * sizeof(double), 256);
  o.total = off;
  return o;
}

struct RidgeParams {
  const unsigned char* Z;   // [B][N][D]
  const int* d2;            // [B][N]
  const float* y;           // [B][L][N]
  const int* cols;          // [B][K] or null
  float* w;                 // [B][N]: the caller's or the workspace's
  float* A;                 // [B][Kp][Kp]
  float* rhs;               // [B][LIME_MAX_L][Kp]
  double* s;                // [B][Kp]
  int* flag;                // [B][Kp]: 0 a live column, 1 a column of equal entries (or a refused index), 2 padding
  double* scal;             // [B][1 + LIME_MAX_L]: W, ybar_l
  float* coef;              // [B][L][K]
  float* intercept;         // [B][L]
  float* score;             // [B][L] or null
  float* local_pred;        // [B][L] or null
  int B, N, D, K, Kp, L;
  double inv2kw2, alpha;
};

__global__ __launch_bounds__(256) void lime_w_kernel(RidgeParams p) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)p.B * p.N) return;
  p.w[i] = (float)exp(-(double)p.d2[i] * p.inv2kw2);
}

// the column of Z behind position k of sample b, or -1 (padding, or an index outside [0, D): never addressed)
__device__ __forceinline__ int lime_col(const RidgeParams& p, int b, int k) {
  if (k >= p.K) return -1;
  const int c = p.cols ? p.cols[(size_t)b * p.K + k] : k;
  return c >= 0 && c < p.D ? c : -1;
}

__global__ __launch_bounds__(128) void lime_moments_kernel(RidgeParams p) {
  const int b = blockIdx.y, k = blockIdx.x * 128 + threadIdx.x, N = p.N, L = p.L;
  if (k >= p.Kp) return;
  const int c = lime_col(p, b, k);
  const unsigned char* z = p.Z + (size_t)b * N * p.D + (c >= 0 ? c : 0);
  const float* w = p.w + (size_t)b * N;
  const float* y = p.y + (size_t)b * L * N;
  double s = 0.0, W = 0.0, r[LIME_MAX_L], yw[LIME_MAX_L];
#pragma unroll
  for (int l = 0; l < LIME_MAX_L; ++l) r[l] = yw[l] = 0.0;
  int cnt = 0;
  for (int n = 0; n < N; ++n) {
    const double wn = (double)w[n];
    const bool one = c >= 0 && z[(size_t)n * p.D] != 0;
    W += wn;
    if (one) { s += wn; ++cnt; }
#pragma unroll
    for (int l = 0; l < LIME_MAX_L; ++l)
      if (l < L) {
        const double t = wn * (double)y[(size_t)l * N + n];
        yw[l] += t;
        if (one) r[l] += t;
      }
  }
  const int flag = k >= p.K ? 2 : ((c < 0 || cnt == 0 || cnt == N) ? 1 : 0);
  p.s[(size_t)b * p.Kp + k] = s;
  p.flag[(size_t)b * p.Kp + k] = flag;
#pragma unroll
  for (int l = 0; l < LIME_MAX_L; ++l)
    if (l < L) p.rhs[((size_t)b * LIME_MAX_L + l) * p.Kp + k] = flag ? 0.f : (float)(r[l] - s * (yw[l] / W));
  if (k == 0) {
    double* sc = p.scal + (size_t)b * (1 + LIME_MAX_L);
    sc[0] = W;
#pragma unroll
    for (int l = 0; l < LIME_MAX_L; ++l)
      if (l < L) sc[1 + l] = yw[l] / W;
  }
}

// grid (T (T + 1) / 2, B), T = ceil(Kp / 64): the 64 x 64 tile (bi, bj), bj <= bi, of sample blockIdx.y.  Wave w owns rows
// 16 w .. 16 w + 15 of the tile and all four 16-column tiles (four independent accumulators).
__global__ __launch_bounds__(256) void lime_gram_kernel(RidgeParams p) {
  __shared__ float wz[32 * LIME_GS];
  __shared__ float zc[32 * LIME_GS];
  const int b = blockIdx.y, N = p.N, D = p.D, Kp = p.Kp;
  int bi = (int)((sqrtf(8.f * (float)blockIdx.x + 1.f) - 1.f) * 0.5f);
  while (bi * (bi + 1) / 2 > (int)blockIdx.x) --bi;
  while ((bi + 1) * (bi + 2) / 2 <= (int)blockIdx.x) ++bi;
  const int bj = (int)blockIdx.x - bi * (bi + 1) / 2;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i16 = lane & 15, g4 = lane >> 4;
  const int lc = tid & 63, lr = tid >> 6;
  const int ci = lime_col(p, b, bi * 64 + lc), cj = lime_col(p, b, bj * 64 + lc);
  const unsigned char* Zb = p.Z + (size_t)b * N * D;
  const float* w = p.w + (size_t)b * N;
  f32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int n0 = 0; n0 < N; n0 += 32) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int r = lr + 4 * q, n = n0 + r;
      const bool ok = n < N;
      const float wv = ok ? w[n] : 0.f;
      const bool zi = ok && ci >= 0 && Zb[(size_t)n * D + ci] != 0;
      const bool zj = ok && cj >= 0 && Zb[(size_t)n * D + cj] != 0;
      wz[r * LIME_GS + lc] = zi ? wv : 0.f;
      zc[r * LIME_GS + lc] = zj ? 1.f : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 32; kk += 4) {
      const float a = wz[(kk + g4) * LIME_GS + wave * 16 + i16];
#pragma unroll
      for (int t = 0; t < 4; ++t)
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, zc[(kk + g4) * LIME_GS + t * 16 + i16], acc[t], 0, 0, 0);
    }
    __syncthreads();
  }
  const double* s = p.s + (size_t)b * Kp;
  const int* flag = p.flag + (size_t)b * Kp;
  const double W = p.scal[(size_t)b * (1 + LIME_MAX_L)];
  float* A = p.A + (size_t)b * Kp * Kp;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int gj = bj * 64 + t * 16 + i16;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int gi = bi * 64 + wave * 16 + g4 * 4 + r;
      if (gi >= Kp || gj > gi) continue;   // one triangle
      const int fi = flag[gi], fj = flag[gj];
      float v;
      if (fi || fj) v = gi == gj ? (fi == 2 ? 1.f : (float)p.alpha) : 0.f;
      else v = (float)((double)acc[t][r] - s[gi] * s[gj] / W + (gi == gj ? p.alpha : 0.0));
      A[(size_t)gi * Kp + gj] = v;
    }
  }
}

__device__ __forceinline__ float lane_bcast(float v, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// LDS: diagonal block [32][33], solved block [LIME_MAX_L][32], panel [Kp - 32][36]
static size_t chol_lds_bytes(int Kp) {
  return ((size_t)LIME_NB * LIME_DS + LIME_MAX_L * LIME_NB + (size_t)(Kp - LIME_NB) * LIME_PS) * sizeof(float);
}

__global__ __launch_bounds__(LIME_CHOL_THREADS) void lime_chol_solve_kernel(RidgeParams p) {
  extern __shared__ float lime_lds[];
  float* Dg = lime_lds;
  float* xs = Dg + LIME_NB * LIME_DS;
  float* P = xs + LIME_MAX_L * LIME_NB;
  const int b = blockIdx.x, Kp = p.Kp, L = p.L;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i16 = lane & 15, g4 = lane >> 4;
  float* A = p.A + (size_t)b * Kp * Kp;
  float* rhs = p.rhs + (size_t)b * LIME_MAX_L * Kp;

  for (int kk = 0; kk < Kp; kk += LIME_NB) {
    const int m = Kp - kk - LIME_NB;   // rows below the diagonal block
    if (wave == 0) {
      // row i of the block in lane i (lanes 32 .. 63 mirror lanes 0 .. 31 and store nothing); entries above the diagonal
      // are carried along and never feed one below it
      const int i = lane & 31;
      float* src = A + (size_t)(kk + i) * Kp + kk;
      float row[LIME_NB];
#pragma unroll
      for (int c = 0; c < LIME_NB; ++c) row[c] = c <= i ? src[c] : 0.f;
#pragma unroll
      for (int j = 0; j < LIME_NB; ++j) {
        const float ljj = sqrtf(lane_bcast(row[j], j));
        row[j] = i == j ? ljj : row[j] / ljj;
#pragma unroll
        for (int c = j + 1; c < LIME_NB; ++c) row[c] -= row[j] * lane_bcast(row[j], c);
      }
      if (lane < 32) {
#pragma unroll
        for (int c = 0; c < LIME_NB; ++c) {
          const float v = c <= i ? row[c] : 0.f;
          Dg[i * LIME_DS + c] = v;
          if (c <= i) src[c] = v;
        }
      }
    }
    __syncthreads();
    // panel: L[i][kk .. kk + 31] = A[i][kk .. kk + 31] L_kk^-T, one row per thread
    for (int r = tid; r < m; r += LIME_CHOL_THREADS) {
      float* src = A + (size_t)(kk + LIME_NB + r) * Kp + kk;
      float x[LIME_NB];
#pragma unroll
      for (int c = 0; c < LIME_NB; ++c) x[c] = src[c];
#pragma unroll
      for (int c = 0; c < LIME_NB; ++c) {
        float t = x[c];
#pragma unroll
        for (int q = 0; q < c; ++q) t -= x[q] * Dg[c * LIME_DS + q];
        x[c] = t / Dg[c * LIME_DS + c];
      }
#pragma unroll
      for (int c = 0; c < LIME_NB; ++c) {
        src[c] = x[c];
        P[r * LIME_PS + c] = x[c];
      }
    }
    __syncthreads();
    // trailing update on the lower-triangle 16 x 16 tiles: A[i][j] -= sum_q L[i][q] L[j][q]
    const int T = m / 16, ntile = T * (T + 1) / 2;
    for (int t = wave; t < ntile; t += LIME_CHOL_THREADS / 64) {
      int ti = (int)((sqrtf(8.f * (float)t + 1.f) - 1.f) * 0.5f);
      while (ti * (ti + 1) / 2 > t) --ti;
      while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
      const int tj = t - ti * (ti + 1) / 2;
      f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < LIME_NB / 4; ++s)
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(P[(ti * 16 + i16) * LIME_PS + 4 * s + g4],
                                                   P[(tj * 16 + i16) * LIME_PS + 4 * s + g4], acc, 0, 0, 0);
      float* c = A + (size_t)(kk + LIME_NB + ti * 16 + g4 * 4) * Kp + kk + LIME_NB + tj * 16 + i16;
#pragma unroll
      for (int r = 0; r < 4; ++r) c[(size_t)r * Kp] -= acc[r];
    }
    __syncthreads();
  }

  // L v = b
  for (int kk = 0; kk < Kp; kk += LIME_NB) {
    const int m = Kp - kk - LIME_NB;
    for (int e = tid; e < LIME_NB * LIME_NB; e += LIME_CHOL_THREADS) {
      const int i = e >> 5, c = e & 31;
      Dg[i * LIME_DS + c] = c <= i ? A[(size_t)(kk + i) * Kp + kk + c] : 0.f;
    }
    __syncthreads();
    if (tid < L) {
      float* v = rhs + (size_t)tid * Kp + kk;
      float x[LIME_NB];
#pragma unroll
      for (int c = 0; c < LIME_NB; ++c) x[c] = v[c];
#pragma unroll
      for (int c = 0; c < LIME_NB; ++c) {
        float t = x[c];
#pragma unroll
        for (int q = 0; q < c; ++q) t -= Dg[c * LIME_DS + q] * x[q];
        x[c] = t / Dg[c * LIME_DS + c];
      }
#pragma unroll
      for (int c = 0; c < LIME_NB; ++c) {
        v[c] = x[c];
        xs[tid * LIME_NB + c] = x[c];
      }
    }
    __syncthreads();
    for (int e = tid; e < m * L; e += LIME_CHOL_THREADS) {
      const int l = e / m, i = kk + LIME_NB + (e - l * m);
      const float* lrow = A + (size_t)i * Kp + kk;
      float t = rhs[(size_t)l * Kp + i];
#pragma unroll
      for (int q = 0; q < LIME_NB; ++q) t -= lrow[q] * xs[l * LIME_NB + q];
      rhs[(size_t)l * Kp + i] = t;
    }
    __syncthreads();
  }
  // L^T beta = v
  for (int kk = Kp - LIME_NB; kk >= 0; kk -= LIME_NB) {
    for (int e = tid; e < LIME_NB * LIME_NB; e += LIME_CHOL_THREADS) {
      const int i = e >> 5, c = e & 31;
      Dg[i * LIME_DS + c] = c <= i ? A[(size_t)(kk + i) * Kp + kk + c] : 0.f;
    }
    __syncthreads();
    if (tid < L) {
      float* v = rhs + (size_t)tid * Kp + kk;
      float x[LIME_NB];
#pragma unroll
      for (int c = 0; c < LIME_NB; ++c) x[c] = v[c];
#pragma unroll
      for (int c = LIME_NB - 1; c >= 0; --c) {
        float t = x[c];
#pragma unroll
        for (int q = c + 1; q < LIME_NB; ++q) t -= Dg[q * LIME_DS + c] * x[q];
        x[c] = t / Dg[c * LIME_DS + c];
      }
#pragma unroll
      for (int c = 0; c < LIME_NB; ++c) {
        v[c] = x[c];
        xs[tid * LIME_NB + c] = x[c];
      }
    }
    __syncthreads();
    for (int e = tid; e < kk * L; e += LIME_CHOL_THREADS) {
      const int l = e / kk, i = e - l * kk;
      float t = rhs[(size_t)l * Kp + i];
#pragma unroll
      for (int q = 0; q < LIME_NB; ++q) t -= A[(size_t)(kk + q) * Kp + i] * xs[l * LIME_NB + q];
      rhs[(size_t)l * Kp + i] = t;
    }
    __syncthreads();
  }
  for (int e = tid; e < p.K * L; e += LIME_CHOL_THREADS) {
    const int l = e / p.K, k = e - l * p.K;
    const bool refused = lime_col(p, b, k) < 0;
    p.coef[((size_t)b * L + l) * p.K + k] = refused ? __builtin_nanf("") : rhs[(size_t)l * Kp + k];
  }
}

__device__ __forceinline__ double block_sum_256(double v, double* red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  return red[0];
}

// grid (L, B): intercept = ybar - sum_k (s_k / W) beta_k, local_pred = intercept + sum_k beta_k, and the weighted R^2 of
// pred_n = intercept + sum_k z_nk beta_k, all in fp64 from the stored fp32 coefficients
__global__ __launch_bounds__(256) void lime_fit_stats_kernel(RidgeParams p) {
  __shared__ double red[256];
  __shared__ float beta[LIME_MAX_K];
  __shared__ int col[LIME_MAX_K];
  const int l = blockIdx.x, b = blockIdx.y, N = p.N, K = p.K, Kp = p.Kp, L = p.L;
  const double* sc = p.scal + (size_t)b * (1 + LIME_MAX_L);
  const double W = sc[0], ybar = sc[1 + l];
  const double* s = p.s + (size_t)b * Kp;
  const float* bsrc = p.rhs + ((size_t)b * LIME_MAX_L + l) * Kp;
  double dot = 0.0, sum = 0.0;
  for (int k = threadIdx.x; k < K; k += 256) {
    const int c = lime_col(p, b, k);
    const float bk = c >= 0 ? bsrc[k] : 0.f;
    beta[k] = bk;
    col[k] = c;
    dot += s[k] / W * (double)bk;
    sum += (double)bk;
  }
  dot = block_sum_256(dot, red);
  sum = block_sum_256(sum, red);
  const double icpt = ybar - dot;
  if (threadIdx.x == 0) {
    p.intercept[(size_t)b * L + l] = (float)icpt;
    if (p.local_pred) p.local_pred[(size_t)b * L + l] = (float)(icpt + sum);
  }
  if (!p.score) return;   // uniform over the block
  const float* w = p.w + (size_t)b * N;
  const float* y = p.y + ((size_t)b * L + l) * N;
  double res = 0.0, tot = 0.0;
  for (int n = threadIdx.x; n < N; n += 256) {
    const unsigned char* z = p.Z + ((size_t)b * N + n) * p.D;
    double pred = icpt;
    for (int k = 0; k < K; ++k)
      if (col[k] >= 0 && z[col[k]] != 0) pred += (double)beta[k];
    const double wn = (double)w[n], yn = (double)y[n];
    res += wn * (yn - pred) * (yn - pred);
    tot += wn * (yn - ybar) * (yn - ybar);
  }
  res = block_sum_256(res, red);
  tot = block_sum_256(tot, red);
  if (threadIdx.x == 0) p.score[(size_t)b * L + l] = tot > 0.0 ? (float)(1.0 - res / tot) : (res == 0.0 ? 1.f : 0.f);
}

__global__ __launch_bounds__(256) void lime_prob_kernel(const float* logits, long long M, int C, int label, float* out,
                                                        long long out_stride) {
  const long long m = (long long)blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  const float* r = logits + (size_t)m * C;
  float mx = r[0];
  for (int c = 1; c < C; ++c) mx = fmaxf(mx, r[c]);
  float den = 0.f;
  for (int c = 0; c < C; ++c) den += expf(r[c] - mx);
  out[(size_t)m * out_stride] = expf(r[label] - mx) / den;
}

}  // namespace

extern "C" int ecgmm_lime_perturb(const float* x, const double* qts, const double* cdf, const double* stats, const float* lim,
                                  const int* nbins, int S, int B, int b0, int N, int D, uint64_t seed, uint64_t offset,
                                  uint8_t* Z, float* inverse, int* d2, double* u_out, void* stream) {
  if (!x || !qts || !cdf || !stats || !lim || !nbins || !Z || !inverse || !d2)
    ECG_FAIL(ECGMM_ERR_SHAPE, "lime_perturb: null operand");
  if (B < 1 || N < 1 || D < 1 || D > LIME_MAX_D || S < 1 || S > LIME_MAX_BINS || b0 < 0 || (long long)b0 + B > LIME_MAX_B ||
      (long long)B * N > 0x7fffffffLL)
    ECG_FAIL(ECGMM_ERR_SHAPE,
             "lime_perturb: need B, N >= 1, 1 <= D <= %d, 1 <= S <= %d, 0 <= b0, b0 + B <= %d, B * N < 2^31 "
             "(B=%d b0=%d N=%d D=%d S=%d)", LIME_MAX_D, LIME_MAX_BINS, LIME_MAX_B, B, b0, N, D, S);
  PerturbParams p;
  memset(&p, 0, sizeof(p));
  p.x = x; p.qts = qts; p.cdf = cdf; p.stats = stats; p.lim = lim; p.nbins = nbins;
  p.Z = Z; p.inverse = inverse; p.d2 = d2; p.u_out = u_out;
  p.S = S; p.B = B; p.b0 = b0; p.N = N; p.D = D; p.seed = seed; p.offset = offset;
  hipLaunchKernelGGL(lime_perturb_kernel, dim3((unsigned)((long long)B * N)), dim3(256), 0, (hipStream_t)stream, p);
  ECG_CHECK_LAUNCH("lime_perturb");
  return 0;
}

extern "C" size_t ecgmm_lime_ridge_workspace(int B, int N, int D) {
  if (B < 1 || N < 1 || D < 1 || D > LIME_MAX_D || (long long)B * N > 0x7fffffffLL) {
    ecg_set_error("lime_ridge_workspace: need B, N >= 1, 1 <= D <= %d, B * N < 2^31 (B=%d N=%d D=%d)", LIME_MAX_D, B, N, D);
    return 0;
  }
  // the fit keeps K <= min(D, LIME_MAX_K) columns, whatever D is
  return ridge_ws((size_t)B, (size_t)N, (size_t)(D < LIME_MAX_K ? D : LIME_MAX_K)).total;
}

extern "C" int ecgmm_lime_ridge(const uint8_t* Z, const int* d2, const float* y, const int* cols, int B, int N, int D, int K,
                                int L, double kernel_width, double alpha, float* coef, float* intercept, float* w,
                                float* score, float* local_pred, void* ws, size_t ws_bytes, void* stream) {
  if (!Z || !d2 || !y || !coef || !intercept || !ws) ECG_FAIL(ECGMM_ERR_SHAPE, "lime_ridge: null operand");
  if (B < 1 || N < 1 || D < 1 || D > LIME_MAX_D || K < 1 || K > D || K > LIME_MAX_K || (!cols && K != D) || L < 1 ||
      L > LIME_MAX_L || B > 65535 || (long long)B * N > 0x7fffffffLL)
    ECG_FAIL(ECGMM_ERR_SHAPE,
             "lime_ridge: need 1 <= B <= 65535, N >= 1, 1 <= K <= D <= %d, K <= %d, K == D without cols, 1 <= L <= %d "
             "(B=%d N=%d D=%d K=%d L=%d)", LIME_MAX_D, LIME_MAX_K, LIME_MAX_L, B, N, D, K, L);
  if (!(kernel_width > 0.0) || !(alpha > 0.0))
    ECG_FAIL(ECGMM_ERR_SHAPE, "lime_ridge: kernel_width and alpha must be positive (%g, %g)", kernel_width, alpha);
  const RidgeWs o = ridge_ws((size_t)B, (size_t)N, (size_t)K);
  if (ws_bytes < o.total)
    ECG_FAIL(ECGMM_ERR_WORKSPACE, "lime_ridge: workspace of %zu bytes, %zu needed", ws_bytes, o.total);
  hipStream_t st = (hipStream_t)stream;
  char* base = (char*)ws;
  RidgeParams p;
  memset(&p, 0, sizeof(p));
  p.Z = Z; p.d2 = d2; p.y = y; p.cols = cols;
  p.w = w ? w : (float*)(base + o.w);
  p.A = (float*)(base + o.A); p.rhs = (float*)(base + o.rhs); p.s = (double*)(base + o.s);
  p.flag = (int*)(base + o.flag); p.scal = (double*)(base + o.scal);
  p.coef = coef; p.intercept = intercept; p.score = score; p.local_pred = local_pred;
  p.B = B; p.N = N; p.D = D; p.K = K; p.Kp = (int)align_up((size_t)K, LIME_NB); p.L = L;
  p.inv2kw2 = 0.5 / (kernel_width * kernel_width); p.alpha = alpha;
  const size_t lds = chol_lds_bytes(p.Kp);
  (void)hipFuncSetAttribute((const void*)lime_chol_solve_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  hipLaunchKernelGGL(lime_w_kernel, dim3((unsigned)(((long long)B * N + 255) / 256)), dim3(256), 0, st, p);
  ECG_CHECK_LAUNCH("lime_ridge weights");
  hipLaunchKernelGGL(lime_moments_kernel, dim3((unsigned)ceil_div(p.Kp, 128), (unsigned)B), dim3(128), 0, st, p);
  ECG_CHECK_LAUNCH("lime_ridge moments");
  const int T = ceil_div(p.Kp, 64);
  hipLaunchKernelGGL(lime_gram_kernel, dim3((unsigned)(T * (T + 1) / 2), (unsigned)B), dim3(256), 0, st, p);
  ECG_CHECK_LAUNCH("lime_ridge gram");
  hipLaunchKernelGGL(lime_chol_solve_kernel, dim3((unsigned)B), dim3(LIME_CHOL_THREADS), lds, st, p);
  ECG_CHECK_LAUNCH("lime_ridge cholesky");
  hipLaunchKernelGGL(lime_fit_stats_kernel, dim3((unsigned)L, (unsigned)B), dim3(256), 0, st, p);
  ECG_CHECK_LAUNCH("lime_ridge statistics");
  return 0;
}

extern "C" int ecgmm_lime_prob(const float* logits, int64_t M, int C, int label, float* out, int64_t out_stride, void* stream) {
  if (!logits || !out) ECG_FAIL(ECGMM_ERR_SHAPE, "lime_prob: null operand");
  if (M < 1 || M > 0x7fffffffLL * 256 || C < 1 || label < 0 || label >= C || out_stride < 1)
    ECG_FAIL(ECGMM_ERR_SHAPE, "lime_prob: need M >= 1, C >= 1, 0 <= label < C, out_stride >= 1 (M=%lld C=%d label=%d stride=%lld)",
             (long long)M, C, label, (long long)out_stride);
  hipLaunchKernelGGL(lime_prob_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, (hipStream_t)stream, logits,
                     (long long)M, C, label, out, (long long)out_stride);
  ECG_CHECK_LAUNCH("lime_prob");
  return 0;
}
