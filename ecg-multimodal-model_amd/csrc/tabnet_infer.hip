// The eval forward of pytorch_tabnet's TabNetNoEmbeddings (ecgmm/tabnet.py; reference multimodal.py:109-148, :170-240) as an
// inference plan: ONE fold launch (ecgmm_tabnet_infer_prepare) and ONE forward launch (ecgmm_tabnet_infer), exact fp32 on
// v_mfma_f32_16x16x4_f32.
//
// Why one kernel.  In eval mode every (Ghost-)BatchNorm is a per-channel affine of its running statistics and every row of the
// batch is independent of the others, so the network is a chain of small dense layers per row.  The layout is that of
// transformer_infer.hip: a wave owns 16 rows, a workgroup is four such waves that share nothing (no LDS, no barrier), every
// product is computed TRANSPOSED (weight tile = A operand, activation tile = B operand), so lane l = (c = l & 15, g = l >> 4)
// holds, of data row c, the features 16 t + 4 g + reg of every 16-feature tile t:
//   * a GLU layer's 2 W outputs (W = n_d + n_a) are 2 W / 16 tiles; the value tile t and its gate tile t + W / 16 are two
//     accumulators of the same lane and register, so a * sigmoid(b) is register work and the result IS the next layer's B
//     operand (the contraction index of an MFMA is a free permutation; every weight load is a float4 of one row);
//   * the sqrt(0.5) residual, the split at n_d (a tile boundary), ReLU, the prior, the masks and M_explain are register work;
//   * a row's D features sit in the four lanes {c, c + 16, c + 32, c + 48}: the sparsemax is Michelot's fixed point
//     tau = (sum_support - 1) / |support| (no sort), one sum over the own registers and two cross-lane exchanges per round.
//     The loop leaves when no row of the wave changed; a round on a converged row reproduces its tau bit for bit, so a row's
//     bits do not depend on its tile-mates.  Padded features (>= D) are never in the support, a sum or a count.
// Folding (prepare): s_j = gamma_j / sqrt(rv_j + eps), W'[j, k] = s_j W[j, k], b'_j = beta_j - rm_j s_j for the BatchNorm behind
// every bias-free fc.  A SHARED fc is used by n_steps + 1 FeatTransformers, each with its own BatchNorm: it gets n_steps + 1
// folded copies.  initial_bn stays a (scale, shift) pair: the masks multiply the NORMALISED input.
// A row's bits depend on that row and the blob alone: not on B, not on the row's place in a tile; no atomics.
#include "ops.h"
#include "plan_common.h"

namespace {

constexpr int TN_WAVES = 4;                 // waves per workgroup
constexpr int TN_ROWS = 16 * TN_WAVES;      // rows per workgroup
constexpr int TN_MAX_STEPS = 8;
constexpr int TN_MAX_LAYERS = 8;            // n_shared + n_independent
constexpr int TN_MAX_D = 64, TN_MAX_W = 128, TN_MAX_OUT = 128;
constexpr int TN_MAX_PTRS = 4 + (TN_MAX_STEPS + 1) * TN_MAX_LAYERS * 5 + TN_MAX_STEPS * 5 + 1;

// the blob, in floats; every piece starts at a multiple of 64 floats (256 bytes):
//   bn0 scale[64] shift[64] | per FeatTransformer f, per layer l: W' [2W, K_l] b' [pad64(2W)] (K_0 = Dp, else W) |
//   per step: attentive W' [Dp, n_a] b' [64] | final_mapping [out_dim, n_d]
struct TnLayout {
  int D, Dp, nd, na, W, steps, layers, out_dim;
  int sz0, szN, ft_stride, att_sz;
  size_t off_ft, off_att, off_final, total;
};
__host__ __device__ inline int pad64(int n) { return (n + 63) / 64 * 64; }

TnLayout make_layout(const ecgmm_tabnet_infer_desc& d) {
  TnLayout q;
  q.D = d.input_dim; q.Dp = (d.input_dim + 15) / 16 * 16;
  q.nd = d.n_d; q.na = d.n_a; q.W = d.n_d + d.n_a; q.steps = d.n_steps; q.layers = d.n_shared + d.n_independent;
  q.out_dim = d.out_dim;
  q.sz0 = 2 * q.W * q.Dp + pad64(2 * q.W);
  q.szN = 2 * q.W * q.W + pad64(2 * q.W);
  q.ft_stride = q.sz0 + (q.layers - 1) * q.szN;
  q.att_sz = q.Dp * q.na + 64;
  q.off_ft = 128;
  q.off_att = q.off_ft + (size_t)(q.steps + 1) * q.ft_stride;
  q.off_final = q.off_att + (size_t)q.steps * q.att_sz;
  q.total = q.off_final + (size_t)q.out_dim * q.nd;
  return q;
}

int check_desc(const ecgmm_tabnet_infer_desc* d, const char* who) {
  if (!d) ECG_FAIL(ECGMM_ERR_SHAPE, "%s: null descriptor", who);
  if (d->input_dim < 1 || d->input_dim > TN_MAX_D)
    ECG_FAIL(ECGMM_ERR_SHAPE, "%s: input_dim=%d (needs 1 <= input_dim <= 64)", who, d->input_dim);
  if (d->n_d < 16 || d->n_d % 16) ECG_FAIL(ECGMM_ERR_SHAPE, "%s: n_d=%d (needs a multiple of 16, >= 16)", who, d->n_d);
  if (d->n_a < 16 || d->n_a % 16) ECG_FAIL(ECGMM_ERR_SHAPE, "%s: n_a=%d (needs a multiple of 16, >= 16)", who, d->n_a);
  if (d->n_d + d->n_a > TN_MAX_W)
    ECG_FAIL(ECGMM_ERR_SHAPE, "%s: n_d + n_a = %d (needs n_d + n_a <= 128)", who, d->n_d + d->n_a);
  if (d->n_steps < 1 || d->n_steps > TN_MAX_STEPS)
    ECG_FAIL(ECGMM_ERR_SHAPE, "%s: n_steps=%d (needs 1 <= n_steps <= 8)", who, d->n_steps);
  if (d->n_shared < 0 || d->n_independent < 0 || d->n_shared + d->n_independent < 1 ||
      d->n_shared + d->n_independent > TN_MAX_LAYERS)
    ECG_FAIL(ECGMM_ERR_SHAPE, "%s: n_shared=%d, n_independent=%d (needs both >= 0 and 1 <= n_shared + n_independent <= 8)", who,
             d->n_shared, d->n_independent);
  if (d->out_dim < 16 || d->out_dim > TN_MAX_OUT || d->out_dim % 16)
    ECG_FAIL(ECGMM_ERR_SHAPE, "%s: out_dim=%d (needs a multiple of 16 with 16 <= out_dim <= 128)", who, d->out_dim);
  if (!(d->gamma >= 0.f && d->gamma <= 1e6f)) ECG_FAIL(ECGMM_ERR_SHAPE, "%s: gamma %g (needs 0 <= gamma <= 1e6)", who, (double)d->gamma);
  if (!(d->epsilon >= 0.f && d->epsilon <= 1.f))
    ECG_FAIL(ECGMM_ERR_SHAPE, "%s: epsilon %g (needs 0 <= epsilon <= 1)", who, (double)d->epsilon);
  if (!(d->bn_eps >= 0.f && d->bn_eps <= 1.f)) ECG_FAIL(ECGMM_ERR_SHAPE, "%s: bn_eps %g (needs 0 <= bn_eps <= 1)", who, (double)d->bn_eps);
  return 0;
}

// ---- prepare: every piece of the blob, its padding included, in one launch --------------------------------------------------
struct TnPrepArgs {
  TnLayout q;
  float eps;
  const float* p[TN_MAX_PTRS];   // the parameter table (state_dict order, num_batches_tracked left out)
};

__device__ __forceinline__ float bn_scale(const float* gamma, const float* rv, int j, float eps) {
  return gamma[j] / sqrtf(rv[j] + eps);
}

// blockIdx.y = the piece: 0 bn0, 1 final_mapping, 2 .. 2 + nft * layers - 1 the GLU layers, then the attentive transformers
__global__ __launch_bounds__(256) void tabnet_fold_kernel(TnPrepArgs a, float* __restrict__ blob) {
  const TnLayout& q = a.q;
  const int piece = blockIdx.y;
  const int first = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;
  const int nglu = (q.steps + 1) * q.layers;
  if (piece == 0) {
    const float *gm = a.p[0], *be = a.p[1], *rm = a.p[2], *rv = a.p[3];
    for (int i = first; i < 128; i += stride) {
      const int f = i & 63;
      float v = 0.f;
      if (f < q.D) {
        const float s = bn_scale(gm, rv, f, a.eps);
        v = i < 64 ? s : fmaf(-rm[f], s, be[f]);
      }
      blob[i] = v;
    }
  } else if (piece == 1) {
    const float* w = a.p[4 + nglu * 5 + q.steps * 5];
    float* dst = blob + q.off_final;
    for (int i = first; i < q.out_dim * q.nd; i += stride) dst[i] = w[i];
  } else if (piece < 2 + nglu) {
    const int k = piece - 2, f = k / q.layers, l = k - f * q.layers;
    const float* const* p = a.p + 4 + k * 5;
    const float *w = p[0], *gm = p[1], *be = p[2], *rm = p[3], *rv = p[4];
    const int Kp = l == 0 ? q.Dp : q.W, K = l == 0 ? q.D : q.W, rows = 2 * q.W;
    float* dst = blob + q.off_ft + (size_t)f * q.ft_stride + (l == 0 ? 0 : q.sz0 + (l - 1) * q.szN);
    for (int i = first; i < rows * Kp; i += stride) {
      const int j = i / Kp, kk = i - j * Kp;
      dst[i] = kk < K ? bn_scale(gm, rv, j, a.eps) * w[(size_t)j * K + kk] : 0.f;
    }
    dst += rows * Kp;
    for (int j = first; j < pad64(rows); j += stride) dst[j] = j < rows ? fmaf(-rm[j], bn_scale(gm, rv, j, a.eps), be[j]) : 0.f;
  } else {
    const int s = piece - 2 - nglu;
    const float* const* p = a.p + 4 + nglu * 5 + s * 5;
    const float *w = p[0], *gm = p[1], *be = p[2], *rm = p[3], *rv = p[4];
    float* dst = blob + q.off_att + (size_t)s * q.att_sz;
    for (int i = first; i < q.Dp * q.na; i += stride) {
      const int j = i / q.na;
      dst[i] = j < q.D ? bn_scale(gm, rv, j, a.eps) * w[i] : 0.f;
    }
    dst += q.Dp * q.na;
    for (int j = first; j < 64; j += stride) dst[j] = j < q.D ? fmaf(-rm[j], bn_scale(gm, rv, j, a.eps), be[j]) : 0.f;
  }
}

// ---- forward ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ f32x4 tn_mfma4(const float4& a, const f32x4& b, f32x4 c) {
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b[0], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b[1], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b[2], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b[3], c, 0, 0, 0);
  return c;
}
__device__ __forceinline__ float4 tn_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
// the sum over the four lanes that hold one row; every one of them ends with the same bits (float addition commutes)
__device__ __forceinline__ float tn_row4_sum(float v) {
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}
__device__ __forceinline__ float tn_row4_max(float v) {
  v = fmaxf(v, __shfl_xor(v, 16, 64));
  v = fmaxf(v, __shfl_xor(v, 32, 64));
  return v;
}

// out[t] = (in W'^T + b')[value tile t] * sigmoid((in W'^T + b')[gate tile t + nw]); W' [2 * 16 nw, Kp] followed by b'
template <int NW, int NIN>
__device__ __forceinline__ void glu_layer(const f32x4 (&in)[NIN], int nin, const float* __restrict__ Wp, int Kp, int nw, int c,
                                          int g, f32x4 (&out)[NW]) {
  const float* bias = Wp + (size_t)32 * nw * Kp;
#pragma unroll
  for (int t = 0; t < NW; ++t)
    if (t < nw) {
      f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
      const float* wa = Wp + (size_t)(16 * t + c) * Kp + 4 * g;
      const float* wb = wa + (size_t)16 * nw * Kp;
#pragma unroll
      for (int kb = 0; kb < NIN; ++kb)
        if (kb < nin) {
          a = tn_mfma4(tn_ld4(wa + 16 * kb), in[kb], a);
          b = tn_mfma4(tn_ld4(wb + 16 * kb), in[kb], b);
        }
      const float4 ba = tn_ld4(bias + 16 * t + 4 * g), bb = tn_ld4(bias + 16 * (t + nw) + 4 * g);
      out[t][0] = (a[0] + ba.x) * (1.f / (1.f + expf(-(b[0] + bb.x))));
      out[t][1] = (a[1] + ba.y) * (1.f / (1.f + expf(-(b[1] + bb.y))));
      out[t][2] = (a[2] + ba.z) * (1.f / (1.f + expf(-(b[2] + bb.z))));
      out[t][3] = (a[3] + ba.w) * (1.f / (1.f + expf(-(b[3] + bb.w))));
    }
}

struct TnArgs {
  TnLayout q;
  const float* x;
  const float* blob;
  float *out, *mexp, *masks, *ent;
  long B;
  float gamma, epsilon;
};

// NW / ND: compile-time tile capacities (W <= 16 NW, Dp <= 16 ND); the live counts are wave-uniform run-time guards
template <int NW, int ND>
__global__ __launch_bounds__(64 * TN_WAVES) void tabnet_infer_kernel(TnArgs a) {
  const TnLayout& q = a.q;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = lane & 15, g = lane >> 4;
  const long row0 = ((long)blockIdx.x * TN_WAVES + wave) * 16;
  if (row0 >= a.B) return;                       // wave-uniform; the kernel has no barrier
  const long r = row0 + c;
  const bool live = r < a.B;
  const long rl = live ? r : a.B - 1;            // a dead lane recomputes the last row and stores nothing
  const int D = q.D, nw = q.W >> 4, ndt = q.nd >> 4, nx = q.Dp >> 4;
  const float scale = 0.70710678118654752440f;   // sqrt(0.5)

  // x after initial_bn; padded features are 0 (scale = shift = 0 there)
  f32x4 xn[ND], prior[ND], M[ND], mexp[ND], in0[ND];
  unsigned valid = 0;                            // bit 4 t + i: feature 16 t + 4 g + i < D
#pragma unroll
  for (int t = 0; t < ND; ++t) {
    const float4 sc = tn_ld4(a.blob + 16 * t + 4 * g), sh = tn_ld4(a.blob + 64 + 16 * t + 4 * g);
    const float scv[4] = {sc.x, sc.y, sc.z, sc.w}, shv[4] = {sh.x, sh.y, sh.z, sh.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int f = 16 * t + 4 * g + i;
      const bool ok = t < nx && f < D;
      if (ok) valid |= 1u << (4 * t + i);
      const float xv = ok ? a.x[(size_t)rl * D + f] : 0.f;
      xn[t][i] = fmaf(xv, scv[i], shv[i]);
      prior[t][i] = 1.f;
      M[t][i] = 0.f;
      mexp[t][i] = 0.f;
      in0[t][i] = xn[t][i];
    }
  }
  f32x4 h[NW], dsum[NW];
#pragma unroll
  for (int t = 0; t < NW; ++t) dsum[t] = h[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  float ent = 0.f;

  // f = 0: the initial splitter on xn; f = 1 .. steps: the FeatTransformer of step f - 1 on M * xn
#pragma unroll 1
  for (int f = 0; f <= q.steps; ++f) {
    const float* Wp = a.blob + q.off_ft + (size_t)f * q.ft_stride;
    glu_layer<NW, ND>(in0, nx, Wp, q.Dp, nw, c, g, h);            // the first layer of a FeatTransformer has no residual
    Wp += q.sz0;
#pragma unroll 1
    for (int l = 1; l < q.layers; ++l, Wp += q.szN) {
      f32x4 o[NW];
      glu_layer<NW, NW>(h, nw, Wp, q.W, nw, c, g, o);
#pragma unroll
      for (int t = 0; t < NW; ++t)
        if (t < nw) {
#pragma unroll
          for (int i = 0; i < 4; ++i) h[t][i] = (h[t][i] + o[t][i]) * scale;
        }
    }
    if (f > 0) {   // d = relu(h[:, :n_d]); its row sum weighs this step's mask in M_explain
      float imp = 0.f;
#pragma unroll
      for (int t = 0; t < NW; ++t)
        if (t < ndt) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float dv = fmaxf(h[t][i], 0.f);
            dsum[t][i] += dv;
            imp += dv;
          }
        }
      imp = tn_row4_sum(imp);
#pragma unroll
      for (int t = 0; t < ND; ++t) {
#pragma unroll
        for (int i = 0; i < 4; ++i) mexp[t][i] = fmaf(M[t][i], imp, mexp[t][i]);
      }
    }
    if (f == q.steps) break;

    // attentive transformer of step f on att = h[:, n_d:], times the prior, sparsemax
    const float* Ap = a.blob + q.off_att + (size_t)f * q.att_sz;
    const float* ab = Ap + q.Dp * q.na;
    float zmax = -INFINITY;
#pragma unroll
    for (int t = 0; t < ND; ++t) {
      f32x4 z = {0.f, 0.f, 0.f, 0.f};
      if (t < nx) {
        const float* wa = Ap + (size_t)(16 * t + c) * q.na + 4 * g;
#pragma unroll
        for (int kb = 0; kb < NW; ++kb)
          if (kb >= ndt && kb < nw) z = tn_mfma4(tn_ld4(wa + 16 * (kb - ndt)), h[kb], z);
        const float4 bi = tn_ld4(ab + 16 * t + 4 * g);
        z[0] = (z[0] + bi.x) * prior[t][0];
        z[1] = (z[1] + bi.y) * prior[t][1];
        z[2] = (z[2] + bi.z) * prior[t][2];
        z[3] = (z[3] + bi.w) * prior[t][3];
      }
      M[t] = z;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (valid >> (4 * t + i) & 1) zmax = fmaxf(zmax, z[i]);
    }
    zmax = tn_row4_max(zmax);
#pragma unroll
    for (int t = 0; t < ND; ++t) {
#pragma unroll
      for (int i = 0; i < 4; ++i) M[t][i] -= zmax;
    }
    // Michelot: drop what is not above tau of the current support until nothing drops (at most D rounds; tau only grows)
    unsigned sup = valid;
    float tau = 0.f;
    for (int it = 0; it <= TN_MAX_D; ++it) {
      float s = 0.f, n = 0.f;
#pragma unroll
      for (int t = 0; t < ND; ++t) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (sup >> (4 * t + i) & 1) {
            s += M[t][i];
            n += 1.f;
          }
      }
      s = tn_row4_sum(s);
      n = tn_row4_sum(n);
      tau = (s - 1.f) / n;
      unsigned keep = 0;
#pragma unroll
      for (int t = 0; t < ND; ++t) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if ((sup >> (4 * t + i) & 1) && M[t][i] > tau) keep |= 1u << (4 * t + i);
      }
      const bool changed = keep != sup;
      sup = keep;
      if (__ballot(changed) == 0) break;         // wave-uniform
    }
#pragma unroll
    for (int t = 0; t < ND; ++t) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float m = (sup >> (4 * t + i) & 1) ? M[t][i] - tau : 0.f;
        M[t][i] = m;
        ent = fmaf(m, logf(m + a.epsilon), ent);
        prior[t][i] = prior[t][i] * (a.gamma - m);
        in0[t][i] = m * xn[t][i];
        if (a.masks && live && (valid >> (4 * t + i) & 1))
          a.masks[((size_t)f * a.B + r) * D + 16 * t + 4 * g + i] = m;
      }
    }
  }

  // res = sum of the steps' d; out = res final_mapping^T
  const float* Fp = a.blob + q.off_final;
#pragma unroll
  for (int t = 0; t < TN_MAX_OUT / 16; ++t)
    if (16 * t < q.out_dim) {
      f32x4 y = {0.f, 0.f, 0.f, 0.f};
      const float* wa = Fp + (size_t)(16 * t + c) * q.nd + 4 * g;
#pragma unroll
      for (int kb = 0; kb < NW; ++kb)
        if (kb < ndt) y = tn_mfma4(tn_ld4(wa + 16 * kb), dsum[kb], y);
      if (live) {
        float* o = a.out + (size_t)r * q.out_dim + 16 * t + 4 * g;
        o[0] = y[0]; o[1] = y[1]; o[2] = y[2]; o[3] = y[3];
      }
    }
  if (a.mexp && live) {
#pragma unroll
    for (int t = 0; t < ND; ++t) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (valid >> (4 * t + i) & 1) a.mexp[(size_t)r * D + 16 * t + 4 * g + i] = mexp[t][i];
    }
  }
  ent = tn_row4_sum(ent);
  if (a.ent && live && g == 0) a.ent[r] = ent;
}

template <int NW>
void launch_nd(const TnArgs& a, dim3 grid, hipStream_t s) {
  if (a.q.Dp <= 16) hipLaunchKernelGGL((tabnet_infer_kernel<NW, 1>), grid, dim3(64 * TN_WAVES), 0, s, a);
  else hipLaunchKernelGGL((tabnet_infer_kernel<NW, 4>), grid, dim3(64 * TN_WAVES), 0, s, a);
}

int n_params(const ecgmm_tabnet_infer_desc& d) {
  return 4 + (d.n_steps + 1) * (d.n_shared + d.n_independent) * 5 + d.n_steps * 5 + 1;
}

}  // namespace

/* multimodal.py:113-123 (the network the blob describes) */
extern "C" size_t ecgmm_tabnet_infer_prepared_bytes(const ecgmm_tabnet_infer_desc* d) {
  if (check_desc(d, "tabnet infer")) return 0;
  return make_layout(*d).total * sizeof(float);
}

/* multimodal.py:113-123 in eval mode: every BatchNorm folded into the fc in front of it */
extern "C" int ecgmm_tabnet_infer_prepare(const ecgmm_tabnet_infer_desc* d, const void* const* params, void* blob,
                                          size_t blob_bytes, void* stream_) {
  ECG_TRY(check_desc(d, "tabnet infer prepare"));
  if (!params) ECG_FAIL(ECGMM_ERR_SHAPE, "tabnet infer prepare: null parameter table");
  const int np = n_params(*d);
  TnPrepArgs a;
  for (int i = 0; i < np; ++i) {
    if (!params[i]) ECG_FAIL(ECGMM_ERR_SHAPE, "tabnet infer prepare: parameter %d is null", i);
    a.p[i] = (const float*)params[i];
  }
  for (int i = np; i < TN_MAX_PTRS; ++i) a.p[i] = nullptr;
  a.q = make_layout(*d);
  a.eps = d->bn_eps;
  ECG_NEED(blob, blob_bytes, a.q.total * sizeof(float), "tabnet infer prepare: blob");
  if ((uintptr_t)blob & 15) ECG_FAIL(ECGMM_ERR_SHAPE, "tabnet infer prepare: the blob must be 16-byte aligned");
  const int pieces = 2 + (a.q.steps + 1) * a.q.layers + a.q.steps;
  hipLaunchKernelGGL(tabnet_fold_kernel, dim3(16, pieces), dim3(256), 0, (hipStream_t)stream_, a, (float*)blob);
  ECG_CHECK_LAUNCH("tabnet infer prepare");
  return 0;
}

/* multimodal.py:141-148 under model.eval() and torch.no_grad(), and the forward_masks behind :170-240 */
extern "C" int ecgmm_tabnet_infer(const ecgmm_tabnet_infer_desc* d, const float* x, int64_t B, const void* blob,
                                  size_t blob_bytes, float* out, float* m_explain, float* masks, float* row_entropy,
                                  void* stream_) {
  ECG_TRY(check_desc(d, "tabnet infer"));
  if (B < 1 || B > ((int64_t)1 << 31) - TN_ROWS)
    ECG_FAIL(ECGMM_ERR_SHAPE, "tabnet infer: B=%lld rows (needs 1 <= B < 2^31 - 64)", (long long)B);
  if (!x || !out) ECG_FAIL(ECGMM_ERR_SHAPE, "tabnet infer: null input / output");
  TnArgs a;
  a.q = make_layout(*d);
  ECG_NEED(blob, blob_bytes, a.q.total * sizeof(float), "tabnet infer: blob");
  if ((uintptr_t)blob & 15) ECG_FAIL(ECGMM_ERR_SHAPE, "tabnet infer: the blob must be 16-byte aligned");
  a.x = x; a.blob = (const float*)blob; a.out = out; a.mexp = m_explain; a.masks = masks; a.ent = row_entropy;
  a.B = (long)B; a.gamma = d->gamma; a.epsilon = d->epsilon;
  const dim3 grid((unsigned)((B + TN_ROWS - 1) / TN_ROWS));
  hipStream_t s = (hipStream_t)stream_;
  if (a.q.W <= 32) launch_nd<2>(a, grid, s);
  else if (a.q.W <= 64) launch_nd<4>(a, grid, s);
  else launch_nd<8>(a, grid, s);
  ECG_CHECK_LAUNCH("tabnet infer");
  return 0;
}
