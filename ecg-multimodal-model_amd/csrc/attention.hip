// Multi-head self-attention of nn.TransformerEncoderLayer (reference: train_physionet.py:219-220, 236;
// multimodal_paper_modal_balance.py:127-194), forward and backward, fp32 on v_mfma_f32_16x16x4_f32, and the model's front
// (train_physionet.py:216-217, 233-235): Conv1d(input_dim, d_model, 3, padding=1) + bias + positional embedding.
//
// Operands.  qkv [rows][3E] is the packed projection as linear(x, in_proj_weight, in_proj_bias) leaves it, E = heads * d;
// row(s, n) = s * N + n (batch_first = 0) or n * S + s (batch_first = 1).  Everything is addressed by stride: no transposed
// or head-split copy exists.  out / dout [rows][E] with the heads concatenated, lse [N][heads][S], dqkv [rows][3E].
//
// Tile structure.  One WAVE is one unit of work and owns a 16-row tile; a workgroup is four independent waves (no LDS, no
// barrier).  All three kernels keep the scores TRANSPOSED with respect to the rows the wave owns, so that the MFMA result
// registers are at once the operand of the next MFMA and nothing is transposed in LDS or by lane shuffles:
//   forward / dQ (the wave owns 16 queries, loops over 16-key tiles):
//     acc[r] = S[key 4 g + r][query i] = sum_c K[key][c] Q[query][c]     A = K rows, B = Q rows   (i = lane & 15, g = lane >> 4)
//     a lane holds four keys of ONE query: the row statistics (max, sum, lse, D) are one register per lane, the reduction
//     over a score row is 3 in-lane operations + v_permlane16_swap + v_permlane32_swap (rows 0..3 of the wave).
//     O^T[c][query] += V[key 4 g + r][c] * P[key 4 g + r][query]: MFMA step r takes acc[r] as its B operand as it stands --
//     the contraction index of an MFMA is a free permutation, here "k-slot g of step r is key 4 g + r".
//   dK / dV (the wave owns 16 keys, loops over 16-query tiles): the same with the roles exchanged,
//     acc[r] = S[query 4 g + r][key i], dV^T[c][key] += dO[query][c] Pd[query][key], dK^T[c][key] += Q[query][c] dS[query][key].
//   The contraction over the head dimension uses the permutation "k-slot g of step s is column g * d/4 + s", so a lane loads
//   its d/4 columns of a row as one or two float4.
// Online softmax over the key tiles in the forward; the backward recomputes P = exp(scale * S - lse) from the stored lse and
// D[query] = dO . O (mha_rowdot_kernel, the only workspace: one float per (n, head, query)).  No S x S tensor exists.
// Every reduction runs in a fixed order and every output is written by exactly one lane: no atomics, identical bits per call.
//
// S <= 8 (the reference as written attends across its batch of 8): floor(16 / S) (n, head) pairs share one wave.  Slot i of
// the 16 query (key) slots is pair i / S, position i % S; a score between slots of different pairs is masked like a key past
// the end.  Each pair's probabilities, outputs and gradients are the same arithmetic as alone in a tile.
//
// Lengths (VL, the _varlen entry points): lengths[n] (device int32, clamped to [0, S] here) live positions per attention-batch
// element, the same in every head; key_padding_mask[n][s] = s >= lengths[n] plus exact zeros in the padding.  A slot at or
// past the length is empty: it is clamped onto position lengths[n] - 1 (so nothing is ever loaded from a padded row of qkv
// or dout, which may hold NaN) and masked like a key past the end.  The tile loops run ceil(lengths[n] / 16) tiles.  A unit
// whose own tile lies wholly in the padding loads nothing and stores its zeros: out, lse, dQ of a padded query and dK, dV
// of a padded key are exact zeros, D of a padded query is 0.  A live row sees the arithmetic and the tile order of the
// same row alone with S = lengths[n].  VL is a template parameter beside PK: the instantiations without lengths carry none
// of this.  Packed form: every slot reads its own pair's length; a pair of length 0 has no live row to clamp onto, so
// its loads are replaced by zeros (Slot::ld).
//
// Dropout on the probabilities: Philox4x32-10 (the generator of head.hip / lime.hip), one block per four consecutive keys,
//   counter = (offset low, offset high, n * heads + head, 0xC0000000 | query * ceil(S / 4) + key / 4), word key % 4,
//   keep iff (word >> 8) * 2^-24 >= p: a function of (seed, offset, n, head, query, key) alone.  c3 is none of 0 (dropout),
//   0x4....... (LIME), 0x8....... (augmentation noise), 0xFFFFFFFD..F (row decisions).  Needs S <= 32768.  With lengths the
//   stride stays ceil(S / 4) of the padded S: the decision does not depend on the lengths.
#include "ops.h"

#include <math.h>

namespace {

struct MhaGeo {
  int S, N, heads, E, P, tiles, G, SB;   // P = N * heads pairs, tiles = ceil(S / 16), G pairs per wave (0: one tile of one pair)
  long long rs, rn;                      // row(s, n) = s * rs + n * rn
  float scale, p_drop, inv_keep;
  unsigned long long seed, offset;
};

// One of the 16 row slots of a tile.  `row`, `h` and `si` always address a real row (an empty slot is clamped onto the last
// position / pair), so loads need no guard: what an empty slot reads is finite and is multiplied by a probability or a
// score gradient that the mask has set to zero, or belongs to a row that is never stored.
struct Slot {
  int pair, s, h;      // pair = n * heads + h
  long long row, si;   // row(s, n); pair * S + s (lse, D)
  bool ok;
  // lengths only: `ok` is "live" (s < lengths[n]); `real` is a position of the padded tensor, live or padding, and wrow /
  // wsi are its own row(s, n) / pair * S + s, where its zeros are stored; `ld` is false when the pair has no live row at all
  bool real, ld;
  long long wrow, wsi;
};

__device__ __forceinline__ int mha_len(const MhaGeo& g, const int* __restrict__ lens, int n) {
  const int v = lens[n];
  return v < 0 ? 0 : (v > g.S ? g.S : v);
}

// the (n, head) of a pair: two integer divisions, kept out of the tile loops (Unit below)
__device__ __forceinline__ void mha_split(const MhaGeo& g, int pair, int& n, int& h) {
  n = pair / g.heads;
  h = pair - n * g.heads;
}

// what a wave owns: one 16-row tile of one pair (n, h), or -- packed, g.G != 0 -- the pairs u * G .. u * G + G - 1
struct Unit {
  int u, tile, n, h;
  int len;   // lengths, one pair per unit: the live positions of n (wave-uniform)
};

// PK: the packed form (g.G != 0), a template parameter so that the tile loops of the long sequences carry none of its code
template <bool PK, bool VL>
__device__ __forceinline__ Unit mha_unit(const MhaGeo& g, long long unit, const int* __restrict__ lens) {
  Unit o;
  o.len = g.S;
  if (PK) { o.u = (int)unit; o.tile = 0; o.n = o.h = 0; }
  else {
    o.u = (int)(unit / g.tiles);
    o.tile = (int)(unit - (long long)o.u * g.tiles);
    mha_split(g, o.u, o.n, o.h);
    if (VL) o.len = __builtin_amdgcn_readfirstlane(mha_len(g, lens, o.n));
  }
  return o;
}

// slot idx (0..15) of tile `tile` of the unit
template <bool PK, bool VL>
__device__ __forceinline__ Slot mha_slot(const MhaGeo& g, const Unit& w, int tile, int idx, const int* __restrict__ lens) {
  Slot o;
  int n, pc, sc;
  o.ld = true;
  if (PK) {
    const int k = idx / g.S;
    o.pair = w.u * g.G + k;
    o.s = idx - k * g.S;
    o.ok = o.real = k < g.G && o.pair < g.P;
    pc = o.pair < g.P ? o.pair : g.P - 1;
    sc = o.s;
    mha_split(g, pc, n, o.h);
    if (VL) {
      const int len = mha_len(g, lens, n);
      o.ok = o.real && o.s < len;
      o.ld = len > 0;
      sc = o.s < len ? o.s : (len > 0 ? len - 1 : 0);
    }
  } else {
    o.pair = pc = w.u;
    o.s = tile * 16 + idx;
    o.ok = o.s < (VL ? w.len : g.S);
    o.real = o.s < g.S;
    sc = o.ok ? o.s : (VL ? w.len : g.S) - 1;
    n = w.n;
    o.h = w.h;
  }
  o.row = (long long)sc * g.rs + (long long)n * g.rn;
  o.si = (long long)pc * g.S + sc;
  if (VL) {
    const int sw = o.real ? o.s : 0;
    o.wrow = (long long)sw * g.rs + (long long)n * g.rn;
    o.wsi = (long long)pc * g.S + sw;
  } else {
    o.wrow = o.row;
    o.wsi = o.si;
  }
  return o;
}

// the tiles a unit loops over: all of them, or those that hold a live position of its pair
template <bool PK, bool VL>
__device__ __forceinline__ int mha_loop_tiles(const MhaGeo& g, const Unit& w) {
  return PK ? 1 : (VL ? (w.len + 15) >> 4 : g.tiles);
}

// lengths: true when none of the unit's own 16 slots (`own` = the lane's slot lane & 15) is live, so that it only stores zeros
template <bool PK, bool VL>
__device__ __forceinline__ bool mha_idle(const Unit& w, const Slot& own) {
  if (!VL) return false;
  return PK ? !__any(own.ok) : w.tile * 16 >= w.len;
}

// Philox4x32-10 exactly as in lime.hip
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

__device__ __forceinline__ void mha_block(const MhaGeo& g, int pair, int i, int jb, unsigned* r) {
  philox4(g.seed, (unsigned)g.offset, (unsigned)(g.offset >> 32), (unsigned)pair,
          0xC0000000u | (unsigned)(i * g.SB + jb), r);
}

__device__ __forceinline__ bool mha_keep_word(const MhaGeo& g, unsigned w) {
  return (float)(w >> 8) * (1.f / 16777216.f) >= g.p_drop;
}

__device__ __forceinline__ bool mha_keep(const MhaGeo& g, int pair, int i, int j) {
  unsigned r[4];
  mha_block(g, pair, i, j >> 2, r);
  return mha_keep_word(g, r[j & 3]);
}

// all-reduce over the four 16-lane rows of the wave (lanes i, i + 16, i + 32, i + 48); both lanes of an exchange evaluate
// the same commutative operation on the same two values, so every lane ends with the same bits
__device__ __forceinline__ float rows_max(float v) {
  const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  const float w = fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
  const auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(w), __float_as_uint(w), false, false);
  return fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1]));
}

__device__ __forceinline__ float rows_sum(float v) {
  const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  const float w = __uint_as_float(a[0]) + __uint_as_float(a[1]);
  const auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(w), __float_as_uint(w), false, false);
  return __uint_as_float(b[0]) + __uint_as_float(b[1]);
}

// the lane's HD / 4 columns of a row
template <int CW>
__device__ __forceinline__ void load_cols(const float* p, float* v) {
#pragma unroll
  for (int q = 0; q < CW / 4; ++q) {
    const float4 t = *reinterpret_cast<const float4*>(p + 4 * q);
    v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
  }
}

// GD (the packed form with lengths): a slot whose pair has no live row reads zeros instead
template <int CW, bool GD>
__device__ __forceinline__ void load_cols(const float* p, float* v, bool ld) {
  if (!GD || ld) load_cols<CW>(p, v);
  else {
#pragma unroll
    for (int q = 0; q < CW; ++q) v[q] = 0.f;
  }
}

template <bool GD>
__device__ __forceinline__ float load_one(const float* p, bool ld) {
  return !GD || ld ? *p : 0.f;
}

// ------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------
template <int HD, bool PK, bool VL>
__global__ __launch_bounds__(256) void mha_fwd_kernel(MhaGeo g, const float* __restrict__ qkv, float* __restrict__ out,
                                                      float* __restrict__ lse, long long units,
                                                      const int* __restrict__ lens) {
  constexpr int CW = HD / 4, NT = HD / 16;
  constexpr bool GD = PK && VL;
  const long long unit = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (unit >= units) return;   // wave-uniform; the kernel has no barrier
  const int lane = threadIdx.x & 63, i16 = lane & 15, g4 = lane >> 4;
  const Unit u = mha_unit<PK, VL>(g, unit, lens);
  const int qtile = u.tile;
  const int E3 = 3 * g.E;
  const Slot q = mha_slot<PK, VL>(g, u, qtile, i16, lens);
  const int hq = q.h;
  if (mha_idle<PK, VL>(u, q)) {   // wave-uniform: every query of the tile is padding
    if (!q.real) return;
    float* dst = out + q.wrow * g.E + hq * HD + g4 * 4;
#pragma unroll
    for (int t = 0; t < NT; ++t) *reinterpret_cast<float4*>(dst + t * 16) = make_float4(0.f, 0.f, 0.f, 0.f);
    if (g4 == 0) lse[q.wsi] = 0.f;
    return;
  }
  float qv[CW];
  load_cols<CW, GD>(qkv + q.row * E3 + hq * HD + g4 * CW, qv, q.ld);
  f32x4 o[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) o[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;
  const int ktiles = mha_loop_tiles<PK, VL>(g, u);
  for (int kt = 0; kt < ktiles; ++kt) {
    const Slot ka = mha_slot<PK, VL>(g, u, kt, i16, lens);
    float kv[CW];
    load_cols<CW, GD>(qkv + ka.row * E3 + g.E + ka.h * HD + g4 * CW, kv, ka.ld);
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < CW; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(kv[s], qv[s], acc, 0, 0, 0);
    Slot kr[4];
    float sc[4];
    float mt = -INFINITY;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      kr[r] = mha_slot<PK, VL>(g, u, kt, g4 * 4 + r, lens);
      const bool valid = kr[r].ok && q.ok && (!PK || kr[r].pair == q.pair);
      sc[r] = valid ? acc[r] * g.scale : -INFINITY;
      mt = fmaxf(mt, sc[r]);
    }
    mt = rows_max(mt);
    const float mn = fmaxf(m, mt), ms = mn == -INFINITY ? 0.f : mn;
    const float alpha = expf(m - ms);
    float p[4], ls = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      p[r] = expf(sc[r] - ms);
      ls += p[r];
    }
    ls = rows_sum(ls);
    l = l * alpha + ls;
    m = mn;
    if (g.p_drop > 0.f) {
      int prev = -1;
      unsigned w[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int jb = kr[r].s >> 2;
        if (jb != prev || r == 0) { mha_block(g, q.pair, q.s, jb, w); prev = jb; }
        p[r] = mha_keep_word(g, w[kr[r].s & 3]) ? p[r] * g.inv_keep : 0.f;
      }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      o[t] *= alpha;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float v = load_one<GD>(qkv + kr[r].row * E3 + 2 * g.E + kr[r].h * HD + t * 16 + i16, kr[r].ld);
        o[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(v, p[r], o[t], 0, 0, 0);
      }
    }
  }
  if (!q.real) return;
  if (VL && !q.ok) {   // a padded query beside live ones: l = 0 here
    m = 0.f;
    l = 1.f;
#pragma unroll
    for (int t = 0; t < NT; ++t) o[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  float* dst = out + q.wrow * g.E + hq * HD + g4 * 4;
#pragma unroll
  for (int t = 0; t < NT; ++t)
    *reinterpret_cast<float4*>(dst + t * 16) = make_float4(o[t][0] / l, o[t][1] / l, o[t][2] / l, o[t][3] / l);
  if (g4 == 0) lse[q.wsi] = m + logf(l);
}

// ------------------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------------------
// D[pair][s] = dout[row] . out[row] over the head's columns, one thread per (pair, s), a fixed serial order
template <int HD, bool VL>
__global__ __launch_bounds__(256) void mha_rowdot_kernel(MhaGeo g, const float* __restrict__ out,
                                                         const float* __restrict__ dout, float* __restrict__ D,
                                                         const int* __restrict__ lens) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)g.P * g.S) return;
  const int pair = (int)(e / g.S), s = (int)(e - (long long)pair * g.S);
  int n, h;
  mha_split(g, pair, n, h);
  if (VL && s >= mha_len(g, lens, n)) {   // a padded query: dout there is never read
    D[e] = 0.f;
    return;
  }
  const long long off = ((long long)s * g.rs + (long long)n * g.rn) * g.E + h * HD;
  float acc = 0.f;
#pragma unroll
  for (int c = 0; c < HD; c += 4) {
    const float4 a = *reinterpret_cast<const float4*>(dout + off + c), b = *reinterpret_cast<const float4*>(out + off + c);
    acc += a.x * b.x;
    acc += a.y * b.y;
    acc += a.z * b.z;
    acc += a.w * b.w;
  }
  D[e] = acc;
}

// the wave owns 16 keys: dK and dV
template <int HD, bool PK, bool VL>
__global__ __launch_bounds__(256) void mha_bwd_kv_kernel(MhaGeo g, const float* __restrict__ qkv,
                                                         const float* __restrict__ lse, const float* __restrict__ D,
                                                         const float* __restrict__ dout, float* __restrict__ dqkv,
                                                         long long units, const int* __restrict__ lens) {
  constexpr int CW = HD / 4, NT = HD / 16;
  constexpr bool GD = PK && VL;
  const long long unit = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (unit >= units) return;
  const int lane = threadIdx.x & 63, i16 = lane & 15, g4 = lane >> 4;
  const Unit u = mha_unit<PK, VL>(g, unit, lens);
  const int ktile = u.tile;
  const int E3 = 3 * g.E;
  const Slot k = mha_slot<PK, VL>(g, u, ktile, i16, lens);
  const int hk = k.h;
  if (mha_idle<PK, VL>(u, k)) {   // wave-uniform: every key of the tile is padding
    if (!k.real) return;
    float* dst = dqkv + k.wrow * E3 + hk * HD + g4 * 4;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      *reinterpret_cast<float4*>(dst + g.E + t * 16) = make_float4(0.f, 0.f, 0.f, 0.f);
      *reinterpret_cast<float4*>(dst + 2 * g.E + t * 16) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    return;
  }
  float kv[CW], vv[CW];
  load_cols<CW, GD>(qkv + k.row * E3 + g.E + hk * HD + g4 * CW, kv, k.ld);
  load_cols<CW, GD>(qkv + k.row * E3 + 2 * g.E + hk * HD + g4 * CW, vv, k.ld);
  f32x4 dk[NT], dv[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) dk[t] = dv[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int qtiles = mha_loop_tiles<PK, VL>(g, u);
  for (int qt = 0; qt < qtiles; ++qt) {
    const Slot qa = mha_slot<PK, VL>(g, u, qt, i16, lens);
    const int ha = qa.h;
    float qv[CW], dov[CW];
    load_cols<CW, GD>(qkv + qa.row * E3 + ha * HD + g4 * CW, qv, qa.ld);
    load_cols<CW, GD>(dout + qa.row * g.E + ha * HD + g4 * CW, dov, qa.ld);
    f32x4 as = f32x4{0.f, 0.f, 0.f, 0.f}, ap = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < CW; ++s) {
      as = __builtin_amdgcn_mfma_f32_16x16x4f32(qv[s], kv[s], as, 0, 0, 0);
      ap = __builtin_amdgcn_mfma_f32_16x16x4f32(dov[s], vv[s], ap, 0, 0, 0);
    }
    Slot qr[4];
    float pd[4], ds[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      qr[r] = mha_slot<PK, VL>(g, u, qt, g4 * 4 + r, lens);
      const bool valid = qr[r].ok && k.ok && (!PK || qr[r].pair == k.pair);
      const float lr = lse[qr[r].si], dr = D[qr[r].si];
      const float p = valid ? expf(as[r] * g.scale - lr) : 0.f;
      float dp = ap[r];
      pd[r] = p;
      if (g.p_drop > 0.f) {
        const bool keep = valid && mha_keep(g, k.pair, qr[r].s, k.s);
        pd[r] = keep ? p * g.inv_keep : 0.f;
        dp = keep ? dp * g.inv_keep : 0.f;
      }
      ds[r] = valid ? p * (dp - dr) : 0.f;
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long long row = qr[r].row;
        const int col = qr[r].h * HD + t * 16 + i16;
        const float a_do = load_one<GD>(dout + row * g.E + col, qr[r].ld);
        const float a_q = load_one<GD>(qkv + row * E3 + col, qr[r].ld);
        dv[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_do, pd[r], dv[t], 0, 0, 0);
        dk[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_q, ds[r], dk[t], 0, 0, 0);
      }
    }
  }
  if (!k.real) return;
  if (VL && !k.ok) {   // a padded key beside live ones
#pragma unroll
    for (int t = 0; t < NT; ++t) dk[t] = dv[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  float* dst = dqkv + k.wrow * E3 + hk * HD + g4 * 4;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    *reinterpret_cast<float4*>(dst + g.E + t * 16) =
        make_float4(dk[t][0] * g.scale, dk[t][1] * g.scale, dk[t][2] * g.scale, dk[t][3] * g.scale);
    *reinterpret_cast<float4*>(dst + 2 * g.E + t * 16) = make_float4(dv[t][0], dv[t][1], dv[t][2], dv[t][3]);
  }
}

// the wave owns 16 queries: dQ
template <int HD, bool PK, bool VL>
__global__ __launch_bounds__(256) void mha_bwd_q_kernel(MhaGeo g, const float* __restrict__ qkv,
                                                        const float* __restrict__ lse, const float* __restrict__ D,
                                                        const float* __restrict__ dout, float* __restrict__ dqkv,
                                                        long long units, const int* __restrict__ lens) {
  constexpr int CW = HD / 4, NT = HD / 16;
  constexpr bool GD = PK && VL;
  const long long unit = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (unit >= units) return;
  const int lane = threadIdx.x & 63, i16 = lane & 15, g4 = lane >> 4;
  const Unit u = mha_unit<PK, VL>(g, unit, lens);
  const int qtile = u.tile;
  const int E3 = 3 * g.E;
  const Slot q = mha_slot<PK, VL>(g, u, qtile, i16, lens);
  const int hq = q.h;
  if (mha_idle<PK, VL>(u, q)) {   // wave-uniform: every query of the tile is padding
    if (!q.real) return;
    float* dst = dqkv + q.wrow * E3 + hq * HD + g4 * 4;
#pragma unroll
    for (int t = 0; t < NT; ++t) *reinterpret_cast<float4*>(dst + t * 16) = make_float4(0.f, 0.f, 0.f, 0.f);
    return;
  }
  float qv[CW], dov[CW];
  load_cols<CW, GD>(qkv + q.row * E3 + hq * HD + g4 * CW, qv, q.ld);
  load_cols<CW, GD>(dout + q.row * g.E + hq * HD + g4 * CW, dov, q.ld);
  const float lq = lse[q.si], dq_row = D[q.si];
  f32x4 dq[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) dq[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int ktiles = mha_loop_tiles<PK, VL>(g, u);
  for (int kt = 0; kt < ktiles; ++kt) {
    const Slot ka = mha_slot<PK, VL>(g, u, kt, i16, lens);
    const int ha = ka.h;
    float kv[CW], vv[CW];
    load_cols<CW, GD>(qkv + ka.row * E3 + g.E + ha * HD + g4 * CW, kv, ka.ld);
    load_cols<CW, GD>(qkv + ka.row * E3 + 2 * g.E + ha * HD + g4 * CW, vv, ka.ld);
    f32x4 as = f32x4{0.f, 0.f, 0.f, 0.f}, ap = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < CW; ++s) {
      as = __builtin_amdgcn_mfma_f32_16x16x4f32(kv[s], qv[s], as, 0, 0, 0);
      ap = __builtin_amdgcn_mfma_f32_16x16x4f32(vv[s], dov[s], ap, 0, 0, 0);
    }
    Slot kr[4];
    float ds[4];
    int prev = -1;
    unsigned w[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      kr[r] = mha_slot<PK, VL>(g, u, kt, g4 * 4 + r, lens);
      const bool valid = kr[r].ok && q.ok && (!PK || kr[r].pair == q.pair);
      const float p = valid ? expf(as[r] * g.scale - lq) : 0.f;
      float dp = ap[r];
      if (g.p_drop > 0.f) {
        const int jb = kr[r].s >> 2;
        if (jb != prev || r == 0) { mha_block(g, q.pair, q.s, jb, w); prev = jb; }
        dp = mha_keep_word(g, w[kr[r].s & 3]) ? dp * g.inv_keep : 0.f;
      }
      ds[r] = valid ? p * (dp - dq_row) : 0.f;
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float a_k = load_one<GD>(qkv + kr[r].row * E3 + g.E + kr[r].h * HD + t * 16 + i16, kr[r].ld);
        dq[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_k, ds[r], dq[t], 0, 0, 0);
      }
    }
  }
  if (!q.real) return;
  if (VL && !q.ok) {   // a padded query beside live ones
#pragma unroll
    for (int t = 0; t < NT; ++t) dq[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  float* dst = dqkv + q.wrow * E3 + hq * HD + g4 * 4;
#pragma unroll
  for (int t = 0; t < NT; ++t)
    *reinterpret_cast<float4*>(dst + t * 16) =
        make_float4(dq[t][0] * g.scale, dq[t][1] * g.scale, dq[t][2] * g.scale, dq[t][3] * g.scale);
}

// mask [N][heads][S][S] bytes: one thread per (pair, query, block of four keys)
__global__ __launch_bounds__(256) void mha_keep_mask_kernel(MhaGeo g, unsigned char* __restrict__ mask) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long per = (long long)g.S * g.SB;
  if (e >= (long long)g.P * per) return;
  const int pair = (int)(e / per);
  const long long rem = e - (long long)pair * per;
  const int i = (int)(rem / g.SB), jb = (int)(rem - (long long)i * g.SB);
  unsigned r[4];
  mha_block(g, pair, i, jb, r);
  unsigned char* dst = mask + ((long long)pair * g.S + i) * g.S;
#pragma unroll
  for (int w = 0; w < 4; ++w)
    if (4 * jb + w < g.S) dst[4 * jb + w] = mha_keep_word(g, r[w]) ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------
// attention maps and the attention-rollout step (ecgmm_mha_weights / ecgmm_mha_rollout_step)
// ------------------------------------------------------------------------------------------------
// Both rebuild p[n,h,i,j] = expf(scale q_i . k_j - lse[n,h,i]) from qkv and the lse the forward stored, the expression of
// the backward kernels, BEFORE dropout (p_drop is ignored: torch's maps in training mode are the dropped ones; in eval mode
// and at dropout 0 there is no difference).  One wave owns one 16-row tile of ONE attention-batch element n and loops over
// the heads inside, so the head average needs no second pass.  Never packed: at S <= 8 a wave holds the one partial tile
// of one n (these are not training kernels; the slots of the other 16 - S rows are empty).  With lengths, live queries
// hold the softmax over the live keys and everything in the padding is an exact 0 -- torch's padded QUERY rows still attend
// to the live keys; here they are zero, as the padded rows of ecgmm_mha_forward_varlen are.
template <bool VL>
__device__ __forceinline__ Unit map_unit(const MhaGeo& g, long long unit, const int* __restrict__ lens) {
  Unit o;
  o.n = (int)(unit / g.tiles);
  o.tile = (int)(unit - (long long)o.n * g.tiles);
  o.h = 0;
  o.u = o.n * g.heads;   // the pair of head 0: head h is at si + h * S
  o.len = VL ? __builtin_amdgcn_readfirstlane(mha_len(g, lens, o.n)) : g.S;
  return o;
}

// four consecutive keys j0 .. j0 + 3 of one row of a map: one 16-byte store where S % 4 == 0 (then all four lie on one
// side of S), else element by element
__device__ __forceinline__ void map_store4(float* __restrict__ row, int j0, int S, bool vec, float a, float b, float c,
                                           float d) {
  if (vec) {
    if (j0 < S) *reinterpret_cast<float4*>(row + j0) = make_float4(a, b, c, d);
  } else {
    if (j0 < S) row[j0] = a;
    if (j0 + 1 < S) row[j0 + 1] = b;
    if (j0 + 2 < S) row[j0 + 2] = c;
    if (j0 + 3 < S) row[j0 + 3] = d;
  }
}

// the wave owns 16 queries of n: w [N][heads][S][S] (PH) or the head average [N][S][S], sum over h = 0, 1, .. then one
// multiplication by inv_heads.  The transposed score layout of the forward: a lane holds four consecutive keys of one query.
template <int HD, bool VL, bool PH>
__global__ __launch_bounds__(256) void mha_weights_kernel(MhaGeo g, const float* __restrict__ qkv,
                                                          const float* __restrict__ lse, float* __restrict__ w,
                                                          long long units, const int* __restrict__ lens, float inv_heads,
                                                          int vec) {
  constexpr int CW = HD / 4, HB = 4;
  const long long unit = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (unit >= units) return;   // wave-uniform; the kernel has no barrier
  const int lane = threadIdx.x & 63, i16 = lane & 15, g4 = lane >> 4;
  const Unit u = map_unit<VL>(g, unit, lens);
  const int E3 = 3 * g.E;
  const Slot q = mha_slot<false, VL>(g, u, u.tile, i16, lens);
  const long long SS = (long long)g.S * g.S;
  // the query's row of head 0 (PH) or of the average
  float* dst = w + (long long)u.n * (PH ? g.heads : 1) * SS + (long long)(q.real ? q.s : 0) * g.S;
  const int nmaps = PH ? g.heads : 1;
  if (mha_idle<false, VL>(u, q)) {   // wave-uniform: every query of the tile is padding
    if (!q.real) return;
    for (int h = 0; h < nmaps; ++h)
      for (int kt = 0; kt < g.tiles; ++kt) map_store4(dst + h * SS, kt * 16 + g4 * 4, g.S, vec, 0.f, 0.f, 0.f, 0.f);
    return;
  }
  const int ktiles = mha_loop_tiles<false, VL>(g, u);
  for (int kt = 0; kt < ktiles; ++kt) {
    const Slot ka = mha_slot<false, VL>(g, u, kt, i16, lens);
    const int j0 = kt * 16 + g4 * 4;
    float sum[4] = {0.f, 0.f, 0.f, 0.f};
    for (int h0 = 0; h0 < g.heads; h0 += HB) {
      // the loads of HB heads are issued together (N * ceil(S / 16) waves: little else hides their latency); a head past
      // the last one is clamped onto it, adds exact zeros to the sum and stores nothing
      float qv[HB][CW], kv[HB][CW], lq[HB];
#pragma unroll
      for (int b = 0; b < HB; ++b) {
        const int h = min(h0 + b, g.heads - 1);
        load_cols<CW>(qkv + q.row * E3 + h * HD + g4 * CW, qv[b]);
        load_cols<CW>(qkv + ka.row * E3 + g.E + h * HD + g4 * CW, kv[b]);
        lq[b] = lse[q.si + (long long)h * g.S];
      }
#pragma unroll
      for (int b = 0; b < HB; ++b) {
        const int h = h0 + b;
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < CW; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(kv[b][s], qv[b][s], acc, 0, 0, 0);
        float p[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool valid = q.ok && j0 + r < u.len && h < g.heads;
          p[r] = valid ? expf(acc[r] * g.scale - lq[b]) : 0.f;
          sum[r] += p[r];
        }
        if (PH && q.real && h < g.heads) map_store4(dst + h * SS, j0, g.S, vec, p[0], p[1], p[2], p[3]);
      }
    }
    if (!PH && q.real)
      map_store4(dst, j0, g.S, vec, sum[0] * inv_heads, sum[1] * inv_heads, sum[2] * inv_heads, sum[3] * inv_heads);
  }
  if (VL && q.real) {   // the key tiles wholly behind the length
    for (int h = 0; h < nmaps; ++h)
      for (int kt = ktiles; kt < g.tiles; ++kt) map_store4(dst + h * SS, kt * 16 + g4 * 4, g.S, vec, 0.f, 0.f, 0.f, 0.f);
  }
}

// the wave owns 16 keys of n:  y[n][j] = a v[n][j] + (1 - a) inv_heads sum_h sum_i v[n][i] p[n,h,i,j], v and y [N][S].
// The score layout of mha_bwd_kv_kernel: acc[r] = S[query 4 g + r][key i16].  A lane's partial sum runs over the heads,
// the query tiles inside and its four queries inside those, by fmaf; then one all-reduce over the four lane rows.  With
// lengths a padded v is never read and a padded y is exact 0; the order of the live terms is that of the element alone.
template <int HD, bool VL>
__global__ __launch_bounds__(256) void mha_rollout_step_kernel(MhaGeo g, const float* __restrict__ qkv,
                                                               const float* __restrict__ lse, const float* __restrict__ v,
                                                               float* __restrict__ y, long long units,
                                                               const int* __restrict__ lens, float a, float inv_heads) {
  constexpr int CW = HD / 4, QB = 4;
  const long long unit = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (unit >= units) return;
  const int lane = threadIdx.x & 63, i16 = lane & 15, g4 = lane >> 4;
  const Unit u = map_unit<VL>(g, unit, lens);
  const int E3 = 3 * g.E;
  const Slot k = mha_slot<false, VL>(g, u, u.tile, i16, lens);
  const float* vn = v + (long long)u.n * g.S;
  float* yn = y + (long long)u.n * g.S;
  if (mha_idle<false, VL>(u, k)) {   // wave-uniform: every key of the tile is padding
    if (k.real && g4 == 0) yn[k.s] = 0.f;
    return;
  }
  float part = 0.f;
  const int qtiles = mha_loop_tiles<false, VL>(g, u);
  const int last = u.len - 1;   // an empty query slot is clamped onto the last live position (u.len = S without lengths)
  for (int h = 0; h < g.heads; ++h) {   // the head outside: its 16 keys are loaded once
    float kv[CW];
    load_cols<CW>(qkv + k.row * E3 + g.E + h * HD + g4 * CW, kv);
    const float* lh = lse + ((long long)u.u + h) * g.S;
    const float* qh = qkv + (long long)u.n * g.rn * E3 + h * HD + g4 * CW;
    for (int q0 = 0; q0 < qtiles; q0 += QB) {
      // the loads of QB query tiles are issued together: with N * ceil(S / 16) waves there is little else to hide their
      // latency behind.  A tile past the last one is clamped like an empty slot and adds exact zeros.
      float qv[QB][CW], lr[QB][4], vr[QB][4];
#pragma unroll
      for (int b = 0; b < QB; ++b) {
        const int t16 = (q0 + b) * 16;
        load_cols<CW>(qh + (long long)min(t16 + i16, last) * g.rs * E3, qv[b]);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int sc = min(t16 + g4 * 4 + r, last);
          lr[b][r] = lh[sc];
          vr[b][r] = vn[sc];
        }
      }
#pragma unroll
      for (int b = 0; b < QB; ++b) {
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < CW; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(qv[b][s], kv[s], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool ok = (q0 + b) * 16 + g4 * 4 + r <= last && k.ok;
          const float p = ok ? expf(acc[r] * g.scale - lr[b][r]) : 0.f;
          part = fmaf(ok ? vr[b][r] : 0.f, p, part);
        }
      }
    }
  }
  part = rows_sum(part);
  if (!k.real || g4 != 0) return;
  yn[k.s] = k.ok ? fmaf(a, vn[k.s], (1.f - a) * (part * inv_heads)) : 0.f;
}

// 0 when the descriptor is accepted, else the message is set
static int mha_geo(const ecgmm_mha_desc* d, const char* what, MhaGeo* out) {
  if (!d) ECG_FAIL(ECGMM_ERR_SHAPE, "%s: null descriptor", what);
  if (d->S < 1 || d->N < 1 || d->heads < 1 || (d->head_dim != 16 && d->head_dim != 32) ||
      (d->batch_first != 0 && d->batch_first != 1) || !(d->p_drop >= 0.f && d->p_drop < 1.f))
    ECG_FAIL(ECGMM_ERR_SHAPE,
             "%s: need S, N, heads >= 1, head_dim 16 or 32, batch_first 0 or 1, 0 <= p_drop < 1 (S=%d N=%d heads=%d "
             "head_dim=%d batch_first=%d p_drop=%g)", what, d->S, d->N, d->heads, d->head_dim, d->batch_first, (double)d->p_drop);
  const long long P = (long long)d->N * d->heads, E = (long long)d->heads * d->head_dim, tiles = (d->S + 15) / 16;
  if (P > 0x7fffffffLL || E > (1 << 20) || P * tiles > 0x7fffffffLL * 4 || P * d->S > 0x7fffffffLL * 256)
    ECG_FAIL(ECGMM_ERR_SHAPE, "%s: N * heads * ceil(S / 16) beyond the launch grid (S=%d N=%d heads=%d)", what, d->S, d->N,
             d->heads);
  if (d->p_drop > 0.f && d->S > 32768)
    ECG_FAIL(ECGMM_ERR_SHAPE, "%s: dropout needs S <= 32768 (the Philox counter), S=%d", what, d->S);
  MhaGeo g;
  memset(&g, 0, sizeof(g));
  g.S = d->S; g.N = d->N; g.heads = d->heads; g.E = (int)E; g.P = (int)P; g.tiles = (int)tiles;
  g.G = d->S <= 8 ? 16 / d->S : 0;
  g.SB = (d->S + 3) / 4;
  g.rs = d->batch_first ? 1 : d->N;
  g.rn = d->batch_first ? d->S : 1;
  g.scale = 1.f / sqrtf((float)d->head_dim);
  g.p_drop = d->p_drop;
  g.inv_keep = 1.f / (1.f - d->p_drop);
  *out = g;
  return 0;
}

static long long mha_units(const MhaGeo& g) {
  return g.G ? ((long long)g.P + g.G - 1) / g.G : (long long)g.P * g.tiles;
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ------------------------------------------------------------------------------------------------
// embedding: y[b][l][c] = bias[c] + sum_{ci, k} w[c][ci][k] x[b][ci][l + k - 1] + pos[l][c]
// ------------------------------------------------------------------------------------------------
constexpr int EMB_MAX_CIN = 12;
constexpr int EMB_ROWS = 64;   // rows of (b, l) per partial sum of the weight gradient

__global__ __launch_bounds__(256) void embed1d_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                          const float* __restrict__ bias, const float* __restrict__ pos,
                                                          float* __restrict__ y, int B, int Cin, int L, int Dm) {
  const long long total = (long long)B * L * Dm;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int c = (int)(e % Dm);
    const long long row = e / Dm;
    const int l = (int)(row % L), b = (int)(row / L);
    float acc = bias[c];
    for (int ci = 0; ci < Cin; ++ci) {
      const float* xr = x + ((long long)b * Cin + ci) * L;
      const float* wr = w + ((long long)c * Cin + ci) * 3;
      if (l > 0) acc += wr[0] * xr[l - 1];
      acc += wr[1] * xr[l];
      if (l + 1 < L) acc += wr[2] * xr[l + 1];
    }
    y[e] = acc + pos[(long long)l * Dm + c];
  }
}

// grid (chunks, ceil(Dm / 64)), one wave: lane = channel, EMB_ROWS rows in order -> partial[chunk][3 Cin + 1][Dm]
__global__ __launch_bounds__(64) void embed1d_wgrad_rows_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                float* __restrict__ partial, int B, int Cin, int L, int Dm) {
  const int c = blockIdx.y * 64 + threadIdx.x;
  const long long rows = (long long)B * L, r0 = (long long)blockIdx.x * EMB_ROWS;
  float acc[3 * EMB_MAX_CIN], accb = 0.f;
#pragma unroll
  for (int j = 0; j < 3 * EMB_MAX_CIN; ++j) acc[j] = 0.f;
  for (int q = 0; q < EMB_ROWS; ++q) {
    const long long row = r0 + q;
    if (row >= rows) break;
    const int l = (int)(row % L), b = (int)(row / L);
    const float g = c < Dm ? dy[row * Dm + c] : 0.f;
    accb += g;
#pragma unroll
    for (int ci = 0; ci < EMB_MAX_CIN; ++ci) {
      if (ci < Cin) {
        const float* xr = x + ((long long)b * Cin + ci) * L;
        acc[3 * ci] += g * (l > 0 ? xr[l - 1] : 0.f);
        acc[3 * ci + 1] += g * xr[l];
        acc[3 * ci + 2] += g * (l + 1 < L ? xr[l + 1] : 0.f);
      }
    }
  }
  if (c >= Dm) return;
  const int J = 3 * Cin + 1;
  float* dst = partial + (long long)blockIdx.x * J * Dm + c;
#pragma unroll
  for (int j = 0; j < 3 * EMB_MAX_CIN; ++j)
    if (j < 3 * Cin) dst[(long long)j * Dm] = acc[j];
  dst[(long long)(J - 1) * Dm] = accb;
}

// one thread per (j, c): the chunks in order
__global__ __launch_bounds__(256) void embed1d_wgrad_sum_kernel(const float* __restrict__ partial, int chunks, int Cin,
                                                                int Dm, float* __restrict__ dw, float* __restrict__ db) {
  const int J = 3 * Cin + 1;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= J * Dm) return;
  const int j = e / Dm, c = e - j * Dm;
  float acc = 0.f;
  for (int k = 0; k < chunks; ++k) acc += partial[((long long)k * J + j) * Dm + c];
  if (j == J - 1) {
    if (db) db[c] = acc;
  } else if (dw) {
    dw[(long long)c * 3 * Cin + j] = acc;
  }
}

// dpos [pos_len][Dm]: rows below L are the sum over the batch (in order), the others zero
__global__ __launch_bounds__(256) void embed1d_dpos_kernel(const float* __restrict__ dy, float* __restrict__ dpos, int B,
                                                           int L, int Dm, int pos_len) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)pos_len * Dm) return;
  const long long l = e / Dm;
  float acc = 0.f;
  if (l < L)
    for (int b = 0; b < B; ++b) acc += dy[(long long)b * L * Dm + e];
  dpos[e] = acc;
}

// one wave per (b, l): dx[b][ci][l] = sum_k sum_c w[c][ci][k] dy[b][l + 1 - k][c]
__global__ __launch_bounds__(256) void embed1d_dx_kernel(const float* __restrict__ dy, const float* __restrict__ w,
                                                         float* __restrict__ dx, int B, int Cin, int L, int Dm) {
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= (long long)B * L) return;   // wave-uniform
  const int lane = threadIdx.x & 63;
  const int l = (int)(row % L), b = (int)(row / L);
  for (int ci = 0; ci < Cin; ++ci) {
    float acc = 0.f;
    for (int k = 0; k < 3; ++k) {
      const int ls = l + 1 - k;
      if (ls < 0 || ls >= L) continue;
      const float* g = dy + ((long long)b * L + ls) * Dm;
      for (int c = lane; c < Dm; c += 64) acc += w[((long long)c * Cin + ci) * 3 + k] * g[c];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) dx[((long long)b * Cin + ci) * L + l] = acc;
  }
}

static int embed_check(const char* what, int B, int Cin, int L, int Dm) {
  if (B < 1 || L < 1 || Cin < 1 || Cin > EMB_MAX_CIN || Dm < 1 || Dm > 4096 || (long long)B * L > 0x7fffffffLL)
    ECG_FAIL(ECGMM_ERR_SHAPE, "%s: need B, L >= 1, 1 <= input_dim <= %d, 1 <= d_model <= 4096, B * L < 2^31 (B=%d input_dim=%d "
             "L=%d d_model=%d)", what, EMB_MAX_CIN, B, Cin, L, Dm);
  return 0;
}

static size_t embed_ws(int B, int Cin, int L, int Dm) {
  const size_t chunks = ((size_t)B * L + EMB_ROWS - 1) / EMB_ROWS;
  return align_up(chunks * (3 * (size_t)Cin + 1) * Dm * sizeof(float), 256);
}

}  // namespace

extern "C" size_t ecgmm_mha_bwd_workspace(const ecgmm_mha_desc* d) {
  MhaGeo g;
  if (mha_geo(d, "mha_bwd_workspace", &g) != 0) return 0;
  return align_up((size_t)g.P * g.S * sizeof(float), 256);
}

// the instantiation of a kernel template for (head_dim, packed, with lengths)
#define MHA_PICK(kernel, hd, pk, vl)                                                               \
  ((hd) == 16 ? ((pk) ? ((vl) ? kernel<16, true, true> : kernel<16, true, false>)                  \
                      : ((vl) ? kernel<16, false, true> : kernel<16, false, false>))               \
              : ((pk) ? ((vl) ? kernel<32, true, true> : kernel<32, true, false>)                  \
                      : ((vl) ? kernel<32, false, true> : kernel<32, false, false>)))

static int mha_forward_impl(const char* what, const ecgmm_mha_desc* d, const float* qkv, const int32_t* lengths, float* out,
                            float* lse, uint64_t seed, uint64_t offset, void* stream) {
  MhaGeo g;
  ECG_TRY(mha_geo(d, what, &g));
  if (!qkv || !out || !lse) ECG_FAIL(ECGMM_ERR_SHAPE, "%s: null operand", what);
  if (!aligned16(qkv) || !aligned16(out)) ECG_FAIL(ECGMM_ERR_SHAPE, "%s: qkv and out must be 16-byte aligned", what);
  g.seed = seed; g.offset = offset;
  const long long units = mha_units(g);
  const dim3 grid((unsigned)((units + 3) / 4));
  auto* fn = MHA_PICK(mha_fwd_kernel, d->head_dim, g.G != 0, lengths != nullptr);
  hipLaunchKernelGGL(fn, grid, dim3(256), 0, (hipStream_t)stream, g, qkv, out, lse, units, (const int*)lengths);
  ECG_CHECK_LAUNCH(what);
  return 0;
}

static int mha_backward_impl(const char* what, const ecgmm_mha_desc* d, const float* qkv, const int32_t* lengths,
                             const float* out, const float* lse, const float* dout, float* dqkv, void* ws, size_t ws_bytes,
                             uint64_t seed, uint64_t offset, void* stream) {
  MhaGeo g;
  ECG_TRY(mha_geo(d, what, &g));
  if (!qkv || !out || !lse || !dout || !dqkv || !ws) ECG_FAIL(ECGMM_ERR_SHAPE, "%s: null operand", what);
  if (!aligned16(qkv) || !aligned16(out) || !aligned16(dout) || !aligned16(dqkv))
    ECG_FAIL(ECGMM_ERR_SHAPE, "%s: qkv, out, dout and dqkv must be 16-byte aligned", what);
  const size_t need = align_up((size_t)g.P * g.S * sizeof(float), 256);
  if (ws_bytes < need) ECG_FAIL(ECGMM_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", what, ws_bytes, need);
  g.seed = seed; g.offset = offset;
  hipStream_t st = (hipStream_t)stream;
  float* D = (float*)ws;
  const long long units = mha_units(g);
  const dim3 grid((unsigned)((units + 3) / 4)), grid_d((unsigned)(((long long)g.P * g.S + 255) / 256));
  const bool vl = lengths != nullptr, pk = g.G != 0;
  const int* lens = (const int*)lengths;
  auto* fn_d = d->head_dim == 16 ? (vl ? mha_rowdot_kernel<16, true> : mha_rowdot_kernel<16, false>)
                                 : (vl ? mha_rowdot_kernel<32, true> : mha_rowdot_kernel<32, false>);
  auto* fn_kv = MHA_PICK(mha_bwd_kv_kernel, d->head_dim, pk, vl);
  auto* fn_q = MHA_PICK(mha_bwd_q_kernel, d->head_dim, pk, vl);
  hipLaunchKernelGGL(fn_d, grid_d, dim3(256), 0, st, g, out, dout, D, lens);
  ECG_CHECK_LAUNCH(what);
  hipLaunchKernelGGL(fn_kv, grid, dim3(256), 0, st, g, qkv, lse, D, dout, dqkv, units, lens);
  ECG_CHECK_LAUNCH(what);
  hipLaunchKernelGGL(fn_q, grid, dim3(256), 0, st, g, qkv, lse, D, dout, dqkv, units, lens);
  ECG_CHECK_LAUNCH(what);
  return 0;
}

extern "C" int ecgmm_mha_forward(const ecgmm_mha_desc* d, const float* qkv, float* out, float* lse, uint64_t seed,
                                 uint64_t offset, void* stream) {
  return mha_forward_impl("mha_forward", d, qkv, nullptr, out, lse, seed, offset, stream);
}

extern "C" int ecgmm_mha_backward(const ecgmm_mha_desc* d, const float* qkv, const float* out, const float* lse,
                                  const float* dout, float* dqkv, void* ws, size_t ws_bytes, uint64_t seed, uint64_t offset,
                                  void* stream) {
  return mha_backward_impl("mha_backward", d, qkv, nullptr, out, lse, dout, dqkv, ws, ws_bytes, seed, offset, stream);
}

extern "C" int ecgmm_mha_forward_varlen(const ecgmm_mha_desc* d, const float* qkv, const int32_t* lengths, float* out,
                                        float* lse, uint64_t seed, uint64_t offset, void* stream) {
  return mha_forward_impl("mha_forward_varlen", d, qkv, lengths, out, lse, seed, offset, stream);
}

extern "C" int ecgmm_mha_backward_varlen(const ecgmm_mha_desc* d, const float* qkv, const int32_t* lengths, const float* out,
                                         const float* lse, const float* dout, float* dqkv, void* ws, size_t ws_bytes,
                                         uint64_t seed, uint64_t offset, void* stream) {
  return mha_backward_impl("mha_backward_varlen", d, qkv, lengths, out, lse, dout, dqkv, ws, ws_bytes, seed, offset, stream);
}

extern "C" int ecgmm_mha_keep_mask(const ecgmm_mha_desc* d, uint8_t* mask, uint64_t seed, uint64_t offset, void* stream) {
  MhaGeo g;
  ECG_TRY(mha_geo(d, "mha_keep_mask", &g));
  if (!mask) ECG_FAIL(ECGMM_ERR_SHAPE, "mha_keep_mask: null operand");
  if (d->S > 32768) ECG_FAIL(ECGMM_ERR_SHAPE, "mha_keep_mask: needs S <= 32768, S=%d", d->S);
  const long long n = (long long)g.P * g.S * g.SB;
  if (n > 0x7fffffffLL * 256) ECG_FAIL(ECGMM_ERR_SHAPE, "mha_keep_mask: N * heads * S * S / 4 beyond the launch grid");
  g.seed = seed; g.offset = offset;
  hipLaunchKernelGGL(mha_keep_mask_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g, mask);
  ECG_CHECK_LAUNCH("mha_keep_mask");
  return 0;
}

extern "C" int ecgmm_mha_weights(const ecgmm_mha_desc* d, const float* qkv, const float* lse, const int32_t* lengths,
                                 float* weights, int per_head, void* stream) {
  MhaGeo g;
  ECG_TRY(mha_geo(d, "mha_weights", &g));
  if (!qkv || !lse || !weights) ECG_FAIL(ECGMM_ERR_SHAPE, "mha_weights: null operand");
  if (!aligned16(qkv)) ECG_FAIL(ECGMM_ERR_SHAPE, "mha_weights: qkv must be 16-byte aligned");
  if (per_head != 0 && per_head != 1) ECG_FAIL(ECGMM_ERR_SHAPE, "mha_weights: per_head must be 0 or 1, got %d", per_head);
  const long long units = (long long)g.N * g.tiles;
  const dim3 grid((unsigned)((units + 3) / 4));
  const bool vl = lengths != nullptr;
  const int vec = g.S % 4 == 0 && aligned16(weights);
  auto* fn = d->head_dim == 16
                 ? (vl ? (per_head ? mha_weights_kernel<16, true, true> : mha_weights_kernel<16, true, false>)
                       : (per_head ? mha_weights_kernel<16, false, true> : mha_weights_kernel<16, false, false>))
                 : (vl ? (per_head ? mha_weights_kernel<32, true, true> : mha_weights_kernel<32, true, false>)
                       : (per_head ? mha_weights_kernel<32, false, true> : mha_weights_kernel<32, false, false>));
  hipLaunchKernelGGL(fn, grid, dim3(256), 0, (hipStream_t)stream, g, qkv, lse, weights, units, (const int*)lengths,
                     1.f / (float)g.heads, vec);
  ECG_CHECK_LAUNCH("mha_weights");
  return 0;
}

extern "C" int ecgmm_mha_rollout_step(const ecgmm_mha_desc* d, const float* qkv, const float* lse, const int32_t* lengths,
                                      const float* v_in, float* v_out, float residual, void* stream) {
  MhaGeo g;
  ECG_TRY(mha_geo(d, "mha_rollout_step", &g));
  if (!qkv || !lse || !v_in || !v_out) ECG_FAIL(ECGMM_ERR_SHAPE, "mha_rollout_step: null operand");
  if (!aligned16(qkv)) ECG_FAIL(ECGMM_ERR_SHAPE, "mha_rollout_step: qkv must be 16-byte aligned");
  if (!(residual >= 0.f && residual < 1.f))
    ECG_FAIL(ECGMM_ERR_SHAPE, "mha_rollout_step: need 0 <= residual < 1, got %g", (double)residual);
  if (v_in == v_out) ECG_FAIL(ECGMM_ERR_SHAPE, "mha_rollout_step: v_out must not be v_in (every unit reads all of v_in)");
  const long long units = (long long)g.N * g.tiles;
  const dim3 grid((unsigned)((units + 3) / 4));
  const bool vl = lengths != nullptr;
  auto* fn = d->head_dim == 16 ? (vl ? mha_rollout_step_kernel<16, true> : mha_rollout_step_kernel<16, false>)
                               : (vl ? mha_rollout_step_kernel<32, true> : mha_rollout_step_kernel<32, false>);
  hipLaunchKernelGGL(fn, grid, dim3(256), 0, (hipStream_t)stream, g, qkv, lse, v_in, v_out, units, (const int*)lengths,
                     residual, 1.f / (float)g.heads);
  ECG_CHECK_LAUNCH("mha_rollout_step");
  return 0;
}

extern "C" int ecgmm_embed1d_fwd(const float* x, const float* w, const float* bias, const float* pos, float* y, int B,
                                 int Cin, int L, int Dm, void* stream) {
  ECG_TRY(embed_check("embed1d_fwd", B, Cin, L, Dm));
  if (!x || !w || !bias || !pos || !y) ECG_FAIL(ECGMM_ERR_SHAPE, "embed1d_fwd: null operand");
  const long long total = (long long)B * L * Dm;
  const long long blocks = (total + 255) / 256;
  hipLaunchKernelGGL(embed1d_fwd_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0,
                     (hipStream_t)stream, x, w, bias, pos, y, B, Cin, L, Dm);
  ECG_CHECK_LAUNCH("embed1d_fwd");
  return 0;
}

extern "C" size_t ecgmm_embed1d_bwd_workspace(int B, int Cin, int L, int Dm) {
  if (embed_check("embed1d_bwd_workspace", B, Cin, L, Dm) != 0) return 0;
  return embed_ws(B, Cin, L, Dm);
}

extern "C" int ecgmm_embed1d_bwd(const float* x, const float* w, const float* dy, float* dw, float* db, float* dpos,
                                 float* dx, int B, int Cin, int L, int Dm, int pos_len, void* ws, size_t ws_bytes,
                                 void* stream) {
  ECG_TRY(embed_check("embed1d_bwd", B, Cin, L, Dm));
  if (!x || !w || !dy) ECG_FAIL(ECGMM_ERR_SHAPE, "embed1d_bwd: null operand");
  if (dpos && pos_len < L) ECG_FAIL(ECGMM_ERR_SHAPE, "embed1d_bwd: pos_len=%d below L=%d", pos_len, L);
  hipStream_t st = (hipStream_t)stream;
  if (dw || db) {
    const size_t need = embed_ws(B, Cin, L, Dm);
    if (!ws || ws_bytes < need)
      ECG_FAIL(ECGMM_ERR_WORKSPACE, "embed1d_bwd: workspace of %zu bytes, %zu needed", ws ? ws_bytes : (size_t)0, need);
    const int chunks = (int)(((long long)B * L + EMB_ROWS - 1) / EMB_ROWS);
    hipLaunchKernelGGL(embed1d_wgrad_rows_kernel, dim3((unsigned)chunks, (unsigned)ceil_div(Dm, 64)), dim3(64), 0, st, x, dy,
                       (float*)ws, B, Cin, L, Dm);
    ECG_CHECK_LAUNCH("embed1d_bwd rows");
    hipLaunchKernelGGL(embed1d_wgrad_sum_kernel, dim3((unsigned)ceil_div((long)(3 * Cin + 1) * Dm, 256)), dim3(256), 0, st,
                       (const float*)ws, chunks, Cin, Dm, dw, db);
    ECG_CHECK_LAUNCH("embed1d_bwd sum");
  }
  if (dpos) {
    hipLaunchKernelGGL(embed1d_dpos_kernel, dim3((unsigned)ceil_div((long)pos_len * Dm, 256)), dim3(256), 0, st, dy, dpos, B,
                       L, Dm, pos_len);
    ECG_CHECK_LAUNCH("embed1d_bwd dpos");
  }
  if (dx) {
    hipLaunchKernelGGL(embed1d_dx_kernel, dim3((unsigned)(((long long)B * L + 3) / 4)), dim3(256), 0, st, dy, w, dx, B, Cin, L,
                       Dm);
    ECG_CHECK_LAUNCH("embed1d_bwd dx");
  }
  return 0;
}
