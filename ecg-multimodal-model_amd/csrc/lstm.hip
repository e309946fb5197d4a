// nn.LSTM (multi-layer, optionally bidirectional), fp32, forward and back-propagation through time.
//
// Per layer and direction (torch semantics, gate order i, f, g, o):
//   gates_t = x_t W_ih^T + b_ih + h_{t-1} W_hh^T + b_hh;  c_t = s(f) c_{t-1} + s(i) tanh(g);  h_t = s(o) tanh(c_t)
// The input projection x W_ih^T + b_ih of ALL time steps is one ecg_linear_fwd launch (linear.hip) per layer and direction;
// what is left is the recurrence, sequential in t and independent across batch rows:
//
//   lstm_seq_fwd_kernel : a persistent workgroup owns LSTM_ROWS = 16 batch rows of one direction (blockIdx.y) for all T
//     steps.  h (double-buffered) and c of the slice live in LDS; W_hh [4H][H] streams from L2 every step.  The 16 batch
//     rows are the M side of v_mfma_f32_16x16x4_f32 (exact fp32 products); the hidden units are split over the 8 waves
//     in tiles of 16, and a wave computes all four gates of its tiles, so the cell update is lane-local in the MFMA's
//     C/D layout.  One workgroup barrier per step.  No synchronisation between workgroups of any kind.
//   lstm_seq_bwd_kernel : the same slices, time in the opposite order.  Per step the gate gradients are formed lane-locally
//     (same ownership as the forward), staged in LDS, and dh_{t-1} = dgates_t W_hh is an MFMA with K = 4H.  Two barriers
//     per step (the staged gate gradients are read by every wave).  It writes dgates [B T][4H]; the parameter and input
//     gradients are the existing GEMMs of ecg_linear_bwd over (dgates, layer input) and (dgates, h_{t-1}).
//
// Rows >= B of a ragged slice are masked at every global access (never read or written); no barrier sits in a branch.
// Any H works: H % 4 != 0 (or a W_hh that is not 16-byte aligned) takes 4-byte W_hh loads in the forward.
// LSTM_MAX_H = 384: the backward stages 16 x (4 Hp + 4) gate gradients + 2 x 16 x (Hp + 4) carries in LDS (Hp = H rounded
// up to 16) = 148 KiB at H = 384 of the 160 KiB of a CU; the forward needs 3 x 16 x (Hp + 4) floats (73 KiB).
//
// Variable lengths (ecg_lstm_forward / _backward with lengths != null) are the VL = true instantiations of the same two
// kernels; VL = false computes what it computed before there were lengths, bit for bit.  Row b is live at step t iff
// t < lengths[b] (clamped to [0, T]), in both directions: torch's packed LSTM re-padded.  A workgroup keeps its 16 lengths behind its other LDS arrays (+ 64 B) and runs
// only tmax = max of them steps (uniform over the workgroup: every barrier is reached by every thread).
//   forward   dead row: h copied to the other buffer, c left, y = 0, hprev = the held h (finite: the dW_hh GEMM reads every
//             row of hprev, and 0 * NaN is NaN).  Steps tmax .. T-1 of the slice get y = 0, hprev = 0 before the walk.
//             h_n is the buffer of parity tmax, not T.
//   backward  the executed steps in the opposite order; c_{t-1} = c0 at the ROW's first step (t = 0 forward, t = len-1
//             reverse); dead row: dgates = 0 (and over tmax .. T-1: the GEMMs read all B T rows), dc and dh carries kept.
//             The cell arithmetic is one code path for both instantiations, contraction pinned (see the kernel): lengths
//             all T give the fixed call's bits.
// The projection / gradient GEMMs stay over all B T rows; padded x meets exact zeros there, so it must be finite.
#include "ops.h"

namespace {

constexpr int LSTM_ROWS = 16;
constexpr int LSTM_THREADS = 512;
constexpr int LSTM_WAVES = LSTM_THREADS / 64;
constexpr int LSTM_MAX_H = 384;
constexpr int LSTM_MAX_LAYERS = 8;

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }   // exp -> inf gives exactly 0

struct LstmFwdDir {
  float* gates;         // [B T][4H]: in x W_ih^T + b_ih; out (save) the activated gates
  const float* w_hh;    // [4H][H]
  const float* b_hh;    // [4H]
  const float* h0;      // [B][H] of this layer and direction, or null (zeros)
  const float* c0;
  float* out;           // layer output + this direction's column offset, row stride ldo
  float* hprev;         // save: [B T][H], h_{t-1} of every step (h0 at the first)
  float* csave;         // save: [B T][H], c_t
  float* hn;            // [B][H] or null
  float* cn;
  int reverse;
};
struct LstmFwdArgs {
  LstmFwdDir d[2];
  const int* lengths;   // [B] or null (VL kernels only)
  int B, T, H, ldo, batch_first, save;
  const u32x4* w_pack[2];   // bf16 kernels: W_hh of each direction as bf16 B fragments (pack_whh_bf16_kernel)
};

struct LstmBwdDir {
  const float* gates;   // activated gates of the forward
  const float* csave;
  const float* c0;      // [B][H] or null
  const float* w_hh;
  const float* dy;      // gradient of the layer output + column offset, row stride ldo; or null
  const float* dhn;     // [B][H] or null
  const float* dcn;
  float* dgates;        // [B T][4H]
  float* dh0;           // [B][H] or null
  float* dc0;
  int reverse;
};
struct LstmBwdArgs {
  LstmBwdDir d[2];
  const int* lengths;   // [B] or null (VL kernels only)
  int B, T, H, ldo, batch_first;
  const u32x4* w_pack[2];   // bf16 kernels: W_hh^T of each direction as bf16 B fragments
};

__device__ __forceinline__ size_t seq_row(int b, int t, int B, int T, int batch_first) {
  return batch_first ? (size_t)b * T + t : (size_t)t * B + b;
}

// the slice's 16 lengths, clamped to [0, T] (0 for rows >= B), into LDS; call before the set-up barrier
__device__ __forceinline__ void load_slice_lengths(int* len, const int* lengths, int b0, int B, int T) {
  if (threadIdx.x < LSTM_ROWS) {
    const int b = b0 + threadIdx.x;
    int l = b < B ? lengths[b] : 0;
    len[threadIdx.x] = l < 0 ? 0 : (l > T ? T : l);
  }
}
__device__ __forceinline__ int slice_tmax(const int* len) {
  int m = 0;
#pragma unroll
  for (int r = 0; r < LSTM_ROWS; ++r) m = len[r] > m ? len[r] : m;
  return m;
}

template <bool V4, bool VL>
__global__ __launch_bounds__(LSTM_THREADS) void lstm_seq_fwd_kernel(LstmFwdArgs a) {
  extern __shared__ float lstm_lds[];
  const LstmFwdDir& p = a.d[blockIdx.y];
  const int H = a.H, Hp = (H + 15) & ~15, HS = Hp + 4, B = a.B, T = a.T;
  float* hb = lstm_lds;                       // [2][16][HS]
  float* cb = lstm_lds + 2 * LSTM_ROWS * HS;  // [16][HS]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i16 = lane & 15, g4 = lane >> 4;
  const int b0 = blockIdx.x * LSTM_ROWS;

  for (int e = tid; e < LSTM_ROWS * HS; e += LSTM_THREADS) {
    const int b = e / HS, j = e - b * HS;
    const bool ok = j < H && b0 + b < B;
    hb[e] = ok && p.h0 ? p.h0[(size_t)(b0 + b) * H + j] : 0.f;
    hb[LSTM_ROWS * HS + e] = 0.f;
    cb[e] = ok && p.c0 ? p.c0[(size_t)(b0 + b) * H + j] : 0.f;
  }
  int* len = reinterpret_cast<int*>(lstm_lds + 3 * LSTM_ROWS * HS);   // [16], VL only
  if (VL) load_slice_lengths(len, a.lengths, b0, B, T);
  __syncthreads();
  const int tmax = VL ? slice_tmax(len) : T;   // executed steps: uniform over the workgroup
  int lr[4];                                   // lengths of this lane's four rows of the C/D tile
#pragma unroll
  for (int r = 0; r < 4; ++r) lr[r] = VL ? len[g4 * 4 + r] : T;
  if (VL) {   // steps tmax .. T-1 of the slice: y = 0 and a finite hprev
    const int nb = B - b0 < LSTM_ROWS ? B - b0 : LSTM_ROWS;
    for (int e = tid; e < (T - tmax) * nb * H; e += LSTM_THREADS) {
      const int tt = tmax + e / (nb * H), q = e % (nb * H), b = b0 + q / H, j = q % H;
      const size_t row = seq_row(b, tt, B, T, a.batch_first);
      p.out[row * a.ldo + j] = 0.f;
      if (a.save) p.hprev[row * H + j] = 0.f;
    }
  }

  const size_t HH = (size_t)H * H;
  const int G4 = 4 * H;
  for (int s = 0; s < tmax; ++s) {
    const int t = p.reverse ? tmax - 1 - s : s;
    const float* hc = hb + (s & 1) * LSTM_ROWS * HS;
    float* hx = hb + ((s + 1) & 1) * LSTM_ROWS * HS;
    for (int ht = wave; ht * 16 < Hp; ht += LSTM_WAVES) {
      const int j = ht * 16 + i16;   // hidden unit: row of W_hh fed as the B operand, column of the C/D tile
      const bool jok = j < H;
      size_t row[4];
      bool rok[4];
      float xg[4][4], bh[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int b = b0 + g4 * 4 + r;
        rok[r] = jok && b < B;
        row[r] = seq_row(b < B ? b : B - 1, t, B, T, a.batch_first);
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        bh[g] = jok ? p.b_hh[g * H + j] : 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) xg[g][r] = rok[r] ? p.gates[row[r] * G4 + g * H + j] : 0.f;
      }
      f32x4 acc[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
      const float* wrow = p.w_hh + (size_t)(jok ? j : 0) * H;
      for (int k0 = 0; k0 < Hp; k0 += 16) {
        const int k = k0 + 4 * g4;   // this lane's four reduction indices of the 16-wide step: k .. k + 3
        const float4 hv = *reinterpret_cast<const float4*>(hc + i16 * HS + k);
        const float av[4] = {hv.x, hv.y, hv.z, hv.w};
        float wv[4][4];
        if (V4) {
          const bool ok = jok && k < H;
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            float4 w = ok ? *reinterpret_cast<const float4*>(wrow + g * HH + k) : float4{0.f, 0.f, 0.f, 0.f};
            wv[g][0] = w.x; wv[g][1] = w.y; wv[g][2] = w.z; wv[g][3] = w.w;
          }
        } else {
#pragma unroll
          for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int u = 0; u < 4; ++u) wv[g][u] = jok && k + u < H ? wrow[g * HH + k + u] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], wv[g][u], acc[g], 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int bl = g4 * 4 + r;
        const float ig = sigmoidf_(acc[0][r] + xg[0][r] + bh[0]);
        const float fg = sigmoidf_(acc[1][r] + xg[1][r] + bh[1]);
        const float gg = tanhf(acc[2][r] + xg[2][r] + bh[2]);
        const float og = sigmoidf_(acc[3][r] + xg[3][r] + bh[3]);
        const float hp = hc[bl * HS + j];
        if (VL && t >= lr[r]) {   // dead row: hold h and c, y = 0; the held h is the finite hprev the dW_hh GEMM reads
          hx[bl * HS + j] = hp;
          if (rok[r]) {
            p.out[row[r] * a.ldo + j] = 0.f;
            if (a.save) p.hprev[row[r] * H + j] = hp;
          }
          continue;
        }
        const float c = fg * cb[bl * HS + j] + ig * gg;
        const float h = og * tanhf(c);
        cb[bl * HS + j] = jok ? c : 0.f;
        hx[bl * HS + j] = jok ? h : 0.f;   // columns H .. Hp stay zero: they are reduction padding of the next step
        if (rok[r]) {
          p.out[row[r] * a.ldo + j] = h;
          if (a.save) {
            float* gp = p.gates + row[r] * G4 + j;
            gp[0] = ig; gp[H] = fg; gp[2 * H] = gg; gp[3 * H] = og;
            p.csave[row[r] * H + j] = c;
            p.hprev[row[r] * H + j] = hp;
          }
        }
      }
    }
    __syncthreads();
  }

  const float* hl = hb + (tmax & 1) * LSTM_ROWS * HS;   // the buffer the last executed step wrote (h0 when none ran)
  for (int e = tid; e < LSTM_ROWS * H; e += LSTM_THREADS) {
    const int b = e / H, j = e - b * H;
    if (b0 + b < B) {
      if (p.hn) p.hn[(size_t)(b0 + b) * H + j] = hl[b * HS + j];
      if (p.cn) p.cn[(size_t)(b0 + b) * H + j] = cb[b * HS + j];
    }
  }
}

template <bool VL>
__global__ __launch_bounds__(LSTM_THREADS) void lstm_seq_bwd_kernel(LstmBwdArgs a) {
  extern __shared__ float lstm_lds[];
  const LstmBwdDir& p = a.d[blockIdx.y];
  const int H = a.H, Hp = (H + 15) & ~15, HS = Hp + 4, GS = 4 * Hp + 4, B = a.B, T = a.T;
  float* dgs = lstm_lds;                  // [16][GS]: gate gradients of the step, gate g at columns g Hp .. g Hp + H
  float* dhb = dgs + LSTM_ROWS * GS;      // [16][HS]: dh carried to the previous step
  float* dcb = dhb + LSTM_ROWS * HS;      // [16][HS]: dc carried
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i16 = lane & 15, g4 = lane >> 4;
  const int b0 = blockIdx.x * LSTM_ROWS;

  for (int e = tid; e < LSTM_ROWS * GS; e += LSTM_THREADS) dgs[e] = 0.f;
  for (int e = tid; e < LSTM_ROWS * HS; e += LSTM_THREADS) {
    const int b = e / HS, j = e - b * HS;
    const bool ok = j < H && b0 + b < B;
    dhb[e] = ok && p.dhn ? p.dhn[(size_t)(b0 + b) * H + j] : 0.f;
    dcb[e] = ok && p.dcn ? p.dcn[(size_t)(b0 + b) * H + j] : 0.f;
  }
  int* len = reinterpret_cast<int*>(dcb + LSTM_ROWS * HS);   // [16], VL only
  if (VL) load_slice_lengths(len, a.lengths, b0, B, T);
  __syncthreads();
  const int tmax = VL ? slice_tmax(len) : T;   // the steps the forward executed: uniform over the workgroup
  int lr[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) lr[r] = VL ? len[g4 * 4 + r] : T;

  const int G4 = 4 * H;
  if (VL) {   // steps tmax .. T-1 of the slice: the GEMMs after this kernel read all B T rows of dgates
    const int nb = B - b0 < LSTM_ROWS ? B - b0 : LSTM_ROWS;
    for (int e = tid; e < (T - tmax) * nb * G4; e += LSTM_THREADS) {
      const int tt = tmax + e / (nb * G4), q = e % (nb * G4), b = b0 + q / G4, n = q % G4;
      p.dgates[seq_row(b, tt, B, T, a.batch_first) * G4 + n] = 0.f;
    }
  }
  for (int s = 0; s < tmax; ++s) {
    const int t = p.reverse ? s : tmax - 1 - s;       // the forward walk, backwards
    const bool first = s == tmax - 1;                 // (fixed lengths) the forward's first step: c_{t-1} = c0
    const int tp = p.reverse ? t + 1 : t - 1;
    for (int ht = wave; ht * 16 < Hp; ht += LSTM_WAVES) {
      const int j = ht * 16 + i16;
      const bool jok = j < H;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int bl = g4 * 4 + r, b = b0 + bl;
        float di = 0.f, df = 0.f, dg = 0.f, dop = 0.f, dcp = 0.f;
        // A dead row (VL) runs the same arithmetic on whatever its position holds (in bounds; the result is dropped by the
        // selects below) instead of branching around it: the live rows' arithmetic then compiles to the contractions of the
        // fixed kernel, so that lengths all T, and a row alone at T = its length, give the fixed call's bits.
        const bool live = !VL || t < lr[r];
        if (jok && b < B) {
          // Contraction is off in this block and the two fused multiply-adds the fixed kernel has always compiled to
          // (1 - tanh^2 c, and dc) are spelled out: left to the compiler, the VL instantiation fuses other products than the
          // fixed one (they land in different basic blocks), and lengths all T would differ from the fixed call in the last bit.
          // From here on these two fmas and the unfused products DEFINE the backward's arithmetic, for both instantiations: they
          // no longer follow a compiler's choice, and a change to them changes the results of the fixed entry point too.
#pragma clang fp contract(off)
          const size_t row = seq_row(b, t, B, T, a.batch_first);
          const float* gp = p.gates + row * G4 + j;
          const float ig = gp[0], fg = gp[H], gg = gp[2 * H], og = gp[3 * H];
          const float c = p.csave[row * H + j];
          // with lengths the ROW's first forward step: t = 0 forward, t = len - 1 reverse (a dead row: no step t +- 1 read)
          const bool rfirst = VL ? (!live || (p.reverse ? t == lr[r] - 1 : t == 0)) : first;
          const float cp = rfirst ? (p.c0 ? p.c0[(size_t)b * H + j] : 0.f)
                                  : p.csave[seq_row(b, tp, B, T, a.batch_first) * H + j];
          const float dh = (p.dy ? p.dy[row * a.ldo + j] : 0.f) + dhb[bl * HS + j];
          const float tc = tanhf(c);
          const float dc = __builtin_fmaf(dh * og, __builtin_fmaf(-tc, tc, 1.f), dcb[bl * HS + j]);
          dop = dh * tc * og * (1.f - og);
          di = dc * gg * ig * (1.f - ig);
          df = dc * cp * fg * (1.f - fg);
          dg = dc * ig * (1.f - gg * gg);
          dcp = dc * fg;
          if (VL) {   // dead row: exact-zero gate gradients, the dc carry kept (dh: below); dy there is not used
            di = live ? di : 0.f; df = live ? df : 0.f; dg = live ? dg : 0.f; dop = live ? dop : 0.f;
            dcp = live ? dcp : dcb[bl * HS + j];
          }
          float* dq = p.dgates + row * G4 + j;
          dq[0] = di; dq[H] = df; dq[2 * H] = dg; dq[3 * H] = dop;
        }
        dcb[bl * HS + j] = dcp;
        float* ds = dgs + bl * GS + j;
        ds[0] = di; ds[Hp] = df; ds[2 * Hp] = dg; ds[3 * Hp] = dop;
      }
    }
    __syncthreads();
    // dh_{t-1}[b][k] = sum_n dgates[b][n] W_hh[n][k]: this wave's tiles of k, the same tiles it owns above
    for (int kt = wave; kt * 16 < Hp; kt += LSTM_WAVES) {
      const int k = kt * 16 + i16;
      const bool kok = k < H;
      const float* wcol = p.w_hh + (kok ? k : 0);
      f32x4 acc[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int j0 = 0; j0 < Hp; j0 += 16) {
        const int jj = j0 + 4 * g4;
        float av[4][4], wv[4][4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const float4 d4 = *reinterpret_cast<const float4*>(dgs + i16 * GS + g * Hp + jj);
          av[g][0] = d4.x; av[g][1] = d4.y; av[g][2] = d4.z; av[g][3] = d4.w;
#pragma unroll
          for (int u = 0; u < 4; ++u) wv[g][u] = kok && jj + u < H ? wcol[(size_t)(g * H + jj + u) * H] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[g][u], wv[g][u], acc[g], 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (!VL || t < lr[r])   // a dead row keeps its dh carry
          dhb[(g4 * 4 + r) * HS + k] = (acc[0][r] + acc[1][r]) + (acc[2][r] + acc[3][r]);
    }
    __syncthreads();
  }

  for (int e = tid; e < LSTM_ROWS * H; e += LSTM_THREADS) {
    const int b = e / H, j = e - b * H;
    if (b0 + b < B) {
      if (p.dh0) p.dh0[(size_t)(b0 + b) * H + j] = dhb[b * HS + j];
      if (p.dc0) p.dc0[(size_t)(b0 + b) * H + j] = dcb[b * HS + j];
    }
  }
}

// ---- compute dtype bf16: the recurrent products on v_mfma_f32_16x16x32_bf16, W_hh held on chip ---------------------------------
// Only the recurrent operands are rounded (f2bf, to nearest even): pre_t = P_t + b_hh + bf(h_{t-1}) bf(W_hh)^T in the forward,
// dh_{t-1} = dy_{t-1} + bf(dgates_t) bf(W_hh) in the backward; products are exact and summed in fp32 in the accumulator, in the
// order of the K steps.  Everything stored (y, h_{t-1}, c_t, gates, dgates, the states) is the unrounded fp32 value.
// Same slices and ownership as the fp32 kernels: tile ht = wave + 8 ti of 16 hidden units belongs to one wave for all steps, so
// c, the fp32 h, and the dh / dc carries are lane-local REGISTERS in the C/D layout (row 4 (lane >> 4) + r, unit lane & 15); LDS
// holds only what every wave reads: bf16 h (double-buffered, one barrier per step) resp. the step's bf16 gate gradients (two
// barriers per step).  K is padded with zeros to a multiple of 32: KS = ceil(Hp / 32) steps forward, 4 Hp / 32 backward.
// One pack launch per call rounds the fp32 W_hh of every layer and direction to bf16 B fragments in operand order, into the
// workspace (written by every call from the parameter itself: there is no copy that could go stale).  Before the time loop a
// wave fetches its own tiles' fragments once, 16 bytes per lane and fragment: the first KR K-steps of each tile stay in
// registers; the rest sits in LDS (REST = 1: no W_hh byte is fetched inside the time loop) or, where it does not fit, streams
// from that copy every step (REST = 2).  (Converting from fp32 inside the set-up was tried: the compiler gathers the eight
// scalar loads of every fragment before the first conversion, and the kernel spills hundreds of registers.)
// Fragment of lane l for K-step ks: elements k = 32 ks + 8 (l >> 4) + 0..7 of A's row / B's column l & 15.

// forward B operand: unit j of gate g, reduction indices k0 .. k0 + 7 of W_hh [4H][H]
__device__ __forceinline__ u32x4 whh_frag_fwd(const float* w, int H, int g, int j, int k0) {
  // every load is in bounds (clamped) and unconditional, then selected: no branch per element
  const float* wrow = w + ((size_t)g * H + (j < H ? j : H - 1)) * H;
  float f[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int k = k0 + u;
    const float v = wrow[k < H ? k : H - 1];
    f[u] = j < H && k < H ? v : 0.f;
  }
  return pack16<bf16_t>(f);
}
// backward B operand: output unit k, reduction indices n0 .. n0 + 7 of the padded gate columns (gate g at g Hp .. g Hp + H)
__device__ __forceinline__ u32x4 whh_frag_bwd(const float* w, int H, int Hp, int k, int n0) {
  const int g = n0 / Hp, j0 = n0 - g * Hp;   // n0 % 8 == 0 and Hp % 16 == 0: the eight columns are of one gate
  const float* wcol = w + (size_t)(g < 4 ? g : 3) * H * H + (k < H ? k : H - 1);
  float f[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int j = j0 + u;
    const float v = wcol[(size_t)(j < H ? j : H - 1) * H];   // in bounds (clamped), unconditional, then selected
    f[u] = g < 4 && k < H && j < H ? v : 0.f;
  }
  return pack16<bf16_t>(f);
}
__device__ __forceinline__ f32x4 mfma_bf16(const u32x4& a, const u32x4& b, const f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
}

struct LstmPackArgs {
  const float* w[2 * LSTM_MAX_LAYERS];
  u32x4* dst[2 * LSTM_MAX_LAYERS];
  int H, transposed;
};
// forward: dst[((ht KS + ks) 4 + g) 64 + lane]; transposed (backward): dst[(kt KSB + ks) 64 + lane].  blockIdx.y = matrix.
__global__ __launch_bounds__(256) void pack_whh_bf16_kernel(LstmPackArgs a) {
  const int H = a.H, Hp = (H + 15) & ~15, tiles = Hp >> 4;
  const float* w = a.w[blockIdx.y];
  u32x4* dst = a.dst[blockIdx.y];
  const int KS = a.transposed ? Hp >> 3 : (Hp + 31) >> 5;
  const int n = tiles * KS * (a.transposed ? 1 : 4) * 64;
  for (int e = blockIdx.x * 256 + threadIdx.x; e < n; e += gridDim.x * 256) {
    const int lane = e & 63, i16 = lane & 15, g4 = lane >> 4;
    int q = e >> 6;
    if (a.transposed) {
      const int ks = q % KS, kt = q / KS;
      dst[e] = whh_frag_bwd(w, H, Hp, kt * 16 + i16, ks * 32 + 8 * g4);
    } else {
      const int g = q & 3;
      q >>= 2;
      const int ks = q % KS, ht = q / KS;
      dst[e] = whh_frag_fwd(w, H, g, ht * 16 + i16, ks * 32 + 8 * g4);
    }
  }
}

// KR K-steps in registers for a wave's first tile, KR1 <= KR for its others (two or three tiles at KR each leave the cell
// update no registers: the compiler spills)
template <int NT, int KR, int KR1, int REST, bool VL>
__global__ __launch_bounds__(LSTM_THREADS) void lstm_seq_fwd_bf16_kernel(LstmFwdArgs a) {
  extern __shared__ float lstm_lds[];
  const LstmFwdDir& p = a.d[blockIdx.y];
  const int H = a.H, Hp = (H + 15) & ~15, KS = (Hp + 31) >> 5, HB = KS * 32 + 8, B = a.B, T = a.T;
  const int rest0 = KS > KR ? KS - KR : 0, rest1 = KS > KR1 ? KS - KR1 : 0;   // K-steps not in registers: tiles 0..7, others
  bf16_t* hb = reinterpret_cast<bf16_t*>(lstm_lds);             // [2][16][HB]: bf(h), columns H .. 32 KS stay zero
  int* len = reinterpret_cast<int*>(hb + 2 * LSTM_ROWS * HB);   // [16]
  u32x4* wl = reinterpret_cast<u32x4*>(len + LSTM_ROWS);        // REST == 1: [tile][rest][4][64] B fragments
  const u32x4* wg = a.w_pack[blockIdx.y];                       // all of bf(W_hh) as B fragments (pack_whh_bf16_kernel)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i16 = lane & 15, g4 = lane >> 4;
  const int b0 = blockIdx.x * LSTM_ROWS;

  for (int e = tid; e < LSTM_ROWS * HB; e += LSTM_THREADS) {
    const int b = e / HB, j = e - b * HB;
    const bool ok = j < H && b0 + b < B;
    hb[e] = ok && p.h0 ? f2bf(p.h0[(size_t)(b0 + b) * H + j]) : (bf16_t)0;
    hb[LSTM_ROWS * HB + e] = 0;
  }
  if (VL) load_slice_lengths(len, a.lengths, b0, B, T);
  u32x4 wr[NT][KR][4];   // this wave's tiles, K-steps 0 .. KR-1, for all T steps
  float hreg[NT][4], creg[NT][4];
#pragma unroll
  for (int ti = 0; ti < NT; ++ti) {
    const int ht = wave + ti * LSTM_WAVES, j = ht * 16 + i16;
#pragma unroll
    for (int ks = 0; ks < KR; ++ks)
#pragma unroll
      for (int g = 0; g < 4; ++g)   // a fragment no MFMA uses (tile or K-step outside H) reads fragment 0: in bounds, unused
        wr[ti][ks][g] = wg[ht * 16 < Hp && ks < KS ? ((ht * KS + ks) * 4 + g) * 64 + lane : lane];
    if (REST == 1 && ht * 16 < Hp) {
      const int kr = ti == 0 ? KR : KR1;
      const int lo = ti == 0 ? ht * rest0 - kr : LSTM_WAVES * rest0 + (ht - LSTM_WAVES) * rest1 - kr;   // + ks: LDS K-step slot
      for (int ks = kr; ks < KS; ++ks)
#pragma unroll
        for (int g = 0; g < 4; ++g) wl[((lo + ks) * 4 + g) * 64 + lane] = wg[((ht * KS + ks) * 4 + g) * 64 + lane];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int b = b0 + g4 * 4 + r;
      const bool ok = j < H && b < B;
      hreg[ti][r] = ok && p.h0 ? p.h0[(size_t)b * H + j] : 0.f;
      creg[ti][r] = ok && p.c0 ? p.c0[(size_t)b * H + j] : 0.f;
    }
  }
  __syncthreads();
  const int tmax = VL ? slice_tmax(len) : T;   // executed steps: uniform over the workgroup
  if (VL) {   // steps tmax .. T-1 of the slice: y = 0 and a finite hprev
    const int nb = B - b0 < LSTM_ROWS ? B - b0 : LSTM_ROWS;
    for (int e = tid; e < (T - tmax) * nb * H; e += LSTM_THREADS) {
      const int tt = tmax + e / (nb * H), q = e % (nb * H), b = b0 + q / H, j = q % H;
      const size_t row = seq_row(b, tt, B, T, a.batch_first);
      p.out[row * a.ldo + j] = 0.f;
      if (a.save) p.hprev[row * H + j] = 0.f;
    }
  }

  const int G4 = 4 * H;
  for (int s = 0; s < tmax; ++s) {
    const int t = p.reverse ? tmax - 1 - s : s;
    const bf16_t* hc = hb + (s & 1) * LSTM_ROWS * HB;
    bf16_t* hx = hb + ((s + 1) & 1) * LSTM_ROWS * HB;
#pragma unroll
    for (int ti = 0; ti < NT; ++ti) {
      const int ht = wave + ti * LSTM_WAVES;
      if (ht * 16 < Hp) {   // uniform over the wave; no barrier inside
        int j = ht * 16 + i16;
        asm volatile("" : "+v"(j));   // addresses are formed anew each step: hoisted out of the time loop, every tile's
                                      // and row's pointers would take the registers the weights live in
        const bool jok = j < H;
        unsigned row[4];   // B T max(4H, In) < 2^31 (check_desc): every element offset below fits 32 bits
        bool rok[4];
        float xg[4][4];   // P_t + b_hh
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int b = b0 + g4 * 4 + r;
          rok[r] = jok && b < B;
          row[r] = (unsigned)seq_row(b < B ? b : B - 1, t, B, T, a.batch_first);
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const float bh = jok ? p.b_hh[g * H + j] : 0.f;
#pragma unroll
          for (int r = 0; r < 4; ++r) xg[g][r] = (rok[r] ? p.gates[row[r] * G4 + g * H + j] : 0.f) + bh;
        }
        f32x4 acc[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
        const bf16_t* ha = hc + i16 * HB + 8 * g4;
        const int kr = ti == 0 ? KR : KR1;
        const int lo = ti == 0 ? ht * rest0 - kr : LSTM_WAVES * rest0 + (ht - LSTM_WAVES) * rest1 - kr;
#pragma unroll
        for (int ks = 0; ks < (ti == 0 ? KR : KR1); ++ks)
          if (ks < KS) {
            const u32x4 av = *reinterpret_cast<const u32x4*>(ha + ks * 32);
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[g] = mfma_bf16(av, wr[ti][ks][g], acc[g]);
          }
        if (REST != 0)
          for (int ks = kr; ks < KS; ++ks) {
            const u32x4 av = *reinterpret_cast<const u32x4*>(ha + ks * 32);
            const u32x4* wp = REST == 1 ? wl + ((lo + ks) * 4) * 64 + lane : wg + ((ht * KS + ks) * 4) * 64 + lane;
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[g] = mfma_bf16(av, wp[g * 64], acc[g]);
          }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int bl = g4 * 4 + r;
          const float ig = sigmoidf_(acc[0][r] + xg[0][r]);
          const float fg = sigmoidf_(acc[1][r] + xg[1][r]);
          const float gg = tanhf(acc[2][r] + xg[2][r]);
          const float og = sigmoidf_(acc[3][r] + xg[3][r]);
          const float hp = hreg[ti][r];
          if (VL && t >= len[bl]) {   // the length from LDS each step: four fewer registers held across the loop   // dead row: hold h and c, y = 0; the held h is the finite hprev the dW_hh GEMM reads
            hx[bl * HB + j] = f2bf(hp);
            if (rok[r]) {
              p.out[row[r] * a.ldo + j] = 0.f;
              if (a.save) p.hprev[row[r] * H + j] = hp;
            }
            continue;
          }
          // spelled out, as in lstm_seq_bwd_kernel: the VL and the fixed instantiation must not differ in what they fuse
          const float c = __builtin_fmaf(fg, creg[ti][r], ig * gg);
          const float h = og * tanhf(c);
          creg[ti][r] = jok ? c : 0.f;
          hreg[ti][r] = jok ? h : 0.f;
          hx[bl * HB + j] = jok ? f2bf(h) : (bf16_t)0;   // columns H .. Hp stay zero: reduction padding of the next step
          if (rok[r]) {
            p.out[row[r] * a.ldo + j] = h;
            if (a.save) {
              float* gp = p.gates + row[r] * G4 + j;
              gp[0] = ig; gp[H] = fg; gp[2 * H] = gg; gp[3 * H] = og;
              p.csave[row[r] * H + j] = c;
              p.hprev[row[r] * H + j] = hp;
            }
          }
        }
      }
    }
    __syncthreads();
  }

#pragma unroll
  for (int ti = 0; ti < NT; ++ti) {
    const int j = (wave + ti * LSTM_WAVES) * 16 + i16;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int b = b0 + g4 * 4 + r;
      if (j < H && b < B) {
        if (p.hn) p.hn[(size_t)b * H + j] = hreg[ti][r];
        if (p.cn) p.cn[(size_t)b * H + j] = creg[ti][r];
      }
    }
  }
}

template <int NT, int KR, int REST, bool VL>
__global__ __launch_bounds__(LSTM_THREADS) void lstm_seq_bwd_bf16_kernel(LstmBwdArgs a) {
  extern __shared__ float lstm_lds[];
  const LstmBwdDir& p = a.d[blockIdx.y];
  const int H = a.H, Hp = (H + 15) & ~15, KS = Hp >> 3, GB = 4 * Hp + 8, B = a.B, T = a.T;   // 4 Hp = 32 KS exactly
  const int rest = KS > KR ? KS - KR : 0;
  bf16_t* dgs = reinterpret_cast<bf16_t*>(lstm_lds);          // [16][GB]: bf(gate gradients) of the step, gate g at g Hp
  int* len = reinterpret_cast<int*>(dgs + LSTM_ROWS * GB);    // [16]
  u32x4* wl = reinterpret_cast<u32x4*>(len + LSTM_ROWS);      // REST == 1: [tile][rest][64] B fragments
  const u32x4* wg = a.w_pack[blockIdx.y];                     // all of bf(W_hh)^T as B fragments
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i16 = lane & 15, g4 = lane >> 4;
  const int b0 = blockIdx.x * LSTM_ROWS;

  for (int e = tid; e < LSTM_ROWS * GB; e += LSTM_THREADS) dgs[e] = 0;
  if (VL) load_slice_lengths(len, a.lengths, b0, B, T);
  u32x4 wr[NT][KR];   // this wave's tiles of dh, K-steps 0 .. KR-1, for all T steps
  float dhreg[NT][4], dcreg[NT][4];
#pragma unroll
  for (int ti = 0; ti < NT; ++ti) {
    const int kt = wave + ti * LSTM_WAVES, k = kt * 16 + i16;
#pragma unroll
    for (int ks = 0; ks < KR; ++ks) wr[ti][ks] = wg[kt * 16 < Hp && ks < KS ? (kt * KS + ks) * 64 + lane : lane];
    if (REST == 1 && kt * 16 < Hp)
      for (int ks = KR; ks < KS; ++ks) wl[(kt * rest + ks - KR) * 64 + lane] = wg[(kt * KS + ks) * 64 + lane];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int b = b0 + g4 * 4 + r;
      const bool ok = k < H && b < B;
      dhreg[ti][r] = ok && p.dhn ? p.dhn[(size_t)b * H + k] : 0.f;
      dcreg[ti][r] = ok && p.dcn ? p.dcn[(size_t)b * H + k] : 0.f;
    }
  }
  __syncthreads();
  const int tmax = VL ? slice_tmax(len) : T;   // the steps the forward executed: uniform over the workgroup
  int lr[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) lr[r] = VL ? len[g4 * 4 + r] : T;

  const int G4 = 4 * H;
  if (VL) {   // steps tmax .. T-1 of the slice: the GEMMs after this kernel read all B T rows of dgates
    const int nb = B - b0 < LSTM_ROWS ? B - b0 : LSTM_ROWS;
    for (int e = tid; e < (T - tmax) * nb * G4; e += LSTM_THREADS) {
      const int tt = tmax + e / (nb * G4), q = e % (nb * G4), b = b0 + q / G4, n = q % G4;
      p.dgates[seq_row(b, tt, B, T, a.batch_first) * G4 + n] = 0.f;
    }
  }
  for (int s = 0; s < tmax; ++s) {
    const int t = p.reverse ? s : tmax - 1 - s;       // the forward walk, backwards
    const bool first = s == tmax - 1;                 // (fixed lengths) the forward's first step: c_{t-1} = c0
    const int tp = p.reverse ? t + 1 : t - 1;
#pragma unroll
    for (int ti = 0; ti < NT; ++ti) {
      const int ht = wave + ti * LSTM_WAVES;
      if (ht * 16 < Hp) {
        int j = ht * 16 + i16;
        asm volatile("" : "+v"(j));   // as in the forward: no per-tile pointers kept across steps
        const bool jok = j < H;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int bl = g4 * 4 + r, b = b0 + bl;
          float di = 0.f, df = 0.f, dg = 0.f, dop = 0.f, dcp = 0.f;
          const bool live = !VL || t < lr[r];   // a dead row runs the same arithmetic and drops it (see lstm_seq_bwd_kernel)
          if (jok && b < B) {
            // the lane-local cell block of lstm_seq_bwd_kernel, contraction pinned the same way
#pragma clang fp contract(off)
            const size_t row = seq_row(b, t, B, T, a.batch_first);
            const float* gp = p.gates + row * G4 + j;
            const float ig = gp[0], fg = gp[H], gg = gp[2 * H], og = gp[3 * H];
            const float c = p.csave[row * H + j];
            const bool rfirst = VL ? (!live || (p.reverse ? t == lr[r] - 1 : t == 0)) : first;
            const float cp = rfirst ? (p.c0 ? p.c0[(size_t)b * H + j] : 0.f)
                                    : p.csave[seq_row(b, tp, B, T, a.batch_first) * H + j];
            const float dh = (p.dy ? p.dy[row * a.ldo + j] : 0.f) + dhreg[ti][r];
            const float tc = tanhf(c);
            const float dc = __builtin_fmaf(dh * og, __builtin_fmaf(-tc, tc, 1.f), dcreg[ti][r]);
            dop = dh * tc * og * (1.f - og);
            di = dc * gg * ig * (1.f - ig);
            df = dc * cp * fg * (1.f - fg);
            dg = dc * ig * (1.f - gg * gg);
            dcp = dc * fg;
            if (VL) {   // dead row: exact-zero gate gradients, the dc carry kept (dh: below); dy there is not used
              di = live ? di : 0.f; df = live ? df : 0.f; dg = live ? dg : 0.f; dop = live ? dop : 0.f;
              dcp = live ? dcp : dcreg[ti][r];
            }
            float* dq = p.dgates + row * G4 + j;
            dq[0] = di; dq[H] = df; dq[2 * H] = dg; dq[3 * H] = dop;   // the unrounded gradients
          }
          dcreg[ti][r] = dcp;
          bf16_t* ds = dgs + bl * GB + j;
          ds[0] = f2bf(di); ds[Hp] = f2bf(df); ds[2 * Hp] = f2bf(dg); ds[3 * Hp] = f2bf(dop);
        }
      }
    }
    __syncthreads();
    // dh_{t-1}[b][k] = sum_n bf(dgates[b][n]) bf(W_hh[n][k]): this wave's tiles of k, the same tiles it owns above
#pragma unroll
    for (int ti = 0; ti < NT; ++ti) {
      const int kt = wave + ti * LSTM_WAVES;
      if (kt * 16 < Hp) {
        f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};   // even and odd K-steps
        const bf16_t* da = dgs + i16 * GB + 8 * g4;
#pragma unroll
        for (int ks = 0; ks < KR; ++ks)
          if (ks < KS) acc[ks & 1] = mfma_bf16(*reinterpret_cast<const u32x4*>(da + ks * 32), wr[ti][ks], acc[ks & 1]);
        if (REST != 0) {
          static_assert(KR % 2 == 0, "even and odd K-steps keep their accumulators");
          const u32x4* wp = REST == 1 ? wl + (kt * rest - KR) * 64 + lane : wg + (kt * KS) * 64 + lane;
          for (int ks = KR; ks < KS; ks += 2) {   // KS is even
            acc[0] = mfma_bf16(*reinterpret_cast<const u32x4*>(da + ks * 32), wp[ks * 64], acc[0]);
            acc[1] = mfma_bf16(*reinterpret_cast<const u32x4*>(da + ks * 32 + 32), wp[ks * 64 + 64], acc[1]);
          }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (!VL || t < lr[r]) dhreg[ti][r] = acc[0][r] + acc[1][r];   // a dead row keeps its dh carry
      }
    }
    __syncthreads();
  }

#pragma unroll
  for (int ti = 0; ti < NT; ++ti) {
    const int k = (wave + ti * LSTM_WAVES) * 16 + i16;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int b = b0 + g4 * 4 + r;
      if (k < H && b < B) {
        if (p.dh0) p.dh0[(size_t)b * H + k] = dhreg[ti][r];
        if (p.dc0) p.dc0[(size_t)b * H + k] = dcreg[ti][r];
      }
    }
  }
}

// out[b][c] = sum_{t < len_b} x[b][t][c] / len_b, t in order; one thread per (b, c), consecutive c in a wave
__global__ __launch_bounds__(256) void seq_mean_varlen_fwd_kernel(const float* __restrict__ x, const int* __restrict__ lengths,
                                                                  float* __restrict__ out, int T, int C) {
  const int b = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  int l = lengths[b];
  l = l < 0 ? 0 : (l > T ? T : l);
  const float* xp = x + (size_t)b * T * C + c;
  float acc = 0.f;
  for (int t = 0; t < l; ++t) acc += xp[(size_t)t * C];
  out[(size_t)b * C + c] = l > 0 ? acc / (float)l : 0.f;
}
// dx[b][t][c] = t < len_b ? dy[b][c] / len_b : 0
__global__ __launch_bounds__(256) void seq_mean_varlen_bwd_kernel(const float* __restrict__ dy, const int* __restrict__ lengths,
                                                                  float* __restrict__ dx, int T, int C) {
  const int b = blockIdx.z, t = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  int l = lengths[b];
  l = l < 0 ? 0 : (l > T ? T : l);
  dx[((size_t)b * T + t) * C + c] = t < l ? dy[(size_t)b * C + c] / (float)l : 0.f;
}

// vl: + the slice's 16 lengths behind the float arrays (148 288 B in the backward at H = 384)
inline size_t fwd_lds(int H, bool vl = false) {
  const int Hp = (H + 15) & ~15;
  return (size_t)3 * LSTM_ROWS * (Hp + 4) * sizeof(float) + (vl ? LSTM_ROWS * sizeof(int) : 0);
}
inline size_t bwd_lds(int H, bool vl = false) {
  const int Hp = (H + 15) & ~15;
  return (size_t)LSTM_ROWS * ((4 * Hp + 4) + 2 * (Hp + 4)) * sizeof(float) + (vl ? LSTM_ROWS * sizeof(int) : 0);
}

int check_desc(const ecgmm_lstm_desc* d, const char* what) {
  if (!d) ECG_FAIL(ECGMM_ERR_SHAPE, "%s: null descriptor", what);
  if (d->B < 1 || d->T < 1 || d->In < 1 || d->H < 1)
    ECG_FAIL(ECGMM_ERR_SHAPE, "%s: B=%d T=%d In=%d H=%d must all be >= 1", what, d->B, d->T, d->In, d->H);
  if (d->H > LSTM_MAX_H)
    ECG_FAIL(ECGMM_ERR_SHAPE, "%s: hidden size H=%d above the cap of %d (LDS budget of the recurrence kernels)", what, d->H,
             LSTM_MAX_H);
  if (d->layers < 1 || d->layers > LSTM_MAX_LAYERS)
    ECG_FAIL(ECGMM_ERR_SHAPE, "%s: layers=%d outside 1..%d", what, d->layers, LSTM_MAX_LAYERS);
  if ((d->bidirectional | d->batch_first | d->save_for_backward) & ~1)
    ECG_FAIL(ECGMM_ERR_SHAPE, "%s: bidirectional / batch_first / save_for_backward must be 0 or 1", what);
  const int D = d->bidirectional ? 2 : 1;
  const int wide = d->In > D * d->H ? d->In : D * d->H;
  if ((double)d->B * d->T * (4.0 * d->H > wide ? 4.0 * d->H : wide) >= 2147483648.0)
    ECG_FAIL(ECGMM_ERR_SHAPE, "%s: B*T*max(4H, In)=%.0f does not fit 31 bits", what, (double)d->B * d->T * 4.0 * d->H);
  return 0;
}

struct FwdLayout {
  float* gates[LSTM_MAX_LAYERS][2];
  float* csave[LSTM_MAX_LAYERS][2];
  float* hprev[LSTM_MAX_LAYERS][2];
  float* out[LSTM_MAX_LAYERS];   // outputs of layers 0 .. L-2 (the last layer writes y)
  u32x4* wpack[LSTM_MAX_LAYERS][2];   // bf16 only: W_hh as B fragments, behind everything else
  size_t wpack_each;
  size_t bytes;
};

// ---- bf16 instantiations per range of H ------------------------------------------------------------------------------------
// NT tiles per wave, KR K-steps of each tile in registers, REST: where the other K-steps are (0 none, 1 LDS, 2 streamed copy).
struct Bf16Cfg { int nt, kr, rest; size_t lds, pack_bytes; };
Bf16Cfg bf16_fwd_cfg(int H) {
  const int Hp = (H + 15) & ~15, tiles = Hp >> 4, KS = (Hp + 31) >> 5;
  Bf16Cfg c;
  int kr1;   // as the kernel's KR1
  if (tiles <= 8) { c = {1, 4, 0, 0, 0}; kr1 = 4; }            // H <= 128: KS <= 4, all of W_hh in registers
  else if (tiles <= 13) { c = {2, 5, 1, 0, 0}; kr1 = 4; }      // H <= 208: K-steps 5, 6 (tiles 8 ..: 4, 5, 6) in LDS, 124 KiB at 13
  else if (tiles <= 16) { c = {2, 5, 2, 0, 0}; kr1 = 4; }      // H <= 256
  else { c = {3, 3, 2, 0, 0}; kr1 = 2; }                       // H <= 384
  const int rest0 = KS > c.kr ? KS - c.kr : 0, rest1 = KS > kr1 ? KS - kr1 : 0;
  const int slots = tiles <= LSTM_WAVES ? tiles * rest0 : LSTM_WAVES * rest0 + (tiles - LSTM_WAVES) * rest1;
  c.lds = (size_t)2 * LSTM_ROWS * (KS * 32 + 8) * sizeof(bf16_t) + LSTM_ROWS * sizeof(int) +
          (c.rest == 1 ? (size_t)slots * 4 * 64 * sizeof(u32x4) : 0);
  c.pack_bytes = (size_t)tiles * KS * 4 * 64 * sizeof(u32x4);
  return c;
}
Bf16Cfg bf16_bwd_cfg(int H) {
  const int Hp = (H + 15) & ~15, tiles = Hp >> 4, KS = Hp >> 3;
  Bf16Cfg c;
  if (tiles <= 8) c = {1, 16, 0, 0, 0};           // H <= 128: KS <= 16
  else if (tiles <= 13) c = {2, 16, 1, 0, 0};     // H <= 208: K-steps 16 .. 25 in LDS (130 KiB at 13 tiles)
  else if (tiles <= 16) c = {2, 16, 2, 0, 0};
  else c = {3, 10, 2, 0, 0};
  const int rest = KS > c.kr ? KS - c.kr : 0;
  c.lds = (size_t)LSTM_ROWS * (4 * Hp + 8) * sizeof(bf16_t) + LSTM_ROWS * sizeof(int) +
          (c.rest == 1 ? (size_t)tiles * rest * 64 * sizeof(u32x4) : 0);
  c.pack_bytes = (size_t)tiles * KS * 64 * sizeof(u32x4);
  return c;
}
int check_dtype(int dtype, const char* what) {
  if (dtype != ECGMM_F32 && dtype != ECGMM_BF16)
    ECG_FAIL(ECGMM_ERR_SHAPE, "%s: compute dtype %d is neither ECGMM_F32 nor ECGMM_BF16", what, dtype);
  return 0;
}

FwdLayout fwd_layout(const ecgmm_lstm_desc* d, void* ws, int dtype = ECGMM_F32) {
  FwdLayout f;
  memset(&f, 0, sizeof(f));
  Arena ar(ws);
  const int D = d->bidirectional ? 2 : 1, L = d->layers;
  const size_t BT = (size_t)d->B * d->T, H = d->H;
  if (d->save_for_backward) {
    for (int l = 0; l < L; ++l) {
      for (int k = 0; k < D; ++k) {
        f.gates[l][k] = ar.take<float>(BT * 4 * H);
        f.csave[l][k] = ar.take<float>(BT * H);
        f.hprev[l][k] = ar.take<float>(BT * H);
      }
      if (l < L - 1) f.out[l] = ar.take<float>(BT * D * H);
    }
  } else {   // one projection buffer per direction and two layer outputs in turn
    float* xg[2] = {nullptr, nullptr};
    for (int k = 0; k < D; ++k) xg[k] = ar.take<float>(BT * 4 * H);
    float* pp[2] = {nullptr, nullptr};
    if (L > 1) { pp[0] = ar.take<float>(BT * D * H); pp[1] = ar.take<float>(BT * D * H); }
    for (int l = 0; l < L; ++l) {
      for (int k = 0; k < D; ++k) f.gates[l][k] = xg[k];
      if (l < L - 1) f.out[l] = pp[l & 1];
    }
  }
  if (dtype == ECGMM_BF16 && bf16_fwd_cfg(d->H).pack_bytes) {
    f.wpack_each = bf16_fwd_cfg(d->H).pack_bytes;
    for (int l = 0; l < L; ++l)
      for (int k = 0; k < D; ++k) f.wpack[l][k] = static_cast<u32x4*>(ar.take_bytes(f.wpack_each));
  }
  f.bytes = align_up(ar.off, 256);
  return f;
}

struct BwdLayout {
  float* dgates[2];
  float* dyb[2];
  float* dxtmp;
  void* lin;
  u32x4* wpack[LSTM_MAX_LAYERS][2];   // bf16 only: W_hh^T as B fragments, behind everything else
  size_t wpack_each;
  size_t lin_bytes, bytes;
};
BwdLayout bwd_layout(const ecgmm_lstm_desc* d, void* scratch, int dtype = ECGMM_F32) {
  BwdLayout b;
  memset(&b, 0, sizeof(b));
  Arena ar(scratch);
  const int D = d->bidirectional ? 2 : 1, L = d->layers, H = d->H;
  const size_t BT = (size_t)d->B * d->T;
  const int rows = (int)BT;
  for (int k = 0; k < D; ++k) b.dgates[k] = ar.take<float>(BT * 4 * H);
  if (L > 1) { b.dyb[0] = ar.take<float>(BT * D * H); b.dyb[1] = ar.take<float>(BT * D * H); }
  const size_t wide = (size_t)(d->In > D * H ? d->In : D * H);
  if (D == 2) b.dxtmp = ar.take<float>(BT * wide);
  size_t lin = ecg_linear_bwd_scratch(rows, d->In, 4 * H);
  if (L > 1 && ecg_linear_bwd_scratch(rows, D * H, 4 * H) > lin) lin = ecg_linear_bwd_scratch(rows, D * H, 4 * H);
  if (ecg_linear_bwd_scratch(rows, H, 4 * H) > lin) lin = ecg_linear_bwd_scratch(rows, H, 4 * H);
  b.lin_bytes = lin;
  b.lin = ar.take_bytes(lin);
  if (dtype == ECGMM_BF16 && bf16_bwd_cfg(H).pack_bytes) {
    b.wpack_each = bf16_bwd_cfg(H).pack_bytes;
    for (int l = 0; l < L; ++l)
      for (int k = 0; k < D; ++k) b.wpack[l][k] = static_cast<u32x4*>(ar.take_bytes(b.wpack_each));
  }
  b.bytes = align_up(ar.off, 256);
  return b;
}

bool lds_attr_done = false;
void set_lds_attrs() {
  if (lds_attr_done) return;
  const void* fns[] = {(const void*)lstm_seq_fwd_kernel<true, false>, (const void*)lstm_seq_fwd_kernel<false, false>,
                       (const void*)lstm_seq_fwd_kernel<true, true>,  (const void*)lstm_seq_fwd_kernel<false, true>,
                       (const void*)lstm_seq_bwd_kernel<false>,       (const void*)lstm_seq_bwd_kernel<true>};
  for (const void* fn : fns) (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  lds_attr_done = true;
}

template <typename A> using SeqKernel = void (*)(A);
template <typename A> void launch_seq(SeqKernel<A> kernel, dim3 grid, size_t lds, hipStream_t s, const A& a) {
  // once per kernel would do; the call is a host-side table write and keeps the launchers free of state
  (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  hipLaunchKernelGGL(kernel, grid, dim3(LSTM_THREADS), lds, s, a);
}
template <bool VL> void launch_fwd_bf16(const Bf16Cfg& c, dim3 grid, hipStream_t s, const LstmFwdArgs& a) {
  if (c.nt == 1) launch_seq<LstmFwdArgs>(lstm_seq_fwd_bf16_kernel<1, 4, 4, 0, VL>, grid, c.lds, s, a);
  else if (c.nt == 2 && c.rest == 1) launch_seq<LstmFwdArgs>(lstm_seq_fwd_bf16_kernel<2, 5, 4, 1, VL>, grid, c.lds, s, a);
  else if (c.nt == 2) launch_seq<LstmFwdArgs>(lstm_seq_fwd_bf16_kernel<2, 5, 4, 2, VL>, grid, c.lds, s, a);
  else launch_seq<LstmFwdArgs>(lstm_seq_fwd_bf16_kernel<3, 3, 2, 2, VL>, grid, c.lds, s, a);
}
template <bool VL> void launch_bwd_bf16(const Bf16Cfg& c, dim3 grid, hipStream_t s, const LstmBwdArgs& a) {
  if (c.nt == 1) launch_seq<LstmBwdArgs>(lstm_seq_bwd_bf16_kernel<1, 16, 0, VL>, grid, c.lds, s, a);
  else if (c.nt == 2 && c.rest == 1) launch_seq<LstmBwdArgs>(lstm_seq_bwd_bf16_kernel<2, 16, 1, VL>, grid, c.lds, s, a);
  else if (c.nt == 2) launch_seq<LstmBwdArgs>(lstm_seq_bwd_bf16_kernel<2, 16, 2, VL>, grid, c.lds, s, a);
  else launch_seq<LstmBwdArgs>(lstm_seq_bwd_bf16_kernel<3, 10, 2, VL>, grid, c.lds, s, a);
}
// one launch per call: every layer's and direction's W_hh into its streamed bf16 copy
int pack_whh(const ecgmm_lstm_desc* d, const float* const* params, u32x4* const (*dst)[2], int transposed, hipStream_t s) {
  const int D = d->bidirectional ? 2 : 1, L = d->layers;
  LstmPackArgs pa;
  memset(&pa, 0, sizeof(pa));
  pa.H = d->H; pa.transposed = transposed;
  for (int l = 0; l < L; ++l)
    for (int k = 0; k < D; ++k) {
      pa.w[l * D + k] = params[(size_t)(l * D + k) * 4 + 1];
      pa.dst[l * D + k] = dst[l][k];
      if (!pa.w[l * D + k]) ECG_FAIL(ECGMM_ERR_SHAPE, "lstm: null W_hh (layer %d)", l);
    }
  hipLaunchKernelGGL(pack_whh_bf16_kernel, dim3(64, L * D), dim3(256), 0, s, pa);
  ECG_CHECK_LAUNCH("pack_whh_bf16");
  return 0;
}

}  // namespace

size_t ecg_lstm_fwd_workspace(const ecgmm_lstm_desc* d, int dtype) {
  if (check_desc(d, "lstm_fwd_workspace") != 0 || check_dtype(dtype, "lstm_fwd_workspace") != 0) return 0;
  return fwd_layout(d, nullptr, dtype).bytes;
}
size_t ecg_lstm_bwd_workspace(const ecgmm_lstm_desc* d, int dtype) {
  if (check_desc(d, "lstm_bwd_workspace") != 0 || check_dtype(dtype, "lstm_bwd_workspace") != 0) return 0;
  return bwd_layout(d, nullptr, dtype).bytes;
}

int ecg_lstm_ws_view(const ecgmm_lstm_desc* d, int dtype, const char* which, int layer, int direction, size_t* offset,
                     size_t* bytes) {
  ECG_TRY(check_desc(d, "lstm_ws_view"));
  ECG_TRY(check_dtype(dtype, "lstm_ws_view"));
  const int D = d->bidirectional ? 2 : 1;
  if (!which || !offset || !bytes) ECG_FAIL(ECGMM_ERR_SHAPE, "lstm_ws_view: null argument");
  if (layer < 0 || layer >= d->layers || direction < 0 || direction >= D)
    ECG_FAIL(ECGMM_ERR_SHAPE, "lstm_ws_view: layer %d / direction %d outside %d x %d", layer, direction, d->layers, D);
  const size_t BT = (size_t)d->B * d->T, H = d->H;
  // the layouts over a base that is never dereferenced (over a null base the arena hands out null pointers)
  unsigned char* const base = reinterpret_cast<unsigned char*>((uintptr_t)1 << 20);
  const FwdLayout f = fwd_layout(d, base, dtype);
  const BwdLayout w = bwd_layout(d, base, dtype);
  const void* at = nullptr;
  bool found = true;
  if (!strcmp(which, "dgates")) { at = w.dgates[direction]; *bytes = BT * 4 * H * sizeof(float); }
  else if (!d->save_for_backward) ECG_FAIL(ECGMM_ERR_SHAPE, "lstm_ws_view: %s is kept only with save_for_backward = 1", which);
  else if (!strcmp(which, "gates")) { at = f.gates[layer][direction]; *bytes = BT * 4 * H * sizeof(float); }
  else if (!strcmp(which, "c")) { at = f.csave[layer][direction]; *bytes = BT * H * sizeof(float); }
  else if (!strcmp(which, "hprev")) { at = f.hprev[layer][direction]; *bytes = BT * H * sizeof(float); }
  else if (!strcmp(which, "out")) {
    if (layer == d->layers - 1) ECG_FAIL(ECGMM_ERR_SHAPE, "lstm_ws_view: the last layer's output is y, not in the workspace");
    at = f.out[layer]; *bytes = BT * D * H * sizeof(float);   // both directions side by side
  } else found = false;
  if (!found) ECG_FAIL(ECGMM_ERR_SHAPE, "lstm_ws_view: unknown view '%s' (gates, c, hprev, out, dgates)", which);
  *offset = (size_t)(static_cast<const unsigned char*>(at) - base);
  return 0;
}

int ecg_lstm_forward(const ecgmm_lstm_desc* d, int dtype, const float* x, const int* lengths, const float* const* params,
                     const float* h0, const float* c0, float* y, float* hn, float* cn, void* ws, size_t ws_bytes,
                     hipStream_t s) {
  ECG_TRY(check_desc(d, "lstm_forward"));
  ECG_TRY(check_dtype(dtype, "lstm_forward"));
  if (!x || !params || !y) ECG_FAIL(ECGMM_ERR_SHAPE, "lstm_forward: x, params and y must not be null");
  const FwdLayout f = fwd_layout(d, ws, dtype);
  if (!ws || ws_bytes < f.bytes)
    ECG_FAIL(ECGMM_ERR_WORKSPACE, "lstm_forward: workspace %zu bytes, need %zu", ws_bytes, f.bytes);
  const int D = d->bidirectional ? 2 : 1, L = d->layers, H = d->H, B = d->B, T = d->T;
  const int rows = B * T;
  const size_t BH = (size_t)B * H;
  set_lds_attrs();
  const Bf16Cfg bc = bf16_fwd_cfg(H);
  if (dtype == ECGMM_BF16 && bc.pack_bytes) ECG_TRY(pack_whh(d, params, f.wpack, 0, s));
  for (int l = 0; l < L; ++l) {
    const float* in = l == 0 ? x : f.out[l - 1];
    const int In = l == 0 ? d->In : D * H;
    float* dst = l == L - 1 ? y : f.out[l];
    LstmFwdArgs a;
    memset(&a, 0, sizeof(a));
    a.B = B; a.T = T; a.H = H; a.ldo = D * H; a.batch_first = d->batch_first; a.save = d->save_for_backward;
    a.lengths = lengths;
    bool v4 = H % 4 == 0;
    for (int k = 0; k < D; ++k) {
      const float* const* pr = params + (size_t)(l * D + k) * 4;   // w_ih, w_hh, b_ih, b_hh
      if (!pr[0] || !pr[1] || !pr[2] || !pr[3]) ECG_FAIL(ECGMM_ERR_SHAPE, "lstm_forward: null parameter (layer %d)", l);
      ECG_TRY(ecg_linear_fwd(in, pr[0], pr[2], f.gates[l][k], rows, In, 4 * H, ECGMM_ACT_NONE, nullptr, s));
      LstmFwdDir& q = a.d[k];
      q.gates = f.gates[l][k]; q.w_hh = pr[1]; q.b_hh = pr[3];
      q.h0 = h0 ? h0 + (size_t)(l * D + k) * BH : nullptr;
      q.c0 = c0 ? c0 + (size_t)(l * D + k) * BH : nullptr;
      q.out = dst + (size_t)k * H;
      q.hprev = f.hprev[l][k]; q.csave = f.csave[l][k];
      q.hn = hn ? hn + (size_t)(l * D + k) * BH : nullptr;
      q.cn = cn ? cn + (size_t)(l * D + k) * BH : nullptr;
      q.reverse = k;
      a.w_pack[k] = f.wpack[l][k];
      v4 = v4 && ((uintptr_t)pr[1] & 15) == 0;
    }
    const dim3 grid(ceil_div(B, LSTM_ROWS), D);
    if (dtype == ECGMM_BF16) {
      if (lengths) launch_fwd_bf16<true>(bc, grid, s, a);
      else launch_fwd_bf16<false>(bc, grid, s, a);
      ECG_CHECK_LAUNCH("lstm_seq_fwd_bf16");
      continue;
    }
    // 2 (4H x H) FLOPs per batch row and step; W_hh once per step and slice from L2 (not HBM: 0 algorithmic bytes beyond
    // the projections, the saved tensors and the output)
    if (lengths) {
      if (v4) hipLaunchKernelGGL((lstm_seq_fwd_kernel<true, true>), grid, dim3(LSTM_THREADS), fwd_lds(H, true), s, a);
      else hipLaunchKernelGGL((lstm_seq_fwd_kernel<false, true>), grid, dim3(LSTM_THREADS), fwd_lds(H, true), s, a);
    } else if (v4) hipLaunchKernelGGL((lstm_seq_fwd_kernel<true, false>), grid, dim3(LSTM_THREADS), fwd_lds(H), s, a);
    else hipLaunchKernelGGL((lstm_seq_fwd_kernel<false, false>), grid, dim3(LSTM_THREADS), fwd_lds(H), s, a);
    ECG_CHECK_LAUNCH("lstm_seq_fwd");
  }
  return 0;
}

int ecg_lstm_backward(const ecgmm_lstm_desc* d, int dtype, const float* x, const int* lengths, const float* const* params,
                      const float* h0, const float* c0, const float* dy, const float* dhn, const float* dcn, const void* ws,
                      float* dx, float* const* grads, float* dh0, float* dc0, void* scratch, size_t scratch_bytes,
                      hipStream_t s) {
  ECG_TRY(check_desc(d, "lstm_backward"));
  ECG_TRY(check_dtype(dtype, "lstm_backward"));
  if (!d->save_for_backward) ECG_FAIL(ECGMM_ERR_SHAPE, "lstm_backward: the forward ran with save_for_backward = 0");
  if (!x || !params || !ws) ECG_FAIL(ECGMM_ERR_SHAPE, "lstm_backward: x, params and the forward workspace must not be null");
  const FwdLayout f = fwd_layout(d, const_cast<void*>(ws), dtype);   // read only
  const BwdLayout w = bwd_layout(d, scratch, dtype);
  if (!scratch || scratch_bytes < w.bytes)
    ECG_FAIL(ECGMM_ERR_WORKSPACE, "lstm_backward: scratch %zu bytes, need %zu", scratch_bytes, w.bytes);
  const int D = d->bidirectional ? 2 : 1, L = d->layers, H = d->H, B = d->B, T = d->T;
  const int rows = B * T;
  const size_t BH = (size_t)B * H;
  (void)h0;   // h_{t-1} of every step, h0 included, is in the forward workspace
  set_lds_attrs();
  const Bf16Cfg bc = bf16_bwd_cfg(H);
  if (dtype == ECGMM_BF16 && bc.pack_bytes) ECG_TRY(pack_whh(d, params, w.wpack, 1, s));
  for (int l = L - 1; l >= 0; --l) {
    const float* in = l == 0 ? x : f.out[l - 1];
    const int In = l == 0 ? d->In : D * H;
    const float* dyl = l == L - 1 ? dy : w.dyb[(l + 1) & 1];
    LstmBwdArgs a;
    memset(&a, 0, sizeof(a));
    a.B = B; a.T = T; a.H = H; a.ldo = D * H; a.batch_first = d->batch_first;
    a.lengths = lengths;
    for (int k = 0; k < D; ++k) {
      const float* const* pr = params + (size_t)(l * D + k) * 4;
      if (!pr[0] || !pr[1]) ECG_FAIL(ECGMM_ERR_SHAPE, "lstm_backward: null weight (layer %d)", l);
      LstmBwdDir& q = a.d[k];
      q.gates = f.gates[l][k]; q.csave = f.csave[l][k];
      q.c0 = c0 ? c0 + (size_t)(l * D + k) * BH : nullptr;
      q.w_hh = pr[1];
      q.dy = dyl ? dyl + (size_t)k * H : nullptr;
      q.dhn = dhn ? dhn + (size_t)(l * D + k) * BH : nullptr;
      q.dcn = dcn ? dcn + (size_t)(l * D + k) * BH : nullptr;
      q.dgates = w.dgates[k];
      q.dh0 = dh0 ? dh0 + (size_t)(l * D + k) * BH : nullptr;
      q.dc0 = dc0 ? dc0 + (size_t)(l * D + k) * BH : nullptr;
      q.reverse = k;
      a.w_pack[k] = w.wpack[l][k];
    }
    const dim3 grid(ceil_div(B, LSTM_ROWS), D);
    if (dtype == ECGMM_BF16) {
      if (lengths) launch_bwd_bf16<true>(bc, grid, s, a);
      else launch_bwd_bf16<false>(bc, grid, s, a);
    } else if (lengths) hipLaunchKernelGGL(lstm_seq_bwd_kernel<true>, grid, dim3(LSTM_THREADS), bwd_lds(H, true), s, a);
    else hipLaunchKernelGGL(lstm_seq_bwd_kernel<false>, grid, dim3(LSTM_THREADS), bwd_lds(H), s, a);
    ECG_CHECK_LAUNCH("lstm_seq_bwd");
    float* dst = l > 0 ? w.dyb[l & 1] : dx;   // dx of layer l is the dy of layer l - 1
    for (int k = 0; k < D; ++k) {
      const float* const* pr = params + (size_t)(l * D + k) * 4;
      float* const* gr = grads ? grads + (size_t)(l * D + k) * 4 : nullptr;
      float* gwi = gr ? gr[0] : nullptr; float* gwh = gr ? gr[1] : nullptr;
      float* gbi = gr ? gr[2] : nullptr; float* gbh = gr ? gr[3] : nullptr;
      float* dxk = dst ? (k == 0 ? dst : w.dxtmp) : nullptr;
      // b_ih's gradient is, like b_hh's, the column sum of dgates: ecg_rows_sum for both, not ecg_linear_bwd's db, whose VALU
      // route sums in another order when dw is requested with it -- the same bits whatever else the caller asked for
      if (dxk || gwi)
        ECG_TRY(ecg_linear_bwd(w.dgates[k], in, pr[0], dxk, gwi, nullptr, rows, In, 4 * H, w.lin, w.lin_bytes, s));
      if (gbi) ECG_TRY(ecg_rows_sum(w.dgates[k], rows, 4 * H, gbi, 0, s));
      if (dxk && k == 1) ECG_TRY(ecg_axpby(1.f, w.dxtmp, 1.f, dst, (long)rows * In, s));   // forward + reverse, in that order
      if (gwh) ECG_TRY(ecg_linear_bwd(w.dgates[k], f.hprev[l][k], pr[1], nullptr, gwh, nullptr, rows, H, 4 * H, w.lin,
                                      w.lin_bytes, s));
      if (gbh) ECG_TRY(ecg_rows_sum(w.dgates[k], rows, 4 * H, gbh, 0, s));
    }
  }
  return 0;
}

int ecg_seq_mean_varlen_fwd(const float* x, const int* lengths, float* out, int B, int T, int C, hipStream_t s) {
  if (!x || !lengths || !out) ECG_FAIL(ECGMM_ERR_SHAPE, "seq_mean_varlen_fwd: x, lengths and out must not be null");
  if (B < 1 || T < 1 || C < 1 || B > 65535) ECG_FAIL(ECGMM_ERR_SHAPE, "seq_mean_varlen_fwd: B=%d (1..65535) T=%d C=%d", B, T, C);
  hipLaunchKernelGGL(seq_mean_varlen_fwd_kernel, dim3(ceil_div(C, 256), B), dim3(256), 0, s, x, lengths, out, T, C);
  ECG_CHECK_LAUNCH("seq_mean_varlen_fwd");
  return 0;
}

int ecg_seq_mean_varlen_bwd(const float* dy, const int* lengths, float* dx, int B, int T, int C, hipStream_t s) {
  if (!dy || !lengths || !dx) ECG_FAIL(ECGMM_ERR_SHAPE, "seq_mean_varlen_bwd: dy, lengths and dx must not be null");
  if (B < 1 || T < 1 || C < 1 || B > 65535 || T > 65535)
    ECG_FAIL(ECGMM_ERR_SHAPE, "seq_mean_varlen_bwd: B=%d T=%d (1..65535 each) C=%d", B, T, C);
  hipLaunchKernelGGL(seq_mean_varlen_bwd_kernel, dim3(ceil_div(C, 256), T, B), dim3(256), 0, s, dy, lengths, dx, T, C);
  ECG_CHECK_LAUNCH("seq_mean_varlen_bwd");
  return 0;
}
