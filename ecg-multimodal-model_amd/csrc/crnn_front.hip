// Kernels of the CRNN convolutional front end (train_physionet2.py:55-65, 87-93): three ConvBlocks
//   Conv2d(k = 5, pad = 2, bias) -> BatchNorm2d -> ReLU -> MaxPool2d(2)
// on a log-spectrogram [B, 1, F, T].  Activations are NHWC with H = frequency, W = time.  Forward and input gradient of
// blocks 2 and 3 are the implicit-GEMM kernel (conv_igemm.hip) at R = S = 5; what lives here is the rest:
//
//   conv5_in1_fwd_kernel    Conv2d(1, 32, 5): [B,F,T] fp32 -> [B,F,T,32] + BatchNorm partial rows.  K = 25: VALU fma, no
//                           im2col; the 25 x 32 weights sit in LDS, a thread owns one pixel x 8 channels (16 / 32 B stores,
//                           64 / 128 contiguous bytes per pixel).  Bound by writing its output.  The BatchNorm rows are
//                           summed from the fp32 accumulators, before the bf16 rounding of the stored y, as the
//                           implicit-GEMM epilogue does (conv_igemm.hip), so all three blocks follow one convention.
//   conv5_in1_wgrad_kernel  its weight + bias gradient: a workgroup walks (image row, 64-column) tiles; the 5 x 68 x patch
//                           and the 64 x 32 dy tile of a tile sit in LDS; thread (channel, slot) owns taps slot + 8k.
//   conv5_in1_dgrad_kernel  its input gradient (what spectrogram.requires_grad_() gives): column strips, a rolling window of
//                           dy rows in LDS, thread = pixel x 8 channels, VALU fma (the GEMM has N = 1), fp32 out
//   conv5_wgrad_kernel      weight gradient of a 5x5 pad-2 stride-1 convolution, Cin and Cout multiples of 32.  GEMM view
//                           per tap: dw[co][ci] = sum_pixels dy[p][co] x[p + tap][ci]; pixels are the MFMA K index.  A
//                           workgroup owns a 32 x 32 (co, ci) tile of ALL 25 taps and walks bands of 32 pixels of one
//                           output row: the dy band [32][32] and the five x rows the band needs [5][36][32] are filled into
//                           LDS once and every tap is taken from there (the taps are split over the 4 waves).
//                           bf16: v_mfma_f32_16x16x32_bf16 (one K step per band); fp32: v_mfma_f32_16x16x4_f32 (exact
//                           fp32 products, 8 K steps per band).
//   pool2_fwd_kernel        relu(bn(y)) -> MaxPool2d(2) (floor) + 2-bit argmax; optionally straight into the LSTM's
//                           layout seq[b][t][c * F' + f] fp32 (permute(0,3,1,2) + Flatten(2), train_physionet2.py:92-93);
//                           there adjacent channel lanes store F' floats apart (scalar strided stores; the tensor is the
//                           smallest of the front end), and the backward reads dseq the same way
//   pool2_bwd_*             backward of [BatchNorm -> ReLU -> MaxPool2d(2)]: reduction over the pooled positions, fixed-
//                           order finalize, apply pass over all N H W conv outputs (rows / columns the floor dropped get a
//                           zero pooled gradient but stay in the BatchNorm sums).
//   relu_pool2_kernel       inference: max(0, MaxPool2d(2)) of a convolution whose BatchNorm is folded into it (no
//                           coefficients, no argmax bytes), 16-byte channel chunks; same two output layouts
//   conv5_in1_relu_pool2_kernel  inference: Conv2d(1, 32, 5) + bias + ReLU + MaxPool2d(2) in one kernel, the [B,F,T,32]
//                           tensor never written; bit-identical to conv5_in1_fwd_kernel + relu_pool2_kernel
//
// Every split reduction goes through per-workgroup partial rows and a fixed-order second pass: no float atomics.
#include "ops.h"

namespace {

constexpr int C5_TAPS = 25;

template <typename T> __device__ __forceinline__ float round_operand(float v);
template <> __device__ __forceinline__ float round_operand<float>(float v) { return v; }
template <> __device__ __forceinline__ float round_operand<bf16_t>(float v) { return bf2f(f2bf(v)); }

// ------------------------------------------------------------------------------------------------
// Conv2d(1, 32, 5, pad 2) forward
// ------------------------------------------------------------------------------------------------
constexpr int IN1_C = 32;
constexpr int IN1_THREADS = 256;
constexpr int IN1_PIX = 64;          // pixels per pass of a workgroup (4 threads per pixel)
constexpr int IN1_PASSES = 8;        // passes per workgroup = pixels per statistics row / 64

template <typename T>
__global__ __launch_bounds__(IN1_THREADS) void conv5_in1_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                   const float* __restrict__ bias, T* __restrict__ y,
                                                                   float* __restrict__ stats, int N, int H, int W) {
  __shared__ float ws[C5_TAPS][IN1_C];
  __shared__ float red[2][IN1_PIX][IN1_C + 1];
  const int tid = threadIdx.x;
  for (int i = tid; i < C5_TAPS * IN1_C; i += IN1_THREADS) {
    const int tap = i / IN1_C, co = i % IN1_C;
    ws[tap][co] = round_operand<T>(w[co * C5_TAPS + tap]);   // OIHW [32][1][5][5]
  }
  __syncthreads();
  const int slot = tid >> 2, cg = (tid & 3) * 8;
  const long M = (long)N * H * W;
  float bv[8], s1[8], s2[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    bv[j] = bias ? bias[cg + j] : 0.f;
    s1[j] = s2[j] = 0.f;
  }
  for (int pass = 0; pass < IN1_PASSES; ++pass) {
    const long pix = ((long)blockIdx.x * IN1_PASSES + pass) * IN1_PIX + slot;
    if (pix >= M) break;
    const int wq = (int)(pix % W);
    const long t = pix / W;
    const int hq = (int)(t % H);
    const float* img = x + (t / H) * (long)H * W;
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
#pragma unroll
    for (int r = 0; r < 5; ++r) {
      const int hh = hq + r - 2;
      if ((unsigned)hh >= (unsigned)H) continue;
#pragma unroll
      for (int s = 0; s < 5; ++s) {
        const int ww = wq + s - 2;
        if ((unsigned)ww >= (unsigned)W) continue;
        const float xv = round_operand<T>(img[(long)hh * W + ww]);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = fmaf(xv, ws[r * 5 + s][cg + j], acc[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      acc[j] += bv[j];
      s1[j] += acc[j];
      s2[j] += acc[j] * acc[j];
    }
    T* o = y + pix * IN1_C + cg;
    if (sizeof(T) == 2) {
      *reinterpret_cast<u32x4*>(o) = pack16<bf16_t>(acc);
    } else {
      *reinterpret_cast<u32x4*>(o) = pack16<float>(acc);
      *reinterpret_cast<u32x4*>(o + 4) = pack16<float>(acc + 4);
    }
  }
  if (!stats) return;   // (uniform)
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    red[0][slot][cg + j] = s1[j];
    red[1][slot][cg + j] = s2[j];
  }
  __syncthreads();
  if (tid < 2 * IN1_C) {
    const int k = tid / IN1_C, c = tid % IN1_C;
    float s = 0.f;
    for (int i = 0; i < IN1_PIX; ++i) s += red[k][i][c];
    stats[((size_t)blockIdx.x * 2 + k) * IN1_C + c] = s;
  }
}

// ------------------------------------------------------------------------------------------------
// Conv2d(1, 32, 5, pad 2) weight + bias gradient.  Partial rows [blocks][832]: 25 x 32 weight sums ([tap][co]) + 32 bias sums.
// ------------------------------------------------------------------------------------------------
constexpr int IN1_WT = 64;                         // tile width (pixels of one image row)
constexpr int IN1_ROW = (C5_TAPS + 1) * IN1_C;     // floats per partial row: tap 25 = the bias gradient
constexpr int IN1_WG_MAX_BLOCKS = 1024;

template <typename T>
__global__ __launch_bounds__(IN1_THREADS) void conv5_in1_wgrad_kernel(const float* __restrict__ x, const T* __restrict__ dy,
                                                                     float* __restrict__ partial, int N, int H, int W,
                                                                     int wsegs, int tiles, int tiles_per_block) {
  __shared__ float xs[5][IN1_WT + 4];
  __shared__ float ds[IN1_WT][IN1_C];
  const int tid = threadIdx.x, co = tid & 31, slot = tid >> 5;   // 8 slots; slot owns taps slot, slot + 8, slot + 16, slot + 24
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  int tr[4], ts[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int tap = slot + 8 * k;
    tr[k] = tap / 5;
    ts[k] = tap % 5;   // tap 25 (tr = 5): x = 1, the bias gradient; taps 26..31 (tr >= 5 too) sum the same and are never written
  }
  const int t0 = blockIdx.x * tiles_per_block, t1 = min(tiles, t0 + tiles_per_block);
  for (int tile = t0; tile < t1; ++tile) {
    const int seg = tile % wsegs, row = tile / wsegs;
    const int h = row % H, n = row / H, w0 = seg * IN1_WT;
    __syncthreads();
    for (int i = tid; i < 5 * (IN1_WT + 4); i += IN1_THREADS) {
      const int r = i / (IN1_WT + 4), c = i % (IN1_WT + 4);
      const int hh = h + r - 2, ww = w0 + c - 2;
      const bool ok = (unsigned)hh < (unsigned)H && (unsigned)ww < (unsigned)W;
      xs[r][c] = ok ? round_operand<T>(x[((long)n * H + hh) * W + ww]) : 0.f;
    }
    for (int i = tid; i < IN1_WT * IN1_C; i += IN1_THREADS) {
      const int p = i >> 5, c = i & 31;
      ds[p][c] = w0 + p < W ? Elem<T>::ld(dy + (((long)n * H + h) * W + w0 + p) * IN1_C + c) : 0.f;
    }
    __syncthreads();
    for (int p = 0; p < IN1_WT; ++p) {
      const float d = ds[p][co];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float xv = tr[k] < 5 ? xs[tr[k]][p + ts[k]] : 1.f;
        acc[k] = fmaf(xv, d, acc[k]);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int tap = slot + 8 * k;
    if (tap <= C5_TAPS) partial[(size_t)blockIdx.x * IN1_ROW + tap * IN1_C + co] = acc[k];
  }
}

// out[co][tap] (OIHW) and db[co] from the partial rows, fixed order, double sums
__global__ __launch_bounds__(256) void conv5_in1_wgrad_reduce_kernel(const float* __restrict__ partial, int rows, float* dw,
                                                                    float* db, int accumulate) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= IN1_ROW) return;
  double s = 0.0;
  for (int r = 0; r < rows; ++r) s += (double)partial[(size_t)r * IN1_ROW + i];
  const int tap = i / IN1_C, co = i % IN1_C;
  if (tap < C5_TAPS) {
    if (dw) dw[co * C5_TAPS + tap] = (accumulate ? dw[co * C5_TAPS + tap] : 0.f) + (float)s;
  } else if (db) {
    db[co] = (accumulate ? db[co] : 0.f) + (float)s;
  }
}

// ------------------------------------------------------------------------------------------------
// Conv2d(1, 32, 5, pad 2) input gradient: dx[n][h][w] = sum_{co, r, s} dy[n][h+2-r][w+2-s][co] * w[co][r][s].
// A workgroup owns DG_STRIP columns of one image and walks down its rows DG_RSTEP at a time.  The DG_WIN = DG_RSTEP + 4
// dy rows a trip reads sit in an LDS ring, so a row is fetched from memory once per strip (plus the four halo rows
// where two workgroups of a strip meet); a trip issues the global loads of the next trip's rows before its own
// arithmetic and parks them in the ring after it.  Thread = one pixel x 8 channels, as the forward; the four threads of a
// pixel are the four lanes of a DPP quad and fold in a fixed order.
// LDS layout: a ring row is NH planes of [DG_COLS][4] 16-byte chunks, plane = which of a thread's NH chunks (bf16: one
// chunk of 8 channels; fp32: two chunks of 4 channels, 16 channels apart).  A wave's ds_read_b128 then covers 16 pixels x
// 64 B = 1 KiB contiguous in both dtypes: no two lanes on one bank, no padding needed.  The weights sit beside it in the
// threads' channel order ([tap][quad lane][8]): four addresses per wave, broadcast.  They are re-read every trip: the loop
// over the tap columns stays rolled, because unrolled the compiler keeps a thread's 25 x 8 weights in registers across the
// row loop (430 of them, one wave per SIMD), which measured three times slower than two to four waves and the re-reads.
// Two output rows per trip share every dy read (30 chunk reads for 50 taps) and every weight read.
// ------------------------------------------------------------------------------------------------
constexpr int DG_STRIP = 64;                 // columns of a strip = pixels of a workgroup (4 threads per pixel)
constexpr int DG_COLS = DG_STRIP + 4;
constexpr int DG_RSTEP = 2;                  // output rows per trip
constexpr int DG_WIN = DG_RSTEP + 4;         // dy rows of a trip = ring slots
constexpr int DG_ROWS_MAX = 64;              // output rows of a workgroup at most

template <typename T>
__global__ __launch_bounds__(IN1_THREADS) void conv5_in1_dgrad_kernel(const T* __restrict__ dy, const float* __restrict__ w,
                                                                     float* __restrict__ dx, int H, int W, int strips,
                                                                     int hchunks, int rows_per) {
  constexpr int VEC = Elem<T>::VEC;          // channels per 16-byte chunk
  constexpr int NH = 8 / VEC;                // chunks of a thread's 8 channels
  constexpr int CH = IN1_C / VEC;            // chunks of a pixel
  constexpr int ROWCH = DG_COLS * CH;        // chunks of a ring row
  constexpr int PF = (DG_RSTEP * ROWCH + IN1_THREADS - 1) / IN1_THREADS;   // chunks a thread fetches per trip
  __shared__ u32x4 dys[DG_WIN * NH * DG_COLS * 4];
  __shared__ float ws[C5_TAPS][4][8];
  const int tid = threadIdx.x, p = tid >> 2, q = tid & 3;
  for (int i = tid; i < C5_TAPS * IN1_C; i += IN1_THREADS) {
    const int tap = i / IN1_C, ql = (i % IN1_C) / 8, k = i % 8;
    const int co = (k / VEC) * (4 * VEC) + ql * VEC + k % VEC;   // channel k of quad lane ql
    ws[tap][ql][k] = round_operand<T>(w[co * C5_TAPS + tap]);
  }
  const int strip = blockIdx.x % strips, t = blockIdx.x / strips;
  const int n = t / hchunks, h0 = (t % hchunks) * rows_per, h1 = min(H, h0 + rows_per);
  const int w0 = strip * DG_STRIP;
  const T* img = dy + (long)n * H * W * IN1_C;
  u32x4 v[PF];
  // rows row0 .. row0 + DG_RSTEP - 1 of the strip (with its two halo columns each side), zeros outside the image
  auto fetch = [&](int row0) {
#pragma unroll
    for (int k = 0; k < PF; ++k) {
      const int i = tid + k * IN1_THREADS;
      const int hh = row0 + i / ROWCH, ww = w0 - 2 + (i % ROWCH) / CH;
      v[k] = (u32x4){0u, 0u, 0u, 0u};
      if (i < DG_RSTEP * ROWCH && (unsigned)hh < (unsigned)H && (unsigned)ww < (unsigned)W)
        v[k] = *reinterpret_cast<const u32x4*>(img + ((long)hh * W + ww) * IN1_C + (i % CH) * VEC);
    }
  };
  auto park = [&](int row0) {
#pragma unroll
    for (int k = 0; k < PF; ++k) {
      const int i = tid + k * IN1_THREADS;
      if (i >= DG_RSTEP * ROWCH) continue;
      const int slot = (row0 + i / ROWCH - (h0 - 2)) % DG_WIN, col = (i % ROWCH) / CH, c = i % CH;
      dys[((slot * NH + c / 4) * DG_COLS + col) * 4 + c % 4] = v[k];
    }
  };
  for (int r0 = h0 - 2; r0 < h0 - 2 + DG_WIN; r0 += DG_RSTEP) {
    fetch(r0);
    park(r0);
  }
  __syncthreads();
  for (int h = h0; h < h1; h += DG_RSTEP) {
    const bool more = h + DG_RSTEP < h1;   // (uniform)
    if (more) fetch(h + DG_WIN - 2);
    const int sb = (h - h0) % DG_WIN;
    float acc[DG_RSTEP][8];
#pragma unroll
    for (int o = 0; o < DG_RSTEP; ++o)
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[o][k] = 0.f;
#pragma unroll 1   // (rolled on purpose: see the weights above)
    for (int s = 0; s < 5; ++s) {
      float d[DG_WIN][8];
#pragma unroll
      for (int j = 0; j < DG_WIN; ++j) {
        const int slot = sb + j < DG_WIN ? sb + j : sb + j - DG_WIN;
#pragma unroll
        for (int hf = 0; hf < NH; ++hf)
          unpack16<T>(dys[((slot * NH + hf) * DG_COLS + p + 4 - s) * 4 + q], d[j] + hf * VEC);
      }
#pragma unroll
      for (int r = 0; r < 5; ++r) {
        float wv[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) wv[k] = ws[r * 5 + s][q][k];
#pragma unroll
        for (int o = 0; o < DG_RSTEP; ++o)   // dy row h + o + 2 - r = ring row o + 4 - r of this trip
#pragma unroll
          for (int k = 0; k < 8; ++k) acc[o][k] = fmaf(d[o + 4 - r][k], wv[k], acc[o][k]);
      }
    }
#pragma unroll
    for (int o = 0; o < DG_RSTEP; ++o) {
      float sum = ((acc[o][0] + acc[o][1]) + (acc[o][2] + acc[o][3])) + ((acc[o][4] + acc[o][5]) + (acc[o][6] + acc[o][7]));
      sum += dpp_mov<0xB1>(sum);   // quad_perm [1,0,3,2]
      sum += dpp_mov<0x4E>(sum);   // quad_perm [2,3,0,1]: every lane of the quad holds the pixel's total
      if (q == 0 && w0 + p < W && h + o < h1) dx[((long)n * H + h + o) * W + w0 + p] = sum;
    }
    if (!more) break;
    __syncthreads();   // every thread has read the rows this trip retires
    park(h + DG_WIN - 2);
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------
// 5x5 weight gradient, Cin and Cout multiples of 32
// ------------------------------------------------------------------------------------------------
constexpr int WG5_THREADS = 256;
constexpr int WG5_BAND = 32;                 // pixels of one output row per band = K of one bf16 MFMA
constexpr int WG5_XCOLS = WG5_BAND + 4;
constexpr int WG5_BANDS_MIN = 16;            // bands per split at least (pick_split)
constexpr int WG5_MAX_BLOCKS = 1024;

template <typename T> struct Wg5;
template <> struct Wg5<bf16_t> {
  static constexpr int STRIDE = 17;          // 4-byte words per LDS pixel row of 32 channels (+1: the four k groups of a
                                             // fragment read land in disjoint banks)
  static constexpr int KSTEPS = 1;
  // 8 consecutive pixels (k = fq * 8 + j) of channel ch, from rows of 32 bf16
  static __device__ __forceinline__ u32x4 frag(const unsigned* base, int px0, int ch, int fq, int) {
    const bf16_t* b = reinterpret_cast<const bf16_t*>(base);
    unsigned v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = b[(size_t)(px0 + fq * 8 + j) * (STRIDE * 2) + ch];
    return (u32x4){v[0] | (v[1] << 16), v[2] | (v[3] << 16), v[4] | (v[5] << 16), v[6] | (v[7] << 16)};
  }
  static __device__ __forceinline__ void mma(f32x4& acc, const u32x4& a, const u32x4& b) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), acc, 0,
                                                  0, 0);
  }
};
template <> struct Wg5<float> {
  static constexpr int STRIDE = 36;          // (+4 words: as above, and rows stay 16-byte aligned)
  static constexpr int KSTEPS = 8;
  // one pixel (k = ks * 4 + fq) of channel ch; only element 0 of the vector is used
  static __device__ __forceinline__ u32x4 frag(const unsigned* base, int px0, int ch, int fq, int ks) {
    return (u32x4){base[(size_t)(px0 + ks * 4 + fq) * STRIDE + ch], 0u, 0u, 0u};
  }
  static __device__ __forceinline__ void mma(f32x4& acc, const u32x4& a, const u32x4& b) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a[0]), __uint_as_float(b[0]), acc, 0, 0, 0);
  }
};

template <typename T>
__global__ __launch_bounds__(WG5_THREADS) void conv5_wgrad_kernel(const T* __restrict__ x, const T* __restrict__ dy,
                                                                 float* __restrict__ slab, int N, int H, int W, int Cin,
                                                                 int Cout, int wsegs, int bands, int bands_per_split) {
  using K = Wg5<T>;
  constexpr int VEC = Elem<T>::VEC;           // elements per 16-byte global load
  constexpr int CHUNKS = 32 / VEC;            // 16-byte chunks per 32-channel pixel row
  constexpr int WPC = 4;                      // 4-byte words per chunk
  __shared__ unsigned dys[WG5_BAND * K::STRIDE];
  __shared__ unsigned xs[5 * WG5_XCOLS * K::STRIDE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int ci0 = blockIdx.y * 32, co0 = blockIdx.z * 32;
  // taps of this wave: wave, wave + 4, ... (7, 6, 6, 6 taps)
  f32x4 acc[7][2][2];
#pragma unroll
  for (int t = 0; t < 7; ++t)
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) acc[t][a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int b0 = blockIdx.x * bands_per_split, b1 = min(bands, b0 + bands_per_split);
  for (int band = b0; band < b1; ++band) {
    const int seg = band % wsegs, row = band / wsegs;
    const int h = row % H, n = row / H, w0 = seg * WG5_BAND;
    __syncthreads();   // the previous band's fragments have been read
    for (int i = tid; i < WG5_BAND * CHUNKS; i += WG5_THREADS) {
      const int p = i / CHUNKS, ch = i % CHUNKS;
      u32x4 v = (u32x4){0u, 0u, 0u, 0u};
      if (w0 + p < W) v = *reinterpret_cast<const u32x4*>(dy + (((size_t)n * H + h) * W + w0 + p) * Cout + co0 + ch * VEC);
      unsigned* d = dys + p * K::STRIDE + ch * WPC;
      d[0] = v[0]; d[1] = v[1]; d[2] = v[2]; d[3] = v[3];
    }
    for (int i = tid; i < 5 * WG5_XCOLS * CHUNKS; i += WG5_THREADS) {
      const int ch = i % CHUNKS, pc = i / CHUNKS;
      const int c = pc % WG5_XCOLS, r = pc / WG5_XCOLS;
      const int hh = h + r - 2, ww = w0 + c - 2;
      u32x4 v = (u32x4){0u, 0u, 0u, 0u};
      if ((unsigned)hh < (unsigned)H && (unsigned)ww < (unsigned)W)
        v = *reinterpret_cast<const u32x4*>(x + (((size_t)n * H + hh) * W + ww) * Cin + ci0 + ch * VEC);
      unsigned* d = xs + pc * K::STRIDE + ch * WPC;
      d[0] = v[0]; d[1] = v[1]; d[2] = v[2]; d[3] = v[3];
    }
    __syncthreads();
#pragma unroll 1
    for (int ks = 0; ks < K::KSTEPS; ++ks) {
      u32x4 fa[2];
#pragma unroll
      for (int a = 0; a < 2; ++a) fa[a] = K::frag(dys, 0, a * 16 + fr, fq, ks);
#pragma unroll
      for (int t = 0; t < 7; ++t) {
        const int tap = wave + 4 * t;
        if (tap < C5_TAPS) {   // (wave-uniform)
          const int r = tap / 5, s = tap % 5;
          u32x4 fb[2];
#pragma unroll
          for (int b = 0; b < 2; ++b) fb[b] = K::frag(xs, r * WG5_XCOLS + s, b * 16 + fr, fq, ks);
#pragma unroll
          for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) K::mma(acc[t][a][b], fa[a], fb[b]);
        }
      }
    }
  }
  // D layout: lane holds co = a * 16 + fq * 4 + j, ci = b * 16 + fr.  Slab [split][Cout][Cin][25] (the OIHW layout).
  float* out = slab + (size_t)blockIdx.x * Cout * Cin * C5_TAPS;
#pragma unroll
  for (int t = 0; t < 7; ++t) {
    const int tap = wave + 4 * t;
    if (tap < C5_TAPS) {
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int co = co0 + a * 16 + fq * 4 + j, ci = ci0 + b * 16 + fr;
            out[((size_t)co * Cin + ci) * C5_TAPS + tap] = acc[t][a][b][j];
          }
    }
  }
}

__global__ __launch_bounds__(256) void conv5_wgrad_reduce_kernel(const float* __restrict__ slab, int splits, long n,
                                                                float* __restrict__ dw, int accumulate) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float s = 0.f;
  if (splits > 8) {   // long columns: double sums (same fixed order)
    double d = 0.0;
    for (int k = 0; k < splits; ++k) d += (double)slab[(size_t)k * n + i];
    s = (float)d;
  } else {
    for (int k = 0; k < splits; ++k) s += slab[(size_t)k * n + i];
  }
  dw[i] = (accumulate ? dw[i] : 0.f) + s;
}

struct Wg5Split { int wsegs, bands, per, splits; };
Wg5Split wg5_split(const ConvGeom& g) {
  Wg5Split s;
  s.wsegs = ceil_div(g.W, WG5_BAND);
  s.bands = g.N * g.H * s.wsegs;
  const int tiles = (g.Cin / 32) * (g.Cout / 32);
  int want = ceil_div(s.bands, WG5_BANDS_MIN);
  const int cap = WG5_MAX_BLOCKS / tiles > 1 ? WG5_MAX_BLOCKS / tiles : 1;
  if (want > cap) want = cap;
  s.per = ceil_div(s.bands, want);
  s.splits = ceil_div(s.bands, s.per);
  return s;
}

int wg5_check(int dtype, const ConvGeom& g, const char* who) {
  if (dtype != ECGMM_BF16 && dtype != ECGMM_F32) ECG_FAIL(ECGMM_ERR_DTYPE, "%s: bad dtype %d", who, dtype);
  if (g.R != 5 || g.S != 5 || g.stride != 1 || g.pad_h != 2 || g.pad_w != 2)
    ECG_FAIL(ECGMM_ERR_SHAPE, "%s: %dx%d stride %d pad %d,%d (5x5, stride 1, pad 2 only)", who, g.R, g.S, g.stride, g.pad_h,
             g.pad_w);
  if (g.N < 1 || g.H < 1 || g.W < 1 || g.Cin < 32 || g.Cout < 32 || g.Cin % 32 || g.Cout % 32)
    ECG_FAIL(ECGMM_ERR_SHAPE, "%s: N=%d H=%d W=%d Cin=%d Cout=%d (channels must be multiples of 32)", who, g.N, g.H, g.W,
             g.Cin, g.Cout);
  if ((long)g.N * g.H * ceil_div(g.W, WG5_BAND) > 0x7fffffffL || (long)g.N * g.H * g.W > 0x7fffffffL)
    ECG_FAIL(ECGMM_ERR_SHAPE, "%s: pixel count out of range", who);
  return 0;
}

// ------------------------------------------------------------------------------------------------
// relu(bn(y)) -> MaxPool2d(2), floor semantics, first-wins ties (row-major window order, as torch)
// ------------------------------------------------------------------------------------------------
constexpr int P2_THREADS = 256;

template <typename T>
__global__ __launch_bounds__(P2_THREADS) void pool2_fwd_kernel(const T* __restrict__ y, const float* __restrict__ coef,
                                                              void* __restrict__ out, unsigned char* __restrict__ idx,
                                                              int N, int H, int W, int C, int PH, int PW, int seq) {
  const long total = (long)N * PH * PW * C;
  const long q = (long)blockIdx.x * P2_THREADS + threadIdx.x;
  if (q >= total) return;
  const int c = (int)(q % C);
  long t = q / C;
  const int pw = (int)(t % PW);
  t /= PW;
  const int ph = (int)(t % PH);
  const long n = t / PH;
  const float sc = coef[c], sh = coef[C + c];
  float best = 0.f;
  int arg = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int h = 2 * ph + (k >> 1), w = 2 * pw + (k & 1);
    const float z = fmaxf(fmaf(Elem<T>::ld(y + ((n * H + h) * W + w) * C + c), sc, sh), 0.f);
    if (k == 0 || z > best) {
      best = z;
      arg = k;
    }
  }
  if (idx) idx[q] = (unsigned char)arg;
  if (seq) reinterpret_cast<float*>(out)[((n * PW + pw) * C + c) * PH + ph] = best;
  else Elem<T>::st(reinterpret_cast<T*>(out) + q, best);
}

struct P2Bwd {
  const void* dp;               // gradient of the pooled output: [N][PH][PW][C] compute dtype, or (seq) [N][PW][C * PH] fp32
  const unsigned char* idx;     // [N][PH][PW][C]
  const void* y;                // raw conv output [N][H][W][C]
  const float* coef;            // [4][C] scale, shift, mean, invstd
  const float* bcoef;           // [2][C] k1, k2 of the apply pass
  void* dy;
  float* rows;                  // reduce: [blocks][2][C]; apply: [blocks][C] (bias gradient) or null
  int N, H, W, C, PH, PW, seq, training;
  long chunk;                   // (pooled) pixels per workgroup
};

template <typename T> __device__ __forceinline__ float p2_dp(const P2Bwd& p, long n, int ph, int pw, int c) {
  if (p.seq) return reinterpret_cast<const float*>(p.dp)[((n * p.PW + pw) * p.C + c) * p.PH + ph];
  return Elem<T>::ld(reinterpret_cast<const T*>(p.dp) + ((n * p.PH + ph) * p.PW + pw) * p.C + c);
}

// sums over a workgroup's slots (256 / C pixel slots per channel), fixed order
template <int NV> __device__ __forceinline__ void p2_block_rows(float (*sh)[P2_THREADS], const float* v, int C, float* row) {
  const int tid = threadIdx.x;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NV; ++k) sh[k][tid] = v[k];
  __syncthreads();
  if (tid < C) {
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      float s = 0.f;
      for (int i = tid; i < P2_THREADS; i += C) s += sh[k][i];
      row[(size_t)k * C + tid] = s;
    }
  }
}

// pass 1: per-channel (sum g, sum g * (y - mean)) over the pooled positions, g = [bn(y) > 0 at the window's winner] * dp
template <typename T> __global__ __launch_bounds__(P2_THREADS) void pool2_bwd_reduce_kernel(P2Bwd p) {
  __shared__ float sh[2][P2_THREADS];
  const int tid = threadIdx.x, c = tid % p.C, slot = tid / p.C, nslot = P2_THREADS / p.C;
  const float sc = p.coef[c], shf = p.coef[p.C + c], mean = p.coef[2 * p.C + c];
  const long PP = (long)p.N * p.PH * p.PW;
  const long q0 = blockIdx.x * p.chunk, q1 = min(PP, q0 + p.chunk);
  const T* y = reinterpret_cast<const T*>(p.y);
  float v[2] = {0.f, 0.f};
  for (long q = q0 + slot; q < q1; q += nslot) {
    const int pw = (int)(q % p.PW);
    const long t = q / p.PW;
    const int ph = (int)(t % p.PH);
    const long n = t / p.PH;
    const int k = p.idx[q * p.C + c] & 3;
    const float yv = Elem<T>::ld(y + ((n * p.H + 2 * ph + (k >> 1)) * p.W + 2 * pw + (k & 1)) * p.C + c);
    const float g = fmaf(yv, sc, shf) > 0.f ? p2_dp<T>(p, n, ph, pw, c) : 0.f;
    v[0] += g;
    v[1] += g * (yv - mean);
  }
  p2_block_rows<2>(sh, v, p.C, p.rows + (size_t)blockIdx.x * 2 * p.C);
}

// dgamma, dbeta and the apply pass's coefficients; count = N H W (every conv output, dropped rows / columns included)
__global__ __launch_bounds__(256) void pool2_bwd_finalize_kernel(const float* __restrict__ rows, int nrows, int C, double count,
                                                                const float* __restrict__ coef, float* dgamma, float* dbeta,
                                                                float* __restrict__ bcoef) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  double s1 = 0.0, s2 = 0.0;
  for (int r = 0; r < nrows; ++r) {
    s1 += (double)rows[((size_t)r * 2) * C + c];
    s2 += (double)rows[((size_t)r * 2 + 1) * C + c];
  }
  const double invstd = (double)coef[3 * C + c];
  if (dgamma) dgamma[c] = (float)(s2 * invstd);
  if (dbeta) dbeta[c] = (float)s1;
  bcoef[c] = (float)(s1 / count);
  bcoef[C + c] = (float)(s2 * invstd * invstd / count);
}

// pass 2: dy over all N H W conv outputs.  training: dy = scale * (g - k1 - (y - mean) * k2); eval: dy = scale * g
template <typename T> __global__ __launch_bounds__(P2_THREADS) void pool2_bwd_apply_kernel(P2Bwd p) {
  __shared__ float sh[1][P2_THREADS];
  const int tid = threadIdx.x, c = tid % p.C, slot = tid / p.C, nslot = P2_THREADS / p.C;
  const float sc = p.coef[c], shf = p.coef[p.C + c], mean = p.coef[2 * p.C + c];
  const float k1 = p.training ? p.bcoef[c] : 0.f, k2 = p.training ? p.bcoef[p.C + c] : 0.f;
  const long M = (long)p.N * p.H * p.W;
  const long m0 = blockIdx.x * p.chunk, m1 = min(M, m0 + p.chunk);
  const T* y = reinterpret_cast<const T*>(p.y);
  T* dy = reinterpret_cast<T*>(p.dy);
  float v[1] = {0.f};
  for (long m = m0 + slot; m < m1; m += nslot) {
    const int w = (int)(m % p.W);
    const long t = m / p.W;
    const int h = (int)(t % p.H);
    const long n = t / p.H;
    const int ph = h >> 1, pw = w >> 1;
    const float yv = Elem<T>::ld(y + m * p.C + c);
    float g = 0.f;
    if (ph < p.PH && pw < p.PW) {
      const int k = p.idx[((n * p.PH + ph) * p.PW + pw) * p.C + c] & 3;
      if (k == (h & 1) * 2 + (w & 1) && fmaf(yv, sc, shf) > 0.f) g = p2_dp<T>(p, n, ph, pw, c);
    }
    const float d = sc * (g - k1 - (yv - mean) * k2);
    Elem<T>::st(dy + m * p.C + c, d);
    v[0] += d;
  }
  if (p.rows) p2_block_rows<1>(sh, v, p.C, p.rows + (size_t)blockIdx.x * p.C);   // (uniform)
}

constexpr int P2_MAX_ROWS = 1024;
int p2_check(int dtype, int N, int H, int W, int C, const char* who) {
  if (dtype != ECGMM_BF16 && dtype != ECGMM_F32) ECG_FAIL(ECGMM_ERR_DTYPE, "%s: bad dtype %d", who, dtype);
  if (N < 1 || H < 2 || W < 2 || C < 32 || C > 256 || P2_THREADS % C != 0)
    ECG_FAIL(ECGMM_ERR_SHAPE, "%s: N=%d H=%d W=%d C=%d (H, W >= 2; C = 32, 64, 128 or 256)", who, N, H, W, C);
  if ((long)N * H * W * C / 4 > 0x7fffffffL) ECG_FAIL(ECGMM_ERR_SHAPE, "%s: tensor too large", who);
  return 0;
}
// pixels per workgroup of a pass over `pixels` (at most P2_MAX_ROWS workgroups, at least 8 pixels per slot)
long p2_chunk(long pixels, int C) {
  const long least = (long)(P2_THREADS / C) * 8;
  const long c = (pixels + P2_MAX_ROWS - 1) / P2_MAX_ROWS;
  return c > least ? c : least;
}

// ------------------------------------------------------------------------------------------------
// Inference forms (plan_infer.hip): the BatchNorm is folded into the convolution, so a block ends in max(0, max over the
// 2x2 window); no coefficients, no argmax bytes.
// ------------------------------------------------------------------------------------------------
// relu -> MaxPool2d(2), floor semantics.  Thread = one pooled pixel x one 16-byte channel chunk: four 16-byte loads, one
// 16-byte store; seq: the chunk's floats go PH apart into seq[n][pw][c * PH + ph], as pool2_fwd_kernel writes it.
template <typename T>
__global__ __launch_bounds__(P2_THREADS) void relu_pool2_kernel(const T* __restrict__ y, void* __restrict__ out, int N, int H,
                                                               int W, int C, int PH, int PW, int seq) {
  constexpr int VEC = Elem<T>::VEC;
  const int cpr = C / VEC;
  const long total = (long)N * PH * PW * cpr;
  const long i = (long)blockIdx.x * P2_THREADS + threadIdx.x;
  if (i >= total) return;
  const int c0 = (int)(i % cpr) * VEC;
  const long q = i / cpr;
  const int pw = (int)(q % PW);
  const long t = q / PW;
  const int ph = (int)(t % PH);
  const long n = t / PH;
  float best[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) best[j] = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int h = 2 * ph + (k >> 1), w = 2 * pw + (k & 1);
    float f[VEC];
    unpack16<T>(*reinterpret_cast<const u32x4*>(y + ((n * H + h) * W + w) * C + c0), f);
#pragma unroll
    for (int j = 0; j < VEC; ++j) best[j] = f[j] > best[j] ? f[j] : best[j];   // (a NaN input never wins, -0 never wins)
  }
  if (seq) {
    float* o = reinterpret_cast<float*>(out) + ((n * PW + pw) * C + c0) * PH + ph;
#pragma unroll
    for (int j = 0; j < VEC; ++j) o[(long)j * PH] = best[j];
  } else {
    *reinterpret_cast<u32x4*>(reinterpret_cast<T*>(out) + q * C + c0) = pack16<T>(best);
  }
}

// Conv2d(1, 32, 5, pad 2) + bias + ReLU + MaxPool2d(2) in one kernel: [N][H][W] fp32 -> [N][H/2][W/2][32].
// Thread = one POOLED pixel x 8 channels (four threads per pixel, as conv5_in1_fwd_kernel).  It reads the 6x6 input patch
// of its 2x2 window once into registers (instead of four 5x5 patches) and keeps the window's four conv outputs in 32
// accumulators, so a weight read from LDS feeds four fma instead of one: the two-launch form spends a ds_read_b128 per
// four fma, this one per sixteen.  Rows / columns the floor drops are never computed; nothing but the pooled tensor is
// written.
// Every conv output is accumulated exactly as conv5_in1_fwd_kernel accumulates it: operands rounded the same way, one fmaf
// per tap in the order (r, then s), the bias added after the taps.  A tap outside the image is a zero in the patch:
// fmaf(0, w, acc) == acc bit for bit for any finite w (acc starts at +0 and a sum is -0 only if both terms are, so acc is
// never -0), which is the skipped tap of conv5_in1_fwd_kernel.  Rounding to the compute dtype is monotone, so it commutes
// with the maxima: max over the fp32 sums, max with 0 (same comparison as relu_pool2_kernel), ONE rounding at the store --
// the bits of conv5_in1_fwd (no statistics) followed by relu_pool2.
constexpr int FP_PASSES = 8;         // passes per workgroup (64 pooled pixels each)

template <typename T>
__global__ __launch_bounds__(IN1_THREADS) void conv5_in1_relu_pool2_kernel(const float* __restrict__ x,
                                                                          const float* __restrict__ w,
                                                                          const float* __restrict__ bias, T* __restrict__ out,
                                                                          int N, int H, int W, int PH, int PW) {
  __shared__ float ws[C5_TAPS][IN1_C];
  const int tid = threadIdx.x;
  for (int i = tid; i < C5_TAPS * IN1_C; i += IN1_THREADS) {
    const int tap = i / IN1_C, co = i % IN1_C;
    ws[tap][co] = round_operand<T>(w[co * C5_TAPS + tap]);   // OIHW [32][1][5][5]
  }
  __syncthreads();
  const int slot = tid >> 2, cg = (tid & 3) * 8;
  const long Q = (long)N * PH * PW;
  float bv[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) bv[j] = bias ? bias[cg + j] : 0.f;
  for (int pass = 0; pass < FP_PASSES; ++pass) {
    const long q = ((long)blockIdx.x * FP_PASSES + pass) * IN1_PIX + slot;
    if (q >= Q) break;
    const int pw = (int)(q % PW);
    const long t = q / PW;
    const int ph = (int)(t % PH);
    const float* img = x + (t / PH) * (long)H * W;
    const int h0 = 2 * ph - 2, w0 = 2 * pw - 2;
    // the 36 loads are unconditional (address clamped into the image, value dropped where the tap lies outside), so they
    // are all in flight before the first wait instead of one branch and one wait each
    float patch[6][6];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      const int hh = h0 + a;
      const bool hok = (unsigned)hh < (unsigned)H;
      const float* row = img + (long)min(max(hh, 0), H - 1) * W;
#pragma unroll
      for (int b = 0; b < 6; ++b) {
        const int ww = w0 + b;
        const float v = row[min(max(ww, 0), W - 1)];
        patch[a][b] = (hok && (unsigned)ww < (unsigned)W) ? round_operand<T>(v) : 0.f;
      }
    }
    float acc[4][8];
#pragma unroll
    for (int o = 0; o < 4; ++o)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[o][j] = 0.f;
#pragma unroll
    for (int r = 0; r < 5; ++r) {
#pragma unroll
      for (int s = 0; s < 5; ++s) {
        float wv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) wv[j] = ws[r * 5 + s][cg + j];
#pragma unroll
        for (int o = 0; o < 4; ++o) {
          const float xv = patch[(o >> 1) + r][(o & 1) + s];
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[o][j] = fmaf(xv, wv[j], acc[o][j]);
        }
      }
    }
    float best[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) best[j] = 0.f;
#pragma unroll
    for (int o = 0; o < 4; ++o)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float v = acc[o][j] + bv[j];
        best[j] = v > best[j] ? v : best[j];
      }
    T* o = out + q * IN1_C + cg;
    if (sizeof(T) == 2) {
      *reinterpret_cast<u32x4*>(o) = pack16<bf16_t>(best);
    } else {
      *reinterpret_cast<u32x4*>(o) = pack16<float>(best);
      *reinterpret_cast<u32x4*>(o + 4) = pack16<float>(best + 4);
    }
  }
}

}  // namespace

// ================================================================================================
// host entry points
// ================================================================================================
int ecg_conv5_in1_stats_rows(int N, int H, int W) { return ceil_div((long)N * H * W, IN1_PIX * IN1_PASSES); }

static int in1_check(int dtype, int N, int H, int W, const char* who) {
  if (dtype != ECGMM_BF16 && dtype != ECGMM_F32) ECG_FAIL(ECGMM_ERR_DTYPE, "%s: bad dtype %d", who, dtype);
  if (N < 1 || H < 1 || W < 1 || (long)N * H * W > 0x7fffffffL / IN1_C)
    ECG_FAIL(ECGMM_ERR_SHAPE, "%s: bad input %dx%dx%d", who, N, H, W);
  return 0;
}

int ecg_conv5_in1_fwd(int dtype, const float* x, const float* w, const float* bias, void* y, float* stats, int N, int H,
                      int W, hipStream_t s) {
  ECG_TRY(in1_check(dtype, N, H, W, "conv5_in1_fwd"));
  if (!x || !w || !y) ECG_FAIL(ECGMM_ERR_SHAPE, "conv5_in1_fwd: x, w and y must not be null");
  const int grid = ecg_conv5_in1_stats_rows(N, H, W);
  if (dtype == ECGMM_BF16)
    hipLaunchKernelGGL(conv5_in1_fwd_kernel<bf16_t>, dim3(grid), dim3(IN1_THREADS), 0, s, x, w, bias, (bf16_t*)y, stats, N, H, W);
  else
    hipLaunchKernelGGL(conv5_in1_fwd_kernel<float>, dim3(grid), dim3(IN1_THREADS), 0, s, x, w, bias, (float*)y, stats, N, H, W);
  ECG_CHECK_LAUNCH("conv5_in1_fwd");
  return 0;
}

static int in1_wgrad_blocks(int N, int H, int W, int* per) {
  const int tiles = N * H * ceil_div(W, IN1_WT);
  const int p = ceil_div(tiles, IN1_WG_MAX_BLOCKS);
  if (per) *per = p;
  return ceil_div(tiles, p);
}
size_t ecg_conv5_in1_wgrad_workspace(int N, int H, int W) {
  if (in1_check(ECGMM_F32, N, H, W, "conv5_in1_bwd_weight_workspace") != 0) return 0;
  return (size_t)in1_wgrad_blocks(N, H, W, nullptr) * IN1_ROW * sizeof(float);
}
int ecg_conv5_in1_wgrad(int dtype, const float* x, const void* dy, float* dw, float* db, int accumulate, void* ws,
                        size_t ws_bytes, int N, int H, int W, hipStream_t s) {
  ECG_TRY(in1_check(dtype, N, H, W, "conv5_in1_bwd_weight"));
  if (!x || !dy) ECG_FAIL(ECGMM_ERR_SHAPE, "conv5_in1_bwd_weight: x and dy must not be null");
  int per = 1;
  const int blocks = in1_wgrad_blocks(N, H, W, &per);
  const size_t need = (size_t)blocks * IN1_ROW * sizeof(float);
  if (!ws || ws_bytes < need) ECG_FAIL(ECGMM_ERR_WORKSPACE, "conv5_in1_bwd_weight: workspace %zu bytes, need %zu", ws_bytes, need);
  const int wsegs = ceil_div(W, IN1_WT), tiles = N * H * wsegs;
  if (dtype == ECGMM_BF16)
    hipLaunchKernelGGL(conv5_in1_wgrad_kernel<bf16_t>, dim3(blocks), dim3(IN1_THREADS), 0, s, x, (const bf16_t*)dy, (float*)ws,
                       N, H, W, wsegs, tiles, per);
  else
    hipLaunchKernelGGL(conv5_in1_wgrad_kernel<float>, dim3(blocks), dim3(IN1_THREADS), 0, s, x, (const float*)dy, (float*)ws,
                       N, H, W, wsegs, tiles, per);
  ECG_CHECK_LAUNCH("conv5_in1_wgrad");
  hipLaunchKernelGGL(conv5_in1_wgrad_reduce_kernel, dim3(ceil_div(IN1_ROW, 256)), dim3(256), 0, s, (const float*)ws, blocks,
                     dw, db, accumulate);
  ECG_CHECK_LAUNCH("conv5_in1_wgrad_reduce");
  return 0;
}

// rows of a workgroup: the height in equal parts of at most DG_ROWS_MAX rows, rounded up to whole trips
static int in1_dgrad_rows(int H) {
  const int parts = ceil_div(H, DG_ROWS_MAX);
  return ceil_div(ceil_div(H, parts), DG_RSTEP) * DG_RSTEP;
}
void ecg_conv5_in1_dgrad_tile(int H, int* strip, int* row_step, int* rows) {
  if (strip) *strip = DG_STRIP;
  if (row_step) *row_step = DG_RSTEP;
  if (rows) *rows = H >= 1 ? in1_dgrad_rows(H) : 0;
}
int ecg_conv5_in1_dgrad(int dtype, const void* dy, const float* w, float* dx, int N, int H, int W, hipStream_t s) {
  ECG_TRY(in1_check(dtype, N, H, W, "conv5_in1_bwd_data"));
  if (!dy || !w || !dx) ECG_FAIL(ECGMM_ERR_SHAPE, "conv5_in1_bwd_data: dy, w and dx must not be null");
  if ((uintptr_t)dy % 16) ECG_FAIL(ECGMM_ERR_SHAPE, "conv5_in1_bwd_data: dy must be 16-byte aligned");
  const int strips = ceil_div(W, DG_STRIP), rows_per = in1_dgrad_rows(H), hchunks = ceil_div(H, rows_per);
  const long blocks = (long)N * hchunks * strips;   // <= N H W <= 2^31 / 32 (in1_check)
  const dim3 grid((unsigned)blocks);
  if (dtype == ECGMM_BF16)
    hipLaunchKernelGGL(conv5_in1_dgrad_kernel<bf16_t>, grid, dim3(IN1_THREADS), 0, s, (const bf16_t*)dy, w, dx, H, W, strips,
                       hchunks, rows_per);
  else
    hipLaunchKernelGGL(conv5_in1_dgrad_kernel<float>, grid, dim3(IN1_THREADS), 0, s, (const float*)dy, w, dx, H, W, strips,
                       hchunks, rows_per);
  ECG_CHECK_LAUNCH("conv5_in1_dgrad");
  return 0;
}

size_t ecg_conv5_wgrad_workspace(int dtype, const ConvGeom& g) {
  if (wg5_check(dtype, g, "conv5_bwd_weight_workspace") != 0) return 0;
  return (size_t)wg5_split(g).splits * g.Cout * g.Cin * C5_TAPS * sizeof(float);
}
int ecg_conv5_wgrad(int dtype, const ConvGeom& g, const void* x, const void* dy, float* dw, int accumulate, void* ws,
                    size_t ws_bytes, hipStream_t s) {
  ECG_TRY(wg5_check(dtype, g, "conv5_bwd_weight"));
  if (!x || !dy || !dw) ECG_FAIL(ECGMM_ERR_SHAPE, "conv5_bwd_weight: x, dy and dw must not be null");
  const Wg5Split sp = wg5_split(g);
  const long n = (long)g.Cout * g.Cin * C5_TAPS;
  const size_t need = (size_t)sp.splits * n * sizeof(float);
  if (!ws || ws_bytes < need) ECG_FAIL(ECGMM_ERR_WORKSPACE, "conv5_bwd_weight: workspace %zu bytes, need %zu", ws_bytes, need);
  const dim3 grid(sp.splits, g.Cin / 32, g.Cout / 32);
  if (dtype == ECGMM_BF16)
    hipLaunchKernelGGL(conv5_wgrad_kernel<bf16_t>, grid, dim3(WG5_THREADS), 0, s, (const bf16_t*)x, (const bf16_t*)dy,
                       (float*)ws, g.N, g.H, g.W, g.Cin, g.Cout, sp.wsegs, sp.bands, sp.per);
  else
    hipLaunchKernelGGL(conv5_wgrad_kernel<float>, grid, dim3(WG5_THREADS), 0, s, (const float*)x, (const float*)dy, (float*)ws,
                       g.N, g.H, g.W, g.Cin, g.Cout, sp.wsegs, sp.bands, sp.per);
  ECG_CHECK_LAUNCH("conv5_wgrad");
  hipLaunchKernelGGL(conv5_wgrad_reduce_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, s, (const float*)ws, sp.splits, n, dw,
                     accumulate);
  ECG_CHECK_LAUNCH("conv5_wgrad_reduce");
  return 0;
}

int ecg_bnrelu_maxpool2(int dtype, const void* y, const float* coef, void* out, unsigned char* idx, int N, int H, int W, int C,
                        int seq_layout, hipStream_t s) {
  ECG_TRY(p2_check(dtype, N, H, W, C, "bnrelu_maxpool2"));
  if (!y || !coef || !out) ECG_FAIL(ECGMM_ERR_SHAPE, "bnrelu_maxpool2: y, coef and out must not be null");
  const int PH = H / 2, PW = W / 2;
  const long total = (long)N * PH * PW * C;
  const dim3 grid(ceil_div(total, P2_THREADS));
  if (dtype == ECGMM_BF16)
    hipLaunchKernelGGL(pool2_fwd_kernel<bf16_t>, grid, dim3(P2_THREADS), 0, s, (const bf16_t*)y, coef, out, idx, N, H, W, C, PH, PW, seq_layout);
  else
    hipLaunchKernelGGL(pool2_fwd_kernel<float>, grid, dim3(P2_THREADS), 0, s, (const float*)y, coef, out, idx, N, H, W, C, PH, PW, seq_layout);
  ECG_CHECK_LAUNCH("bnrelu_maxpool2");
  return 0;
}

int ecg_relu_maxpool2(int dtype, const void* y, void* out, int N, int H, int W, int C, int seq_layout, hipStream_t s) {
  if (dtype != ECGMM_BF16 && dtype != ECGMM_F32) ECG_FAIL(ECGMM_ERR_DTYPE, "relu_maxpool2: bad dtype %d", dtype);
  if (!y || !out) ECG_FAIL(ECGMM_ERR_SHAPE, "relu_maxpool2: y and out must not be null");
  const int vec = dtype == ECGMM_BF16 ? 8 : 4;
  if (N < 1 || H < 2 || W < 2 || C < vec || C % vec)
    ECG_FAIL(ECGMM_ERR_SHAPE, "relu_maxpool2: N=%d H=%d W=%d C=%d (H, W >= 2; C a multiple of %d)", N, H, W, C, vec);
  if ((long)N * H * W * C / 4 > 0x7fffffffL) ECG_FAIL(ECGMM_ERR_SHAPE, "relu_maxpool2: tensor too large");
  if ((uintptr_t)y % 16 || (!seq_layout && (uintptr_t)out % 16))
    ECG_FAIL(ECGMM_ERR_SHAPE, "relu_maxpool2: y and out must be 16-byte aligned");
  const int PH = H / 2, PW = W / 2;
  const long total = (long)N * PH * PW * (C / vec);
  const dim3 grid(ceil_div(total, P2_THREADS));
  if (dtype == ECGMM_BF16)
    hipLaunchKernelGGL(relu_pool2_kernel<bf16_t>, grid, dim3(P2_THREADS), 0, s, (const bf16_t*)y, out, N, H, W, C, PH, PW, seq_layout);
  else
    hipLaunchKernelGGL(relu_pool2_kernel<float>, grid, dim3(P2_THREADS), 0, s, (const float*)y, out, N, H, W, C, PH, PW, seq_layout);
  ECG_CHECK_LAUNCH("relu_maxpool2");
  return 0;
}

int ecg_conv5_in1_relu_pool2(int dtype, const float* x, const float* w, const float* bias, void* out, int N, int H, int W,
                             hipStream_t s) {
  ECG_TRY(in1_check(dtype, N, H, W, "conv5_in1_relu_pool2"));
  if (H < 2 || W < 2) ECG_FAIL(ECGMM_ERR_SHAPE, "conv5_in1_relu_pool2: %dx%d (a 2x2 pool needs H, W >= 2)", H, W);
  if (!x || !w || !out) ECG_FAIL(ECGMM_ERR_SHAPE, "conv5_in1_relu_pool2: x, w and out must not be null");
  if ((uintptr_t)out % 16) ECG_FAIL(ECGMM_ERR_SHAPE, "conv5_in1_relu_pool2: out must be 16-byte aligned");
  const int PH = H / 2, PW = W / 2;
  const dim3 grid(ceil_div((long)N * PH * PW, IN1_PIX * FP_PASSES));
  if (dtype == ECGMM_BF16)
    hipLaunchKernelGGL(conv5_in1_relu_pool2_kernel<bf16_t>, grid, dim3(IN1_THREADS), 0, s, x, w, bias, (bf16_t*)out, N, H, W, PH, PW);
  else
    hipLaunchKernelGGL(conv5_in1_relu_pool2_kernel<float>, grid, dim3(IN1_THREADS), 0, s, x, w, bias, (float*)out, N, H, W, PH, PW);
  ECG_CHECK_LAUNCH("conv5_in1_relu_pool2");
  return 0;
}

// workspace: reduce rows [P2_MAX_ROWS][2][C] | bcoef [2][C] | bias rows [P2_MAX_ROWS][C]
size_t ecg_pool2_bn_bwd_workspace(int N, int H, int W, int C) {
  if (p2_check(ECGMM_F32, N, H, W, C, "pool2_bn_bwd_workspace") != 0) return 0;
  return ((size_t)P2_MAX_ROWS * 3 * C + 2 * C) * sizeof(float);
}
int ecg_pool2_bn_bwd(int dtype, const void* dp, const unsigned char* idx, const void* y, const float* coef, int training,
                     float* dgamma, float* dbeta, void* dy, float* dbias, int N, int H, int W, int C, int seq_layout, void* ws,
                     size_t ws_bytes, hipStream_t s) {
  ECG_TRY(p2_check(dtype, N, H, W, C, "pool2_bn_bwd"));
  if (!dp || !idx || !y || !coef) ECG_FAIL(ECGMM_ERR_SHAPE, "pool2_bn_bwd: dp, idx, y and coef must not be null");
  const size_t need = ecg_pool2_bn_bwd_workspace(N, H, W, C);
  if (!ws || ws_bytes < need) ECG_FAIL(ECGMM_ERR_WORKSPACE, "pool2_bn_bwd: workspace %zu bytes, need %zu", ws_bytes, need);
  float* rows = (float*)ws;
  float* bcoef = rows + (size_t)P2_MAX_ROWS * 2 * C;
  float* brows = bcoef + 2 * C;
  P2Bwd p;
  memset(&p, 0, sizeof(p));
  p.dp = dp; p.idx = idx; p.y = y; p.coef = coef; p.N = N; p.H = H; p.W = W; p.C = C; p.PH = H / 2; p.PW = W / 2;
  p.seq = seq_layout; p.training = training;
  const long PP = (long)N * p.PH * p.PW, M = (long)N * H * W;
  if (training || dgamma || dbeta) {
    p.rows = rows;
    p.chunk = p2_chunk(PP, C);
    const int nb = ceil_div(PP, p.chunk);
    if (dtype == ECGMM_BF16) hipLaunchKernelGGL(pool2_bwd_reduce_kernel<bf16_t>, dim3(nb), dim3(P2_THREADS), 0, s, p);
    else hipLaunchKernelGGL(pool2_bwd_reduce_kernel<float>, dim3(nb), dim3(P2_THREADS), 0, s, p);
    ECG_CHECK_LAUNCH("pool2_bwd_reduce");
    hipLaunchKernelGGL(pool2_bwd_finalize_kernel, dim3(ceil_div(C, 256)), dim3(256), 0, s, (const float*)rows, nb, C, (double)M,
                       coef, dgamma, dbeta, bcoef);
    ECG_CHECK_LAUNCH("pool2_bwd_finalize");
  }
  if (!dy) return 0;
  p.bcoef = bcoef; p.dy = dy; p.rows = dbias ? brows : nullptr;
  p.chunk = p2_chunk(M, C);
  const int nb = ceil_div(M, p.chunk);
  if (dtype == ECGMM_BF16) hipLaunchKernelGGL(pool2_bwd_apply_kernel<bf16_t>, dim3(nb), dim3(P2_THREADS), 0, s, p);
  else hipLaunchKernelGGL(pool2_bwd_apply_kernel<float>, dim3(nb), dim3(P2_THREADS), 0, s, p);
  ECG_CHECK_LAUNCH("pool2_bwd_apply");
  if (dbias) ECG_TRY(ecg_rows_sum(brows, nb, C, dbias, 0, s));
  return 0;
}
