// Input gradient of the two stem convolutions (7x7 / 1x7, stride 2, pad 3, 64 output channels), gfx950.
//   2-D: dy [N, OH, OW, 64] (compute dtype, channels-last) x conv1.weight [64, Cin, 7, 7] -> dx [N, Cin, H, W] fp32
//   1-D: dy [N, 1,  L1, 64]                                x initial.0.weight [64, Cin, 7] -> dx [N, Cin, L]   fp32
// == autograd of F.conv2d(x, w, stride=2, padding=3) / F.conv1d(...) w.r.t. x (torchvision resnet18.conv1; PMB:100).
//
// Formulation.  An input pixel (h, w) receives dy[oh][ow] through tap kh = h + 3 - 2 oh, kw = w + 3 - 2 ow: rows of odd h
// see kh in {0,2,4,6}, rows of even h see {1,3,5} (the same along w): <= 4 x 4 contributing output positions.  The 64
// output channels are the reduction dimension of an MFMA whose narrow side is (input channel, kw); the row taps kh
// extend the reduction:    Z[(ci, kw)][ow] = sum_kh sum_co W[co][ci][kh][kw] * dy[oh(h, kh)][ow][co]
// is one accumulator chain of (3 or 4) x 64 products per output row h, and what is left is the 1-D scatter along w,
//                          dx[ci][h][w] = sum_kw Z[(ci, kw)][(w + 3 - kw) / 2],
// taken as a GATHER from LDS: every dx element is written once, in full, no memset and no atomics.
//
// Work item = one wave = one strip: PR x 16 output positions of dy held in REGISTERS for the whole strip (each value is
// loaded from memory once per strip; the 3-position halo between neighbouring strips is re-read through L2), producing
// 2 (PR - 3) x 26 input pixels per input channel.  Waves of a workgroup share only the packed weights in LDS (built once
// per workgroup from the fp32 OIHW master weights, workgroups are persistent); each wave has its own Z buffer, so the
// strip loop has no workgroup barrier.
//   bf16: PR = 16, v_mfma_f32_16x16x32_bf16 (K = 32 per instruction); fp32: PR = 7, 4 x v_mfma_f32_16x16x4_f32 per
//   16-byte fragment (exact fp32 products, the 1e-3 parity path); 1-D: PR = 1.
// (ci, kw) is laid out as ci * 8 + kw (kw = 7 is a zero column), so a 16-column MFMA block holds two whole input channels
// and the gather of a block never needs another block's columns.
#include "ops.h"

namespace {

template <typename T> struct SdMma;
template <> struct SdMma<bf16_t> {
  static __device__ __forceinline__ f32x4 run(f32x4 acc, const u32x4& a, const u32x4& b) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), acc,
                                                   0, 0, 0);
  }
};
template <> struct SdMma<float> {
  static __device__ __forceinline__ f32x4 run(f32x4 acc, const u32x4& a, const u32x4& b) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a[j]), __uint_as_float(b[j]), acc, 0, 0, 0);
    return acc;
  }
};

struct StemDgradParams {
  const void* dy;
  const float* w;   // [64][Cin][R][7] fp32
  float* dx;        // [N][Cin][H][W]
  int N, Cin, H, W, OH, OW;
  int nbw;          // 16-column blocks of (ci, kw): ceil(Cin / 2)
  int strips_w, strips_h;
  long nstrips;
};

constexpr int SD_THREADS = 256;
constexpr int SD_STRIP_W = 13;   // useful output positions of a 16-position strip (3 halo positions)

// everything this wave wrote to its LDS buffer is visible to its own later reads (one wave's LDS operations execute in
// order; this only keeps the compiler from moving them across)
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <typename T, bool TWO_D, int PR>
__global__ __launch_bounds__(SD_THREADS, 2) void stem_dgrad_kernel(StemDgradParams p) {
  constexpr int FK = 16 / sizeof(T);   // K elements per lane and fragment
  constexpr int KSTEP = 4 * FK;        // K per fragment
  constexpr int NKS = 64 / KSTEP;      // fragments per 64 output channels
  constexpr int UR = TWO_D ? PR - 3 : 1;   // output-position rows whose 2 UR input rows are complete in this strip
  constexpr int NEH = TWO_D ? 2 : 1;       // row parity classes
  constexpr int R = TWO_D ? 7 : 1;
  extern __shared__ __align__(16) unsigned char sd_lds[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int li = lane & 15, g = lane >> 4;
  // fragments: class 0 (even h: kh = 1, 3, 5; 1-D: the only row) then class 1 (odd h: kh = 0, 2, 4, 6)
  const int nth0 = TWO_D ? 3 : 1;
  const int frags0 = p.nbw * nth0 * NKS;
  const int nfrags = frags0 + (TWO_D ? p.nbw * 4 * NKS : 0);
  u32x4* wl = reinterpret_cast<u32x4*>(sd_lds);
  float* zw = reinterpret_cast<float*>(sd_lds + (size_t)nfrags * 64 * 16) + wv * (UR * 256);

  // ---- packed weights: A fragment (row i = column (ci, kw) of the block, K = output channels) per (class, block, kh tap, K step)
  for (int idx = threadIdx.x; idx < nfrags * 64; idx += SD_THREADS) {
    int f = idx >> 6;
    const int l = idx & 63, i = l & 15, gg = l >> 4;
    const int eh = f >= frags0 ? 1 : 0;
    if (eh) f -= frags0;
    const int nth = TWO_D ? 3 + eh : 1;
    const int ks = f % NKS, th = (f / NKS) % nth, nb = f / (NKS * nth);
    const int ci = nb * 2 + (i >> 3), kw = i & 7;
    const int kh = TWO_D ? 2 * th + 1 - eh : 0;
    float v[FK];
#pragma unroll
    for (int e = 0; e < FK; ++e) {
      const int co = ks * KSTEP + FK * gg + e;
      v[e] = (ci < p.Cin && kw < 7) ? p.w[(((size_t)co * p.Cin + ci) * R + kh) * 7 + kw] : 0.f;
    }
    wl[idx] = pack16<T>(v);
  }
  __syncthreads();

  const T* dy = (const T*)p.dy;
  for (long s = (long)blockIdx.x * 4 + wv; s < p.nstrips; s += (long)gridDim.x * 4) {
    const int sc = (int)(s % p.strips_w);
    const int tr = (int)((s / p.strips_w) % p.strips_h);
    const int img = (int)(s / ((long)p.strips_w * p.strips_h));
    const int pr0 = TWO_D ? UR * tr - 1 : 0, pc0 = SD_STRIP_W * sc - 1;
    const int h0 = TWO_D ? 2 * UR * tr : 0, w0 = 2 * SD_STRIP_W * sc;
    // ---- the strip's dy values: B fragments (column = position li of the row, K = output channels)
    u32x4 fb[PR][NKS];
    {
      const int ow = pc0 + li;
      const bool okw = ow >= 0 && ow < p.OW;
#pragma unroll
      for (int r = 0; r < PR; ++r) {
        const int oh = pr0 + r;
        const bool ok = okw && oh >= 0 && oh < p.OH;
        const T* src = dy + (((size_t)img * p.OH + (ok ? oh : 0)) * p.OW + (ok ? ow : 0)) * 64 + FK * g;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
          u32x4 v = {0u, 0u, 0u, 0u};
          if (ok) v = *reinterpret_cast<const u32x4*>(src + ks * KSTEP);
          fb[r][ks] = v;
        }
      }
    }
#pragma unroll
    for (int eh = 0; eh < NEH; ++eh) {
      const int nth = TWO_D ? 3 + eh : 1;   // (compile-time after unrolling)
      for (int nb = 0; nb < p.nbw; ++nb) {
        u32x4 fa[4][NKS];
        const u32x4* wsrc = wl + ((size_t)(eh ? frags0 : 0) + (size_t)nb * nth * NKS) * 64 + lane;
#pragma unroll
        for (int th = 0; th < 4; ++th)
#pragma unroll
          for (int ks = 0; ks < NKS; ++ks)
            if (th < nth) fa[th][ks] = wsrc[(th * NKS + ks) * 64];
#pragma unroll
        for (int r = 0; r < UR; ++r) {
          f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int th = 0; th < 4; ++th) {
            if (th < nth) {
#pragma unroll
              for (int ks = 0; ks < NKS; ++ks) acc = SdMma<T>::run(acc, fa[th][ks], fb[r + nth - 1 - th][ks]);
            }
          }
          // D[row = 4 g + j][col = li] -> Z[r][column 4 g + j][position li]
#pragma unroll
          for (int j = 0; j < 4; ++j) zw[(r * 16 + 4 * g + j) * 16 + li] = acc[j];
        }
        wave_lds_sync();
        // ---- gather along w: lanes 0-31 take the block's first input channel, 32-63 its second; 26 pixels per row
        {
          const int half = lane >> 5, pl = lane & 31;
          const int ci = nb * 2 + half;
          const int e = pl & 1, c = pl >> 1;
          const int w = w0 + pl;
          const bool okp = pl < 2 * SD_STRIP_W && w < p.W && ci < p.Cin;
          // tap tw: kw = 2 tw + 1 - e at position c + 2 + e - tw  (tw < 3 + e)
          const float* zb = zw + (half * 8 + 1 - e) * 16 + c + 2 + e;
          float* dst = p.dx + (((size_t)img * p.Cin + (ci < p.Cin ? ci : 0)) * p.H) * p.W + w;
#pragma unroll
          for (int r = 0; r < UR; ++r) {
            const int h = h0 + 2 * r + eh;
            float v = 0.f;
            if (okp) {
              const float* z = zb + r * 256;
              v = z[0] + z[2 * 16 - 1] + z[4 * 16 - 2];
              if (e) v += z[6 * 16 - 3];
              if (h < p.H) dst[(size_t)h * p.W] = v;
            }
          }
        }
        wave_lds_sync();
      }
    }
  }
}

template <typename T, bool TWO_D, int PR>
int stem_dgrad_launch(const StemDgradParams& p0, hipStream_t stream) {
  StemDgradParams p = p0;
  constexpr int FK = 16 / sizeof(T), NKS = 64 / (4 * FK);
  constexpr int UR = TWO_D ? PR - 3 : 1;
  p.nbw = (p.Cin + 1) / 2;
  p.strips_w = ceil_div(p.W, 2 * SD_STRIP_W);
  p.strips_h = TWO_D ? ceil_div(p.H, 2 * UR) : 1;
  p.nstrips = (long)p.N * p.strips_w * p.strips_h;
  const int nfrags = p.nbw * (TWO_D ? 7 : 1) * NKS;
  const size_t lds = (size_t)nfrags * 64 * 16 + (size_t)4 * UR * 256 * sizeof(float);
  if (lds > 160 * 1024) ECG_FAIL(ECGMM_ERR_SHAPE, "stem_bwd_data: Cin=%d needs %zu bytes of LDS", p.Cin, lds);
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)stem_dgrad_kernel<T, TWO_D, PR>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024);
    attr_set = true;
  }
  // persistent workgroups: two per CU where the LDS allows it
  long grid = (p.nstrips + 3) / 4;
  if (grid > 512) grid = 512;
  hipLaunchKernelGGL((stem_dgrad_kernel<T, TWO_D, PR>), dim3((unsigned)grid), dim3(SD_THREADS), lds, stream, p);
  ECG_CHECK_LAUNCH("stem_bwd_data");
  return 0;
}

}  // namespace

// R = 7: the 2-D stem (7x7); R = 1: the 1-D stem (1x7, H = 1).  w = the fp32 master weights [64][Cin][R][7].
int ecg_stem_dgrad(int dtype, const void* dy, const float* w, float* dx, int N, int Cin, int H, int W, int R,
                   hipStream_t stream) {
  if (R != 7 && R != 1) ECG_FAIL(ECGMM_ERR_SHAPE, "stem_bwd_data: R=%d (7 or 1)", R);
  if (R == 1 && H != 1) ECG_FAIL(ECGMM_ERR_SHAPE, "stem_bwd_data: R=1 needs H=1, got %d", H);
  if (N < 1 || Cin < 1 || H < 1 || W < 1) ECG_FAIL(ECGMM_ERR_SHAPE, "stem_bwd_data: bad shape %dx%dx%dx%d", N, Cin, H, W);
  if (!dy || !w || !dx) ECG_FAIL(ECGMM_ERR_SHAPE, "stem_bwd_data: null pointer");
  StemDgradParams p;
  memset(&p, 0, sizeof(p));
  p.dy = dy; p.w = w; p.dx = dx; p.N = N; p.Cin = Cin; p.H = H; p.W = W;
  p.OH = R == 7 ? (H + 6 - 7) / 2 + 1 : 1;
  p.OW = (W + 6 - 7) / 2 + 1;
  if (p.OW < 1 || p.OH < 1) ECG_FAIL(ECGMM_ERR_SHAPE, "stem_bwd_data: input %dx%d smaller than the kernel", H, W);
  if (dtype == ECGMM_BF16) {
    return R == 7 ? stem_dgrad_launch<bf16_t, true, 16>(p, stream) : stem_dgrad_launch<bf16_t, false, 1>(p, stream);
  } else if (dtype == ECGMM_F32) {
    return R == 7 ? stem_dgrad_launch<float, true, 7>(p, stream) : stem_dgrad_launch<float, false, 1>(p, stream);
  }
  ECG_FAIL(ECGMM_ERR_DTYPE, "stem_bwd_data: bad dtype %d", dtype);
}
