// Log-spectrogram of train_physionet2.py:30-34: np.log1p(np.abs(scipy.signal.stft(x, window, nperseg=64, noverlap)))
// for a whole zero-padded [S][L] matrix in one launch (boundary='zeros', padded=True, one-sided, scaling='spectrum').
//   Z[k][t] = sum_j table[k][j] * x[hop*t - 32 + j],   table[k][j] = w[j] / sum(w) * (cos, -sin)(2 pi j k / 64),
//   out[s][k][t] = log1p(|Z[k][t]|),   k = 0..32,  t = 0..T-1,  T = ceil(L / hop) + 1,  x = 0 outside [0, L).
// The table comes from the host (ecgmm/spectrogram.py builds it in float64), so the kernel evaluates no sin / cos and
// knows nothing about windows.  A direct DFT on the vector ALU: 2 * 64 * 66 flop per frame against 4 * 33 bytes written.
#include "ops.h"

namespace {

constexpr int SG_NPERSEG = 64, SG_BINS = 33, SG_FRAMES = 64, SG_WAVES = 4;
// samples of one tile at the largest hop, in the padded image below
constexpr int SG_TILE = (SG_FRAMES - 1) * 64 + SG_NPERSEG;
constexpr int SG_LDS = SG_TILE + SG_TILE / 32;

struct SgShape {
  int S, L, T, hop, tiles;
};

// Sample i of the tile sits at LDS dword i + i / 32: at hop 32 lane t starts at dword 33 t, so the 64 lanes' reads of their
// j-th sample fall in distinct banks (the unpadded stride of 32 dwords would put all of them on one).
__device__ __forceinline__ int sg_at(int i) { return i + (i >> 5); }

// One workgroup = one record and 64 consecutive frames.  Lanes run along t, the four waves share the 33 bins (k = wave,
// wave + 4, ...): every wave keeps its lane's 64 samples in registers and streams the table rows, whose address is the same
// in all lanes.  Each output row segment is 64 consecutive floats.  The sum over j runs in one fixed order: no atomics,
// nothing depends on S or on the grid.  x [S][L], table [33][64][2], out [S][33][T]; the pointers are __restrict__ so that
// the table reads, which no store of this kernel can touch, may go through the scalar cache into SGPR operands.
__global__ __launch_bounds__(SG_WAVES * 64) void log_spectrogram_kernel(const float* __restrict__ xin,
                                                                        const float* __restrict__ table,
                                                                        float* __restrict__ out, SgShape p) {
  __shared__ float xs[SG_LDS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int s = blockIdx.x / p.tiles, t0 = (blockIdx.x % p.tiles) * SG_FRAMES;
  const int hop = p.hop, L = p.L;
  const float* xr = xin + (size_t)s * L;
  const long long g0 = (long long)hop * t0 - SG_NPERSEG / 2;   // record index of the tile's first sample
  const int n = (SG_FRAMES - 1) * hop + SG_NPERSEG;            // <= SG_TILE
  for (int i = tid; i < n; i += SG_WAVES * 64) {
    const long long g = g0 + i;
    xs[sg_at(i)] = (g >= 0 && g < L) ? xr[g] : 0.f;            // boundary='zeros' in front, the zero tail behind
  }
  __syncthreads();

  float x[SG_NPERSEG];
  const int b = hop * lane;
#pragma unroll
  for (int j = 0; j < SG_NPERSEG; ++j) x[j] = xs[sg_at(b + j)];

  const int t = t0 + lane;
  for (int k = wave; k < SG_BINS; k += SG_WAVES) {
    const float2* tk = reinterpret_cast<const float2*>(table) + k * SG_NPERSEG;
    float re = 0.f, im = 0.f;
#pragma unroll
    for (int j = 0; j < SG_NPERSEG; ++j) {
      const float2 c = tk[j];
      re = fmaf(x[j], c.x, re);
      im = fmaf(x[j], c.y, im);
    }
    if (t < p.T) out[((size_t)s * SG_BINS + k) * p.T + t] = log1pf(sqrtf(re * re + im * im));   // zero frame: exactly 0
  }
}

// T(L) = ceil(L / hop) + 1, or 0 with the message set
int sg_frames(const char* who, int L, int nperseg, int hop) {
  if (nperseg != SG_NPERSEG) {
    ecg_set_error("%s: nperseg %d is not supported (the kernel is built for nperseg 64 = 33 bins)", who, nperseg);
    return 0;
  }
  if (hop < 1 || hop > nperseg) {
    ecg_set_error("%s: hop %d outside 1..%d (hop = nperseg - noverlap)", who, hop, nperseg);
    return 0;
  }
  if (L < nperseg) {
    ecg_set_error("%s: record length %d is shorter than nperseg %d (scipy would shrink the window; refused here)", who, L,
                  nperseg);
    return 0;
  }
  const long long T = ((long long)L + hop - 1) / hop + 1;
  if (T > 0x7fffffffLL) {
    ecg_set_error("%s: record length %d at hop %d gives %lld frames, more than an int holds", who, L, hop, T);
    return 0;
  }
  return (int)T;
}

}  // namespace

extern "C" int ecgmm_log_spectrogram_frames(int L, int nperseg, int hop) {
  return sg_frames("log_spectrogram_frames", L, nperseg, hop);
}

extern "C" int ecgmm_log_spectrogram(const float* x, int S, int L, const float* table, int nperseg, int hop, float* out,
                                     int T, void* stream) {
  const int frames = sg_frames("log_spectrogram", L, nperseg, hop);
  if (frames == 0) return ECGMM_ERR_SHAPE;
  if (T != frames)
    ECG_FAIL(ECGMM_ERR_SHAPE, "log_spectrogram: T=%d but a record of %d samples at hop %d has %d frames", T, L, hop, frames);
  if (!x || !table || !out) ECG_FAIL(ECGMM_ERR_SHAPE, "log_spectrogram: null operand");
  if (S < 1) ECG_FAIL(ECGMM_ERR_SHAPE, "log_spectrogram: need S >= 1 (S=%d)", S);
  SgShape p;
  p.S = S; p.L = L; p.T = T; p.hop = hop;
  p.tiles = ceil_div(T, SG_FRAMES);
  const long long blocks = (long long)S * p.tiles;
  if (blocks > 0x7fffffffLL)
    ECG_FAIL(ECGMM_ERR_SHAPE, "log_spectrogram: S=%d records of %d frames need %lld workgroups, more than one launch takes",
             S, T, blocks);
  hipLaunchKernelGGL(log_spectrogram_kernel, dim3((unsigned)blocks), dim3(SG_WAVES * 64), 0, (hipStream_t)stream, x, table, out,
                     p);
  ECG_CHECK_LAUNCH("log_spectrogram");
  return 0;
}
