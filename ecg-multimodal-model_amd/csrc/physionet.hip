// PhysioNet-2017 single-lead path (train_physionet.py:22-86, train_physionet_multi.py:20-64), the two steps in front of
// ResNet1D_SE that the reference runs per sample on the CPU at every __getitem__:
//   signal_filter_zscore  -- scipy.signal.filtfilt(b, a, x) (odd padding 3*(n+1), lfilter_zi initial state) followed by
//                            (x - mean) / (std + eps) over the record, for a whole [S][L] matrix in one launch.
//                            fp64 arithmetic (the reference computes in float64; the band-pass has poles at radius 0.992),
//                            fp32 result.  Same structure as signal_preprocess_lds_kernel (preprocess.hip): one wave per
//                            record, the odd-extended record resident in LDS, the time axis cut into 64 odd-length chunks.
//   signal_gather_augment -- out[i] = augment(src[index[i]]): the batch gather fused with augment_signal
//                            (noise N(0, sigma^2) -> scale U[lo, hi) -> circular roll), Philox4x32-10 as in head.hip.
//   weighted_sample       -- WeightedRandomSampler(weights, count, replacement=True) = torch.multinomial with replacement
//                            (train_signal_only_ptb.py:230-235,241): one epoch's indices in one launch.
#include "ops.h"

namespace {

// ------------------------------------------------------------------------------------------------
// filtfilt + z-score
// ------------------------------------------------------------------------------------------------
struct FzParams {
  const float* x;   // [S][L]
  float* out;       // [S][L]
  int S, L, zscore;
  int nl;           // lanes that run the recurrences (ecg_iir_lanes): 64, 32, .., 2, or 1 = the sequential pass
  double eps;
  double b[9], a[9], zi[8];
};

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// The IIR recurrence z' = A z + B x is linear, so the time axis is cut into 64 chunks of C samples:
//   (1) every lane filters its chunk from a ZERO state and keeps only the final state s_t;
//   (2) lane 0 chains the true chunk-entry states  z_{t+1} = A^C z_t + s_t  (A^C built once by lanes 0..N-1);
//   (3) every lane re-filters its chunk from its true entry state, writing y in place.
// C is odd, so the 64 lanes' cursors (stride C doubles) fall in distinct LDS banks.  Both directions run in place.
// As in signal_preprocess_lds_kernel only p.nl lanes run the recurrences (C = ceil(E / nl) | 1): the chain is exact only
// algebraically, and ecg_iir_lanes keeps its rounding under the fp32 result's.  nl = 1 is the sequential pass, without A^C; the
// lanes >= nl help with the loads, the extension, the z-score and the stores.
template <int N>
__global__ __launch_bounds__(64) void signal_filter_zscore_kernel(FzParams p) {
  extern __shared__ double sm[];
  constexpr int T = 64, PAD = 3 * (N + 1);
  const int L = p.L, E = L + 2 * PAD;
  const int lane = threadIdx.x, s = blockIdx.x;
  double* B = sm;            // [E]     odd-extended record; filtered in place
  double* st = B + E;        // [T][8]  chunk states
  double* Mx = st + T * 8;   // [8][8]  A^C, row-major
  double b[N + 1], a[N + 1];
#pragma unroll
  for (int i = 0; i <= N; ++i) { b[i] = p.b[i]; a[i] = p.a[i]; }

  const float* xr = p.x + (size_t)s * L;
  for (int t = lane; t < L; t += T) B[PAD + t] = (double)xr[t];
  const int nl = p.nl;
  const int C = ((E + nl - 1) / nl) | 1;
  if (lane < N && nl > 1) {  // column `lane` of A^C: C zero-input steps from the unit state
    double z[N];
#pragma unroll
    for (int i = 0; i < N; ++i) z[i] = i == lane ? 1.0 : 0.0;
    for (int k = 0; k < C; ++k) {
      const double y = z[0];
#pragma unroll
      for (int i = 0; i < N - 1; ++i) z[i] = z[i + 1] - a[i + 1] * y;
      z[N - 1] = -a[N] * y;
    }
#pragma unroll
    for (int i = 0; i < N; ++i) Mx[i * 8 + lane] = z[i];
  }
  __syncthreads();
  if (lane < PAD) {  // odd extension about both ends (PAD <= 27 < 64, and the host checks L > PAD)
    B[lane] = 2.0 * B[PAD] - B[PAD + (PAD - lane)];
    B[PAD + L + lane] = 2.0 * B[PAD + L - 1] - B[PAD + L - 2 - lane];
  }
  __syncthreads();

  const int k0 = lane < nl ? min(E, lane * C) : E, k1 = min(E, k0 + C);   // lanes >= nl own no chunk
#pragma unroll 1
  for (int pass = 0; pass < 2; ++pass) {
    auto at = [&](int k) -> double& { return B[pass ? E - 1 - k : k]; };
    double z[N];
    if (nl > 1 && k0 < E && k1 - k0 == C) {  // a full chunk hands a state on
#pragma unroll
      for (int i = 0; i < N; ++i) z[i] = 0.0;
      for (int k = k0; k < k1; ++k) {
        const double e = at(k);
        const double y = b[0] * e + z[0];
#pragma unroll
        for (int i = 0; i < N - 1; ++i) z[i] = b[i + 1] * e + z[i + 1] - a[i + 1] * y;
        z[N - 1] = b[N] * e - a[N] * y;
      }
#pragma unroll
      for (int i = 0; i < N; ++i) st[lane * 8 + i] = z[i];
    } else {
#pragma unroll
      for (int i = 0; i < N; ++i) st[lane * 8 + i] = 0.0;   // never handed on; keeps the chain free of stale LDS
    }
    __syncthreads();
    if (lane == 0) {
      const double e0 = at(0);
      double m[N][N];
#pragma unroll
      for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = 0; j < N; ++j) m[i][j] = Mx[i * 8 + j];
#pragma unroll
      for (int i = 0; i < N; ++i) z[i] = p.zi[i] * e0;
      const int nchunks = nl > 1 ? (E + C - 1) / C : 0;   // <= nl
      if (nl == 1) {
#pragma unroll
        for (int i = 0; i < N; ++i) st[i] = z[i];
      }
      for (int t = 0; t < nchunks; ++t) {
        double sv[N], zn[N];
#pragma unroll
        for (int i = 0; i < N; ++i) { sv[i] = st[t * 8 + i]; st[t * 8 + i] = z[i]; }
#pragma unroll
        for (int i = 0; i < N; ++i) {
          double acc = sv[i];
#pragma unroll
          for (int j = 0; j < N; ++j) acc += m[i][j] * z[j];
          zn[i] = acc;
        }
#pragma unroll
        for (int i = 0; i < N; ++i) z[i] = zn[i];
      }
    }
    __syncthreads();
    if (k0 < E) {
#pragma unroll
      for (int i = 0; i < N; ++i) z[i] = st[lane * 8 + i];
      for (int k = k0; k < k1; ++k) {
        double& r = at(k);
        const double e = r;
        const double y = b[0] * e + z[0];
#pragma unroll
        for (int i = 0; i < N - 1; ++i) z[i] = b[i + 1] * e + z[i + 1] - a[i + 1] * y;
        z[N - 1] = b[N] * e - a[N] * y;
        r = y;
      }
    }
    __syncthreads();
  }
  // z_score_normalize over the resident record: mean, then the sum of squared deviations (two passes, no cancellation)
  const double* y = B + PAD;
  double mean = 0.0, den = 1.0;
  if (p.zscore) {
    double acc = 0.0;
    for (int t = lane; t < L; t += T) acc += y[t];
    mean = wave_sum_f64(acc) / (double)L;
    double q = 0.0;
    for (int t = lane; t < L; t += T) {
      const double d = y[t] - mean;
      q += d * d;
    }
    den = sqrt(wave_sum_f64(q) / (double)L) + p.eps;   // np.std: population standard deviation
  }
  float* orow = p.out + (size_t)s * L;
  for (int t = lane; t < L; t += T) orow[t] = (float)(p.zscore ? (y[t] - mean) / den : y[t]);
}

constexpr size_t FZ_LDS_MAX = 160 * 1024;
inline size_t fz_lds_bytes(int L, int order) { return ((size_t)L + 6 * (order + 1) + 64 * 8 + 64) * sizeof(double); }

template <int N>
void launch_fz(const FzParams& p, size_t lds, hipStream_t st) {
  (void)hipFuncSetAttribute((const void*)signal_filter_zscore_kernel<N>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)FZ_LDS_MAX);
  hipLaunchKernelGGL(signal_filter_zscore_kernel<N>, dim3(p.S), dim3(64), lds, st, p);
}

// ------------------------------------------------------------------------------------------------
// gather + augment_signal
// ------------------------------------------------------------------------------------------------
// Philox4x32-10, the generator of dropout_fwd_kernel (head.hip).  Counter layout of this kernel:
//   c0, c1 = the call's 64-bit offset;  c2 = the row's position i within the call;
//   c3 = 0x80000000 | g  for the noise of output elements 4g .. 4g+3,  0xFFFFFFFF / 0xFFFFFFFE for the row's decisions.
// c3 is never 0, so no counter of this kernel coincides with one of the dropout stream (c2 = c3 = 0) under the same seed.
// weighted_sample_kernel: c0, c1 = the call's offset; c2 = the draw's position i; c3 = 0xFFFFFFFD, which is neither 0, nor a
// row decision, nor a noise group (g < 2^28 since L <= 2^30, so 0x80000000 | g <= 0x8FFFFFFF).
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

__device__ __forceinline__ float u01(unsigned w) { return (float)(w >> 8) * (1.f / 16777216.f); }   // [0, 1)

// Box-Muller on two words: two independent N(0, 1) deviates
__device__ __forceinline__ void box_muller(unsigned w0, unsigned w1, float& n0, float& n1) {
  const float u = ((float)(w0 >> 8) + 1.f) * (1.f / 16777216.f);   // (0, 1]: the logarithm stays finite
  const float r = sqrtf(-2.f * __logf(u));
  const float ang = 6.28318530717958647692f * u01(w1);
  n0 = r * __cosf(ang);
  n1 = r * __sinf(ang);
}

struct GaParams {
  const float* src;          // [n][L]
  const long long* index;    // [B]
  float* out;                // [B][L]
  float* dec;                // [B][4] or null
  long long n;
  int L, B, augment, vec;
  float p, sigma, scale_lo, scale_hi;
  int shift_lo, shift_n;     // shift uniform on shift_lo .. shift_lo + shift_n - 1
  unsigned long long seed, offset;
};

// grid (ceil(L / 1024), B): one row per blockIdx.y, four consecutive OUTPUT elements per thread.  The stores are the aligned,
// 16-byte side; the roll lands on the loads (four dword loads per thread, consecutive across the wave).
__global__ __launch_bounds__(256) void signal_gather_augment_kernel(GaParams p) {
  __shared__ float sh_scale;
  __shared__ int sh_flags, sh_shift;
  const int i = blockIdx.y, L = p.L;
  const unsigned o_lo = (unsigned)p.offset, o_hi = (unsigned)(p.offset >> 32);
  if (threadIdx.x == 0) {
    int flags = 0, shift = 0;
    float scale = 1.f;
    if (p.augment) {
      unsigned r[4], q[4];
      philox4(p.seed, o_lo, o_hi, (unsigned)i, 0xFFFFFFFFu, r);
      philox4(p.seed, o_lo, o_hi, (unsigned)i, 0xFFFFFFFEu, q);
      flags = (u01(r[0]) < p.p ? 1 : 0) | (u01(r[1]) < p.p ? 2 : 0) | (u01(r[2]) < p.p ? 4 : 0);
      if (flags & 2) {
        scale = p.scale_lo + u01(q[0]) * (p.scale_hi - p.scale_lo);
        if (scale >= p.scale_hi) scale = p.scale_lo;   // the fp32 rounding of the last step may reach the open end
      }
      if (flags & 4) shift = p.shift_lo + (int)__umulhi(q[1], (unsigned)p.shift_n);
    }
    sh_flags = flags; sh_scale = scale; sh_shift = shift;
    if (p.dec && blockIdx.x == 0) {
      float* d = p.dec + (size_t)i * 4;
      d[0] = (float)(flags & 1); d[1] = scale; d[2] = (float)shift; d[3] = (float)flags;
    }
  }
  __syncthreads();
  const int flags = sh_flags, shift = sh_shift;
  const float scale = sh_scale;
  const int g = blockIdx.x * 256 + threadIdx.x, o = g * 4;
  if (o >= L) return;
  const long long row = p.index[i];
  const bool ok = row >= 0 && row < p.n;   // the host refuses such an index; a bad one never addresses memory
  const float* sr = p.src + (size_t)(ok ? row : 0) * L;
  int t = (o - shift) % L;                 // out[(t + shift) mod L] = v[t]
  if (t < 0) t += L;
  float v[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    int tj = t + j;
    if (tj >= L) tj -= L;
    v[j] = (o + j < L && ok) ? sr[tj] : __builtin_nanf("");
  }
  if (flags & 1) {
    unsigned r[4];
    float nz[4];
    philox4(p.seed, o_lo, o_hi, (unsigned)i, 0x80000000u | (unsigned)g, r);
    box_muller(r[0], r[1], nz[0], nz[1]);
    box_muller(r[2], r[3], nz[2], nz[3]);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] += p.sigma * nz[j];
  }
  if (flags & 2) {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] *= scale;
  }
  float* orow = p.out + (size_t)i * L;
  if (p.vec && o + 4 <= L) {
    *reinterpret_cast<float4*>(orow + o) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (o + j < L) orow[o + j] = v[j];
  }
}

// ------------------------------------------------------------------------------------------------
// sampling with replacement from a weight vector
// ------------------------------------------------------------------------------------------------
struct WsParams {
  const double* cdf;         // [n] inclusive prefix sum of the weights
  long long* out;            // [count]
  double* u_out;             // [count] or null
  long long n, count, last;  // last: the last index of positive weight
  unsigned long long seed, offset;
};

// One draw per thread: a 53-bit uniform from two Philox words, then the first j with cdf[j] > u * cdf[n-1] by binary search.
// cdf[j] > x >= cdf[j-1] makes weight j positive, so an index of weight 0 is never returned; when the product rounds up to
// cdf[n-1] itself no such j exists and the draw goes to `last`.  Every probe index lies in [0, n).
__global__ __launch_bounds__(256) void weighted_sample_kernel(WsParams p) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= p.count) return;
  unsigned r[4];
  philox4(p.seed, (unsigned)p.offset, (unsigned)(p.offset >> 32), (unsigned)i, 0xFFFFFFFDu, r);
  const double u = ((double)(r[0] >> 5) * 67108864.0 + (double)(r[1] >> 6)) * (1.0 / 9007199254740992.0);   // [0, 1)
  const double x = u * p.cdf[p.n - 1];
  long long lo = 0, hi = p.n;
  while (lo < hi) {
    const long long mid = lo + ((hi - lo) >> 1);
    if (p.cdf[mid] > x) hi = mid; else lo = mid + 1;
  }
  p.out[i] = lo < p.n ? lo : p.last;
  if (p.u_out) p.u_out[i] = u;
}

}  // namespace

extern "C" int ecgmm_weighted_sample(const double* cdf, int64_t n, int64_t last_positive, int64_t* out, double* u_out,
                                     int64_t count, uint64_t seed, uint64_t offset, void* stream) {
  if (!cdf || !out) ECG_FAIL(ECGMM_ERR_SHAPE, "weighted_sample: null operand");
  if (n < 1 || count < 1 || count > 0x7fffffffLL || last_positive < 0 || last_positive >= n)
    ECG_FAIL(ECGMM_ERR_SHAPE, "weighted_sample: need n >= 1, 1 <= count < 2^31, 0 <= last_positive < n (n=%lld count=%lld last=%lld)",
             (long long)n, (long long)count, (long long)last_positive);
  WsParams q;
  memset(&q, 0, sizeof(q));
  q.cdf = cdf; q.out = (long long*)out; q.u_out = u_out; q.n = n; q.count = count; q.last = last_positive;
  q.seed = seed; q.offset = offset;
  hipLaunchKernelGGL(weighted_sample_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, (hipStream_t)stream, q);
  ECG_CHECK_LAUNCH("weighted_sample");
  return 0;
}

extern "C" int ecgmm_signal_filter_zscore(const float* x, float* out, int S, int L, const double* b, const double* a,
                                          const double* zi, int order, int zscore, double eps, void* stream) {
  if (order < 1 || order > 8) ECG_FAIL(ECGMM_ERR_SHAPE, "signal_filter_zscore: filter order %d outside 1..8", order);
  if (!x || !out || !b || !a || !zi) ECG_FAIL(ECGMM_ERR_SHAPE, "signal_filter_zscore: null operand");
  if (S < 1 || L <= 3 * (order + 1))
    ECG_FAIL(ECGMM_ERR_SHAPE, "signal_filter_zscore: need S >= 1 and L > padlen = 3*(order+1) (S=%d L=%d order=%d)", S, L, order);
  if (a[0] != 1.0) ECG_FAIL(ECGMM_ERR_SHAPE, "signal_filter_zscore: a[0] must be 1 (normalised transfer function)");
  const size_t lds = fz_lds_bytes(L, order);
  if (lds > FZ_LDS_MAX)
    ECG_FAIL(ECGMM_ERR_SHAPE, "signal_filter_zscore: a record of %d samples does not fit one CU's LDS (largest L at order %d: %d)",
             L, order, (int)(FZ_LDS_MAX / sizeof(double)) - 6 * (order + 1) - 64 * 8 - 64);
  FzParams p;
  memset(&p, 0, sizeof(p));
  p.x = x; p.out = out; p.S = S; p.L = L; p.zscore = zscore ? 1 : 0; p.eps = eps;
  for (int i = 0; i <= order; ++i) { p.b[i] = b[i]; p.a[i] = a[i]; }
  for (int i = 0; i < order; ++i) p.zi[i] = zi[i];
  p.nl = ecg_iir_lanes(a, order, L + 6 * (order + 1));
  hipStream_t st = (hipStream_t)stream;
  switch (order) {
    case 1: launch_fz<1>(p, lds, st); break;
    case 2: launch_fz<2>(p, lds, st); break;
    case 3: launch_fz<3>(p, lds, st); break;
    case 4: launch_fz<4>(p, lds, st); break;
    case 5: launch_fz<5>(p, lds, st); break;
    case 6: launch_fz<6>(p, lds, st); break;
    case 7: launch_fz<7>(p, lds, st); break;
    default: launch_fz<8>(p, lds, st); break;
  }
  ECG_CHECK_LAUNCH("signal_filter_zscore");
  return 0;
}

extern "C" int ecgmm_signal_gather_augment(const float* src, int64_t n, int L, const int64_t* index, int B, float* out,
                                           float* decisions, int augment, float p, float sigma, float scale_lo,
                                           float scale_hi, int shift_lo, int shift_hi, uint64_t seed, uint64_t offset,
                                           void* stream) {
  if (!src || !index || !out) ECG_FAIL(ECGMM_ERR_SHAPE, "signal_gather_augment: null operand");
  if (n < 1 || L < 1 || B < 1 || B > 65535 || L > (1 << 30))
    ECG_FAIL(ECGMM_ERR_SHAPE, "signal_gather_augment: need n >= 1, 1 <= L <= 2^30, 1 <= B <= 65535 (n=%lld L=%d B=%d)",
             (long long)n, L, B);
  if (augment) {
    if (!(p >= 0.f && p <= 1.f) || !(sigma >= 0.f)) ECG_FAIL(ECGMM_ERR_SHAPE, "signal_gather_augment: p=%f sigma=%f", p, sigma);
    if (!(scale_lo > 0.f && scale_lo < scale_hi))
      ECG_FAIL(ECGMM_ERR_SHAPE, "signal_gather_augment: scale range [%f, %f) must be positive and non-empty", scale_lo, scale_hi);
    if (shift_lo >= shift_hi || shift_lo <= -L || shift_hi > L)
      ECG_FAIL(ECGMM_ERR_SHAPE, "signal_gather_augment: shift range [%d, %d) must be non-empty and inside (-L, L)", shift_lo, shift_hi);
  }
  GaParams q;
  memset(&q, 0, sizeof(q));
  q.src = src; q.index = (const long long*)index; q.out = out; q.dec = decisions; q.n = n; q.L = L; q.B = B;
  q.augment = augment ? 1 : 0;
  q.vec = (L % 4 == 0) && (((uintptr_t)out) & 15) == 0;
  q.p = p; q.sigma = sigma; q.scale_lo = scale_lo; q.scale_hi = scale_hi; q.shift_lo = shift_lo; q.shift_n = shift_hi - shift_lo;
  q.seed = seed; q.offset = offset;
  hipLaunchKernelGGL(signal_gather_augment_kernel, dim3(ceil_div(ceil_div(L, 4), 256), B), dim3(256), 0, (hipStream_t)stream, q);
  ECG_CHECK_LAUNCH("signal_gather_augment");
  return 0;
}
