// resample_signal of the PhysioNet-2017 front end (train_physionet.py:35-39): scipy.signal.resample(x, num), the Fourier
// method, for a whole [S][L] fp32 matrix.  fp64 arithmetic, fp32 result, as the other two steps of that path (physionet.hip).
//   X[k] = sum_n x[n] e^{-2 pi i k n / N},  k < K = m / 2 + 1,  m = min(N, num)                      (analysis)
//   y[j] = (X[0] + sum_{1 <= k < K} w_k 2 Re(X[k] e^{+2 pi i k j / num})) / N                         (synthesis)
//   w_k = 1 except at k = m / 2 with m even: the term is 2 Re X[k] (-1)^j when num < N (the two aliased bins fold onto the
//   output's Nyquist bin) and Re X[k] cos(2 pi k j / num) when num > N (the input's Nyquist bin is halved).
// Both stages are direct sums: the cost is paid once per dataset and every term's error can be written down.
// The phase k n mod N is carried as an integer r (one add and one conditional subtract per term), and the twiddle
// e^{-+2 pi i r / N} is the product of two table entries, T1[r >> 8] T0[r & 255], r = 256 a + b < N <= 65536.  Each workgroup
// builds the two 256-entry tables of its row in LDS with sincospi on an argument reduced in integers to [0, 1/4].
// Every sum runs in ascending n (or k) in one thread: no atomics, nothing depends on S, on L or on the grid.
#include "ops.h"

namespace {

constexpr int RS_THREADS = 256;     // threads of a workgroup = bins (analysis) or outputs (synthesis) of a chunk = entries of a table
constexpr int RS_MAX = 65536;       // largest N and num: r = 256 a + b < 65536 keeps a and b below 256

struct RsParams {
  const float* x;      // [S][L]
  const int* lengths;  // [S] or null
  float* out;          // [S][T_out]
  int* out_lengths;    // [S] or null
  double2* X;          // [S][Kmax] workspace
  int S, L, T_out, Kmax;
  int num;             // without lengths: every row L -> num
  double ratio;        // with lengths: row s goes N_s -> (int)((double)N_s * ratio)
  int kchunks, jchunks;
};

// e^{sign 2 pi i p / N} for 0 <= p < N.  4 p = q N + rem splits off the quadrant in integers; a remainder beyond half a
// quadrant is taken from the next quadrant boundary backwards, so sincospi sees rem / (2 N) in [0, 1/4] (one rounding, of
// the division) and quarter turns come out exact.
__device__ __forceinline__ double2 rs_unit_root(int p, int N, int sign) {
  const long long t = 4LL * p;
  int q = (int)(t / N);
  long long rem = t - (long long)q * N;
  const bool back = 2 * rem > N;
  if (back) { rem = N - rem; q += 1; }
  double s, c;
  sincospi((double)rem / (double)(2LL * N), &s, &c);
  if (back) s = -s;
  double re, im;
  switch (q & 3) {
    case 0: re = c; im = s; break;
    case 1: re = -s; im = c; break;
    case 2: re = -c; im = -s; break;
    default: re = s; im = -c; break;
  }
  return make_double2(re, sign < 0 ? -im : im);
}

// the two tables of e^{sign 2 pi i r / N}: lo[b] for r = b, hi[a] for r = 256 a (indices that no r < N reaches are reduced mod N)
__device__ __forceinline__ void rs_build_tables(double2* lo, double2* hi, int N, int sign) {
  const int t = threadIdx.x;
  lo[t] = rs_unit_root(t % N, N, sign);
  hi[t] = rs_unit_root((int)((256LL * t) % N), N, sign);
}

__device__ __forceinline__ double2 rs_twiddle(const double2* lo, const double2* hi, int r) {
  const double2 a = hi[r >> 8], b = lo[r & 255];
  return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

// (N_s, num_s) of row s, both inside the buffers: lengths clamped to [0, L], num_s to [0, T_out]
__device__ __forceinline__ void rs_row_shape(const RsParams& p, int s, int& N, int& num) {
  if (p.lengths) {
    N = min(max(p.lengths[s], 0), p.L);
    num = min(max((int)((double)N * p.ratio), 0), p.T_out);
  } else {
    N = p.L;
    num = p.num;
  }
}

// grid: S * kchunks workgroups; thread t of chunk c owns bin k = 256 c + t and walks the row in ascending n
__global__ __launch_bounds__(RS_THREADS) void resample_analysis_kernel(RsParams p) {
  __shared__ double2 lo[RS_THREADS], hi[RS_THREADS];
  __shared__ double xs[RS_THREADS];
  const int s = blockIdx.x / p.kchunks, k0 = (blockIdx.x % p.kchunks) * RS_THREADS;
  int N, num;
  rs_row_shape(p, s, N, num);
  if (N < 1 || num < 1 || num == N) return;       // zeros / the copy: the synthesis kernel reads no X
  const int K = min(N, num) / 2 + 1;
  if (k0 >= K) return;
  rs_build_tables(lo, hi, N, -1);
  const int k = k0 + threadIdx.x;
  const bool live = k < K;
  const int step = live ? k : 0;                  // k <= N / 2 < N (N = 1: k = 0)
  const float* xr = p.x + (size_t)s * p.L;
  double re = 0.0, im = 0.0;
  int r = 0;
  for (int n0 = 0; n0 < N; n0 += RS_THREADS) {
    __syncthreads();                              // the tables on the first trip, the previous tile's readers after it
    const int n = n0 + threadIdx.x;
    xs[threadIdx.x] = n < N ? (double)xr[n] : 0.0;   // x at and beyond N_s is never read
    __syncthreads();
    const int cnt = min(RS_THREADS, N - n0);
    for (int i = 0; i < cnt; ++i) {
      const double2 w = rs_twiddle(lo, hi, r);
      const double v = xs[i];
      re = fma(v, w.x, re);
      im = fma(v, w.y, im);
      r += step;
      if (r >= N) r -= N;
    }
  }
  if (live) p.X[(size_t)s * p.Kmax + k] = make_double2(re, im);
}

// grid: S * jchunks workgroups; thread t of chunk c owns output j = 256 c + t and walks the bins in ascending k
__global__ __launch_bounds__(RS_THREADS) void resample_synthesis_kernel(RsParams p) {
  __shared__ double2 lo[RS_THREADS], hi[RS_THREADS];
  __shared__ double2 Xs[RS_THREADS];
  const int s = blockIdx.x / p.jchunks, j0 = (blockIdx.x % p.jchunks) * RS_THREADS;
  int N, num;
  rs_row_shape(p, s, N, num);
  const int j = j0 + threadIdx.x;
  float* orow = p.out + (size_t)s * p.T_out;
  if (p.out_lengths && blockIdx.x % p.jchunks == 0 && threadIdx.x == 0) p.out_lengths[s] = N < 1 ? 0 : num;
  if (N < 1 || num < 1 || j0 >= num) {            // an empty row, or a chunk wholly behind the row's end
    if (j < p.T_out) orow[j] = 0.f;
    return;
  }
  if (num == N) {                                 // equal lengths: the row itself, bit for bit
    if (j < p.T_out) orow[j] = j < num ? p.x[(size_t)s * p.L + j] : 0.f;
    return;
  }
  const int m = min(N, num), K = m / 2 + 1;
  const int Kg = (m & 1) ? K : K - 1;             // bins 1 .. Kg - 1 take the general term
  rs_build_tables(lo, hi, num, +1);
  const bool live = j < num;
  const int step = live ? j : 0;
  const double2* Xr = p.X + (size_t)s * p.Kmax;
  double acc = 0.0;
  int r = step;                                   // k j mod num at k = 1
  for (int kb = 1; kb < Kg; kb += RS_THREADS) {
    __syncthreads();
    const int kk = kb + threadIdx.x;
    Xs[threadIdx.x] = kk < Kg ? Xr[kk] : make_double2(0.0, 0.0);
    __syncthreads();
    const int cnt = min(RS_THREADS, Kg - kb);
    for (int i = 0; i < cnt; ++i) {
      const double2 w = rs_twiddle(lo, hi, r);
      const double2 v = Xs[i];
      acc = fma(v.x, w.x, acc);
      acc = fma(-v.y, w.y, acc);
      r += step;
      if (r >= num) r -= num;
    }
  }
  __syncthreads();                                // the tables when the loop above ran no trip
  double sum = Xr[0].x + 2.0 * acc;
  if (!(m & 1)) {
    const double xn = Xr[K - 1].x;                // Re X[m / 2]; r = (m / 2) j mod num here
    if (num < N) sum += (j & 1) ? -2.0 * xn : 2.0 * xn;
    else sum = fma(xn, rs_twiddle(lo, hi, r).x, sum);
  }
  if (j < p.T_out) orow[j] = live ? (float)(sum / (double)N) : 0.f;
}

// 0 with the message set for a refused shape
size_t rs_workspace(const char* who, int S, int L, int T_out) {
  if (S < 1 || L < 1 || T_out < 1 || L > RS_MAX || T_out > RS_MAX) {
    ecg_set_error("%s: need S >= 1 and 1 <= L, T_out <= %d (S=%d L=%d T_out=%d)", who, RS_MAX, S, L, T_out);
    return 0;
  }
  return (size_t)S * (size_t)(min(L, T_out) / 2 + 1) * sizeof(double2);
}

}  // namespace

extern "C" int ecgmm_signal_resample_len(int n, double ratio) {
  if (n < 0 || !(ratio > 0.0) || !(ratio <= 1.7976931348623157e308)) {
    ecg_set_error("signal_resample_len: need n >= 0 and a finite ratio > 0 (n=%d ratio=%g)", n, ratio);
    return -1;
  }
  const double v = (double)n * ratio;
  if (!(v < 2147483648.0)) {
    ecg_set_error("signal_resample_len: %d samples at ratio %g give more than an int holds", n, ratio);
    return -1;
  }
  return (int)v;
}

extern "C" size_t ecgmm_signal_resample_workspace(int S, int L, int T_out) {
  return rs_workspace("signal_resample_workspace", S, L, T_out);
}

extern "C" int ecgmm_signal_resample(const float* x, int S, int L, const int32_t* lengths, int num, double ratio, float* out,
                                     int T_out, int32_t* out_lengths, void* ws, size_t ws_bytes, void* stream) {
  if (!x || !out || !ws) ECG_FAIL(ECGMM_ERR_SHAPE, "signal_resample: null operand");
  const size_t need = rs_workspace("signal_resample", S, L, T_out);
  if (need == 0) return ECGMM_ERR_SHAPE;
  if (lengths) {
    if (num != 0) ECG_FAIL(ECGMM_ERR_SHAPE, "signal_resample: with lengths every row has its own num, pass num = 0 (num=%d)", num);
    if (!(ratio > 0.0) || !(ratio <= 1.7976931348623157e308))
      ECG_FAIL(ECGMM_ERR_SHAPE, "signal_resample: ratio %g must be finite and > 0", ratio);
    const double top = (double)L * ratio;
    if (!(top < (double)RS_MAX + 1.0) || T_out < (int)top)
      ECG_FAIL(ECGMM_ERR_SHAPE, "signal_resample: a row of L=%d samples at ratio %g gives %.0f samples, T_out=%d (limit %d)", L,
               ratio, top < 4e9 ? (double)(long long)top : top, T_out, RS_MAX);
  } else {
    if (out_lengths) ECG_FAIL(ECGMM_ERR_SHAPE, "signal_resample: out_lengths needs lengths");
    if (num < 1 || num > T_out) ECG_FAIL(ECGMM_ERR_SHAPE, "signal_resample: need 1 <= num <= T_out (num=%d T_out=%d)", num, T_out);
  }
  if (ws_bytes < need)
    ECG_FAIL(ECGMM_ERR_SHAPE, "signal_resample: workspace of %zu bytes, %zu needed (ecgmm_signal_resample_workspace)", ws_bytes, need);
  if (((uintptr_t)ws) & 15) ECG_FAIL(ECGMM_ERR_SHAPE, "signal_resample: the workspace must be 16-byte aligned");
  RsParams p;
  memset(&p, 0, sizeof(p));
  p.x = x; p.lengths = lengths; p.out = out; p.out_lengths = out_lengths; p.X = (double2*)ws;
  p.S = S; p.L = L; p.T_out = T_out; p.Kmax = min(L, T_out) / 2 + 1;
  p.num = num; p.ratio = ratio;
  p.kchunks = ceil_div(p.Kmax, RS_THREADS);
  p.jchunks = ceil_div(T_out, RS_THREADS);
  const long long ga = (long long)S * p.kchunks, gs = (long long)S * p.jchunks;
  if (ga > 0x7fffffffLL || gs > 0x7fffffffLL)
    ECG_FAIL(ECGMM_ERR_SHAPE, "signal_resample: S=%d rows need %lld workgroups, more than one launch takes", S, ga > gs ? ga : gs);
  hipStream_t st = (hipStream_t)stream;
  const bool copy_only = !lengths && num == L;
  if (!copy_only) hipLaunchKernelGGL(resample_analysis_kernel, dim3((unsigned)ga), dim3(RS_THREADS), 0, st, p);
  hipLaunchKernelGGL(resample_synthesis_kernel, dim3((unsigned)gs), dim3(RS_THREADS), 0, st, p);
  ECG_CHECK_LAUNCH("signal_resample");
  return 0;
}
