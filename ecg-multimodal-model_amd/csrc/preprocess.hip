// On-device ECG signal pre-processing: the reference runs, per sample on CPU workers,
//   StandardScaler (per time column) -> 200-tap moving-average baseline removal (np.convolve 'same')
//   -> 5th-order Butterworth low-pass applied forward-backward (scipy.signal.filtfilt, odd padding of
//   3*(order+1) samples, steady-state initial conditions)          dataset.py:66-71,81-95;
//   train_signal_12_af.py:19-34 (same functions over [leads, time]).
// Two kernels: the LDS-resident chunk-parallel one below (one wave per signal, used whenever the padded
// record fits a CU's 160 KiB LDS -- every ECG length the reference uses), and a one-lane-per-signal
// kernel whose intermediates live transposed ([time][signal]) in a caller-owned fp64 workspace, for
// longer records.  All arithmetic in fp64 (the reference computes in float64), output fp32
// (the reference casts with torch.tensor(..., dtype=torch.float)).
#include "ops.h"

namespace {

struct PreParams {
  const float* x;          // [S][L]
  float* out;              // [S][L]
  const float* sc_mean;    // [L] or null
  const float* sc_scale;   // [L] or null
  double* ws;              // [L + E][S]
  int S, L, window, order;
  int nl;                  // lanes that run the recurrences (ecg_iir_lanes): 64, 32, .., 2, or 1 = the sequential pass
  double b[8], a[8], zi[8];
  // WFDB format-16 rows (ecgmm_signal_preprocess_i16): row s = (record s / nc, channel chan[s % nc]); L is then Lf
  const int16_t* raw;      // [R][T][nsig], the .dat payload
  const double* gain;      // [R][nc]
  const int* baseline;     // [R][nc]
  int T, nsig, nc, step, out_len;
  int chan[16];
};

__global__ __launch_bounds__(64) void signal_preprocess_kernel(PreParams p) {
  const int s = blockIdx.x * 64 + threadIdx.x;
  if (s >= p.S) return;
  const int L = p.L, S = p.S, M = p.window, N = p.order;
  const int PAD = 3 * (N + 1), E = L + 2 * PAD;
  double* u = p.ws + s;                    // u[t * S]: scaled, baseline-removed signal
  double* f = p.ws + (size_t)L * S + s;    // f[k * S]: forward-filtered padded signal
  const float* xr = p.x + (size_t)s * L;
  auto xs = [&](int t) -> double {
    double v = (double)xr[t];
    if (p.sc_mean) v = (v - (double)p.sc_mean[t]) / (double)p.sc_scale[t];
    return v;
  };
  // ---- moving-average baseline: np.convolve(x, ones(M)/M, 'same') = mean over [i - bk, i + fw]
  const int fw = (M - 1) / 2, bk = M - 1 - fw;
  double run = 0.0;
  for (int t = 0; t <= fw && t < L; ++t) run += xs(t);
  for (int i = 0; i < L; ++i) {
    u[(size_t)i * S] = xs(i) - run / (double)M;
    const int add = i + fw + 1, sub = i - bk;
    if (add < L) run += xs(add);
    if (sub >= 0) run -= xs(sub);
  }
  // ---- forward pass over the odd-extended signal (direct form II transposed, as scipy's lfilter)
  auto ext = [&](int k) -> double {
    if (k < PAD) return 2.0 * u[0] - u[(size_t)(PAD - k) * S];
    if (k < PAD + L) return u[(size_t)(k - PAD) * S];
    return 2.0 * u[(size_t)(L - 1) * S] - u[(size_t)(L - 2 - (k - PAD - L)) * S];
  };
  double z[8];
  const double e0 = ext(0);
  for (int i = 0; i < N; ++i) z[i] = p.zi[i] * e0;
  for (int k = 0; k < E; ++k) {
    const double e = ext(k);
    const double y = p.b[0] * e + z[0];
    for (int i = 0; i < N - 1; ++i) z[i] = p.b[i + 1] * e + z[i + 1] - p.a[i + 1] * y;
    z[N - 1] = p.b[N] * e - p.a[N] * y;
    f[(size_t)k * S] = y;
  }
  // ---- backward pass; keep the un-padded part
  const double r0 = f[(size_t)(E - 1) * S];
  for (int i = 0; i < N; ++i) z[i] = p.zi[i] * r0;
  float* orow = p.out + (size_t)s * L;
  for (int k = 0; k < E; ++k) {
    const double e = f[(size_t)(E - 1 - k) * S];
    const double y = p.b[0] * e + z[0];
    for (int i = 0; i < N - 1; ++i) z[i] = p.b[i + 1] * e + z[i + 1] - p.a[i + 1] * y;
    z[N - 1] = p.b[N] * e - p.a[N] * y;
    const int t = E - 1 - k - PAD;
    if (t >= 0 && t < L) orow[t] = (float)y;
  }
}

// ---- LDS-resident variant: one wave per signal, the whole padded signal in LDS (fp64) ----
// The IIR recurrence z' = A z + B x is linear, so the time axis is cut into 64 chunks of C samples:
//   (1) every lane filters its chunk from a ZERO state and keeps only the final state s_t;
//   (2) lane 0 chains the true chunk-entry states  z_{t+1} = A^C z_t + s_t  (A^C built once by lanes
//       0..N-1 running C zero-input steps from the unit states);
//   (3) every lane re-filters its chunk from its true entry state, writing y in place.
// C is forced odd so the 64 lanes' chunk cursors (stride C doubles) fall in distinct LDS banks.
// The chain is exact algebraically, not numerically: A is far from normal for a narrow-band, high-order design, the entries of
// A^C built from unit states reach 1e4 .. 1e8 and cancel in A^C z.  So only p.nl of the lanes run the recurrences
// (C = ceil(E / nl) | 1, fewer and longer chunks: a smaller A^C and fewer links), chosen on the host by ecg_iir_lanes; the
// other lanes help with the loads, the baseline, the extension and the stores.  nl = 1 is the plain sequential pass from the
// zi state and needs no A^C.
// I16: the loader decodes int16 frames (sample t = frame t*step, one channel of nsig) and the epilogue crops or zero-pads
// to out_len; everything between the two is the same code for both row sources.
template <int N, bool I16>
__global__ __launch_bounds__(64) void signal_preprocess_lds_kernel(PreParams p) {
  extern __shared__ double sm[];
  constexpr int T = 64, PAD = 3 * (N + 1);
  const int L = p.L, M = p.window, E = L + 2 * PAD;
  const int lane = threadIdx.x, s = blockIdx.x;
  double* A = sm;            // [L]     scaled input
  double* B = sm + L;        // [E]     odd-extended, baseline-removed signal; filtered in place
  double* st = B + E;        // [T][8]  chunk states
  double* Mx = st + T * 8;   // [8][8]  A^C, row-major
  double b[N + 1], a[N + 1];
#pragma unroll
  for (int i = 0; i <= N; ++i) { b[i] = p.b[i]; a[i] = p.a[i]; }

  if constexpr (I16) {
    // p_signal of wfdb: (d - baseline) / gain in float64 (int16 -> double is exact); -32768 is the format's invalid-sample
    // code and becomes NaN.  2-byte loads step*nsig*2 bytes apart: uncoalesced, and dwarfed by the recurrences below.
    const int r = s / p.nc, c = s - r * p.nc;
    const int16_t* xr = p.raw + (size_t)r * p.T * p.nsig + p.chan[c];
    const double g = p.gain[s], bl = (double)p.baseline[s];
    const size_t stride = (size_t)p.step * p.nsig;
    for (int t = lane; t < L; t += T) {
      const int d = xr[(size_t)t * stride];
      A[t] = d == -32768 ? __builtin_nan("") : ((double)d - bl) / g;
    }
  } else {
    const float* xr = p.x + (size_t)s * L;
    for (int t = lane; t < L; t += T) {
      double v = (double)xr[t];
      if (p.sc_mean) v = (v - (double)p.sc_mean[t]) / (double)p.sc_scale[t];
      A[t] = v;
    }
  }
  const int nl = p.nl;
  const int C = ((E + nl - 1) / nl) | 1;
  if (lane < N && nl > 1) {  // column `lane` of A^C
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
  {  // moving-average baseline, np.convolve(x, ones(M)/M, 'same'): mean over [i - bk, i + fw], zero outside
    const int fw = (M - 1) / 2, bk = M - 1 - fw;
    const int Cm = ((L + T - 1) / T) | 1;
    const int i0 = lane * Cm, i1 = min(L, i0 + Cm);
    if (i0 < L) {
      double run = 0.0;
      for (int j = max(0, i0 - bk); j <= min(L - 1, i0 + fw); ++j) run += A[j];
      for (int i = i0; i < i1; ++i) {
        B[PAD + i] = A[i] - run / (double)M;
        const int add = i + fw + 1, sub = i - bk;
        if (add < L) run += A[add];
        if (sub >= 0) run -= A[sub];
      }
    }
  }
  __syncthreads();
  if (lane < PAD) {  // odd extension about both ends
    B[lane] = 2.0 * B[PAD] - B[PAD + (PAD - lane)];
    B[PAD + L + lane] = 2.0 * B[PAD + L - 1] - B[PAD + L - 2 - lane];
  }
  __syncthreads();

  const int k0 = lane < nl ? min(E, lane * C) : E, k1 = min(E, k0 + C);   // lanes >= nl own no chunk
#pragma unroll 1
  for (int pass = 0; pass < 2; ++pass) {
    auto at = [&](int k) -> double& { return B[pass ? E - 1 - k : k]; };
    double z[N];
    if (nl > 1 && k1 - k0 == C) {  // a full chunk hands a state on
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
  if constexpr (I16) {  // signal[:out_len], or the signal followed by zeros (train_signal_only_ptb.py:48-52)
    float* orow = p.out + (size_t)s * p.out_len;
    for (int t = lane; t < p.out_len; t += T) orow[t] = t < L ? (float)B[PAD + t] : 0.0f;
  } else {
    float* orow = p.out + (size_t)s * L;
    for (int t = lane; t < L; t += T) orow[t] = (float)B[PAD + t];
  }
}

constexpr size_t PRE_LDS_MAX = 160 * 1024;
// scaled copy [L] + odd-extended signal [L + 6(N+1)] + chunk states [64][8] + A^C [8][8], all fp64
inline size_t pre_lds_bytes(int L, int order) { return ((size_t)L + L + 6 * (order + 1) + 64 * 8 + 64) * sizeof(double); }

template <int N, bool I16>
int launch_lds(const PreParams& p, size_t lds, hipStream_t st) {
  (void)hipFuncSetAttribute((const void*)signal_preprocess_lds_kernel<N, I16>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)PRE_LDS_MAX);
  hipLaunchKernelGGL((signal_preprocess_lds_kernel<N, I16>), dim3(p.S), dim3(64), lds, st, p);
  return 0;
}

template <bool I16>
void launch_lds_order(const PreParams& p, size_t lds, hipStream_t st) {
  switch (p.order) {
    case 1: launch_lds<1, I16>(p, lds, st); break;
    case 2: launch_lds<2, I16>(p, lds, st); break;
    case 3: launch_lds<3, I16>(p, lds, st); break;
    case 4: launch_lds<4, I16>(p, lds, st); break;
    case 5: launch_lds<5, I16>(p, lds, st); break;
    case 6: launch_lds<6, I16>(p, lds, st); break;
    default: launch_lds<7, I16>(p, lds, st); break;
  }
}

}  // namespace

// Lane rule of the chunked kernels (DESIGN "Lane rule").  The rounding of the chain z_{t+1} = A^C z_t + s_t reaches the output
// as about 2^-53 * G * P relative to the row, G = max_{0<=k<=E} max|A^k| (how far a state error can grow on its way out) and
// P = max|A^C| (the size of the terms that cancel in A^C z), both from the unit states in double, exactly as the kernels build
// A^C.  Measured against a long-double filtfilt with the float64 restatement of the scheme (tests/iir_ref.py), the error over
// that product is 0.5 .. 7.5 (5th .. 95th percentile), so K = 8; the largest nl with  8 * K * 2^-53 * G * P(nl) <= 2^-24
// is taken, i.e. G * P <= 2^23, and 1 (sequential, no chain at all) when there is none.  O(E order^2) on the host, so the last
// answer is kept per thread: a loader asks the same question for every batch.
int ecg_iir_lanes(const double* a, int order, int E) {
  struct Memo { int order, E, nl; double a[9]; };
  static thread_local Memo memo = {0, 0, 0, {0}};
  if (order < 1 || order > 8 || E < 1) return 1;
  if (memo.order == order && memo.E == E && memcmp(memo.a, a, sizeof(double) * (order + 1)) == 0) return memo.nl;
  constexpr int NL = 6;
  const int lanes[NL] = {64, 32, 16, 8, 4, 2};
  int want[NL];
  double P[NL];
  for (int i = 0; i < NL; ++i) { want[i] = ((E + lanes[i] - 1) / lanes[i]) | 1; P[i] = HUGE_VAL; }
  double z[8][8];   // z[i][j]: state i of the column started from unit state j
  for (int i = 0; i < order; ++i)
    for (int j = 0; j < order; ++j) z[i][j] = i == j ? 1.0 : 0.0;
  double G = 1.0;
  for (int k = 1; k <= E; ++k) {
    double m = 0.0;
    for (int j = 0; j < order; ++j) {
      const double y = z[0][j];
      for (int i = 0; i < order - 1; ++i) z[i][j] = z[i + 1][j] - a[i + 1] * y;
      z[order - 1][j] = -a[order] * y;
      for (int i = 0; i < order; ++i) {
        const double v = fabs(z[i][j]);
        if (!(v <= m)) m = v;   // a NaN sticks
      }
    }
    if (!(m < HUGE_VAL)) m = HUGE_VAL;
    if (m > G) G = m;
    for (int i = 0; i < NL; ++i)
      if (want[i] == k) P[i] = m;
  }
  int nl = 1;
  for (int i = 0; i < NL; ++i)
    if (G * P[i] <= 8388608.0) { nl = lanes[i]; break; }   // 2^23 = 2^-24 / (8 * K * 2^-53), K = 8
  memo.order = order; memo.E = E; memo.nl = nl;
  memcpy(memo.a, a, sizeof(double) * (order + 1));
  return nl;
}

extern "C" int ecgmm_signal_filter_lanes(const double* a, int order, int L) {
  if (!a || order < 1 || order > 8 || L < 1 || a[0] != 1.0)   // 0 with the message set: no lane count is 0
    ECG_FAIL(0, "signal_filter_lanes: need a with a[0] = 1, 1 <= order <= 8, L >= 1 (order=%d L=%d)", order, L);
  return ecg_iir_lanes(a, order, L + 6 * (order + 1));
}

extern "C" size_t ecgmm_signal_preprocess_workspace(int S, int L, int order) {
  return ((size_t)L + (size_t)L + 6 * (order + 1)) * (size_t)S * sizeof(double);
}

extern "C" int ecgmm_signal_preprocess(const float* x, float* out, int S, int L, const float* sc_mean,
                                       const float* sc_scale, int window, const double* b, const double* a,
                                       const double* zi, int order, void* ws, size_t ws_bytes, void* stream) {
  if (order < 1 || order > 7) ECG_FAIL(ECGMM_ERR_SHAPE, "signal_preprocess: filter order %d outside 1..7", order);
  if (S < 1 || L < window || L <= 3 * (order + 1))
    ECG_FAIL(ECGMM_ERR_SHAPE, "signal_preprocess: need L >= window and L > 3*(order+1) (S=%d L=%d window=%d)", S, L,
             window);
  if ((sc_mean == nullptr) != (sc_scale == nullptr)) ECG_FAIL(ECGMM_ERR_SHAPE, "signal_preprocess: scaler needs mean AND scale");
  if (!ws || ws_bytes < ecgmm_signal_preprocess_workspace(S, L, order))
    ECG_FAIL(ECGMM_ERR_WORKSPACE, "signal_preprocess: workspace too small");
  if (a[0] != 1.0) ECG_FAIL(ECGMM_ERR_SHAPE, "signal_preprocess: a[0] must be 1 (normalised transfer function)");
  PreParams p;
  memset(&p, 0, sizeof(p));
  p.x = x; p.out = out; p.sc_mean = sc_mean; p.sc_scale = sc_scale; p.ws = (double*)ws;
  p.S = S; p.L = L; p.window = window; p.order = order;
  for (int i = 0; i <= order; ++i) { p.b[i] = b[i]; p.a[i] = a[i]; }
  for (int i = 0; i < order; ++i) p.zi[i] = zi[i];
  // LDS-resident chunk-parallel kernel whenever one padded signal (+ the scaled copy) fits one CU's LDS;
  // longer records take the one-lane-per-signal kernel over the global workspace.
  const size_t lds = pre_lds_bytes(L, order);
  if (lds <= PRE_LDS_MAX) {
    p.nl = ecg_iir_lanes(a, order, L + 6 * (order + 1));
    launch_lds_order<false>(p, lds, (hipStream_t)stream);
  } else {
    hipLaunchKernelGGL(signal_preprocess_kernel, dim3(ceil_div(S, 64)), dim3(64), 0, (hipStream_t)stream, p);
  }
  ECG_CHECK_LAUNCH("signal_preprocess");
  return 0;
}

// WFDB format-16 frames -> the PTB-XL trainer's rows, one launch (train_signal_only_ptb.py:40-53).  Every check is on the
// host and no device address is formed from data: chan[] is validated here, gain / baseline are read at [row].
extern "C" int ecgmm_signal_preprocess_i16(const int16_t* raw, int R, int T, int nsig, const int* chan, int nc,
                                           const double* gain, const int* baseline, int step, float* out, int out_len,
                                           int window, const double* b, const double* a, const double* zi, int order,
                                           void* stream) {
  if (order < 1 || order > 7) ECG_FAIL(ECGMM_ERR_SHAPE, "signal_preprocess_i16: filter order %d outside 1..7", order);
  if (!raw || !chan || !gain || !baseline || !out || !b || !a || !zi)
    ECG_FAIL(ECGMM_ERR_SHAPE, "signal_preprocess_i16: null operand");
  if (R < 1 || T < 1 || nsig < 1 || nc < 1 || nc > 16 || step < 1 || out_len < 1 || window < 1)
    ECG_FAIL(ECGMM_ERR_SHAPE, "signal_preprocess_i16: need R, T, nsig, step, out_len, window >= 1 and 1 <= nc <= 16 "
             "(R=%d T=%d nsig=%d nc=%d step=%d out_len=%d window=%d)", R, T, nsig, nc, step, out_len, window);
  for (int i = 0; i < nc; ++i)
    if (chan[i] < 0 || chan[i] >= nsig)
      ECG_FAIL(ECGMM_ERR_SHAPE, "signal_preprocess_i16: channel %d (entry %d) outside the record's %d signals", chan[i], i, nsig);
  if ((long long)R * nc > 0x7fffffffLL) ECG_FAIL(ECGMM_ERR_SHAPE, "signal_preprocess_i16: %d x %d rows exceed the grid", R, nc);
  const int Lf = (T + step - 1) / step;
  if (Lf < window || Lf <= 3 * (order + 1))
    ECG_FAIL(ECGMM_ERR_SHAPE, "signal_preprocess_i16: need Lf >= window and Lf > 3*(order+1) (T=%d step=%d Lf=%d window=%d)",
             T, step, Lf, window);
  if (a[0] != 1.0) ECG_FAIL(ECGMM_ERR_SHAPE, "signal_preprocess_i16: a[0] must be 1 (normalised transfer function)");
  // a row that would take the whole 160 KiB is refused as well: Lf <= 9933 at order 5
  const size_t lds = pre_lds_bytes(Lf, order);
  if (lds >= PRE_LDS_MAX)
    ECG_FAIL(ECGMM_ERR_SHAPE, "signal_preprocess_i16: a row of %d samples does not fit one CU's LDS (largest Lf at order %d: %d); "
             "there is no workspace route", Lf, order, (int)((PRE_LDS_MAX / sizeof(double) - 1 - 6 * (order + 1) - 64 * 8 - 64) / 2));
  PreParams p;
  memset(&p, 0, sizeof(p));
  p.raw = raw; p.gain = gain; p.baseline = baseline; p.out = out;
  p.S = R * nc; p.L = Lf; p.window = window; p.order = order;
  p.nl = ecg_iir_lanes(a, order, Lf + 6 * (order + 1));
  p.T = T; p.nsig = nsig; p.nc = nc; p.step = step; p.out_len = out_len;
  for (int i = 0; i < nc; ++i) p.chan[i] = chan[i];
  for (int i = 0; i <= order; ++i) { p.b[i] = b[i]; p.a[i] = a[i]; }
  for (int i = 0; i < order; ++i) p.zi[i] = zi[i];
  launch_lds_order<true>(p, lds, (hipStream_t)stream);
  ECG_CHECK_LAUNCH("signal_preprocess_i16");
  return 0;
}
