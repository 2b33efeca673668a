// The array arithmetic of one batched simulator step on the device: the counterpart of csrc/v2xsim.c's channels_env,
// interference_row + observe_row + observe_env and reward_one for E independent simulator states whose large arrays
// (shadowing, path loss + shadowing, fast fading: a few hundred KB of fp64) stay in HBM.  The host library stays the
// definition; this file restates its expressions one for one -- same operation order, same branches, same fold orders,
// fp64, no contraction, no fast-math -- on the device library's log / sqrt / cos / sin / exp / log10 / hypot / pow / log2, so
// the two agree to the rounding of the two math libraries (tests/test_gpu_device_sim.py: 1e-11 relative on dB values), and
// bit for bit where no transcendental is involved (the observation).  Mobility and the MT19937 streams stay on the host: a
// step receives its uniforms.  Entry points: v2x_sim_* in include/v2xgnn.h; Python: rl/device_sim.py.
//
// One launch per entry point, all on the caller's stream, no allocation, no synchronisation (capturable):
//   k_sim_channels  grid (ceil((n + n^2) / 256), E): thread t < n updates V2I link t (shadowing, path loss, its rb fast-fading
//                   values), thread n + i n + j the V2V pair (i, j).  A thread touches only its own elements of the in-place
//                   shadowing arrays, and recomputes the Box-Muller pairs it needs from the uniforms (no workspace).
//   k_sim_observe   grid (E), one wave: lane k writes link k's interference row, observation row and packed row, lane q the
//                   source mask and CSR sources of destination q.
//   k_sim_rates     grid (ceil((n + rb) / 64), E): thread k < n the V2V rate of link k, thread n + r the base-station sum,
//                   V2I interference and V2I rate of resource block r.
#include "../../include/v2xgnn.h"
#include "../../include/v2xsim_const.h"

#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>

namespace v2x {
void set_global_error(const char* text);   // v2x_last_error(NULL) text (v2xgnn.hip)
}

namespace {

constexpr int SIM_CH_BLOCK = 256;
constexpr int SIM_ROW_BLOCK = 64;                 // observe / rates workgroup: one wave
constexpr int SIM_MAX_N = 128, SIM_MAX_RB = 16, SIM_MAX_E = 65535;
constexpr int SIM_OBS_MIN_N = 3, SIM_OBS_MAX_N = 31, SIM_XE_WIDTH = V2X_XE_WIDTH;

#define SIM_FAIL(code, ...)                      \
  do {                                           \
    char _b[512];                                \
    snprintf(_b, sizeof(_b), __VA_ARGS__);       \
    v2x::set_global_error(_b);                   \
    return code;                                 \
  } while (0)

// ---- path loss: csrc/v2xsim.c los / nlos / v2v_pathloss / v2i_pathloss (Environment.py:94-122, :139-146) -------------------
__device__ inline double sim_los(double x, double d_bp, double off) {
#pragma clang fp contract(off)
  if (x < 1e-300) x = 1e-300;
  if (x <= 3) return 22.7 * log10(3.0) + off;
  if (x < d_bp) return 22.7 * log10(x) + off;
  return 40.0 * log10(x) + 9.45 - 17.3 * log10(V2V_H) - 17.3 * log10(V2V_H) + 2.7 * log10(FC / 5);
}
__device__ inline double sim_nlos(double da, double db, double d_bp, double off) {
#pragma clang fp contract(off)
  if (db < 1e-300) db = 1e-300;
  double nj = 2.8 - 0.0024 * db;
  if (nj < 1.84) nj = 1.84;
  return sim_los(da, d_bp, off) + 20 - 12.5 * nj + 10 * nj * log10(db) + 3 * log10(FC / 5);
}
__device__ inline double sim_v2v_pathloss(double x0, double y0, double x1, double y1) {
#pragma clang fp contract(off)
  const double d1 = fabs(x0 - x1), d2 = fabs(y0 - y1);
  const double d = hypot(d1, d2) + 0.001;
  const double d_bp = 4 * (V2V_H - 1) * (V2V_H - 1) * FC * 1e9 / 3e8;
  const double off = 41 + 20 * log10(FC / 5);
  if ((d1 < d2 ? d1 : d2) < 7) return sim_los(d, d_bp, off);
  const double a = sim_nlos(d1, d2, d_bp, off), b = sim_nlos(d2, d1, d_bp, off);
  return a < b ? a : b;
}
__device__ inline double sim_v2i_pathloss(double x, double y) {
#pragma clang fp contract(off)
  const double dist = hypot(fabs(x - BS_X), fabs(y - BS_Y));
  return 128.1 + 37.6 * log10(sqrt(dist * dist + (V2I_H_BS - V2I_H_MS) * (V2I_H_BS - V2I_H_MS)) / 1000);
}

// Gaussian k of a state: cos(2 pi u[k & ~1]) sqrt(-2 log(1 - u[k | 1])) for even k, the sin for odd k (random.gauss order).
// The pair last computed is kept, so two neighbours of one pair cost one log / sqrt / cos / sin each.
struct SimPair {
  int pair;
  double c, s;
};
__device__ inline double sim_gauss(const double* __restrict__ ue, int k, SimPair& gp) {
#pragma clang fp contract(off)
  const int p = k >> 1;
  if (p != gp.pair) {
    const double x2pi = ue[2 * p] * TWOPI;
    const double g2rad = sqrt(-2.0 * log(1.0 - ue[2 * p + 1]));
    gp.c = cos(x2pi) * g2rad;
    gp.s = sin(x2pi) * g2rad;
    gp.pair = p;
  }
  return (k & 1) ? gp.s : gp.c;
}

struct SimChannelsArgs {
  int n, rb, n_u;
  const double *u, *vel, *pos;
  double *v2i_shadow, *v2v_shadow, *v2v_abs, *v2i_abs, *v2v_ff, *v2i_ff;
};

// channels_env of csrc/v2xsim.c.  Draw order inside a state: V2I shadowing (n), V2V shadowing (n^2), V2I fast fading real
// (n rb) and imaginary (n rb), V2V fast fading real (n^2 rb) and imaginary (n^2 rb); n_u is their exact (even) sum, so every
// pair index a thread forms lies inside the state's uniforms.
__global__ __launch_bounds__(SIM_CH_BLOCK) void k_sim_channels(SimChannelsArgs q) {
#pragma clang fp contract(off)
  const int n = q.n, rb = q.rb;
  const int t = (int)(blockIdx.x * SIM_CH_BLOCK + threadIdx.x);
  if (t >= n + n * n) return;
  const int64_t e = blockIdx.y;
  const double* ue = q.u + e * q.n_u;
  const double* ve = q.vel + e * n;
  const double* pe = q.pos + e * n * 2;
  const int n_sh = n + n * n, a = n * rb, b = n * n * rb;
  const double rs2 = 1 / sqrt(2.0);
  SimPair gre = { -1, 0.0, 0.0 }, gim = { -1, 0.0, 0.0 };
  if (t < n) {
    const int i = t;
    double* si = q.v2i_shadow + e * n;
    const double dd = 0.002 * ve[i];
    const double g = sim_gauss(ue, i, gre);
    const double s = exp(-1 * (dd / V2I_DECORR)) * si[i] + sqrt(1 - exp(-2 * (dd / V2I_DECORR))) * (g * V2I_SHADOW_STD);
    si[i] = s;
    const double ai = sim_v2i_pathloss(pe[2 * i], pe[2 * i + 1]) + s;
    q.v2i_abs[e * n + i] = ai;
    double* fi = q.v2i_ff + e * a;
    for (int r = 0; r < rb; ++r) {                 /* 20 log10 |(re + j im) / sqrt 2| */
      const int k = i * rb + r;
      const double re = rs2 * sim_gauss(ue, n_sh + k, gre), im = rs2 * sim_gauss(ue, n_sh + a + k, gim);
      fi[k] = ai - 20 * log10(hypot(re, im));
    }
  } else {
    const int ij = t - n, i = ij / n, j = ij - i * n;
    double* sv = q.v2v_shadow + e * n * n;
    const double ddm = 0.002 * ve[i] + 0.002 * ve[j];
    const double g = sim_gauss(ue, n + ij, gre);
    const double s = exp(-1 * (ddm / V2V_DECORR)) * sv[ij] + sqrt(1 - exp(-2 * (ddm / V2V_DECORR))) * (g * V2V_SHADOW_STD);
    sv[ij] = s;
    const double av = sim_v2v_pathloss(pe[2 * i], pe[2 * i + 1], pe[2 * j], pe[2 * j + 1]) + s + (i == j ? 50.0 : 0.0);
    q.v2v_abs[e * n * n + ij] = av;
    double* fv = q.v2v_ff + e * b;
    for (int r = 0; r < rb; ++r) {
      const int k = ij * rb + r;
      const double re = rs2 * sim_gauss(ue, n_sh + 2 * a + k, gre), im = rs2 * sim_gauss(ue, n_sh + 2 * a + b + k, gim);
      fv[k] = av - 20 * log10(hypot(re, im));
    }
  }
}

struct SimObserveArgs {
  int n, C;
  const int64_t* dest;
  const double *v2v_ff, *v2i_ff;
  double p_v2i, veh_gain, veh_nf, sig2, power;
  double *interf_db, *state;
  float* xe;
  int32_t *mask, *col;
  uint8_t* regular;
};

// interference_row + observe_row + observe_env of csrc/v2xsim.c for one state per workgroup (n <= 31 lanes at work).
// A receiver outside [0, n) is never used as an index: the state's rows become NaN and it is reported as not regular.
__global__ __launch_bounds__(SIM_ROW_BLOCK) void k_sim_observe(SimObserveArgs q) {
#pragma clang fp contract(off)
  const int n = q.n, C = q.C, W = 3 * C + 1;
  const int k = threadIdx.x;
  if (k >= n) return;
  const int64_t e = blockIdx.x;
  const int64_t* d = q.dest + e * n;
  const double* vv = q.v2v_ff + e * n * n * C;
  const double* vi = q.v2i_ff + e * n * C;
  bool bad = false, reg = true;
  for (int l = 0; l < n; ++l) {
    const int64_t x = d[l];
    if (x < 0 || x >= n) bad = true;
    if (x == l) reg = false;
  }
  if (bad) reg = false;
  double* st = q.state + (e * n + k) * W;
  float* xe = q.xe + (e * n + k) * SIM_XE_WIDTH;
  double* itf = q.interf_db + (e * n + k) * C;
  if (bad) {
    const double nan = __builtin_nan("");
    for (int c = 0; c < C; ++c) itf[c] = nan;
    for (int c = 0; c < W; ++c) st[c] = nan;
  } else {
    const int rx = (int)d[k];
    for (int r = 0; r < C; ++r) {                  /* Compute_Interference: noise + the V2I transmitter of block r, vehicle r */
      double v = q.sig2;
      v += pow(10.0, (q.p_v2i - vv[(r * n + rx) * C + r] + 2 * q.veh_gain - q.veh_nf) / 10);
      itf[r] = 10 * log10(v);
    }
    const double A = 80, Bc = 60;
    for (int c = 0; c < C; ++c) {
      const double chv = (vv[(k * n + rx) * C + c] - A) / Bc;
      double tot = 0.0;
      for (int p = 0; p < n; ++p) tot += vv[(p * n + rx) * C + c];          /* np.sum over p, ascending */
      const double edge = (((tot - vv[(rx * n + rx) * C + c]) - (n - 1) * A) / Bc - chv) / (n - 2);
      st[c] = chv;
      st[C + c] = (vi[k * C + c] - A) / Bc;
      st[2 * C + 1 + c] = edge;
    }
    st[2 * C] = q.power;
  }
  for (int c = 0; c < SIM_XE_WIDTH; ++c) xe[c] = c < W ? (float)st[c] : 0.0f;
  /* destination k: every p sends to it except k itself and k's receiver */
  uint32_t m = ((1u << n) - 1u) & ~(1u << k);
  if (!bad) m &= ~(1u << (int)d[k]);
  q.mask[e * n + k] = (int32_t)m;
  int32_t* col = q.col + e * n * (n - 2) + k * (n - 2);
  if (reg) {
    int o = 0;
    for (int p = 0; p < n; ++p)
      if ((m >> p) & 1u) col[o++] = p;             /* a regular graph: exactly n - 2 bits */
  } else {
    for (int o = 0; o < n - 2; ++o) col[o] = 0;
  }
  if (k == 0) q.regular[e] = reg ? 1 : 0;
}

struct SimRatesArgs {
  int n, rb;
  const int32_t* ch;
  const int64_t* dest;
  const double *v2v_ff, *v2i_ff, *v2i_abs;
  double p_v2v, p_v2i, veh_gain, bs_gain, bs_nf, veh_nf, sig2;
  double *v2v_rate, *v2i_rate, *interference, *v2i_interf, *v2v_interf;
};

// reward_one of csrc/v2xsim.c.  A channel outside [0, rb) anywhere in the state makes all its outputs NaN, a receiver
// outside [0, n) those of its link; neither is used as an index.
__global__ __launch_bounds__(SIM_ROW_BLOCK) void k_sim_rates(SimRatesArgs a) {
#pragma clang fp contract(off)
  const int n = a.n, rb = a.rb, m = rb < n ? rb : n;
  const int t = (int)(blockIdx.x * SIM_ROW_BLOCK + threadIdx.x);
  if (t >= n + rb) return;
  const int64_t e = blockIdx.y;
  const int32_t* c = a.ch + e * n;
  const int64_t* d = a.dest + e * n;
  const double* vv = a.v2v_ff + e * n * n * rb;
  const double* vi = a.v2i_ff + e * n * rb;
  const double nan = __builtin_nan("");
  bool ok = true;
  for (int l = 0; l < n; ++l)
    if (c[l] < 0 || c[l] >= rb) ok = false;
  if (t >= n) {
    const int r = t - n;
    double itf = 0.0;
    if (ok) {
      for (int k = 0; k < n; ++k)                  /* (at_bs * onehot).sum(axis=1): ascending k per block */
        if (c[k] == r) itf += pow(10.0, (a.p_v2v - vi[k * rb + r] + a.veh_gain + a.bs_gain - a.bs_nf) / 10);
    } else {
      itf = nan;
    }
    const double with_noise = itf + a.sig2;
    if (a.interference) a.interference[e * rb + r] = itf;
    if (a.v2i_interf) a.v2i_interf[e * rb + r] = with_noise;
    if (r < m) {
      const double s = a.p_v2i - a.v2i_abs[e * n + r] + a.veh_gain + a.bs_gain - a.bs_nf;
      a.v2i_rate[e * m + r] = log2(1 + pow(10.0, s / 10) / with_noise);
    }
    return;
  }
  const int k = t;
  const int64_t rx = d[k];
  double tot = nan, rate = nan;
  if (ok && rx >= 0 && rx < n) {
    const double gain = 2 * a.veh_gain - a.veh_nf;
    const int r = c[k];
    const double signal = pow(10.0, (a.p_v2v - vv[(k * n + rx) * rb + r] + gain) / 10);
    double acc = 0.0;
    if (r < n) acc += pow(10.0, (a.p_v2i - vv[(r * n + rx) * rb + r] + gain) / 10);   /* the V2I transmitter of block r is vehicle r */
    double cross = 0.0;
    for (int j = 0; j < n; ++j)
      if (j != k && c[j] == r) cross += pow(10.0, (a.p_v2v - vv[(j * n + rx) * rb + r] + gain) / 10);
    acc += cross;
    tot = acc + a.sig2;
    rate = log2(1 + signal / tot);
  }
  if (a.v2v_interf) a.v2v_interf[e * n + k] = tot;
  a.v2v_rate[e * n + k] = rate;
}

}  // namespace

extern "C" {

int v2x_sim_channels(int32_t E, int32_t n, int32_t rb, const double* u, int32_t n_u, const double* vel, const double* pos,
                     double* v2i_shadow, double* v2v_shadow, double* v2v_abs, double* v2i_abs, double* v2v_ff, double* v2i_ff,
                     void* stream) {
  if (E < 1 || E > SIM_MAX_E || n < 1 || n > SIM_MAX_N || rb < 1 || rb > SIM_MAX_RB)
    SIM_FAIL(V2X_EINVAL, "sim_channels: 1..%d states, 1..%d links and 1..%d resource blocks supported, got E = %d, n = %d, rb = %d",
             SIM_MAX_E, SIM_MAX_N, SIM_MAX_RB, E, n, rb);
  const int want = n + n * n + 2 * n * rb + 2 * n * n * rb;
  if (n_u != want)
    SIM_FAIL(V2X_EINVAL, "sim_channels: n_u = %d, but a step of %d links x %d resource blocks draws %d uniforms per state", n_u, n,
             rb, want);
  if (!u || !vel || !pos || !v2i_shadow || !v2v_shadow || !v2v_abs || !v2i_abs || !v2v_ff || !v2i_ff)
    SIM_FAIL(V2X_EINVAL, "sim_channels: null pointer");
  SimChannelsArgs q = { n, rb, n_u, u, vel, pos, v2i_shadow, v2v_shadow, v2v_abs, v2i_abs, v2v_ff, v2i_ff };
  const dim3 grid((unsigned)((n + n * n + SIM_CH_BLOCK - 1) / SIM_CH_BLOCK), (unsigned)E);
  hipLaunchKernelGGL(k_sim_channels, grid, dim3(SIM_CH_BLOCK), 0, (hipStream_t)stream, q);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) SIM_FAIL(V2X_EHIP, "sim_channels: launch failed: %s", hipGetErrorString(err));
  return V2X_OK;
}

int v2x_sim_observe(int32_t E, int32_t n, int32_t C, const int64_t* dest, const double* v2v_ff, const double* v2i_ff,
                    double p_v2i, double veh_gain, double veh_nf, double sig2, double power, double* interf_db, double* state,
                    float* xe, int32_t* mask, int32_t* col, uint8_t* regular, void* stream) {
  if (E < 1 || E > SIM_MAX_E) SIM_FAIL(V2X_EINVAL, "sim_observe: 1..%d states supported, got E = %d", SIM_MAX_E, E);
  if (n < SIM_OBS_MIN_N || n > SIM_OBS_MAX_N || C < 1 || C > n || 3 * C + 1 > SIM_XE_WIDTH)
    SIM_FAIL(V2X_EINVAL, "sim_observe: %d..%d links, 1 <= C <= n and 3 C + 1 <= %d supported, got n = %d, C = %d", SIM_OBS_MIN_N,
             SIM_OBS_MAX_N, SIM_XE_WIDTH, n, C);
  if (!dest || !v2v_ff || !v2i_ff || !interf_db || !state || !xe || !mask || !col || !regular)
    SIM_FAIL(V2X_EINVAL, "sim_observe: null pointer");
  SimObserveArgs q = { n, C, dest, v2v_ff, v2i_ff, p_v2i, veh_gain, veh_nf, sig2, power, interf_db, state, xe, mask, col, regular };
  hipLaunchKernelGGL(k_sim_observe, dim3((unsigned)E), dim3(SIM_ROW_BLOCK), 0, (hipStream_t)stream, q);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) SIM_FAIL(V2X_EHIP, "sim_observe: launch failed: %s", hipGetErrorString(err));
  return V2X_OK;
}

int v2x_sim_rates(const v2x_opt_problem* p, const int32_t* ch, double* v2v_rate, double* v2i_rate, double* interference,
                  double* v2i_interf, double* v2v_interf, void* stream) {
  if (!p) SIM_FAIL(V2X_EINVAL, "sim_rates: null problem");
  if (p->E < 1 || p->E > SIM_MAX_E || p->n < 1 || p->n > SIM_MAX_N || p->rb < 1 || p->rb > SIM_MAX_RB)
    SIM_FAIL(V2X_EINVAL, "sim_rates: 1..%d states, 1..%d links and 1..%d resource blocks supported, got E = %d, n = %d, rb = %d",
             SIM_MAX_E, SIM_MAX_N, SIM_MAX_RB, p->E, p->n, p->rb);
  if (!p->v2v_ff || !p->v2i_ff || !p->v2i_abs || !p->dest) SIM_FAIL(V2X_EINVAL, "sim_rates: null input array");
  if (!ch || !v2v_rate || !v2i_rate) SIM_FAIL(V2X_EINVAL, "sim_rates: null actions or rate output");
  SimRatesArgs a = { p->n, p->rb, ch, p->dest, p->v2v_ff, p->v2i_ff, p->v2i_abs, p->p_v2v, p->p_v2i, p->veh_gain, p->bs_gain,
                     p->bs_nf, p->veh_nf, p->sig2, v2v_rate, v2i_rate, interference, v2i_interf, v2v_interf };
  const dim3 grid((unsigned)((p->n + p->rb + SIM_ROW_BLOCK - 1) / SIM_ROW_BLOCK), (unsigned)p->E);
  hipLaunchKernelGGL(k_sim_rates, grid, dim3(SIM_ROW_BLOCK), 0, (hipStream_t)stream, a);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) SIM_FAIL(V2X_EHIP, "sim_rates: launch failed: %s", hipGetErrorString(err));
  return V2X_OK;
}

}  // extern "C"
