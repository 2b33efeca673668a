// Exhaustive search for the optimal channel allocation of a simulator state (the brute-force baseline of the
// evaluation drivers, BS_brain.py:1060-1100, :1286-1330, :1339-1380): every joint action of N links over C resource
// blocks is scored with the reward of compute_reward_with_channel_selection (rl/environment.py) in fp64, and the best
// one (lowest index among exact ties, like np.argmax) is kept.  Entry points: v2x_opt_* in include/v2xgnn.h.
//
// Joint action index  idx = sum_l a_l * C^(N-1-l)  (link 0 most significant: itertools.product order).
//
// Launches, all on the caller's stream:
//   k_opt_prep    dB inputs -> linear-domain tables per state in the workspace (the only pow() calls)
//   k_opt_search  grid (chunk, state); a thread fixes the high p = N - m digits (the prefix) and walks the C^m suffixes;
//                 the prefix links' interference is folded once per prefix into thread-private LDS slots
//   k_opt_reduce  one workgroup per state folds the per-workgroup partials in a fixed order
//   k_opt_rewards the reward of every index of a range (m = 0: every link is a prefix link)
// Search and rewards call the same opt_prefix_init / opt_eval, and every sum is a left fold in ascending link order that
// only skips links on other channels, so where the prefix ends does not change a single bit: rewards[best] == best.
#include "../../include/v2xgnn.h"

#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>

namespace v2x {
void set_global_error(const char* text);   // v2x_last_error(NULL) text (v2xgnn.hip)
}

namespace {

constexpr int OPT_BLOCK = 128;                    // search / rewards workgroup
constexpr int OPT_PREP_BLOCK = 256;
constexpr int OPT_REDUCE_BLOCK = 256;
constexpr int OPT_MAX_N = 32, OPT_MIN_C = 2, OPT_MAX_C = 16;
constexpr int OPT_MAX_SUFFIX = 15;                // digits walked per thread (4 bits each in one 64-bit word)
constexpr int64_t OPT_MAX_SEARCH = 1ll << 36;     // joint actions per state the search accepts
constexpr int64_t OPT_MAX_INDEX = 1ll << 62;      // joint actions per state the rewards entry accepts
constexpr int64_t OPT_TARGET_THREADS = 1 << 19;   // prefixes of one search launch before the walk grows (~8 waves per SIMD)
constexpr int64_t OPT_MAX_WGS = 8192;             // workgroups of one search launch (grid-stride beyond)
constexpr int64_t OPT_REWARDS_WGS = 16384;
constexpr size_t OPT_LDS_CAP = 63 * 1024;           // dynamic LDS (the reductions add a few static bytes)

#define OPT_FAIL(code, ...)                      \
  do {                                           \
    char _b[512];                                \
    snprintf(_b, sizeof(_b), __VA_ARGS__);       \
    v2x::set_global_error(_b);                   \
    return code;                                 \
  } while (0)

// per-state table of linear-domain terms (doubles): sig[n][C] | tx[n][C] | bs[n][C] | cross[n][n][C] | v2i[C]
__host__ __device__ inline int64_t opt_tab_doubles(int n, int C) { return 3ll * n * C + (int64_t)n * n * C + C; }

struct OptParams {
  int n, C, nr;       // links, resource blocks, V2I links (min(C, n))
  int p, m;           // prefix digits fixed per thread, suffix digits walked (p + m == n)
  int64_t tab;        // doubles per state table
  double sig2, w_v2v, w_v2i;
};

__device__ __forceinline__ int opt_digit(uint64_t lo, uint64_t hi, int l) {
  return (int)(((l < 16) ? (lo >> (4 * l)) : (hi >> (4 * (l - 16)))) & 15u);
}
__device__ __forceinline__ int opt_sdigit(uint64_t s, int j) { return (int)((s >> (4 * j)) & 15u); }

// Thread-private fold state (LDS, slot j at st[j * ld]):
//   Q[l]        l < p   tx[l][a_l] + sum over prefix links k != l on a_l of cross[l][k][a_l]
//   P[j][c]     j < m   tx[p+j][c] + sum over prefix links k on c of cross[p+j][k][c]
//   B[r]        r < nr  sum over prefix links k on r of bs[k][r]
// Every sum runs over ascending k; opt_eval continues it with the suffix links, again ascending.
__device__ __forceinline__ void opt_prefix_init(const OptParams& q, const double* __restrict__ tab, uint64_t lo, uint64_t hi,
                                                double* st, int ld) {
#pragma clang fp contract(off)
  const int n = q.n, C = q.C, p = q.p;
  const double* tx = tab + (int64_t)n * C;
  const double* bs = tab + 2ll * n * C;
  const double* cross = tab + 3ll * n * C;
  for (int l = 0; l < p; ++l) {
    const int c = opt_digit(lo, hi, l);
    double acc = tx[l * C + c];
    for (int k = 0; k < p; ++k)
      if (k != l && opt_digit(lo, hi, k) == c) acc += cross[(l * n + k) * C + c];
    st[l * ld] = acc;
  }
  for (int j = 0; j < q.m; ++j) {
    const int l = p + j;
    for (int c = 0; c < C; ++c) {
      double acc = tx[l * C + c];
      for (int k = 0; k < p; ++k)
        if (opt_digit(lo, hi, k) == c) acc += cross[(l * n + k) * C + c];
      st[(p + j * C + c) * ld] = acc;
    }
  }
  for (int r = 0; r < q.nr; ++r) {
    double acc = 0.0;
    for (int k = 0; k < p; ++k)
      if (opt_digit(lo, hi, k) == r) acc += bs[k * C + r];
    st[(p + q.m * C + r) * ld] = acc;
  }
}

// reward of the joint action (prefix digits lo/hi, suffix digits s) -- rl/environment.py:241-274 in linear terms:
// one log2(1 + x) per rate, V2V rates in link order, then V2I rates in RB order
__device__ __forceinline__ double opt_eval(const OptParams& q, const double* __restrict__ tab, uint64_t lo, uint64_t hi,
                                           uint64_t s, const double* st, int ld) {
#pragma clang fp contract(off)
  const int n = q.n, C = q.C, p = q.p, m = q.m;
  const double* sig = tab;
  const double* bs = tab + 2ll * n * C;
  const double* cross = tab + 3ll * n * C;
  const double* v2i = tab + 3ll * n * C + (int64_t)n * n * C;
  double v2v_sum = 0.0;
  for (int l = 0; l < n; ++l) {
    int c;
    double acc;
    if (l < p) {
      c = opt_digit(lo, hi, l);
      acc = st[l * ld];
    } else {
      c = opt_sdigit(s, l - p);
      acc = st[(p + (l - p) * C + c) * ld];
    }
    for (int j = 0; j < m; ++j) {
      const int k = p + j;
      if (k != l && opt_sdigit(s, j) == c) acc += cross[(l * n + k) * C + c];
    }
    v2v_sum += log2(1.0 + sig[l * C + c] / (acc + q.sig2));
  }
  double v2i_sum = 0.0;
  for (int r = 0; r < q.nr; ++r) {
    double b = st[(p + m * C + r) * ld];
    for (int j = 0; j < m; ++j)
      if (opt_sdigit(s, j) == r) b += bs[(p + j) * C + r];
    v2i_sum += log2(1.0 + v2i[r] / (b + q.sig2));
  }
  return q.w_v2v * v2v_sum + q.w_v2i * v2i_sum;
}

// index of the prefix -> its digits, link p - 1 least significant
__device__ __forceinline__ void opt_decode_prefix(int64_t t, int p, int C, uint64_t& lo, uint64_t& hi) {
  lo = 0;
  hi = 0;
  for (int l = p - 1; l >= 0; --l) {
    const uint64_t d = (uint64_t)(t % C);
    t /= C;
    if (l < 16) lo |= d << (4 * l);
    else hi |= d << (4 * (l - 16));
  }
}

// (r, i) beats (br, bi): larger reward, or the same reward at a lower index
__device__ __forceinline__ bool opt_better(double r, int64_t i, double br, int64_t bi) {
  return r > br || (r == br && i < bi);
}

// best of the workgroup into lane 0 of wave 0 (fixed-order comparisons: the result does not depend on the order anyway,
// the rule picks the unique (max reward, min index) pair)
template <int BLOCK>
__device__ __forceinline__ void opt_block_best(double& br, int64_t& bi) {
  __shared__ double sr[BLOCK / 64];
  __shared__ int64_t si[BLOCK / 64];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double r = __shfl_xor(br, off, 64);
    const long long i = __shfl_xor((long long)bi, off, 64);
    if (opt_better(r, i, br, bi)) { br = r; bi = i; }
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sr[wave] = br; si[wave] = bi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < BLOCK / 64; ++w)
      if (opt_better(sr[w], si[w], br, bi)) { br = sr[w]; bi = si[w]; }
  }
}

struct OptPrepArgs {
  const double *v2v_ff, *v2i_ff, *v2i_abs;
  const int64_t* dest;
  double p_v2v, p_v2i, veh_gain, bs_gain, bs_nf, veh_nf, sig2;
  int n, C;
  int64_t tab;
  double* tabs;
};

__device__ __forceinline__ double opt_db(double x) { return pow(10.0, x / 10.0); }

// grid (ceil(tab / 256), E): one table entry per thread.  A receiver outside [0, n) poisons the link's entries with NaN
// instead of reading out of bounds.
__global__ __launch_bounds__(OPT_PREP_BLOCK) void k_opt_prep(OptPrepArgs a) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * OPT_PREP_BLOCK + threadIdx.x;
  if (i >= a.tab) return;
  const int e = blockIdx.y, n = a.n, C = a.C;
  const int64_t nC = (int64_t)n * C;
  const double* v2v = a.v2v_ff + (int64_t)e * n * nC;     // [n][n][C]
  const double* v2if = a.v2i_ff + (int64_t)e * nC;        // [n][C]
  const double* v2ia = a.v2i_abs + (int64_t)e * n;        // [n]
  const int64_t* dst = a.dest + (int64_t)e * n;
  const double gain = 2 * a.veh_gain - a.veh_nf;
  const double nan = __builtin_nan("");
  double out;
  if (i < 3 * nC) {
    const int part = (int)(i / nC), l = (int)((i % nC) / C), c = (int)(i % C);
    if (part == 2) {
      out = opt_db((((a.p_v2v - v2if[l * C + c]) + a.veh_gain) + a.bs_gain) - a.bs_nf);
    } else {
      const int64_t rx = dst[l];
      if (rx < 0 || rx >= n) out = nan;
      else if (part == 0) out = opt_db((a.p_v2v - v2v[((int64_t)l * n + rx) * C + c]) + gain);
      else out = c < n ? opt_db((a.p_v2i - v2v[((int64_t)c * n + rx) * C + c]) + gain) : 0.0;
    }
  } else if (i < 3 * nC + (int64_t)n * nC) {
    const int64_t j = i - 3 * nC;
    const int l = (int)(j / nC), k = (int)((j / C) % n), c = (int)(j % C);
    const int64_t rx = dst[l];
    out = (rx < 0 || rx >= n) ? nan : opt_db((a.p_v2v - v2v[((int64_t)k * n + rx) * C + c]) + gain);
  } else {
    const int r = (int)(i - 3 * nC - (int64_t)n * nC);
    out = r < n ? opt_db((((a.p_v2i - v2ia[r]) + a.veh_gain) + a.bs_gain) - a.bs_nf) : 0.0;
  }
  a.tabs[(int64_t)e * a.tab + i] = out;
}

// grid (wgs, E).  LDS: the state's table, then OPT_BLOCK-strided thread slots (p + m*C + C of them).
__global__ __launch_bounds__(OPT_BLOCK) void k_opt_search(OptParams q, const double* __restrict__ tabs, int64_t n_pre,
                                                          int64_t n_suf, double* part_r, int64_t* part_i) {
  extern __shared__ double opt_lds[];
  const int e = blockIdx.y;
  const double* src = tabs + (int64_t)e * q.tab;
  for (int64_t i = threadIdx.x; i < q.tab; i += OPT_BLOCK) opt_lds[i] = src[i];
  __syncthreads();
  const int64_t tab_pad = (q.tab + 1) & ~1ll;
  double* st = opt_lds + tab_pad + threadIdx.x;
  double br = -INFINITY;
  int64_t bi = INT64_MAX;
  const int64_t stride = (int64_t)gridDim.x * OPT_BLOCK;
  for (int64_t t = (int64_t)blockIdx.x * OPT_BLOCK + threadIdx.x; t < n_pre; t += stride) {
    uint64_t lo, hi;
    opt_decode_prefix(t, q.p, q.C, lo, hi);
    opt_prefix_init(q, opt_lds, lo, hi, st, OPT_BLOCK);
    uint64_t s = 0;                                     // suffix digits, link p + j in bits 4j..4j+3
    const int64_t base = t * n_suf;
    for (int64_t j = 0; j < n_suf; ++j) {
      const double r = opt_eval(q, opt_lds, lo, hi, s, st, OPT_BLOCK);
      if (r > br) { br = r; bi = base + j; }           // ascending indices: strict > keeps the first maximiser
      for (int d = q.m - 1; d >= 0; --d) {             // odometer, link n - 1 fastest
        if (opt_sdigit(s, d) + 1 < q.C) { s += 1ull << (4 * d); break; }
        s &= ~(15ull << (4 * d));
      }
    }
  }
  opt_block_best<OPT_BLOCK>(br, bi);
  if (threadIdx.x == 0) {
    part_r[(int64_t)e * gridDim.x + blockIdx.x] = br;
    part_i[(int64_t)e * gridDim.x + blockIdx.x] = bi;
  }
}

// grid E: the partials of one state, in a fixed order
__global__ __launch_bounds__(OPT_REDUCE_BLOCK) void k_opt_reduce(const double* part_r, const int64_t* part_i, int wgs,
                                                                 int64_t* best_index, double* best_reward) {
  const int e = blockIdx.x;
  double br = -INFINITY;
  int64_t bi = INT64_MAX;
  for (int w = threadIdx.x; w < wgs; w += OPT_REDUCE_BLOCK) {
    const double r = part_r[(int64_t)e * wgs + w];
    const int64_t i = part_i[(int64_t)e * wgs + w];
    if (opt_better(r, i, br, bi)) { br = r; bi = i; }
  }
  opt_block_best<OPT_REDUCE_BLOCK>(br, bi);
  if (threadIdx.x == 0) {
    best_index[e] = bi;
    best_reward[e] = br;
  }
}

// grid (chunks, E): out[e][j] = reward of index first + j.  Tables read from global memory (a table of 16 RBs may not
// fit beside the slots); thread slots in LDS: n + C of them.
__global__ __launch_bounds__(OPT_BLOCK) void k_opt_rewards(OptParams q, const double* __restrict__ tabs, int64_t first,
                                                           int64_t count, double* out) {
  extern __shared__ double opt_lds[];
  const int e = blockIdx.y;
  const double* tab = tabs + (int64_t)e * q.tab;
  double* st = opt_lds + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * OPT_BLOCK;
  for (int64_t j = (int64_t)blockIdx.x * OPT_BLOCK + threadIdx.x; j < count; j += stride) {
    uint64_t lo, hi;
    opt_decode_prefix(first + j, q.n, q.C, lo, hi);
    opt_prefix_init(q, tab, lo, hi, st, OPT_BLOCK);
    out[(int64_t)e * count + j] = opt_eval(q, tab, lo, hi, 0, st, OPT_BLOCK);
  }
}

// ---------------------------------------------------------------------------------------------------------------- host

struct OptPlan {
  OptParams q;
  int64_t total;        // C^n, or -1 above OPT_MAX_INDEX
  int64_t n_pre, n_suf; // search: C^p prefixes, C^m suffixes
  int wgs;              // search workgroups per state
  size_t lds;           // search dynamic LDS bytes
};

inline int64_t opt_ipow(int64_t C, int k, int64_t cap) {   // C^k, or -1 above cap
  int64_t v = 1;
  for (int i = 0; i < k; ++i) {
    if (v > cap / C) return -1;
    v *= C;
  }
  return v;
}

inline size_t opt_search_lds(const OptParams& q, int m) {
  const int64_t slots = (q.n - m) + (int64_t)m * q.C + q.C;
  return (size_t)(((q.tab + 1) & ~1ll) + slots * OPT_BLOCK) * sizeof(double);
}

int opt_plan(const v2x_opt_problem* p, const char* who, OptPlan& pl) {
  if (!p) OPT_FAIL(V2X_EINVAL, "%s: null problem", who);
  if (p->E < 1 || p->E > 65535) OPT_FAIL(V2X_EINVAL, "%s: E = %d states (1..65535)", who, p->E);
  if (p->n < 1 || p->n > OPT_MAX_N) OPT_FAIL(V2X_EINVAL, "%s: n = %d links (1..%d)", who, p->n, OPT_MAX_N);
  if (p->rb < OPT_MIN_C || p->rb > OPT_MAX_C) OPT_FAIL(V2X_EINVAL, "%s: rb = %d channels (%d..%d)", who, p->rb, OPT_MIN_C, OPT_MAX_C);
  OptParams& q = pl.q;
  q.n = p->n;
  q.C = p->rb;
  q.nr = std::min(p->rb, p->n);
  q.tab = opt_tab_doubles(q.n, q.C);
  q.sig2 = p->sig2;
  q.w_v2v = p->w_v2v;
  q.w_v2i = p->w_v2i;
  pl.total = opt_ipow(q.C, q.n, OPT_MAX_INDEX);
  // search plan: walk more suffix digits per thread while the launch has more prefixes than it needs
  int m = 0;
  const int64_t want = std::max<int64_t>(1, OPT_TARGET_THREADS / p->E);
  while (m < q.n && m < OPT_MAX_SUFFIX && opt_search_lds(q, m + 1) <= OPT_LDS_CAP) {
    const int64_t pre = opt_ipow(q.C, q.n - m, OPT_MAX_INDEX);
    if (pre >= 0 && pre <= want) break;
    ++m;
  }
  q.m = m;
  q.p = q.n - m;
  pl.n_pre = opt_ipow(q.C, q.p, OPT_MAX_INDEX);
  pl.n_suf = opt_ipow(q.C, m, OPT_MAX_INDEX);
  const int64_t wgs_cap = std::max<int64_t>(1, OPT_MAX_WGS / p->E);
  pl.wgs = (int)std::min<int64_t>(pl.n_pre < 0 ? wgs_cap : (pl.n_pre + OPT_BLOCK - 1) / OPT_BLOCK, wgs_cap);
  pl.lds = opt_search_lds(q, m);
  return V2X_OK;
}

int64_t opt_tables_bytes(const v2x_opt_problem* p, const OptPlan& pl) {
  return ((int64_t)p->E * pl.q.tab * (int64_t)sizeof(double) + 255) & ~255ll;
}

int opt_prep(const v2x_opt_problem* p, const OptPlan& pl, void* workspace, hipStream_t stream, const char* who) {
  if (!workspace) OPT_FAIL(V2X_EINVAL, "%s: null workspace", who);
  if (!p->v2v_ff || !p->v2i_ff || !p->v2i_abs || !p->dest) OPT_FAIL(V2X_EINVAL, "%s: null input array", who);
  OptPrepArgs a;
  a.v2v_ff = p->v2v_ff;
  a.v2i_ff = p->v2i_ff;
  a.v2i_abs = p->v2i_abs;
  a.dest = p->dest;
  a.p_v2v = p->p_v2v;
  a.p_v2i = p->p_v2i;
  a.veh_gain = p->veh_gain;
  a.bs_gain = p->bs_gain;
  a.bs_nf = p->bs_nf;
  a.veh_nf = p->veh_nf;
  a.sig2 = p->sig2;
  a.n = pl.q.n;
  a.C = pl.q.C;
  a.tab = pl.q.tab;
  a.tabs = (double*)workspace;
  const dim3 grid((unsigned)((pl.q.tab + OPT_PREP_BLOCK - 1) / OPT_PREP_BLOCK), (unsigned)p->E);
  hipLaunchKernelGGL(k_opt_prep, grid, dim3(OPT_PREP_BLOCK), 0, stream, a);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) OPT_FAIL(V2X_EHIP, "%s: prep launch failed: %s", who, hipGetErrorString(err));
  return V2X_OK;
}

}  // namespace

extern "C" {

int64_t v2x_opt_workspace_bytes(const v2x_opt_problem* p) {
  OptPlan pl;
  if (opt_plan(p, "opt_workspace_bytes", pl) != V2X_OK) return V2X_EINVAL;
  return opt_tables_bytes(p, pl) + (int64_t)p->E * pl.wgs * (int64_t)(sizeof(double) + sizeof(int64_t));
}

int v2x_opt_search(const v2x_opt_problem* p, void* workspace, int64_t* best_index, double* best_reward, void* stream) {
  OptPlan pl;
  int rc = opt_plan(p, "opt_search", pl);
  if (rc != V2X_OK) return rc;
  if (pl.total < 0 || pl.total > OPT_MAX_SEARCH)
    OPT_FAIL(V2X_EINVAL, "opt_search: %d^%d joint actions exceed the search limit of 2^36", pl.q.C, pl.q.n);
  if (!best_index || !best_reward) OPT_FAIL(V2X_EINVAL, "opt_search: null output");
  if (pl.lds > OPT_LDS_CAP) OPT_FAIL(V2X_EINVAL, "opt_search: %zu bytes of LDS needed (n = %d, rb = %d)", pl.lds, pl.q.n, pl.q.C);
  hipStream_t s = (hipStream_t)stream;
  rc = opt_prep(p, pl, workspace, s, "opt_search");
  if (rc != V2X_OK) return rc;
  const double* tabs = (const double*)workspace;
  double* part_r = (double*)((char*)workspace + opt_tables_bytes(p, pl));
  int64_t* part_i = (int64_t*)(part_r + (int64_t)p->E * pl.wgs);
  hipLaunchKernelGGL(k_opt_search, dim3((unsigned)pl.wgs, (unsigned)p->E), dim3(OPT_BLOCK), pl.lds, s, pl.q, tabs, pl.n_pre,
                     pl.n_suf, part_r, part_i);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) OPT_FAIL(V2X_EHIP, "opt_search: search launch failed: %s", hipGetErrorString(err));
  hipLaunchKernelGGL(k_opt_reduce, dim3((unsigned)p->E), dim3(OPT_REDUCE_BLOCK), 0, s, part_r, part_i, pl.wgs, best_index,
                     best_reward);
  err = hipGetLastError();
  if (err != hipSuccess) OPT_FAIL(V2X_EHIP, "opt_search: reduce launch failed: %s", hipGetErrorString(err));
  return V2X_OK;
}

int v2x_opt_rewards(const v2x_opt_problem* p, void* workspace, int64_t first, int64_t count, double* out, void* stream) {
  OptPlan pl;
  int rc = opt_plan(p, "opt_rewards", pl);
  if (rc != V2X_OK) return rc;
  if (pl.total < 0) OPT_FAIL(V2X_EINVAL, "opt_rewards: %d^%d joint actions exceed 2^62 (64-bit indices)", pl.q.C, pl.q.n);
  if (first < 0 || count < 1 || count > pl.total - first)
    OPT_FAIL(V2X_EINVAL, "opt_rewards: range [%lld, %lld + %lld) outside [0, %lld)", (long long)first, (long long)first,
             (long long)count, (long long)pl.total);
  if (count > INT64_MAX / 8 / p->E) OPT_FAIL(V2X_EINVAL, "opt_rewards: E * count = %d * %lld outputs", p->E, (long long)count);
  if (!out) OPT_FAIL(V2X_EINVAL, "opt_rewards: null output");
  hipStream_t s = (hipStream_t)stream;
  rc = opt_prep(p, pl, workspace, s, "opt_rewards");
  if (rc != V2X_OK) return rc;
  OptParams q = pl.q;
  q.m = 0;
  q.p = q.n;
  const size_t lds = (size_t)(q.n + q.C) * OPT_BLOCK * sizeof(double);
  const unsigned chunks = (unsigned)std::min<int64_t>((count + OPT_BLOCK - 1) / OPT_BLOCK, OPT_REWARDS_WGS);
  hipLaunchKernelGGL(k_opt_rewards, dim3(chunks, (unsigned)p->E), dim3(OPT_BLOCK), lds, s, q, (const double*)workspace, first,
                     count, out);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) OPT_FAIL(V2X_EHIP, "opt_rewards: launch failed: %s", hipGetErrorString(err));
  return V2X_OK;
}

}  // extern "C"
