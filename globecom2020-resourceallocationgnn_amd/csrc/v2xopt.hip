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
//   k_opt_landscape, k_opt_landscape_reduce  the search's walk, kept as a histogram of all rewards and their sum
//                 (v2x_opt_landscape; described above its kernels)
//   k_opt_bound_* the same optimum by branch and bound (v2x_opt_search_bound; described above its kernels)
//   k_opt_count_* the joint actions above / at given thresholds, counted over the same tree (v2x_opt_count_bound; described
//                 above its kernels)
//   k_opt_local_* a near-optimal allocation for up to 128 links by multi-start local search (v2x_opt_search_local; described
//                 above its kernels), k_opt_rewards_actions: the reward of joint actions given as channel arrays
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

// ---------------------------------------------------------------------------------------------------- reward landscape
// v2x_opt_landscape: a histogram of ALL C^N rewards of a state over caller-given edges, and their fp64 sum.  The walk is
// k_opt_search's (same plan, same LDS layout, same opt_decode_prefix / opt_prefix_init / opt_eval calls), so every reward
// has the bits v2x_opt_rewards returns for its index.
//
// Slots: slot(r) = number of edges j with edges[j] <= r, i.e. 0 .. n_edges; a NaN reward takes slot n_edges + 1 (a NaN edge
// never satisfies <=).  nb = n_edges + 2 <= 64 slots.
//
// Counting is integer only and needs neither LDS nor atomics: lane b of every wave owns the 64-bit counter of slot b.
// Per evaluated action each lane computes its slot (edge k is kept in lane k and read with v_readlane: no memory access
// in the loop), then for b = 0 .. nb - 1
// the wave takes popcount(ballot(slot == b)) and lane b adds it.  Because a lane owns a counter whether or not it has
// a prefix to walk, the grid-stride loop runs per WAVE (its base prefix is wave-uniform): every lane iterates while lane 0
// of the wave has work, and a lane past n_pre evaluates nothing and votes slot -1, which matches no b.
//
// Sum: per thread in ascending index order, then a wave butterfly (the same bits in every lane), then wave 0 + wave 1: one
// partial per workgroup; k_opt_landscape_reduce adds the partials per thread in ascending order, then the same butterfly
// and the waves in order.  The order depends on the plan (hence on E) and on nothing else.

__device__ __forceinline__ uint64_t opt_suffix_next(uint64_t s, int m, int C) {   // odometer step, link n - 1 fastest
  for (int d = m - 1; d >= 0; --d) {
    if (opt_sdigit(s, d) + 1 < C) return s + (1ull << (4 * d));
    s &= ~(15ull << (4 * d));
  }
  return s;
}

__device__ __forceinline__ double opt_wave_sum(double x) {
#pragma clang fp contract(off)
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
  return x;
}

// grid (wgs, E), LDS as k_opt_search.  part_c [E][wgs][64], part_s [E][wgs].
__global__ __launch_bounds__(OPT_BLOCK) void k_opt_landscape(OptParams q, const double* __restrict__ tabs, int64_t n_pre,
                                                             int64_t n_suf, const double* __restrict__ edges, int n_edges,
                                                             int64_t* part_c, double* part_s) {
#pragma clang fp contract(off)
  extern __shared__ double opt_lds[];
  const int e = blockIdx.y;
  const double* src = tabs + (int64_t)e * q.tab;
  for (int64_t i = threadIdx.x; i < q.tab; i += OPT_BLOCK) opt_lds[i] = src[i];
  __syncthreads();
  const int64_t tab_pad = (q.tab + 1) & ~1ll;
  double* st = opt_lds + tab_pad + threadIdx.x;
  const double* ed = edges + (int64_t)e * n_edges;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nb = n_edges + 2;
  const double my_edge = lane < n_edges ? ed[lane] : 0.0;   // edge k lives in lane k: read back wave-uniformly below
  const int edge_lo = __double2loint(my_edge), edge_hi = __double2hiint(my_edge);
  int64_t cnt = 0;                                       // the counter of slot `lane`
  double sum = 0.0;
  const int64_t stride = (int64_t)gridDim.x * OPT_BLOCK;
  for (int64_t tb = (int64_t)blockIdx.x * OPT_BLOCK + wave * 64; tb < n_pre; tb += stride) {   // wave-uniform
    const int64_t t = tb + lane;
    const bool work = t < n_pre;
    uint64_t lo = 0, hi = 0;
    if (work) {
      opt_decode_prefix(t, q.p, q.C, lo, hi);
      opt_prefix_init(q, opt_lds, lo, hi, st, OPT_BLOCK);
    }
    uint64_t s = 0;
    for (int64_t j = 0; j < n_suf; ++j) {
      int slot = -1;
      if (work) {
        const double r = opt_eval(q, opt_lds, lo, hi, s, st, OPT_BLOCK);
        sum += r;
        if (r != r) {
          slot = n_edges + 1;
        } else {
          slot = 0;
          for (int k = 0; k < n_edges; ++k)
            slot += __hiloint2double(__builtin_amdgcn_readlane(edge_hi, k), __builtin_amdgcn_readlane(edge_lo, k)) <= r ? 1 : 0;
        }
      }
      for (int b = 0; b < nb; ++b) {
        const int c = __popcll(__ballot(slot == b));
        if (lane == b) cnt += c;
      }
      s = opt_suffix_next(s, q.m, q.C);
    }
  }
  sum = opt_wave_sum(sum);
  // wave 1 hands its counters and its sum to wave 0 through the thread slots, which nobody reads any more (at least
  // n + C >= 3 slots of OPT_BLOCK doubles; counters travel as bit patterns)
  __syncthreads();
  double* hand = opt_lds + tab_pad;
  if (wave == 1) {
    hand[lane] = __longlong_as_double((long long)cnt);
    if (lane == 0) hand[64] = sum;
  }
  __syncthreads();
  if (wave == 0) {
    const int64_t w = (int64_t)e * gridDim.x + blockIdx.x;
    part_c[w * 64 + lane] = cnt + (int64_t)__double_as_longlong(hand[lane]);
    if (lane == 0) part_s[w] = sum + hand[64];
  }
}

// grid E: counts[e][b] = sum over the workgroups' partials (integers: any order), sums[e] in a fixed order
__global__ __launch_bounds__(OPT_REDUCE_BLOCK) void k_opt_landscape_reduce(const int64_t* part_c, const double* part_s, int wgs,
                                                                           int nb, int64_t* counts, double* sums) {
#pragma clang fp contract(off)
  __shared__ int64_t sc[OPT_REDUCE_BLOCK];
  __shared__ double ss[OPT_REDUCE_BLOCK / 64];
  const int e = blockIdx.x;
  const int b = threadIdx.x & 63, part = threadIdx.x >> 6;
  int64_t c = 0;
  for (int w = part; w < wgs; w += OPT_REDUCE_BLOCK / 64) c += part_c[((int64_t)e * wgs + w) * 64 + b];
  sc[threadIdx.x] = c;
  double x = 0.0;
  for (int w = threadIdx.x; w < wgs; w += OPT_REDUCE_BLOCK) x += part_s[(int64_t)e * wgs + w];
  x = opt_wave_sum(x);
  if (b == 0) ss[part] = x;
  __syncthreads();
  if (part == 0 && b < nb) {
    for (int k = 1; k < OPT_REDUCE_BLOCK / 64; ++k) c += sc[k * 64 + b];
    counts[(int64_t)e * nb + b] = c;
  }
  if (threadIdx.x == 0 && sums) {
    for (int k = 1; k < OPT_REDUCE_BLOCK / 64; ++k) x += ss[k];
    sums[e] = x;
  }
}

// ------------------------------------------------------------------------------------------------ branch and bound
// The same optimum without enumerating C^N joint actions (v2x_opt_search_bound): a depth-first search over the links in
// their natural order, link d branched at depth d, with an admissible upper bound on every completion of a prefix.
//
// Node state of a lane (its slots, in LDS):  I[l][c] = tx[l][c] + sum over ASSIGNED k != l on c of cross[l][k][c]
// for every link l and channel c, and B[r] = sum over assigned k on r of bs[k][r].  Both are left folds over ascending k, as
// in opt_prefix_init: descending appends the largest k, and backtracking recomputes the one column that changed from
// scratch, so a slot's bits depend on the prefix alone, never on the path that led to it.  That makes the order of a node's
// children (by own rate sig / (I + sig2), descending, lower channel first among equals) a function of the prefix too: a
// lane needs no stack beyond the prefix digits, and a suspended search resumes from (root depth, depth, digits).
//
// Bound of a prefix of d links (every factor can only fall as more links are assigned, because interference only grows):
//   ub = w_v2v * log2( prod_{l < d} (1 + sig[l][a_l] / (I[l][a_l] + sig2)) * prod_{l >= d} (1 + max_c sig[l][c] / (I[l][c] + sig2)) )
//      + w_v2i * log2( prod_{r < nr} (1 + v2i[r] / (B[r] + sig2)) )
// -- the sum of every rate's own bound, each sum of logarithms taken as ONE logarithm of a product (two log2, not
// N * C + C, per node; a product that overflows gives ub = inf, which never prunes).
//
// Rounding margin.  u = 2^-53.  I is a sum of <= N positive terms (relative error <= N u), + sig2, the quotient and 1 + x
// add 3 u: each factor is within (N + 3) u; a product of N of them within N (N + 4) u; so log2 of the product is off by at
// most 1.4427 * N (N + 4) u <= 1.9e-13 absolutely (N = 32), per unit weight.  A leaf's sum of N logarithms carries the same
// (N + 3) u per argument, hence the same absolute 1.9e-13 per unit weight, plus relative terms: log2's own rounding, the
// N + C additions and the two weights, <= (N + C + 8) u <= 6.3e-15.  OPT_BOUND_EPS = 2^-40 = 9.1e-13 is used BOTH as the
// absolute margin per unit weight (> 2 * 1.9e-13) and as the relative margin (> 140 times 6.3e-15).  A node is pruned only
// when  ub * (1 + EPS) + EPS * (w_v2v + w_v2i) < incumbent,  strictly: every completion then scores strictly below the
// incumbent as a leaf would score it, so neither a better action nor an equal one with a lower index is lost.
//
// Launches of one round, all on the caller's stream (the host reads two counters back per round, nothing else):
//   k_opt_bound_search   lanes take work items (state, root depth, depth, prefix digits) through an integer counter and run
//                        the depth-first search of each for at most `cap` nodes.  An unfinished item goes back into the
//                        item's own slot of the output queue; while the queue has room its untried siblings along the
//                        path are split off as items of their own first (that is the breadth-first seeding: round 0 runs
//                        the root for N + 1 nodes, a greedy dive to the first leaf = the first incumbent).  Leaves are
//                        scored with opt_prefix_init / opt_eval; the incumbent's bit pattern is shared per state with a
//                        64-bit integer atomicMax; a lane whose best leaf equals the incumbent when its item ends appends
//                        (state, index, bits) to the round's candidate list.
//   k_opt_bound_fold_a/b per state: forget the index when the incumbent rose; per candidate that still equals the
//                        incumbent: integer atomicMin on the index = opt_better's rule among equal rewards.
//   k_opt_bound_compact  output queue (with holes: finished items, failed reservations) -> dense input queue of the next
//                        round, one integer atomic per wave.
// Every loop is bounded: a lane visits <= cap nodes per item and an item runs once per launch.

constexpr int OPTB_BLOCK = 64;                    // one wave per workgroup: lanes diverge freely, nothing is shared
constexpr int OPTB_QCAP = 1 << 18;                // work items of a queue
constexpr int OPTB_CUS = 256;                     // search workgroups: as many per CU as their LDS allows, 3 at most
constexpr size_t OPTB_LDS_CU = 160 * 1024;        // LDS of a CU; a workgroup may take all of it (15 x 16: 128 KiB of slots)
constexpr int OPTB_CAP_SEED = 256;                // nodes per item and launch while the queue is short of items ...
constexpr int OPTB_CAP_RUN = 4096;                // ... and once every lane has several
constexpr int OPTB_ITEMS_PER_LANE = 4;            // split suspended items while the queue holds fewer than this per lane
constexpr int OPTB_POLL = 16;                     // nodes between two reads of the shared incumbent
constexpr double OPT_BOUND_EPS = 0x1p-40;         // see "Rounding margin" above
constexpr unsigned long long OPTB_NO_INDEX = (unsigned long long)INT64_MAX;

struct OptItem {            // 32 bytes; e < 0: a hole
  uint64_t lo, hi;          // digits of links 0 .. d - 1
  int32_t e;                // state
  int16_t d0, d;            // the item's root depth (never backtracked above), depth of the node to visit next
  int64_t pad_;
};
struct OptCand {
  unsigned long long bits;  // reward bit pattern
  int64_t idx;
  int32_t e, pad_;
};
enum { OPTB_HEAD = 0, OPTB_TAIL = 1, OPTB_NCAND = 2, OPTB_OUT = 3, OPTB_NODES = 4, OPTB_CTRL = 8 };

struct OptBoundArgs {
  OptParams q;                      // p = n, m = 0: the leaf's opt_prefix_init / opt_eval
  const double* tabs;
  const OptItem* qin;
  OptItem* qout;
  int n_in, cap, allow_split;
  unsigned long long* ctrl;         // OPTB_* counters
  unsigned long long* inc;          // [E] incumbent reward bits
  OptCand* cand;
  double* leaf;                     // [n + C][lanes] scratch of opt_prefix_init
};

struct OptSlots {             // slot i of this lane: lane-strided, so a wave's lanes hit consecutive words
  double* base;
  __device__ __forceinline__ double& operator[](int i) const { return base[i * OPTB_BLOCK]; }
};

__device__ __forceinline__ void opt_set_digit(uint64_t& lo, uint64_t& hi, int l, int c) {
  if (l < 16) lo = (lo & ~(15ull << (4 * l))) | ((uint64_t)c << (4 * l));
  else hi = (hi & ~(15ull << (4 * (l - 16)))) | ((uint64_t)c << (4 * (l - 16)));
}

// tx[l][c] + sum over k < dlim, k != l, on channel c of cross[l][k][c], ascending k
__device__ __forceinline__ double opt_row_fold(const OptParams& q, const double* __restrict__ tab, uint64_t lo, uint64_t hi,
                                               int l, int c, int dlim) {
  const int n = q.n, C = q.C;
  const double* cross = tab + 3ll * n * C;
  double acc = tab[(int64_t)n * C + l * C + c];
  for (int k = 0; k < dlim; ++k)
    if (k != l && opt_digit(lo, hi, k) == c) acc += cross[(l * n + k) * C + c];
  return acc;
}

// the child after `cur` (cur < 0: the first) in the order: key descending, lower channel first among equal keys; -1: none
template <class Key>
__device__ __forceinline__ int opt_pick_child(Key key, int C, int cur) {
  const double xc = cur >= 0 ? key(cur) : 0.0;
  int best = -1;
  double xb = 0.0;
  for (int c = 0; c < C; ++c) {
    const double x = key(c);
    if (cur >= 0 && !(x < xc || (x == xc && c > cur))) continue;
    if (best < 0 || x > xb) { best = c; xb = x; }
  }
  return best;
}

// LDS: [the state's table when TAB_LDS (one state, E = 1: every item reads the same table)] [n * C + C slots x 64 lanes].
// Measured, ten 20-link states: median 317 ms per state with the table read from global memory, 251 ms from LDS; 147 ms
// with the folds restructured (column-wise, only the links on the channel) and the quotients of the bound four in flight.
template <bool TAB_LDS>
__global__ __launch_bounds__(OPTB_BLOCK) void k_opt_bound_search(OptBoundArgs a) {
#pragma clang fp contract(off)
  extern __shared__ double opt_lds[];
  const OptParams q = a.q;
  const int n = q.n, C = q.C, nr = q.nr;
  const int64_t lanes = (int64_t)gridDim.x * OPTB_BLOCK, lane = (int64_t)blockIdx.x * OPTB_BLOCK + threadIdx.x;
  const int64_t tab_pad = TAB_LDS ? ((q.tab + 1) & ~1ll) : 0;
  if constexpr (TAB_LDS) {
    for (int64_t i = threadIdx.x; i < q.tab; i += OPTB_BLOCK) opt_lds[i] = a.tabs[i];
    __syncthreads();
  }
  OptSlots S;
  S.base = opt_lds + tab_pad + threadIdx.x;
  double* lf = a.leaf + lane;
  unsigned long long visited = 0;
  for (;;) {                                                   // <= n_in items in all lanes together
    const unsigned long long it = atomicAdd(&a.ctrl[OPTB_HEAD], 1ull);
    if (it >= (unsigned long long)a.n_in) break;
    const OptItem item = a.qin[it];
    const int e = item.e, d0 = item.d0;
    int d = item.d;
    uint64_t lo = item.lo, hi = item.hi;
    const double* tab = TAB_LDS ? opt_lds : a.tabs + (int64_t)e * q.tab;
    const double* sig = tab;
    const double* tx = tab + (int64_t)n * C;
    const double* bs = tab + 2ll * n * C;
    const double* cross = tab + 3ll * n * C;
    const double* v2i = cross + (int64_t)n * n * C;
    // the folds of opt_row_fold for every (l, c) at once: per slot the same additions in the same (ascending k) order
    for (int i = 0; i < n * C; ++i) S[i] = tx[i];
    for (int k = 0; k < d; ++k) {
      const int c = opt_digit(lo, hi, k);
      for (int l = 0; l < n; ++l)
        if (l != k) S[l * C + c] += cross[(l * n + k) * C + c];
    }
    for (int r = 0; r < C; ++r) {
      double acc = 0.0;
      if (r < nr)
        for (int k = 0; k < d; ++k)
          if (opt_digit(lo, hi, k) == r) acc += bs[k * C + r];
      S[n * C + r] = acc;
    }
    double incumbent = __longlong_as_double((long long)__hip_atomic_load(&a.inc[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    double lr = -1.0;                                          // best leaf of this run of the item
    int64_t li = INT64_MAX;
    int cnt = 0;
    bool visit = true, finished = false;
    // every iteration visits a node (<= cap of them) or steps one level back (<= n in a row)
    for (;;) {
      if (visit) {
        if (cnt >= a.cap) break;                               // suspended: the node at depth d is still to visit
        ++cnt;
        if (d == n) {                                          // leaf: the exhaustive search's own arithmetic
          opt_prefix_init(q, tab, lo, hi, lf, (int)lanes);
          const double r = opt_eval(q, tab, lo, hi, 0, lf, (int)lanes);
          if (r >= 0.0) {                                      // (not NaN)
            int64_t idx = 0;
            for (int l = 0; l < n; ++l) idx = idx * C + opt_digit(lo, hi, l);
            const unsigned long long bits = (unsigned long long)__double_as_longlong(r);
            const unsigned long long old = atomicMax(&a.inc[e], bits);
            incumbent = __longlong_as_double((long long)(old > bits ? old : bits));
            if (opt_better(r, idx, lr, li)) { lr = r; li = idx; }
          }
          visit = false;
          continue;
        }
        if ((cnt & (OPTB_POLL - 1)) == 0)
          incumbent = __longlong_as_double((long long)__hip_atomic_load(&a.inc[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        double pv = 1.0, pi = 1.0;
        // independent quotients, four in flight: at one wave per SIMD nothing else hides the divide's latency
#pragma unroll 4
        for (int l = 0; l < d; ++l) {
          const int c = opt_digit(lo, hi, l);
          pv *= 1.0 + sig[l * C + c] / (S[l * C + c] + q.sig2);
        }
        for (int l = d; l < n; ++l) {
          double x = 0.0;
#pragma unroll 4
          for (int c = 0; c < C; ++c) x = fmax(x, sig[l * C + c] / (S[l * C + c] + q.sig2));
          pv *= 1.0 + x;
        }
#pragma unroll 4
        for (int r = 0; r < nr; ++r) pi *= 1.0 + v2i[r] / (S[n * C + r] + q.sig2);
        const double ub = q.w_v2v * log2(pv) + q.w_v2i * log2(pi);
        if (ub * (1.0 + OPT_BOUND_EPS) + OPT_BOUND_EPS * (q.w_v2v + q.w_v2i) < incumbent) {
          visit = false;
          continue;
        }
        const int c = opt_pick_child([&](int cc) { return sig[d * C + cc] / (S[d * C + cc] + q.sig2); }, C, -1);
        for (int l = 0; l < n; ++l)
          if (l != d) S[l * C + c] += cross[(l * n + d) * C + c];
        if (c < nr) S[n * C + c] += bs[d * C + c];
        opt_set_digit(lo, hi, d, c);
        ++d;
      } else {
        if (d == d0) { finished = true; break; }
        const int k = d - 1, c = opt_digit(lo, hi, k);
        d = k;
        for (int l = 0; l < n; ++l) S[l * C + c] = tx[l * C + c];          // column c again from scratch (opt_row_fold's order)
        for (int kk = 0; kk < d; ++kk)
          if (opt_digit(lo, hi, kk) == c)
            for (int l = 0; l < n; ++l)
              if (l != kk) S[l * C + c] += cross[(l * n + kk) * C + c];
        if (c < nr) {
          double acc = 0.0;
          for (int kk = 0; kk < d; ++kk)
            if (opt_digit(lo, hi, kk) == c) acc += bs[kk * C + c];
          S[n * C + c] = acc;
        }
        const int c2 = opt_pick_child([&](int cc) { return sig[k * C + cc] / (S[k * C + cc] + q.sig2); }, C, c);
        if (c2 >= 0) {
          for (int l = 0; l < n; ++l)
            if (l != k) S[l * C + c2] += cross[(l * n + k) * C + c2];
          if (c2 < nr) S[n * C + c2] += bs[k * C + c2];
          opt_set_digit(lo, hi, k, c2);
          d = k + 1;
          visit = true;
        }
      }
    }
    visited += (unsigned long long)cnt;
    if (lr >= 0.0) {
      const unsigned long long bits = (unsigned long long)__double_as_longlong(lr);
      if (bits == __hip_atomic_load(&a.inc[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
        const unsigned long long at = atomicAdd(&a.ctrl[OPTB_NCAND], 1ull);     // <= one per item: at < n_in <= OPTB_QCAP
        OptCand cd;
        cd.bits = bits;
        cd.idx = li;
        cd.e = e;
        cd.pad_ = 0;
        a.cand[at] = cd;
      }
    }
    OptItem back;
    back.lo = lo;
    back.hi = hi;
    back.e = finished ? -1 : e;
    back.d0 = (int16_t)d0;
    back.d = (int16_t)d;
    back.pad_ = 0;
    if (!finished && a.allow_split && d > d0) {
      // the untried siblings along the path d0 .. d - 1 become items of their own, the node at depth d its own root.
      // A sibling of link j is ordered by link j's keys at the prefix of j links: the same bits the search would see.
      int need = 0;
      for (int j = d0; j < d; ++j) {
        const int cj = opt_digit(lo, hi, j);
        const double xc = sig[j * C + cj] / (opt_row_fold(q, tab, lo, hi, j, cj, j) + q.sig2);
        for (int c = 0; c < C; ++c) {
          const double x = sig[j * C + c] / (opt_row_fold(q, tab, lo, hi, j, c, j) + q.sig2);
          if (x < xc || (x == xc && c > cj)) ++need;
        }
      }
      const unsigned long long at = a.n_in + atomicAdd(&a.ctrl[OPTB_TAIL], (unsigned long long)need);
      if (at + need <= (unsigned long long)OPTB_QCAP) {
        unsigned long long w = at;
        for (int j = d0; j < d; ++j) {
          const int cj = opt_digit(lo, hi, j);
          const double xc = sig[j * C + cj] / (opt_row_fold(q, tab, lo, hi, j, cj, j) + q.sig2);
          for (int c = 0; c < C; ++c) {
            const double x = sig[j * C + c] / (opt_row_fold(q, tab, lo, hi, j, c, j) + q.sig2);
            if (x < xc || (x == xc && c > cj)) {
              OptItem sib;
              sib.lo = j < 16 ? (lo & ((1ull << (4 * j)) - 1)) : lo;
              sib.hi = j < 16 ? 0ull : (hi & ((1ull << (4 * (j - 16))) - 1));
              opt_set_digit(sib.lo, sib.hi, j, c);
              sib.e = e;
              sib.d0 = sib.d = (int16_t)(j + 1);
              sib.pad_ = 0;
              a.qout[w++] = sib;
            }
          }
        }
        back.d0 = (int16_t)d;
      } else {                                                 // no room: holes where the reservation lies inside the queue
        OptItem hole;
        hole.lo = hole.hi = 0;
        hole.e = -1;
        hole.d0 = hole.d = 0;
        hole.pad_ = 0;
        for (unsigned long long w = at; w < at + need && w < (unsigned long long)OPTB_QCAP; ++w) a.qout[w] = hole;
      }
    }
    a.qout[it] = back;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) visited += __shfl_xor(visited, off, 64);
  if (threadIdx.x == 0 && visited) atomicAdd(&a.ctrl[OPTB_NODES], visited);
}

// grid ceil(E / 256): a fresh search -- one root item per state, no incumbent
__global__ __launch_bounds__(256) void k_opt_bound_init(int E, OptItem* q0, unsigned long long* inc, unsigned long long* best_idx,
                                                        unsigned long long* idx_bits, unsigned long long* ctrl) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < OPTB_CTRL) ctrl[e] = 0;
  if (e >= E) return;
  OptItem it;
  it.lo = it.hi = 0;
  it.e = e;
  it.d0 = it.d = 0;
  it.pad_ = 0;
  q0[e] = it;
  inc[e] = 0;                                  // +0.0: rewards are >= 0
  best_idx[e] = OPTB_NO_INDEX;
  idx_bits[e] = ~0ull;
}

// grid-stride over the states (v2x_opt_search_bound_seeded): the caller's start action of state e, scored as a leaf with
// the search's own arithmetic, becomes the incumbent, and its index the first candidate -- exactly the state a lane leaves
// behind that found this leaf.  A start with a channel outside [0, C) or a reward that is not a number seeds nothing.
// slots: [n + C][ld] scratch of opt_prefix_init, ld = threads of the launch.
__global__ __launch_bounds__(256) void k_opt_bound_seed(OptParams q, const double* __restrict__ tabs, int E,
                                                        const int32_t* __restrict__ start, unsigned long long* inc,
                                                        unsigned long long* best_idx, unsigned long long* idx_bits, double* slots) {
  const int ld = (int)(gridDim.x * 256), t = (int)(blockIdx.x * 256 + threadIdx.x);
  for (int e = t; e < E; e += ld) {
    uint64_t lo = 0, hi = 0;
    int64_t idx = 0;
    bool ok = true;
    for (int l = 0; l < q.n; ++l) {
      int c = start[(int64_t)e * q.n + l];
      if (c < 0 || c >= q.C) { ok = false; c = 0; }
      opt_set_digit(lo, hi, l, c);
      idx = idx * q.C + c;
    }
    if (!ok) continue;
    const double* tab = tabs + (int64_t)e * q.tab;
    opt_prefix_init(q, tab, lo, hi, slots + t, ld);
    const double r = opt_eval(q, tab, lo, hi, 0, slots + t, ld);
    if (r >= 0.0) {                                            // (not NaN)
      const unsigned long long bits = (unsigned long long)__double_as_longlong(r);
      inc[e] = bits;
      best_idx[e] = (unsigned long long)idx;
      idx_bits[e] = bits;
    }
  }
}

// grid ceil(E / 256): the index kept so far belongs to a reward the incumbent has passed
__global__ __launch_bounds__(256) void k_opt_bound_fold_a(int E, const unsigned long long* inc, unsigned long long* best_idx,
                                                          unsigned long long* idx_bits) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  if (idx_bits[e] != inc[e]) {
    idx_bits[e] = inc[e];
    best_idx[e] = OPTB_NO_INDEX;
  }
}

// grid-stride over the round's candidates: the lowest index among those equal to the incumbent
__global__ __launch_bounds__(256) void k_opt_bound_fold_b(const unsigned long long* ctrl, const OptCand* cand,
                                                          const unsigned long long* inc, unsigned long long* best_idx) {
  const unsigned long long nc = ctrl[OPTB_NCAND];
  for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < nc; i += (unsigned long long)gridDim.x * 256) {
    const OptCand cd = cand[i];
    if (cd.bits == inc[cd.e]) atomicMin(&best_idx[cd.e], (unsigned long long)cd.idx);
  }
}

// grid-stride, whole waves: src[0, min(n_in + tail, QCAP)) without its holes -> dst, count in ctrl[OPTB_OUT]
__global__ __launch_bounds__(256) void k_opt_bound_compact(int n_in, unsigned long long* ctrl, const OptItem* src, OptItem* dst) {
  const unsigned long long total = std::min<unsigned long long>((unsigned long long)n_in + ctrl[OPTB_TAIL], (unsigned long long)OPTB_QCAP);
  const int ln = threadIdx.x & 63;
  for (unsigned long long base = ((unsigned long long)blockIdx.x * 256 + threadIdx.x) - ln; base < total;
       base += (unsigned long long)gridDim.x * 256) {
    const unsigned long long i = base + ln;
    OptItem it;
    it.e = -1;
    if (i < total) it = src[i];
    const bool keep = i < total && it.e >= 0;
    const unsigned long long mask = __ballot(keep);
    unsigned long long at = 0;
    if (ln == 0 && mask) at = atomicAdd(&ctrl[OPTB_OUT], (unsigned long long)__popcll(mask));
    at = __shfl(at, 0, 64);
    if (keep) dst[at + __popcll(mask & ((1ull << ln) - 1ull))] = it;
  }
}

// grid ceil(E / 256)
__global__ __launch_bounds__(256) void k_opt_bound_finish(int E, const unsigned long long* inc, const unsigned long long* best_idx,
                                                          int64_t* best_index, double* best_reward) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  best_index[e] = (int64_t)best_idx[e];
  best_reward[e] = __longlong_as_double((long long)inc[e]);
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

// ---- reward landscape: workspace = tables | per-workgroup counters [E][wgs][64] | per-workgroup sums [E][wgs]
namespace {

int opt_landscape_plan(const v2x_opt_problem* p, int32_t n_edges, const char* who, OptPlan& pl) {
  int rc = opt_plan(p, who, pl);
  if (rc != V2X_OK) return rc;
  if (n_edges < 1 || n_edges > 62) OPT_FAIL(V2X_EINVAL, "%s: n_edges = %d (1..62)", who, n_edges);
  if (pl.total < 0 || pl.total > OPT_MAX_SEARCH)
    OPT_FAIL(V2X_EINVAL, "%s: %d^%d joint actions exceed the search limit of 2^36", who, pl.q.C, pl.q.n);
  if (pl.lds > OPT_LDS_CAP) OPT_FAIL(V2X_EINVAL, "%s: %zu bytes of LDS needed (n = %d, rb = %d)", who, pl.lds, pl.q.n, pl.q.C);
  return V2X_OK;
}

}  // namespace

extern "C" {

int64_t v2x_opt_landscape_workspace_bytes(const v2x_opt_problem* p, int32_t n_edges) {
  OptPlan pl;
  if (opt_landscape_plan(p, n_edges, "opt_landscape_workspace_bytes", pl) != V2X_OK) return V2X_EINVAL;
  return opt_tables_bytes(p, pl) + (int64_t)p->E * pl.wgs * (int64_t)(64 * sizeof(int64_t) + sizeof(double));
}

int v2x_opt_landscape(const v2x_opt_problem* p, void* workspace, const double* edges, int32_t n_edges, int64_t* counts,
                      double* sums, void* stream) {
  OptPlan pl;
  int rc = opt_landscape_plan(p, n_edges, "opt_landscape", pl);
  if (rc != V2X_OK) return rc;
  if (!edges) OPT_FAIL(V2X_EINVAL, "opt_landscape: null edges");
  if (!counts) OPT_FAIL(V2X_EINVAL, "opt_landscape: null output");
  hipStream_t s = (hipStream_t)stream;
  rc = opt_prep(p, pl, workspace, s, "opt_landscape");
  if (rc != V2X_OK) return rc;
  const double* tabs = (const double*)workspace;
  int64_t* part_c = (int64_t*)((char*)workspace + opt_tables_bytes(p, pl));
  double* part_s = (double*)(part_c + (int64_t)p->E * pl.wgs * 64);
  hipLaunchKernelGGL(k_opt_landscape, dim3((unsigned)pl.wgs, (unsigned)p->E), dim3(OPT_BLOCK), pl.lds, s, pl.q, tabs, pl.n_pre,
                     pl.n_suf, edges, (int)n_edges, part_c, part_s);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) OPT_FAIL(V2X_EHIP, "opt_landscape: landscape launch failed: %s", hipGetErrorString(err));
  hipLaunchKernelGGL(k_opt_landscape_reduce, dim3((unsigned)p->E), dim3(OPT_REDUCE_BLOCK), 0, s, part_c, part_s, pl.wgs,
                     (int)n_edges + 2, counts, sums);
  err = hipGetLastError();
  if (err != hipSuccess) OPT_FAIL(V2X_EHIP, "opt_landscape: reduce launch failed: %s", hipGetErrorString(err));
  return V2X_OK;
}

}  // extern "C"

// ---- branch and bound: workspace = tables | counters | per-state incumbent, index, index's reward | two queues | candidates
//      | leaf scratch
namespace {

struct OptBoundPlan {
  bool tab_lds;             // the table of the (one) state beside the slots in LDS
  int wgs;                  // workgroups of a search launch at most
  size_t lds_bytes;
  int64_t off_ctrl, off_inc, off_idx, off_bits, off_qa, off_qb, off_cand, off_leaf, bytes;
};

// need_index: the caller returns a joint action as a 64-bit index (the search); the counting search names none
int opt_bound_plan(const v2x_opt_problem* p, int64_t max_nodes, const char* who, OptPlan& pl, OptBoundPlan& bp,
                   bool need_index = true) {
  int rc = opt_plan(p, who, pl);
  if (rc != V2X_OK) return rc;
  if (need_index && pl.total < 0)
    OPT_FAIL(V2X_EINVAL, "%s: %d^%d joint actions exceed 2^62 (64-bit indices)", who, pl.q.C, pl.q.n);
  if (max_nodes < 1) OPT_FAIL(V2X_EINVAL, "%s: max_nodes = %lld (>= 1)", who, (long long)max_nodes);
  if (!(p->w_v2v >= 0.0) || !(p->w_v2i >= 0.0))
    OPT_FAIL(V2X_EINVAL, "%s: weights %g / %g (the bound needs both >= 0)", who, p->w_v2v, p->w_v2i);
  pl.q.p = pl.q.n;
  pl.q.m = 0;
  const int64_t slots = (int64_t)pl.q.n * pl.q.C + pl.q.C;
  bp.lds_bytes = (size_t)slots * OPTB_BLOCK * sizeof(double);       // <= 128 KiB: rb^n <= 2^62 caps n * rb + rb at 256
  const size_t with_tab = bp.lds_bytes + (size_t)((pl.q.tab + 1) & ~1ll) * sizeof(double);
  bp.tab_lds = p->E == 1 && with_tab <= OPTB_LDS_CU - 1024;
  if (bp.tab_lds) bp.lds_bytes = with_tab;
  if (bp.lds_bytes > OPTB_LDS_CU - 1024)
    OPT_FAIL(V2X_EINVAL, "%s: %zu bytes of LDS needed (n = %d, rb = %d)", who, bp.lds_bytes, pl.q.n, pl.q.C);
  bp.wgs = OPTB_CUS * (int)std::min<size_t>(3, (OPTB_LDS_CU - 1024) / bp.lds_bytes);
  const int64_t lanes = (int64_t)bp.wgs * OPTB_BLOCK;
  auto al = [](int64_t v) { return (v + 255) & ~255ll; };
  int64_t o = opt_tables_bytes(p, pl);
  bp.off_ctrl = o;  o += al(OPTB_CTRL * 8);
  bp.off_inc = o;   o += al((int64_t)p->E * 8);
  bp.off_idx = o;   o += al((int64_t)p->E * 8);
  bp.off_bits = o;  o += al((int64_t)p->E * 8);
  bp.off_qa = o;    o += al((int64_t)OPTB_QCAP * (int64_t)sizeof(OptItem));
  bp.off_qb = o;    o += al((int64_t)OPTB_QCAP * (int64_t)sizeof(OptItem));
  bp.off_cand = o;  o += al((int64_t)OPTB_QCAP * (int64_t)sizeof(OptCand));
  bp.off_leaf = o;  o += al((int64_t)(pl.q.n + pl.q.C) * lanes * 8);
  bp.bytes = o;
  return V2X_OK;
}

}  // namespace

extern "C" {

int64_t v2x_opt_bound_workspace_bytes(const v2x_opt_problem* p, int64_t max_nodes) {
  OptPlan pl;
  OptBoundPlan bp;
  if (opt_bound_plan(p, max_nodes, "opt_bound_workspace_bytes", pl, bp) != V2X_OK) return V2X_EINVAL;
  return bp.bytes;
}

}  // extern "C"

namespace {

// v2x_opt_search_bound (start_actions NULL: the launches it always made) and v2x_opt_search_bound_seeded
int opt_search_bound_impl(const v2x_opt_problem* p, void* workspace, int64_t max_nodes, const int32_t* start_actions,
                          int64_t* best_index, double* best_reward, int64_t* nodes_visited, void* stream) {
  OptPlan pl;
  OptBoundPlan bp;
  int rc = opt_bound_plan(p, max_nodes, "opt_search_bound", pl, bp);
  if (rc != V2X_OK) return rc;
  if (!best_index || !best_reward) OPT_FAIL(V2X_EINVAL, "opt_search_bound: null output");
  hipStream_t s = (hipStream_t)stream;
  rc = opt_prep(p, pl, workspace, s, "opt_search_bound");
  if (rc != V2X_OK) return rc;
  char* ws = (char*)workspace;
  unsigned long long* ctrl = (unsigned long long*)(ws + bp.off_ctrl);
  unsigned long long* inc = (unsigned long long*)(ws + bp.off_inc);
  unsigned long long* idx = (unsigned long long*)(ws + bp.off_idx);
  unsigned long long* bits = (unsigned long long*)(ws + bp.off_bits);
  OptItem* qa = (OptItem*)(ws + bp.off_qa);
  OptItem* qb = (OptItem*)(ws + bp.off_qb);
  const unsigned egrid = (unsigned)((p->E + 255) / 256);
  hipError_t err;
#define OPTB_LAUNCHED(what)                                                                                        \
  if ((err = hipGetLastError()) != hipSuccess)                                                                     \
  OPT_FAIL(V2X_EHIP, "opt_search_bound: %s failed: %s", what, hipGetErrorString(err))
  hipLaunchKernelGGL(k_opt_bound_init, dim3(egrid), dim3(256), 0, s, p->E, qa, inc, idx, bits, ctrl);
  OPTB_LAUNCHED("init launch");
  if (start_actions) {
    const int64_t lanes = (int64_t)bp.wgs * OPTB_BLOCK;          // the leaf scratch holds this many slot columns
    const unsigned sgrid = (unsigned)std::min<int64_t>(egrid, lanes / 256);
    hipLaunchKernelGGL(k_opt_bound_seed, dim3(sgrid), dim3(256), 0, s, pl.q, (const double*)workspace, p->E, start_actions, inc,
                       idx, bits, (double*)(ws + bp.off_leaf));
    OPTB_LAUNCHED("seed launch");
  }
  OptBoundArgs a;
  a.q = pl.q;
  a.tabs = (const double*)workspace;
  a.qin = qa;
  a.qout = qb;
  a.ctrl = ctrl;
  a.inc = inc;
  a.cand = (OptCand*)(ws + bp.off_cand);
  a.leaf = (double*)(ws + bp.off_leaf);
  if (bp.lds_bytes > 64 * 1024) {          // above the default dynamic-LDS size a kernel has to be told; the launch check decides
    if (bp.tab_lds) (void)hipFuncSetAttribute((const void*)k_opt_bound_search<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bp.lds_bytes);
    else (void)hipFuncSetAttribute((const void*)k_opt_bound_search<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bp.lds_bytes);
    (void)hipGetLastError();
  }
  const int64_t short_of = (int64_t)bp.wgs * OPTB_BLOCK * OPTB_ITEMS_PER_LANE;
  int64_t n_in = p->E, nodes = 0;
  // one round per pass; every round visits at least one node per item, so the node budget also bounds the rounds
  for (int64_t round = 0; n_in > 0 && nodes < max_nodes; ++round) {
    const bool few = n_in < short_of;
    a.n_in = (int)n_in;
    a.cap = round == 0 ? pl.q.n + 1 : (few ? OPTB_CAP_SEED : OPTB_CAP_RUN);
    a.allow_split = few ? 1 : 0;
    if ((err = hipMemsetAsync(ctrl, 0, 4 * sizeof(unsigned long long), s)) != hipSuccess)
      OPT_FAIL(V2X_EHIP, "opt_search_bound: counter reset failed: %s", hipGetErrorString(err));
    const unsigned wgs = (unsigned)std::min<int64_t>(bp.wgs, (n_in + OPTB_BLOCK - 1) / OPTB_BLOCK);
    if (bp.tab_lds) hipLaunchKernelGGL(k_opt_bound_search<true>, dim3(wgs), dim3(OPTB_BLOCK), bp.lds_bytes, s, a);
    else hipLaunchKernelGGL(k_opt_bound_search<false>, dim3(wgs), dim3(OPTB_BLOCK), bp.lds_bytes, s, a);
    OPTB_LAUNCHED("search launch");
    hipLaunchKernelGGL(k_opt_bound_fold_a, dim3(egrid), dim3(256), 0, s, p->E, inc, idx, bits);
    OPTB_LAUNCHED("fold launch");
    hipLaunchKernelGGL(k_opt_bound_fold_b, dim3(64), dim3(256), 0, s, ctrl, a.cand, inc, idx);
    OPTB_LAUNCHED("fold launch");
    hipLaunchKernelGGL(k_opt_bound_compact, dim3(256), dim3(256), 0, s, a.n_in, ctrl, a.qout, qa);
    OPTB_LAUNCHED("compact launch");
    unsigned long long back[2];                                  // { items of the next round, nodes visited so far }
    if ((err = hipMemcpyAsync(back, ctrl + OPTB_OUT, sizeof(back), hipMemcpyDeviceToHost, s)) != hipSuccess ||
        (err = hipStreamSynchronize(s)) != hipSuccess)
      OPT_FAIL(V2X_EHIP, "opt_search_bound: round %lld failed: %s", (long long)round, hipGetErrorString(err));
    n_in = (int64_t)back[0];
    nodes = (int64_t)back[1];
  }
#undef OPTB_LAUNCHED
  hipLaunchKernelGGL(k_opt_bound_finish, dim3(egrid), dim3(256), 0, s, p->E, inc, idx, best_index, best_reward);
  if ((err = hipGetLastError()) != hipSuccess)
    OPT_FAIL(V2X_EHIP, "opt_search_bound: finish launch failed: %s", hipGetErrorString(err));
  if (nodes_visited) *nodes_visited = nodes;
  if (n_in > 0)
    OPT_FAIL(V2X_EBUDGET, "opt_search_bound: node budget spent at %d links x %d channels: %lld nodes visited (max_nodes = %lld), "
             "%lld subtrees open; the result is the best leaf found, not proven optimal", pl.q.n, pl.q.C, (long long)nodes,
             (long long)max_nodes, (long long)n_in);
  return V2X_OK;
}

}  // namespace

extern "C" {

int v2x_opt_search_bound(const v2x_opt_problem* p, void* workspace, int64_t max_nodes, int64_t* best_index, double* best_reward,
                         int64_t* nodes_visited, void* stream) {
  return opt_search_bound_impl(p, workspace, max_nodes, nullptr, best_index, best_reward, nodes_visited, stream);
}

int v2x_opt_search_bound_seeded(const v2x_opt_problem* p, void* workspace, int64_t max_nodes, const int32_t* start_actions,
                                int64_t* best_index, double* best_reward, int64_t* nodes_visited, void* stream) {
  if (!start_actions) OPT_FAIL(V2X_EINVAL, "opt_search_bound_seeded: null start_actions");
  return opt_search_bound_impl(p, workspace, max_nodes, start_actions, best_index, best_reward, nodes_visited, stream);
}

}  // extern "C"

// ------------------------------------------------------------------------------------- counting branch and bound
// How many joint actions of a state score above / exactly at a threshold v (v2x_opt_count_bound): the search's tree, queue
// and round loop with a FIXED threshold in the incumbent's place.  A node is pruned when
//   ub * (1 + EPS) + EPS * (w_v2v + w_v2i) < v,  strictly
// -- by the rounding margin above no leaf below it scores >= v as a leaf is scored, so no better and no equal action is
// lost -- and every leaf that is reached is scored with opt_prefix_init / opt_eval and compared with v exactly.  What a
// subtree contributes depends on the subtree and v alone, and the contributions are integers: `better` and `equal` do not
// depend on the schedule.  There is no incumbent, hence no atomicMax, no candidates and no fold kernels; children are
// visited in natural channel order (the order does not change a count).
//
// A work item is an OptItem whose pad_ holds the threshold slot: (state, slot) pairs are searched independently, E * n_thr
// root items.  Per item end a lane adds its two integer counters to the (state, slot) totals with 64-bit integer
// atomicAdd.  When the node budget is spent, k_opt_count_open books every item still in the queue into per-depth counts
// of open subtrees -- the node it would visit next at depth d, and the untried siblings along its path d0 .. d - 1 at
// their depths -- and k_opt_count_open_fold turns the counts into the 128-bit number of unexamined leaves
// sum_k count[k] * C^(n - k), one lane per (state, slot) doing the carries (opt_open_leaves).
//
// The node state is that of the search (I[l][c] and B[r] in the lane's LDS slots, every slot a left fold over ascending
// assigned k); the three helpers below are its slot arithmetic as functions.
namespace {

// slots of the prefix of d links
__device__ __forceinline__ void opt_slots_init(const OptParams& q, const double* __restrict__ tab, uint64_t lo, uint64_t hi, int d,
                                               const OptSlots& S) {
  const int n = q.n, C = q.C, nr = q.nr;
  const double* tx = tab + (int64_t)n * C;
  const double* bs = tab + 2ll * n * C;
  const double* cross = tab + 3ll * n * C;
  for (int i = 0; i < n * C; ++i) S[i] = tx[i];
  for (int k = 0; k < d; ++k) {
    const int c = opt_digit(lo, hi, k);
    for (int l = 0; l < n; ++l)
      if (l != k) S[l * C + c] += cross[(l * n + k) * C + c];
  }
  for (int r = 0; r < C; ++r) {
    double acc = 0.0;
    if (r < nr)
      for (int k = 0; k < d; ++k)
        if (opt_digit(lo, hi, k) == r) acc += bs[k * C + r];
    S[n * C + r] = acc;
  }
}

// link k (the largest assigned one) joins channel c
__device__ __forceinline__ void opt_slots_push(const OptParams& q, const double* __restrict__ tab, int k, int c, const OptSlots& S) {
  const int n = q.n, C = q.C;
  const double* bs = tab + 2ll * n * C;
  const double* cross = tab + 3ll * n * C;
  for (int l = 0; l < n; ++l)
    if (l != k) S[l * C + c] += cross[(l * n + k) * C + c];
  if (c < q.nr) S[n * C + c] += bs[k * C + c];
}

// column c again from scratch over the d assigned links (opt_row_fold's order)
__device__ __forceinline__ void opt_slots_column(const OptParams& q, const double* __restrict__ tab, uint64_t lo, uint64_t hi, int d,
                                                 int c, const OptSlots& S) {
  const int n = q.n, C = q.C;
  const double* tx = tab + (int64_t)n * C;
  const double* bs = tab + 2ll * n * C;
  const double* cross = tab + 3ll * n * C;
  for (int l = 0; l < n; ++l) S[l * C + c] = tx[l * C + c];
  for (int kk = 0; kk < d; ++kk)
    if (opt_digit(lo, hi, kk) == c)
      for (int l = 0; l < n; ++l)
        if (l != kk) S[l * C + c] += cross[(l * n + kk) * C + c];
  if (c < q.nr) {
    double acc = 0.0;
    for (int kk = 0; kk < d; ++kk)
      if (opt_digit(lo, hi, kk) == c) acc += bs[kk * C + c];
    S[n * C + c] = acc;
  }
}

// the bound of the prefix of d links ("Bound of a prefix" above): two log2 per node
__device__ __forceinline__ double opt_node_bound(const OptParams& q, const double* __restrict__ tab, uint64_t lo, uint64_t hi, int d,
                                                 const OptSlots& S) {
#pragma clang fp contract(off)
  const int n = q.n, C = q.C, nr = q.nr;
  const double* sig = tab;
  const double* v2i = tab + 3ll * n * C + (int64_t)n * n * C;
  double pv = 1.0, pi = 1.0;
#pragma unroll 4
  for (int l = 0; l < d; ++l) {
    const int c = opt_digit(lo, hi, l);
    pv *= 1.0 + sig[l * C + c] / (S[l * C + c] + q.sig2);
  }
  for (int l = d; l < n; ++l) {
    double x = 0.0;
#pragma unroll 4
    for (int c = 0; c < C; ++c) x = fmax(x, sig[l * C + c] / (S[l * C + c] + q.sig2));
    pv *= 1.0 + x;
  }
#pragma unroll 4
  for (int r = 0; r < nr; ++r) pi *= 1.0 + v2i[r] / (S[n * C + r] + q.sig2);
  return q.w_v2v * log2(pv) + q.w_v2i * log2(pi);
}

enum { OPTC_BAD = 5 };                // ctrl word beside OPTB_*: a threshold that is not a number was seen
constexpr int OPTC_MAX_THR = 31;

struct OptCountArgs {
  OptParams q;                      // p = n, m = 0: the leaf's opt_prefix_init / opt_eval
  const double* tabs;
  const OptItem* qin;
  OptItem* qout;
  int n_in, cap, allow_split, n_thr;
  unsigned long long* ctrl;         // OPTB_* counters
  const double* thr;                // [E][n_thr]
  unsigned long long* better;       // [E][n_thr] totals
  unsigned long long* equal;
  double* leaf;                     // [n + C][lanes] scratch of opt_prefix_init
};

// LDS as k_opt_bound_search: [the state's table when TAB_LDS (E = 1)] [n * C + C slots x 64 lanes]
template <bool TAB_LDS>
__global__ __launch_bounds__(OPTB_BLOCK) void k_opt_count_bound(OptCountArgs a) {
#pragma clang fp contract(off)
  extern __shared__ double opt_lds[];
  const OptParams q = a.q;
  const int n = q.n, C = q.C;
  const int64_t lanes = (int64_t)gridDim.x * OPTB_BLOCK, lane = (int64_t)blockIdx.x * OPTB_BLOCK + threadIdx.x;
  const int64_t tab_pad = TAB_LDS ? ((q.tab + 1) & ~1ll) : 0;
  if constexpr (TAB_LDS) {
    for (int64_t i = threadIdx.x; i < q.tab; i += OPTB_BLOCK) opt_lds[i] = a.tabs[i];
    __syncthreads();
  }
  OptSlots S;
  S.base = opt_lds + tab_pad + threadIdx.x;
  double* lf = a.leaf + lane;
  unsigned long long visited = 0;
  for (;;) {                                                   // <= n_in items in all lanes together
    const unsigned long long it = atomicAdd(&a.ctrl[OPTB_HEAD], 1ull);
    if (it >= (unsigned long long)a.n_in) break;
    const OptItem item = a.qin[it];
    const int e = item.e, d0 = item.d0;
    const int64_t slot = item.pad_;
    int d = item.d;
    uint64_t lo = item.lo, hi = item.hi;
    const double* tab = TAB_LDS ? opt_lds : a.tabs + (int64_t)e * q.tab;
    const double v = a.thr[(int64_t)e * a.n_thr + slot];
    opt_slots_init(q, tab, lo, hi, d, S);
    unsigned long long nb = 0, ne = 0;                         // leaves of this run of the item above / at the threshold
    int cnt = 0;
    bool visit = true, finished = false;
    // every iteration visits a node (<= cap of them) or steps one level back (<= n in a row)
    for (;;) {
      if (visit) {
        if (cnt >= a.cap) break;                               // suspended: the node at depth d is still to visit
        ++cnt;
        if (d == n) {                                          // leaf: the exhaustive search's own arithmetic
          opt_prefix_init(q, tab, lo, hi, lf, (int)lanes);
          const double r = opt_eval(q, tab, lo, hi, 0, lf, (int)lanes);
          nb += r > v ? 1ull : 0ull;                           // (a reward that is not a number is neither)
          ne += r == v ? 1ull : 0ull;
          visit = false;
          continue;
        }
        const double ub = opt_node_bound(q, tab, lo, hi, d, S);
        if (ub * (1.0 + OPT_BOUND_EPS) + OPT_BOUND_EPS * (q.w_v2v + q.w_v2i) < v) {
          visit = false;
          continue;
        }
        opt_slots_push(q, tab, d, 0, S);
        opt_set_digit(lo, hi, d, 0);
        ++d;
      } else {
        if (d == d0) { finished = true; break; }
        const int k = d - 1, c = opt_digit(lo, hi, k);
        d = k;
        opt_slots_column(q, tab, lo, hi, d, c, S);
        if (c + 1 < C) {
          opt_slots_push(q, tab, k, c + 1, S);
          opt_set_digit(lo, hi, k, c + 1);
          d = k + 1;
          visit = true;
        }
      }
    }
    visited += (unsigned long long)cnt;
    if (nb) atomicAdd(&a.better[(int64_t)e * a.n_thr + slot], nb);
    if (ne) atomicAdd(&a.equal[(int64_t)e * a.n_thr + slot], ne);
    OptItem back;
    back.lo = lo;
    back.hi = hi;
    back.e = finished ? -1 : e;
    back.d0 = (int16_t)d0;
    back.d = (int16_t)d;
    back.pad_ = slot;
    if (!finished && a.allow_split && d > d0) {
      // the untried siblings along the path d0 .. d - 1 (the channels above the one taken) become items of their own, the
      // node at depth d its own root
      int need = 0;
      for (int j = d0; j < d; ++j) need += C - 1 - opt_digit(lo, hi, j);
      const unsigned long long at = a.n_in + atomicAdd(&a.ctrl[OPTB_TAIL], (unsigned long long)need);
      if (at + need <= (unsigned long long)OPTB_QCAP) {
        unsigned long long w = at;
        for (int j = d0; j < d; ++j)
          for (int c = opt_digit(lo, hi, j) + 1; c < C; ++c) {
            OptItem sib;
            sib.lo = j < 16 ? (lo & ((1ull << (4 * j)) - 1)) : lo;
            sib.hi = j < 16 ? 0ull : (hi & ((1ull << (4 * (j - 16))) - 1));
            opt_set_digit(sib.lo, sib.hi, j, c);
            sib.e = e;
            sib.d0 = sib.d = (int16_t)(j + 1);
            sib.pad_ = slot;
            a.qout[w++] = sib;
          }
        back.d0 = (int16_t)d;
      } else {                                                 // no room: holes where the reservation lies inside the queue
        OptItem hole;
        hole.lo = hole.hi = 0;
        hole.e = -1;
        hole.d0 = hole.d = 0;
        hole.pad_ = 0;
        for (unsigned long long w = at; w < at + need && w < (unsigned long long)OPTB_QCAP; ++w) a.qout[w] = hole;
      }
    }
    a.qout[it] = back;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) visited += __shfl_xor(visited, off, 64);
  if (threadIdx.x == 0 && visited) atomicAdd(&a.ctrl[OPTB_NODES], visited);
}

// grid ceil(E * n_thr / 256): one root item per (state, slot), totals at zero; a threshold that is not a number is flagged
__global__ __launch_bounds__(256) void k_opt_count_init(int E, int n_thr, const double* __restrict__ thr, OptItem* q0,
                                                        unsigned long long* better, unsigned long long* equal,
                                                        unsigned long long* ctrl) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= E * n_thr) return;
  OptItem it;
  it.lo = it.hi = 0;
  it.e = i / n_thr;
  it.d0 = it.d = 0;
  it.pad_ = i % n_thr;
  q0[i] = it;
  better[i] = 0;
  equal[i] = 0;
  const double v = thr[i];
  if (v != v) ctrl[OPTC_BAD] = 1;
}

// grid-stride over the items the budget left open: open subtrees per (state, slot) and depth, depth[(e * n_thr + slot)][n + 1]
__global__ __launch_bounds__(256) void k_opt_count_open(int n_in, int n, int C, int n_thr, const OptItem* __restrict__ items,
                                                        unsigned long long* depth) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n_in; i += gridDim.x * 256) {
    const OptItem it = items[i];
    if (it.e < 0) continue;
    unsigned long long* row = depth + ((int64_t)it.e * n_thr + it.pad_) * (n + 1);
    atomicAdd(&row[it.d], 1ull);                               // the node to visit next
    for (int j = it.d0; j < it.d; ++j) {                       // the untried siblings of link j: subtrees rooted at depth j + 1
      const int left = C - 1 - opt_digit(it.lo, it.hi, j);
      if (left > 0) atomicAdd(&row[j + 1], (unsigned long long)left);
    }
  }
}

__host__ __device__ inline unsigned long long opt_mulhi64(unsigned long long x, unsigned long long y) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(x, y);
#else
  return (unsigned long long)(((unsigned __int128)x * y) >> 64);
#endif
}

// sum_k count[k] * C^(n - k) as a 128-bit integer (modulo 2^128; C^n < 2^102 at every size the search accepts)
__host__ __device__ inline void opt_open_leaves(const unsigned long long* count, int n, int C, unsigned long long& hi,
                                                unsigned long long& lo) {
  hi = 0;
  lo = 0;
  unsigned long long ph = 0, pl = 1;                           // C^(n - k)
  for (int k = n; k >= 0; --k) {
    const unsigned long long c = count[k];
    if (c) {
      const unsigned long long add_lo = c * pl, add_hi = opt_mulhi64(c, pl) + c * ph;
      const unsigned long long s = lo + add_lo;
      hi += add_hi + (s < lo ? 1ull : 0ull);
      lo = s;
    }
    ph = ph * (unsigned long long)C + opt_mulhi64(pl, (unsigned long long)C);
    pl = pl * (unsigned long long)C;
  }
}

// grid ceil(E * n_thr / 256): a lane per (state, slot) does the carries
__global__ __launch_bounds__(256) void k_opt_count_open_fold(int rows, int n, int C, const unsigned long long* __restrict__ depth,
                                                             unsigned long long* open_hi, unsigned long long* open_lo) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= rows) return;
  unsigned long long hi, lo;
  opt_open_leaves(depth + (int64_t)i * (n + 1), n, C, hi, lo);
  open_hi[i] = hi;
  open_lo[i] = lo;
}

// workspace = that of v2x_opt_search_bound | per-depth open counts [E * n_thr][n + 1]
int opt_count_plan(const v2x_opt_problem* p, int32_t n_thr, int64_t max_nodes, const char* who, OptPlan& pl, OptBoundPlan& bp,
                   int64_t& off_depth, int64_t& bytes) {
  int rc = opt_bound_plan(p, max_nodes, who, pl, bp, false);
  if (rc != V2X_OK) return rc;
  if (n_thr < 1 || n_thr > OPTC_MAX_THR) OPT_FAIL(V2X_EINVAL, "%s: n_thr = %d thresholds per state (1..%d)", who, n_thr, OPTC_MAX_THR);
  if ((int64_t)p->E * n_thr > OPTB_QCAP)
    OPT_FAIL(V2X_EINVAL, "%s: E * n_thr = %d * %d root items exceed the queue of %d", who, p->E, n_thr, OPTB_QCAP);
  off_depth = bp.bytes;
  bytes = bp.bytes + (((int64_t)p->E * n_thr * (pl.q.n + 1) * 8 + 255) & ~255ll);
  return V2X_OK;
}

}  // namespace

extern "C" {

int64_t v2x_opt_count_bound_workspace_bytes(const v2x_opt_problem* p, int32_t n_thr, int64_t max_nodes) {
  OptPlan pl;
  OptBoundPlan bp;
  int64_t off_depth, bytes;
  if (opt_count_plan(p, n_thr, max_nodes, "opt_count_bound_workspace_bytes", pl, bp, off_depth, bytes) != V2X_OK) return V2X_EINVAL;
  return bytes;
}

int v2x_opt_count_open_leaves(const uint64_t* depth_counts, int32_t n, int32_t rb, uint64_t* open_hi, uint64_t* open_lo) {
  if (!depth_counts || !open_hi || !open_lo) OPT_FAIL(V2X_EINVAL, "opt_count_open_leaves: null argument");
  if (n < 1 || n > OPT_MAX_N || rb < OPT_MIN_C || rb > OPT_MAX_C)
    OPT_FAIL(V2X_EINVAL, "opt_count_open_leaves: %d links x %d channels (1..%d, %d..%d)", n, rb, OPT_MAX_N, OPT_MIN_C, OPT_MAX_C);
  unsigned long long cnt[OPT_MAX_N + 1], hi, lo;
  for (int k = 0; k <= n; ++k) cnt[k] = depth_counts[k];
  opt_open_leaves(cnt, n, rb, hi, lo);
  *open_hi = hi;
  *open_lo = lo;
  return V2X_OK;
}

int v2x_opt_count_bound(const v2x_opt_problem* p, void* workspace, const double* thresholds, int32_t n_thr, int64_t max_nodes,
                        int64_t* better, int64_t* equal, uint64_t* open_hi, uint64_t* open_lo, int64_t* nodes_visited,
                        void* stream) {
  OptPlan pl;
  OptBoundPlan bp;
  int64_t off_depth, bytes;
  int rc = opt_count_plan(p, n_thr, max_nodes, "opt_count_bound", pl, bp, off_depth, bytes);
  if (rc != V2X_OK) return rc;
  if (!thresholds) OPT_FAIL(V2X_EINVAL, "opt_count_bound: null thresholds");
  if (!better || !equal || !open_hi || !open_lo) OPT_FAIL(V2X_EINVAL, "opt_count_bound: null output");
  hipStream_t s = (hipStream_t)stream;
  rc = opt_prep(p, pl, workspace, s, "opt_count_bound");
  if (rc != V2X_OK) return rc;
  char* ws = (char*)workspace;
  unsigned long long* ctrl = (unsigned long long*)(ws + bp.off_ctrl);
  unsigned long long* depth = (unsigned long long*)(ws + off_depth);
  OptItem* qa = (OptItem*)(ws + bp.off_qa);
  OptItem* qb = (OptItem*)(ws + bp.off_qb);
  const int rows = p->E * n_thr;
  const unsigned rgrid = (unsigned)((rows + 255) / 256);
  hipError_t err;
#define OPTC_LAUNCHED(what)                                                                                        \
  if ((err = hipGetLastError()) != hipSuccess)                                                                     \
  OPT_FAIL(V2X_EHIP, "opt_count_bound: %s failed: %s", what, hipGetErrorString(err))
  if ((err = hipMemsetAsync(ctrl, 0, OPTB_CTRL * sizeof(unsigned long long), s)) != hipSuccess ||
      (err = hipMemsetAsync(depth, 0, (size_t)rows * (pl.q.n + 1) * sizeof(unsigned long long), s)) != hipSuccess)
    OPT_FAIL(V2X_EHIP, "opt_count_bound: counter reset failed: %s", hipGetErrorString(err));
  hipLaunchKernelGGL(k_opt_count_init, dim3(rgrid), dim3(256), 0, s, p->E, (int)n_thr, thresholds, qa, (unsigned long long*)better,
                     (unsigned long long*)equal, ctrl);
  OPTC_LAUNCHED("init launch");
  unsigned long long bad = 0;
  if ((err = hipMemcpyAsync(&bad, ctrl + OPTC_BAD, sizeof(bad), hipMemcpyDeviceToHost, s)) != hipSuccess ||
      (err = hipStreamSynchronize(s)) != hipSuccess)
    OPT_FAIL(V2X_EHIP, "opt_count_bound: threshold check failed: %s", hipGetErrorString(err));
  if (bad) OPT_FAIL(V2X_EINVAL, "opt_count_bound: a threshold is not a number (NaN)");
  OptCountArgs a;
  a.q = pl.q;
  a.tabs = (const double*)workspace;
  a.qin = qa;
  a.qout = qb;
  a.n_thr = (int)n_thr;
  a.ctrl = ctrl;
  a.thr = thresholds;
  a.better = (unsigned long long*)better;
  a.equal = (unsigned long long*)equal;
  a.leaf = (double*)(ws + bp.off_leaf);
  if (bp.lds_bytes > 64 * 1024) {          // above the default dynamic-LDS size a kernel has to be told; the launch check decides
    if (bp.tab_lds) (void)hipFuncSetAttribute((const void*)k_opt_count_bound<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bp.lds_bytes);
    else (void)hipFuncSetAttribute((const void*)k_opt_count_bound<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bp.lds_bytes);
    (void)hipGetLastError();
  }
  const int64_t short_of = (int64_t)bp.wgs * OPTB_BLOCK * OPTB_ITEMS_PER_LANE;
  int64_t n_in = rows, nodes = 0;
  // one round per pass; every round visits at least one node per item, so the node budget also bounds the rounds
  for (int64_t round = 0; n_in > 0 && nodes < max_nodes; ++round) {
    const bool few = n_in < short_of;
    a.n_in = (int)n_in;
    a.cap = round == 0 ? pl.q.n + 1 : (few ? OPTB_CAP_SEED : OPTB_CAP_RUN);
    a.allow_split = few ? 1 : 0;
    if ((err = hipMemsetAsync(ctrl, 0, 4 * sizeof(unsigned long long), s)) != hipSuccess)
      OPT_FAIL(V2X_EHIP, "opt_count_bound: counter reset failed: %s", hipGetErrorString(err));
    const unsigned wgs = (unsigned)std::min<int64_t>(bp.wgs, (n_in + OPTB_BLOCK - 1) / OPTB_BLOCK);
    if (bp.tab_lds) hipLaunchKernelGGL(k_opt_count_bound<true>, dim3(wgs), dim3(OPTB_BLOCK), bp.lds_bytes, s, a);
    else hipLaunchKernelGGL(k_opt_count_bound<false>, dim3(wgs), dim3(OPTB_BLOCK), bp.lds_bytes, s, a);
    OPTC_LAUNCHED("count launch");
    hipLaunchKernelGGL(k_opt_bound_compact, dim3(256), dim3(256), 0, s, a.n_in, ctrl, a.qout, qa);
    OPTC_LAUNCHED("compact launch");
    unsigned long long back[2];                                  // { items of the next round, nodes visited so far }
    if ((err = hipMemcpyAsync(back, ctrl + OPTB_OUT, sizeof(back), hipMemcpyDeviceToHost, s)) != hipSuccess ||
        (err = hipStreamSynchronize(s)) != hipSuccess)
      OPT_FAIL(V2X_EHIP, "opt_count_bound: round %lld failed: %s", (long long)round, hipGetErrorString(err));
    n_in = (int64_t)back[0];
    nodes = (int64_t)back[1];
  }
  if (n_in > 0) {
    hipLaunchKernelGGL(k_opt_count_open, dim3((unsigned)std::min<int64_t>(256, (n_in + 255) / 256)), dim3(256), 0, s, (int)n_in,
                       pl.q.n, pl.q.C, (int)n_thr, qa, depth);
    OPTC_LAUNCHED("open launch");
  }
  hipLaunchKernelGGL(k_opt_count_open_fold, dim3(rgrid), dim3(256), 0, s, rows, pl.q.n, pl.q.C, depth,
                     (unsigned long long*)open_hi, (unsigned long long*)open_lo);
  OPTC_LAUNCHED("open fold launch");
#undef OPTC_LAUNCHED
  if (nodes_visited) *nodes_visited = nodes;
  if (n_in > 0)
    OPT_FAIL(V2X_EBUDGET, "opt_count_bound: node budget spent at %d links x %d channels: %lld nodes visited (max_nodes = %lld), "
             "%lld subtrees open; better / equal are lower bounds, open the leaves not examined", pl.q.n, pl.q.C, (long long)nodes,
             (long long)max_nodes, (long long)n_in);
  return V2X_OK;
}

}  // extern "C"

// -------------------------------------------------------------------------------------------------- local search
// A near-optimal allocation where the exact searches cannot go (v2x_opt_search_local: 1..128 links): a multi-start
// best-response local search, one wave per (state, restart), a lane per link (two above 64 links).  A joint action is an
// array of channel numbers here, never an index.
//
//   start    restart 0: a[l] = l mod C; restart r: a[l] = splitmix64((seed << 32) ^ (r << 8) ^ l) mod C
//   sweep    for l = 0 .. n - 1: the total reward of each of the C channels of link l with the other links fixed; move to the
//            best one (lowest channel among equals) if it is strictly larger than the current total.  Sweeps repeat until
//            one makes no move, max_sweeps at most.
//   result   of a restart: its action, scored from scratch by optl_score -- the additions of opt_prefix_init / opt_eval with
//            every link a prefix link, in their order, so the reward equals v2x_opt_rewards of the action's index bit for
//            bit; of a state: the best restart by (larger reward, else lexicographically lower action): opt_better's rule.
//
// Wave state in LDS: I[c][l] = tx[l][c] + sum over the OTHER links k on c of cross[l][k][c] for every channel c (what link l
// would suffer on c), B[r] = sum over the links on r of bs[k][r].  A visit of link k (k on channel o):
//   1. column o is folded again over the links that remain -- never `big + small - big`: linear-domain terms span ten orders
//      of magnitude.  The wave's ballot of "on channel o" gives the links to add; each is one coalesced load of the
//      receiver-minor copy crossT[k][c][l] of the cross table (k_opt_local_transpose).
//   2. every other link l holds two rates: without k, and with k on l's channel.  The total of candidate c is one wave sum of
//      (l on c ? with : without), lane c adding link k's own rate on c and the V2I rates: C wave sums, 2 log2 per lane.
//      A butterfly sum leaves the same bits in every lane, so the decision is wave-uniform.
//   3. k is appended to the column of its new channel.
constexpr int OPTL_MAX_N = 128, OPTL_MAX_RESTARTS = 65536;
constexpr int OPTL_BLOCK = 64;                    // one wave
constexpr int OPTL_BATCH = 8;                     // interferer columns in flight while a column is folded again
constexpr int64_t OPTL_REWARDS_WGS = 1 << 20;     // workgroups of a v2x_opt_rewards_actions launch (grid-stride beyond)

namespace {

struct OptLocalArgs {
  OptParams q;                 // p = n, m = 0
  const double* tabs;          // [E][tab]
  const double* crossT;        // [E][n][C][n]: cross[l][k][c] at [k][c][l]
  int restarts, max_sweeps;
  unsigned long long seed;
  uint8_t* act;                // [E][R][n]   final action of every restart
  double* rew;                 // [E][R]
  uint8_t* conv;               // [E][R]      the last sweep made no move
  int32_t* all_actions;        // [E][R][n], may be null
  double* all_rewards;         // [E][R], may be null
};

__host__ __device__ inline unsigned long long optl_splitmix64(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

__device__ __forceinline__ double optl_wave_sum(double x) {
#pragma clang fp contract(off)
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
  return x;
}

// doubles of dynamic LDS of a wave: I[C][n] | B[C] | rates[n + C] | action bytes
inline size_t optl_search_lds(int n, int C) { return (size_t)((int64_t)C * n + C + n + C) * sizeof(double) + (size_t)((n + 7) & ~7); }
inline size_t optl_score_lds(int n, int C) { return (size_t)(n + C) * sizeof(double) + (size_t)((n + 7) & ~7); }

// grid (ceil(n * n * C / 256), E): crossT[k][c][l] = cross[l][k][c]
__global__ __launch_bounds__(256) void k_opt_local_transpose(int n, int C, int64_t tab, const double* __restrict__ tabs,
                                                             double* __restrict__ crossT) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, total = (int64_t)n * n * C;
  if (i >= total) return;
  const int e = blockIdx.y;
  const int l = (int)(i % n), c = (int)((i / n) % C), k = (int)(i / ((int64_t)n * C));
  crossT[(int64_t)e * total + i] = tabs[(int64_t)e * tab + 3ll * n * C + ((int64_t)l * n + k) * C + c];
}

// The wave's reward of the joint action ab[0..n) (LDS bytes, every one in [0, C)), valid in lane 0: per link the left fold
// of opt_prefix_init (ascending k, only the links on the same channel), per rate the expression of opt_eval, then the two
// sums in link / RB order by one lane.  red: n + C doubles of LDS.
template <int LPL>
__device__ __forceinline__ double optl_score(const OptParams& q, const double* __restrict__ tab, const double* __restrict__ crossT,
                                             const uint8_t* ab, double* red, int lane) {
#pragma clang fp contract(off)
  const int n = q.n, C = q.C;
  const double* sig = tab;
  const double* tx = tab + (int64_t)n * C;
  const double* bs = tab + 2ll * n * C;
  const double* v2i = tab + 3ll * n * C + (int64_t)n * n * C;
#pragma unroll
  for (int h = 0; h < LPL; ++h) {
    const int l = lane + 64 * h;
    if (l < n) {
      const int c = ab[l];
      double acc = tx[l * C + c];
      for (int k = 0; k < n; ++k)
        if (k != l && ab[k] == c) acc += crossT[((int64_t)k * C + c) * n + l];
      red[l] = log2(1.0 + sig[l * C + c] / (acc + q.sig2));
    }
  }
  if (lane < q.nr) {
    double b = 0.0;
    for (int k = 0; k < n; ++k)
      if (ab[k] == lane) b += bs[k * C + lane];
    red[n + lane] = log2(1.0 + v2i[lane] / (b + q.sig2));
  }
  __syncthreads();
  double out = 0.0;
  if (lane == 0) {
    double v2v_sum = 0.0, v2i_sum = 0.0;
    for (int l = 0; l < n; ++l) v2v_sum += red[l];
    for (int r = 0; r < q.nr; ++r) v2i_sum += red[n + r];
    out = q.w_v2v * v2v_sum + q.w_v2i * v2i_sum;
  }
  __syncthreads();
  return out;
}

// grid (restarts, E): the restarts of a state are neighbours in dispatch order and share its tables in L2.
template <int LPL>
__global__ __launch_bounds__(OPTL_BLOCK) void k_opt_local_search(OptLocalArgs a) {
#pragma clang fp contract(off)
  extern __shared__ double opt_lds[];
  const OptParams q = a.q;
  const int n = q.n, C = q.C, nr = q.nr;
  const int lane = threadIdx.x, r = blockIdx.x, e = blockIdx.y;
  const double* tab = a.tabs + (int64_t)e * q.tab;
  const double* crossT = a.crossT + (int64_t)e * n * n * C;
  const double* sig = tab;
  const double* tx = tab + (int64_t)n * C;
  const double* bs = tab + 2ll * n * C;
  const double* v2i = tab + 3ll * n * C + (int64_t)n * n * C;
  double* I = opt_lds;                       // [C][n]
  double* B = I + C * n;                     // [C]
  double* red = B + C;                       // [n + C]
  uint8_t* ab = (uint8_t*)(red + n + C);     // [n]
  int act[LPL];
#pragma unroll
  for (int h = 0; h < LPL; ++h) {
    const int l = lane + 64 * h;
    act[h] = -1;
    if (l < n) {
      act[h] = r == 0 ? l % C
                      : (int)(optl_splitmix64((a.seed << 32) ^ ((unsigned long long)r << 8) ^ (unsigned long long)l) % (unsigned)C);
      ab[l] = (uint8_t)act[h];
    }
  }
  __syncthreads();
#pragma unroll
  for (int h = 0; h < LPL; ++h) {
    const int l = lane + 64 * h;
    if (l < n) {
      for (int c = 0; c < C; ++c) I[c * n + l] = tx[l * C + c];
      for (int j = 0; j < n; ++j) {
        const int cj = ab[j];
        if (j != l) I[cj * n + l] += crossT[((int64_t)j * C + cj) * n + l];
      }
    }
  }
  if (lane < C) {
    double b = 0.0;
    if (lane < nr)
      for (int j = 0; j < n; ++j)
        if (ab[j] == lane) b += bs[j * C + lane];
    B[lane] = b;
  }
  __syncthreads();
  int converged = 0;
  for (int sweep = 0; sweep < a.max_sweeps; ++sweep) {
    bool moved = false;
    for (int k = 0; k < n; ++k) {
      const int o = ab[k];
      // 1. column o without link k, folded over the links that remain (ascending)
      double acc[LPL];
#pragma unroll
      for (int h = 0; h < LPL; ++h) {
        const int l = lane + 64 * h;
        acc[h] = l < n ? tx[l * C + o] : 0.0;
      }
      double bo = 0.0;
#pragma unroll
      for (int g = 0; g < LPL; ++g) {
        unsigned long long on = __ballot(act[g] == o);
        if ((k >> 6) == g) on &= ~(1ull << (k & 63));
        while (on) {                                           // <= 64 links, OPTL_BATCH per turn
          // the loads of a batch are independent and go out together; the additions keep their ascending order
          int jj[OPTL_BATCH];
          double v[OPTL_BATCH][LPL], vb[OPTL_BATCH];
#pragma unroll
          for (int u = 0; u < OPTL_BATCH; ++u) {
            jj[u] = on ? 64 * g + (int)__builtin_ctzll(on) : -1;
            on &= on - 1;                                      // (0 stays 0)
          }
#pragma unroll
          for (int u = 0; u < OPTL_BATCH; ++u) {
            const double* col = crossT + ((int64_t)(jj[u] < 0 ? 0 : jj[u]) * C + o) * n;
#pragma unroll
            for (int h = 0; h < LPL; ++h) {
              const int l = lane + 64 * h;
              v[u][h] = (jj[u] >= 0 && l < n) ? col[l] : 0.0;
            }
            vb[u] = (jj[u] >= 0 && o < nr) ? bs[jj[u] * C + o] : 0.0;
          }
#pragma unroll
          for (int u = 0; u < OPTL_BATCH; ++u) {
            if (jj[u] >= 0) {
#pragma unroll
              for (int h = 0; h < LPL; ++h)
                if (lane + 64 * h != jj[u]) acc[h] += v[u][h];
              if (o < nr) bo += vb[u];
            }
          }
        }
      }
#pragma unroll
      for (int h = 0; h < LPL; ++h) {
        const int l = lane + 64 * h;
        if (l < n) I[o * n + l] = acc[h];
      }
      if (lane == 0) B[o] = bo;
      __syncthreads();
      // 2. both rates of every other link; lane c: link k's own rate on c and the V2I rate of RB c without / with k
      double r0[LPL], r1[LPL];
#pragma unroll
      for (int h = 0; h < LPL; ++h) {
        const int l = lane + 64 * h;
        r0[h] = r1[h] = 0.0;
        if (l < n && l != k) {
          const int c = act[h];
          const double x = I[c * n + l], s = sig[l * C + c];
          r0[h] = log2(1.0 + s / (x + q.sig2));
          r1[h] = log2(1.0 + s / ((x + crossT[((int64_t)k * C + c) * n + l]) + q.sig2));
        }
      }
      double own = 0.0, v0 = 0.0, v1 = 0.0;
      if (lane < C) {
        own = log2(1.0 + sig[k * C + lane] / (I[lane * n + k] + q.sig2));
        if (lane < nr) {
          v0 = log2(1.0 + v2i[lane] / (B[lane] + q.sig2));
          v1 = log2(1.0 + v2i[lane] / ((B[lane] + bs[k * C + lane]) + q.sig2));
        }
      }
      int best = 0;
      double best_t = 0.0, cur_t = 0.0;
      for (int c = 0; c < C; ++c) {
        double t = 0.0;
#pragma unroll
        for (int h = 0; h < LPL; ++h) t += (lane + 64 * h != k && act[h] == c) ? r1[h] : r0[h];
        t *= q.w_v2v;
        if (lane < C) t += lane == c ? q.w_v2v * own + q.w_v2i * v1 : q.w_v2i * v0;
        t = optl_wave_sum(t);
        if (c == o) cur_t = t;
        if (c == 0 || t > best_t) { best = c; best_t = t; }
      }
      const int to = best_t > cur_t ? best : o;
      // 3. link k joins the column of its channel
      const double* colk = crossT + ((int64_t)k * C + to) * n;
#pragma unroll
      for (int h = 0; h < LPL; ++h) {
        const int l = lane + 64 * h;
        if (l < n && l != k) I[to * n + l] += colk[l];
        if (l == k) { act[h] = to; ab[k] = (uint8_t)to; }
      }
      if (lane == 0 && to < nr) B[to] += bs[k * C + to];
      moved |= to != o;
      __syncthreads();
    }
    if (!moved) { converged = 1; break; }
  }
  const double reward = optl_score<LPL>(q, tab, crossT, ab, red, lane);
  const int64_t at = (int64_t)e * a.restarts + r;
#pragma unroll
  for (int h = 0; h < LPL; ++h) {
    const int l = lane + 64 * h;
    if (l < n) {
      a.act[at * n + l] = (uint8_t)act[h];
      if (a.all_actions) a.all_actions[at * n + l] = act[h];
    }
  }
  if (lane == 0) {
    a.rew[at] = reward;
    a.conv[at] = (uint8_t)converged;
    if (a.all_rewards) a.all_rewards[at] = reward;
  }
}

// restart i beats restart b of the same state: larger reward (a reward that is not a number counts as -inf), else the
// lexicographically lower action, else the lower restart (the same action: only the reported restart depends on it)
__device__ __forceinline__ bool optl_better(const double* rew, const uint8_t* act, int n, int i, int b) {
  if (b < 0) return true;
  const double ri = rew[i] == rew[i] ? rew[i] : -INFINITY, rb = rew[b] == rew[b] ? rew[b] : -INFINITY;
  if (ri != rb) return ri > rb;
  const uint8_t* ai = act + (int64_t)i * n;
  const uint8_t* ab = act + (int64_t)b * n;
  for (int l = 0; l < n; ++l)
    if (ai[l] != ab[l]) return ai[l] < ab[l];
  return i < b;
}

// grid E: the best restart of a state; the rule has a unique answer, so the order of the comparisons does not matter
__global__ __launch_bounds__(256) void k_opt_local_best(int n, int restarts, const double* __restrict__ rew,
                                                        const uint8_t* __restrict__ act, const uint8_t* __restrict__ conv,
                                                        int32_t* best_actions, double* best_reward, int32_t* best_info) {
  __shared__ int cand[256];
  const int e = blockIdx.x;
  rew += (int64_t)e * restarts;
  act += (int64_t)e * restarts * n;
  int b = -1;
  for (int i = threadIdx.x; i < restarts; i += 256)
    if (optl_better(rew, act, n, i, b)) b = i;
  cand[threadIdx.x] = b;
  __syncthreads();
  for (int half = 128; half > 0; half >>= 1) {
    if ((int)threadIdx.x < half) {
      const int i = cand[threadIdx.x + half];
      if (i >= 0 && optl_better(rew, act, n, i, cand[threadIdx.x])) cand[threadIdx.x] = i;
    }
    __syncthreads();
  }
  b = cand[0];                                                 // >= 0: restarts >= 1
  for (int l = threadIdx.x; l < n; l += 256) best_actions[(int64_t)e * n + l] = act[(int64_t)b * n + l];
  if (threadIdx.x == 0) {
    best_reward[e] = rew[b];
    if (best_info) {
      best_info[2 * e] = b;
      best_info[2 * e + 1] = conv[(int64_t)e * restarts + b];
    }
  }
}

// grid (chunks, E), one wave per joint action: out[e][j] = reward of actions[e][j][0..n); a channel outside [0, C): NaN
template <int LPL>
__global__ __launch_bounds__(OPTL_BLOCK) void k_opt_rewards_actions(OptParams q, const double* __restrict__ tabs,
                                                                    const double* __restrict__ crossT_all,
                                                                    const int32_t* __restrict__ actions, int64_t K, double* out) {
  extern __shared__ double opt_lds[];
  const int n = q.n, C = q.C, lane = threadIdx.x, e = blockIdx.y;
  const double* tab = tabs + (int64_t)e * q.tab;
  const double* crossT = crossT_all + (int64_t)e * n * n * C;
  double* red = opt_lds;                     // [n + C]
  uint8_t* ab = (uint8_t*)(red + n + C);     // [n]
  for (int64_t j = blockIdx.x; j < K; j += gridDim.x) {
    const int32_t* src = actions + ((int64_t)e * K + j) * n;
    bool bad = false;
#pragma unroll
    for (int h = 0; h < LPL; ++h) {
      const int l = lane + 64 * h;
      if (l < n) {
        const int c = src[l];
        if (c < 0 || c >= C) bad = true;
        else ab[l] = (uint8_t)c;
      }
    }
    const bool any_bad = __ballot(bad) != 0ull;
    __syncthreads();
    double r = __builtin_nan("");
    if (!any_bad) r = optl_score<LPL>(q, tab, crossT, ab, red, lane);
    if (lane == 0) out[(int64_t)e * K + j] = r;
    __syncthreads();
  }
}

struct OptLocalPlan {
  OptParams q;
  int64_t off_crossT, off_rew, off_act, off_conv, bytes;
};

int opt_local_plan(const v2x_opt_problem* p, int restarts, const char* who, OptLocalPlan& lp) {
  if (!p) OPT_FAIL(V2X_EINVAL, "%s: null problem", who);
  if (p->E < 1 || p->E > 65535) OPT_FAIL(V2X_EINVAL, "%s: E = %d states (1..65535)", who, p->E);
  if (p->n < 1 || p->n > OPTL_MAX_N) OPT_FAIL(V2X_EINVAL, "%s: n = %d links (1..%d)", who, p->n, OPTL_MAX_N);
  if (p->rb < OPT_MIN_C || p->rb > OPT_MAX_C) OPT_FAIL(V2X_EINVAL, "%s: rb = %d channels (%d..%d)", who, p->rb, OPT_MIN_C, OPT_MAX_C);
  if (restarts < 1 || restarts > OPTL_MAX_RESTARTS)
    OPT_FAIL(V2X_EINVAL, "%s: restarts = %d (1..%d)", who, restarts, OPTL_MAX_RESTARTS);
  OptParams& q = lp.q;
  q.n = q.p = p->n;
  q.m = 0;
  q.C = p->rb;
  q.nr = std::min(p->rb, p->n);
  q.tab = opt_tab_doubles(q.n, q.C);
  q.sig2 = p->sig2;
  q.w_v2v = p->w_v2v;
  q.w_v2i = p->w_v2i;
  auto al = [](int64_t v) { return (v + 255) & ~255ll; };
  const int64_t ER = (int64_t)p->E * restarts;
  int64_t o = al((int64_t)p->E * q.tab * 8);
  lp.off_crossT = o;  o += al((int64_t)p->E * q.n * q.n * q.C * 8);
  lp.off_rew = o;     o += al(ER * 8);
  lp.off_act = o;     o += al(ER * q.n);
  lp.off_conv = o;    o += al(ER);
  lp.bytes = o;
  return V2X_OK;
}

// tables and their receiver-minor cross copy: two launches
int opt_local_prep(const v2x_opt_problem* p, const OptLocalPlan& lp, void* workspace, hipStream_t s, const char* who) {
  OptPlan pl;
  pl.q = lp.q;
  int rc = opt_prep(p, pl, workspace, s, who);
  if (rc != V2X_OK) return rc;
  const int64_t total = (int64_t)lp.q.n * lp.q.n * lp.q.C;
  hipLaunchKernelGGL(k_opt_local_transpose, dim3((unsigned)((total + 255) / 256), (unsigned)p->E), dim3(256), 0, s, lp.q.n, lp.q.C,
                     lp.q.tab, (const double*)workspace, (double*)((char*)workspace + lp.off_crossT));
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) OPT_FAIL(V2X_EHIP, "%s: transpose launch failed: %s", who, hipGetErrorString(err));
  return V2X_OK;
}

}  // namespace

extern "C" {

int64_t v2x_opt_local_workspace_bytes(const v2x_opt_problem* p, int32_t restarts) {
  OptLocalPlan lp;
  if (opt_local_plan(p, restarts, "opt_local_workspace_bytes", lp) != V2X_OK) return V2X_EINVAL;
  return lp.bytes;
}

int v2x_opt_search_local(const v2x_opt_problem* p, void* workspace, int32_t restarts, uint64_t seed, int32_t max_sweeps,
                         int32_t* best_actions, double* best_reward, int32_t* best_info, int32_t* all_actions,
                         double* all_rewards, void* stream) {
  OptLocalPlan lp;
  int rc = opt_local_plan(p, restarts, "opt_search_local", lp);
  if (rc != V2X_OK) return rc;
  if (max_sweeps < 1) OPT_FAIL(V2X_EINVAL, "opt_search_local: max_sweeps = %d (>= 1)", max_sweeps);
  if (!best_actions || !best_reward) OPT_FAIL(V2X_EINVAL, "opt_search_local: null output");
  hipStream_t s = (hipStream_t)stream;
  rc = opt_local_prep(p, lp, workspace, s, "opt_search_local");
  if (rc != V2X_OK) return rc;
  char* ws = (char*)workspace;
  OptLocalArgs a;
  a.q = lp.q;
  a.tabs = (const double*)workspace;
  a.crossT = (const double*)(ws + lp.off_crossT);
  a.restarts = restarts;
  a.max_sweeps = max_sweeps;
  a.seed = seed;
  a.act = (uint8_t*)(ws + lp.off_act);
  a.rew = (double*)(ws + lp.off_rew);
  a.conv = (uint8_t*)(ws + lp.off_conv);
  a.all_actions = all_actions;
  a.all_rewards = all_rewards;
  const size_t lds = optl_search_lds(lp.q.n, lp.q.C);          // <= 17.5 KiB (128 x 16)
  const dim3 grid((unsigned)restarts, (unsigned)p->E);
  if (lp.q.n <= 64) hipLaunchKernelGGL(k_opt_local_search<1>, grid, dim3(OPTL_BLOCK), lds, s, a);
  else hipLaunchKernelGGL(k_opt_local_search<2>, grid, dim3(OPTL_BLOCK), lds, s, a);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) OPT_FAIL(V2X_EHIP, "opt_search_local: search launch failed: %s", hipGetErrorString(err));
  hipLaunchKernelGGL(k_opt_local_best, dim3((unsigned)p->E), dim3(256), 0, s, lp.q.n, restarts, a.rew, a.act, a.conv, best_actions,
                     best_reward, best_info);
  err = hipGetLastError();
  if (err != hipSuccess) OPT_FAIL(V2X_EHIP, "opt_search_local: reduce launch failed: %s", hipGetErrorString(err));
  return V2X_OK;
}

int v2x_opt_rewards_actions(const v2x_opt_problem* p, void* workspace, const int32_t* actions, int64_t K, double* out, void* stream) {
  OptLocalPlan lp;
  int rc = opt_local_plan(p, 1, "opt_rewards_actions", lp);
  if (rc != V2X_OK) return rc;
  if (K < 1 || K > INT64_MAX / 8 / p->E / lp.q.n) OPT_FAIL(V2X_EINVAL, "opt_rewards_actions: K = %lld joint actions per state", (long long)K);
  if (!actions || !out) OPT_FAIL(V2X_EINVAL, "opt_rewards_actions: null actions or output");
  hipStream_t s = (hipStream_t)stream;
  rc = opt_local_prep(p, lp, workspace, s, "opt_rewards_actions");
  if (rc != V2X_OK) return rc;
  const double* crossT = (const double*)((char*)workspace + lp.off_crossT);
  const size_t lds = optl_score_lds(lp.q.n, lp.q.C);
  const dim3 grid((unsigned)std::min<int64_t>(K, OPTL_REWARDS_WGS), (unsigned)p->E);
  if (lp.q.n <= 64)
    hipLaunchKernelGGL(k_opt_rewards_actions<1>, grid, dim3(OPTL_BLOCK), lds, s, lp.q, (const double*)workspace, crossT, actions, K, out);
  else
    hipLaunchKernelGGL(k_opt_rewards_actions<2>, grid, dim3(OPTL_BLOCK), lds, s, lp.q, (const double*)workspace, crossT, actions, K, out);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) OPT_FAIL(V2X_EHIP, "opt_rewards_actions: launch failed: %s", hipGetErrorString(err));
  return V2X_OK;
}

}  // extern "C"
