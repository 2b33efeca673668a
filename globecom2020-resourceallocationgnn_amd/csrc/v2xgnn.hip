// Host side of libv2xgnn.so: the C ABI declared in include/v2xgnn.h.
// Owns parameters, optimizer state and activation workspaces in HBM, sequences the kernels of
// kernels.hpp for Model.predict / Model.fit (BS_brain.py:218-235), optionally as a hipGraph.
#include "../../include/v2xgnn.h"
#include "kernels.hpp"
#include "kernels_wide.hpp"
#include "kernels_fused.hpp"
#include "kernels_fused_split.hpp"
#include "kernels_mlpwg.hpp"
#include "kernels_small.hpp"
#include "kernels_ragged.hpp"
#include "kernels_ragged_small.hpp"
#include "host_pack.hpp"
#include "knobs.hpp"

#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

using namespace v2x;

namespace {

thread_local std::string g_err;

struct LayerDesc {
  int64_t off;          // offset of slot 0 in the flat parameter buffer
  int64_t slot_stride;  // floats per slot: k_real*n_out + n_out
  int k_real, n_out;    // real weight shape
  int kp, np;           // padded (multiples of 16)
  RowPad pad;           // padded K row -> real row
  int n_slabs = 0;      // partial-sum slabs the last weight-gradient launch wrote for this layer
};

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
};

struct ProfRec { int id; hipEvent_t ev0, ev1; };

struct GraphKey {
  int kind; const void* ptrs[12]; int sizes[6]; double scalar;
  int64_t gen;          // workspace generation of ANOTHER model whose buffers the graph bakes in (v2x_dqn_step: the target)
  bool operator<(const GraphKey& o) const { return memcmp(this, &o, sizeof(GraphKey)) < 0; }
};

struct WideWgradPlan { WideWgradArgs a; int kt, nt, ntw, sp; };     // one layer's wide weight gradient: arguments + tiling

}  // namespace

struct v2x_model {
  v2x_config cfg;
  int S, Dn, De, L, F, N, C;
  std::vector<LayerDesc> gnn, dense;
  int64_t P = 0;
  float *params = nullptr, *grads = nullptr, *mom = nullptr, *vel = nullptr;
  int64_t iterations = 0;
  // activation workspace (capacity in rows)
  int64_t cap_rows = 0;
  std::vector<float*> h, a;
  float *z1 = nullptr, *z2 = nullptr, *z3 = nullptr, *q = nullptr;
  float *dq = nullptr, *dz1 = nullptr, *dz2 = nullptr, *dz3 = nullptr, *gha = nullptr, *rowloss = nullptr;
  std::vector<float*> dpre;     // one pre-activation gradient per GNN stage (read concurrently by k_wgrad)
  unsigned* nbmask = nullptr;            // [cap_rows] non-neighbour masks: fused forward -> fused backward (complement form)
  bool frag_live = false;                // h_L, a_L (and then gha) of the last training forward are fragment-major (BatchPlan::frag_ok)
  unsigned short* gate_bits = nullptr;   // ReLU' gates of the fused forward for the fused backward: [L][gate_stride]
  int64_t gate_stride = 0;               // ushorts per stage: N x ceil(B / 16) x 64 <= 4 R + 64 N
  hipStream_t cap = nullptr;    // hipGraphs are recorded on this stream and launched on the caller's (run_maybe_graph)
  float* loss_dev = nullptr;
  float* loss_part = nullptr;  // 64 partial sums + the arrival counter of the split loss reduction
  float* zero_buf = nullptr;   // 4 KiB of zeros
  float* slab = nullptr; int slab_cap = 0;
  int reduce_groups = 0;        // AdamArgs::groups of the last launch_reduce_adam (v2x_debug_layer_slabs)
  // v2x_debug_wide_tiling: {ny, mbs, n_full_rb, n_rb} of the k_wide_gemm launches and {kt, nt, sp, folded} of the wide
  // weight-gradient roles enqueued since it was last read (the first WIDE_REC_LAUNCHES / WIDE_REC_ROLES of them)
  std::vector<int32_t> wide_rec_tiles, wide_rec_roles;
  // staging for host-side inputs
  DevBuf st_xe, st_nbr, st_goff, st_rp, st_ci, st_y, st_q;
  DevBuf adj_mask;              // adjacency bit masks of the current batch (dense-graph aggregation)
  DevBuf plan_buf;              // work plan of the ragged fused forward (kernels_ragged.hpp): first graph of every workgroup
  int plan_len = 0;             // entries of the last plan (workgroups + 1)
  Knobs knobs;                                  // the environment switches, read once at v2x_create (knobs.hpp)
  long long* ts_buf = nullptr;                  // Knobs::fused_ts: phase time stamps of the fused forward (measurement)
  bool raw_params = false;                      // v2x_param_ptr was called: re-pack before every fused forward
  bool pk_stale = false;                        // the fragment-major copy must be rebuilt before the next fused forward
  unsigned long long* small_h = nullptr;        // exchange buffer of the few-graph predict (kernels_small.hpp) [L + 1][SMALL_ROWS][F] tagged words
  unsigned long long* small_sync = nullptr;     // and per-graph departure counters [SMALL_ROWS] (64-bit)
  char* pin_h = nullptr; char* pin_d = nullptr;  // pinned, device-mapped window for host-resident few-graph predicts: the
                                                // kernel reads the batch and writes q THROUGH it (no copy launches)
  float *pk_fwd = nullptr, *pk_bwd = nullptr;   // fragment-major copies of the GNN weights (kernels_fused.hpp)
  // split-tile fused kernels (kernels_fused_split.hpp): K workgroups per 16-graph tile at the shares of the global batch
  unsigned long long* xchg_buf = nullptr;       // [2 L slabs][xchg_cap_tiles][N][F / 16][64][4] tagged words
  unsigned long long* xchg_sync = nullptr;      // [xchg_cap_tiles] departures
  int xchg_cap_tiles = 0;
  int* flag_host = nullptr;     // pinned, device-mapped word the kernels raise on a contract violation (tile guards,
  int* flag_dev = nullptr;      // k_validate_batch); read by the host after any synchronising call
  bool phase0_done = false;                     // phase 0 of v2x_forward_backward_phase left its activations and dz / gha for the later
                                                // phases; every other call that runs a forward clears it
  std::string err;
  // profiling
  bool prof = false;
  std::vector<std::string> prof_names;
  std::vector<ProfRec> prof_recs;
  // hipGraph cache
  // a captured step + the per-layer slab counts its weight-gradient launches write (host state that the launches
  // OUTSIDE the graph -- the Adam / slab-sum kernel of train_step -- depend on)
  struct GraphEntry { hipGraphExec_t exec; std::vector<int> n_slabs; bool frag_live; int reduce_groups; };
  int64_t ws_gen = 0;           // bumped whenever a workspace buffer is re-allocated (keys of graphs that bake in ANOTHER model's workspace)
  std::map<GraphKey, GraphEntry> graphs;
  bool capturing = false;
  float* adam_scal = nullptr;                   // {lr_t, beta1, beta2, eps} of the current step, in device memory (WideWgradArgs::adam)
  bool prof_no_fuse = false;
  // v2x_train_step_dp (dp_native.hpp): the stream the bucket collectives run on and its events, made on first use
  hipStream_t dp_st = nullptr;
  std::vector<hipEvent_t> dp_ev;
};

namespace {

#define FAIL(m, code, ...)                                   \
  do {                                                       \
    char _b[512];                                            \
    snprintf(_b, sizeof(_b), __VA_ARGS__);                   \
    if (m) (m)->err = _b; else g_err = _b;                   \
    return code;                                             \
  } while (0)

#define HIPCHK(m, call)                                                                     \
  do {                                                                                      \
    hipError_t _e = (call);                                                                 \
    if (_e != hipSuccess) FAIL(m, V2X_EHIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(_e), __FILE__, __LINE__); \
  } while (0)

#define CHK(x)                 \
  do {                         \
    int _r = (x);              \
    if (_r != V2X_OK) return _r; \
  } while (0)

// the switches of a call: the model's, or the process-wide copy for the entry points that may come without a model
const Knobs& knobs_of(const v2x_model* m) { return m ? m->knobs : process_knobs(); }

// Captured graphs bake in the addresses of the workspace buffers: whenever one of them is re-allocated every cached
// graph is dropped (it would replay into freed memory and its outputs would no longer be where the caller reads them).
void drop_graphs(v2x_model* m) {
  for (auto& kv : m->graphs) hipGraphExecDestroy(kv.second.exec);
  m->graphs.clear();
  m->ws_gen += 1;               // every caller is about to re-allocate (or has invalidated) something captured graphs point at
}

int ensure(v2x_model* m, DevBuf& b, size_t bytes) {
  if (bytes <= b.cap) return V2X_OK;
  if (m->capturing) FAIL(m, V2X_ESTATE, "buffer growth during graph capture");
  drop_graphs(m);
  if (b.p) HIPCHK(m, hipFree(b.p));
  b.p = nullptr; b.cap = 0;
  HIPCHK(m, hipMalloc(&b.p, bytes));
  b.cap = bytes;
  return V2X_OK;
}

template <typename T>
int dev_alloc(v2x_model* m, T** p, size_t n) {
  HIPCHK(m, hipMalloc(reinterpret_cast<void**>(p), n * sizeof(T)));
  return V2X_OK;
}

int prof_id(v2x_model* m, const char* name) {
  for (size_t i = 0; i < m->prof_names.size(); ++i)
    if (m->prof_names[i] == name) return (int)i;
  m->prof_names.push_back(name);
  return (int)m->prof_names.size() - 1;
}

// launch wrapper: optional HIP-event bracket per kernel for in-situ timing
#define LAUNCH(m, kname, kern, grid, threads, lds, stream, ...)                          \
  do {                                                                                  \
    ProfRec _r;                                                                         \
    const bool _p = (m) && (m)->prof && !(m)->capturing;                                \
    if (_p) {                                                                           \
      _r.id = prof_id(m, kname);                                                          \
      hipEventCreate(&_r.ev0); hipEventCreate(&_r.ev1);                                     \
      hipEventRecord(_r.ev0, stream);                                                     \
    }                                                                                   \
    hipLaunchKernelGGL(kern, grid, dim3(threads), lds, stream, __VA_ARGS__);            \
    if (_p) { hipEventRecord(_r.ev1, stream); (m)->prof_recs.push_back(_r); }             \
    hipError_t _e = hipGetLastError();                                                  \
    if (_e != hipSuccess) FAIL(m, V2X_EHIP, "launch %s failed: %s", kname, hipGetErrorString(_e)); \
  } while (0)

// A run-time value as a template argument: f(std::integral_constant<int, V>{}) for the V among Vs that equals v, and what it
// returns (V2X_OK or a launch error); V2X_EINVAL when no V does -- the caller names the unsupported shape
template <int... Vs, typename Fn>
int with_const(int v, Fn&& f) {
  int rc = V2X_EINVAL;
  (void)((v == Vs && ((rc = f(std::integral_constant<int, Vs>{})), true)) || ...);
  return rc;
}

// ------------------------------------------------------------------------------------ layout
void build_layout(v2x_model* m) {
  const int F = m->F, Dn = m->Dn, De = m->De, C = m->C;
  const int xr = Dn + De;   // real rows of the packed xe block
  int64_t off = 0;
  auto push = [&](std::vector<LayerDesc>& v, int k_real, int n_out, int kp, int np, RowPad pad) {
    LayerDesc d;
    d.off = off; d.k_real = k_real; d.n_out = n_out; d.kp = kp; d.np = np; d.pad = pad;
    d.slot_stride = (int64_t)k_real * n_out + n_out;
    off += d.slot_stride * m->S;
    v.push_back(d);
  };
  push(m->gnn, xr + F, F, XE + F, F, RowPad{xr, XE - xr, xr + F});
  for (int s = 1; s <= m->L; ++s)
    push(m->gnn, 2 * F + xr, F, 2 * F + XE, F, RowPad{F + xr, XE - xr, 2 * F + xr});
  push(m->dense, 2 * F + Dn, H1, 2 * F + XE, H1, RowPad{F + Dn, XE - Dn, 2 * F + Dn});
  push(m->dense, H1, H2, H1, H2P, RowPad{H1, 0, H1});
  push(m->dense, H2, H3, H2P, H3P, RowPad{H2, H2P - H2, H2});
  push(m->dense, H3, C, H3P, CP, RowPad{H3, H3P - H3, H3});
  m->P = off;
}

// dynamic LDS above 64 KiB has to be opted into per kernel; done once per model at create time so
// that nothing but kernel launches happens inside a stream capture
void allow_big_lds(const void* f) { hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); }

template <int F>
void set_attrs_f() {
  allow_big_lds((const void*)k_gemm_rows<F, false, false, false>);
  allow_big_lds((const void*)k_gemm_rows<F, false, true, false>);
  allow_big_lds((const void*)k_gemm_rows<F, true, true, false>);
  allow_big_lds((const void*)k_gemm_rows<F, true, false, true>);
  allow_big_lds((const void*)k_mlp_fwd<F>);
  allow_big_lds((const void*)k_mlp_train_wg<F>);
  allow_big_lds((const void*)k_mlp_train_wg<F, true>);
  allow_big_lds((const void*)k_wgrad<F, 0>);
}

template <int F>
void set_attrs_fused() {
  allow_big_lds((const void*)k_gnn_fwd_fused<F, 1>); allow_big_lds((const void*)k_gnn_fwd_fused<F, 1, false, true>);
  allow_big_lds((const void*)k_gnn_fwd_fused<F, 2>); allow_big_lds((const void*)k_gnn_fwd_fused<F, 2, false, true>);
  allow_big_lds((const void*)k_gnn_fwd_fused<F, 3>); allow_big_lds((const void*)k_gnn_fwd_fused<F, 3, false, true>);
  allow_big_lds((const void*)k_gnn_fwd_fused<F, 4>); allow_big_lds((const void*)k_gnn_fwd_fused<F, 4, false, true>);
  allow_big_lds((const void*)k_gnn_bwd_fused<F, 1>); allow_big_lds((const void*)k_gnn_bwd_fused<F, 1, false, true>);
  allow_big_lds((const void*)k_gnn_bwd_fused<F, 2>); allow_big_lds((const void*)k_gnn_bwd_fused<F, 2, false, true>);
  allow_big_lds((const void*)k_gnn_bwd_fused<F, 3>); allow_big_lds((const void*)k_gnn_bwd_fused<F, 3, false, true>);
  allow_big_lds((const void*)k_gnn_bwd_fused<F, 4>); allow_big_lds((const void*)k_gnn_bwd_fused<F, 4, false, true>);
  allow_big_lds((const void*)k_gnn_fwd_split<F, 1>); allow_big_lds((const void*)k_gnn_bwd_split<F, 1>);
  allow_big_lds((const void*)k_gnn_fwd_split<F, 2>); allow_big_lds((const void*)k_gnn_bwd_split<F, 2>);
  allow_big_lds((const void*)k_gnn_fwd_split<F, 3>); allow_big_lds((const void*)k_gnn_bwd_split<F, 3>);
  if (F == 64) {
    allow_big_lds((const void*)k_gnn_fwd_split<64, 2, true>); allow_big_lds((const void*)k_gnn_bwd_split<64, 2, true>);
    allow_big_lds((const void*)k_gnn_fwd_fused<64, 3, true>); allow_big_lds((const void*)k_gnn_bwd_fused<64, 3, true>);
    allow_big_lds((const void*)k_gnn_fwd_fused<64, 3, true, true>); allow_big_lds((const void*)k_gnn_bwd_fused<64, 3, true, true>);
  }
}

void set_attrs(int F, const Knobs& kn) {
  if (F == 16) set_attrs_fused<16>();
  if (F == 32) set_attrs_fused<32>();
  if (F == 64) set_attrs_fused<64>();
  allow_big_lds((const void*)k_agg<false>);
  allow_big_lds((const void*)k_agg<true>);
  allow_big_lds((const void*)k_agg_dense<false>);
  allow_big_lds((const void*)k_agg_dense<true>);
  if (F == 16) set_attrs_f<16>();
  if (F == 32) set_attrs_f<32>();
  if (F == 64) set_attrs_f<64>();
  if (F >= 128) {                     // wide path: tail MLP kernels + the narrow weight-gradient kernel for Dense 1..3
    if (kn.debug_occ) {
      int n1 = 0, n2 = 0, n3 = 0, n4 = 0;
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&n1, k_wide_gemm<false, 4>, 256, 0);
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&n2, k_wide_gemm<true, 4>, 256, 0);
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&n3, k_wide_wgrad_multi, 256, 0);
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&n4, k_agg_dense<false>, 256, 36 * 1024);
      hipFuncAttributes fa;
      hipFuncGetAttributes(&fa, (const void*)k_wide_gemm<false, 4>);
      fprintf(stderr, "occupancy (workgroups per CU): k_wide_gemm<false,4> %d, <true,4> %d, k_wide_wgrad_multi %d, k_agg_dense(36 KB) %d; "
              "k_wide_gemm<false,4>: %d regs, %zu B static LDS, maxDynamic %d\n", n1, n2, n3, n4, fa.numRegs, fa.sharedSizeBytes, fa.maxDynamicSharedSizeBytes);
    }
    allow_big_lds((const void*)k_mlp_fwd<0>);
    allow_big_lds((const void*)k_mlp_bwd<0>);
    allow_big_lds((const void*)k_wgrad<64, 1>);
  }
}

inline bool is_wide(const v2x_model* m) { return m->F >= 128; }

int ensure_rows(v2x_model* m, int64_t R) {
  if (R <= m->cap_rows) return V2X_OK;
  if (m->capturing) FAIL(m, V2X_ESTATE, "workspace growth during graph capture");
  drop_graphs(m);
  auto re = [&](float*& p, int64_t w) -> int {
    if (p) HIPCHK(m, hipFree(p));
    p = nullptr;
    HIPCHK(m, hipMalloc(reinterpret_cast<void**>(&p), (size_t)(R * w) * sizeof(float)));
    return V2X_OK;
  };
  const int F = m->F;
  for (int s = 0; s <= m->L; ++s) { CHK(re(m->h[s], F)); CHK(re(m->a[s], F)); }
  CHK(re(m->z1, H1)); CHK(re(m->z2, H2)); CHK(re(m->z3, H3)); CHK(re(m->q, m->C));
  CHK(re(m->dq, m->C)); CHK(re(m->dz1, H1)); CHK(re(m->dz2, H2)); CHK(re(m->dz3, H3));
  CHK(re(m->gha, 2 * F)); CHK(re(m->rowloss, 1));
  for (int s = 0; s <= m->L; ++s) CHK(re(m->dpre[s], F));
  if (m->gate_bits) HIPCHK(m, hipFree(m->gate_bits));
  m->gate_bits = nullptr;
  if (m->nbmask) HIPCHK(m, hipFree(m->nbmask));
  m->nbmask = nullptr;
  HIPCHK(m, hipMalloc(reinterpret_cast<void**>(&m->nbmask), (size_t)R * sizeof(unsigned)));
  m->gate_stride = 4 * R + 64 * (int64_t)m->N;
  HIPCHK(m, hipMalloc(reinterpret_cast<void**>(&m->gate_bits), (size_t)((m->L + 1) * m->gate_stride) * sizeof(unsigned short)));
  m->cap_rows = R;
  return V2X_OK;
}

// Weight-gradient decomposition.  A role (= one layer) is cut into `nc` row chunks per slot, one workgroup and
// one partial-sum slab each.  A workgroup walks its chunk sequentially (4 waves, 16-row blocks round-robin), so
// the launch is as long as its longest workgroup: the chunk count of every role fused into a launch is chosen
// proportional to the role's MFMA work (KT*NT tiles) so that the whole launch is about ONE balanced round of
// the chip (Knobs::wg_rounds rounds), instead of the same chunking for a 45-tile and a 2-tile layer.
int n_cus();
int role_chunks(const Knobs& kn, int n_idx, int n_slots, int work, int total_work, int* chunk_out, int dflt_rows = 768) {
  const int rounds = kn.wg_rounds;
  const int rows = kn.wg_chunk > 0 ? kn.wg_chunk : dflt_rows;
  int nc;
  if (rounds > 0) {                                             // work-proportional workgroup counts
    long target = ((long)n_cus() * rounds * work + total_work / 2) / total_work;
    nc = (int)(target / n_slots);
  } else {                                                      // uniform rows per workgroup (measured best: 768)
    nc = (n_idx + rows - 1) / rows;
  }
  if (nc < 1) nc = 1;
  const int max_nc = (n_idx + 4 * WG_TR - 1) / (4 * WG_TR);                         // >= one block per wave
  if (nc > max_nc) nc = max_nc;
  if (nc < 1) nc = 1;
  int chunk = (n_idx + nc - 1) / nc;
  chunk = (chunk + 4 * WG_TR - 1) / (4 * WG_TR) * (4 * WG_TR);
  nc = (n_idx + chunk - 1) / chunk;
  if (nc < 1) nc = 1;
  *chunk_out = chunk;
  return nc;
}

int ensure_slabs(v2x_model* m, int nc) {
  if (nc <= m->slab_cap) return V2X_OK;
  if (m->capturing) FAIL(m, V2X_ESTATE, "slab growth during graph capture");
  drop_graphs(m);
  if (m->slab) HIPCHK(m, hipFree(m->slab));
  m->slab = nullptr;
  HIPCHK(m, hipMalloc(reinterpret_cast<void**>(&m->slab), (size_t)nc * m->P * sizeof(float)));
  HIPCHK(m, hipMemset(m->slab, 0, (size_t)nc * m->P * sizeof(float)));
  // (hipMemset runs on the null stream, which does not order against the caller's stream when that is non-blocking -- as
  //  every stream of PyTorch's pool is: wait here, or the zeroing may land after this step's first launches)
  HIPCHK(m, hipDeviceSynchronize());
  m->slab_cap = nc;
  return V2X_OK;
}

// ------------------------------------------------------------------------------------ device-side error flag
struct FlagWord { int* host = nullptr; int* dev = nullptr; };
int alloc_flag(FlagWord* f) {
  void* h = nullptr;
  if (hipHostMalloc(&h, 64, hipHostMallocMapped) != hipSuccess) return V2X_EHIP;
  memset(h, 0, 64);
  void* d = nullptr;
  if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess) { hipHostFree(h); return V2X_EHIP; }
  f->host = (int*)h; f->dev = (int*)d;
  return V2X_OK;
}
FlagWord* global_flag() {            // the per-kernel entry points that take no model handle
  static FlagWord f;
  static const bool once = [] { alloc_flag(&f); return true; }();
  (void)once;
  return &f;
}
int* flag_dev_of(v2x_model* m) { return m ? m->flag_dev : global_flag()->dev; }

// the one-launch predict's exchange buffer and departure counters back to their initial state (synchronous)
int arm_xchg(v2x_model* m, int tiles, unsigned long long floor);
int xchg_max_count(v2x_model* m, unsigned long long* out);
size_t xchg_bytes(const v2x_model* m, int tiles) {
  return (size_t)std::max(1, 2 * m->L) * tiles * m->N * (m->F / 16) * 256 * sizeof(unsigned long long);
}
int reset_exchange(v2x_model* m) {
  if (!m->small_h && !m->xchg_buf) return V2X_OK;
  HIPCHK(m, hipDeviceSynchronize());
  if (m->small_h) {
    HIPCHK(m, hipMemset(m->small_h, 0, (size_t)(m->L + 1) * 256 * m->F * sizeof(unsigned long long)));     // tag 0 = never written
    HIPCHK(m, hipMemset(m->small_sync, 0, (size_t)256 * sizeof(unsigned long long)));
  }
  if (m->xchg_buf) {
    unsigned long long seen = 0;
    CHK(xchg_max_count(m, &seen));
    CHK(arm_xchg(m, m->xchg_cap_tiles, seen + 2));          // (+ 2: a launch that died half-way may not have advanced its tiles)
  }
  return V2X_OK;
}

// to be called after the stream was synchronised: reports and clears what the kernels raised
int check_flag(v2x_model* m) {
  volatile int* p = m ? m->flag_host : global_flag()->host;
  if (!p) return V2X_OK;
  const int v = *p;
  if (!v) return V2X_OK;
  *p = 0;
  if (v & SM_ERR_TIMEOUT) {
    // k_predict_small gave up waiting for a neighbour row (kernels_small.hpp, SM_POLL_CAP): the exchange state is not the one
    // the launch expected -- an earlier launch of this model died half-way (departure counters between two multiples of N),
    // or the caller corrupted it.  Re-arm it, so that the NEXT predict works, and report this one.
    if (m) reset_exchange(m);
    FAIL(m, V2X_ESTATE, "predict: the one-launch kernel timed out waiting for a neighbour's row (exchange buffer out of step: an "
                        "earlier launch was aborted?); the exchange was reset, this call's q is invalid%s",
         (v & SM_ERR_SOURCE) ? "; the batch also holds a source id outside its graph" : "");
  }
  if (v & FZ_ERR_XCHG) {
    // a member of a split tile (kernels_fused_split.hpp) gave up waiting for its partners' rows: same remedy
    if (m) reset_exchange(m);
    FAIL(m, V2X_ESTATE, "fused graph layers: a split-tile workgroup timed out waiting for its partners' rows (exchange out of step: an "
                        "earlier launch was aborted, or the partners were not co-resident); the exchange was reset, this call's results are invalid");
  }
  if (v & 1) FAIL(m, V2X_EINVAL, "batch: a graph has more rows / edges than max_nodes / max_edges allow (LDS tile guard); results are invalid");
  FAIL(m, V2X_EINVAL, "batch violates the layout contract:%s%s%s%s", (v >> 4) & 1 ? " graph sizes vs max_nodes / graph_off;" : "",
       (v >> 4) & 2 ? " row_ptr not monotone / edge counts vs max_edges;" : "", (v >> 4) & 4 ? " source id outside its graph;" : "",
       (v >> 4) & 8 ? " sources of a row not strictly ascending (duplicate edges);" : "");
}

// ------------------------------------------------------------------------------------ batches
struct DevBatch {
  int B, R, E, max_nodes, max_edges;
  const float* xe; const float* nbr;
  const int32_t* goff; const int32_t* rp; const int32_t* ci;
};

// Host batches are checked against the layout contract before anything is copied (O(B) for the sizes that size the
// LDS tiles, O(E) for the edge list; V2X_TRUSTED_BATCHES=1 skips the O(E) part).  Device batches: v2x_validate_batch.
int validate_host_batch(v2x_model* m, const v2x_batch* b, int n_nodes) {
  const int B = b->n_graphs, R = b->n_rows;
  const int32_t *go = b->graph_off, *rp = b->row_ptr, *ci = b->col_idx;
  if (rp[0] != 0 || rp[R] != b->n_edges) FAIL(m, V2X_EINVAL, "batch: row_ptr[0] != 0 or row_ptr[n_rows] != n_edges");
  if (go && (go[0] != 0 || go[B] != R)) FAIL(m, V2X_EINVAL, "batch: graph_off[0] != 0 or graph_off[n_graphs] != n_rows");
  const bool trusted = knobs_of(m).trusted_batches;
  for (int g = 0; g < B; ++g) {
    const int64_t r0 = go ? go[g] : (int64_t)g * n_nodes, r1 = go ? go[g + 1] : r0 + n_nodes;
    const int64_t n = r1 - r0;
    if (n < 1 || n > b->max_nodes || r0 < 0 || r1 > R)
      FAIL(m, V2X_EINVAL, "batch: graph %d has %lld rows, max_nodes is %d", g, (long long)n, b->max_nodes);
    const int64_t e0 = rp[r0], e1 = rp[r1];
    if (e1 < e0 || e1 - e0 > b->max_edges)
      FAIL(m, V2X_EINVAL, "batch: graph %d has %lld edges, max_edges is %d", g, (long long)(e1 - e0), b->max_edges);
    if (trusted) continue;
    for (int64_t q = r0; q < r1; ++q) {
      const int a0 = rp[q], a1 = rp[q + 1];
      if (a1 < a0 || a0 < e0 || a1 > e1) FAIL(m, V2X_EINVAL, "batch: row_ptr not monotone at row %lld", (long long)q);
      int prev = -1;
      for (int e = a0; e < a1; ++e) {
        const int c = ci[e];
        if (c < 0 || c >= n) FAIL(m, V2X_EINVAL, "batch: source id %d of row %lld lies outside its %lld-node graph", c, (long long)q, (long long)n);
        if (c <= prev) FAIL(m, V2X_EINVAL, "batch: sources of row %lld are not strictly ascending (duplicate edge?)", (long long)q);
        prev = c;
      }
    }
  }
  return V2X_OK;
}

int resolve_batch(v2x_model* m, const v2x_batch* b, DevBatch* d, hipStream_t st) {
  if (!b || b->n_graphs <= 0 || b->n_rows <= 0 || !b->xe || !b->row_ptr || (b->n_edges > 0 && !b->col_idx))
    FAIL(m, V2X_EINVAL, "batch: null pointer or non-positive size");
  if (!m->cfg.variable_graphs && b->n_rows != b->n_graphs * m->N)
    FAIL(m, V2X_EINVAL, "batch: n_rows (%d) != n_graphs*n_nodes (%d*%d)", b->n_rows, b->n_graphs, m->N);
  if (m->cfg.variable_graphs && !b->graph_off) FAIL(m, V2X_EINVAL, "batch: variable_graphs needs graph_off");
  if (b->max_nodes <= 0 || b->max_edges < 0) FAIL(m, V2X_EINVAL, "batch: max_nodes/max_edges not set");
  if (!m->cfg.variable_graphs && b->max_nodes != m->N)      // max_nodes selects kernels and sizes LDS tiles: one meaning only
    FAIL(m, V2X_EINVAL, "batch: max_nodes (%d) must equal n_nodes (%d) for a fixed-size model", b->max_nodes, m->N);
  d->B = b->n_graphs; d->R = b->n_rows; d->E = b->n_edges;
  d->max_nodes = b->max_nodes; d->max_edges = b->max_edges;
  if (b->on_device) {
    d->xe = b->xe; d->nbr = b->nbr_init; d->goff = b->graph_off; d->rp = b->row_ptr; d->ci = b->col_idx;
    return V2X_OK;
  }
  CHK(validate_host_batch(m, b, m->N));
  const size_t R = b->n_rows;
  CHK(ensure(m, m->st_xe, R * XE * sizeof(float)));
  HIPCHK(m, hipMemcpyAsync(m->st_xe.p, b->xe, R * XE * sizeof(float), hipMemcpyHostToDevice, st));
  d->xe = (const float*)m->st_xe.p;
  d->nbr = nullptr;
  if (b->nbr_init) {
    CHK(ensure(m, m->st_nbr, R * m->F * sizeof(float)));
    HIPCHK(m, hipMemcpyAsync(m->st_nbr.p, b->nbr_init, R * m->F * sizeof(float), hipMemcpyHostToDevice, st));
    d->nbr = (const float*)m->st_nbr.p;
  }
  d->goff = nullptr;
  if (b->graph_off) {
    CHK(ensure(m, m->st_goff, (size_t)(b->n_graphs + 1) * 4));
    HIPCHK(m, hipMemcpyAsync(m->st_goff.p, b->graph_off, (size_t)(b->n_graphs + 1) * 4, hipMemcpyHostToDevice, st));
    d->goff = (const int32_t*)m->st_goff.p;
  }
  CHK(ensure(m, m->st_rp, (R + 1) * 4));
  HIPCHK(m, hipMemcpyAsync(m->st_rp.p, b->row_ptr, (R + 1) * 4, hipMemcpyHostToDevice, st));
  d->rp = (const int32_t*)m->st_rp.p;
  CHK(ensure(m, m->st_ci, (size_t)(b->n_edges > 0 ? b->n_edges : 1) * 4));
  if (b->n_edges > 0)
    HIPCHK(m, hipMemcpyAsync(m->st_ci.p, b->col_idx, (size_t)b->n_edges * 4, hipMemcpyHostToDevice, st));
  d->ci = (const int32_t*)m->st_ci.p;
  return V2X_OK;
}

// ------------------------------------------------------------------------------------ launchers

// Every launch covers the whole batch: the kernels' g_base / idx_base arguments are 0, their g_end is B.
struct IdxMap { int idx_base, n_idx, row_stride, base_mul, grid_y; };
IdxMap idx_map(const v2x_model* m, const DevBatch& d) {
  IdxMap x;
  x.idx_base = 0;
  if (m->S == 1) {            // shared weights: the GEMM row index is the node row
    x.row_stride = 1; x.base_mul = 0; x.grid_y = 1;
    x.n_idx = m->cfg.variable_graphs ? d.R : d.B * m->N;
  } else {                    // per-node weights: slot k owns rows b*N + k, index = graph b
    x.n_idx = d.B; x.row_stride = m->N; x.base_mul = 1; x.grid_y = m->N;
  }
  return x;
}

// How one batch runs: every path decision of the dispatcher, made ONCE per C-ABI call by plan_batch (below, with the predicates
// and their measurements) and handed down by const reference.  A pure function of the model's shape and switches, what the
// model allocated at create (pk_fwd, pk_bwd, small_h, adam_scal; prof_no_fuse, which nothing sets), the batch's sizes, whether
// graph_off / nbr_init are given, and the chip's CU count: never cached, cheap to recompute, so the launches
// outside a replayed hipGraph agree with the ones inside it.
enum class GraphLayers { Layerwise, Fused, Ragged };
enum class RaggedPlan { Interval, Packed, Folded };     // by k_adj_masks per row interval; k_ragged_plan; k_ragged_plan's tables by workgroup 0 of k_adj_masks
struct BatchPlan {
  IdxMap x;                              // GEMM row index of the whole batch
  GraphLayers form = GraphLayers::Layerwise;
  bool mlp_wg = false;                   // the decision MLP trains in one launch (k_mlp_train_wg): narrow features
  bool small_predict = false;            // a forward alone is the one-launch few-graph predict
  // fused graph layers
  int tiles = 0, split = 1;              // 16-graph tiles; K workgroups per tile (1: whole tiles)
  bool split_fwd = false, split_bwd = false;   // K > 1 and the direction's debugging switch leaves it on
  bool compl_sums = false;               // aggregation through the complement (whole tiles only: already combined with K <= 1)
  size_t fused_lds_fwd = 0, fused_lds_bwd = 0;
  // ragged fused graph layers
  bool ragged_small = false, ragged_bwd = false;       // small-tile kernels; the backward is fused too
  int cap = 0, capp = 0, wgs = 0, plan_words = 0;
  RaggedPlan plan_form = RaggedPlan::Interval;
  // layer-wise aggregation
  bool dense_agg = false, need_adj_masks = false;
  // weight gradients and the hand-off to the MLP launch
  bool embed_rides = false, dense0_rides = false;      // on the graph layers' k_wgrad roles
  bool frag_ok = false;                  // h_L / a_L / gha may travel fragment-major between the fused kernels and k_mlp_train_wg
  bool wide_merge = false;               // wide model: every layer's weight gradient in ONE launch (unless the call is bucketed)
  bool wide_adam_fusable = false;        // ... whose epilogues may apply Adam
};

int n_cus() {
  static int n = 0;
  if (!n) {
    hipDeviceProp_t p;
    int dev = 0;
    hipGetDevice(&dev);
    n = (hipGetDeviceProperties(&p, dev) == hipSuccess && p.multiProcessorCount > 0) ? p.multiProcessorCount : 256;
  }
  return n;
}

// Large dense graphs (e.g. 100 links, in-degree 98): the contraction runs on the MFMA pipe against adjacency
// bit masks (k_agg_dense) instead of one LDS gather per edge.
bool use_dense_agg(const Knobs& kn, const DevBatch& d, int F) {
  const int dense_min_nodes = kn.agg_dense_min_nodes;
  const size_t rows_cap = (d.max_nodes + 15) / 16 * 16, mw = (d.max_nodes + 31) / 32;
  return F >= 64 && d.max_nodes >= dense_min_nodes && (int64_t)d.max_edges * 4 >= (int64_t)d.max_nodes * d.max_nodes &&
         rows_cap * AD_LDT * 4 + rows_cap * mw * 4 + 4 * 64 * 4 <= 160 * 1024;
}

AggDenseArgs agg_dense_args(const DevBatch& d, int N, int F) {
  AggDenseArgs q;
  memset(&q, 0, sizeof(q));
  q.graph_off = d.goff; q.row_ptr = d.rp; q.col_idx = d.ci;
  q.g_base = 0; q.n_graphs = d.B; q.n_nodes = N; q.F = F; q.n_fg = F / 64;
  q.rows_cap = (d.max_nodes + 15) / 16 * 16;
  q.mask_words = (d.max_nodes + 31) / 32;
  return q;
}

// bytes of the packed plan's 16-bit tables when it rides on the mask launch (AggDenseArgs::plan_cap)
size_t plan16_bytes(int n_graphs, int n_wgs) { return (size_t)(n_graphs + 1) * 4 + ((size_t)2 * (n_graphs + 1) + n_wgs + 1) * 2 + 8; }   // offsets + two tables + starts
int build_adj_masks(v2x_model* m, hipStream_t st, const AggDenseArgs& q) {
  size_t lds = (size_t)2 * q.rows_cap * q.mask_words * 4 + (size_t)(q.rows_cap + 1) * 4;   // by source + by destination + row_ptr slice
  int grid = q.n_graphs;
  if (q.plan_cap > 0) lds = std::max(lds, plan16_bytes(q.n_graphs, q.plan_n));                   // workgroup 0 makes the plan first
  LAUNCH(m, "k_adj_masks", k_adj_masks, dim3(grid), 256, lds, st, q);
  return V2X_OK;
}

// dense_agg: BatchPlan::dense_agg of a model's batch; use_dense_agg for the entry points that come without a model
int launch_agg(v2x_model* m, hipStream_t st, const DevBatch& d, bool dense_agg, int N, int F, const float* src, int src_stride,
               const float* add, int add_stride, const float* mask, float* out, int transpose) {
  if (F < 16 || F > 256 || (F & (F - 1))) FAIL(m, V2X_EINVAL, "agg: feat_dim must be a power of two in [16,256]");
  static const bool attrs_once = [] {        // the per-kernel entry points can get here without any model
    allow_big_lds((const void*)k_agg<false>); allow_big_lds((const void*)k_agg<true>);
    allow_big_lds((const void*)k_agg_small<false, false, false>); allow_big_lds((const void*)k_agg_small<true, true, true>);
    allow_big_lds((const void*)k_agg_small<true, true, false>); allow_big_lds((const void*)k_agg_small<true, false, false>);
    allow_big_lds((const void*)k_agg_dense<false>); allow_big_lds((const void*)k_agg_dense<true>);
    return true;
  }();
  (void)attrs_once;
  const Knobs& kn = knobs_of(m);
  if (dense_agg) {
    AggDenseArgs q = agg_dense_args(d, N, F);
    q.src = src; q.src_stride = src_stride; q.add = add; q.add_stride = add_stride; q.mask = mask; q.out = out;
    q.err = flag_dev_of(m);
    if (m) {
      q.adj = (unsigned*)m->adj_mask.p;                 // built by run_forward for this batch
      q.adjT = q.adj + (size_t)d.R * q.mask_words;
    } else {                                            // handle-less entry point: build into a scratch buffer
      static thread_local DevBuf scratch;
      const size_t need = (size_t)2 * d.R * q.mask_words * 4;
      if (need > scratch.cap) {
        if (scratch.p) hipFree(scratch.p);
        scratch.p = nullptr; scratch.cap = 0;
        HIPCHK(m, hipMalloc(&scratch.p, need));
        scratch.cap = need;
      }
      q.adj = (unsigned*)scratch.p;
      q.adjT = q.adj + (size_t)d.R * q.mask_words;
      CHK(build_adj_masks(m, st, q));
    }
    const size_t lds = (size_t)q.rows_cap * AD_LDT * 4 + (size_t)q.rows_cap * q.mask_words * 4 + 4 * 64 * 4;   // + partial column sums
    const dim3 grid((d.B + 7) / 8 * 8 * q.n_fg);
    if (transpose) { auto k = k_agg_dense<true>; LAUNCH(m, "k_agg_bwd", k, grid, 256, lds, st, q); }
    else { auto k = k_agg_dense<false>; LAUNCH(m, "k_agg_fwd", k, grid, 256, lds, st, q); }
    return V2X_OK;
  }
  AggArgs a;
  a.src = src; a.src_stride = src_stride; a.add = add; a.add_stride = add_stride; a.mask = mask; a.out = out;
  a.graph_off = d.goff; a.row_ptr = d.rp; a.col_idx = d.ci;
  a.g_base = 0; a.g_end = d.B; a.n_nodes = N; a.F = F;
  int sh = 0; while ((4 << sh) < F) ++sh;
  a.lpr_shift = sh;
  a.mask_words = (d.max_nodes + 31) / 32;
  a.transpose = transpose;
  a.err = flag_dev_of(m);
  const int nworkers = 256 >> sh;
  const size_t per_graph = (size_t)d.max_nodes * F * 4 + (size_t)(d.max_nodes + 1) * 4 + (size_t)d.max_edges * 4 +
                           (transpose ? (size_t)d.max_nodes * a.mask_words * 4 : 0);
  int gpw = 1;
  // few graphs per workgroup => many workers per graph => short per-worker row loops (the kernel is a
  // latency chain: stage -> barrier -> LDS gathers -> store); keep >= 8 workers per graph when F allows
  const int wpg_min = kn.agg_workers_per_graph;
  while (gpw * 2 <= nworkers && nworkers / (gpw * 2) >= wpg_min && (size_t)(gpw * 2) * per_graph <= 48 * 1024 && gpw * 2 <= d.B) gpw *= 2;
  a.gpw = gpw;
  a.rows_cap = gpw * d.max_nodes;
  a.edges_cap = gpw * d.max_edges;
  const size_t lds = (size_t)a.rows_cap * F * 4 + (size_t)(a.rows_cap + 1) * 4 + (size_t)(gpw + 1) * 4 +
                     (size_t)a.edges_cap * 4 + (transpose ? (size_t)a.rows_cap * a.mask_words * 4 : 0);
  if (lds > 160 * 1024) FAIL(m, V2X_EINVAL, "agg: graph tile (%zu B) exceeds the 160 KiB LDS", lds);
  const dim3 grid((d.B + gpw - 1) / gpw);
  // small tiles (the 20-link graphs of the headline configuration): everything fetched before the first wait
  const bool small_off = kn.agg_no_small;
  const int wpg = nworkers / gpw;
  const bool small = !small_off && d.ci != nullptr && (a.rows_cap << sh) <= 1024 && a.rows_cap + 1 <= 256 && a.edges_cap <= 1024 &&
                     (d.max_nodes + wpg - 1) / wpg <= 4;
  if (small) {
#define V2X_AGG_SMALL(T, A, M, NAME) { auto k = k_agg_small<T, A, M>; LAUNCH(m, NAME, k, grid, 256, lds, st, a); return V2X_OK; }
    if (!transpose) {
      if (!add && !mask) V2X_AGG_SMALL(false, false, false, "k_agg_fwd")
    } else {
      if (add && mask) V2X_AGG_SMALL(true, true, true, "k_agg_bwd")
      if (add && !mask) V2X_AGG_SMALL(true, true, false, "k_agg_bwd")
      if (!add && !mask) V2X_AGG_SMALL(true, false, false, "k_agg_bwd")
    }
#undef V2X_AGG_SMALL
  }
  if (transpose) { auto k = k_agg<true>; LAUNCH(m, "k_agg_bwd", k, grid, 256, lds, st, a); }
  else { auto k = k_agg<false>; LAUNCH(m, "k_agg_fwd", k, grid, 256, lds, st, a); }
  return V2X_OK;
}

// persistent-grid sizing: ~`wgs_per_cu` workgroups per CU in total, split evenly over the slots, so that
// every SIMD ends up with the same number of 16-row tiles (fp32 MFMA is the scarce resource)
int persistent_wgs_per_slot(int n_idx, int n_slots, int wgs_per_cu) {
  const int n_tiles = (n_idx + 15) / 16;
  int w = (n_cus() * wgs_per_cu) / n_slots;
  if (w < 1) w = 1;
  const int max_useful = (n_tiles + 3) / 4;          // at least one tile per wave
  if (w > max_useful) w = max_useful;
  if (w < 1) w = 1;
  return w;
}


// ---- wide-feature path (feat_dim >= 128): LDS-tiled GEMMs of kernels_wide.hpp -------------------------------
void set_idx(WideGemmArgs& a, const IdxMap& x) {
  a.n_idx = x.n_idx; a.row_stride = x.row_stride; a.base_mul = x.base_mul; a.idx_base = x.idx_base;
}

// Output tile width in 16-column tiles.  Measured at 100 links x 1024 graphs x 256 features: whole-width (256-column)
// tiles cut the operand re-reads 4x but leave 800 workgroups at 2 waves/SIMD and are SLOWER for the node update and
// its data gradient (343 / 295 us vs 276 / 253 us with 64-column tiles at 5 waves/SIMD: L2 absorbs the re-reads);
// Dense-0's 80 columns are one 5-tile strip instead of a 64 + 16 split (154 -> 110 us).
int wide_nt(int n_out) { return n_out <= 80 ? 5 : 4; }

// Tiling of one k_wide_gemm launch (kernels_wide.hpp, WideTiling) over `slots` resident workgroups, host arithmetic only:
// 128-row tiles; when the launch is more than one round of the slots (the chip's: five per CU) and its last round would be
// less than three quarters full, the row blocks of that last round run as two 64-row tiles each, dispatched last
// (tail = V2X_WIDE_TAIL; 0: whole tiles only)
WideTiling wide_tiling_plan(int n_idx, int grid_z, int n_out, int slots, int tail) {
  const int nt = wide_nt(n_out);
  WideTiling t;
  t.ny = (n_out + 16 * nt - 1) / (16 * nt);
  t.mbs = (n_idx + WD_TM - 1) / WD_TM;
  t.n_rb = t.mbs * grid_z;
  t.n_full_rb = t.n_rb;
  const int T = t.n_rb * t.ny, C = slots, rem = T % C;
  if (tail && T > C && rem > 0 && 4 * rem < 3 * C) t.n_full_rb = t.n_rb - rem / t.ny;
  // a launch that does not fill the resident slots at all (Dense-0 at configs[3]'s share: 800 tiles of 128 x 80 on 1,280
  // slots, three workgroups per CU instead of five): every row block as two half tiles (V2X_WIDE_TAIL=2 only: measured)
  if (tail == 2 && T < C && 2 * T > C) t.n_full_rb = 0;
  return t;
}

constexpr int WIDE_REC_LAUNCHES = 32, WIDE_REC_ROLES = 16;      // what v2x_debug_wide_tiling keeps between two reads

int launch_wide_gemm(v2x_model* m, hipStream_t st, WideGemmArgs& a, int grid_z, bool trans, const char* name) {
  const int nt = wide_nt(a.n_out);
  // V2X_WIDE_SLOTS: the rule plans for so many slots instead of the chip's (which row blocks run as half tiles, nothing else)
  const int slots = m->knobs.wide_slots > 0 ? m->knobs.wide_slots : 5 * n_cus();
  const WideTiling t = wide_tiling_plan(a.n_idx, grid_z, a.n_out, slots, m->knobs.wide_tail);
  if ((int)m->wide_rec_tiles.size() < 4 * WIDE_REC_LAUNCHES) m->wide_rec_tiles.insert(m->wide_rec_tiles.end(), {t.ny, t.mbs, t.n_full_rb, t.n_rb});
  const dim3 grid(t.n_full_rb * t.ny + 2 * (t.n_rb - t.n_full_rb) * t.ny);
#define V2X_WIDE_GEMM(T_, NTV) { auto k = k_wide_gemm<T_, NTV>; LAUNCH(m, name, k, grid, 256, 0, st, a, t); return V2X_OK; }
  if (!trans) {
    if (nt == 5) V2X_WIDE_GEMM(false, 5)
    V2X_WIDE_GEMM(false, 4)
  }
  V2X_WIDE_GEMM(true, 4)
#undef V2X_WIDE_GEMM
}

// out = act([seg...] W + b) of layer `ld`
int wide_fwd(v2x_model* m, hipStream_t st, const LayerDesc& ld, const IdxMap& x, const WideSeg* segs, int n_seg,
             float* out, int out_stride, int relu, const char* name) {
  WideGemmArgs a;
  memset(&a, 0, sizeof(a));
  int k = 0;
  for (int i = 0; i < n_seg; ++i) { a.seg[i] = segs[i]; k += segs[i].width; }
  a.n_seg = n_seg;
  a.W = m->params + ld.off; a.slot_stride = ld.slot_stride; a.pad = ld.pad; a.n_real = ld.n_out;
  a.k_total = k; a.n_out = ld.n_out; a.out = out; a.out_stride = out_stride; a.relu = relu; a.has_bias = 1;
  set_idx(a, x);
  return launch_wide_gemm(m, st, a, x.grid_y, false, name);
}

// gha[R][2F] = [dpre . W[h rows]^T | dpre . W[agg rows]^T];  `skip` = real weight rows between the two blocks
int wide_dgrad(v2x_model* m, hipStream_t st, const LayerDesc& ld, const IdxMap& x, const float* dpre, int d_width,
               int skip, float* gha, const char* name) {
  WideGemmArgs a;
  memset(&a, 0, sizeof(a));
  a.seg[0] = WideSeg{dpre, d_width, d_width}; a.n_seg = 1;
  a.W = m->params + ld.off; a.slot_stride = ld.slot_stride; a.pad = ld.pad; a.n_real = ld.n_out;
  a.k_total = d_width; a.n_out = 2 * m->F; a.split = m->F; a.skip = skip;
  a.out = gha; a.out_stride = 2 * m->F;
  set_idx(a, x);
  return launch_wide_gemm(m, st, a, x.grid_y, true, name);
}

// row splits of a wide weight gradient: enough workgroups to fill the chip; one split (= the gradient is written
// in place, no slab to sum) as soon as tiles x slots alone do that
int wide_splits(int n_idx, int n_tiles, int n_slots) {
  int sp = (3 * n_cus() / 2 + n_tiles * n_slots - 1) / (n_tiles * n_slots);
  const int max_sp = (n_idx + 255) / 256;                      // at least 256 rows per split
  if (sp > max_sp) sp = max_sp;
  return sp < 1 ? 1 : sp;
}

// arguments + tiling of one layer's wide weight gradient (and the memsets of an absent input segment's weight rows)
// merged: a role of the merged launch (wide_wgrad_flush); adam: its epilogue applies Adam (WideWgradArgs::adam)
int wide_wgrad_plan(v2x_model* m, hipStream_t st, LayerDesc& ld, const IdxMap& x, const WideSeg* segs, const int* seg_kpad,
                    int n_seg, const float* dpre, int d_stride, int zero_row0, int zero_rows, bool merged, bool adam, WideWgradPlan* out) {
  WideWgradArgs& a = out->a;
  memset(&a, 0, sizeof(a));
  int k_width = 0;
  for (int i = 0; i < n_seg; ++i) k_width += segs[i].width;
  // weight gradients: 128 input features x the whole output width per workgroup (324 -> 315 us for a GNN stage,
  // 180 -> 123 us for Dense-0); the 16-wide embed layer keeps 64 x 64 tiles
  const int KW = k_width <= 64 ? 64 : 128;
  int kt = 0, ns = 0;
  // the 16-wide [x | e] segment of a wide layer rides on the workgroup of K tile 0 (WideWgradArgs::xseg) instead of
  // costing a whole 128-wide K tile of its own.  Only worth it when the launch is balanced over many workgroups per CU
  // (the merged launch): on its own a stage is 500 workgroups on 256 CUs and as long as its fullest CU either way
  // (measured: 298 us unfolded, 333 us folded -- 400 workgroups, the same two per CU, one of them 12.5 % longer)
  const int fold = m->knobs.wide_fold;
  for (int i = 0; i < n_seg; ++i) {
    if (fold && merged && KW == 128 && n_seg > 1 && segs[i].width == XE && !a.xseg.ptr) { a.xseg = segs[i]; a.xseg_kpad = seg_kpad[i]; continue; }
    a.seg[ns] = segs[i]; a.seg_kpad[ns] = seg_kpad[i]; kt += (segs[i].width + KW - 1) / KW;
    ++ns;
  }
  a.n_seg = ns;
  a.dpre = dpre; a.d_stride = d_stride; a.n_real = ld.n_out; a.pad = ld.pad;
  a.slab = m->slab; a.slab_stride = m->P; a.layer_off = ld.off; a.slot_stride = ld.slot_stride;
  a.n_idx = x.n_idx; a.row_stride = x.row_stride; a.base_mul = x.base_mul; a.idx_base = x.idx_base;
  const int ntw = KW == 64 ? 4 : (ld.n_out <= 80 ? 5 : (ld.n_out <= 128 ? 8 : 16));   // output tile = ntw x 16 columns
  const int nt = (ld.n_out + 16 * ntw - 1) / (16 * ntw);
  const int sp = wide_splits(x.n_idx, kt * nt, x.grid_y);
  if (sp > m->slab_cap) FAIL(m, V2X_ESTATE, "wide wgrad: slabs not pre-sized (%d > %d)", sp, m->slab_cap);
  a.n_split = sp;
  a.rows_per_split = ((x.n_idx + sp - 1) / sp + 31) / 32 * 32;
  ld.n_slabs = sp;
  if (sp == 1) {            // no partial sums to add: write the gradient buffer itself (saves a 2 x P-float round trip)
    a.slab = m->grads;
    ld.n_slabs = 0;
  }
  if (adam && &ld != &m->gnn[0]) {         // (the embed layer keeps k_reduce_adam: its absent-input rows have no tile)
    if (sp != 1 || zero_rows > 0) FAIL(m, V2X_ESTATE, "wide wgrad: Adam cannot ride on a split weight gradient");
    a.adam = 1; a.param = m->params; a.mom = m->mom; a.vel = m->vel; a.adam_scal = m->adam_scal;
  }
  if (zero_rows > 0) {      // weight rows of an absent (identically zero) input segment: exact zero gradient
    const int64_t count = (int64_t)zero_rows * ld.n_out;
    for (int c = 0; c < sp; ++c) {
      float* dst = a.slab + (int64_t)c * a.slab_stride + ld.off + (int64_t)zero_row0 * ld.n_out;
      const dim3 zg((unsigned)std::min<int64_t>((count / 4 + 255) / 256, 64), x.grid_y);
      hipLaunchKernelGGL(k_zero_rows, zg, dim3(256), 0, st, dst, ld.slot_stride, count);
    }
  }
  out->kt = kt; out->nt = nt; out->ntw = ntw; out->sp = sp;
  if ((int)m->wide_rec_roles.size() < 4 * WIDE_REC_ROLES) m->wide_rec_roles.insert(m->wide_rec_roles.end(), {kt, nt, sp, a.xseg.ptr != nullptr ? 1 : 0});
  return V2X_OK;
}

// The roles of a backward pass that launches every wide weight gradient as ONE grid (wide_wgrad_flush); null = each on its own
struct WideRoles { std::vector<WideWgradPlan> v; bool adam = false; };     // adam: the epilogues apply Adam (single-GPU fit step)

int wide_wgrad(v2x_model* m, hipStream_t st, LayerDesc& ld, const IdxMap& x, const WideSeg* segs, const int* seg_kpad,
               int n_seg, const float* dpre, int d_stride, const char* name, WideRoles* roles, int zero_row0 = 0, int zero_rows = 0) {
  WideWgradPlan p;
  CHK(wide_wgrad_plan(m, st, ld, x, segs, seg_kpad, n_seg, dpre, d_stride, zero_row0, zero_rows, roles != nullptr, roles && roles->adam, &p));
  if (roles) {              // collected for the merged launch (wide_wgrad_flush)
    if ((int)roles->v.size() >= WWM_ROLES) FAIL(m, V2X_ESTATE, "wide wgrad: too many roles for one launch");
    roles->v.push_back(p);
    return V2X_OK;
  }
  const WideWgradArgs& a = p.a;
  const dim3 grid(p.kt, p.nt, x.grid_y * p.sp);
  if (p.ntw == 4) { auto k = k_wide_wgrad<64, 4>; LAUNCH(m, name, k, grid, 256, 0, st, a); }
  else if (p.ntw == 5) { auto k = k_wide_wgrad<128, 5>; LAUNCH(m, name, k, grid, 256, 0, st, a); }
  else if (p.ntw == 8) { auto k = k_wide_wgrad<128, 8>; LAUNCH(m, name, k, grid, 256, 0, st, a); }
  else { auto k = k_wide_wgrad<128, 16>; LAUNCH(m, name, k, grid, 256, 0, st, a); }
  return V2X_OK;
}

// launch the collected roles as one grid, heaviest workgroups first (they are dispatched in block order and the launch is
// as long as its last-finishing workgroup)
int wide_wgrad_flush(v2x_model* m, hipStream_t st, const IdxMap& x, std::vector<WideWgradPlan>& roles) {
  if (roles.empty()) return V2X_OK;
  std::stable_sort(roles.begin(), roles.end(), [](const WideWgradPlan& p, const WideWgradPlan& q) {
    auto w = [](const WideWgradPlan& r) { return (r.ntw == 4 ? 64 : 128) * 16 * r.ntw; };     // MFMA work of one workgroup
    return w(p) > w(q);
  });
  WideWgradMulti mu;
  memset(&mu, 0, sizeof(mu));
  int n = 0, total = 0;
  for (const WideWgradPlan& p : roles) {
    mu.w[n] = p.a; mu.kt[n] = p.kt; mu.nt[n] = p.nt;
    mu.kind[n] = p.ntw == 16 ? WWM_128x16 : (p.ntw == 8 ? WWM_128x8 : (p.ntw == 5 ? WWM_128x5 : WWM_64x4));
    mu.start[n] = total;
    total += p.kt * p.nt * x.grid_y * p.sp;
    ++n;
  }
  for (int i = n; i <= WWM_ROLES; ++i) mu.start[i] = total;
  mu.n_roles = n;
  LAUNCH(m, "k_wgrad_wide_all", k_wide_wgrad_multi, dim3(total), 256, 0, st, mu);
  return V2X_OK;
}

void set_idx(GemmArgs& a, const IdxMap& x) {
  a.n_idx = x.n_idx; a.row_stride = x.row_stride; a.base_mul = x.base_mul; a.idx_base = x.idx_base;
}

template <int F, bool HAS0, bool HAS2, bool DGRAD>
int launch_gemm_t(v2x_model* m, hipStream_t st, GemmArgs& a, int grid_y, const char* name) {
  constexpr int FB = F / 16;
  constexpr int KB = DGRAD ? FB : ((HAS0 ? FB : 0) + 1 + (HAS2 ? FB : 0));
  constexpr int KP = DGRAD ? (2 * F + XE) : KB * 16;
  const size_t lds = (size_t)(KP * (F + 4) + F) * 4;
  const int gx = persistent_wgs_per_slot(a.n_idx, grid_y, m->knobs.gemm_wgs_per_cu);
  auto k = k_gemm_rows<F, HAS0, HAS2, DGRAD>;
  LAUNCH(m, name, k, dim3(gx, grid_y), 256, lds, st, a);
  return V2X_OK;
}

template <int F>
int launch_node_fwd_f(v2x_model* m, hipStream_t st, int stage, GemmArgs& a, int grid_y) {
  if (stage == 0) {
    if (a.seg2) return launch_gemm_t<F, false, true, false>(m, st, a, grid_y, "k_node_fwd_embed");
    return launch_gemm_t<F, false, false, false>(m, st, a, grid_y, "k_node_fwd_embed");
  }
  return launch_gemm_t<F, true, true, false>(m, st, a, grid_y, "k_node_fwd");
}

// GNNLayer forward of `stage`
int launch_node_fwd(v2x_model* m, hipStream_t st, int stage, const IdxMap& x, const float* xe, const float* h_prev,
                    const float* agg_prev, float* out) {
  const LayerDesc& ld = m->gnn[stage];
  GemmArgs a;
  a.seg0 = h_prev; a.seg0_stride = m->F; a.xe = xe; a.seg2 = agg_prev; a.seg2_stride = m->F;
  a.W = m->params + ld.off; a.slot_stride = ld.slot_stride; a.pad = ld.pad;
  a.out = out; a.out_stride = m->F; a.relu = stage < m->L ? 1 : 0;
  set_idx(a, x);
  if (stage > 0 && (!h_prev || !agg_prev)) FAIL(m, V2X_EINVAL, "node_update: stage>0 needs h_prev and agg_prev");
  if (is_wide(m)) {
    const int F = m->F;
    WideSeg s[3];
    int n = 0;
    if (stage > 0) { s[n++] = WideSeg{h_prev, F, F}; s[n++] = WideSeg{xe, XE, XE}; s[n++] = WideSeg{agg_prev, F, F}; }
    else { s[n++] = WideSeg{xe, XE, XE}; if (agg_prev) s[n++] = WideSeg{agg_prev, F, F}; }
    return wide_fwd(m, st, ld, x, s, n, out, F, a.relu, stage ? "k_node_fwd" : "k_node_fwd_embed");
  }
  switch (m->F) {
    case 16: return launch_node_fwd_f<16>(m, st, stage, a, x.grid_y);
    case 32: return launch_node_fwd_f<32>(m, st, stage, a, x.grid_y);
    case 64: return launch_node_fwd_f<64>(m, st, stage, a, x.grid_y);
  }
  FAIL(m, V2X_EINVAL, "unsupported feat_dim %d", m->F);
}

// data gradient of stage >= 1: gha[R][2F] = [dpre.W1h^T | dpre.W3^T]
int launch_dgrad(v2x_model* m, hipStream_t st, int stage, const IdxMap& x, const float* dpre, float* gha) {
  const LayerDesc& ld = m->gnn[stage];
  GemmArgs a;
  a.seg0 = dpre; a.seg0_stride = m->F; a.xe = nullptr; a.seg2 = nullptr; a.seg2_stride = 0;
  a.W = m->params + ld.off; a.slot_stride = ld.slot_stride; a.pad = ld.pad;
  a.out = gha; a.out_stride = 2 * m->F; a.relu = 0;
  set_idx(a, x);
  if (is_wide(m)) return wide_dgrad(m, st, ld, x, dpre, m->F, m->Dn + m->De, gha, "k_node_dgrad");
  switch (m->F) {
    case 16: return launch_gemm_t<16, true, false, true>(m, st, a, x.grid_y, "k_node_dgrad");
    case 32: return launch_gemm_t<32, true, false, true>(m, st, a, x.grid_y, "k_node_dgrad");
    case 64: return launch_gemm_t<64, true, false, true>(m, st, a, x.grid_y, "k_node_dgrad");
  }
  FAIL(m, V2X_EINVAL, "unsupported feat_dim %d", m->F);
}

// rows per slot of the slot-major MLP internals (z2, z3, dz2, dz3, dq, rowloss): the workspace capacity, so that the
// kernel that writes them and the weight-gradient launch that reads them agree whatever the batch size
int64_t srow_stride(const v2x_model* m) { return m->S == 1 ? 0 : m->cap_rows / m->N; }

void mlp_args(v2x_model* m, MlpArgs& a, const IdxMap& x, const float* xe, const float* h, const float* agg) {
  memset(&a, 0, sizeof(a));
  a.srow_stride = srow_stride(m);
  a.h = h; a.xe = xe; a.agg = agg;
  for (int i = 0; i < 4; ++i) { a.W[i] = m->params + m->dense[i].off; a.slot_stride[i] = m->dense[i].slot_stride; }
  a.C = m->C;
  a.z1 = m->z1; a.z2 = m->z2; a.z3 = m->z3; a.q = m->q;
  a.dq = m->dq; a.dz1 = m->dz1; a.dz2 = m->dz2; a.dz3 = m->dz3; a.gha = m->gha; a.rowloss = m->rowloss;
  a.n_idx = x.n_idx; a.row_stride = x.row_stride; a.base_mul = x.base_mul; a.idx_base = x.idx_base;
}

template <int F>
int launch_mlp_fwd_f(v2x_model* m, hipStream_t st, MlpArgs& a, int grid_y) {
  const size_t lds = (size_t)MlpLds<F>::TOTAL * 4;
  const int gx = persistent_wgs_per_slot(a.n_idx, grid_y, m->knobs.mlp_wgs_per_cu);
  auto k = k_mlp_fwd<F>;
  LAUNCH(m, "k_mlp_fwd", k, dim3(gx, grid_y), 256, lds, st, a);
  return V2X_OK;
}

// Training of a narrow model (F <= 64): forward + Huber + backward of the decision MLP and the four Dense weight gradients in
// ONE launch (k_mlp_train_wg, kernels_mlpwg.hpp): one workgroup per CU, each writes one partial-sum slab of the Dense layers.
// A wide model runs k_mlp_fwd<0> / k_mlp_bwd<0> around its wide GEMMs (launch_mlp) and wgrad_mlp.
bool mlp_wg_path(const v2x_model* m) { return !is_wide(m); }

// work split of k_mlp_train_wg (MlpWgArgs): one workgroup per CU, equal shares of the slot-major tile list
struct MlpWgSplit { int tiles_per_slot, slot_span, tiles_per_wg, n_wgs, n_slabs; };
MlpWgSplit mlp_wg_split(int n_idx, int n_slots) {
  MlpWgSplit s;
  const int T = (n_idx + 15) / 16, cus = n_cus();
  s.tiles_per_slot = T;
  auto up4 = [](int v) { return (v + 3) / 4 * 4; };          // whole rounds of the 4 waves
  // whole workgroups per slot (see MlpWgArgs for the packed alternative that was tried)
  int gx = std::max(1, std::min(cus / std::max(n_slots, 1), (T + 3) / 4));
  const int qa = up4((T + gx - 1) / gx);
  gx = (T + qa - 1) / qa;
  s.slot_span = gx * qa; s.tiles_per_wg = qa;
  s.n_wgs = gx * n_slots;
  s.n_slabs = gx;
  return s;
}

template <int F>
int launch_mlp_train_wg_f(v2x_model* m, hipStream_t st, const MlpArgs& a, int n_slots, bool wg0) {
  const size_t lds = (size_t)MlpWgLds<F>::TOTAL * 4;
  const MlpWgSplit sp = mlp_wg_split(a.n_idx, n_slots);
  if (sp.n_slabs > m->slab_cap) FAIL(m, V2X_ESTATE, "mlp_train_wg: slabs not pre-sized (%d > %d)", sp.n_slabs, m->slab_cap);
  MlpTrainWgArgs t;
  memset(&t, 0, sizeof(t));
  t.a = a;
  t.w.slab = m->slab; t.w.slab_stride = m->P;
  t.w.tiles_per_slot = sp.tiles_per_slot; t.w.slot_span = sp.slot_span; t.w.tiles_per_wg = sp.tiles_per_wg; t.w.n_slots = n_slots; t.w.n_slabs = sp.n_slabs;
  t.w.ts = m->ts_buf ? m->ts_buf + 2 * 8 * 64 : nullptr;
  for (int i = 0; i < 4; ++i) {
    LayerDesc& ld = m->dense[i];
    ld.n_slabs = sp.n_slabs;              // remembered for the slab reduction
    t.w.l[i] = MlpWgLayer{ld.off, ld.slot_stride, ld.n_out, ld.pad};
  }
  if constexpr (F == 64) {
    if (!wg0) {             // Dense-0's weight gradient is a role of the graph layers' launch (dense0_rides): dz1 rows instead
      if (a.frag_groups > 0) { auto k = k_mlp_train_wg<F, true, false>; LAUNCH(m, "k_mlp_train_wg123", k, dim3(sp.n_wgs), 256, lds, st, t); }
      else { auto k = k_mlp_train_wg<F, false, false>; LAUNCH(m, "k_mlp_train_wg123", k, dim3(sp.n_wgs), 256, lds, st, t); }
      return V2X_OK;
    }
  }
  if (!wg0) FAIL(m, V2X_ESTATE, "mlp_train_wg: Dense-0 outside the launch needs feat_dim 64");
  if (a.frag_groups > 0) { auto k = k_mlp_train_wg<F, true>; LAUNCH(m, "k_mlp_train_wg", k, dim3(sp.n_wgs), 256, lds, st, t); }
  else { auto k = k_mlp_train_wg<F>; LAUNCH(m, "k_mlp_train_wg", k, dim3(sp.n_wgs), 256, lds, st, t); }
  return V2X_OK;
}

int launch_mlp_train_wg(v2x_model* m, hipStream_t st, const MlpArgs& a, bool wg0 = true) {
  const int gy = m->S == 1 ? 1 : m->N;
  switch (m->F) {
    case 16: return launch_mlp_train_wg_f<16>(m, st, a, gy, wg0);
    case 32: return launch_mlp_train_wg_f<32>(m, st, a, gy, wg0);
    case 64: return launch_mlp_train_wg_f<64>(m, st, a, gy, wg0);
  }
  FAIL(m, V2X_EINVAL, "unsupported feat_dim %d", m->F);
}

int launch_mlp(v2x_model* m, hipStream_t st, MlpArgs& a, bool bwd) {
  const int gy = m->S == 1 ? 1 : m->N;
  if (is_wide(m)) {
    // Dense-0 and its data gradient are wide GEMMs; Dense 1..3 (+ Huber) stay register-chained ("tail" form)
    IdxMap x;
    x.idx_base = a.idx_base; x.n_idx = a.n_idx; x.row_stride = a.row_stride; x.base_mul = a.base_mul; x.grid_y = gy;
    const int F = m->F;
    if (!bwd) {
      WideSeg s[3] = {WideSeg{a.h, F, F}, WideSeg{a.xe, XE, XE}, WideSeg{a.agg, F, F}};
      CHK(wide_fwd(m, st, m->dense[0], x, s, 3, m->z1, H1, 1, "k_dense0_fwd"));
      return launch_mlp_fwd_f<0>(m, st, a, gy);
    }
    const int gx = persistent_wgs_per_slot(a.n_idx, gy, m->knobs.mlp_wgs_per_cu);
    auto k = k_mlp_bwd<0>;
    LAUNCH(m, "k_mlp_bwd", k, dim3(gx, gy), 256, (size_t)MlpLds<0>::TOTAL * 4, st, a);
    return wide_dgrad(m, st, m->dense[0], x, m->dz1, H1, m->Dn, m->gha, "k_dense0_dgrad");
  }
  if (bwd) FAIL(m, V2X_ESTATE, "mlp: the backward of a narrow model is part of k_mlp_train_wg");
  switch (m->F) {
    case 16: return launch_mlp_fwd_f<16>(m, st, a, gy);
    case 32: return launch_mlp_fwd_f<32>(m, st, a, gy);
    case 64: return launch_mlp_fwd_f<64>(m, st, a, gy);
  }
  FAIL(m, V2X_EINVAL, "unsupported feat_dim %d", m->F);
}

// weight gradients: build the role description of one layer ...
int layer_work(const LayerDesc& ld) { return (ld.kp / 16) * (ld.np / 16); }

int wgrad_role(v2x_model* m, LayerDesc& ld, int kind, const IdxMap& x, int total_work, const WgSeg* segs, int n_seg,
               const float* dpre, int d_stride, WgradArgs& a, int rows_override = 0) {
  int chunk;
  const bool gnn_kind = kind < WG_KIND_DENSE0 || kind >= WG_KIND_EMBED_NONBR;
  // measured at batch 4096 x 20 nodes in the merged launch: the SAME 1024 rows per workgroup for every role (87 us) beats
  // 1024 / 768 for the GNN / Dense families (102 us, the optimum when the two families were separate launches)
  // (the graph layers on their own -- the Dense gradients come out of k_mlp_train_wg -- : 896, i.e. 5 x 832 rows per
  //  slot at batch 4096: 46.8 us against 53.1 at 1024, 48.7 at 768, 49.4 at 704, 57.2 at 640)
  const Knobs& kn = m->knobs;
  const int rows_dense = kn.wg_chunk_dense, rows_embed = kn.wg_chunk_embed;       // (the light embed role may have its own chunking)
  int rows_g = kn.wg_chunk_gnn > 0 ? kn.wg_chunk_gnn : (is_wide(m) ? 1024 : 896);
  if (rows_embed > 0 && (kind == WG_KIND_EMBED || kind == WG_KIND_EMBED_NONBR)) rows_g = rows_embed;
  if (rows_override > 0) rows_g = rows_override;
  const int nc = role_chunks(kn, x.n_idx, x.grid_y, layer_work(ld), total_work, &chunk, (gnn_kind || rows_override > 0) ? rows_g : rows_dense);
  if (nc > m->slab_cap) FAIL(m, V2X_ESTATE, "wgrad: slabs not pre-sized (%d > %d)", nc, m->slab_cap);
  ld.n_slabs = nc;                       // remembered for the slab reduction
  memset(&a, 0, sizeof(a));
  for (int i = 0; i < n_seg; ++i) a.seg[i] = segs[i];
  a.n_seg = n_seg;
  a.dpre = dpre; a.d_stride = d_stride; a.n_real = ld.n_out;
  a.kp = ld.kp; a.np = ld.np; a.pad = ld.pad;
  a.slab = m->slab; a.slab_stride = m->P; a.layer_off = ld.off; a.slot_stride = ld.slot_stride;
  a.n_idx = x.n_idx; a.row_stride = x.row_stride; a.base_mul = x.base_mul; a.chunk = chunk;
  a.idx_base = x.idx_base; a.chunk_base = 0; a.n_chunks = nc; a.kind = kind;
  a.dpre_slot_major = (kind >= WG_KIND_DENSE1 && kind <= WG_KIND_DENSE3) ? 1 : 0;      // dz2, dz3, dq (MlpArgs::srow_stride)
  a.srow_stride = (int)srow_stride(m);
  a.zeros = m->zero_buf;
  a.ts = (m->ts_buf && (kind == WG_KIND_GNN || kind >= WG_KIND_GNN_E1)) ? m->ts_buf + 3 * 8 * 64 : nullptr;
  return V2X_OK;
}

// ... and launch up to WG_MAX_ROLES of them as one grid (blockIdx.z = role)
int launch_wgrad_multi(v2x_model* m, hipStream_t st, const IdxMap& x, WgradMulti& mu, int n_roles, const char* name) {
  int maxt = 1, nc = 1;
  for (int i = 0; i < n_roles; ++i) {
    maxt = std::max(maxt, (mu.w[i].kp / 16) * (mu.w[i].np / 16) + (mu.w[i].kind >= WG_KIND_GNN_E1 ? 4 : 0));
    nc = std::max(nc, mu.w[i].n_chunks);
  }
  for (int i = 0; i < n_roles; ++i)     // phase stamps (Knobs::fused_ts): of ONE role, Knobs::wg_ts_role (default: the first)
    if (i != m->knobs.wg_ts_role) mu.w[i].ts = nullptr;
  const size_t lds = (size_t)(2 * maxt * 64 * 4 + 4 * 9 * 16) * 4;      // accumulator exchange (two sets) + bias (per wave)
  dim3 grid(nc, x.grid_y, n_roles);
  {                                     // unequal chunk counts: a packed 1-D grid of the real workgroups (kernels.hpp WgradMulti)
    bool uneven = false;
    for (int i = 0; i < n_roles; ++i) uneven = uneven || mu.w[i].n_chunks != nc;
    mu.packed = uneven ? 1 : 0;
    int at = 0;
    for (int i = 0; i <= WG_MAX_ROLES; ++i) {
      mu.wg_begin[i] = at;
      if (i < n_roles) at += mu.w[i].n_chunks * x.grid_y;
    }
    if (uneven) grid = dim3(at, 1, 1);
  }
  // a narrow model's launch holds graph-layer roles (+ the Dense-0 halves); a wide model's only Dense 1..3
  bool dense = false, halves = false;
  for (int i = 0; i < n_roles; ++i) {
    if (mu.w[i].kind >= WG_KIND_DENSE0A) halves = true;
    else if (mu.w[i].kind >= WG_KIND_DENSE0 && mu.w[i].kind <= WG_KIND_DENSE3) dense = true;
  }
#define V2X_WG_CASE(FF)                                                              \
  if (m->F == FF && !dense) {                                                        \
    if (halves) { auto k = k_wgrad<FF, 3>; LAUNCH(m, name, k, grid, 256, lds, st, mu); }    \
    else { auto k = k_wgrad<FF, 0>; LAUNCH(m, name, k, grid, 256, lds, st, mu); }           \
    return V2X_OK;                                                                   \
  }
  V2X_WG_CASE(16) V2X_WG_CASE(32) V2X_WG_CASE(64)
#undef V2X_WG_CASE
  if (is_wide(m) && dense && !halves) { // (the operand widths of Dense 1..3 do not depend on F)
    auto k = k_wgrad<64, 1>;
    LAUNCH(m, name, k, grid, 256, lds, st, mu);
    return V2X_OK;
  }
  FAIL(m, V2X_EINVAL, "wgrad: no kernel for these roles at feat_dim %d", m->F);
}

int wgrad_gnn_role(v2x_model* m, int stage, const IdxMap& x, int total_work, const float* xe, const float* h_prev,
                   const float* agg_prev, const float* dpre, WgradArgs& a, int embed_tiles = 0, int rows_override = 0) {
  const int F = m->F;
  WgSeg s[3];
  int n = 0;
  if (stage > 0) { s[n++] = WgSeg{h_prev, F, F, 0, 0}; s[n++] = WgSeg{xe, XE, XE, F, 0}; s[n++] = WgSeg{agg_prev, F, F, F + XE, 0}; }
  else { s[n++] = WgSeg{xe, XE, XE, 0, 0}; s[n++] = WgSeg{agg_prev /* neighbour-init or null */, F, F, XE, 0}; }
  int kind = stage ? WG_KIND_GNN : (agg_prev ? WG_KIND_EMBED : WG_KIND_EMBED_NONBR);
  if (stage && embed_tiles) kind = embed_tiles == 1 ? WG_KIND_GNN_E1 : (embed_tiles == 2 ? WG_KIND_GNN_E2 : WG_KIND_GNN_E4);
  CHK(wgrad_role(m, m->gnn[stage], kind, x, total_work, s, n, dpre, F, a, rows_override));
  if (stage && embed_tiles) {            // + the embed layer's columns [(stage - 1) * 16 * embed_tiles, ...): kernels.hpp, wgrad_body EN
    const LayerDesc& e = m->gnn[0];
    a.e_dpre = m->dpre[0]; a.e_stride = F; a.e_col0 = (stage - 1) * 16 * embed_tiles; a.e_n_real = e.n_out;
    a.e_layer_off = e.off; a.e_slot_stride = e.slot_stride; a.e_pad = e.pad;
  }
  return V2X_OK;
}

int wide_wgrad_gnn(v2x_model* m, hipStream_t st, int stage, const IdxMap& x, const float* xe, const float* h_prev,
                   const float* agg_prev, const float* dpre, WideRoles* roles = nullptr) {
  const int F = m->F;
  WideSeg s[3];
  int kp[3], n = 0;
  if (stage > 0) {
    s[n] = WideSeg{h_prev, F, F}; kp[n++] = 0;
    s[n] = WideSeg{xe, XE, XE}; kp[n++] = F;
    s[n] = WideSeg{agg_prev, F, F}; kp[n++] = F + XE;
  } else {
    s[n] = WideSeg{xe, XE, XE}; kp[n++] = 0;
    if (agg_prev) { s[n] = WideSeg{agg_prev, F, F}; kp[n++] = XE; }
    // neighbour-init absent (the reference always feeds zeros): its F weight rows (real rows Dn+De ..) are memset
    else return wide_wgrad(m, st, m->gnn[0], x, s, kp, n, dpre, F, "k_wgrad_embed", roles, m->Dn + m->De, F);
  }
  return wide_wgrad(m, st, m->gnn[stage], x, s, kp, n, dpre, F, stage ? "k_wgrad_gnn" : "k_wgrad_embed", roles);
}

// rows per workgroup of the graph layers' roles when the embed gradient rides on them: one workgroup per CU if that
// leaves >= 64 rows each (one 16-row block per wave), else the default chunking (0).  (Until round 3 the bound was 256
// rows: a 512- or 1024-graph share of a fixed global batch -- 8 / 4 GPUs -- then fell back to 896-row chunks, i.e. 40 / 80
// workgroups walking 8 blocks per wave: 33.8 / 34.1 us per launch against 19.2 / 20.6 us with 128- / 192-row chunks.)
// extra_roles: roles of about a graph layer's weight that ride in the same grid (Dense-0 at small batches, dense0_rides)
int merged_wg_rows(const v2x_model* m, int n_idx, int n_slots, int extra_roles = 0) {
  if (m->knobs.wg_chunk_merged > 0) return m->knobs.wg_chunk_merged;
  const int nc_fit = n_cus() / std::max(1, (m->L + extra_roles) * n_slots);
  const int min_rows = m->knobs.wg_merged_min_rows;
  if (nc_fit >= 1 && n_idx / nc_fit >= min_rows) return ((n_idx + nc_fit - 1) / nc_fit + 63) / 64 * 64;
  return 0;
}

// one GNN stage on its own (per-kernel entry point)
int wgrad_gnn(v2x_model* m, hipStream_t st, int stage, const IdxMap& x, const float* xe, const float* h_prev,
              const float* agg_prev, const float* dpre) {
  if (is_wide(m)) return wide_wgrad_gnn(m, st, stage, x, xe, h_prev, agg_prev, dpre);
  WgradMulti mu;
  memset(&mu, 0, sizeof(mu));
  CHK(wgrad_gnn_role(m, stage, x, layer_work(m->gnn[stage]), xe, h_prev, agg_prev, dpre, mu.w[0]));
  return launch_wgrad_multi(m, st, x, mu, 1, stage ? "k_wgrad_gnn" : "k_wgrad_embed");
}

// What one backward pass was asked for by its C-ABI call: arguments handed down, nothing here outlives the call
struct BwdCall {
  bool bucketed = false;               // data parallelism wants each layer's gradient as soon as it is final: no merged wide launch
  bool fuse_adam = false;              // the merged wide launch applies Adam in its epilogues (BatchPlan::wide_adam_fusable)
  const float* tq = nullptr;           // a DQN replay step whose MLP launch forms the targets itself (MlpArgs::tq): replaced entries, actions
  float* y_out = nullptr;              // ... and where y goes
  bool phased = false;                 // one half of v2x_forward_backward_phase, not run_backward: see dense0_out and ragged_fused_bwd
};
// wide path: every layer's weight gradient in ONE launch after the data chain -- unless somebody wants a layer's gradient
// as soon as it is final (per-layer all-reduce buckets of data parallelism)
bool wide_merged(const BatchPlan& p, const BwdCall& c) { return p.wide_merge && !c.bucketed; }
// The MLP launch leaves dz1 instead of Dense-0's weight gradient, which is then a role of wgrad_gnn_all: backward_mlp and
// wgrad_gnn_all both ask here, so the two cannot disagree.
// (phased: the phases always keep it in the MLP launch, although phase 0's forward consults dense0_rides for the hand-off layout)
bool dense0_out(const BatchPlan& p, const BwdCall& c) { return p.dense0_rides && !c.phased; }
// A ragged batch takes its one-launch backward.  (phased: phase 1 runs a ragged batch's data chain layer by layer)
bool ragged_fused_bwd(const BatchPlan& p, const BwdCall& c) { return p.ragged_bwd && !c.phased; }

// all GNN stages (needs dpre[0..L]): one launch when the embed rides on the stage roles (embed_rides), else
// ceil((L+1)/WG_MAX_ROLES) launches of at most WG_MAX_ROLES stage roles -- one up to L = 7, two at L = 8
int wgrad_gnn_all(v2x_model* m, hipStream_t st, const DevBatch& d, const BatchPlan& p, const BwdCall& c) {
  const IdxMap& x = p.x;
  if (is_wide(m)) {
    WideRoles merged;                                                   // collect: L + 1 graph layers (+ Dense-0), one grid
    merged.adam = c.fuse_adam;
    WideRoles* roles = wide_merged(p, c) ? &merged : nullptr;
    for (int s = m->L; s >= 0; --s)
      CHK(wide_wgrad_gnn(m, st, s, x, d.xe, s ? m->h[s - 1] : nullptr, s ? m->a[s - 1] : d.nbr, m->dpre[s], roles));
    if (!roles) return V2X_OK;
    const int F = m->F, L = m->L;
    WideSeg w0[3] = {WideSeg{m->h[L], F, F}, WideSeg{d.xe, XE, XE}, WideSeg{m->a[L], F, F}};
    const int kp[3] = {0, F, F + XE};
    CHK(wide_wgrad(m, st, m->dense[0], x, w0, kp, 3, m->dz1, H1, "k_wgrad_dense0", roles));
    return wide_wgrad_flush(m, st, x, merged.v);
  }
  WgradMulti mu;
  // The embed layer's gradient (16 MFMAs per block, load-bound) rides on the graph layers' roles when its F / 16 output
  // tiles divide evenly over the L stages: no workgroups of its own, and the heavy roles get one workgroup per CU --
  // n_cus / (L * slots) chunks per slot (batch 4096 x 20 slots x 2 stages: 6 chunks = 240 workgroups x 11 blocks per wave
  // instead of 5 chunks = 200 x 13 with 100 embed workgroups queueing behind them).
  const int NTf = m->F / 16;
  if (p.embed_rides) {
    const int en = NTf / m->L;
    const bool d0 = dense0_out(p, c);                            // + Dense-0 (k_mlp_train_wg left dz1 instead of dW0)
    const int rows = merged_wg_rows(m, x.n_idx, x.grid_y, d0 ? 1 : 0);
    memset(&mu, 0, sizeof(mu));
    int total = 0, n = 0;
    for (int t = m->L; t >= 1; --t) total += layer_work(m->gnn[t]);
    for (int s = m->L; s >= 1; --s)
      CHK(wgrad_gnn_role(m, s, x, total, d.xe, m->h[s - 1], m->a[s - 1], m->dpre[s], mu.w[n++], en, rows));
    if (d0) {
      // Dense-0 in two halves along K, [h | x] (25 accumulator tiles) and [agg] (20): lighter than a graph layer's role (36 + the
      // embed's; those go first: workgroups are dispatched in role order), so they take HALF as many row chunks -- at the 512- and 1024-graph shares 4 chunks per graph-layer role and 2
      // per half is 240 workgroups, one per CU
      const int F = m->F, L = m->L;
      const int groups = m->frag_live ? d.B / FZ_TG : 0;
      int chunk_g;
      const int nc_g = role_chunks(m->knobs, x.n_idx, x.grid_y, 1, 1, &chunk_g, rows > 0 ? rows : 896);
      const int rows_d = (((x.n_idx + std::max(1, nc_g / 2) - 1) / std::max(1, nc_g / 2)) + 63) / 64 * 64;
      WgSeg sa[2] = {WgSeg{m->h[L], F, F, 0, 0}, WgSeg{d.xe, XE, XE, F, 0}};
      CHK(wgrad_role(m, m->dense[0], groups ? WG_KIND_DENSE0A_F : WG_KIND_DENSE0A, x, total, sa, 2, m->dz1, H1, mu.w[n], rows_d));
      mu.w[n].frag_groups = groups; mu.w[n].kp = F + XE;
      ++n;
      WgSeg sb[1] = {WgSeg{m->a[L], F, F, 0, 0}};
      CHK(wgrad_role(m, m->dense[0], groups ? WG_KIND_DENSE0B_F : WG_KIND_DENSE0B, x, total, sb, 1, m->dz1, H1, mu.w[n], rows_d));
      mu.w[n].frag_groups = groups; mu.w[n].kp = F; mu.w[n].k_off = F + XE; mu.w[n].no_bias = 1;
      ++n;
    }
    m->gnn[0].n_slabs = m->gnn[1].n_slabs;                     // every stage role writes its columns of every embed slab
    return launch_wgrad_multi(m, st, x, mu, n, d0 ? "k_wgrad_gnn_d0" : "k_wgrad_gnn");
  }
  if (dense0_out(p, c)) FAIL(m, V2X_ESTATE, "wgrad: Dense-0 was left to a launch that cannot take it");
  int n = 0, s_first = m->L;
  for (int s = m->L; s >= 0; --s) {
    if (n == 0) { memset(&mu, 0, sizeof(mu)); s_first = s; }
    int total = 0;                                    // work of the stages sharing this launch
    for (int t = s_first; t >= 0 && t > s_first - WG_MAX_ROLES; --t) total += layer_work(m->gnn[t]);
    CHK(wgrad_gnn_role(m, s, x, total, d.xe, s ? m->h[s - 1] : nullptr, s ? m->a[s - 1] : d.nbr, m->dpre[s], mu.w[n]));
    if (++n == WG_MAX_ROLES || s == 0) { CHK(launch_wgrad_multi(m, st, x, mu, n, "k_wgrad_gnn")); n = 0; }
  }
  return V2X_OK;
}

// the Dense layers of a wide model: Dense-0 as a wide weight gradient (or a role of the merged launch), Dense 1..3 in one k_wgrad
// launch.  (A narrow model's Dense gradients come out of k_mlp_train_wg, Dense-0's at small batches out of wgrad_gnn_all.)
int wgrad_mlp(v2x_model* m, hipStream_t st, const IdxMap& x, const float* xe, const float* h, const float* agg, bool dense0_merged = false) {
  if (!is_wide(m)) FAIL(m, V2X_ESTATE, "wgrad_mlp: a narrow model's Dense gradients are part of k_mlp_train_wg");
  const int F = m->F;
  int total = 0;
  for (int i = 0; i < 4; ++i) total += layer_work(m->dense[i]);
  WgradMulti mu;
  memset(&mu, 0, sizeof(mu));
  WideSeg w0[3] = {WideSeg{h, F, F}, WideSeg{xe, XE, XE}, WideSeg{agg, F, F}};
  const int kp[3] = {0, F, F + XE};
  if (!dense0_merged) CHK(wide_wgrad(m, st, m->dense[0], x, w0, kp, 3, m->dz1, H1, "k_wgrad_dense0", nullptr));   // else: a role of the merged launch
  WgSeg t1[1] = {WgSeg{m->z1, H1, H1, 0, 0}};
  CHK(wgrad_role(m, m->dense[1], WG_KIND_DENSE1, x, total, t1, 1, m->dz2, H2, mu.w[0]));
  WgSeg t2[1] = {WgSeg{m->z2, H2, H2, 0, 1}};
  CHK(wgrad_role(m, m->dense[2], WG_KIND_DENSE2, x, total, t2, 1, m->dz3, H3, mu.w[1]));
  WgSeg t3[1] = {WgSeg{m->z3, H3, H3, 0, 1}};
  CHK(wgrad_role(m, m->dense[3], WG_KIND_DENSE3, x, total, t3, 1, m->dq, m->C, mu.w[2]));
  return launch_wgrad_multi(m, st, x, mu, 3, "k_wgrad_dense");
}

struct LossJob { int n_out, n_idx, stride; float scale; int64_t slot_stride; };   // n_out == 0: no loss role;
                                                                                 // rowloss(slot, i) = slot*slot_stride + i*stride

// bucket: -1 = the whole flat buffer, 0 = the Dense layers (its tail), 1 = the graph layers (its head)
int64_t bucket_begin(const v2x_model* m, int bucket) { return bucket == 0 ? m->dense[0].off : 0; }
int64_t bucket_end(const v2x_model* m, int bucket) { return bucket == 1 ? m->dense[0].off : m->P; }

// Gradient buckets of the phased forward+backward (data parallelism, v2x_forward_backward_phase), in the order in which they
// become final.  Narrow features (graph-major fused kernels: the graph layers finish together): [Dense layers], [graph
// layers].  Wide features (layer-wise kernels, one weight-gradient launch per layer): [Dense layers], [stage L], ...,
// [stage 1], [embed] -- L + 2 buckets, the all-reduce of each overlappable with the rest of the backward pass.
int n_phase_buckets(const v2x_model* m) { return m->F >= 128 ? m->L + 2 : 2; }
void phase_bucket_range(const v2x_model* m, int bucket, int64_t* b, int64_t* e) {
  if (m->F < 128) { *b = bucket_begin(m, bucket); *e = bucket_end(m, bucket); return; }
  if (bucket == 0) { *b = m->dense[0].off; *e = m->P; return; }
  const LayerDesc& ld = m->gnn[m->L + 1 - bucket];
  *b = ld.off; *e = ld.off + ld.slot_stride * m->S;
}

float adam_lr_t(const v2x_model* m, int64_t iteration) {
  const double t = (double)iteration;
  return (float)(m->cfg.lr * std::sqrt(1.0 - std::pow((double)m->cfg.beta2, t)) / (1.0 - std::pow((double)m->cfg.beta1, t)));
}

// fused_adam: the layers gnn[1..L] and dense[0] were updated by their weight-gradient launch (WideWgradArgs::adam): this
// launch covers what is left of the flat buffer, [0, gnn[1].off) and [dense[1].off, P)
int launch_reduce_adam(v2x_model* m, hipStream_t st, int n_slabs, bool do_adam, float* grad_dst, LossJob lj = LossJob{0, 0, 0, 0.f, 0},
                       int bucket = -1, bool fused_adam = false, int64_t range_begin = -1, int64_t range_end = -1,
                       bool advance_iteration = true) {
  AdamArgs a;
  memset(&a, 0, sizeof(a));
  a.param = m->params; a.grad = grad_dst ? grad_dst : m->grads; a.mom = m->mom; a.vel = m->vel;
  if (n_slabs > 0) {
    a.n_slabs = n_slabs; a.slab = m->slab; a.slab_stride = m->P;
    int nl = 0;
    for (auto* v : {&m->gnn, &m->dense})
      for (const LayerDesc& ld : *v) {
        a.layer_end4[nl] = (ld.off + ld.slot_stride * m->S) / 4;
        a.layer_slabs[nl] = ld.n_slabs;
        ++nl;
      }
    a.n_layers = nl;
  }
  a.n4 = m->P / 4;
  a.range_begin4 = bucket_begin(m, bucket) / 4; a.range_end4 = bucket_end(m, bucket) / 4;
  if (range_begin >= 0) { a.range_begin4 = range_begin / 4; a.range_end4 = range_end / 4; }
  if (fused_adam) {
    a.range_begin4 = 0; a.range_end4 = m->gnn[1].off / 4;
    a.range2_begin4 = m->dense[1].off / 4; a.range2_end4 = m->P / 4;
  }
  a.do_adam = do_adam ? 1 : 0;
  if (do_adam) {
    if (advance_iteration) m->iterations += 1;
    a.lr_t = adam_lr_t(m, m->iterations);
    a.beta1 = m->cfg.beta1; a.beta2 = m->cfg.beta2; a.eps = m->cfg.eps;
    if (m->pk_fwd) { a.pack.fwd = m->pk_fwd; a.pack.bwd = m->pk_bwd; a.pack.F = m->F; a.pack.S = m->S; a.pack.L = m->L; a.pack.xr = m->Dn + m->De; }
  }
  int max_slabs_used = 0;
  for (int l = 0; l < a.n_layers; ++l) max_slabs_used = std::max(max_slabs_used, a.layer_slabs[l]);
  a.groups = 1;
  if (a.slab && a.n4 < 256 * 1024 && max_slabs_used >= 16) a.groups = a.n4 < 64 * 1024 ? 16 : 4;
  m->reduce_groups = a.groups;
  const int cols = 256 / a.groups;
  int blocks = (int)((a.range_end4 - a.range_begin4 + a.range2_end4 - a.range2_begin4 + cols - 1) / cols);
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  a.n_adam_blocks = blocks;
  a.rowloss = m->rowloss; a.loss = m->loss_dev; a.loss_n_idx = lj.n_idx; a.loss_stride = lj.stride; a.loss_scale = lj.scale; a.loss_slot_stride = lj.slot_stride;
  a.grad_direct = m->grads;
  a.loss_split = (lj.n_out == 1 && lj.n_idx > 16384) ? 64 : 1;
  a.loss_part = m->loss_part; a.loss_cnt = reinterpret_cast<unsigned*>(m->loss_part + 64);
  LAUNCH(m, do_adam ? (n_slabs > 0 ? "k_reduce_adam" : "k_adam") : "k_grad_reduce", k_reduce_adam,
         dim3(blocks + lj.n_out * a.loss_split), 256, 0, st, a);
  return V2X_OK;
}

LossJob loss_job(const v2x_model* m, const DevBatch& d, int n_global) {
  const float inv = 1.0f / (float)((double)n_global * m->C);
  if (m->cfg.variable_graphs) return LossJob{1, d.R, 1, inv, 0};
  if (m->S == 1) return LossJob{m->N, d.B, m->N, inv, 1};          // shared weights: rowloss in node-row order
  return LossJob{m->N, d.B, 1, inv, srow_stride(m)};                // per-node weights: slot-major
}

__global__ void k_set4(float* dst, float a, float b, float c, float d) {
  if (threadIdx.x == 0) { dst[0] = a; dst[1] = b; dst[2] = c; dst[3] = d; }
}
int launch_check(v2x_model* m, const char* kname) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) FAIL(m, V2X_EHIP, "launch %s failed: %s", kname, hipGetErrorString(e));
  return V2X_OK;
}

// The launch counters of a (re)allocated or re-armed exchange start at a value no counter of this process has had: tags must
// never repeat at an address, also not across buffers (a freed buffer's address is handed out again) or across a re-arm.
unsigned long long g_xchg_epoch_next = 1;
std::mutex g_xchg_epoch_mutex;                       // (models may be created from several host threads)
int arm_xchg(v2x_model* m, int tiles, unsigned long long floor) {
  unsigned long long base;
  {
    std::lock_guard<std::mutex> lock(g_xchg_epoch_mutex);
    g_xchg_epoch_next = std::max(g_xchg_epoch_next, floor);
    base = g_xchg_epoch_next;
    g_xchg_epoch_next += 1ull << 16;
  }
  std::vector<unsigned long long> init((size_t)tiles, base);
  HIPCHK(m, hipMemset(m->xchg_buf, 0, xchg_bytes(m, tiles)));                 // tag 0 = never written
  HIPCHK(m, hipMemcpy(m->xchg_sync, init.data(), (size_t)tiles * sizeof(unsigned long long), hipMemcpyHostToDevice));
  HIPCHK(m, hipDeviceSynchronize());
  return V2X_OK;
}
int xchg_max_count(v2x_model* m, unsigned long long* out) {
  *out = 0;
  if (!m->xchg_sync || m->xchg_cap_tiles <= 0) return V2X_OK;
  std::vector<unsigned long long> cur((size_t)m->xchg_cap_tiles);
  HIPCHK(m, hipMemcpy(cur.data(), m->xchg_sync, cur.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  for (unsigned long long v : cur) *out = std::max(*out, v);
  return V2X_OK;
}
int ensure_xchg(v2x_model* m, int tiles) {
  if (tiles <= m->xchg_cap_tiles) return V2X_OK;
  if (m->capturing) FAIL(m, V2X_ESTATE, "exchange buffer growth during graph capture");
  drop_graphs(m);
  HIPCHK(m, hipDeviceSynchronize());
  unsigned long long seen = 0;
  CHK(xchg_max_count(m, &seen));
  if (m->xchg_buf) HIPCHK(m, hipFree(m->xchg_buf));
  if (m->xchg_sync) HIPCHK(m, hipFree(m->xchg_sync));
  m->xchg_buf = nullptr; m->xchg_sync = nullptr; m->xchg_cap_tiles = 0;
  HIPCHK(m, hipMalloc(reinterpret_cast<void**>(&m->xchg_buf), xchg_bytes(m, tiles)));
  HIPCHK(m, hipMalloc(reinterpret_cast<void**>(&m->xchg_sync), (size_t)tiles * sizeof(unsigned long long)));
  CHK(arm_xchg(m, tiles, seen + 1));
  m->xchg_cap_tiles = tiles;
  return V2X_OK;
}
FzXchg xchg_args(const v2x_model* m, int K) { return FzXchg{m->xchg_buf, m->xchg_sync, m->xchg_cap_tiles, K}; }

int launch_pack(v2x_model* m, hipStream_t st) {
  PackArgs p;
  memset(&p, 0, sizeof(p));
  p.params = m->params; p.pk_fwd = m->pk_fwd; p.pk_bwd = m->pk_bwd; p.S = m->S;
  for (int s = 0; s <= m->L; ++s) { p.layer_off[s] = m->gnn[s].off; p.slot_stride[s] = m->gnn[s].slot_stride; p.pad[s] = m->gnn[s].pad; }
  const dim3 grid(4, m->S, m->L + 1);
  const int rc = with_const<16, 32, 64>(m->F, [&](auto Fc) -> int {
    LAUNCH(m, "k_pack_weights", k_pack_weights<decltype(Fc)::value>, grid, 256, 0, st, p);
    return V2X_OK;
  });
  if (rc == V2X_EINVAL) FAIL(m, V2X_EINVAL, "pack: unsupported feat_dim %d", m->F);
  return rc;
}

// ------------------------------------------------------------------------------------ the plan of a batch
// plan_batch decides every path of a batch once; the predicates below are its helpers and nothing else calls them.

// ---- fused graph layers
// (kernels_fused.hpp) fixed-size graphs of <= 32 nodes, narrow features, no neighbour-init input, tile fits the LDS
int fused_rowf(int F) { return 4 * ((F / 16) | 1); }
size_t fused_lds(const v2x_model* m, const DevBatch& d, bool bwd, bool compl_sums = false) {
  const size_t rows = (size_t)FZ_TG * m->N;
  size_t b = 4 * rows * fused_rowf(m->F) * 4 + (rows + 1) * 4 + (size_t)FZ_TG * d.max_edges;
  b += rows * 4;                                       // bit masks: backward always, forward with compl_sums
  if (compl_sums) b += (size_t)(FZ_SUMS_ROWS + FZ_TOT_ROWS) * fused_rowf(m->F) * 4;
  return (b + 15) / 16 * 16 + 64;                      // + the turn flags of the backward (FzCtxB::sFlag)
}
bool fused_path(const v2x_model* m, const DevBatch& d) {
  if (!m->pk_fwd || m->cfg.variable_graphs || d.goff || d.nbr || m->F > 64 || m->N > 32 || m->L > FZ_MAXL) return false;
  if (d.max_nodes != m->N) return false;
  return fused_lds(m, d, true) <= 160 * 1024;
}
// Aggregations through the complement (kernels_fused.hpp, compl_sums): dense graphs whose extra LDS fits
bool fused_compl(const v2x_model* m, const DevBatch& d) {
  if (!m->knobs.fused_compl || m->N < 4) return false;
  if (2 * (int64_t)d.E <= (int64_t)d.B * m->N * (m->N - 1)) return false;      // average in-degree <= (N - 1) / 2
  return fused_lds(m, d, true, true) <= 160 * 1024;
}
// Split tiles (kernels_fused_split.hpp): K workgroups per 16-graph tile when whole-tile workgroups would leave most of the
// chip idle (the shares of the metric's global batch).  All K x tiles workgroups must be co-resident (one per CU: their LDS
// tile admits no second one), and a member should keep at least four slots (below that the hand-overs cost more than the
// node updates they spread).  Edge form only.  (Of a batch on the fused path.)
int fused_split(const v2x_model* m, const DevBatch& d) {
  const int split_env = m->knobs.fused_split;                        // -1 auto, 0 / 1 off, K forced
  if (split_env == 0 || split_env == 1 || m->L < 1 || m->L > 3) return 1;
  if (fused_lds(m, d, true) + (size_t)m->N * m->F * 4 > 160 * 1024) return 1;      // + the embed biases of all slots (forward)
  const int tiles = (d.B + FZ_TG - 1) / FZ_TG;
  auto fits = [&](int k) { return (m->N + k - 1) / k <= FZ_WAVES && tiles * k <= n_cus(); };      // one slot per wave, all co-resident
  if (split_env > 1) return (2 * split_env <= m->N && fits(split_env)) ? split_env : 1;
  for (int k : {5, 4, 3, 2})
    if (4 * k <= m->N && fits(k)) return k;
  return 1;
}

// ---- few-graph predict, one launch (kernels_small.hpp)
constexpr int SMALL_ROWS = 256;             // node rows (= workgroups) of one launch: all co-resident on any gfx950 part
bool small_path(const v2x_model* m, const DevBatch& d) {
  if (!m->knobs.small_predict || !m->small_h || m->cfg.variable_graphs || d.goff || d.nbr || m->F > 64 || m->L > FZ_MAXL) return false;
  if (m->N > 32) return false;                 // the kernel keeps a node's in-neighbours in a 32-entry LDS list
  return d.max_nodes == m->N && d.R <= std::min(SMALL_ROWS, n_cus());
}

// ---- ragged fused graph layers
// (kernels_ragged.hpp) variable-size graphs of <= 128 nodes, shared weights, narrow features, dense enough for the bit masks
bool ragged_fused_path(const v2x_model* m, const DevBatch& d) {
  // (any density: a row's aggregation walks its mask's one bits or -- rows with more edges than non-edges in graphs of >= 16
  //  nodes -- the zero bits; the masks are built for this path whether or not the dense MFMA aggregation wants them)
  return m->knobs.ragged_fused && m->cfg.variable_graphs && m->S == 1 && d.goff && !d.nbr && m->F <= 64 && m->L <= FZ_MAXL && d.max_nodes <= 128 &&
         d.max_nodes <= RG_CAP / 2;
}
// Small tiles (kernels_ragged_small.hpp: 160-row tiles, 4-wave workgroups, weights as fragments from L2, three workgroups per
// CU): built and measured in round 5 -- forward 123 us against 101, backward 161 against 103 at configs[4]'s share, + 19 us for
// the plan as a launch of its own (profiles/r05_ragged_small_ab.txt) -- so OFF unless Knobs::ragged_small (read at create:
// the fragment-major copy of a ragged model's weights is only kept then)
bool ragged_small(const v2x_model* m, const DevBatch& d) {
  return m->knobs.ragged_small && m->pk_fwd && m->pk_bwd && d.max_nodes <= 128 && m->L >= 1;
}

// ---- weight gradients that ride on the graph layers' launch, and the hand-off to the MLP launch
// The embed layer's gradient rides on the graph layers' roles (wgrad_gnn_all)
bool embed_rides(const v2x_model* m, const DevBatch& d) {
  const int merge_env = m->knobs.wg_embed_merge;
  const int NTf = m->F / 16;
  return merge_env && !is_wide(m) && !d.nbr && m->L >= 1 && m->L <= NTf && NTf % m->L == 0 && m->L + 3 <= WG_MAX_ROLES;
}
// Small batches (the shares of the metric's global batch on 4 / 8 GPUs): k_mlp_train_wg is ONE wave's latency chain there (<= 2
// tiles per wave) and the graph layers' weight-gradient launch leaves a third of the chip idle: Dense-0's weight gradient -- 180
// of a tile's 796 MFMAs, 45 of the 68 accumulator tiles the MLP launch exchanges and writes at its end -- moves over as a role
// of that launch (kernels_mlpwg.hpp WG0 = false, kernels.hpp WG_KIND_DENSE0_FRAG).  Knobs::mlp_wg0 = 1: never, 0: whenever possible.
bool dense0_rides(const v2x_model* m, const BatchPlan& p) {
  const int env = m->knobs.mlp_wg0;
  if (env == 1 || !p.mlp_wg || m->F != 64 || m->cfg.variable_graphs || !p.embed_rides) return false;
  if (p.x.n_idx % 16) return false;                              // whole 16-row groups (the fragment-major reader)
  if (env == 0) return true;
  // tiles per workgroup = 4 x tiles per wave.  Measured (profiles/r06_dense0_role_shares.txt): 512 / 1024 / 2048 graphs of 20 links
  // (4 / 8 / 12 tiles per workgroup) 0.1201 -> 0.1131, 0.1512 -> 0.1463, 0.1929 -> 0.1880 ms per step; at 4096 (20-24 tiles) the chip
  // is full either way and the heavier weight-gradient launch costs more than the MLP launch saves (0.2554 -> 0.2658)
  return mlp_wg_split(p.x.n_idx, p.x.grid_y).tiles_per_wg <= m->knobs.mlp_wg0_tiles;
}
// Fragment-major hand-off between the fused graph-layer kernels and k_mlp_train_wg (MlpArgs::frag_groups): whole batch in
// whole 16-graph groups, per-node weights (a tile of the MLP kernel is then a group of one node), at least one graph layer.
bool frag_layout(const v2x_model* m, const DevBatch& d, const BatchPlan& p) {
  // (Knobs::frag_with_dense0_role = 0: row-major hand-over where Dense-0's weight gradient is a role of k_wgrad -- measured slower: the
  //  fragment-major reader of that role costs nothing next to what the MLP launch and the fused kernels gain from 1 KiB accesses,
  //  0.1131 against 0.1157 ms at the 512-graph share)
  const int on = m->knobs.frag_handoff, frag_d0 = m->knobs.frag_with_dense0_role;
  return on && p.form == GraphLayers::Fused && p.mlp_wg && m->S == m->N && m->L >= 1 && d.B % FZ_TG == 0 && (frag_d0 || !p.dense0_rides);
}

BatchPlan plan_batch(const v2x_model* m, const DevBatch& d) {
  const Knobs& kn = m->knobs;
  BatchPlan p;
  p.x = idx_map(m, d);
  p.mlp_wg = mlp_wg_path(m);
  p.small_predict = small_path(m, d);
  p.form = fused_path(m, d) ? GraphLayers::Fused : (ragged_fused_path(m, d) ? GraphLayers::Ragged : GraphLayers::Layerwise);
  p.tiles = (d.B + FZ_TG - 1) / FZ_TG;
  if (p.form == GraphLayers::Fused) {
    p.split = fused_split(m, d);
    p.split_fwd = p.split > 1 && kn.fused_split_fwd;      // (debugging: one direction on whole tiles)
    p.split_bwd = p.split > 1 && kn.fused_split_bwd;
    // (a batch the split-tile kernels are picked for runs the edge form in BOTH directions, also when a debugging switch keeps one
    //  of them on whole tiles: the two kernels hand the rows' IN-neighbour sets over, the complement form would read them as
    //  non-neighbour sets)
    p.compl_sums = p.split <= 1 && fused_compl(m, d);
    p.fused_lds_fwd = p.split_fwd ? fused_lds(m, d, false, false) + (size_t)m->N * m->F * 4 : fused_lds(m, d, false, p.compl_sums);
    p.fused_lds_bwd = fused_lds(m, d, true, p.compl_sums);
  }
  if (p.form == GraphLayers::Ragged) {
    p.ragged_small = ragged_small(m, d);
    p.ragged_bwd = kn.ragged_fused_bwd;
    p.cap = p.ragged_small ? RGS_CAP : RG_CAP;
    p.capp = p.cap - d.max_nodes + 1;
    p.wgs = (d.R + p.capp - 1) / p.capp;
    // k_ragged_plan's tables in LDS; past that (tens of thousands of graphs in one batch) the interval plan of k_adj_masks
    p.plan_words = 3 * (d.B + 1) + p.wgs + 1;
    const bool packed = kn.ragged_packed && p.plan_words <= RG_PLAN_LDS_WORDS;
    // the packed plan by workgroup 0 of the mask launch while its offsets + 16-bit tables leave the mask workgroups their
    // eight per CU (<= 19 KB of LDS: ~2,200 graphs); a launch of its own (k_ragged_plan, 32-bit tables) beyond
    const bool folded = packed && kn.ragged_plan_fold && d.B < 65000 && plan16_bytes(d.B, p.wgs) <= 19 * 1024;
    p.plan_form = folded ? RaggedPlan::Folded : (packed ? RaggedPlan::Packed : RaggedPlan::Interval);
  }
  p.dense_agg = use_dense_agg(kn, d, m->F);
  p.need_adj_masks = p.dense_agg || p.form == GraphLayers::Ragged;
  p.embed_rides = embed_rides(m, d);
  p.dense0_rides = dense0_rides(m, p);
  p.frag_ok = frag_layout(m, d, p);
  p.wide_merge = is_wide(m) && kn.wide_merge && m->L + 2 <= WWM_ROLES;
  // Adam in the weight-gradient epilogues (single-GPU fit step of a wide model): needs the merged launch and ONE row split
  // for every layer it covers (gnn[1..L], dense[0]) -- true as soon as K tiles x slots fill the chip (per-node weights)
  const int kt = 2 * ((m->F + 127) / 128);                    // [h | agg] K tiles ([x | e] folded or one more: more tiles = fewer splits)
  p.wide_adam_fusable = kn.wide_adam && p.wide_merge && !m->prof_no_fuse && m->adam_scal && wide_splits(p.x.n_idx, kt, p.x.grid_y) == 1;
  return p;
}

// ------------------------------------------------------------------------------------ fused graph layers: the launches
struct FusedFwd { using Args = FusedFwdArgs; static constexpr bool bwd = false; static constexpr const char* name = "k_gnn_fwd_fused"; };
struct FusedBwd { using Args = FusedBwdArgs; static constexpr bool bwd = true; static constexpr const char* name = "k_gnn_bwd_fused"; };

// whole tiles: (F, slots per wave, time stamps, complement form)
template <typename D, int F, int SPW, bool TS, bool COMPL>
int launch_fused_tiles_k(v2x_model* m, hipStream_t st, dim3 grid, size_t lds, const typename D::Args& a) {
  if constexpr (D::bwd) LAUNCH(m, D::name, (k_gnn_bwd_fused<F, SPW, TS, COMPL>), grid, FZ_THREADS, lds, st, a);
  else LAUNCH(m, D::name, (k_gnn_fwd_fused<F, SPW, TS, COMPL>), grid, FZ_THREADS, lds, st, a);
  return V2X_OK;
}
// split tiles: (F, L, time stamps); recorded by the profiler under the whole-tile kernel's name
template <typename D, int F, int L, bool TS>
int launch_fused_split_k(v2x_model* m, hipStream_t st, dim3 grid, size_t lds, const typename D::Args& a, const FzXchg& xg) {
  if constexpr (D::bwd) LAUNCH(m, D::name, (k_gnn_bwd_split<F, L, TS>), grid, FZ_THREADS, lds, st, a, xg);
  else LAUNCH(m, D::name, (k_gnn_fwd_split<F, L, TS>), grid, FZ_THREADS, lds, st, a, xg);
  return V2X_OK;
}

// one direction of the fused graph layers, `a` filled in but for ts and compl_sums
template <typename D>
int launch_fused(v2x_model* m, hipStream_t st, const BatchPlan& p, typename D::Args& a) {
  const size_t lds = D::bwd ? p.fused_lds_bwd : p.fused_lds_fwd;
  if (D::bwd ? p.split_bwd : p.split_fwd) {                             // the shares of the global batch: K workgroups per tile
    CHK(ensure_xchg(m, p.tiles));
    const FzXchg xg = xchg_args(m, p.split);
    a.ts = m->ts_buf;
    const dim3 grid((p.tiles + 7) / 8 * 8 * p.split);
    const int rc = with_const<16, 32, 64>(m->F, [&](auto Fc) { return with_const<1, 2, 3>(m->L, [&](auto Lc) {
      constexpr int F = decltype(Fc)::value, L = decltype(Lc)::value;
      if constexpr (F == 64 && L == 2) {                                // (the time-stamp form exists for this shape only)
        if (m->ts_buf) return launch_fused_split_k<D, 64, 2, true>(m, st, grid, lds, a, xg);
      }
      return launch_fused_split_k<D, F, L, false>(m, st, grid, lds, a, xg);
    }); });
    if (rc == V2X_EINVAL) FAIL(m, V2X_EINVAL, "split fused %s: unsupported shape", D::bwd ? "backward" : "forward");
    return rc;
  }
  a.compl_sums = p.compl_sums ? 1 : 0;
  const dim3 grid(p.tiles);
  const int rc = with_const<16, 32, 64>(m->F, [&](auto Fc) { return with_const<1, 2, 3, 4>((m->N + FZ_WAVES - 1) / FZ_WAVES, [&](auto Sc) {
    constexpr int F = decltype(Fc)::value, SPW = decltype(Sc)::value;
    if constexpr (F == 64 && SPW == 3) {                                // (the time-stamp forms exist for this shape only)
      if (m->ts_buf) {
        a.ts = m->ts_buf;
        return p.compl_sums ? launch_fused_tiles_k<D, 64, 3, true, true>(m, st, grid, lds, a) : launch_fused_tiles_k<D, 64, 3, true, false>(m, st, grid, lds, a);
      }
    }
    return p.compl_sums ? launch_fused_tiles_k<D, F, SPW, false, true>(m, st, grid, lds, a) : launch_fused_tiles_k<D, F, SPW, false, false>(m, st, grid, lds, a);
  }); });
  if (rc == V2X_EINVAL) FAIL(m, V2X_EINVAL, "fused %s: unsupported shape", D::bwd ? "backward" : "forward");
  return rc;
}

int launch_fused_fwd(v2x_model* m, hipStream_t st, const DevBatch& d, const BatchPlan& p, bool frag_out) {
  // The copy follows the parameters by itself: Adam writes both (k_reduce_adam / pack_scatter), set / copy_weights
  // re-pack eagerly.  Only a caller that took the raw parameter pointer (v2x_param_ptr) forces a re-pack per forward.
  if (m->pk_stale) { CHK(launch_pack(m, st)); m->pk_stale = m->raw_params; }
  FusedFwdArgs a;
  memset(&a, 0, sizeof(a));
  a.xe = d.xe; a.row_ptr = d.rp; a.col_idx = d.ci; a.pk = m->pk_fwd;
  for (int s = 0; s <= m->L; ++s) { a.h[s] = m->h[s]; a.a[s] = m->a[s]; a.gate[s] = m->gate_bits + s * m->gate_stride; }
  a.n_graphs = d.B; a.N = m->N; a.L = m->L; a.S = m->S; a.edges_cap = FZ_TG * d.max_edges; a.n_edges = d.E; a.err = m->flag_dev;
  a.frag_out = frag_out ? 1 : 0;
  a.nbmask = m->nbmask;
  return launch_fused<FusedFwd>(m, st, p, a);
}

int launch_fused_bwd(v2x_model* m, hipStream_t st, const DevBatch& d, const BatchPlan& p) {
  FusedBwdArgs a;
  memset(&a, 0, sizeof(a));
  a.row_ptr = d.rp; a.col_idx = d.ci; a.pk = m->pk_bwd; a.gha = m->gha;
  for (int s = 0; s <= m->L; ++s) a.dpre[s] = m->dpre[s];
  for (int s = 0; s < m->L; ++s) a.gate[s] = m->gate_bits + s * m->gate_stride;
  a.n_graphs = d.B; a.N = m->N; a.L = m->L; a.S = m->S; a.edges_cap = FZ_TG * d.max_edges; a.n_edges = d.E; a.err = m->flag_dev;
  a.frag_gha = m->frag_live ? 1 : 0;
  a.nbmask = m->nbmask;
  return launch_fused<FusedBwd>(m, st, p, a);
}

// ------------------------------------------------------------------------------------ passes
// ------------------------------------------------------------------------------------ few-graph predict, one launch
constexpr size_t PIN_XE = 0, PIN_RP = 16384, PIN_CI = 20480, PIN_Q = 53248, PIN_BYTES = 65536;   // SMALL_ROWS rows, <= 31 in-edges each

int launch_small_forward(v2x_model* m, hipStream_t st, const DevBatch& d, float* q_dst = nullptr) {
  SmallFwdArgs a;
  memset(&a, 0, sizeof(a));
  a.xe = d.xe; a.row_ptr = d.rp; a.col_idx = d.ci; a.params = m->params;
  for (int s = 0; s <= m->L; ++s) { a.gnn_off[s] = m->gnn[s].off; a.gnn_sstride[s] = m->gnn[s].slot_stride; }
  for (int i = 0; i < 4; ++i) { a.dense_off[i] = m->dense[i].off; a.dense_sstride[i] = m->dense[i].slot_stride; }
  a.hbuf = m->small_h; a.sync = m->small_sync; a.err = m->flag_dev; a.q = q_dst ? q_dst : m->q;
  a.N = m->N; a.L = m->L; a.S = m->S; a.C = m->C; a.Dn = m->Dn; a.De = m->De; a.n_rows = d.R; a.slab_rows = SMALL_ROWS;
  const dim3 grid(m->N, d.B);
  const int rc = with_const<16, 32, 64>(m->F, [&](auto Fc) -> int {
    LAUNCH(m, "k_predict_small", k_predict_small<decltype(Fc)::value>, grid, SM_BLOCK, 0, st, a);
    return V2X_OK;
  });
  if (rc == V2X_EINVAL) FAIL(m, V2X_EINVAL, "small forward: unsupported feat_dim %d", m->F);
  return rc;
}

template <int F>
int launch_ragged_fwd_f(v2x_model* m, hipStream_t st, const RaggedFwdArgs& a, int n_wgs) {
  auto k = k_gnn_fwd_ragged<F>;
  static const bool once = [] { allow_big_lds((const void*)k_gnn_fwd_ragged<F>); return true; }();
  (void)once;
  LAUNCH(m, "k_gnn_fwd_ragged", k, dim3(n_wgs), RG_THREADS, (size_t)RaggedLds<F>::TOTAL * 4, st, a);
  return V2X_OK;
}

template <int F, bool BWD, typename Args>
int launch_ragged_small_f(v2x_model* m, hipStream_t st, const Args& a, int n_wgs) {
  if constexpr (BWD) {
    auto k = k_gnn_bwd_ragged_s<F>;
    LAUNCH(m, "k_gnn_bwd_ragged", k, dim3(n_wgs), RGS_THREADS, (size_t)RaggedSmallBwdLds<F>::TOTAL * 4, st, a);
  } else {
    auto k = k_gnn_fwd_ragged_s<F>;
    LAUNCH(m, "k_gnn_fwd_ragged", k, dim3(n_wgs), RGS_THREADS, (size_t)RaggedSmallLds<F>::TOTAL * 4, st, a);
  }
  return V2X_OK;
}

int launch_ragged_fwd(v2x_model* m, hipStream_t st, const DevBatch& d, const BatchPlan& p) {
  RaggedFwdArgs a;
  memset(&a, 0, sizeof(a));
  a.xe = d.xe; a.graph_off = d.goff; a.row_ptr = d.rp;
  a.mask_words = (d.max_nodes + 31) / 32;
  a.adjT = (const unsigned*)m->adj_mask.p + (size_t)d.R * a.mask_words;
  a.plan = (const int32_t*)m->plan_buf.p;
  for (int s = 0; s <= m->L; ++s) { a.W[s] = m->params + m->gnn[s].off; a.h[s] = m->h[s]; a.a[s] = m->a[s]; }
  a.n_graphs = d.B; a.n_rows = d.R; a.L = m->L; a.capp = p.capp; a.xr = m->Dn + m->De; a.err = m->flag_dev;
  a.ts = m->ts_buf;
  const int n_wgs = p.wgs;
  int rc;
  if (p.ragged_small) {                                 // 160-row tiles, weights as fragments from L2 (kernels_ragged_small.hpp)
    if (m->pk_stale) { CHK(launch_pack(m, st)); m->pk_stale = m->raw_params; }
    RaggedSmallFwdArgs sa{a, m->pk_fwd};
    rc = with_const<16, 32, 64>(m->F, [&](auto Fc) { return launch_ragged_small_f<decltype(Fc)::value, false>(m, st, sa, n_wgs); });
  } else {
    rc = with_const<16, 32, 64>(m->F, [&](auto Fc) { return launch_ragged_fwd_f<decltype(Fc)::value>(m, st, a, n_wgs); });
  }
  if (rc == V2X_EINVAL) FAIL(m, V2X_EINVAL, "ragged forward: unsupported feat_dim %d", m->F);
  return rc;
}

template <int F>
int launch_ragged_bwd_f(v2x_model* m, hipStream_t st, const RaggedBwdArgs& a, int n_wgs) {
  auto k = k_gnn_bwd_ragged<F>;
  static const bool once = [] { allow_big_lds((const void*)k_gnn_bwd_ragged<F>); return true; }();
  (void)once;
  LAUNCH(m, "k_gnn_bwd_ragged", k, dim3(n_wgs), RG_THREADS, (size_t)RaggedBwdLds<F>::TOTAL * 4, st, a);
  return V2X_OK;
}

// L + 1 transposed aggregations + L data gradients of ragged graphs in one launch (masks and plan: the forward's)
int launch_ragged_bwd(v2x_model* m, hipStream_t st, const DevBatch& d, const BatchPlan& p) {
  RaggedBwdArgs a;
  memset(&a, 0, sizeof(a));
  a.gha = m->gha; a.graph_off = d.goff;
  a.mask_words = (d.max_nodes + 31) / 32;
  a.adj = (const unsigned*)m->adj_mask.p;
  a.plan = (const int32_t*)m->plan_buf.p;
  for (int s = 0; s <= m->L; ++s) { a.W[s] = m->params + m->gnn[s].off; a.h[s] = m->h[s]; a.dpre[s] = m->dpre[s]; }
  a.n_graphs = d.B; a.n_rows = d.R; a.L = m->L; a.capp = p.capp; a.xr = m->Dn + m->De; a.err = m->flag_dev;
  const int n_wgs = p.wgs;
  int rc;
  if (p.ragged_small) {
    RaggedSmallBwdArgs sa{a, m->pk_bwd};
    rc = with_const<16, 32, 64>(m->F, [&](auto Fc) { return launch_ragged_small_f<decltype(Fc)::value, true>(m, st, sa, n_wgs); });
  } else {
    rc = with_const<16, 32, 64>(m->F, [&](auto Fc) { return launch_ragged_bwd_f<decltype(Fc)::value>(m, st, a, n_wgs); });
  }
  if (rc == V2X_EINVAL) FAIL(m, V2X_EINVAL, "ragged backward: unsupported feat_dim %d", m->F);
  return rc;
}

int run_forward(v2x_model* m, hipStream_t st, const DevBatch& d, const BatchPlan& p, bool with_mlp = true) {
  const int F = m->F, L = m->L;
  const IdxMap& x = p.x;
  const bool ragged = p.form == GraphLayers::Ragged;
  m->frag_live = !with_mlp && p.frag_ok;
  if (p.form == GraphLayers::Fused) {
    CHK(launch_fused_fwd(m, st, d, p, m->frag_live));    // embed + L stages + L+1 aggregations: one launch
  } else {
    if (p.need_adj_masks) {
      AggDenseArgs q = agg_dense_args(d, m->N, F);
      q.adj = (unsigned*)m->adj_mask.p;
      q.adjT = q.adj + (size_t)d.R * q.mask_words;
      q.err = m->flag_dev;
      if (ragged) m->plan_len = p.wgs + 1;
      if (ragged && p.plan_form == RaggedPlan::Interval) { q.plan = (int32_t*)m->plan_buf.p; q.plan_capp = p.capp; q.plan_n = p.wgs; }
      if (ragged && p.plan_form == RaggedPlan::Folded) { q.plan = (int32_t*)m->plan_buf.p; q.plan_cap = p.cap; q.plan_n = p.wgs; }
      // (the plan reads the offsets, the masks the CSR: independent -- but as a forked branch of the captured step the two
      //  cost MORE than one after the other: 0.466 against 0.455 ms per configs[4] step, the graph's cross-branch
      //  dependencies outweigh the 5 us the plan takes)
      if (ragged && p.plan_form == RaggedPlan::Packed) {
        static const bool once = [] { allow_big_lds((const void*)k_ragged_plan); return true; }();
        (void)once;
        RaggedPlanArgs pa{d.goff, (int32_t*)m->plan_buf.p, d.B, p.wgs, p.cap};
        LAUNCH(m, "k_ragged_plan", k_ragged_plan, dim3(1), RG_PLAN_THREADS, (size_t)p.plan_words * 4, st, pa);
      }
      CHK(build_adj_masks(m, st, q));
    }
    if (ragged) {                                        // embed + L stages + L + 1 aggregations of ragged graphs: one launch
      CHK(launch_ragged_fwd(m, st, d, p));
    } else {
      CHK(launch_node_fwd(m, st, 0, x, d.xe, nullptr, d.nbr, m->h[0]));
      CHK(launch_agg(m, st, d, p.dense_agg, m->N, F, m->h[0], F, nullptr, 0, nullptr, m->a[0], 0));
      for (int s = 1; s <= L; ++s) {
        CHK(launch_node_fwd(m, st, s, x, d.xe, m->h[s - 1], m->a[s - 1], m->h[s]));
        CHK(launch_agg(m, st, d, p.dense_agg, m->N, F, m->h[s], F, nullptr, 0, nullptr, m->a[s], 0));
      }
    }
  }
  if (!with_mlp) return V2X_OK;          // training: the MLP runs fused with its backward (k_mlp_train_wg)
  MlpArgs a;
  mlp_args(m, a, x, d.xe, m->h[L], m->a[L]);
  return launch_mlp(m, st, a, false);
}

float loss_denominator(const v2x_model* m, int n_global) {
  // fixed-N: per-output mean over (B_global, C)  (tf.losses.huber_loss per output, BS_brain.py:214)
  // variable graphs: n_global counts node rows; single mean over (rows_global, C)
  return (float)((double)n_global * m->C);
}

// The decision MLP of a backward pass, after run_forward(with_mlp = wide).  A narrow model: forward + Huber + backward + the Dense
// weight gradients in one launch.  A wide model: k_mlp_bwd, Dense-0's data gradient, Dense 1..3 (+ Dense-0 unless merged below).
int backward_mlp(v2x_model* m, hipStream_t st, const DevBatch& d, const BatchPlan& p, const BwdCall& c, const float* y_dev, int n_global) {
  const int L = m->L;
  MlpArgs a;
  mlp_args(m, a, p.x, d.xe, m->h[L], m->a[L]);
  a.y = y_dev;
  a.inv_denom = 1.0f / loss_denominator(m, n_global);
  if (m->frag_live && !p.frag_ok) FAIL(m, V2X_ESTATE, "backward: the saved forward is fragment-major, this backward cannot read it");
  a.frag_groups = m->frag_live ? d.B / FZ_TG : 0;
  if (c.tq) {
    if (!p.mlp_wg) FAIL(m, V2X_ESTATE, "backward: in-kernel DQN targets need the k_mlp_train_wg path");
    a.tq = c.tq; a.y = c.tq; a.q = c.y_out;
  }
  if (p.mlp_wg) return launch_mlp_train_wg(m, st, a, !dense0_out(p, c));      // the Dense weight gradients come out of the MLP launch itself
  CHK(launch_mlp(m, st, a, true));
  return wgrad_mlp(m, st, p.x, d.xe, m->h[L], m->a[L], wide_merged(p, c));
}

// The graph layers of a backward pass: their data chain, then all L + 1 weight gradients (+ what rides on them): one launch up to L = 7.
int backward_graph_layers(v2x_model* m, hipStream_t st, const DevBatch& d, const BatchPlan& p, const BwdCall& c) {
  const int F = m->F, L = m->L;
  if (p.form == GraphLayers::Fused) {
    CHK(launch_fused_bwd(m, st, d, p));    // L+1 transposed aggregations + L data gradients: one launch
  } else if (ragged_fused_bwd(p, c)) {
    CHK(launch_ragged_bwd(m, st, d, p));   // the same for ragged graphs (masks and plan from this step's forward)
  } else {
    for (int s = L; s >= 1; --s) {
      // dpre_s = (dh_direct + Agg^T(dagg)) * relu'(h_s)
      CHK(launch_agg(m, st, d, p.dense_agg, m->N, F, m->gha + F, 2 * F, m->gha, 2 * F, s < L ? m->h[s] : nullptr, m->dpre[s], 1));
      CHK(launch_dgrad(m, st, s, p.x, m->dpre[s], m->gha));
    }
    CHK(launch_agg(m, st, d, p.dense_agg, m->N, F, m->gha + F, 2 * F, m->gha, 2 * F, m->h[0], m->dpre[0], 1));
  }
  return wgrad_gnn_all(m, st, d, p, c);
}

int run_backward(v2x_model* m, hipStream_t st, const DevBatch& d, const BatchPlan& p, const BwdCall& c, const float* y_dev, int n_global) {
  CHK(backward_mlp(m, st, d, p, c, y_dev, n_global));
  return backward_graph_layers(m, st, d, p, c);
}

// forward + backward of the whole batch
int run_step(v2x_model* m, hipStream_t st, const DevBatch& d, const BatchPlan& p, const BwdCall& c, const float* y_dev, int n_global) {
  CHK(run_forward(m, st, d, p, !p.mlp_wg));
  return run_backward(m, st, d, p, c, y_dev, n_global);
}

int resolve_y(v2x_model* m, const float* y, int y_on_device, int R, hipStream_t st, const float** out) {
  if (!y) FAIL(m, V2X_EINVAL, "targets y are null");
  if (y_on_device) { *out = y; return V2X_OK; }
  CHK(ensure(m, m->st_y, (size_t)R * m->C * sizeof(float)));
  HIPCHK(m, hipMemcpyAsync(m->st_y.p, y, (size_t)R * m->C * sizeof(float), hipMemcpyHostToDevice, st));
  *out = (const float*)m->st_y.p;
  return V2X_OK;
}

int emit_loss(v2x_model* m, float* loss_out, int loss_on_device, hipStream_t st) {
  if (!loss_out) return V2X_OK;
  const int n = m->cfg.variable_graphs ? 1 : m->N;
  if (loss_on_device) {
    HIPCHK(m, hipMemcpyAsync(loss_out, m->loss_dev, n * sizeof(float), hipMemcpyDeviceToDevice, st));
  } else {
    HIPCHK(m, hipMemcpyAsync(loss_out, m->loss_dev, n * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(m, hipStreamSynchronize(st));
    CHK(check_flag(m));
  }
  return V2X_OK;
}

// Run `body` either eagerly or through a cached hipGraph keyed on the pointers / sizes it bakes in.
// Capture happens on a PRIVATE stream (m->cap), not on the caller's: a hipGraph does not remember the stream it was recorded on,
// and the caller's stream is the one the host framework's collectives synchronise with -- RCCL's watchdog thread polls events
// that were last recorded on it, and polling such an event while the stream is capturing is an error that takes the process down
// (hipErrorCapturedEvent: seen once in five runs of tools/dp_host_overhead.py, round 6).  `st` is the caller's local stream
// variable, taken by reference: the body's lambdas read it, so it names the capture stream while the body records.
template <typename Body>
int run_maybe_graph(v2x_model* m, hipStream_t& st, const GraphKey& key, Body body) {
  const bool want = m->cfg.use_graph && !m->prof && st != nullptr;
  if (!want) return body();
  auto it = m->graphs.find(key);
  if (it != m->graphs.end()) {
    size_t i = 0;                                   // what the captured host code had left in the layer descriptors
    for (auto* v : {&m->gnn, &m->dense})
      for (LayerDesc& ld : *v) ld.n_slabs = it->second.n_slabs[i++];
    m->frag_live = it->second.frag_live;            // ... and in the model (layout of the saved h_L / a_L / gha)
    m->reduce_groups = it->second.reduce_groups;
    HIPCHK(m, hipGraphLaunch(it->second.exec, st));
    return V2X_OK;
  }
  // make sure every lazily-sized buffer and function attribute exists before capture: run once eagerly
  // is not possible without side effects on optimizer state, so callers pre-size buffers (see below).
  hipGraph_t g = nullptr;
  hipStream_t const user = st, cap = m->cap ? m->cap : st;
  HIPCHK(m, hipStreamBeginCapture(cap, hipStreamCaptureModeThreadLocal));
  m->capturing = true;
  st = cap;
  const int r = body();
  st = user;
  m->capturing = false;
  hipError_t e = hipStreamEndCapture(cap, &g);
  if (r != V2X_OK) { if (g) hipGraphDestroy(g); return r; }
  if (e != hipSuccess) FAIL(m, V2X_EHIP, "hipStreamEndCapture: %s", hipGetErrorString(e));
  hipGraphExec_t ge = nullptr;
  e = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
  hipGraphDestroy(g);
  if (e != hipSuccess) FAIL(m, V2X_EHIP, "hipGraphInstantiate: %s", hipGetErrorString(e));
  if (m->graphs.size() >= 16) drop_graphs(m);
  v2x_model::GraphEntry entry;
  entry.exec = ge;
  entry.frag_live = m->frag_live;
  entry.reduce_groups = m->reduce_groups;
  for (auto* v : {&m->gnn, &m->dense})
    for (const LayerDesc& ld : *v) entry.n_slabs.push_back(ld.n_slabs);
  m->graphs[key] = entry;
  HIPCHK(m, hipGraphLaunch(ge, st));
  return V2X_OK;
}

GraphKey make_key(int kind, const DevBatch& d, const void* y, int n_global) {
  GraphKey k;
  memset(&k, 0, sizeof(k));
  k.kind = kind;
  k.ptrs[0] = d.xe; k.ptrs[1] = d.nbr; k.ptrs[2] = d.goff; k.ptrs[3] = d.rp; k.ptrs[4] = d.ci; k.ptrs[5] = y;
  k.sizes[0] = d.B; k.sizes[1] = d.R; k.sizes[2] = d.E; k.sizes[3] = d.max_nodes; k.sizes[4] = d.max_edges;
  k.sizes[5] = n_global;
  return k;
}

int max_slabs(const v2x_model* m, int n_idx, int n_slots) {
  int chunk, nc = 1;
  const int mr = m->L >= 1 ? merged_wg_rows(m, n_idx, n_slots) : 0;
  const Knobs& kn = m->knobs;
  for (int rows : {kn.wg_chunk_gnn, kn.wg_chunk_dense, kn.wg_chunk_embed, kn.wg_chunk_d123, 768, 896, 1024, mr})
    if (rows > 0) nc = std::max(nc, role_chunks(kn, n_idx, n_slots, 1000, 1000, &chunk, rows));  // (a switch at 0 = a default, listed here)
  if (is_wide(m)) nc = std::max(nc, wide_splits(n_idx, 1, n_slots));     // the fewest tiles (one) split most
  else nc = std::max(nc, mlp_wg_split(n_idx, n_slots).n_slabs);         // k_mlp_train_wg: one slab per workgroup and slot
  return nc + 1;
}

int presize(v2x_model* m, const DevBatch& d, const BatchPlan& p) {
  CHK(ensure_rows(m, d.R));
  if (p.need_adj_masks) CHK(ensure(m, m->adj_mask, (size_t)2 * d.R * ((d.max_nodes + 31) / 32) * 4));
  if (p.form == GraphLayers::Ragged) CHK(ensure(m, m->plan_buf, (size_t)(p.wgs + 2) * 4));
  if (p.split > 1) CHK(ensure_xchg(m, p.tiles));
  CHK(ensure_slabs(m, max_slabs(m, p.x.n_idx, p.x.grid_y)));
  return V2X_OK;
}

// helpers for the per-kernel entry points, which take rows and no batch
IdxMap idx_map_rows(const v2x_model* m, int n_rows) {
  DevBatch d;
  memset(&d, 0, sizeof(d));
  d.R = n_rows; d.B = m->cfg.variable_graphs ? 1 : n_rows / m->N;
  return idx_map(m, d);
}

int presize_rows(v2x_model* m, int n_rows) {
  CHK(ensure_rows(m, n_rows));
  const IdxMap x = idx_map_rows(m, n_rows);
  CHK(ensure_slabs(m, max_slabs(m, x.n_idx, x.grid_y)));
  return V2X_OK;
}

}  // namespace

// the v2x_last_error(NULL) text, for the entry points of the other translation units (v2xopt.hip)
namespace v2x {
void set_global_error(const char* text) { g_err = text; }
// links, channels and whether the graphs may differ in size: what v2x_rollout_step (v2xsimdev.hip) checks a batch against
// before it launches anything
void model_dims(const v2x_model* m, int* n_nodes, int* n_channels, int* variable_graphs) {
  *n_nodes = m->N; *n_channels = m->C; *variable_graphs = m->cfg.variable_graphs;
}
// feature width, message-passing layers and weight sharing: with model_dims what v2x_eval_sweep_mixed (v2xsimdev.hip) compares
// between the networks of a sweep
void model_shape(const v2x_model* m, int* feat_dim, int* n_mp_layers, int* share_weights) {
  *feat_dim = m->cfg.feat_dim; *n_mp_layers = m->cfg.n_mp_layers; *share_weights = m->cfg.share_weights;
}
}

// ======================================================================================= C ABI
extern "C" {

const char* v2x_version(void) { return "v2xgnn 0.1 (gfx950)"; }

const char* v2x_last_error(const v2x_model* m) { return m ? m->err.c_str() : g_err.c_str(); }

int v2x_create(const v2x_config* cfg, v2x_model** out) {
  v2x_model* nullm = nullptr;
  if (!cfg || !out) FAIL(nullm, V2X_EINVAL, "v2x_create: null argument");
  *out = nullptr;
  if (cfg->n_channels != 4) FAIL(nullm, V2X_EINVAL, "n_channels must be 4 in this build (got %d)", cfg->n_channels);
  if (cfg->feat_dim != 16 && cfg->feat_dim != 32 && cfg->feat_dim != 64 && cfg->feat_dim != 128 && cfg->feat_dim != 256)
    FAIL(nullm, V2X_EINVAL, "feat_dim must be 16, 32, 64, 128 or 256 in this build (got %d)", cfg->feat_dim);
  if (cfg->n_nodes < 1) FAIL(nullm, V2X_EINVAL, "n_nodes must be >= 1");
  if (cfg->n_mp_layers < 1 || cfg->n_mp_layers > 8) FAIL(nullm, V2X_EINVAL, "n_mp_layers must be in [1,8]");
  if (cfg->variable_graphs && !cfg->share_weights)
    FAIL(nullm, V2X_EINVAL, "variable_graphs requires share_weights (per-node weights need a fixed node count)");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    FAIL(nullm, V2X_EHIP, "no HIP device available: the v2xgnn engine has no CPU fallback");
  if (cfg->device < 0 || cfg->device >= ndev) FAIL(nullm, V2X_EINVAL, "device %d out of range (%d devices)", cfg->device, ndev);
  if (hipSetDevice(cfg->device) != hipSuccess) FAIL(nullm, V2X_EHIP, "hipSetDevice(%d) failed", cfg->device);

  v2x_model* m = new v2x_model();
  m->cfg = *cfg;
  if (m->cfg.lr <= 0.f) m->cfg.lr = 1e-3f;
  if (m->cfg.beta1 <= 0.f) m->cfg.beta1 = 0.5f;      // BS_brain.py:212
  if (m->cfg.beta2 <= 0.f) m->cfg.beta2 = 0.999f;
  if (m->cfg.eps <= 0.f) m->cfg.eps = 1e-7f;         // K.epsilon()
  m->N = cfg->n_nodes; m->C = cfg->n_channels; m->F = cfg->feat_dim; m->L = cfg->n_mp_layers;
  m->S = cfg->share_weights ? 1 : cfg->n_nodes;
  m->Dn = 2 * m->C + 1; m->De = m->C;               // BS_brain.py:101-102 with node_info=3, edge_info=1
  m->knobs = read_knobs();        // every environment switch, fixed for the life of the model (knobs.hpp)
  build_layout(m);
  set_attrs(m->F, m->knobs);
  m->h.assign(m->L + 1, nullptr);
  m->a.assign(m->L + 1, nullptr);
  m->dpre.assign(m->L + 1, nullptr);
  auto fail = [&](const char* what) {
    g_err = std::string("v2x_create: ") + what + ": " + m->err;
    v2x_destroy(m);
    return V2X_EHIP;
  };
  const size_t pb = (size_t)m->P * sizeof(float);
  if (dev_alloc(m, &m->params, m->P) || dev_alloc(m, &m->grads, m->P) || dev_alloc(m, &m->mom, m->P) ||
      dev_alloc(m, &m->vel, m->P) || dev_alloc(m, &m->loss_dev, (size_t)m->N + 1) || dev_alloc(m, &m->zero_buf, 1024) ||
      dev_alloc(m, &m->loss_part, 128) || dev_alloc(m, &m->adam_scal, 16))
    return fail("allocation");
  const Knobs& kn = m->knobs;
  if (kn.small_predict && !m->cfg.variable_graphs && m->F <= 64 && m->L <= FZ_MAXL) {
    const size_t hb = (size_t)(m->L + 1) * SMALL_ROWS * m->F * sizeof(unsigned long long), sb = (size_t)2 * SMALL_ROWS * sizeof(unsigned);
    void *ph = nullptr, *ps = nullptr;
    if (hipMalloc(&ph, hb) != hipSuccess || hipMalloc(&ps, sb) != hipSuccess) return fail("allocation");
    m->small_h = static_cast<unsigned long long*>(ph);
    if (hipMemset(ph, 0, hb)) return fail("memset");             // tag 0 = never written
    m->small_sync = static_cast<unsigned long long*>(ps);
    void *hh = nullptr, *hdv = nullptr;
    if (kn.small_pinned && hipHostMalloc(&hh, PIN_BYTES, hipHostMallocMapped) == hipSuccess &&
        hipHostGetDevicePointer(&hdv, hh, 0) == hipSuccess) {
      m->pin_h = static_cast<char*>(hh); m->pin_d = static_cast<char*>(hdv);
    } else {
      (void)hipGetLastError();
      if (hh) hipHostFree(hh);
    }
    if (hipMemset(m->small_sync, 0, (size_t)2 * SMALL_ROWS * sizeof(unsigned))) return fail("memset");
  }
  // Knobs::fused = 0 keeps the layer-by-layer kernels: A/B measurements and the test that the two paths agree bitwise
  // (ragged models with shared weights stream the same copy in their small-tile kernels, kernels_ragged_small.hpp)
  if (kn.fused && (!m->cfg.variable_graphs || (m->S == 1 && kn.ragged_small)) && m->F <= 64 && m->L <= FZ_MAXL) {
    const int FB = m->F / 16, KB = 2 * FB + 1;
    const size_t fwd0 = (size_t)FB * 256 + m->F, fwd = (size_t)KB * FB * 256 + m->F, bwd = (size_t)FB * 2 * FB * 256;
    if (dev_alloc(m, &m->pk_fwd, (size_t)m->S * fwd0 + (size_t)m->L * m->S * fwd) || dev_alloc(m, &m->pk_bwd, (size_t)m->L * m->S * bwd))
      return fail("allocation");
    m->pk_stale = true;             // first forward packs whatever the parameters are by then
  }
  if ((m->pk_fwd || m->cfg.variable_graphs) && kn.fused_ts) {
    if (dev_alloc(m, &m->ts_buf, 4 * 8 * 64)) return fail("allocation");
    hipMemset(m->ts_buf, 0, 4 * 8 * 64 * 8);
  }
  if (hipMemset(m->zero_buf, 0, 4096) || hipMemset(m->loss_part, 0, 512) || hipMemset(m->params, 0, pb) || hipMemset(m->grads, 0, pb) || hipMemset(m->mom, 0, pb) || hipMemset(m->vel, 0, pb))
    return fail("memset");
  {
    FlagWord f;
    if (alloc_flag(&f) != V2X_OK) return fail("pinned flag word");
    m->flag_host = f.host; m->flag_dev = f.dev;
  }
  if (hipStreamCreateWithFlags(&m->cap, hipStreamNonBlocking) != hipSuccess) return fail("capture stream");
  // The memsets above run on the null stream and may still be in flight when this returns; the caller's next call
  // (v2x_set_weights: a copy into the parameters) goes to ITS stream, which a non-blocking stream -- every stream of PyTorch's
  // pool -- does not order behind the null stream.  Without this wait the zeroing could land on top of the weights just set:
  // seen as zeroed leading parameters after set_weights on a side stream, now and then, once a process had made and freed models.
  if (hipDeviceSynchronize() != hipSuccess) return fail("synchronisation");
  *out = m;
  return V2X_OK;
}

void v2x_destroy(v2x_model* m) {
  if (!m) return;
  hipSetDevice(m->cfg.device);
  hipDeviceSynchronize();
  for (auto& kv : m->graphs) hipGraphExecDestroy(kv.second.exec);
  for (auto& r : m->prof_recs) { hipEventDestroy(r.ev0); hipEventDestroy(r.ev1); }
  float* ptrs[] = {m->params, m->grads, m->mom, m->vel, m->z1, m->z2, m->z3, m->q, m->dq, m->dz1, m->dz2, m->dz3,
                   m->gha, m->rowloss, m->loss_dev, m->slab, m->zero_buf, m->loss_part, m->pk_fwd, m->pk_bwd, m->adam_scal};
  for (float* p : m->dpre) if (p) hipFree(p);
  if (m->gate_bits) hipFree(m->gate_bits);
  if (m->nbmask) hipFree(m->nbmask);
  for (auto& e : m->dp_ev) if (e) hipEventDestroy(e);
  if (m->dp_st) hipStreamDestroy(m->dp_st);
  if (m->cap) hipStreamDestroy(m->cap);
  for (float* p : ptrs) if (p) hipFree(p);
  for (float* p : m->h) if (p) hipFree(p);
  for (float* p : m->a) if (p) hipFree(p);
  DevBuf* bufs[] = {&m->st_xe, &m->st_nbr, &m->st_goff, &m->st_rp, &m->st_ci, &m->st_y, &m->st_q, &m->adj_mask, &m->plan_buf};
  for (DevBuf* b : bufs) if (b->p) hipFree(b->p);
  if (m->flag_host) hipHostFree(m->flag_host);
  if (m->ts_buf) hipFree(m->ts_buf);
  if (m->small_h) hipFree(m->small_h);
  if (m->xchg_sync) {                  // the process-wide epoch base moves past everything this buffer's address has seen
    unsigned long long seen = 0;
    if (xchg_max_count(m, &seen) == V2X_OK) {
      std::lock_guard<std::mutex> lock(g_xchg_epoch_mutex);
      g_xchg_epoch_next = std::max(g_xchg_epoch_next, seen + 1);
    }
  }
  if (m->xchg_buf) hipFree(m->xchg_buf);
  if (m->xchg_sync) hipFree(m->xchg_sync);
  if (m->small_sync) hipFree(m->small_sync);
  if (m->pin_h) hipHostFree(m->pin_h);
  delete m;
}

int64_t v2x_param_count(const v2x_model* m) { return m ? m->P : 0; }
float* v2x_param_ptr(v2x_model* m) {
  if (m) {
    // the caller may write the parameters behind the library's back from now on: every fused forward re-packs its
    // fragment-major copy first -- a launch that graphs captured BEFORE this call do not contain, so they are dropped
    if (!m->raw_params) drop_graphs(m);
    m->pk_stale = m->raw_params = true;
  }
  return m ? m->params : nullptr;
}
float* v2x_grad_ptr(v2x_model* m) { return m ? m->grads : nullptr; }

int v2x_get_weights(v2x_model* m, float* host_out, void* stream) {
  if (!m || !host_out) FAIL(m, V2X_EINVAL, "get_weights: null argument");
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(m, hipMemcpyAsync(host_out, m->params, (size_t)m->P * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(m, hipStreamSynchronize(st));
  return V2X_OK;
}

int v2x_set_weights(v2x_model* m, const float* host_in, void* stream) {
  if (!m || !host_in) FAIL(m, V2X_EINVAL, "set_weights: null argument");
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(m, hipMemcpyAsync(m->params, host_in, (size_t)m->P * 4, hipMemcpyHostToDevice, st));
  if (m->pk_fwd) { CHK(launch_pack(m, st)); m->pk_stale = m->raw_params; }
  HIPCHK(m, hipStreamSynchronize(st));
  return V2X_OK;
}

int v2x_copy_weights(v2x_model* dst, const v2x_model* src, void* stream) {
  if (!dst || !src) FAIL(dst, V2X_EINVAL, "copy_weights: null argument");
  if (dst->P != src->P || dst->F != src->F || dst->N != src->N || dst->S != src->S || dst->L != src->L)
    FAIL(dst, V2X_EINVAL, "copy_weights: models have different shapes");
  HIPCHK(dst, hipMemcpyAsync(dst->params, src->params, (size_t)dst->P * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  if (dst->pk_fwd) { CHK(launch_pack(dst, (hipStream_t)stream)); dst->pk_stale = dst->raw_params; }
  return V2X_OK;
}

int v2x_get_optimizer_state(v2x_model* m, float* host_m, float* host_v, int64_t* iterations, void* stream) {
  if (!m) FAIL(m, V2X_EINVAL, "null model");
  hipStream_t st = (hipStream_t)stream;
  if (host_m) HIPCHK(m, hipMemcpyAsync(host_m, m->mom, (size_t)m->P * 4, hipMemcpyDeviceToHost, st));
  if (host_v) HIPCHK(m, hipMemcpyAsync(host_v, m->vel, (size_t)m->P * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(m, hipStreamSynchronize(st));
  if (iterations) *iterations = m->iterations;
  return V2X_OK;
}

int v2x_set_optimizer_state(v2x_model* m, const float* host_m, const float* host_v, int64_t iterations, void* stream) {
  if (!m) FAIL(m, V2X_EINVAL, "null model");
  hipStream_t st = (hipStream_t)stream;
  if (host_m) HIPCHK(m, hipMemcpyAsync(m->mom, host_m, (size_t)m->P * 4, hipMemcpyHostToDevice, st));
  if (host_v) HIPCHK(m, hipMemcpyAsync(m->vel, host_v, (size_t)m->P * 4, hipMemcpyHostToDevice, st));
  HIPCHK(m, hipStreamSynchronize(st));
  m->iterations = iterations;
  return V2X_OK;
}

int v2x_forward(v2x_model* m, const v2x_batch* b, float* q_out, int q_on_device, void* stream) {
  if (!m || !q_out) FAIL(m, V2X_EINVAL, "forward: null argument");
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(m, hipSetDevice(m->cfg.device));
  // host batch in, host q out, a few graphs (BS.predict in the rollout loop): the kernel reads the batch from, and writes q
  // to, a pinned device-mapped window -- one launch and one stream synchronisation, no copy launches at all
  if (b && !b->on_device && !q_on_device && m->pin_h && b->xe && b->row_ptr && b->n_rows > 0 && b->n_rows <= SMALL_ROWS &&
      b->n_edges >= 0 && (size_t)b->n_edges * 4 <= PIN_Q - PIN_CI && (b->n_edges == 0 || b->col_idx)) {
    DevBatch hd;
    memset(&hd, 0, sizeof(hd));
    hd.B = b->n_graphs; hd.R = b->n_rows; hd.E = b->n_edges; hd.max_nodes = b->max_nodes; hd.max_edges = b->max_edges;
    hd.goff = b->graph_off; hd.nbr = b->nbr_init;
    if (hd.B > 0 && !m->cfg.variable_graphs && hd.R == hd.B * m->N && plan_batch(m, hd).small_predict) {
      CHK(validate_host_batch(m, b, m->N));
      memcpy(m->pin_h + PIN_XE, b->xe, (size_t)hd.R * XE * sizeof(float));
      memcpy(m->pin_h + PIN_RP, b->row_ptr, (size_t)(hd.R + 1) * 4);
      if (hd.E > 0) memcpy(m->pin_h + PIN_CI, b->col_idx, (size_t)hd.E * 4);
      hd.xe = reinterpret_cast<const float*>(m->pin_d + PIN_XE);
      hd.rp = reinterpret_cast<const int32_t*>(m->pin_d + PIN_RP);
      hd.ci = reinterpret_cast<const int32_t*>(m->pin_d + PIN_CI);
      float* qd = reinterpret_cast<float*>(m->pin_d + PIN_Q);
      CHK(run_maybe_graph(m, st, make_key(8, hd, qd, 0), [&]() { return launch_small_forward(m, st, hd, qd); }));
      m->phase0_done = false;
      HIPCHK(m, hipStreamSynchronize(st));
      CHK(check_flag(m));
      memcpy(q_out, m->pin_h + PIN_Q, (size_t)hd.R * m->C * sizeof(float));
      return V2X_OK;
    }
  }
  DevBatch d;
  CHK(resolve_batch(m, b, &d, st));
  const BatchPlan p = plan_batch(m, d);
  CHK(presize(m, d, p));
  // a few graphs (the rollout predict): the whole network in one launch, nothing saved for a backward pass
  const bool small = p.small_predict;
  if (small) CHK(run_maybe_graph(m, st, make_key(7, d, nullptr, 0), [&]() { return launch_small_forward(m, st, d); }));
  else CHK(run_maybe_graph(m, st, make_key(1, d, nullptr, 0), [&]() { return run_forward(m, st, d, p); }));
  m->phase0_done = false;
  const size_t qb = (size_t)d.R * m->C * sizeof(float);
  if (q_on_device) {
    HIPCHK(m, hipMemcpyAsync(q_out, m->q, qb, hipMemcpyDeviceToDevice, st));
  } else {
    HIPCHK(m, hipMemcpyAsync(q_out, m->q, qb, hipMemcpyDeviceToHost, st));
    HIPCHK(m, hipStreamSynchronize(st));
    CHK(check_flag(m));
  }
  return V2X_OK;
}

static int fwd_bwd(v2x_model* m, const v2x_batch* b, const float* y, int y_on_device, int32_t n_global,
                   float* loss_out, int loss_on_device, void* stream, bool with_adam) {
  if (!m) FAIL(m, V2X_EINVAL, "null model");
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(m, hipSetDevice(m->cfg.device));
  DevBatch d;
  CHK(resolve_batch(m, b, &d, st));
  if (n_global <= 0) n_global = m->cfg.variable_graphs ? d.R : d.B;
  const float* yd;
  CHK(resolve_y(m, y, y_on_device, d.R, st, &yd));
  const BatchPlan p = plan_batch(m, d);
  CHK(presize(m, d, p));
  if (with_adam) {
    // lr_t depends on the iteration count, so the Adam node stays outside the replayed graph.  Wide path: Adam rides on the
    // weight-gradient launch for the layers that launch writes in place; this step's lr_t reaches the (replayed) kernels
    // through device memory, written by a one-thread launch whose ARGUMENTS carry the values (copied when the launch is
    // enqueued: no asynchronous read of host stack memory, no host / stream synchronisation -- ADVICE r04)
    const bool fuse = p.wide_adam_fusable;
    if (fuse) {
      hipLaunchKernelGGL(k_set4, dim3(1), dim3(64), 0, st, m->adam_scal, adam_lr_t(m, m->iterations + 1), m->cfg.beta1, m->cfg.beta2, m->cfg.eps);
      CHK(launch_check(m, "k_set4"));
    }
    BwdCall c;
    c.fuse_adam = fuse;
    CHK(run_maybe_graph(m, st, make_key(fuse ? 9 : 2, d, yd, n_global), [&]() { return run_step(m, st, d, p, c, yd, n_global); }));
    CHK(launch_reduce_adam(m, st, 1, true, nullptr, loss_job(m, d, n_global), -1, fuse));
  } else {
    CHK(run_maybe_graph(m, st, make_key(3, d, yd, n_global), [&]() {
      CHK(run_step(m, st, d, p, BwdCall{}, yd, n_global));
      return launch_reduce_adam(m, st, 1, false, nullptr, loss_job(m, d, n_global));
    }));
  }
  m->phase0_done = false;
  return emit_loss(m, loss_out, loss_on_device, st);
}

// Data-parallel step in two phases (dp.py): phase 0 = forward, decision-MLP forward + Huber + backward, the Dense layers'
// weight gradients reduced into their bucket of the flat gradient; phase 1 = graph-layer backward, their weight gradients,
// the per-output losses.  After phase 0 the Dense bucket is final, so the host can start its all-reduce (RCCL runs on its
// own stream) while phase 1 computes.
int v2x_forward_backward_phase(v2x_model* m, const v2x_batch* b, const float* y, int y_on_device, int32_t n_global, int phase,
                               float* loss_out, int loss_on_device, void* stream) {
  if (!m) FAIL(m, V2X_EINVAL, "null model");
  if (phase < 0 || phase >= n_phase_buckets(m)) FAIL(m, V2X_EINVAL, "forward_backward_phase: phase must be in [0, %d)", n_phase_buckets(m));
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(m, hipSetDevice(m->cfg.device));
  DevBatch d;
  CHK(resolve_batch(m, b, &d, st));
  if (n_global <= 0) n_global = m->cfg.variable_graphs ? d.R : d.B;
  const float* yd;
  CHK(resolve_y(m, y, y_on_device, d.R, st, &yd));
  const BatchPlan p = plan_batch(m, d);
  CHK(presize(m, d, p));
  const IdxMap& x = p.x;
  const int F = m->F, L = m->L;
  if (is_wide(m)) {
    // one weight-gradient launch per layer: phase 0 = forward, decision MLP backward, the Dense layers' gradients; phase k =
    // the data gradient handed down by stage s + 1 (not before: the all-reduce of the bucket a phase completes starts when the
    // phase's LAST launch is done), the transposed aggregation and the weight gradient of stage s = L + 1 - k
    if (phase > 0 && !m->phase0_done) FAIL(m, V2X_ESTATE, "forward_backward_phase: phase %d before phase 0", phase);
    BwdCall c;
    c.bucketed = c.phased = true;
    CHK(run_maybe_graph(m, st, make_key(20 + phase, d, yd, n_global), [&]() -> int {
      int64_t rb, re;
      phase_bucket_range(m, phase, &rb, &re);
      if (phase == 0) {
        CHK(run_forward(m, st, d, p, true));
        CHK(backward_mlp(m, st, d, p, c, yd, n_global));
        return launch_reduce_adam(m, st, 1, false, nullptr, LossJob{0, 0, 0, 0.f, 0}, -1, false, rb, re);
      }
      const int s = L + 1 - phase;
      if (s < L) CHK(launch_dgrad(m, st, s + 1, x, m->dpre[s + 1], m->gha));
      CHK(launch_agg(m, st, d, p.dense_agg, m->N, F, m->gha + F, 2 * F, m->gha, 2 * F, (s < L) ? m->h[s] : nullptr, m->dpre[s], 1));
      CHK(wide_wgrad_gnn(m, st, s, x, d.xe, s ? m->h[s - 1] : nullptr, s ? m->a[s - 1] : d.nbr, m->dpre[s]));
      const bool last = s == 0;
      if (m->gnn[s].n_slabs > 0 || last)
        return launch_reduce_adam(m, st, 1, false, nullptr, last ? loss_job(m, d, n_global) : LossJob{0, 0, 0, 0.f, 0}, -1, false, rb, re);
      return V2X_OK;
    }));
    if (phase == 0) m->phase0_done = true;
    return phase == n_phase_buckets(m) - 1 ? emit_loss(m, loss_out, loss_on_device, st) : V2X_OK;
  }
  BwdCall c;
  c.phased = true;           // Dense-0's weight gradient stays in the MLP launch, a ragged data chain runs layer by layer (run_backward follows the plan)
  if (phase == 0) {
    CHK(run_maybe_graph(m, st, make_key(5, d, yd, n_global), [&]() -> int {
      CHK(run_forward(m, st, d, p, false));              // narrow: the MLP runs inside its training launch
      CHK(backward_mlp(m, st, d, p, c, yd, n_global));
      return launch_reduce_adam(m, st, 1, false, nullptr, LossJob{0, 0, 0, 0.f, 0}, 0);
    }));
    m->phase0_done = true;
    return V2X_OK;
  }
  if (!m->phase0_done) FAIL(m, V2X_ESTATE, "forward_backward_phase: phase 1 before phase 0");
  CHK(run_maybe_graph(m, st, make_key(6, d, yd, n_global), [&]() -> int {
    CHK(backward_graph_layers(m, st, d, p, c));
    return launch_reduce_adam(m, st, 1, false, nullptr, loss_job(m, d, n_global), 1);
  }));
  return emit_loss(m, loss_out, loss_on_device, st);
}

int v2x_grad_bucket_count(const v2x_model* m) { return m ? n_phase_buckets(m) : 0; }

int64_t v2x_grad_bucket(const v2x_model* m, int bucket, int64_t* offset) {
  if (!m || bucket < 0 || bucket >= n_phase_buckets(m)) return 0;
  int64_t b, e;
  phase_bucket_range(m, bucket, &b, &e);
  if (offset) *offset = b;
  return e - b;
}

int v2x_apply_gradients_range(v2x_model* m, int64_t offset, int64_t count, int advance_iteration, void* stream) {
  if (!m) FAIL(m, V2X_EINVAL, "null model");
  if (offset < 0 || count <= 0 || offset + count > m->P || (offset & 3) || (count & 3))
    FAIL(m, V2X_EINVAL, "apply_gradients_range: [%lld, +%lld) must lie inside the %lld parameters and be float4-aligned",
         (long long)offset, (long long)count, (long long)m->P);
  HIPCHK(m, hipSetDevice(m->cfg.device));
  return launch_reduce_adam(m, (hipStream_t)stream, 0, true, nullptr, LossJob{0, 0, 0, 0.f, 0}, -1, false, offset, offset + count,
                            advance_iteration != 0);
}

int v2x_forward_call(void* closure) {
  v2x_forward_closure* c = (v2x_forward_closure*)closure;
  v2x_model* nullm = nullptr;
  if (!c) FAIL(nullm, V2X_EINVAL, "forward_call: null closure");
  return v2x_forward(c->m, &c->b, c->q_out, c->q_on_device, c->stream);
}

int v2x_train_step(v2x_model* m, const v2x_batch* b, const float* y, int y_on_device, int32_t n_graphs_global,
                   float* loss_out, int loss_on_device, void* stream) {
  return fwd_bwd(m, b, y, y_on_device, n_graphs_global, loss_out, loss_on_device, stream, true);
}

int v2x_forward_backward(v2x_model* m, const v2x_batch* b, const float* y, int y_on_device, int32_t n_graphs_global,
                         float* loss_out, int loss_on_device, void* stream) {
  return fwd_bwd(m, b, y, y_on_device, n_graphs_global, loss_out, loss_on_device, stream, false);
}

// One DQN replay step (Agent.replay, BS_brain.py:555-748) in a single call: target forward on s', online forward on s
// (its activations are kept), y = q with the taken action's entry replaced by r + gamma * max q', then backward +
// Adam on the online network WITHOUT a second forward of the graph layers (predict + fit would run them twice).
// comm: the data-parallel form, v2x_dqn_step_dp (dp_native.hpp); NULL on one GPU
static int dp_dqn_collectives(v2x_model* m, const v2x_comm* comm, bool want_loss, hipStream_t st);
static int dqn_step(v2x_model* online, v2x_model* target, const v2x_batch* s, const v2x_batch* s_next, const int32_t* action,
                    const double* reward, double gamma, int32_t n_graphs_global, float* y_out, float* loss_out,
                    int loss_on_device, void* stream, const v2x_comm* comm) {
  v2x_model* m = online;
  if (!online || !target || !action || !reward) FAIL(m, V2X_EINVAL, "dqn_step: null argument");
  if (online == target) FAIL(m, V2X_EINVAL, "dqn_step: online and target must be different models");
  // ragged form: two variable_graphs models on batches of graphs of different sizes (one reward per graph, one action per row)
  const bool ragged = online->cfg.variable_graphs != 0;
  if (ragged != (target->cfg.variable_graphs != 0))
    FAIL(m, V2X_EINVAL, "dqn_step: online and target must both be variable_graphs models or both fixed-size (online %s, target %s)",
         ragged ? "variable" : "fixed", ragged ? "fixed" : "variable");
  if (target->N != online->N || target->F != online->F || target->L != online->L ||
      target->S != online->S || target->cfg.device != online->cfg.device)
    FAIL(m, V2X_EINVAL, "dqn_step: two models of the same shape on the same device are required");
  if (!s || !s_next || !s->on_device || !s_next->on_device) FAIL(m, V2X_EINVAL, "dqn_step takes device-resident batches");
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(m, hipSetDevice(online->cfg.device));
  DevBatch ds, dn;
  CHK(resolve_batch(online, s, &ds, st));
  if (int rc = resolve_batch(target, s_next, &dn, st)) { online->err = target->err; return rc; }
  if (dn.R != ds.R) FAIL(m, V2X_EINVAL, "dqn_step: s and s' have different sizes");
  // a transition's s and s' are the same links: ONE offset array (the graph's key has a slot for one, and bakes it in)
  if (ragged && dn.goff != ds.goff)
    FAIL(m, V2X_EINVAL, "dqn_step: s_next->graph_off must be the same device pointer as s->graph_off (s and s' of a transition are the same links)");
  if (ragged && dn.B != ds.B) FAIL(m, V2X_EINVAL, "dqn_step: s and s' have different numbers of graphs (%d, %d)", ds.B, dn.B);
  if (n_graphs_global <= 0) n_graphs_global = ragged ? ds.R : ds.B;          // a variable_graphs model counts node rows
  const BatchPlan po = plan_batch(online, ds), pt = plan_batch(target, dn);
  CHK(presize(online, ds, po));
  if (int rc = presize(target, dn, pt)) { online->err = target->err; return rc; }
  CHK(ensure(online, online->st_y, (size_t)ds.R * online->C * sizeof(float)));
  float* y = y_out ? y_out : (float*)online->st_y.p;
  // Everything up to the slab reduction is one replayable hipGraph (the Adam launch stays outside: lr_t changes per
  // step).  The key holds every pointer the launches bake in -- both batches, action / reward / target buffers and the
  // TARGET model's workspace, whose re-allocation must not leave a stale graph in the online model's cache.
  GraphKey key = make_key(4, ds, y, n_graphs_global);
  key.ptrs[6] = dn.xe; key.ptrs[7] = dn.rp; key.ptrs[8] = dn.ci; key.ptrs[9] = action; key.ptrs[10] = reward;
  key.ptrs[11] = target->q;
  key.gen = target->ws_gen;                              // the graph bakes in EVERY workspace pointer of the target (h, a, z,
  key.scalar = gamma;                                    // masks, ...), not q only
  // Narrow models (k_mlp_train_wg): the online network's decision MLP runs ONCE, inside the training launch, which forms the
  // targets from its own forward output (MlpArgs::tq) -- as Keras' fit re-computes the prediction it was handed as target, so
  // that the untouched entries carry exactly zero error (BS_brain.py:664-692, :728); the separate MLP forward of the online
  // network, and the target kernel's pass over q, are gone (38 us of a 520-us step at 20 links, batch 4096).
  // Knobs::dqn_fused_targets = 0: the three-launch form (forward, k_dqn_targets, training launch on y).
  const bool fuse_targets = online->knobs.dqn_fused_targets && po.mlp_wg && online->C == 4;
  const dim3 ragged_grid((ds.B + DQN_RAGGED_GRAPHS_PER_WG - 1) / DQN_RAGGED_GRAPHS_PER_WG);      // ragged: one wave per graph
  CHK(run_maybe_graph(online, st, key, [&]() -> int {
    target->capturing = online->capturing;
    int rc = run_forward(target, st, dn, pt, true);
    target->capturing = false;
    if (rc) { online->err = target->err; return rc; }
    if (!fuse_targets) {
      CHK(run_forward(online, st, ds, po, true));
      if (ragged)
        hipLaunchKernelGGL(k_dqn_targets_ragged, ragged_grid, dim3(256), 0, st, online->q, target->q, action, reward, gamma, ds.goff,
                           ds.B, ds.R, online->C, y);
      else
        hipLaunchKernelGGL(k_dqn_targets, dim3((ds.R + 255) / 256), dim3(256), 0, st, online->q, target->q, action, reward, gamma,
                           ds.R, online->N, online->C, y);
      return run_backward(online, st, ds, po, BwdCall{}, y, n_graphs_global);
    }
    CHK(run_forward(online, st, ds, po, false));                           // graph layers only
    float* tq = online->dq;                                                // (a workspace this path does not use otherwise: [R][4])
    if (ragged)
      hipLaunchKernelGGL(k_dqn_tq_ragged, ragged_grid, dim3(256), 0, st, target->q, action, reward, gamma, ds.goff, ds.B, ds.R, online->C, tq);
    else
      hipLaunchKernelGGL(k_dqn_tq, dim3((ds.R + 255) / 256), dim3(256), 0, st, target->q, action, reward, gamma, ds.R, online->N, online->C, tq);
    BwdCall c;
    c.tq = tq; c.y_out = y;
    return run_backward(online, st, ds, po, c, y, n_graphs_global);
  }));
  if (!comm) {
    CHK(launch_reduce_adam(online, st, 1, true, nullptr, loss_job(online, ds, n_graphs_global)));
  } else {
    // data parallelism: the slab sums and the losses, the collectives (eager, never captured), then Adam alone
    CHK(launch_reduce_adam(online, st, 1, false, nullptr, loss_job(online, ds, n_graphs_global)));
    CHK(dp_dqn_collectives(online, comm, loss_out != nullptr, st));
    CHK(launch_reduce_adam(online, st, 0, true, nullptr));
  }
  online->phase0_done = target->phase0_done = false;
  return emit_loss(online, loss_out, loss_on_device, st);
}

int v2x_dqn_step(v2x_model* online, v2x_model* target, const v2x_batch* s, const v2x_batch* s_next, const int32_t* action,
                 const double* reward, double gamma, int32_t n_graphs_global, float* y_out, float* loss_out,
                 int loss_on_device, void* stream) {
  return dqn_step(online, target, s, s_next, action, reward, gamma, n_graphs_global, y_out, loss_out, loss_on_device, stream,
                  nullptr);
}

int v2x_apply_gradients(v2x_model* m, void* stream) {
  if (!m) FAIL(m, V2X_EINVAL, "null model");
  HIPCHK(m, hipSetDevice(m->cfg.device));
  return launch_reduce_adam(m, (hipStream_t)stream, 0, true, nullptr);
}

// ---------------------------------------------------------------------------- per-kernel entry points
static int batch_dev_only(const v2x_batch* b, DevBatch* d) {
  v2x_model* nullm = nullptr;
  if (!b || !b->on_device) FAIL(nullm, V2X_EINVAL, "per-kernel entry points take device-resident batches");
  if (!b->row_ptr || b->n_graphs <= 0 || b->n_rows <= 0 || b->max_nodes <= 0) FAIL(nullm, V2X_EINVAL, "batch: bad sizes");
  d->B = b->n_graphs; d->R = b->n_rows; d->E = b->n_edges; d->max_nodes = b->max_nodes; d->max_edges = b->max_edges;
  d->xe = b->xe; d->nbr = b->nbr_init; d->goff = b->graph_off; d->rp = b->row_ptr; d->ci = b->col_idx;
  return V2X_OK;
}

int v2x_agg_fwd(const v2x_batch* b, int32_t n_nodes, int32_t feat_dim, const float* h, float* out, void* stream) {
  DevBatch d;
  CHK(batch_dev_only(b, &d));
  return launch_agg(nullptr, (hipStream_t)stream, d, use_dense_agg(process_knobs(), d, feat_dim), n_nodes, feat_dim, h, feat_dim, nullptr, 0, nullptr, out, 0);
}

int v2x_agg_bwd(const v2x_batch* b, int32_t n_nodes, int32_t feat_dim, const float* g, float* out, void* stream) {
  DevBatch d;
  CHK(batch_dev_only(b, &d));
  return launch_agg(nullptr, (hipStream_t)stream, d, use_dense_agg(process_knobs(), d, feat_dim), n_nodes, feat_dim, g, feat_dim, nullptr, 0, nullptr, out, 1);
}

int v2x_node_update_fwd(v2x_model* m, int32_t stage, int32_t n_rows, const float* xe, const float* h_prev,
                        const float* agg_prev, float* out, void* stream) {
  if (!m || !xe || !out || stage < 0 || stage > m->L || n_rows <= 0) FAIL(m, V2X_EINVAL, "node_update_fwd: bad argument");
  if (m->S > 1 && n_rows % m->N) FAIL(m, V2X_EINVAL, "node_update_fwd: n_rows not a multiple of n_nodes");
  return launch_node_fwd(m, (hipStream_t)stream, stage, idx_map_rows(m, n_rows), xe, h_prev, agg_prev, out);
}

static int copy_cols(v2x_model* m, float* dst, int dst_w, const float* src, int src_w, int col, int rows, hipStream_t st) {
  HIPCHK(m, hipMemcpy2DAsync(dst, (size_t)dst_w * 4, src + col, (size_t)src_w * 4, (size_t)dst_w * 4, rows,
                             hipMemcpyDeviceToDevice, st));
  return V2X_OK;
}

int v2x_node_update_bwd(v2x_model* m, int32_t stage, int32_t n_rows, const float* xe, const float* h_prev,
                        const float* agg_prev, const float* dpre, float* dh_prev, float* dagg_prev, float* grad_out,
                        void* stream) {
  if (!m || !xe || !dpre || stage < 0 || stage > m->L || n_rows <= 0) FAIL(m, V2X_EINVAL, "node_update_bwd: bad argument");
  if (m->S > 1 && n_rows % m->N) FAIL(m, V2X_EINVAL, "node_update_bwd: n_rows not a multiple of n_nodes");
  hipStream_t st = (hipStream_t)stream;
  CHK(presize_rows(m, n_rows));
  const IdxMap x = idx_map_rows(m, n_rows);
  CHK(wgrad_gnn(m, st, stage, x, xe, h_prev, agg_prev, dpre));
  if (grad_out) CHK(launch_reduce_adam(m, st, 1, false, grad_out));
  if (stage > 0 && (dh_prev || dagg_prev)) {
    CHK(launch_dgrad(m, st, stage, x, dpre, m->gha));
    if (dh_prev) CHK(copy_cols(m, dh_prev, m->F, m->gha, 2 * m->F, 0, n_rows, st));
    if (dagg_prev) CHK(copy_cols(m, dagg_prev, m->F, m->gha, 2 * m->F, m->F, n_rows, st));
  }
  return V2X_OK;
}

int v2x_mlp_fwd(v2x_model* m, int32_t n_rows, const float* xe, const float* h, const float* agg, float* q_out, void* stream) {
  if (!m || !xe || !h || !agg || !q_out || n_rows <= 0) FAIL(m, V2X_EINVAL, "mlp_fwd: bad argument");
  hipStream_t st = (hipStream_t)stream;
  CHK(ensure_rows(m, n_rows));
  MlpArgs a;
  mlp_args(m, a, idx_map_rows(m, n_rows), xe, h, agg);
  CHK(launch_mlp(m, st, a, false));
  HIPCHK(m, hipMemcpyAsync(q_out, m->q, (size_t)n_rows * m->C * 4, hipMemcpyDeviceToDevice, st));
  return V2X_OK;
}

int v2x_mlp_huber_bwd(v2x_model* m, int32_t n_rows, int32_t n_global, const float* xe, const float* h, const float* agg,
                      const float* y, float* dh, float* dagg, float* grad_out, float* loss_out, void* stream) {
  if (!m || !xe || !h || !agg || !y || n_rows <= 0) FAIL(m, V2X_EINVAL, "mlp_huber_bwd: bad argument");
  hipStream_t st = (hipStream_t)stream;
  CHK(presize_rows(m, n_rows));
  const IdxMap x = idx_map_rows(m, n_rows);
  if (n_global <= 0) n_global = m->cfg.variable_graphs ? n_rows : n_rows / m->N;
  MlpArgs a;
  mlp_args(m, a, x, xe, h, agg);
  a.y = y;
  a.inv_denom = 1.0f / loss_denominator(m, n_global);
  if (mlp_wg_path(m)) {
    CHK(launch_mlp_train_wg(m, st, a));
  } else {
    CHK(launch_mlp(m, st, a, false));
    CHK(launch_mlp(m, st, a, true));
    CHK(wgrad_mlp(m, st, x, xe, h, agg));
  }
  if (grad_out) CHK(launch_reduce_adam(m, st, 1, false, grad_out));
  if (dh) CHK(copy_cols(m, dh, m->F, m->gha, 2 * m->F, 0, n_rows, st));
  if (dagg) CHK(copy_cols(m, dagg, m->F, m->gha, 2 * m->F, m->F, n_rows, st));
  if (loss_out) {
    if (m->cfg.variable_graphs)
      hipLaunchKernelGGL(k_loss_reduce, dim3(1), dim3(256), 0, st, m->rowloss, m->loss_dev, n_rows, 1, (int64_t)0, a.inv_denom);
    else
      hipLaunchKernelGGL(k_loss_reduce, dim3(m->N), dim3(256), 0, st, m->rowloss, m->loss_dev, n_rows / m->N,
                         m->S == 1 ? m->N : 1, m->S == 1 ? (int64_t)1 : srow_stride(m), a.inv_denom);
    HIPCHK(m, hipMemcpyAsync(loss_out, m->loss_dev, (m->cfg.variable_graphs ? 1 : m->N) * sizeof(float),
                             hipMemcpyDeviceToDevice, st));
  }
  return V2X_OK;
}

int v2x_adam_step(float* param, const float* grad, float* mom, float* vel, int64_t n, int64_t iteration, float lr,
                  float beta1, float beta2, float eps, void* stream) {
  v2x_model* nullm = nullptr;
  if (!param || !grad || !mom || !vel || n <= 0 || iteration < 1) FAIL(nullm, V2X_EINVAL, "adam_step: bad argument");
  const double t = (double)iteration;
  const float lr_t = (float)(lr * std::sqrt(1.0 - std::pow((double)beta2, t)) / (1.0 - std::pow((double)beta1, t)));
  int blocks = (int)((n + 255) / 256);
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(k_adam_scalar, dim3(blocks), dim3(256), 0, (hipStream_t)stream, param, grad, mom, vel, n, lr_t,
                     beta1, beta2, eps);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) FAIL(nullm, V2X_EHIP, "adam launch failed: %s", hipGetErrorString(e));
  return V2X_OK;
}

// ---------------------------------------------------------------------------- DQN replay glue
int v2x_device_addressable(const void* p) {
  v2x_model* nullm = nullptr;
  if (!p) FAIL(nullm, V2X_EINVAL, "device_addressable: null pointer");
  hipPointerAttribute_t at;
  hipError_t e = hipPointerGetAttributes(&at, p);
  if (e != hipSuccess) { (void)hipGetLastError(); return 0; }     // unknown to the runtime: pageable host memory
  if (at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged) return 1;
  if (at.type == hipMemoryTypeHost) return at.devicePointer == p ? 1 : 0;
  return 0;
}

int v2x_gather_rows(const void* src, const int32_t* idx, void* dst, int64_t n_idx, int64_t row_bytes, void* stream) {
  v2x_model* nullm = nullptr;
  if (!src || !idx || !dst || n_idx <= 0 || row_bytes <= 0 || (row_bytes & 3))
    FAIL(nullm, V2X_EINVAL, "gather_rows: null pointer, empty selection or row_bytes not a multiple of 4");
  const int64_t words = row_bytes / 4;
  const bool vec = (row_bytes & 15) == 0 && ((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 15) == 0;
  const int64_t total = n_idx * (vec ? words / 4 : words);
  int blocks = (int)std::min<int64_t>((total + 255) / 256, 8192);
  if (vec)
    hipLaunchKernelGGL(k_gather_rows<4>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const uint32_t*)src, idx,
                       (uint32_t*)dst, n_idx, words);
  else
    hipLaunchKernelGGL(k_gather_rows<1>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const uint32_t*)src, idx,
                       (uint32_t*)dst, n_idx, words);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) FAIL(nullm, V2X_EHIP, "gather_rows launch failed: %s", hipGetErrorString(e));
  return V2X_OK;
}

int v2x_gather_rows_multi(int32_t n_jobs, const void* const* src, void* const* dst, const int64_t* row_bytes, const int32_t* idx,
                          int64_t n_idx, void* stream) {
  v2x_model* nullm = nullptr;
  if (n_jobs < 1 || n_jobs > GATHER_MAX_JOBS || !src || !dst || !row_bytes || !idx || n_idx <= 0)
    FAIL(nullm, V2X_EINVAL, "gather_rows_multi: 1..%d jobs, non-null arrays, a non-empty selection", GATHER_MAX_JOBS);
  GatherJobs jobs;
  memset(&jobs, 0, sizeof(jobs));
  int64_t most = 0;
  for (int j = 0; j < n_jobs; ++j) {
    if (!src[j] || !dst[j] || row_bytes[j] <= 0 || (row_bytes[j] & 3)) FAIL(nullm, V2X_EINVAL, "gather_rows_multi: job %d: null pointer or row_bytes not a multiple of 4", j);
    jobs.src[j] = (const uint32_t*)src[j]; jobs.dst[j] = (uint32_t*)dst[j]; jobs.words[j] = row_bytes[j] / 4;
    jobs.vec[j] = ((row_bytes[j] & 15) == 0 && ((uintptr_t)src[j] & 15) == 0 && ((uintptr_t)dst[j] & 15) == 0) ? 1 : 0;
    most = std::max(most, n_idx * (jobs.vec[j] ? jobs.words[j] / 4 : jobs.words[j]));
  }
  const int blocks = (int)std::min<int64_t>((most + 255) / 256, 2048);
  hipLaunchKernelGGL(k_gather_rows_multi, dim3(blocks, n_jobs), dim3(256), 0, (hipStream_t)stream, jobs, idx, n_idx);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) FAIL(nullm, V2X_EHIP, "gather_rows_multi launch failed: %s", hipGetErrorString(e));
  return V2X_OK;
}

int v2x_q_stats(const float* y, int32_t n_graphs, int32_t n_nodes, int32_t n_channels, double* out, void* stream) {
  v2x_model* nullm = nullptr;
  if (!y || !out || n_graphs <= 0 || n_nodes <= 0 || n_channels <= 0) FAIL(nullm, V2X_EINVAL, "q_stats: bad argument");
  // scratch of the two-level sum: per (device, stream) -- launches on one stream are ordered, two streams must not share the
  // arrival counters --, grown on demand, zeroed when allocated (the kernel re-arms its counters)
  static std::mutex mu;
  static std::map<std::pair<int, void*>, std::pair<void*, int>> scratch;          // -> (buffer, links it holds)
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) FAIL(nullm, V2X_EHIP, "q_stats: no device");
  double* part = nullptr;
  unsigned* cnt = nullptr;
  {
    std::lock_guard<std::mutex> lk(mu);
    auto& e = scratch[std::make_pair(dev, stream)];
    if (e.second < n_nodes) {
      if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) FAIL(nullm, V2X_EHIP, "q_stats: synchronise failed");
      if (e.first) (void)hipFree(e.first);
      const int cap = std::max(n_nodes, 64);
      const size_t bytes = (size_t)cap * QS_PARTS * 2 * sizeof(double) + (size_t)cap * sizeof(unsigned);
      if (hipMalloc(&e.first, bytes) != hipSuccess) { e.first = nullptr; e.second = 0; FAIL(nullm, V2X_ENOMEM, "q_stats: scratch"); }
      if (hipMemset(e.first, 0, bytes) != hipSuccess) FAIL(nullm, V2X_EHIP, "q_stats: memset failed");
      e.second = cap;
    }
    part = (double*)e.first;
    cnt = (unsigned*)(part + (size_t)e.second * QS_PARTS * 2);
  }
  hipLaunchKernelGGL(k_q_stats, dim3(n_nodes, QS_PARTS), dim3(256), 0, (hipStream_t)stream, y, n_graphs, n_nodes, n_channels, out, part, cnt);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) FAIL(nullm, V2X_EHIP, "q_stats launch failed: %s", hipGetErrorString(e));
  return V2X_OK;
}

int v2x_dqn_targets(const float* q, const float* q_next, const int32_t* action, const double* reward, double gamma,
                    int32_t n_graphs, int32_t n_nodes, int32_t n_channels, float* y_out, void* stream) {
  v2x_model* nullm = nullptr;
  if (!q || !q_next || !action || !reward || !y_out || n_graphs <= 0 || n_nodes <= 0 || n_channels <= 0)
    FAIL(nullm, V2X_EINVAL, "dqn_targets: bad argument");
  const int n_rows = n_graphs * n_nodes;
  hipLaunchKernelGGL(k_dqn_targets, dim3((n_rows + 255) / 256), dim3(256), 0, (hipStream_t)stream, q, q_next, action,
                     reward, gamma, n_rows, n_nodes, n_channels, y_out);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) FAIL(nullm, V2X_EHIP, "dqn_targets launch failed: %s", hipGetErrorString(e));
  return V2X_OK;
}

int v2x_dqn_targets_ragged(const float* q, const float* q_next, const int32_t* action, const double* reward, double gamma,
                           const int32_t* graph_off, int32_t n_graphs, int32_t n_rows, int32_t n_channels, float* y_out, void* stream) {
  v2x_model* nullm = nullptr;
  if (!q || !q_next || !action || !reward || !graph_off || !y_out || n_graphs <= 0 || n_rows <= 0 || n_channels <= 0)
    FAIL(nullm, V2X_EINVAL, "dqn_targets_ragged: bad argument");
  hipLaunchKernelGGL(k_dqn_targets_ragged, dim3((n_graphs + DQN_RAGGED_GRAPHS_PER_WG - 1) / DQN_RAGGED_GRAPHS_PER_WG), dim3(256), 0,
                     (hipStream_t)stream, q, q_next, action, reward, gamma, graph_off, n_graphs, n_rows, n_channels, y_out);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) FAIL(nullm, V2X_EHIP, "dqn_targets_ragged launch failed: %s", hipGetErrorString(e));
  return V2X_OK;
}

int v2x_replay_gather_mixed(int32_t n_pools, const v2x_replay_pool* pools, const v2x_mixed_batch* out, void* stream) {
  v2x_model* nullm = nullptr;
  if (n_pools < 1 || n_pools > MIXED_MAX_POOLS || !pools || !out)
    FAIL(nullm, V2X_EINVAL, "replay_gather_mixed: 1..%d pools, non-null pool table and output struct", MIXED_MAX_POOLS);
  if (!out->xe || !out->xe_next || !out->action || !out->reward || !out->graph_off || !out->row_ptr || !out->col_idx)
    FAIL(nullm, V2X_EINVAL, "replay_gather_mixed: a null output pointer");
  if (((uintptr_t)out->xe & 15) || ((uintptr_t)out->xe_next & 15))
    FAIL(nullm, V2X_EINVAL, "replay_gather_mixed: out->xe / out->xe_next must be 16-byte aligned");
  MixedArgs a;
  memset(&a, 0, sizeof(a));
  int64_t B = 0, R = 0, E = 0;
  for (int k = 0; k < n_pools; ++k) {
    const v2x_replay_pool& p = pools[k];
    if (p.n_nodes < 3 || p.n_nodes > 31) FAIL(nullm, V2X_EINVAL, "replay_gather_mixed: pool %d: n_nodes %d outside 3..31", k, p.n_nodes);
    if (p.count < 0) FAIL(nullm, V2X_EINVAL, "replay_gather_mixed: pool %d: negative count %d", k, p.count);
    if (p.count > 0 && (!p.xe || !p.xe_next || !p.col || !p.action || !p.reward || !p.idx))
      FAIL(nullm, V2X_EINVAL, "replay_gather_mixed: pool %d contributes %d graphs but has a null pointer", k, p.count);
    if (p.count > 0 && (((uintptr_t)p.xe & 15) || ((uintptr_t)p.xe_next & 15)))
      FAIL(nullm, V2X_EINVAL, "replay_gather_mixed: pool %d: xe / xe_next must be 16-byte aligned", k);
    if (R > INT32_MAX || E > INT32_MAX) break;           // (reported below; the bases are ints)
    MixedPool& q = a.p[k];
    q.xe = p.xe; q.xe_next = p.xe_next; q.col = p.col; q.action = p.action; q.reward = p.reward; q.idx = p.idx;
    q.n = p.n_nodes; q.gbase = (int)B; q.rbase = (int)R; q.ebase = (int)E;
    B += p.count;
    R += (int64_t)p.count * p.n_nodes;
    E += (int64_t)p.count * p.n_nodes * (p.n_nodes - 2);
  }
  if (R >= INT32_MAX || E >= INT32_MAX)
    FAIL(nullm, V2X_EINVAL, "replay_gather_mixed: the batch's rows or edges do not fit int32");
  if (B == 0) FAIL(nullm, V2X_EINVAL, "replay_gather_mixed: the pools' counts sum to 0");
  a.xe = out->xe; a.xe_next = out->xe_next; a.action = out->action; a.reward = out->reward;
  a.graph_off = out->graph_off; a.row_ptr = out->row_ptr; a.col_idx = out->col_idx;
  a.n_pools = n_pools; a.B = (int)B; a.R = (int)R; a.E = (int)E;
  hipLaunchKernelGGL(k_replay_gather_mixed, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) FAIL(nullm, V2X_EHIP, "replay_gather_mixed launch failed: %s", hipGetErrorString(e));
  return V2X_OK;
}

int v2x_replay_gather_recv(const v2x_replay_recv* src, const v2x_mixed_batch* out, void* stream) {
  v2x_model* nullm = nullptr;
  if (!src || !out) FAIL(nullm, V2X_EINVAL, "replay_gather_recv: null source or output struct");
  if (src->n_nodes < 3 || src->n_nodes > RECV_MAX_LINKS)
    FAIL(nullm, V2X_EINVAL, "replay_gather_recv: n_nodes %d outside 3..%d", src->n_nodes, RECV_MAX_LINKS);
  if (src->count < 1) FAIL(nullm, V2X_EINVAL, "replay_gather_recv: count %d, at least 1 sampled transition", src->count);
  if (!src->xe || !src->xe_next || !src->recv || !src->action || !src->reward || !src->idx)
    FAIL(nullm, V2X_EINVAL, "replay_gather_recv: a null source pointer (only edge_base may be null)");
  if (!out->xe || !out->xe_next || !out->action || !out->reward || !out->row_ptr || !out->col_idx)
    FAIL(nullm, V2X_EINVAL, "replay_gather_recv: a null output pointer (only graph_off may be null)");
  if (((uintptr_t)src->xe & 15) || ((uintptr_t)src->xe_next & 15) || ((uintptr_t)out->xe & 15) || ((uintptr_t)out->xe_next & 15))
    FAIL(nullm, V2X_EINVAL, "replay_gather_recv: xe / xe_next of the source and of the output must be 16-byte aligned");
  const int64_t n = src->n_nodes, K = src->count;
  if (K * n > INT32_MAX || K * n * (n - 1) > INT32_MAX)
    FAIL(nullm, V2X_EINVAL, "replay_gather_recv: the batch's rows (%lld) or edges (up to %lld) do not fit int32", (long long)(K * n),
         (long long)(K * n * (n - 1)));
  RecvArgs a;
  a.xe = src->xe; a.xe_next = src->xe_next; a.recv = src->recv; a.action = src->action; a.reward = src->reward;
  a.idx = src->idx; a.edge_base = src->edge_base;
  a.oxe = out->xe; a.oxe_next = out->xe_next; a.oaction = out->action; a.oreward = out->reward;
  a.row_ptr = out->row_ptr; a.col_idx = out->col_idx;
  a.n = (int)n; a.K = (int)K; a.parts = (int)((n + RECV_ROWS_PER_WG - 1) / RECV_ROWS_PER_WG);
  hipLaunchKernelGGL(k_replay_gather_recv, dim3((unsigned)(K * a.parts)), dim3(256), 0, (hipStream_t)stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) FAIL(nullm, V2X_EHIP, "replay_gather_recv launch failed: %s", hipGetErrorString(e));
  return V2X_OK;
}

int v2x_csr_from_recv(int32_t G, int32_t E, int32_t n, const int32_t* recv, const int32_t* edge_base, int32_t* row_ptr,
                      int32_t* col_idx, void* stream) {
  v2x_model* nullm = nullptr;
  if (n < 3 || n > RECV_MAX_LINKS) FAIL(nullm, V2X_EINVAL, "csr_from_recv: n %d outside 3..%d", n, RECV_MAX_LINKS);
  if (G < 1 || E < 1) FAIL(nullm, V2X_EINVAL, "csr_from_recv: G = %d graphs over E = %d states, at least 1 of each", G, E);
  if (!recv || !row_ptr || !col_idx) FAIL(nullm, V2X_EINVAL, "csr_from_recv: a null pointer (only edge_base may be null)");
  if ((int64_t)G * n >= INT32_MAX || (int64_t)G * n * (n - 1) > INT32_MAX)
    FAIL(nullm, V2X_EINVAL, "csr_from_recv: the batch's rows (%lld) or edges (up to %lld) do not fit int32", (long long)G * n,
         (long long)G * n * (n - 1));
  CsrRecvArgs a;
  a.recv = recv; a.edge_base = edge_base; a.row_ptr = row_ptr; a.col_idx = col_idx;
  a.n = n; a.G = G; a.E = E; a.parts = (n + RECV_ROWS_PER_WG - 1) / RECV_ROWS_PER_WG;
  hipLaunchKernelGGL(k_csr_from_recv, dim3((unsigned)((int64_t)G * a.parts)), dim3(256), 0, (hipStream_t)stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) FAIL(nullm, V2X_EHIP, "csr_from_recv launch failed: %s", hipGetErrorString(e));
  return V2X_OK;
}

// ---------------------------------------------------------------------------- dict payload -> packed host batch
int v2x_pack_feed(const v2x_feed* f, int check_kron, float* xe_out, int32_t* row_ptr_out, int32_t* col_idx_out,
                  float* nbr_out, int32_t* info_out) {
  v2x_model* nullm = nullptr;
  if (!f || !xe_out || !row_ptr_out || !col_idx_out || !info_out || !f->node || !f->edge || !f->is_f64 || !f->adjacency)
    FAIL(nullm, V2X_EINVAL, "pack_feed: null argument");
  if (f->n_graphs <= 0 || f->n_nodes <= 0 || f->feat_dim <= 0 || f->node_in <= 0 || f->edge_in < 0 ||
      f->node_in + f->edge_in > XE)
    FAIL(nullm, V2X_EINVAL, "pack_feed: bad sizes (node_in + edge_in must fit the %d-wide packed row)", XE);
  if ((int64_t)f->n_graphs * f->n_nodes * f->n_nodes > INT32_MAX) FAIL(nullm, V2X_EINVAL, "pack_feed: batch too large");
  for (int k = 0; k < f->n_nodes; ++k)
    if (!f->node[k] || !f->edge[k] || (f->nbr && !f->nbr[k])) FAIL(nullm, V2X_EINVAL, "pack_feed: null input array");
  v2x_host::FeedView v{f->n_graphs, f->n_nodes, f->feat_dim, f->node_in, f->edge_in, f->node, f->edge, f->nbr, f->is_f64, f->adjacency};
  int bad = -1;
  const int rc = v2x_host::pack_feed(v, check_kron != 0, xe_out, row_ptr_out, col_idx_out, nbr_out, info_out, &bad);
  if (rc == v2x_host::PACK_NOT_01)
    FAIL(nullm, V2X_EINVAL, "adjacency entries must be 0 or 1 (the engine aggregates unweighted edges); sample %d", bad);
  if (rc == v2x_host::PACK_NOT_KRON) FAIL(nullm, V2X_EINVAL, "Adjacency_Matrix is not kron(Adj, I_F) (sample %d)", bad);
  return V2X_OK;
}

// ---------------------------------------------------------------------------- contract checks
int v2x_validate_batch(v2x_model* m, const v2x_batch* b, int32_t n_nodes, void* stream) {
  if (!b || b->n_graphs <= 0 || b->n_rows <= 0 || !b->row_ptr || (b->n_edges > 0 && !b->col_idx) || b->max_nodes <= 0 ||
      b->max_edges < 0)
    FAIL(m, V2X_EINVAL, "validate_batch: null pointer or non-positive size");
  if (m) n_nodes = m->N;
  if (!b->graph_off && (n_nodes <= 0 || (int64_t)b->n_graphs * n_nodes != b->n_rows))
    FAIL(m, V2X_EINVAL, "validate_batch: n_rows (%d) != n_graphs*n_nodes (%d*%d)", b->n_rows, b->n_graphs, n_nodes);
  if (!b->on_device) return validate_host_batch(m, b, n_nodes);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_validate_batch, dim3(std::min(b->n_graphs, 4096)), dim3(256), 0, st, b->graph_off, b->row_ptr, b->col_idx,
                     b->n_graphs, b->n_rows, b->n_edges, n_nodes, b->max_nodes, b->max_edges, flag_dev_of(m));
  HIPCHK(m, hipGetLastError());
  HIPCHK(m, hipStreamSynchronize(st));
  return check_flag(m);
}

int v2x_reset_exchange(v2x_model* m) {
  if (!m) FAIL(m, V2X_EINVAL, "null model");
  HIPCHK(m, hipSetDevice(m->cfg.device));
  return reset_exchange(m);
}

void* v2x_debug_exchange_counters(v2x_model* m) { return m ? (void*)m->small_sync : nullptr; }
void* v2x_debug_split_counters(v2x_model* m, int32_t* n_tiles) {
  if (n_tiles) *n_tiles = m ? m->xchg_cap_tiles : 0;
  return m ? (void*)m->xchg_sync : nullptr;
}

int v2x_check_errors(v2x_model* m, void* stream) {
  HIPCHK(m, hipStreamSynchronize((hipStream_t)stream));
  return check_flag(m);
}

// ---------------------------------------------------------------------------- measurement
int v2x_path_info(v2x_model* m, const v2x_batch* b, char* out, int cap) {
  if (!m || !b || !out || cap < 16) FAIL(m, V2X_EINVAL, "path_info: bad argument");
  DevBatch d;
  memset(&d, 0, sizeof(d));
  d.B = b->n_graphs; d.R = b->n_rows; d.E = b->n_edges; d.max_nodes = b->max_nodes; d.max_edges = b->max_edges;
  d.goff = b->graph_off; d.nbr = b->nbr_init;
  const BatchPlan p = plan_batch(m, d);
  const bool fused = p.form == GraphLayers::Fused;
  // "edge-bitset-walk": what the fused kernels do with the edge index (N <= 32) -- every CSR row becomes a 32-bit set, a wave
  // walks the graph's rows in LDS once and adds each to the slots whose set holds it (sparse lanes walk their set bits only);
  // "edge-gather": the per-edge CSR gather / segment sum of k_agg (layer-wise path, any N)
  const char* agg = fused ? (p.compl_sums ? "complement" : "edge-bitset-walk")
                          : (p.dense_agg ? "dense(complement-or-mfma-per-graph)" : "edge-gather");
  char gl[48];
  if (p.split > 1) snprintf(gl, sizeof(gl), "fused(split%d)", p.split);
  else snprintf(gl, sizeof(gl), "%s", fused ? "fused" : (p.form == GraphLayers::Ragged ? "fused(ragged)" : "layerwise"));
  // dense0_dw: which launch takes Dense-0's weight gradient in a fit step -- the MLP launch itself, or (small batches) a role of
  // the graph layers' weight-gradient launch (BatchPlan::dense0_rides)
  snprintf(out, cap, "graph_layers=%s aggregation=%s mlp=%s handoff=%s dense0_dw=%s", gl, agg,
           p.mlp_wg ? "train_wg" : "fwd+bwd", p.frag_ok ? "fragment-major" : "row-major",
           p.dense0_rides ? "k_wgrad" : (p.mlp_wg ? "k_mlp_train_wg" : "k_wide_wgrad"));
  return V2X_OK;
}

int v2x_debug_phase_stamps(v2x_model* m, int64_t* out, int n) {
  if (!m || !out) FAIL(m, V2X_EINVAL, "null argument");
  if (!m->ts_buf) FAIL(m, V2X_ESTATE, "phase stamps need V2X_FUSED_TS=1 when the model is created");
  HIPCHK(m, hipDeviceSynchronize());
  HIPCHK(m, hipMemcpy(out, m->ts_buf, (size_t)std::min(n, 4 * 8 * 64) * 8, hipMemcpyDeviceToHost));
  return V2X_OK;
}

int v2x_debug_ragged_plan(v2x_model* m, int32_t* out, int n) {
  if (!m || !out || n < 0) FAIL(m, V2X_EINVAL, "null argument");
  if (!m->plan_buf.p || m->plan_len <= 0) FAIL(m, V2X_ESTATE, "no ragged fused forward has run on this model");
  HIPCHK(m, hipDeviceSynchronize());
  HIPCHK(m, hipMemcpy(out, m->plan_buf.p, (size_t)std::min(n, m->plan_len) * 4, hipMemcpyDeviceToHost));
  return m->plan_len;
}

int v2x_debug_layer_slabs(v2x_model* m, int32_t* out, int n) {
  if (!m || !out || n < 0) FAIL(m, V2X_EINVAL, "null argument");
  const int want = (int)(m->gnn.size() + m->dense.size()) + 1;
  if (n < want) FAIL(m, V2X_EINVAL, "layer_slabs: room for %d values needed", want);
  HIPCHK(m, hipDeviceSynchronize());
  int k = 0;
  for (auto* v : {&m->gnn, &m->dense})
    for (const LayerDesc& ld : *v) out[k++] = ld.n_slabs;
  out[k++] = m->reduce_groups;
  return k;
}

int v2x_wide_tiling_plan(int32_t n_idx, int32_t grid_z, int32_t n_out, int32_t slots, int32_t tail, int32_t out[4]) {
  v2x_model* m = nullptr;
  if (!out) FAIL(m, V2X_EINVAL, "wide_tiling_plan: null output");
  if (n_idx < 1 || grid_z < 1 || n_out < 1 || slots < 1 || tail < 0 || tail > 2) FAIL(m, V2X_EINVAL, "wide_tiling_plan: n_idx, grid_z, n_out, slots >= 1 and tail in 0..2");
  if (slots > (1 << 28) || ((int64_t)n_idx + WD_TM - 1) / WD_TM * grid_z * (((int64_t)n_out + 63) / 64) > (1 << 28))
    FAIL(m, V2X_EINVAL, "wide_tiling_plan: more than 2^28 slots or tiles");
  const WideTiling t = wide_tiling_plan(n_idx, grid_z, n_out, slots, tail);
  out[0] = t.ny; out[1] = t.mbs; out[2] = t.n_full_rb; out[3] = t.n_rb;
  return V2X_OK;
}

int v2x_debug_wide_tiling(v2x_model* m, int32_t* out, int n) {
  if (!m || !out || n < 0) FAIL(m, V2X_EINVAL, "null argument");
  const int nl = (int)m->wide_rec_tiles.size(), nr = (int)m->wide_rec_roles.size(), want = 2 + nl + nr;
  if (n < want) FAIL(m, V2X_EINVAL, "wide_tiling: room for %d values needed", want);
  out[0] = nl / 4; out[1] = nr / 4;
  std::copy(m->wide_rec_tiles.begin(), m->wide_rec_tiles.end(), out + 2);
  std::copy(m->wide_rec_roles.begin(), m->wide_rec_roles.end(), out + 2 + nl);
  m->wide_rec_tiles.clear(); m->wide_rec_roles.clear();
  return want;
}

int v2x_profile_enable(v2x_model* m, int enable) {
  if (!m) FAIL(m, V2X_EINVAL, "null model");
  m->prof = enable != 0;
  if (!enable) {
    for (auto& r : m->prof_recs) { hipEventDestroy(r.ev0); hipEventDestroy(r.ev1); }
    m->prof_recs.clear();
  }
  return V2X_OK;
}

int v2x_profile_read(v2x_model* m, char* names_out, int names_cap, double* ms_out, int64_t* calls_out, int max_entries) {
  if (!m || !names_out || !ms_out || !calls_out) FAIL(m, V2X_EINVAL, "profile_read: null argument");
  HIPCHK(m, hipDeviceSynchronize());
  std::vector<double> ms(m->prof_names.size(), 0.0);
  std::vector<int64_t> calls(m->prof_names.size(), 0);
  for (auto& r : m->prof_recs) {
    float t = 0.f;
    if (hipEventElapsedTime(&t, r.ev0, r.ev1) == hipSuccess) { ms[r.id] += t; calls[r.id] += 1; }
    hipEventDestroy(r.ev0); hipEventDestroy(r.ev1);
  }
  m->prof_recs.clear();
  std::string names;
  int n = 0;
  for (size_t i = 0; i < m->prof_names.size() && n < max_entries; ++i) {
    if (!calls[i]) continue;
    if ((int)(names.size() + m->prof_names[i].size() + 2) > names_cap) break;
    names += m->prof_names[i]; names += '\n';
    ms_out[n] = ms[i]; calls_out[n] = calls[i];
    ++n;
  }
  snprintf(names_out, names_cap, "%s", names.c_str());
  return n;
}

}  // extern "C"

// data parallelism driven by the library: the collective table, the RCCL table, v2x_train_step_dp, v2x_dqn_step_dp
#include "dp_native.hpp"
