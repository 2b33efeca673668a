/*
 * v2xgnn.h -- C ABI of the MI355X (gfx950) GNN message-passing engine that replaces the
 * Keras/TF1 Q-network of the reference (`/root/reference/BS_brain.py`).
 *
 * This is the drop-in boundary.  The reference has no FFI of its own
 * (it is pure Python on Keras); the entry points below are what a `ctypes` binding of the
 * reference's `BS` class needs, one per reference call site:
 *
 *   v2x_create / v2x_destroy      <- BS._create_model            BS_brain.py:108-216
 *   v2x_forward                   <- Model.predict               BS_brain.py:225-235
 *   v2x_train_step                <- Model.fit (1 step)          BS_brain.py:218-223
 *   v2x_copy_weights              <- BS.update_target_model      BS_brain.py:237-239
 *   v2x_get_weights/set_weights   <- get_weights / set_weights / save_weights / load_weights
 *                                                                BS_brain.py:239,863,869,1254
 *   v2x_gather_rows / v2x_dqn_targets / v2x_dqn_step
 *                                 <- Agent.replay batching, target rule, whole step  BS_brain.py:555-748
 *   v2x_agg_* / v2x_node_update_* / v2x_mlp_* / v2x_adam_step
 *                                 <- the implicit TF op set of GNNLayer.call (:44-51),
 *                                    AggLayer.call (:69-76), Dense (:176-179), huber (:86-87),
 *                                    Adam (:212); exported so each kernel is parity-testable
 *                                    on its own.
 *
 * Conventions
 *   - plain C, no exceptions; every call returns 0 on success or a negative V2X_E* code;
 *     `v2x_last_error(model)` (or `v2x_last_error(NULL)` for create failures) gives text.
 *   - all arithmetic is fp32 (Keras floatx), edge indices int32.
 *   - pointers marked [dev] are device (HBM) pointers, [host] host pointers, [any] either,
 *     selected by the `on_device` flag next to them.  The caller owns every buffer it
 *     passes; the engine never retains input pointers beyond the call.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  Calls are
 *     asynchronous on that stream except where host buffers are read or written.
 *   - one model handle per (network, device); a handle is not thread-safe; distinct
 *     handles are independent (online and target networks are two handles).
 *
 * Data layout (DESIGN.md "Data layout in HBM")
 *   A batch of B graphs is R node rows, graph-major; node order inside a graph is the
 *   reference's D1..DN order.  Features are packed per row as
 *       xe[R][16] = [ node features (Dn = 2C+1) | edge features (De = C) | zero pad ]
 *   (the reference's `D{k}_Node_Input` / `D{k}_Edge_Input`, BS_brain.py:461-467).
 *   Adjacency is CSR by DESTINATION row: sources of global row q are the graph-local node
 *   ids col_idx[row_ptr[q] .. row_ptr[q+1]) , ascending, no duplicates; this is
 *   Adj[p,q] == 1  (BS_brain.py:441-445) and  agg_q = sum_p Adj[p,q] h_p  (:72-76).
 *   graph_off[B+1] gives the first row of every graph (NULL => fixed n_nodes per graph).
 *
 * Flat parameter layout (v2x_get_weights / v2x_set_weights / gradient buffer), fp32:
 *   stage-major, slot-minor.  S = n_nodes weight sets (reference: one per node) or 1 when
 *   share_weights.  For every layer, for every slot:  W[K][N_out] row-major, then bias[N_out].
 *     GNN stage 0      K rows = [ x(Dn) | e(De) | neighbor(F) ]            (W1 ; W2 ; W3 of :121)
 *     GNN stage s>=1   K rows = [ h(F) | x(Dn) | e(De) | agg(F) ]         (W1 ; W2 ; W3 of :154/:161)
 *     Dense 0          K rows = [ h(F) | x(Dn) | agg(F) ]   N_out = 80     (:176, rows permuted
 *                                                                          from Keras' [x|h|agg])
 *     Dense 1..3       [80][40], [40][20], [20][C]                         (:177-179)
 */
#ifndef V2XGNN_H
#define V2XGNN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define V2X_OK            0
#define V2X_EINVAL       -1   /* bad argument / unsupported configuration */
#define V2X_EHIP         -2   /* a HIP runtime call failed                */
#define V2X_ENOMEM       -3
#define V2X_ESTATE       -4   /* call order violated (e.g. backward before forward) */
#define V2X_ECOMM        -5   /* a collective of a v2x_comm table returned non-zero   */
#define V2X_EBUDGET      -6   /* v2x_opt_search_bound spent its node budget: the result is a lower bound, not proven */
                              /* (v2x_opt_count_bound: the counts are lower bounds, `open` brackets them)             */

#define V2X_XE_WIDTH     16   /* packed [x|e|pad] row width */

typedef struct v2x_model v2x_model;

typedef struct v2x_config {
  int32_t n_nodes;        /* N: nodes per graph (num_D2D, BS_brain.py:95); >=1             */
  int32_t n_channels;     /* C: num_CH (:97); this build supports C == 4                     */
  int32_t feat_dim;       /* F: num_Feedback (:98); 16, 32, 64 (register-chained path), 128 or
                             256 (LDS-tiled wide path) in this build                         */
  int32_t n_mp_layers;    /* L: message-passing stages after the embed (reference: 2)        */
  int32_t share_weights;  /* 0 = one weight set per node slot (reference), 1 = shared        */
  int32_t variable_graphs;/* 1 = graphs of different sizes (needs share_weights)             */
  int32_t device;         /* HIP device ordinal                                              */
  int32_t use_graph;      /* 1 = capture/replay the step as a hipGraph when shapes repeat    */
  float   lr, beta1, beta2, eps;   /* Keras Adam (:212): 1e-3, 0.5, 0.999, 1e-7             */
} v2x_config;

typedef struct v2x_batch {
  int32_t n_graphs;        /* B */
  int32_t n_rows;          /* R = sum of nodes                                              */
  int32_t n_edges;         /* E = row_ptr[R]                                                */
  int32_t max_nodes;       /* max nodes of any graph in the batch                           */
  int32_t max_edges;       /* max edges of any graph in the batch                           */
  int32_t on_device;       /* 1: all pointers below are [dev]; 0: [host] (copied per call)  */
  const float*   xe;        /* [R][16]                                                      */
  const float*   nbr_init;  /* [R][F] or NULL (reference always feeds zeros, :478-490)      */
  const int32_t* graph_off; /* [B+1] or NULL when every graph has n_nodes rows              */
  const int32_t* row_ptr;   /* [R+1] global edge offsets                                    */
  const int32_t* col_idx;   /* [E] graph-local source node                                  */
} v2x_batch;

/* ---- model lifetime -------------------------------------------------------------------- */
int  v2x_create(const v2x_config* cfg, v2x_model** out);
void v2x_destroy(v2x_model* m);
const char* v2x_last_error(const v2x_model* m);
const char* v2x_version(void);

/* ---- parameters ------------------------------------------------------------------------ */
int64_t v2x_param_count(const v2x_model* m);
int  v2x_get_weights(v2x_model* m, float* host_out, void* stream);        /* [host] P floats */
int  v2x_set_weights(v2x_model* m, const float* host_in, void* stream);   /* [host] P floats */
int  v2x_copy_weights(v2x_model* dst, const v2x_model* src, void* stream);/* device-to-device */
int  v2x_get_optimizer_state(v2x_model* m, float* host_m, float* host_v, int64_t* iterations, void* stream);
int  v2x_set_optimizer_state(v2x_model* m, const float* host_m, const float* host_v, int64_t iterations, void* stream);
/* device pointers of the flat fp32 buffers (length v2x_param_count): for RCCL all-reduce of
 * the gradient by the host framework, and for zero-copy inspection.                        */
float* v2x_param_ptr(v2x_model* m);
float* v2x_grad_ptr(v2x_model* m);

/* ---- the hot path ---------------------------------------------------------------------- */
/* forward only: q_out[R][C]  (Model.predict, BS_brain.py:225-231).  Batches of at most 256 node
 * rows of fixed-size graphs (the rollout predict, BS_brain.py:336,1108,1394: one graph per call) run as
 * ONE launch (csrc/kernels_small.hpp); nothing is saved for a backward pass, which is only ever
 * driven by v2x_forward_backward / v2x_train_step / v2x_dqn_step (they run their own forward).      */
int  v2x_forward(v2x_model* m, const v2x_batch* b, float* q_out, int q_on_device, void* stream);

/* v2x_forward as a plain callback `int (*)(void*)` for host code that takes one: the closure holds the arguments (the batch
 * descriptor may point into page-locked host buffers the caller refills between calls, on_device = 1, see
 * v2x_device_addressable; q_on_device = 0 copies Q back and synchronises).  The rollout of ONE simulator as a single
 * library call (include/v2xsim.h, v2xsim_rollout: BS_brain.py:308-352 inside :409-553) scores its observations through it.   */
typedef struct v2x_forward_closure {
  v2x_model* m; v2x_batch b; float* q_out; int32_t q_on_device; int32_t pad_; void* stream;
} v2x_forward_closure;
int  v2x_forward_call(void* closure);

/* one fit step = forward + Huber + backward + Keras-Adam (Model.fit, BS_brain.py:218-223).
 *   y[R][C] targets;  loss_out[n_nodes] per-output Huber means (History 'D{k}_Decide_Output_loss'),
 *   may be NULL.  n_graphs_global: B of the GLOBAL batch (== b->n_graphs on one GPU): the
 *   Huber mean is taken over it, so per-rank gradients SUM to the global-batch gradient.   */
int  v2x_train_step(v2x_model* m, const v2x_batch* b, const float* y, int y_on_device,
                    int32_t n_graphs_global, float* loss_out, int loss_on_device, void* stream);

/* the same step split for data parallelism: (1) forward+backward leaves the local gradient
 * in v2x_grad_ptr(); the host all-reduces (sum) it over ranks; (2) apply the Adam update.
 * (v2x_train_step_dp below runs the whole data-parallel step, collectives included, in one call.)  */
int  v2x_forward_backward(v2x_model* m, const v2x_batch* b, const float* y, int y_on_device,
                          int32_t n_graphs_global, float* loss_out, int loss_on_device, void* stream);
int  v2x_apply_gradients(v2x_model* m, void* stream);
/* the same forward+backward in v2x_grad_bucket_count(m) calls ("phases"), for overlapping the gradient all-reduce with the
 * backward pass: after phase k, bucket k of the flat gradient is final and the host may start its collective while the
 * later phases compute.  v2x_grad_bucket gives a bucket's length and its offset (floats) inside v2x_grad_ptr().
 *   feat_dim <= 64 (graph-major fused kernels): 2 phases -- [the Dense layers] (tail of the flat layout), [the graph layers]
 *   feat_dim >= 128 (one weight-gradient launch per layer): L + 2 phases -- [the Dense layers], [stage L], ..., [stage 1],
 *     [embed]: 4.6 + 3 x 13.5 + 6.9 M floats at configs[3] ("bandwidth-bound, overlappable with the tail
 *     of backward")
 * loss_out is written by the last phase.  Phases must be called in order, 0 first.                                        */
int  v2x_forward_backward_phase(v2x_model* m, const v2x_batch* b, const float* y, int y_on_device,
                                int32_t n_graphs_global, int phase, float* loss_out, int loss_on_device, void* stream);
int  v2x_grad_bucket_count(const v2x_model* m);
int64_t v2x_grad_bucket(const v2x_model* m, int bucket, int64_t* offset);
/* Keras Adam on parameters [offset, offset + count) only (float4-aligned), from the gradient buffer: the optimizer step of
 * a rank that owns a 1 / G slice of every bucket after a reduce-scatter (the host all-gathers the parameters afterwards).
 * advance_iteration != 0 on the first call of a step (Adam's t), 0 on the others.                                       */
int  v2x_apply_gradients_range(v2x_model* m, int64_t offset, int64_t count, int advance_iteration, void* stream);

/* ---- data parallelism driven by the library ----------------------------------------------------------------------
 * A collective table: the library calls it between the backward pass and Adam, on the caller's stream (the bucket collectives
 * of forms V2X_DP_BUCKETS and V2X_DP_SHARDED on a stream the model owns, joined back into the caller's stream).  Every entry returns 0 on success; `stream` is a hipStream_t.  Ordering contract: a call
 * sees all work enqueued on `stream` before it, and work enqueued on `stream` after it sees its result.  A table may also
 * block the host until the collective is done.
 *   all_reduce_sum      in place: buf[0..n) = sum over ranks
 *   reduce_scatter_sum  in place over a bucket of n floats (n % world == 0): afterwards rank r's slice
 *                       [r n / world, (r + 1) n / world) holds the sum; the rest of buf is unspecified (ncclReduceScatter)
 *   all_gather          in place: rank r's slice of the n floats is its input (ncclAllGather)                             */
typedef struct v2x_comm {
  int32_t world, rank;
  void* ctx;
  int (*all_reduce_sum)(float* buf, int64_t n, void* stream, void* ctx);
  int (*reduce_scatter_sum)(float* buf, int64_t n, void* stream, void* ctx);
  int (*all_gather)(float* buf, int64_t n, void* stream, void* ctx);
} v2x_comm;

/* The RCCL table, built by the library.  RCCL is resolved at run time (dlopen "librccl.so.1" -- inside a PyTorch process
 * that is torch's own copy -- then /opt/rocm/lib): libv2xgnn.so has no link-time dependency on it.  Without RCCL these
 * return V2X_EINVAL with the text in v2x_last_error(NULL).  create: every rank passes rank 0's unique id; fills `out` (ctx =
 * the communicator) for HIP device `device`.                                                                            */
int  v2x_comm_rccl_unique_id(uint8_t out[128]);
int  v2x_comm_rccl_create(const uint8_t id[128], int32_t world, int32_t rank, int32_t device, v2x_comm* out);
int  v2x_comm_rccl_destroy(v2x_comm* c);

#define V2X_DP_ALLREDUCE  0   /* forward + backward, ONE all-reduce of the flat gradient, Adam on every rank              */
#define V2X_DP_BUCKETS    1   /* the v2x_forward_backward_phase phases; bucket k's all-reduce starts on a stream of the model
                                 as soon as phase k is done and overlaps the later phases; Adam after all of them          */
#define V2X_DP_SHARDED    2   /* per bucket: reduce-scatter, Adam on this rank's slice, all-gather of the parameters.  A bucket
                                 of n floats is cut into `world` slices only when n % (4 world) == 0; otherwise it is
                                 all-reduced and updated whole.  Adam's moments are then current on the owned slices only.  */

/* One data-parallel fit step on this rank's shard `b` of a global batch of n_graphs_global graphs (node rows for
 * variable_graphs models; > 0, no local default): forward + backward, the collectives of `form` through `comm`, Keras Adam.
 * The same launches and collectives, in the same order, as v2xgnn.dp.DataParallelTrainer.train_step in that form; the
 * collectives are never captured into a hipGraph (with use_graph the compute part is replayed, the rest goes out eagerly).
 * loss_out: the per-output losses summed over the ranks.  Host batches run forms 1 and 2 without phases (as the Python
 * trainer does).  A collective that fails: V2X_ECOMM, the text names it and its bucket; in forms 0 and 1, and for a failing
 * reduction in form 2, Adam is not applied and the iteration count does not advance (a failing all-gather of form 2 comes
 * after Adam on the owned slices).                                                                                       */
int  v2x_train_step_dp(v2x_model* m, const v2x_batch* b, const float* y, int y_on_device, int32_t n_graphs_global,
                       const v2x_comm* comm, int form, float* loss_out, int loss_on_device, void* stream);
/* v2x_dqn_step under data parallelism: s / s_next / action / reward are this rank's share of a minibatch of n_graphs_global
 * graphs; one all-reduce of the gradient and of the losses before Adam (form V2X_DP_ALLREDUCE only).                      */
int  v2x_dqn_step_dp(v2x_model* online, v2x_model* target, const v2x_batch* s, const v2x_batch* s_next,
                     const int32_t* action, const double* reward, double gamma, int32_t n_graphs_global,
                     const v2x_comm* comm, float* y_out, float* loss_out, int loss_on_device, void* stream);

/* ---- per-kernel entry points (parity tests; all pointers [dev]) ------------------------ */
/* AggLayer.call forward: out[q] = sum_{p in N(q)} h[p]            (BS_brain.py:69-76)      */
int  v2x_agg_fwd(const v2x_batch* b, int32_t n_nodes, int32_t feat_dim,
                 const float* h, float* out, void* stream);
/* its transpose (backward):   out[p] = sum_{q : p in N(q)} g[q]                            */
int  v2x_agg_bwd(const v2x_batch* b, int32_t n_nodes, int32_t feat_dim,
                 const float* g, float* out, void* stream);
/* GNNLayer.call of stage `stage` with the model's weights (BS_brain.py:44-51):
 *   out = act( [h_prev|x]W1 + e W2 + agg_prev W3 + b ), act = relu for stage < L.          */
int  v2x_node_update_fwd(v2x_model* m, int32_t stage, int32_t n_rows, const float* xe,
                         const float* h_prev, const float* agg_prev, float* out, void* stream);
/* backward of the same: given dpre[R][F] (gradient at the pre-activation) writes
 * dh_prev[R][F], dagg_prev[R][F] (either may be NULL for stage 0) and ACCUMULATES nothing:
 * the layer's weight gradient is written to grad_out (flat layout, only this layer's range). */
int  v2x_node_update_bwd(v2x_model* m, int32_t stage, int32_t n_rows, const float* xe,
                         const float* h_prev, const float* agg_prev, const float* dpre,
                         float* dh_prev, float* dagg_prev, float* grad_out, void* stream);
/* decision MLP (Dense 80-40-20-C, :176-179) forward and Huber+backward.                    */
int  v2x_mlp_fwd(v2x_model* m, int32_t n_rows, const float* xe, const float* h, const float* agg,
                 float* q_out, void* stream);
int  v2x_mlp_huber_bwd(v2x_model* m, int32_t n_rows, int32_t n_graphs_global, const float* xe,
                       const float* h, const float* agg, const float* y,
                       float* dh, float* dagg, float* grad_out, float* loss_out, void* stream);
/* Keras Adam on arbitrary flat device buffers (BS_brain.py:212)     */
int  v2x_adam_step(float* param, const float* grad, float* mom, float* vel, int64_t n,
                   int64_t iteration /* 1-based t */, float lr, float beta1, float beta2, float eps,
                   void* stream);

/* ---- DQN replay glue on device ------------------------------------------------------------
 * Counterparts of the minibatch assembly (BS_brain.py:573-640: per-sample Python loops filling the
 * 13 input arrays) and of the target rule (BS_brain.py:670-692) of Agent.replay, for transitions
 * that stay resident in HBM.  All pointers [dev].                                              */
/* 1 when the device can dereference p as it stands: device or managed memory, or page-locked host memory that is mapped
 * at the SAME address (hipHostMalloc defaults under unified addressing: what the zero-copy predict and the replay's index
 * ring hand to kernels, rl/agent.py, rl/replay.py); 0 for pageable host memory or a mapping at another address; a negative
 * V2X_E* code when the runtime cannot say.  Callers check once per buffer, before they set on_device = 1 on host arrays.    */
int  v2x_device_addressable(const void* p);
/* dst[i][0..row_bytes) = src[idx[i]][0..row_bytes)   (row_bytes a multiple of 4)               */
int  v2x_gather_rows(const void* src, const int32_t* idx, void* dst, int64_t n_idx, int64_t row_bytes,
                     void* stream);
/* up to 8 such gathers by the SAME index list as one launch (a replay minibatch: s, s', actions, rewards, CSR sources):
 * dst[j][i][0..row_bytes[j]) = src[j][idx[i]][0..row_bytes[j]).  src / dst / row_bytes: [host] arrays of n_jobs entries.       */
int  v2x_gather_rows_multi(int32_t n_jobs, const void* const* src, void* const* dst, const int64_t* row_bytes,
                           const int32_t* idx, int64_t n_idx, void* stream);
/* Q statistics of the fitted targets y[n_graphs][n_nodes][n_channels] (BS_brain.py:730-746) as float64 sums per link:
 * out[0][k] = sum over samples and channels, out[1][k] = sum over samples of the per-sample maximum; the caller divides
 * (by n_graphs * n_channels, by n_graphs).  out: [dev] [2][n_nodes] doubles.  Deterministic (fixed summation order).       */
int  v2x_q_stats(const float* y, int32_t n_graphs, int32_t n_nodes, int32_t n_channels, double* out, void* stream);
/* y = q (online net on s), except y[b][k][action[b][k]] = reward[b] + gamma * max_c q_next[b][k][c]
 * (q_next: target net on s'); evaluated like the reference's numpy-1.x scalar expression (float64
 * product and sum, rounded to fp32 once).  q, q_next, y: [n_graphs*n_nodes][n_channels]; action: [n_graphs][n_nodes];
 * reward: [n_graphs] double.                                                                    */
int  v2x_dqn_targets(const float* q, const float* q_next, const int32_t* action, const double* reward,
                     double gamma, int32_t n_graphs, int32_t n_nodes, int32_t n_channels, float* y_out,
                     void* stream);
/* The same rule on a RAGGED batch (graphs of different sizes, a variable_graphs model): row r takes the reward of the graph
 * that graph_off [n_graphs + 1] puts it in.  q, q_next, y: [n_rows][n_channels]; action: [n_rows]; reward: [n_graphs] double.
 * One launch on `stream`, no allocation, no synchronisation.                                                              */
int  v2x_dqn_targets_ragged(const float* q, const float* q_next, const int32_t* action, const double* reward,
                            double gamma, const int32_t* graph_off, int32_t n_graphs, int32_t n_rows,
                            int32_t n_channels, float* y_out, void* stream);

/* A replay minibatch of graphs of DIFFERENT sizes assembled in one launch.  Every pool is the storage of one link count in
 * the layout of rl/replay.py; every stored graph is regular (in-degree n - 2).  The graphs of pool 0 come first, in its idx
 * order, then pool 1's, ...: graph j of pool k starts at row rbase_k + j n_k and at edge ebase_k + j n_k (n_k - 2), the
 * bases being the sums over the pools before it.  Written: xe / xe_next [R][16], action [R], reward [B], graph_off [B + 1],
 * row_ptr [R + 1] and col_idx [E] (graph-local sources, as stored), with B = sum count, R = sum count n, E = sum count
 * n (n - 2): the arrays of two ragged v2x_batch (s and s') that share graph_off / row_ptr / col_idx.  `pools` is a [host]
 * array (the kernel takes the table by value), all pointers inside [dev]; `out` is a [host] struct of [dev] pointers, xe /
 * xe_next 16-byte aligned.  One launch on `stream`, no allocation, no synchronisation, no environment variable read.
 * V2X_EINVAL with the reason (v2x_last_error(NULL)): n_pools outside 1..8, counts that sum to 0 or a negative one, n_nodes
 * outside 3..31, a null pointer in a pool with count > 0 or in `out`, R or E beyond int32.  Slots are not range-checked.   */
typedef struct v2x_replay_pool {      /* one link count's replay storage (rl/replay.py layout) */
  int32_t n_nodes, count;             /* 3..31 links; graphs this pool contributes (>= 0) */
  const float *xe, *xe_next;          /* [cap][n][16] */
  const int32_t *col, *action;        /* [cap][n (n-2)], [cap][n] */
  const double* reward;               /* [cap] */
  const int32_t* idx;                 /* [count] storage slots, device-addressable */
} v2x_replay_pool;
typedef struct v2x_mixed_batch {
  float *xe, *xe_next; int32_t* action; double* reward;
  int32_t *graph_off, *row_ptr, *col_idx;
} v2x_mixed_batch;
int  v2x_replay_gather_mixed(int32_t n_pools /*1..8*/, const v2x_replay_pool* pools /*[host]*/,
                             const v2x_mixed_batch* out /*[dev] pointers*/, void* stream);

/* A replay minibatch of 3..128-link graphs from a storage that keeps the adjacency of a transition as its RECEIVERS
 * (rl/replay.py ReceiverReplay): with one receiver per link, Adj[p, q] = 1 unless p == q or p is the receiver of link q
 * (BS_brain.py:441-445), so recv[n] stands for the whole matrix; recv[q] == q marks a link that is its own receiver (two
 * vehicles on one spot: in-degree n - 1 instead of n - 2).  For graph g with slot s = idx[g] the call writes xe / xe_next
 * rows [g n, (g + 1) n) (16-byte copies), action [g][n], reward [g], and the CSR in packing.adj_to_csr's order:
 *   row_ptr[g n + q] = base_g + q (n - 2) + #{q' < q : recv[q'] == q'},  base_g = edge_base ? edge_base[g] : g n (n - 2),
 *   row q: every p in [0, n) except q and recv[q], ascending (graph-local sources),
 * and the last graph writes row_ptr[K n].  edge_base [K + 1] (first edge of every graph; needed as soon as one sampled graph
 * has an own-receiver link) is the caller's cumulative sum of n (n - 2) + own(slot); no store goes at or beyond
 * edge_base[g + 1] nor beyond (g + 1) n (n - 1), so col_idx of K n (n - 1) entries is always enough.  recv is only compared,
 * never used as an index; slots are not range-checked.  `src` is a [host] struct of [dev] pointers (idx and edge_base
 * device-addressable), `out` a [host] struct of [dev] pointers whose graph_off is not used and may be NULL; xe / xe_next of
 * both 16-byte aligned.  One launch on `stream`, no allocation, no synchronisation, no environment variable read.
 * V2X_EINVAL with the reason (v2x_last_error(NULL)): n_nodes outside 3..128, count < 1, a null pointer other than edge_base
 * and out->graph_off, a misaligned xe, K n or K n (n - 1) beyond int32.                                                       */
typedef struct v2x_replay_recv {
  int32_t n_nodes, count;             /* 3..128 links; K >= 1 sampled transitions */
  const float *xe, *xe_next;          /* [cap][n][16] */
  const int32_t *recv, *action;       /* [cap][n]: recv[q] = receiver of link q; recv[q] == q: link q is its own receiver */
  const double* reward;               /* [cap] */
  const int32_t* idx;                 /* [K] storage slots, device-addressable */
  const int32_t* edge_base;           /* [K + 1] first edge of every graph, device-addressable; NULL: every graph regular */
} v2x_replay_recv;
int  v2x_replay_gather_recv(const v2x_replay_recv* src /*[host]*/, const v2x_mixed_batch* out /*[dev] pointers*/, void* stream);

/* One whole replay step (BS_brain.py:664-728: predict on s, predict(target) on s', target rule, train_dnn) as a
 * single call on device-resident batches: the graph layers of the online network run ONCE (their activations feed
 * the backward pass), where predict + fit would run them twice.  y_out: optional [dev] [n_rows][C] buffer that
 * receives the training targets (for the caller's Q statistics, BS_brain.py:730-746); loss_out: per-output Huber
 * means like v2x_train_step.
 * Ragged form: online and target are both variable_graphs models of the same F and L.  Both batches carry graph_off and
 * s_next->graph_off is the SAME device pointer as s->graph_off (a transition's s and s' are the same links; n_graphs and
 * n_rows are equal too); action is [n_rows], one per node row; reward is [n_graphs], one per graph -- row r takes the
 * reward of its graph; loss_out is the single Huber mean over rows x C; n_graphs_global <= 0 defaults to the batch's node
 * rows (variable_graphs models count rows).  Anything else is V2X_EINVAL with a text that names the problem.            */
int  v2x_dqn_step(v2x_model* online, v2x_model* target, const v2x_batch* s, const v2x_batch* s_next,
                  const int32_t* action, const double* reward, double gamma, int32_t n_graphs_global,
                  float* y_out, float* loss_out, int loss_on_device, void* stream);

/* ---- the dict payload of the reference -> a packed host batch ---------------------------------
 * Model.predict / Model.fit of the reference take, per call, 3 N arrays 'D{k}_Node_Input' [B][Dn], 'D{k}_Edge_Input'
 * [B][De], 'D{k}_Neighbor_Input' [B][F] and the dense 'Adjacency_Matrix' [B][N F][N F] = kron(Adj, I_F)
 * (BS_brain.py:492-504, :603, :642-651, :704-716).  v2x_pack_feed turns that payload into the arrays of a host v2x_batch
 * in one pass of compiled host code (csrc/host_pack.hpp; no GPU involved): xe_out [B N][16], row_ptr_out [B N + 1],
 * col_idx_out [capacity B N N], nbr_out [B N][F] (written only when some Neighbor_Input entry is non-zero -- the
 * reference always feeds zeros, :478-490), info_out = {n_edges, max_edges, neighbour input non-zero}.
 * Every array is C-contiguous float32 or float64 (is_f64[3 N + 1]: node[0..N), edge[0..N), nbr[0..N), adjacency).
 * check_kron != 0: V2X_EINVAL unless the adjacency is exactly kron(Adj, I_F); entries other than 0 / 1 are always
 * V2X_EINVAL (the engine aggregates unweighted edges).  Error text: v2x_last_error(NULL).                              */
typedef struct v2x_feed {
  int32_t n_graphs, n_nodes, feat_dim, node_in, edge_in;
  const void* const* node;        /* [n_nodes] pointers */
  const void* const* edge;        /* [n_nodes] pointers */
  const void* const* nbr;         /* [n_nodes] pointers, or NULL */
  const uint8_t* is_f64;          /* [3 * n_nodes + 1] */
  const void* adjacency;
} v2x_feed;
int  v2x_pack_feed(const v2x_feed* feed, int check_kron, float* xe_out, int32_t* row_ptr_out, int32_t* col_idx_out,
                   float* nbr_out, int32_t* info_out);

/* ---- contract checks -------------------------------------------------------------------
 * The kernels size their LDS tiles from max_nodes / max_edges and rely on the CSR contract above (sources inside
 * their graph, strictly ascending => no duplicates).  HOST batches are checked on every call before anything is copied
 * (V2X_EINVAL).  DEVICE batches are the caller's responsibility: v2x_validate_batch checks one (synchronises `stream`;
 * `m` may be NULL, then n_nodes is used for fixed-size graphs).  Independently, a workgroup that finds a graph larger than
 * its LDS tile stages nothing and raises a flag; the flag is reported (V2X_EINVAL, results invalid) by the next call
 * that synchronises with the host (host-side q / loss outputs) or by v2x_check_errors.                              */
int  v2x_validate_batch(v2x_model* m, const v2x_batch* b, int32_t n_nodes, void* stream);
int  v2x_check_errors(v2x_model* m, void* stream);
/* The one-launch rollout predict (csrc/kernels_small.hpp) hands node rows between its workgroups through an exchange buffer
 * whose only state across launches is a per-graph departure count.  A launch that was aborted half-way leaves that state out
 * of step; the next predict then does not hang: its polls are bounded, it raises a flag and the synchronising call returns
 * V2X_ESTATE after re-arming the exchange by itself.  v2x_reset_exchange does the same re-arming on request (synchronises
 * the device).  v2x_debug_exchange_counters: [dev] pointer to the 256 64-bit departure counters (tests corrupt one on purpose).
 * The split-tile fused graph layers (csrc/kernels_fused_split.hpp: K workgroups per 16-graph tile for batches that leave most
 * of the chip idle) hand stage rows between a tile's workgroups the same way, with one 64-bit launch counter per tile; the
 * same bounded polls, the same V2X_ESTATE + self re-arming, and v2x_reset_exchange re-arms that exchange as well.           */
int  v2x_reset_exchange(v2x_model* m);
void* v2x_debug_exchange_counters(v2x_model* m);
/* [dev] pointer to the split-tile exchange's per-tile 64-bit launch counters (*n_tiles of them; NULL before the first split-tile
 * launch of the model): tests push one out of step on purpose.                                                                    */
void* v2x_debug_split_counters(v2x_model* m, int32_t* n_tiles);

/* ---- optimal channel allocation (csrc/v2xopt.hip) ---------------------------------------------------------------
 * The brute-force baseline of the evaluation drivers (BS_brain.py:1060-1100, :1286-1330, :1339-1380): for each of E
 * simulator states (one receiver per link, every link active), the joint action a[0..n) in [0, rb)^n with the largest
 *   w_v2v * sum_l log2(1 + signal_l / I_l) + w_v2i * sum_{r < min(rb, n)} log2(1 + V2I signal_r / (BS_r + sig2))
 * in fp64 (the rates of compute_reward_with_channel_selection, rl/environment.py).  Joint action index
 * idx = sum_l a_l * rb^(n-1-l): link 0 most significant, the order of itertools.product(range(rb), repeat=n).  Among exact
 * ties the lowest index wins (np.argmax).  Limits: 1 <= n <= 32, 2 <= rb <= 16, E <= 65535; the search takes
 * rb^n <= 2^36, the reward range rb^n <= 2^62.  All pointers [dev]; the dB inputs are the simulator's own arrays.
 * Every call is asynchronous on `stream` (no allocation, no synchronisation: capturable).  Error text: v2x_last_error(NULL). */
typedef struct v2x_opt_problem {
  int32_t E, n, rb, pad_;
  const double* v2v_ff;    /* [E][n][n][rb] dB, V2V_channels_with_fastfading                                         */
  const double* v2i_ff;    /* [E][n][rb]    dB, V2I_channels_with_fastfading                                         */
  const double* v2i_abs;   /* [E][n]        dB, V2I_channels_abs                                                     */
  const int64_t* dest;     /* [E][n]        receiver of link l (destinations[0]); outside [0, n): that link's rewards NaN */
  double p_v2v, p_v2i, veh_gain, bs_gain, bs_nf, veh_nf, sig2, w_v2v, w_v2i;
} v2x_opt_problem;
/* bytes of the workspace both calls below need (tables of all E states + the search's partial results); < 0 on a bad
 * problem */
int64_t v2x_opt_workspace_bytes(const v2x_opt_problem* p);
/* best_index[E], best_reward[E]: the optimum of every state */
int  v2x_opt_search(const v2x_opt_problem* p, void* workspace, int64_t* best_index, double* best_reward, void* stream);
/* out[E][count]: the reward of every index in [first, first + count) (the reference's Curr_Feasible_Reward vector); the
 * same device arithmetic as the search, so out[best_index - first] == best_reward bit for bit */
int  v2x_opt_rewards(const v2x_opt_problem* p, void* workspace, int64_t first, int64_t count, double* out, void* stream);
/* The reward landscape of every state over ALL rb^n joint actions (rb^n <= 2^36, the limits of v2x_opt_search).
 * edges [dev] [E][n_edges] doubles, 1 <= n_edges <= 62.  For a reward r, bin(r) = number of j with edges[e][j] <= r
 * (for ascending edges: np.searchsorted(edges[e], r, side='right')); a NaN edge is legal and never satisfies <=.
 * counts [dev] [E][n_edges + 2] int64: slots 0..n_edges count the joint actions per bin, slot n_edges + 1 counts NaN
 * rewards; the slots of a state sum to rb^n.  Every reward has the bits v2x_opt_rewards returns for its index, and the
 * counts are exact integers: a state's counts do not depend on the states stacked around it.  sums [dev] [E] (may be
 * NULL): the fp64 sum of the state's rewards (NaN if any reward is), added in a fixed order: bit-identical from call to
 * call for the same problem, but the order follows the launch plan, which depends on E, so the last bits may differ
 * between a stacked and a single-state call.  Asynchronous on `stream`, three launches, no allocation, no
 * synchronisation (capturable). */
int64_t v2x_opt_landscape_workspace_bytes(const v2x_opt_problem* p, int32_t n_edges);
int  v2x_opt_landscape(const v2x_opt_problem* p, void* workspace, const double* edges, int32_t n_edges,
                       int64_t* counts, double* sums, void* stream);
/* The same optimum by branch and bound (a depth-first search with an admissible upper bound on every completion of a
 * partial assignment; csrc/v2xopt.hip): no cap on rb^n beyond the 64-bit index (rb^n <= 2^62), so 20 links x 4 channels and
 * more.  Bit for bit the pair v2x_opt_search defines: leaves are scored with the same arithmetic, and nothing is pruned
 * that could equal the incumbent.  Both weights must be >= 0 (V2X_EINVAL).  max_nodes (>= 1): search-tree nodes the call
 * may visit over all E states, checked between launches (a launch visits a bounded number); when it is spent the call
 * returns V2X_EBUDGET with links, channels and nodes in v2x_last_error(NULL), and best_index / best_reward hold the best
 * leaf found so far: a lower bound, not proven optimal.  nodes_visited: [host], may be NULL; varies from run to run, the
 * result does not.  Unlike the calls above this one synchronises `stream` once per round of launches to read two counters
 * back (not capturable); it allocates nothing.  v2x_opt_bound_workspace_bytes: its workspace (>= what v2x_opt_rewards
 * needs for the same problem); < 0 on a bad problem or budget.                                                          */
int64_t v2x_opt_bound_workspace_bytes(const v2x_opt_problem* p, int64_t max_nodes);
int  v2x_opt_search_bound(const v2x_opt_problem* p, void* workspace, int64_t max_nodes, int64_t* best_index,
                          double* best_reward, int64_t* nodes_visited, void* stream);

/* v2x_opt_search_bound with a start: the incumbent of state e begins as the reward of start_actions[e] ([dev] [E][n] channel
 * numbers) scored as a leaf, and that action is entered as a candidate exactly like a leaf a lane found.  Same limits and
 * the same (index, reward) bits as the unseeded call: a node is still pruned only strictly below the incumbent, so an equal
 * reward at a lower index is still found; only nodes_visited changes.  A start with a channel outside [0, rb) seeds nothing.
 * Workspace: v2x_opt_bound_workspace_bytes. */
int  v2x_opt_search_bound_seeded(const v2x_opt_problem* p, void* workspace, int64_t max_nodes, const int32_t* start_actions,
                                 int64_t* best_index, double* best_reward, int64_t* nodes_visited, void* stream);
/* Counting branch and bound: how many joint actions of state e score strictly above / exactly at thresholds[e][a] -- the
 * pair a landscape with the edges { v, nextafter(v) } yields, each reward with the bits v2x_opt_rewards returns for its index --
 * without walking rb^n joint actions: v2x_opt_search_bound's tree with the fixed threshold in the incumbent's place.  A
 * subtree is dropped only when its upper bound lies strictly below the threshold by the search's rounding margin, so no
 * better and no equal action is lost, and every leaf reached is compared with the threshold exactly.  Limits: 1..32 links,
 * 2..16 channels (no cap on rb^n: no index is returned; rb * (n + 1) <= 318, the lanes' LDS), both weights >= 0,
 * 1 <= n_thr <= 31, E * n_thr <= 262144, no NaN threshold, max_nodes >= 1: V2X_EINVAL otherwise.
 * thresholds [dev] [E][n_thr]; better, equal [dev] [E][n_thr] int64: exact integers, the same from run to run and whatever
 * states are stacked around a state.  max_nodes: nodes the call may visit over all (state, threshold) pairs, checked between
 * launches; when it is spent the call returns V2X_EBUDGET, better / equal hold what has been counted (certified lower
 * bounds) and open_hi : open_lo [dev] [E][n_thr] the 128-bit number of leaves not examined, so that
 * better <= true better <= better + open, and the same for equal; nothing is dropped silently.  On V2X_OK open is 0.
 * nodes_visited: [host], may be NULL; varies from run to run.  Synchronises `stream` once for the threshold check and once
 * per round of launches (not capturable); allocates nothing.  v2x_opt_count_bound_workspace_bytes:
 * v2x_opt_bound_workspace_bytes + E * n_thr * (n + 1) * 8 rounded up to 256; < 0 on a bad argument. */
int64_t v2x_opt_count_bound_workspace_bytes(const v2x_opt_problem* p, int32_t n_thr, int64_t max_nodes);
int  v2x_opt_count_bound(const v2x_opt_problem* p, void* workspace, const double* thresholds, int32_t n_thr, int64_t max_nodes,
                         int64_t* better, int64_t* equal, uint64_t* open_hi, uint64_t* open_lo, int64_t* nodes_visited,
                         void* stream);
/* The arithmetic behind `open`, on the host (no device is touched): depth_counts [host] [n + 1], entry k the open subtrees
 * rooted at depth k -> open_hi : open_lo = sum_k depth_counts[k] * rb^(n - k) modulo 2^128. */
int  v2x_opt_count_open_leaves(const uint64_t* depth_counts, int32_t n, int32_t rb, uint64_t* open_hi, uint64_t* open_lo);
/* A near-optimal allocation where the exact searches cannot go: multi-start best-response local search, one wave per
 * (state, restart) -- a LOWER BOUND on the optimum, not the optimum.  1 <= n <= 128 links, 2 <= rb <= 16, E <= 65535; a joint
 * action is an array of n channel numbers, never an index.  Restart 0 starts from a[l] = l mod rb, restart r from
 * a[l] = splitmix64((seed << 32) ^ (r << 8) ^ l) mod rb; a sweep visits the links in order and moves each to the channel
 * with the largest total reward if that is strictly larger than the current total (lowest channel among equals); sweeps
 * repeat until one makes no move, max_sweeps (>= 1) at most.  A restart's reward is its final action scored from scratch
 * with the arithmetic of v2x_opt_rewards; a state's result is the best restart by (larger reward, else lexicographically
 * lower action), so it does not depend on the states around it or on the order of anything.  restarts: 1..65536.
 * best_info[e] = { winning restart, 1 if its last sweep made no move }.  all_actions / all_rewards: every restart's result.
 * Asynchronous on `stream`, four launches, no allocation, no synchronisation (capturable). */
int64_t v2x_opt_local_workspace_bytes(const v2x_opt_problem* p, int32_t restarts);
int  v2x_opt_search_local(const v2x_opt_problem* p, void* workspace, int32_t restarts, uint64_t seed, int32_t max_sweeps,
                          int32_t* best_actions /*[E][n]*/, double* best_reward /*[E]*/,
                          int32_t* best_info /*[E][2]; may be NULL*/, int32_t* all_actions /*[E][restarts][n]; may be NULL*/,
                          double* all_rewards /*[E][restarts]; may be NULL*/, void* stream);
/* out[E][K]: the reward of the joint actions actions[E][K][n] ([dev] channel numbers), 1 <= n <= 128; for n <= 32 bit for bit
 * what v2x_opt_rewards returns for the action's index.  A channel outside [0, rb) gives that action the reward NaN.
 * Workspace: v2x_opt_local_workspace_bytes(p, 1).  Asynchronous on `stream`, three launches (capturable). */
int  v2x_opt_rewards_actions(const v2x_opt_problem* p, void* workspace, const int32_t* actions, int64_t K, double* out,
                             void* stream);

/* ---- the simulator's channel step, observation and rates on the device (csrc/v2xsimdev.hip) ------------------------
 * Device counterparts of the host simulator library (include/v2xsim.h, csrc/v2xsim.c: v2xsim_channels, v2xsim_interference +
 * v2xsim_observe_packed, v2xsim_reward) for E independent simulator states of n vehicles = links and rb resource blocks
 * whose arrays live in HBM, in the simulator's own layouts (C-contiguous, state major).  The host library stays the
 * definition: the same expressions in the same order in fp64, no contraction, on the device math library, so results agree
 * with it to the rounding of the two math libraries, and bit for bit where only sums, differences, divides and casts are
 * involved (v2x_sim_observe's state / xe / mask / col / regular; v2x_sim_stream's positions, directions, stream states and
 * uniforms).  Mobility and the MT19937 streams may stay on the host (a step then receives its uniforms) or live in HBM too
 * (v2x_sim_stream, v2x_sim_advance).  All pointers [dev].  Every call is ONE launch (v2x_sim_advance: four), asynchronous on
 * `stream`: no allocation, no synchronisation, no environment variable read (capturable).  A bad argument is V2X_EINVAL
 * with text in v2x_last_error(NULL), before anything is launched.  E <= 65535.
 *
 * v2x_sim_channels: one channel update (renew_channel + renew_channels_fastfading, Environment.py:378-406 with the path loss
 * of :94-146) from the step's uniforms u[E][n_u], n_u = n + n^2 + 2 n rb + 2 n^2 rb exactly (always even; anything else
 * is V2X_EINVAL).  Gaussian k of a state is cos(2 pi u[k & ~1]) sqrt(-2 log(1 - u[k | 1])) for even k and the sin for odd k
 * (random.gauss order); draw order: V2I shadowing (n), V2V shadowing (n^2, row-major i n + j), V2I fast fading real then
 * imaginary (n rb each), V2V fast fading real then imaginary (n^2 rb each).  vel[E][n], pos[E][n][2].  v2i_shadow[E][n] and
 * v2v_shadow[E][n][n] are read and updated IN PLACE; written: v2v_abs[E][n][n] (path loss + shadowing, + 50 on the diagonal),
 * v2i_abs[E][n], v2v_ff[E][n][n][rb] and v2i_ff[E][n][rb] (abs - 20 log10 |(re + j im) / sqrt 2|).  The outputs must not
 * overlap each other or the inputs.  1 <= n <= 128, 1 <= rb <= 16.                                                          */
int  v2x_sim_channels(int32_t E, int32_t n, int32_t rb, const double* u, int32_t n_u, const double* vel, const double* pos,
                      double* v2i_shadow, double* v2v_shadow, double* v2v_abs, double* v2i_abs, double* v2v_ff,
                      double* v2i_ff, void* stream);
/* v2x_sim_observe: Compute_Interference (Environment.py:460-493, the observable part) and Agent.observe (BS_brain.py:389-407,
 * :441-445, :458-467) in the engine's packed form, for C = rb channels.  dest[E][n]: the receiver of every link;
 * v2v_ff[E][n][n][C], v2i_ff[E][n][C].  Written: interf_db[E][n][C] = 10 log10(sig2 + the V2I transmitter of block r
 * (vehicle r) at link k's receiver); state[E][n][3 C + 1] fp64 = [V2V gain | V2I gain | power | edge gain], the sum over
 * senders p taken in ascending p; xe[E][n][16] float32 = the state row cast to float32, zero padded; mask[E][n]: bit p of
 * mask[e][q] set when p sends to q (every p but q and q's receiver); col[E][n (n - 2)]: the CSR sources ascending per
 * destination, all zeros for a state where some dest[k] == k; regular[E] (bytes): 1 unless some dest[k] == k.  A receiver
 * outside [0, n) is never used as an index: that state's interf_db / state / xe rows are NaN and its regular flag is 0.
 * 3 <= n <= 31, 1 <= C <= n, 3 C + 1 <= 16 (the limits of v2xsim_observe_packed).                                          */
int  v2x_sim_observe(int32_t E, int32_t n, int32_t C, const int64_t* dest, const double* v2v_ff, const double* v2i_ff,
                     double p_v2i, double veh_gain, double veh_nf, double sig2, double power, double* interf_db,
                     double* state, float* xe, int32_t* mask, int32_t* col, uint8_t* regular, void* stream);
/* v2x_sim_rates: compute_reward_with_channel_selection (Environment.py:408-458; every link active, one receiver per link)
 * of ONE joint action per state, ch[E][n] channel numbers, on the arrays and constants of a v2x_opt_problem (w_v2v / w_v2i
 * unused).  Written: v2v_rate[E][n], v2i_rate[E][min(rb, n)]; may be NULL: interference[E][rb] (V2V power received at the
 * base station per block, without noise), v2i_interf[E][rb] and v2v_interf[E][n] (with noise).  Fold orders of the host
 * library: the base-station sum over ascending k per block; at a receiver the V2I transmitter's term first, then the
 * co-channel links in ascending j.  A channel outside [0, rb) anywhere in a state makes all outputs of that state NaN, a
 * receiver outside [0, n) those of its link; neither is used as an index.  1 <= n <= 128, 1 <= rb <= 16.                   */
int  v2x_sim_rates(const v2x_opt_problem* p, const int32_t* ch /*[E][n]*/, double* v2v_rate /*[E][n]*/,
                   double* v2i_rate /*[E][min(rb,n)]*/, double* interference /*[E][rb]*/, double* v2i_interf /*[E][rb]*/,
                   double* v2v_interf /*[E][n]*/, void* stream);
/* v2x_sim_stream: mobility and the random streams of E states (v2xsim_positions, then v2xsim_mt_uniforms), bit for bit the
 * host library's.  keys[E][624] / mtpos[E]: the MT19937 states in numpy's RandomState layout, advanced in place; a block of
 * 624 words is regenerated only when a word is needed and the position is 624, never eagerly, so after a call that ends
 * exactly at a block's end mtpos is 624 and keys is the block just used up (what RandomState.get_state() reports).  A
 * position outside [0, 624] reads as 624.  xy[E][n][2] / dirs[E][n] (0 up, 1 down, 2 left, 3 right) / vel[E][n]: one
 * renew_positions step of `timestep` seconds (Environment.py:236-345): vehicles in index order, the crossing lanes of
 * lanes[4][n_lanes] (tables up, down, left, right) in the reference's checking order, one 53-bit draw per reached lane (turn
 * when it is < 0.4), then re-entry of the vehicles that left [0, width] x [0, height].  xy == NULL: no mobility (dirs, vel
 * and lanes are not read).  Then u[E][n_u] = the next n_u doubles of every stream, (a >> 5, b >> 6) -> (a 2^26 + b) / 2^53 of
 * consecutive tempered words.  1 <= n <= 128, 1 <= n_lanes <= 64, n_u even and >= 2.                                         */
int  v2x_sim_stream(int32_t E, int32_t n, uint32_t* keys /*[E][624]*/, int32_t* mtpos /*[E]*/,
                    double* xy /*[E][n][2] or NULL: no mobility*/, int8_t* dirs /*[E][n]*/, const double* vel /*[E][n]*/,
                    double timestep, int32_t n_lanes, const double* lanes /*[4][n_lanes]: up, down, left, right*/,
                    double width, double height, double* u /*[E][n_u]*/, int32_t n_u, void* stream);
/* v2x_sim_advance: one whole simulator step of E states from nothing but the actions -- the device counterpart of
 * v2xsim_advance (include/v2xsim.h).  Enqueues, in this order, v2x_sim_rates of `actions` on the CURRENT channels (skipped
 * when actions is NULL), v2x_sim_stream (mobility, then the step's n_u uniforms into u), v2x_sim_channels on the moved
 * positions and v2x_sim_observe with C = rb: four launches on one stream, no parallel branches (capturable).  Every
 * argument check of the four calls is made before the first launch.  problem: E, n, rb, the constants, dest, and v2v_ff /
 * v2i_ff / v2i_abs, which must be the step's own arrays of the same names.  Limits: those of v2x_sim_observe (3..31 links,
 * rb <= n, 3 rb + 1 <= 16) and n_u == n + n^2 + 2 n rb + 2 n^2 rb, even.                                                      */
typedef struct v2x_sim_step {
  v2x_opt_problem problem;
  uint32_t* keys;          /* [E][624]  */
  int32_t* mtpos;          /* [E]       */
  double* xy;              /* [E][n][2] */
  int8_t* dirs;            /* [E][n]    */
  const double* vel;       /* [E][n]    */
  const double* lanes;     /* [4][n_lanes] */
  double* u;               /* [E][n_u]: the uniforms of the step (written, then read by the channel update) */
  int32_t n_lanes, n_u;
  double timestep, width, height;
  double *v2i_shadow, *v2v_shadow, *v2v_abs, *v2i_abs, *v2v_ff, *v2i_ff;        /* as v2x_sim_channels */
  double power;                                                                   /* as v2x_sim_observe  */
  double *interf_db, *state;
  float* xe;
  int32_t *mask, *col;
  uint8_t* regular;
  double *v2v_rate, *v2i_rate, *interference, *v2i_interf, *v2v_interf;          /* as v2x_sim_rates; the last three may be NULL */
  const int32_t* actions;  /* [E][n]; NULL: no rates */
} v2x_sim_step;
int  v2x_sim_advance(const v2x_sim_step* s, void* stream);

/* v2x_sim_reset: the episode reset (new_random_game, Environment.py:495-506) of E resident states -- the device counterpart of
 * v2xsim_reset_vehicles, the initial shadowing out of v2xsim_mt_uniforms, the reset's channel update and v2xsim_sample_dest on
 * the ranked neighbours.  Enqueues, in this order, k_sim_reset_draw (grid E, 256 threads, one state per workgroup, the key
 * array in LDS throughout), v2x_sim_channels and v2x_sim_observe with C = rb: three launches on one stream.
 * v2x_sim_reset_draw enqueues the first launch alone.  Same rules as v2x_sim_advance: all pointers [dev], no allocation, no
 * synchronisation, no environment variable read; every check comes before the first launch; a refusal is V2X_EINVAL with
 * text in v2x_last_error(NULL).  step: a v2x_sim_step whose actions is NULL (timestep is not read).  vel must be the step's
 * vel, dest the problem's dest: both are WRITTEN here and read by the two launches that follow.
 * Limits: n a multiple of 4 in 4..28; rb <= n and 3 rb + 1 <= 16; 1 <= n_lanes <= 64; width and height integral in [0, 2^31);
 * n_u == n + n^2 + 2 n rb + 2 n^2 rb.
 * k_sim_reset_draw consumes every state's stream in the host library's order:
 *   1. vehicles: per group of four, below(n_lanes); for down and for up below(height + 1), then 10 + below(6); for left and
 *      for right below(width + 1), then 10 + below(6).  below(m) takes the top bit_length(m) bits of successive tempered
 *      words until the value is < m.  lanes[4][n_lanes] is the step's table (up, down, left, right), the direction codes are
 *      v2x_sim_stream's.  Written: xy, dirs, vel.
 *   2. initial shadowing: the next 2 (n^2 + n) doubles go through the state's u; Gaussians n^2 + n .. 2 (n^2 + n) - 1 of them
 *      (v2x_sim_channels' pairing) give v2v_shadow = g * 3 (row-major) and v2i_shadow = g * 8; the first n^2 + n are consumed
 *      and dropped (the reference's unused V2V_Shadowing / V2I_Shadowing).
 *   3. the channel update's uniforms: the next n_u doubles into u, as v2x_sim_stream writes them.
 *   4. receivers: vehicles are ranked per link i by (d2, index) ascending, d2 = dx dx + dy dy to vehicle i in fp64 without
 *      contraction; then, in link order, j = below(n - 3) and dest[i] = the vehicle of rank 1 + j.
 *   5. keys and mtpos are written back with v2x_sim_stream's lazy block rule.
 * status[e], written: bit 0 -- for some link another vehicle (the link itself included) has exactly the chosen receiver's d2:
 * the host's answer then depends on the order its argsort leaves among equal keys, the device's rule is ascending index;
 * bit 1 -- a draw was not accepted within 64 words (probability below 1e-27 per draw with a working generator): the state's
 * work ended there with its stream state written back, its other outputs are unspecified.  On a lane grid whose coordinates
 * are multiples of 2^-10 below 2^15, d2 is exact and the order by d2 is the order by the host's np.abs.                    */
typedef struct v2x_sim_reset_args {
  v2x_sim_step step;
  double* vel;             /* [E][n], == step.vel          */
  int64_t* dest;           /* [E][n], == step.problem.dest */
  uint8_t* status;         /* [E] */
} v2x_sim_reset_args;
int  v2x_sim_reset(const v2x_sim_reset_args* r, void* stream);
int  v2x_sim_reset_draw(const v2x_sim_reset_args* r, void* stream);

/* ---- one DQN rollout iteration on the resident state (csrc/v2xsimdev.hip) --------------------------------------------
 * Agent._packed_iteration (BS_brain.py:308-352 inside :409-553) for E simulator states whose observation, simulator arrays and
 * replay memory all live in HBM: score, pick the actions, step the simulators, compute the reward, write the transitions into
 * their replay slots.  The host contributes the draws of the epsilon-greedy policy (which do not depend on device state) and
 * reads one small result row back.  Same rules as the v2x_sim_* calls: all pointers [dev], one asynchronous launch per
 * kernel on `stream`, no allocation, no synchronisation, no environment variable read; a bad argument is V2X_EINVAL with
 * text in v2x_last_error(NULL), before anything is launched.  Limits: those of v2x_sim_observe (3 <= n <= 31, 1 <= C <= n,
 * 3 C + 1 <= 16) and 1 <= E <= capacity.  State e's transition goes to replay slot (head + e) % capacity: a block may wrap.
 *
 * v2x_rollout_pick (before the simulator step): actions[e][k] = explore[e] ? random_actions[e][k] : argmax_c q[e n + k][c],
 * np.argmax's argmax (the first maximiser in ascending c; the first NaN wins over any number).  q == NULL: nobody is greedy,
 * explore is not read and every state takes its random actions.  The same launch copies the state's observation half --
 * xe[e] ([n][16] float32), col[e] ([n (n - 2)] int32) and mask[e] ([n] int32) -- to its slot of rep_xe / rep_col / rep_mask,
 * because the step overwrites it, and regular[e] to regular_out[e].
 *
 * v2x_rollout_store (after the step): reward[e] = w_v2v * S(v2v_rate[e][0..n)) + w_v2i * S(v2i_rate[e][0..min(rb, n))) in
 * fp64, no contraction, S being numpy's summation of a contiguous row (fewer than 8 terms: left to right; otherwise eight
 * accumulators r[j] = a[j], r[j] += a[i + j] over the whole groups of eight, ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)),
 * then the remaining terms one by one), so it equals w * v2v.sum(axis=(1, 2)) + w * v2i.sum(axis=1) bit for bit.  Written to
 * the state's slot: xe[e] (now the next observation) to rep_xe_next, actions[e] to rep_action, reward[e] to rep_reward; and
 * reward[e] to reward_out[e], regular[e] (of the next observation) to regular_out[e].                                        */
int  v2x_rollout_pick(int32_t E, int32_t n, int32_t C, const float* q /*[E n][C] or NULL*/, const uint8_t* explore /*[E]*/,
                      const int32_t* random_actions /*[E][n]*/, int32_t* actions /*[E][n], written*/, const float* xe,
                      const int32_t* col, const int32_t* mask, const uint8_t* regular, float* rep_xe, int32_t* rep_col,
                      int32_t* rep_mask, int64_t head, int64_t capacity, uint8_t* regular_out /*[E]*/, void* stream);
int  v2x_rollout_store(int32_t E, int32_t n, int32_t rb, const double* v2v_rate /*[E][n]*/,
                       const double* v2i_rate /*[E][min(rb,n)]*/, double w_v2v, double w_v2i, const float* xe,
                       const int32_t* actions, const uint8_t* regular, float* rep_xe_next, int32_t* rep_action,
                       double* rep_reward, int64_t head, int64_t capacity, double* reward_out /*[E]*/,
                       uint8_t* regular_out /*[E]*/, void* stream);
/* v2x_rollout_step: the iteration.  Enqueues, in this order on one stream with no parallel branches, v2x_forward of `batch`
 * on `model` into q (skipped when model is NULL: nobody is greedy), v2x_rollout_pick, the four launches of v2x_sim_advance
 * with `actions` as the step's actions, and v2x_rollout_store.  Every check of every part is made before the first launch.
 * batch: on_device = 1, n_graphs = E fixed-size graphs of n nodes, xe = step.xe, col_idx = step.col (the resident
 * observation; every state must be regular: the CSR has n - 2 sources per row), a model of n nodes and rb channels.
 * step.actions must be NULL or `actions`.  The result row: result_reward[E] doubles, result_regular[2][E] bytes (the flags
 * of the stored observation, then those of the next one).  Capturable once the model's workspaces exist (one eager call
 * first) on a model created without use_graph.                                                                             */
typedef struct v2x_rollout {
  v2x_model* model;                /* the online network, or NULL */
  v2x_batch batch;
  float* q;                        /* [E n][rb] Q workspace (required with a model) */
  const uint8_t* explore;          /* [E]    */
  const int32_t* random_actions;   /* [E][n] */
  int32_t* actions;                /* [E][n]: written by the pick, read by the step and the store */
  v2x_sim_step step;
  double w_v2v, w_v2i;
  float *rep_xe, *rep_xe_next;     /* [capacity][n][16]     */
  int32_t *rep_col, *rep_mask, *rep_action;   /* [capacity][n (n - 2)], [capacity][n], [capacity][n] */
  double* rep_reward;              /* [capacity] */
  int64_t head, capacity;
  double* result_reward;           /* [E]    */
  uint8_t* result_regular;         /* [2][E] */
} v2x_rollout;
int  v2x_rollout_step(const v2x_rollout* r, void* stream);

/* v2x_rollout_steps: T iterations of v2x_rollout_step in one call.  Nothing in a simulator step depends on the actions except
 * the rates paid for them, and the network does not change inside a rollout: all T observations are known before any action
 * is.  Enqueues, in this order on one stream with no parallel branches,
 *   k_sim_trajectory  grid (E), 256 threads: every state walks its T steps (stream, channels, observation: the device functions
 *                     of the single-step kernels, so the same bits), the MT19937 key array in LDS throughout.  It leaves the
 *                     resident arrays as T calls of v2x_sim_advance leave them and writes the trajectory: the observation at
 *                     entry and after every step (entries 0..T), and what the rates read before every step (snapshots 0..T-1);
 *   v2x_forward       of the T E observations of entries 0..T-1 (`r.batch`: on_device, T E graphs of n rows, xe = traj_xe,
 *                     col_idx = traj_col, n - 2 sources per row) into r.q -- skipped when r.model is NULL (nobody is greedy);
 *   k_rollout_finish  grid (T E), one wave per transition (t, e): the pick of v2x_rollout_pick, the rates of v2x_sim_rates on
 *                     snapshot t (same fold orders), the reward of v2x_rollout_store, and the transition -- xe / col / mask of
 *                     entry t, xe_next of entry t + 1, actions, reward -- into slot (head + t E + e) % capacity.  The
 *                     transitions of t = T - 1 also leave actions / v2v_rate / v2i_rate / interference / v2i_interf /
 *                     v2v_interf in the resident arrays.
 * In `r`: explore is [T][E], random_actions [T][E][n], q [T E n][rb], result_reward [T][E], result_regular [T][2][E] (row t:
 * the flags of the stored observation, then of the next one); everything else as for v2x_rollout_step.  Same rules: all
 * pointers [dev], asynchronous, no allocation, no synchronisation, no environment variable read; every check of every part
 * before the first launch (V2X_EINVAL, text in v2x_last_error(NULL)).  Limits: those of v2x_rollout_step, 1 <= T,
 * T E <= capacity (every transition of the block has its own slot), T E n (n - 2) < 2^31, non-NULL workspaces.
 * The trajectory workspace is seven arrays; one allocation of v2x_rollout_steps_workspace_bytes(E, n, rb, T) bytes holds
 * them back to back in the order of the struct, each rounded up to a multiple of 256 bytes:
 *   A(4 (T+1) E n 16) + A(4 (T+1) E n (n-2)) + A(4 (T+1) E n) + A((T+1) E) + A(8 T E n n rb) + A(8 T E n rb) + A(8 T E n),
 *   A(x) = ceil(x / 256) * 256.  A negative V2X_E* code on sizes outside the limits.                                          */
typedef struct v2x_rollout_traj {
  v2x_rollout r;
  int32_t T, pad_;
  float* traj_xe;                  /* [T+1][E][n][16]      */
  int32_t* traj_col;               /* [T+1][E][n (n - 2)]  */
  int32_t* traj_mask;              /* [T+1][E][n]          */
  uint8_t* traj_regular;           /* [T+1][E]             */
  double* traj_v2v_ff;             /* [T][E][n][n][rb]     */
  double* traj_v2i_ff;             /* [T][E][n][rb]        */
  double* traj_v2i_abs;            /* [T][E][n]            */
} v2x_rollout_traj;
int64_t v2x_rollout_steps_workspace_bytes(int32_t E, int32_t n, int32_t rb, int32_t T);
int  v2x_rollout_steps(const v2x_rollout_traj* r, void* stream);

/* v2x_rollout_steps_mixed: v2x_rollout_steps for up to 8 pools of DIFFERENT link counts in one call, all scored by one forward
 * of one ragged batch on a variable_graphs model (rl/mixed.py: one shared-weight network over several scenario sizes).  Pool k
 * is the v2x_rollout_traj of its own resident state, trajectory workspace and replay storage (E_k states of n_k links), and
 * every pool walks the same T steps.  With B = T S(E_k) graphs, R = T S(E_k n_k) rows and Ed = T S(E_k n_k (n_k - 2)) edges,
 * the batch is pool-major and inside a pool in the trajectory's own order (t, e): pool k's graphs start at graph
 * gbase_k = T S_{j<k}(E_j), at row rbase_k = T S_{j<k}(E_j n_j) and at edge ebase_k = T S_{j<k}(E_j n_j (n_j - 2)); transition
 * (k, t, e) reads the Q rows rbase_k + (t E_k + e) n_k + i.  Enqueues, in this order on one stream with no parallel branches,
 *   k_sim_trajectory_mixed  grid (S E_k), 256 threads: one workgroup per state, the body of k_sim_trajectory on its pool's
 *                           arguments (the states of the largest n in the lowest block indices);
 *   k_traj_assemble_mixed   grid (ceil(B / 4)), one wave per graph: xe [R][16] and col_idx [Ed] are entries 0..T-1 of every
 *                           pool's traj_xe and traj_col one after the other (graph-local sources, as v2x_replay_gather_mixed
 *                           leaves them), graph_off [B + 1] and row_ptr [R + 1] in closed form (n_k - 2 sources per row) --
 *                           skipped without a model;
 *   v2x_forward             of that batch on `model` into q [R][rb] -- skipped when model is NULL (nobody is greedy);
 *   k_rollout_finish_mixed  grid (B), one wave per transition: the body of k_rollout_finish on its pool's arguments with
 *                           q + rbase_k rb, into the pool's own replay slot (head_k + t E_k + e) % capacity_k, result row and
 *                           resident arrays.
 * The device functions are those of v2x_rollout_steps: per pool the bits of that call (given the same Q rows).  Same rules:
 * all pointers [dev] except `pools` ([host]; the kernels take their tables by value), asynchronous, no allocation, no
 * synchronisation, no environment variable read; every check of every pool and of the mixed part before the first launch.
 * V2X_EINVAL with a text that names the pool (v2x_last_error(NULL)): n_pools outside 1..8, link counts not strictly ascending,
 * a pool whose T is not the call's, a pool with a model of its own, anything v2x_rollout_steps refuses of a pool, pools that
 * differ in rb, a model that is not variable_graphs or whose channel count is not rb, a null xe / graph_off / row_ptr /
 * col_idx / q or a pool's null explore with a model (xe and every traj_xe 16-byte aligned), 16 R or Ed beyond INT32_MAX (the
 * float count of xe and the edge count are 32-bit sizes of a batch).  v2x_rollout_steps_mixed_wide (below, after the split
 * stream phase) is this call with the wide walk in k_sim_trajectory_mixed's place.                                            */
typedef struct v2x_rollout_mixed {
  int32_t n_pools, T;               /* 1..8 pools; every pool walks the same T >= 1 steps */
  const v2x_rollout_traj* pools;    /* [host][n_pools], strictly ascending step.problem.n; pools[k].T == T;
                                       pools[k].r.model must be NULL; r.batch and r.q are not read */
  v2x_model* model;                 /* a variable_graphs model with rb channels, or NULL: nobody is greedy */
  float* xe; int32_t *graph_off, *row_ptr, *col_idx;   /* [dev] the ragged batch, written by the call (unused without a model) */
  float* q;                         /* [dev] [R][rb] */
} v2x_rollout_mixed;
int  v2x_rollout_steps_mixed(const v2x_rollout_mixed* m, void* stream);

/* v2x_eval_steps: the T steps of an EVALUATION episode in one call -- v2x_rollout_steps without a replay memory, paying up to
 * two schemes per state and returning their rates, not only a reward.  Enqueues, in this order on one stream with no parallel
 * branches,
 *   k_sim_trajectory  as in v2x_rollout_steps, unchanged;
 *   v2x_forward       of the T E observations of entries 0..T-1 (`batch`: as in v2x_rollout_steps) into q -- skipped when model
 *                     is NULL (the policy scheme then takes random_actions everywhere and explore is not read);
 *   k_eval_finish     grid (S T E), one wave per (scheme, t, e), S = 2 with baseline_actions, else 1.  Scheme 0, the policy:
 *                     link k takes random_actions[t][e][k] when explore[t][e], else np.argmax of its Q row (the rule of
 *                     v2x_rollout_pick).  Scheme 1: baseline_actions[t][e].  Per scheme the rates of v2x_sim_rates on snapshot
 *                     t (same fold orders; a channel outside [0, rb) makes that (scheme, t, e) NaN and is never an index) and
 *                     reward = w_v2v * S(v2v_rate) + w_v2i * S(v2i_rate) in the summation order of v2x_rollout_store.  The
 *                     policy scheme at t = T - 1 also leaves actions / v2v_rate / v2i_rate / interference / v2i_interf /
 *                     v2v_interf in the resident arrays: after the call the resident state is what T calls of v2x_sim_advance
 *                     under the policy's actions leave.
 * Results, scheme major: result_actions [S][T][E][n], result_v2v_rate [S][T][E][n], result_v2i_rate [S][T][E][min(rb, n)],
 * result_interference [S][T][E][rb] (V2V power at the base station, without noise), result_reward [S][T][E], and
 * result_regular [T+1][E] (the flags of entries 0..T).  One allocation of v2x_eval_steps_result_bytes(E, n, rb, T, S) bytes
 * holds them back to back, unpadded, in the order v2v_rate, v2i_rate, interference, reward (doubles), actions (int32), regular
 * (bytes), the total rounded up to a multiple of 8: 8 S T E (n + min(rb, n) + rb + 1) + 4 S T E n + (T + 1) E.
 * Same rules as v2x_rollout_steps: all pointers [dev], asynchronous, no allocation, no synchronisation, no environment variable
 * read; every check of every part before the first launch (V2X_EINVAL, text in v2x_last_error(NULL)).  Limits: those of
 * v2x_rollout_step (without a replay ring), 1 <= T, T E <= 65535 (the stacked searches of v2x_opt_* accept the T E snapshots as
 * one problem), T E n (n - 2) < 2^31, non-NULL workspaces (layout and size: v2x_rollout_steps_workspace_bytes).
 * step.actions must be NULL or `actions`.                                                                                    */
typedef struct v2x_eval {
  v2x_model* model;                /* the network, or NULL */
  v2x_batch batch;
  float* q;                        /* [T E n][rb] Q workspace (required with a model) */
  const uint8_t* explore;          /* [T][E] (required with a model) */
  const int32_t* random_actions;   /* [T][E][n]: the policy's random actions */
  const int32_t* baseline_actions; /* [T][E][n], or NULL: no baseline scheme */
  int32_t* actions;                /* [E][n]: the resident actions (written: the policy's of t = T - 1) */
  v2x_sim_step step;
  double w_v2v, w_v2i;
  int32_t T, pad_;
  float* traj_xe;                  /* [T+1][E][n][16]      */
  int32_t* traj_col;               /* [T+1][E][n (n - 2)]  */
  int32_t* traj_mask;              /* [T+1][E][n]          */
  uint8_t* traj_regular;           /* [T+1][E]             */
  double* traj_v2v_ff;             /* [T][E][n][n][rb]     */
  double* traj_v2i_ff;             /* [T][E][n][rb]        */
  double* traj_v2i_abs;            /* [T][E][n]            */
  int32_t* result_actions;         /* [S][T][E][n]         */
  double* result_v2v_rate;         /* [S][T][E][n]         */
  double* result_v2i_rate;         /* [S][T][E][min(rb,n)] */
  double* result_interference;     /* [S][T][E][rb]        */
  double* result_reward;           /* [S][T][E]            */
  uint8_t* result_regular;         /* [T+1][E]             */
} v2x_eval;
int64_t v2x_eval_steps_result_bytes(int32_t E, int32_t n, int32_t rb, int32_t T, int32_t schemes);
int  v2x_eval_steps(const v2x_eval* r, void* stream);

/* v2x_eval_steps_mixed: v2x_eval_steps for up to 8 pools of DIFFERENT link counts in one call, all scored by one forward of one
 * ragged batch on a variable_graphs model -- the evaluation sibling of v2x_rollout_steps_mixed (rl/mixed.py MixedAgent.test_run:
 * an episode of every link count at once).  Pool k is the v2x_eval of its own resident state, trajectory workspace and result
 * block (E_k states of n_k links); every pool walks the same T steps and pays the same S schemes (S = 2 when the pools have
 * baseline_actions, else 1).  The ragged batch, gbase_k, rbase_k and ebase_k are those of v2x_rollout_steps_mixed.  Enqueues,
 * in this order on one stream with no parallel branches,
 *   k_sim_trajectory_mixed  as in v2x_rollout_steps_mixed, unchanged;
 *   k_traj_assemble_mixed   as in v2x_rollout_steps_mixed, unchanged -- skipped without a model;
 *   v2x_forward             of that batch on `model` into q [R][rb] -- skipped when model is NULL (nobody is greedy);
 *   k_eval_finish_mixed     grid (S T S(E_k)), one wave per (pool, scheme, t, e): the body of k_eval_finish on its pool's arguments
 *                           with q + rbase_k rb.  Pool-major: pool k owns blocks S gbase_k .. S gbase_k + S T E_k - 1, and inside
 *                           a pool the order is k_eval_finish's (scheme, t, e): every pool's result block has exactly the layout
 *                           of v2x_eval_steps (v2x_eval_steps_result_bytes(E_k, n_k, rb, T, S)), and the policy scheme at
 *                           t = T - 1 leaves the pool's resident arrays as v2x_eval_steps does.
 * The device functions are those of v2x_eval_steps: per pool the bits of that call (given the same Q rows).  Same rules: all
 * pointers [dev] except `pools` ([host]; the kernels take their tables by value), asynchronous, no allocation, no
 * synchronisation, no environment variable read; every check of every pool and of the mixed part before the first launch.
 * V2X_EINVAL with a text that names the pool (v2x_last_error(NULL)): n_pools outside 1..8 or a null table, link counts not
 * strictly ascending, a pool whose T is not the call's, a pool with a model of its own, anything v2x_eval_steps refuses of a
 * pool (T E_k <= 65535 among it), pools that differ in rb or in having baseline_actions, a model that is not variable_graphs
 * or whose channel count is not rb, a null xe / graph_off / row_ptr / col_idx / q or a pool's null explore with a model (xe and
 * every traj_xe 16-byte aligned), 16 R or Ed beyond INT32_MAX.  v2x_eval_steps_mixed_wide (below, after the split stream
 * phase) is this call with the wide walk in k_sim_trajectory_mixed's place.                                                   */
typedef struct v2x_eval_mixed {
  int32_t n_pools, T;               /* 1..8 pools; every pool walks the same T >= 1 steps */
  const v2x_eval* pools;            /* [host][n_pools], strictly ascending step.problem.n; pools[k].T == T;
                                       pools[k].model must be NULL; batch and q of a pool are not read */
  v2x_model* model;                 /* a variable_graphs model with rb channels, or NULL: nobody is greedy */
  float* xe; int32_t *graph_off, *row_ptr, *col_idx;   /* [dev] the ragged batch, written by the call (unused without a model) */
  float* q;                         /* [dev] [R][rb] */
} v2x_eval_mixed;
int  v2x_eval_steps_mixed(const v2x_eval_mixed* m, void* stream);

/* The wide walk: v2x_rollout_steps and v2x_eval_steps with the trajectory spread over the chip.  k_sim_trajectory walks a
 * state's T steps one after the other in one workgroup; of a step only mobility with the MT19937 stream position and the
 * shadowing recursion depend on the step before.  The wide forms replace that one launch by four, in this order on the one
 * stream, no parallel branches, no allocation, no synchronisation; the forward and the finish launch are the serial forms':
 *   k_traj_stream   grid (E), 256 threads, the key array in LDS: entry 0 and snapshot 0 as k_sim_trajectory copies them, then
 *                   T times the walk and the draws of v2x_sim_stream -- the uniforms of every step into u_all, the moved
 *                   positions into xy_all;
 *   k_traj_terms    one thread per (t, e, element), elements as in v2x_sim_channels: the path loss, the shadowing Gaussian
 *                   times its standard deviation, and the rb terms 20 log10 |h| of the fast fading, written where step t's
 *                   fast fading lives (snapshot t + 1, or the resident v2v_ff / v2i_ff for t = T - 1);
 *   k_traj_scan     one thread per (e, element): the shadowing recursion over t from the resident shadowing, path loss +
 *                   shadowing into traj_v2i_abs, the fast fading in place over its terms;
 *   k_traj_observe  one wave per (t, e), entries 1..T: the observation of v2x_sim_observe on step t's fast fading, straight
 *                   into trajectory entry t.
 * Every expression is a piece of the serial walk's, cut where that one rounds to a double: the trajectory, the results, the
 * replay slots and the resident state are the serial call's bit for bit, and the two forms (and v2x_rollout_step /
 * v2x_sim_advance) mix freely on one state.  Resident arrays written: keys, mtpos, xy, dirs, u (the uniforms of step T - 1),
 * v2i_shadow, v2v_shadow, v2v_abs, v2i_abs, v2v_ff, v2i_ff, interf_db, state, xe, mask, col, regular, and what the finish
 * launch leaves (actions, rates, interference) -- those of T calls of v2x_sim_advance.
 * wide_ws [dev]: the call's own workspace, contents undefined afterwards.  Six arrays back to back, each rounded up to a
 * multiple of 256 bytes, with n_u = n + n^2 + 2 n rb + 2 n^2 rb the uniforms of a step and n_el = n + n^2 its elements:
 *   u_all [T][E][n_u], xy_all [T][E][n][2], path loss [T][E][n_el], Gaussian term [T][E][n_el] (doubles), and what the
 *   observations of entries 1..T-1 leave beside the trajectory: state [T-1][E][n][3 rb + 1], interf_db [T-1][E][n][rb]:
 *   A(8 T E n_u) + A(16 T E n) + A(8 T E n_el) + A(8 T E n_el) + A(8 (T-1) E n (3 rb + 1)) + A(8 (T-1) E n rb),
 *   A(x) = ceil(x / 256) * 256.  v2x_traj_wide_workspace_bytes: that sum, or a negative V2X_E* code on sizes outside the limits
 *   of v2x_rollout_steps_workspace_bytes.
 * Checks: every check of v2x_rollout_steps / v2x_eval_steps, then wide_ws non-NULL and wide_ws_bytes >= the need, all before
 * the first launch (V2X_EINVAL, text in v2x_last_error(NULL)).                                                               */
int64_t v2x_traj_wide_workspace_bytes(int32_t E, int32_t n, int32_t rb, int32_t T);
int  v2x_rollout_steps_wide(const v2x_rollout_traj* r, void* wide_ws, int64_t wide_ws_bytes, void* stream);
int  v2x_eval_steps_wide(const v2x_eval* r, void* wide_ws, int64_t wide_ws_bytes, void* stream);

/* The split stream phase: the wide forms with k_traj_stream, their one serial launch, as three.  Of that launch only the
 * MT19937 recurrence, mobility (how many words a vehicle draws depends on the values drawn) and the stream position where a
 * step's uniforms begin are serial; tempering, the conversion to doubles and the stores of u_all are not.  In k_traj_stream's
 * place, in this order on the one stream (no parallel branches, no allocation, no synchronisation):
 *   k_traj_words    grid (E), 256 threads: the raw word stream of state e -- block 0 the key array at entry, word i + 624 from
 *                   words i, i + 1 and i + 397 -- 227 words per barrier through a ring in LDS, every word also stored to the
 *                   workspace; entry 0 and snapshot 0 as k_traj_stream copies them;
 *   k_traj_walk     grid (E), one wave, lane v = vehicle v: the walk of v2x_sim_stream for all T steps on those words, the
 *                   moved positions into xy_all, the offset of every step's uniforms, and keys / mtpos / xy / dirs at the end;
 *   k_traj_uniforms one thread per (t, e, i < n_u): uniform i of step t into u_all (step T - 1 also into the resident u).
 * k_traj_terms, k_traj_scan, k_traj_observe, the forward and the finish launch are the wide forms': six launches in
 * k_sim_trajectory's place.  Integer and exactly rounded arithmetic only: every byte the call leaves is the wide form's, and
 * the three forms (and v2x_rollout_step / v2x_sim_advance) mix freely on one state.
 * wide_ws [dev]: the wide forms' workspace, same size and layout.
 * split_ws [dev]: the call's own second workspace, contents undefined afterwards.  Two arrays back to back, each rounded up
 * to a multiple of 256 bytes: the words [E][NB][624] (uint32) and the offsets [T + 1][E] (int64), where
 *   NB = 1 + ceil(T (2 n_u + 4 n n_lanes) / 624)
 * blocks bound what a state can consume: a step draws 2 n_u words for its uniforms and at most one double (two words) per
 * pair of a vehicle and a lane of its two tables, and the entry position is at most 624:
 *   A(4 E NB 624) + A(8 (T + 1) E),  A(x) = ceil(x / 256) * 256.
 * v2x_traj_split_workspace_bytes: that sum, or a negative V2X_E* code on sizes outside the limits of
 * v2x_rollout_steps_workspace_bytes or n_lanes outside 1..64.  The call sizes its need by the step's own n_lanes.
 * Checks: every check of the _wide form, then split_ws non-NULL and split_ws_bytes >= the need, all before the first launch
 * (V2X_EINVAL, text in v2x_last_error(NULL)).                                                                                */
int64_t v2x_traj_split_workspace_bytes(int32_t E, int32_t n, int32_t rb, int32_t T, int32_t n_lanes);
int  v2x_rollout_steps_split(const v2x_rollout_traj* r, void* wide_ws, int64_t wide_ws_bytes, void* split_ws,
                             int64_t split_ws_bytes, void* stream);
int  v2x_eval_steps_split(const v2x_eval* r, void* wide_ws, int64_t wide_ws_bytes, void* split_ws, int64_t split_ws_bytes,
                          void* stream);

/* ---- resident rollouts of 3..128 links on the receiver replay (csrc/v2xsimdev.hip, csrc/kernels.hpp) --------------------------
 * The observation's mask / col outputs keep one 32-bit source mask per link and the one-wave observe and finish kernels need
 * n + rb <= 64: both stop the calls above at 31 links.  With one receiver per link the receivers ARE the adjacency
 * (v2x_replay_recv above), so these forms write receivers where the others write mask / col / regular, and the CSR of a
 * resident batch is one closed-form launch.  Same rules as every v2x_sim_* call: all pointers [dev], asynchronous on `stream`,
 * no allocation, no synchronisation, no environment variable read; a refusal is V2X_EINVAL with text in v2x_last_error(NULL),
 * made before anything is launched.
 *
 * v2x_sim_observe_recv: v2x_sim_observe for 3 <= n <= 128 (1 <= C <= n, 3 C + 1 <= 16).  interf_db, state and xe are
 * v2x_sim_observe's, bit for bit (one __device__ function computes the rows of both).  In place of mask / col / regular:
 * recv[E][n] int32, recv[e][q] = dest[e][q], the encoding of v2x_replay_recv (recv[q] == q: link q is its own receiver), and
 * flags[E] bytes: bit 0 -- some link of the state is its own receiver; bit 1 -- some receiver lies outside [0, n).  A state
 * with bit 1 gets NaN rows, recv[q] = q for EVERY q and bit 0 as well (that is what its recv row says), so nothing downstream
 * ever indexes with the bad receiver.  One workgroup of 128 threads per state, thread k = link k, the receivers in LDS.      */
int  v2x_sim_observe_recv(int32_t E, int32_t n, int32_t C, const int64_t* dest, const double* v2v_ff, const double* v2i_ff,
                          double p_v2i, double veh_gain, double veh_nf, double sig2, double power, double* interf_db,
                          double* state, float* xe, int32_t* recv, uint8_t* flags, void* stream);
/* v2x_csr_from_recv: row_ptr[G n + 1] and col_idx of G resident graphs of n links, nothing else.  Graph g takes the receivers
 * of state g % E of recv[E][n] (the T E observations of a trajectory share their states' receivers).  The closed form, the
 * order (packing.adj_to_csr's) and the meaning of edge_base[G + 1] (NULL: every graph regular) are v2x_replay_gather_recv's,
 * written by the same __device__ column writer; so are the bounds: no store below 0, at or beyond edge_base[g + 1] or beyond
 * (g + 1) n (n - 1); recv is compared, never used as an index.  One launch.  V2X_EINVAL: n outside 3..128, G or E < 1, a
 * null pointer other than edge_base, G n or G n (n - 1) beyond int32.                                                         */
int  v2x_csr_from_recv(int32_t G, int32_t E, int32_t n, const int32_t* recv /*[E][n]*/, const int32_t* edge_base /*[G + 1] or NULL*/,
                       int32_t* row_ptr /*[G n + 1]*/, int32_t* col_idx, void* stream);
/* v2x_rollout_steps_recv: v2x_rollout_steps_wide for 3 <= n <= 128 links (rb <= n, 3 rb + 1 <= 16, T >= 1, T E <= capacity,
 * T E n (n - 1) < 2^31), storing into ReceiverReplay's layout.  Enqueues, in this order on one stream, no parallel branches:
 *   1. the wide walk: k_traj_stream (entry 0 copied in the receiver form: xe, recv, flags; snapshot 0 unchanged), k_traj_terms
 *      and k_traj_scan -- the device functions of v2x_rollout_steps_wide, so the same bits in every stream, position and
 *      channel array;
 *   2. k_traj_observe_recv, one workgroup of 128 threads per (t, e): v2x_sim_observe_recv for entries 1..T;
 *   3. v2x_csr_from_recv for the G = T E graphs of entries 0..T-1 from the resident recv (skipped without a model);
 *   4. v2x_forward of those graphs into q (skipped without a model);
 *   5. k_rollout_finish_recv, one workgroup of 192 threads per transition (n + rb <= 144 of them compute a rate): the pick,
 *      rates, summation and reward functions of k_rollout_finish; xe of entry t and xe' of entry t + 1 (16-byte words), recv,
 *      action and reward into slot (head + t E + e) % capacity; the transitions of t = T - 1 also leave the resident actions
 *      and rate arrays.
 * A state with an own-receiver link is scored and stored like any other (its CSR is closed-form): there is no fallback.
 * The caller validates dest on the host, and, only when some state has an own-receiver link, passes edge_base[T E + 1] (the
 * cumulative sum of n (n - 2) + own(g % E)) and sizes batch.n_edges / batch.max_edges by it (v2x_replay_gather_recv's rule).
 * In `r`: `step` is a v2x_sim_step whose mask / col / regular are not read (the resident observation is xe / state /
 * interf_db of `step` plus recv / flags here); batch: on_device, T E graphs of n rows, max_nodes = n, xe = traj_xe, row_ptr /
 * col_idx those of this struct, n_edges = T E n (n - 2) and max_edges = n (n - 2) without edge_base, else T E n (n - 2) <=
 * n_edges <= T E n (n - 1) and max_edges = n (n - 1); explore [T][E], random_actions [T][E][n], q [T E n][rb]; result_reward
 * [T][E], result_flags [T][2][E] (row t: the flags of the stored observation, then of the next one).
 * ws: ONE allocation of v2x_rollout_recv_workspace_bytes(E, n, rb, T) bytes, fourteen arrays back to back, each rounded up
 * to a multiple of 256 bytes -- first the eight the struct points into, which MUST be these sections in this order,
 *   traj_xe, traj_recv, traj_flags, traj_v2v_ff, traj_v2i_ff, traj_v2i_abs, row_ptr, col_idx,
 * then the wide walk's own six (v2x_traj_wide_workspace_bytes), contents undefined afterwards:
 *   A(4 (T+1) E n 16) + A(4 (T+1) E n) + A((T+1) E) + A(8 T E n n rb) + A(8 T E n rb) + A(8 T E n) + A(4 (T E n + 1))
 *   + A(4 T E n (n-1)) + A(8 T E n_u) + A(16 T E n) + A(8 T E n_el) + A(8 T E n_el) + A(8 (T-1) E n (3 rb + 1))
 *   + A(8 (T-1) E n rb),   n_u = n + n^2 + 2 n rb + 2 n^2 rb, n_el = n + n^2, A(x) = ceil(x / 256) * 256.
 * v2x_rollout_recv_workspace_bytes: that sum, or a negative V2X_E* code outside the limits.  ws must be 256-byte aligned;
 * rep_xe / rep_xe_next 16-byte aligned.  A refused call leaves state and storage alone.                                      */
typedef struct v2x_rollout_recv {
  v2x_model* model;                /* the online network, or NULL: nobody is greedy */
  v2x_batch batch;
  float* q;                        /* [T E n][rb] Q workspace (required with a model) */
  const uint8_t* explore;          /* [T][E]    */
  const int32_t* random_actions;   /* [T][E][n] */
  int32_t* actions;                /* [E][n]: the resident actions (those of step T - 1) */
  v2x_sim_step step;               /* mask / col / regular not read; actions NULL or `actions` */
  int32_t* recv;                   /* [E][n]  the resident observation's receivers */
  uint8_t* flags;                  /* [E]     and flag bytes */
  double w_v2v, w_v2i;
  int32_t T, pad_;
  float* traj_xe;                  /* [T+1][E][n][16]  */
  int32_t* traj_recv;              /* [T+1][E][n]      */
  uint8_t* traj_flags;             /* [T+1][E]         */
  double* traj_v2v_ff;             /* [T][E][n][n][rb] */
  double* traj_v2i_ff;             /* [T][E][n][rb]    */
  double* traj_v2i_abs;            /* [T][E][n]        */
  int32_t* row_ptr;                /* [T E n + 1]      */
  int32_t* col_idx;                /* [T E n (n - 1)]  */
  const int32_t* edge_base;        /* [T E + 1] device-addressable, or NULL: every state regular */
  float *rep_xe, *rep_xe_next;     /* [capacity][n][16] */
  int32_t *rep_recv, *rep_action;  /* [capacity][n]     */
  double* rep_reward;              /* [capacity]        */
  int64_t head, capacity;
  double* result_reward;           /* [T][E]    */
  uint8_t* result_flags;           /* [T][2][E] */
} v2x_rollout_recv;
int64_t v2x_rollout_recv_workspace_bytes(int32_t E, int32_t n, int32_t rb, int32_t T);
int  v2x_rollout_steps_recv(const v2x_rollout_recv* r, void* ws, int64_t ws_bytes, void* stream);
/* v2x_rollout_steps_recv_split: v2x_rollout_steps_recv with the split stream phase -- step 1's k_traj_stream as three launches,
 *   k_traj_words_recv  grid (E), 256 threads: k_traj_words with entry 0 copied in the receiver form (xe, recv, flags);
 *   k_traj_walk_recv   grid (E), one wave, lane l = vehicles l and l + 64: k_traj_walk's walk for up to 128 vehicles, walkers
 *                      in vehicle index order (the low half, then the high half), the same word reads, draws and arithmetic;
 *   k_traj_uniforms    as in v2x_rollout_steps_split;
 * then k_traj_terms, k_traj_scan and steps 2..5 of v2x_rollout_steps_recv with the same arguments.  Integer and exactly rounded
 * arithmetic only: every byte the call leaves (state, workspace sections, storage, results) is v2x_rollout_steps_recv's, and
 * the two forms mix freely on one state.  `r`, ws, ws_bytes: as there.
 * split_ws [dev]: the call's own second workspace, 256-byte aligned, contents undefined afterwards: the words [E][NB][624]
 * (uint32) and the offsets [T + 1][E] (int64) of v2x_traj_split_workspace_bytes, the same formula for 3..128 links,
 *   NB = 1 + ceil(T (2 n_u + 4 n n_lanes) / 624),   A(4 E NB 624) + A(8 (T + 1) E),   A(x) = ceil(x / 256) * 256
 * (about 36 MB per state at 100 links, rb = 4, T = 50, 59.9 MB at 128 links with 2 lanes per direction; linear in E).
 * v2x_rollout_recv_split_workspace_bytes: that sum, or a negative V2X_E* code on sizes outside the limits of
 * v2x_rollout_recv_workspace_bytes or n_lanes outside 1..64.  The call sizes its need by the step's own n_lanes.
 * Checks: every check of v2x_rollout_steps_recv, then split_ws non-NULL, 256-byte aligned and split_ws_bytes >= the need, all
 * before the first launch (V2X_EINVAL, text in v2x_last_error(NULL)); a refused call leaves state and storage alone.          */
int64_t v2x_rollout_recv_split_workspace_bytes(int32_t E, int32_t n, int32_t rb, int32_t T, int32_t n_lanes);
int  v2x_rollout_steps_recv_split(const v2x_rollout_recv* r, void* ws, int64_t ws_bytes, void* split_ws, int64_t split_ws_bytes,
                                  void* stream);
/* v2x_eval_steps_recv: v2x_eval_steps for 3 <= n <= 128 links -- the T steps of an EVALUATION episode in one call on the
 * receiver-form resident state, no replay memory.  Enqueues, in this order on one stream, no parallel branches: steps 1..4 of
 * v2x_rollout_steps_recv with the same arguments (the wide walk, k_traj_observe_recv, v2x_csr_from_recv and v2x_forward, the
 * last two skipped without a model: one body serves both calls), then
 *   5. k_eval_finish_recv, grid (S T E), scheme major, one workgroup of 192 threads per (scheme, t, e), S = 2 with
 *      baseline_actions, else 1: the body of k_eval_finish (one __device__ function, called by both), so the pick, the rates of
 *      v2x_sim_rates on snapshot t, the summation and the reward of v2x_eval_steps, scheme 0 the policy, scheme 1 the baseline;
 *      the policy scheme at t = T - 1 leaves actions / v2v_rate / v2i_rate / interference / v2i_interf / v2v_interf in the
 *      resident arrays.
 * After the call the resident state (streams, positions, channel arrays, xe / state / interf_db / recv / flags of entry T,
 * actions and rates) is what T calls of v2x_sim_advance under the policy's actions leave.  A state with an own-receiver link is
 * scored like any other: edge_base and the batch's n_edges / max_edges follow v2x_rollout_steps_recv's rule; no fallback.
 * Results, scheme major, the layout and section order of v2x_eval_steps: result_v2v_rate [S][T][E][n], result_v2i_rate
 * [S][T][E][min(rb, n)], result_interference [S][T][E][rb], result_reward [S][T][E] (doubles), result_actions [S][T][E][n]
 * (int32), then result_flags [T+1][E], the FLAG BYTES of entries 0..T (v2x_sim_observe_recv's bits) where v2x_eval_steps has
 * result_regular.  v2x_eval_recv_result_bytes(E, n, rb, T, S): 8 S T E (n + min(rb, n) + rb + 1) + 4 S T E n + (T + 1) E rounded
 * up to a multiple of 8, or a negative V2X_E* code outside the limits of v2x_rollout_recv_workspace_bytes, S outside {1, 2} or
 * T E > 65535 (the stacked searches of v2x_opt_* take the T E snapshots as one problem).
 * ws, ws_bytes: the workspace of v2x_rollout_recv_workspace_bytes(E, n, rb, T), its first eight sections checked as there (a
 * rollout and an evaluation of one T may share it).  Same rules: all pointers [dev], asynchronous, no allocation, no
 * synchronisation, no environment variable read; every check before the first launch (V2X_EINVAL, text in
 * v2x_last_error(NULL)); a refused call leaves the resident state and the result block alone.                              */
typedef struct v2x_eval_recv {
  v2x_model* model;                /* the network, or NULL: the policy takes random_actions everywhere, explore is not read */
  v2x_batch batch;
  float* q;                        /* [T E n][rb] Q workspace (required with a model) */
  const uint8_t* explore;          /* [T][E] (required with a model) */
  const int32_t* random_actions;   /* [T][E][n]: the policy's random actions */
  const int32_t* baseline_actions; /* [T][E][n], or NULL: no baseline scheme */
  int32_t* actions;                /* [E][n]: the resident actions (written: the policy's of t = T - 1) */
  v2x_sim_step step;               /* mask / col / regular not read; actions NULL or `actions` */
  int32_t* recv;                   /* [E][n]  the resident observation's receivers */
  uint8_t* flags;                  /* [E]     and flag bytes */
  double w_v2v, w_v2i;
  int32_t T, pad_;
  float* traj_xe;                  /* [T+1][E][n][16]  */
  int32_t* traj_recv;              /* [T+1][E][n]      */
  uint8_t* traj_flags;             /* [T+1][E]         */
  double* traj_v2v_ff;             /* [T][E][n][n][rb] */
  double* traj_v2i_ff;             /* [T][E][n][rb]    */
  double* traj_v2i_abs;            /* [T][E][n]        */
  int32_t* row_ptr;                /* [T E n + 1]      */
  int32_t* col_idx;                /* [T E n (n - 1)]  */
  const int32_t* edge_base;        /* [T E + 1] device-addressable, or NULL: every state regular */
  int32_t* result_actions;         /* [S][T][E][n]         */
  double* result_v2v_rate;         /* [S][T][E][n]         */
  double* result_v2i_rate;         /* [S][T][E][min(rb,n)] */
  double* result_interference;     /* [S][T][E][rb]        */
  double* result_reward;           /* [S][T][E]            */
  uint8_t* result_flags;           /* [T+1][E]             */
} v2x_eval_recv;
int64_t v2x_eval_recv_result_bytes(int32_t E, int32_t n, int32_t rb, int32_t T, int32_t schemes);
int  v2x_eval_steps_recv(const v2x_eval_recv* r, void* ws, int64_t ws_bytes, void* stream);
/* v2x_eval_steps_recv_split: v2x_eval_steps_recv with the split stream phase of v2x_rollout_steps_recv_split (k_traj_words_recv,
 * k_traj_walk_recv, k_traj_uniforms in k_traj_stream's place) on the second workspace of
 * v2x_rollout_recv_split_workspace_bytes.  Every byte the call leaves is v2x_eval_steps_recv's; the forms mix freely on one
 * state.  Checks: every check of v2x_eval_steps_recv first, then split_ws non-NULL, 256-byte aligned and split_ws_bytes >= the
 * need, all before the first launch.                                                                                        */
int  v2x_eval_steps_recv_split(const v2x_eval_recv* r, void* ws, int64_t ws_bytes, void* split_ws, int64_t split_ws_bytes,
                               void* stream);

/* The mixed wide walk: v2x_rollout_steps_mixed and v2x_eval_steps_mixed with every pool's trajectory spread over the chip --
 * the wide walk with the split stream phase, for all link counts at once.  Both calls enqueue, on the one stream with no
 * parallel branches, exactly what their serial siblings enqueue, with six launches in k_sim_trajectory_mixed's place; each is
 * the body of its single-size kernel on the arguments of the block's pool (one table of the pools' arguments by value, the
 * pool found from the block index alone, the largest pool's blocks in the lowest indices):
 *   k_traj_words_mixed     grid (S E_k), 256 threads: the body of k_traj_words for state e of its pool;
 *   k_traj_walk_mixed      grid (S E_k), one wave: the body of k_traj_walk;
 *   k_traj_uniforms_mixed  grid (S_k ceil(T E_k n_u,k / 256)), 256 threads: the body of k_traj_uniforms, one thread per
 *                          (t, e, i < n_u,k) of its pool -- a pool's padded last block touches nothing of the next pool;
 *   k_traj_terms_mixed     grid (S_k ceil(T E_k n_el,k / 256)): the body of k_traj_terms, n_el,k = n_k + n_k^2;
 *   k_traj_scan_mixed      grid (S_k ceil(E_k n_el,k / 256)): the body of k_traj_scan;
 *   k_traj_observe_mixed   grid (T S E_k), one wave: the body of k_traj_observe for entry (t, e) of its pool.
 * k_traj_assemble_mixed, v2x_forward and k_rollout_finish_mixed / k_eval_finish_mixed follow unchanged.  Per pool every byte
 * the call leaves -- resident state, trajectory, replay slots or results, and the pool's two workspaces -- is that of the
 * serial mixed call and of the pool's own v2x_rollout_steps_split / v2x_eval_steps_split; the forms mix freely on one state.
 * There is no mixed form of the chained k_traj_stream.
 * ws [host][n_pools]: per pool its own wide and split workspaces [dev], sized by the pool's own E_k, n_k, rb, T and n_lanes
 * (v2x_traj_wide_workspace_bytes, v2x_traj_split_workspace_bytes), contents undefined afterwards.
 * Checks: every check of the serial mixed call, then ws non-NULL and per pool the checks of the _wide and _split forms, all
 * before the first launch (V2X_EINVAL, the text names the pool: "pool k (n links): ..."); a refused call writes nothing.     */
typedef struct v2x_traj_ws {
  void* wide_ws;  int64_t wide_ws_bytes;     /* v2x_traj_wide_workspace_bytes(E_k, n_k, rb, T)            */
  void* split_ws; int64_t split_ws_bytes;    /* v2x_traj_split_workspace_bytes(E_k, n_k, rb, T, n_lanes_k) */
} v2x_traj_ws;
int  v2x_rollout_steps_mixed_wide(const v2x_rollout_mixed* m, const v2x_traj_ws* ws /*[host][n_pools]*/, void* stream);
int  v2x_eval_steps_mixed_wide(const v2x_eval_mixed* m, const v2x_traj_ws* ws /*[host][n_pools]*/, void* stream);

/* v2x_eval_sweep_mixed: K networks scored on the SAME T steps of up to 8 pools of different link counts -- the checkpoints of a
 * training run on one walked episode (rl/mixed.py MixedAgent.evaluate_training).  Nothing in a simulator step depends on the
 * actions except the rates paid for them, so the walk, the ragged batch and the baseline are those of ONE v2x_eval_steps_mixed
 * call; only the forward and the policy's pick differ between the networks.  Enqueues, in this order on one stream with no
 * parallel branches,
 *   the walk                    k_sim_trajectory_mixed (ws NULL), or the six launches of the mixed wide walk on `ws`, unchanged;
 *   k_traj_assemble_mixed       unchanged, once -- skipped without models;
 *   v2x_forward                 K times, of that one batch: models[k] into q + k R rb -- skipped without models;
 *   k_eval_finish_sweep_mixed   grid (S T S(E_j)), S = K + 1 with baseline_actions, else K; one wave per (pool, scheme, t, e): the
 *                               body of k_eval_finish on its pool's arguments.  Scheme k < K is the policy of network k: link i
 *                               takes random_actions[t][e][i] when explore[t][e], else np.argmax of its row of models[k]'s Q --
 *                               explore and random_actions are shared by all K.  Scheme K is the baseline.  Scheme K - 1 at
 *                               t = T - 1 leaves the pool's resident actions, rates and interference, as scheme 0 of
 *                               v2x_eval_steps_mixed does: the resident state afterwards is that of K calls of
 *                               v2x_eval_steps_mixed with models[0..K-1], each started from the state before the first.
 *                               Pool-major: pool j owns blocks S gbase_j .. S gbase_j + S T E_j - 1, inside a pool (scheme, t, e).
 * Results: pool j's result pointers hold S schemes, scheme major, [S][T][E_j][..] -- the layout of v2x_eval_steps with S in the
 * place of its 1 or 2; v2x_eval_sweep_result_bytes(E, n, rb, T, S) is the formula of v2x_eval_steps_result_bytes for
 * 1 <= S <= 65.  Scheme k of the sweep holds the bits of scheme 0 of v2x_eval_steps_mixed with models[k], scheme K those of its
 * scheme 1.
 * Same rules as v2x_eval_steps_mixed: all pointers [dev] except `base.pools` and `models` ([host]), asynchronous, no allocation,
 * no synchronisation, no environment variable read; every check of every part before the first launch.  V2X_EINVAL (text in
 * v2x_last_error(NULL)): K outside 1..64, a NULL entry of models, models that are not variable_graphs or differ in channels,
 * feature width, depth or weight sharing, a null q with models, and everything v2x_eval_steps_mixed (with ws: and
 * v2x_eval_steps_mixed_wide) refuses of base, its pools and the ragged batch.                                               */
typedef struct v2x_eval_sweep {
  v2x_eval_mixed base;              /* as for v2x_eval_steps_mixed; base.model and base.q are ignored */
  int32_t K, pad_;                  /* 1..64 networks */
  v2x_model* const* models;         /* [host][K] variable_graphs models of one spec with rb channels, or NULL: everybody explores */
  float* q;                         /* [dev] [K][R][rb] Q workspace, R the rows of the ragged batch (required with models) */
} v2x_eval_sweep;
int64_t v2x_eval_sweep_result_bytes(int32_t E, int32_t n, int32_t rb, int32_t T, int32_t schemes);
int  v2x_eval_sweep_mixed(const v2x_eval_sweep* s, const v2x_traj_ws* ws /*[host][n_pools] or NULL*/, void* stream);

/* v2x_eval_sweep_recv: v2x_eval_sweep_mixed's idea for 3 <= n <= 128 links on the receiver-form resident state -- K fixed-size
 * networks (the checkpoints of a training run, rl/agent.py Agent.evaluate_training_sweep) scored on the SAME T steps.  Enqueues,
 * in this order on one stream with no parallel branches,
 *   the front of v2x_eval_steps_recv   once, unchanged, with model = models[0] and q = this struct's q: the wide walk (chain
 *                                      stream phase), k_traj_observe_recv and, with models, v2x_csr_from_recv and models[0]'s forward;
 *   v2x_forward                        K - 1 times, of that one batch (same CSR, same edge_base): models[k] into q + k T E n rb;
 *   k_eval_finish_sweep_recv           grid (S T E), scheme major, S = K + 1 with base.baseline_actions, else K; 192 threads per
 *                                      (scheme, t, e): the body of k_eval_finish_recv on the block's view.  Scheme k < K is the
 *                                      policy of network k on the shared explore / random_actions, scheme K the baseline.  Only
 *                                      network K - 1 at t = T - 1 leaves the resident actions, rates and interference.
 * Results: the layout of v2x_eval_steps_recv with S in place of its 1 or 2, [S][T][E][..] sections in the same order, then
 * result_flags [T+1][E]; v2x_eval_sweep_recv_result_bytes(E, n, rb, T, S) is the formula of v2x_eval_recv_result_bytes for
 * 1 <= S <= 65 (negative outside, and for T E > 65535 or outside the limits of v2x_rollout_recv_workspace_bytes).  Scheme k
 * holds the bits of scheme 0 of v2x_eval_steps_recv with models[k] from the state before the call, scheme K those of its scheme
 * 1; every byte of resident state and of the workspace's eight sections afterwards is what v2x_eval_steps_recv with
 * models[K - 1] leaves.  v2x_eval_sweep_recv_split: the same with the split stream phase on the second workspace of
 * v2x_rollout_recv_split_workspace_bytes; every byte it leaves is the chain form's.
 * Same rules as v2x_eval_steps_recv: all pointers [dev] except `models` ([host]), asynchronous, no allocation, no
 * synchronisation, no environment variable read; every check before the first launch.  V2X_EINVAL (text in
 * v2x_last_error(NULL)), nothing launched or written: a null s, K outside 1..64, a NULL entry of models, models that are not
 * fixed-size models of n links and rb channels or differ in feature width, depth or weight sharing, a null q with models, and
 * everything v2x_eval_steps_recv / _split refuses of base, ws and split_ws.  (An error v2x_forward itself returns for
 * models[k], k >= 1 -- none is known for a model that passed these checks, its shape being models[0]'s -- comes back after the
 * front has run: the walk is made, the results are not; the same holds for v2x_eval_sweep_mixed.)                            */
struct v2x_eval_sweep_recv {         /* (a tag, not a typedef: the call below bears the same name) */
  v2x_eval_recv base;               /* as for v2x_eval_steps_recv; base.model and base.q are ignored */
  int32_t K, pad_;                  /* 1..64 networks */
  v2x_model* const* models;         /* [host][K], or NULL: everybody explores, no CSR, no forward */
  float* q;                         /* [dev] [K][T E n][rb] (required with models) */
};
int64_t v2x_eval_sweep_recv_result_bytes(int32_t E, int32_t n, int32_t rb, int32_t T, int32_t schemes);
int  v2x_eval_sweep_recv(const struct v2x_eval_sweep_recv* s, void* ws, int64_t ws_bytes, void* stream);
int  v2x_eval_sweep_recv_split(const struct v2x_eval_sweep_recv* s, void* ws, int64_t ws_bytes, void* split_ws, int64_t split_ws_bytes,
                               void* stream);

/* ---- jump-ahead MT19937: the words of the split stream phase drawn in chunks ---------------------------------------------
 * MT19937 is linear over GF(2).  Let w[0..623] be a key array and w[i + 624] = twist(w[i], w[i + 1], w[i + 397]) -- the raw word
 * stream k_traj_words_recv writes.  Let phi be the characteristic polynomial of that recurrence (degree 19937), and for J >= 0
 * g = x^J mod phi with coefficients g_0 .. g_19936.  Then for every m >= 1, on all 32 bits,
 *     w[J + m] = XOR over { i : g_i = 1 } of w[i + m]
 * (m = 0 holds on bit 31 only: the low 31 bits of w[0] are not part of the generator's state).  So the 624 words from stream
 * index c on are   w[c + k] = XOR_i g_i w[1 + i + k],  k = 0..623,  g = x^(c - 1) mod phi:   they need the prefix w[1 .. 20560]
 * and a polynomial that depends on c alone, not on the seed or the simulator.
 * v2x_mt_jump_polys [host, no GPU call]: out[p] = the coefficients of x^(first - 1 + p stride) mod phi, p = 0 .. count - 1,
 * coefficient i in bit i & 31 of word i >> 5 (the 31 unused top bits of word 623 are zero).  phi comes from Berlekamp-Massey on
 * the library's own word stream (once per process); the first power by square-and-reduce, each further one by a product with
 * x^stride mod phi.  V2X_EINVAL (text in v2x_last_error(NULL)): first < 20561, stride < 624, count < 1, a null out.
 *
 * v2x_rollout_steps_recv_jump / v2x_eval_steps_recv_jump / v2x_eval_sweep_recv_jump: the _split forms with k_traj_words_recv's
 * work cut into chunks.  Chunk 0 is [0, first); chunk p = 1 .. count is [c_p, c_p+1) with c_p = first + (p - 1) stride and the
 * last one running to nbw = 624 NB.  Three launches stand in k_traj_words_recv's place:
 *   k_traj_words_recv   grid (E): unchanged, with its loop bound at `first` instead of nbw (entry 0 copied as before);
 *   k_traj_jump_seeds   grid (8, count, E), 256 threads: slice s of polynomial p against the prefix of state e -- the prefix words
 *                       the slice needs staged in LDS, three k per thread, the coefficient bits walked on the scalar side --
 *                       into scratch[e][p][s][624];
 *   k_traj_jump_chunks  grid (count, E), 256 threads: the XOR of the eight slices is words[c_p .. c_p + 624), stored and loaded
 *                       into the ring at the slots k_traj_words_recv uses for those indices, then the same round loop (one
 *                       function) up to the chunk's end.
 * Every word of the array has one writer, and the array is k_traj_words_recv's bit for bit, so k_traj_walk_recv, k_traj_uniforms
 * and everything after them run unchanged: every byte the calls leave is the _split form's.
 * jump->polys [dev]: the table of v2x_mt_jump_polys(first, stride, count); jump->scratch [dev]: v2x_mt_jump_scratch_bytes(E,
 * count) = A(4 E count 8 624) bytes (0 for count = 0; negative V2X_EINVAL for E < 1 or count < 0), contents undefined afterwards.
 * count = 0, or first >= nbw, is legal and runs the _split form's launches.  Checks, after every check of the _split form and
 * before the first launch (V2X_EINVAL, text in v2x_last_error(NULL), nothing written): a null jump; first < 20561; stride < 624;
 * count < 0; with chunks to run, polys or scratch null or not 256-byte aligned, first + (count - 1) stride >= nbw (an empty last
 * chunk), scratch_bytes below the need.                                                                                      */
typedef struct v2x_mt_jump {
  int64_t first, stride;            /* chunk p >= 1 begins at first + (p - 1) stride */
  int32_t count, pad_;              /* polynomials = chunks after the prefix */
  const uint32_t* polys;            /* [dev] [count][624] */
  void* scratch;                    /* [dev] v2x_mt_jump_scratch_bytes(E, count) */
  int64_t scratch_bytes;
} v2x_mt_jump;
int  v2x_mt_jump_polys(int64_t first, int64_t stride, int32_t count, uint32_t* out /* [host] [count][624] */);
int64_t v2x_mt_jump_scratch_bytes(int32_t E, int32_t count);
int  v2x_rollout_steps_recv_jump(const v2x_rollout_recv* r, void* ws, int64_t ws_bytes, void* split_ws, int64_t split_ws_bytes,
                                 const v2x_mt_jump* jump, void* stream);
int  v2x_eval_steps_recv_jump(const v2x_eval_recv* r, void* ws, int64_t ws_bytes, void* split_ws, int64_t split_ws_bytes,
                              const v2x_mt_jump* jump, void* stream);
int  v2x_eval_sweep_recv_jump(const struct v2x_eval_sweep_recv* s, void* ws, int64_t ws_bytes, void* split_ws, int64_t split_ws_bytes,
                              const v2x_mt_jump* jump, void* stream);

/* ---- measurement ------------------------------------------------------------------------ */
/* When enabled, every kernel launch of this model is bracketed by HIP events on its stream
 * (eager, no graph); v2x_profile_read returns per-kernel-name call counts and total ms.    */
int  v2x_profile_enable(v2x_model* m, int enable);
/* Which kernels a fit step of `b` runs on this model, as text ("graph_layers=fused aggregation=complement mlp=train_wg
 * handoff=fragment-major"): the aggregation is the general edge-index gather / segment sum of AggLayer.call
 * (BS_brain.py:69-76) unless the batch is dense enough for one of its rewritings -- through the complement in the fused
 * graph-layer kernels ("complement"), per graph through the complement or as an MFMA product with adjacency bit masks for large dense graphs
 * ("dense(complement-or-mfma-per-graph)").
 * Only sizes and null-ness of the batch pointers are read.  bench.py prints it in `config.aggregation`.              */
int  v2x_path_info(v2x_model* m, const v2x_batch* b, char* out, int cap);
/* Models created with V2X_FUSED_TS=1 in the environment run a measurement build of the fused forward kernel in which
 * workgroup 7 writes 100 MHz time stamps at its phase boundaries: out[wave * 64 + mark], n <= 512 entries.            */
int  v2x_debug_phase_stamps(v2x_model* m, int64_t* out, int n);
/* Tests: the work plan of the last ragged fused forward (csrc/kernels_ragged.hpp) -- out[w] = first graph of workgroup w for
 * w = 0 .. n - 1 (entries past the plan's length are left alone); returns the plan's length (launched workgroups + 1) or a
 * negative error code.  [host] out. */
int  v2x_debug_ragged_plan(v2x_model* m, int32_t* out, int n);
/* Tests: how the last backward pass cut its weight gradients -- the partial-sum slabs written per layer, graph layers 0 .. L
 * (0 = the embed layer) and then Dense 0 .. 3 (0 slabs: the layer's gradient was written in place), followed by the threads per
 * column (1, 4 or 16) of the last slab sum / Adam launch.  n >= L + 6; returns the number of values written (L + 6) or a
 * negative error code.  Launches nothing.  [host] out. */
int  v2x_debug_layer_slabs(v2x_model* m, int32_t* out, int n);
/* Tests: how a wide GEMM launch (feat_dim >= 128: node update, Dense-0 and their data gradients) of n_idx rows per weight slot,
 * grid_z slots and n_out output columns is cut for `slots` resident workgroups -- out = {ny column tiles, mbs 128-row blocks per
 * slot, n_full_rb, n_rb}: row blocks [0, n_full_rb) of the slot-major enumeration run as one 128-row tile per column tile, the
 * other n_rb - n_full_rb as two 64-row half tiles.  tail = V2X_WIDE_TAIL (0, 1 or 2).  The rule the launches themselves use,
 * with slots = five per compute unit unless V2X_WIDE_SLOTS says otherwise.  Host arithmetic: no model, no GPU.  [host] out. */
int  v2x_wide_tiling_plan(int32_t n_idx, int32_t grid_z, int32_t n_out, int32_t slots, int32_t tail, int32_t out[4]);
/* Tests: what the model's wide launches were since the previous call of this function -- out[0] = A wide GEMM launches kept (the
 * first 32), out[1] = B wide weight-gradient roles kept (the first 16), then A x {ny, mbs, n_full_rb, n_rb} (v2x_wide_tiling_plan)
 * in launch order, then B x {K tiles, column tiles, row splits, 1 if the [x | e] segment rides on K tile 0} in the order the roles
 * were planned.  Recorded where the launches are enqueued: a hipGraph capture records, its replays do not.  n >= 2 + 4 A + 4 B
 * (194 is always enough); returns the number of values written or a negative error code.  Launches nothing.  [host] out. */
int  v2x_debug_wide_tiling(v2x_model* m, int32_t* out, int n);
int  v2x_profile_read(v2x_model* m, char* names_out, int names_cap, double* ms_out, int64_t* calls_out,
                      int max_entries);   /* returns number of entries, names '\n'-separated */

#ifdef __cplusplus
}
#endif
#endif /* V2XGNN_H */
