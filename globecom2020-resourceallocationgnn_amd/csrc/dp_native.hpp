// dp_native.hpp -- data parallelism driven by the library (include/v2xgnn.h, "data parallelism driven by the library").
// Included at the end of v2xgnn.hip: the orchestration below uses that translation unit's helpers (fwd_bwd, the phases,
// launch_reduce_adam, launch_pack, emit_loss).  No kernels of its own: the collectives come from a v2x_comm table, either the
// caller's or the RCCL table built here.
#include <dlfcn.h>

namespace {

// ------------------------------------------------------------------------------------------------------- RCCL at run time
// RCCL is resolved with dlopen, so that libv2xgnn.so loads where RCCL is absent.  Inside a PyTorch process the soname finds
// torch's bundled copy (the same soname): one RCCL per process.
struct NcclId { char internal[128]; };
constexpr int NCCL_FLOAT32 = 7, NCCL_SUM = 0;

struct Rccl {
  void* h = nullptr;
  std::string err;
  int (*get_unique_id)(NcclId*) = nullptr;
  int (*comm_init_rank)(void**, int, NcclId, int) = nullptr;
  int (*comm_destroy)(void*) = nullptr;
  int (*all_reduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*reduce_scatter)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*all_gather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
  const char* (*error_string)(int) = nullptr;
};

Rccl load_rccl() {
  Rccl r;
  for (const char* name : {"librccl.so.1", "/opt/rocm/lib/librccl.so.1"}) {
    r.h = dlopen(name, RTLD_NOW | RTLD_LOCAL);
    if (r.h) break;
    const char* e = dlerror();
    r.err += std::string(r.err.empty() ? "" : "; ") + (e ? e : name);
  }
  if (!r.h) { r.err = "RCCL not found (" + r.err + ")"; return r; }
  bool ok = true;
  auto sym = [&](auto& fn, const char* name) {
    fn = reinterpret_cast<std::remove_reference_t<decltype(fn)>>(dlsym(r.h, name));
    if (!fn) { ok = false; r.err += std::string(" missing ") + name; }
  };
  sym(r.get_unique_id, "ncclGetUniqueId");
  sym(r.comm_init_rank, "ncclCommInitRank");
  sym(r.comm_destroy, "ncclCommDestroy");
  sym(r.all_reduce, "ncclAllReduce");
  sym(r.reduce_scatter, "ncclReduceScatter");
  sym(r.all_gather, "ncclAllGather");
  sym(r.error_string, "ncclGetErrorString");
  if (!ok) { dlclose(r.h); r.h = nullptr; r.err = "RCCL lacks symbols:" + r.err; }
  return r;
}

const Rccl* rccl(std::string* why) {
  static const Rccl r = load_rccl();          // once per process
  if (!r.h) { *why = r.err; return nullptr; }
  return &r;
}

struct RcclCtx { const Rccl* r; void* comm; int world, rank; };

// the table's entries: in place, on `stream`
int rccl_all_reduce(float* buf, int64_t n, void* stream, void* ctx) {
  const RcclCtx* c = static_cast<const RcclCtx*>(ctx);
  return c->r->all_reduce(buf, buf, (size_t)n, NCCL_FLOAT32, NCCL_SUM, c->comm, (hipStream_t)stream);
}
int rccl_reduce_scatter(float* buf, int64_t n, void* stream, void* ctx) {
  const RcclCtx* c = static_cast<const RcclCtx*>(ctx);
  if (n % c->world) return -1;
  const size_t cnt = (size_t)(n / c->world);
  return c->r->reduce_scatter(buf, buf + c->rank * cnt, cnt, NCCL_FLOAT32, NCCL_SUM, c->comm, (hipStream_t)stream);
}
int rccl_all_gather(float* buf, int64_t n, void* stream, void* ctx) {
  const RcclCtx* c = static_cast<const RcclCtx*>(ctx);
  if (n % c->world) return -1;
  const size_t cnt = (size_t)(n / c->world);
  return c->r->all_gather(buf + c->rank * cnt, buf, cnt, NCCL_FLOAT32, c->comm, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------------------- the step
int n_loss_outputs(const v2x_model* m) { return m->cfg.variable_graphs ? 1 : m->N; }

int dp_check_comm(v2x_model* m, const v2x_comm* c, int form, const char* who) {
  if (!c) FAIL(m, V2X_EINVAL, "%s: null comm", who);
  if (c->world < 1 || c->rank < 0 || c->rank >= c->world)
    FAIL(m, V2X_EINVAL, "%s: comm rank %d of world %d", who, (int)c->rank, (int)c->world);
  if (form < V2X_DP_ALLREDUCE || form > V2X_DP_SHARDED) FAIL(m, V2X_EINVAL, "%s: unknown form %d", who, form);
  if (!c->all_reduce_sum) FAIL(m, V2X_EINVAL, "%s: comm.all_reduce_sum is null", who);
  if (form == V2X_DP_SHARDED && (!c->reduce_scatter_sum || !c->all_gather))
    FAIL(m, V2X_EINVAL, "%s: the sharded form needs comm.reduce_scatter_sum and comm.all_gather", who);
  return V2X_OK;
}

typedef int (*CollFn)(float*, int64_t, void*, void*);

// one collective of the table; `what` names its buffer for the error text
int dp_call(v2x_model* m, const v2x_comm* c, CollFn fn, const char* coll, const char* what, float* buf, int64_t n,
            hipStream_t st) {
  const int rc = fn(buf, n, (void*)st, c->ctx);
  if (rc != 0) FAIL(m, V2X_ECOMM, "%s of %s (%lld floats) returned %d", coll, what, (long long)n, rc);
  return V2X_OK;
}

// the model's collective stream and its events: made on the first data-parallel step, freed by v2x_destroy
int dp_ensure_stream(v2x_model* m) {
  if (!m->dp_st) HIPCHK(m, hipStreamCreateWithFlags(&m->dp_st, hipStreamNonBlocking));
  const size_t need = (size_t)n_phase_buckets(m) + 1;
  while (m->dp_ev.size() < need) {
    hipEvent_t e = nullptr;
    HIPCHK(m, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    m->dp_ev.push_back(e);
  }
  return V2X_OK;
}

// `to` waits for everything enqueued on `from` so far
int dp_join(v2x_model* m, hipEvent_t ev, hipStream_t from, hipStream_t to) {
  HIPCHK(m, hipEventRecord(ev, from));
  HIPCHK(m, hipStreamWaitEvent(to, ev, 0));
  return V2X_OK;
}

// the slice of an n-float bucket a rank owns under the sharded form (DataParallelTrainer._slice_of): cut into `world` equal
// float4-aligned slices, or not at all (-1)
int64_t dp_slice(const v2x_comm* c, int64_t n, int64_t* count) {
  if (n % (4 * (int64_t)c->world)) return -1;
  *count = n / c->world;
  return c->rank * *count;
}

int dp_reduce_losses(v2x_model* m, const v2x_comm* c, bool want_loss, hipStream_t st) {
  if (!want_loss) return V2X_OK;
  return dp_call(m, c, c->all_reduce_sum, "all_reduce_sum", "the losses", m->loss_dev, n_loss_outputs(m), st);
}

int train_step_dp(v2x_model* m, const v2x_batch* b, const float* y, int y_on_device, int32_t n_global, const v2x_comm* c,
                  int form, float* loss_out, int loss_on_device, hipStream_t st) {
  const bool want_loss = loss_out != nullptr;
  // forms 1 and 2 run the phases on device batches only, as the Python trainer does (its _overlapped)
  const bool phased = form != V2X_DP_ALLREDUCE && b && b->on_device;
  if (form == V2X_DP_ALLREDUCE || (form == V2X_DP_BUCKETS && !phased)) {
    // forward + backward + slab sums (the replayed graph with use_graph), ONE all-reduce, Adam
    CHK(fwd_bwd(m, b, y, y_on_device, n_global, nullptr, 0, st, false));
    CHK(dp_call(m, c, c->all_reduce_sum, "all_reduce_sum", "the gradient", m->grads, m->P, st));
    CHK(dp_reduce_losses(m, c, want_loss, st));
    CHK(launch_reduce_adam(m, st, 0, true, nullptr));
    return emit_loss(m, loss_out, loss_on_device, st);
  }
  CHK(dp_ensure_stream(m));
  const int nb = n_phase_buckets(m);
  hipEvent_t* ev = m->dp_ev.data();
  const bool sharded = form == V2X_DP_SHARDED;
  if (!phased) CHK(fwd_bwd(m, b, y, y_on_device, n_global, nullptr, 0, st, false));
  // bucket k's collective starts on the model's stream once phase k is done, behind the collectives of the earlier buckets
  int rc = V2X_OK;
  for (int k = 0; k < nb && rc == V2X_OK; ++k) {
    if (phased) {
      rc = v2x_forward_backward_phase(m, b, y, y_on_device, n_global, k, nullptr, 0, st);
      if (rc) break;
    }
    int64_t off, e, cnt = 0;
    phase_bucket_range(m, k, &off, &e);
    char what[48];
    snprintf(what, sizeof(what), "bucket %d", k);
    if ((rc = dp_join(m, ev[k], st, m->dp_st))) break;
    if (sharded && dp_slice(c, e - off, &cnt) >= 0)
      rc = dp_call(m, c, c->reduce_scatter_sum, "reduce_scatter_sum", what, m->grads + off, e - off, m->dp_st);
    else
      rc = dp_call(m, c, c->all_reduce_sum, "all_reduce_sum", what, m->grads + off, e - off, m->dp_st);
  }
  // the caller's stream waits for every collective before Adam (and so does the next step's phase 0)
  CHK(dp_join(m, ev[nb], m->dp_st, st));
  CHK(rc);
  CHK(dp_reduce_losses(m, c, want_loss, st));
  if (!sharded) {
    CHK(launch_reduce_adam(m, st, 0, true, nullptr));
    return emit_loss(m, loss_out, loss_on_device, st);
  }
  // Adam on the owned slice of every bucket (t advances on the first call only), then the slice travels to the other ranks
  bool first = true;
  for (int k = 0; k < nb && rc == V2X_OK; ++k) {
    int64_t off, e, cnt = 0;
    phase_bucket_range(m, k, &off, &e);
    const int64_t s0 = dp_slice(c, e - off, &cnt);
    if (s0 < 0) {                                // not cut: every rank updates all of it
      rc = launch_reduce_adam(m, st, 0, true, nullptr, LossJob{0, 0, 0, 0.f, 0}, -1, false, off, e, first);
    } else {
      rc = launch_reduce_adam(m, st, 0, true, nullptr, LossJob{0, 0, 0, 0.f, 0}, -1, false, off + s0, off + s0 + cnt, first);
      char what[48];
      snprintf(what, sizeof(what), "bucket %d", k);
      // (on the caller's stream, behind this bucket's Adam: no stream hand-over per bucket)
      if (!rc) rc = dp_call(m, c, c->all_gather, "all_gather", what, m->params + off, e - off, st);
    }
    first = false;
  }
  CHK(rc);
  // Adam kept the fragment-major weight copy in step on the owned slices only: re-pack it once from the gathered parameters.
  // (Eagerly, here, rather than through pk_stale: a forward replayed from a hipGraph captured with a clean copy would not.)
  // The raw-pointer mode of v2x_param_ptr, and its re-pack before every forward, is not involved.
  if (m->pk_fwd) CHK(launch_pack(m, st));
  return emit_loss(m, loss_out, loss_on_device, st);
}

}  // namespace

extern "C" {

// the collectives of v2x_dqn_step_dp, between the slab sums and Adam
static int dp_dqn_collectives(v2x_model* m, const v2x_comm* comm, bool want_loss, hipStream_t st) {
  CHK(dp_call(m, comm, comm->all_reduce_sum, "all_reduce_sum", "the gradient", m->grads, m->P, st));
  return dp_reduce_losses(m, comm, want_loss, st);
}

int v2x_comm_rccl_unique_id(uint8_t out[128]) {
  v2x_model* nullm = nullptr;
  if (!out) FAIL(nullm, V2X_EINVAL, "comm_rccl_unique_id: null argument");
  std::string why;
  const Rccl* r = rccl(&why);
  if (!r) FAIL(nullm, V2X_EINVAL, "comm_rccl_unique_id: %s", why.c_str());
  NcclId id;
  const int rc = r->get_unique_id(&id);
  if (rc != 0) FAIL(nullm, V2X_ECOMM, "ncclGetUniqueId: %s", r->error_string(rc));
  memcpy(out, id.internal, sizeof(id.internal));
  return V2X_OK;
}

int v2x_comm_rccl_create(const uint8_t id[128], int32_t world, int32_t rank, int32_t device, v2x_comm* out) {
  v2x_model* nullm = nullptr;
  if (!id || !out) FAIL(nullm, V2X_EINVAL, "comm_rccl_create: null argument");
  if (world < 1 || rank < 0 || rank >= world) FAIL(nullm, V2X_EINVAL, "comm_rccl_create: rank %d of world %d", rank, world);
  std::string why;
  const Rccl* r = rccl(&why);
  if (!r) FAIL(nullm, V2X_EINVAL, "comm_rccl_create: %s", why.c_str());
  HIPCHK(nullm, hipSetDevice(device));
  NcclId nid;
  memcpy(nid.internal, id, sizeof(nid.internal));
  void* comm = nullptr;
  const int rc = r->comm_init_rank(&comm, world, nid, rank);
  if (rc != 0) FAIL(nullm, V2X_ECOMM, "ncclCommInitRank: %s", r->error_string(rc));
  memset(out, 0, sizeof(*out));
  out->world = world; out->rank = rank;
  out->ctx = new RcclCtx{r, comm, world, rank};
  out->all_reduce_sum = rccl_all_reduce;
  out->reduce_scatter_sum = rccl_reduce_scatter;
  out->all_gather = rccl_all_gather;
  return V2X_OK;
}

int v2x_comm_rccl_destroy(v2x_comm* c) {
  if (!c || !c->ctx) return V2X_OK;
  RcclCtx* ctx = static_cast<RcclCtx*>(c->ctx);
  const Rccl* r = ctx->r;
  const int rc = r->comm_destroy(ctx->comm);
  delete ctx;
  memset(c, 0, sizeof(*c));
  v2x_model* nullm = nullptr;
  if (rc != 0) FAIL(nullm, V2X_ECOMM, "ncclCommDestroy: %s", r->error_string(rc));
  return V2X_OK;
}

int v2x_train_step_dp(v2x_model* m, const v2x_batch* b, const float* y, int y_on_device, int32_t n_graphs_global,
                      const v2x_comm* comm, int form, float* loss_out, int loss_on_device, void* stream) {
  if (!m) FAIL(m, V2X_EINVAL, "null model");
  if (n_graphs_global <= 0)
    FAIL(m, V2X_EINVAL, "train_step_dp: n_graphs_global must be the global batch (> 0, got %d)", (int)n_graphs_global);
  CHK(dp_check_comm(m, comm, form, "train_step_dp"));
  HIPCHK(m, hipSetDevice(m->cfg.device));
  return train_step_dp(m, b, y, y_on_device, n_graphs_global, comm, form, loss_out, loss_on_device, (hipStream_t)stream);
}

int v2x_dqn_step_dp(v2x_model* online, v2x_model* target, const v2x_batch* s, const v2x_batch* s_next,
                    const int32_t* action, const double* reward, double gamma, int32_t n_graphs_global,
                    const v2x_comm* comm, float* y_out, float* loss_out, int loss_on_device, void* stream) {
  v2x_model* m = online;
  if (!m) FAIL(m, V2X_EINVAL, "dqn_step_dp: null argument");
  if (m->cfg.variable_graphs || (target && target->cfg.variable_graphs))
    FAIL(m, V2X_EINVAL, "dqn_step_dp: variable_graphs models are not supported (the ragged replay step runs on one GPU: v2x_dqn_step)");
  if (n_graphs_global <= 0)
    FAIL(m, V2X_EINVAL, "dqn_step_dp: n_graphs_global must be the global batch (> 0, got %d)", (int)n_graphs_global);
  CHK(dp_check_comm(m, comm, V2X_DP_ALLREDUCE, "dqn_step_dp"));
  return dqn_step(online, target, s, s_next, action, reward, gamma, n_graphs_global, y_out, loss_out, loss_on_device, stream,
                  comm);
}

}  // extern "C"
