"""ctypes binding of libv2xgnn.so (the C ABI in include/v2xgnn.h).

The library is built in-tree (`csrc/Makefile`, or `__graft_entry__.build()`); if it is
missing this module raises -- there is deliberately no Python/CPU fallback for the hot path.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

V2X_OK = 0
V2X_EINVAL = -1
V2X_ECOMM = -5          # a collective of a v2x_comm table returned non-zero
V2X_EBUDGET = -6        # v2x_opt_search_bound spent its node budget (the result is a lower bound)

# forms of v2x_train_step_dp
V2X_DP_ALLREDUCE, V2X_DP_BUCKETS, V2X_DP_SHARDED = 0, 1, 2


class V2XError(RuntimeError):
    pass


class V2XInvalidArgument(V2XError, ValueError):
    """V2X_EINVAL: a library error (V2XError) and the exception class Keras raises on bad inputs (ValueError)."""


class V2XCommError(V2XError):
    """V2X_ECOMM: a collective of the v2x_comm table failed (the text names it and its bucket)."""


class Config(C.Structure):
    _fields_ = [("n_nodes", C.c_int32), ("n_channels", C.c_int32), ("feat_dim", C.c_int32),
                ("n_mp_layers", C.c_int32), ("share_weights", C.c_int32), ("variable_graphs", C.c_int32),
                ("device", C.c_int32), ("use_graph", C.c_int32),
                ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float)]


class Batch(C.Structure):
    _fields_ = [("n_graphs", C.c_int32), ("n_rows", C.c_int32), ("n_edges", C.c_int32),
                ("max_nodes", C.c_int32), ("max_edges", C.c_int32), ("on_device", C.c_int32),
                ("xe", C.c_void_p), ("nbr_init", C.c_void_p), ("graph_off", C.c_void_p),
                ("row_ptr", C.c_void_p), ("col_idx", C.c_void_p)]


class ForwardClosure(C.Structure):
    """v2x_forward_closure of include/v2xgnn.h"""
    _fields_ = [("m", C.c_void_p), ("b", Batch), ("q_out", C.c_void_p), ("q_on_device", C.c_int32), ("pad_", C.c_int32),
                ("stream", C.c_void_p)]


class Feed(C.Structure):
    _fields_ = [("n_graphs", C.c_int32), ("n_nodes", C.c_int32), ("feat_dim", C.c_int32), ("node_in", C.c_int32),
                ("edge_in", C.c_int32), ("node", C.POINTER(C.c_void_p)), ("edge", C.POINTER(C.c_void_p)),
                ("nbr", C.POINTER(C.c_void_p)), ("is_f64", C.POINTER(C.c_uint8)), ("adjacency", C.c_void_p)]


class OptProblem(C.Structure):
    """v2x_opt_problem of include/v2xgnn.h"""
    _fields_ = [("E", C.c_int32), ("n", C.c_int32), ("rb", C.c_int32), ("pad_", C.c_int32),
                ("v2v_ff", C.c_void_p), ("v2i_ff", C.c_void_p), ("v2i_abs", C.c_void_p), ("dest", C.c_void_p)] + \
        [(k, C.c_double) for k in ("p_v2v", "p_v2i", "veh_gain", "bs_gain", "bs_nf", "veh_nf", "sig2", "w_v2v", "w_v2i")]


class SimStep(C.Structure):
    """v2x_sim_step of include/v2xgnn.h"""
    _fields_ = [("problem", OptProblem)] + \
        [(k, C.c_void_p) for k in ("keys", "mtpos", "xy", "dirs", "vel", "lanes", "u")] + \
        [("n_lanes", C.c_int32), ("n_u", C.c_int32), ("timestep", C.c_double), ("width", C.c_double), ("height", C.c_double)] + \
        [(k, C.c_void_p) for k in ("v2i_shadow", "v2v_shadow", "v2v_abs", "v2i_abs", "v2v_ff", "v2i_ff")] + \
        [("power", C.c_double)] + \
        [(k, C.c_void_p) for k in ("interf_db", "state", "xe", "mask", "col", "regular", "v2v_rate", "v2i_rate", "interference",
                                   "v2i_interf", "v2v_interf", "actions")]


class SimReset(C.Structure):
    """v2x_sim_reset_args of include/v2xgnn.h"""
    _fields_ = [("step", SimStep), ("vel", C.c_void_p), ("dest", C.c_void_p), ("status", C.c_void_p)]


class Rollout(C.Structure):
    """v2x_rollout of include/v2xgnn.h"""
    _fields_ = [("model", C.c_void_p), ("batch", Batch)] + \
        [(k, C.c_void_p) for k in ("q", "explore", "random_actions", "actions")] + \
        [("step", SimStep), ("w_v2v", C.c_double), ("w_v2i", C.c_double)] + \
        [(k, C.c_void_p) for k in ("rep_xe", "rep_xe_next", "rep_col", "rep_mask", "rep_action", "rep_reward")] + \
        [("head", C.c_int64), ("capacity", C.c_int64), ("result_reward", C.c_void_p), ("result_regular", C.c_void_p)]


class RolloutTraj(C.Structure):
    """v2x_rollout_traj of include/v2xgnn.h"""
    _fields_ = [("r", Rollout), ("T", C.c_int32), ("pad_", C.c_int32)] + \
        [(k, C.c_void_p) for k in ("traj_xe", "traj_col", "traj_mask", "traj_regular", "traj_v2v_ff", "traj_v2i_ff", "traj_v2i_abs")]


class RolloutRecv(C.Structure):
    """v2x_rollout_recv of include/v2xgnn.h"""
    _fields_ = [("model", C.c_void_p), ("batch", Batch)] + \
        [(k, C.c_void_p) for k in ("q", "explore", "random_actions", "actions")] + \
        [("step", SimStep), ("recv", C.c_void_p), ("flags", C.c_void_p), ("w_v2v", C.c_double), ("w_v2i", C.c_double),
         ("T", C.c_int32), ("pad_", C.c_int32)] + \
        [(k, C.c_void_p) for k in ("traj_xe", "traj_recv", "traj_flags", "traj_v2v_ff", "traj_v2i_ff", "traj_v2i_abs", "row_ptr",
                                   "col_idx", "edge_base", "rep_xe", "rep_xe_next", "rep_recv", "rep_action", "rep_reward")] + \
        [("head", C.c_int64), ("capacity", C.c_int64), ("result_reward", C.c_void_p), ("result_flags", C.c_void_p)]


class EvalRecv(C.Structure):
    """v2x_eval_recv of include/v2xgnn.h"""
    _fields_ = [("model", C.c_void_p), ("batch", Batch)] + \
        [(k, C.c_void_p) for k in ("q", "explore", "random_actions", "baseline_actions", "actions")] + \
        [("step", SimStep), ("recv", C.c_void_p), ("flags", C.c_void_p), ("w_v2v", C.c_double), ("w_v2i", C.c_double),
         ("T", C.c_int32), ("pad_", C.c_int32)] + \
        [(k, C.c_void_p) for k in ("traj_xe", "traj_recv", "traj_flags", "traj_v2v_ff", "traj_v2i_ff", "traj_v2i_abs", "row_ptr",
                                   "col_idx", "edge_base", "result_actions", "result_v2v_rate", "result_v2i_rate",
                                   "result_interference", "result_reward", "result_flags")]


class RolloutMixed(C.Structure):
    """v2x_rollout_mixed of include/v2xgnn.h"""
    _fields_ = [("n_pools", C.c_int32), ("T", C.c_int32), ("pools", C.POINTER(RolloutTraj)), ("model", C.c_void_p)] + \
        [(k, C.c_void_p) for k in ("xe", "graph_off", "row_ptr", "col_idx", "q")]


TRAJ_WORKSPACES = ("traj_xe", "traj_col", "traj_mask", "traj_regular", "traj_v2v_ff", "traj_v2i_ff", "traj_v2i_abs")
EVAL_RESULTS = ("result_actions", "result_v2v_rate", "result_v2i_rate", "result_interference", "result_reward", "result_regular")


class Eval(C.Structure):
    """v2x_eval of include/v2xgnn.h"""
    _fields_ = [("model", C.c_void_p), ("batch", Batch)] + \
        [(k, C.c_void_p) for k in ("q", "explore", "random_actions", "baseline_actions", "actions")] + \
        [("step", SimStep), ("w_v2v", C.c_double), ("w_v2i", C.c_double), ("T", C.c_int32), ("pad_", C.c_int32)] + \
        [(k, C.c_void_p) for k in TRAJ_WORKSPACES + EVAL_RESULTS]


class EvalMixed(C.Structure):
    """v2x_eval_mixed of include/v2xgnn.h"""
    _fields_ = [("n_pools", C.c_int32), ("T", C.c_int32), ("pools", C.POINTER(Eval)), ("model", C.c_void_p)] + \
        [(k, C.c_void_p) for k in ("xe", "graph_off", "row_ptr", "col_idx", "q")]


class TrajWs(C.Structure):
    """v2x_traj_ws of include/v2xgnn.h"""
    _fields_ = [("wide_ws", C.c_void_p), ("wide_ws_bytes", C.c_int64), ("split_ws", C.c_void_p), ("split_ws_bytes", C.c_int64)]


class EvalSweep(C.Structure):
    """v2x_eval_sweep of include/v2xgnn.h"""
    _fields_ = [("base", EvalMixed), ("K", C.c_int32), ("pad_", C.c_int32), ("models", C.POINTER(C.c_void_p)), ("q", C.c_void_p)]


SWEEP_MAX_MODELS = 64


class EvalSweepRecv(C.Structure):
    """struct v2x_eval_sweep_recv of include/v2xgnn.h"""
    _fields_ = [("base", EvalRecv), ("K", C.c_int32), ("pad_", C.c_int32), ("models", C.POINTER(C.c_void_p)), ("q", C.c_void_p)]


class MtJump(C.Structure):
    """v2x_mt_jump of include/v2xgnn.h"""
    _fields_ = [("first", C.c_int64), ("stride", C.c_int64), ("count", C.c_int32), ("pad_", C.c_int32), ("polys", C.c_void_p),
                ("scratch", C.c_void_p), ("scratch_bytes", C.c_int64)]


class ReplayPool(C.Structure):
    """v2x_replay_pool of include/v2xgnn.h"""
    _fields_ = [("n_nodes", C.c_int32), ("count", C.c_int32)] + \
        [(k, C.c_void_p) for k in ("xe", "xe_next", "col", "action", "reward", "idx")]


class MixedBatch(C.Structure):
    """v2x_mixed_batch of include/v2xgnn.h"""
    _fields_ = [(k, C.c_void_p) for k in ("xe", "xe_next", "action", "reward", "graph_off", "row_ptr", "col_idx")]


MIXED_MAX_POOLS = 8


class ReplayRecv(C.Structure):
    """v2x_replay_recv of include/v2xgnn.h"""
    _fields_ = [("n_nodes", C.c_int32), ("count", C.c_int32)] + \
        [(k, C.c_void_p) for k in ("xe", "xe_next", "recv", "action", "reward", "idx", "edge_base")]


RECV_MAX_LINKS = 128

# int (*)(float* buf, int64_t n, void* stream, void* ctx): an entry of v2x_comm
COLLECTIVE = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p)


class Comm(C.Structure):
    """v2x_comm of include/v2xgnn.h"""
    _fields_ = [("world", C.c_int32), ("rank", C.c_int32), ("ctx", C.c_void_p), ("all_reduce_sum", COLLECTIVE),
                ("reduce_scatter_sum", COLLECTIVE), ("all_gather", COLLECTIVE)]


# every symbol include/v2xgnn.h declares: (name, restype, argtypes)
_P, _I, _L, _F = C.c_void_p, C.c_int32, C.c_int64, C.c_float
SYMBOLS = [
    ("v2x_create", C.c_int, [C.POINTER(Config), C.POINTER(_P)]),
    ("v2x_destroy", None, [_P]),
    ("v2x_last_error", C.c_char_p, [_P]),
    ("v2x_version", C.c_char_p, []),
    ("v2x_param_count", _L, [_P]),
    ("v2x_get_weights", C.c_int, [_P, _P, _P]),
    ("v2x_set_weights", C.c_int, [_P, _P, _P]),
    ("v2x_copy_weights", C.c_int, [_P, _P, _P]),
    ("v2x_get_optimizer_state", C.c_int, [_P, _P, _P, C.POINTER(_L), _P]),
    ("v2x_set_optimizer_state", C.c_int, [_P, _P, _P, _L, _P]),
    ("v2x_param_ptr", _P, [_P]),
    ("v2x_grad_ptr", _P, [_P]),
    ("v2x_forward", C.c_int, [_P, C.POINTER(Batch), _P, C.c_int, _P]),
    ("v2x_forward_call", C.c_int, [_P]),
    ("v2x_train_step", C.c_int, [_P, C.POINTER(Batch), _P, C.c_int, _I, _P, C.c_int, _P]),
    ("v2x_forward_backward", C.c_int, [_P, C.POINTER(Batch), _P, C.c_int, _I, _P, C.c_int, _P]),
    ("v2x_apply_gradients", C.c_int, [_P, _P]),
    ("v2x_forward_backward_phase", C.c_int, [_P, C.POINTER(Batch), _P, C.c_int, _I, C.c_int, _P, C.c_int, _P]),
    ("v2x_grad_bucket", _L, [_P, C.c_int, C.POINTER(_L)]),
    ("v2x_grad_bucket_count", C.c_int, [_P]),
    ("v2x_apply_gradients_range", C.c_int, [_P, _L, _L, C.c_int, _P]),
    ("v2x_agg_fwd", C.c_int, [C.POINTER(Batch), _I, _I, _P, _P, _P]),
    ("v2x_agg_bwd", C.c_int, [C.POINTER(Batch), _I, _I, _P, _P, _P]),
    ("v2x_node_update_fwd", C.c_int, [_P, _I, _I, _P, _P, _P, _P, _P]),
    ("v2x_node_update_bwd", C.c_int, [_P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P]),
    ("v2x_mlp_fwd", C.c_int, [_P, _I, _P, _P, _P, _P, _P]),
    ("v2x_mlp_huber_bwd", C.c_int, [_P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    ("v2x_adam_step", C.c_int, [_P, _P, _P, _P, _L, _L, _F, _F, _F, _F, _P]),
    ("v2x_device_addressable", C.c_int, [_P]),
    ("v2x_gather_rows", C.c_int, [_P, _P, _P, _L, _L, _P]),
    ("v2x_gather_rows_multi", C.c_int, [_I, _P, _P, _P, _P, _L, _P]),
    ("v2x_q_stats", C.c_int, [_P, _I, _I, _I, _P, _P]),
    ("v2x_dqn_targets", C.c_int, [_P, _P, _P, _P, C.c_double, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    ("v2x_dqn_targets_ragged", C.c_int, [_P, _P, _P, _P, C.c_double, _P, _I, _I, _I, _P, _P]),
    ("v2x_replay_gather_mixed", C.c_int, [_I, C.POINTER(ReplayPool), C.POINTER(MixedBatch), _P]),
    ("v2x_replay_gather_recv", C.c_int, [C.POINTER(ReplayRecv), C.POINTER(MixedBatch), _P]),
    ("v2x_dqn_step", C.c_int, [_P, _P, _P, _P, _P, _P, C.c_double, C.c_int32, _P, _P, C.c_int, _P]),
    ("v2x_comm_rccl_unique_id", C.c_int, [_P]),
    ("v2x_comm_rccl_create", C.c_int, [_P, _I, _I, _I, C.POINTER(Comm)]),
    ("v2x_comm_rccl_destroy", C.c_int, [C.POINTER(Comm)]),
    ("v2x_train_step_dp", C.c_int, [_P, C.POINTER(Batch), _P, C.c_int, _I, C.POINTER(Comm), C.c_int, _P, C.c_int, _P]),
    ("v2x_dqn_step_dp", C.c_int, [_P, _P, C.POINTER(Batch), C.POINTER(Batch), _P, _P, C.c_double, C.c_int32, C.POINTER(Comm),
                                  _P, _P, C.c_int, _P]),
    ("v2x_pack_feed", C.c_int, [C.POINTER(Feed), C.c_int, _P, _P, _P, _P, _P]),
    ("v2x_validate_batch", C.c_int, [_P, C.POINTER(Batch), _I, _P]),
    ("v2x_check_errors", C.c_int, [_P, _P]),
    ("v2x_reset_exchange", C.c_int, [_P]),
    ("v2x_debug_exchange_counters", _P, [_P]),
    ("v2x_debug_split_counters", _P, [_P, C.POINTER(C.c_int32)]),
    ("v2x_debug_phase_stamps", C.c_int, [_P, _P, C.c_int]),
    ("v2x_debug_ragged_plan", C.c_int, [_P, _P, C.c_int]),
    ("v2x_debug_layer_slabs", C.c_int, [_P, _P, C.c_int]),
    ("v2x_wide_tiling_plan", C.c_int, [_I, _I, _I, _I, _I, C.POINTER(_I)]),
    ("v2x_debug_wide_tiling", C.c_int, [_P, _P, C.c_int]),
    ("v2x_profile_enable", C.c_int, [_P, C.c_int]),
    ("v2x_path_info", C.c_int, [_P, _P, C.c_char_p, C.c_int]),
    ("v2x_profile_read", C.c_int, [_P, C.c_char_p, C.c_int, C.POINTER(C.c_double), C.POINTER(_L), C.c_int]),
    ("v2x_opt_workspace_bytes", _L, [C.POINTER(OptProblem)]),
    ("v2x_opt_search", C.c_int, [C.POINTER(OptProblem), _P, _P, _P, _P]),
    ("v2x_opt_rewards", C.c_int, [C.POINTER(OptProblem), _P, _L, _L, _P, _P]),
    ("v2x_opt_landscape_workspace_bytes", _L, [C.POINTER(OptProblem), C.c_int32]),
    ("v2x_opt_landscape", C.c_int, [C.POINTER(OptProblem), _P, _P, C.c_int32, _P, _P, _P]),
    ("v2x_opt_bound_workspace_bytes", _L, [C.POINTER(OptProblem), _L]),
    ("v2x_opt_search_bound", C.c_int, [C.POINTER(OptProblem), _P, _L, _P, _P, C.POINTER(_L), _P]),
    ("v2x_opt_search_bound_seeded", C.c_int, [C.POINTER(OptProblem), _P, _L, _P, _P, _P, C.POINTER(_L), _P]),
    ("v2x_opt_count_bound_workspace_bytes", _L, [C.POINTER(OptProblem), C.c_int32, _L]),
    ("v2x_opt_count_bound", C.c_int, [C.POINTER(OptProblem), _P, _P, C.c_int32, _L, _P, _P, _P, _P, C.POINTER(_L), _P]),
    ("v2x_opt_count_open_leaves", C.c_int, [C.POINTER(C.c_uint64), C.c_int32, C.c_int32, C.POINTER(C.c_uint64),
                                            C.POINTER(C.c_uint64)]),
    ("v2x_opt_local_workspace_bytes", _L, [C.POINTER(OptProblem), C.c_int32]),
    ("v2x_opt_search_local", C.c_int, [C.POINTER(OptProblem), _P, C.c_int32, C.c_uint64, C.c_int32, _P, _P, _P, _P, _P, _P]),
    ("v2x_opt_rewards_actions", C.c_int, [C.POINTER(OptProblem), _P, _P, _L, _P, _P]),
    ("v2x_sim_channels", C.c_int, [_I, _I, _I, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    ("v2x_sim_observe", C.c_int, [_I, _I, _I, _P, _P, _P] + [C.c_double] * 5 + [_P] * 7),
    ("v2x_sim_rates", C.c_int, [C.POINTER(OptProblem), _P, _P, _P, _P, _P, _P, _P]),
    ("v2x_sim_stream", C.c_int, [_I, _I, _P, _P, _P, _P, _P, C.c_double, _I, _P, C.c_double, C.c_double, _P, _I, _P]),
    ("v2x_sim_advance", C.c_int, [C.POINTER(SimStep), _P]),
    ("v2x_sim_reset", C.c_int, [C.POINTER(SimReset), _P]),
    ("v2x_sim_reset_draw", C.c_int, [C.POINTER(SimReset), _P]),
    ("v2x_rollout_pick", C.c_int, [_I, _I, _I] + [_P] * 11 + [_L, _L, _P, _P]),
    ("v2x_rollout_store", C.c_int, [_I, _I, _I, _P, _P, C.c_double, C.c_double] + [_P] * 6 + [_L, _L, _P, _P, _P]),
    ("v2x_rollout_step", C.c_int, [C.POINTER(Rollout), _P]),
    ("v2x_rollout_steps_workspace_bytes", _L, [_I, _I, _I, _I]),
    ("v2x_rollout_steps", C.c_int, [C.POINTER(RolloutTraj), _P]),
    ("v2x_rollout_steps_mixed", C.c_int, [C.POINTER(RolloutMixed), _P]),
    ("v2x_eval_steps_result_bytes", _L, [_I, _I, _I, _I, _I]),
    ("v2x_eval_steps", C.c_int, [C.POINTER(Eval), _P]),
    ("v2x_eval_steps_mixed", C.c_int, [C.POINTER(EvalMixed), _P]),
    ("v2x_traj_wide_workspace_bytes", _L, [_I, _I, _I, _I]),
    ("v2x_rollout_steps_wide", C.c_int, [C.POINTER(RolloutTraj), _P, _L, _P]),
    ("v2x_eval_steps_wide", C.c_int, [C.POINTER(Eval), _P, _L, _P]),
    ("v2x_traj_split_workspace_bytes", _L, [_I, _I, _I, _I, _I]),
    ("v2x_rollout_steps_split", C.c_int, [C.POINTER(RolloutTraj), _P, _L, _P, _L, _P]),
    ("v2x_eval_steps_split", C.c_int, [C.POINTER(Eval), _P, _L, _P, _L, _P]),
    ("v2x_rollout_steps_mixed_wide", C.c_int, [C.POINTER(RolloutMixed), C.POINTER(TrajWs), _P]),
    ("v2x_eval_steps_mixed_wide", C.c_int, [C.POINTER(EvalMixed), C.POINTER(TrajWs), _P]),
    ("v2x_eval_sweep_result_bytes", _L, [_I, _I, _I, _I, _I]),
    ("v2x_eval_sweep_mixed", C.c_int, [C.POINTER(EvalSweep), C.POINTER(TrajWs), _P]),
    ("v2x_sim_observe_recv", C.c_int, [_I, _I, _I, _P, _P, _P] + [C.c_double] * 5 + [_P] * 6),
    ("v2x_csr_from_recv", C.c_int, [_I, _I, _I, _P, _P, _P, _P, _P]),
    ("v2x_rollout_recv_workspace_bytes", _L, [_I, _I, _I, _I]),
    ("v2x_rollout_steps_recv", C.c_int, [C.POINTER(RolloutRecv), _P, _L, _P]),
    ("v2x_rollout_recv_split_workspace_bytes", _L, [_I, _I, _I, _I, _I]),
    ("v2x_rollout_steps_recv_split", C.c_int, [C.POINTER(RolloutRecv), _P, _L, _P, _L, _P]),
    ("v2x_eval_recv_result_bytes", _L, [_I, _I, _I, _I, _I]),
    ("v2x_eval_steps_recv", C.c_int, [C.POINTER(EvalRecv), _P, _L, _P]),
    ("v2x_eval_steps_recv_split", C.c_int, [C.POINTER(EvalRecv), _P, _L, _P, _L, _P]),
    ("v2x_eval_sweep_recv_result_bytes", _L, [_I, _I, _I, _I, _I]),
    ("v2x_eval_sweep_recv", C.c_int, [C.POINTER(EvalSweepRecv), _P, _L, _P]),
    ("v2x_eval_sweep_recv_split", C.c_int, [C.POINTER(EvalSweepRecv), _P, _L, _P, _L, _P]),
    ("v2x_mt_jump_polys", C.c_int, [_L, _L, _I, _P]),
    ("v2x_mt_jump_scratch_bytes", _L, [_I, _I]),
    ("v2x_rollout_steps_recv_jump", C.c_int, [C.POINTER(RolloutRecv), _P, _L, _P, _L, C.POINTER(MtJump), _P]),
    ("v2x_eval_steps_recv_jump", C.c_int, [C.POINTER(EvalRecv), _P, _L, _P, _L, C.POINTER(MtJump), _P]),
    ("v2x_eval_sweep_recv_jump", C.c_int, [C.POINTER(EvalSweepRecv), _P, _L, _P, _L, C.POINTER(MtJump), _P]),
]


def library_path():
    return os.environ.get("V2XGNN_LIB", os.path.join(_HERE, "libv2xgnn.so"))


def load_library():
    """dlopen libv2xgnn.so and bind every exported symbol.  Raises V2XError when the HIP
    extension has not been built (run `python -c "import __graft_entry__ as g; g.build()"`)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise V2XError("HIP extension %s is missing: build it with `make -C %s` (no CPU fallback exists)"
                       % (path, os.path.join(_HERE, "csrc")))
    # PyTorch-ROCm ships its own HIP runtime (torch/lib/libamdhip64.so).  Whichever copy of that soname is mapped
    # first serves the whole process, and torch does not find its GPUs through /opt/rocm's copy: load torch's first.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    try:
        lib = C.CDLL(path)
    except OSError as exc:
        raise V2XError("cannot load %s: %s" % (path, exc))
    for name, restype, argtypes in SYMBOLS:
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise V2XError("%s does not export %s (stale build?)" % (path, name))
        fn.restype = restype
        fn.argtypes = argtypes
    _LIB = lib
    return lib


def check(lib, rc, handle=None):
    if rc != V2X_OK:
        msg = lib.v2x_last_error(handle)
        text = msg.decode() if msg else "unknown error"
        if rc == V2X_EINVAL:
            raise V2XInvalidArgument(text)
        if rc == V2X_ECOMM:
            raise V2XCommError("v2xgnn error %d: %s" % (rc, text))
        raise V2XError("v2xgnn error %d: %s" % (rc, text))
