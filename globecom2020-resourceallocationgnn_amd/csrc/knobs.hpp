// Every environment switch of libv2xgnn.so: one struct, one function that reads the environment.  Nothing else in the
// library calls getenv.  v2x_create stores read_knobs() in the model, so a switch is fixed for the life of a model (and a
// cached hipGraph can never be stale against one); the entry points that take no model use process_knobs(), read once.
// Defaults are the measured best (DESIGN.md section 9 lists the same names).
#pragma once
#include <cstdlib>

namespace v2x {

struct Knobs {
  // ---- which kernels run
  int fused = 1;                  // V2X_FUSED=0: layer-by-layer kernels instead of the fused graph layers
  int fused_compl = 1;            // V2X_FUSED_COMPL=0: dense graphs aggregate edge by edge, not through the complement
  int fused_split = -1;           // V2X_FUSED_SPLIT: -1 auto, 0 / 1 whole tiles, K forced (kernels_fused_split.hpp)
  int fused_split_fwd = 1;        // V2X_FUSED_SPLIT_FWD=0: forward on whole tiles (debugging)
  int fused_split_bwd = 1;        // V2X_FUSED_SPLIT_BWD=0: backward on whole tiles (debugging)
  int fused_ts = 0;               // V2X_FUSED_TS=1: phase time stamps of the fused kernels (measurement)
  int small_predict = 1;          // V2X_SMALL_PREDICT=0: no one-launch few-graph forward (kernels_small.hpp)
  int small_pinned = 1;           // V2X_SMALL_PINNED=0: ... and no pinned window for its host-resident batches
  int ragged_fused = 1;           // V2X_RAGGED_FUSED=0: ragged graphs layer by layer (forward and backward)
  int ragged_fused_bwd = 1;       // V2X_RAGGED_FUSED_BWD=0: ... the backward only
  int ragged_packed = 1;          // V2X_RAGGED_PACKED=0: the row-interval plan of k_adj_masks instead of k_ragged_plan's tiles
  int ragged_plan_fold = 1;       // V2X_RAGGED_PLAN_FOLD=0: the packed plan always as a launch of its own
  int ragged_small = 0;           // V2X_RAGGED_SMALL=1: the small-tile ragged kernels (kernels_ragged_small.hpp)
  int frag_handoff = 1;           // V2X_FRAG_HANDOFF=0: row-major h_L / a_L between the fused kernels and k_mlp_train_wg
  int frag_with_dense0_role = 1;  // V2X_FRAG_WITH_DENSE0_ROLE=0: ... row-major where Dense-0's gradient is a role of k_wgrad
  int mlp_wg0 = -1;               // V2X_MLP_WG0: Dense-0's weight gradient as roles of k_wgrad: -1 auto, 0 whenever possible, 1 never
  int mlp_wg0_tiles = 12;         // V2X_MLP_WG0_TILES: auto = up to so many tiles per MLP workgroup
  int dqn_fused_targets = 1;      // V2X_DQN_FUSED_TARGETS=0: forward, k_dqn_targets and the training launch on y
  int wide_merge = 1;             // V2X_WIDE_MERGE=0: one wide weight-gradient launch per layer
  int wide_fold = 1;              // V2X_WIDE_FOLD=0: the [x | e] segment of a wide layer as a K tile of its own
  int wide_adam = 1;              // V2X_WIDE_ADAM=0: Adam never in the wide weight-gradient epilogues
  int wide_tail = 1;              // V2X_WIDE_TAIL: 0 whole 128-row tiles only, 2 half tiles for a launch below one round
  int wide_slots = 0;             // V2X_WIDE_SLOTS: resident slots the half-tile rule plans for (0: five per CU; tests)
  // ---- launch sizes
  int wg_embed_merge = 1;        // V2X_WG_EMBED_MERGE=0: the embed layer's gradient as a role of its own
  int wg_rounds = 0;              // V2X_WG_ROUNDS: > 0 work-proportional chunk counts, so many rounds of the chip
  int wg_chunk = 0;               // V2X_WG_CHUNK: rows per weight-gradient workgroup, every role (0: per-role defaults)
  int wg_chunk_gnn = 0;           // V2X_WG_CHUNK_GNN: ... of the graph layers' roles (0: 896, wide 1024)
  int wg_chunk_dense = 1024;      // V2X_WG_CHUNK_DENSE: ... of the Dense roles
  int wg_chunk_embed = 0;         // V2X_WG_CHUNK_EMBED: ... of the embed role (0: as the graph layers)
  int wg_chunk_d123 = 512;        // V2X_WG_CHUNK_D123: slabs are pre-sized for this chunking too
  int wg_chunk_merged = 0;        // V2X_WG_CHUNK_MERGED: ... of the graph layers' roles that carry the embed gradient (0: one per CU)
  int wg_merged_min_rows = 64;    // V2X_WG_MERGED_MIN_ROWS: fewest rows per workgroup for that one-per-CU chunking
  int wg_ts_role = 0;             // V2X_WG_TS_ROLE: the role of a weight-gradient launch that writes phase stamps
  int gemm_wgs_per_cu = 2;        // V2X_GEMM_WGS_PER_CU: persistent workgroups per CU of the layer-wise GEMMs
  int mlp_wgs_per_cu = 2;         // V2X_MLP_WGS_PER_CU: ... of k_mlp_fwd / k_mlp_bwd
  int agg_dense_min_nodes = 32;   // V2X_AGG_DENSE_MIN_NODES: fewest nodes for the MFMA aggregation against bit masks
  int agg_workers_per_graph = 8;  // V2X_AGG_WORKERS_PER_GRAPH: fewest workers per graph in k_agg
  bool agg_no_small = false;      // V2X_AGG_NO_SMALL (set): never k_agg_small
  // ---- host side
  bool trusted_batches = false;   // V2X_TRUSTED_BATCHES (set): skip the O(E) part of the host batch check
  int pack_threads = 0;           // V2X_PACK_THREADS: threads of v2x_pack_feed's scan (0: by size, at most 8)
  bool debug_occ = false;         // V2X_DEBUG_OCC (set): print the wide kernels' occupancy
};

inline Knobs read_knobs() {
  Knobs k;
  auto num = [](const char* name, int& v) { if (const char* s = getenv(name)) v = atoi(s); };
  auto set = [](const char* name, bool& v) { v = getenv(name) != nullptr; };
  num("V2X_FUSED", k.fused);
  num("V2X_FUSED_COMPL", k.fused_compl);
  num("V2X_FUSED_SPLIT", k.fused_split);
  num("V2X_FUSED_SPLIT_FWD", k.fused_split_fwd);
  num("V2X_FUSED_SPLIT_BWD", k.fused_split_bwd);
  num("V2X_FUSED_TS", k.fused_ts);
  num("V2X_SMALL_PREDICT", k.small_predict);
  num("V2X_SMALL_PINNED", k.small_pinned);
  num("V2X_RAGGED_FUSED", k.ragged_fused);
  num("V2X_RAGGED_FUSED_BWD", k.ragged_fused_bwd);
  num("V2X_RAGGED_PACKED", k.ragged_packed);
  num("V2X_RAGGED_PLAN_FOLD", k.ragged_plan_fold);
  num("V2X_RAGGED_SMALL", k.ragged_small);
  num("V2X_FRAG_HANDOFF", k.frag_handoff);
  num("V2X_FRAG_WITH_DENSE0_ROLE", k.frag_with_dense0_role);
  num("V2X_MLP_WG0", k.mlp_wg0);
  num("V2X_MLP_WG0_TILES", k.mlp_wg0_tiles);
  num("V2X_DQN_FUSED_TARGETS", k.dqn_fused_targets);
  num("V2X_WIDE_MERGE", k.wide_merge);
  num("V2X_WIDE_FOLD", k.wide_fold);
  num("V2X_WIDE_ADAM", k.wide_adam);
  num("V2X_WIDE_TAIL", k.wide_tail);
  num("V2X_WIDE_SLOTS", k.wide_slots);
  num("V2X_WG_EMBED_MERGE", k.wg_embed_merge);
  num("V2X_WG_ROUNDS", k.wg_rounds);
  num("V2X_WG_CHUNK", k.wg_chunk);
  num("V2X_WG_CHUNK_GNN", k.wg_chunk_gnn);
  num("V2X_WG_CHUNK_DENSE", k.wg_chunk_dense);
  num("V2X_WG_CHUNK_EMBED", k.wg_chunk_embed);
  num("V2X_WG_CHUNK_D123", k.wg_chunk_d123);
  num("V2X_WG_CHUNK_MERGED", k.wg_chunk_merged);
  num("V2X_WG_MERGED_MIN_ROWS", k.wg_merged_min_rows);
  num("V2X_WG_TS_ROLE", k.wg_ts_role);
  num("V2X_GEMM_WGS_PER_CU", k.gemm_wgs_per_cu);
  num("V2X_MLP_WGS_PER_CU", k.mlp_wgs_per_cu);
  num("V2X_AGG_DENSE_MIN_NODES", k.agg_dense_min_nodes);
  num("V2X_AGG_WORKERS_PER_GRAPH", k.agg_workers_per_graph);
  set("V2X_AGG_NO_SMALL", k.agg_no_small);
  set("V2X_TRUSTED_BATCHES", k.trusted_batches);
  num("V2X_PACK_THREADS", k.pack_threads);
  set("V2X_DEBUG_OCC", k.debug_occ);
  return k;
}

// the copy of the entry points that take no model (v2x_agg_fwd / bwd, v2x_pack_feed): read on first use
inline const Knobs& process_knobs() {
  static const Knobs k = read_knobs();
  return k;
}

}  // namespace v2x
