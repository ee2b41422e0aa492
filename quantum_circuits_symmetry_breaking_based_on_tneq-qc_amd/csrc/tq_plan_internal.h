// What the plan sources share behind tq_plan.h (the interface tq_capi.cpp sees):
//   tq_plan.cpp            the plan compiler's lowering (class Compiler, plan_compile and the
//                          compile-time plan functions)
//   tq_sweep2_layout.cpp   the sweep-chain layout planner (chain_shape, s2_layout, s2_blob, ...) and
//                          the inspectors of a plan's sweep2 descriptors; the layout functions see
//                          neither the Plan nor the Compiler
//   tq_plan_finish.cpp     plan_finish: arena / lane layout, assign_amax, tables, build_schedule,
//                          the describe text; plan_planes_layout, plan_tables_digest
//   tq_plan_compile.h      the compile-time types those three share (Live, Chain, ChainShape, ...)
//   tq_plan_exec.cpp       Exec: one plan's (or a lockstep group's) launch sequence on a stream
//   tq_plan_run.cpp        materialize / release, the hipGraph cache, plan_run, plan_run_group
#pragma once
#include "tq_env.h"
#include "tq_plan.h"

#include <climits>

namespace tq {

// ---- the compiler's knobs: each read once per process --------------------
// cooperative chain launches (TQ_S2_COOP=1, default 0; tq_plan_set "sweep_coop") for levels of
// ops of at most TQ_S2_COOPCH chunks (default 16).  Measured r04 (C2, complex64, 26 levels in
// one launch of 4 workgroups): 0.379 ms against 0.363 one launch per level -- the launch gaps
// it removes (~1.7 us each, 46 us in all) come back as longer ops (write-through stores
// drained before the arrival, the poll, L2-missing loads: +1.1 us per op), so it is off
inline bool s2_coop_enabled() { static const bool v = env_opt_in("TQ_S2_COOP"); return v; }
inline int s2_coop_max_chunks() { static const int v = env_int("TQ_S2_COOPCH", 16, INT_MIN, 16); return v; }
// chain launches take small ops of at most this many chunks, in their one-chunk layout
// (TQ_S2_SEQCH, default 2).  Measured r04: C2's 29 levels of 4-chunk ops as one chain are
// 0.404 ms against 0.363 one launch per level on a fast box -- ~6 us of gate passes per op on
// ONE CU cost more than the ~3 us launch gap they save -- though 0.596 against 0.677 on a box
// with slow memory round trips; C3's 2-chunk levels: 0.677 against 0.684 ms
inline int s2_seq_max_chunks() { static const int v = env_int("TQ_S2_SEQCH", 2); return v; }
// chain launches: the next op's descriptor prefetched (TQ_S2_SEQPF, default 1)
inline bool s2_seq_prefetch() { static const bool v = env_on("TQ_S2_SEQPF"); return v; }
// chain launches on (TQ_S2_SEQ, default 1; tq_plan_set "sweep_chain" per plan)
inline bool s2_seq_enabled() { static const bool v = env_on("TQ_S2_SEQ"); return v; }
// tensors of more elements than this (TQ_S2_SMALL, default 2^22) keep >= 32 columns per chunk
inline int64_t s2_small_elems() { static const int64_t v = env_int64("TQ_S2_SMALL", int64_t(1) << 22); return v; }
// chunks a big sweep2 op is split into at least (TQ_S2_MINCHUNKS): 128 since r05 (the deferred
// C4 path's 2^19-element levels, two halves per launch: 0.766 -> 0.747 ms per block, two blocks
// in flight 0.565 -> 0.520; C2 / C3 +-0; 64 / 512: 0.80 / 0.88, profiles/knobs_r05.txt)
inline int s2_min_chunks() { static const int v = env_int("TQ_S2_MINCHUNKS", 128); return v; }
// arena the lane copies may add in total (TQ_LANE_ARENA_MB, default 6 GiB of the 288 GB):
// C3's 6-MiB per-slice part gets 16 lanes, C4's 1.1 GiB gets 4 (measured: 16.4 -> 15.9 ms/step)
inline size_t lane_arena_budget() {
  static const size_t v = (size_t)env_int("TQ_LANE_ARENA_MB", 6144, 0, INT_MAX) << 20;
  return v;
}
// slices per batch when the per-slice working set is small (TQ_SLICE_LANES, default 32; 1 = off;
// C3 with the capped sweep2 launches: 1.27 ms per step at 8 lanes, 1.18 at 16; r04 with 32-op
// sweep2 launches: 0.778 -> 0.726 ms at 32 (two launches per per-slice level, half the GEMM /
// reduce / permute batches), profiles/knobs_r04.jsonl)
inline int slice_lanes() { static const int v = env_int("TQ_SLICE_LANES", 32, 1, 64); return v; }
// TQ_S2_SWZ=0: sweep2 tiles keep the r04 column-only swizzle instead of the modeled one
inline bool s2_swz_model() { static const bool v = env_on("TQ_S2_SWZ"); return v; }
// TQ_S2_LANEBLK=1: register blocks of 6 positions over 4 lanes (lane blocks; off by default:
// 28 % fewer passes on C4's big sweep ops, the same time -- DESIGN.md §3.3)
inline bool s2_lane_blocks() { static const bool v = env_opt_in("TQ_S2_LANEBLK"); return v; }
// TQ_S2_WAVELOCAL=0: a workgroup barrier between every two sweep2 passes
inline bool s2_wave_local() { static const bool v = env_on("TQ_S2_WAVELOCAL"); return v; }
// narrowest chunk (log2 columns) of the small-tensor rule (TQ_S2_MINLC; 1 since r04: with the
// 32-lane batches and 4096-element register-block tiles C2 0.399 -> 0.365 ms, C3 0.786 ->
// 0.700, C4 N = 8 rank 2.21 -> 2.12, profiles/knobs_r04.jsonl; r03 measured 2 better alone)
inline int s2_min_logc() { static const int v = env_int("TQ_S2_MINLC", 1, 0, 5); return v; }
// ... for tiles of >= 2^9 positions (TQ_S2_MINLC_BIG, default 0: one column): such a chunk
// holds >= 512 elements per column, so a narrower chunk halves a workgroup's gate-pass VALU
// (passes are VALU-issue bound, probes/pass_probe.hip) and doubles the workgroups.  Measured
// r04 (C2: 26 levels of 1024-position tiles, 2 -> 1 column, 4 -> 8 chunks): 0.323 -> 0.303 ms;
// applied to every small tensor it left C3 / the C4 N = 8 rank +-0.4 % (not kept there)
inline int s2_min_logc_big() { static const int v = env_int("TQ_S2_MINLC_BIG", 0, 0, 5); return v; }
// narrowest chunk (log2 columns) of a sweep2 op before the tile / min-chunk caps (TQ_S2_LC):
// 7 since r03 (C3's per-slice ops, 128-element tiles: 32 -> 128 columns per chunk, 1.16 ->
// 1.04 ms per step with the capped launches; C4 and C2 +-0; 8-10 no better)
inline int s2_base_logc() { static const int v = env_int("TQ_S2_LC", 7, 0, 10); return v; }
// TQ_S2_BLOCKS=0: no register blocks; TQ_S2_EPI=0: no store-phase epilogue; TQ_SWEEP2=0: chains
// run as table sweeps (tq_sweep.hip); TQ_S2_DENSE=0: no dense form (tq_sweepd.hip)
inline bool s2_blocks_enabled() { static const bool v = env_on("TQ_S2_BLOCKS"); return v; }
inline bool s2_epi_enabled() { static const bool v = env_on("TQ_S2_EPI"); return v; }
inline bool s2_enabled() { static const bool v = env_on("TQ_SWEEP2"); return v; }
inline bool s2_dense_enabled() { static const bool v = env_on("TQ_S2_DENSE"); return v; }
// the pre-split boundary GEMM (TQ_GEMM_PLANES=0: the GEMM-side split kernel instead)
inline bool planes_enabled() { static const bool v = env_on("TQ_GEMM_PLANES"); return v; }
// TQ_FOLD_SLICES=0: an execute call that covers every slice runs the slice lanes all the same
// (default 1: the plan's whole program, Plan::whole; tq_plan_set "fold_slices" per plan)
inline bool fold_slices_enabled() { static const bool v = env_on("TQ_FOLD_SLICES"); return v; }
// TQ_S2_REORDER (default 1): commute a chain's square gates into fuller register blocks
inline bool s2_reorder_on() { static const bool v = env_on("TQ_S2_REORDER"); return v; }
// TQ_SKINNY_STRIDED=0: tiny-output GEMM steps permute their operands like any other
inline bool skinny_strided_enabled() { static const bool v = env_on("TQ_SKINNY_STRIDED"); return v; }
// TQ_S2_DUMP (set: any value): every sweep2 op's passes, and the block-gate histogram of
// plan_s2_gate_work, on stderr; read at each use
inline bool s2_dump() { return env_set("TQ_S2_DUMP"); }

// the launch sequence of one execute call of a plan / of a lockstep group (tq_plan_exec.cpp)
int plan_enqueue(Plan& P, const void* const* inputs, void* out, int64_t s_begin, int64_t s_end,
                 int64_t s_step, int accumulate, hipStream_t stream);
int group_enqueue(Plan* const* plans, int n, const void* const* const* inputs, void* const* outs, int64_t s_begin,
                  int64_t s_end, int64_t s_step, int accumulate, hipStream_t stream);
// the pre-split boundary GEMM runs: the plan has one, its buffers exist, the plan option is on
// and the pre-split (predicted-scale) mode of the split kernel is not running
inline bool planes_active(const Plan& P) {
  return P.planes_gemm >= 0 && P.d_planes != nullptr && P.use_planes && !P.run_mode;
}
uint64_t next_plan_serial();   // process-unique plan ids (Plan::serial; tq_plan_run.cpp)

}  // namespace tq
