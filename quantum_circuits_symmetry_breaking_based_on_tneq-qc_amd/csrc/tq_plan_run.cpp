// A plan's device life and its execute calls:
//   * plan_materialize uploads the tables and allocates the arena (or takes the caller's),
//     plan_release frees what the plan holds (retryable: nothing is forgotten before its release
//     succeeded), plan_profile_read sums the executor's event records;
//   * plan_prepare takes the device memory of the program an execute call runs -- the slice lanes,
//     or the plan's whole program (Plan::whole) when the call covers every slice (plan_folds) --
//     at that program's first use;
//   * frozen_begin / frozen_ran keep a program's frozen results (Plan::n_sched_frozen): which
//     pointers they were computed from, whether a call may skip their schedule, the event behind it;
//   * plan_run checks the call, picks the pre-split mode, runs the call (plan_launch) and re-runs
//     the slices whose pre-split scale window was missed; plan_run_group does the same for a
//     lockstep group of plans compiled from one network;
//   * both replay the call as a hipGraph unless it has to run eagerly (run_eagerly): graph_run is
//     the one cache of instantiated graphs, keyed by the call's pointers, slice range and flags
//     (a group's graph lives in its first plan, keyed by every member's serial as well).
// What a call launches is plan_enqueue / group_enqueue (the executor, tq_plan_exec.cpp).
#include "tq_plan_internal.h"

#include <algorithm>
#include <atomic>
#include <cstring>

namespace tq {

int plan_materialize(Plan& P, void* arena, void* tables, hipStream_t stream) {
  TQ_HIP(hipGetDevice(&P.device));
  if (!P.serial) P.serial = next_plan_serial();
  if (arena || tables) {
    P.d_arena = arena;
    P.d_tables = tables;
    P.owns_device = false;
  } else {
    P.owns_device = true;
    if (P.arena_bytes) TQ_HIP(hipMalloc(&P.d_arena, P.arena_bytes));
    if (P.table_bytes) TQ_HIP(hipMalloc(&P.d_tables, P.table_bytes));
  }
  if (P.table_bytes) {
    std::vector<char> host(P.table_bytes, 0);
    for (size_t i = 0; i < P.perms.size(); ++i)
      if (perm_plan_table_bytes(P.perms[i])) perm_plan_pack_table(P.perms[i], host.data() + P.perm_tab_off[i]);
    for (size_t i = 0; i < P.gtabs.size(); ++i)
      std::memcpy(host.data() + P.gtab_off[i], P.gtabs[i].data(), P.gtabs[i].size() * sizeof(int32_t));
    for (size_t i = 0; i < P.stabs.size(); ++i)
      std::memcpy(host.data() + P.stab_off[i], P.stabs[i].data(), P.stabs[i].size());
    TQ_HIP(hipMemcpyAsync(P.d_tables, host.data(), P.table_bytes, hipMemcpyHostToDevice, stream));
    TQ_HIP(hipStreamSynchronize(stream));
  }
  if (P.n_ps && !P.h_bad) TQ_HIP(hipHostMalloc((void**)&P.h_bad, P.n_slices * sizeof(uint32_t), hipHostMallocDefault));
  // the pre-split boundary GEMM's planes, partials and scale words (plan-owned plans only)
  if (P.planes_gemm >= 0 && P.owns_device && !P.d_planes) {
    plan_planes_layout(P);
    if (hipMalloc(&P.d_planes, P.planes_bytes) != hipSuccess) {
      (void)hipGetLastError();
      P.d_planes = nullptr;   // no room: the GEMM-side split path runs instead
    }
  }
  P.resident = true;
  return TQ_OK;
}

bool plan_folds(const Plan& P, int64_t s_begin, int64_t s_end, int64_t s_step) {
  // (cooperative chain launches, opt-in and checked after the call, stay with the slice lanes)
  return P.whole && P.fold_ok && P.use_fold && !P.fold_failed && !P.use_coop && s_begin == 0 &&
         s_end == P.n_slices && s_step == 1;
}

int plan_prepare(Plan& P, int64_t s_begin, int64_t s_end, int64_t s_step, hipStream_t stream) {
  if (P.device < 0) TQ_HIP(hipGetDevice(&P.device));
  if (!P.serial) P.serial = next_plan_serial();
  if (plan_folds(P, s_begin, s_end, s_step)) {
    Plan& W = *P.whole;
    if (W.resident) return TQ_OK;
    if (plan_materialize(W, nullptr, nullptr, stream) == TQ_OK) return TQ_OK;
    // no room for the whole program: what it took is given back and the plan keeps to the slice
    // lanes for good (like a missing d_planes keeps the GEMM-side split path)
    (void)hipGetLastError();
    (void)plan_release(W);
    P.fold_failed = true;
  }
  if (!P.resident) TQ_TRY(plan_materialize(P, nullptr, nullptr, stream));
  return TQ_OK;
}

int plan_prepare_group(Plan* const* plans, int n, int64_t s_begin, int64_t s_end, int64_t s_step, hipStream_t stream) {
  // a group folds when every member does; one member without its whole program puts all on the lanes
  bool fold = true;
  for (int k = 0; k < n; ++k) fold = fold && plan_folds(*plans[k], s_begin, s_end, s_step);
  if (fold) {
    for (int k = 0; k < n; ++k) TQ_TRY(plan_prepare(*plans[k], s_begin, s_end, s_step, stream));
    for (int k = 0; k < n; ++k) fold = fold && plan_folds(*plans[k], s_begin, s_end, s_step);
    if (fold) return TQ_OK;
  }
  for (int k = 0; k < n; ++k)
    if (!plans[k]->resident) TQ_TRY(plan_materialize(*plans[k], nullptr, nullptr, stream));
  return TQ_OK;
}

void plan_profile_set(Plan& P, unsigned mask) {
  for (Plan* q : {&P, P.whole.get()}) {
    if (!q) continue;
    for (auto& ev : q->ev_used) q->ev_free.push_back(ev);  // reset: recycle recorded events
    q->ev_used.clear();
    q->profile = mask;
  }
}

int plan_profile_read(Plan& P, int kind, double* ms, int64_t* launches, double* flops,
                      double* bytes) {
  double t = 0, f = 0, b = 0;
  int64_t n = 0;
  // (a folded call's records are the whole program's)
  for (Plan* q : {&P, P.whole.get()}) {
    if (!q) continue;
    for (auto& ev : q->ev_used) {
      if (kind >= 0 && ev.kind != kind) continue;
      TQ_HIP(hipEventSynchronize(ev.b));
      float e = 0;
      TQ_HIP(hipEventElapsedTime(&e, ev.a, ev.b));
      t += e; f += ev.flops; b += ev.bytes; ++n;
    }
  }
  if (ms) *ms = t;
  if (launches) *launches = n;
  if (flops) *flops = f;
  if (bytes) *bytes = b;
  return TQ_OK;
}

bool graphs_enabled() {
  static const bool v = env_on("TQ_GRAPH");
  return v;
}

uint64_t next_plan_serial() {
  static std::atomic<uint64_t> c{0};
  return ++c;
}

namespace {

// HIP release calls: the first failure is recorded (tq_last_error) and reported; a resource is
// forgotten only once its release succeeded, so a release refused mid-way (e.g. by a stream
// capture elsewhere in the process: HIP refuses hipGraphExecDestroy / hipFree while any stream
// captures in global mode) can be retried later with nothing leaked or freed twice
int rel(hipError_t e, const char* what, int& rc) {
  if (e == hipSuccess) return 1;
  if (rc == TQ_OK) set_error(std::string("HIP error ") + hipGetErrorString(e) + " releasing " + what);
  rc = TQ_ERR_HIP;
  return 0;
}

int drop_graph_entry(Plan::GraphEntry& g) {
  int rc = TQ_OK;
  if (g.done && rel(hipEventSynchronize(g.done), "graph event", rc) && rel(hipEventDestroy(g.done), "graph event", rc))
    g.done = nullptr;
  if (g.exec && rel(hipGraphExecDestroy(g.exec), "graph exec", rc)) g.exec = nullptr;
  if (g.graph && rel(hipGraphDestroy(g.graph), "graph", rc)) g.graph = nullptr;
  if (rc == TQ_OK) g = Plan::GraphEntry{};
  return rc;
}

int drop_graph(Plan& P) {
  int rc = TQ_OK;
  std::vector<Plan::GraphEntry> keep;
  for (auto& g : P.graphs)
    if (drop_graph_entry(g) != TQ_OK) {
      rc = TQ_ERR_HIP;
      keep.push_back(g);
    }
  P.graphs.swap(keep);
  return rc;
}

// An execute call runs eagerly (its launches go into the caller's stream, not through a graph of
// the plan's own) when profiling is on, the plan's "graph" option is 0, TQ_GRAPH=0, or the
// caller's stream is capturing (a torch.cuda.graph around the call).  A capture forces it: a graph
// of the plan's own, built on its side stream and launched into the capturing stream, ran once at
// capture time and was not part of the caller's replays.  The stream is queried only when the
// first three leave the choice open.
int run_eagerly(const Plan& P, hipStream_t stream, bool* eager) {
  *eager = true;
  if (P.profile || !P.use_graph || !graphs_enabled()) return TQ_OK;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  TQ_HIP(hipStreamIsCapturing(stream, &cs));
  *eager = cs != hipStreamCaptureStatusNone;
  return TQ_OK;
}

// The graph cache (Plan::graphs of P, at most kMaxGraphs entries): replay the graph cached under
// `key` on `stream`; on a miss, first capture what enqueue(P.cap_stream) launches and instantiate
// it, evicting the least recently used entry of a full cache.  Every launch is followed by the
// entry's `done` event, which a later eviction or plan_release waits on.
template <typename Enqueue>
int graph_run(Plan& P, const Plan::GraphKey& key, hipStream_t stream, Enqueue&& enqueue) {
  constexpr size_t kMaxGraphs = 8;
  Plan::GraphEntry* hit = nullptr;
  for (auto& g : P.graphs) if (g.key == key) hit = &g;
  if (!hit) {
    if (P.graphs.size() >= kMaxGraphs) {  // evict the least recently used (after it finished)
      auto lru = std::min_element(P.graphs.begin(), P.graphs.end(),
                                  [](const Plan::GraphEntry& a, const Plan::GraphEntry& b) { return a.used < b.used; });
      drop_graph_entry(*lru);
      P.graphs.erase(lru);
    }
    if (!P.cap_stream) TQ_HIP(hipStreamCreateWithFlags(&P.cap_stream, hipStreamNonBlocking));
    TQ_HIP(hipStreamBeginCapture(P.cap_stream, hipStreamCaptureModeThreadLocal));
    const int rc = enqueue(P.cap_stream);
    hipGraph_t g = nullptr;
    const hipError_t ce = hipStreamEndCapture(P.cap_stream, &g);
    if (rc != TQ_OK) {
      if (g) (void)hipGraphDestroy(g);
      return rc;
    }
    TQ_HIP(ce);
    Plan::GraphEntry e;
    e.key = key;
    e.graph = g;
    TQ_HIP(hipGraphInstantiate(&e.exec, g, nullptr, nullptr, 0));
    TQ_HIP(hipEventCreateWithFlags(&e.done, hipEventDisableTiming));
    P.graphs.push_back(e);
    hit = &P.graphs.back();
    ++P.graph_builds;
  }
  hit->used = ++P.graph_clock;
  TQ_HIP(hipGraphLaunch(hit->exec, stream));
  TQ_HIP(hipEventRecord(hit->done, stream));
  ++P.graph_launches;
  return TQ_OK;
}

// Frozen results of program R (Plan::n_sched_frozen > 0), before an execute call with `inputs` on
// `stream`: *live = the call skips the frozen schedule (the results are valid and were computed
// from these pointers; on another stream than theirs the call first waits for them), *track = the
// call updates the state afterwards (frozen_ran).  A call enqueued into a caller's capture runs
// everything and leaves the state alone: a capture must not bake in the skip.
int frozen_begin(Plan& R, const void* const* inputs, bool empty, hipStream_t stream, bool* live, bool* track) {
  *live = *track = false;
  R.live_only = false;
  if (!R.n_sched_frozen || empty) return TQ_OK;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  TQ_HIP(hipStreamIsCapturing(stream, &cs));
  if (cs != hipStreamCaptureStatusNone) return TQ_OK;
  *track = true;
  bool ok = R.frozen_valid && R.frozen_ptrs.size() == R.frozen_inputs.size();
  for (size_t q = 0; ok && q < R.frozen_inputs.size(); ++q) ok = inputs[R.frozen_inputs[q]] == R.frozen_ptrs[q];
  if (!ok) {
    R.frozen_valid = false;
    return TQ_OK;
  }
  if (stream != R.frozen_stream) TQ_HIP(hipStreamWaitEvent(stream, R.frozen_ev, 0));
  *live = R.live_only = true;
  return TQ_OK;
}

// ... after a tracked call that ran the frozen schedule: remember the pointers, record the event
int frozen_ran(Plan& R, const void* const* inputs, hipStream_t stream) {
  R.frozen_ptrs.clear();
  for (int i : R.frozen_inputs) R.frozen_ptrs.push_back(inputs[i]);
  if (!R.frozen_ev) TQ_HIP(hipEventCreateWithFlags(&R.frozen_ev, hipEventDisableTiming));
  TQ_HIP(hipEventRecord(R.frozen_ev, stream));
  R.frozen_stream = stream;
  R.frozen_valid = true;
  ++R.frozen_runs;
  return TQ_OK;
}

// one execute call of one plan: eagerly, or as the replay of its hipGraph.  W: the plan's whole
// program when the call runs it (its one "slice" is the sum over every slice); the graph is P's
int plan_launch(Plan& P, Plan* W, const void* const* inputs, void* out, int64_t s_begin, int64_t s_end,
                int64_t s_step, int accumulate, hipStream_t stream) {
  Plan& R = W ? *W : P;
  bool live = false, track = false;
  TQ_TRY(frozen_begin(R, inputs, !W && s_begin >= s_end, stream, &live, &track));
  auto enqueue = [&](hipStream_t s) {
    if (W) return plan_enqueue(*W, inputs, out, 0, 1, 1, accumulate, s);
    return plan_enqueue(P, inputs, out, s_begin, s_end, s_step, accumulate, s);
  };
  auto done = [&](int rc) {
    if (rc == TQ_OK && track && !live) rc = frozen_ran(R, inputs, stream);
    return rc;
  };
  bool eager = true;
  TQ_TRY(run_eagerly(P, stream, &eager));
  if (eager) return done(enqueue(stream));
  Plan::GraphKey key;
  key.inputs.assign(inputs, inputs + P.n_inputs);
  key.out = out; key.b = s_begin; key.e = s_end; key.s = s_step; key.acc = accumulate;
  key.mode = P.run_mode;
  key.planes = planes_active(W ? *W : P) ? 1 : 0;
  key.seq = P.use_seq;
  key.coop = P.use_coop;
  key.prog = W ? 1 : 0;
  key.live = live ? 1 : 0;
  return done(graph_run(P, key, stream, enqueue));
}

// the plans of a group are the same compiled network (identical op lists and schedules)
bool same_structure(const Plan& a, const Plan& b) {
  if (a.dtype != b.dtype || a.ops.size() != b.ops.size() || a.sched_once != b.sched_once ||
      a.sched_slice != b.sched_slice || a.n_sched_frozen != b.n_sched_frozen || a.full_steps != b.full_steps ||
      a.lanes != b.lanes ||
      a.n_slices != b.n_slices || a.seq_once != b.seq_once || a.seq_stream != b.seq_stream ||
      a.use_seq != b.use_seq || a.use_coop != b.use_coop || a.coop_once != b.coop_once || a.n_inputs != b.n_inputs ||
      planes_active(a) != planes_active(b) || a.planes_gemm != b.planes_gemm)
    return false;
  for (size_t i = 0; i < a.ops.size(); ++i)
    if (a.ops[i].kind != b.ops[i].kind || a.ops[i].stab != b.ops[i].stab || a.ops[i].stab1 != b.ops[i].stab1 ||
        a.ops[i].invariant != b.ops[i].invariant || a.ops[i].frozen != b.ops[i].frozen ||
        a.ops[i].writes_output != b.ops[i].writes_output)
      return false;
  return true;
}

}  // namespace

int plan_release(Plan& P) {
  int rc = drop_graph(P);
  // the whole program's memory: after this plan's graphs (which address it) have finished
  if (P.whole && rc == TQ_OK) rc = plan_release(*P.whole);
  if (P.cap_stream && rel(hipStreamDestroy(P.cap_stream), "capture stream", rc)) P.cap_stream = nullptr;
  auto drop_events = [&](std::vector<Plan::Ev>& v) {
    std::vector<Plan::Ev> keep;
    for (auto& ev : v) {
      if (ev.a && rel(hipEventDestroy(ev.a), "event", rc)) ev.a = nullptr;
      if (ev.b && rel(hipEventDestroy(ev.b), "event", rc)) ev.b = nullptr;
      if (ev.a || ev.b) keep.push_back(ev);
    }
    v.swap(keep);
  };
  drop_events(P.ev_used);
  drop_events(P.ev_free);
  {
    std::vector<hipStream_t> ks;
    for (auto s : P.side_streams)
      if (!rel(hipStreamDestroy(s), "group side stream", rc)) ks.push_back(s);
    P.side_streams.swap(ks);
    std::vector<hipEvent_t> ke;
    for (auto e : P.side_events)
      if (!rel(hipEventDestroy(e), "group event", rc)) ke.push_back(e);
    P.side_events.swap(ke);
  }
  if (P.owns_device) {
    if (P.d_arena && rel(hipFree(P.d_arena), "arena", rc)) P.d_arena = nullptr;
    if (P.d_tables && rel(hipFree(P.d_tables), "tables", rc)) P.d_tables = nullptr;
  } else {
    P.d_arena = P.d_tables = nullptr;
  }
  if (P.h_bad && rel(hipHostFree(P.h_bad), "host flag", rc)) P.h_bad = nullptr;
  if (P.d_planes && rel(hipFree(P.d_planes), "planes", rc)) P.d_planes = nullptr;
  // (the frozen results go with the arena)
  P.frozen_valid = false;
  if (P.frozen_ev && rel(hipEventDestroy(P.frozen_ev), "frozen event", rc)) P.frozen_ev = nullptr;
  if (!P.d_arena && !P.d_tables) P.resident = false;
  return rc;
}

namespace {
int run_one(Plan& P, const void* const* inputs, void* out, int64_t s_begin, int64_t s_end,
            int64_t s_step, int accumulate, hipStream_t stream);
int run_group(Plan* const* plans, int n, const void* const* const* inputs, void* const* outs, int64_t s_begin,
              int64_t s_end, int64_t s_step, int accumulate, hipStream_t stream);
}  // namespace

// (an execute call that returned an error leaves no frozen results behind)
int plan_run(Plan& P, const void* const* inputs, void* out, int64_t s_begin, int64_t s_end,
             int64_t s_step, int accumulate, hipStream_t stream) {
  const int rc = run_one(P, inputs, out, s_begin, s_end, s_step, accumulate, stream);
  if (rc != TQ_OK) plan_frozen_invalidate(P);
  return rc;
}

int plan_run_group(Plan* const* plans, int n, const void* const* const* inputs, void* const* outs, int64_t s_begin,
                   int64_t s_end, int64_t s_step, int accumulate, hipStream_t stream) {
  TQ_CHECK_ARG(n >= 1 && plans && inputs && outs, "empty group");
  if (n == 1) return plan_run(*plans[0], inputs[0], outs[0], s_begin, s_end, s_step, accumulate, stream);
  const int rc = run_group(plans, n, inputs, outs, s_begin, s_end, s_step, accumulate, stream);
  if (rc != TQ_OK)
    for (int k = 0; k < n; ++k) plan_frozen_invalidate(*plans[k]);
  return rc;
}

namespace {

int run_one(Plan& P, const void* const* inputs, void* out, int64_t s_begin, int64_t s_end,
            int64_t s_step, int accumulate, hipStream_t stream) {
  TQ_CHECK_ARG(s_step >= 1, "slice_step");
  TQ_CHECK_ARG(s_begin >= 0 && s_end <= P.n_slices, "slice range");
  // the whole program runs a call over every slice once its memory is there (plan_prepare)
  Plan* W = plan_folds(P, s_begin, s_end, s_step) && P.whole->resident ? P.whole.get() : nullptr;
  TQ_CHECK_ARG(W ? (W->arena_bytes == 0 || W->d_arena) : (P.arena_bytes == 0 || P.d_arena), "plan not materialized");
  {
    // a plan's arena, tables and graphs live on one device; running it with another device
    // current would hand that device foreign pointers
    int cur = -1;
    TQ_HIP(hipGetDevice(&cur));
    TQ_CHECK_ARG(P.device < 0 || cur == P.device,
                 "plan was materialized on device " + std::to_string(P.device) +
                     " but device " + std::to_string(cur) + " is current");
  }
  // pre-split GEMM operands (Op::ps_cand) when every candidate still takes the f16 split path
  // under the current library switches, and the stream is not being captured by the caller
  // (the window check below synchronizes)
  P.run_mode = 0;
  if (W) {
    // the per-plan options follow the parent; no pre-split (predicted-scale) GEMM mode
    W->use_seq = P.use_seq;
    W->use_planes = P.use_planes;
    W->use_coop = false;
    W->profile = P.profile;
    W->run_mode = 0;
    TQ_TRY(plan_launch(P, W, inputs, out, s_begin, s_end, s_step, accumulate, stream));
    ++P.folded_executes;
    return TQ_OK;
  }
  if (P.n_ps && P.h_bad) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    TQ_HIP(hipStreamIsCapturing(stream, &cs));
    bool ok = cs == hipStreamCaptureStatusNone;
    for (const Op& op : P.ops)
      if (op.ps_cand && !gemm_c64_presplit_ok(op.transA, op.transB, op.M, op.N, op.K, op.batch, op.lda, op.ldb))
        ok = false;
    P.run_mode = ok ? 1 : 0;
  }
  TQ_TRY(plan_launch(P, nullptr, inputs, out, s_begin, s_end, s_step, accumulate, stream));
  if (P.use_coop && !P.coop_once.empty() && P.d_tables) {
    // cooperative chain launches (opt-in) rely on their workgroups being co-resident; a wait
    // that gave up (sync[1], counted by the kernel) means the op read stale data: the execute
    // synchronizes to check (outside a caller's capture) and fails instead of returning it
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    TQ_HIP(hipStreamIsCapturing(stream, &cs));
    if (cs == hipStreamCaptureStatusNone) {
      uint32_t gaveup = 0;
      for (size_t r = 0; r < P.coop_once.size(); ++r) {
        uint32_t w = 0;
        char* slot = (char*)P.d_tables + P.sync_off + r * Plan::kSyncSlot + 4;
        TQ_HIP(hipMemcpyAsync(&w, slot, 4, hipMemcpyDeviceToHost, stream));
        TQ_HIP(hipStreamSynchronize(stream));
        if (w) TQ_HIP(hipMemsetAsync(slot, 0, 4, stream));
        gaveup += w;
      }
      if (gaveup) {
        TQ_HIP(hipStreamSynchronize(stream));
        set_error("cooperative sweep chain: " + std::to_string(gaveup) +
                  " workgroup wait(s) gave up (workgroups not co-resident); the result is invalid -- "
                  "run with sweep_coop 0");
        return TQ_ERR_HIP;
      }
    }
  }
  if (P.run_mode) {
    // slices whose operand max left its scale window produced zeros: add them on the split path
    const uint32_t* dbad = reinterpret_cast<const uint32_t*>((const char*)P.d_tables + P.bad_off);
    TQ_HIP(hipMemcpyAsync(P.h_bad, dbad, P.n_slices * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    TQ_HIP(hipStreamSynchronize(stream));
    // a lane-batched candidate GEMM flags its whole batch in the batch's first slice (the
    // other lanes' words are not written): batches are consecutive groups of `lanes` slices
    bool batched = false;
    for (const Op& op : P.ops) batched = batched || (op.ps_cand && op.lane_batch);
    std::vector<int64_t> redo, batch;
    for (int64_t sl = s_begin; sl < s_end; sl += s_step * std::max(1, P.lanes)) {
      batch.clear();
      for (int64_t q = sl; q < s_end && (int64_t)batch.size() < std::max(1, P.lanes); q += s_step) batch.push_back(q);
      for (int64_t q : batch)
        if (batched ? P.h_bad[batch[0]] != 0 : P.h_bad[q] != 0) redo.push_back(q);
    }
    P.run_mode = 0;
    P.live_only = P.n_sched_frozen > 0 && P.frozen_valid;   // (the call above has left them valid)
    for (int64_t sl : redo) TQ_TRY(plan_enqueue(P, inputs, out, sl, sl + 1, 1, 1, stream));
    P.ps_fallbacks += (int64_t)redo.size();
  }
  return TQ_OK;
}

int run_group(Plan* const* plans, int n, const void* const* const* inputs, void* const* outs, int64_t s_begin,
              int64_t s_end, int64_t s_step, int accumulate, hipStream_t stream) {
  Plan& P0 = *plans[0];
  TQ_CHECK_ARG(s_step >= 1, "slice_step");
  TQ_CHECK_ARG(s_begin >= 0 && s_end <= P0.n_slices, "slice range");
  int cur = -1;
  TQ_HIP(hipGetDevice(&cur));
  // every member's whole program (a call over every slice, each one's memory there), or the lanes
  bool fold = true;
  for (int k = 0; k < n; ++k)
    fold = fold && plan_folds(*plans[k], s_begin, s_end, s_step) && plans[k]->whole->resident;
  std::vector<Plan*> run(plans, plans + n);
  for (int k = 0; k < n; ++k) {
    Plan& P = *plans[k];
    if (fold) {
      Plan& W = *P.whole;
      W.use_seq = P.use_seq;
      W.use_planes = P.use_planes;
      W.use_coop = false;
      W.profile = P.profile;
      run[k] = &W;
    }
    TQ_CHECK_ARG(run[k]->arena_bytes == 0 || run[k]->d_arena, "plan not materialized");
    TQ_CHECK_ARG(P.device < 0 || cur == P.device, "a group plan was materialized on another device");
    for (int q = 0; q < k; ++q)
      TQ_CHECK_ARG(plans[q] != plans[k] && outs[q] != outs[k], "a group runs distinct plans into distinct outputs");
    P.run_mode = run[k]->run_mode = 0;   // no pre-split (predicted-scale) GEMM mode in a group
    TQ_CHECK_ARG(same_structure(P0, P) && same_structure(*run[0], *run[k]),
                 "the plans of a group must be compiled from the same network");
  }
  TQ_CHECK_ARG(!P0.use_coop, "cooperative chain launches do not run in a group");
  auto enqueue = [&](hipStream_t s) {
    if (fold) return group_enqueue(run.data(), n, inputs, outs, 0, 1, 1, accumulate, s);
    return group_enqueue(plans, n, inputs, outs, s_begin, s_end, s_step, accumulate, s);
  };
  if (fold)
    for (int k = 0; k < n; ++k) ++plans[k]->folded_executes;
  // the group is live-only when every member's frozen results are valid; otherwise every member
  // runs its frozen schedule again (idempotent; one rule keeps the lockstep schedule uniform)
  bool live = true, track = true;
  for (int k = 0; k < n; ++k) {
    bool lk = false, tk = false;
    TQ_TRY(frozen_begin(*run[k], inputs[k], !fold && s_begin >= s_end, stream, &lk, &tk));
    live = live && lk;
    track = track && tk;
  }
  for (int k = 0; k < n; ++k) run[k]->live_only = live;
  auto done = [&](int rc) {
    for (int k = 0; k < n && rc == TQ_OK && track && !live; ++k) rc = frozen_ran(*run[k], inputs[k], stream);
    return rc;
  };
  bool eager = true;
  TQ_TRY(run_eagerly(P0, stream, &eager));
  if (eager) return done(enqueue(stream));
  // one hipGraph of the whole group, cached in the first plan under every member's serial,
  // inputs and output (a serial is never reused, so a replay cannot address a freed plan)
  Plan::GraphKey key;
  for (int k = 0; k < n; ++k) {
    key.inputs.insert(key.inputs.end(), inputs[k], inputs[k] + plans[k]->n_inputs);
    key.group.push_back(outs[k]);
    key.group.push_back(reinterpret_cast<const void*>((uintptr_t)plans[k]->serial));
  }
  key.out = outs[0]; key.b = s_begin; key.e = s_end; key.s = s_step; key.acc = accumulate;
  key.planes = planes_active(*run[0]) ? 1 : 0;
  key.seq = P0.use_seq;
  key.prog = fold ? 1 : 0;
  key.live = live ? 1 : 0;
  return done(graph_run(P0, key, stream, enqueue));
}

}  // namespace

}  // namespace tq
