// Plan executor: the launch sequence of one execute call, enqueued into a stream (eagerly, or
// into the capture the graph cache of tq_plan_run.cpp replays).  One plan, or a GROUP of plans
// compiled from the same network (blocks as lanes).
// A group executes its plans' schedules in lockstep: every sweep2 level (and dense-sweep level,
// and chain launch) of all instances is ONE launch whose op list holds every instance's ops --
// the slice-lane mechanism with an instance index -- so G amplitude blocks in flight cost the
// launches of one; the other ops (GEMM, permute, lane sum, ...) run per instance, member k > 0 on
// a side stream of its own.  A group of one plan is exactly the single-plan executor.
// Per execute call: the hoisted (slice-invariant) schedule once -- without its frozen entries when
// the call is live-only (Plan::live_only) -- as single launches, chain launches
// (Plan::seq_once) and opt-in cooperative chain launches (Plan::coop_once) -- then the per-slice
// schedule for every batch of Plan::lanes slices: sweep2 levels merged across the batch's lanes,
// lane-batched GEMMs, lane sums, and lane by lane whatever writes the output.
#include "tq_plan_internal.h"
#include "tq_sweep.h"

#include <algorithm>

namespace tq {

namespace {

// TQ_SWEEP_LANES (default 1): per-slice table sweeps lane-merged
bool sweep_lanes_on() {
  static const bool v = env_on("TQ_SWEEP_LANES");
  return v;
}

struct Inst {
  Plan* P = nullptr;
  const void* const* inputs = nullptr;
  void* out = nullptr;
  std::vector<std::vector<int64_t>> lane_in_off;
  std::vector<int64_t> lane_sl;
  int cur = 0;             // lane the launches address
  double beta_out = 0.0;   // the first slice of a non-accumulating call overwrites the output
  bool first = true;
  bool lanes_summed = false;
};

class Exec {
 public:
  Exec(std::vector<Inst>& insts, hipStream_t stream) : I_(insts), st_(stream), P0_(*insts[0].P) {}

  int run(int64_t s_begin, int64_t s_end, int64_t s_step, int accumulate);

 private:
  std::vector<Inst>& I_;
  hipStream_t st_;
  Plan& P0_;
  int lane_gemm_ = 1;   // > 1: the GEMM launch below covers that many lanes

  size_t esz() const { return P0_.esz; }
  char* ptr(const Inst& x, const BufRef& b) const {
    const Plan& P = *x.P;
    switch (b.kind) {
      case BUF_INPUT: return (char*)x.inputs[b.index] + (x.lane_in_off[x.cur][b.index] + b.off) * P.esz;
      case BUF_ARENA: return (char*)P.d_arena + P.lane_phys + (size_t)x.cur * P.lane_stride + b.off * P.esz;
      case BUF_PINNED: return (char*)P.d_arena + b.off * P.esz;
      case BUF_OUTPUT: return (char*)x.out + b.off * P.esz;
      case BUF_TABLE: return (char*)P.d_tables + b.off;
    }
    return nullptr;
  }
  static void set_lane(Inst& x, int j) {
    x.cur = j;
    x.beta_out = (x.first && x.cur == 0) ? 0.0 : 1.0;
  }
  void set_lane_all(int j) {
    for (auto& x : I_) set_lane(x, j);
  }
  static uint32_t* amax_word(const Inst& x, int w) {
    return reinterpret_cast<uint32_t*>((char*)x.P->d_tables + x.P->amax_off) + w;
  }
  // lane j's copy of max word w: per-slice words have one set per lane (the pre-split mode keeps
  // one shared set: its scales are predicted per batch)
  static int lane_amax_stride(const Inst& x, int w) {
    return (w >= x.P->n_amax_once && !x.P->run_mode) ? x.P->n_amax_slice : 0;
  }
  static uint32_t* amax_lane(const Inst& x, int w, int j) { return amax_word(x, w + j * lane_amax_stride(x, w)); }
  // scale word of per-slice max word w; window flag of slice q
  static int32_t* sc_word(const Inst& x, int w) {
    return reinterpret_cast<int32_t*>((char*)x.P->d_tables + x.P->sc_off) + (w - x.P->n_amax_once);
  }
  static uint32_t* bad_word(const Inst& x, int64_t q) {
    return reinterpret_cast<uint32_t*>((char*)x.P->d_tables + x.P->bad_off) + q;
  }
  // the pre-split boundary GEMM: lane j's planes of operand r (0 = A, 1 = B) and scale words
  static _Float16* planes_ptr(const Inst& x, int j, int r) {
    const Plan& P = *x.P;
    return reinterpret_cast<_Float16*>((char*)P.d_planes + (size_t)j * P.planes_lane_bytes +
                                       (r ? (size_t)12 * P.planes_n[0] : 0));
  }
  static int32_t* planes_sc(const Inst& x, int j, int r) {
    return reinterpret_cast<int32_t*>((char*)x.P->d_planes + x.P->planes_sc_off) + 2 * j + r;
  }

  // profiling (HIP events on the stream; the group's first plan holds the records)
  Plan::Ev ev_begin(int kind) {
    Plan::Ev ev{};
    if (P0_.ev_free.empty()) {
      if (hipEventCreate(&ev.a) != hipSuccess || hipEventCreate(&ev.b) != hipSuccess) ev.kind = -1;
    } else {
      ev = P0_.ev_free.back();
      P0_.ev_free.pop_back();
    }
    if (ev.kind == -1) return ev;
    ev.kind = kind;
    ev.flops = 0;
    ev.bytes = 0;
    return ev;
  }

  int launch_one(Inst& x, const Op& op);
  int fill_s2(const Inst& x, S2Op& o, const Op& op, int stab) const;
  SweepArgs sweep_args(const Inst& x, const Op& op, double beta) const;
  int sweep_lanes_ = 0;   // > 0: the OP_SWEEP entry below runs every lane of the batch in one launch
  // per-instance work of a group: member k > 0 on side stream k - 1 (forked from and joined back
  // into the execution stream: parallel branches of the captured graph), member 0 on the stream
  hipStream_t ost_ = nullptr;   // the stream launch_one / lane sums use (st_ unless forked)
  template <typename F>
  int each_instance(F&& f);
  int launch_chain(int b, int e, int coop);
  int launch(const std::vector<int>& grp);
};

// the table-driven sweep op's launch record for instance x's current lane
SweepArgs Exec::sweep_args(const Inst& x, const Op& op, double beta) const {
  const Plan& P = *x.P;
      SweepArgs a;
      const char* blob = (const char*)P.d_tables + P.stab_off[op.stab];
      a.X = ptr(x, op.a);
      a.Y = ptr(x, op.c);
      a.ncols = op.ncols;
      auto lg = [](int64_t v) {
        if (v <= 0 || (v & (v - 1))) return -1;
        int l = 0;
        while ((int64_t(1) << l) < v) ++l;
        return l;
      };
      a.nruns = op.nruns;
      for (int r = 0; r < op.nruns; ++r) {
        a.run_ext[r] = op.run_ext[r]; a.run_in[r] = op.run_in[r]; a.run_out[r] = op.run_out[r];
        a.run_shift[r] = lg(op.run_ext[r]);
      }
      a.tin = op.tin;
      a.tout = op.tout;
      a.tin_shift = lg(op.tin);
      a.tout_shift = lg(op.tout);
      a.tabs = (const int32_t*)(blob + op.tabs_at);
      a.tab_len = op.tab_len;
      a.tin_off = (const int64_t*)blob;
      a.tout_off = (const int64_t*)(blob + op.tout_off_at);
      a.ngates = (int)op.sgates.size();
      for (int j = 0; j < a.ngates; ++j) {
        const SweepGate& g = op.sgates[j];
        a.G[j] = ptr(x, g.g);
        a.gidx[j] = g.gtab >= 0 ? (const int32_t*)((char*)P.d_tables + P.gtab_off[g.gtab]) : nullptr;
        a.K[j] = g.K; a.N[j] = g.N; a.W[j] = g.W;
        a.tab_at[j] = (int)g.tab_off;
      }
      // power-of-two outer extents: per-bit column-offset weights
      {
        bool p2 = true;
        int nb = 0;
        for (int r = 0; r < op.nruns && p2; ++r) {
          const int l = lg(op.run_ext[r]);
          if (l < 0 || nb + l > 48) { p2 = false; break; }
          for (int b = 0; b < l; ++b) {
            a.w_in[nb + b] = op.run_in[r] << b;
            a.w_out[nb + b] = op.run_out[r] << b;
          }
          nb += l;
        }
        a.colbits = p2 ? nb : -1;
      }
      a.load_colfast = op.load_colfast;
      a.store_colfast = op.store_colfast;
      a.use_beta = beta != 0.0;
      a.beta = beta;
  return a;
}

template <typename F>
int Exec::each_instance(F&& f) {
  static const bool fork = env_on("TQ_GROUP_FORK");
  const int n = (int)I_.size();
  if (n == 1 || !fork) {
    ost_ = st_;
    for (auto& x : I_) TQ_TRY(f(x));
    return TQ_OK;
  }
  Plan& P = P0_;
  while ((int)P.side_streams.size() < n - 1) {
    hipStream_t s = nullptr;
    TQ_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    P.side_streams.push_back(s);
  }
  while ((int)P.side_events.size() < n) {
    hipEvent_t e = nullptr;
    TQ_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    P.side_events.push_back(e);
  }
  TQ_HIP(hipEventRecord(P.side_events[0], st_));
  int rc = TQ_OK;
  for (int k = 1; k < n && rc == TQ_OK; ++k) {
    hipStream_t s = P.side_streams[k - 1];
    TQ_HIP(hipStreamWaitEvent(s, P.side_events[0], 0));
    ost_ = s;
    rc = f(I_[k]);
    TQ_HIP(hipEventRecord(P.side_events[k], s));
  }
  ost_ = st_;
  if (rc == TQ_OK) rc = f(I_[0]);
  for (int k = 1; k < n; ++k) TQ_HIP(hipStreamWaitEvent(st_, P.side_events[k], 0));
  return rc;
}

int Exec::launch_one(Inst& x, const Op& op) {
  Plan& P = *x.P;
  const hipStream_t st = ost_ ? ost_ : st_;
  const double beta = op.writes_output ? x.beta_out : 0.0;
  const bool planes_on = planes_active(P);
  if (planes_on && op.kind == OP_GEMM && &op == &P.ops[P.planes_gemm]) {
    // lane batch: entries = the batch's lanes (planes and scale words at their lane strides),
    // the combine sums them into lane 0's result when the plan sums the lanes (Op::lane_sum)
    const int j0 = lane_gemm_ > 1 ? 0 : x.cur;
    PlanesGemmArgs a;
    a.A = planes_ptr(x, j0, 0);
    a.B = planes_ptr(x, j0, 1);
    a.sA = a.sB = (int64_t)(P.planes_lane_bytes / 2);
    a.psA = P.planes_n[0];
    a.psB = P.planes_n[1];
    a.lda = op.lda;
    a.ldb = op.ldb;
    a.M = (int)op.M;
    a.N = (int)op.N;
    a.K = op.K;
    a.batch = lane_gemm_;
    a.W = reinterpret_cast<float*>((char*)P.d_planes + P.planes_ws_off);
    a.ws_bytes = P.planes_sc_off - P.planes_ws_off;
    PlanesCombineArgs c;
    c.sc_a = planes_sc(x, j0, 0);
    c.sc_b = planes_sc(x, j0, 1);
    c.sc_stride = 2;
    c.C = ptr(x, op.c);
    c.ldc = op.ldc;
    c.sC = (int64_t)(P.lane_stride / P.esz);
    c.lane_sum = lane_gemm_ > 1 && op.lane_sum;
    c.beta = (float)beta;
    return planes_gemm_launch(a, c, st);
  }
  switch (op.kind) {
    case OP_PERMUTE:
      TQ_TRY(perm_plan_launch(P.perms[op.perm], (char*)P.d_tables + P.perm_tab_off[op.perm], ptr(x, op.a),
                              ptr(x, op.c), beta, st));
      break;
    case OP_GEMM: {
      if (op.skinny) {
        SkinnyArgs a = op.sk;
        a.A = ptr(x, op.a);
        a.B = ptr(x, op.b);
        a.C = ptr(x, op.c);
        a.W = op.ws_bytes ? ptr(x, op.ws) : nullptr;
        a.beta = beta;
        TQ_TRY(skinny_strided_launch(P.dtype, a, st));
        break;
      }
      GemmPresplit ps;
      const bool pre = P.run_mode && op.ps_cand;
      if (pre) {
        ps.sc_a = sc_word(x, op.amax_a);
        ps.sc_b = sc_word(x, op.amax_b);
        ps.bad = bad_word(x, x.lane_sl[x.cur]);
      }
      if (lane_gemm_ > 1) {   // every lane of the batch in one launch (Op::lane_batch)
        const int64_t ls = (int64_t)(P.lane_stride / P.esz);
        // pre-split: one window flag for the batch, in its first slice's word
        TQ_TRY(gemm_launch(P.dtype, op.transA, op.transB, op.M, op.N, op.K, lane_gemm_, ptr(x, op.a), op.lda,
                           op.a.kind == BUF_ARENA ? ls : 0, ptr(x, op.b), op.ldb, op.b.kind == BUF_ARENA ? ls : 0,
                           beta, ptr(x, op.c), op.ldc, ls, (char*)P.d_arena + P.lane_ws_off, P.lane_ws_bytes, st,
                           op.amax_a >= 0 ? amax_word(x, op.amax_a) : nullptr,
                           op.amax_b >= 0 ? amax_word(x, op.amax_b) : nullptr, pre ? &ps : nullptr,
                           op.amax_a >= 0 ? lane_amax_stride(x, op.amax_a) : 0,
                           op.amax_b >= 0 ? lane_amax_stride(x, op.amax_b) : 0));
        break;
      }
      TQ_TRY(gemm_launch(P.dtype, op.transA, op.transB, op.M, op.N, op.K, op.batch, ptr(x, op.a), op.lda, op.sA,
                         ptr(x, op.b), op.ldb, op.sB, beta, ptr(x, op.c), op.ldc, op.sC,
                         op.ws_bytes ? ptr(x, op.ws) : nullptr, op.ws_bytes, st,
                         op.amax_a >= 0 ? amax_lane(x, op.amax_a, x.cur) : nullptr,
                         op.amax_b >= 0 ? amax_lane(x, op.amax_b, x.cur) : nullptr, pre ? &ps : nullptr));
      break;
    }
    case OP_APPLY:
      TQ_TRY(apply_launch(P.dtype, op.O, op.K, op.M, op.K2, op.I, op.N, ptr(x, op.a), ptr(x, op.b),
                          op.gtab >= 0 ? (const int32_t*)((char*)P.d_tables + P.gtab_off[op.gtab]) : nullptr,
                          ptr(x, op.c), beta, st));
      break;
    case OP_AXPY:
      TQ_TRY(axpy_launch(P.dtype, op.n, ptr(x, op.a), ptr(x, op.c), beta, st));
      break;
    case OP_SWEEP: {
      const SweepArgs a = sweep_args(x, op, beta);
      TQ_TRY(sweep_launch(P.dtype, a, st));
      break;
    }
    default:
      set_error("internal: op kind");
      return TQ_ERR_INVALID;
  }
  return TQ_OK;
}

// a sweep2 op's launch record from descriptor stabs[stab] (the instance's current lane)
int Exec::fill_s2(const Inst& x, S2Op& o, const Op& op, int stab) const {
  const Plan& P = *x.P;
  o.desc = (const S2Desc*)((const char*)P.d_tables + P.stab_off[stab]);
  o.X = ptr(x, op.a);
  o.Y = ptr(x, op.c);
  const S2Desc* hd = reinterpret_cast<const S2Desc*>(P.stabs[stab].data());
  for (size_t g = 0; g < op.sgates.size(); ++g) {
    o.G[g] = ptr(x, op.sgates[g].g);
    int mx = 0;
    for (int t = 0; t < hd->gate[g].K * hd->gate[g].N; ++t) mx = std::max(mx, hd->gate[g].gidx[t] + 1);
    if (mx > kS2GateRaw) {
      set_error("internal: sweep2 gate tensor too large");
      return TQ_ERR_INVALID;
    }
    o.gnum[g] = (uint8_t)mx;
  }
  o.beta = op.writes_output ? x.beta_out : 0.0;
  o.use_beta = o.beta != 0.0;
  o.amax = op.amax_word >= 0 ? amax_lane(x, op.amax_word, x.cur) : nullptr;
  o.split_sc = P.run_mode && op.ps_gemm >= 0 ? sc_word(x, op.amax_word) : nullptr;
  // host-built lane / chunk-base tables behind the descriptor (TQ_S2_HOSTTAB=0: computed in the
  // kernel, the r05 prologue)
  static const bool host_tabs = env_on("TQ_S2_HOSTTAB");
  const char* blob = (const char*)P.d_tables + P.stab_off[stab];
  o.rows = host_tabs ? (hd->npass & 0xff) | (hd->ngates & 0xff) << 8 | (hd->colbits & 0xff) << 16 : 0;
  o.lanes = host_tabs && hd->aux_lanes ? reinterpret_cast<const uint4*>(blob + hd->aux_lanes) : nullptr;
  o.cbase = host_tabs && hd->aux_cb ? reinterpret_cast<const int64_t*>(blob + hd->aux_cb) : nullptr;
  return TQ_OK;
}

// Plan::seq_once run [b, e): its ops in order, a workgroup per (instance, stream), one launch (as
// many instances per launch as kS2SeqMaxStreams allows); or (coop >= 0) Plan::coop_once run
// `coop`: its ops in order on coop_width workgroups each, one launch per instance
int Exec::launch_chain(int b, int e, int coop) {
  const bool prof = (P0_.profile >> (int)OP_SWEEP) & 1;
  if (coop >= 0) {
    for (auto& x : I_) {
      Plan& P = *x.P;
      Plan::Ev ev{};
      if (prof) {
        ev = ev_begin((int)OP_SWEEP);
        TQ_HIP(hipEventRecord(ev.a, st_));
      }
      const int w = P.coop_width[coop];
      S2Launch L;
      L.seq = 1;
      L.sync = reinterpret_cast<uint32_t*>((char*)P.d_tables + P.sync_off + (size_t)coop * Plan::kSyncSlot);
      for (int i = b; i < e; ++i) {
        const Op& op = P.ops[P.sched_once[i][0]];
        S2Op& o = L.op[L.nops];
        TQ_TRY(fill_s2(x, o, op, op.stab));
        o.block_begin = 0;
        o.nblocks = w;
        o.lds_io = kS2Coop | (L.nops * w) << 8 | (op.lds_io & 4);   // (bit 2: set by the planner)
        ++L.nops;
        ev.flops += op.flops;
        ev.bytes += op.bytes;
      }
      L.sync_total = L.nops * w;
      TQ_TRY(sweep2_launch(P.dtype, L, st_));
      if (prof) {
        TQ_HIP(hipEventRecord(ev.b, st_));
        P0_.ev_used.push_back(ev);
      }
    }
    return TQ_OK;
  }
  int nstreams = 1, nops = 0;
  for (int i = b; i < e; ++i)
    for (int j : P0_.sched_once[i]) {
      nstreams = std::max(nstreams, P0_.seq_stream[j] + 1);
      ++nops;
    }
  const int per = std::max(1, std::min(kS2SeqMaxStreams / nstreams, kS2MaxOps / std::max(1, nops)));
  for (size_t k0 = 0; k0 < I_.size(); k0 += (size_t)per) {
    Plan::Ev ev{};
    if (prof) {
      ev = ev_begin((int)OP_SWEEP);
      TQ_HIP(hipEventRecord(ev.a, st_));
    }
    S2Launch L;
    L.seq = 1;
    for (size_t k = k0; k < std::min(I_.size(), k0 + (size_t)per); ++k) {
      const Inst& x = I_[k];
      const Plan& P = *x.P;
      for (int i = b; i < e; ++i)
        for (int j : P.sched_once[i]) {
          const Op& op = P.ops[j];
          S2Op& o = L.op[L.nops++];
          TQ_TRY(fill_s2(x, o, op, op.stab1));
          o.lds_io = op.lds_io;
          // an LDS hand-off moves the whole tensor: the kernel's first-chunk path only
          if ((o.lds_io & 3) && reinterpret_cast<const S2Desc*>(P.stabs[op.stab1].data())->nchunks != 1) {
            set_error("internal: sweep2 LDS hand-off on a multi-chunk layout");
            return TQ_ERR_INVALID;
          }
          o.block_begin = (int)(k - k0) * nstreams + P.seq_stream[j];   // the (instance, stream) workgroup
          o.nblocks = 1;
          ev.flops += op.flops;
          ev.bytes += op.bytes;
        }
    }
    TQ_TRY(sweep2_launch(P0_.dtype, L, st_));
    if (prof) {
      TQ_HIP(hipEventRecord(ev.b, st_));
      P0_.ev_used.push_back(ev);
    }
  }
  return TQ_OK;
}

// one entry of the schedule: a single op (per instance), or independent sweep2 ops of every
// instance (and, merged across the batch, of every lane) in one launch
int Exec::launch(const std::vector<int>& grp) {
  const Op& op0 = P0_.ops[grp[0]];
  const int pkind = op0.kind == OP_SWEEP2 ? (int)OP_SWEEP : op0.kind;
  const int nl = (int)I_[0].lane_sl.size();
  Plan::Ev ev{};
  const bool prof = (P0_.profile >> pkind) & 1;
  bool lanes_merge = op0.kind == OP_SWEEP2 && nl > 1 && !op0.invariant;
  for (int j : grp) lanes_merge = lanes_merge && !P0_.ops[j].writes_output;
  if (prof) {
    ev = ev_begin(pkind);
    // a lane-batched GEMM or a sweep level merged across the batch's lanes does every lane's
    // work; a group does every instance's
    const int mult = (lanes_merge ? nl : sweep_lanes_ > 1 ? sweep_lanes_ : lane_gemm_) * (int)I_.size();
    for (int j : grp) {
      ev.flops += P0_.ops[j].flops * mult;
      ev.bytes += P0_.ops[j].bytes * mult;
    }
    TQ_HIP(hipEventRecord(ev.a, st_));
  }
  if (op0.kind == OP_SWEEP2) {
    // (instance, lane, op) triples of this level: every lane's ops when the level is merged
    // across the batch, else each instance's current lane; at most kS2MaxOps per launch
    struct Item { int k, lane, q; };
    std::vector<Item> items, dense;
    for (int k = 0; k < (int)I_.size(); ++k)
      for (int j = 0; j < (lanes_merge ? nl : 1); ++j)
        for (int q : grp) (P0_.ops[q].s2_dense ? dense : items).push_back({k, lanes_merge ? j : I_[k].cur, q});
    std::vector<int> keep(I_.size());
    for (size_t k = 0; k < I_.size(); ++k) keep[k] = I_[k].cur;
    // dense ops (tq_sweepd.hip): their own launches, at most two input tile sizes each
    // (TQ_S2D_MIX=0: one)
    static const bool s2d_mix = env_on("TQ_S2D_MIX");
    const bool s2d_nt = s2d_nt_stores();
    while (!dense.empty()) {
      S2DLaunch L;
      const int tin = P0_.ops[dense[0].q].tin;
      int tin2 = 0;
      std::vector<Item> rest;
      int blocks = 0;
      for (auto& it : dense) {
        Inst& x = I_[it.k];
        const Plan& P = *x.P;
        const Op& op = P.ops[it.q];
        if (op.tin != tin && tin2 == 0 && s2d_mix && !s2d_nt) tin2 = op.tin;
        if ((op.tin != tin && op.tin != tin2) || L.nops == kS2MaxOps) {
          rest.push_back(it);
          continue;
        }
        set_lane(x, it.lane);
        S2DOp& o = L.op[L.nops++];
        o.desc = (const S2Dense*)((const char*)P.d_tables + P.stab_off[op.stab]);
        o.X = ptr(x, op.a);
        o.M = ptr(x, op.b);
        o.Y = ptr(x, op.c);
        o.tin = op.tin;
        o.tout = op.tout;
        o.block_begin = blocks;
        o.nblocks = s2d_blocks(op.ncols);
        o.ncols = op.ncols;
        blocks += o.nblocks;
        o.beta = op.writes_output ? x.beta_out : 0.0;
        o.use_beta = o.beta != 0.0;
        o.amax = op.amax_word >= 0 ? amax_lane(x, op.amax_word, x.cur) : nullptr;
        o.split_sc = P.run_mode && op.ps_gemm >= 0 ? sc_word(x, op.amax_word) : nullptr;
        if (planes_active(P) && op.planes_role) {
          o.planes = planes_ptr(x, x.cur, op.planes_role - 1);
          o.pstride = P.planes_n[op.planes_role - 1];
          o.amax_in = amax_lane(x, op.planes_in_amax, x.cur);
          o.sc_out = planes_sc(x, x.cur, op.planes_role - 1);
          o.amax = nullptr;
        }
      }
      TQ_TRY(sweepd_launch(P0_.dtype, L, st_));
      dense.swap(rest);
    }
    for (size_t i0 = 0; i0 < items.size(); i0 += kS2MaxOps) {
      S2Launch L;
      L.nops = (int)std::min<size_t>(kS2MaxOps, items.size() - i0);
      int blocks = 0;
      for (int q = 0; q < L.nops; ++q) {
        const Item& it = items[i0 + q];
        Inst& x = I_[it.k];
        set_lane(x, it.lane);
        const Op& op = x.P->ops[it.q];
        S2Op& o = L.op[q];
        TQ_TRY(fill_s2(x, o, op, op.stab));
        o.block_begin = blocks;
        o.nblocks = s2_blocks(op.s2_nchunks);
        blocks += o.nblocks;
      }
      TQ_TRY(sweep2_launch(P0_.dtype, L, st_));
    }
    for (size_t k = 0; k < I_.size(); ++k) set_lane(I_[k], keep[k]);
  } else if (op0.kind == OP_SWEEP && sweep_lanes_ > 1) {
    // the per-slice table sweep of every lane in one launch (grid.y = lane; SweepLanes)
    TQ_TRY(each_instance([&](Inst& x) -> int {
      const Op& op = x.P->ops[grp[0]];
      const int keep = x.cur;
      SweepLanes ls;
      ls.n = sweep_lanes_;
      for (int j = 0; j < sweep_lanes_; ++j) {
        set_lane(x, j);
        ls.X[j] = ptr(x, op.a);
        ls.Y[j] = ptr(x, op.c);
        for (size_t g = 0; g < op.sgates.size(); ++g) ls.G[j][g] = ptr(x, op.sgates[g].g);
      }
      set_lane(x, 0);
      const SweepArgs a = sweep_args(x, op, 0.0);
      set_lane(x, keep);
      return sweep_launch_lanes(x.P->dtype, a, ls, ost_ ? ost_ : st_);
    }));
  } else {
    TQ_TRY(each_instance([&](Inst& x) -> int { return launch_one(x, x.P->ops[grp[0]]); }));
  }
  if (prof) {
    TQ_HIP(hipEventRecord(ev.b, st_));
    P0_.ev_used.push_back(ev);
  }
  return TQ_OK;
}

int Exec::run(int64_t s_begin, int64_t s_end, int64_t s_step, int accumulate) {
  const int ns = (int)P0_.sliced.size();
  for (auto& x : I_) x.first = !accumulate;
  if (s_begin >= s_end) {
    for (auto& x : I_)
      if (!accumulate && x.P->out_numel) TQ_HIP(hipMemsetAsync(x.out, 0, x.P->out_numel * esz(), st_));
    return TQ_OK;
  }
  // Slices run in batches of P.lanes (slice lanes, Plan::lanes): lane j owns its own copy of the
  // per-slice arena part, the batch's sweep2 levels share launches across lanes, other ops run
  // lane by lane in lane order (so output accumulation keeps its order)
  const int64_t nlanes = std::max(1, P0_.lanes);
  std::vector<int64_t> in_off;
  for (int64_t s0 = s_begin; s0 < s_end; s0 += s_step * nlanes) {
    for (auto& x : I_) {
      const Plan& P = *x.P;
      x.lane_sl.clear();
      x.lane_in_off.clear();
      in_off.assign(P.n_inputs, 0);
      for (int64_t sl = s0; sl < s_end && (int64_t)x.lane_sl.size() < nlanes; sl += s_step) {
        // decode slice id (row-major over sliced modes) -> per-input element offsets
        std::vector<int64_t> idx(ns);
        int64_t rem = sl;
        for (int q = ns - 1; q >= 0; --q) {
          idx[q] = rem % P.sliced_ext[q];
          rem /= P.sliced_ext[q];
        }
        for (int i = 0; i < P.n_inputs; ++i) {
          int64_t o = 0;
          for (int q = 0; q < ns; ++q) o += idx[q] * P.inputs[i].slice_stride[q];
          in_off[i] = o;
        }
        x.lane_sl.push_back(sl);
        x.lane_in_off.push_back(in_off);
      }
      set_lane(x, 0);
      x.lanes_summed = false;
    }
    const int nl = (int)I_[0].lane_sl.size();
    if (s0 == s_begin) {
      // max words are zeroed by a kernel, not hipMemsetAsync: with the zeroing as a memset node
      // of the plan's captured graph, replays left the f16-split GEMM a max of 0 or one too small
      // (all-zero / all-NaN outputs; mis-ordered node or carried-over max: DESIGN.md §5)
      // one launch for the hoisted part's words and (not pre-split) the first batch's per-slice
      // words behind them
      // a live-only call (Plan::live_only: the frozen results are valid) leaves the frozen
      // producers' words as they are and starts behind the frozen schedule
      const bool live = P0_.live_only;
      for (auto& x : I_) {
        const int n = x.P->n_amax_once + (x.P->run_mode ? 0 : x.P->n_amax_slice * nl);
        const int z0 = live ? x.P->n_amax_frozen : 0;
        TQ_TRY(zero_words_launch(amax_word(x, z0), n - z0, st_));
      }
      // entries [b, e) of sched_once: chain / cooperative runs as one launch each, the rest singly
      auto entries = [&](int b, int e) -> int {
        size_t run = 0, crun = 0;
        for (int i = b; i < e;) {
          while (P0_.use_seq && run < P0_.seq_once.size() && P0_.seq_once[run].first < i) ++run;
          if (P0_.use_seq && run < P0_.seq_once.size() && P0_.seq_once[run].first == i) {
            TQ_TRY(launch_chain(i, P0_.seq_once[run].second, -1));
            i = P0_.seq_once[run].second;
            continue;
          }
          while (P0_.use_coop && crun < P0_.coop_once.size() && P0_.coop_once[crun].first < i) ++crun;
          if (P0_.use_coop && crun < P0_.coop_once.size() && P0_.coop_once[crun].first == i) {
            TQ_TRY(launch_chain(i, P0_.coop_once[crun].second, (int)crun));
            i = P0_.coop_once[crun].second;
            continue;
          }
          TQ_TRY(launch(P0_.sched_once[i]));
          ++i;
        }
        return TQ_OK;
      };
      // the end of the unit (a run, or one entry) that starts at entry i
      auto unit_end = [&](int i) {
        for (auto& r : P0_.seq_once) if (r.first == i) return r.second;
        for (auto& r : P0_.coop_once) if (r.first == i) return r.second;
        return i + 1;
      };
      if (live || P0_.full_steps.empty()) {
        TQ_TRY(entries(live ? P0_.n_sched_frozen : 0, (int)P0_.sched_once.size()));
      } else {
        // the full run of a plan with frozen ops (Plan::full_steps): both schedules, zipped
        for (auto& st : P0_.full_steps) {
          if (st.first >= 0 && st.second >= 0) {
            std::vector<int> both = P0_.sched_once[st.first];
            both.insert(both.end(), P0_.sched_once[st.second].begin(), P0_.sched_once[st.second].end());
            TQ_TRY(launch(both));
          } else {
            const int i = st.first >= 0 ? st.first : st.second;
            TQ_TRY(entries(i, unit_end(i)));
          }
        }
      }
    }
    // per-slice max words: one set per lane (pre-split mode: one set shared by the batch's
    // lanes, max-ed over all of them -- an upper bound of every lane's operand)
    for (auto& x : I_) {
      const Plan& P = *x.P;
      if (P.n_amax_slice && P.run_mode)   // scales from the previous slice's max, then max = 0
        TQ_TRY(presplit_prep_launch(amax_word(x, P.n_amax_once), sc_word(x, P.n_amax_once), P.n_amax_slice, st_));
      else if (P.n_amax_slice && s0 != s_begin)   // (the first batch's: zeroed above)
        TQ_TRY(zero_words_launch(amax_word(x, P.n_amax_once), P.n_amax_slice * nl, st_));
    }
    for (auto& grp : P0_.sched_slice) {
      const Op& op0 = P0_.ops[grp[0]];
      bool merged = op0.kind == OP_SWEEP2;
      for (int j : grp) merged = merged && !P0_.ops[j].writes_output;
      if (merged || nl == 1) {
        set_lane_all(0);
        TQ_TRY(launch(grp));
        bool sums = false;
        for (int j : grp) sums = sums || P0_.ops[j].lane_sum;
        if (merged && nl > 1 && sums)
          TQ_TRY(each_instance([&](Inst& x) -> int {
            for (int j : grp)
              if (x.P->ops[j].lane_sum) {   // a lane-merged level whose lanes an output permute sums
                TQ_TRY(lane_sum_launch(x.P->dtype, x.P->ops[j].nc, ptr(x, x.P->ops[j].c),
                                       (int64_t)(x.P->lane_stride / esz()), nl, ost_));
                x.lanes_summed = true;
              }
            return TQ_OK;
          }));
      } else if (op0.kind == OP_GEMM && op0.lane_batch) {
        set_lane_all(0);
        lane_gemm_ = nl;
        const int rc = each_instance([&](Inst& x) -> int {
          TQ_TRY(launch_one(x, x.P->ops[grp[0]]));
          if (op0.lane_sum) {
            // (the pre-split GEMM's combine has summed the lanes already)
            if (!(planes_active(*x.P) && grp[0] == x.P->planes_gemm))
              TQ_TRY(lane_sum_launch(x.P->dtype, op0.nc, ptr(x, op0.c), (int64_t)(x.P->lane_stride / esz()), nl,
                                     ost_));
            x.lanes_summed = true;
          }
          return TQ_OK;
        });
        lane_gemm_ = 1;
        TQ_TRY(rc);
      } else if (op0.lane_once && I_[0].lanes_summed) {
        set_lane_all(0);
        TQ_TRY(launch(grp));
      } else if (op0.kind == OP_SWEEP && grp.size() == 1 && !op0.writes_output && sweep_lanes_on() &&
                 nl <= kSweepMaxLanes) {
        // a per-slice table sweep whose lanes write their own copies: one launch for the batch
        set_lane_all(0);
        sweep_lanes_ = nl;
        const int rc = launch(grp);
        sweep_lanes_ = 0;
        TQ_TRY(rc);
      } else {
        for (int j = 0; j < nl; ++j) {
          set_lane_all(j);
          TQ_TRY(launch(grp));
        }
      }
    }
    for (auto& x : I_) x.first = false;
  }
  return TQ_OK;
}


}  // namespace

int plan_enqueue(Plan& P, const void* const* inputs, void* out, int64_t s_begin, int64_t s_end,
                 int64_t s_step, int accumulate, hipStream_t stream) {
  std::vector<Inst> I(1);
  I[0].P = &P;
  I[0].inputs = inputs;
  I[0].out = out;
  Exec ex(I, stream);
  return ex.run(s_begin, s_end, s_step, accumulate);
}

int group_enqueue(Plan* const* plans, int n, const void* const* const* inputs, void* const* outs, int64_t s_begin,
                  int64_t s_end, int64_t s_step, int accumulate, hipStream_t stream) {
  std::vector<Inst> I((size_t)n);
  for (int k = 0; k < n; ++k) {
    I[k].P = plans[k];
    I[k].inputs = inputs[k];
    I[k].out = outs[k];
  }
  Exec ex(I, stream);
  return ex.run(s_begin, s_end, s_step, accumulate);
}

}  // namespace tq
