// Contraction-plan compiler: the GPU-resident replacement of the reference's
// opt_einsum ContractExpression (tneq_qc/contractor/einsum_strategy.py:622-643, executed by
// ComputeBackend.execute_expression, tneq_qc/backends/backend_pytorch.py:99-105).
//
// Compile time (host, once per expression + dtype + strides):
//   * walks the SSA pairwise path, tracks which modes are still needed (mode reference counts),
//     classifies every mode of each pair (batch / contracted / free / single-side sum),
//   * marks the steps that read no sliced input (hoisted: run once per execute call, results
//     pinned), among them those that read no volatile input either (frozen: run once per binding,
//     Plan::n_sched_frozen), and the two independent subtrees of the join step (branches, own
//     arena regions),
//   * picks per step the cheapest lowering:
//       APPLY  one operand small (<= 32 x 32) and its contracted modes forming at most two runs
//              in the big operand -> one streaming pass, no transpose (tq_apply.hip); the small
//              operand is read in any layout through a gather table (no extra launch);
//              consecutive APPLY steps on one tensor form a sweep chain, flushed as ONE op: the
//              in-place sweep2 (tq_sweep2.hip), its dense form (tq_sweepd.hip) -- both laid out by
//              tq_sweep2_layout.cpp -- or the table sweep (tq_sweep.hip);
//       GEMM   TTGT: reuse any operand whose layout is already [batch][M][K] / [batch][K][M]
//              (no transpose), otherwise permute it (tq_permute.hip); operand roles and the
//              K order are chosen to minimise transposed bytes; MFMA GEMM (tq_gemm.hip); a
//              tiny-output GEMM reads both operands in place (skinny);
//   * lays intermediates out in per-branch arenas (first fit over live ranges).
// The lowered plan is then finished by tq_plan_finish.cpp (plan_finish): the slice lanes' copies
// and lane-batched GEMMs, the operand-max words (assign_amax), the launches by dependency level
// with chain launches over runs of small hoisted sweep2 levels (build_schedule), every table's
// place.  tq_plan_compile.h holds the compile-time types the three files share.
// Run time: tq_plan_exec.cpp (the launch sequence of an execute call) and tq_plan_run.cpp
// (materialize / release, the hipGraph replay of that sequence, plan_run, plan_run_group).
#include "tq_plan_internal.h"
#include "tq_sweep.h"
#include "tq_sweep2_layout.h"

#include <algorithm>
#include <array>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <map>
#include <numeric>
#include <set>
#include <sstream>

namespace tq {

// TQ_SWEEP (default 1): fused sweep chains; the one reader, also behind tq_library_query "sweep"
bool sweeps_enabled() {
  static const bool v = env_on("TQ_SWEEP");
  return v;
}

namespace {

class Arena {
 public:
  int64_t alloc(int64_t bytes) {
    bytes = std::max<int64_t>(kAlign, (bytes + kAlign - 1) / kAlign * kAlign);
    int64_t cur = 0;
    auto it = used_.begin();
    for (; it != used_.end(); ++it) {
      if (it->first - cur >= bytes) break;
      cur = it->first + it->second;
    }
    used_.insert(it, {cur, bytes});
    peak_ = std::max(peak_, cur + bytes);
    return cur;
  }
  void release(int64_t off) {
    for (auto it = used_.begin(); it != used_.end(); ++it)
      if (it->first == off) { used_.erase(it); return; }
  }
  int64_t peak() const { return peak_; }

 private:
  std::vector<std::pair<int64_t, int64_t>> used_;  // sorted by offset
  int64_t peak_ = 0;
};

std::string modes_str(const std::vector<int>& m) {
  std::ostringstream o;
  o << "(";
  for (size_t i = 0; i < m.size(); ++i) o << (i ? "," : "") << m[i];
  o << ")";
  return o.str();
}

class Compiler {
 public:
  // lanes_hint > 1: the plan will run its slices in batches of that many lanes, so a
  // slice-dependent sweep op needs only min_chunks / lanes chunks to fill the GPU
  // group_hint > 1: the plan will run in lockstep groups of that many plans (blocks as lanes,
  // plan_run_group), so every sweep op shares its launches with group_hint - 1 others
  // min_chunks > 0: the smallest chunk count of a big sweep op (else TQ_S2_MINCHUNKS / 128)
  // steady: per input, 1 = its contents stay the same between execute calls (not volatile);
  // empty: every input is volatile
  Compiler(Plan& P, int lanes_hint = 1, int group_hint = 1, int min_chunks = 0, std::vector<char> steady = {})
      : P_(P), x_{P.dtype, P.esz, ext_, lanes_hint, std::max(1, group_hint), min_chunks},
        steady_(std::move(steady)) {}

  int run(int n_inputs, const int32_t* in_ranks, const int32_t* in_modes, const int64_t* in_ext,
          const int64_t* in_strides, int out_rank, const int32_t* out_modes, int n_steps,
          const int32_t* path, int n_sliced, const int32_t* sliced) {
    P_.esz = x_.esz = dtype_size(P_.dtype);
    x_.dtype = P_.dtype;
    cplx_ = dtype_complex(P_.dtype);
    P_.n_inputs = n_inputs;
    n_inputs_ = n_inputs;
    std::set<int> sl(sliced, sliced + n_sliced);
    TQ_CHECK_ARG((int)sl.size() == n_sliced, "duplicate sliced mode");
    P_.sliced.assign(sliced, sliced + n_sliced);
    P_.sliced_ext.assign(n_sliced, 0);
    // ---- inputs
    size_t cur = 0;
    for (int i = 0; i < n_inputs; ++i) {
      TQ_CHECK_ARG(in_ranks[i] >= 0 && in_ranks[i] <= TQ_MAX_RANK, "input rank");
      InputView v;
      Live L;
      std::vector<int64_t> ext(in_ext + cur, in_ext + cur + in_ranks[i]);
      std::vector<int64_t> st;
      if (in_strides) st.assign(in_strides + cur, in_strides + cur + in_ranks[i]);
      else st = contig_strides(ext);
      v.slice_stride.assign(n_sliced, 0);
      for (int d = 0; d < in_ranks[i]; ++d) {
        const int m = in_modes[cur + d];
        TQ_CHECK_ARG(ext[d] >= 1, "input extent < 1");
        TQ_TRY(note_extent(m, ext[d]));
        for (int q = 0; q < d; ++q)
          TQ_CHECK_ARG(in_modes[cur + q] != m, "repeated mode within one input (diagonal) unsupported");
        auto it = std::find(P_.sliced.begin(), P_.sliced.end(), m);
        if (it != P_.sliced.end()) {
          const int si = (int)(it - P_.sliced.begin());
          v.slice_stride[si] = st[d];
          P_.sliced_ext[si] = ext[d];
          continue;
        }
        v.modes.push_back(m); v.ext.push_back(ext[d]); v.stride.push_back(st[d]);
      }
      cur += in_ranks[i];
      L.modes = v.modes; L.ext = v.ext; L.stride = v.stride;
      L.buf.kind = BUF_INPUT; L.buf.index = i; L.buf.off = 0;
      for (int64_t ss : v.slice_stride) L.dep |= ss != 0;
      L.vol = L.dep || !(i < (int)steady_.size() && steady_[i]);
      P_.inputs.push_back(v);
      live_.push_back(L);
    }
    for (int s = 0; s < n_sliced; ++s) {
      TQ_CHECK_ARG(P_.sliced_ext[s] > 0, "sliced mode not present in any input");
      P_.n_slices *= P_.sliced_ext[s];
    }
    // ---- output
    std::set<int> outset;
    for (int d = 0; d < out_rank; ++d) {
      const int m = out_modes[d];
      TQ_CHECK_ARG(!outset.count(m), "repeated output mode");
      TQ_CHECK_ARG(!sl.count(m), "sliced mode in output");
      TQ_CHECK_ARG(ext_.count(m), "output mode not in any input");
      outset.insert(m);
      P_.out_modes.push_back(m);
      P_.out_ext.push_back(ext_[m]);
    }
    P_.out_numel = prod(P_.out_ext);
    // reference counts: live tensors + output
    for (auto& L : live_) for (int m : L.modes) cnt_[m]++;
    for (int m : P_.out_modes) cnt_[m]++;
    // ---- pre-pass: which SSA ids depend on a sliced input, and which slice-invariant results
    // are read by slice-dependent steps (those are "pinned": kept in a region of their own that
    // no slice-dependent buffer ever reuses, since invariant ops do not re-run per slice)
    // The same one tier down: a frozen result (no sliced and no volatile input in its subtree;
    // the final step is never frozen) that a step of a later tier reads is pinned too, since a
    // live-only execute call does not run the frozen ops again.  Tiers: 0 frozen, 1 hoisted, 2 per slice
    {
      std::vector<char> tier(n_inputs + n_steps, 0);
      for (int i = 0; i < n_inputs; ++i) tier[i] = live_[i].dep ? 2 : live_[i].vol ? 1 : 0;
      pinned_.assign(n_inputs + n_steps, 0);
      std::set<int> fin;
      for (int s = 0; s < n_steps; ++s) {
        const int x = path[2 * s], y = path[2 * s + 1];
        if (x < 0 || y < 0 || x >= n_inputs + s || y >= n_inputs + s) break;  // checked below
        const int t = std::max<int>({tier[x], tier[y], s == n_steps - 1 ? 1 : 0});
        tier[n_inputs + s] = (char)t;
        if (tier[x] < t && x >= n_inputs) pinned_[x] = 1;
        if (tier[y] < t && y >= n_inputs) pinned_[y] = 1;
        if (t == 0)
          for (int z : {x, y}) if (z < n_inputs) fin.insert(z);
      }
      P_.frozen_inputs.assign(fin.begin(), fin.end());
    }
    // ---- branches: the two subtrees of the join step are independent (run concurrently, arena
    // regions of their own); the join and every step outside its subtrees are branch 2 (region
    // 0).  The join is the step whose smaller subtree holds the most inputs: the final step of a
    // plain partition path, the boundary contraction when the sweeps' tails are absorbed after
    // it (einsum.partition_path defer=...)
    step_branch_.assign(n_steps, 2);
    if (n_steps >= 1) {
      std::vector<int> leaves(n_inputs + n_steps, 1);
      int last = n_steps - 1, best = -1;
      for (int s = 0; s < n_steps; ++s) {
        const int x = path[2 * s], y = path[2 * s + 1];
        if (x < 0 || y < 0 || x >= n_inputs + s || y >= n_inputs + s) break;  // checked below
        leaves[n_inputs + s] = leaves[x] + leaves[y];
        const int m = std::min(leaves[x], leaves[y]);
        if (m >= best) { best = m; last = s; }
      }
      step_branch_[last] = 2;
      for (int side = 0; side < 2; ++side) {
        std::vector<int> stack{path[2 * last + side]};
        while (!stack.empty()) {
          const int id = stack.back();
          stack.pop_back();
          if (id < n_inputs || id - n_inputs >= last) continue;
          step_branch_[id - n_inputs] = side;
          stack.push_back(path[2 * (id - n_inputs)]);
          stack.push_back(path[2 * (id - n_inputs) + 1]);
        }
      }
    }
    // ---- steps
    std::vector<bool> used(n_inputs + n_steps, false);
    for (int s = 0; s < n_steps; ++s) {
      const int x = path[2 * s], y = path[2 * s + 1];
      const int nid = n_inputs + s;
      TQ_CHECK_ARG(x >= 0 && x < nid && y >= 0 && y < nid && x != y, "path id out of range");
      TQ_CHECK_ARG(!used[x] && !used[y], "path uses a tensor twice");
      used[x] = used[y] = true;
      Live res;
      pin_next_ = pinned_[nid];
      br_ = step_branch_[s];
      TQ_TRY(step(s, live_[x], live_[y], s == n_steps - 1, res));
      live_.push_back(res);
    }
    TQ_TRY(flush_chain(false));  // (the final step always closes a chain; kept for safety)
    int remaining = 0, last = -1;
    for (int i = 0; i < n_inputs + n_steps; ++i) if (!used[i]) { ++remaining; last = i; }
    TQ_CHECK_ARG(remaining == 1, "path does not reduce to a single tensor");
    if (n_steps == 0) {
      // single input: permute (and sum) into the output
      Live& L = live_[last];
      for (int m : L.modes)
        TQ_CHECK_ARG(outset.count(m), "single-input trace/sum is unsupported");
      TQ_TRY(emit_permute(L, P_.out_modes, {}, BufRef{BUF_OUTPUT, 0, 0}, true, -1, "copy->out"));
    }
    const int64_t apeak[2] = {arenas_[0].peak(), arenas_[1].peak()};
    const int64_t ppeak[2] = {pinned_arenas_[0].peak(), pinned_arenas_[1].peak()};
    plan_finish(P_, apeak, ppeak);
    return TQ_OK;
  }

 private:
  int note_extent(int m, int64_t e) {
    auto it = ext_.find(m);
    if (it == ext_.end()) { ext_[m] = e; return TQ_OK; }
    if (it->second != e) {
      set_error("invalid argument: mode " + std::to_string(m) + " has inconsistent extents");
      return TQ_ERR_INVALID;
    }
    return TQ_OK;
  }

  int region() const { return br_ == 1 ? 1 : 0; }
  BufRef new_buf(int64_t numel, int64_t* off_out) {
    const int64_t off = arenas_[region()].alloc(numel * (int64_t)P_.esz);
    *off_out = off;
    BufRef b;
    b.kind = BUF_ARENA;
    b.off = off / (int64_t)P_.esz;
    b.region = region();
    return b;
  }
  void release(const Live& L) {
    if (L.owned && L.buf.kind == BUF_ARENA) arenas_[L.buf.region].release(L.buf.off * (int64_t)P_.esz);
  }
  // the step result's buffer: pinned results live in the separate pinned region
  BufRef new_result_buf(int64_t numel, int64_t* off_out) {
    if (!pin_next_) return new_buf(numel, off_out);
    const int64_t off = pinned_arenas_[region()].alloc(numel * (int64_t)P_.esz);
    *off_out = off;
    BufRef b;
    b.kind = BUF_PINNED;
    b.off = off / (int64_t)P_.esz;
    b.region = region();
    return b;
  }

  // permute X into contiguous `order` (+ broadcast modes `bcast` with stride 0) at dst
  int emit_permute(const Live& X, const std::vector<int>& order, const std::map<int, int64_t>& bcast,
                   BufRef dst, bool to_output, int step, const std::string& why) {
    std::vector<int64_t> shape, sst;
    for (int m : order) {
      const int p = X.pos(m);
      if (p >= 0) { shape.push_back(X.ext[p]); sst.push_back(X.stride[p]); }
      else {
        auto it = bcast.find(m);
        if (it == bcast.end()) { set_error("internal: permute mode missing"); return TQ_ERR_INVALID; }
        shape.push_back(it->second); sst.push_back(0);
      }
    }
    PermPlan pp;
    TQ_TRY(build_perm_plan(P_.dtype, (int)shape.size(), shape.data(), sst.data(), &pp));
    Op op;
    op.kind = OP_PERMUTE;
    op.a = X.buf;
    op.c = dst;
    op.writes_output = to_output;
    op.perm = (int)P_.perms.size();
    op.step = step;
    const int64_t n = prod(shape);
    op.na = X.numel();
    op.nc = n;
    op.bytes = 2.0 * n * P_.esz;
    std::ostringstream o;
    o << "step " << step << " PERMUTE " << why << " " << modes_str(X.modes) << "->" << modes_str(order)
      << " n=" << n << " [" << perm_plan_kind(pp) << "]" << (to_output ? " ->OUT" : "");
    op.note = o.str();
    P_.perms.push_back(std::move(pp));
    P_.ops.push_back(op);
    return TQ_OK;
  }

  static bool runs_equal(const std::vector<int>& modes, const std::vector<std::vector<int>>& runs) {
    size_t k = 0;
    for (auto& r : runs)
      for (int m : r) {
        if (k >= modes.size() || modes[k] != m) return false;
        ++k;
      }
    return k == modes.size();
  }

  std::vector<int> filter(const std::vector<int>& modes, const std::set<int>& s) {
    std::vector<int> r;
    for (int m : modes) if (s.count(m)) r.push_back(m);
    return r;
  }

  int64_t ext_of(const std::vector<int>& ms) const { return tq::ext_of(x_, ms); }

  int step(int s, Live A0, Live B0, bool final, Live& res) {
    for (int m : A0.modes) cnt_[m]--;
    for (int m : B0.modes) cnt_[m]--;
    std::set<int> inA(A0.modes.begin(), A0.modes.end()), inB(B0.modes.begin(), B0.modes.end());
    std::set<int> batch, contr, freeA, freeB, sumA, sumB;
    for (int m : A0.modes) {
      const bool need = cnt_[m] > 0;
      if (inB.count(m)) (need ? batch : contr).insert(m);
      else (need ? freeA : sumA).insert(m);
    }
    for (int m : B0.modes) if (!inA.count(m)) (cnt_[m] > 0 ? freeB : sumB).insert(m);
    const bool dep = A0.dep || B0.dep;
    const bool vol = dep || A0.vol || B0.vol || final;   // (the final step is never frozen)
    const int nid = n_inputs_ + s;

    ApplyDesc d;
    const bool can_apply = apply_desc(A0, B0, batch, contr, sumA, sumB, d);
    // ---- fused sweep chains: an APPLY whose big operand is the open chain's result extends it
    if (chain_.active) {
      const bool pendA = A0.buf.kind == BUF_PENDING, pendB = B0.buf.kind == BUF_PENDING;
      bool extended = false;
      if (can_apply && (d.a_big ? pendA : pendB) && !(d.a_big ? pendB : pendA) && dep == chain_.dep &&
          vol == chain_.vol && br_ == chain_.br) {
        Chain::Gate g = make_gate(s, d, d.a_big ? B0 : A0, dep);
        chain_.gates.push_back(g);
        ChainShape sh;
        if (sweeps_enabled() && chain_shape(x_, chain_, d.order, sh)) {
          chain_.out_modes = d.order;
          chain_.id = nid;
          extended = true;
        } else {
          chain_.gates.pop_back();
        }
      }
      if (!extended) {
        TQ_TRY(flush_chain(false));
        // the flushed result now has a real buffer: refresh this step's copies
        if (A0.buf.kind == BUF_PENDING) A0 = live_[chain_.flushed_id];
        if (B0.buf.kind == BUF_PENDING) B0 = live_[chain_.flushed_id];
      } else {
        res.modes = d.order;
        for (int m : d.order) res.ext.push_back(ext_[m]);
        res.stride = contig_strides(res.ext);
        res.buf = BufRef{BUF_PENDING, nid, 0};
        res.owned = true;
        res.dep = dep;
        res.vol = vol;
        for (int m : res.modes) cnt_[m]++;
        if (final) {
          live_.push_back(res);  // flush patches live_[id]; the caller's push is replaced below
          TQ_TRY(flush_chain(true));
          res = live_.back();
          live_.pop_back();
        }
        return TQ_OK;
      }
    }
    const size_t first_op = P_.ops.size();
    if (can_apply && !final && sweeps_enabled() && A0.buf.kind != BUF_PENDING &&
        B0.buf.kind != BUF_PENDING) {
      // open a chain with this gate (emitted at flush: as APPLY if it stays a single gate)
      chain_ = Chain{};
      chain_.active = true;
      chain_.dep = dep;
      chain_.vol = vol;
      chain_.br = br_;
      chain_.X0 = d.a_big ? A0 : B0;
      chain_.release_X0 = !(dep && !chain_.X0.dep);
      chain_.gates.push_back(make_gate(s, d, d.a_big ? B0 : A0, dep));
      chain_.out_modes = d.order;
      chain_.id = nid;
      ChainShape sh;
      if (chain_shape(x_, chain_, d.order, sh)) {
        res.modes = d.order;
        for (int m : d.order) res.ext.push_back(ext_[m]);
        res.stride = contig_strides(res.ext);
        res.buf = BufRef{BUF_PENDING, nid, 0};
        res.owned = true;
        res.dep = dep;
        res.vol = vol;
        for (int m : res.modes) cnt_[m]++;
        return TQ_OK;
      }
      chain_ = Chain{};  // does not fit a sweep tile: plain APPLY below
    }
    if (can_apply) {
      TQ_TRY(emit_apply(s, d, final, A0, B0, res));
    } else {
      TQ_TRY(gemm_step(s, A0, B0, final, batch, contr, freeA, freeB, sumA, sumB, res));
    }
    for (int m : res.modes) cnt_[m]++;
    // slice-invariant hoisting: a step that reads no sliced input runs once per execute; its
    // result is pinned in the arena when a slice-dependent step consumes it
    res.dep = dep;
    res.vol = vol;
    for (size_t k = first_op; k < P_.ops.size(); ++k) {
      P_.ops[k].invariant = !res.dep;
      P_.ops[k].frozen = !vol;
      P_.ops[k].branch = br_;
    }
    if (!(res.dep && !A0.dep)) release(A0);
    if (!(res.dep && !B0.dep)) release(B0);
    return TQ_OK;
  }

  // write the step result either straight into the output (final step, matching order)
  // or into a fresh arena buffer (then permuted to the output if final).
  BufRef result_target(bool final, const std::vector<int>& order, int64_t numel, bool* direct,
                       int64_t* off) {
    *direct = final && order == P_.out_modes;
    if (*direct) { *off = -1; return BufRef{BUF_OUTPUT, 0, 0}; }
    return new_result_buf(numel, off);
  }

  // ---- APPLY lowering (ApplyDesc, tq_plan_compile.h)
  bool apply_desc(const Live& A0, const Live& B0, const std::set<int>& batch,
                  const std::set<int>& contr, const std::set<int>& sumA, const std::set<int>& sumB,
                  ApplyDesc& d) {
    if (!batch.empty() || !sumA.empty() || !sumB.empty() || contr.empty()) return false;
    d.a_big = A0.numel() >= B0.numel();
    const Live& Bg = d.a_big ? A0 : B0;
    const Live& Sm = d.a_big ? B0 : A0;
    if (Bg.buf.kind != BUF_PENDING && !Bg.contiguous()) return false;
    d.K = ext_of(std::vector<int>(contr.begin(), contr.end()));
    d.N = Sm.numel() / d.K;
    if (Sm.numel() > 1024 || d.K > 32 || d.N > 32) return false;
    std::vector<std::pair<int, int>> runs;  // (start, length)
    for (int i = 0; i < (int)Bg.modes.size(); ++i) {
      if (!contr.count(Bg.modes[i])) continue;
      if (!runs.empty() && runs.back().first + runs.back().second == i) runs.back().second++;
      else runs.push_back({i, 1});
    }
    if (runs.empty() || runs.size() > 2) return false;
    const int p1 = runs[0].first, c1 = runs[0].second;
    const int p2 = runs.size() == 2 ? runs[1].first : p1 + c1;
    const int c2 = runs.size() == 2 ? runs[1].second : 0;
    d.korder.assign(Bg.modes.begin() + p1, Bg.modes.begin() + p1 + c1);
    d.korder.insert(d.korder.end(), Bg.modes.begin() + p2, Bg.modes.begin() + p2 + c2);
    for (int m : Sm.modes) if (!contr.count(m)) d.nfree.push_back(m);
    std::vector<int> gorder = d.korder;
    gorder.insert(gorder.end(), d.nfree.begin(), d.nfree.end());
    if (!(Sm.contiguous() && Sm.modes == gorder)) {
      std::vector<int64_t> gext, gst;
      for (int m : gorder) {
        const int p = Sm.pos(m);
        gext.push_back(Sm.ext[p]);
        gst.push_back(Sm.stride[p]);
      }
      const int64_t n = prod(gext);
      d.gtab.resize(n);
      for (int64_t t = 0; t < n; ++t) {
        int64_t rem = t, off = 0;
        for (int q = (int)gext.size() - 1; q >= 0; --q) { off += (rem % gext[q]) * gst[q]; rem /= gext[q]; }
        d.gtab[t] = (int32_t)off;
      }
    }
    d.order.assign(Bg.modes.begin(), Bg.modes.begin() + p1);
    d.order.insert(d.order.end(), d.nfree.begin(), d.nfree.end());
    d.order.insert(d.order.end(), Bg.modes.begin() + p1 + c1, Bg.modes.begin() + p2);
    d.order.insert(d.order.end(), Bg.modes.begin() + p2 + c2, Bg.modes.end());
    for (int i = 0; i < p1; ++i) d.O *= Bg.ext[i];
    for (int i = p1; i < p1 + c1; ++i) d.K1 *= Bg.ext[i];
    for (int i = p1 + c1; i < p2; ++i) d.M *= Bg.ext[i];
    for (int i = p2; i < p2 + c2; ++i) d.K2 *= Bg.ext[i];
    for (size_t i = p2 + c2; i < Bg.modes.size(); ++i) d.I *= Bg.ext[i];
    return true;
  }

  int add_gtab(const std::vector<int32_t>& t) {
    if (t.empty()) return -1;
    P_.gtabs.push_back(t);
    return (int)P_.gtabs.size() - 1;
  }

  int emit_apply(int s, const ApplyDesc& d, bool final, const Live& A0, const Live& B0, Live& res) {
    const Live& Bg = d.a_big ? A0 : B0;
    const Live& Sm = d.a_big ? B0 : A0;
    const int64_t outn = d.O * d.N * d.M * d.I;
    bool direct;
    int64_t roff;
    BufRef tgt = result_target(final, d.order, outn, &direct, &roff);
    Op op;
    op.kind = OP_APPLY;
    op.a = Bg.buf;
    op.b = Sm.buf;
    op.gtab = add_gtab(d.gtab);
    op.c = tgt;
    op.writes_output = direct;
    op.O = d.O; op.K = d.K1; op.M = d.M; op.K2 = d.K2; op.N = d.N; op.I = d.I;
    op.na = d.O * d.K1 * d.M * d.K2 * d.I;
    op.nb = Sm.numel();
    op.nc = outn;
    op.step = s;
    op.flops = (double)d.O * d.M * d.I * d.K * d.N * (cplx_ ? 8.0 : 2.0);
    op.bytes = (double)(d.O * d.K * d.M * d.I + outn + d.K * d.N) * P_.esz;
    std::ostringstream o;
    o << "step " << s << " APPLY O=" << d.O << " K1=" << d.K1 << " M=" << d.M << " K2=" << d.K2
      << " I=" << d.I << " N=" << d.N << (direct ? " ->OUT" : "");
    op.note = o.str();
    P_.ops.push_back(op);
    res.modes = d.order;
    res.ext.clear();
    for (int m : d.order) res.ext.push_back(ext_[m]);
    res.stride = contig_strides(res.ext);
    res.buf = tgt;
    res.owned = !direct;
    if (final && !direct)
      TQ_TRY(emit_permute(res, P_.out_modes, {}, BufRef{BUF_OUTPUT, 0, 0}, true, s, "result->out"));
    return TQ_OK;
  }

  // ---- sweep chains (Chain / ChainShape: tq_plan_compile.h; their layouts: tq_sweep2_layout.cpp)
  Chain::Gate make_gate(int s, const ApplyDesc& d, const Live& Sm, bool dep) {
    Chain::Gate g;
    g.Sm = Sm;
    g.step = s;
    g.d = d;
    g.release = !(dep && !Sm.dep);
    return g;
  }

  // one OP_SWEEP2 op: chain c (shape sh, layout d) from src (n0 elements) into tgt (nq)
  void emit_s2(const Chain& c, const ChainShape& sh, const S2Desc& d, BufRef src, int64_t n0, BufRef tgt,
               int64_t nq, bool direct, const char* what, const S2Desc* d1 = nullptr) {
    Op op;
    op.kind = OP_SWEEP2;
    op.a = src;
    op.c = tgt;
    op.writes_output = direct;
    int step0 = c.gates.front().step;   // a re-listed chain (s2_reorder_squares): first / last path step
    op.step = step0;
    for (auto& g : c.gates) step0 = std::min(step0, g.step), op.step = std::max(op.step, g.step);
    op.tin = (int)sh.tin_n;
    op.tout = (int)sh.tout_n;
    op.ncols = d.ncols;
    op.s2_nchunks = d.nchunks;
    op.na = src.kind == BUF_TABLE ? 0 : n0;
    op.nc = nq;
    double flops = 0;
    for (size_t j = 0; j < c.gates.size(); ++j) {
      SweepGate sg;
      sg.g = c.gates[j].Sm.buf;
      sg.K = (int)c.gates[j].d.K;
      sg.N = (int)c.gates[j].d.N;
      sg.n = c.gates[j].Sm.numel();
      op.sgates.push_back(sg);
      flops += (double)d.ncols * ext_of(sh.W[j]) * sg.K * (cplx_ ? 8.0 : 2.0);
    }
    op.stab = (int)P_.stabs.size();
    P_.stabs.push_back(s2_blob(d, P_.esz));
    if (d.nchunks == 1) {
      op.stab1 = op.stab;
    } else if (d1) {
      op.stab1 = (int)P_.stabs.size();
      P_.stabs.push_back(s2_blob(*d1, P_.esz));
    }
    op.flops = flops;
    op.bytes = (double)(n0 + nq) * P_.esz;
    std::ostringstream o;
    o << "step " << step0 << ".." << op.step << " SWEEP2 " << what << "gates=" << c.gates.size()
      << " tin=" << op.tin << " tout=" << op.tout << " cols=" << op.ncols << " C=" << (1 << d.logC)
      << " chunks=" << d.nchunks << (direct ? " ->OUT" : "") << " KxN=";
    for (int j = 0; j < d.ngates; ++j) o << (j ? "," : "") << d.gate[j].K << "x" << d.gate[j].N;
    o << " passes=" << d.npass;
    {
      int nl = 0;
      for (int q = 0; q < d.npass; ++q) nl += (d.k.pmeta[q][kS2PmB] & kS2PmLanes) != 0;
      if (nl) o << " lanes=" << nl;
    }
    if (d.epi) o << " epi";
    {
      char b[48];
      snprintf(b, sizeof b, " ldsx=%.2f->%.2f syncs=%d/%d", d.lds_model[0], d.lds_model[1], d.nsync, d.npass);
      o << b;
    }
    op.note = o.str();
    P_.ops.push_back(op);
  }

  int flush_chain(bool final) {
    if (!chain_.active) return TQ_OK;
    Chain c = chain_;
    chain_ = Chain{};
    chain_.flushed_id = c.id;
    const size_t first_op = P_.ops.size();
    Live res;
    const bool saved_pin = pin_next_;
    const int saved_br = br_;
    pin_next_ = pinned_[c.id];
    br_ = c.br;
    ChainShape sh0;
    const bool shape_ok = chain_shape(x_, c, c.out_modes, sh0);
    if (c.gates.size() == 1 && !(shape_ok && sh0.s2)) {
      const auto& g = c.gates[0];
      const Live& A0 = g.d.a_big ? c.X0 : g.Sm;
      const Live& B0 = g.d.a_big ? g.Sm : c.X0;
      TQ_TRY(emit_apply(g.step, g.d, final, A0, B0, res));
    } else if (shape_ok && sh0.s2) {
      const int64_t n0 = c.X0.numel();
      const int64_t nq = n0 / sh0.tin_n * sh0.tout_n;
      S2Dense dd;
      const bool dense = s2_dense_layout(x_, c, sh0, c.out_modes, &dd);
      // dense: the chain composed on the identity first (a tiny sweep2 op into an arena matrix)
      int64_t moff = -1;
      BufRef mbuf;
      if (dense) {
        const int vm = 1 << 30;   // a column mode of its own: the basis vector index
        ext_[vm] = sh0.tin_n;
        Chain c2 = c;
        c2.X0 = Live{};
        c2.X0.modes = sh0.tin;
        c2.X0.modes.push_back(vm);
        for (int m : c2.X0.modes) c2.X0.ext.push_back(ext_[m]);
        c2.X0.stride = contig_strides(c2.X0.ext);
        std::vector<char> ident((size_t)(sh0.tin_n * sh0.tin_n) * P_.esz, 0);
        for (int64_t k = 0; k < sh0.tin_n; ++k) {
          const float one = 1.0f;
          std::memcpy(ident.data() + (size_t)(k * sh0.tin_n + k) * P_.esz, &one, sizeof(float));
        }
        c2.X0.buf = BufRef{BUF_TABLE, (int64_t)P_.stabs.size(), 0, 0};
        P_.stabs.push_back(std::move(ident));
        std::vector<int> out2 = sh0.tout;
        out2.push_back(vm);
        ChainShape sh2;
        S2Desc d2;
        if (!chain_shape(x_, c2, out2, sh2) || !sh2.s2 || !s2_layout(x_, c2, sh2, out2, &d2)) {
          ext_.erase(vm);
          set_error("internal: sweep2 compose layout");
          return TQ_ERR_INVALID;
        }
        ext_.erase(vm);
        mbuf = new_buf(sh0.tin_n * sh0.tout_n, &moff);
        emit_s2(c2, sh2, d2, c2.X0.buf, sh0.tin_n * sh0.tin_n, mbuf, sh0.tin_n * sh0.tout_n, false, "compose ");
      }
      bool direct;
      int64_t roff;
      BufRef tgt = result_target(final, c.out_modes, nq, &direct, &roff);
      if (dense) {
        Op op;
        op.kind = OP_SWEEP2;
        op.s2_dense = true;
        op.a = c.X0.buf;
        op.b = mbuf;
        op.c = tgt;
        op.writes_output = direct;
        op.step = c.gates.back().step;
        op.tin = (int)sh0.tin_n;
        op.tout = (int)sh0.tout_n;
        op.ncols = dd.ncols;
        op.na = n0;
        op.nb = sh0.tin_n * sh0.tout_n;
        op.nc = nq;
        std::vector<char> blob(sizeof(S2Dense));
        std::memcpy(blob.data(), &dd, sizeof(S2Dense));
        op.stab = (int)P_.stabs.size();
        P_.stabs.push_back(std::move(blob));
        op.flops = (double)nq * sh0.tin_n * 8.0;
        op.bytes = (double)(n0 + nq) * P_.esz;
        std::ostringstream o;
        o << "step " << c.gates.front().step << ".." << op.step << " SWEEP2 DENSE gates=" << c.gates.size()
          << " tin=" << op.tin << " tout=" << op.tout << " cols=" << op.ncols << (direct ? " ->OUT" : "");
        op.note = o.str();
        P_.ops.push_back(op);
        arenas_[region()].release(moff);
      } else {
        S2Desc d;
        if (!s2_layout(x_, c, sh0, c.out_modes, &d)) { set_error("internal: sweep2 layout"); return TQ_ERR_INVALID; }
        // the square gates re-listed into fuller register blocks, when that saves passes
        Chain cr;
        if (s2_reorder_on() && d.npass > 1 && s2_reorder_squares(x_, c, cr, 4)) {
          ChainShape shr;
          S2Desc dr;
          if (chain_shape(x_, cr, cr.out_modes, shr) && shr.s2 && shr.tin_n == sh0.tin_n && shr.tout_n == sh0.tout_n &&
              s2_layout(x_, cr, shr, cr.out_modes, &dr) && dr.npass < d.npass) {
            c = cr;
            sh0 = shr;
            d = dr;
          }
        }
        // a small tensor split into chunks for parallelism: also its one-chunk form, which a
        // chain launch (one workgroup running consecutive dependent ops) uses
        S2Desc d1;
        bool has1 = false;
        if (d.nchunks > 1 && d.nchunks <= s2_seq_max_chunks() &&
            (d.ncols * (int64_t)sh0.tout_n) <= (int64_t(1) << s2_chunk_bits((int)P_.esz))) {
          has1 = s2_layout(x_, c, sh0, c.out_modes, &d1, true) && d1.nchunks == 1;
        }
        emit_s2(c, sh0, d, c.X0.buf, n0, tgt, nq, direct, "", has1 ? &d1 : nullptr);
      }
      res.modes = c.out_modes;
      for (int m : c.out_modes) res.ext.push_back(ext_[m]);
      res.stride = contig_strides(res.ext);
      res.buf = tgt;
      res.owned = !direct;
      if (final && !direct)
        TQ_TRY(emit_permute(res, P_.out_modes, {}, BufRef{BUF_OUTPUT, 0, 0}, true, c.gates.back().step,
                            "result->out"));
    } else {
      ChainShape sh = sh0;
      if (!shape_ok) { set_error("internal: chain shape"); return TQ_ERR_INVALID; }
      const int64_t n0 = c.X0.numel();
      const int64_t nq = n0 / sh.tin_n * sh.tout_n;
      bool direct;
      int64_t roff;
      BufRef tgt = result_target(final, c.out_modes, nq, &direct, &roff);
      Op op;
      op.kind = OP_SWEEP;
      op.a = c.X0.buf;
      op.c = tgt;
      op.writes_output = direct;
      op.step = c.gates.back().step;
      op.tin = (int)sh.tin_n;
      op.tout = (int)sh.tout_n;
      op.ncols = n0 / sh.tin_n;
      // strides of X0 (contiguous, its own order) and of Y (contiguous, out order)
      std::map<int, int64_t> sx, sy;
      chain_strides(x_, c, c.out_modes, sx, sy);
      // outer runs (merge neighbours contiguous in both X and Y), innermost first
      std::vector<std::array<int64_t, 3>> runs;  // ext, in stride, out stride (outer->inner)
      for (int m : sh.outer) {
        const int64_t e = ext_[m];
        if (e == 1) continue;
        if (!runs.empty() && runs.back()[1] == sx[m] * e && runs.back()[2] == sy[m] * e) {
          runs.back()[0] *= e;
          runs.back()[1] = sx[m];
          runs.back()[2] = sy[m];
        } else {
          runs.push_back({e, sx[m], sy[m]});
        }
      }
      if (runs.size() > (size_t)kSweepMaxRuns) { set_error("internal: sweep runs"); return TQ_ERR_INVALID; }
      std::reverse(runs.begin(), runs.end());
      op.nruns = (int)runs.size();
      for (size_t r = 0; r < runs.size(); ++r) {
        op.run_ext[r] = runs[r][0]; op.run_in[r] = runs[r][1]; op.run_out[r] = runs[r][2];
      }
      // tables: tin_off (int64) | tout_off (int64) | per gate [W][K+1] int16
      std::vector<char> blob;
      auto put64 = [&](int64_t v) { const char* p = (const char*)&v; blob.insert(blob.end(), p, p + 8); };
      std::map<int, int64_t> dig;
      for (int64_t t = 0; t < sh.tin_n; ++t) {
        digits(x_, t, sh.tin, dig);
        int64_t o = 0;
        for (int m : sh.tin) o += dig[m] * sx[m];
        put64(o);
      }
      op.tout_off_at = blob.size();
      for (int64_t t = 0; t < sh.tout_n; ++t) {
        digits(x_, t, sh.tout, dig);
        int64_t o = 0;
        for (int m : sh.tout) o += dig[m] * sy[m];
        put64(o);
      }
      std::vector<int> prev = sh.tin;
      double flops = 0;
      op.tabs_at = blob.size();
      size_t entries = 0;
      for (size_t j = 0; j < c.gates.size(); ++j) {
        const auto& g = c.gates[j];
        const std::vector<int>& w = sh.W[j];
        SweepGate sg;
        sg.g = g.Sm.buf;
        sg.gtab = add_gtab(g.d.gtab);
        sg.K = (int)g.d.K;
        sg.N = (int)g.d.N;
        sg.n = g.Sm.numel();
        sg.W = (int)ext_of(w);
        sg.tab_off = entries;
        for (int64_t e = 0; e < sg.W; ++e) {
          std::map<int, int64_t> de;
          digits(x_, e, w, de);
          std::map<int, int64_t> dn;
          for (int m : g.d.nfree) dn[m] = de[m];
          const int64_t n = index_of(x_, g.d.nfree, dn);
          for (int64_t k = 0; k < sg.K; ++k) {
            std::map<int, int64_t> dk = de;
            std::map<int, int64_t> kd;
            digits(x_, k, g.d.korder, kd);
            for (auto& kv : kd) dk[kv.first] = kv.second;
            const int32_t v = (int32_t)index_of(x_, prev, dk);
            blob.insert(blob.end(), (const char*)&v, (const char*)&v + 4);
          }
          const int32_t nv = (int32_t)n;
          blob.insert(blob.end(), (const char*)&nv, (const char*)&nv + 4);
          entries += sg.K + 1;
        }
        flops += (double)op.ncols * sg.W * sg.K * (cplx_ ? 8.0 : 2.0);
        op.sgates.push_back(sg);
        prev = w;
      }
      op.tab_len = (int)entries;
      op.stab = (int)P_.stabs.size();
      P_.stabs.push_back(std::move(blob));
      // coalescing: walk columns fastest when the innermost outer run is unit-stride
      op.load_colfast = (op.nruns > 0 && op.run_in[0] == 1 && op.run_ext[0] >= 16) ? 1 : 0;
      op.store_colfast = (op.nruns > 0 && op.run_out[0] == 1 && op.run_ext[0] >= 16) ? 1 : 0;
      op.flops = flops;
      op.bytes = (double)(n0 + nq) * P_.esz;
      op.na = n0;
      op.nc = nq;
      std::ostringstream o;
      o << "step " << c.gates.front().step << ".." << op.step << " SWEEP gates=" << c.gates.size()
        << " tin=" << op.tin << " tout=" << op.tout << " cols=" << op.ncols << " runs=" << op.nruns
        << (direct ? " ->OUT" : "");
      op.note = o.str();
      P_.ops.push_back(op);
      res.modes = c.out_modes;
      for (int m : c.out_modes) res.ext.push_back(ext_[m]);
      res.stride = contig_strides(res.ext);
      res.buf = tgt;
      res.owned = !direct;
      if (final && !direct)
        TQ_TRY(emit_permute(res, P_.out_modes, {}, BufRef{BUF_OUTPUT, 0, 0}, true, op.step, "result->out"));
    }
    for (size_t k = first_op; k < P_.ops.size(); ++k) {
      P_.ops[k].invariant = !c.dep;
      P_.ops[k].frozen = !c.vol;
      P_.ops[k].branch = c.br;
    }
    res.dep = c.dep;
    res.vol = c.vol;
    // the pending result gets its real buffer
    Live& L = live_[c.id];
    L.buf = res.buf;
    L.owned = res.owned;
    L.modes = res.modes;
    L.ext = res.ext;
    L.stride = res.stride;
    L.dep = c.dep;
    L.vol = c.vol;
    // operands are released only now, after the result buffer was placed
    if (c.release_X0) release(c.X0);
    for (auto& g : c.gates) if (g.release) release(g.Sm);
    pin_next_ = saved_pin;
    br_ = saved_br;
    return TQ_OK;
  }

  // A GEMM step whose output is tiny (M * N <= 16, no batch modes, no single-side sums) and whose
  // operands would need a permute: one strided skinny op reads both in place (bit weights from the
  // operands' own strides; every M / N / K mode a power of two).  true: emitted (*rc its status)
  bool skinny_step(int s, const Live* A, const Live* B, const std::set<int>& sA, const std::set<int>& sB,
                   const std::vector<int>& bord, const std::vector<int>& mord, const std::vector<int>& nord,
                   const std::vector<int>& kord, bool final, Live& res, int* rc) {
    if (!skinny_strided_enabled() || !bord.empty() || !sA.empty() || !sB.empty()) return false;
    const int64_t M = ext_of(mord), N = ext_of(nord), K = ext_of(kord);
    auto p2 = [](int64_t v) { return v >= 1 && (v & (v - 1)) == 0; };
    if (!p2(M) || !p2(N) || M * N > 16 || !p2(K) || K < 256 || K > (int64_t(1) << kSkMaxKBits)) return false;
    for (const auto* ord : {&mord, &nord, &kord})
      for (int m : *ord) if (!p2(ext_[m])) return false;
    if (A->buf.kind == BUF_PENDING || B->buf.kind == BUF_PENDING) return false;
    // bit weights, least significant bit first (row-major index: the last mode is fastest)
    auto weights = [&](const Live& X, const std::vector<int>& ord, int64_t* w, int cap) {
      int nb = 0;
      for (auto it = ord.rbegin(); it != ord.rend(); ++it) {
        const int pos = X.pos(*it);
        int e = 0;
        while ((int64_t(1) << e) < ext_[*it]) ++e;
        for (int b = 0; b < e; ++b) {
          if (nb >= cap) return -1;
          w[nb++] = X.stride[pos] << b;
        }
      }
      return nb;
    };
    SkinnyArgs sk;
    sk.K = K;
    sk.M = (int)M;
    sk.N = (int)N;
    if (weights(*A, mord, sk.wam, 4) < 0 || weights(*B, nord, sk.wbn, 4) < 0) return false;
    const int nka = weights(*A, kord, sk.wak, kSkMaxKBits), nkb = weights(*B, kord, sk.wbk, kSkMaxKBits);
    if (nka < 0 || nkb < 0 || nka != nkb) return false;
    sk.nkb = nka;
    std::vector<int> rord = mord;
    rord.insert(rord.end(), nord.begin(), nord.end());
    bool direct;
    int64_t roff;
    BufRef tgt = result_target(final, rord, M * N, &direct, &roff);
    Op op;
    op.kind = OP_GEMM;
    op.skinny = true;
    op.sk = sk;
    op.a = A->buf; op.b = B->buf; op.c = tgt;
    op.writes_output = direct;
    op.M = M; op.N = N; op.K = K; op.batch = 1;
    const int P = skinny_blocks(K);
    op.ws_bytes = P > 1 ? (size_t)P * M * N * P_.esz : 0;
    op.na = A->numel();
    op.nb = B->numel();
    op.nc = M * N;
    op.nws = (int64_t)((op.ws_bytes + P_.esz - 1) / P_.esz);
    int64_t wsoff = -1;
    if (op.ws_bytes) {
      wsoff = arenas_[region()].alloc((int64_t)op.ws_bytes);
      op.ws = BufRef{BUF_ARENA, 0, wsoff / (int64_t)P_.esz, region()};
    }
    op.step = s;
    op.flops = (double)M * N * K * (cplx_ ? 8.0 : 2.0);
    op.bytes = (double)(M * K + K * N + M * N) * P_.esz;
    std::ostringstream o;
    o << "step " << s << " SKINNY M=" << M << " N=" << N << " K=" << K << " (strided, no permutes)"
      << (direct ? " ->OUT" : "");
    op.note = o.str();
    P_.ops.push_back(op);
    if (wsoff >= 0) arenas_[region()].release(wsoff);
    res.modes = rord;
    res.ext.clear();
    for (int m : rord) res.ext.push_back(ext_[m]);
    res.stride = contig_strides(res.ext);
    res.buf = tgt;
    res.owned = !direct;
    *rc = TQ_OK;
    if (final && !direct)
      *rc = emit_permute(res, P_.out_modes, {}, BufRef{BUF_OUTPUT, 0, 0}, true, s, "result->out");
    return true;
  }

  struct GemmChoice {
    bool swap = false;          // roles: A = second operand
    int korder_from = 0;        // 0: A's order, 1: B's order
    double cost = 1e300;
  };

  int gemm_step(int s, const Live& X, const Live& Y, bool final, const std::set<int>& batch,
                const std::set<int>& contr, const std::set<int>& freeX, const std::set<int>& freeY,
                const std::set<int>& sumX, const std::set<int>& sumY, Live& res) {
    // Evaluate role assignments and the source of the (batch, K) order.
    struct Cand {
      const Live* A; const Live* B;
      std::set<int> fA, fB, sA, sB;
      std::vector<int> bord, kord, mord, nord;
      bool a_ok = false, b_ok = false; int ta = 0, tb = 0;
      double cost = 0;
    };
    std::vector<Cand> cands;
    for (int swap = 0; swap < 2; ++swap)
      for (int from = 0; from < 2; ++from) {
        Cand c;
        c.A = swap ? &Y : &X; c.B = swap ? &X : &Y;
        c.fA = swap ? freeY : freeX; c.fB = swap ? freeX : freeY;
        c.sA = swap ? sumY : sumX; c.sB = swap ? sumX : sumY;
        std::set<int> kset = contr;
        kset.insert(c.sA.begin(), c.sA.end());
        kset.insert(c.sB.begin(), c.sB.end());
        const Live& src = from == 0 ? *c.A : *c.B;
        c.bord = filter(src.modes, batch);
        c.kord = filter(src.modes, kset);
        // sum modes absent from src go last in K
        for (int m : (from == 0 ? c.sB : c.sA)) c.kord.push_back(m);
        c.mord = filter(c.A->modes, c.fA);
        c.nord = filter(c.B->modes, c.fB);
        // A layouts: [b][M][K] (ta=0) or [b][K][M] (ta=1)
        if (c.A->contiguous() && c.sB.empty()) {
          if (runs_equal(c.A->modes, {c.bord, c.mord, c.kord})) { c.a_ok = true; c.ta = 0; }
          else if (runs_equal(c.A->modes, {c.bord, c.kord, c.mord})) { c.a_ok = true; c.ta = 1; }
        }
        if (c.B->contiguous() && c.sA.empty()) {
          if (runs_equal(c.B->modes, {c.bord, c.kord, c.nord})) { c.b_ok = true; c.tb = 0; }
          else if (runs_equal(c.B->modes, {c.bord, c.nord, c.kord})) { c.b_ok = true; c.tb = 1; }
        }
        const int64_t bsz = ext_of(c.bord), msz = ext_of(c.mord), nsz = ext_of(c.nord),
                      ksz = ext_of(c.kord);
        if (!c.a_ok) c.cost += 2.0 * bsz * msz * ksz;
        if (!c.b_ok) c.cost += 2.0 * bsz * ksz * nsz;
        std::vector<int> rord = c.bord;
        rord.insert(rord.end(), c.mord.begin(), c.mord.end());
        rord.insert(rord.end(), c.nord.begin(), c.nord.end());
        if (final && rord != P_.out_modes) c.cost += 2.0 * bsz * msz * nsz;
        // mild preference for the larger operand as A with M >= N (taller tiles)
        c.cost += 1e-3 * (double)(swap);
        cands.push_back(c);
      }
    auto best = std::min_element(cands.begin(), cands.end(),
                                 [](const Cand& a, const Cand& b) { return a.cost < b.cost; });
    Cand c = *best;
    const int64_t bsz = ext_of(c.bord), M = ext_of(c.mord), N = ext_of(c.nord),
                  K = ext_of(c.kord);
    if (!(c.a_ok && c.b_ok)) {
      int rc = 0;
      if (skinny_step(s, c.A, c.B, c.sA, c.sB, c.bord, c.mord, c.nord, c.kord, final, res, &rc)) return rc;
    }
    // materialise operands
    BufRef abuf = c.A->buf, bbuf = c.B->buf;
    int64_t aoff = -1, boff = -1;
    if (!c.a_ok) {
      std::vector<int> ord = c.bord;
      ord.insert(ord.end(), c.mord.begin(), c.mord.end());
      ord.insert(ord.end(), c.kord.begin(), c.kord.end());
      std::map<int, int64_t> bc;
      for (int m : c.sB) bc[m] = ext_[m];
      abuf = new_buf(bsz * M * K, &aoff);
      TQ_TRY(emit_permute(*c.A, ord, bc, abuf, false, s, "A->[b][M][K]"));
      c.ta = 0;
    }
    if (!c.b_ok) {
      std::vector<int> ord = c.bord;
      ord.insert(ord.end(), c.kord.begin(), c.kord.end());
      ord.insert(ord.end(), c.nord.begin(), c.nord.end());
      std::map<int, int64_t> bc;
      for (int m : c.sA) bc[m] = ext_[m];
      bbuf = new_buf(bsz * K * N, &boff);
      TQ_TRY(emit_permute(*c.B, ord, bc, bbuf, false, s, "B->[b][K][N]"));
      c.tb = 0;
    }
    std::vector<int> rord = c.bord;
    rord.insert(rord.end(), c.mord.begin(), c.mord.end());
    rord.insert(rord.end(), c.nord.begin(), c.nord.end());
    bool direct;
    int64_t roff;
    BufRef tgt = result_target(final, rord, bsz * M * N, &direct, &roff);
    Op op;
    op.kind = OP_GEMM;
    op.a = abuf; op.b = bbuf; op.c = tgt;
    op.writes_output = direct;
    op.transA = c.ta; op.transB = c.tb;
    op.M = M; op.N = N; op.K = K; op.batch = bsz;
    op.lda = c.ta ? M : K; op.sA = M * K;
    op.ldb = c.tb ? K : N; op.sB = K * N;
    op.ldc = N; op.sC = M * N;
    op.ws_bytes = gemm_workspace(P_.dtype, M, N, K, bsz);
    op.na = bsz * M * K;
    op.nb = bsz * K * N;
    op.nc = bsz * M * N;
    op.nws = (int64_t)((op.ws_bytes + P_.esz - 1) / P_.esz);
    int64_t wsoff = -1;
    if (op.ws_bytes) {
      wsoff = arenas_[region()].alloc((int64_t)op.ws_bytes);
      op.ws = BufRef{BUF_ARENA, 0, wsoff / (int64_t)P_.esz, region()};
    }
    op.step = s;
    op.flops = (double)bsz * M * N * K * (cplx_ ? 8.0 : 2.0);
    op.bytes = (double)bsz * (M * K + K * N + M * N) * P_.esz;
    std::ostringstream o;
    o << "step " << s << " GEMM b=" << bsz << " M=" << M << " N=" << N << " K=" << K
      << " tA=" << c.ta << " tB=" << c.tb << (c.a_ok ? "" : " permA") << (c.b_ok ? "" : " permB")
      << (direct ? " ->OUT" : "");
    op.note = o.str();
    P_.ops.push_back(op);
    if (wsoff >= 0) arenas_[region()].release(wsoff);
    if (aoff >= 0) arenas_[region()].release(aoff);
    if (boff >= 0) arenas_[region()].release(boff);
    res.modes = rord;
    for (int m : rord) res.ext.push_back(ext_[m]);
    res.stride = contig_strides(res.ext);
    res.buf = tgt;
    res.owned = !direct;
    if (final && !direct)
      TQ_TRY(emit_permute(res, P_.out_modes, {}, BufRef{BUF_OUTPUT, 0, 0}, true, s, "result->out"));
    return TQ_OK;
  }

  Plan& P_;
  std::map<int, int64_t> ext_;
  S2Ctx x_;                  // what the sweep-chain layouts read (tq_sweep2_layout.h): dtype, the
                             // hints, and ext_ by reference
  std::vector<char> steady_;
  bool cplx_ = false;
  int n_inputs_ = 0;
  Chain chain_;
  std::vector<Live> live_;
  std::map<int, int> cnt_;
  Arena arenas_[2];          // per branch, so the two subtrees can run concurrently
  Arena pinned_arenas_[2];
  int br_ = 0;               // branch of the step being compiled (0, 1, 2 = join)
  std::vector<int> step_branch_;
  std::vector<char> pinned_;
  bool pin_next_ = false;
};

}  // namespace

int plan_compile(Plan& P, int dtype, int n_inputs, const int32_t* in_ranks, const int32_t* in_modes,
                 const int64_t* in_extents, const int64_t* in_strides, int out_rank,
                 const int32_t* out_modes, int n_steps, const int32_t* path, int n_sliced,
                 const int32_t* sliced_modes, int group_hint, int min_chunks, int n_volatile,
                 const int32_t* volatile_ids) {
  TQ_CHECK_ARG(dtype_valid(dtype), "dtype");
  TQ_CHECK_ARG(group_hint >= 1, "group_hint");
  TQ_CHECK_ARG(min_chunks >= 0, "min_chunks");
  TQ_CHECK_ARG(n_inputs >= 1, "need at least one input");
  TQ_CHECK_ARG(n_steps == n_inputs - 1, "a pairwise path has n_inputs - 1 steps");
  TQ_CHECK_ARG(out_rank >= 0 && out_rank <= TQ_MAX_RANK, "output rank");
  TQ_CHECK_ARG(n_sliced >= 0 && n_sliced <= 62, "n_sliced");
  // declared volatile inputs: every other input is steady (n_volatile < 0: none is)
  std::vector<char> steady;
  if (n_volatile >= 0) {
    TQ_CHECK_ARG(n_volatile == 0 || volatile_ids != nullptr, "null volatile input list");
    steady.assign(n_inputs, 1);
    for (int q = 0; q < n_volatile; ++q) {
      TQ_CHECK_ARG(volatile_ids[q] >= 0 && volatile_ids[q] < n_inputs, "volatile input id out of range");
      steady[volatile_ids[q]] = 0;
    }
  }
  P = Plan{};
  P.dtype = dtype;
  Compiler c(P, 1, group_hint, min_chunks, steady);
  TQ_TRY(c.run(n_inputs, in_ranks, in_modes, in_extents, in_strides, out_rank, out_modes, n_steps,
               path, n_sliced, sliced_modes));
  if (P.lanes > 1) {
    // slice lanes: compile again with wider chunks for the slice-dependent sweeps (the lanes of
    // a batch share their launches); kept if the second plan runs with the same lanes
    Plan Q{};
    Q.dtype = dtype;
    Compiler c2(Q, P.lanes, group_hint, min_chunks, steady);
    if (c2.run(n_inputs, in_ranks, in_modes, in_extents, in_strides, out_rank, out_modes, n_steps,
               path, n_sliced, sliced_modes) == TQ_OK && Q.lanes == P.lanes)
      P = std::move(Q);
  }
  plan_planes_layout(P);   // sizes known at compile time (queries, CPU tests); allocated at materialize
  // the compile arguments, kept for a recompile with another group hint (plan_recompile)
  CompileArgs& a = P.args;
  int nm = 0;
  for (int i = 0; i < n_inputs; ++i) nm += in_ranks[i];
  a.in_ranks.assign(in_ranks, in_ranks + n_inputs);
  a.in_modes.assign(in_modes, in_modes + nm);
  a.in_extents.assign(in_extents, in_extents + nm);
  a.in_strides.clear();
  if (in_strides) a.in_strides.assign(in_strides, in_strides + nm);
  a.out_modes.assign(out_modes, out_modes + out_rank);
  a.path.assign(path, path + 2 * n_steps);
  a.sliced.assign(sliced_modes, sliced_modes + n_sliced);
  a.declared = n_volatile >= 0;
  a.volatile_ids.clear();
  if (n_volatile > 0) a.volatile_ids.assign(volatile_ids, volatile_ids + n_volatile);
  P.group_hint = group_hint;
  P.min_chunks = min_chunks;
  static const bool prog_default = env_on("TQ_S2_PROG");   // TQ_S2_PROG=0: every block pass on the interpreter
  plan_s2_programs(P, prog_default);
  P.use_fold = fold_slices_enabled();
  if (n_sliced > 0) {
    // the whole program: the same network and path with no sliced modes (Plan::whole).  Eligible
    // by cost only: nothing it needs may exceed the sliced program's, and the sliced program's
    // per-slice part holds no GEMM (folding a sliced leg into a GEMM's K changes its f16-split
    // rounding, which the parity bounds pin)
    auto W = std::make_shared<Plan>();
    if (plan_compile(*W, dtype, n_inputs, in_ranks, in_modes, in_extents, in_strides, out_rank, out_modes,
                     n_steps, path, 0, nullptr, group_hint, min_chunks, n_volatile, volatile_ids) == TQ_OK) {
      bool slice_gemm = false;
      for (const Op& op : P.ops) slice_gemm = slice_gemm || (op.kind == OP_GEMM && !op.invariant);
      P.fold_ok = !slice_gemm && W->bytes <= P.bytes && W->flops <= P.flops && W->arena_bytes <= P.arena_bytes;
      P.whole = std::move(W);
    }
  }
  return TQ_OK;
}

namespace {
int recompile(Plan& P, const CompileArgs& a, int group_hint, int min_chunks);
}

int plan_recompile(Plan& P, int group_hint, int min_chunks) {
  TQ_CHECK_ARG(P.d_arena == nullptr && P.d_tables == nullptr, "a plan is recompiled before its first execute only");
  TQ_CHECK_ARG(!P.args.in_ranks.empty(), "plan has no compile arguments");
  if (group_hint == P.group_hint && min_chunks == P.min_chunks) return TQ_OK;
  return recompile(P, P.args, group_hint, min_chunks);
}

int plan_set_volatile(Plan& P, int n, const int32_t* ids) {
  TQ_CHECK_ARG(!P.resident && !(P.whole && P.whole->resident) && P.d_arena == nullptr && P.d_tables == nullptr,
               "volatile inputs are declared before the plan's first execute only");
  TQ_CHECK_ARG(!P.args.in_ranks.empty(), "plan has no compile arguments");
  TQ_CHECK_ARG(n <= 0 || ids != nullptr, "null volatile input list");
  CompileArgs a = P.args;
  a.declared = n >= 0;
  a.volatile_ids.clear();
  if (n > 0) a.volatile_ids.assign(ids, ids + n);
  std::sort(a.volatile_ids.begin(), a.volatile_ids.end());
  a.volatile_ids.erase(std::unique(a.volatile_ids.begin(), a.volatile_ids.end()), a.volatile_ids.end());
  if (a.declared == P.args.declared && a.volatile_ids == P.args.volatile_ids) return TQ_OK;
  return recompile(P, a, P.group_hint, P.min_chunks);
}

void plan_frozen_invalidate(Plan& P) {
  P.frozen_valid = false;
  if (P.whole) P.whole->frozen_valid = false;
}

namespace {
// compile P again from arguments `a0`, keeping its per-plan options
int recompile(Plan& P, const CompileArgs& a0, int group_hint, int min_chunks) {
  const CompileArgs a = a0;
  const bool seq = P.use_seq, coop = P.use_coop, planes = P.use_planes, graph = P.use_graph;
  const bool prog = P.use_s2_prog, fold = P.use_fold;
  Plan Q;
  TQ_TRY(plan_compile(Q, P.dtype, (int)a.in_ranks.size(), a.in_ranks.data(), a.in_modes.data(),
                      a.in_extents.data(), a.in_strides.empty() ? nullptr : a.in_strides.data(),
                      (int)a.out_modes.size(), a.out_modes.data(), (int)a.path.size() / 2, a.path.data(),
                      (int)a.sliced.size(), a.sliced.data(), group_hint, min_chunks,
                      a.declared ? (int)a.volatile_ids.size() : -1, a.volatile_ids.data()));
  Q.use_seq = seq;
  Q.use_coop = coop;
  Q.use_planes = planes;
  Q.use_graph = graph;
  Q.use_fold = fold;
  plan_s2_programs(Q, prog);
  P = std::move(Q);
  return TQ_OK;
}
}  // namespace

void plan_clone_compiled(const Plan& src, Plan& dst) {
  dst = src;
  dst.d_arena = dst.d_tables = dst.d_planes = nullptr;
  dst.owns_device = false;
  dst.device = -1;
  dst.serial = 0;
  dst.h_bad = nullptr;
  dst.profile = 0;
  dst.ev_used.clear();
  dst.ev_free.clear();
  dst.graphs.clear();
  dst.graph_clock = 0;
  dst.cap_stream = nullptr;
  dst.side_streams.clear();
  dst.side_events.clear();
  dst.graph_builds = dst.graph_launches = 0;
  dst.ps_fallbacks = 0;
  dst.run_mode = 0;
  dst.resident = dst.fold_failed = false;
  dst.folded_executes = 0;
  dst.frozen_valid = dst.live_only = false;
  dst.frozen_ptrs.clear();
  dst.frozen_ev = nullptr;
  dst.frozen_stream = nullptr;
  dst.frozen_runs = 0;
  if (src.whole) {
    dst.whole = std::make_shared<Plan>();
    plan_clone_compiled(*src.whole, *dst.whole);
  }
}

}  // namespace tq
