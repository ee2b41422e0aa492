// Plan finishing: what happens to a lowered plan (the ops, tables and arena peaks tq_plan.cpp's
// Compiler leaves) before it can run -- arena bases and slice lanes, lane-batched GEMMs and lane
// sums, absolute offsets, the operand-max words (assign_amax), the table layout, the counters,
// the launch schedule (build_schedule) and the describe text.  Apart from the four arena peaks
// everything here reads and writes the Plan alone.  Also the plan's host-only layouts and
// digests that queries read (plan_planes_layout, plan_tables_digest).
#include "tq_plan_compile.h"
#include "tq_plan_internal.h"

#include <algorithm>
#include <cstddef>
#include <sstream>

namespace tq {

namespace {

int64_t al(int64_t b) { return (b + kAlign - 1) / kAlign * kAlign; }

// arena layout: [region 0][region 1] | pinned: [region 0][region 1], then the slice lanes' copies
// of the per-slice part
void layout_arena(Plan& P, int64_t arena_end, int64_t pinned_bytes) {
  P.pinned_base = (size_t)al(arena_end);
  P.arena_bytes = P.pinned_base + (size_t)pinned_bytes;
  P.lane0_bytes = P.arena_bytes;
  P.lanes = 1;
  if (const int want = slice_lanes(); P.n_slices > 1 && want > 1 && P.pinned_base > 0) {
    const int64_t cap = std::min<int64_t>({(int64_t)want, P.n_slices,
                                           (int64_t)(lane_arena_budget() / P.pinned_base)});
    while (P.lanes * 2 <= cap) P.lanes *= 2;   // a power of two
  }
  P.lane_phys = (size_t)al((int64_t)(P.arena_bytes - P.pinned_base));
  P.lane_stride = P.pinned_base;
  P.lane_ws_off = P.lane_phys + (size_t)P.lanes * P.lane_stride;
  P.arena_bytes = P.lane_ws_off;   // + the lane-batched GEMM workspace (batch_lanes)
}

// lane-batched GEMMs and their shared workspace, and the lane sums
void batch_lanes(Plan& P) {
  if (P.lanes > 1) {
    size_t wsmax = 0;
    for (auto& op : P.ops) {
      const bool okab = (op.a.kind == BUF_ARENA || op.a.kind == BUF_PINNED) &&
                        (op.b.kind == BUF_ARENA || op.b.kind == BUF_PINNED);
      if (op.kind != OP_GEMM || op.skinny || op.invariant || op.batch != 1 || op.writes_output || !okab ||
          op.c.kind != BUF_ARENA || (P.lane_stride / P.esz) % 2)
        continue;
      op.lane_batch = true;
      op.note += " lanes";
      wsmax = std::max(wsmax, gemm_workspace(P.dtype, op.M, op.N, op.K, P.lanes));
    }
    // a lane-batched GEMM or a lane-merged sweep2 level (a per-slice op: every lane's copy in
    // one launch) whose result only an output permute reads: sum the lanes first, then permute
    // once per batch instead of once per lane
    for (size_t i = 0; i < P.ops.size(); ++i) {
      Op& g = P.ops[i];
      const bool s2 = g.kind == OP_SWEEP2 && !g.s2_dense && !g.invariant && !g.writes_output &&
                      g.c.kind == BUF_ARENA;
      if (!g.lane_batch && !s2) continue;
      const int64_t lo = g.c.off, hi = g.c.off + g.nc;
      int reader = -1, nread = 0;
      for (size_t k = i + 1; k < P.ops.size(); ++k) {
        const Op& o = P.ops[k];
        auto rd = [&](const BufRef& r, int64_t n) { return r.kind == BUF_ARENA && r.off < hi && lo < r.off + n; };
        if (rd(o.a, o.na) || rd(o.b, o.nb) || (o.kind == OP_AXPY && rd(o.c, o.nc))) { ++nread; reader = (int)k; }
        for (auto& sg : o.sgates) if (rd(sg.g, std::max<int64_t>(sg.n, 1))) ++nread;
        if (o.c.kind == BUF_ARENA && o.c.off < hi && lo < o.c.off + o.nc) break;   // overwritten
      }
      if (nread != 1) continue;
      Op& pm = P.ops[reader];
      if (pm.kind != OP_PERMUTE || !pm.writes_output || pm.invariant || pm.a.off != g.c.off) continue;
      g.lane_sum = pm.lane_once = true;
      g.note += " lane-sum";
    }
    P.lane_ws_bytes = (size_t)al((int64_t)wsmax);
    P.arena_bytes += P.lane_ws_bytes;
  }
}

// region-relative offsets become absolute
void fix_offsets(Plan& P, const int64_t abase[2], const int64_t pbase[2]) {
  const int64_t esz = (int64_t)P.esz;
  auto fix = [&](BufRef& b) {
    if (b.kind == BUF_ARENA) b.off += abase[b.region] / esz;
    else if (b.kind == BUF_PINNED) b.off += pbase[b.region] / esz;
    b.region = 0;
  };
  for (auto& op : P.ops) {
    fix(op.a); fix(op.b); fix(op.c); fix(op.ws);
    for (auto& g : op.sgates) fix(g.g);
  }
}

// table layout: permute tables, gather tables, descriptor blobs, then the max / scale / flag words
void layout_tables(Plan& P) {
  size_t tb = 0;
  P.perm_tab_off.clear();
  for (auto& pp : P.perms) {
    P.perm_tab_off.push_back(tb);
    tb += (perm_plan_table_bytes(pp) + kAlign - 1) / kAlign * kAlign;
  }
  P.gtab_off.clear();
  for (auto& g : P.gtabs) {
    P.gtab_off.push_back(tb);
    tb += (g.size() * sizeof(int32_t) + kAlign - 1) / kAlign * kAlign;
  }
  P.stab_off.clear();
  for (auto& b : P.stabs) {
    P.stab_off.push_back(tb);
    tb += (b.size() + kAlign - 1) / kAlign * kAlign;
  }
  // constant operands in the tables (the compose ops' identity matrices): BufRef::index = blob
  for (auto& op : P.ops)
    for (BufRef* r : {&op.a, &op.b})
      if (r->kind == BUF_TABLE) r->off = (int64_t)P.stab_off[r->index];
  P.amax_off = tb;
  // per-slice words: one set per slice lane (every lane's operands scaled by their own max)
  tb += ((size_t)(P.n_amax_once + P.n_amax_slice * std::max(1, P.lanes)) * sizeof(uint32_t) + kAlign - 1) /
        kAlign * kAlign;
  P.sc_off = tb;
  tb += ((size_t)P.n_amax_slice * sizeof(int32_t) + kAlign - 1) / kAlign * kAlign;
  P.bad_off = tb;
  if (P.n_ps) tb += ((size_t)P.n_slices * sizeof(uint32_t) + kAlign - 1) / kAlign * kAlign;
  P.table_bytes = tb;
}

void count_ops(Plan& P) {
  for (auto& op : P.ops) {
    (op.frozen ? P.flops_frozen : op.invariant ? P.flops_once : P.flops_slice) += op.flops;
    (op.frozen ? P.bytes_frozen : op.invariant ? P.bytes_once : P.bytes_slice) += op.bytes;
    if (op.frozen && op.c.kind == BUF_PINNED) P.frozen_kept_bytes += (size_t)op.nc * P.esz;
    P.n_gemm += op.kind == OP_GEMM;
    P.n_apply += op.kind == OP_APPLY;
    P.n_permute += op.kind == OP_PERMUTE;
    P.n_sweep += op.kind == OP_SWEEP || op.kind == OP_SWEEP2;
    if (op.kind == OP_SWEEP || op.kind == OP_SWEEP2) P.n_sweep_gates += (int)op.sgates.size();
  }
  P.flops = P.flops_frozen + P.flops_once + P.flops_slice * (double)P.n_slices;
  P.bytes = P.bytes_frozen + P.bytes_once + P.bytes_slice * (double)P.n_slices;
}

// the ops, the launch schedule and the merged launches as text (tq_plan_describe)
std::string describe(const Plan& P) {
  std::ostringstream d;
  for (size_t i = 0; i < P.ops.size(); ++i)
    d << (P.ops[i].frozen ? "[frozen] " : P.ops[i].invariant ? "[once]  " : "[slice] ") << "b"
      << P.ops[i].branch << " "
      << P.ops[i].note << "\n";
  d << "# schedule (launch: op indices)\n";
  for (int set = 0; set < 2; ++set) {
    int e = 0;
    for (auto& g : set == 0 ? P.sched_once : P.sched_slice) {
      d << "# " << (set == 1 ? "slice" : e++ < P.n_sched_frozen ? "frozen" : "once ");
      for (int j : g) d << " " << j;
      d << "\n";
    }
  }
  for (auto& st : P.full_steps)
    if (st.first >= 0 && st.second >= 0)
      d << "# full run: frozen entry " << st.first << " and once entry " << st.second << " share a launch\n";
  for (auto& r : P.seq_once) {
    d << "# chain launch (a workgroup per stream, one-chunk layouts): once entries " << r.first << ".."
      << r.second - 1 << ", ops";
    for (int i = r.first; i < r.second; ++i)
      for (int j : P.sched_once[i])
        d << " " << j << "/s" << P.seq_stream[j] << ((P.ops[j].lds_io & 1) ? "<" : "")
          << ((P.ops[j].lds_io & 2) ? ">" : "");
    d << "   (< input from LDS, > result left in LDS)\n";
  }
  for (size_t r = 0; r < P.coop_once.size(); ++r) {
    d << "# cooperative chain launch (" << P.coop_width[r]
      << " workgroups, a counter barrier between ops): once entries " << P.coop_once[r].first << ".."
      << P.coop_once[r].second - 1 << ", ops";
    for (int i = P.coop_once[r].first; i < P.coop_once[r].second; ++i) d << " " << P.sched_once[i][0];
    d << "\n";
  }
  return d.str();
}

// Operand-max words for the complex64 f16-split GEMM (tq_gemm.hip): when a GEMM that can take
// the K-outer fast path reads an operand that one sweep2 op stored in full (same buffer, same
// element count, no other writer in between), that sweep op max-es |re|, |im| of what it
// stores into a word the GEMM reads, instead of the GEMM re-reading both operands (1 GiB per
// C4 slice) for their max.  Words of slice-invariant producers are zeroed once per execute
// call, the others before every slice.
void assign_amax(Plan& P) {
  P.n_amax_once = P.n_amax_slice = P.n_amax_frozen = 0;
  if (P.dtype != TQ_C64) return;
  const int64_t esz = (int64_t)P.esz;
  auto span = [&](const BufRef& b, int64_t n, int* space, int64_t* lo, int64_t* hi) {
    if (b.kind == BUF_ARENA) { *space = 0; *lo = b.off * esz; }
    else if (b.kind == BUF_PINNED) { *space = 0; *lo = (int64_t)P.pinned_base + b.off * esz; }
    else if (b.kind == BUF_OUTPUT) { *space = 1; *lo = b.off * esz; }
    else return false;
    *hi = *lo + n * esz;
    return true;
  };
  std::vector<int> frozen, once, slice;  // producer op indices, in word order
  auto words_of = [&](int j) -> std::vector<int>& {
    return P.ops[j].frozen ? frozen : P.ops[j].invariant ? once : slice;
  };
  auto producer = [&](int gi, const BufRef& r, int64_t n) -> int {
    int sp, spw;
    int64_t lo, hi, wlo, whi;
    if (!span(r, n, &sp, &lo, &hi)) return -1;
    for (int j = gi - 1; j >= 0; --j) {
      const Op& w = P.ops[j];
      if (!span(w.c, w.nc, &spw, &wlo, &whi)) continue;
      if (spw != sp || whi <= lo || hi <= wlo) continue;
      // the latest writer of these bytes: usable only if it stored exactly this operand
      if (w.kind == OP_SWEEP2 && !w.writes_output && wlo == lo && whi == hi) return j;
      return -1;
    }
    return -1;
  };
  std::vector<int> prod_a(P.ops.size(), -1), prod_b(P.ops.size(), -1);
  for (size_t i = 0; i < P.ops.size(); ++i) {
    const Op& g = P.ops[i];
    if (g.kind != OP_GEMM || g.transA != 1 || g.transB != 0) continue;
    if (g.M % 128 || g.N % 128 || g.K % 16 || g.lda % 2 || g.ldb % 2) continue;
    if (g.lda >= (int64_t(1) << 24) || g.ldb >= (int64_t(1) << 24)) continue;
    if (g.batch > 1 && (g.sA % 2 || g.sB % 2)) continue;
    const int pa = producer((int)i, g.a, g.na), pb = producer((int)i, g.b, g.nb);
    if (pa < 0 || pb < 0) continue;
    prod_a[i] = pa;
    prod_b[i] = pb;
    for (int j : {pa, pb}) {
      auto& v = words_of(j);
      if (std::find(v.begin(), v.end(), j) == v.end()) v.push_back(j);
    }
  }
  // the pre-split boundary GEMM (tq_gemmp.hip): a per-slice GEMM whose operands are each stored
  // in full by one per-slice dense sweep op and read by nothing else; those ops then store the
  // operand as six f16 term planes, scaled from a bound built on the max of their own input,
  // whose producer (a sweep2 op storing exactly that input) gets a max word too.  The largest
  // such GEMM of the plan (C4 / C3: the boundary contraction of the cut network)
  P.planes_gemm = -1;
  std::vector<int> planes_x(P.ops.size(), -1);
  if (planes_enabled()) {
    auto only_reader = [&](int j, int gi) {
      int sp, spo;
      int64_t lo, hi, olo, ohi;
      const Op& w = P.ops[j];
      if (!span(w.c, w.nc, &sp, &lo, &hi)) return false;
      auto hits = [&](const BufRef& r, int64_t n) {
        return span(r, n, &spo, &olo, &ohi) && spo == sp && olo < hi && lo < ohi;
      };
      for (size_t k = j + 1; k < P.ops.size(); ++k) {
        const Op& o = P.ops[k];
        if ((int)k != gi) {
          if (hits(o.a, o.na) || hits(o.b, o.nb) || (o.kind == OP_AXPY && hits(o.c, o.nc))) return false;
          for (auto& g : o.sgates) if (hits(g.g, std::max<int64_t>(g.n, 1))) return false;
        }
        if (hits(o.c, o.nc) || (o.nws && hits(o.ws, o.nws))) break;
      }
      return true;
    };
    double best = 0;
    for (size_t i = 0; i < P.ops.size(); ++i) {
      const Op& g = P.ops[i];
      const int pa = prod_a[i], pb = prod_b[i];
      if (pa < 0 || pa == pb || g.invariant || g.batch != 1 || g.writes_output || g.skinny) continue;
      if (!planes_gemm_ok(g.M, g.N, g.K, g.lda, g.ldb)) continue;
      const Op& da = P.ops[pa];
      const Op& db = P.ops[pb];
      if (!da.s2_dense || !db.s2_dense || da.invariant || db.invariant || da.writes_output || db.writes_output) continue;
      if (!only_reader(pa, (int)i) || !only_reader(pb, (int)i)) continue;
      const int xa = producer(pa, da.a, da.na), xb = producer(pb, db.a, db.na);
      if (xa < 0 || xb < 0 || P.ops[xa].s2_dense || P.ops[xb].s2_dense) continue;
      if (P.ops[xa].invariant != P.ops[xb].invariant) continue;
      const double w = (double)g.M * g.N * g.K;
      if (w > best) {
        best = w;
        P.planes_gemm = (int)i;
        planes_x[pa] = xa;
        planes_x[pb] = xb;
      }
    }
    if (P.planes_gemm >= 0) {
      const Op& g = P.ops[P.planes_gemm];
      const int pab[2] = {prod_a[P.planes_gemm], prod_b[P.planes_gemm]};
      for (int r = 0; r < 2; ++r) {
        const int j = pab[r], x = planes_x[j];
        P.ops[j].planes_role = r + 1;
        auto& v = words_of(x);
        if (std::find(v.begin(), v.end(), x) == v.end()) v.push_back(x);
        // the planes (12 B per element) replace the complex64 store (8 B)
        P.ops[j].bytes += (double)P.ops[j].nc * 4.0;
        P.ops[j].note += r ? " planes(B)" : " planes(A)";
      }
      P.planes_n[0] = g.na;
      P.planes_n[1] = g.nb;
      P.ops[P.planes_gemm].note += " planes";
    }
  }
  // words: [frozen producers][the other hoisted producers][per slice, a set per lane]
  P.n_amax_frozen = (int)frozen.size();
  P.n_amax_once = (int)(frozen.size() + once.size());
  P.n_amax_slice = (int)slice.size();
  for (size_t q = 0; q < frozen.size(); ++q) P.ops[frozen[q]].amax_word = (int)q;
  for (size_t q = 0; q < once.size(); ++q) P.ops[once[q]].amax_word = P.n_amax_frozen + (int)q;
  for (size_t q = 0; q < slice.size(); ++q) P.ops[slice[q]].amax_word = P.n_amax_once + (int)q;
  for (size_t j = 0; j < P.ops.size(); ++j)
    if (P.ops[j].planes_role) P.ops[j].planes_in_amax = P.ops[planes_x[j]].amax_word;
  for (size_t i = 0; i < P.ops.size(); ++i) {
    if (prod_a[i] < 0) continue;
    P.ops[i].amax_a = P.ops[prod_a[i]].amax_word;
    P.ops[i].amax_b = P.ops[prod_b[i]].amax_word;
    P.ops[i].note += " amax<-op" + std::to_string(prod_a[i]) + ",op" + std::to_string(prod_b[i]);
  }
  // pre-split candidates: per-slice GEMM, per-slice producers that store nothing else read
  // (scan forward from the producer until its bytes are overwritten), batch 1, no beta
  P.n_ps = 0;
  auto exclusive = [&](int j, int gi) {
    int sp, spo;
    int64_t lo, hi, olo, ohi;
    const Op& w = P.ops[j];
    if (!span(w.c, w.nc, &sp, &lo, &hi)) return false;
    auto hits = [&](const BufRef& r, int64_t n) {
      return span(r, n, &spo, &olo, &ohi) && spo == sp && olo < hi && lo < ohi;
    };
    for (size_t k = j + 1; k < P.ops.size(); ++k) {
      const Op& o = P.ops[k];
      if ((int)k != gi) {
        if (hits(o.a, o.na) || hits(o.b, o.nb) || (o.kind == OP_AXPY && hits(o.c, o.nc))) return false;
        for (auto& g : o.sgates) if (hits(g.g, std::max<int64_t>(g.n, 1))) return false;
      }
      if (hits(o.c, o.nc) || (o.nws && hits(o.ws, o.nws))) break;
    }
    return true;
  };
  const int64_t max_slices = 1 << 16;
  for (size_t i = 0; i < P.ops.size(); ++i) {
    Op& g = P.ops[i];
    const int pa = prod_a[i], pb = prod_b[i];
    if (pa < 0 || pa == pb || g.invariant || g.batch != 1 || P.n_slices > max_slices) continue;
    if ((int)i == P.planes_gemm) continue;
    if (P.ops[pa].invariant || P.ops[pb].invariant) continue;
    if (P.ops[pa].ps_gemm >= 0 || P.ops[pb].ps_gemm >= 0) continue;
    if (!exclusive(pa, (int)i) || !exclusive(pb, (int)i)) continue;
    g.ps_cand = true;
    P.ops[pa].ps_gemm = P.ops[pb].ps_gemm = (int)i;
    g.note += " presplit";
    ++P.n_ps;
  }
}

struct Acc { int space; int64_t lo, hi; };   // a byte range of the arena (space 0) or the output (1)
bool overlap(const std::vector<Acc>& x, const std::vector<Acc>& y) {
  for (auto& a : x)
    for (auto& b : y)
      if (a.space == b.space && a.lo < b.hi && b.lo < a.hi) return true;
  return false;
}
// the byte ranges every op reads and writes
struct Hazards {
  const Plan& P;
  const int64_t esz;
  std::vector<std::vector<Acc>> rd, wr;
  explicit Hazards(const Plan& plan) : P(plan), esz((int64_t)plan.esz), rd(plan.ops.size()), wr(plan.ops.size()) {
    for (size_t i = 0; i < P.ops.size(); ++i) {
      const Op& op = P.ops[i];
      add(rd[i], op.a, op.na);
      add(rd[i], op.b, op.nb);
      add(wr[i], op.c, op.nc);
      add(rd[i], op.c, op.nc);    // beta accumulation reads the target
      add(wr[i], op.ws, op.nws);
      add(rd[i], op.ws, op.nws);
      for (auto& g : op.sgates) add(rd[i], g.g, g.n);
    }
  }
  void add(std::vector<Acc>& v, const BufRef& b, int64_t n) const {
    if (n <= 0) return;
    switch (b.kind) {
      case BUF_ARENA: v.push_back({0, b.off * esz, (b.off + n) * esz}); break;
      case BUF_PINNED:
        v.push_back({0, (int64_t)P.pinned_base + b.off * esz, (int64_t)P.pinned_base + (b.off + n) * esz});
        break;
      case BUF_OUTPUT: v.push_back({1, b.off * esz, (b.off + n) * esz}); break;
      default: break;  // inputs are never written
    }
  }
  bool conflict(int i, int j) const {   // RAW, WAW or WAR
    return overlap(wr[i], rd[j]) || overlap(wr[i], wr[j]) || overlap(rd[i], wr[j]);
  }
};

// three sets, in execution order: frozen, hoisted, per slice (the first two in sched_once)
void schedule_levels(Plan& P, const Hazards& H) {
  const size_t n = P.ops.size();
  P.sched_once.clear();
  P.sched_slice.clear();
  for (int set = 0; set < 3; ++set) {
    std::vector<int> ids;
    for (size_t i = 0; i < n; ++i)
      if ((P.ops[i].frozen ? 0 : P.ops[i].invariant ? 1 : 2) == set) ids.push_back((int)i);
    std::vector<int> lev(ids.size(), 0);
    int maxlev = -1;
    for (size_t b = 0; b < ids.size(); ++b) {
      const int j = ids[b];
      for (size_t a = 0; a < b; ++a) {
        const int i = ids[a];
        if (lev[a] + 1 <= lev[b]) continue;
        if (H.conflict(i, j)) lev[b] = lev[a] + 1;
      }
      maxlev = std::max(maxlev, lev[b]);
    }
    auto& sched = set < 2 ? P.sched_once : P.sched_slice;
    for (int L = 0; L <= maxlev; ++L) {
      std::vector<int> grp;
      for (size_t b = 0; b < ids.size(); ++b) {
        if (lev[b] != L) continue;
        const int j = ids[b];
        if (P.ops[j].kind != OP_SWEEP2) { sched.push_back({j}); continue; }
        grp.push_back(j);
        if ((int)grp.size() == kS2MaxOps) { sched.push_back(grp); grp.clear(); }
      }
      if (!grp.empty()) sched.push_back(grp);
    }
    if (set == 0) P.n_sched_frozen = (int)P.sched_once.size();
  }
  P.n_launch_frozen = P.n_sched_frozen;
  P.n_launch_once = (int)P.sched_once.size() - P.n_sched_frozen;
  P.n_launch_slice = (int)P.sched_slice.size();
}

// chain launches: consecutive hoisted levels that are each one small sweep2 op (C2's whole
// contraction, the first levels of C3 / C4's hoisted chains: 1-4 workgroups per launch) run
// in order by one workgroup in one launch
// Levels of several such ops (the left and right halves of a cut network) run as several
// streams of one launch, a workgroup each, when every op conflicts (RAW / WAR / WAW) with
// earlier ops of at most one stream: that stream's workgroup runs it after them.
void chain_launches(Plan& P, const Hazards& H) {
  P.seq_once.clear();
  P.seq_stream.assign(P.ops.size(), -1);
  P.use_seq = s2_seq_enabled();
  auto chainable = [&](const std::vector<int>& g) {
    if (g.empty() || (int)g.size() > kS2SeqMaxStreams) return false;
    for (int j : g) {
      const Op& op = P.ops[j];
      if (op.kind != OP_SWEEP2 || op.s2_dense || op.stab1 < 0) return false;
    }
    return true;
  };
  const int ns = (int)P.sched_once.size();
  for (int i = 0; i < ns;) {
    if (!chainable(P.sched_once[i])) { ++i; continue; }
    std::vector<int> in_run;   // ops of the run so far
    int nstreams = 0, nops = 0, e = i;
    const int seg_end = i < P.n_sched_frozen ? P.n_sched_frozen : ns;   // (a run stays in its schedule)
    for (; e < seg_end && chainable(P.sched_once[e]); ++e) {
      const auto& g = P.sched_once[e];
      if (nops + (int)g.size() > kS2MaxOps) break;
      std::vector<int> st(g.size(), -1);
      int fresh = nstreams;
      bool ok = true;
      for (size_t q = 0; q < g.size() && ok; ++q) {
        int s = -1;
        for (int k : in_run)
          if (H.conflict(k, g[q])) {
            if (s >= 0 && P.seq_stream[k] != s) { ok = false; break; }
            s = P.seq_stream[k];
          }
        st[q] = s >= 0 ? s : fresh++;
      }
      if (!ok || fresh > kS2SeqMaxStreams) break;
      for (size_t q = 0; q < g.size(); ++q) { P.seq_stream[g[q]] = st[q]; in_run.push_back(g[q]); }
      nstreams = fresh;
      nops += (int)g.size();
    }
    if (e - i >= 2) {
      P.seq_once.push_back({i, e});
    } else {
      for (int k : in_run) P.seq_stream[k] = -1;
      e = std::max(e, i + 1);
    }
    i = e;
  }
}

// LDS hand-offs inside a chain launch: op j's result stays in the workgroup's LDS for the
// next op k of its stream when k reads exactly that tensor, it fits 64 KiB, and no other op
// reads it before it is overwritten (true reads: a, b, gate tensors; the scan follows the
// execution order: the rest of the hoisted launches, then every per-slice launch)
void lds_handoffs(Plan& P, const Hazards& H) {
  const size_t n = P.ops.size();
  const int64_t esz = H.esz;
  const auto& wr = H.wr;
  auto add = [&](std::vector<Acc>& v, const BufRef& b, int64_t cnt) { H.add(v, b, cnt); };
  for (auto& o : P.ops) o.lds_io = 0;
  std::vector<int> order;   // execution order of the ops (hoisted, then per slice)
  for (auto& g : P.sched_once) for (int j : g) order.push_back(j);
  for (auto& g : P.sched_slice) for (int j : g) order.push_back(j);
  std::vector<int> at(n, -1);
  for (size_t q = 0; q < order.size(); ++q) at[order[q]] = (int)q;
  auto true_reads = [&](int i) {
    std::vector<Acc> v;
    const Op& op = P.ops[i];
    add(v, op.a, op.na);
    add(v, op.b, op.nb);
    for (auto& g : op.sgates) add(v, g.g, g.n);
    return v;
  };
  for (auto& r : P.seq_once) {
    std::vector<int> run;
    for (int i = r.first; i < r.second; ++i) for (int j : P.sched_once[i]) run.push_back(j);
    // bit 2: no op of the launch writes this op's gate tensors (prefetch while the previous
    // op of its stream runs)
    for (int k : run) {
      std::vector<Acc> gr;
      for (auto& g : P.ops[k].sgates) add(gr, g.g, g.n);
      bool clean = true;
      for (int i : run) clean = clean && !overlap(wr[i], gr);
      if (clean && s2_seq_prefetch()) P.ops[k].lds_io |= 4;
    }
    for (size_t x = 0; x < run.size(); ++x) {
      const int j = run[x];
      int k = -1;
      for (size_t y = x + 1; y < run.size() && k < 0; ++y)
        if (P.seq_stream[run[y]] == P.seq_stream[j]) k = run[y];
      if (k < 0) continue;
      const Op& oj = P.ops[j];
      const Op& ok = P.ops[k];
      if (oj.writes_output || oj.amax_word >= 0 || oj.ps_gemm >= 0 || oj.c.kind != ok.a.kind ||
          oj.c.off != ok.a.off || oj.c.index != ok.a.index || oj.c.region != ok.a.region || oj.nc != ok.na || oj.nc * esz > kS2ChunkBytes)
        continue;
      std::vector<Acc> out;
      add(out, oj.c, oj.nc);
      if (out.size() != 1) continue;
      bool alone = true;
      for (size_t q = (size_t)at[j] + 1; q < order.size() && alone; ++q) {
        const int i = order[q];
        if (i == k) continue;
        if (overlap(true_reads(i), out)) { alone = false; break; }
        std::vector<Acc> w;
        add(w, P.ops[i].c, P.ops[i].nc);
        add(w, P.ops[i].ws, P.ops[i].nws);
        bool covered = false;
        for (auto& a : w) covered = covered || (a.space == out[0].space && a.lo <= out[0].lo && a.hi >= out[0].hi);
        if (covered) break;   // overwritten: no later op reads j's values
      }
      if (!alone) continue;
      P.ops[j].lds_io |= 2;
      P.ops[k].lds_io |= 1;
    }
  }
}

// cooperative chain launches: consecutive hoisted levels that are each ONE multi-chunk sweep2
// op outside a chain launch (C2: 27 levels of 4-chunk ops after its one-chunk chain) run as
// one launch of n workgroups, every op's chunks spread over all of them and a counter barrier
// between consecutive ops (S2Launch::sync).  Plain ops only (no beta / max / split / output:
// their stores and loads are the coherent forms), and no op of a run writes a gate tensor of
// the run (gates are read through the caches, and prefetched)
void coop_launches(Plan& P, const Hazards& H) {
  const int ns = (int)P.sched_once.size();
  const auto& wr = H.wr;
  P.coop_once.clear();
  P.coop_width.clear();
  P.use_coop = s2_coop_enabled();
  std::vector<char> in_chain(ns, 0);
  for (auto& r : P.seq_once)
    for (int i = r.first; i < r.second; ++i) in_chain[i] = 1;
  auto coop_ok = [&](int i) {
    if (in_chain[i] || P.sched_once[i].size() != 1) return false;
    const Op& op = P.ops[P.sched_once[i][0]];
    return op.kind == OP_SWEEP2 && !op.s2_dense && !op.writes_output && op.amax_word < 0 && op.ps_gemm < 0 &&
           op.s2_nchunks >= 2 && op.s2_nchunks <= s2_coop_max_chunks();
  };
  for (int i = 0; i < ns;) {
    if (!coop_ok(i)) { ++i; continue; }
    std::vector<Acc> gates, writes;
    int e = i;
    const int seg_end = i < P.n_sched_frozen ? P.n_sched_frozen : ns;
    for (; e < seg_end && coop_ok(e) && e - i < kS2MaxOps; ++e) {
      const int j = P.sched_once[e][0];
      std::vector<Acc> g;
      for (auto& sg : P.ops[j].sgates) H.add(g, sg.g, sg.n);
      if (overlap(wr[j], gates) || overlap(writes, g) || overlap(wr[j], g)) break;
      gates.insert(gates.end(), g.begin(), g.end());
      writes.insert(writes.end(), wr[j].begin(), wr[j].end());
    }
    if (e - i >= 2) {
      // workgroups: the most common chunk count of the run (an op of more chunks strides them)
      std::vector<int> cnt(17, 0);
      for (int q = i; q < e; ++q) ++cnt[(int)P.ops[P.sched_once[q][0]].s2_nchunks];
      int w = 2;
      for (int c = 2; c <= 16; ++c) if (cnt[c] > cnt[w]) w = c;
      P.coop_once.push_back({i, e});
      P.coop_width.push_back(std::min(w, kS2SeqMaxStreams));
      // the next op's descriptor and gates prefetched (no op of the run writes a gate of it)
      for (int q = i; q < e; ++q) P.ops[P.sched_once[q][0]].lds_io = s2_seq_prefetch() ? 4 : 0;
    }
    i = std::max(e, i + 1);
  }
}

// The full run (a call that runs the frozen schedule too): the frozen entries and the hoisted
// ones in their own orders, zipped -- a hoisted plain sweep2 level that conflicts with no frozen
// entry still to come shares the launch of the next frozen plain sweep2 level, as the two
// halves' levels do in a plan that declares nothing.  Chain and cooperative runs stay whole
// and unmerged, and every op runs in the launch form it has in a live-only call (the same
// descriptor and chunks), so a full and a live-only call compute the same bits.
void full_run(Plan& P, const Hazards& H) {
  const int ns = (int)P.sched_once.size();
  P.full_steps.clear();
  P.n_full_merged = 0;
  if (P.n_sched_frozen > 0) {
    const int nf = P.n_sched_frozen;
    // units of sched_once: a run (chain or cooperative) or one entry; [first, last)
    auto units = [&](int b, int e) {
      std::vector<std::pair<int, int>> u;
      for (int i = b; i < e;) {
        int last = i + 1;
        for (auto& r : P.seq_once) if (r.first == i) last = r.second;
        for (auto& r : P.coop_once) if (r.first == i) last = r.second;
        u.push_back({i, last});
        i = last;
      }
      return u;
    };
    const auto F = units(0, nf), L = units(nf, ns);
    auto plain = [&](const std::pair<int, int>& u) {
      if (u.second - u.first != 1) return false;
      for (int j : P.sched_once[u.first])
        if (P.ops[j].kind != OP_SWEEP2 || P.ops[j].s2_dense) return false;
      return true;
    };
    auto unit_conflict = [&](const std::pair<int, int>& a, const std::pair<int, int>& b) {
      for (int x = a.first; x < a.second; ++x)
        for (int y = b.first; y < b.second; ++y)
          for (int i : P.sched_once[x])
            for (int j : P.sched_once[y])
              if (H.conflict(i, j)) return true;
      return false;
    };
    size_t fi = 0, li = 0;
    while (fi < F.size()) {
      bool merge = li < L.size() && plain(F[fi]) && plain(L[li]) &&
                   P.sched_once[F[fi].first].size() + P.sched_once[L[li].first].size() <= (size_t)kS2MaxOps;
      for (size_t k = fi; merge && k < F.size(); ++k) merge = !unit_conflict(F[k], L[li]);
      if (merge) {
        P.full_steps.push_back({F[fi].first, L[li].first});
        ++P.n_full_merged;
        ++li;
      } else {
        P.full_steps.push_back({F[fi].first, -1});
      }
      ++fi;
    }
    for (; li < L.size(); ++li) P.full_steps.push_back({-1, L[li].first});
  }
}

// Launch schedule.  Ops of one set (slice-invariant / per slice) are ordered by dependency
// level: an op's level is one more than that of every earlier op it conflicts with (RAW, WAR
// or WAW on overlapping bytes of the arena, the output or a workspace; inputs are read-only).
// Ops of one level commute, so the independent in-place sweeps of a level (e.g. the left and
// right subtrees of a cut network, or the tiny vector pre-absorption chains) share a launch.
// Then the launches that merge consecutive levels, and the full run's order.
void build_schedule(Plan& P) {
  const Hazards H(P);
  schedule_levels(P, H);
  chain_launches(P, H);
  lds_handoffs(P, H);
  coop_launches(P, H);
  full_run(P, H);
}

}  // namespace

void plan_finish(Plan& P, const int64_t arena_peak[2], const int64_t pinned_peak[2]) {
  const int64_t abase[2] = {0, al(arena_peak[0])};
  const int64_t pbase[2] = {0, al(pinned_peak[0])};
  layout_arena(P, abase[1] + arena_peak[1], pbase[1] + pinned_peak[1]);
  batch_lanes(P);
  fix_offsets(P, abase, pbase);
  assign_amax(P);
  layout_tables(P);
  count_ops(P);
  build_schedule(P);
  // cooperative chain counters (S2Launch::sync): a 256-byte slot each, behind the other tables
  // (zero from the upload; every launch leaves its counter at zero)
  P.sync_off = P.table_bytes;
  P.table_bytes += P.coop_once.size() * Plan::kSyncSlot;
  P.describe = describe(P);
}

void plan_planes_layout(Plan& P) {
  if (P.planes_gemm < 0) return;
  const Op& g = P.ops[P.planes_gemm];
  const size_t lanes = (size_t)std::max(1, P.lanes);
  auto al = [](size_t b) { return (b + 255) / 256 * 256; };
  P.planes_lane_bytes = al((size_t)12 * (size_t)(P.planes_n[0] + P.planes_n[1]));
  P.planes_ws_off = lanes * P.planes_lane_bytes;
  // every lane-batch size up to the lane count: a partial batch may pick more K splits (r05c)
  P.planes_sc_off = P.planes_ws_off + al(planes_gemm_workspace(g.M, g.N, g.K, (int64_t)lanes));
  P.planes_bytes = P.planes_sc_off + al(lanes * 2 * sizeof(int32_t));
}

int64_t plan_tables_digest(const Plan& P) {
  uint64_t h = 0xcbf29ce484222325ull;   // FNV-1a-64
  auto bytes = [&](const void* p, size_t n) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 0x100000001b3ull;
  };
  auto i64 = [&](int64_t v) { bytes(&v, sizeof v); };
  auto ref = [&](const BufRef& r) { i64(r.kind); i64(r.off); i64(r.index); };
  for (auto& g : P.gtabs) bytes(g.data(), g.size() * sizeof(int32_t));
  // an S2Desc blob holds the struct's one padding hole (in front of the 8-aligned gate array)
  constexpr size_t hole = offsetof(S2Desc, aux_cb) + sizeof(int32_t), hole_end = offsetof(S2Desc, gate);
  static_assert(hole_end - hole < 8 && sizeof(S2Desc) == hole_end + kS2MaxGates * sizeof(S2Gate), "S2Desc padding");
  std::vector<char> is_desc(P.stabs.size(), 0);
  for (auto& op : P.ops)
    if (op.kind == OP_SWEEP2 && !op.s2_dense)
      for (int s : {op.stab, op.stab1}) if (s >= 0) is_desc[s] = 1;
  for (size_t s = 0; s < P.stabs.size(); ++s) {
    const auto& b = P.stabs[s];
    if (is_desc[s] && b.size() >= sizeof(S2Desc)) {
      bytes(b.data(), hole);
      bytes(b.data() + hole_end, b.size() - hole_end);
    } else {
      bytes(b.data(), b.size());
    }
  }
  for (auto& op : P.ops) {
    i64(op.kind);
    for (const BufRef* r : {&op.a, &op.b, &op.c, &op.ws}) ref(*r);
    for (int64_t v : {op.na, op.nb, op.nc, op.nws, (int64_t)op.tin, (int64_t)op.tout, op.ncols, op.s2_nchunks,
                      (int64_t)op.stab, (int64_t)op.stab1, (int64_t)op.transA, (int64_t)op.transB, op.M, op.N, op.K,
                      op.batch, op.lda, op.ldb, op.ldc, op.sA, op.sB, op.sC, (int64_t)op.ws_bytes, op.O, op.I, op.K2,
                      (int64_t)op.gtab, (int64_t)op.perm, op.n, (int64_t)op.nruns, (int64_t)op.tout_off_at,
                      (int64_t)op.tabs_at, (int64_t)op.tab_len, (int64_t)op.load_colfast, (int64_t)op.store_colfast,
                      (int64_t)op.lds_io, (int64_t)op.amax_word, (int64_t)op.amax_a, (int64_t)op.amax_b,
                      (int64_t)op.ps_gemm, (int64_t)op.planes_role, (int64_t)op.planes_in_amax, (int64_t)op.branch})
      i64(v);
    for (bool f : {op.writes_output, op.invariant, op.frozen, op.s2_dense, op.ps_cand, op.lane_batch, op.lane_sum,
                   op.lane_once, op.skinny})
      i64(f);
    for (int r = 0; r < op.nruns; ++r) { i64(op.run_ext[r]); i64(op.run_in[r]); i64(op.run_out[r]); }
    for (auto& g : op.sgates) {
      ref(g.g);
      for (int64_t v : {(int64_t)g.gtab, (int64_t)g.K, (int64_t)g.N, (int64_t)g.W, g.n, (int64_t)g.tab_off}) i64(v);
    }
    if (op.skinny) {
      i64(op.sk.K); i64(op.sk.nkb); i64(op.sk.M); i64(op.sk.N);
      for (int64_t v : op.sk.wam) i64(v);
      for (int64_t v : op.sk.wbn) i64(v);
      for (int b = 0; b < op.sk.nkb; ++b) { i64(op.sk.wak[b]); i64(op.sk.wbk[b]); }
    }
  }
  return (int64_t)(h & 0x7fffffffffffffffull);
}

}  // namespace tq
