// The sweep-chain layout planner: which chains fit a sweep kernel (chain_shape), the dense form
// (s2_dense_layout), the re-listing of commuting square gates (s2_reorder_squares), the in-place
// butterfly sweep's descriptor (s2_layout: seven phases over one Layout) and its blob (s2_blob);
// behind them the inspectors of a compiled plan's descriptors (plan_s2_programs,
// plan_s2_prog_passes, plan_s2_gate_work).  The layout functions read the chain, the S2Ctx and
// the process-wide knobs, and nothing else.
#include "tq_sweep2_layout.h"

#include "tq_plan_internal.h"
#include "tq_sweep.h"

#include <algorithm>
#include <array>
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <type_traits>

namespace tq {

namespace {

// extent of a mode (0: unknown, which no layout accepts)
int64_t ext1(const S2Ctx& x, int m) {
  auto it = x.ext.find(m);
  return it == x.ext.end() ? 0 : it->second;
}

int ilog2(int64_t v) {
  if (v <= 0 || (v & (v - 1))) return -1;
  int l = 0;
  while ((int64_t(1) << l) < v) ++l;
  return l;
}

// GF(2) rank of a few small bit vectors
int gf2_rank(std::vector<int> v) {
  int r = 0;
  for (int bit = 31; bit >= 0; --bit) {
    int piv = -1;
    for (size_t i = r; i < v.size(); ++i) if ((v[i] >> bit) & 1) { piv = (int)i; break; }
    if (piv < 0) continue;
    std::swap(v[r], v[piv]);
    for (size_t i = 0; i < v.size(); ++i) if ((int)i != r && ((v[i] >> bit) & 1)) v[i] ^= v[r];
    ++r;
  }
  return r;
}

std::vector<int> ascending(uint32_t m) {
  std::vector<int> v;
  for (; m; m &= m - 1) v.push_back(__builtin_ctz(m));
  return v;
}

}  // namespace

int64_t ext_of(const S2Ctx& x, const std::vector<int>& ms) {
  int64_t p = 1;
  for (int m : ms) p *= ext1(x, m);
  return p;
}

void digits(const S2Ctx& x, int64_t t, const std::vector<int>& modes, std::map<int, int64_t>& dig) {
  for (int q = (int)modes.size() - 1; q >= 0; --q) {
    const int64_t e = ext1(x, modes[q]);
    dig[modes[q]] = t % e;
    t /= e;
  }
}

int64_t index_of(const S2Ctx& x, const std::vector<int>& modes, const std::map<int, int64_t>& dig) {
  int64_t t = 0;
  for (int m : modes) t = t * ext1(x, m) + dig.at(m);
  return t;
}

void chain_strides(const S2Ctx& x, const Chain& c, const std::vector<int>& out_modes,
                   std::map<int, int64_t>& sx, std::map<int, int64_t>& sy) {
  auto cs = contig_strides(c.X0.ext);
  for (size_t q = 0; q < c.X0.modes.size(); ++q) sx[c.X0.modes[q]] = cs[q];
  std::vector<int64_t> ye;
  for (int m : out_modes) ye.push_back(ext1(x, m));
  auto cy = contig_strides(ye);
  for (size_t q = 0; q < out_modes.size(); ++q) sy[out_modes[q]] = cy[q];
}

// A sweep2 op's descriptor blob: the S2Desc, then the host-built tables the kernel reads instead
// of walking the descriptor in LDS (S2Op::lanes / cbase): per thread of the 512 its load / store
// element's byte offset and LDS address (threads beyond a small chunk duplicate element tid % n,
// as the kernel's own enumeration), and per chunk (when there are at most kS2MaxCbTab) the memory
// base of its load / store elements.
std::vector<char> s2_blob(const S2Desc& d0, size_t esz) {
  S2Desc d = d0;
  auto al16 = [](size_t b) { return (b + 15) / 16 * 16; };
  const size_t off_l = al16(sizeof(S2Desc));
  const size_t off_c = off_l + (size_t)(1 << kS2LogThreads) * 16;
  const bool cb = d.nchunks >= 1 && d.nchunks <= kS2MaxCbTab;
  d.aux_lanes = (int32_t)off_l;
  d.aux_cb = cb ? (int32_t)off_c : 0;
  std::vector<char> blob(off_c + (cb ? (size_t)d.nchunks * 16 : 0), 0);
  std::memcpy(blob.data(), &d, sizeof(S2Desc));
  const int nin = 1 << d.nld, nout = 1 << d.nst;
  uint32_t* lt = reinterpret_cast<uint32_t*>(blob.data() + off_l);
  for (int tid = 0; tid < (1 << kS2LogThreads); ++tid) {
    const int ti = tid & (nin - 1), to = tid & (nout - 1);
    int64_t ldm = 0, stm = 0;
    int lda = 0, sta = 0;
    for (int b = 0; b < kS2LogThreads; ++b) {
      if (b < d.nld && ((ti >> b) & 1)) { ldm += d.ld_w[b]; lda ^= d.ld_a[b]; }
      if (b < d.nst && ((to >> b) & 1)) { stm += d.st_w[b]; sta ^= d.st_a[b]; }
    }
    lt[4 * tid + 0] = (uint32_t)(ldm * (int64_t)esz);
    lt[4 * tid + 1] = (uint32_t)(stm * (int64_t)esz);
    lt[4 * tid + 2] = (uint32_t)lda;
    lt[4 * tid + 3] = (uint32_t)sta;
  }
  if (cb) {
    int64_t* ct = reinterpret_cast<int64_t*>(blob.data() + off_c);
    for (int64_t ch = 0; ch < d.nchunks; ++ch) {
      int64_t bi = 0, bo = 0;
      for (int b = d.logC; b < d.colbits; ++b)
        if ((ch >> (b - d.logC)) & 1) { bi += d.k.w_in[b]; bo += d.k.w_out[b]; }
      ct[2 * ch] = bi;
      ct[2 * ch + 1] = bo;
    }
  }
  return blob;
}

bool chain_shape(const S2Ctx& x, const Chain& c, const std::vector<int>& out_modes, ChainShape& sh) {
  if ((int)c.gates.size() > std::max(kSweepMaxGates, kS2MaxGates)) return false;
  std::set<int> contracted;
  for (auto& g : c.gates) {
    if (g.d.K * g.d.N > kSweepMaxKN) return false;
    contracted.insert(g.d.korder.begin(), g.d.korder.end());
  }
  for (int m : c.X0.modes) (contracted.count(m) ? sh.tin : sh.outer).push_back(m);
  std::vector<int> w = sh.tin;
  sh.W.clear();
  for (size_t j = 0; j < c.gates.size(); ++j) {
    const auto& g = c.gates[j];
    std::vector<int> nw;
    for (int m : w) if (std::find(g.d.korder.begin(), g.d.korder.end(), m) == g.d.korder.end()) nw.push_back(m);
    for (int m : g.d.korder)
      if (std::find(w.begin(), w.end(), m) == w.end()) return false;  // contracts an outer mode
    nw.insert(nw.end(), g.d.nfree.begin(), g.d.nfree.end());
    w = nw;
    sh.W.push_back(w);
    sh.wmax = std::max(sh.wmax, ext_of(x, w));
  }
  std::set<int> wset(w.begin(), w.end());
  for (int m : out_modes) if (wset.count(m)) sh.tout.push_back(m);
  if (sh.tout.size() != w.size()) return false;
  sh.W.back() = sh.tout;
  // untouched modes keep their relative order (APPLY preserves it)
  std::vector<int> outer_y;
  for (int m : out_modes) if (!wset.count(m)) outer_y.push_back(m);
  if (outer_y != sh.outer) return false;
  sh.tin_n = ext_of(x, sh.tin);
  sh.tout_n = ext_of(x, sh.tout);
  sh.wmax = std::max({sh.wmax, sh.tin_n, sh.tout_n});
  int64_t tab = 0;
  for (size_t j = 0; j < c.gates.size(); ++j) tab += ext_of(x, sh.W[j]) * (c.gates[j].d.K + 1);
  const bool old_ok = (int)c.gates.size() <= kSweepMaxGates && sh.wmax <= sweep_wmax((int)x.esz) &&
                      tab <= kSweepTabMax;
  {
    S2Desc scratch;  // the full layout (every limit checked), so flush_chain cannot fail on it
    sh.s2 = s2_layout(x, c, sh, out_modes, &scratch);
  }
  return old_ok || sh.s2;
}

// Dense form of a sweep chain (tq_sweepd.hip): complex64, a small input tile (tin <= 16), an
// output tile of <= 256, a big tensor (>= 2^20 output elements), and the six lowest column bits
// memory-fastest and contiguous in X and Y (a wave's 64 lanes = 64 consecutive elements).
bool s2_dense_layout(const S2Ctx& x, const Chain& c, const ChainShape& sh, const std::vector<int>& out_modes,
                     S2Dense* dd) {
  if (!s2_dense_enabled() || x.dtype != TQ_C64 || !c.X0.contiguous()) return false;
  // whole 32-output MFMA tiles (tq_sweepd.hip)
  if (sh.tin_n < 2 || sh.tin_n > kS2DMaxTin || sh.tout_n < 32 || sh.tout_n > kS2DMaxTout || sh.tout_n % 32)
    return false;
  if (ilog2(sh.tin_n) < 0 || ilog2(sh.tout_n) < 0) return false;
  std::map<int, int64_t> sx, sy;
  chain_strides(x, c, out_modes, sx, sy);
  std::vector<std::pair<int64_t, int64_t>> cb;
  for (int m : sh.outer) {
    const int nb = ilog2(ext1(x, m));
    if (nb < 0) return false;
    for (int i = 0; i < nb; ++i) cb.push_back({sx[m] << i, sy.at(m) << i});
  }
  std::sort(cb.begin(), cb.end());
  if (cb.size() < 6 || (int)cb.size() > kS2MaxColBits) return false;
  for (int b = 0; b < 6; ++b)
    if (cb[b].first != (int64_t(1) << b) || cb[b].second != (int64_t(1) << b)) return false;
  const int64_t ncols = int64_t(1) << cb.size();
  if (ncols * sh.tout_n < (int64_t(1) << 20)) return false;
  dd->ncols = ncols;
  dd->colbits = (int)cb.size();
  dd->tin = (int)sh.tin_n;
  dd->tout = (int)sh.tout_n;
  for (size_t b = 0; b < cb.size(); ++b) { dd->w_in[b] = cb[b].first; dd->w_out[b] = cb[b].second; }
  std::map<int, int64_t> dig;
  for (int64_t t = 0; t < sh.tin_n; ++t) {
    digits(x, t, sh.tin, dig);
    int64_t o = 0;
    for (int m : sh.tin) o += dig[m] * sx[m];
    if (o >= (int64_t(1) << 31)) return false;   // staged as int32 by the kernel
    dd->in_off[t] = o;
  }
  for (int64_t t = 0; t < sh.tout_n; ++t) {
    digits(x, t, sh.tout, dig);
    int64_t o = 0;
    for (int m : sh.tout) o += dig[m] * sy.at(m);
    if (o >= (int64_t(1) << 31)) return false;   // the kernel stages them as int32
    dd->out_off[t] = o;
  }
  return true;
}

// Register blocks take CONSECUTIVE square gates whose positions fit B bits (block_span).  A
// brick-wall chain lists a layer's gates before the next layer's, so the greedy
// run closes a block at every layer's edge: (0,1)(2,3) | (4,5)(6,7) | (1,2)(3,4) ...  Square gates
// on disjoint positions commute (a square gate's outputs take its inputs' positions), so within
// each maximal run of square gates the gates are re-listed block by block: a block starts at
// the first unscheduled gate and takes every later gate whose overlapping predecessors (in the
// chain's order) are already scheduled or in the block, while the block's positions fit B bits.
// The result is a linear extension of the overlap order: per amplitude the same products,
// summed in another order of commuting factors (the rounding differs, the value does not).
// Non-square gates (expanding / contracting the working set) stay where they are.  False if
// the order is unchanged.
bool s2_reorder_squares(const S2Ctx& x, const Chain& c, Chain& out, int B) {
  const int ng = (int)c.gates.size();
  if (ng < 3) return false;
  auto nbits = [&](int m) { return ilog2(ext1(x, m)); };
  std::map<std::pair<int, int>, int> slot;   // (mode, bit) -> slot: s2_layout's positions, relabelled
  int next = 0;
  for (int m : c.X0.modes) for (int i = 0; i < nbits(m); ++i) slot[{m, i}] = next++;
  std::vector<std::vector<int>> sl(ng);
  std::vector<char> sq(ng, 0);
  for (int j = 0; j < ng; ++j) {
    const auto& g = c.gates[j];
    std::vector<int> freed;
    for (auto it = g.d.korder.rbegin(); it != g.d.korder.rend(); ++it)
      for (int i = 0; i < nbits(*it); ++i) {
        auto f = slot.find({*it, i});
        if (f == slot.end()) return false;
        freed.push_back(f->second);
        slot.erase(f);
      }
    size_t fi = 0, nout = 0;
    sl[j] = freed;
    for (auto it = g.d.nfree.rbegin(); it != g.d.nfree.rend(); ++it)
      for (int i = 0; i < nbits(*it); ++i, ++nout) {
        const int s = fi < freed.size() ? freed[fi++] : next++;
        slot[{*it, i}] = s;
        if (nout >= freed.size()) sl[j].push_back(s);
      }
    sq[j] = g.d.K == g.d.N && (g.d.K == 2 || g.d.K == 4) && nout == freed.size();
  }
  auto overlap = [&](int a, int b) {
    for (int p : sl[a]) for (int q : sl[b]) if (p == q) return true;
    return false;
  };
  std::vector<int> order;
  std::vector<char> done(ng, 0), inblk(ng, 0);
  for (int j = 0; j < ng;) {
    if (!sq[j]) { order.push_back(j++); continue; }
    int e = j;
    while (e < ng && sq[e]) ++e;
    std::vector<int> rem;
    for (int q = j; q < e; ++q) rem.push_back(q);
    while (!rem.empty()) {
      std::vector<int> blk{rem[0]}, U = sl[rem[0]];
      inblk[rem[0]] = 1;
      for (size_t t = 1; t < rem.size() && (int)blk.size() < kS2BlkMaxGates; ++t) {
        const int g = rem[t];
        bool ready = true;
        for (int h = j; h < g && ready; ++h) if (!done[h] && !inblk[h] && overlap(h, g)) ready = false;
        if (!ready) continue;
        std::vector<int> u2 = U;
        for (int p : sl[g]) if (std::find(u2.begin(), u2.end(), p) == u2.end()) u2.push_back(p);
        if ((int)u2.size() > B) continue;
        U = u2;
        blk.push_back(g);
        inblk[g] = 1;
      }
      for (int g : blk) {
        done[g] = 1;
        inblk[g] = 0;
        order.push_back(g);
        rem.erase(std::find(rem.begin(), rem.end(), g));
      }
    }
    j = e;
  }
  bool same = true;
  for (int j = 0; j < ng; ++j) same = same && order[j] == j;
  if (same) return false;
  out = c;
  for (int j = 0; j < ng; ++j) out.gates[j] = c.gates[order[j]];
  return true;
}

// ---- s2_layout -------------------------------------------------------------------------------
namespace {

typedef std::pair<int, int> MB;   // (mode, bit of its index)
struct CBit { int64_t w; int col; int pos; };  // a chunk bit; col >= 0: column bit, else tile position

// One pass over the tile: a single gate, a register block of consecutive square gates, or a lane
// block (TQ_S2_LANEBLK): a register block over 6 positions, 4 in a thread's registers and 2 on
// its lane bits 4 and 5 (group-index bits 4 and 5: the other 3 threads of the block are lanes
// l ^ 16, l ^ 32, l ^ 48 of the same wave).  A gate whose position sits on a lane bit first trades
// it with a register bit the gate does not use (a swap: v_permlane16 / 32_swap, 2 instructions per
// element pair and dword; the register position evicted is the one used again latest).  C4's
// light-cone staircases hold 3 gates in 4 positions and 5 in 6: about 40 % fewer LDS passes on
// its big sweep ops for ~0.3 swaps per gate (r06 model).
struct PPlan {
  int first = 0, end = 0;          // gates [first, end)
  bool block = false, lanes = false;
  uint32_t bm = 0, mask = 0;       // block positions (plain: B of them; lane: the 4 start
                                   // registers), group positions (pass mask)
  int reg0[4] = {}, reg1[4] = {};  // lane block: register bits' positions at start / end
  int ln0[2] = {}, ln1[2] = {};    // lane bits 4 / 5: positions at start / end
  std::vector<std::array<int, 3>> ops;   // lane block: {gate, slot i, slot j (-1: 2x2)} or {-1, lane bit, slot}
  std::vector<int> order;          // group-index bits (after the columns) -> position
};

// what s2_layout's phases hand on to each other
struct Layout {
  const S2Ctx& x;
  const Chain& c;
  const ChainShape& sh;
  const std::vector<int>& out_modes;
  int maxpos = 0;                        // tile positions this tensor may use
  std::map<int, int64_t> sx, sy;         // element strides in X / Y
  std::map<MB, int> pos_in, pos;         // position of every input-tile / output-tile mode bit
  std::vector<std::vector<int>> kdep, ndep;   // per gate: position bits of input k / output n
  std::vector<uint32_t> kmask;           // per gate: its input positions
  int used = 0;                          // positions in use (log2 tile rows)
  std::vector<int> last_np;              // output positions of the last gate, index bit order
  int last_nk = 0;                       // its input index bits (they are the first output bits)
  std::vector<std::pair<int64_t, int64_t>> cb;   // column bits: (stride in X, stride in Y), ascending
  std::vector<CBit> ld, st;              // load / store enumerations: chunk bits by memory stride
  int B = 3;                             // register-block bits
  bool blocks = false, lane_ok = false;  // register blocks / lane blocks may be planned
  std::vector<PPlan> plan;               // the passes (the epilogue gate is none)
  S2Desc d;
  int nbits(int m) const { return ilog2(ext1(x, m)); }
  int ngates() const { return (int)c.gates.size(); }
};

// Phase 1.  Every mode bit of the working set gets a tile position (input tile bits
// memory-fastest first; a gate's outputs reuse the positions it frees); the gates' K / N, pass
// masks and coefficient indices.  False if the chain does not fit: non power-of-two extents, K or
// N beyond the kernel's, more than maxpos live bits, a final working set that is not the output tile.
bool assign_positions(Layout& L) {
  const S2Ctx& x = L.x;
  const Chain& c = L.c;
  // tiles beyond 2^(chunk bits - 5) positions leave fewer than 32 columns per chunk and the
  // gate passes 2- to 4-way LDS bank conflicts: only small (latency-bound) tensors use them,
  // where the longer chains save launches
  L.maxpos = s2_max_pos((int)x.esz);
  {
    int64_t nx = 1, ny = 1;
    for (int m : c.X0.modes) nx *= ext1(x, m);
    for (int m : L.out_modes) ny *= ext1(x, m);
    if (std::max(nx, ny) > s2_small_elems()) L.maxpos = std::min(L.maxpos, s2_chunk_bits((int)x.esz) - 5);
  }
  for (int m : c.X0.modes) if (L.nbits(m) < 0) return false;
  if (!c.X0.contiguous()) return false;
  for (auto& g : c.gates) {
    if (g.d.K > kS2MaxK || g.d.N > kS2MaxKN) return false;
    for (int m : g.d.nfree) if (L.nbits(m) < 0) return false;
  }
  chain_strides(x, c, L.out_modes, L.sx, L.sy);
  std::map<MB, int>& pos = L.pos;
  std::vector<std::pair<int64_t, MB>> tb;
  for (int m : L.sh.tin) for (int i = 0; i < L.nbits(m); ++i) tb.push_back({L.sx[m] << i, {m, i}});
  std::sort(tb.begin(), tb.end());
  uint32_t live = 0;
  for (auto& t : tb) {
    if (L.used >= L.maxpos) return false;
    pos[t.second] = L.used;
    live |= 1u << L.used;
    ++L.used;
  }
  L.pos_in = pos;
  S2Desc& d = L.d;
  d.ngates = L.ngates();
  L.kdep.resize(c.gates.size());
  L.ndep.resize(c.gates.size());
  L.kmask.assign(c.gates.size(), 0);
  for (size_t j = 0; j < c.gates.size(); ++j) {
    const auto& g = c.gates[j];
    std::vector<MB> kb, nb;   // index bits, least significant first
    for (auto it = g.d.korder.rbegin(); it != g.d.korder.rend(); ++it)
      for (int i = 0; i < L.nbits(*it); ++i) kb.push_back({*it, i});
    for (auto it = g.d.nfree.rbegin(); it != g.d.nfree.rend(); ++it)
      for (int i = 0; i < L.nbits(*it); ++i) nb.push_back({*it, i});
    if ((int64_t(1) << kb.size()) != g.d.K || (int64_t(1) << nb.size()) != g.d.N) return false;
    uint32_t kmask = 0;
    std::vector<int> freed, kp;
    for (auto& b : kb) {
      auto f = pos.find(b);
      if (f == pos.end()) return false;
      kmask |= 1u << f->second;
      freed.push_back(f->second);
      kp.push_back(f->second);
      pos.erase(f);
    }
    L.kmask[j] = kmask;
    S2Gate& G = d.gate[j];
    G.K = (int)g.d.K;
    G.N = (int)g.d.N;
    G.pass_mask = live & ~kmask;
    live &= ~kmask;
    std::vector<int> np;
    size_t fi = 0;
    for (auto& b : nb) {
      int p;
      if (fi < freed.size()) p = freed[fi++];
      else {
        p = 0;
        while (p < L.maxpos && ((live >> p) & 1)) ++p;
        if (p >= L.maxpos) return false;
      }
      pos[b] = p;
      live |= 1u << p;
      np.push_back(p);
      L.used = std::max(L.used, p + 1);
    }
    if (j + 1 == c.gates.size()) { L.last_np = np; L.last_nk = (int)kp.size(); }
    for (int k = 0; k < G.K; ++k) {
      int v = 0;
      for (size_t t = 0; t < kp.size(); ++t) if ((k >> t) & 1) v |= 1 << kp[t];
      L.kdep[j].push_back(v);
    }
    for (int n = 0; n < G.N; ++n) {
      int v = 0;
      for (size_t t = 0; t < np.size(); ++t) if ((n >> t) & 1) v |= 1 << np[t];
      L.ndep[j].push_back(v);
    }
    for (int t = 0; t < G.K * G.N; ++t) {
      G.gidx[t] = g.d.gtab.empty() ? t : g.d.gtab[t];
      if (G.gidx[t] >= kS2GateRaw) return false;   // the kernel stages kS2GateRaw elements per gate
      d.cgidx[j][t] = (uint8_t)G.gidx[t];
    }
  }
  // the final working set must be the output tile
  std::set<MB> want;
  for (int m : L.sh.tout) for (int i = 0; i < L.nbits(m); ++i) want.insert({m, i});
  std::set<MB> have;
  for (auto& kv : pos) have.insert(kv.first);
  return want == have;
}

// Phase 2.  The columns are the untouched mode bits by increasing stride; the chunk width.
bool choose_columns(Layout& L, bool one_chunk) {
  const S2Ctx& x = L.x;
  S2Desc& d = L.d;
  auto& cb = L.cb;
  for (int m : L.sh.outer)
    for (int i = 0; i < L.nbits(m); ++i) cb.push_back({L.sx[m] << i, L.sy.at(m) << i});
  std::sort(cb.begin(), cb.end());
  if ((int)cb.size() > kS2MaxColBits) return false;
  d.colbits = (int)cb.size();
  d.ncols = int64_t(1) << d.colbits;
  for (size_t j = 0; j < cb.size(); ++j) { d.k.w_in[j] = cb[j].first; d.k.w_out[j] = cb[j].second; }
  const int lc_cap = s2_chunk_bits((int)x.esz) - L.used;
  if (lc_cap < 0) return false;
  int lc = std::max(s2_base_logc(), d.colbits - 10);
  lc = std::min(lc, lc_cap);
  lc = std::min(lc, d.colbits);
  // small tensors: narrower chunks, so that the op still spreads over >= s2_min_chunks()
  // workgroups (a 2^19-element tensor with a 256-element tile has only 64 chunks of 32 columns)
  if (const int mc = std::max(1, (x.min_chunks > 0 ? x.min_chunks : s2_min_chunks()) /
                                     (x.group_hint * ((L.c.dep && x.lanes_hint > 1) ? x.lanes_hint : 1)));
      mc > 1) {
    int lg = 0;
    while ((2 << lg) <= mc) ++lg;
    const int minlc = L.used >= 9 ? std::min(s2_min_logc(), s2_min_logc_big()) : s2_min_logc();
    lc = std::min(lc, std::max(std::min(minlc, d.colbits), d.colbits - lg));
  }
  if (one_chunk) lc = std::min(lc_cap, d.colbits);
  d.logC = lc;
  d.nchunks = int64_t(1) << (d.colbits - lc);
  return true;
}

// Phase 3.  Load / store enumerations: the chunk bits (the chunk's columns and the tile
// positions) by increasing memory stride in X / Y.
void build_enumerations(Layout& L) {
  for (int j = 0; j < L.d.logC; ++j) {
    L.ld.push_back({L.cb[j].first, j, -1});
    L.st.push_back({L.cb[j].second, j, -1});
  }
  for (auto& kv : L.pos_in) L.ld.push_back({L.sx[kv.first.first] << kv.first.second, -1, kv.second});
  for (auto& kv : L.pos) L.st.push_back({L.sy.at(kv.first.first) << kv.first.second, -1, kv.second});
  auto by_w = [](const CBit& a, const CBit& b) { return a.w < b.w; };
  std::sort(L.ld.begin(), L.ld.end(), by_w);
  std::sort(L.st.begin(), L.st.end(), by_w);
}

// ---- phase 4: passes.  Register blocks of consecutive square gates (S2Desc::pmeta).
bool square(const Layout& L, int j) {
  const S2Gate& G = L.d.gate[j];
  if (G.K != G.N || (G.K != 2 && G.K != 4)) return false;
  for (int k = 0; k < G.K; ++k) if (L.kdep[j][k] != L.ndep[j][k]) return false;
  return true;
}

void block_params(Layout& L) {
  // TQ_S2_B4MIN: the smallest tile (elements) that gets 16-element register blocks (default
  // 4096 since r04: a 4096-element tile then leaves half the threads idle in its block passes,
  // but needs fewer passes -- C2 0.386 -> 0.370 ms, C4 N = 8 rank -0.3 %; 8192 before)
  static const int64_t b4min = env_int64("TQ_S2_B4MIN", 4096);
  const int64_t tile_elems = int64_t(1) << (L.d.logC + L.used);
  L.B = (L.x.esz <= 8 && tile_elems >= b4min) ? 4 : s2_block_bits((int)L.x.esz, tile_elems);
  L.blocks = s2_blocks_enabled();
  L.lane_ok = s2_lane_blocks() && L.blocks && L.B == 4 && L.d.logC <= 4;
}

// the pass starting at gate j ends before block_span(j, ng); bm = its block positions, live = the
// live positions
int block_span(const Layout& L, int j, int ng, uint32_t* bm_out, uint32_t* live_out) {
  int e = j + 1;
  uint32_t bm = 0, live = 0;
  if (L.blocks && square(L, j)) {
    bm = L.kmask[j];
    live = L.d.gate[j].pass_mask | bm;
    while (e < ng && e - j < kS2BlkMaxGates && square(L, e) && __builtin_popcount(bm | L.kmask[e]) <= L.B)
      bm |= L.kmask[e], ++e;
  }
  if (e - j >= 2) {
    // pad the block with untouched live positions up to B bits (fewer, larger groups)
    for (int q = 0; q < kS2MaxPos && __builtin_popcount(bm) < L.B; ++q)
      if (((live >> q) & 1) && !((bm >> q) & 1)) bm |= 1u << q;
    if (__builtin_popcount(bm) != L.B) e = j + 1;
  }
  *bm_out = bm;
  *live_out = live;
  return e;
}

// the lane block starting at gate j that takes more gates than the plain block's e4, if any
bool lane_span(const Layout& L, int j, int ng, int e4, PPlan& lp) {
  const S2Desc& d = L.d;
  if (!L.lane_ok || !square(L, j)) return false;
  const uint32_t live = d.gate[j].pass_mask | L.kmask[j];
  int e = j + 1;
  uint32_t u = L.kmask[j];
  while (e < ng && e - j < kS2BlkMaxGates && square(L, e) && __builtin_popcount(u | L.kmask[e]) <= 6)
    u |= L.kmask[e], ++e;
  for (; e > e4 && e - j >= 2; --e) {
    // positions in order of first use, then untouched live positions (they stay on the lanes)
    std::vector<int> first_use;
    for (int q = j; q < e; ++q)
      for (int p : ascending(L.kmask[q]))
        if (std::find(first_use.begin(), first_use.end(), p) == first_use.end()) first_use.push_back(p);
    if (first_use.size() <= 4 || first_use.size() > 6) continue;
    uint32_t padded = 0;
    for (int p : first_use) padded |= 1u << p;
    for (int p : ascending(live & ~padded)) {
      if (first_use.size() >= 6) break;
      first_use.push_back(p);
      padded |= 1u << p;
    }
    if (first_use.size() != 6) return false;
    const std::vector<int> oth = ascending(live & ~padded);
    if ((int)oth.size() < 4 - d.logC) return false;
    int reg[4], ln[2];
    for (int b = 0; b < 4; ++b) reg[b] = first_use[b];
    ln[0] = first_use[4];
    ln[1] = first_use[5];
    PPlan r;
    r.first = j;
    r.end = e;
    r.block = r.lanes = true;
    std::copy(reg, reg + 4, r.reg0);
    std::copy(ln, ln + 2, r.ln0);
    auto slot = [&](int p) {
      for (int b = 0; b < 4; ++b) if (reg[b] == p) return b;
      return -1;
    };
    for (int q = j; q < e; ++q) {
      const std::vector<int> gp = ascending(L.kmask[q]);
      for (int p : gp) {
        if (slot(p) >= 0) continue;
        const int l = ln[0] == p ? 0 : 1;
        // evict the register position (not this gate's) whose next use is latest
        int best = -1, best_next = -1;
        for (int b = 0; b < 4; ++b) {
          if (std::find(gp.begin(), gp.end(), reg[b]) != gp.end()) continue;
          int nx = 1 << 20;
          for (int t = q + 1; t < e; ++t)
            if ((L.kmask[t] >> reg[b]) & 1) { nx = t; break; }
          if (nx > best_next) best_next = nx, best = b;
        }
        r.ops.push_back({-1, l, best});
        std::swap(reg[best], ln[l]);
      }
      // index bit t of the gate <-> position of input k = 1 << t
      const int i0 = slot(__builtin_ctz((uint32_t)L.kdep[q][1]));
      const int j0 = d.gate[q].K == 4 ? slot(__builtin_ctz((uint32_t)L.kdep[q][2])) : -1;
      r.ops.push_back({q, i0, j0});
    }
    if ((int)r.ops.size() > kS2BlkMaxGates) continue;
    std::copy(reg, reg + 4, r.reg1);
    std::copy(ln, ln + 2, r.ln1);
    for (int b = 0; b < 4; ++b) r.bm |= 1u << r.reg0[b];
    r.mask = live & ~r.bm;
    // lane bits 4 / 5 are group-index bits 4 / 5: the lane positions at order 4 - logC, 5 - logC
    r.order.assign(oth.begin(), oth.begin() + (4 - d.logC));
    r.order.push_back(r.ln0[0]);
    r.order.push_back(r.ln0[1]);
    r.order.insert(r.order.end(), oth.begin() + (4 - d.logC), oth.end());
    lp = r;
    return true;
  }
  return false;
}

// the passes of gates [0, ng)
std::vector<PPlan> plan_passes(const Layout& L, int ng) {
  std::vector<PPlan> v;
  for (int j = 0; j < ng;) {
    uint32_t bm = 0, lv = 0;
    const int e = block_span(L, j, ng, &bm, &lv);
    PPlan pp;
    if (lane_span(L, j, ng, e, pp)) {
      v.push_back(pp);
      j = pp.end;
      continue;
    }
    pp.first = j;
    pp.end = e;
    pp.block = e - j >= 2;
    pp.bm = pp.block ? bm : 0;
    pp.mask = pp.block ? (lv & ~bm) : L.d.gate[j].pass_mask;
    pp.order = ascending(pp.mask);
    v.push_back(pp);
    j = e;
  }
  return v;
}

// Phase 5.  Store-phase epilogue: the last gate (K <= N, its inputs on the first output
// positions) is applied in registers while the tile leaves LDS -- one LDS write + read of the
// largest working set and one barrier less per chunk.  Its output position bits move to the
// lowest register-slot bits of the store enumeration (the lane bits keep the smallest strides);
// the positions it adds are not live before it, so input k sits in slot r0 + k.
void choose_epilogue(Layout& L) {
  S2Desc& d = L.d;
  std::vector<CBit>& st = L.st;
  // a last gate inside a register block costs no pass of its own: no epilogue then
  bool last_alone = true;
  {
    const std::vector<PPlan> pl = plan_passes(L, L.ngates());
    if (!pl.empty()) last_alone = pl.back().end - pl.back().first == 1;
  }
  d.epi = 0;
  if (!(s2_epi_enabled() && last_alone && !L.last_np.empty())) return;
  const S2Gate& G = d.gate[L.ngates() - 1];
  const int nn = (int)L.last_np.size();
  bool ok = G.K <= G.N && G.K * G.N <= 16 && G.N >= 2 && L.last_nk <= nn &&
            (int)st.size() >= kS2LogThreads + nn && (int)st.size() <= kS2LogThreads + 4;
  std::vector<CBit> rest, moved(nn);
  for (size_t t = 0; ok && t < st.size(); ++t) {
    const auto it = std::find(L.last_np.begin(), L.last_np.end(), st[t].pos);
    if (st[t].col >= 0 || it == L.last_np.end()) { rest.push_back(st[t]); continue; }
    if (t < 5) ok = false;   // keep the coalesced 32-lane runs
    moved[it - L.last_np.begin()] = st[t];
  }
  if (!ok) return;
  st.assign(rest.begin(), rest.begin() + kS2LogThreads);
  st.insert(st.end(), moved.begin(), moved.end());
  st.insert(st.end(), rest.begin() + kS2LogThreads, rest.end());
  d.epi = L.ngates();
}

// ---- phase 6: the swizzle.  The tile image of (position set p, column c) is
//   ((p << logC) | c) ^ S(p),  S(p) = XOR of vsw[q] over the positions q in p,
// vsw[q] a 5-bit vector: only address bits below 5 are XOR-ed, so the map is a bijection of
// the tile when the images of the address bits below 5 stay independent (columns j: 1 << j,
// positions q with q + logC < 5: (1 << (q + logC)) ^ vsw[q]; BankModel::valid).
// A wave's LDS access is served in lane groups (MI355X_MICROARCH.md §LDS; 8-byte elements:
// ds_read_b64 2 x 32 lanes on element mod 32, ds_write_b64 4 x 16 lanes on element mod 16);
// every access of the kernel is XOR-linear in its lane bits, so a group of 2^k lanes whose
// address differences span k directions with bank effects of rank r is 2^(k - r)-way.  The
// lane directions: the load (LDS writes) and store (reads) enumerations, and for every pass
// the columns then the pass positions (tq_sweep2.hip gate_pass_u / block_pass group index).
// Chunks of fewer than 32 columns put pass positions into the lane groups, which a swizzle
// of the column bits alone (r04) could not separate: the r04 PMC's 0.9 conflict cycles per
// sweep2 LDS instruction on C4's 8-column slice ops.  The vectors: the enumerations' choice,
// then a coordinate descent on the modeled cost (0 on every sweep op of C2 / C3 / C4).
struct BankModel {
  struct Pat { std::vector<int> dirs; double rd, wr; };   // column j -> -(j + 1), position q -> q
  std::vector<Pat> pats;
  int logC = 0, lowb = 0;     // lowb: address bits the swizzle may write
  int rl, rm, wl, wm;         // log2 lanes per group / log2 bank modulus (elements), reads / writes
  uint32_t rel = 0;           // positions that reach a lane group: the only ones whose vector matters

  double ideal() const {
    double v = 0;
    for (auto& pt : pats) v += pt.rd / double(1 << rl) + pt.wr / double(1 << wl);
    return v;
  }
  double cost(const int* w) const {   // modeled extra LDS cycles per chunk
    double c = 0;
    for (auto& pt : pats)
      for (int side = 0; side < 2; ++side) {
        const double n = side ? pt.wr : pt.rd;
        const int lg = side ? wl : rl, mb = (1 << (side ? wm : rm)) - 1;
        if (n <= 0) continue;
        std::vector<int> eff;
        for (int t = 0; t < (int)pt.dirs.size() && t < lg; ++t) {
          const int dd = pt.dirs[t];
          eff.push_back((dd < 0 ? (1 << (-dd - 1)) : ((1 << (dd + logC)) ^ w[dd])) & mb);
        }
        const int k = (int)eff.size();
        c += n * double((1 << (k - gf2_rank(eff))) - 1) / double(1 << lg);
      }
    return c;
  }
  bool valid(const int* w) const {
    std::vector<int> im;
    for (int b = 0; b < lowb; ++b) im.push_back(b < logC ? 1 << b : (1 << b) ^ w[b - logC]);
    return gf2_rank(im) == lowb;
  }
  // coordinate descent over the eligible positions' vectors (strict improvements only: a
  // conflict-free start stays as it was)
  double descend(int* w) const {
    double b = cost(w);
    for (int it = 0; it < 6 && b > 0; ++it) {
      bool moved = false;
      for (int q = 0; q < kS2MaxPos; ++q) {
        if (!((rel >> q) & 1)) continue;
        int bv = w[q];
        for (int v = 0; v < (1 << lowb); ++v) {
          if (v == bv) continue;
          w[q] = v;
          if (q + logC < 5 && !valid(w)) continue;
          const double c = cost(w);
          if (c < b - 1e-9) b = c, bv = v, moved = true;
        }
        w[q] = bv;
      }
      if (!moved) break;
    }
    return b;
  }
};

// swizzle vectors of the enumerations' own choice: the first 4 / 5 chunk bits of each
// enumeration (one 16- / 32-lane group) must map to independent bank slots (mod 16 / mod 32)
void enum_swizzle(const std::vector<CBit>& e, int* vsw) {
  std::vector<int> vec;
  for (size_t t = 0; t < e.size() && t < 5; ++t) {
    if (e[t].col >= 0) { vec.push_back(e[t].col < 5 ? (1 << e[t].col) : 0); continue; }
    int& v = vsw[e[t].pos];
    if (v < 0) {
      static const int order[] = {1, 2, 4, 8, 16, 3, 5, 6, 9, 10, 12, 17, 18, 20, 24, 7, 11, 13,
                                  14, 19, 21, 22, 25, 26, 28, 15, 23, 27, 29, 30, 31};
      v = 0;
      for (int cand : order) {
        std::vector<int> a = vec, b;
        a.push_back(cand);
        for (size_t q = 0; q < a.size() && q < 4; ++q) b.push_back(a[q] & 15);
        if (gf2_rank(a) == (int)a.size() && gf2_rank(b) == (int)b.size()) { v = cand; break; }
      }
    }
    vec.push_back(v);
  }
}

void choose_swizzle(Layout& L) {
  S2Desc& d = L.d;
  int vsw[kS2MaxPos];
  for (int& v : vsw) v = -1;
  enum_swizzle(L.ld, vsw);
  enum_swizzle(L.st, vsw);
  BankModel M;
  M.logC = d.logC;
  if (L.x.esz <= 4) M.rl = M.rm = M.wl = M.wm = 5;
  else if (L.x.esz == 8) { M.rl = M.rm = 5; M.wl = M.wm = 4; }
  else { M.rl = M.rm = 4; M.wl = M.wm = 3; }
  auto enum_dirs = [&](const std::vector<CBit>& e) {
    std::vector<int> v;
    for (size_t t = 0; t < e.size() && t < 5; ++t) v.push_back(e[t].col >= 0 ? -(e[t].col + 1) : e[t].pos);
    return v;
  };
  // (the enumerations weigh one access each: d.nld / d.nst are filled in after this phase)
  M.pats.push_back({enum_dirs(L.ld), 0.0, double(int64_t(1) << d.nld)});
  M.pats.push_back({enum_dirs(L.st), double(int64_t(1) << d.nst), 0.0});
  // as fill_passes (the lane bits of a lane block: its start layout)
  for (const PPlan& pp : L.plan) {
    double rd, wr;
    if (!pp.block) rd = d.gate[pp.first].K, wr = d.gate[pp.first].N;
    else rd = wr = double(1 << L.B);
    std::vector<int> v;
    for (int q = 0; q < d.logC && v.size() < 5; ++q) v.push_back(-(q + 1));
    for (size_t t = 0; t < pp.order.size() && v.size() < 5; ++t) v.push_back(pp.order[t]);
    const double groups = double(int64_t(1) << (d.logC + __builtin_popcount(pp.mask)));
    M.pats.push_back({v, groups * rd, groups * wr});
  }
  for (auto& pt : M.pats)
    for (int dd : pt.dirs)
      if (dd >= 0 && dd < L.used) M.rel |= 1u << dd;
  M.lowb = std::min(5, d.logC + L.used);
  const double ideal = M.ideal();
  int swl[kS2MaxPos];
  const int cm = (1 << d.logC) - 1;
  for (int q = 0; q < kS2MaxPos; ++q) swl[q] = (vsw[q] < 0 ? 0 : vsw[q]) & cm;   // the r04 layout
  d.lds_model[0] = (float)(ideal > 0 ? M.cost(swl) / ideal : 0.0);
  double best;
  if (!s2_swz_model()) {   // TQ_S2_SWZ=0: the r04 column-only swizzle (A/B)
    best = M.cost(swl);
  } else {
    // start from the enumerations' choice
    for (int q = 0; q < kS2MaxPos; ++q) swl[q] = (vsw[q] < 0 || q + d.logC < 5) ? 0 : vsw[q];
    best = M.descend(swl);
  }
  d.lds_model[1] = (float)(ideal > 0 ? best / ideal : 0.0);
  for (int p = 0; p < kS2MaxPos; ++p) d.vsw[p] = swl[p];
}

// ---- phase 7: the descriptor
// group table of a pass: group-index bits (after the columns) -> positions, in `order`
void group_lut(const Layout& L, const std::vector<int>& order, int32_t* lut) {
  const S2Desc& d = L.d;
  for (int jj = 0; jj < 64; ++jj) {
    const int half = jj >> 5, v = jj & 31;
    int base = 0, sw = 0;
    for (int t = 0; t < (int)order.size(); ++t) {
      const int lo = order[t];
      if (half == 0 && t < 5 && ((v >> t) & 1)) { base |= 1 << lo; sw ^= d.vsw[lo]; }
      if (half == 1 && t >= 5 && ((v >> (t - 5)) & 1)) { base |= 1 << lo; sw ^= d.vsw[lo]; }
    }
    lut[jj] = ((base << d.logC) ^ sw) * (int32_t)L.x.esz;   // bytes
  }
}

// codes and LDS addresses of the enumerations' chunk bits, the register slots and the gates'
// inputs / outputs.  False if the enumerations do not fit the kernel
bool fill_addresses(Layout& L) {
  S2Desc& d = L.d;
  auto code = [&](const CBit& b) {
    if (b.col >= 0) return 1 << b.col;
    return ((1 << b.pos) << kS2CodeP) | (d.vsw[b.pos] << kS2CodeS);
  };
  d.nld = (int)L.ld.size();
  d.nst = (int)L.st.size();
  if (d.nld > 16 || d.nst > 16) return false;
  for (size_t t = 0; t < L.ld.size(); ++t) { d.ld_w[t] = L.ld[t].w; d.ld_code[t] = code(L.ld[t]); }
  for (size_t t = 0; t < L.st.size(); ++t) { d.st_w[t] = L.st[t].w; d.st_code[t] = code(L.st[t]); }
  // the kernel carries the lane part of a load / store offset (the low kS2LogThreads chunk
  // bits) as a 32-bit byte offset: chains on high-order legs of huge tensors do not fit
  if (!s2_lane_offsets_fit(d.ld_w, d.nld, d.st_w, d.nst, (int64_t)L.x.esz)) return false;
  // LDS element address of a code: ((p << logC) | c) ^ s -- XOR-linear in the code
  auto lds_addr = [&](int cd) {
    const int p = (cd >> kS2CodeP) & ((1 << kS2MaxPos) - 1), cc = cd & ((1 << kS2CodeP) - 1),
              sv = (cd >> kS2CodeS) & 31;
    return ((p << d.logC) | cc) ^ sv;
  };
  for (int t = 0; t < d.nld; ++t) d.ld_a[t] = lds_addr(d.ld_code[t]);
  for (int t = 0; t < d.nst; ++t) d.st_a[t] = lds_addr(d.st_code[t]);
  const int rin = std::max(1, (1 << d.nld) >> kS2LogThreads), rout = std::max(1, (1 << d.nst) >> kS2LogThreads);
  for (int r = 0; r < kS2MaxSlots; ++r) {
    const int ri = r % rin, ro = r % rout;
    for (int b = kS2LogThreads; b < d.nld; ++b)
      if ((ri >> (b - kS2LogThreads)) & 1) { d.k.ld_hm[r] += d.ld_w[b]; d.ld_hc[r] ^= d.ld_code[b]; }
    for (int b = kS2LogThreads; b < d.nst; ++b)
      if ((ro >> (b - kS2LogThreads)) & 1) { d.k.st_hm[r] += d.st_w[b]; d.st_hc[r] ^= d.st_code[b]; }
    d.k.ld_ha[r] = lds_addr(d.ld_hc[r]);
    d.k.st_ha[r] = lds_addr(d.st_hc[r]);
  }
  auto swz = [&](int bits) {
    int v = 0;
    for (int p = 0; p < kS2MaxPos; ++p) if ((bits >> p) & 1) v ^= d.vsw[p];
    return v;
  };
  for (int j = 0; j < L.ngates(); ++j) {
    S2Gate& G = d.gate[j];
    for (int k = 0; k < G.K; ++k) {
      G.kdep[k] = L.kdep[j][k];
      G.ksw[k] = swz(L.kdep[j][k]);
      G.kaddr[k] = (G.kdep[k] << d.logC) ^ G.ksw[k];
    }
    for (int n = 0; n < G.N; ++n) {
      G.ndep[n] = L.ndep[j][n];
      G.nsw[n] = swz(L.ndep[j][n]);
      G.naddr[n] = (G.ndep[n] << d.logC) ^ G.nsw[n];
    }
  }
  return true;
}

// gate fields and per-gate group tables (what the kernel used to build per workgroup)
void fill_gates(Layout& L) {
  S2Desc& d = L.d;
  for (int j = 0; j < L.ngates(); ++j) {
    const S2Gate& G = d.gate[j];
    int32_t* gm = d.k.gmeta[j];
    gm[kS2GmK] = G.K;
    gm[kS2GmN] = G.N;
    gm[kS2GmPass] = (int32_t)G.pass_mask;
    for (int k = 0; k < kS2MaxK; ++k) gm[kS2GmKaddr + k] = k < G.K ? G.kaddr[k] : 0;
    for (int n = 0; n < kS2MaxKN; ++n) gm[kS2GmNaddr + n] = n < G.N ? G.naddr[n] : 0;
    group_lut(L, ascending(G.pass_mask), d.k.lut[j]);
  }
}

// a gate's block code from its register slots; canonical placement I < J: swap the gate's
// two legs -- input / output index bits 0 and 1 of every coefficient (a square gate: its
// outputs sit on its inputs' positions).  The kernel then needs 6 (B = 4) / 3 (B = 3)
// block-gate bodies instead of 12 / 6 (instruction-cache footprint, tq_sweep2.hip blk_gate)
int gate_code(S2Desc& d, int q, int i0, int j0) {
  if (d.gate[q].K != 4) return i0;
  if (i0 > j0) {
    uint8_t cg[16];
    auto sw = [](int v) { return ((v & 1) << 1) | ((v >> 1) & 1); };
    for (int k = 0; k < 4; ++k)
      for (int n = 0; n < 4; ++n) cg[sw(k) * 4 + sw(n)] = d.cgidx[q][k * 4 + n];
    for (int t = 0; t < 16; ++t) d.cgidx[q][t] = cg[t];
    std::swap(i0, j0);
  }
  return i0 | (j0 << 2) | 16;
}

// passes: register blocks of consecutive square gates (S2Desc::pmeta) -- plain, or lane
// blocks (plan_passes) -- single gates otherwise; then the group tables by pass
bool fill_passes(Layout& L) {
  S2Desc& d = L.d;
  const int B = L.B;
  if ((int)L.plan.size() > kS2MaxGates) return false;
  auto addr = [&](int pos) { return ((1 << pos) << d.logC) ^ d.vsw[pos]; };   // elements
  d.npass = 0;
  for (const PPlan& pp : L.plan) {
    const int j = pp.first;
    int32_t* pm = d.k.pmeta[d.npass++];
    pm[kS2PmFirst] = j;
    if (!pp.block) {
      // a single-gate pass carries the gate's fields itself (S2Keep::pmeta): the kernel
      // reads a pass's whole head in one batch, ahead of the pass
      const S2Gate& G = d.gate[j];
      pm[kS2PmCount] = 1 | ((G.K * 16 + G.N) << 8);
      pm[kS2PmB] = 0;
      pm[kS2PmPass] = (int32_t)G.pass_mask;
      for (int k = 0; k < kS2MaxK; ++k) pm[kS2PmAddr + k] = k < G.K ? G.kaddr[k] : 0;
      for (int n = 0; n < kS2MaxKN; ++n) pm[kS2PmCode + n] = n < G.N ? G.naddr[n] : 0;
      group_lut(L, pp.order, d.k.lut[j]);
      continue;
    }
    pm[kS2PmPass] = (int32_t)pp.mask;
    if (pp.lanes) {
      pm[kS2PmCount] = (int)pp.ops.size();
      pm[kS2PmB] = 4 | kS2PmLanes;
      for (int b = 0; b < 4; ++b) {
        pm[kS2PmAddr + b] = addr(pp.reg0[b]);
        pm[kS2PmAddrEnd + b] = addr(pp.reg1[b]);
      }
      pm[kS2PmLaneDelta] = addr(pp.ln0[0]) ^ addr(pp.ln1[0]);
      pm[kS2PmLaneDelta + 1] = addr(pp.ln0[1]) ^ addr(pp.ln1[1]);
      for (size_t t = 0; t < pp.ops.size(); ++t) {
        const auto& o = pp.ops[t];
        pm[kS2PmCode + (int)t] = o[0] < 0 ? (kS2SwapCode | (o[1] << 2) | o[2]) : gate_code(d, o[0], o[1], o[2]);
      }
    } else {
      pm[kS2PmCount] = pp.end - pp.first;
      pm[kS2PmB] = B;
      int bp[4], nb = 0;
      for (int q = 0; q < kS2MaxPos; ++q)
        if ((pp.bm >> q) & 1) bp[nb++] = q;
      for (int b = 0; b < B; ++b) pm[kS2PmAddr + b] = pm[kS2PmAddrEnd + b] = addr(bp[b]);
      pm[kS2PmLaneDelta] = pm[kS2PmLaneDelta + 1] = 0;
      auto local = [&](int pos) {
        for (int b = 0; b < B; ++b) if (bp[b] == pos) return b;
        return -1;
      };
      for (int q = pp.first; q < pp.end; ++q) {
        // index bit t of the gate <-> position of input k = 1 << t
        const int i0 = local(__builtin_ctz((uint32_t)L.kdep[q][1]));
        const int j0 = d.gate[q].K == 4 ? local(__builtin_ctz((uint32_t)L.kdep[q][2])) : -1;
        pm[kS2PmCode + (q - pp.first)] = gate_code(d, q, i0, j0);
      }
    }
    group_lut(L, pp.order, d.k.lut[j]);
  }
  // group tables by pass (row p = the table of pass p's first gate): the kernel reads a
  // pass's row without first reading which gate starts it
  for (int q = 0; q < d.npass; ++q) {
    const int g = d.k.pmeta[q][kS2PmFirst];
    if (g != q) std::copy(d.k.lut[g], d.k.lut[g] + 64, d.k.lut[q]);
  }
  return true;
}

// Barriers between passes (kS2PmSync, bit 16 of a pass's count word: the workgroup barrier
// before that pass).  Thread t of the 512 takes the groups gi = t (mod 512) in every pass
// (tq_sweep2.hip gate_pass_u / block_pass), so wave w owns the groups whose gi bits 6..8
// (kS2WaveBits .. kS2LogThreads - 1, asserted in the kernel) are
// w, i.e. the elements whose address bits behind those group bits (columns below logC, then
// the pass's group positions in its order) are w.  Two consecutive passes with the same
// wave-select address bits leave every element with one wave: no barrier between them (LDS
// accesses of one wave complete in order; a lane block's swaps stay inside the wave: its
// lane bits are group bits 4 and 5).
void fill_sync(Layout& L) {
  S2Desc& d = L.d;
  auto wave_sig = [&](int q) {
    const std::vector<int>& order = L.plan[q].order;
    const int lg = d.logC + (int)order.size();   // log2 groups
    std::vector<int> sig;
    for (int b = kS2WaveBits; b < kS2LogThreads && b < lg; ++b)
      sig.push_back(b < d.logC ? -1 - b : order[b - d.logC]);
    return sig;
  };
  d.nsync = 0;
  for (int q = 0; q < d.npass; ++q) {
    const bool sync = q == 0 || !s2_wave_local() || wave_sig(q) != wave_sig(q - 1);
    if (sync) d.k.pmeta[q][kS2PmCount] |= kS2PmSync;
    d.nsync += sync;
  }
}

uint32_t or_all(const std::vector<int>& v) {
  uint32_t m = 0;
  for (int b : v) m |= (uint32_t)b;
  return m;
}

// TQ_S2_DUMP: the op's passes
void dump_passes(const Layout& L) {
  const S2Desc& d = L.d;
  fprintf(stderr, "s2 op: %d gates, %d passes, logC %d, used %d:", d.ngates, d.npass, d.logC, L.used);
  auto gate_pos = [&](int g) {
    const uint32_t m = L.kmask[g] | or_all(L.ndep[g]);
    fprintf(stderr, " %dx%d:", d.gate[g].K, d.gate[g].N);
    for (int b = 0; b < 16; ++b) if ((m >> b) & 1) fprintf(stderr, "%d", b);
  };
  for (const PPlan& pp : L.plan) {
    fprintf(stderr, " |%s", pp.lanes ? "L" : "");
    if (pp.lanes) {
      for (const auto& o : pp.ops) {
        if (o[0] < 0) fprintf(stderr, " s%d%d", o[1] + 4, o[2]);
        else gate_pos(o[0]);
      }
    } else {
      for (int g = pp.first; g < pp.end; ++g) gate_pos(g);
    }
  }
  fprintf(stderr, "\n");
}

// TQ_DEBUG_S2: the enumerations, swizzle vectors and gates
void dump_layout(const Layout& L) {
  const S2Desc& d = L.d;
  fprintf(stderr, "S2 cols=2^%d logC=%d used=%d epi=%d ld:", d.colbits, d.logC, L.used, d.epi);
  for (int t = 0; t < d.nld; ++t) fprintf(stderr, " %lld/%x", (long long)d.ld_w[t], d.ld_code[t]);
  fprintf(stderr, " | st:");
  for (int t = 0; t < d.nst; ++t) fprintf(stderr, " %lld/%x", (long long)d.st_w[t], d.st_code[t]);
  fprintf(stderr, " | vsw:");
  for (int p = 0; p < kS2MaxPos; ++p) fprintf(stderr, " %d", d.vsw[p]);
  fprintf(stderr, " | gates:");
  for (int j = 0; j < L.ngates(); ++j)
    fprintf(stderr, " [K%d N%d pass%x in%x out%x]", d.gate[j].K, d.gate[j].N, d.gate[j].pass_mask, L.kmask[j],
            or_all(L.ndep[j]));
  fprintf(stderr, "\n");
}

}  // namespace

// Layout of an in-place butterfly sweep (tq_sweep2.hip): every mode bit of the working set
// gets a tile position, the columns are the untouched mode bits ordered by stride, and a
// per-position XOR swizzle keeps the half-wave LDS accesses of the load / store phases and of
// the passes conflict-free.  False if the chain does not fit.
bool s2_layout(const S2Ctx& x, const Chain& c, const ChainShape& sh, const std::vector<int>& out_modes,
               S2Desc* out, bool one_chunk) {
  if (!s2_enabled() || c.gates.empty() || (int)c.gates.size() > kS2MaxGates) return false;
  Layout L{x, c, sh, out_modes};
  if (!assign_positions(L)) return false;
  if (!out) return true;
  if (!choose_columns(L, one_chunk)) return false;
  build_enumerations(L);
  block_params(L);
  choose_epilogue(L);
  L.plan = plan_passes(L, L.ngates() - (L.d.epi ? 1 : 0));   // the epilogue gate is no pass
  choose_swizzle(L);
  if (!fill_addresses(L)) return false;
  fill_gates(L);
  if (!fill_passes(L)) return false;
  fill_sync(L);
  if (s2_dump()) dump_passes(L);
  if (env_set("TQ_DEBUG_S2")) dump_layout(L);
  *out = L.d;
  return true;
}

// ---- inspectors of a compiled plan's sweep2 descriptors ----------------------------------------
namespace {
// every descriptor of the plan's (non-dense) sweep2 ops: fn(op, descriptor, is the op's default layout)
template <typename PlanT, typename F>
void for_s2_descs(PlanT& P, F fn) {
  for (auto& op : P.ops) {
    if (op.kind != OP_SWEEP2 || op.s2_dense || op.stab < 0) continue;
    using D = typename std::conditional<std::is_const<PlanT>::value, const S2Desc, S2Desc>::type;
    fn(op, *reinterpret_cast<D*>(P.stabs[op.stab].data()), true);
    if (op.stab1 >= 0 && op.stab1 != op.stab) fn(op, *reinterpret_cast<D*>(P.stabs[op.stab1].data()), false);
  }
}
bool s2_plain_block(const int32_t* pm) {
  return (pm[kS2PmB] & 0xff) != 0 && !(pm[kS2PmB] & kS2PmLanes);
}
}  // namespace

void plan_s2_programs(Plan& P, bool on) {
  P.use_s2_prog = on;
  for_s2_descs(P, [&](Op&, S2Desc& d, bool) {
    for (int p = 0; p < d.npass; ++p) {
      int32_t* pm = d.k.pmeta[p];
      if (!s2_plain_block(pm)) continue;
      const int B = pm[kS2PmB] & 0xff;
      pm[kS2PmB] = B | (on ? s2_prog_bits(B, pm + kS2PmCode, pm[kS2PmCount] & 0xff) : 0);
    }
  });
  if (P.whole) plan_s2_programs(*P.whole, on);
}

int64_t plan_s2_prog_passes(const Plan& P, int id) {
  int64_t n = 0;
  for_s2_descs(P, [&](const Op&, const S2Desc& d, bool) {
    for (int p = 0; p < d.npass; ++p)
      n += s2_plain_block(d.k.pmeta[p]) && ((d.k.pmeta[p][kS2PmB] >> kS2ProgShift) & 0xff) == id;
  });
  return n;
}

int64_t plan_s2_gate_work(const Plan& P, bool programs_only) {
  double w = 0;
  std::map<std::string, double> hist;
  const bool dump = s2_dump() && !programs_only;
  for_s2_descs(P, [&](const Op& op, const S2Desc& d, bool dflt) {
    if (!dflt) return;
    for (int p = 0; p < d.npass; ++p) {
      const int32_t* pm = d.k.pmeta[p];
      if (!s2_plain_block(pm)) continue;
      const int B = pm[kS2PmB] & 0xff, cnt = pm[kS2PmCount] & 0xff;
      const double elems = (double)((int64_t(1) << d.logC) << (__builtin_popcount((uint32_t)pm[kS2PmPass]) + B));
      const double pw = cnt * elems * (double)d.nchunks * (op.invariant ? 1 : P.lanes);
      if (!programs_only || ((pm[kS2PmB] >> kS2ProgShift) & 0xff)) w += pw;
      if (dump) {
        std::string key = "B" + std::to_string(B) + " id" + std::to_string((pm[kS2PmB] >> kS2ProgShift) & 0xff) + ":";
        for (int q = 0; q < cnt; ++q) {
          const int c = pm[kS2PmCode + q];
          key += " " + std::to_string(c & 3) + ((c & 16) ? std::to_string((c >> 2) & 3) : std::string());
        }
        hist[key] += pw;
      }
    }
  });
  if (dump) {
    std::vector<std::pair<double, std::string>> v;
    for (auto& h : hist) v.push_back({h.second, h.first});
    std::sort(v.rbegin(), v.rend());
    for (auto& h : v) fprintf(stderr, "s2 block gate work %.4f  %s\n", w > 0 ? h.first / w : 0.0, h.second.c_str());
  }
  return (int64_t)w;
}

}  // namespace tq
