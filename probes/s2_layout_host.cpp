// Host harness of the sweep-chain layout planner: links tq_sweep2_layout.cpp and nothing else of
// the library, builds synthetic chains on tensors of extent-2 modes (brick-wall layers of 4x4
// gates on adjacent modes, a 2x2 gate, one expanding last gate K = 2, N = 4), lays them out for
// element sizes 4 / 8 / 16 and checks every accepted descriptor for what needs no GPU.  Built and
// run by `make -C csrc host-check` under ASan + UBSan (CPU only).  TQ_S2_LANEBLK=1 needs a run of
// its own: the knob is read once per process.
#include "tq_sweep2_layout.h"

#include "tq_plan_internal.h"

#include <cstdio>
#include <cstring>
#include <map>
#include <vector>

using namespace tq;

namespace {

int g_fail = 0;
#define CHECK(cond, ...)                                       \
  do {                                                         \
    if (!(cond)) {                                             \
      ++g_fail;                                                \
      fprintf(stderr, "FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); \
      fprintf(stderr, __VA_ARGS__);                            \
      fprintf(stderr, "\n");                                   \
    }                                                          \
  } while (0)

struct Counts { int tried = 0, accepted = 0, plain_block = 0, epilogue = 0, relisted = 0, one_chunk = 0, lanes = 0; };

// a chain under construction: the tensor's current mode order, every mode of extent 2
struct Builder {
  std::map<int, int64_t> ext;
  Chain c;
  std::vector<int> cur;
  int next = 0;
  explicit Builder(int nmodes) {
    for (int m = 0; m < nmodes; ++m) { cur.push_back(m); ext[m] = 2; }
    next = nmodes;
    c.active = true;
    c.X0.modes = cur;
    c.X0.ext.assign(nmodes, 2);
    c.X0.stride = contig_strides(c.X0.ext);
    c.X0.buf.kind = BUF_INPUT;
  }
  // a gate contracting the nk adjacent modes at `at` into nn new ones in their place
  void gate(int at, int nk, int nn) {
    Chain::Gate g;
    ApplyDesc& d = g.d;
    d.korder.assign(cur.begin() + at, cur.begin() + at + nk);
    for (int q = 0; q < nn; ++q) { d.nfree.push_back(next); ext[next++] = 2; }
    cur.erase(cur.begin() + at, cur.begin() + at + nk);
    cur.insert(cur.begin() + at, d.nfree.begin(), d.nfree.end());
    d.order = cur;
    d.K = int64_t(1) << nk;
    d.N = int64_t(1) << nn;
    g.Sm.modes = d.korder;
    g.Sm.modes.insert(g.Sm.modes.end(), d.nfree.begin(), d.nfree.end());
    g.Sm.ext.assign(g.Sm.modes.size(), 2);
    g.Sm.stride = contig_strides(g.Sm.ext);
    g.Sm.buf.kind = BUF_INPUT;
    g.step = (int)c.gates.size();
    c.gates.push_back(g);
    c.out_modes = cur;
  }
  // brick-wall layers of 4x4 gates over modes [lo, hi): even layers start at lo, odd at lo + 1
  void brick_wall(int lo, int hi, int layers) {
    for (int l = 0; l < layers; ++l)
      for (int at = lo + (l & 1); at + 2 <= hi; at += 2) gate(at, 2, 2);
  }
};

// what can be checked of an accepted layout without a GPU
void check_desc(const S2Desc& d, size_t esz, const char* what, Counts& n) {
  CHECK(d.nld >= 0 && d.nld <= 16 && d.nst >= 0 && d.nst <= 16, "%s: nld %d nst %d", what, d.nld, d.nst);
  CHECK(d.ngates >= 1 && d.ngates <= kS2MaxGates, "%s: ngates %d", what, d.ngates);
  CHECK(d.npass >= 0 && d.npass <= kS2MaxGates, "%s: npass %d", what, d.npass);
  CHECK(d.logC >= 0 && d.logC <= d.colbits && d.nchunks == (int64_t(1) << (d.colbits - d.logC)), "%s: chunks", what);
  // positions in use: the highest position bit of any gate input / output or enumeration code
  uint32_t posm = 0;
  for (int g = 0; g < d.ngates; ++g) {
    for (int k = 0; k < d.gate[g].K; ++k) posm |= (uint32_t)d.gate[g].kdep[k];
    for (int k = 0; k < d.gate[g].N; ++k) posm |= (uint32_t)d.gate[g].ndep[k];
  }
  for (int t = 0; t < d.nld && t < 16; ++t) posm |= ((uint32_t)d.ld_code[t] >> kS2CodeP) & ((1u << kS2MaxPos) - 1);
  for (int t = 0; t < d.nst && t < 16; ++t) posm |= ((uint32_t)d.st_code[t] >> kS2CodeP) & ((1u << kS2MaxPos) - 1);
  int used = 0;
  while (used < kS2MaxPos && (posm >> used)) ++used;
  CHECK((posm >> kS2MaxPos) == 0, "%s: position mask %x", what, posm);
  const int lt = d.logC + used;   // log2 tile elements
  CHECK(lt <= s2_chunk_bits((int)esz), "%s: tile 2^%d", what, lt);
  if (lt > s2_chunk_bits((int)esz)) return;
  // the tile address map ((p << logC) | c) ^ S(p) is a bijection of the tile
  std::vector<char> hit(size_t(1) << lt, 0);
  bool bij = true;
  for (int p = 0; p < (1 << used); ++p) {
    int s = 0;
    for (int q = 0; q < used; ++q) if ((p >> q) & 1) s ^= d.vsw[q];
    for (int c = 0; c < (1 << d.logC); ++c) {
      const int a = ((p << d.logC) | c) ^ s;
      if (a < 0 || a >= (1 << lt) || hit[a]) { bij = false; continue; }
      hit[a] = 1;
    }
  }
  CHECK(bij, "%s: the swizzled tile map is no bijection (logC %d, used %d)", what, d.logC, used);
  const int64_t tile_bytes = (int64_t(1) << lt) * (int64_t)esz;
  const int rows = d.npass > d.ngates ? d.npass : d.ngates;
  for (int r = 0; r < rows && r < kS2MaxGates; ++r)
    for (int j = 0; j < 64; ++j)
      CHECK(d.k.lut[r][j] >= 0 && d.k.lut[r][j] < tile_bytes, "%s: lut[%d][%d] = %d", what, r, j, d.k.lut[r][j]);
  bool plain = false, lanes = false;
  for (int p = 0; p < d.npass && p < kS2MaxGates; ++p) {
    const int32_t* pm = d.k.pmeta[p];
    const int first = pm[kS2PmFirst], B = pm[kS2PmB] & 0xff, cnt = pm[kS2PmCount] & 0xff;
    CHECK(first >= 0 && first < d.ngates, "%s: pass %d starts at gate %d of %d", what, p, first, d.ngates);
    if (B == 0) { CHECK(cnt == 1, "%s: single-gate pass of %d gates", what, cnt); continue; }
    CHECK(cnt >= 1 && cnt <= kS2BlkMaxGates, "%s: block of %d codes", what, cnt);
    if (pm[kS2PmB] & kS2PmLanes) { lanes = true; continue; }
    plain = true;
    CHECK(first + cnt <= d.ngates, "%s: pass %d gates [%d, %d) of %d", what, p, first, first + cnt, d.ngates);
  }
  CHECK(d.epi == 0 || d.epi == d.ngates, "%s: epi %d", what, d.epi);
  // the blob: its size is what its own offsets imply
  const std::vector<char> blob = s2_blob(d, esz);
  S2Desc b;
  CHECK(blob.size() >= sizeof(S2Desc), "%s: blob of %zu bytes", what, blob.size());
  if (blob.size() < sizeof(S2Desc)) return;
  std::memcpy(&b, blob.data(), sizeof(S2Desc));
  const size_t lanes_end = (size_t)b.aux_lanes + (size_t(1) << kS2LogThreads) * 16;
  CHECK(b.aux_lanes >= (int)sizeof(S2Desc) && b.aux_lanes % 16 == 0, "%s: aux_lanes %d", what, b.aux_lanes);
  if (b.aux_cb) {
    CHECK((size_t)b.aux_cb == lanes_end && blob.size() == (size_t)b.aux_cb + (size_t)b.nchunks * 16,
          "%s: blob %zu, aux_cb %d, %lld chunks", what, blob.size(), b.aux_cb, (long long)b.nchunks);
  } else {
    CHECK(blob.size() == lanes_end && b.nchunks > kS2MaxCbTab, "%s: blob %zu without a chunk table", what, blob.size());
  }
  ++n.accepted;
  n.plain_block += plain;
  n.lanes += lanes;
  n.epilogue += d.epi != 0;
  n.one_chunk += d.nchunks == 1;
}

// shape, layout, re-listing and the one-chunk form of one chain, as flush_chain asks for them
void run_chain(const char* name, Builder& b, int dtype, size_t esz, int group_hint, int min_chunks, bool one_chunk,
               Counts& n) {
  const S2Ctx x{dtype, esz, b.ext, 1, group_hint, min_chunks};
  char what[128];
  snprintf(what, sizeof what, "%s esz %zu group %d min_chunks %d%s", name, esz, group_hint, min_chunks,
           one_chunk ? " one-chunk" : "");
  ++n.tried;
  ChainShape sh;
  if (!chain_shape(x, b.c, b.c.out_modes, sh) || !sh.s2) return;
  S2Desc d;
  if (!s2_layout(x, b.c, sh, b.c.out_modes, &d, one_chunk)) return;
  check_desc(d, esz, what, n);
  Chain cr;
  if (s2_reorder_squares(x, b.c, cr, 4)) {
    ChainShape shr;
    S2Desc dr;
    CHECK(cr.gates.size() == b.c.gates.size(), "%s: re-listing changed the gate count", what);
    if (chain_shape(x, cr, cr.out_modes, shr) && shr.s2 && s2_layout(x, cr, shr, cr.out_modes, &dr, one_chunk)) {
      CHECK(shr.tin_n == sh.tin_n && shr.tout_n == sh.tout_n, "%s: re-listing changed the tiles", what);
      check_desc(dr, esz, what, n);
      ++n.relisted;
    }
  }
}

}  // namespace

int main() {
  const struct { int dtype; size_t esz; } types[] = {{TQ_F32, 4}, {TQ_C64, 8}, {TQ_C128, 16}};
  Counts n;
  for (auto& t : types) {
    // 10 modes, every one in the tile: the tile is the tensor, one chunk (9 modes: complex128's 9 positions)
    for (int nm : {9, 10}) {
      Builder b(nm);
      b.brick_wall(0, nm, 3);
      b.gate(nm - 1, 1, 1);
      run_chain(nm == 9 ? "9 modes" : "10 modes", b, t.dtype, t.esz, 1, 0, false, n);
    }
    // 13 modes, 9 in the tile, the slowest one doubled by the last gate: 4096-element tiles
    // (register blocks of 4 bits) when at least two chunks are asked for, and its one-chunk form
    {
      Builder b(13);
      b.brick_wall(0, 9, 3);
      b.gate(4, 1, 1);
      b.gate(0, 1, 2);
      run_chain("13 modes", b, t.dtype, t.esz, 1, 2, false, n);
      run_chain("13 modes", b, t.dtype, t.esz, 1, 0, false, n);
      run_chain("13 modes", b, t.dtype, t.esz, 1, 0, true, n);
    }
    // 19 modes, 6 in the tile: columns and the min-chunk rule
    for (int gh : {1, 4}) {
      Builder b(19);
      b.brick_wall(0, 6, 2);
      b.gate(2, 1, 1);
      b.gate(0, 1, 2);
      run_chain("19 modes", b, t.dtype, t.esz, gh, 0, false, n);
    }
  }
  printf("layouts tried %d accepted %d: plain block pass %d, epilogue %d, re-listed %d, one chunk %d, lane block %d\n",
         n.tried, n.accepted, n.plain_block, n.epilogue, n.relisted, n.one_chunk, n.lanes);
  CHECK(n.accepted > 0 && n.plain_block > 0 && n.epilogue > 0 && n.relisted > 0 && n.one_chunk > 0,
        "a kind of layout the chains were chosen for did not occur");
  CHECK((n.lanes > 0) == s2_lane_blocks(), "lane blocks: %d layouts with TQ_S2_LANEBLK %d", n.lanes, (int)s2_lane_blocks());
  if (g_fail) fprintf(stderr, "%d checks failed\n", g_fail);
  return g_fail ? 1 : 0;
}
