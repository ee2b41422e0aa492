// The k most probable elements of a block of amplitudes on the device (post-selection): the
// other consumer of tq_plan_execute's output, next to the Born-rule sampler (tq_born.hip).  The
// reference has no counterpart; the nearest thing is EngineSiamese.sample
// (tneq_qc/core/engine_siamese.py:740-915).  Without this entry point a user copies every 8 MB
// block to the host, or chains widen / square / add / topk / gather through three block-sized
// float64 temporaries.
//
//     p_i = re(a_i)^2 + im(a_i)^2 (float64, complex64 widened first, no FP contraction)
//     key_i = the bits of p_i as uint64 when p_i > 0, else 0 (p >= +0, so the bit pattern keeps
//             the order; +inf is the largest key; NaN and 0 are no candidates)
//     result = the first k candidates by (key descending, index ascending)
//
// A radix select of the k-th largest key T from the most significant digit down, then a gather
// and a sort; nine launches whatever the data:
//  * topk_zero    — zeroes the five histograms and the gather counter, seeds the select state.
//  * topk_hist x5 — digit d of the keys that match the digits chosen so far: bits 62..52 (the
//    exponent, 2048 bins), then four mantissa digits of 13 bits (8192 bins).  A workgroup covers
//    a contiguous span; it counts in an LDS histogram (a lane merges equal consecutive digits
//    before it touches LDS: an all-equal block costs one LDS atomic per lane, not sixteen) and adds
//    only its occupied bins to the global one.  Picking the bin of digit d - 1 is the prologue of
//    pass d (every workgroup walks the same histogram to the same answer; workgroup 0 records
//    it), not a launch of its own.  Random-circuit amplitudes share a handful of exponents, so
//    the first digit discriminates poorly and the first mantissa digit does the work; from the
//    third pass on almost nothing matches and a pass is one read of the block.
//  * topk_gather  — picks the last digit (T is complete), appends every element with key > T to
//    the candidate list (fewer than k of them, slots from one integer counter) and writes each
//    workgroup's count of key == T.
//  * topk_ties    — the k - #(key > T) ties of lowest index: a workgroup's base is the sum of the
//    tie counts of the workgroups before it, ranks inside it come from scans in index order.
//    Only workgroups that hold a tie below the cut read anything.
//  * topk_sort    — one workgroup: a bitonic sort of the at most 4096 (key, index) pairs in LDS
//    by (key descending, index ascending), then index -> word, key -> probability, the -1 / 0
//    padding and the count.
//
// Deterministic: every count is an integer (atomics commute), so T, the tie quota and the SET of
// survivors are fixed by the data; the order they were appended in is not, and the sort's total
// order (indices are distinct) removes it.  Fewer than k candidates: the first pick finds no bin,
// the select state says "all" (T = 0, no ties), the later passes return at once and the gather
// takes every key > 0.
#include "tq_born_common.h"

namespace tq {

namespace {

constexpr int kTkNT = 256;                    // lanes per workgroup of the passes over the block
constexpr int kTkPL = 16;                     // elements per lane and tile
constexpr int kTkTile = kTkNT * kTkPL;        // 4096
constexpr int kTkMaxBlocks = 1024;            // spans: at most this many workgroups per pass
constexpr int kTkDigits = 5;
constexpr int kTkMaxBins = 8192;
constexpr int kTkSortNT = 1024;
constexpr int kTkHistWords = 2048 + 4 * kTkMaxBins;

__host__ __device__ constexpr int tk_shift(int d) { return d == 0 ? 52 : 13 * (4 - d); }
__host__ __device__ constexpr int tk_width(int d) { return d == 0 ? 11 : 13; }
__host__ __device__ constexpr int tk_hist_off(int d) { return d == 0 ? 0 : 2048 + (d - 1) * kTkMaxBins; }

// the select before digit d: the digits chosen so far (as a number) and how many elements are
// still to be taken among the keys that start with them; krem = 0: every candidate is taken
struct TkState {
  uint64_t prefix;
  int64_t krem;
};

struct TkWs {
  TkState* state;      // [kTkDigits + 1]
  uint64_t* ckey;      // [k]  survivors, in no particular order
  uint32_t* ngt;       // [2]  number of keys > T appended (word 1 pads); the histograms follow
  uint32_t* hist;      // [kTkHistWords]
  uint32_t* tiecnt;    // [kTkMaxBlocks]  keys == T per workgroup
  uint32_t* cidx;      // [k]
};

inline size_t topk_ws_bytes(int64_t k) {
  const size_t b = sizeof(TkState) * (kTkDigits + 1) + (size_t)k * 8 +
                   4 * (size_t)(2 + kTkHistWords + kTkMaxBlocks) + (size_t)k * 4;
  return (b + 15) & ~(size_t)15;
}

inline TkWs topk_ws(void* ws, int64_t k) {
  TkWs w;
  w.state = reinterpret_cast<TkState*>(ws);
  w.ckey = reinterpret_cast<uint64_t*>(w.state + kTkDigits + 1);
  w.ngt = reinterpret_cast<uint32_t*>(w.ckey + k);
  w.hist = w.ngt + 2;
  w.tiecnt = w.hist + kTkHistWords;
  w.cidx = w.tiecnt + kTkMaxBlocks;
  return w;
}

// workgroup b covers elements [b span, min(n, (b + 1) span)); span is a multiple of the tile
struct TkGeom {
  int64_t span;
  int nblk;
};

inline TkGeom topk_geom(int64_t n) {
  const int64_t tiles = (n + kTkTile - 1) / kTkTile;
  const int64_t per = (tiles + kTkMaxBlocks - 1) / kTkMaxBlocks;
  TkGeom g;
  g.span = per * kTkTile;
  g.nblk = (int)((n + g.span - 1) / g.span);
  return g;
}

__device__ __forceinline__ uint64_t tk_key(double p) {
  return p > 0.0 ? (uint64_t)__double_as_longlong(p) : (uint64_t)0;
}

// tile element of a lane's j-th key (16-B loads: a lane holds runs of 16 / sizeof(T) elements)
template <typename T>
__device__ __forceinline__ int tk_elem(int j, int tid) {
  constexpr int EPL = 16 / (int)sizeof(T);
  return (j / EPL) * (kTkNT * EPL) + tid * EPL + (j % EPL);
}

// the lane's 16 keys of the tile at `a` (rem = elements from `a` to the end of the block;
// elements beyond it give key 0)
template <typename T, bool VEC>
__device__ __forceinline__ void tk_load(const T* __restrict__ a, int64_t rem, int tid,
                                        uint64_t (&key)[kTkPL]) {
#pragma clang fp contract(off)
  constexpr int EPL = 16 / (int)sizeof(T);
  constexpr int NLD = kTkPL / EPL;
#pragma unroll
  for (int j = 0; j < NLD; ++j) {
    const int e = j * (kTkNT * EPL) + tid * EPL;
    if constexpr (VEC && EPL == 2) {
      if (e + 2 <= rem) {
        const float4 q = *reinterpret_cast<const float4*>(a + e);
        const double r0 = (double)q.x, i0 = (double)q.y, r1 = (double)q.z, i1 = (double)q.w;
        key[2 * j] = tk_key(r0 * r0 + i0 * i0);
        key[2 * j + 1] = tk_key(r1 * r1 + i1 * i1);
        continue;
      }
    }
    if constexpr (VEC && EPL == 1) {
      if (e < rem) {
        const double2 q = *reinterpret_cast<const double2*>(a + e);
        key[j] = tk_key(q.x * q.x + q.y * q.y);
        continue;
      }
    }
#pragma unroll
    for (int x = 0; x < EPL; ++x)
      key[j * EPL + x] = (e + x < rem) ? tk_key(born_p<T>(a, e + x)) : (uint64_t)0;
  }
}

struct TkScanLds {
  uint32_t w[kTkNT / 64];
  uint64_t res[2];
};

// exclusive prefix of v over the workgroup's lanes in lane order; the total to every lane
__device__ __forceinline__ uint32_t tk_excl_scan(uint32_t v, uint32_t& total, TkScanLds& S) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(inc, o);
    if (lane >= o) inc += t;
  }
  __syncthreads();   // the previous scan's wave totals have been read
  if (lane == 63) S.w[wv] = inc;
  __syncthreads();
  uint32_t off = 0, tot = 0;
#pragma unroll
  for (int x = 0; x < kTkNT / 64; ++x) {
    if (x == wv) off = tot;
    tot += S.w[x];
  }
  total = tot;
  return off + inc - v;
}

// The next select state from the histogram of the digit just counted: walking the bins from the
// top, the bin in which the running count reaches prev.krem.  Every lane of the workgroup calls
// it and gets the same answer; no bin (fewer candidates than wanted) gives "all" = {0, 0}.
__device__ __forceinline__ TkState tk_pick(const TkState prev, const uint32_t* __restrict__ hist,
                                           int width, TkScanLds& S) {
  if (prev.krem <= 0) return TkState{0, 0};
  const int nb = 1 << width, per = nb / kTkNT;
  const int tid = threadIdx.x;
  const int hi = nb - 1 - tid * per;     // lane 0 holds the top bins
  uint32_t s = 0;
  for (int b = 0; b < per; ++b) s += hist[hi - b];
  uint32_t total;
  const uint32_t excl = tk_excl_scan(s, total, S);
  const uint32_t kr = (uint32_t)prev.krem;
  if (tid == 0) {
    S.res[0] = 0;
    S.res[1] = 0;
  }
  __syncthreads();
  if (excl < kr && excl + s >= kr) {     // exactly one lane: the running count is monotone
    uint32_t acc = excl;
    for (int b = 0; b < per; ++b) {
      const uint32_t h = hist[hi - b];
      if (acc + h >= kr) {
        S.res[0] = (prev.prefix << width) | (uint64_t)(hi - b);
        S.res[1] = kr - acc;
        break;
      }
      acc += h;
    }
  }
  __syncthreads();
  return TkState{S.res[0], (int64_t)S.res[1]};
}

__global__ void __launch_bounds__(kTkNT) topk_zero(TkWs W, int64_t k) {
  const int i = blockIdx.x * kTkNT + threadIdx.x;
  if (i < 2 + kTkHistWords) W.ngt[i] = 0;   // the counter, its pad and the histograms behind them
  if (i == 0) W.state[0] = TkState{0, k};
}

template <typename T, bool VEC>
__global__ void __launch_bounds__(kTkNT)
topk_hist(const T* __restrict__ amps, int64_t n, int64_t span, int d, TkWs W) {
  __shared__ uint32_t h[kTkMaxBins];
  __shared__ TkScanLds S;
  const int tid = threadIdx.x;
  TkState st;
  if (d == 0) {
    st = W.state[0];
  } else {
    st = tk_pick(W.state[d - 1], W.hist + tk_hist_off(d - 1), tk_width(d - 1), S);
    if (blockIdx.x == 0 && tid == 0) W.state[d] = st;
  }
  if (st.krem <= 0) return;
  const int shift = tk_shift(d), width = tk_width(d), nb = 1 << width;
  for (int b = tid; b < nb; b += kTkNT) h[b] = 0;
  __syncthreads();
  const int64_t e0 = (int64_t)blockIdx.x * span;
  const int64_t e1 = e0 + span < n ? e0 + span : n;
  int cur = 0;
  uint32_t run = 0;
  for (int64_t t0 = e0; t0 < e1; t0 += kTkTile) {
    uint64_t key[kTkPL];
    tk_load<T, VEC>(amps + t0, n - t0, tid, key);
#pragma unroll
    for (int j = 0; j < kTkPL; ++j) {
      const uint64_t x = key[j];
      if (x != 0 && (x >> (shift + width)) == st.prefix) {
        const int dg = (int)((x >> shift) & (uint64_t)(nb - 1));
        if (dg != cur) {
          if (run) atomicAdd(&h[cur], run);
          cur = dg;
          run = 0;
        }
        ++run;
      }
    }
  }
  if (run) atomicAdd(&h[cur], run);
  __syncthreads();
  uint32_t* __restrict__ g = W.hist + tk_hist_off(d);
  for (int b = tid; b < nb; b += kTkNT) {
    const uint32_t c = h[b];
    if (c) atomicAdd(&g[b], c);
  }
}

template <typename T, bool VEC>
__global__ void __launch_bounds__(kTkNT)
topk_gather(const T* __restrict__ amps, int64_t n, int64_t span, int64_t k, TkWs W) {
  __shared__ TkScanLds S;
  const int tid = threadIdx.x;
  const TkState st = tk_pick(W.state[kTkDigits - 1], W.hist + tk_hist_off(kTkDigits - 1),
                             tk_width(kTkDigits - 1), S);
  if (blockIdx.x == 0 && tid == 0) W.state[kTkDigits] = st;
  const uint64_t thr = st.prefix;       // 0: fewer than k candidates, every key > 0 is taken
  const int64_t e0 = (int64_t)blockIdx.x * span;
  const int64_t e1 = e0 + span < n ? e0 + span : n;
  uint32_t ties = 0;
  for (int64_t t0 = e0; t0 < e1; t0 += kTkTile) {
    uint64_t key[kTkPL];
    tk_load<T, VEC>(amps + t0, n - t0, tid, key);
#pragma unroll
    for (int j = 0; j < kTkPL; ++j) {
      const uint64_t x = key[j];
      if (x > thr) {
        const uint32_t slot = atomicAdd(W.ngt, 1u);
        if (slot < (uint64_t)k) {
          W.ckey[slot] = x;
          W.cidx[slot] = (uint32_t)(t0 + tk_elem<T>(j, tid));
        }
      } else if (x == thr && thr != 0) {
        ++ties;
      }
    }
  }
  uint32_t total;
  tk_excl_scan(ties, total, S);
  if (tid == 0) W.tiecnt[blockIdx.x] = total;
}

template <typename T>
__global__ void __launch_bounds__(kTkNT)
topk_ties(const T* __restrict__ amps, int64_t n, int64_t span, int64_t k, TkWs W) {
  __shared__ TkScanLds S;
  const int tid = threadIdx.x;
  const TkState st = W.state[kTkDigits];
  const uint64_t thr = st.prefix;
  const uint32_t want = (uint32_t)st.krem;
  if (thr == 0 || want == 0) return;
  const int blk = blockIdx.x;
  if (W.tiecnt[blk] == 0) return;
  uint32_t s = 0;
  for (int i = tid; i < blk; i += kTkNT) s += W.tiecnt[i];
  uint32_t run;                           // ties before this workgroup, then before this step
  tk_excl_scan(s, run, S);
  if (run >= want) return;
  const uint32_t ngt = W.ngt[0];
  const int64_t e0 = (int64_t)blk * span;
  const int64_t e1 = e0 + span < n ? e0 + span : n;
  for (int64_t t0 = e0; t0 < e1 && run < want; t0 += kTkNT) {
    const int64_t i = t0 + tid;
    const bool tie = i < e1 && tk_key(born_p<T>(amps, i)) == thr;
    uint32_t total;
    const uint32_t r = run + tk_excl_scan(tie ? 1u : 0u, total, S);
    if (tie && r < want) {
      const uint64_t slot = (uint64_t)ngt + r;
      if (slot < (uint64_t)k) {
        W.ckey[slot] = thr;
        W.cidx[slot] = (uint32_t)i;
      }
    }
    run += total;
  }
}

// a sorts before b: the larger key, then the smaller index
__device__ __forceinline__ bool tk_before(uint64_t ka, uint32_t ia, uint64_t kb, uint32_t ib) {
  return ka > kb || (ka == kb && ia < ib);
}

__global__ void __launch_bounds__(kTkSortNT)
topk_sort(int64_t k, int P, TkWs W, int64_t* __restrict__ index, double* __restrict__ prob,
          int64_t* __restrict__ count, int n_axes, BornAxes ax, uint64_t base) {
  __shared__ uint64_t sk[TQ_BORN_TOPK_MAX_K];
  __shared__ uint32_t si[TQ_BORN_TOPK_MAX_K];
  const int tid = threadIdx.x;
  const TkState st = W.state[kTkDigits];
  uint64_t have = (uint64_t)W.ngt[0] + (st.prefix != 0 ? (uint64_t)st.krem : (uint64_t)0);
  const int m = (int)(have < (uint64_t)k ? have : (uint64_t)k);
  for (int i = tid; i < P; i += kTkSortNT) {
    sk[i] = i < m ? W.ckey[i] : (uint64_t)0;
    si[i] = i < m ? W.cidx[i] : 0xffffffffu;
  }
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int t = tid; t < (P >> 1); t += kTkSortNT) {
        const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
        const uint64_t ka = sk[lo], kb = sk[hi];
        const uint32_t ia = si[lo], ib = si[hi];
        const bool up = (lo & size) == 0;
        if (up ? tk_before(kb, ib, ka, ia) : tk_before(ka, ia, kb, ib)) {
          sk[lo] = kb;
          si[lo] = ib;
          sk[hi] = ka;
          si[hi] = ia;
        }
      }
    }
  }
  __syncthreads();
  for (int j = tid; j < k; j += kTkSortNT) {
    index[j] = j < m ? born_word((int64_t)si[j], n_axes, ax, base) : (int64_t)-1;
    prob[j] = j < m ? __longlong_as_double((long long)sk[j]) : 0.0;
  }
  if (tid == 0) count[0] = m;
}

template <typename T, bool VEC>
int topk_t(int64_t n, const void* amps, int64_t k, int64_t* index, double* prob, int64_t* count,
           int n_axes, const BornAxes& ax, uint64_t base, void* ws, hipStream_t st) {
  const TkGeom g = topk_geom(n);
  const TkWs W = topk_ws(ws, k);
  const T* a = reinterpret_cast<const T*>(amps);
  const dim3 grid((unsigned)g.nblk), block(kTkNT);
  hipLaunchKernelGGL(topk_zero, dim3((2 + kTkHistWords + kTkNT - 1) / kTkNT), block, 0, st, W, k);
  TQ_HIP(hipGetLastError());
  for (int d = 0; d < kTkDigits; ++d) {
    hipLaunchKernelGGL((topk_hist<T, VEC>), grid, block, 0, st, a, n, g.span, d, W);
    TQ_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL((topk_gather<T, VEC>), grid, block, 0, st, a, n, g.span, k, W);
  TQ_HIP(hipGetLastError());
  hipLaunchKernelGGL((topk_ties<T>), grid, block, 0, st, a, n, g.span, k, W);
  TQ_HIP(hipGetLastError());
  int P = 1;
  while (P < k) P <<= 1;
  hipLaunchKernelGGL(topk_sort, dim3(1), dim3(kTkSortNT), 0, st, k, P, W, index, prob, count,
                     n_axes, ax, base);
  TQ_HIP(hipGetLastError());
  return TQ_OK;
}

}  // namespace

size_t born_topk_workspace(int dtype, int64_t n, int64_t k) {
  if (dtype != TQ_C64 && dtype != TQ_C128) {
    set_error("born_topk: amplitudes must be TQ_C64 or TQ_C128");
    return 0;
  }
  if (n < 1 || n > ((int64_t)1 << 31)) {
    set_error("born_topk: n must be in [1, 2^31]");
    return 0;
  }
  if (k < 1 || k > TQ_BORN_TOPK_MAX_K) {
    set_error("born_topk: k must be in [1, TQ_BORN_TOPK_MAX_K]");
    return 0;
  }
  return topk_ws_bytes(k);
}

int born_topk_launch(int dtype, int64_t n, const void* amps, int64_t k, int64_t* index, double* prob,
                     int64_t* count, int n_axes, const int32_t* axis_qubit, uint64_t base,
                     void* workspace, size_t ws_bytes, hipStream_t stream) {
  const size_t need = born_topk_workspace(dtype, n, k);
  if (need == 0) return TQ_ERR_INVALID;
  TQ_CHECK_ARG(amps && index && prob && count && workspace, "born_topk: null pointer");
  TQ_CHECK_ARG(ws_bytes >= need, "born_topk: workspace smaller than tq_born_topk_workspace");
  TQ_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "born_topk: workspace must be 8-byte aligned");
  TQ_CHECK_ARG((((uintptr_t)index | (uintptr_t)prob | (uintptr_t)count) & 7) == 0,
               "born_topk: index, prob and count must be 8-byte aligned");
  const size_t ralign = dtype == TQ_C64 ? 4 : 8;
  TQ_CHECK_ARG(((uintptr_t)amps & (ralign - 1)) == 0, "born_topk: misaligned amplitudes");
  BornAxes ax{};
  int na = -1;
  TQ_TRY(born_axes("born_topk", n, n_axes, axis_qubit, base, ax, na));
  const bool vec = ((uintptr_t)amps & 15) == 0;
  if (dtype == TQ_C64)
    return vec ? topk_t<c64, true>(n, amps, k, index, prob, count, na, ax, base, workspace, stream)
               : topk_t<c64, false>(n, amps, k, index, prob, count, na, ax, base, workspace, stream);
  return vec ? topk_t<c128, true>(n, amps, k, index, prob, count, na, ax, base, workspace, stream)
             : topk_t<c128, false>(n, amps, k, index, prob, count, na, ax, base, workspace, stream);
}

}  // namespace tq
