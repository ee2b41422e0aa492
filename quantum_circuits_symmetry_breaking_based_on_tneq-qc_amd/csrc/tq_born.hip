// Born-rule sampling of a block of amplitudes on the device: the consumer of tq_plan_execute's
// output for SURVEY.md §8(e) ("shard bitstrings").  Replaces nothing in the reference, which has
// no bitstring sampler; the nearest is the continuous EngineSiamese.sample
// (tneq_qc/core/engine_siamese.py:740-915, here icdf_kernel in tq_data.hip), one draw per row on
// a grid of <= 8192 points.  Without this entry point a user copies every 8 MB block to the host
// and runs cumsum + searchsorted there.
//
//     p_i = re(a_i)^2 + im(a_i)^2 (float64; complex64 widened first, so both squares are exact)
//     C_i = inclusive prefix sum of p,  S1 = C_{n-1},  S2 = sum p_i^2
//     index_j = min{ i : C_i > u_j S1 }, else the last i with p_i > 0; -1 when S1 is not in (0, inf)
//     prob_j = p_{index_j}
//
// Three launches, no float atomics, bitwise reproducible:
//  * born_totals  — one workgroup (256 lanes) per chunk of 4096 elements: coalesced 16-B loads,
//    p into LDS, chunk_scan; the chunk's total, sum p^2 and last positive element go to a slab.
//  * born_bases   — one workgroup: the chunk ends within groups of 16 chunks (cend), the group
//    bases (sbase), S1, S2 and the last positive element; writes stats.
//  * born_resolve — one workgroup per chunk: every lane tests draws against the chunk's interval
//    [Elo, Ehi); a chunk that owns a draw re-runs chunk_scan (the same device function) keeping
//    the 4096 local values in LDS, and each owned draw binary-searches them.
//
// The kernel's C is defined by one nested expression, every level accumulated in index order:
//     C_i = sbase[g] + (cbase[c] + (woff[w] + (io[l] + run_k)))
// run_k: the lane's running sum over its 16 consecutive elements; io: the running sum of the lane
// totals of the 64 lanes of a wave; woff: of the 4 wave totals; cbase: of the chunk totals of the
// group (cbase[c + 1] = cend[c] = cbase[c] + total[c]); sbase: of the group totals.  At every level
// the value at a unit's last element IS the next unit's base (the same float64 add of the same
// operands), and a unit's first element adds a non-negative number to that base; float64 addition
// is monotone, so C is non-decreasing in i, and the bound that selects a chunk for a threshold
// (Ehi = sbase[g] + cend[c]) is bit-identical to C at the chunk's last element.  FP contraction is
// off so that both passes round identically whatever the compiler does with either kernel.
//
// tq_born_pool_sample / tq_born_pool_merge (further down) sample ACROSS blocks with a weighted
// reservoir; their candidates come from the same chunk_scan, bases_scan and resolve_chunk.
#include "tq_born_common.h"

namespace tq {

namespace {

constexpr int kBornNT = 256;                     // lanes per workgroup
constexpr int kBornPL = 16;                      // consecutive elements per lane
constexpr int kBornChunk = kBornNT * kBornPL;    // 4096
constexpr int kBornGroup = 16;                   // chunks per group of the base scan
constexpr int kBornTile = 4 * kBornNT;           // draws tested per round of born_resolve

// workspace layout (all 8-byte words first, then the int32 slab)
struct BornWs {
  double* total;      // [nchunks]  chunk totals (chunk_scan's last local value)
  double* s2;         // [nchunks]  chunk sums of p^2
  double* cend;       // [nchunks]  end of chunk c within its group
  double* sbase;      // [ngroups + 1]
  double* meta;       // [0] = S1, [1] = last positive element (int64 bits)
  int32_t* lastloc;   // [nchunks]  last positive element within the chunk, -1 = none
};

inline int64_t born_chunks(int64_t n) { return (n + kBornChunk - 1) / kBornChunk; }
inline int64_t born_groups(int64_t nchunks) { return (nchunks + kBornGroup - 1) / kBornGroup; }

inline size_t born_ws_bytes(int64_t n) {
  const int64_t nc = born_chunks(n), ng = born_groups(nc);
  const size_t words = (size_t)(3 * nc + (ng + 1) + 2);
  return (words * 8 + (size_t)nc * 4 + 15) & ~(size_t)15;
}

inline BornWs born_ws(void* ws, int64_t n) {
  const int64_t nc = born_chunks(n), ng = born_groups(nc);
  BornWs w;
  double* d = reinterpret_cast<double*>(ws);
  w.total = d;
  w.s2 = w.total + nc;
  w.cend = w.s2 + nc;
  w.sbase = w.cend + nc;
  w.meta = w.sbase + ng + 1;
  w.lastloc = reinterpret_cast<int32_t*>(w.meta + 2);
  return w;
}

// LDS position of chunk element e: one pad word per lane segment, so that lane l reading its
// segment (stride 17 doubles) touches every bank once per 32 lanes
__device__ __forceinline__ int born_pad(int e) { return e + (e >> 4); }

struct BornLds {
  double v[kBornChunk + kBornNT];   // p, then the local inclusive values
  double lt[kBornNT];               // lane totals
  double wt[kBornNT / 64];          // wave totals
  double ws2[kBornNT / 64];         // wave sums of p^2
  int wl[kBornNT / 64];             // last positive element per wave
};

// The chunk scan: loads chunk c (elements beyond n count as p = 0), leaves in L.v either nothing
// useful (KEEP = false) or local_i = woff + (io + run_k) for every element, and returns the
// chunk total = local value of the chunk's last element.  STATS: also the chunk's sum of p^2
// (a fixed reduction order) and its last element with p > 0 (-1 = none), for the first pass.
template <typename T, bool VEC, bool KEEP, bool STATS>
__device__ __forceinline__ double chunk_scan(const T* __restrict__ amps, int64_t n, int64_t c,
                                             BornLds& L, double& s2_out, int& last_out) {
#pragma clang fp contract(off)
  constexpr int EPL = 16 / (int)sizeof(T);          // elements per 16-B load
  constexpr int NLD = kBornPL / EPL;                // loads per lane
  const int tid = threadIdx.x;
  const int64_t e0 = c * kBornChunk;
  const int64_t rem = n - e0;                       // > 0
  const T* __restrict__ a = amps + e0;
#pragma unroll
  for (int j = 0; j < NLD; ++j) {
    const int e = j * (kBornNT * EPL) + tid * EPL;
    if constexpr (VEC && EPL == 2) {
      if (e + 2 <= rem) {
        const float4 q = *reinterpret_cast<const float4*>(a + e);
        const double r0 = (double)q.x, i0 = (double)q.y, r1 = (double)q.z, i1 = (double)q.w;
        L.v[born_pad(e)] = r0 * r0 + i0 * i0;
        L.v[born_pad(e + 1)] = r1 * r1 + i1 * i1;
        continue;
      }
    }
    if constexpr (VEC && EPL == 1) {
      if (e < rem) {
        const double2 q = *reinterpret_cast<const double2*>(a + e);
        L.v[born_pad(e)] = q.x * q.x + q.y * q.y;
        continue;
      }
    }
#pragma unroll
    for (int k = 0; k < EPL; ++k) L.v[born_pad(e + k)] = (e + k < rem) ? born_p<T>(a, e + k) : 0.0;
  }
  __syncthreads();
  double* __restrict__ seg = L.v + tid * (kBornPL + 1);
  double run = 0.0, s2 = 0.0;
  int last = -1;
#pragma unroll
  for (int k = 0; k < kBornPL; ++k) {
    const double p = seg[k];
    run += p;
    if constexpr (KEEP) seg[k] = run;
    if constexpr (STATS) {
      s2 += p * p;
      if (p > 0.0) last = tid * kBornPL + k;
    }
  }
  L.lt[tid] = run;
  __syncthreads();
  // io: running sum of the lane totals of this wave, in lane order (every lane walks the same
  // 64 broadcast reads)
  const int lane = tid & 63, w = tid >> 6;
  double io = 0.0, acc = 0.0;
#pragma unroll 8
  for (int s = 0; s < 64; ++s) {
    if (s == lane) io = acc;
    acc += L.lt[w * 64 + s];
  }
  if constexpr (STATS) {
    // sum p^2 and the last positive element of the wave: a fixed butterfly, the same every run
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
      s2 += __shfl_xor(s2, m);
      last = max(last, __shfl_xor(last, m));
    }
  }
  if (lane == 0) {
    L.wt[w] = acc;
    if constexpr (STATS) {
      L.ws2[w] = s2;
      L.wl[w] = last;
    }
  }
  __syncthreads();
  double woff = 0.0, tot = 0.0;
#pragma unroll
  for (int x = 0; x < kBornNT / 64; ++x) {
    if (x == w) woff = tot;
    tot += L.wt[x];
  }
  if constexpr (KEEP) {
#pragma unroll
    for (int k = 0; k < kBornPL; ++k) seg[k] = woff + (io + seg[k]);
  }
  if constexpr (STATS) {
    s2_out = 0.0;
    last_out = -1;
#pragma unroll
    for (int x = 0; x < kBornNT / 64; ++x) {
      s2_out += L.ws2[x];
      last_out = max(last_out, L.wl[x]);
    }
  }
  return tot;
}

template <typename T, bool VEC>
__global__ void __launch_bounds__(kBornNT)
born_totals(const T* __restrict__ amps, int64_t n, BornWs W) {
  __shared__ BornLds L;
  const int64_t c = blockIdx.x;
  double s2 = 0.0;
  int last = -1;
  const double tot = chunk_scan<T, VEC, false, true>(amps, n, c, L, s2, last);
  if (threadIdx.x == 0) {
    W.total[c] = tot;
    W.s2[c] = s2;
    W.lastloc[c] = last;
  }
}

// The base scan of one workgroup; lane 0 returns S1 and S2 (what it wrote to stats).
__device__ __forceinline__ void bases_scan(int64_t nchunks, int64_t ngroups, const BornWs& W,
                                           double* __restrict__ stats, double& S1, double& S2) {
#pragma clang fp contract(off)
  __shared__ double gt[kBornNT], gs[kBornNT];
  __shared__ int64_t gl[kBornNT];
  const int tid = threadIdx.x;
  double acc0 = 0.0, s20 = 0.0;   // lane 0: running over the groups
  int64_t last0 = -1;
  for (int64_t g0 = 0; g0 < ngroups; g0 += kBornNT) {
    const int64_t g = g0 + tid;
    if (g < ngroups) {
      // the group's slab first (independent loads), then the running sums in chunk order
      const int64_t c0 = g * kBornGroup;
      const int nc = (int)(nchunks - c0 < kBornGroup ? nchunks - c0 : kBornGroup);
      double t[kBornGroup], q[kBornGroup];
      int32_t l[kBornGroup];
#pragma unroll
      for (int k = 0; k < kBornGroup; ++k) {
        const bool in = k < nc;
        t[k] = in ? W.total[c0 + k] : 0.0;
        q[k] = in ? W.s2[c0 + k] : 0.0;
        l[k] = in ? W.lastloc[c0 + k] : -1;
      }
      double acc = 0.0, s2 = 0.0;
      int64_t last = -1;
#pragma unroll
      for (int k = 0; k < kBornGroup; ++k) {
        acc += t[k];
        s2 += q[k];
        if (k < nc) W.cend[c0 + k] = acc;
        if (l[k] >= 0) last = (c0 + k) * kBornChunk + l[k];
      }
      gt[tid] = acc;
      gs[tid] = s2;
      gl[tid] = last;
    }
    __syncthreads();
    if (tid == 0) {
      if (g0 == 0) W.sbase[0] = 0.0;
      const int ng = (int)(ngroups - g0 < kBornNT ? ngroups - g0 : kBornNT);
      for (int k = 0; k < ng; ++k) {
        acc0 += gt[k];
        W.sbase[g0 + k + 1] = acc0;
        s20 += gs[k];
        if (gl[k] >= 0) last0 = gl[k];
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    W.meta[0] = acc0;
    reinterpret_cast<int64_t*>(W.meta)[1] = last0;
    stats[0] = acc0;
    stats[1] = s20;
  }
  S1 = acc0;
  S2 = s20;
}

__global__ void __launch_bounds__(kBornNT)
born_bases(int64_t nchunks, int64_t ngroups, BornWs W, double* __restrict__ stats) {
  double S1, S2;
  bases_scan(nchunks, ngroups, W, stats, S1, S2);
}

// The resolve step of chunk blockIdx.x over `n_items` draws.  SEL = false (tq_born_sample): item s
// is draw s.  SEL = true (tq_born_pool_sample): item s is draw sel[s], the accepted draws of the
// call in any order; only those slots of index / prob are written, and a block without mass
// writes nothing (its list is empty).
template <typename T, bool VEC, bool SEL>
__device__ __forceinline__ void resolve_chunk(const T* __restrict__ amps, int64_t n, int64_t n_items,
                                              const double* __restrict__ u, const int32_t* __restrict__ sel,
                                              int64_t* __restrict__ index, double* __restrict__ prob,
                                              const BornWs& W, int n_axes, const BornAxes& ax,
                                              uint64_t base) {
#pragma clang fp contract(off)
  __shared__ BornLds L;
  __shared__ int list[kBornTile];
  __shared__ int cnt;
  const int tid = threadIdx.x;
  const int64_t c = blockIdx.x;
  const double S1 = W.meta[0];
  if (!(S1 > 0.0 && S1 < __builtin_huge_val())) {
    if constexpr (!SEL) {
      if (c == 0)
        for (int64_t j = tid; j < n_items; j += kBornNT) {
          index[j] = -1;
          if (prob) prob[j] = 0.0;
        }
    }
    return;
  }
  const int64_t g = c / kBornGroup;
  const double G = W.sbase[g];
  const double cb = (c % kBornGroup) ? W.cend[c - 1] : 0.0;
  const double Elo = G + cb, Ehi = G + W.cend[c];
  if (c != 0 && !(Ehi > Elo)) return;   // no mass here: no threshold selects this chunk
  const int64_t lastpos = reinterpret_cast<const int64_t*>(W.meta)[1];
  if (tid == 0) cnt = 0;
  __syncthreads();
  bool scanned = false;
  for (int64_t j0 = 0; j0 < n_items; j0 += kBornTile) {
#pragma unroll
    for (int q = 0; q < kBornTile / kBornNT; ++q) {
      const int64_t s = j0 + q * kBornNT + tid;
      if (s < n_items) {
        int64_t j = s;
        if constexpr (SEL) j = sel[s];
        const double t = u[j] * S1;
        if (Ehi > t && (c == 0 || !(Elo > t))) {
          list[atomicAdd(&cnt, 1)] = (int)(s - j0);
        } else if (c == 0 && !(S1 > t)) {
          // no C_i exceeds t (u >= 1, NaN, rounding): the last element with p > 0
          index[j] = lastpos >= 0 ? born_word(lastpos, n_axes, ax, base) : -1;
          if (prob) prob[j] = lastpos >= 0 ? born_p<T>(amps, lastpos) : 0.0;
        }
      }
    }
    __syncthreads();
    const int m = cnt;
    if (m > 0) {
      if (!scanned) {
        double s2;
        int last;
        chunk_scan<T, VEC, true, false>(amps, n, c, L, s2, last);
        __syncthreads();
        scanned = true;
      }
      for (int s = tid; s < m; s += kBornNT) {
        int64_t j = j0 + list[s];
        if constexpr (SEL) j = sel[j];
        const double t = u[j] * S1;
        // first i with C_i > t; C at the chunk's last element is Ehi > t
        int lo = 0, hi = kBornChunk - 1;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (G + (cb + L.v[born_pad(mid)]) > t) hi = mid; else lo = mid + 1;
        }
        // (the padded tail of the last chunk repeats the last element's value, so idx < n)
        const int64_t at = c * kBornChunk + lo;
        const int64_t idx = at < n ? at : n - 1;
        index[j] = born_word(idx, n_axes, ax, base);
        if (prob) prob[j] = born_p<T>(amps, idx);
      }
    }
    __syncthreads();
    if (tid == 0) cnt = 0;
    __syncthreads();
  }
}

template <typename T, bool VEC>
__global__ void __launch_bounds__(kBornNT)
born_resolve(const T* __restrict__ amps, int64_t n, int64_t n_draws, const double* __restrict__ u,
             int64_t* __restrict__ index, double* __restrict__ prob, BornWs W, int n_axes,
             BornAxes ax, uint64_t base) {
  resolve_chunk<T, VEC, false>(amps, n, n_draws, u, nullptr, index, prob, W, n_axes, ax, base);
}

// ---- the pool: a weighted reservoir over blocks (tq_born_pool_sample / tq_born_pool_merge) -------
//
// Four launches per block, the first unchanged: born_totals, born_pool_bases (born_bases' scan,
// then lane 0 reads the pool, decides whether the block contributes, leaves W, W', S1 and that flag
// in the workspace, zeroes the accepted counter and updates pool[0..2]), born_pool_accept (a grid
// over the draws: the acceptance rule, accepted j appended to a list), born_pool_resolve
// (resolve_chunk over that list; workgroup 0 writes the count to pool[3]).  Every grid that needs
// W / W' reads the workspace copy, written one launch earlier by one workgroup; pool itself is read
// and written by that workgroup's lane 0 only, and pool[3] by one lane of the last launch.

struct PoolWs {
  double* pm;        // [0] = W before, [1] = W', [2] = S1 (sample) / W_b (merge), [3] = 0 no-op, 1 rule, 2 all
  int32_t* count;    // accepted / taken slots (8 bytes reserved)
  int32_t* list;     // [n_draws] accepted draws (sample only)
};

constexpr size_t kPoolHead = 4 * 8 + 8;

inline size_t born_pool_ws_bytes(int64_t n, int64_t n_draws) {
  return (born_ws_bytes(n) + kPoolHead + (size_t)n_draws * 4 + 15) & ~(size_t)15;
}

inline PoolWs pool_ws(void* at) {
  PoolWs p;
  p.pm = reinterpret_cast<double*>(at);
  p.count = reinterpret_cast<int32_t*>(p.pm + 4);
  p.list = p.count + 2;
  return p;
}

__device__ __forceinline__ bool born_mass(double x) { return x > 0.0 && x < __builtin_huge_val(); }

__global__ void __launch_bounds__(kBornNT)
born_pool_bases(int64_t nchunks, int64_t ngroups, BornWs W, double* __restrict__ stats,
                double* __restrict__ pool, PoolWs P) {
#pragma clang fp contract(off)
  double S1, S2;
  bases_scan(nchunks, ngroups, W, stats, S1, S2);
  if (threadIdx.x == 0) {
    const double w0 = pool[0];
    const bool ok = born_mass(S1);
    const double w1 = w0 + S1;
    P.pm[0] = w0;
    P.pm[1] = w1;
    P.pm[2] = S1;
    P.pm[3] = !ok ? 0.0 : (w0 == 0.0 ? 2.0 : 1.0);
    *P.count = 0;
    if (ok) {
      pool[0] = w1;
      pool[1] = pool[1] + S2;
      pool[2] = pool[2] + 1.0;
    }
  }
}

// take(j): pm[3] == 2, or pm[3] == 1 and v_j * W' < mass (one multiply, one compare; NaN: false)
__device__ __forceinline__ bool pool_take(const PoolWs& P, const double* __restrict__ v, int64_t j) {
#pragma clang fp contract(off)
  const double mode = P.pm[3];
  if (mode == 0.0) return false;
  if (mode == 2.0) return true;
  return v[j] * P.pm[1] < P.pm[2];
}

__global__ void __launch_bounds__(kBornNT)
born_pool_accept(int64_t n_draws, const double* __restrict__ v, PoolWs P) {
  const int64_t j = (int64_t)blockIdx.x * kBornNT + threadIdx.x;
  if (j < n_draws && pool_take(P, v, j)) P.list[atomicAdd(P.count, 1)] = (int32_t)j;
}

template <typename T, bool VEC>
__global__ void __launch_bounds__(kBornNT)
born_pool_resolve(const T* __restrict__ amps, int64_t n, const double* __restrict__ u,
                  int64_t* __restrict__ index, double* __restrict__ prob, double* __restrict__ pool,
                  BornWs W, PoolWs P, int n_axes, BornAxes ax, uint64_t base) {
  const int64_t m = *P.count;
  if (blockIdx.x == 0 && threadIdx.x == 0) pool[3] = (double)m;
  if (m == 0) return;   // before anything of the block is read
  resolve_chunk<T, VEC, true>(amps, n, m, u, P.list, index, prob, W, n_axes, ax, base);
}

__global__ void born_merge_head(const double* __restrict__ pool_a, const double* __restrict__ pool_b,
                                PoolWs P) {
#pragma clang fp contract(off)
  if (threadIdx.x == 0) {
    const double wa = pool_a[0], wb = pool_b[0];
    P.pm[0] = wa;
    P.pm[1] = wa + wb;
    P.pm[2] = wb;
    P.pm[3] = !born_mass(wb) ? 0.0 : (wa == 0.0 ? 2.0 : 1.0);
    *P.count = 0;
  }
}

__global__ void __launch_bounds__(kBornNT)
born_merge_take(int64_t n_draws, const double* __restrict__ v, int64_t* __restrict__ index_a,
                double* __restrict__ prob_a, const int64_t* __restrict__ index_b,
                const double* __restrict__ prob_b, PoolWs P) {
  const int64_t j = (int64_t)blockIdx.x * kBornNT + threadIdx.x;
  if (j < n_draws && pool_take(P, v, j)) {
    index_a[j] = index_b[j];
    if (prob_a) prob_a[j] = prob_b[j];
    atomicAdd(P.count, 1);
  }
}

__global__ void born_merge_tail(double* __restrict__ pool_a, const double* __restrict__ pool_b, PoolWs P) {
#pragma clang fp contract(off)
  if (threadIdx.x == 0) {
    if (P.pm[3] != 0.0) {
      pool_a[0] = P.pm[1];
      pool_a[1] = pool_a[1] + pool_b[1];
      pool_a[2] = pool_a[2] + pool_b[2];
    }
    pool_a[3] = (double)*P.count;
  }
}

template <typename T, bool VEC>
int born_pool_t(int64_t n, const void* amps, int64_t n_draws, const double* u, const double* v,
                int64_t* index, double* prob, double* pool, double* stats, int n_axes,
                const BornAxes& ax, uint64_t base, void* ws, hipStream_t st) {
  const int64_t nc = born_chunks(n), ng = born_groups(nc);
  const BornWs W = born_ws(ws, n);
  const PoolWs P = pool_ws(reinterpret_cast<char*>(ws) + born_ws_bytes(n));
  const T* a = reinterpret_cast<const T*>(amps);
  hipLaunchKernelGGL((born_totals<T, VEC>), dim3((unsigned)nc), dim3(kBornNT), 0, st, a, n, W);
  TQ_HIP(hipGetLastError());
  hipLaunchKernelGGL(born_pool_bases, dim3(1), dim3(kBornNT), 0, st, nc, ng, W, stats, pool, P);
  TQ_HIP(hipGetLastError());
  hipLaunchKernelGGL(born_pool_accept, dim3((unsigned)((n_draws + kBornNT - 1) / kBornNT)), dim3(kBornNT),
                     0, st, n_draws, v, P);
  TQ_HIP(hipGetLastError());
  hipLaunchKernelGGL((born_pool_resolve<T, VEC>), dim3((unsigned)nc), dim3(kBornNT), 0, st, a, n, u,
                     index, prob, pool, W, P, n_axes, ax, base);
  TQ_HIP(hipGetLastError());
  return TQ_OK;
}

template <typename T, bool VEC>
int born_t(int64_t n, const void* amps, int64_t n_draws, const double* u, int64_t* index,
           double* prob, double* stats, int n_axes, const BornAxes& ax, uint64_t base, void* ws,
           hipStream_t st) {
  const int64_t nc = born_chunks(n), ng = born_groups(nc);
  const BornWs W = born_ws(ws, n);
  const T* a = reinterpret_cast<const T*>(amps);
  hipLaunchKernelGGL((born_totals<T, VEC>), dim3((unsigned)nc), dim3(kBornNT), 0, st, a, n, W);
  TQ_HIP(hipGetLastError());
  hipLaunchKernelGGL(born_bases, dim3(1), dim3(kBornNT), 0, st, nc, ng, W, stats);
  TQ_HIP(hipGetLastError());
  if (n_draws > 0) {
    hipLaunchKernelGGL((born_resolve<T, VEC>), dim3((unsigned)nc), dim3(kBornNT), 0, st, a, n,
                       n_draws, u, index, prob, W, n_axes, ax, base);
    TQ_HIP(hipGetLastError());
  }
  return TQ_OK;
}

}  // namespace

size_t born_workspace(int dtype, int64_t n, int64_t n_draws) {
  if (dtype != TQ_C64 && dtype != TQ_C128) {
    set_error("born_sample: amplitudes must be TQ_C64 or TQ_C128");
    return 0;
  }
  if (n < 1 || n > ((int64_t)1 << 31)) {
    set_error("born_sample: n must be in [1, 2^31]");
    return 0;
  }
  if (n_draws < 0 || n_draws >= ((int64_t)1 << 31)) {
    set_error("born_sample: n_draws must be in [0, 2^31)");
    return 0;
  }
  return born_ws_bytes(n);
}

int born_launch(int dtype, int64_t n, const void* amps, int64_t n_draws, const double* u,
                int64_t* index, double* prob, double* stats, int n_axes, const int32_t* axis_qubit,
                uint64_t base, void* workspace, size_t ws_bytes, hipStream_t stream) {
  const size_t need = born_workspace(dtype, n, n_draws);
  if (need == 0) return TQ_ERR_INVALID;
  TQ_CHECK_ARG(amps && stats && workspace, "born_sample: null pointer");
  TQ_CHECK_ARG(n_draws == 0 || (u && index), "born_sample: null u / index");
  TQ_CHECK_ARG(ws_bytes >= need, "born_sample: workspace smaller than tq_born_sample_workspace");
  TQ_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "born_sample: workspace must be 8-byte aligned");
  const size_t ralign = dtype == TQ_C64 ? 4 : 8;
  TQ_CHECK_ARG(((uintptr_t)amps & (ralign - 1)) == 0, "born_sample: misaligned amplitudes");
  BornAxes ax{};
  int na = -1;
  TQ_TRY(born_axes("born_sample", n, n_axes, axis_qubit, base, ax, na));
  const bool vec = ((uintptr_t)amps & 15) == 0;
  if (dtype == TQ_C64)
    return vec ? born_t<c64, true>(n, amps, n_draws, u, index, prob, stats, na, ax, base, workspace, stream)
               : born_t<c64, false>(n, amps, n_draws, u, index, prob, stats, na, ax, base, workspace, stream);
  return vec ? born_t<c128, true>(n, amps, n_draws, u, index, prob, stats, na, ax, base, workspace, stream)
             : born_t<c128, false>(n, amps, n_draws, u, index, prob, stats, na, ax, base, workspace, stream);
}

size_t born_pool_workspace(int dtype, int64_t n, int64_t n_draws) {
  if (dtype != TQ_C64 && dtype != TQ_C128) {
    set_error("born_pool: amplitudes must be TQ_C64 or TQ_C128");
    return 0;
  }
  if (n < 1 || n > ((int64_t)1 << 31)) {
    set_error("born_pool: n must be in [1, 2^31]");
    return 0;
  }
  if (n_draws < 1 || n_draws >= ((int64_t)1 << 31)) {
    set_error("born_pool: n_draws must be in [1, 2^31)");
    return 0;
  }
  return born_pool_ws_bytes(n, n_draws);
}

int born_pool_launch(int dtype, int64_t n, const void* amps, int64_t n_draws, const double* u,
                     const double* v, int64_t* index, double* prob, double* pool, double* stats,
                     int n_axes, const int32_t* axis_qubit, uint64_t base, void* workspace,
                     size_t ws_bytes, hipStream_t stream) {
  const size_t need = born_pool_workspace(dtype, n, n_draws);
  if (need == 0) return TQ_ERR_INVALID;
  TQ_CHECK_ARG(amps && u && v && index && pool && stats && workspace, "born_pool: null pointer");
  TQ_CHECK_ARG(ws_bytes >= need, "born_pool: workspace smaller than tq_born_pool_workspace");
  TQ_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "born_pool: workspace must be 8-byte aligned");
  const size_t ralign = dtype == TQ_C64 ? 4 : 8;
  TQ_CHECK_ARG(((uintptr_t)amps & (ralign - 1)) == 0, "born_pool: misaligned amplitudes");
  BornAxes ax{};
  int na = -1;
  TQ_TRY(born_axes("born_pool", n, n_axes, axis_qubit, base, ax, na));
  const bool vec = ((uintptr_t)amps & 15) == 0;
  if (dtype == TQ_C64)
    return vec ? born_pool_t<c64, true>(n, amps, n_draws, u, v, index, prob, pool, stats, na, ax, base, workspace, stream)
               : born_pool_t<c64, false>(n, amps, n_draws, u, v, index, prob, pool, stats, na, ax, base, workspace, stream);
  return vec ? born_pool_t<c128, true>(n, amps, n_draws, u, v, index, prob, pool, stats, na, ax, base, workspace, stream)
             : born_pool_t<c128, false>(n, amps, n_draws, u, v, index, prob, pool, stats, na, ax, base, workspace, stream);
}

int born_pool_merge_launch(int64_t n_draws, const double* v, int64_t* index_a, double* prob_a,
                           double* pool_a, const int64_t* index_b, const double* prob_b,
                           const double* pool_b, void* workspace, size_t ws_bytes, hipStream_t stream) {
  TQ_CHECK_ARG(n_draws >= 1 && n_draws < ((int64_t)1 << 31), "born_pool: n_draws must be in [1, 2^31)");
  TQ_CHECK_ARG(v && index_a && pool_a && index_b && pool_b && workspace, "born_pool: null pointer");
  TQ_CHECK_ARG((prob_a == nullptr) == (prob_b == nullptr), "born_pool: prob_a and prob_b are both NULL or neither");
  static_assert(kPoolHead <= TQ_BORN_POOL_MERGE_WORKSPACE, "the merge uses the head of the pool workspace");
  TQ_CHECK_ARG(ws_bytes >= TQ_BORN_POOL_MERGE_WORKSPACE, "born_pool: merge workspace smaller than TQ_BORN_POOL_MERGE_WORKSPACE");
  TQ_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "born_pool: workspace must be 8-byte aligned");
  TQ_CHECK_ARG(index_a != index_b && pool_a != pool_b, "born_pool: a reservoir cannot be merged into itself");
  const PoolWs P = pool_ws(workspace);
  hipLaunchKernelGGL(born_merge_head, dim3(1), dim3(64), 0, stream, pool_a, pool_b, P);
  TQ_HIP(hipGetLastError());
  hipLaunchKernelGGL(born_merge_take, dim3((unsigned)((n_draws + kBornNT - 1) / kBornNT)), dim3(kBornNT),
                     0, stream, n_draws, v, index_a, prob_a, index_b, prob_b, P);
  TQ_HIP(hipGetLastError());
  hipLaunchKernelGGL(born_merge_tail, dim3(1), dim3(64), 0, stream, pool_a, pool_b, P);
  TQ_HIP(hipGetLastError());
  return TQ_OK;
}

}  // namespace tq
