// What the consumers of an amplitude block share (tq_born.hip: Born-rule sampling, tq_topk.hip:
// the k most probable elements): the probability of one element, the index -> bitstring word
// scatter, and the host-side check of the axis table.
#pragma once

#include "tq_common.h"

namespace tq {

constexpr int kBornMaxAxes = 31;

struct BornAxes {
  int8_t q[kBornMaxAxes + 1];
};

// p_i = re^2 + im^2 in float64 (complex64 widened first); both products and the sum are rounded
// on their own, so p is numpy's bit for bit whatever the compiler does around the call
template <typename T>
__device__ __forceinline__ double born_p(const T* __restrict__ amps, int64_t i) {
#pragma clang fp contract(off)
  using R = typename Traits<T>::R;
  const R* __restrict__ r = reinterpret_cast<const R*>(amps) + 2 * i;
  const double re = (double)r[0], im = (double)r[1];
  return re * re + im * im;
}

__device__ __forceinline__ int64_t born_word(int64_t idx, int n_axes, const BornAxes& ax, uint64_t base) {
  if (n_axes < 0) return idx;
  uint64_t wd = base;
  for (int a = 0; a < n_axes; ++a)
    wd |= (uint64_t)((idx >> (n_axes - 1 - a)) & 1) << ax.q[a];
  return (int64_t)wd;
}

// axis_qubit == NULL: plain indices (na = -1).  Otherwise n == 2^n_axes, the entries distinct and
// in [0, 62], base clear at the axis qubits; `who` prefixes the error message.
inline int born_axes(const char* who, int64_t n, int n_axes, const int32_t* axis_qubit, uint64_t base,
                     BornAxes& ax, int& na) {
  const std::string w = std::string(who) + ": ";
  na = -1;
  if (!axis_qubit) return TQ_OK;
  TQ_CHECK_ARG(n_axes >= 0 && n_axes <= kBornMaxAxes && n == ((int64_t)1 << n_axes),
               w + "n must equal 2^n_axes");
  uint64_t seen = 0;
  for (int a = 0; a < n_axes; ++a) {
    const int q = axis_qubit[a];
    TQ_CHECK_ARG(q >= 0 && q <= 62, w + "axis qubit outside [0, 62]");
    TQ_CHECK_ARG(!((seen >> q) & 1), w + "repeated axis qubit");
    seen |= (uint64_t)1 << q;
    ax.q[a] = (int8_t)q;
  }
  TQ_CHECK_ARG((base & seen) == 0, w + "base overlaps an axis qubit");
  na = n_axes;
  return TQ_OK;
}

}  // namespace tq
