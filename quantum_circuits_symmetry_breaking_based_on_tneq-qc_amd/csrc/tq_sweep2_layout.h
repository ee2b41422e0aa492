// The sweep-chain layout planner (tq_sweep2_layout.cpp): from a chain of APPLY steps to the
// descriptors tq_sweep2.hip / tq_sweepd.hip read.  Pure functions of the chain, the context below
// and the process-wide knobs (tq_plan_internal.h); they see neither the Plan nor the compiler.
#pragma once
#include "tq_plan_compile.h"

#include <map>

namespace tq {

struct S2Ctx {
  int dtype = TQ_C64;
  size_t esz = 8;
  // mode -> extent.  A reference into the compiler's map: flush_chain inserts its temporary
  // compose mode (1 << 30) there around the layout calls of a dense chain's compose op
  const std::map<int, int64_t>& ext;
  int lanes_hint = 1;    // > 1: slices run in batches of that many lanes (fewer chunks per dependent op)
  int group_hint = 1;    // lockstep groups of that many plans share every sweep launch
  int min_chunks = 0;    // smallest chunk count of a big sweep op (0: TQ_S2_MINCHUNKS)
};

// product of the modes' extents
int64_t ext_of(const S2Ctx& x, const std::vector<int>& ms);
// mixed-radix digits of index t over `modes` (last fastest), and back
void digits(const S2Ctx& x, int64_t t, const std::vector<int>& modes, std::map<int, int64_t>& dig);
int64_t index_of(const S2Ctx& x, const std::vector<int>& modes, const std::map<int, int64_t>& dig);
// element strides of every mode of X0 (contiguous, its own order) and of Y (contiguous, out order)
void chain_strides(const S2Ctx& x, const Chain& c, const std::vector<int>& out_modes,
                   std::map<int, int64_t>& sx, std::map<int, int64_t>& sy);

// tile modes / working sets of a chain; false if it fits neither sweep kernel's limits
bool chain_shape(const S2Ctx& x, const Chain& c, const std::vector<int>& out_modes, ChainShape& sh);
// the dense form of a chain (tq_sweepd.hip); false if it does not apply
bool s2_dense_layout(const S2Ctx& x, const Chain& c, const ChainShape& sh, const std::vector<int>& out_modes,
                     S2Dense* dd);
// the chain's square gates re-listed into fuller register blocks of B bits; false if unchanged
bool s2_reorder_squares(const S2Ctx& x, const Chain& c, Chain& out, int B);
// the in-place butterfly sweep's descriptor (tq_sweep2.hip); false if the chain does not fit.
// one_chunk: the chain-launch form (Op::stab1), one chunk of the whole tensor when the tile holds it
bool s2_layout(const S2Ctx& x, const Chain& c, const ChainShape& sh, const std::vector<int>& out_modes,
               S2Desc* out, bool one_chunk = false);
// a sweep2 op's descriptor blob: the S2Desc, then the host-built lane and chunk-base tables
std::vector<char> s2_blob(const S2Desc& d, size_t esz);

}  // namespace tq
