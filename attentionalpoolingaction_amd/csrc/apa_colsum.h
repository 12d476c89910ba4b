// apa_colsum.h -- the one descriptor of the fixed-order column sum that ends every backward pass, for the host
// declarations (apa_internal.h) and the device body (apa_device.h: colsum_block) alike.  Passed to kernels by value.
#pragma once
#include <stdint.h>

namespace apa {

// Column c of the [nblk][ld] partial matrix `pdwa` is summed over its rows in a fixed order and stored by section:
//   [0, C1) -> dwa,  [C1, C2) -> dwa2,  [C2, C3) -> dwa3,  [C3, C4) -> dwa4,  [C4, C) -> dwa5
// (up to five outputs from one partial matrix: dW2 | db1 | db2 | dWa | dba of the cfg 003 pose head).  A section whose
// pointer is null is absent: colsum_prepare moves its boundary to C, so a single output needs pdwa / dwa / nblk / C /
// ld only.
//   pdba / dba   optional: dba[0] = sum of pdba[0 .. nblk), by block 0
//   perm_nthr    > 0: the first section holds the pose head's dW2 partials in the permuted order of
//                pose_bwd_rows_kernel (perm_cp = Cp); colsum_block undoes the permutation when it writes dwa
//   rng_bump     optional: the device-side dropout counter, advanced by block 0 (the call's last launch)
//   aux_*        optional scalar reduction by the LAST block: aux_dst[0] = aux_scale * sum(aux_src[0 .. aux_n)) -- a
//                launch of its own otherwise (the pose loss of the fused cfg 003 step); aux_n < 0: the batch mean of
//                -aux_n per-example losses in apa_softmax_xent_fwd_bwd's own summation order
struct ColsumArgs {
  const float* pdwa = nullptr; const float* pdba = nullptr; int nblk = 0, C = 0, ld = 0;
  float* dwa = nullptr;
  float* dwa2 = nullptr; int C1 = 0;
  float* dwa3 = nullptr; int C2 = 0;
  float* dwa4 = nullptr; int C3 = 0;
  float* dwa5 = nullptr; int C4 = 0;
  float* dba = nullptr;
  int perm_nthr = 0, perm_cp = 0;
  uint64_t* rng_bump = nullptr;
  const float* aux_src = nullptr; int aux_n = 0; float aux_scale = 0.f; float* aux_dst = nullptr;
};

// The descriptor as the kernels take it -- absent sections end at C -- and the number of 1024-thread blocks (32 columns
// each) that sum it.
inline int colsum_prepare(ColsumArgs& a) {
  if (!a.dwa2) a.C1 = a.C;
  if (!a.dwa3) a.C2 = a.C;
  if (!a.dwa4) a.C3 = a.C;
  if (!a.dwa5) a.C4 = a.C;
  return (a.C + 31) / 32;
}

}  // namespace apa
