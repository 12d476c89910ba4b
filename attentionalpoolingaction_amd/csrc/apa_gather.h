// apa_gather.h -- the argument the gathered instances of the M == 1 streaming kernels take (apa_device.h: m1_src_image),
// shared by the device code and the host launchers (apa_internal.h: M1Call).
#pragma once
#include <stdint.h>

#include <type_traits>

namespace apa {

struct M1Gather {
  const int32_t* index;      // [N]
  int T;                     // images behind X; an id outside [0, T) is clamped
  int32_t* status;           // nullable: += 1 per clamped id (forward pass only)
  const int64_t* labels;     // nullable: [T] labels, read through index ...
  int64_t* labels_out;       // ... into [N] (workspace), where the loss reducers behind the pass read them
};
// the trailing argument of a streaming kernel: M1Gather on the gathered instances, nothing on the plain ones.  A
// launcher passes m1_gather_arg<G>(c) for either, G being the tag m1_pool_form hands it (apa_internal.h)
struct M1NoGather {};
template <bool GATHER> using M1GatherArg = std::conditional_t<GATHER, M1Gather, M1NoGather>;

// ... and of the two per-class kernels that read X (apa_pc_fused.hip).  Their blocks own ROWS of the flat [N * P] batch,
// not images, so the pixels per image travel along: batch row r is pixel r - n P of batch image n = r / P and its
// feature row is m1_src_image(n, g) * P + that pixel.
struct PcGather {
  M1Gather g;
  int P;
};
template <bool GATHER> using PcGatherArg = std::conditional_t<GATHER, PcGather, M1NoGather>;

// ... and of operand A of a dense product (GemmDesc::rmap, the MAP instances of apa_gemm_bf16.hip): the same row rule,
// row r of A is fetched from row clamp(index[r / P], 0, T - 1) * P + r % P of the buffer behind A.  Clamped silently:
// the status word and the labels are the forward pooling pass's (m1_gather_note), once per step.  index == nullptr: A
// is a plain batch
struct GemmRowMap {
  const int32_t* index = nullptr;   // [rows of A / P]
  int T = 0;                        // images behind A
  int P = 0;                        // rows per image
};

}  // namespace apa
