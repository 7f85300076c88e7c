// The raw fp32 tensors of one NAT block (views onto the caller's state dict), as the pack kernels of the three wave-private level
// kernels read them (nat_l0w.h, nat_l1w.h, nat_l2w.h): filled once per block by the model load (model_load.h).
#pragma once
#include "opfmt.h"

namespace RIFT_NS {
struct NatBlkSrc { const float *ln1_g, *ln1_b, *wqkv, *bqkv, *rpb, *wproj, *bproj, *ln2_g, *ln2_b, *w1, *b1, *w2, *b2; };
}  // namespace RIFT_NS
