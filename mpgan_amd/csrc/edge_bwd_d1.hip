// The byte-threshold-dropout variants of the eight-wave data-gradient kernel (edge_bwd1_impl.h; see edge_bwd.hip).
#include "edge_bwd1_impl.h"

int mpg_edge_bwd_d1(const MpgEdgeBwd* p, hipStream_t st) { return b1_launch<1>(p, st); }
