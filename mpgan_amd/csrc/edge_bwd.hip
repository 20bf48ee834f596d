// mpg_edge_bwd, the data-gradient kernel of the fused edge network: the entry point.  Launches without edge scalars take the
// eight-wave kernel (edge_bwd1_impl.h): this unit holds its no-dropout variants, edge_bwd_d1.hip / edge_bwd_d2.hip those with
// dropout, so that the three parts of the slow-to-compile template build side by side.  Launches with edge scalars take the
// four-wave kernel (edge_bwd2_impl.h): edge_bwd_q{0,1,2}.hip.
#include "edge_bwd1_impl.h"

#ifndef MPG_SINGLE_VARIANT
int mpg_edge_bwd_d0(const MpgEdgeBwd* p, hipStream_t st) { return b1_launch<0>(p, st); }   // (this unit's share of the eight-wave kernel)
#endif

extern "C" int mpg_edge_bwd(const MpgEdgeBwd* p, void* stream) {
    if (p->B <= 0 || p->N <= 0 || p->SC <= 0) return -1;
    if (p->sign3 == nullptr || p->stageE2 == nullptr) return -3;   // the forward's by-products: sign words of Z3, parked E2
    if (!(p->alpha >= 0.f && p->alpha <= 1.f)) return -4;
    if (!p->f16) return -8;   // both gradient products take fp16 images
    if ((p->N + p->SC - 1) / p->SC > B2_LIST_MAX) return -6;  // senders per chunk (the list of unmasked ones lives in LDS)
    if (edge_park_over32(p->B, (p->N + 31) / 32, p->N)) return -7;  // staging offsets are 32-bit
    if (p->stageZ2 != nullptr && p->gexp == nullptr) return -9;
    hipStream_t st = (hipStream_t)stream;
#ifdef MPG_SINGLE_VARIANT
#ifdef MPG_BWD1   // (-DMPG_BWD1: the eight-wave form, edge_bwd1_impl.h; without it the four-wave one, no edge scalars)
    return b1_launch<MPG_SINGLE_VARIANT>(p, st);
#else
    return b2_launch<MPG_SINGLE_VARIANT>(p, st);
#endif
#else
    static constexpr EdgeBwdUnit* UNIT[2][3] = {{mpg_edge_bwd_d0, mpg_edge_bwd_d1, mpg_edge_bwd_d2},    // [edge scalars][dropout mode]
                                                {mpg_edge_bwd_q0, mpg_edge_bwd_q1, mpg_edge_bwd_q2}};
    if (p->es != nullptr) {
        if (p->wq == nullptr || p->des == nullptr || p->daq == nullptr) return -3;
        if ((p->N + p->SC - 1) / p->SC > B2_LIST_MAX_Q) return -6;
    }
    return UNIT[p->es != nullptr][edge_drop_mode(p->thr)](p, st);
#endif
}
