// Internal, host only: what the translation units of the fused edge family share across the unit boundary.  The slow kernel
// templates compile side by side, one unit per dropout mode (and per SIGN / NEEDW for the epilogue forms); every unit defines one
// launcher, declared HERE once, and the entry units (edge.hip, edge_fwd_fn.hip, edge_bwd.hip, edge_bwd_fn.hip, edge_dw.hip)
// index constant tables of them.  Beside the launchers: the host predicates that more than one entry point applies.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/mpgan_amd.h"

// ---- launchers, by the unit that defines them (d<dm>: dropout mode, edge_drop_mode below) ----
using EdgeFwdUnit = int(const MpgEdgeFwd* p, hipStream_t st);
using EdgeFwdFnUnit = int(const MpgEdgeFwd* p, const MpgChain* c, const MpgChain* c2, bool sl, hipStream_t st);
using EdgeBwdUnit = int(const MpgEdgeBwd* p, hipStream_t st);
using EdgeBwdFnUnit = int(const MpgEdgeBwd* p, const MpgChain* cdx, const MpgChain* cnx, int epi, hipStream_t st);
using EdgeDwUnit = int(const MpgEdgeDw* p, int R, hipStream_t st);

EdgeFwdUnit mpg_edge_fwd_d0, mpg_edge_fwd_d1, mpg_edge_fwd_d2;   // eight-wave forward: edge.hip, edge_fwd_d{1,2}.hip
EdgeFwdUnit mpg_edge_fwd_q0, mpg_edge_fwd_q1, mpg_edge_fwd_q2;   // four-wave forward with edge scalars: edge_fwd_q{0,1,2}.hip
EdgeFwdFnUnit mpg_edge_fwd_fn_d0s0, mpg_edge_fwd_fn_d0s1, mpg_edge_fwd_fn_d1s0, mpg_edge_fwd_fn_d1s1, mpg_edge_fwd_fn_d2s0,
    mpg_edge_fwd_fn_d2s1;                                        // forward + node network: edge_fwd_fn_d{0,1,2}s{0,1}.hip (s1: SIGN)
EdgeBwdUnit mpg_edge_bwd_d0, mpg_edge_bwd_d1, mpg_edge_bwd_d2;   // eight-wave data gradients: edge_bwd.hip, edge_bwd_d{1,2}.hip
EdgeBwdUnit mpg_edge_bwd_q0, mpg_edge_bwd_q1, mpg_edge_bwd_q2;   // four-wave, with edge scalars: edge_bwd_q{0,1,2}.hip
EdgeBwdFnUnit mpg_edge_bwd_fn_d0w0, mpg_edge_bwd_fn_d0w1, mpg_edge_bwd_fn_d1w0, mpg_edge_bwd_fn_d1w1, mpg_edge_bwd_fn_d2w0,
    mpg_edge_bwd_fn_d2w1;                                        // with epilogue chains: edge_bwd_fn_d{0,1,2}w{0,1}.hip (w1: NEEDW)
EdgeDwUnit mpg_edge_dw_q;                                        // weight gradients with edge scalars: edge_dw_q.hip

// ---- host predicates ----
// dropout mode of a launch from its threshold (the DROP argument of every fused kernel): 0 off, 1 a byte per element,
// 2 a bit per element (p = 1/2); common.h's drop_apply
inline int edge_drop_mode(uint32_t thr) { return thr == 0 ? 0 : (thr == 128 ? 2 : 1); }

// The parked E2 / dZ2 fragments of one block (jet, receiver block, sender): NFR2 = 10 fragments of 1 KiB (edge_common.h asserts
// it).  The kernels address them, and the sign words, with 32-bit offsets behind a buffer descriptor whose record count is an
// int: does a launch of `B` jets x `RB` receiver blocks x `N` senders go past that?
constexpr long long EDGE_PARK_BYTES = 10240;
inline bool edge_park_over32(int B, int RB, int N) { return (long long)B * RB * N * EDGE_PARK_BYTES > 0x7fffffffLL; }

// an absent second chain of the epilogue forms travels as a chain of no layers
inline const MpgChain& chain_or_none(const MpgChain* c) {
    static const MpgChain none = {};   // nlayers = 0
    return c != nullptr ? *c : none;
}

// rows of whole 16-byte groups (the chains' vector stores)?
inline bool rows_vec(const MpgChainLayer& L) {
    return L.N % 4 == 0 && (L.out == nullptr || (L.ldo % 4 == 0 && ((uintptr_t)L.out & 15) == 0));
}
