// Internal: the specialised schedule of mpg_chain (chain2.hip), tried first by the entry point in chain.hip.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/mpgan_amd.h"
#define MPG_CHAIN2_NA (-100)   // "not one of my shapes": the caller runs the general kernel
// One row of chain2's shape table with the options it is launched with: what mpg_chain2_decide found, what
// mpg_chain2_launch runs.  (mpg_chain and mpg_chain_route share the decision; only mpg_chain launches.)
enum MpgChain2Shape { C2_FN_FWD, C2_AC_PROJ, C2_FN_GRAD, C2_DX };
struct MpgChain2Plan {
    MpgChain2Shape shape;
    int drop;   // 0 none, 1 byte mode, 2 bit mode -- one mode for every site of the call
    bool sl;    // the last layer's rows are not whole 16-byte groups
};
int mpg_chain2_decide(const MpgChain* p, MpgChain2Plan* plan);   // 0 and *plan filled, or MPG_CHAIN2_NA; host only
int mpg_chain2_launch(const MpgChain* p, const MpgChain2Plan& plan, hipStream_t st);
