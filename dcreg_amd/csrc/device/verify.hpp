// Per-thread device function of the verification call (include/dcreg.h: dcreg_verify_poses): one point of the cloud at one candidate
// pose - transform, the finite test, exact 1-NN on the cell grid inside the inlier distance, the strict gate, the integer term.  The rule
// is the header's, operation by operation; tests/verify_ref.py states it in numpy.  Included by verify.hip (the kernel and the host seam)
// and, like normal_icp.hpp, compiled for the host under DCREG_HOST_EMUL by the test suite's replay (tests/host_emul/emul_verify.cpp).
#pragma once
#include "normal_icp.hpp"

namespace dcreg {

struct VerifyArgs {
    double dd;                    // d * d in double: the gate (double)d2 < dd
    float bound_f;                // the search bound: the smallest float >= dd (a d2 below dd is below it; d2 == bound stays out)
    int max_ring;                 // rings that cover it (-1: sweep the grid)
};

// what a point leaves: the nearest map point's original index and float d2 when it is an inlier (kNoIdx, +inf otherwise), and the term
struct VerifyPoint {
    uint32_t idx;
    float d2;
    uint64_t e;                   // floor((d2 / dd) * 2^20), at most 2^20 - 1; 0 for a point that is no inlier
    uint32_t n_eval;              // candidates the search evaluated (host replay)
};

// One point of dcreg_verify_poses at the pose P (R row-major, t; state / fresh are not read).  Returns whether the point is an inlier.
// The search is bounded by the inlier distance and starts with HeapOne's key at that bound, so a point with no map point strictly inside
// the bound costs the walk of the cells the ball touches and nothing else; the minimum (d2, index) key over the candidates inside the
// bound is the minimum over the whole map whenever the gate can pass.  A transformed point with a non-finite coordinate (an overflow of
// the float store) is no inlier: tested here, not left to the cell arithmetic of the walk.
DCREG_DEVFN bool verify_point(const GridDev &g, RunList &rl, const PoseArg &P, const VerifyArgs &a, const float4 &s4, VerifyPoint &o) {
#pragma clang fp contract(off)
    float qx, qy, qz;
    body_to_global(P, (double)s4.x, (double)s4.y, (double)s4.z, qx, qy, qz);
    o.idx = kNoIdx; o.d2 = __builtin_inff(); o.e = 0ull; o.n_eval = 0u;
    if (!(nlin_finite(qx) && nlin_finite(qy) && nlin_finite(qz))) return false;
    HeapOne hp;
    hp.start = (uint64_t)__float_as_uint(a.bound_f) << 32;                 // index 0: d2 == bound does not enter
    knn_search<HeapOne>(g, rl, qx, qy, qz, a.bound_f, a.max_ring, hp);
    o.n_eval = hp.n_eval;
    if (hp.pos == kNoIdx) return false;
    const float d2 = __uint_as_float((uint32_t)(hp.key >> 32));
    if (!((double)d2 < a.dd)) return false;
    o.idx = (uint32_t)hp.key; o.d2 = d2;
    o.e = (uint64_t)floor(((double)d2 / a.dd) * 1048576.0);
    return true;
}

}  // namespace dcreg
