// The arithmetic of a check of the fixed-point layered min-sum engines (acg_ldpc_quant, include/acg_ldpc.h): ONE definition for
// bp_layered_q.hip (a frame in LDS) and bp_streamed_q.hip (a frame in device memory).  Device code only.
#pragma once

#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace acg {

// mu -> max(((mu * scale_num + rnd) >> scale_shift) - offset, 0)
__device__ __forceinline__ int q_normalise(const int mu, const QuantArgs &qa) {
    const int v = ((mu * qa.scale_num + qa.rnd) >> qa.scale_shift) - qa.offset;
    return v > 0 ? v : 0;
}

// What pass 1 gathers over the edges of a check, and what an edge becomes once all of them have been seen.
struct QCheck {
    int m1, m2;             // the two smallest min(|q|, rmax); both start at rmax — every a_j <= rmax, so the two smallest of {a_j}
                            // and two rmax ARE the two smallest a_j, and a check of one variable gets m2 = rmax
    uint32_t parity, S;     // bit 0: XOR of (P < 0) and of (q < 0) over the edges
    int mu1, mu2;           // normalised m1, m2 (q_close)
};
__device__ __forceinline__ void q_open(QCheck &c, const QuantArgs &qa) {
    c.m1 = c.m2 = qa.rmax;
    c.parity = c.S = 0;
}
__device__ __forceinline__ void q_reduce(QCheck &c, const int p, const int q, const QuantArgs &qa) {
    c.parity ^= (uint32_t) p >> 31;
    c.S ^= (uint32_t) q >> 31;
    const int m = min(abs(q), qa.rmax);
    c.m2 = min(c.m2, max(m, c.m1));
    c.m1 = min(c.m1, m);
}
__device__ __forceinline__ void q_close(QCheck &c, const QuantArgs &qa) {
    c.mu1 = q_normalise(c.m1, qa);
    c.mu2 = q_normalise(c.m2, qa);
}
// the edge with q = p - r: its new message rn and posterior pn
__device__ __forceinline__ void q_update(const QCheck &c, const int q, const QuantArgs &qa, int &rn, int &pn) {
    const int mag = (min(abs(q), qa.rmax) == c.m1) ? c.mu2 : c.mu1;   // a tie makes m2 == m1: either answer is the same
    rn = ((c.S ^ ((uint32_t) q >> 31)) & 1u) ? -mag : mag;
    pn = min(max(q + rn, -qa.pmax), qa.pmax);
}

}  // namespace acg
