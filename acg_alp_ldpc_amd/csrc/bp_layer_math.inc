// The per-check arithmetic of the layered schedule, shared by the wavefront-group kernel (bp_layered.hip) and the
// workgroup-per-frame kernel (bp_layered_block.hip): both include this file inside namespace acg, behind bp_core.inc
// (Dom<float>::phi).  One definition, so the two engines cannot drift apart: tests/layered_ref.py restates exactly these
// functions.
//
// G is the distance, in message cells, between consecutive edges of one check as seen from `Rl`, the address of edge 0 of the
// calling lane's check: the group width in bp_layered.hip (R[layer][edge][lane]), 1 in bp_layered_block.hip (R[check][edge]).

typedef const int32_t __attribute__((address_space(4))) *lsconst_i32;
// a wave-uniform scalar load (I: int here, size_t in the streamed layered engines, whose edge numbers are size_t throughout)
template <typename I>
__device__ __forceinline__ int lsload(const int32_t *p, I i) { return ((lsconst_i32) (p))[i]; }

constexpr int LMAXD = 8;
constexpr float LAYERED_SATURATION = 59968.0f;   // message of a one-variable check ("certainly 0"); representable in fp16
template <int D>
__device__ __forceinline__ void layer_front(unsigned char *__restrict__ Pb, const int (&pos)[LMAXD], const float (&r)[LMAXD],
                                            float *(&addr)[LMAXD], float (&p)[LMAXD], float (&q)[LMAXD]) {
#pragma unroll
    for (int j = 0; j < D; ++j) addr[j] = reinterpret_cast<float *>(Pb + pos[j]);
#pragma unroll
    for (int j = 0; j < D; ++j) p[j] = *addr[j];
#pragma unroll
    for (int j = 0; j < D; ++j) q[j] = p[j] - r[j];
}
// -> sign bit set <=> the step was not quiet for this lane
template <int D, int G, typename RT>
__device__ __forceinline__ uint32_t layer_back(RT *__restrict__ Rl, float *const (&addr)[LMAXD], const float (&p)[LMAXD], const float (&q)[LMAXD],
                                               const bool store, const float scale) {
    uint32_t S = 0, noisy = 0;
    float a[D];
    float m1 = INFINITY, m2 = INFINITY;
#pragma unroll
    for (int j = 0; j < D; ++j) {
        noisy ^= __float_as_uint(p[j]);                     // parity of the hard decisions this check sees
        S ^= __float_as_uint(q[j]);
        a[j] = __uint_as_float(__float_as_uint(q[j]) & 0x7FFFFFFFu);
        m2 = __builtin_amdgcn_fmed3f(a[j], m1, m2);
        m1 = __builtin_fminf(m1, a[j]);
    }
    // the two minima are scaled once per check (made opaque: the compiler would otherwise turn select(s*m2, s*m1) back into
    // s * select(m2, m1), one multiply per edge)
    // (RT = _Float16: rounded to the storage type here, once per check, so that P' adds exactly what the next iteration subtracts)
    uint32_t m1s = __float_as_uint((float) (RT) (scale * m1)) & 0x7FFFFFFFu, m2s = __float_as_uint((float) (RT) (scale * m2)) & 0x7FFFFFFFu;
    // a check with ONE variable pins it to 0: the minimum over its (empty) set of other edges is +inf, and an infinite message
    // would turn the next Q = P - R into inf - inf.  It saturates at a value far above any real message instead (exact in fp16).
    if constexpr (D == 1) m2s = __float_as_uint((float) (RT) LAYERED_SATURATION);
    asm volatile("" : "+v"(m1s), "+v"(m2s));
    float rn[D], pn[D];
#pragma unroll
    for (int j = 0; j < D; ++j) {
        const uint32_t mag = (a[j] == m1) ? m2s : m1s;      // a tie makes m2 == m1: either answer is the same
        rn[j] = __uint_as_float(mag | ((S ^ __float_as_uint(q[j])) & 0x80000000u));
        pn[j] = q[j] + rn[j];
        noisy |= __float_as_uint(pn[j]) ^ __float_as_uint(p[j]);   // a hard decision flipped
    }
    if (store) {
#pragma unroll
        for (int j = 0; j < D; ++j) *addr[j] = pn[j];
#pragma unroll
        for (int j = 0; j < D; ++j) Rl[j * G] = (RT) rn[j];   // (exact: the magnitude is already a value of RT)
    }
    return noisy;
}

// The same step for SUM-PRODUCT (ALGO = 0; the reference's check rule, bp.h:49-57, in the layered schedule): magnitudes through
// phi, exclude-self sums by prefix / suffix (never total - own: an infinite term would turn into NaN), phi again — two phi per
// edge and iteration, as in the flooding kernels, but about half the iterations.  The posteriors and messages live in the
// log2(e)-scaled domain of Dom<float>.  A message saturates at LAYERED_SPA_SATURATION (57.7 in natural units, far beyond the
// reference's own saturation of phi at 45.7): an infinite message would turn the next P - R into inf - inf.
constexpr float LAYERED_SPA_SATURATION = 83.25f;
template <int D, int G, typename RT>
__device__ __forceinline__ uint32_t layer_back_spa(RT *__restrict__ Rl, float *const (&addr)[LMAXD], const float (&p)[LMAXD], const float (&q)[LMAXD],
                                                   const bool store) {
    uint32_t S = 0, noisy = 0;
    float mag[D], pre[D];
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < D; ++j) {
        noisy ^= __float_as_uint(p[j]);                     // parity of the hard decisions this check sees
        S ^= __float_as_uint(q[j]);
        mag[j] = Dom<float>::phi(__uint_as_float(__float_as_uint(q[j]) & 0x7FFFFFFFu));
        pre[j] = s;
        s += mag[j];
    }
    float rn[D], pn[D];
    float suf = 0.0f;
#pragma unroll
    for (int j = D - 1; j >= 0; --j) {
        float out = __builtin_fminf(Dom<float>::phi(pre[j] + suf), LAYERED_SPA_SATURATION);
        suf += mag[j];
        out = (float) (RT) out;                              // (fp16 storage: P' adds exactly what the next iteration subtracts)
        rn[j] = __uint_as_float((__float_as_uint(out) & 0x7FFFFFFFu) | ((S ^ __float_as_uint(q[j])) & 0x80000000u));
        pn[j] = q[j] + rn[j];
        noisy |= __float_as_uint(pn[j]) ^ __float_as_uint(p[j]);
    }
    if (store) {
#pragma unroll
        for (int j = 0; j < D; ++j) *addr[j] = pn[j];
#pragma unroll
        for (int j = 0; j < D; ++j) Rl[j * G] = (RT) rn[j];
    }
    return noisy;
}

#define ACG_LAYER_SWITCH(md, CALL) \
    switch (md) {                  \
        case 1: CALL(1); break;    \
        case 2: CALL(2); break;    \
        case 3: CALL(3); break;    \
        case 4: CALL(4); break;    \
        case 5: CALL(5); break;    \
        case 6: CALL(6); break;    \
        case 7: CALL(7); break;    \
        case 8: CALL(8); break;    \
        default: break;            \
    }
