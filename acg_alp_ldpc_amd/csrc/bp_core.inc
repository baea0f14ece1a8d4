// Fused BP kernel body — included by bp_inst_*.hip (one translation unit per (type, algorithm) so the
// instantiations compile in parallel) and by bp_kernels.hip (debug kernels).  See bp_kernels.hip for the
// design notes.  Everything here lives in namespace acg.


// ------------------------------------------------------------------------------------------
// bit-level helpers
template <typename T> struct FpBits;
template <> struct FpBits<float> {
    using U = uint32_t;
    static constexpr U SIGN = 0x80000000u;
    static __device__ __forceinline__ U to(float x) { return __float_as_uint(x); }
    static __device__ __forceinline__ float from(U u) { return __uint_as_float(u); }
};
template <> struct FpBits<double> {
    using U = uint64_t;
    static constexpr U SIGN = 0x8000000000000000ull;
    static __device__ __forceinline__ U to(double x) { return (U) __double_as_longlong(x); }
    static __device__ __forceinline__ double from(U u) { return __longlong_as_double((long long) u); }
};

// Single-wave producer/consumer ordering through LDS: the DS queue of one wavefront is in-order,
// so only the compiler has to be stopped from moving accesses across the phase boundary.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// L lanes own a frame: inside one wavefront (L <= 64) ordering is free; a workgroup-sized group needs a barrier
template <int L>
__device__ __forceinline__ void group_sync() {
    if (L <= 64) wave_sync();
    else __syncthreads();
}

// ------------------------------------------------------------------------------------------
// phi(x) = -log(tanh(x/2))   (bp.h:34), x >= 0.
//
// The reference evaluates it in x87 long double, where tanh(x/2) rounds to 1 and phi becomes
// (minus) zero for x >= 45.7477...; phi(0) = +inf; phi(NaN) = NaN.  Those three behaviours are
// reproduced by both variants below.
// fp32 (Dom<float>::phi): ONE transcendental per branch — v_exp_f32 / v_log_f32 issue at 8 cycles per wave
// on gfx950 against 2 for an FMA (tools/microbench/valu_rates.hip, profiles/r02_valu_rates.txt), so they, not the
// polynomials, set the cost of a message:
//   x <  1 : phi = -ln(y) - w*G(w),  y = x/2, w = y^2,  w*G(w) = ln(tanh(y)/y)   (minimax, deg 3 in w)
//   x >= 1 : phi = 2t*(1 + u*R(u)),  t = e^-x, u = t^2, 1 + u*R(u) = atanh(t)/t  (minimax, deg 3 in u)
// (coefficients fitted in long double on Chebyshev nodes; max error 1.4e-8 abs / 4.4e-8 rel before rounding),
// evaluated in the log2(e)-scaled message domain described at Dom<float>.
// fp64 ("strict" mode): library accuracy (~1e-16), natural domain.
__device__ __forceinline__ double phi_f(double x) {
    if (x >= 45.747713916956390) return 0.0;
    if (x >= 1.0) {
        const double t = exp(-x);
        return log1p(2.0 * t / (1.0 - t));
    }
    return -log(tanh(0.5 * x));
}

// ------------------------------------------------------------------------------------------
// Message domain.  The fp32 kernels keep every LLR-domain and phi-domain quantity multiplied by log2(e):
// the algorithm is invariant under a common scale (sums, signs and the self-inverse map
// F(x') = log2(e) * phi(x' * ln 2) are all that is used), and in that domain e^-x is exp2(-x') and ln is
// log2 — the two multiplies in front of / behind the transcendental instructions disappear and the exp
// argument is exact.  F(x') = -log2(x') + C0 + w'*G3(w'), w' = x'^2                 for x' <  log2(e)
//                      = t*(K + u*R2(u)),  t = 2^-x', u = t^2                        for x' >= log2(e)
// (the natural-log minimax fits of phi_f re-expressed; fp32 error <= 1.6e-7 relative over (0, 66)).
// The reference's long-double saturation point 45.7477... is exactly 66 in this domain (2e^-x < 2^-65).
// fp64 ("strict") kernels stay in the natural domain.
#ifndef ACG_IDX_BYTES
#define ACG_IDX_BYTES 1
#endif
#ifndef ACG_SPEC_VIREG
#define ACG_SPEC_VIREG 0
#endif
#ifndef ACG_FUSED_MERGED
#define ACG_FUSED_MERGED 1
#endif
template <typename T> struct Dom;
template <> struct Dom<float> {
    static constexpr double scale = 1.44269504088896341;
    static __device__ __forceinline__ float phi(float x) {
        const float w = x * x;
        float g = fmaf(w, -1.7256659564749327e-06f, 5.431033644982242e-05f);
        g = fmaf(g, w, -0.001618721877195048f);
        g = fmaf(g, w, 0.057762255617977924f);
        const float ps = fmaf(w, g, 1.5287663729448977f) - __builtin_amdgcn_logf(x);
        const float t = __builtin_amdgcn_exp2f(-x);
        const float u = t * t;
        float r = fmaf(u, 0.40731721508362195f, 0.40423844622223065f);
        r = fmaf(r, u, 0.5773059513734762f);
        r = fmaf(r, u, 0.961795680143378f);
        const float pl = t * fmaf(u, r, 2.8853900817779268f);
        // the branch that is out of its range underestimates (pl: truncated series of positive terms; ps: its polynomial runs
        // away to -inf), so the selection by x is the larger of the two — except between 1.397 and 1.500, where both are
        // within their error bound and differ by at most 2.2e-7 relative.  One v_max_f32 instead of compare + select.
        // NaN -> both NaN -> NaN; x = 0 -> ps = +inf; x = +inf -> ps = -inf, pl = 0.
        float o = __builtin_fmaxf(ps, pl);
        // saturation of the reference; also +inf -> 0.  (Measured: replacing this compare + select by a multiplication with
        // clamp((66 - x) * 2^40) — 4 issue cycles instead of 6 by tools/microbench/valu_op_rates — made the kernel 11 % slower.)
        o = (x >= 66.0f) ? 0.0f : o;
        return o;
    }
    // The two series of phi on their own, each with phi's operations, constants and order: what max(ps, pl) picks when x lies
    // well inside one range.  pl >= ps for 2 <= x < 66 and ps >= pl for 0 < x <= 1, with a gap of more than 170 ulps at the
    // thresholds (tests/phi_split_check.cpp in the float model, tests/test_phi_split_gpu.py on every bit pattern), so there
    // the one series gives phi's bits.  See BpPass::word_c / word_v (SPLIT).
    static __device__ __forceinline__ float phi_small(float x) {
        const float w = x * x;
        float g = fmaf(w, -1.7256659564749327e-06f, 5.431033644982242e-05f);
        g = fmaf(g, w, -0.001618721877195048f);
        g = fmaf(g, w, 0.057762255617977924f);
        return fmaf(w, g, 1.5287663729448977f) - __builtin_amdgcn_logf(x);
    }
    static __device__ __forceinline__ float phi_large(float x) {
        const float t = __builtin_amdgcn_exp2f(-x);
        const float u = t * t;
        float r = fmaf(u, 0.40731721508362195f, 0.40423844622223065f);
        r = fmaf(r, u, 0.5773059513734762f);
        r = fmaf(r, u, 0.961795680143378f);
        return t * fmaf(u, r, 2.8853900817779268f);
    }
};
// the thresholds of the split, in the scaled domain (not 1.397 and 1.5, where the two series are one ulp apart)
#define ACG_PHI_SPLIT_LO 1.0f
#define ACG_PHI_SPLIT_HI 2.0f
template <> struct Dom<double> {
    static constexpr double scale = 1.0;
    static __device__ __forceinline__ double phi(double x) { return phi_f(x); }
};

// ------------------------------------------------------------------------------------------
// Philox4x32-10 (Salmon et al. 2011), counter = (frame_lo, frame_hi, quad, 0), key = seed.
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                              uint32_t k1, uint32_t out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0;
        c1 = lo1;
        c2 = n2;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0;
    out[1] = c1;
    out[2] = c2;
    out[3] = c3;
}

// two uint32 -> two N(0,1) (Box-Muller; u1 in (0,1) with a 2^-33 floor: tails to 6.7 sigma)
__device__ __forceinline__ void box_muller(uint32_t a, uint32_t b, float &z0, float &z1) {
    const float u1 = ((float) a + 0.5f) * 2.3283064365386963e-10f;          // (a+0.5)/2^32
    const float u2 = (float) (b >> 8) * 5.9604644775390625e-08f;           // [0,1) 24 bits, in revolutions
    const float r = sqrtf(-2.0f * 0.693147180559945309f * __builtin_amdgcn_logf(u1));
    z0 = r * __builtin_amdgcn_cosf(u2);
    z1 = r * __builtin_amdgcn_sinf(u2);
}

// ------------------------------------------------------------------------------------------
// Wave-uniform tables are read through the constant address space so the compiler issues scalar
// (SMEM) loads into SGPRs instead of per-lane vector loads followed by v_readfirstlane.
typedef const int32_t __attribute__((address_space(4))) *sconst_i32;
__device__ __forceinline__ int sload(const int32_t *p, int i) { return ((sconst_i32) (p))[i]; }

// ------------------------------------------------------------------------------------------
// One pass = the L nodes dealt to the L lanes of a frame group.  D (the largest degree in the
// pass) is a compile-time constant: the D LDS reads are issued back to back, then everything is
// straight-line register code, then the D LDS writes.  Dispatch on D is a wave-uniform switch.
// SAT: the phi fast path (phi_c / phi_v) in check, check_abs and var_at, for fp32 sum-product (BpCore::SATSKIP)
template <typename T, int D, int L, int ALGO, bool SAT = false>
struct BpPass {
    using B = FpBits<T>;
    using U = typename B::U;
    static constexpr U SIGN = B::SIGN;
    static constexpr U ONE = (U) 1;

    // phi where its value is fixed, without evaluating it (in fixed-work runs most frames have converged and their messages
    // saturated long before the last sweep).  The test sits under the lane's store predicate, so phi runs under
    // EXEC = (store && not saturated): a 32-lane half of the wavefront with no such lane issues it in one pass, or none.
    //   check side: an exclude-self sum (>= 0) that is exactly +0 (integer test: NaN and denormals fail) -> +inf
    //   variable side: a magnitude ax >= 66 (the saturation point, +inf included; NaN fails) -> +0
    // The check side is a one-entry memo: an input whose bits are mb gives G = phi(mb), computed once per frame (mb = +0,
    // G = +inf is the rule above).  Bit-identical by construction: phi would see the same bits.
    static __device__ __forceinline__ T phi_c(T s, U mb, T G) {
        T o = G;
        if (B::to(s) != mb) o = Dom<T>::phi(s);
        return o;
    }
    static __device__ __forceinline__ T phi_c(T s) { return phi_c(s, (U) 0, (T) INFINITY); }
    static __device__ __forceinline__ T phi_v(T ax) {
        T o = (T) 0;
        if (!(ax >= (T) 66)) o = Dom<T>::phi(ax);
        return o;
    }
    // The sweeps do not merge phi_c / phi_v's default value with phi's result: they form the word to store on both paths (the
    // same bits; one copy of the default and the merge behind the branch less per row).
    //   check side: sg = the sign of the outgoing message; the word is sg | magnitude bits of G, or of phi(s)
    //   variable side: w = the sign and the hard-decision LSB; phi's magnitude bits are or-ed in unless phi is +0
    // test: the row keeps its fast-path test (bit of the pass's row mask, see PassRuntime); without it phi is evaluated under
    // the store predicate alone, which gives the same bits: phi(+0) = +inf, phi(>= 66) = +0, and the memo returns phi of the
    // bits phi would see.
    // SPLIT / split (fp32; a row that keeps its test and whose bit of the pass's split mask is set, see PassRuntime): the lanes
    // that evaluate phi are those left under EXEC by the test.  A wavefront none of whose evaluating lanes lies on the wrong side
    // of a threshold needs one series of phi only: check side every s <= 1 -> phi_small, variable side every ax >= 2 -> phi_large
    // (the same bits, Dom<float>::phi_small).  One v_cmp into a scalar mask and a scalar branch between two alternative blocks;
    // NaN fails both compares and takes the full phi, and the x >= 66 select exists on the full path only (a wavefront that is
    // all <= 1 cannot reach it).  The decision per 32-lane half, with the second series under the mask of the halves that need
    // it, evaluates fewer series and measured slower (DESIGN §3).
    template <bool SPLIT = false>
    static __device__ __forceinline__ U word_c(T s, U mb, T G, U sg, bool test, bool split = false) {
        if (!test) return (B::to(Dom<T>::phi(s)) & ~SIGN) | sg;
        U w = (B::to(G) & ~SIGN) | sg;
        if constexpr (SPLIT && sizeof(T) == 4) {
            if (split) {
                if (B::to(s) != mb) {
                    T o;
                    if (__ballot(!(s <= (T) ACG_PHI_SPLIT_LO)) == 0ull) o = Dom<T>::phi_small(s);
                    else o = Dom<T>::phi(s);
                    w = (B::to(o) & ~SIGN) | sg;
                }
                return w;
            }
        }
        if (B::to(s) != mb) w = (B::to(Dom<T>::phi(s)) & ~SIGN) | sg;
        return w;
    }
    template <bool SPLIT = false>
    static __device__ __forceinline__ U word_v(T ax, U w, bool test, bool split = false) {
        if (!test) return w | (B::to(Dom<T>::phi(ax)) & ~SIGN & ~ONE);
        if constexpr (SPLIT && sizeof(T) == 4) {
            if (split) {
                if (!(ax >= (T) 66)) {
                    T o;
                    if (__ballot(!(ax >= (T) ACG_PHI_SPLIT_HI)) == 0ull) o = Dom<T>::phi_large(ax);
                    else o = Dom<T>::phi(ax);
                    w |= B::to(o) & ~SIGN & ~ONE;
                }
                return w;
            }
        }
        if (!(ax >= (T) 66)) w |= B::to(Dom<T>::phi(ax)) & ~SIGN & ~ONE;
        return w;
    }

    // check(), sum-product with the fast path: the exclude-self sums first, phi per edge under its store predicate
    // rows: bit j set = edge row j keeps its fast-path test (a constant of the pass: all ones, or a static policy's c_sat_rows)
    // SPLIT / srows: bit j set = edge row j takes the one-series phi where its unit allows (word_c; a constant of the pass as rows is)
    template <bool SPLIT = false>
    static __device__ __forceinline__ U check_sat(T *__restrict__ Ap, int slot, const int *cnt, bool write, unsigned rows, unsigned srows = 0u) {
        T x[D];
#pragma unroll
        for (int j = 0; j < D; ++j) x[j] = Ap[j * L];
        U S = 0;
#pragma unroll
        for (int j = 0; j < D; ++j) S ^= B::to(x[j]);
        T mag[D], pre[D], es[D];
        T s = 0;
#pragma unroll
        for (int j = 0; j < D; ++j) {
            mag[j] = B::from(B::to(x[j]) & ~SIGN & ~ONE);
            pre[j] = s;
            s += mag[j];
        }
        T suf = 0;
#pragma unroll
        for (int j = D - 1; j >= 0; --j) {
            es[j] = pre[j] + suf;
            suf += mag[j];
        }
#pragma unroll
        for (int j = 0; j < D; ++j) {
            if (write && slot < cnt[j + 1])
                Ap[j * L] = B::from(word_c<SPLIT>(es[j], (U) 0, (T) INFINITY, (S ^ B::to(x[j])) & SIGN, (rows >> j) & 1u, (srows >> j) & 1u));
        }
        return S;
    }

    // syndrome contribution of the checks in this pass (LSB of the XOR of the v->c words)
    static __device__ __forceinline__ U syn(const T *__restrict__ Ap) {
        T x[D];
#pragma unroll
        for (int j = 0; j < D; ++j) x[j] = Ap[j * L];
        U S = 0;
#pragma unroll
        for (int j = 0; j < D; ++j) S ^= B::to(x[j]);
        return S;
    }

    // the same for a pass with an absorbed variable (BpLayout::n_apass): D - 1 rows of words, then the register word aw
    static __device__ __forceinline__ U syn_abs(const T *__restrict__ Ap, U aw) {
        T x[D];
#pragma unroll
        for (int j = 0; j < D - 1; ++j) x[j] = Ap[j * L];
        U S = aw;
#pragma unroll
        for (int j = 0; j < D - 1; ++j) S ^= B::to(x[j]);
        return S;
    }

    // check -> variable (bp.h:171-181 / CNode::message bp.h:49-57), in place.  cnt[j] = number of
    // checks of degree >= j: slot < cnt[j+1] <=> edge j of this lane's check exists.
    // Returns the XOR of the incoming words: its LSB is the syndrome bit of this lane's check (padding words are +0).
    // UNI: every check of the code has degree D (the caller checked c_cnt_ge[D] == m): one write predicate for the whole
    // pass instead of one compare + EXEC mask + branch per edge
    template <bool UNI = false, bool SPLIT = false>
    static __device__ __forceinline__ U check(T *__restrict__ Ap, int slot, const int *cnt, bool write, T ms_scale, unsigned rows = ~0u, unsigned srows = 0u) {
        if constexpr (SAT && ALGO == 0 && !UNI) return check_sat<SPLIT>(Ap, slot, cnt, write, rows, srows);
        T x[D];
#pragma unroll
        for (int j = 0; j < D; ++j) x[j] = Ap[j * L];
        U S = 0;
#pragma unroll
        for (int j = 0; j < D; ++j) S ^= B::to(x[j]);
        T out[D];
        if (ALGO == 0) {
            // exclude-self sums of the phi magnitudes: prefix + suffix (bp.h:50-55)
            T mag[D], pre[D];
            T s = 0;
#pragma unroll
            for (int j = 0; j < D; ++j) {
                mag[j] = B::from(B::to(x[j]) & ~SIGN & ~ONE);  // the LSB is the hard bit, not magnitude: inf|1 would be NaN
                pre[j] = s;
                s += mag[j];
            }
            T suf = 0;
#pragma unroll
            for (int j = D - 1; j >= 0; --j) {
                out[j] = Dom<T>::phi(pre[j] + suf);
                suf += mag[j];
            }
        } else {
            // min-sum: two smallest magnitudes (padding slots are +0 and must not take part)
            // the new second minimum is the median of (a, m1, m2), the new minimum min(m1, a): two instructions per edge
            // (v_med3_f32 / v_min_f32) instead of two compares and four selects; the edge that holds the minimum is found
            // again by value (a tie makes m2 == m1, so it does not matter which of the tied edges "is" the minimum)
            T m1 = (T) INFINITY, m2 = (T) INFINITY;
            T mag[D];
#pragma unroll
            for (int j = 0; j < D; ++j) {
                const T a0 = B::from(B::to(x[j]) & ~SIGN & ~ONE);
                const T a = (UNI || slot < cnt[j + 1]) ? a0 : (T) INFINITY;  // (UNI: lanes beyond the last check see zeros and never write)
                mag[j] = a;
                if constexpr (sizeof(T) == 4) m2 = __builtin_amdgcn_fmed3f(a, m1, m2);
                else m2 = __builtin_fmin(m2, __builtin_fmax(a, m1));
                m1 = (sizeof(T) == 4) ? (T) __builtin_fminf((float) m1, (float) a) : (T) __builtin_fmin((double) m1, (double) a);
            }
            // (the two minima are scaled once per check, not the selected one once per edge: same products, D - 2 fewer)
            const T m1s = ms_scale * m1, m2s = ms_scale * m2;
#pragma unroll
            for (int j = 0; j < D; ++j) out[j] = (mag[j] == m1) ? m2s : m1s;
        }
        if (UNI) {
            U obv[D];
#pragma unroll
            for (int j = 0; j < D; ++j) obv[j] = (B::to(out[j]) & ~SIGN) | ((S ^ B::to(x[j])) & SIGN);  // sign product, bp.h:54
            if (write && slot < cnt[D]) {
#pragma unroll
                for (int j = 0; j < D; ++j) Ap[j * L] = B::from(obv[j]);
            }
            return S;
        }
#pragma unroll
        for (int j = 0; j < D; ++j) {
            const U ob = (B::to(out[j]) & ~SIGN) | ((S ^ B::to(x[j])) & SIGN);  // sign product, bp.h:54
            // predicated store: hipcc sinks the phi evaluation under the same EXEC mask, and a wave64 op whose
            // upper or lower 32 lanes are all masked off issues in one pass on the SIMD-32 — measured faster
            // than a branch-free variant that stores padding to a dump word
            if (write && slot < cnt[j + 1]) Ap[j * L] = B::from(ob);
        }
        return S;
    }

    // Sum-product check sweep of a pass whose edge D - 1 is an absorbed degree-1 variable (BpLayout::n_apass): edges
    // 0 .. D-2 are message words as in check() (a check of lower degree has padding rows before the absorbed edge: +0
    // added to the non-negative phi sums changes no bit, so every sum is the one check() forms), edge D - 1 is the
    // variable's v->c word aw, held in a register.  That word never changes but for its LSB: the variable has no other
    // check, so its v->c message is llr + (empty sum), i.e. F(|llr|) with the sign of llr <= 0 (bp.h:78-82), built once per
    // frame.  The c->v word R of edge D - 1 is not stored; it gives the variable's posterior hard decision llr + R <= 0
    // (bp.h:85-90,193, NaN -> 0), which becomes the LSB of aw, exactly as the variable sweep would have set it.  Lanes
    // without a check (slot >= cnt[1]) keep aw = +0.  r_out: R (debug trace).
    // SAT: the exclude-self sum of every edge but D - 1 contains aw's magnitude m, and once the check's other inputs have
    // saturated to +0 (or fall below half an ulp of m) it IS m, in every sweep that follows: the memo of phi_c holds m's
    // bits (aw & am; am = the magnitude mask, or 0 to turn the memo off) and ag = phi(m), built with aw (BpCore::abs_phi).
    // Edge D - 1 keeps the +0 rule.  rows: as check_sat's, bit D - 1 is the register edge's.
    template <bool SPLIT = false>
    static __device__ __forceinline__ U check_abs(T *__restrict__ Ap, int slot, const int *cnt, bool write, U &aw, T allr, T &r_out,
                                                  T ag = (T) INFINITY, U am = 0, unsigned rows = ~0u, unsigned srows = 0u) {
        T x[D];
#pragma unroll
        for (int j = 0; j < D - 1; ++j) x[j] = Ap[j * L];
        x[D - 1] = B::from(aw);
        U S = 0;
#pragma unroll
        for (int j = 0; j < D; ++j) S ^= B::to(x[j]);
        T out[D];
        T mag[D], pre[D];
        T s = 0;
#pragma unroll
        for (int j = 0; j < D; ++j) {
            mag[j] = B::from(B::to(x[j]) & ~SIGN & ~ONE);
            pre[j] = s;
            s += mag[j];
        }
        T suf = 0;
        if constexpr (SAT) {  // exclude-self sums; phi (fast path) per edge under its store predicate
#pragma unroll
            for (int j = D - 1; j >= 0; --j) {
                out[j] = pre[j] + suf;
                suf += mag[j];
            }
            const U mb = aw & am;
#pragma unroll
            for (int j = 0; j < D - 1; ++j) {
                if (write && slot < cnt[j + 2])
                    Ap[j * L] = B::from(word_c<SPLIT>(out[j], mb, ag, (S ^ B::to(x[j])) & SIGN, (rows >> j) & 1u, (srows >> j) & 1u));
            }
            if (write && slot < cnt[1]) {
                const T R = B::from(word_c<SPLIT>(out[D - 1], (U) 0, (T) INFINITY, (S ^ aw) & SIGN, (rows >> (D - 1)) & 1u, (srows >> (D - 1)) & 1u));
                r_out = R;
                aw = (aw & ~ONE) | ((allr + R <= (T) 0) ? ONE : (U) 0);
            }
            return S;
        }
#pragma unroll
        for (int j = D - 1; j >= 0; --j) {
            out[j] = Dom<T>::phi(pre[j] + suf);
            suf += mag[j];
        }
#pragma unroll
        for (int j = 0; j < D - 1; ++j) {
            const U ob = (B::to(out[j]) & ~SIGN) | ((S ^ B::to(x[j])) & SIGN);
            if (write && slot < cnt[j + 2]) Ap[j * L] = B::from(ob);  // edge j is a message word of checks of degree >= j + 2
        }
        if (write && slot < cnt[1]) {
            const T R = B::from((B::to(out[D - 1]) & ~SIGN) | ((S ^ aw) & SIGN));
            r_out = R;
            aw = (aw & ~ONE) | ((allr + R <= (T) 0) ? ONE : (U) 0);
        }
        return S;
    }

    // variable -> check (bp.h:160-169 / VNode::message bp.h:77-83) + posterior hard decision
    // (bp.h:85-90,193), whose bit rides in the LSB of every outgoing magnitude.
    // BYTES: the positions are byte offsets into A (the fused kernels' LDS copy of the table is stored that way: a
    // plain add instead of a shift-add, which issues at half the rate on gfx950, per message access)
    template <bool BYTES>
    static __device__ __forceinline__ T &at(T *__restrict__ A, int pos) {
        return BYTES ? *reinterpret_cast<T *>(reinterpret_cast<unsigned char *>(A) + pos) : A[pos];
    }
    template <typename IdxPtr, bool BYTES = false, bool SPLIT = false>
    static __device__ __forceinline__ U var(T *__restrict__ A, IdxPtr ip, T llr, int slot, const int *cnt, bool write, unsigned rows = ~0u, unsigned srows = 0u) {
        int pos[D];
#pragma unroll
        for (int k = 0; k < D; ++k) pos[k] = ip[k * L];
        return var_at<false, BYTES, SPLIT>(A, pos, llr, slot, cnt, write, rows, srows);
    }

    // the same sweep with the D message positions already known (register-resident index table)
    // Returns the posterior hard decision (0 / 1).
    // rows (SAT): bit k set = edge row k keeps its fast-path test, as check_sat's; SPLIT / srows: as check_sat's (word_v)
    template <bool UNI = false, bool BYTES = false, bool SPLIT = false>
    static __device__ __forceinline__ U var_at(T *__restrict__ A, const int (&pos)[D], T llr, int slot, const int *cnt, bool write,
                                               unsigned rows = ~0u, unsigned srows = 0u) {
        T c[D];
#pragma unroll
        for (int k = 0; k < D; ++k) c[k] = at<BYTES>(A, pos[k]);
        T pre[D];
        T s = 0;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            pre[k] = s;
            s += c[k];
        }
        const T total = llr + s;                            // estimate(), bp.h:85-90
        const U hard = (total <= (T) 0) ? ONE : (U) 0;      // bp.h:193 (NaN -> 0)
        const U hard_neg = hard | SIGN;
        T suf = 0;
        if constexpr (SAT && ALGO == 0 && !UNI) {  // phi (fast path) per edge under its store predicate
            T xs[D];
#pragma unroll
            for (int k = D - 1; k >= 0; --k) {
                xs[k] = llr + (pre[k] + suf);
                suf += c[k];
            }
#pragma unroll
            for (int k = 0; k < D; ++k) {
                if (write && slot < cnt[k + 1])
                    at<BYTES>(A, pos[k]) = B::from(word_v<SPLIT>(B::from(B::to(xs[k]) & ~SIGN), (xs[k] <= (T) 0) ? hard_neg : hard, (rows >> k) & 1u, (srows >> k) & 1u));
            }
            return hard;
        }
        U ob[D];
#pragma unroll
        for (int k = D - 1; k >= 0; --k) {
            const T xk = llr + (pre[k] + suf);              // bp.h:78-82
            suf += c[k];
            const T ax = B::from(B::to(xk) & ~SIGN);
            const T mg = (ALGO == 0) ? Dom<T>::phi(ax) : ax;
            // magnitude bits | hard-decision LSB | message sign (x <= 0 -> -1, bp.h:82): one and-or
            ob[k] = (B::to(mg) & ~SIGN & ~ONE) | ((xk <= (T) 0) ? hard_neg : hard);
        }
        if (UNI) {  // every variable has degree D: one predicate for the pass
            if (write && slot < cnt[D]) {
#pragma unroll
                for (int k = 0; k < D; ++k) at<BYTES>(A, pos[k]) = B::from(ob[k]);
            }
            return hard;
        }
#pragma unroll
        for (int k = 0; k < D; ++k)
            if (write && slot < cnt[k + 1]) at<BYTES>(A, pos[k]) = B::from(ob[k]);
        return hard;
    }

    // first variable -> check sweep of a frame (bp.h:184): every mailbox is (0, +1), so all D outgoing messages
    // of a variable are the same word phi(|llr|) — one evaluation instead of D, and A need not be cleared first
    template <typename IdxPtr, bool BYTES = false>
    static __device__ __forceinline__ void var_init(T *__restrict__ A, IdxPtr ip, T llr, int slot, const int *cnt, bool write) {
        int pos[D];
#pragma unroll
        for (int k = 0; k < D; ++k) pos[k] = ip[k * L];
        const U hard = (llr <= (T) 0) ? ONE : (U) 0;
        const T ax = B::from(B::to(llr) & ~SIGN);
        const T mg = (ALGO == 0) ? Dom<T>::phi(ax) : ax;
        const U ob = (B::to(mg) & ~SIGN & ~ONE) | ((llr <= (T) 0) ? (hard | SIGN) : hard);
#pragma unroll
        for (int k = 0; k < D; ++k)
            if (write && slot < cnt[k + 1]) at<BYTES>(A, pos[k]) = B::from(ob);
    }
};

// ------------------------------------------------------------------------------------------
// Pass structure policy: where a kernel takes the values that are the same for every lane of every frame of a code — the
// pass tables (c_pass, v_pass), the degree histograms (c_cnt_ge, v_cnt_ge) and the pass counts.
//   PassRuntime (the default): from BpTables, through scalar loads; one instance serves every code.
//   a static policy (generated per code by tools/bp_spec_gen.cpp, see bp_inst_spec.hip): STATIC = true, the counts as
//   constants n_cpass / n_apass / n_vpass and the tables as constexpr look-ups c_pass(i), v_pass(i), c_cnt_ge(j), v_cnt_ge(j).
//   The pass loops are then unrolled at compile time: the switch on the degree, the table loads, the register indexing
//   and every store predicate that is true (or false) for a whole pass fold away.  The index tables, the messages and
//   all arithmetic are the run-time policy's, so the results are the same bit for bit.
// The phi fast-path tests are a per-row property of the policy as well: c_sat_rows(p) / v_sat_rows(p), bit j set = edge row j
// of check / variable pass p keeps its test (BpPass::word_c / word_v; in an absorbed pass bit D - 1 is the register edge, the
// bits below it the memo rows).  The mask reaches the sweeps as an argument that is a constant once the unrolled pass loop is
// inlined, like the pass tables.  The generator can clear rows from a census of the code (tools/bp_spec_gen.cpp -t); by default,
// and in the run-time policy, every row keeps its test: on H05 no cleared row measured faster (DESIGN §3).
struct PassRuntime {
    static constexpr bool STATIC = false;
    static constexpr unsigned c_sat_rows(int) { return ~0u; }
    static constexpr unsigned v_sat_rows(int) { return ~0u; }
    // rows that take the one-series phi where the wavefront allows (BpPass::word_c / word_v, SPLIT), same bit order: every row
    static constexpr unsigned c_split_rows(int) { return ~0u; }
    static constexpr unsigned v_split_rows(int) { return ~0u; }
};
// the pass loops: `for (p = 0 .. n - 1) BODY` as a loop (run-time policy) or as straight-line code (static policy: n is one
// of its constants).  BODY is a macro that holds the braces of the loop body.
#define ACG_PASS_LOOP(ST, p, n, BODY)                                                                          \
    if constexpr (ST) {                                                                                        \
        _Pragma("unroll") for (int p = 0; p < (n); ++p) BODY                                                   \
    } else {                                                                                                   \
        for (int p = 0; p < (n); ++p) BODY                                                                     \
    }

#define ACG_PASS_SWITCH(md, CALL)                                                                              \
    switch (md) {                                                                                              \
        case 1: CALL(1); break;                                                                                \
        case 2: CALL(2); break;                                                                                \
        case 3: CALL(3); break;                                                                                \
        case 4: CALL(4); break;                                                                                \
        case 5: CALL(5); break;                                                                                \
        case 6: CALL(6); break;                                                                                \
        case 7: CALL(7); break;                                                                                \
        case 8: CALL(8); break;                                                                                \
        default: break;                                                                                        \
    }

// One frame-group's view of the kernel state.
// NVP > 0: the channel LLRs of a lane's variables live in registers (llr_reg[pass], addressed with the wave-uniform
// pass index -> s_set_gpr_idx), which takes them out of LDS: 4.8 -> 3.6 KB per frame for H05 at L=32, i.e. 5 instead
// of 4 resident workgroups per CU.  NVP = 0 (more than NVP variable passes): LLRs in LDS.
// IDXB: the table behind IDX holds byte offsets into A (see BpPass::at)
// SAT: the phi fast path in the sweeps, see SATSKIP
// PS: the pass structure policy (PassRuntime, or a code's constants)
template <typename T, int MAXD, int L, int ALGO, bool IDXLDS, int NVP, bool IDXB = false, bool SAT = false, typename PS = PassRuntime>
struct BpCore {
    using B = FpBits<T>;
    using U = typename B::U;
    static constexpr U SIGN = B::SIGN;
    static constexpr U ONE = (U) 1;

    const BpTables &t;
    T *__restrict__ A;          // messages, in place (LDS)
    T *__restrict__ LLR;        // channel LLR per variable slot (LDS)
    uint32_t *__restrict__ OB;  // packed hard decisions staging (LDS)
    const uint16_t *IDX;        // variable-side index table: block-shared LDS copy or global
    const int l;                // lane within the frame group
    const T ms_scale;
    int ccnt[MAXD + 2], vcnt[MAXD + 2];  // wave-uniform (SGPR) degree histograms
    // the register copy of the LLRs is a plain local array of the kernel (a struct member indexed dynamically
    // would push the whole object into scratch); it is handed to the sweeps by reference
    using LlrRegs = T[NVP > 0 ? NVP : 1];
    using VarIds = int[NVP > 0 ? NVP : 1];  // variable id of (pass, this lane): frame independent, loaded once per kernel
    // absorbed degree-1 variables (BpPass::check_abs): per absorbed pass q, the variable's channel LLR and its v->c word
    // (hard decision in the LSB) in registers of its check's lane.  Instances with register LLRs, fp32 sum-product only
    // (the host absorbs nothing for the others) and wave-group kernels (L <= 64).
    static constexpr int NAP = (NVP > 0 && ALGO == 0 && sizeof(T) == 4 && MAXD <= 8 && L <= 64) ? BP_MAX_APASS : 0;
    using AbsLlr = T[NAP > 0 ? NAP : 1];
    using AbsWord = U[NAP > 0 ? NAP : 1];
    __device__ __forceinline__ int n_apass() const {
        if constexpr (PS::STATIC) return NAP > 0 ? PS::n_apass : 0;
        else return NAP > 0 ? t.n_apass : 0;
    }
    // the pass structure, by policy
    static constexpr bool STATIC = PS::STATIC;
    __device__ __forceinline__ int n_cpass() const {
        if constexpr (PS::STATIC) return PS::n_cpass;
        else return t.n_cpass;
    }
    __device__ __forceinline__ int n_vpass() const {
        if constexpr (PS::STATIC) return PS::n_vpass;
        else return t.n_vpass;
    }
    __device__ __forceinline__ int c_pass(int i) const {
        if constexpr (PS::STATIC) return PS::c_pass(i);
        else return sload(t.c_pass, i);
    }
    __device__ __forceinline__ int v_pass(int i) const {
        if constexpr (PS::STATIC) return PS::v_pass(i);
        else return sload(t.v_pass, i);
    }
    __device__ __forceinline__ int abs_var(int q) const { return t.a_var[q * L + l]; }
    // the constant v->c word of an absorbed variable: var_init's word (its first sweep) for a variable of degree 1
    static __device__ __forceinline__ U abs_word(T llr) {
        const T ax = B::from(B::to(llr) & ~SIGN);
        const T mg = Dom<T>::phi(ax);
        return (B::to(mg) & ~SIGN & ~ONE) | ((llr <= (T) 0) ? (ONE | SIGN) : (U) 0);
    }
    // the memo of the absorbed pass's phi_c (SATSKIP, BpPass::check_abs): phi of the word's magnitude, once per frame; memo
    // mask am = 0 (off) -> +inf, the +0 rule
    static __device__ __forceinline__ T abs_phi(U aw, U am) { return am != 0 ? Dom<T>::phi(B::from(aw & am)) : (T) INFINITY; }
    static constexpr U MEMO_MASK = ~SIGN & ~ONE;
    // phi fast path (BpPass::phi_c / phi_v) of the fp32 sum-product wave-group sweeps.  Its own instances, which the host
    // takes for fixed-work decoders only: with early exit few frames stay long enough to saturate, and the test and its
    // EXEC-mask branch per edge (2 vector + 3 scalar instructions) would cost more than the skipped phi evaluations save
    static constexpr bool SATSKIP = SAT && ALGO == 0 && sizeof(T) == 4 && L <= 64;
    // REGS = false: read from the table every time (an instance that needs the registers more than the load, see bp_fused_body)
    template <bool REGS = true>
    __device__ __forceinline__ int var_id(const VarIds &vi, int p) const { return (NVP > 0 && REGS) ? vi[p] : t.v_var[p * L + l]; }
    __device__ __forceinline__ T get_llr(const LlrRegs &lr, int p, int slot) const { return NVP > 0 ? lr[p] : LLR[slot]; }
    __device__ __forceinline__ void set_llr(LlrRegs &lr, int p, int slot, T v) {
        if (NVP > 0) lr[p] = v;
        else LLR[slot] = v;
    }

    __device__ BpCore(const BpTables &t_, T *A_, T *LLR_, uint32_t *OB_, const uint16_t *IDX_, int l_, float s_)
        : t(t_), A(A_), LLR(LLR_), OB(OB_), IDX(IDX_), l(l_), ms_scale((T) s_) {
#pragma unroll
        for (int j = 0; j < MAXD + 2; ++j) {
            if constexpr (PS::STATIC) {
                ccnt[j] = PS::c_cnt_ge(j);
                vcnt[j] = PS::v_cnt_ge(j);
            } else {
                ccnt[j] = sload(t.c_cnt_ge, j);
                vcnt[j] = sload(t.v_cnt_ge, j);
            }
        }
    }

    // XOR of the hard-decision bits of each check's variables -> true if any check of this lane fails
    __device__ __forceinline__ bool syndrome_bad(const AbsWord &aw) const {
        U acc = 0;
        const int nc = n_cpass() - n_apass();
#pragma unroll
        for (int q = 0; q < NAP; ++q) {
            if (q < n_apass()) {
                const int md = c_pass(2 * (nc + q));
                const T *Ap = A + c_pass(2 * (nc + q) + 1) + l;
#define ACG_CALL(D) acc |= BpPass<T, D, L, ALGO>::syn_abs(Ap, aw[q])
                ACG_PASS_SWITCH(md, ACG_CALL)
#undef ACG_CALL
            }
        }
#define ACG_CALL(D) acc |= BpPass<T, D, L, ALGO>::syn(Ap)
#define ACG_BODY                                                       \
    {                                                                  \
        const int md = c_pass(2 * p);                                  \
        const T *Ap = A + c_pass(2 * p + 1) + l;                       \
        if (MAXD <= 8 || md <= 8) {                                    \
            ACG_PASS_SWITCH(md, ACG_CALL)                              \
        } else {                                                       \
            U S = 0;                                                   \
            for (int j = 0; j < md; ++j) S ^= B::to(Ap[j * L]);        \
            acc |= S;                                                  \
        }                                                              \
    }
        ACG_PASS_LOOP(STATIC, p, nc, ACG_BODY)
#undef ACG_BODY
#undef ACG_CALL
        return (acc & ONE) != 0;
    }

    // Returns the OR over this lane's checks of the XOR of the incoming words: bit 0 set <=> one of them fails the syndrome of
    // the hard decisions that ride in the v->c words (the estimate of the previous variable sweep).
    // aw / al / ar: the absorbed variables' words, LLRs and (debug trace) c->v messages, see BpPass::check_abs; ag / am: the
    // phi memo of the SATSKIP sweeps (abs_phi, wave-uniform mask am)
    // SPLIT: the sweep compiled with the one-series phi of BpPass::word_c in the rows of PS::c_split_rows
    template <bool SPLIT = false>
    __device__ __forceinline__ U check_phase(bool write, AbsWord &aw, const AbsLlr &al, AbsLlr &ar, const AbsLlr &ag, U am) {
        U acc = 0;
        const int nc = n_cpass() - n_apass();
#define ACG_CALL(D) acc |= BpPass<T, D, L, ALGO, SATSKIP>::template check<false, SPLIT>(Ap, slot, ccnt, write, ms_scale, PS::c_sat_rows(p), PS::c_split_rows(p))
#define ACG_BODY                                                       \
    {                                                                  \
        const int md = c_pass(2 * p);                                  \
        T *Ap = A + c_pass(2 * p + 1) + l;                             \
        const int slot = p * L + l;                                    \
        if (MAXD <= 8 || md <= 8) {                                    \
            ACG_PASS_SWITCH(md, ACG_CALL)                              \
        } else {                                                       \
            acc |= check_generic(Ap, slot, md, write);                 \
        }                                                              \
    }
        ACG_PASS_LOOP(STATIC, p, nc, ACG_BODY)
#undef ACG_BODY
#undef ACG_CALL
        // the absorbed passes (the last ones) with their register operands addressed directly: unrolled over q
#pragma unroll
        for (int q = 0; q < NAP; ++q) {
            if (q < n_apass()) {
                const int p = nc + q;
                const int md = c_pass(2 * p);
                T *Ap = A + c_pass(2 * p + 1) + l;
                const int slot = p * L + l;
#define ACG_CALL(D) acc |= BpPass<T, D, L, ALGO, SATSKIP>::template check_abs<SPLIT>(Ap, slot, ccnt, write, aw[q], al[q], ar[q], ag[q], am, PS::c_sat_rows(p), PS::c_split_rows(p))
                ACG_PASS_SWITCH(md, ACG_CALL)
#undef ACG_CALL
            }
        }
        return acc;
    }
    __device__ __forceinline__ bool syndrome_bad() const {
        AbsWord aw = {};
        return syndrome_bad(aw);
    }
    __device__ __forceinline__ U check_phase(bool write) {
        AbsWord aw = {};
        AbsLlr al = {}, ar = {}, ag;
#pragma unroll
        for (int q = 0; q < (NAP > 0 ? NAP : 1); ++q) ag[q] = (T) INFINITY;
        return check_phase(write, aw, al, ar, ag, 0);
    }

    template <bool SPLIT = false>
    __device__ __forceinline__ void var_phase(const LlrRegs &lr, bool write) {
#define ACG_CALL(D) BpPass<T, D, L, ALGO, SATSKIP>::template var<const uint16_t *, IDXB, SPLIT>(A, ip, llr, slot, vcnt, write, PS::v_sat_rows(p), PS::v_split_rows(p))
#define ACG_BODY                                                       \
    {                                                                  \
        const int md = v_pass(2 * p);                                  \
        const int ioff = v_pass(2 * p + 1);                            \
        const int slot = p * L + l;                                    \
        const T llr = get_llr(lr, p, slot);                            \
        const uint16_t *ip = IDX + ioff + l;                           \
        if (MAXD <= 8 || md <= 8) {                                    \
            ACG_PASS_SWITCH(md, ACG_CALL)                              \
        } else {                                                       \
            var_generic(ip, llr, slot, md, write);                     \
        }                                                              \
    }
        ACG_PASS_LOOP(STATIC, p, n_vpass(), ACG_BODY)
#undef ACG_BODY
#undef ACG_CALL
    }

    // var_phase that also returns the posterior hard decisions of this lane's variables (bit p = pass p); for the
    // workgroup-per-frame kernel, whose output path reads them from registers (see check_phase_syndrome)
    __device__ __forceinline__ uint32_t var_phase_hard(const LlrRegs &lr, bool write) {
        uint32_t hard = 0;
        for (int p = 0; p < t.n_vpass; ++p) {
            const int md = sload(t.v_pass, 2 * p);
            const int ioff = sload(t.v_pass, 2 * p + 1);
            const int slot = p * L + l;
            const T llr = get_llr(lr, p, slot);
            const uint16_t *ip = IDX + ioff + l;
            if (md == 0) {
                hard |= ((llr <= (T) 0) ? 1u : 0u) << p;  // isolated variables: estimate() == channel LLR
            } else if (MAXD <= 8 || md <= 8) {
#define ACG_CALL(D) hard |= (uint32_t) BpPass<T, D, L, ALGO>::template var<const uint16_t *, IDXB>(A, ip, llr, slot, vcnt, write) << p
                ACG_PASS_SWITCH(md, ACG_CALL)
#undef ACG_CALL
            }
        }
        return hard;
    }

    // Variable sweep with the index table in registers: ir[2p + j] packs the positions of edges 2j and 2j + 1 of the
    // variable in (pass p, this lane) (padding -> zero_pos).  For codes of variable degree <= 4 whose table does not
    // fit in LDS next to the messages (the 5000 x 10000 (3,6) code): takes the dependent global index load out of every
    // pass of every sweep.
    static constexpr int IDXREG_MAXD = 4;
    using IdxRegs = uint32_t[NVP > 0 ? 2 * NVP : 1];
    __device__ __forceinline__ void load_idx_regs(IdxRegs &ir) const {
#pragma unroll
        for (int p = 0; p < (NVP > 0 ? NVP : 0); ++p) {
            uint32_t w[IDXREG_MAXD];
#pragma unroll
            for (int k = 0; k < IDXREG_MAXD; ++k) w[k] = (uint32_t) t.zero_pos;
            if (p < t.n_vpass) {
                const int md = sload(t.v_pass, 2 * p), ioff = sload(t.v_pass, 2 * p + 1);
#pragma unroll
                for (int k = 0; k < IDXREG_MAXD; ++k)
                    if (k < md) w[k] = t.v_apos[ioff + k * L + l];
            }
            ir[2 * p] = w[0] | (w[1] << 16);
            ir[2 * p + 1] = w[2] | (w[3] << 16);
        }
    }
    // -> bit p = posterior hard decision of the variable in (pass p, this lane)
    template <int D, bool UNI = false>
    __device__ __forceinline__ uint32_t var_pass_regs(const LlrRegs &lr, const IdxRegs &ir, int p, bool write) {
        const uint32_t w0 = ir[2 * p], w1 = ir[2 * p + 1];
        int pos[D];
#pragma unroll
        for (int k = 0; k < D; ++k) pos[k] = (int) (((k < 2 ? w0 : w1) >> (16 * (k & 1))) & 0xFFFFu);
        return (uint32_t) BpPass<T, D, L, ALGO>::template var_at<UNI>(A, pos, get_llr(lr, p, p * L + l), p * L + l, vcnt, write) << p;
    }
    // REG: the instance for regular codes (the host checked: every variable has the same degree <= IDXREG_MAXD) — the other
    // paths are compiled out, not branched around (a third of the kernel text; +8 % on the (3,6) 5000 x 10000 code)
    template <bool REG = false>
    __device__ __forceinline__ uint32_t var_phase_regs(const LlrRegs &lr, const IdxRegs &ir, bool write) {
        uint32_t hard = 0;
        const int md0 = sload(t.v_pass, 0);
        if (REG || (md0 >= 1 && md0 <= IDXREG_MAXD && sload(t.v_cnt_ge, md0) == t.n)) {
            // every VARIABLE has the same degree: one dispatch per sweep, one write predicate per pass, and the pass loop
            // unrolled so that the LLR and index registers are addressed directly (no s_set_gpr_idx pairs: the scalar
            // instructions, not the vector ones, are what this sweep runs out of — 385 against 824 per wavefront before).
            // The unpacked positions must not be hoisted out of the sweep loop (they would double the index registers):
            // the caller makes `ir` opaque once per sweep.
#define ACG_VREG(D)                                                                                  \
    _Pragma("unroll") for (int p = 0; p < (NVP > 0 ? NVP : 1); ++p)                                  \
        if (p < t.n_vpass) hard |= var_pass_regs<D, true>(lr, ir, p, write);
            switch (md0) {
                case 1: ACG_VREG(1) break;
                case 2: ACG_VREG(2) break;
                case 3: ACG_VREG(3) break;
                default: ACG_VREG(4) break;
            }
#undef ACG_VREG
            return hard;
        }
        if constexpr (!REG) {
        if (md0 >= 1 && md0 == sload(t.v_pass, 2 * (t.n_vpass - 1))) {
            // every pass has the same degree (regular code): one dispatch per sweep instead of one per pass
            switch (md0) {
                case 1: for (int p = 0; p < t.n_vpass; ++p) hard |= var_pass_regs<1>(lr, ir, p, write); break;
                case 2: for (int p = 0; p < t.n_vpass; ++p) hard |= var_pass_regs<2>(lr, ir, p, write); break;
                case 3: for (int p = 0; p < t.n_vpass; ++p) hard |= var_pass_regs<3>(lr, ir, p, write); break;
                default: for (int p = 0; p < t.n_vpass; ++p) hard |= var_pass_regs<4>(lr, ir, p, write); break;
            }
            return hard;
        }
        for (int p = 0; p < t.n_vpass; ++p) {
            const int md = sload(t.v_pass, 2 * p);
            const int slot = p * L + l;
            const T llr = get_llr(lr, p, slot);
            const uint32_t w0 = ir[2 * p], w1 = ir[2 * p + 1];
            switch (md) {
                case 1: { const int pos[1] = {(int) (w0 & 0xFFFFu)}; hard |= (uint32_t) BpPass<T, 1, L, ALGO>::var_at(A, pos, llr, slot, vcnt, write) << p; } break;
                case 2: { const int pos[2] = {(int) (w0 & 0xFFFFu), (int) (w0 >> 16)}; hard |= (uint32_t) BpPass<T, 2, L, ALGO>::var_at(A, pos, llr, slot, vcnt, write) << p; } break;
                case 3: { const int pos[3] = {(int) (w0 & 0xFFFFu), (int) (w0 >> 16), (int) (w1 & 0xFFFFu)}; hard |= (uint32_t) BpPass<T, 3, L, ALGO>::var_at(A, pos, llr, slot, vcnt, write) << p; } break;
                case 4: { const int pos[4] = {(int) (w0 & 0xFFFFu), (int) (w0 >> 16), (int) (w1 & 0xFFFFu), (int) (w1 >> 16)}; hard |= (uint32_t) BpPass<T, 4, L, ALGO>::var_at(A, pos, llr, slot, vcnt, write) << p; } break;
                default: hard |= ((llr <= (T) 0) ? 1u : 0u) << p; break;  // isolated variable: estimate() == channel LLR
            }
        }
        }
        return hard;
    }
    // hard decisions before the first sweep (bp.h:184: mailboxes empty, estimate() == channel LLR)
    __device__ __forceinline__ uint32_t llr_hard_mask(const LlrRegs &lr) const {
        uint32_t hard = 0;
        for (int p = 0; p < t.n_vpass; ++p) hard |= ((get_llr(lr, p, p * L + l) <= (T) 0) ? 1u : 0u) << p;
        return hard;
    }
    // pack the frame's hard decisions (register copy, bit per pass) into OB[0..nwords)
    __device__ __forceinline__ void pack_bits_mask(uint32_t hard, const VarIds &vi) {
        for (int w = l; w < t.nwords; w += L) OB[w] = 0u;
        group_sync<L>();
        for (int p = 0; p < t.n_vpass; ++p) {
            const int v = var_id(vi, p);
            if (v >= 0 && ((hard >> p) & 1u)) atomicOr(&OB[v >> 5], 1u << (v & 31));
        }
        group_sync<L>();
    }

    // Check sweep that also yields the syndrome of the hard decisions riding in the incoming words: true if any check
    // of this lane fails.  Used by the workgroup-per-frame kernel, which then needs no separate syndrome pass (and one
    // barrier less per sweep); the hard decisions themselves are kept in registers by var_phase_regs.
    // REG: every check has the same degree <= 8 (checked by the host), see var_phase_regs
    template <bool REG = false>
    __device__ __forceinline__ bool check_phase_syndrome(bool write) {
        U acc = 0;
        const int cd0 = sload(t.c_pass, 0);
        if (REG || (cd0 >= 1 && cd0 <= 8 && sload(t.c_cnt_ge, cd0) == t.m)) {
            // every CHECK has the same degree: one dispatch per sweep, one write predicate per pass
#define ACG_CALL(D)                                                                                            \
    for (int p = 0; p < t.n_cpass; ++p)                                                                        \
        acc |= BpPass<T, D, L, ALGO>::template check<true>(A + p * (D * L) + l, p * L + l, ccnt, write, ms_scale);
            ACG_PASS_SWITCH(cd0, ACG_CALL)
#undef ACG_CALL
            return (acc & ONE) != 0;
        }
        if constexpr (!REG) {
        if (cd0 >= 1 && cd0 <= 8 && cd0 == sload(t.c_pass, 2 * (t.n_cpass - 1))) {
            // every pass has the same degree: one dispatch per sweep, pass p starts at word p * degree * L
#define ACG_CALL(D)                                                                                            \
    for (int p = 0; p < t.n_cpass; ++p) acc |= BpPass<T, D, L, ALGO>::check(A + p * (D * L) + l, p * L + l, ccnt, write, ms_scale)
            ACG_PASS_SWITCH(cd0, ACG_CALL)
#undef ACG_CALL
            return (acc & ONE) != 0;
        }
        for (int p = 0; p < t.n_cpass; ++p) {
            const int md = sload(t.c_pass, 2 * p);
            T *Ap = A + sload(t.c_pass, 2 * p + 1) + l;
            const int slot = p * L + l;
            if (MAXD <= 8 || md <= 8) {
#define ACG_CALL(D) acc |= BpPass<T, D, L, ALGO>::check(Ap, slot, ccnt, write, ms_scale)
                ACG_PASS_SWITCH(md, ACG_CALL)
#undef ACG_CALL
            } else {
                U S = 0;
                for (int j = 0; j < md; ++j) S ^= B::to(Ap[j * L]);
                acc |= S;
                check_generic(Ap, slot, md, write);
            }
        }
        }
        return (acc & ONE) != 0;
    }

    __device__ __forceinline__ void var_init_phase(const LlrRegs &lr, bool write) {
#define ACG_CALL(D) BpPass<T, D, L, ALGO>::template var_init<const uint16_t *, IDXB>(A, ip, llr, slot, vcnt, write)
#define ACG_BODY                                                                                       \
    {                                                                                                  \
        const int md = v_pass(2 * p);                                                                  \
        const int ioff = v_pass(2 * p + 1);                                                            \
        const int slot = p * L + l;                                                                    \
        const T llr = get_llr(lr, p, slot);                                                            \
        const uint16_t *ip = IDX + ioff + l;                                                           \
        if (MAXD <= 8 || md <= 8) {                                                                    \
            ACG_PASS_SWITCH(md, ACG_CALL)                                                              \
        } else {                                                                                       \
            const U hard = (llr <= (T) 0) ? ONE : (U) 0;                                               \
            const T ax = B::from(B::to(llr) & ~SIGN);                                                  \
            const T mg = (ALGO == 0) ? Dom<T>::phi(ax) : ax;                                           \
            const U ob = (B::to(mg) & ~SIGN & ~ONE) | ((llr <= (T) 0) ? (hard | SIGN) : hard);         \
            for (int k = 0; k < md; ++k)                                                               \
                if (write && slot < vcnt[k + 1]) A[ip[k * L]] = B::from(ob);                           \
        }                                                                                              \
    }
        ACG_PASS_LOOP(STATIC, p, n_vpass(), ACG_BODY)
#undef ACG_BODY
#undef ACG_CALL
    }

    // ---- degree > 8: rolled loops (rare: high-rate codes); same arithmetic -------------------
    __device__ __noinline__ U check_generic(T *__restrict__ Ap, int slot, int md, bool write) {
        T x[MAXD], pre[MAXD];
        U S = 0;
        T s = 0;
        for (int j = 0; j < md; ++j) {
            x[j] = Ap[j * L];
            S ^= B::to(x[j]);
            pre[j] = s;
            s += B::from(B::to(x[j]) & ~SIGN & ~ONE);
        }
        if (ALGO == 0) {
            T suf = 0;
            for (int j = md - 1; j >= 0; --j) {
                const T ph = Dom<T>::phi(pre[j] + suf);
                suf += B::from(B::to(x[j]) & ~SIGN & ~ONE);
                const U ob = (B::to(ph) & ~SIGN) | ((S ^ B::to(x[j])) & SIGN);
                if (write && slot < ccnt[j + 1]) Ap[j * L] = B::from(ob);
            }
        } else {
            T m1 = (T) INFINITY, m2 = (T) INFINITY;  // as in BpPass::check: median / minimum, the minimum found again by value
            for (int j = 0; j < md; ++j) {
                const T a0 = B::from(B::to(x[j]) & ~SIGN & ~ONE);
                const T a = (slot < ccnt[j + 1]) ? a0 : (T) INFINITY;
                if constexpr (sizeof(T) == 4) m2 = __builtin_amdgcn_fmed3f(a, m1, m2);
                else m2 = __builtin_fmin(m2, __builtin_fmax(a, m1));
                m1 = (sizeof(T) == 4) ? (T) __builtin_fminf((float) m1, (float) a) : (T) __builtin_fmin((double) m1, (double) a);
            }
            for (int j = 0; j < md; ++j) {
                const T a0 = B::from(B::to(x[j]) & ~SIGN & ~ONE);
                const T mg = ms_scale * ((a0 == m1 && slot < ccnt[j + 1]) ? m2 : m1);
                const U ob = (B::to(mg) & ~SIGN) | ((S ^ B::to(x[j])) & SIGN);
                if (write && slot < ccnt[j + 1]) Ap[j * L] = B::from(ob);
            }
        }
        return S;
    }

    __device__ __noinline__ void var_generic(const uint16_t *ip, T llr, int slot, int md, bool write) {
        int pos[MAXD];
        T c[MAXD], pre[MAXD];
        T s = 0;
        for (int k = 0; k < md; ++k) {
            pos[k] = IDXB ? (int) (ip[k * L] / sizeof(T)) : (int) ip[k * L];
            c[k] = A[pos[k]];
            pre[k] = s;
            s += c[k];
        }
        const T total = llr + s;
        const U hard = (total <= (T) 0) ? ONE : (U) 0;
        T suf = 0;
        for (int k = md - 1; k >= 0; --k) {
            const T xk = llr + (pre[k] + suf);
            suf += c[k];
            const T ax = B::from(B::to(xk) & ~SIGN);
            const T mg = (ALGO == 0) ? Dom<T>::phi(ax) : ax;
            const U ob = (B::to(mg) & ~SIGN & ~ONE) | hard | ((xk <= (T) 0) ? SIGN : (U) 0);
            if (write && slot < vcnt[k + 1]) A[pos[k]] = B::from(ob);
        }
    }

    // hard decision of the variable in (pass p, this lane) as stored by the last var_phase
    __device__ __forceinline__ uint32_t hard_bit(const LlrRegs &lr, int p) const {
        const int slot = p * L + l;
        if (slot < vcnt[1]) {
            const int pos0 = IDX[v_pass(2 * p + 1) + l];
            return (uint32_t) (B::to(BpPass<T, 1, L, ALGO>::template at<IDXB>(A, pos0)) & ONE);
        }
        return (get_llr(lr, p, slot) <= (T) 0) ? 1u : 0u;  // isolated variable: estimate() == channel LLR
    }

    // pack the frame's hard decisions into OB[0..nwords)
    template <bool REGS = true>
    __device__ __forceinline__ void pack_bits(const LlrRegs &lr, const VarIds &vi, const AbsWord &aw) {
        for (int w = l; w < t.nwords; w += L) OB[w] = 0u;
        group_sync<L>();
#define ACG_BODY                                                                   \
    {                                                                              \
        const int v = var_id<REGS>(vi, p);                                         \
        if (v >= 0 && hard_bit(lr, p)) atomicOr(&OB[v >> 5], 1u << (v & 31));      \
    }
        ACG_PASS_LOOP(STATIC, p, n_vpass(), ACG_BODY)
#undef ACG_BODY
#pragma unroll
        for (int q = 0; q < NAP; ++q) {
            if (q < n_apass()) {
                const int v = abs_var(q);
                if (v >= 0 && (aw[q] & ONE)) atomicOr(&OB[v >> 5], 1u << (v & 31));
            }
        }
        group_sync<L>();
    }
    __device__ __forceinline__ void pack_bits(const LlrRegs &lr, const VarIds &vi) {
        AbsWord aw = {};
        pack_bits(lr, vi, aw);
    }
};

// group-wide OR of a per-lane predicate (groups are L consecutive lanes of the wavefront)
template <int L>
__device__ __forceinline__ bool group_any(bool pred, int g) {
    const unsigned long long b = __ballot(pred);
    if (L == 64) return b != 0ull;
    const unsigned long long mask = ((1ull << (L & 63)) - 1ull) << (g * L);
    return (b & mask) != 0ull;
}

template <int L>
__device__ __forceinline__ int group_sum(int v, int l) {
#pragma unroll
    for (int o = L / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ------------------------------------------------------------------------------------------
// Register budget: LDS admits 7-8 frames' waves per SIMD for the small codes, so the degree<=8 fp32 kernels are
// held to 64 VGPRs (8 waves/SIMD; they need 58-60 and do not spill); wider arrays get proportionally more.
template <typename T, int MAXD, int L, int NVP>
constexpr int bp_min_waves() {
    // with the LLRs in registers (NVP > 0) LDS admits 8 (L=64) / 5 (L=32) workgroups per CU for H05-sized codes
    return (NVP > 0 ? (L == 64 ? 6 : (L == 32 ? 5 : 3)) : (MAXD <= 8 ? 8 : (MAXD <= 16 ? 4 : 2))) / (sizeof(T) == 8 ? 2 : 1);
}

// DBG (tests only, acg_ldpc_debug_bp_trace): the raw message words of a frame are copied out of LDS after the check
// sweep and after the variable sweep of its LAST iteration (a.dbg_c2v / a.dbg_v2c: [frame][a_words]) together with the
// channel LLRs in slot order (a.dbg_post: [frame][n_vpass * L]); the product instances are compiled with DBG = false.
// SAT: the phi fast path of the sweeps (BpCore::SATSKIP; fixed-work decoders), see sat::bp_fused_kernel
// PS: the pass structure policy (PassRuntime: any code; a static policy: the instances of bp_inst_spec.hip)
// SPLIT: the sweeps of a wavefront whose groups have all latched evaluate one series of phi where that gives phi's bits
// (BpPass::word_c / word_v); instances of their own (split::), which a handle takes unless ACG_BP_NO_PHISPLIT=1 is set
template <typename T, int MAXD, int L, int ALGO, bool MC, bool IDXLDS, int NVP, bool DBG, bool SAT, typename PS = PassRuntime, bool SPLIT = false>
__device__ __forceinline__ void bp_fused_body(const BpTables &t, const DecodeArgs &a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    using Core = BpCore<T, MAXD, L, ALGO, IDXLDS, NVP, IDXLDS && ACG_IDX_BYTES, SAT, PS>;  // the LDS copy of the index table is in byte offsets
    constexpr int FPW = 64 / L;  // frames in flight per wavefront
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int l = lane % L;
    const int g = lane / L;
    const int grp_in_block = wave * FPW + g;
    // block-shared copy of the variable-side index table (read every iteration by every wave)
    const uint16_t *IDX = t.v_apos;
    if (IDXLDS) {
        uint16_t *idx_lds = reinterpret_cast<uint16_t *>(smem);
        for (int i = threadIdx.x; i < t.v_apos_len; i += blockDim.x) idx_lds[i] = (uint16_t) (t.v_apos[i] * (ACG_IDX_BYTES ? sizeof(T) : 1));  // (the host checked that it fits)
        __syncthreads();
        IDX = idx_lds;
    }
    unsigned char *base = smem + t.idx_lds_bytes + (size_t) grp_in_block * t.lds_bytes_per_frame;
    T *A = reinterpret_cast<T *>(base);
    T *LLR = A + t.a_words;
    uint32_t *OB = reinterpret_cast<uint32_t *>(LLR + t.llr_words);
    Core core(t, A, LLR, OB, IDX, l, a.ms_scale);
    // the instances with the freeze path (see `fz` below) and what they pay for its registers: the variable ids are read from the
    // table when a frame starts and when it is written out, not held for the whole kernel
    constexpr bool FREEZE = Core::SATSKIP && NVP > 0 && !DBG;  // (NVP > 0: the instances the host takes for fixed-work decoders)
    // (ACG_SPEC_VIREG: the static-policy instances, whose sweeps need fewer registers, hold them again — see DESIGN §3)
    constexpr bool VIREG = !FREEZE || (PS::STATIC && ACG_SPEC_VIREG);
    // the one-series phi: the instances with the freeze path, and their debug twin (DBG: `latched` in the place of `fz`)
    constexpr bool PHISPLIT = SPLIT && Core::SATSKIP && NVP > 0;
    typename Core::LlrRegs lr;
    typename Core::VarIds vi;
#pragma unroll
    for (int p = 0; p < (NVP > 0 ? NVP : 1); ++p) {
        lr[p] = (T) 0;
        vi[p] = (VIREG && NVP > 0 && p < core.n_vpass()) ? t.v_var[p * L + l] : -1;
    }
    // absorbed degree-1 variables (BpPass::check_abs): LLR, v->c word, c->v word (debug trace only) per absorbed pass
    // and, in the SATSKIP instances, the phi memo of its check's other edges (Core::abs_phi; memo off: am = 0, ag = +inf)
    typename Core::AbsLlr al, ar, ag;
    typename Core::AbsWord aw;
    const typename Core::U am = (Core::SATSKIP && a.phi_memo) ? Core::MEMO_MASK : 0;
#pragma unroll
    for (int q = 0; q < (Core::NAP > 0 ? Core::NAP : 1); ++q) {
        al[q] = (T) 0;
        ar[q] = (T) 0;
        ag[q] = (T) INFINITY;
        aw[q] = 0;
    }

    // Frames are handed out dynamically: a wavefront draws chunks of CHUNK consecutive frame indices from one
    // global counter (one atomic per CHUNK frames) and deals them to its groups as they become free.  With early
    // exit the work per frame varies by 50x (1..max_iter sweeps); a static stripe of ~100 frames per group left
    // the slowest group ~40% behind the mean at the end of a 1M-frame launch.
    constexpr int CHUNK = 4 * FPW;
    int64_t wnext = 0, wend = 0;  // wave-uniform: the unassigned part of the current chunk
    int64_t frame = 0;
    bool active = false;
    bool want = true;             // this group needs a frame
    bool need_init = false;
    bool latched = false;
    int it = 0;
    // FREEZE (fixed-work SAT instances, a.freeze_ws set): a latched frame stops sweeping once its state recurs.  A flooding sweep
    // is a function of (A, aw) and of per-frame constants (LLRs, ag); a latched frame writes no output any more.  So when the
    // words after sweep k equal, bit for bit, those after sweep k - p, every later state is one already seen and the remaining
    // sweeps can change nothing the caller gets: the frame retires as if it had run them (it = max_iter).  The words of p
    // sweeps ago are kept in the group's slot of a.freeze_ws; a lane reads back only the words it wrote itself.
    // fz = 0 until the frame latches (it takes the place of `latched` in these instances), then
    //      sweeps until the next detection << 2 | the slot holds a snapshot taken since the latch << 1 | 1.
    int fz = 0;
    // the gate in front of the compare: the sum of this lane's words at the snapshot in the slot (valid while fz & 2)
    typename Core::U fc = 0;
    int ham = 0;  // raw-channel errors of the current frame (MC)
    // per-group MC accumulators (flushed once at the end)
    unsigned int acc_correct = 0, acc_pseudo = 0, acc_total = 0;
    unsigned long long acc_ham = 0, acc_ham_ok = 0, acc_ham_wrong = 0, acc_iters = 0;

    // padding words and the zero cell are +0.0 for the whole launch: no sweep ever writes them
    for (int w = l; w < t.a_words; w += L) A[w] = (T) 0;
    wave_sync();

    // MERGED: the check sweep reads every v->c word anyway, so it also delivers the syndrome of the hard decisions that ride in
    // them (BpPass::check returns the XOR) — no separate syndrome pass per sweep (about 5 % of the instructions of a sweep);
    // the hard decisions of a lane's variables are kept in a register (bit per pass) by the variable sweep, because the
    // check sweep has overwritten the words they rode in by the time a frame is found converged.  A sweep is then
    // [check sweep + syndrome] -> decide / output -> hand out and initialise new frames (whose first variable sweep
    // this is: var_init) -> variable sweep of the frames that continue.  A frame costs one check sweep more than it has
    // iterations (the one that finds it converged, or its last) and no syndrome passes.
    // Min-sum instances only: there the extra check sweep is cheap (+8 % fixed-50, +4.6 % with early exit on H05); a sum-product
    // check sweep is half an iteration of phi evaluations, which the early-exit runs (12 sweeps per frame at -2 dB) lose more
    // by than the syndrome passes cost (measured: +1.1 % fixed-50, -3.4 % with early exit).
    constexpr bool MERGED = ACG_FUSED_MERGED && ALGO == 1 && MAXD <= 8 && NVP > 0;  // (NVP > 0: at most 12 variable passes, the bit mask holds them)
    uint32_t hard = 0;  // MERGED: posterior hard decisions of my variables, bit p = pass p
    auto is_latched = [&]() -> bool {
        if constexpr (FREEZE) return fz != 0;
        else return latched;
    };
    auto emit = [&](const bool out_now, const bool fail_now) {
        if (__ballot(out_now || fail_now) != 0ull) {
            if (out_now) {
                if (MERGED) core.pack_bits_mask(hard, vi);
                else core.template pack_bits<VIREG>(lr, vi, aw);
            }
            else if (fail_now) {
                for (int w = l; w < t.nwords; w += L) OB[w] = 0u;  // reference returns an empty vector, bp.h:198
                wave_sync();
            }
            if (out_now || fail_now) {
                if (a.out_bits)
                    for (int w = l; w < t.nwords; w += L) a.out_bits[(size_t) frame * t.nwords + w] = OB[w];
                if (l == 0) {
                    if (a.out_ok) a.out_ok[frame] = out_now ? 1 : 0;
                    if (a.out_iters) a.out_iters[frame] = it < a.max_iter ? it : a.max_iter;
                }
                if (MC) {
                    bool neq = false;
                    const int64_t gf = a.first_frame + frame;
                    for (int w = l; w < t.nwords; w += L) {
                        const uint32_t cwv = a.cw_packed ? a.cw_packed[(size_t) (gf % a.n_cw) * t.nwords + w] : 0u;
                        neq |= (OB[w] != cwv);
                    }
                    // every lane of a group is in this branch together: the ballot is complete per group
                    const bool differ = group_any<L>(neq, g);
                    const bool correct = out_now && !differ;  // experiment.h:110-114
                    acc_correct += correct;
                    acc_pseudo += (out_now && differ);          // experiment.h:115-116
                    acc_total += 1;
                    acc_ham += ham;
                    acc_ham_ok += correct ? ham : 0;
                    acc_ham_wrong += correct ? 0 : ham;
                    acc_iters += it < a.max_iter ? it : a.max_iter;
                }
                if constexpr (FREEZE) fz = (int) ((a.freeze_cfg & 0xFFFu) << 2) | 1;
                else latched = true;
            }
        }
    };
    auto deal_frames = [&]() {
        // deal new frames to the groups that want one (wave-uniform loop over at most FPW leaders)
        unsigned long long wm = __ballot(want && l == 0);
        while (wm != 0ull) {
            const int leader = __builtin_ctzll(wm);
            wm &= wm - 1ull;
            if (wnext >= wend) {
                unsigned long long base = 0;
                if (lane == 0) base = atomicAdd(a.work_counter, (unsigned long long) CHUNK);
                const uint32_t blo = __builtin_amdgcn_readfirstlane((uint32_t) base);
                const uint32_t bhi = __builtin_amdgcn_readfirstlane((uint32_t) (base >> 32));
                wnext = (int64_t) (((unsigned long long) bhi << 32) | blo);
                wend = wnext + CHUNK < a.frames ? wnext + CHUNK : a.frames;
            }
            const bool got = wnext < wend;
            const int64_t f = wnext;
            if (got) wnext += 1;
            if (lane / L == leader / L) {
                frame = f;
                active = got;
                need_init = got;
                want = false;
            }
        }
    };
    auto init_frames = [&]() {
        // ---- (re)start groups on a new frame -------------------------------------------------
        if (__ballot(need_init) != 0ull) {
            wave_sync();
            const uint32_t *cw = nullptr;
            if (MC && need_init) {
                const int64_t gf = a.first_frame + frame;
                if (a.cw_packed) cw = a.cw_packed + (size_t) (gf % a.n_cw) * t.nwords;
                // stage the frame's noisy symbols in natural order in A[0..n)
                const int nq = (t.n + 3) >> 2;
                for (int q = l; q < nq; q += L) {
                    uint32_t r[4];
                    philox4x32_10((uint32_t) gf, (uint32_t) (gf >> 32), (uint32_t) q, 0u, (uint32_t) a.seed,
                                  (uint32_t) (a.seed >> 32), r);
                    float z[4];
                    box_muller(r[0], r[1], z[0], z[1]);
                    box_muller(r[2], r[3], z[2], z[3]);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int v = 4 * q + e;
                        if (v < t.n) {
                            const uint32_t bit = cw ? ((cw[v >> 5] >> (v & 31)) & 1u) : 0u;
                            A[v] = (T) __builtin_fmaf(a.sigma, z[e], bit ? -1.0f : 1.0f);  // channel.h:24 (explicit fma: same symbol in every kernel)
                        }
                    }
                }
            }
            wave_sync();
            int my_ham = 0;
            if (need_init) {
                // channel LLRs (channel.h:14-16) into slot order
                auto chan_llr = [&](const int v) -> T {
                    T llr = (T) 0;
                    if (v >= 0) {
                        if (MC) {
                            const T yv = A[v];
                            const uint32_t bit = cw ? ((cw[v >> 5] >> (v & 31)) & 1u) : 0u;
                            // HammingDistanceTracker (experiment.h:33-46)
                            my_ham += ((!bit && yv <= (T) 0) || (bit && yv > (T) 0)) ? 1 : 0;
                            llr = (T) ((double) yv * (a.inv_var2 * Dom<T>::scale));
                        } else if (a.y_is_f64) {
                            // llr = 2*y/sigma^2 exactly as channel.h:14-16 (double divide; only on the fp64-input path)
                            const double yv = reinterpret_cast<const double *>(a.y)[(size_t) frame * t.n + v];
                            llr = (T) (2 * yv / a.var * Dom<T>::scale);
                        } else {
                            // fp32 symbols: one double multiply by 2/sigma^2 (the quotient differs from the exact
                            // one by < 1 ulp of a double before it is rounded to T)
                            const float yv = reinterpret_cast<const float *>(a.y)[(size_t) frame * t.n + v];
                            llr = (T) ((double) yv * (a.inv_var2 * Dom<T>::scale));
                        }
                    }
                    return llr;
                };
#define ACG_BODY core.set_llr(lr, p, p * L + l, chan_llr(core.template var_id<VIREG>(vi, p)));
                ACG_PASS_LOOP(Core::STATIC, p, core.n_vpass(), ACG_BODY)
#undef ACG_BODY
                // absorbed variables: LLR and the constant v->c word (+0 for a lane without one)
#pragma unroll
                for (int q = 0; q < Core::NAP; ++q) {
                    if (q < core.n_apass()) {
                        const int v = core.abs_var(q);
                        al[q] = chan_llr(v);
                        aw[q] = v >= 0 ? Core::abs_word(al[q]) : 0;
                        if constexpr (Core::SATSKIP) ag[q] = Core::abs_phi(aw[q], am);
                    }
                }
            }
            wave_sync();  // all reads of the staged symbols are done before A is cleared
            if (MC) {
                const int hs = group_sum<L>(need_init ? my_ham : 0, l);
                if (need_init) ham = hs;
            }
            if (MC && need_init)
                for (int w = l; w < ((t.n + 3) & ~3); w += L) A[w] = (T) 0;  // staged symbols may sit on padding words
            wave_sync();
            core.var_init_phase(lr, need_init);  // initial c_receive_messages() on empty mailboxes, bp.h:184,40-43,70-73
            wave_sync();
            if (MERGED && need_init) hard = core.llr_hard_mask(lr);  // bp.h:184: mailboxes empty, estimate() == channel LLR
            if (need_init) {
                it = 0;
                latched = false;
                if constexpr (FREEZE) fz = 0;
                need_init = false;
            }
            // a fresh frame with max_iter == 0 must fail without iterating; handled by the next round's test
        }

    };

    if (MERGED) {
        for (;;) {
            // ---- check sweep (bp.h:186) + syndrome of the estimate the previous variable sweep produced -------------------
            // (a group without a frame, or fresh from var_init with it == 0, ignores the result)
            const bool bad = group_any<L>((core.check_phase(active) & Core::ONE) != 0, g);
            wave_sync();
            if (DBG && active && it == a.max_iter - 1 && a.dbg_c2v)
                for (int w = l; w < t.a_words; w += L) reinterpret_cast<T *>(a.dbg_c2v)[(size_t) frame * t.a_words + w] = A[w];
            const bool conv = active && it > 0 && it <= a.max_iter && !bad;     // bp.h:195 (max_iter = 0: never)
            const bool out_now = conv && !latched;
            const bool finish = active && ((a.early_exit && conv) || it >= a.max_iter);
            const bool fail_now = finish && !conv && !latched;
            emit(out_now, fail_now);
            if (finish) {
                active = false;
                want = true;
            }
            deal_frames();
            if (__ballot(active) == 0ull) break;
            const bool fresh = need_init;  // its var_init IS its variable sweep of this trip
            init_frames();
            // ---- variable sweep (bp.h:187-188) of the frames that continue ------------------------------------------
            const bool cont = active && !fresh;
            const uint32_t hv = core.var_phase_hard(lr, cont);
            hard = cont ? hv : hard;
            wave_sync();
            if (DBG && cont && it == a.max_iter - 1 && a.dbg_v2c) {
                for (int w = l; w < t.a_words; w += L) reinterpret_cast<T *>(a.dbg_v2c)[(size_t) frame * t.a_words + w] = A[w];
                for (int p = 0; p < t.n_vpass; ++p)
                    reinterpret_cast<T *>(a.dbg_post)[(size_t) frame * (t.n_vpass * L) + p * L + l] = core.get_llr(lr, p, p * L + l);
            }
            it += cont ? 1 : 0;
        }
    } else
    for (;;) {
        // ---- syndrome of the estimate produced by the previous variable phase -----------------
        // (a group that has not been initialised yet has it == 0 and ignores the result)
        // fixed work: once every group of the wave has latched its output (or is idle) the syndrome feeds nothing
        const bool pend = active && !is_latched() && it > 0;
        const bool bad = __ballot(pend) != 0ull ? group_any<L>(core.syndrome_bad(aw), g) : true;
        const bool conv = active && it > 0 && it <= a.max_iter && !bad;     // bp.h:195 (max_iter = 0: never)
        const bool out_now = conv && !is_latched();
        const bool finish = active && ((a.early_exit && conv) || it >= a.max_iter);
        const bool fail_now = finish && !conv && !is_latched();
        emit(out_now, fail_now);
        if (finish) {
            active = false;
            want = true;
        }
        deal_frames();
        if (__ballot(active) == 0ull) break;
        init_frames();
        // ---- one flooding iteration (bp.h:186-188) -------------------------------------------
        // PHISPLIT: each sweep exists twice, and the one with the one-series phi runs while every group of the wavefront that has
        // a frame has latched: before its latch a frame has next to no unit on one side of a threshold (0.6 % on the check side,
        // 20 % on the variable side against 65 % and 92 % behind it, tools/phi_census.cpp --split), and a wavefront decides as a whole.
        // One scalar branch per sweep, no predicate per row.
        bool split_now = false;
        if constexpr (PHISPLIT) split_now = __ballot(active && !is_latched()) == 0ull;
        if constexpr (PHISPLIT) {
            if (split_now) core.template check_phase<true>(active, aw, al, ar, ag, am);
            else core.check_phase(active, aw, al, ar, ag, am);
        } else
        core.check_phase(active, aw, al, ar, ag, am);
        wave_sync();
        // debug dumps: per frame the message array, then the absorbed edges' words (absorbed pass q, lane l at a_words + q*L + l);
        // LLRs in slot order, then the absorbed variables' (n_vpass*L + q*L + l)
        const int dbg_cw = t.a_words + core.n_apass() * L, dbg_pw = (t.n_vpass + core.n_apass()) * L;
        if (DBG && active && it == a.max_iter - 1 && a.dbg_c2v) {
            for (int w = l; w < t.a_words; w += L) reinterpret_cast<T *>(a.dbg_c2v)[(size_t) frame * dbg_cw + w] = A[w];
            for (int q = 0; q < Core::NAP; ++q)
                if (q < core.n_apass()) reinterpret_cast<T *>(a.dbg_c2v)[(size_t) frame * dbg_cw + t.a_words + q * L + l] = ar[q];
        }
        if constexpr (PHISPLIT) {
            if (split_now) core.template var_phase<true>(lr, active);
            else core.var_phase(lr, active);
        } else
        core.var_phase(lr, active);
        wave_sync();
        if (DBG && active && it == a.max_iter - 1 && a.dbg_v2c) {
            for (int w = l; w < t.a_words; w += L) reinterpret_cast<T *>(a.dbg_v2c)[(size_t) frame * dbg_cw + w] = A[w];
            for (int p = 0; p < t.n_vpass; ++p)
                reinterpret_cast<T *>(a.dbg_post)[(size_t) frame * dbg_pw + p * L + l] = core.get_llr(lr, p, p * L + l);
            for (int q = 0; q < Core::NAP; ++q)
                if (q < core.n_apass()) {
                    reinterpret_cast<T *>(a.dbg_v2c)[(size_t) frame * dbg_cw + t.a_words + q * L + l] = FpBits<T>::from(aw[q]);
                    reinterpret_cast<T *>(a.dbg_post)[(size_t) frame * dbg_pw + (t.n_vpass + q) * L + l] = al[q];
                }
        }
        if constexpr (FREEZE) {
            if (a.freeze_ws) {
                const bool cand = active && fz != 0;
                fz -= cand ? 4 : 0;
                const bool due = cand && fz < 4 && it + 1 < a.max_iter;  // (nothing left to save behind the last sweep)
                if (__ballot(due) != 0ull) {
                    // moved: a word differs from the snapshot, or the group did not compare (or is not due)
                    typename Core::U moved = 1;
                    if (due) {
                        // the slot's address is formed here, from values the compiler cannot trace back to the loop-invariant
                        // thread and block ids: hoisted out of the sweep loop it would hold registers the sweeps need
                        uint32_t tid = threadIdx.x, bid = blockIdx.x;
                        asm volatile("" : "+v"(tid), "+s"(bid));
                        const uint32_t slot = bid * (blockDim.x / L) + tid / L;  // (the host keeps the workspace below 2^31 words)
                        uint32_t *snap = a.freeze_ws + FREEZE_WS_HEAD + (size_t) (slot * (uint32_t) (t.a_words + Core::NAP * L));
                        const int lo = (int) (tid % L);  // (= l, as opaque as the address; no trip-count set-up to hoist)
                        // A pass costs what it issues, not what it moves (profiles/r12_freeze_gate_summary.md), so every pass goes
                        // over the state four words at a time: a lane owns the quads lo, lo + L, ... of the message array (a_words
                        // is a multiple of 4, frames and slots start on 16 bytes) and its own absorbed words.
                        static_assert(sizeof(T) == 4 && sizeof(typename Core::U) == 4, "the freeze passes read the message array as uint4");
                        const uint4 *A4 = reinterpret_cast<const uint4 *>(A);
                        uint4 *snap4 = reinterpret_cast<uint4 *>(snap);
                        const int nq = t.a_words >> 2;
                        // the gate: the sum of the words this lane would compare, read from LDS alone.  Equal states have equal
                        // sums, so a lane whose sum differs from the one it took at the previous snapshot proves that the state
                        // moved, and the group then only writes the new snapshot: no load, no wait for one.
                        typename Core::U cs = 0;
                        if (!(a.freeze_cfg & FREEZE_CFG_NO_GATE)) {
#pragma unroll 1
                            for (int q = lo; q < nq; q += 2 * L) {
#pragma unroll
                                for (int k = 0; k < 2; ++k) {
                                    if (q + k * L < nq) {
                                        const uint4 c = A4[q + k * L];
                                        cs += (c.x + c.y) + (c.z + c.w);
                                    }
                                }
                            }
#pragma unroll
                            for (int q = 0; q < Core::NAP; ++q)
                                if (q < core.n_apass()) cs += aw[q];
                        }
                        // (the first detection behind a latch has nothing to compare with: it only writes)
                        const bool differs = !(fz & 2) || cs != fc;
                        fc = cs;
                        const bool cmp = !group_any<L>(differs, g);
                        if (cmp) {
                            moved = 0;
#pragma unroll 1
                            for (int q = lo; q < nq; q += 2 * L) {
                                uint4 cur[2], old[2];
#pragma unroll
                                for (int k = 0; k < 2; ++k) old[k] = q + k * L < nq ? snap4[q + k * L] : uint4{0, 0, 0, 0};  // two loads in flight
#pragma unroll
                                for (int k = 0; k < 2; ++k) cur[k] = q + k * L < nq ? A4[q + k * L] : uint4{0, 0, 0, 0};
#pragma unroll
                                for (int k = 0; k < 2; ++k) {
                                    moved |= ((cur[k].x ^ old[k].x) | (cur[k].y ^ old[k].y)) | ((cur[k].z ^ old[k].z) | (cur[k].w ^ old[k].w));
                                    if (q + k * L < nq) snap4[q + k * L] = cur[k];
                                }
                            }
#pragma unroll
                            for (int q = 0; q < Core::NAP; ++q) {
                                if (q < core.n_apass()) {
                                    moved |= aw[q] ^ snap[t.a_words + q * L + lo];
                                    snap[t.a_words + q * L + lo] = aw[q];
                                }
                            }
                        } else {
#pragma unroll 1
                            for (int q = lo; q < nq; q += 2 * L) {
#pragma unroll
                                for (int k = 0; k < 2; ++k)
                                    if (q + k * L < nq) snap4[q + k * L] = A4[q + k * L];
                            }
#pragma unroll
                            for (int q = 0; q < Core::NAP; ++q)
                                if (q < core.n_apass()) snap[t.a_words + q * L + lo] = aw[q];
                        }
                        if ((int32_t) a.freeze_cfg < 0 && lo == 0)
                            atomicAdd(reinterpret_cast<unsigned long long *>(a.freeze_ws) + (cmp ? FREEZE_WS_COMPARES : FREEZE_WS_STORES), 1ull);
                        fz = (int) (((a.freeze_cfg >> 12) & 0xFFFu) << 2) | 3;
                    }
                    if (!group_any<L>(moved != 0, g)) {
                        if ((int32_t) a.freeze_cfg < 0 && l == 0)
                            atomicAdd(reinterpret_cast<unsigned long long *>(a.freeze_ws),
                                      (1ull << FREEZE_STATS_SHIFT) + (unsigned long long) (a.max_iter - (it + 1)));
                        it = a.max_iter - 1;  // retires at the head of the loop: finish, already latched
                    }
                }
            }
        }
        it += 1;
    }

    if (MC && l == 0 && acc_total) {
        atomicAdd(&a.counters[MC_CORRECT], (unsigned long long) acc_correct);
        atomicAdd(&a.counters[MC_PSEUDO], (unsigned long long) acc_pseudo);
        atomicAdd(&a.counters[MC_TOTAL], (unsigned long long) acc_total);
        atomicAdd(&a.counters[MC_HAM], acc_ham);
        atomicAdd(&a.counters[MC_HAM_OK], acc_ham_ok);
        atomicAdd(&a.counters[MC_HAM_WRONG], acc_ham_wrong);
        atomicAdd(&a.counters[MC_ITERS], acc_iters);
    }
}

template <typename T, int MAXD, int L, int ALGO, bool MC, bool IDXLDS, int NVP, bool DBG = false>
__global__ void __launch_bounds__(256, (bp_min_waves<T, MAXD, L, NVP>())) bp_fused_kernel(const BpTables t, const DecodeArgs a) {
    bp_fused_body<T, MAXD, L, ALGO, MC, IDXLDS, NVP, DBG, false>(t, a);
}

// the same kernel with the phi fast path (BpCore::SATSKIP), for fixed-work decoders.  Same name and template arguments in a
// namespace of its own: profiles and tools that look a kernel up by "bp_fused_kernel<...>" find either instance.
namespace sat {
template <typename T, int MAXD, int L, int ALGO, bool MC, bool IDXLDS, int NVP, bool DBG = false>
__global__ void __launch_bounds__(256, (bp_min_waves<T, MAXD, L, NVP>())) bp_fused_kernel(const BpTables t, const DecodeArgs a) {
    bp_fused_body<T, MAXD, L, ALGO, MC, IDXLDS, NVP, DBG, true>(t, a);
}
}  // namespace sat

// the fixed-work instances with the one-series phi as well (bp_fused_body, SPLIT): same name and template arguments again
namespace split {
template <typename T, int MAXD, int L, int ALGO, bool MC, bool IDXLDS, int NVP, bool DBG = false>
__global__ void __launch_bounds__(256, (bp_min_waves<T, MAXD, L, NVP>())) bp_fused_kernel(const BpTables t, const DecodeArgs a) {
    bp_fused_body<T, MAXD, L, ALGO, MC, IDXLDS, NVP, DBG, true, PassRuntime, true>(t, a);
}
}  // namespace split
