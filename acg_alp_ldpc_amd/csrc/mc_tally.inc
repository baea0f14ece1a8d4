// The seven sums of acg_ldpc_mc_result as one wavefront keeps them (wave-uniform) until it adds them to a counters row: ONE
// definition for the classifiers of mc_kernels.hip and mc_rm_kernels.hip.  Included inside namespace acg, device code only.
struct Tally {
    unsigned long long ok = 0, ps = 0, tot = 0, h = 0, hok = 0, hw = 0, it = 0;
    __device__ void add(bool correct, bool pseudo, int ham, int iters) {
        ok += correct;
        ps += pseudo;
        tot += 1;
        h += ham;
        hok += correct ? ham : 0;
        hw += correct ? 0 : ham;
        it += iters;
    }
    // lane 0 adds the sums to row[MC_NCOUNTERS] (nothing when no frame was added); the sums start again from zero
    __device__ void flush(unsigned long long *row) {
        if ((threadIdx.x & 63) == 0 && tot) {
            atomicAdd(&row[MC_CORRECT], ok);
            atomicAdd(&row[MC_PSEUDO], ps);
            atomicAdd(&row[MC_TOTAL], tot);
            atomicAdd(&row[MC_HAM], h);
            atomicAdd(&row[MC_HAM_OK], hok);
            atomicAdd(&row[MC_HAM_WRONG], hw);
            atomicAdd(&row[MC_ITERS], it);
        }
        *this = Tally();
    }
};
