// The glue of a two-stage decode (acg_ldpc_cascade_*, cascade.hip): the hand-over of the frames the first decoder fails to
// the second one stays on the device.  Three kernels per chunk of at most 65536 frames — select the failed frames, gather
// their symbol rows into a compact batch, scatter the second decoder's outputs back — and the sum of the second stage's
// sweeps for the Monte-Carlo run.  None of them computes anything: they are sized by their bytes (DESIGN, two-stage decoding).
#include <algorithm>

#include "launchers.hpp"

namespace acg {

constexpr int SELECT_THREADS = 1024;  // ONE workgroup: the compaction is stable because one scan orders the whole chunk

// idx[0 .. K) = the frames of the chunk with ok == 0 in ascending order, *count = K, stage[f] = 1 for every frame (stage may
// be null).  Tiles of 1024 flags: a lane's rank among the failures of its wavefront from the ballot, the wavefront's offset
// from the 16 ballot counts in LDS, the tile's offset carried in a register.  K <= frames, so idx needs `frames` entries.
// (One byte per lane and tile: ok + f0 of a caller's buffer is only byte-aligned, and 64 KiB of flags is 64 such tiles.)
__global__ __launch_bounds__(SELECT_THREADS) void cascade_select_kernel(const uint8_t *ok, int32_t frames, int32_t *idx, int32_t *count,
                                                                         uint8_t *stage) {
    __shared__ int wsum[SELECT_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int base = 0;
    for (int t0 = 0; t0 < frames; t0 += SELECT_THREADS) {
        const int f = t0 + tid;
        const bool fail = f < frames && ok[f] == 0;
        if (stage && f < frames) stage[f] = 1;
        const unsigned long long m = __ballot(fail);
        const int before = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[w] = __popcll(m);
        __syncthreads();
        int woff = 0, tot = 0;
        for (int k = 0; k < SELECT_THREADS / 64; k++) {
            const int v = wsum[k];
            woff += k < w ? v : 0;
            tot += v;
        }
        if (fail) idx[base + woff + before] = f;
        base += tot;
        __syncthreads();  // (wsum is rewritten by the next tile)
    }
    if (tid == 0) *count = base;
}

// row k of dst = row idx[k] of src, rows of `units` elements of T: one wavefront per row, the lanes along it.  T is the widest
// type the host could prove every row of BOTH buffers aligned to (cascade_gather_launch).
template <typename T>
__global__ __launch_bounds__(256) void cascade_gather_kernel(const T *src, T *dst, const int32_t *idx, int32_t K, int32_t units) {
    const int lane = threadIdx.x & 63;
    const int wid = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), nw = gridDim.x * (blockDim.x >> 6);
    for (int k = wid; k < K; k += nw) {
        const T *s = src + (size_t) idx[k] * units;
        T *d = dst + (size_t) k * units;
        for (int u = lane; u < units; u += 64) d[u] = s[u];
    }
}

// rows idx[k] of the caller's outputs = row k of the compact ones: nwords words, then (slot nwords of the row) the flag, the
// iteration count where asked for and stage = 2 where asked for.  One thread per (row, slot): the compact side is read in
// order, the caller's side is written in runs of a row.
__global__ __launch_bounds__(256) void cascade_scatter_kernel(const uint32_t *cbits, const uint8_t *cok, const int32_t *citers,
                                                               const int32_t *idx, int32_t K, int32_t nwords, uint32_t *bits, uint8_t *ok,
                                                               int32_t *iters, uint8_t *stage) {
    const int64_t total = (int64_t) K * (nwords + 1);
    for (int64_t t = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t) gridDim.x * blockDim.x) {
        const int k = (int) (t / (nwords + 1)), w = (int) (t - (int64_t) k * (nwords + 1));
        const size_t f = (size_t) idx[k];
        if (w < nwords) {
            bits[f * nwords + w] = cbits[(size_t) k * nwords + w];
        } else {
            ok[f] = cok[k];
            if (iters) iters[f] = citers[k];
            if (stage) stage[f] = 2;
        }
    }
}

// *sum += iters[0 .. K): one atomic per wavefront
__global__ __launch_bounds__(256) void cascade_sum_iters_kernel(const int32_t *iters, int32_t K, unsigned long long *sum) {
    unsigned long long v = 0;
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < K; k += gridDim.x * blockDim.x) v += (unsigned long long) iters[k];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(sum, v);
}

hipError_t cascade_select_launch(const uint8_t *ok, int32_t frames, int32_t *idx, int32_t *count, uint8_t *stage, hipStream_t s) {
    hipLaunchKernelGGL(cascade_select_kernel, dim3(1), dim3(SELECT_THREADS), 0, s, ok, frames, idx, count, stage);
    return hipGetLastError();
}

hipError_t cascade_gather_launch(const void *y, int elem, int32_t n, const int32_t *idx, int32_t K, void *out, hipStream_t s) {
    const size_t row = (size_t) n * elem;
    const int grid = std::max(1, std::min((K + 3) / 4, 2048));
    // rows lie `row` bytes apart from each base: 16-byte accesses where both bases and the row length are multiples of 16,
    // else one element per access (the element's own alignment is all an odd n leaves)
    if (((uintptr_t) y | (uintptr_t) out | row) % 16 == 0)
        hipLaunchKernelGGL(cascade_gather_kernel<uint4>, dim3(grid), dim3(256), 0, s, (const uint4 *) y, (uint4 *) out, idx, K, (int32_t) (row / 16));
    else if (elem == 2)
        hipLaunchKernelGGL(cascade_gather_kernel<uint16_t>, dim3(grid), dim3(256), 0, s, (const uint16_t *) y, (uint16_t *) out, idx, K, n);
    else if (elem == 8)
        hipLaunchKernelGGL(cascade_gather_kernel<uint64_t>, dim3(grid), dim3(256), 0, s, (const uint64_t *) y, (uint64_t *) out, idx, K, n);
    else
        hipLaunchKernelGGL(cascade_gather_kernel<uint32_t>, dim3(grid), dim3(256), 0, s, (const uint32_t *) y, (uint32_t *) out, idx, K, n);
    return hipGetLastError();
}

hipError_t cascade_scatter_launch(const uint32_t *cbits, const uint8_t *cok, const int32_t *citers, const int32_t *idx, int32_t K,
                                  int32_t nwords, uint32_t *bits, uint8_t *ok, int32_t *iters, uint8_t *stage, hipStream_t s) {
    const int64_t total = (int64_t) K * (nwords + 1);
    const int grid = (int) std::max<int64_t>(1, std::min<int64_t>((total + 255) / 256, 4096));
    hipLaunchKernelGGL(cascade_scatter_kernel, dim3(grid), dim3(256), 0, s, cbits, cok, citers, idx, K, nwords, bits, ok, iters, stage);
    return hipGetLastError();
}

hipError_t cascade_sum_iters_launch(const int32_t *iters, int32_t K, unsigned long long *sum, hipStream_t s) {
    const int grid = std::max(1, std::min((K + 255) / 256, 256));
    hipLaunchKernelGGL(cascade_sum_iters_kernel, dim3(grid), dim3(256), 0, s, iters, K, sum);
    return hipGetLastError();
}

}  // namespace acg
