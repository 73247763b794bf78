// avatarcraft_amd/csrc/ac_scan.hpp -- the scan primitives under the ordered passes of the mesh index kernels (mesh_index.hpp builds the passes on them): a
// workgroup's exclusive scan, a wave's inclusive scan and the one-workgroup scan of the per-workgroup totals.  No atomics, no waits between workgroups: every
// position is a function of the input alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

// workgroup-wide exclusive scan of one value per thread (256 threads), in thread order; total -> every thread
__device__ __forceinline__ uint32_t block_exscan_256(uint32_t v, uint32_t *sh /* [8] */, uint32_t &total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t o = (uint32_t)__shfl_up((int)inc, d); if (lane >= d) inc += o; }
    __syncthreads();                              // (sh may still be read by a previous call)
    if (lane == 63) sh[wave] = inc;
    __syncthreads();
    uint32_t base = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) if (w < wave) base += sh[w];
    total = sh[0] + sh[1] + sh[2] + sh[3];
    return base + inc - v;
}

__device__ __forceinline__ uint32_t wave_incscan(uint32_t v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t o = (uint32_t)__shfl_up((int)v, d); if (lane >= d) v += o; }
    return v;
}

// exclusive scan of the per-workgroup totals, a PAIR of counts per word (one in the low, one in the high 16 bits: a workgroup's total of either stays below
// 65536) -> boff[2 * b], boff[2 * b + 1]; totals -> counts[0..1].
// One workgroup of 16 waves; a wave owns a contiguous range of the totals and walks it 64 at a time (coalesced loads, shuffle scan, running carry);
// the waves' totals are combined through LDS and added in a second coalesced pass (131 072 totals at 512^3: 128 steps per wave and pass).
__global__ __launch_bounds__(1024) void pair_scan_kernel(const uint32_t *__restrict__ bsum, uint32_t nblk, uint32_t *__restrict__ boff, uint32_t *__restrict__ counts)
{
    __shared__ uint32_t wv[16], wt[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t per = (((nblk + 15u) / 16u) + 63u) & ~63u, lo = (uint32_t)wave * per, hi = lo + per < nblk ? lo + per : nblk;
    uint32_t cv = 0, ct = 0;
    for (uint32_t b0 = lo; b0 < hi; b0 += 64u) {
        const uint32_t b = b0 + (uint32_t)lane;
        const uint32_t sv = b < hi ? bsum[b] : 0u;
        const uint32_t v = sv & 0xffffu, t = sv >> 16;
        const uint32_t iv = wave_incscan(v, lane), it = wave_incscan(t, lane);
        if (b < hi) { boff[2 * b] = cv + iv - v; boff[2 * b + 1] = ct + it - t; }
        cv += (uint32_t)__shfl((int)iv, 63); ct += (uint32_t)__shfl((int)it, 63);
    }
    if (lane == 0) { wv[wave] = cv; wt[wave] = ct; }
    __syncthreads();
    uint32_t bv = 0, bt = 0;
    for (int w = 0; w < wave; ++w) { bv += wv[w]; bt += wt[w]; }
    if (bv | bt)
        for (uint32_t b = lo + (uint32_t)lane; b < hi; b += 64u) { boff[2 * b] += bv; boff[2 * b + 1] += bt; }
    if (threadIdx.x == 1023) { counts[0] = bv + cv; counts[1] = bt + ct; }
}

}  // namespace
