// avatarcraft_amd/csrc/shade_tile.hpp -- what the consumers of "normal and colour of the field at a point" share (mesh_shade.hip: vertices and texels;
// mesh_occlusion.hip: texels with their occlusion; surface_rays.hip: first hits of rays): the refine-and-shade body of one tile of 16 points, the ride-along rule for the lanes of a tile that have no
// point of their own, and the launch of the persistent tile kernels.  Anonymous namespace, like field_tile.hpp: each translation unit gets its own copy.
#pragma once
#include "field_tile.hpp"

namespace {

// "refine and shade one tile of 16 points": the loop stated at mesh_attrs_kernel (mesh_shade.hip) and the evaluation at the final p; the renderers call it with steps = 0.  In: lane
// (n, g)'s point p (clamped; the four lanes of a point agree) and whether it may move.  Out: the final p, sdf, status, normal and colour there (rgb in the lanes
// g == 0).  dirs / di: the launch's view directions and this lane's row in them, or NULL: -normal.  Every lane of the wave calls it.
struct RefineOpts { int steps; float target, tol, max_move; bool want_rgb; };
struct TileShade { float s; uint32_t st; FdNormal fn; float rgb[3]; };

__device__ __forceinline__ TileShade refine_shade_tile(float *lds, float *fsl, const FieldCtx &fc, const RenderArgs &a, const RefineOpts &m, int lane,
                                                       const float *dirs, size_t di, bool moving, float &px, float &py, float &pz)
{
    const int n = lane & 15;
    const float bound = a.bound, eps = a.eps;
    const float p0x = px, p0y = py, p0z = pz;
    uint32_t st = 1u;
    f32x4 o16;
    float gr[3], s;
#pragma unroll 1
    for (int it = 0;; ++it) {
        float fe0[4][2];
        encode_stencil(lds, fsl, fc, lane, px, py, pz, eps, fe0);
        fd_forward(lds, fsl, lane, px, py, pz, eps, bound, fe0, o16, gr);
        s = __shfl(o16[0], n);                                               // output 0 lives in the lanes g == 0
        wave_sync();                                                         // (every lane is done with the feature slab)
        bool moved = false;
        if (moving && it < m.steps) {
            const float r = s - m.target;
            const float gg = (gr[0] * gr[0] + gr[1] * gr[1]) + gr[2] * gr[2];
            if (__builtin_fabsf(r) <= m.tol) { moving = false; st = 0u; }
            else if (!(gg > 1e-12f)) { moving = false; st = 2u; }
            else {
                const float t = r / gg;
                const float qx = clampf(px - t * gr[0], -bound, bound), qy = clampf(py - t * gr[1], -bound, bound), qz = clampf(pz - t * gr[2], -bound, bound);
                const float dm = __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(qx - p0x), __builtin_fabsf(qy - p0y)), __builtin_fabsf(qz - p0z));
                if (dm > m.max_move) { moving = false; st = 3u; }
                else { px = qx; py = qy; pz = qz; moved = true; }
            }
        }
        if (it >= m.steps || __ballot(moved) == 0ull) break;               // (wave-uniform)
    }
    TileShade r{ s, st, fd_normal(gr[0], gr[1], gr[2]), { 0.0f, 0.0f, 0.0f } };
    if (m.want_rgb) {                                                        // (uniform over the launch)
        if (a.Wsh) {
            float dx = -r.fn.nx, dy = -r.fn.ny, dz = -r.fn.nz;
            if (dirs) { const float *d = dirs + 3 * di; dx = d[0]; dy = d[1]; dz = d[2]; }
            sample_sh_bias(fsl, a.Wsh, dx, dy, dz, lane);
            color_tile(lds, lane, px, py, pz, r.fn.nx, r.fn.ny, r.fn.nz, o16, r.rgb, fsl + 4 * lane, 256);
        } else color_tile(lds, lane, px, py, pz, r.fn.nx, r.fn.ny, r.fn.nz, o16, r.rgb);
    }
    return r;
}

// The ride-along rule: a wave evaluates the field at 64 points whether or not every lane has one, so a lane without a point evaluates at the point of the
// first lane of the wave that has one (the four lanes of a point agree, so that one's lane g == 0 is the lowest set bit) and drops the result.
// In: whether this lane has a point, and the point.  Out: the ballot of `has` -- 0: no lane has a point, (x, y, z) are untouched and the caller skips the
// evaluation (wave-uniform) -- and (x, y, z) = the point this lane evaluates at.  Every lane of the wave calls it.
__device__ __forceinline__ unsigned long long ride_along(bool has, float &x, float &y, float &z)
{
    const unsigned long long mask = __ballot(has);
    if (mask) {
        const int first = __builtin_ctzll(mask) & 15;
        const float fx = __shfl(x, first), fy = __shfl(y, first), fz = __shfl(z, first);
        if (!has) { x = fx; y = fy; z = fz; }
    }
    return mask;
}

// The launch of a kernel that walks tiles of 16 points with FW waves per workgroup: persistent, one workgroup per CU (the 140 KB of LDS of a workgroup with
// feature slabs admit no second one), like ac_field_samples; lds_bytes above 64 KB are allowed once per device and kernel.
uint32_t tile_blocks(uint32_t ntiles)
{
    const uint32_t blocks = (ntiles + FW - 1) / FW, cus = ac::cu_count();
    return blocks > cus ? cus : blocks;
}
template <auto Kernel, typename... Args>
void launch_tiles(uint32_t ntiles, size_t lds_bytes, hipStream_t stream, const Args &...args)
{
    static uint64_t seen = 0;
    ac::allow_dynamic_lds(seen, reinterpret_cast<const void *>(Kernel), lds_bytes);
    hipLaunchKernelGGL(Kernel, dim3(tile_blocks(ntiles)), dim3(FBLOCK), lds_bytes, stream, args...);
}

}  // namespace
