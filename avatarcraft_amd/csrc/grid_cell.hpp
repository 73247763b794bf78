// avatarcraft_amd/csrc/grid_cell.hpp -- hash-grid addressing of the training-path encoder (hash_stencil.hip and the table-gradient scatter it includes,
// table_scatter.hpp): a level's constants, the table index of a grid vertex (from coordinates, or from pre-multiplied axis terms), and the cell + fraction of a
// coordinate on one axis.  Arithmetic per point is the one of hash_fwd_kernel (fma(x, scale, 0.5), floor, trilinear weights as products in d order).
// Anonymous namespace, like field_tile.hpp: the including translation unit gets its own copy.
#pragma once
#include "ac_common.hpp"
#include "ac_devmath.hpp"

using namespace acdev;

namespace {

struct LevelC { float scale; uint32_t stride1, size, hashed, mask; };

__device__ __forceinline__ LevelC level_of(const ac::LevelTable &lt, uint32_t level)
{
    LevelC L;
    L.scale = lt.scale[level]; L.stride1 = lt.stride1[level]; L.size = lt.size[level]; L.hashed = lt.hashed[level]; L.mask = lt.pow2mask[level];
    return L;
}

__device__ __forceinline__ uint32_t gindex(const LevelC &L, uint32_t x, uint32_t y, uint32_t z)
{
    uint32_t index;
    if (L.hashed) index = x ^ (y * 2654435761u) ^ (z * 805459861u);
    else index = x + (y + z * L.stride1) * L.stride1;
    if (L.mask) index &= L.mask;
    else if (index >= L.size) index %= L.size;
    return index;
}

// the same index from PRE-MULTIPLIED axis terms: ty = y * my, tz = z * mz with (my, mz) = the two hash primes on a hashed level, (stride, stride^2) on a dense one
// (x + (y + z s) s = x + y s + z s^2 in 32-bit arithmetic).  A cell's corners and its neighbour planes differ from it by +-1 / +2 along an axis, i.e. by multiples of
// my / mz: their terms are ADDS on the cell's -- two 32-bit multiplications (quarter rate) per point and level instead of two per corner (round 6: the scatter's fill
// kernel spent a quarter of its vector-pipe time in v_mul_lo_u32, each inside a predicated per-corner block the compiler cannot hoist it out of).  Same bits.
__device__ __forceinline__ uint32_t gindex_t(const LevelC &L, uint32_t tx, uint32_t ty, uint32_t tz)
{
    uint32_t index = L.hashed ? (tx ^ ty ^ tz) : (tx + ty + tz);
    if (L.mask) index &= L.mask;
    else if (index >= L.size) index %= L.size;
    return index;
}
__device__ __forceinline__ uint32_t level_my(const LevelC &L) { return L.hashed ? 2654435761u : L.stride1; }
__device__ __forceinline__ uint32_t level_mz(const LevelC &L) { return L.hashed ? 805459861u : L.stride1 * L.stride1; }

// corner k (bit d set: + 1 along axis d) of the cell whose pre-multiplied terms are (x0, ty0, tz0)
__device__ __forceinline__ uint32_t cell_corner(const LevelC &L, uint32_t x0, uint32_t ty0, uint32_t tz0, uint32_t my, uint32_t mz, uint32_t k)
{
    return gindex_t(L, x0 + (k & 1u), ty0 + (((k >> 1) & 1u) ? my : 0u), tz0 + (((k >> 2) & 1u) ? mz : 0u));
}

struct Loc { uint32_t pg; float fr; bool oob; };

// coordinate in [0,1] (the reference's operator takes its inputs like this) -> cell + fraction on one axis
__device__ __forceinline__ Loc locate_unit(float u, float scale)
{
    Loc r;
    r.oob = (u < 0.0f) | (u > 1.0f);
    const float p = fma_(u, scale, 0.5f);
    const float fl = __builtin_floorf(p);
    r.pg = (uint32_t)fl;
    r.fr = p - (float)r.pg;
    return r;
}

// world coordinate -> cell + fraction on one axis; the normalisation to [0,1] is (x + bound) / (2 bound) with a true division, like the fused renderer.
// inv_tb: RN(1 / two_bound) for a divisor unit_div is verified for (ac::verified_reciprocal), else 0 = IEEE division -- the same bits either way
__device__ __forceinline__ Loc locate(float xw, float bound, float two_bound, float scale, float inv_tb = 0.0f)
{
    return locate_unit(inv_tb != 0.0f ? unit_div(xw + bound, two_bound, inv_tb) : (xw + bound) / two_bound, scale);
}

}  // namespace
