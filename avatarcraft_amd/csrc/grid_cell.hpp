// avatarcraft_amd/csrc/grid_cell.hpp -- hash-grid addressing of the encoder operators (hashgrid.hip; hash_stencil.hip and the table-gradient scatter it includes,
// table_scatter.hpp): a level's constants, the table index of a grid vertex (from coordinates, or from pre-multiplied axis terms), a cell's corners with their
// interpolation weights, and the cell + fraction of a coordinate on one axis.  Arithmetic per point is the reference's (hashencoder.cu:122-166: fma(x, scale, 0.5),
// floor, trilinear weights as products in d order).
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

// the table index of grid vertex pg (hashencoder.cu:46-70): the hash of its coordinates on a hashed level, its row-major position on a dense one
template <uint32_t D>
__device__ __forceinline__ uint32_t gindex(const LevelC &L, const uint32_t (&pg)[D])
{
    constexpr uint32_t primes[3] = { 1u, 2654435761u, 805459861u };
    uint32_t index;
    if (L.hashed) {
        index = pg[0];
#pragma unroll
        for (uint32_t d = 1; d < D; ++d) index ^= pg[d] * primes[d];
    } else {
        index = pg[D - 1];
#pragma unroll
        for (uint32_t d = D - 1; d-- > 0;) index = pg[d] + index * L.stride1;
    }
    if (L.mask) index &= L.mask;
    else if (index >= L.size) index %= L.size;
    return index;
}

__device__ __forceinline__ uint32_t gindex(const LevelC &L, uint32_t x, uint32_t y, uint32_t z)
{
    const uint32_t pg[3] = { x, y, z };
    return gindex<3>(L, pg);
}

// corner idx of the cell pg with fractions pos: its grid vertex pl and its interpolation weight, w0 times the factors of the axes in d order.  Bit n of idx
// set: + 1 along the n-th axis.  skip < D leaves that axis out of both (the derivative along it, hashencoder.cu:177-220: the caller sets pl[skip], and
// seeds the weight with the level's scale); skip = D: all axes
template <uint32_t D>
__device__ __forceinline__ float cell_vertex(uint32_t idx, uint32_t skip, float w0, const float (&pos)[D], const uint32_t (&pg)[D], uint32_t (&pl)[D])
{
    float w = w0;
    uint32_t n = 0;
#pragma unroll
    for (uint32_t d = 0; d < D; ++d) {
        if (d == skip) continue;
        if ((idx & (1u << n)) == 0) { w *= 1.0f - pos[d]; pl[d] = pg[d]; }
        else { w *= pos[d]; pl[d] = pg[d] + 1u; }
        ++n;
    }
    return w;
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
