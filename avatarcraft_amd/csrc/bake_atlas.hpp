// avatarcraft_amd/csrc/bake_atlas.hpp -- what the two kernels that walk the texels of the closed-form atlas share (mesh_shade.hip: texture_bake_kernel;
// mesh_occlusion.hip: bake_maps_kernel): the launch's arguments, the texel -> triangle -> point prologue, the per-texel stores, and the refusals of their entries.
// Anonymous namespace, like shade_tile.hpp: each translation unit gets its own copy.
#pragma once
#include "shade_tile.hpp"
#include "field_host.hpp"

namespace {

// The atlas is closed form (avatarcraft_amd/geometry.py: atlas_layout): the S x S image is cut into R x R cells of c x c texels, R = S / c; triangle t
// lives in cell t >> 1 (column k % R, row k / R), half t & 1.  Texel (i, j) of a cell belongs to half 0 iff i + j <= c - 2.  Its barycentric weights, in fp32, every
// operation rounded once, L = c - 5:  half 0: w1 = (i - 1) / L, w2 = (j - 1) / L;  half 1: w1 = (c - 2 - i) / L, w2 = (c - 2 - j) / L;  w1 = max(w1, 0),
// w2 = max(w2, 0), s = w1 + w2;  s > 1: w1 /= s, w2 /= s, w0 = 0;  else w0 = 1 - s -- a texel outside the UV triangle takes a point ON the triangle (the gutter).
// Its point, per coordinate: p = (w0 P0 + w1 P1) + w2 P2, clamped to +-bound.
// A wave takes tiles of 16 consecutive texels of an image row (ceil(S / 16) tiles per row).
struct BakeArgs {
    const float *pos;           // [V,3]
    const int32_t *tris;        // [T,3], every index in [0, V)
    uint32_t T, S, c, R;
    RefineOpts ro;
    float *rgb, *nrm, *sdf;     // [S,S,3] | NULL (bake_maps_kernel only), [S,S,3] | NULL, [S,S] | NULL
    int32_t *owner;             // [S,S]
    uint8_t *status;            // [S,S] | NULL
};

struct BakeTexel { uint32_t x, y, t; bool owned; };

// texel n of tile `tile` -> where it is, whose it is and (owned texels; the others keep 0) its point on the triangle
__device__ __forceinline__ BakeTexel bake_texel_point(const BakeArgs &m, uint32_t tile, int n, float bound, float &px, float &py, float &pz)
{
    const uint32_t S = m.S, c = m.c, per_row = (S + 15) / 16;
    const float L = (float)(c - 5u);
    const uint32_t y = tile / per_row, x = (tile - y * per_row) * 16 + n;
    const uint32_t cx = x / c, cy = y / c, i = x - cx * c, j = y - cy * c;
    const uint32_t h = i + j + 2 <= c ? 0u : 1u, t = 2 * (cy * m.R + cx) + h;
    const bool owned = x < S && cx < m.R && cy < m.R && t < m.T;
    px = 0.0f; py = 0.0f; pz = 0.0f;
    if (owned) {
        const int di = h ? (int)(c - 2u - i) : (int)i - 1, dj = h ? (int)(c - 2u - j) : (int)j - 1;
        float w1 = __builtin_fmaxf((float)di / L, 0.0f), w2 = __builtin_fmaxf((float)dj / L, 0.0f), w0 = 0.0f;
        const float s = w1 + w2;
        if (s > 1.0f) { w1 = w1 / s; w2 = w2 / s; } else w0 = 1.0f - s;
        const int32_t *tv = m.tris + 3 * (size_t)t;
        const float *P0 = m.pos + 3 * (size_t)tv[0], *P1 = m.pos + 3 * (size_t)tv[1], *P2 = m.pos + 3 * (size_t)tv[2];
        px = clampf((w0 * P0[0] + w1 * P1[0]) + w2 * P2[0], -bound, bound);
        py = clampf((w0 * P0[1] + w1 * P1[1]) + w2 * P2[1], -bound, bound);
        pz = clampf((w0 * P0[2] + w1 * P1[2]) + w2 * P2[2], -bound, bound);
    }
    return BakeTexel{ x, y, t, owned };
}

// what a texel stores of its shading (the lanes g == 0 of the texels inside the image call it): an unowned texel stores owner = -1 and zeros
__device__ __forceinline__ void bake_texel_store(const BakeArgs &m, const BakeTexel &tx, const TileShade &r)
{
    const size_t b = (size_t)tx.y * m.S + tx.x;
    const bool owned = tx.owned;
    m.owner[b] = owned ? (int32_t)tx.t : -1;
    if (m.rgb) { m.rgb[3 * b] = owned ? r.rgb[0] : 0.0f; m.rgb[3 * b + 1] = owned ? r.rgb[1] : 0.0f; m.rgb[3 * b + 2] = owned ? r.rgb[2] : 0.0f; }
    if (m.nrm) { m.nrm[3 * b] = owned ? r.fn.nx : 0.0f; m.nrm[3 * b + 1] = owned ? r.fn.ny : 0.0f; m.nrm[3 * b + 2] = owned ? r.fn.nz : 0.0f; }
    if (m.sdf) m.sdf[b] = owned ? r.s : 0.0f;
    if (m.status) m.status[b] = owned ? (uint8_t)r.st : (uint8_t)0;
}

// the refusal of ac_mesh_attr_opts that every entry taking one makes first
int check_attr_opts(const char *who, const ac_mesh_attr_opts *opts)
{
    if (opts->refine_steps < 0 || opts->refine_steps > 16 || !(opts->max_move > 0.0f) || !(opts->fd_eps > 0.0f) || !(opts->bound > 0.0f)) {
        ac::set_error("%s: refine_steps outside 0..16, or max_move, fd_eps or bound not > 0", who); return AC_ERR_BAD_ARG;
    }
    return AC_OK;
}

// the refusals of the two bake entries, in this order, then the launch's arguments: RenderArgs of the field and BakeArgs without the output pointers
int prep_bake(const char *who, RenderArgs &a, BakeArgs &m, const ac_field *field, const float *positions, uint32_t V, const int32_t *triangles, uint32_t T,
              const ac_atlas_opts *atlas, const ac_mesh_attr_opts *opts, bool have_required_out, bool want_rgb)
{
    if (!atlas || !opts) { ac::set_error("%s: NULL atlas or opts", who); return AC_ERR_BAD_ARG; }
    if (int rc = check_attr_opts(who, opts)) return rc;
    const uint32_t S = atlas->size, c = atlas->cell;
    if (c < 8) { ac::set_error("%s: cell %u < 8", who, c); return AC_ERR_BAD_ARG; }
    if (S < c || S > 32768u) { ac::set_error("%s: size %u outside cell .. 32768", who, S); return AC_ERR_BAD_ARG; }
    const uint32_t R = S / c;
    if ((uint64_t)T > 2ull * R * R) { ac::set_error("%s: %u triangles, but a %u x %u atlas of %u-texel cells holds 2 (size / cell)^2 = %llu", who, T, S, S, c, 2ull * R * R); return AC_ERR_BAD_ARG; }
    if (!have_required_out || (T && (!positions || !triangles || !V))) { ac::set_error("%s: NULL buffer", who); return AC_ERR_BAD_ARG; }
    if (int rc = prep_args(a, field, opts->bound, opts->fd_eps)) return rc;
    m = BakeArgs{ positions, triangles, T, S, c, R, { opts->refine_steps, opts->target_sdf, opts->tol, opts->max_move, want_rgb }, nullptr, nullptr, nullptr, nullptr, nullptr };
    return AC_OK;
}

}  // namespace
