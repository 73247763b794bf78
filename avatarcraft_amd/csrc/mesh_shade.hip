// avatarcraft_amd/csrc/mesh_shade.hip -- position on the level set, normal and colour for the points of an exported mesh: its vertices
// (ac_mesh_vertex_attrs) and the texels of its atlas (ac_mesh_bake_texture).  Nothing in the reference: utils.save_mesh(vert, face, ...)
// (stylize.py:263-269) writes geometry only.  Both kernels are the refine-and-shade tile body of shade_tile.hpp over tiles of 16 points.
#include "shade_tile.hpp"
#include "field_host.hpp"

namespace {

// ---------------------------------------------------------------------------------------------------------------- attributes of a mesh's vertices
// What a coloured export needs per vertex and marching cubes does not give: a position ON the level set (the linear zero crossing of a grid edge is off it by
// up to 8.6e-3 on the golden field at 24^3), the field's normal and the colour network there.  Shaped like field_samples_kernel (render_occupancy.hip): a wave owns
// tiles of 16 vertices, lane (n, g) works on vertex n of the tile, the four lanes of a vertex hold the same position.  Per vertex, all in fp32:
//   p = clamp((float)vertex); at most `steps` times: stencil at p -> s, g; r = s - target; |r| <= tol: stop; gg = (gx gx + gy gy) + gz gz; not gg > 1e-12:
//   stop (status 2); q = clamp(p - (r / gg) g); max_k |q_k - p0_k| > max_move: stop (status 3); p = q.  Then normal and colour at the final p.
// The status is the reason the steps ended: 0 the tolerance test of a step was met, 1 all `steps` steps were taken (the value at the final p is in `sdf`).
// One copy of the stencil code serves the steps AND the final evaluation: iteration `it` evaluates at p, then the lanes still moving step; when no lane of the
// wave moved (or it == steps: no step is allowed) that evaluation was at every lane's final position and the loop ends -- at most steps + 1 trips, the count
// wave-uniform, stopped lanes ride along at their p.  No atomics, no waits on other waves.
struct MeshAttrArgs {
    const double *verts;        // [V,3] as mc_vertices_kernel writes them
    const float *dirs;          // [V,3] or NULL: -normal
    uint32_t V;
    int steps;
    float target, tol, max_move;
    float *pos, *nrm, *rgb, *sdf;      // [V,3] [V,3] [V,3] | NULL, [V] | NULL
    uint8_t *status;                   // [V] | NULL
};


__global__ __launch_bounds__(FBLOCK) void mesh_attrs_kernel(const RenderArgs a, const MeshAttrArgs m)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    fill_lds_sdf(lds, a);
    if (m.rgb) fill_lds_color(lds, a);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, g = lane >> 4;
    float *fsl = lds + OFF_WAVE + wave * FE_SLAB;
    const FieldCtx fc = make_ctx(a);
    const float bound = a.bound;
    const RefineOpts ro{ m.steps, m.target, m.tol, m.max_move, m.rgb != nullptr };
    const uint32_t ntiles = (m.V + 15) / 16;
    for (uint32_t tile = blockIdx.x * FW + wave; tile < ntiles; tile += gridDim.x * FW) {
        const uint32_t b = tile * 16 + n, bb = b < m.V ? b : m.V - 1;
        const double *vx = m.verts + 3 * (size_t)bb;
        float px = clampf((float)vx[0], -bound, bound), py = clampf((float)vx[1], -bound, bound), pz = clampf((float)vx[2], -bound, bound);
        const TileShade r = refine_shade_tile(lds, fsl, fc, a, ro, lane, m.dirs, (size_t)bb, true, px, py, pz);
        if (b < m.V && g == 0) {
            m.pos[3 * (size_t)b] = px; m.pos[3 * (size_t)b + 1] = py; m.pos[3 * (size_t)b + 2] = pz;
            m.nrm[3 * (size_t)b] = r.fn.nx; m.nrm[3 * (size_t)b + 1] = r.fn.ny; m.nrm[3 * (size_t)b + 2] = r.fn.nz;
            if (m.rgb) { m.rgb[3 * (size_t)b] = r.rgb[0]; m.rgb[3 * (size_t)b + 1] = r.rgb[1]; m.rgb[3 * (size_t)b + 2] = r.rgb[2]; }
            if (m.sdf) m.sdf[b] = r.s;
            if (m.status) m.status[b] = (uint8_t)r.st;
        }
        wave_sync();
    }
}

// ---------------------------------------------------------------------------------------------------------------- texture bake: the same body over texels
// The atlas is closed form (avatarcraft_amd/geometry.py: atlas_layout): the S x S image is cut into R x R cells of c x c texels, R = S / c; triangle t
// lives in cell t >> 1 (column k % R, row k / R), half t & 1.  Texel (i, j) of a cell belongs to half 0 iff i + j <= c - 2.  Its barycentric weights, in fp32, every
// operation rounded once, L = c - 5:  half 0: w1 = (i - 1) / L, w2 = (j - 1) / L;  half 1: w1 = (c - 2 - i) / L, w2 = (c - 2 - j) / L;  w1 = max(w1, 0),
// w2 = max(w2, 0), s = w1 + w2;  s > 1: w1 /= s, w2 /= s, w0 = 0;  else w0 = 1 - s -- a texel outside the UV triangle takes a point ON the triangle (the gutter).
// Its point, per coordinate: p = (w0 P0 + w1 P1) + w2 P2, clamped to +-bound; then refine_shade_tile, view direction -normal.
// A wave takes tiles of 16 consecutive texels of an image row (ceil(S / 16) tiles per row).  A tile without an owned texel issues no field evaluation (the test is
// wave-uniform); in a tile with some, the lanes of the others ride along at the first owned texel's point without moving, and store owner = -1 and zeros.
struct BakeArgs {
    const float *pos;           // [V,3]
    const int32_t *tris;        // [T,3], every index in [0, V)
    uint32_t T, S, c, R;
    RefineOpts ro;
    float *rgb, *nrm, *sdf;     // [S,S,3], [S,S,3] | NULL, [S,S] | NULL
    int32_t *owner;             // [S,S]
    uint8_t *status;            // [S,S] | NULL
};

__global__ __launch_bounds__(FBLOCK) void texture_bake_kernel(const RenderArgs a, const BakeArgs m)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    fill_lds_sdf(lds, a);
    fill_lds_color(lds, a);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, g = lane >> 4;
    float *fsl = lds + OFF_WAVE + wave * FE_SLAB;
    const FieldCtx fc = make_ctx(a);
    const float bound = a.bound;
    const uint32_t S = m.S, c = m.c, per_row = (S + 15) / 16, ntiles = per_row * S;
    const float L = (float)(c - 5u);
    for (uint32_t tile = blockIdx.x * FW + wave; tile < ntiles; tile += gridDim.x * FW) {
        const uint32_t y = tile / per_row, x = (tile - y * per_row) * 16 + n;
        const uint32_t cx = x / c, cy = y / c, i = x - cx * c, j = y - cy * c;
        const uint32_t h = i + j + 2 <= c ? 0u : 1u, t = 2 * (cy * m.R + cx) + h;
        const bool owned = x < S && cx < m.R && cy < m.R && t < m.T;
        float px = 0.0f, py = 0.0f, pz = 0.0f;
        TileShade r{};
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
        if (ride_along(owned, px, py, pz))                                       // (wave-uniform)
            r = refine_shade_tile(lds, fsl, fc, a, m.ro, lane, nullptr, 0, owned, px, py, pz);
        if (x < S && g == 0) {
            const size_t b = (size_t)y * S + x;
            m.owner[b] = owned ? (int32_t)t : -1;
            m.rgb[3 * b] = owned ? r.rgb[0] : 0.0f; m.rgb[3 * b + 1] = owned ? r.rgb[1] : 0.0f; m.rgb[3 * b + 2] = owned ? r.rgb[2] : 0.0f;
            if (m.nrm) { m.nrm[3 * b] = owned ? r.fn.nx : 0.0f; m.nrm[3 * b + 1] = owned ? r.fn.ny : 0.0f; m.nrm[3 * b + 2] = owned ? r.fn.nz : 0.0f; }
            if (m.sdf) m.sdf[b] = owned ? r.s : 0.0f;
            if (m.status) m.status[b] = owned ? (uint8_t)r.st : (uint8_t)0;
        }
        wave_sync();
    }
}

// the refusal of ac_mesh_attr_opts that both entries make first
int check_attr_opts(const char *who, const ac_mesh_attr_opts *opts)
{
    if (opts->refine_steps < 0 || opts->refine_steps > 16 || !(opts->max_move > 0.0f) || !(opts->fd_eps > 0.0f) || !(opts->bound > 0.0f)) {
        ac::set_error("%s: refine_steps outside 0..16, or max_move, fd_eps or bound not > 0", who); return AC_ERR_BAD_ARG;
    }
    return AC_OK;
}

}  // namespace

AC_API int ac_mesh_vertex_attrs(const ac_field *field, const double *vertices, uint32_t V, const float *dirs, const ac_mesh_attr_opts *opts,
                                float *positions, float *normals, float *rgb, float *sdf, uint8_t *status, ac_stream_t stream)
{
    if (!opts) { ac::set_error("mesh_vertex_attrs: NULL opts"); return AC_ERR_BAD_ARG; }
    if (int rc = check_attr_opts("mesh_vertex_attrs", opts)) return rc;
    if (V == 0) return AC_OK;
    if (!vertices || !positions || !normals) { ac::set_error("mesh_vertex_attrs: NULL buffer"); return AC_ERR_BAD_ARG; }
    if (V > 0xffffffe0u) { ac::set_error("mesh_vertex_attrs: more than 2^32 - 32 vertices"); return AC_ERR_BAD_ARG; }
    RenderArgs a{};
    if (int rc = prep_args(a, field, opts->bound, opts->fd_eps)) return rc;
    MeshAttrArgs m{ vertices, dirs, V, opts->refine_steps, opts->target_sdf, opts->tol, opts->max_move, positions, normals, rgb, sdf, status };
    launch_tiles<mesh_attrs_kernel>((V + 15) / 16, FWD_LDS_FLOATS * sizeof(float), (hipStream_t)stream, a, m);
    return ac::check_launch("mesh_vertex_attrs");
}

AC_API int ac_mesh_bake_texture(const ac_field *field, const float *positions, uint32_t V, const int32_t *triangles, uint32_t T, const ac_atlas_opts *atlas,
                                const ac_mesh_attr_opts *opts, float *rgb, int32_t *owner, float *normals, float *sdf, uint8_t *status, ac_stream_t stream)
{
    if (!atlas || !opts) { ac::set_error("mesh_bake_texture: NULL atlas or opts"); return AC_ERR_BAD_ARG; }
    if (int rc = check_attr_opts("mesh_bake_texture", opts)) return rc;
    const uint32_t S = atlas->size, c = atlas->cell;
    if (c < 8) { ac::set_error("mesh_bake_texture: cell %u < 8", c); return AC_ERR_BAD_ARG; }
    if (S < c || S > 32768u) { ac::set_error("mesh_bake_texture: size %u outside cell .. 32768", S); return AC_ERR_BAD_ARG; }
    const uint32_t R = S / c;
    if ((uint64_t)T > 2ull * R * R) { ac::set_error("mesh_bake_texture: %u triangles, but a %u x %u atlas of %u-texel cells holds 2 (size / cell)^2 = %llu", T, S, S, c, 2ull * R * R); return AC_ERR_BAD_ARG; }
    if (!rgb || !owner || (T && (!positions || !triangles || !V))) { ac::set_error("mesh_bake_texture: NULL buffer"); return AC_ERR_BAD_ARG; }
    RenderArgs a{};
    if (int rc = prep_args(a, field, opts->bound, opts->fd_eps)) return rc;
    BakeArgs m{ positions, triangles, T, S, c, R, { opts->refine_steps, opts->target_sdf, opts->tol, opts->max_move, true }, rgb, normals, sdf, owner, status };
    launch_tiles<texture_bake_kernel>(((S + 15) / 16) * S, FWD_LDS_FLOATS * sizeof(float), (hipStream_t)stream, a, m);
    return ac::check_launch("mesh_bake_texture");
}
