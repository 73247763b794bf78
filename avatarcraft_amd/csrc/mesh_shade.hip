// avatarcraft_amd/csrc/mesh_shade.hip -- position on the level set, normal and colour for the points of an exported mesh: its vertices
// (ac_mesh_vertex_attrs) and the texels of its atlas (ac_mesh_bake_texture).  Nothing in the reference: utils.save_mesh(vert, face, ...)
// (stylize.py:263-269) writes geometry only.  Both kernels are the refine-and-shade tile body of shade_tile.hpp over tiles of 16 points.
#include "bake_atlas.hpp"

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
// The atlas, a texel's point on its triangle and what a texel stores: bake_atlas.hpp (shared with bake_maps_kernel, mesh_occlusion.hip); then refine_shade_tile,
// view direction -normal.  A tile without an owned texel issues no field evaluation (the test is wave-uniform); in a tile with some, the lanes of the others ride
// along at the first owned texel's point without moving, and store owner = -1 and zeros.
__global__ __launch_bounds__(FBLOCK) void texture_bake_kernel(const RenderArgs a, const BakeArgs m)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    fill_lds_sdf(lds, a);
    fill_lds_color(lds, a);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, g = lane >> 4;
    float *fsl = lds + OFF_WAVE + wave * FE_SLAB;
    const FieldCtx fc = make_ctx(a);
    const uint32_t ntiles = ((m.S + 15) / 16) * m.S;
    for (uint32_t tile = blockIdx.x * FW + wave; tile < ntiles; tile += gridDim.x * FW) {
        float px, py, pz;
        const BakeTexel tx = bake_texel_point(m, tile, n, a.bound, px, py, pz);
        TileShade r{};
        if (ride_along(tx.owned, px, py, pz))                                    // (wave-uniform)
            r = refine_shade_tile(lds, fsl, fc, a, m.ro, lane, nullptr, 0, tx.owned, px, py, pz);
        if (tx.x < m.S && g == 0) bake_texel_store(m, tx, r);
        wave_sync();
    }
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
    RenderArgs a{};
    BakeArgs m{};
    if (int rc = prep_bake("mesh_bake_texture", a, m, field, positions, V, triangles, T, atlas, opts, rgb && owner, true)) return rc;
    m.rgb = rgb; m.nrm = normals; m.sdf = sdf; m.owner = owner; m.status = status;
    const uint32_t S = m.S;
    launch_tiles<texture_bake_kernel>(((S + 15) / 16) * S, FWD_LDS_FLOATS * sizeof(float), (hipStream_t)stream, a, m);
    return ac::check_launch("mesh_bake_texture");
}
