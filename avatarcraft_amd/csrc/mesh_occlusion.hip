// avatarcraft_amd/csrc/mesh_occlusion.hip -- ambient occlusion for the exported mesh and the surface renders: how open the space above a point of the level set is,
// asked of the SDF itself by cone taps (occlusion_tile.hpp; the procedure, operation by operation: include/avatarcraft_hip.h, ac_field_occlusion) -- at arbitrary
// points (ac_field_occlusion: the vertices, the first hits of rays) and fused into the texel bake (ac_mesh_bake_maps: one launch refines a texel's point, shades it
// and takes its occlusion).  Nothing in the reference: its export writes geometry only.
#include "occlusion_tile.hpp"
#include "bake_atlas.hpp"

namespace {

// ---------------------------------------------------------------------------------------------------------------- occlusion at arbitrary points
// A wave owns tiles of 16 points, lane (n, g) serves point n of the tile.  Only the SDF side of the field is laid out in LDS (like posed_trip_kernel,
// surface_rays.hip), the kit's tables behind it.  A point is active if the mask says so (NULL: every point) and its point and normal are finite; inactive points
// store 0 and are never evaluated.  No atomics, no waits on other waves, plain vector stores; a short last tile reads point N - 1 and stores nothing for its
// padding lanes.
struct OccArgs {
    const float *pts, *nrm;     // [N,3] [N,3]
    const uint8_t *active;      // [N] | NULL
    uint32_t N;
    float *out;                 // [N]
};

__global__ __launch_bounds__(FBLOCK) void field_occlusion_kernel(const RenderArgs a, const OccArgs m, const OccKit k)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    fill_lds_sdf(lds, a);
    float *kit = lds + OFF_WAVE;
    fill_lds_kit(kit, k);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, g = lane >> 4;
    const FieldCtx fc = make_ctx(a);
    const float bound = a.bound;
    const uint32_t ntiles = (m.N + 15) / 16;
    for (uint32_t tile = blockIdx.x * FW + wave; tile < ntiles; tile += gridDim.x * FW) {
        const uint32_t b = tile * 16 + n, bb = b < m.N ? b : m.N - 1;
        const float *pp = m.pts + 3 * (size_t)bb, *pn = m.nrm + 3 * (size_t)bb;
        const float x = pp[0], y = pp[1], z = pp[2], nx = pn[0], ny = pn[1], nz = pn[2];
        const bool active = b < m.N && (!m.active || m.active[bb] != 0) && finite3(x, y, z) && finite3(nx, ny, nz);
        const float o = occlusion_tile(lds, kit, fc, lane, k.K, k.J, k.gain, k.level, bound, active,
                                       clampf(x, -bound, bound), clampf(y, -bound, bound), clampf(z, -bound, bound), nx, ny, nz);
        if (b < m.N && g == 0) m.out[b] = o;
    }
}

// ---------------------------------------------------------------------------------------------------------------- the texel bake with its maps
// texture_bake_kernel (mesh_shade.hip) with more to store per texel: the prologue and the stores are bake_atlas.hpp's, then refine_shade_tile (the colour network
// only when rgb is wanted), then -- with a kit -- the occlusion tile at the refined point and normal of the owned texels: colour and occlusion share the texel's
// refine.  The kit's tables sit behind the waves' feature slabs.
struct MapArgs {
    float *pos, *occ;           // [S,S,3] | NULL, [S,S] | NULL (exactly when k.K == 0)
};

__global__ __launch_bounds__(FBLOCK) void bake_maps_kernel(const RenderArgs a, const BakeArgs m, const MapArgs x, const OccKit k)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    fill_lds_sdf(lds, a);
    if (m.rgb) fill_lds_color(lds, a);
    float *kit = lds + FWD_LDS_FLOATS;
    if (k.K) fill_lds_kit(kit, k);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, g = lane >> 4;
    float *fsl = lds + OFF_WAVE + wave * FE_SLAB;
    const FieldCtx fc = make_ctx(a);
    const uint32_t ntiles = ((m.S + 15) / 16) * m.S;
    for (uint32_t tile = blockIdx.x * FW + wave; tile < ntiles; tile += gridDim.x * FW) {
        float px, py, pz;
        const BakeTexel tx = bake_texel_point(m, tile, n, a.bound, px, py, pz);
        TileShade r{};
        float o = 0.0f;
        if (ride_along(tx.owned, px, py, pz)) {                                  // (wave-uniform)
            r = refine_shade_tile(lds, fsl, fc, a, m.ro, lane, nullptr, 0, tx.owned, px, py, pz);
            if (k.K)                                                             // (uniform over the launch)
                o = occlusion_tile(lds, kit, fc, lane, k.K, k.J, k.gain, k.level, a.bound, tx.owned && finite3(px, py, pz) && finite3(r.fn.nx, r.fn.ny, r.fn.nz),
                                   px, py, pz, r.fn.nx, r.fn.ny, r.fn.nz);
        }
        if (tx.x < m.S && g == 0) {
            bake_texel_store(m, tx, r);
            const size_t b = (size_t)tx.y * m.S + tx.x;
            if (x.pos) { x.pos[3 * b] = tx.owned ? px : 0.0f; x.pos[3 * b + 1] = tx.owned ? py : 0.0f; x.pos[3 * b + 2] = tx.owned ? pz : 0.0f; }
            if (x.occ) x.occ[b] = o;
        }
        wave_sync();
    }
}

// the refusals of ac_occlusion_opts that both entries make, on the host, and the kit as the kernels take it
int make_kit(const char *who, const ac_occlusion_opts *o, OccKit &k)
{
    if (o->n_dirs < 1 || o->n_dirs > OCC_MAX_DIRS || o->n_steps < 1 || o->n_steps > OCC_MAX_STEPS) {
        ac::set_error("%s: occlusion kit with n_dirs %d outside 1..32 or n_steps %d outside 1..16", who, o->n_dirs, o->n_steps); return AC_ERR_BAD_ARG;
    }
    if (!o->dirs || !o->weights || !o->dists) { ac::set_error("%s: occlusion kit with a NULL table", who); return AC_ERR_BAD_ARG; }
    auto fin = [](float v) { return fabsf(v) < INFINITY; };
    if (!fin(o->gain) || !(o->gain > 0.0f) || !fin(o->level)) { ac::set_error("%s: occlusion kit needs a finite gain > 0 and a finite level", who); return AC_ERR_BAD_ARG; }
    k = OccKit{};
    k.K = o->n_dirs; k.J = o->n_steps; k.gain = o->gain; k.level = o->level;
    double sum = 0.0;
    for (int i = 0; i < k.K; ++i) {
        const float *l = o->dirs + 3 * i;
        const float w = o->weights[i];
        if (!fin(l[0]) || !fin(l[1]) || !fin(l[2]) || !fin(w)) { ac::set_error("%s: occlusion kit: direction or weight %d is not finite", who, i); return AC_ERR_BAD_ARG; }
        if (!(l[2] >= 0.05f)) { ac::set_error("%s: occlusion kit: direction %d has lz %g < 0.05", who, i, (double)l[2]); return AC_ERR_BAD_ARG; }
        const double len = sqrt(((double)l[0] * l[0] + (double)l[1] * l[1]) + (double)l[2] * l[2]);
        if (!(fabs(len - 1.0) <= 1e-3)) { ac::set_error("%s: occlusion kit: direction %d has length %g, not within 1e-3 of 1", who, i, len); return AC_ERR_BAD_ARG; }
        if (!(w >= 0.0f)) { ac::set_error("%s: occlusion kit: weight %d is negative", who, i); return AC_ERR_BAD_ARG; }
        sum += (double)w;
        k.tab[OCC_DIRS + 3 * i] = l[0]; k.tab[OCC_DIRS + 3 * i + 1] = l[1]; k.tab[OCC_DIRS + 3 * i + 2] = l[2];
        k.tab[OCC_WEIGHTS + i] = w;
    }
    if (!(fabs(sum - 1.0) <= 1e-5)) { ac::set_error("%s: occlusion kit: the weights sum to %.9g, not within 1e-5 of 1", who, sum); return AC_ERR_BAD_ARG; }
    for (int j = 0; j < k.J; ++j) {
        const float t = o->dists[j];
        if (!fin(t) || !(t > 0.0f) || (j && !(t > o->dists[j - 1]))) { ac::set_error("%s: occlusion kit: the distances must be finite, > 0 and strictly ascending (distance %d)", who, j); return AC_ERR_BAD_ARG; }
        k.tab[OCC_DISTS + j] = t;
    }
    return AC_OK;
}

}  // namespace

AC_API int ac_field_occlusion(const ac_field *field, const float *points, const float *normals, const uint8_t *active, uint32_t N, float bound,
                              const ac_occlusion_opts *opts, float *occlusion, ac_stream_t stream)
{
    const char *who = "field_occlusion";
    if (!opts) { ac::set_error("%s: NULL opts", who); return AC_ERR_BAD_ARG; }
    OccKit k;
    if (int rc = make_kit(who, opts, k)) return rc;
    if (!(bound > 0.0f)) { ac::set_error("%s: bound not > 0", who); return AC_ERR_BAD_ARG; }
    if (N == 0) return AC_OK;
    if (!points || !normals || !occlusion) { ac::set_error("%s: NULL buffer", who); return AC_ERR_BAD_ARG; }
    if (N > 0xffffffe0u) { ac::set_error("%s: more than 2^32 - 32 points", who); return AC_ERR_BAD_ARG; }
    RenderArgs a{};
    if (int rc = fill_args(a, field, bound)) return rc;
    launch_tiles<field_occlusion_kernel>((N + 15) / 16, (OFF_WAVE + OCC_FLOATS) * sizeof(float), (hipStream_t)stream, a, OccArgs{ points, normals, active, N, occlusion }, k);
    return ac::check_launch(who);
}

AC_API int ac_mesh_bake_maps(const ac_field *field, const float *positions, uint32_t V, const int32_t *triangles, uint32_t T, const ac_atlas_opts *atlas,
                             const ac_mesh_attr_opts *attr_opts, const ac_occlusion_opts *occ_opts, const ac_bake_out *out, ac_stream_t stream)
{
    const char *who = "mesh_bake_maps";
    if (!out) { ac::set_error("%s: NULL out", who); return AC_ERR_BAD_ARG; }
    if ((out->occlusion == nullptr) != (occ_opts == nullptr)) { ac::set_error("%s: out->occlusion and occ_opts go together: both or neither", who); return AC_ERR_BAD_ARG; }
    OccKit k{};
    if (occ_opts) if (int rc = make_kit(who, occ_opts, k)) return rc;
    RenderArgs a{};
    BakeArgs m{};
    if (int rc = prep_bake(who, a, m, field, positions, V, triangles, T, atlas, attr_opts, out->owner != nullptr, out->rgb != nullptr)) return rc;
    m.rgb = out->rgb; m.nrm = out->normals; m.sdf = out->sdf; m.owner = out->owner; m.status = out->status;
    launch_tiles<bake_maps_kernel>(((m.S + 15) / 16) * m.S, (FWD_LDS_FLOATS + OCC_FLOATS) * sizeof(float), (hipStream_t)stream, a, m, MapArgs{ out->positions, out->occlusion }, k);
    return ac::check_launch(who);
}
