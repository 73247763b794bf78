// avatarcraft_amd/csrc/field_host.hpp -- host only: RenderArgs of a launch from an ac_field -- the level records and gather modes (fill_args), the
// finite-difference step with its fine-level flags (set_fd_eps), both at once (prep_args).
// Included by the files whose entries call them: field_grid.hip, render_occupancy.hip, sdf_stencil_train.hip, color_train.hip, render_core_backward.hip,
// bake_atlas.hpp (mesh_shade.hip, mesh_occlusion.hip), surface_rays.hip, and render_slab.hpp for the two ray renderers (fill_render_common).
// Anonymous namespace: each of them gets its own copy.
#pragma once
#include "field_args.hpp"

namespace {

int fill_args(RenderArgs &a, const ac_field *f, float bound)
{
    if (!f || !f->table || !f->W1 || !f->b1 || !f->W2 || !f->b2 || !f->Wc1 || !f->Wc2 || !f->Wc3) {
        ac::set_error("ac_field: NULL parameter pointer"); return AC_ERR_BAD_ARG;
    }
    ac::LevelTable lt; ac::make_level_table(lt, 16, 3, f->S, f->H, f->offsets);
    for (int l = 0; l < 16; ++l) {
        const bool hashed = lt.hashed[l] != 0, pow2 = lt.pow2mask[l] != 0;
        a.lvl[l].scale = lt.scale[l]; a.lvl[l].offset = lt.offset[l]; a.lvl[l].hashed = hashed ? 1u : 0u;
        a.lvl[l].my = hashed ? 2654435761u : lt.stride1[l];
        a.lvl[l].mz = hashed ? 805459861u : lt.stride1[l] * lt.stride1[l];
        a.lvl[l].mask = (hashed && pow2) ? lt.pow2mask[l] : 0xffffffffu;
        a.lvl[l].wsize = (hashed && !pow2) ? lt.size[l] : 0u;
        a.lvl[l].pad = 0;
        if (a.lvl[l].wsize) {
            ac::set_error("ac_field: level %d is hashed with a non power-of-two size %u; the fused renderer supports tables "
                          "allocated by HashEncoder only (use ac_hash_encode_forward for arbitrary layouts)", l, lt.size[l]);
            return AC_ERR_BAD_ARG;
        }
        if (lt.size[l] == 0) { ac::set_error("ac_field: level %d has zero size", l); return AC_ERR_BAD_ARG; }
    }
    for (int j = 0; j < 4; ++j) {
        int nh = 0;
        for (int g = 0; g < 4; ++g) nh += lt.hashed[4 * j + g] ? 1 : 0;
        a.jmode[j] = nh == 0 ? 0 : (nh == 4 ? 1 : 2);
    }
    a.prepared = static_cast<const float *>(f->prepared);
    a.Wsh = f->Wc1_sh;
    a.table = f->table; a.table_bytes = (uint32_t)f->offsets[16] * 8u; a.W1 = f->W1; a.b1 = f->b1; a.W2 = f->W2; a.b2 = f->b2; a.Wc1 = f->Wc1; a.Wc2 = f->Wc2; a.Wc3 = f->Wc3;
    a.bound = bound; a.two_bound = (float)(2.0 * (double)bound);
    a.inv_tb = ac::verified_reciprocal(a.two_bound);
    return AC_OK;
}

// the finite-difference step, and per gather round of encode_stencil whether one of its levels reaches past the neighbouring cell (jfine)
void set_fd_eps(RenderArgs &a, float eps)
{
    a.eps = eps;
    for (int j = 0; j < 4; ++j) {
        a.jfine[j] = 0;
        for (int g = 0; g < 4; ++g) {
            const double cells = (double)eps / (double)a.two_bound * (double)a.lvl[4 * j + g].scale;
            if (!(cells * 1.001 + 1e-3 < 1.0)) a.jfine[j] = 1;
        }
    }
}

int prep_args(RenderArgs &a, const ac_field *field, float bound, float eps)
{
    if (int rc = fill_args(a, field, bound)) return rc;
    set_fd_eps(a, eps);
    return AC_OK;
}

}  // namespace
