// avatarcraft_amd/csrc/field_stencil.hpp -- the hash features of the seven points of the finite-difference stencil in one pass (encode_stencil): the centre's
// features in registers, the six offset points' in the wave's feature slab; coarse levels share the centre's corner fetches, fine levels gather their own.
// Included by field_tile.hpp and by the two ray renderers.
// Everything lives in an anonymous namespace: each translation unit gets its own copy.
#pragma once
#include "hash_gather.hpp"

namespace {

// ---- finite-difference stencil: hash features of the centre point and of p +- eps*e_k (k = x,y,z) ------------------
// The 7 evaluations of finite_difference_normals_approximator (instant_nsr.py:687-704) share most grid corners
// on the coarse levels (eps*scale < 1 cell up to level 11).  Every evaluation still computes ITS OWN position,
// cell and interpolation weights exactly as a stand-alone evaluation would (bit-identical features); only the
// memory fetches are shared: a face of the offset point's cell that coincides with a face of the centre cell
// re-uses the centre's 4 corner values, other faces are gathered under an exec mask.
// fe[e][j][c]: e = 0 centre, 1..6 = +x,-x,+y,-y,+z,-z ; pe[e] = the offset coordinate (clamped) of evaluation e.
struct LvlC { float scale; uint32_t my, mz, offset, mask, hashed; };

// GM (wave-uniform, RenderArgs::jmode of the level group): 1 = all four levels of the group are hashed -- xor only, which the compiler folds with the mask
// into one three-input bit operation per corner; anything else = the per-lane choice between the dense and the hashed index
template <int GM>
__device__ __forceinline__ uint32_t gidx(const LvlC &L, uint32_t tx, uint32_t ty, uint32_t tz)
{
    if constexpr (GM == 1) return (tx ^ ty ^ tz) & L.mask;
    else return (L.hashed ? (tx ^ ty ^ tz) : (tx + ty + tz)) & L.mask;
}
// corner index (0..7) of the i-th corner (i = 0..3, other two axes in increasing order) on face b of axis K
template <int K> __device__ __forceinline__ constexpr int face_corner(int b, int i)
{
    return K == 0 ? (b | (i << 1)) : (K == 1 ? ((i & 1) | (b << 1) | ((i >> 1) << 2)) : (i | (b << 2)));
}

// ---- coarse level (eps*scale < 1 cell): an offset point lies in the centre cell or in the adjacent one, so it needs at
// most ONE face the centre does not have (coordinate g+2 for +eps, g-1 for -eps).  All 8 + 6*4 gathers of the level
// are issued as one batch (lanes that need nothing are masked out; rounds 1 - 2 sent them an out-of-range offset instead), then the 7 interpolations
// run from registers: one memory round trip per level instead of seven.  (As compiled, the compiler folds
// coarse_finish's select into the offset points' loads -- register pre-set to the centre's corner, load under an exec mask, skipped when no lane of the
// wave needs it -- so they leave after the centre's have returned: two round trips.  Forcing one batch was measured and changes nothing, the other wave
// of the SIMD covers the second trip: profiles/r02_experiments.txt.)
template <int K, int SIGN>   // SIGN 0: +eps, 1: -eps
struct AxisGeo { float qk; bool need, oob; };

template <int K, int SIGN, int GM, bool H16>
__device__ __forceinline__ AxisGeo<K, SIGN> coarse_issue(rsrc_t table, const LvlC &L, const uint32_t (&gc)[3], const uint32_t (&tx)[2],
                                                       const uint32_t (&ty)[2], const uint32_t (&tz)[2], bool oob_c, float u,
                                                       u32x2 (&w)[4])
{
    AxisGeo<K, SIGN> a;
    a.oob = oob_c | (u < 0.0f) | (u > 1.0f);
    const float pos = fma_(u, L.scale, 0.5f);
    const uint32_t gk = (uint32_t)__builtin_floorf(pos);
    a.qk = pos - (float)gk;
    a.need = gk != gc[K];                                   // shifted by exactly one cell (host guarantees |shift| <= 1)
    const uint32_t mk = K == 0 ? 1u : (K == 1 ? L.my : L.mz);
    const uint32_t base = K == 0 ? tx[0] : (K == 1 ? ty[0] : tz[0]);
    const uint32_t tk = SIGN == 0 ? base + 2u * mk : base - mk;   // coordinate g+2 / g-1 along K
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = face_corner<K>(0, i);
        const uint32_t ax = K == 0 ? tk : tx[c & 1], ay = K == 1 ? tk : ty[(c >> 1) & 1], az = K == 2 ? tk : tz[(c >> 2) & 1];
        w[i] = u32x2{ 0u, 0u };
        if (a.need) w[i] = table_entry<H16>(table, L.offset + gidx<GM>(L, ax, ay, az));
    }
    return a;
}

template <int K, int SIGN>
__device__ __forceinline__ void coarse_finish(const AxisGeo<K, SIGN> &a, const u32x2 (&vc)[8], const u32x2 (&w)[4], const float (&qc)[3],
                                              float &f0, float &f1)
{
    constexpr int NEWBIT = SIGN == 0 ? 1 : 0;               // +eps: the new face is face 1 of the shifted cell
    u32x2 v2[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int bk = (c >> K) & 1;
        const int i = K == 0 ? (c >> 1) : (K == 1 ? ((c & 1) | ((c >> 2) << 1)) : (c & 3));
        if (bk == NEWBIT) { v2[c].x = a.need ? w[i].x : vc[c].x; v2[c].y = a.need ? w[i].y : vc[c].y; }
        else { v2[c].x = a.need ? vc[c ^ (1 << K)].x : vc[c].x; v2[c].y = a.need ? vc[c ^ (1 << K)].y : vc[c].y; }
    }
    interp8(v2, K == 0 ? a.qk : qc[0], K == 1 ? a.qk : qc[1], K == 2 ? a.qk : qc[2], a.oob, f0, f1);
}

// coarse offset points from bilinear face values (fast precision only): removed, the one run-to-run non-determinism ever seen -- DESIGN.md section 2.1

// ---- fine level (eps spans one cell or more): every offset point gathers its own 8 corners ---------------------------
// the offset point's own cell along K: its two index terms tk[0 / 1], its weight and its out-of-range flag
template <int K>
__device__ __forceinline__ void fine_geo(const LvlC &L, bool oob_c, float u, uint32_t (&tk)[2], float &qk, bool &oob)
{
    oob = oob_c | (u < 0.0f) | (u > 1.0f);
    const float pos = fma_(u, L.scale, 0.5f);
    const uint32_t gk = (uint32_t)__builtin_floorf(pos);
    qk = pos - (float)gk;
    const uint32_t mk = K == 0 ? 1u : (K == 1 ? L.my : L.mz);
    tk[0] = gk * mk; tk[1] = tk[0] + mk;
}
template <int K, int GM, bool H16>
__device__ __forceinline__ void fine_issue(rsrc_t table, const LvlC &L, const uint32_t (&tx)[2], const uint32_t (&ty)[2],
                                           const uint32_t (&tz)[2], bool oob_c, float u, u32x2 (&v)[8], float &qk, bool &oob)
{
    uint32_t tk[2];
    fine_geo<K>(L, oob_c, u, tk, qk, oob);
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const uint32_t ax = K == 0 ? tk[c & 1] : tx[c & 1], ay = K == 1 ? tk[(c >> 1) & 1] : ty[(c >> 1) & 1], az = K == 2 ? tk[(c >> 2) & 1] : tz[(c >> 2) & 1];
        v[c] = table_entry<H16>(table, L.offset + gidx<GM>(L, ax, ay, az));
    }
}

#define AC_FSTORE(E, F0, F1) { fslab[((E - 1) * 8 + 2 * j) * 64 + lane] = F0; fslab[((E - 1) * 8 + 2 * j + 1) * 64 + lane] = F1; }

// one group of four levels (4j + g) of the stencil: centre features in c0 / c1, the six offset points' features to the slab
template <int GM, bool H16>
__device__ __forceinline__ void stencil_levels(const float *__restrict__ lds, float *__restrict__ fslab, rsrc_t table, int lane, int g, int j, bool fine,
                                               float ux, float uy, float uz, bool oob, float xp, float xm, float yp, float ym, float zp, float zm,
                                               float &c0, float &c1)
{
    const uint4 r0 = *reinterpret_cast<const uint4 *>(lds + OFF_LVL + (4 * j + g) * 8);
    const uint4 r1 = *reinterpret_cast<const uint4 *>(lds + OFF_LVL + (4 * j + g) * 8 + 4);
    LvlC L; L.scale = __uint_as_float(r0.x); L.my = r0.y; L.mz = r0.z; L.offset = r0.w; L.mask = r1.x; L.hashed = r1.y;
    float qc[3]; uint32_t gc[3];
    {
        const float qx = fma_(ux, L.scale, 0.5f), qy = fma_(uy, L.scale, 0.5f), qz = fma_(uz, L.scale, 0.5f);
        gc[0] = (uint32_t)__builtin_floorf(qx); gc[1] = (uint32_t)__builtin_floorf(qy); gc[2] = (uint32_t)__builtin_floorf(qz);
        qc[0] = qx - (float)gc[0]; qc[1] = qy - (float)gc[1]; qc[2] = qz - (float)gc[2];
    }
    uint32_t tx[2], ty[2], tz[2];
    tx[0] = gc[0]; tx[1] = gc[0] + 1u; ty[0] = gc[1] * L.my; ty[1] = ty[0] + L.my; tz[0] = gc[2] * L.mz; tz[1] = tz[0] + L.mz;
    u32x2 vc[8];                // the centre's corners: each branch issues them where its order wants them
    if (!fine) {
        u32x2 w0[4], w1[4], w2[4], w3[4], w4[4], w5[4];
#pragma unroll
        for (int c = 0; c < 8; ++c)
            vc[c] = table_entry<H16>(table, L.offset + gidx<GM>(L, tx[c & 1], ty[(c >> 1) & 1], tz[c >> 2]));
        const auto a0 = coarse_issue<0, 0, GM, H16>(table, L, gc, tx, ty, tz, oob, xp, w0);
        const auto a1 = coarse_issue<0, 1, GM, H16>(table, L, gc, tx, ty, tz, oob, xm, w1);
        const auto a2 = coarse_issue<1, 0, GM, H16>(table, L, gc, tx, ty, tz, oob, yp, w2);
        const auto a3 = coarse_issue<1, 1, GM, H16>(table, L, gc, tx, ty, tz, oob, ym, w3);
        const auto a4 = coarse_issue<2, 0, GM, H16>(table, L, gc, tx, ty, tz, oob, zp, w4);
        const auto a5 = coarse_issue<2, 1, GM, H16>(table, L, gc, tx, ty, tz, oob, zm, w5);
        __builtin_amdgcn_sched_barrier(0);
        interp8(vc, qc[0], qc[1], qc[2], oob, c0, c1);
        float f0, f1;
        coarse_finish<0, 0>(a0, vc, w0, qc, f0, f1); AC_FSTORE(1, f0, f1)
        coarse_finish<0, 1>(a1, vc, w1, qc, f0, f1); AC_FSTORE(2, f0, f1)
        coarse_finish<1, 0>(a2, vc, w2, qc, f0, f1); AC_FSTORE(3, f0, f1)
        coarse_finish<1, 1>(a3, vc, w3, qc, f0, f1); AC_FSTORE(4, f0, f1)
        coarse_finish<2, 0>(a4, vc, w4, qc, f0, f1); AC_FSTORE(5, f0, f1)
        coarse_finish<2, 1>(a5, vc, w5, qc, f0, f1); AC_FSTORE(6, f0, f1)
    } else {                // all 56 gathers of the seven points in flight at once: one memory round trip instead of three (221 VGPRs, -2 % time)
        u32x2 va[8], vb[8], vc2[8], vd[8], ve[8], vf[8];
        float qa, qb, qc2, qd, qe, qf, f0, f1; bool oa, ob, oc2, od, oe, of;
        // Issue order.  The centre and the +x / -x points share the (y, z) terms of their corners and lie within a few cells in x, and entries that differ
        // in x inside an aligned block of 8 share a 64-byte sector (dense levels: linear in x; hashed levels: xor with the (y, z) term permutes a block
        // within itself).  Eight waves of gathers go through the CU's L1 at once, so a line is found there only if it is asked for again within a few
        // instructions: for each of the four (y, z) combinations the x-pairs of the three points leave back to back (6 gathers on 1 - 2 sectors), then
        // the +-y / +-z points with their x-pairs adjacent as before.  The barriers pin that order; same values into the same registers.
        // L1 -> L2 requests of a 4096-ray launch 107.2 M -> 100.4 M, launch 0.742 -> 0.715 ms: profiles/stencil_gather_order.txt
        uint32_t xa[2], xb[2];
        fine_geo<0>(L, oob, xp, xa, qa, oa);
        fine_geo<0>(L, oob, xm, xb, qb, ob);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t y = ty[i & 1], z = tz[i >> 1];
            vc[2 * i] = table_entry<H16>(table, L.offset + gidx<GM>(L, tx[0], y, z));
            vc[2 * i + 1] = table_entry<H16>(table, L.offset + gidx<GM>(L, tx[1], y, z));
            va[2 * i] = table_entry<H16>(table, L.offset + gidx<GM>(L, xa[0], y, z));
            va[2 * i + 1] = table_entry<H16>(table, L.offset + gidx<GM>(L, xa[1], y, z));
            vb[2 * i] = table_entry<H16>(table, L.offset + gidx<GM>(L, xb[0], y, z));
            vb[2 * i + 1] = table_entry<H16>(table, L.offset + gidx<GM>(L, xb[1], y, z));
            __builtin_amdgcn_sched_barrier(0);
        }
        fine_issue<1, GM, H16>(table, L, tx, ty, tz, oob, yp, vc2, qc2, oc2);
        fine_issue<1, GM, H16>(table, L, tx, ty, tz, oob, ym, vd, qd, od);
        fine_issue<2, GM, H16>(table, L, tx, ty, tz, oob, zp, ve, qe, oe);
        fine_issue<2, GM, H16>(table, L, tx, ty, tz, oob, zm, vf, qf, of);
        __builtin_amdgcn_sched_barrier(0);
        interp8(vc, qc[0], qc[1], qc[2], oob, c0, c1);
        interp8(va, qa, qc[1], qc[2], oa, f0, f1); AC_FSTORE(1, f0, f1)
        interp8(vb, qb, qc[1], qc[2], ob, f0, f1); AC_FSTORE(2, f0, f1)
        interp8(vc2, qc[0], qc2, qc[2], oc2, f0, f1); AC_FSTORE(3, f0, f1)
        interp8(vd, qc[0], qd, qc[2], od, f0, f1); AC_FSTORE(4, f0, f1)
        interp8(ve, qc[0], qc[1], qe, oe, f0, f1); AC_FSTORE(5, f0, f1)
        interp8(vf, qc[0], qc[1], qf, of, f0, f1); AC_FSTORE(6, f0, f1)
    }
}

template <bool H16 = false>
__device__ __forceinline__ void encode_stencil(const float *__restrict__ lds, float *__restrict__ fslab, const FieldCtx &fc, int lane,
                                               float px, float py, float pz, float eps, float (&fe0)[4][2])
{
    const int g = lane >> 4;
    const rsrc_t table = fc.table;
    const float bound = fc.bound, two_bound = fc.two_bound, inv_tb = fc.inv_tb;
    // normalised coordinates of the centre and of the six offset points (one quotient each, hoisted out of the level loop): unit_div for a verified divisor
    const float ax = px + bound, ay = py + bound, az = pz + bound;
    const float axp = clampf(px + eps, -bound, bound) + bound, axm = clampf(px + (-eps), -bound, bound) + bound;
    const float ayp = clampf(py + eps, -bound, bound) + bound, aym = clampf(py + (-eps), -bound, bound) + bound;
    const float azp = clampf(pz + eps, -bound, bound) + bound, azm = clampf(pz + (-eps), -bound, bound) + bound;
    float ux, uy, uz, xp, xm, yp, ym, zp, zm;
    if (inv_tb != 0.0f) {                                   // wave-uniform
        ux = unit_div(ax, two_bound, inv_tb); uy = unit_div(ay, two_bound, inv_tb); uz = unit_div(az, two_bound, inv_tb);
        xp = unit_div(axp, two_bound, inv_tb); xm = unit_div(axm, two_bound, inv_tb); yp = unit_div(ayp, two_bound, inv_tb);
        ym = unit_div(aym, two_bound, inv_tb); zp = unit_div(azp, two_bound, inv_tb); zm = unit_div(azm, two_bound, inv_tb);
    } else {
        ux = ax / two_bound; uy = ay / two_bound; uz = az / two_bound;
        xp = axp / two_bound; xm = axm / two_bound; yp = ayp / two_bound; ym = aym / two_bound; zp = azp / two_bound; zm = azm / two_bound;
    }
    const bool oob = (ux < 0.0f) | (ux > 1.0f) | (uy < 0.0f) | (uy > 1.0f) | (uz < 0.0f) | (uz > 1.0f);
    // jmode (2 bits each) and jfine (1 bit each) of the four level groups in one scalar register: indexed by the loop counter as arrays they
    // would live in scratch memory, and the load of jfine[j] would sit between the centre's gathers and the offset points' (one more round trip)
    const uint32_t jbits = (uint32_t)fc.jmode[0] | ((uint32_t)fc.jmode[1] << 2) | ((uint32_t)fc.jmode[2] << 4) | ((uint32_t)fc.jmode[3] << 6)
                         | ((fc.jfine[0] ? 1u : 0u) << 8) | ((fc.jfine[1] ? 1u : 0u) << 9) | ((fc.jfine[2] ? 1u : 0u) << 10) | ((fc.jfine[3] ? 1u : 0u) << 11);
#pragma unroll 1
    for (int j = 0; j < 4; ++j) {                           // one copy of each code path; results go to LDS / a rotating fe0
        float c0, c1;
        const bool fine = (jbits >> (8 + j)) & 1u, hashed4 = ((jbits >> (2 * j)) & 3u) == 1u, dense4 = ((jbits >> (2 * j)) & 3u) == 0u;
        (void)dense4;                                       // (unused; taking it out moves register-allocation comments in the assembly)
        // level groups hashed throughout get a second copy of the stencil code (xor-only index arithmetic)
        if (hashed4) stencil_levels<1, H16>(lds, fslab, table, lane, g, j, fine, ux, uy, uz, oob, xp, xm, yp, ym, zp, zm, c0, c1);
        else stencil_levels<2, H16>(lds, fslab, table, lane, g, j, fine, ux, uy, uz, oob, xp, xm, yp, ym, zp, zm, c0, c1);
        // rotate the centre features into place: after the 4th iteration fe0[j] holds level 4j+g
        fe0[0][0] = fe0[1][0]; fe0[0][1] = fe0[1][1]; fe0[1][0] = fe0[2][0]; fe0[1][1] = fe0[2][1];
        fe0[2][0] = fe0[3][0]; fe0[2][1] = fe0[3][1]; fe0[3][0] = c0; fe0[3][1] = c1;
        __builtin_amdgcn_sched_barrier(0);
    }
}
#undef AC_FSTORE

}  // namespace
