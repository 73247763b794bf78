// avatarcraft_amd/csrc/hashgrid.hip -- multiresolution hash-grid encoder for gfx950 (stand-alone operator).
//
// Replaces the reference's `_hash_encoder` extension (encoder/hashencoder/src/hashencoder.cu):
//   kernel_grid (:73-220)           -> hash_fwd_kernel<T, D, C>
//   kernel_grid_backward (:223-308) -> hash_bwd_kernel<T, D, C>
//   kernel_input_backward (:311-337)-> hash_input_bwd_kernel<T>
// T = float, __half or double, as the reference dispatches over the dtype of its tensors (:352,391 AT_DISPATCH_FLOATING_TYPES_AND_HALF): one kernel
// template per operator, and what depends on T is in HgTy<T> and the scatter overloads.  Grid addressing (level constants, cell of a coordinate, vertex
// index, corner weights) is grid_cell.hpp's, shared with the training path (hash_stencil.hip).
// The fused renderer (render_fused.hip) has its own in-register copy of the gather; this file is
// the drop-in operator behind `_backend.hash_encode_forward/backward`.
//
// MI355X notes: HBM/L2-bound gather.  One lane = one (point, level); the level is blockIdx.y so
// that a workgroup only touches one level's table (coarse levels stay L2/MALL resident).  The
// C features of a corner are one load of up to 16 bytes (two for 8 floats); level constants (scale, resolution, offset,
// hashed?) come in as launch constants from the host table, no exp2f on the device (bit-exact
// corner indices, SURVEY section 7 hard part ii).
#include "grid_cell.hpp"
#include <hip/hip_fp16.h>
#include <type_traits>

namespace {

// Storage type T, accumulator type A.  What does not depend on T, as in the reference: cell position and interpolation weights in fp32 from (float)inputs
// (hashencoder.cu:125-133,142-154); the range test is on the stored value (a double is tested as a double, :98).  half: features widened on load, the eight
// corners accumulated in fp32 with fma and rounded ONCE on store (the reference rounds every partial sum to half through c10::Half's operators -- lower
// accuracy, never exercised and not reproducible without its CUDA build: DESIGN.md section 3); table gradient as packed half2 atomics for even C
// like hashencoder.cu:293-299 (scalar half atomics for C = 1).  double: accumulated in double; fp64 atomics.
template <class T> struct HgTy;
template <> struct HgTy<float> {
    using A = float;
    static __device__ __forceinline__ float up(float v) { return v; }
    static __device__ __forceinline__ float down(float v) { return v; }
    static __device__ __forceinline__ float fma(float a, float b, float c) { return fma_(a, b, c); }
};
template <> struct HgTy<__half> {
    using A = float;
    static __device__ __forceinline__ float up(__half v) { return __half2float(v); }
    // the fp32 value is pinned in a register first: left alone, the compiler fuses the last fma and the conversion into v_fma_mixlo_f16 (ONE rounding of
    // the exact fma to half), which differs from "fp32 result, then rounded to half" whenever the fp32 result sits on a half tie -- common with half operands
    static __device__ __forceinline__ __half down(float v) { asm volatile("" : "+v"(v)); return __float2half(v); }
    static __device__ __forceinline__ float fma(float a, float b, float c) { return fma_(a, b, c); }
};
template <> struct HgTy<double> {
    using A = double;
    static __device__ __forceinline__ double up(double v) { return v; }
    static __device__ __forceinline__ double down(double v) { return v; }
    static __device__ __forceinline__ double fma(double a, double b, double c) { return __builtin_fma(a, b, c); }
};

// the C features of one table entry, fetched with the widest loads their size allows (entries are C * sizeof(T) apart from an aligned table)
template <class T, uint32_t C> struct alignas(sizeof(T) * C < 16 ? sizeof(T) * C : 16) Feat { T v[C]; };
template <class T, uint32_t C> __device__ __forceinline__ Feat<T, C> feat(const T *g, uint32_t index)
{
    return *reinterpret_cast<const Feat<T, C> *>(g + (size_t)index * C);
}

template <class T, uint32_t D, uint32_t C>
__global__ __launch_bounds__(256) void hash_fwd_kernel(const T *__restrict__ inputs, const T *__restrict__ grid, T *__restrict__ outputs, uint32_t B,
                                                       ac::LevelTable lt, int calc_grad, T *__restrict__ dy_dx)
{
    using Y = HgTy<T>; using A = typename Y::A;
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const uint32_t level = blockIdx.y, L = lt.L;
    const LevelC lv = level_of(lt, level);
    const T *g = grid + (size_t)lt.offset[level] * C;
    A x[D];
    bool oob = false;
#pragma unroll
    for (uint32_t d = 0; d < D; ++d) { x[d] = Y::up(inputs[(size_t)b * D + d]); oob |= (x[d] < 0) | (x[d] > 1); }
    T *out = outputs + ((size_t)level * B + b) * C;
    T *dd = dy_dx + (size_t)b * D * L * C + (size_t)level * D * C;
    if (oob) {
#pragma unroll
        for (uint32_t c = 0; c < C; ++c) out[c] = Y::down((A)0);
        if (calc_grad) for (uint32_t i = 0; i < D * C; ++i) dd[i] = Y::down((A)0);
        return;
    }
    float pos[D]; uint32_t pg[D];
#pragma unroll
    for (uint32_t d = 0; d < D; ++d) { const Loc q = locate_unit((float)x[d], lv.scale); pg[d] = q.pg; pos[d] = q.fr; }
    A acc[C];
#pragma unroll
    for (uint32_t c = 0; c < C; ++c) acc[c] = (A)0;
#pragma unroll
    for (uint32_t idx = 0; idx < (1u << D); ++idx) {
        uint32_t pl[D];
        const float w = cell_vertex<D>(idx, D, 1.0f, pos, pg, pl);
        const Feat<T, C> f = feat<T, C>(g, gindex<D>(lv, pl));
#pragma unroll
        for (uint32_t c = 0; c < C; ++c) acc[c] = Y::fma((A)w, Y::up(f.v[c]), acc[c]);
    }
#pragma unroll
    for (uint32_t c = 0; c < C; ++c) out[c] = Y::down(acc[c]);
    if (calc_grad) {
#pragma unroll
        for (uint32_t gd = 0; gd < D; ++gd) {
            A rg[C];
#pragma unroll
            for (uint32_t c = 0; c < C; ++c) rg[c] = (A)0;
#pragma unroll
            for (uint32_t idx = 0; idx < (1u << (D - 1)); ++idx) {
                uint32_t pl[D];
                const float w = cell_vertex<D>(idx, gd, lv.scale, pos, pg, pl);
                pl[gd] = pg[gd];
                const Feat<T, C> fl = feat<T, C>(g, gindex<D>(lv, pl));
                pl[gd] = pg[gd] + 1u;
                const Feat<T, C> fr = feat<T, C>(g, gindex<D>(lv, pl));
#pragma unroll
                for (uint32_t c = 0; c < C; ++c) rg[c] = Y::fma((A)w, Y::up(fr.v[c]) - Y::up(fl.v[c]), rg[c]);
            }
#pragma unroll
            for (uint32_t c = 0; c < C; ++c) dd[gd * C + c] = Y::down(rg[c]);
        }
    }
}

template <uint32_t C> __device__ __forceinline__ void scatter(float *t, float w, const float (&gc)[C])
{
#pragma unroll
    for (uint32_t c = 0; c < C; ++c) unsafeAtomicAdd(t + c, w * gc[c]);
}
template <uint32_t C> __device__ __forceinline__ void scatter(double *t, float w, const double (&gc)[C])
{
#pragma unroll
    for (uint32_t c = 0; c < C; ++c) unsafeAtomicAdd(t + c, (double)w * gc[c]);
}
template <uint32_t C> __device__ __forceinline__ void scatter(__half *t, float w, const float (&gc)[C])
{
    if constexpr (C % 2 == 0) {
#pragma unroll
        for (uint32_t c = 0; c < C; c += 2) unsafeAtomicAdd(reinterpret_cast<__half2 *>(t + c), __halves2half2(HgTy<__half>::down(w * gc[c]), HgTy<__half>::down(w * gc[c + 1])));
    } else {
#pragma unroll
        for (uint32_t c = 0; c < C; ++c) unsafeAtomicAdd(t + c, HgTy<__half>::down(w * gc[c]));
    }
}

template <class T, uint32_t D, uint32_t C>
__global__ __launch_bounds__(256) void hash_bwd_kernel(const T *__restrict__ grad, const T *__restrict__ inputs, T *__restrict__ grad_grid, uint32_t B,
                                                       ac::LevelTable lt)
{
    using Y = HgTy<T>; using A = typename Y::A;
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const uint32_t level = blockIdx.y;
    const LevelC lv = level_of(lt, level);
    T *gg = grad_grid + (size_t)lt.offset[level] * C;
    float pos[D]; uint32_t pg[D];
#pragma unroll
    for (uint32_t d = 0; d < D; ++d) {
        const A x = Y::up(inputs[(size_t)b * D + d]);
        if (x < 0 || x > 1) return;                 // grad_embeddings is zero-initialised by the caller
        const Loc q = locate_unit((float)x, lv.scale);
        pg[d] = q.pg; pos[d] = q.fr;
    }
    A gcur[C];
#pragma unroll
    for (uint32_t c = 0; c < C; ++c) gcur[c] = Y::up(grad[((size_t)level * B + b) * C + c]);
#pragma unroll
    for (uint32_t idx = 0; idx < (1u << D); ++idx) {
        uint32_t pl[D];
        const float w = cell_vertex<D>(idx, D, 1.0f, pos, pg, pl);
        scatter<C>(gg + (size_t)gindex<D>(lv, pl) * C, w, gcur);
    }
}

// grad_inputs[b,d] = sum_l sum_c grad[l,b,c] * dy_dx[b,l,d,c]   (hashencoder.cu:311-337)
template <class T>
__global__ __launch_bounds__(256) void hash_input_bwd_kernel(const T *__restrict__ grad, const T *__restrict__ dy_dx, T *__restrict__ grad_inputs,
                                                             uint32_t B, uint32_t D, uint32_t C, uint32_t L)
{
    using Y = HgTy<T>; using A = typename Y::A;
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= B * D) return;
    const uint32_t b = t / D, d = t - b * D;
    const T *dd = dy_dx + (size_t)b * L * D * C;
    A r = (A)0;
    for (uint32_t l = 0; l < L; ++l)
        for (uint32_t ch = 0; ch < C; ++ch)
            r = Y::fma(Y::up(grad[((size_t)l * B + b) * C + ch]), Y::up(dd[l * D * C + d * C + ch]), r);
    grad_inputs[t] = Y::down(r);
}

template <uint32_t D>
__global__ __launch_bounds__(256) void hash_corner_kernel(const float *__restrict__ inputs, uint32_t *__restrict__ out,
                                                          uint32_t B, ac::LevelTable lt)
{
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const uint32_t level = blockIdx.y;
    const LevelC lv = level_of(lt, level);
    uint32_t pg[D]; bool oob = false;
#pragma unroll
    for (uint32_t d = 0; d < D; ++d) {
        const Loc q = locate_unit(inputs[(size_t)b * D + d], lv.scale);
        oob |= q.oob; pg[d] = q.pg;
    }
    uint32_t *o = out + ((size_t)level * B + b) * (1u << D);
#pragma unroll
    for (uint32_t idx = 0; idx < (1u << D); ++idx) {
        uint32_t pl[D];
#pragma unroll
        for (uint32_t d = 0; d < D; ++d) pl[d] = pg[d] + ((idx >> d) & 1u);
        o[idx] = oob ? 0xffffffffu : gindex<D>(lv, pl);
    }
}

int check_cfg(uint32_t D, uint32_t C, uint32_t L, const int32_t *offsets_host)
{
    if (!(D == 2 || D == 3) || !(C == 1 || C == 2 || C == 4 || C == 8)) {
        ac::set_error("GridEncoding: C must be 1, 2, 4, or 8 (and D 2 or 3); got D=%u C=%u", D, C);
        return AC_ERR_BAD_ARG;
    }
    if (L == 0 || L > AC_MAX_LEVELS) { ac::set_error("GridEncoding: L=%u out of range (1..%d)", L, AC_MAX_LEVELS); return AC_ERR_BAD_ARG; }
    if (!offsets_host) { ac::set_error("GridEncoding: offsets_host is NULL"); return AC_ERR_BAD_ARG; }
    return AC_OK;
}

// f(d, c) with (D, C) as compile-time constants (d() and c()), for the configurations check_cfg admits
template <uint32_t N> using K = std::integral_constant<uint32_t, N>;
template <class F> void with_dims(uint32_t D, uint32_t C, F &&f)
{
    auto over_c = [&](auto d) {
        switch (C) {
        case 1: f(d, K<1>()); break;
        case 2: f(d, K<2>()); break;
        case 4: f(d, K<4>()); break;
        case 8: f(d, K<8>()); break;
        }
    };
    if (D == 2) over_c(K<2>()); else over_c(K<3>());
}

template <class T>
int encode_forward(const void *inputs, const void *embeddings, const int32_t *offsets_host, void *outputs, uint32_t B, uint32_t D, uint32_t C, uint32_t L,
                   float S, uint32_t H, int calc_grad_inputs, void *dy_dx, ac_stream_t stream)
{
    if (int rc = check_cfg(D, C, L, offsets_host)) return rc;
    if (B == 0) return AC_OK;
    if (!inputs || !embeddings || !outputs || (calc_grad_inputs && !dy_dx)) { ac::set_error("hash_encode_forward: NULL buffer"); return AC_ERR_BAD_ARG; }
    ac::LevelTable lt; ac::make_level_table(lt, L, D, S, H, offsets_host);
    with_dims(D, C, [&](auto d, auto c) {
        hipLaunchKernelGGL((hash_fwd_kernel<T, d(), c()>), dim3((B + 255) / 256, L), dim3(256), 0, (hipStream_t)stream, (const T *)inputs,
                           (const T *)embeddings, (T *)outputs, B, lt, calc_grad_inputs, (T *)dy_dx);
    });
    return ac::check_launch("hash_encode_forward");
}

template <class T>
int encode_backward(const void *grad, const void *inputs, const int32_t *offsets_host, void *grad_embeddings, uint32_t B, uint32_t D, uint32_t C, uint32_t L,
                    float S, uint32_t H, int calc_grad_inputs, const void *dy_dx, void *grad_inputs, ac_stream_t stream)
{
    if (int rc = check_cfg(D, C, L, offsets_host)) return rc;
    if (B == 0) return AC_OK;
    if (!grad || !inputs || !grad_embeddings || (calc_grad_inputs && (!dy_dx || !grad_inputs))) { ac::set_error("hash_encode_backward: NULL buffer"); return AC_ERR_BAD_ARG; }
    ac::LevelTable lt; ac::make_level_table(lt, L, D, S, H, offsets_host);
    hipStream_t st = (hipStream_t)stream;
    with_dims(D, C, [&](auto d, auto c) {
        hipLaunchKernelGGL((hash_bwd_kernel<T, d(), c()>), dim3((B + 255) / 256, L), dim3(256), 0, st, (const T *)grad, (const T *)inputs,
                           (T *)grad_embeddings, B, lt);
    });
    if (calc_grad_inputs)
        hipLaunchKernelGGL(hash_input_bwd_kernel<T>, dim3((B * D + 255) / 256), dim3(256), 0, st, (const T *)grad, (const T *)dy_dx, (T *)grad_inputs, B, D, C, L);
    return ac::check_launch("hash_encode_backward");
}

}  // namespace

AC_API int ac_hash_encode_forward_typed(int dtype, const void *inputs, const void *embeddings, const int32_t *offsets, const int32_t *offsets_host,
                                        void *outputs, uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H, int calc_grad_inputs,
                                        void *dy_dx, ac_stream_t stream)
{
    (void)offsets;
    switch (dtype) {
    case AC_DTYPE_F32: return encode_forward<float>(inputs, embeddings, offsets_host, outputs, B, D, C, L, S, H, calc_grad_inputs, dy_dx, stream);
    case AC_DTYPE_F16: return encode_forward<__half>(inputs, embeddings, offsets_host, outputs, B, D, C, L, S, H, calc_grad_inputs, dy_dx, stream);
    case AC_DTYPE_F64: return encode_forward<double>(inputs, embeddings, offsets_host, outputs, B, D, C, L, S, H, calc_grad_inputs, dy_dx, stream);
    }
    ac::set_error("hash_encode_forward: inputs must be a floating tensor (dtype code %d)", dtype);
    return AC_ERR_BAD_ARG;
}

AC_API int ac_hash_encode_backward_typed(int dtype, const void *grad, const void *inputs, const void *embeddings, const int32_t *offsets,
                                         const int32_t *offsets_host, void *grad_embeddings, uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S,
                                         uint32_t H, int calc_grad_inputs, const void *dy_dx, void *grad_inputs, ac_stream_t stream)
{
    (void)offsets; (void)embeddings;
    switch (dtype) {
    case AC_DTYPE_F32: return encode_backward<float>(grad, inputs, offsets_host, grad_embeddings, B, D, C, L, S, H, calc_grad_inputs, dy_dx, grad_inputs, stream);
    case AC_DTYPE_F16: return encode_backward<__half>(grad, inputs, offsets_host, grad_embeddings, B, D, C, L, S, H, calc_grad_inputs, dy_dx, grad_inputs, stream);
    case AC_DTYPE_F64: return encode_backward<double>(grad, inputs, offsets_host, grad_embeddings, B, D, C, L, S, H, calc_grad_inputs, dy_dx, grad_inputs, stream);
    }
    ac::set_error("hash_encode_backward: grad must be a floating tensor (dtype code %d)", dtype);
    return AC_ERR_BAD_ARG;
}

AC_API int ac_hash_encode_forward(const float *inputs, const float *embeddings, const int32_t *offsets,
                                  const int32_t *offsets_host, float *outputs, uint32_t B, uint32_t D, uint32_t C,
                                  uint32_t L, float S, uint32_t H, int calc_grad_inputs, float *dy_dx, ac_stream_t stream)
{
    return ac_hash_encode_forward_typed(AC_DTYPE_F32, inputs, embeddings, offsets, offsets_host, outputs, B, D, C, L, S, H, calc_grad_inputs, dy_dx, stream);
}

AC_API int ac_hash_encode_backward(const float *grad, const float *inputs, const float *embeddings, const int32_t *offsets,
                                   const int32_t *offsets_host, float *grad_embeddings, uint32_t B, uint32_t D, uint32_t C,
                                   uint32_t L, float S, uint32_t H, int calc_grad_inputs, const float *dy_dx,
                                   float *grad_inputs, ac_stream_t stream)
{
    return ac_hash_encode_backward_typed(AC_DTYPE_F32, grad, inputs, embeddings, offsets, offsets_host, grad_embeddings, B, D, C, L, S, H, calc_grad_inputs,
                                         dy_dx, grad_inputs, stream);
}

AC_API int ac_hash_corner_indices(const float *inputs, const int32_t *offsets_host, uint32_t *corner_idx, uint32_t B,
                                  uint32_t D, uint32_t L, float S, uint32_t H, ac_stream_t stream)
{
    if (int rc = check_cfg(D, 1, L, offsets_host)) return rc;
    if (B == 0) return AC_OK;
    ac::LevelTable lt; ac::make_level_table(lt, L, D, S, H, offsets_host);
    dim3 grid((B + 255) / 256, L);
    hipStream_t st = (hipStream_t)stream;
    if (D == 2) hipLaunchKernelGGL((hash_corner_kernel<2>), grid, dim3(256), 0, st, inputs, corner_idx, B, lt);
    else hipLaunchKernelGGL((hash_corner_kernel<3>), grid, dim3(256), 0, st, inputs, corner_idx, B, lt);
    return ac::check_launch("hash_corner_indices");
}
