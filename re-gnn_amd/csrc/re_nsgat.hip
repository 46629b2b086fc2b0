// mag REGATConv attention over one device-sampled block as the sampler leaves it (regnn_ns_hop's
// capacity-sized CSR: ptr [cap_dst + 1], idx / rel [cap_e], rows past the live ones empty):
// mag/regnn_layers.py:253-273 with the softmax of mag/utils.py:45-57 (ONE maximum over every live
// entry and head, + 1e-16 in the denominator). No host size anywhere: a row is live when it has
// entries. Rows are short (fan-out <= 64 plus the self loop), so a wave takes a row, holds up to
// 64 of its entries in LDS and loops in entry order past that; there is no long-segment plan.
//
//   launch 1  ns_gat_score_kernel   s[e,h] into the `a` buffer, one maximum per workgroup
//   launch 2  ns_gat_fwd_kernel     every wave folds the workgroup maxima (a maximum does not
//                                   depend on the order; every slot is rewritten each call, so a
//                                   replayed graph needs no reset), den in entry order, a, out
//   backward  ns_gat_bwd_kernel     ga, D, gs, gl per row; g_er and the relation slab in entry
//                                   order; g_el / g_ft by float atomics (form (b), regnn_hip.h)
//   or        ns_gat_bwd_rows_kernel  the same row pass without the atomics, gl per entry kept,
//             + re_nsgat_src.h        then g_ft / g_el by a gather over the block's transposed
//                                   index (form (a), regnn_ns_gat_bwd_gather): no atomics
#include "re_nsgat_common.h"
#include "re_nsgat_src.h"

namespace regnn {
namespace {

__device__ __forceinline__ float pre_act(const float* __restrict__ el, const float* __restrict__ er,
                                         const float* __restrict__ tab, int u, int64_t v, int r,
                                         int H, int h) {
    const float x = el[int64_t(u) * H + h] + er[v * H + h];
    return tab ? x + tab[r * H + h] : x;
}

__global__ void __launch_bounds__(kBlock)
ns_gat_score_kernel(const int32_t* __restrict__ ptr, const int32_t* __restrict__ idx,
                    const uint8_t* __restrict__ rel, const float* __restrict__ el,
                    const float* __restrict__ er, const float* __restrict__ tab, float slope,
                    int64_t n_rows, int64_t n_src, int H, float* __restrict__ s,
                    float* __restrict__ wgmax) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float m = -INFINITY;
    for (int64_t v = int64_t(blockIdx.x) * kWaves + wave; v < n_rows;
         v += int64_t(gridDim.x) * kWaves) {
        const int e0 = ptr[v], e1 = ptr[v + 1];
        const int n = (e1 - e0) * H;
        for (int i = lane; i < n; i += 64) {
            const int j = i / H, h = i - j * H;
            const int e = e0 + j;
            const int u = idx[e];
            float x = -INFINITY;
            if (src_ok(u, n_src)) {
                x = pre_act(el, er, tab, u, v, tab ? rel[e] : 0, H, h);
                x = x > 0.f ? x : x * slope;
                m = fmaxf(m, x);
            }
            s[int64_t(e) * H + h] = x;
        }
    }
    store_wg_max(m, wgmax);
}

__global__ void __launch_bounds__(kBlock)
ns_gat_fwd_kernel(const int32_t* __restrict__ ptr, const int32_t* __restrict__ idx,
                  const float* __restrict__ ft, const float* __restrict__ wgmax, int n_wg,
                  int64_t n_rows, int64_t n_src, int H, int C, float* __restrict__ a,
                  float* __restrict__ out) {
    ns_softmax_aggregate(ptr, idx, ft, wgmax, n_wg, n_rows, n_src, H, C, a, out);
}

// One wave per row. Pass 1 over the row's chunks (NsRow, re_nsgat_common.h, shared with GATv2):
// ga[e,h] = <gy[v,h,:], ft[u,h,:]> (a lane per (entry, head), columns in order) and D[v,h] =
// sum a ga in entry order. Pass 2, this operator's own: gs, gl (the pre-activation's sign
// recomputed from el + er + tab), g_er and the wave's relation bins by lane h in entry order, g_el
// and g_ft by atomics -- g_ft as one instruction per 64 consecutive columns of a source row (256
// contiguous bytes). A row of more than one chunk recomputes ga in pass 2 (the same instructions
// on the same operands: the same bits).
//
// kGather (regnn_ns_gat_bwd_gather's row pass): this one body with the atomics compiled out --
// gl[e,h] goes to the per-entry scratch `ent` (0 for an entry that takes no part) and g_ft / g_el
// are left to the source pass (re_nsgat_src.h).
template <bool kGather>
__device__ __forceinline__ void
ns_gat_bwd_body(const int32_t* __restrict__ ptr, const int32_t* __restrict__ idx,
                const uint8_t* __restrict__ rel, const float* __restrict__ el,
                const float* __restrict__ er, const float* __restrict__ tab,
                const float* __restrict__ ft, const float* __restrict__ a,
                const float* __restrict__ gy, float slope, int64_t n_rows, int64_t n_src, int H,
                int C, int n_rel, float* __restrict__ g_ft, float* __restrict__ g_el,
                float* __restrict__ g_er, float* __restrict__ slab, float* __restrict__ ent) {
    extern __shared__ float bins_[];           // [kWaves][n_rel * H] when slab
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const NsRow s = ns_row(idx, rel, tab != nullptr, ft, a, n_src, H, C);
    const int W = n_rel * H;
    float* bins = bins_ + wave * W;
    if (slab) ns_bins_zero(bins_, W);
    const int HC = H * C;
    for (int64_t v = int64_t(blockIdx.x) * kWaves + wave; v < n_rows;
         v += int64_t(gridDim.x) * kWaves) {
        const int e0 = ptr[v], e1 = ptr[v + 1];
        if (e1 <= e0) {
            if (lane < H) g_er[v * H + lane] = 0.f;
            continue;
        }
        const float* gyr = gy + v * HC;
        const bool one = s.pass1(gyr, e0, e1);
        float ger = 0.f;
        for (int cb = e0; cb < e1; cb += kChunk) {
            const int nc = min(kChunk, e1 - cb);
            if (!one) s.fill(gyr, cb, nc);
            else wave_lds_sync();              // sD written
            for (int i = lane; i < nc * H; i += 64) {
                const int j = i / H, hh = i - j * H;
                const int u = s.su[j];
                float gl = 0.f;
                if (u >= 0) {
                    const float gs = s.sa[i] * (s.sg[i] - s.sD[hh]);
                    gl = pre_act(el, er, tab, u, v, s.sr[j], H, hh) > 0.f ? gs : gs * slope;
                    if constexpr (!kGather) unsafeAtomicAdd(g_el + int64_t(u) * H + hh, gl);
                }
                if constexpr (kGather) ent[int64_t(cb + j) * H + hh] = gl;
                s.sg[i] = gl;                  // (this lane's own slot)
            }
            wave_lds_sync();
            if (lane < H) {
                for (int j = 0; j < nc; ++j) {
                    const float gl = s.sg[j * H + lane];
                    ger += gl;
                    const int r = s.sr[j];
                    if (slab && r < n_rel) bins[r * H + lane] += gl;
                }
            }
            if constexpr (!kGather) {
                for (int col = lane; col < HC; col += 64) {
                    const int h = col / C;
                    const float g = gyr[col];
                    for (int j = 0; j < nc; ++j) {
                        const int u = s.su[j];
                        if (u >= 0)
                            unsafeAtomicAdd(g_ft + int64_t(u) * HC + col, s.sa[j * H + h] * g);
                    }
                }
            }
        }
        if (lane < H) g_er[v * H + lane] = ger;
    }
    if (slab) ns_bins_store(bins_, W, slab);
}

__global__ void __launch_bounds__(kBlock)
ns_gat_bwd_kernel(const int32_t* __restrict__ ptr, const int32_t* __restrict__ idx,
                  const uint8_t* __restrict__ rel, const float* __restrict__ el,
                  const float* __restrict__ er, const float* __restrict__ tab,
                  const float* __restrict__ ft, const float* __restrict__ a,
                  const float* __restrict__ gy, float slope, int64_t n_rows, int64_t n_src, int H,
                  int C, int n_rel, float* __restrict__ g_ft, float* __restrict__ g_el,
                  float* __restrict__ g_er, float* __restrict__ slab) {
    ns_gat_bwd_body<false>(ptr, idx, rel, el, er, tab, ft, a, gy, slope, n_rows, n_src, H, C,
                           n_rel, g_ft, g_el, g_er, slab, nullptr);
}

__global__ void __launch_bounds__(kBlock)
ns_gat_bwd_rows_kernel(const int32_t* __restrict__ ptr, const int32_t* __restrict__ idx,
                       const uint8_t* __restrict__ rel, const float* __restrict__ el,
                       const float* __restrict__ er, const float* __restrict__ tab,
                       const float* __restrict__ ft, const float* __restrict__ a,
                       const float* __restrict__ gy, float slope, int64_t n_rows, int64_t n_src,
                       int H, int C, int n_rel, float* __restrict__ g_er,
                       float* __restrict__ slab, float* __restrict__ ent) {
    ns_gat_bwd_body<true>(ptr, idx, rel, el, er, tab, ft, a, gy, slope, n_rows, n_src, H, C,
                          n_rel, nullptr, nullptr, g_er, slab, ent);
}

// Both backward entry points (x: the gather form's own arguments). The refusals, before any
// launch: invalid arguments, the shape gate, the budgets, then the gather form's capacities. The
// row pass: with a slab exactly slab_rows workgroups (each writes its row), without one and
// without rows nothing. The source pass runs either way: every g_ft / g_el row is written.
template <bool kGather>
inline int gat_bwd(const int32_t* ptr, const int32_t* idx, const uint8_t* rel, const float* el,
                   const float* er, const float* tab, const float* ft, const float* a,
                   const float* gy, float slope, int64_t cap_dst, int64_t n_src, int32_t H,
                   int32_t C, int32_t n_rel, float* g_ft, float* g_el, float* g_er, float* slab,
                   int32_t slab_rows, const SrcIdx& x, hipStream_t stream) {
    if (!ptr || !idx || !el || !er || !ft || !a || !gy || !g_ft || !g_el || !g_er ||
        (tab && !rel) || (slab && !tab) || cap_dst < 0 || n_src < 0 || n_rel < 0 ||
        (tab && n_rel < 1) || (slab && slab_rows < 1) || (kGather && x.invalid()))
        return REGNN_EINVAL;
    if (const int rc = ns_gat_shape_rc(H, C)) return rc;
    if (slab &&
        (int64_t(n_rel) * H > REGNN_NS_GAT_MAX_BINS || slab_rows > REGNN_NS_GAT_WORK_FLOATS))
        return REGNN_EUNSUPPORTED;
    if (kGather && x.over(cap_dst, int64_t(H) * C)) return REGNN_EUNSUPPORTED;
    if (cap_dst > 0 || slab) {
        const int grid = slab ? int(slab_rows) : ns_gat_grid(cap_dst);
        const size_t lds = slab ? size_t(kWaves) * n_rel * H * sizeof(float) : 0;
        if constexpr (kGather) {
            hipLaunchKernelGGL(ns_gat_bwd_rows_kernel, dim3(grid), dim3(kBlock), lds, stream, ptr,
                               idx, rel, el, er, tab, ft, a, gy, slope, cap_dst, n_src, int(H),
                               int(C), int(n_rel), g_er, slab, x.ent);
        } else {
            hipLaunchKernelGGL(ns_gat_bwd_kernel, dim3(grid), dim3(kBlock), lds, stream, ptr, idx,
                               rel, el, er, tab, ft, a, gy, slope, cap_dst, n_src, int(H), int(C),
                               int(n_rel), g_ft, g_el, g_er, slab);
        }
        REGNN_LAUNCH_CHECK();
    }
    if constexpr (kGather)
        return ns_src_launch<false>(ns_src_args(x, a, gy, slope, cap_dst, H, C, g_ft, g_el),
                                    stream);
    return REGNN_OK;
}

}  // namespace
}  // namespace regnn

using namespace regnn;

extern "C" int regnn_ns_gat_fwd(const int32_t* ptr, const int32_t* idx, const uint8_t* rel,
                                const float* el, const float* er, const float* tab,
                                const float* ft, float slope, int64_t cap_dst, int64_t n_src,
                                int32_t H, int32_t C, float* a, float* out, float* work,
                                hipStream_t stream) {
    if (!ptr || !idx || !el || !er || !ft || !a || !out || !work || (tab && !rel) ||
        cap_dst < 0 || n_src < 0)
        return REGNN_EINVAL;
    if (const int rc = ns_gat_shape_rc(H, C)) return rc;
    if (cap_dst == 0) return REGNN_OK;
    const int grid = ns_gat_grid(cap_dst);
    hipLaunchKernelGGL(ns_gat_score_kernel, dim3(grid), dim3(kBlock), 0, stream, ptr, idx, rel,
                       el, er, tab, slope, cap_dst, n_src, int(H), a, work);
    REGNN_LAUNCH_CHECK();
    hipLaunchKernelGGL(ns_gat_fwd_kernel, dim3(grid), dim3(kBlock), 0, stream, ptr, idx, ft,
                       static_cast<const float*>(work), grid, cap_dst, n_src, int(H), int(C), a,
                       out);
    REGNN_LAUNCH_CHECK();
    return REGNN_OK;
}

extern "C" int regnn_ns_gat_bwd(const int32_t* ptr, const int32_t* idx, const uint8_t* rel,
                                const float* el, const float* er, const float* tab,
                                const float* ft, const float* a, const float* gy, float slope,
                                int64_t cap_dst, int64_t n_src, int32_t H, int32_t C,
                                int32_t n_rel, float* g_ft, float* g_el, float* g_er, float* slab,
                                int32_t slab_rows, hipStream_t stream) {
    return gat_bwd<false>(ptr, idx, rel, el, er, tab, ft, a, gy, slope, cap_dst, n_src, H, C,
                          n_rel, g_ft, g_el, g_er, slab, slab_rows, SrcIdx{}, stream);
}

extern "C" int64_t regnn_ns_gat_src_work_floats(int64_t cap_e, int32_t HC) {
    return cap_e < 0 || HC < 0 ? 0 : ns_src_work_floats(cap_e, HC);
}

extern "C" int regnn_ns_gat_bwd_gather(
    const int32_t* ptr, const int32_t* idx, const uint8_t* rel, const float* el, const float* er,
    const float* tab, const float* ft, const float* a, const float* gy, float slope,
    int64_t cap_dst, int64_t n_src, int32_t H, int32_t C, int32_t n_rel, float* g_ft, float* g_el,
    float* g_er, float* slab, int32_t slab_rows, const int32_t* t_ptr, const int32_t* t_pos,
    const int32_t* t_row, const int32_t* t_long, int64_t cap_src, int64_t n_out, int64_t cap_e,
    float* ent, float* piece_work, int64_t piece_work_floats, hipStream_t stream) {
    const SrcIdx x{t_ptr, t_pos, t_row, t_long, cap_src, n_out, cap_e, ent, piece_work,
                   piece_work_floats};
    return gat_bwd<true>(ptr, idx, rel, el, er, tab, ft, a, gy, slope, cap_dst, n_src, H, C, n_rel,
                         g_ft, g_el, g_er, slab, slab_rows, x, stream);
}
