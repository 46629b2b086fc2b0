// mag REGATv2Conv attention over one device-sampled block as the sampler leaves it (regnn_ns_hop's
// capacity-sized CSR, see re_nsgat.hip): mag/regnn_layers.py:399-413 with the softmax of
// mag/utils.py:45-57 (ONE maximum over every live entry and head, + 1e-16 in the denominator).
// xs is both the score operand and the message (lin_dst is lin_src, propagate sends x_src).
//
//   launch 1  ns_gatv2_score_kernel  s[e,h] = sum_d att[h,d] LeakyReLU(xs[u,h,d] + xd[v,h,d])
//                                    + tab[rel_e,h] into the `a` buffer: a lane per (entry, head),
//                                    d ascending in ONE fmaf chain from 0, the relation term added
//                                    last; one maximum per workgroup
//   launch 2  ns_gatv2_fwd_kernel    re_nsgat_common.h's softmax and aggregation (as ns_gat's)
//   backward  ns_gatv2_bwd_kernel    ga, D, gs per row as ns_gat's; then a lane per column of the
//                                    row: pre recomputed, g_xd and the workgroup's g_att partial
//                                    in entry order in registers, the relation bins by lane h, and
//                                    ONE float atomic per element per entry into g_xs (message
//                                    and score terms folded; form (b), regnn_hip.h)
//   or        ns_gatv2_bwd_rows_kernel  the same row pass without the atomic, gs per entry kept,
//             + re_nsgat_src.h       then g_xs by a gather over the block's transposed index
//                                    (form (a), regnn_ns_gatv2_bwd_gather): no atomics
#include "re_nsgat_common.h"
#include "re_nsgat_src.h"

namespace regnn {
namespace {

constexpr int kMaxWidth = 2048;             // H * C: <= 32 columns per lane, in registers

__global__ void __launch_bounds__(kBlock)
ns_gatv2_score_kernel(const int32_t* __restrict__ ptr, const int32_t* __restrict__ idx,
                      const uint8_t* __restrict__ rel, const float* __restrict__ xs,
                      const float* __restrict__ xd, const float* __restrict__ att,
                      const float* __restrict__ tab, float slope, int64_t n_rows, int64_t n_src,
                      int H, int C, float* __restrict__ s, float* __restrict__ wgmax) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int HC = H * C, nv = C >> 2;
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
                const float4* xp = reinterpret_cast<const float4*>(xs + int64_t(u) * HC + h * C);
                const float4* dp = reinterpret_cast<const float4*>(xd + v * HC + h * C);
                const float4* ap = reinterpret_cast<const float4*>(att + h * C);
                x = 0.f;
                for (int c = 0; c < nv; ++c) {
                    const float4 p = xp[c], q = dp[c], w = ap[c];
                    const float p0 = p.x + q.x, p1 = p.y + q.y, p2 = p.z + q.z, p3 = p.w + q.w;
                    x = fmaf(w.x, p0 > 0.f ? p0 : p0 * slope, x);
                    x = fmaf(w.y, p1 > 0.f ? p1 : p1 * slope, x);
                    x = fmaf(w.z, p2 > 0.f ? p2 : p2 * slope, x);
                    x = fmaf(w.w, p3 > 0.f ? p3 : p3 * slope, x);
                }
                if (tab) x += tab[int(rel[e]) * H + h];
                m = fmaxf(m, x);
            }
            s[int64_t(e) * H + h] = x;
        }
    }
    store_wg_max(m, wgmax);
}

__global__ void __launch_bounds__(kBlock)
ns_gatv2_fwd_kernel(const int32_t* __restrict__ ptr, const int32_t* __restrict__ idx,
                    const float* __restrict__ xs, const float* __restrict__ wgmax, int n_wg,
                    int64_t n_rows, int64_t n_src, int H, int C, float* __restrict__ a,
                    float* __restrict__ out) {
    ns_softmax_aggregate(ptr, idx, xs, wgmax, n_wg, n_rows, n_src, H, C, a, out);
}

// One wave per row, T = the columns per lane (column lane + 64 t of the row's H*C, t < T).
// Pass 1 over the row's chunks: ga[e,h] = <gy[v,h,:], xs[u,h,:]> (a lane per (entry, head),
// columns in order) and D[v,h] = sum a ga in entry order. Pass 2: gs = a (ga - D) into LDS, the
// wave's relation bins by lane h in entry order, then per column: pre = xs[u] + xd[v] again,
// q = gs att LeakyReLU'(pre), g_xd and g_att += in entry order, and the one atomic a gy + q into
// g_xs -- one instruction per 64 consecutive columns of a source row (256 contiguous bytes). A row
// of more than one chunk recomputes ga in pass 2 (the same instructions on the same operands: the
// same bits) and carries its g_xd sums from chunk to chunk through the row it writes (the lane's
// own stores: still one chain in entry order). The chunk fill, pass 1 and the relation bins are
// ns_gat's (NsRow, re_nsgat_common.h); pass 2 is this operator's own.
//
// kGather (regnn_ns_gatv2_bwd_gather's row pass): this one body with the atomic compiled out --
// gs[e,h] goes to the per-entry scratch `ent` (0 for an entry that takes no part) and g_xs is left
// to the source pass (re_nsgat_src.h).
template <int T, bool kGather>
__device__ __forceinline__ void
ns_gatv2_bwd_body(const int32_t* __restrict__ ptr, const int32_t* __restrict__ idx,
                  const uint8_t* __restrict__ rel, const float* __restrict__ xs,
                  const float* __restrict__ xd, const float* __restrict__ att,
                  const float* __restrict__ tab, const float* __restrict__ a,
                  const float* __restrict__ gy, float slope, int64_t n_rows, int64_t n_src,
                  int H, int C, int n_rel, float* __restrict__ g_xs, float* __restrict__ g_xd,
                  float* __restrict__ att_slab, float* __restrict__ tab_slab,
                  float* __restrict__ ent) {
    extern __shared__ float dyn_[];            // [kWaves][n_rel * H] when tab_slab, then [H * C]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const NsRow s = ns_row(idx, rel, tab != nullptr, xs, a, n_src, H, C);
    const int W = tab_slab ? n_rel * H : 0;
    float* bins = dyn_ + wave * W;
    float* attred = dyn_ + kWaves * W;
    if (tab_slab) ns_bins_zero(dyn_, W);
    const int HC = H * C;
    float gatt[T];
#pragma unroll
    for (int t = 0; t < T; ++t) gatt[t] = 0.f;
    for (int64_t v = int64_t(blockIdx.x) * kWaves + wave; v < n_rows;
         v += int64_t(gridDim.x) * kWaves) {
        const int e0 = ptr[v], e1 = ptr[v + 1];
        float* gxdr = g_xd + v * HC;
        if (e1 <= e0) {
            for (int c = lane; c < (HC >> 2); c += 64)
                *reinterpret_cast<float4*>(gxdr + 4 * c) = make_float4(0.f, 0.f, 0.f, 0.f);
            continue;
        }
        const float* gyr = gy + v * HC;
        const float* xdr = xd + v * HC;
        const bool one = s.pass1(gyr, e0, e1);
        for (int cb = e0; cb < e1; cb += kChunk) {
            const int nc = min(kChunk, e1 - cb);
            if (!one) s.fill(gyr, cb, nc);
            else wave_lds_sync();              // sD written
            for (int i = lane; i < nc * H; i += 64) {
                const int hh = i % H;
                s.sg[i] = s.sa[i] * (s.sg[i] - s.sD[hh]);  // gs (the lane's own slot; 0 where a is)
                if constexpr (kGather) ent[int64_t(cb) * H + i] = s.sg[i];
            }
            wave_lds_sync();
            if (tab_slab && lane < H) {
                for (int j = 0; j < nc; ++j) {
                    const int r = s.sr[j];
                    if (s.su[j] >= 0 && r < n_rel) bins[r * H + lane] += s.sg[j * H + lane];
                }
            }
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const int col = lane + 64 * t;
                if (col >= HC) continue;
                const int h = col / C;
                const float g = gyr[col], dv = xdr[col], w = att[col];
                float gd = cb == e0 ? 0.f : gxdr[col];
                float ga = gatt[t];
                for (int j = 0; j < nc; ++j) {
                    const int u = s.su[j];
                    if (u < 0) continue;
                    [[maybe_unused]] float* dst = g_xs + int64_t(u) * HC + col;
                    const float pre = xs[int64_t(u) * HC + col] + dv;
                    const float gs = s.sg[j * H + h];
                    const float q = gs * w * (pre > 0.f ? 1.f : slope);
                    gd += q;
                    ga = fmaf(gs, pre > 0.f ? pre : pre * slope, ga);
                    if constexpr (!kGather) unsafeAtomicAdd(dst, fmaf(s.sa[j * H + h], g, q));
                }
                gxdr[col] = gd;
                gatt[t] = ga;
            }
        }
    }
    if (tab_slab) ns_bins_store(dyn_, W, tab_slab);
    if (!att_slab) return;
    for (int w = 0; w < kWaves; ++w) {         // the waves' g_att partials in wave order
        if (wave == w) {
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const int col = lane + 64 * t;
                if (col < HC) attred[col] = w ? attred[col] + gatt[t] : gatt[t];
            }
        }
        __syncthreads();
    }
    for (int i = threadIdx.x; i < HC; i += kBlock)
        att_slab[int64_t(blockIdx.x) * HC + i] = attred[i];
}

template <int T>
__global__ void __launch_bounds__(kBlock)
ns_gatv2_bwd_kernel(const int32_t* __restrict__ ptr, const int32_t* __restrict__ idx,
                    const uint8_t* __restrict__ rel, const float* __restrict__ xs,
                    const float* __restrict__ xd, const float* __restrict__ att,
                    const float* __restrict__ tab, const float* __restrict__ a,
                    const float* __restrict__ gy, float slope, int64_t n_rows, int64_t n_src,
                    int H, int C, int n_rel, float* __restrict__ g_xs, float* __restrict__ g_xd,
                    float* __restrict__ att_slab, float* __restrict__ tab_slab) {
    ns_gatv2_bwd_body<T, false>(ptr, idx, rel, xs, xd, att, tab, a, gy, slope, n_rows, n_src, H,
                                C, n_rel, g_xs, g_xd, att_slab, tab_slab, nullptr);
}

template <int T>
__global__ void __launch_bounds__(kBlock)
ns_gatv2_bwd_rows_kernel(const int32_t* __restrict__ ptr, const int32_t* __restrict__ idx,
                         const uint8_t* __restrict__ rel, const float* __restrict__ xs,
                         const float* __restrict__ xd, const float* __restrict__ att,
                         const float* __restrict__ tab, const float* __restrict__ a,
                         const float* __restrict__ gy, float slope, int64_t n_rows,
                         int64_t n_src, int H, int C, int n_rel, float* __restrict__ g_xd,
                         float* __restrict__ att_slab, float* __restrict__ tab_slab,
                         float* __restrict__ ent) {
    ns_gatv2_bwd_body<T, true>(ptr, idx, rel, xs, xd, att, tab, a, gy, slope, n_rows, n_src, H, C,
                               n_rel, nullptr, g_xd, att_slab, tab_slab, ent);
}

inline int ns_gatv2_shape_rc(int32_t H, int32_t C) {
    if (const int rc = ns_gat_shape_rc(H, C)) return rc;
    return H * C > kMaxWidth ? REGNN_EUNSUPPORTED : REGNN_OK;
}

// Both backward entry points, as re_nsgat.hip's gat_bwd: the refusals in one order before any
// launch, the row pass (with a slab exactly slab_rows workgroups, each writes its rows; T by the
// row width), then the gather form's source pass. x is unread in the atomic form.
template <bool kGather>
inline int gatv2_bwd(const int32_t* ptr, const int32_t* idx, const uint8_t* rel, const float* xs,
                     const float* xd, const float* att, const float* tab, const float* a,
                     const float* gy, float slope, int64_t cap_dst, int64_t n_src, int32_t H,
                     int32_t C, int32_t n_rel, float* g_xs, float* g_xd, float* att_slab,
                     float* tab_slab, int32_t slab_rows, const SrcIdx& x, hipStream_t stream) {
    const bool slabs = att_slab || tab_slab;
    if (!ptr || !idx || !xs || !xd || !att || !a || !gy || !g_xs || !g_xd || (tab && !rel) ||
        (tab_slab && !tab) || cap_dst < 0 || n_src < 0 || n_rel < 0 || (tab && n_rel < 1) ||
        (slabs && slab_rows < 1) || (kGather && x.invalid()))
        return REGNN_EINVAL;
    if (const int rc = ns_gatv2_shape_rc(H, C)) return rc;
    if ((tab_slab && int64_t(n_rel) * H > REGNN_NS_GAT_MAX_BINS) ||
        (slabs && slab_rows > REGNN_NS_GAT_WORK_FLOATS))
        return REGNN_EUNSUPPORTED;
    const int HC = H * C;
    if (kGather && x.over(cap_dst, HC)) return REGNN_EUNSUPPORTED;
    if (cap_dst > 0 || slabs) {
        const int grid = slabs ? int(slab_rows) : ns_gat_grid(cap_dst);
        const size_t lds = ((tab_slab ? size_t(kWaves) * n_rel * H : 0) + (att_slab ? HC : 0)) *
                           sizeof(float);
        auto launch = [&](auto rows_kernel, auto bwd_kernel) {
            if constexpr (kGather) {
                hipLaunchKernelGGL(rows_kernel, dim3(grid), dim3(kBlock), lds, stream, ptr, idx,
                                   rel, xs, xd, att, tab, a, gy, slope, cap_dst, n_src, int(H),
                                   int(C), int(n_rel), g_xd, att_slab, tab_slab, x.ent);
            } else {
                hipLaunchKernelGGL(bwd_kernel, dim3(grid), dim3(kBlock), lds, stream, ptr, idx,
                                   rel, xs, xd, att, tab, a, gy, slope, cap_dst, n_src, int(H),
                                   int(C), int(n_rel), g_xs, g_xd, att_slab, tab_slab);
            }
        };
        if (HC <= 64) launch(ns_gatv2_bwd_rows_kernel<1>, ns_gatv2_bwd_kernel<1>);
        else if (HC <= 128) launch(ns_gatv2_bwd_rows_kernel<2>, ns_gatv2_bwd_kernel<2>);
        else if (HC <= 256) launch(ns_gatv2_bwd_rows_kernel<4>, ns_gatv2_bwd_kernel<4>);
        else if (HC <= 512) launch(ns_gatv2_bwd_rows_kernel<8>, ns_gatv2_bwd_kernel<8>);
        else if (HC <= 1024) launch(ns_gatv2_bwd_rows_kernel<16>, ns_gatv2_bwd_kernel<16>);
        else launch(ns_gatv2_bwd_rows_kernel<32>, ns_gatv2_bwd_kernel<32>);
        REGNN_LAUNCH_CHECK();
    }
    if constexpr (kGather) {
        SrcArgs p = ns_src_args(x, a, gy, slope, cap_dst, H, C, g_xs, nullptr);
        p.xs = xs, p.xd = xd, p.att = att;
        return ns_src_launch<true>(p, stream);
    }
    return REGNN_OK;
}

}  // namespace
}  // namespace regnn

using namespace regnn;

extern "C" int regnn_ns_gatv2_fwd(const int32_t* ptr, const int32_t* idx, const uint8_t* rel,
                                  const float* xs, const float* xd, const float* att,
                                  const float* tab, float slope, int64_t cap_dst, int64_t n_src,
                                  int32_t H, int32_t C, float* a, float* out, float* work,
                                  hipStream_t stream) {
    if (!ptr || !idx || !xs || !xd || !att || !a || !out || !work || (tab && !rel) ||
        cap_dst < 0 || n_src < 0)
        return REGNN_EINVAL;
    if (const int rc = ns_gatv2_shape_rc(H, C)) return rc;
    if (cap_dst == 0) return REGNN_OK;
    const int grid = ns_gat_grid(cap_dst);
    hipLaunchKernelGGL(ns_gatv2_score_kernel, dim3(grid), dim3(kBlock), 0, stream, ptr, idx, rel,
                       xs, xd, att, tab, slope, cap_dst, n_src, int(H), int(C), a, work);
    REGNN_LAUNCH_CHECK();
    hipLaunchKernelGGL(ns_gatv2_fwd_kernel, dim3(grid), dim3(kBlock), 0, stream, ptr, idx, xs,
                       static_cast<const float*>(work), grid, cap_dst, n_src, int(H), int(C), a,
                       out);
    REGNN_LAUNCH_CHECK();
    return REGNN_OK;
}

extern "C" int regnn_ns_gatv2_bwd(const int32_t* ptr, const int32_t* idx, const uint8_t* rel,
                                  const float* xs, const float* xd, const float* att,
                                  const float* tab, const float* a, const float* gy, float slope,
                                  int64_t cap_dst, int64_t n_src, int32_t H, int32_t C,
                                  int32_t n_rel, float* g_xs, float* g_xd, float* att_slab,
                                  float* tab_slab, int32_t slab_rows, hipStream_t stream) {
    return gatv2_bwd<false>(ptr, idx, rel, xs, xd, att, tab, a, gy, slope, cap_dst, n_src, H, C,
                            n_rel, g_xs, g_xd, att_slab, tab_slab, slab_rows, SrcIdx{}, stream);
}

extern "C" int regnn_ns_gatv2_bwd_gather(
    const int32_t* ptr, const int32_t* idx, const uint8_t* rel, const float* xs, const float* xd,
    const float* att, const float* tab, const float* a, const float* gy, float slope,
    int64_t cap_dst, int64_t n_src, int32_t H, int32_t C, int32_t n_rel, float* g_xs, float* g_xd,
    float* att_slab, float* tab_slab, int32_t slab_rows, const int32_t* t_ptr,
    const int32_t* t_pos, const int32_t* t_row, const int32_t* t_long, int64_t cap_src,
    int64_t n_out, int64_t cap_e, float* ent, float* piece_work, int64_t piece_work_floats,
    hipStream_t stream) {
    const SrcIdx x{t_ptr, t_pos, t_row, t_long, cap_src, n_out, cap_e, ent, piece_work,
                   piece_work_floats};
    return gatv2_bwd<true>(ptr, idx, rel, xs, xd, att, tab, a, gy, slope, cap_dst, n_src, H, C,
                           n_rel, g_xs, g_xd, att_slab, tab_slab, slab_rows, x, stream);
}
