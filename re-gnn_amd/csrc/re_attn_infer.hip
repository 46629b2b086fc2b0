// Forward-only attention for the layer-wise full-neighbour inference of the ogbn-mag REGAT /
// REGATv2 models (mag/regnn_ns.py:348-369, mag/regnn_layers.py:253-325, 394-436):
//  * regnn_mag_attn_fwd: score + online softmax + per-head aggregation over a CSR in one pass
//    (gat_fused_fwd_kernel, re_gat_fused.h, in its INF forms): per (row, head) the unnormalised
//    accumulator acc = sum_e exp(s_e - m) x[u], the row's running maximum m and S = sum_e
//    exp(s_e - m). No [E, H] tensor is written; GATv2 forms its score from the gathered row it
//    aggregates, so an edge makes one random access. Hub rows take the long-segment plan exactly
//    as regnn_gat_fused_fwd does (chunk partial rows [acc | max | sum], seg_tree_level<1>), then
//    seg_emit_online writes the combined row as it is.
//  * regnn_mag_attn_epilogue: the ogbn-mag softmax (mag/utils.py:45-57: ONE maximum gmax over
//    every entry and head, + eps in the denominator) from the per-row quantities,
//        a_e = exp(s_e - gmax) / (sum exp(s_e' - gmax) + eps) = exp(s_e - m) / (S + eps exp(gmax - m)),
//    then bias, residual, LayerNorm and relu, one launch over the rows.
#include "regnn_common.h"
#include "re_segplan.h"
#include "re_gat_fused.h"

namespace regnn {

// acc / rmax / rsum of long segment l = its combined online-softmax row, unchanged
__global__ void __launch_bounds__(kBlock)
seg_emit_online(const float* __restrict__ part, const int32_t* __restrict__ chunk_off,
                int64_t base, int n_levels, const int32_t* __restrict__ long_ids, int n_long,
                int F, int H, float* __restrict__ acc, float* __restrict__ rmax,
                float* __restrict__ rsum) {
    const int W = F + 2 * H;
    for (int l = blockIdx.x; l < n_long; l += gridDim.x) {
        const float* __restrict__ pr = part + final_row(chunk_off, base, n_levels, l) * W;
        const int64_t row = long_ids[l];
        for (int f = threadIdx.x; f < F; f += kBlock) acc[row * F + f] = pr[f];
        for (int h = threadIdx.x; h < H; h += kBlock) {
            rmax[row * H + h] = pr[F + h];
            rsum[row * H + h] = pr[F + H + h];
        }
    }
}

// lane tiers of gat_fused_fwd_kernel: F / 4 vectors over LPR lanes x NV vectors; the ELX and
// GATv2 scores reduce over a head's D / 4 lanes, which must lie within one vector slot (<= LPR)
template <int SC>
int dispatch_attn_infer(GatFusedArgs p, const regnn_seg_plan* pl, hipStream_t stream) {
    const int F = p.H * p.D;
    const int nvec = F / 4, dl = p.D / 4;
    const LongPlan P = long_plan(pl);
#define REGNN_ATTN_INF(LPR, NV)                                                                \
    if (nvec <= (LPR) * (NV) && (SC == kScoreEl || dl <= (LPR))) {                             \
        hipLaunchKernelGGL((gat_fused_fwd_kernel<float, LPR, NV, false, SC, true>),            \
                           dim3(grid_for(p.n_seg, kBlock / (LPR))), dim3(kBlock), 0, stream,   \
                           p, P);                                                              \
        REGNN_LAUNCH_CHECK();                                                                  \
        if (P.n_chunk > 0) {                                                                   \
            hipLaunchKernelGGL((gat_fused_fwd_kernel<float, LPR, NV, true, SC, true>),         \
                               dim3(grid_for(P.n_chunk, kBlock / (LPR))), dim3(kBlock), 0,     \
                               stream, p, P);                                                  \
            const int64_t base = run_tree(pl, 1, F + 2 * p.H, F, p.H, p.D, stream);            \
            hipLaunchKernelGGL(seg_emit_online, dim3(long_grid(P.n_long)), dim3(kBlock), 0,    \
                               stream, P.part, P.chunk_off, base, pl->n_levels, P.long_ids,    \
                               P.n_long, F, p.H, static_cast<float*>(p.out), p.rmax, p.rsum);  \
            REGNN_LAUNCH_CHECK();                                                              \
        }                                                                                      \
        return REGNN_OK;                                                                       \
    }
    REGNN_ATTN_INF(16, 1)
    REGNN_ATTN_INF(16, 2)
    REGNN_ATTN_INF(16, 4)
    REGNN_ATTN_INF(64, 2)
    REGNN_ATTN_INF(64, 4)
    REGNN_ATTN_INF(64, 8)
#undef REGNN_ATTN_INF
    return REGNN_EUNSUPPORTED;
}

// One wave per row. The lanes first form 1 / (S + eps exp(gmax - m)) per head (fp64: the
// exponent reaches hundreds where a row lies far below the global maximum, and the quotient is
// still above the fp32 denormals there) into the wave's LDS slice, then stride over the row:
// v = acc * inv + bias + res into y and the row sum; LayerNorm re-reads the lane's own y.
__global__ void __launch_bounds__(kBlock)
mag_attn_epilogue_kernel(const float* __restrict__ acc, const float* __restrict__ rmax,
                         const float* __restrict__ rsum, const float* __restrict__ gmax,
                         float eps, const float* __restrict__ bias,
                         const float* __restrict__ res, const float* __restrict__ lw,
                         const float* __restrict__ lb, float ln_eps, int flags, int64_t n,
                         int H, int D, float* __restrict__ y) {
    extern __shared__ float inv_s[];             // [waves][H]
    constexpr int WPB = kBlock / 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int F = H * D;
    float* __restrict__ inv = inv_s + wave * H;
    const double gm = double(*gmax);
    // (the trip count is the block's, so the barriers are uniform)
    for (int64_t r0 = (int64_t)blockIdx.x * WPB; r0 < n; r0 += (int64_t)gridDim.x * WPB) {
        const int64_t row = r0 + wave;
        const bool live = row < n;
        if (live) {
            for (int h = lane; h < H; h += 64) {
                const float sv = rsum[row * H + h];
                float w = 0.f;                    // no entries: a zero attention term
                if (sv > 0.f) {
                    const double den = double(sv) + double(eps) * exp(gm - double(rmax[row * H + h]));
                    w = float(1.0 / den);         // den = +inf: 0
                }
                inv[h] = w;
            }
        }
        __syncthreads();
        if (live) {
            float* __restrict__ yr = y + row * F;
            float sum = 0.f;
            for (int f = lane; f < F; f += 64) {
                float v = acc[row * F + f] * inv[f / D];
                if (bias) v += bias[f];
                if (res) v += res[row * F + f];
                if (!(flags & 1) && (flags & 2)) v = fmaxf(v, 0.f);
                yr[f] = v;
                sum += v;
            }
            if (flags & 1) {
                const float mean = group_sum<64>(sum) / float(F);
                float sq = 0.f;
                for (int f = lane; f < F; f += 64) {
                    const float d = yr[f] - mean;
                    sq = fmaf(d, d, sq);
                }
                const float rstd = rsqrtf(group_sum<64>(sq) / float(F) + ln_eps);
                for (int f = lane; f < F; f += 64) {
                    float v = (yr[f] - mean) * rstd;
                    if (lw) v *= lw[f];
                    if (lb) v += lb[f];
                    yr[f] = (flags & 2) ? fmaxf(v, 0.f) : v;
                }
            }
        }
        __syncthreads();
    }
}

}  // namespace regnn

using namespace regnn;

extern "C" {

int regnn_mag_attn_fwd(const int32_t* ptr, const int32_t* idx, const uint8_t* rel,
                       const float* tab, int32_t kind, const float* el, const float* er,
                       const float* att, const float* x, const float* xd, float* acc,
                       float* rmax, float* rsum, int64_t n_seg, int32_t H, int32_t D, float slope,
                       const regnn_seg_plan* plan, hipStream_t stream) {
    if (!ptr || !idx || !x || !acc || !rmax || !rsum || n_seg < 0 || (tab && !rel))
        return REGNN_EINVAL;
    if (kind == REGNN_ATTN_GAT) {
        if (!er || (!el && !att)) return REGNN_EINVAL;
    } else if (kind == REGNN_ATTN_GATV2) {
        if (!att || !xd) return REGNN_EINVAL;
    } else {
        return REGNN_EINVAL;
    }
    if (H <= 0 || D <= 0 || D % 4 || int64_t(H) * D > REGNN_MAG_ATTN_MAX_WIDTH)
        return REGNN_EUNSUPPORTED;
    const bool dots = kind == REGNN_ATTN_GATV2 || !el;    // a D / 4-lane reduction per head
    if (dots && !attn_dots_vec_ok(D)) return REGNN_EUNSUPPORTED;
    if (const int rc = check_plan(plan, int64_t(H) * D + 2 * H)) return rc;
    if (n_seg == 0) return REGNN_OK;
    GatFusedArgs p{ptr, idx, rel, tab, el, er, x, acc, nullptr, att, n_seg, H, D, slope,
                   xd, rmax, rsum};
    if (kind == REGNN_ATTN_GATV2) return dispatch_attn_infer<kScoreV2>(p, plan, stream);
    if (!el) return dispatch_attn_infer<kScoreElx>(p, plan, stream);
    return dispatch_attn_infer<kScoreEl>(p, plan, stream);
}

int regnn_mag_attn_epilogue(const float* acc, const float* rmax, const float* rsum,
                            const float* gmax, float eps, const float* bias, const float* res,
                            const float* ln_weight, const float* ln_bias, float ln_eps,
                            int32_t flags, int64_t n, int32_t H, int32_t D, float* y,
                            hipStream_t stream) {
    if (!acc || !rmax || !rsum || !gmax || !y || n < 0 || (flags & ~3) || !(eps >= 0.f))
        return REGNN_EINVAL;
    if (H <= 0 || D <= 0 || int64_t(H) * D > REGNN_MAG_ATTN_MAX_WIDTH) return REGNN_EUNSUPPORTED;
    if (n == 0) return REGNN_OK;
    hipLaunchKernelGGL(mag_attn_epilogue_kernel, dim3(grid_for(n, kBlock / 64)), dim3(kBlock),
                       size_t(kBlock / 64) * H * sizeof(float), stream, acc, rmax, rsum, gmax,
                       eps, bias, res, ln_weight, ln_bias, ln_eps, flags, n, H, D, y);
    REGNN_LAUNCH_CHECK();
    return REGNN_OK;
}

}  // extern "C"
