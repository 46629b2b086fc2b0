// The source pass of the gather form of the two sampled-block attention backwards
// (regnn_ns_gat_bwd_gather, regnn_ns_gatv2_bwd_gather): per source row u, a walk over its slots of
// the block's canonical transposed index (regnn_ns_block_tidx: CSR positions ascending), the sum in
// the lanes' registers, every row u < n_out written once by 16-byte stores -- exact zeros for a
// row without slots. No atomics: the same bits on every run.
//
//   GAT    g_ft[u,h,:] = sum a[e,h] gy[v,h,:]          g_el[u,h] = sum gl[e,h]
//   GATv2  g_xs[u,h,d] = sum ( a[e,h] gy[v,h,d] + gs[e,h] att[h,d] (xs[u,h,d] + xd[v,h,d] > 0 ?
//                              1 : slope) )            (xs[u] and att in registers for the row)
// gl / gs [cap_e, H] are the row pass's per-entry scratch (`ent`).
//
//   ns_src_rows_kernel<G, V2>   segments of <= REGNN_NS_TIDX_CHUNK slots: G lanes per source (a
//                               16-byte vector each; rows wider than G vectors take several
//                               passes over the segment), 64 / G sources per wave; the group
//                               fetches G slots' ids at once, 8 slots' rows are in flight
//   ns_src_piece_kernel<V2>     a wave per piece of a long segment, into the piece workspace
//   ns_src_sum_kernel<V2>       a wave per long row: its pieces added in piece order
#pragma once
#include "re_nsgat_common.h"

namespace regnn {
namespace {

constexpr int kSrcPad = kMaxHeads;          // a piece's workspace row: H * C floats, then g_el's

struct SrcArgs {
    const int32_t* t_ptr;
    const int32_t* t_pos;
    const int32_t* t_row;
    const int32_t* t_long;
    const float* a;       // [cap_e, H]
    const float* ent;     // [cap_e, H]: gl (GAT) or gs (GATv2)
    const float* gy;      // [cap_dst, H, C]
    const float* xs;      // GATv2: [>= n_out, H, C]
    const float* xd;      // GATv2: [cap_dst, H, C]
    const float* att;     // GATv2: [H, C]
    float slope;
    int64_t cap_src, n_out, cap_dst;
    int cap_e, max_pieces, H, C;
    float* g_main;        // g_ft / g_xs [n_out, H, C]
    float* g_el;          // GAT: [n_out, H]
    float* work;          // [max_pieces, H * C + kSrcPad]
};

struct SrcSlot {
    int e, v;
    bool ok;
};

// slot s of the index: the entry and its row, refused (weight 0) where either leaves the block
__device__ __forceinline__ SrcSlot src_slot(const SrcArgs& p, int s) {
    SrcSlot t;
    t.e = p.t_pos[s];
    t.v = p.t_row[s];
    t.ok = t.e >= 0 && t.e < p.cap_e && t.v >= 0 && int64_t(t.v) < p.cap_dst;
    if (!t.ok) t.e = t.v = 0;
    return t;
}

template <bool V2>
__device__ __forceinline__ void src_add(const SrcArgs& p, float wa, float ws, const float4& g,
                                        const float4& d, const float4& x, const float4& w,
                                        float4& acc) {
    if constexpr (V2) {
        const float p0 = x.x + d.x, p1 = x.y + d.y, p2 = x.z + d.z, p3 = x.w + d.w;
        acc.x += fmaf(wa, g.x, ws * w.x * (p0 > 0.f ? 1.f : p.slope));
        acc.y += fmaf(wa, g.y, ws * w.y * (p1 > 0.f ? 1.f : p.slope));
        acc.z += fmaf(wa, g.z, ws * w.z * (p2 > 0.f ? 1.f : p.slope));
        acc.w += fmaf(wa, g.w, ws * w.w * (p3 > 0.f ? 1.f : p.slope));
    } else {
        acc.x = fmaf(wa, g.x, acc.x);
        acc.y = fmaf(wa, g.y, acc.y);
        acc.z = fmaf(wa, g.z, acc.z);
        acc.w = fmaf(wa, g.w, acc.w);
    }
}

// the slots [s0, s1) of source u by the G lanes of a group (gl = the lane in the group), in slot
// order: the group's lanes fetch G slots' ids at once (one coalesced load) and hand them round
// by shuffles, the gathered rows of kSrcFlight slots are in flight at a time; orow [H * C] and
// (GAT) elrow [H] are written once. Every lane of the group runs every iteration (the shuffles
// need them all): a lane past the row's last vector only skips its store.
constexpr int kSrcFlight = 8;

template <bool V2>
__device__ __forceinline__ void src_accumulate(const SrcArgs& p, int64_t u, int s0, int s1, int gl,
                                               int G, float* __restrict__ orow,
                                               float* __restrict__ elrow) {
    const int H = p.H, C = p.C, HC = H * C, nvec = HC >> 2;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    const int npass = (nvec + G - 1) / G;
    for (int pass = 0; pass < npass; ++pass) {
        const bool active = pass * G + gl < nvec;
        const int c4 = active ? pass * G + gl : 0;
        const int h = (4 * c4) / C;
        const bool with_el = !V2 && pass == 0 && gl < H;   // (G >= H C / 4 >= H, or G = 64 >= 16)
        float4 x = zero, w = zero;
        if constexpr (V2) {
            x = *reinterpret_cast<const float4*>(p.xs + u * HC + 4 * c4);
            w = *reinterpret_cast<const float4*>(p.att + 4 * c4);
        }
        float4 acc = zero;
        float gel = 0.f;
        for (int sb = s0; sb < s1; sb += G) {
            const int m = min(G, s1 - sb);
            int me = 0, mv = -1;                   // this lane's slot of the G: row -1 = none
            if (gl < m) {
                const SrcSlot t = src_slot(p, sb + gl);
                me = t.e;
                mv = t.ok ? t.v : -1;
            }
            for (int j0 = 0; j0 < m; j0 += kSrcFlight) {
                int e[kSrcFlight], v[kSrcFlight];
                float wa[kSrcFlight], ws[kSrcFlight], ge[kSrcFlight];
                float4 g[kSrcFlight], d[kSrcFlight];
#pragma unroll
                for (int k = 0; k < kSrcFlight; ++k) {
                    const int j = j0 + k < m ? j0 + k : 0;
                    e[k] = __shfl(me, j, G);
                    v[k] = __shfl(mv, j, G);
                    if (j0 + k >= m) v[k] = -1;
                }
#pragma unroll
                for (int k = 0; k < kSrcFlight; ++k) {
                    const bool ok = v[k] >= 0;
                    const int64_t ee = ok ? e[k] : 0, vv = ok ? v[k] : 0;
                    wa[k] = p.a[ee * H + h];
                    ws[k] = V2 ? p.ent[ee * H + h] : 0.f;
                    ge[k] = with_el ? p.ent[ee * H + gl] : 0.f;
                    g[k] = *reinterpret_cast<const float4*>(p.gy + vv * HC + 4 * c4);
                    d[k] = V2 ? *reinterpret_cast<const float4*>(p.xd + vv * HC + 4 * c4) : zero;
                }
#pragma unroll
                for (int k = 0; k < kSrcFlight; ++k) {
                    if (v[k] < 0) continue;
                    src_add<V2>(p, wa[k], ws[k], g[k], d[k], x, w, acc);
                    gel += ge[k];
                }
            }
        }
        if (active) *reinterpret_cast<float4*>(orow + 4 * c4) = acc;
        if (with_el) elrow[gl] = gel;
    }
}

// u's segment, clamped to the entry capacity; empty past the index's rows
__device__ __forceinline__ void src_segment(const SrcArgs& p, int64_t u, int& s0, int& s1) {
    s0 = s1 = 0;
    if (u < p.cap_src) {
        s0 = max(0, min(p.t_ptr[u], p.cap_e));
        s1 = max(s0, min(p.t_ptr[u + 1], p.cap_e));
    }
}

template <int G, bool V2>
__global__ void __launch_bounds__(kBlock)
ns_src_rows_kernel(SrcArgs p) {
    constexpr int S = 64 / G;                      // sources per wave
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int grp = lane / G, gl = lane % G;
    const int HC = p.H * p.C;
    for (int64_t base = (int64_t(blockIdx.x) * kWaves + wave) * S; base < p.n_out;
         base += int64_t(gridDim.x) * kWaves * S) {
        const int64_t u = base + grp;
        if (u >= p.n_out) continue;
        int s0, s1;
        src_segment(p, u, s0, s1);
        if (s1 - s0 > REGNN_NS_TIDX_CHUNK) continue;       // a long row: the pieces' launches
        src_accumulate<V2>(p, u, s0, s1, gl, G, p.g_main + u * HC, V2 ? nullptr : p.g_el + u * p.H);
    }
}

__device__ __forceinline__ int src_n_pieces(const SrcArgs& p) {
    return max(0, min(p.t_long[0], p.max_pieces));
}

template <bool V2>
__global__ void __launch_bounds__(kBlock)
ns_src_piece_kernel(SrcArgs p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = src_n_pieces(p);
    const int64_t stride = int64_t(p.H) * p.C + kSrcPad;
    for (int i = blockIdx.x * kWaves + wave; i < n; i += gridDim.x * kWaves) {
        const int32_t* q = p.t_long + 4 + 4 * i;
        const int64_t u = q[0];
        const int s0 = max(0, min(q[1], p.cap_e));
        const int s1 = max(s0, min(q[1] + min(q[2], REGNN_NS_TIDX_CHUNK), p.cap_e));
        if (u < 0 || u >= p.n_out) continue;
        float* row = p.work + i * stride;
        src_accumulate<V2>(p, u, s0, s1, lane, 64, row, row + int64_t(p.H) * p.C);
    }
}

template <bool V2>
__global__ void __launch_bounds__(kBlock)
ns_src_sum_kernel(SrcArgs p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = src_n_pieces(p);
    const int HC = p.H * p.C, nvec = HC >> 2;
    const int64_t stride = int64_t(HC) + kSrcPad;
    for (int i = blockIdx.x * kWaves + wave; i < n; i += gridDim.x * kWaves) {
        const int32_t* q = p.t_long + 4 + 4 * i;
        if (q[3] >> 16) continue;                          // the row's first piece leads
        const int64_t u = q[0];
        const int k = min(q[3] & 0xffff, n - i);
        if (u < 0 || u >= p.n_out) continue;
        const float* row = p.work + i * stride;
        for (int c4 = lane; c4 < nvec; c4 += 64) {
            float4 acc = *reinterpret_cast<const float4*>(row + 4 * c4);
            for (int j = 1; j < k; ++j) {                  // in piece order
                const float4 t = *reinterpret_cast<const float4*>(row + j * stride + 4 * c4);
                acc.x += t.x;
                acc.y += t.y;
                acc.z += t.z;
                acc.w += t.w;
            }
            *reinterpret_cast<float4*>(p.g_main + u * HC + 4 * c4) = acc;
        }
        if constexpr (!V2) {
            if (lane < p.H) {
                float t = row[HC + lane];
                for (int j = 1; j < k; ++j) t += row[j * stride + HC + lane];
                p.g_el[u * p.H + lane] = t;
            }
        }
    }
}

inline int64_t ns_src_max_pieces(int64_t cap_e) {          // regnn_ns_tidx_long_ints' bound
    return 2 * (cap_e / REGNN_NS_TIDX_CHUNK) + 2;
}

inline int64_t ns_src_work_floats(int64_t cap_e, int64_t HC) {
    return ns_src_max_pieces(cap_e) * (HC + kSrcPad);
}

// The gather forms' own arguments, in the entry points' order (regnn_hip.h). invalid(): a NULL or
// negative one, REGNN_EINVAL with the operator's own invalid arguments. over(): a capacity beyond
// the int32 slots or a piece workspace below the query's value, REGNN_EUNSUPPORTED after the
// operator's shape gate and budgets.
struct SrcIdx {
    const int32_t *t_ptr, *t_pos, *t_row, *t_long;
    int64_t cap_src, n_out, cap_e;
    float *ent, *piece_work;
    int64_t piece_work_floats;
    bool invalid() const {
        return !t_ptr || !t_pos || !t_row || !t_long || !ent || !piece_work || cap_src < 0 ||
               n_out < 0 || cap_e < 0 || piece_work_floats < 0;
    }
    bool over(int64_t cap_dst, int64_t HC) const {
        return cap_e > 0x7ffffffe || cap_src > 0x7ffffffe || cap_dst > 0x7ffffffe ||
               piece_work_floats < ns_src_work_floats(cap_e, HC);
    }
};

// what both operators' source passes read and write; GATv2 adds xs, xd, att and has no g_el
inline SrcArgs ns_src_args(const SrcIdx& x, const float* a, const float* gy, float slope,
                           int64_t cap_dst, int H, int C, float* g_main, float* g_el) {
    SrcArgs p{};
    p.t_ptr = x.t_ptr, p.t_pos = x.t_pos, p.t_row = x.t_row, p.t_long = x.t_long;
    p.a = a, p.ent = x.ent, p.gy = gy, p.slope = slope;
    p.cap_src = x.cap_src, p.n_out = x.n_out, p.cap_dst = cap_dst, p.cap_e = int(x.cap_e);
    p.max_pieces = int(ns_src_max_pieces(x.cap_e)), p.H = H, p.C = C;
    p.g_main = g_main, p.g_el = g_el, p.work = x.piece_work;
    return p;
}

// the three launches of the source pass
template <bool V2>
inline int ns_src_launch(const SrcArgs& p, hipStream_t stream) {
    if (p.n_out == 0) return REGNN_OK;
    const int nvec = (p.H * p.C) >> 2;
#define REGNN_NS_SRC_ROWS(G)                                                                     \
    hipLaunchKernelGGL((ns_src_rows_kernel<G, V2>),                                              \
                       dim3(grid_for(p.n_out, kWaves * (64 / G))), dim3(kBlock), 0, stream, p)
    if (nvec <= 2) REGNN_NS_SRC_ROWS(2);
    else if (nvec <= 4) REGNN_NS_SRC_ROWS(4);
    else if (nvec <= 8) REGNN_NS_SRC_ROWS(8);
    else if (nvec <= 16) REGNN_NS_SRC_ROWS(16);
    else if (nvec <= 32) REGNN_NS_SRC_ROWS(32);
    else REGNN_NS_SRC_ROWS(64);
#undef REGNN_NS_SRC_ROWS
    REGNN_LAUNCH_CHECK();
    const int pg = grid_for(p.max_pieces, kWaves);
    hipLaunchKernelGGL((ns_src_piece_kernel<V2>), dim3(pg), dim3(kBlock), 0, stream, p);
    REGNN_LAUNCH_CHECK();
    hipLaunchKernelGGL((ns_src_sum_kernel<V2>), dim3(pg), dim3(kBlock), 0, stream, p);
    REGNN_LAUNCH_CHECK();
    return REGNN_OK;
}

}  // namespace
}  // namespace regnn
