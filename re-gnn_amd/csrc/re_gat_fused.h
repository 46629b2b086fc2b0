// The fused score + online softmax + per-head aggregation body shared by regnn_gat_fused_fwd
// (re_gat.hip: training forward, writes out / lse) and regnn_mag_attn_fwd (re_attn_infer.hip:
// forward-only inference, writes the unnormalised accumulator and the row's running max / sum).
#pragma once
#include "regnn_common.h"
#include "re_segplan.h"
#include <type_traits>

namespace regnn {

__device__ __forceinline__ float lrelu(float x, float slope) { return x > 0.f ? x : x * slope; }

// ---- fused score + edge softmax + weighted SpMM (layer/REGATConv.py:80-92) ---------------
// One pass per destination v: for each in-edge u -> v and head h the score
// e = LeakyReLU(el[u,h] + er[v,h] + ee[rel,h]) enters an online softmax (running max m, sum s,
// accumulator rescaled when the max grows) while the same lanes gather x[u,h,:]:
//   out[v,h,:] = sum_e exp(e - m) x[u,h,:] / s,   lse[v,h] = m + log s.
// Every lane of a head carries its own copy of (m, s) (identical: the same scores), so no
// cross-lane reduction is needed; a[e,h] is never written (the backward re-forms it from lse).
// Lanes / vectors as spmm_heads_kernel; edge ids loaded cooperatively, UN rows in flight.
struct GatFusedArgs {
    const int32_t* ptr;
    const int32_t* idx;
    const uint8_t* rel;
    const float* ee;
    const float* el;
    const float* er;
    const void* x;
    void* out;
    float* lse;
    const float* al;    // attn_l [H, D] (ELX kernels: el re-formed from the gathered row)
    int64_t n_seg;
    int H, D;
    float slope;
    // the inference forms (INF, re_attn_infer.hip)
    const float* xd;    // GATv2: the destinations' rows [n_seg, H*D]; al is then att [H, D]
    float* rmax;        // [n_seg, H] running max of the row's scores (-inf: no entries)
    float* rsum;        // [n_seg, H] sum_e exp(s_e - rmax)
};

// regnn_gat_fused_fwd_drop: the attention dropout's seed (device memory), threshold and scale.
// A struct of its own, so the kernel arguments of the undropped instantiations stay as they are.
struct GatFusedDropArgs : GatFusedArgs {
    const uint64_t* dseed;
    uint32_t dthresh;
    float dscale;
};

// Attention dropout (regnn_hip.h, regnn_gat_fused_fwd_drop): the fused-dropout mask of
// regnn_common.h (drop_key / drop_apply, EV = 4) over the [E, Hq] matrix of (CSR edge position,
// head), Hq = max(4, H rounded up to a multiple of 4). Returns the factor of element (e, h):
// scale when kept, 0 when dropped. One hash per (edge, 4-head group), a second for heads 2, 3 of
// the group with 16-bit draws.
__device__ __forceinline__ int attn_drop_nvec(int H) { return H <= 4 ? 1 : (H + 3) >> 2; }

template <int BITS>
__device__ __forceinline__ float attn_drop_w(uint32_t key, uint32_t thresh, float scale, int e,
                                             int nvec, int h) {
    const uint64_t c = uint64_t(e) * uint64_t(nvec) + uint64_t(h >> 2);
    const uint32_t hi = uint32_t(c >> 32);
    uint32_t x = fmix32(uint32_t(c) ^ key ^ ((hi << 16) | (hi >> 16)));
    const int b = h & 3;
    if constexpr (BITS == 16) {
        const uint32_t x1 = fmix32(x + 0x9E3779B9u);
        x = (b & 2) ? x1 : x;
        return ((b & 1) ? x >> 16 : x & 0xFFFFu) < thresh ? scale : 0.f;
    } else {
        return ((x >> (8 * b)) & 0xFFu) < (thresh >> 8) ? scale : 0.f;
    }
}

// how a lane forms the score of an edge
constexpr int kScoreEl = 0;      // el[u,h] read per edge
constexpr int kScoreElx = 1;     // el[u,h] re-formed from the gathered row (head_dot4)
constexpr int kScoreV2 = 2;      // GATv2: <att[h], LeakyReLU(x[u,h] + xd[v,h])> + ee, no outer act

// el[u,h] as attn_dots_fwd_vec forms it: lane l of the head's D/4 lanes takes x[u,h,4l..4l+3]
// (an fmaf chain from 0), then an xor butterfly over the D/4 lanes (every lane ends with the same
// sum). The ELX forward forms it from the row it already holds, so each edge makes one random
// access (the row) instead of two (the row and el[u], 32 B of another array): bitwise the el the
// backward re-forms the attention from.
__device__ __forceinline__ float head_dot4(const float (&v)[4], const float (&a)[4], int dl) {
    float d = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) d = fmaf(v[t], a[t], d);
    for (int o = dl >> 1; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);
    return d;
}

// the GATv2 score's dot over the same lanes: <att[h], LeakyReLU(x[u,h] + xd[v,h])>
__device__ __forceinline__ float head_dot4_v2(const float (&v)[4], const float (&xd)[4],
                                              const float (&a)[4], float slope, int dl) {
    float d = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) d = fmaf(a[t], lrelu(v[t] + xd[t], slope), d);
    for (int o = dl >> 1; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);
    return d;
}

// attn_dots_fwd in the order head_dot4 uses: D % 4 == 0 and D / 4 a power of two <= 64
inline bool attn_dots_vec_ok(int D) {
    const int dl = D / 4;
    return D > 0 && D % 4 == 0 && dl <= 64 && (dl & (dl - 1)) == 0;
}

// CH: the units are the chunks of long segments (partial rows [acc | max | sum], unnormalised);
// otherwise the segments, long ones skipped. SC: the score form (kScore*). INF: the per-segment
// pass writes the unnormalised accumulator with rmax / rsum instead of out / lse.
// DR: attention dropout with DR-bit draws (0: none). The mask factor multiplies only the term an
// edge adds to the accumulator: running max, running sum, lse and the chunk partials' max / sum
// are those of the undropped softmax, so out = sum_e (m_e / keep) a_e x_u with a undropped.
template <typename T, int LPR, int NV, bool CH, int SC, bool INF, int DR = 0>
__global__ void __launch_bounds__(kBlock)
gat_fused_fwd_kernel(std::conditional_t<DR != 0, GatFusedDropArgs, GatFusedArgs> p, LongPlan P) {
    constexpr int EV = Vec<T>::N;
    static_assert(DR == 0 || DR == 8 || DR == 16, "draw width");
    static_assert(DR == 0 || !INF, "dropout: the training forward");
    uint32_t dkey = 0;
    int dnvec = 1;
    if constexpr (DR != 0) {
        dkey = drop_key(p.dseed);
        dnvec = attn_drop_nvec(p.H);
    }
    constexpr bool ELX = SC == kScoreElx, V2 = SC == kScoreV2;
    static_assert(SC == kScoreEl || EV == 4, "ELX / GATv2: fp32 rows");
#ifdef REGNN_GATF_UN
    constexpr int UN = NV <= 2 ? REGNN_GATF_UN : (NV <= 4 ? 4 : 2);
#else
    constexpr int UN = NV <= 4 ? 4 : 2;    // 8 rows for NV <= 2: 25.5 / 18.2 ms against 24.7 / 17.2
#endif
    constexpr int GPB = kBlock / LPR;
    const int tid = threadIdx.x, lane = tid & (LPR - 1);
    const int F = p.H * p.D;
    const T* __restrict__ src = static_cast<const T*>(p.x);
    const int64_t n_units = CH ? P.n_chunk : p.n_seg;
    for (int64_t unit = (int64_t)blockIdx.x * GPB + tid / LPR; unit < n_units;
         unit += (int64_t)gridDim.x * GPB) {
        int64_t seg;
        int beg, end;
        if (CH) {
            chunk_range(P, p.ptr, unit, seg, beg, end);
        } else {
            seg = unit;
            beg = p.ptr[seg];
            end = p.ptr[seg + 1];
            if (end - beg > P.split) continue;         // a long segment: its chunks
        }
        float acc[NV][EV] = {};
        float m[NV], s[NV], erv[NV];
        float alv[ELX || V2 ? NV : 1][4];
        float xdv[V2 ? NV : 1][4];
        int head[NV];
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            const int o = (q * LPR + lane) * EV;
            head[q] = o < F ? o / p.D : 0;
            if constexpr (!V2) erv[q] = p.er[seg * p.H + head[q]];
            m[q] = -INFINITY;
            s[q] = 0.f;
            if constexpr (ELX || V2) {
#pragma unroll
                for (int t = 0; t < 4; ++t) alv[q][t] = o < F ? p.al[o + t] : 0.f;
            }
            if constexpr (V2) {     // the destination's slice, held for the whole row
#pragma unroll
                for (int t = 0; t < 4; ++t) xdv[q][t] = o < F ? p.xd[seg * F + o + t] : 0.f;
            }
        }
        for (int e0 = beg; e0 < end; e0 += LPR) {
            const int e = e0 + lane;
            int j = 0, r = 0;
            if (e < end) {
                j = p.idx[e];
                r = p.ee ? int(p.rel[e]) : 0;
            }
            const int cnt = min(LPR, end - e0);
            for (int k0 = 0; k0 < cnt; k0 += UN) {
                float v[UN][NV][EV];
                float sc[UN][NV];
#pragma unroll
                for (int u = 0; u < UN; ++u) {
                    const int kk = min(k0 + u, cnt - 1);
                    const int jj = __shfl(j, kk, LPR);
                    const int rr = __shfl(r, kk, LPR);
#pragma unroll
                    for (int q = 0; q < NV; ++q) {
                        const int o = (q * LPR + lane) * EV;
                        if (o < F) {
                            Vec<T>::load(src + (int64_t)jj * F + o, v[u][q]);
                            if constexpr (ELX || V2) {  // the relation bias; the dot once the row is in
                                sc[u][q] = p.ee ? p.ee[rr * p.H + head[q]] : 0.f;
                            } else {
                                float z = p.el[(int64_t)jj * p.H + head[q]] + erv[q];
                                if (p.ee) z += p.ee[rr * p.H + head[q]];
                                sc[u][q] = lrelu(z, p.slope);
                            }
                        } else {
#pragma unroll
                            for (int t = 0; t < EV; ++t) v[u][q][t] = 0.f;
                            sc[u][q] = 0.f;
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < UN; ++u) {
                    if (k0 + u >= cnt) break;
                    if constexpr (ELX) {
#pragma unroll
                        for (int q = 0; q < NV; ++q) {
                            float z = head_dot4(v[u][q], alv[q], p.D >> 2) + erv[q];
                            if (p.ee) z += sc[u][q];
                            sc[u][q] = lrelu(z, p.slope);
                        }
                    }
                    if constexpr (V2) {
#pragma unroll
                        for (int q = 0; q < NV; ++q) {
                            const float z = head_dot4_v2(v[u][q], xdv[q], alv[q], p.slope,
                                                         p.D >> 2);
                            sc[u][q] = p.ee ? z + sc[u][q] : z;
                        }
                    }
#pragma unroll
                    for (int q = 0; q < NV; ++q) {
                        const float d = sc[u][q] - m[q];
                        const bool grow = d > 0.f;                   // new running max
                        const float ex = __expf(grow ? -d : d);
                        const float sa = grow ? ex : 1.f, sv = grow ? 1.f : ex;
                        float sw = sv;
                        if constexpr (DR != 0)
                            sw *= attn_drop_w<DR>(dkey, p.dthresh, p.dscale, e0 + k0 + u, dnvec,
                                                  head[q]);
#pragma unroll
                        for (int t = 0; t < EV; ++t) acc[q][t] = fmaf(acc[q][t], sa, sw * v[u][q][t]);
                        s[q] = fmaf(s[q], sa, sv);
                        m[q] = grow ? sc[u][q] : m[q];
                    }
                }
            }
        }
        if (CH) {
            float* __restrict__ pr = P.part + unit * (F + 2 * p.H);
#pragma unroll
            for (int q = 0; q < NV; ++q) {
                const int o = (q * LPR + lane) * EV;
                if (o < F) {
#pragma unroll
                    for (int t = 0; t < EV; ++t) pr[o + t] = acc[q][t];
                    if (o % p.D == 0) {
                        pr[F + head[q]] = m[q];
                        pr[F + p.H + head[q]] = s[q];
                    }
                }
            }
            continue;
        }
        T* __restrict__ out = static_cast<T*>(p.out) + seg * F;
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            const int o = (q * LPR + lane) * EV;
            if (o < F) {
                if constexpr (INF) {
                    Vec<T>::store(out + o, acc[q]);
                    if (o % p.D == 0) {
                        p.rmax[seg * p.H + head[q]] = m[q];
                        p.rsum[seg * p.H + head[q]] = s[q];
                    }
                } else {
                    const float inv = s[q] > 0.f ? 1.f / s[q] : 0.f;
                    float w[EV];
#pragma unroll
                    for (int t = 0; t < EV; ++t) w[t] = acc[q][t] * inv;
                    Vec<T>::store(out + o, w);
                    if (o % p.D == 0)
                        p.lse[seg * p.H + head[q]] = s[q] > 0.f ? m[q] + __logf(s[q]) : -INFINITY;
                }
            }
        }
    }
}

}  // namespace regnn
