// What the two sampled-block attention operators share (re_nsgat.hip: REGATConv's scores,
// re_nsgatv2.hip: REGATv2Conv's): the wave helpers, the shape gate, the grid, the second forward
// launch -- the global-max softmax and the aggregation over a block whose scores already lie in
// the `a` buffer with one maximum per workgroup in `wgmax` -- and the opening of both backwards'
// row pass (NsRow: the chunk fill and pass 1; the relation bins' zeroing and wave-order sum).
#pragma once
#include "regnn_common.h"

#include <math.h>

namespace regnn {
namespace {

constexpr int kChunk = 64;                  // entries of a row held in LDS at a time
constexpr int kMaxHeads = 16;
constexpr int kWaves = kBlock / 64;

// LDS written by some lanes of this wave, read by others: the wave's own LDS traffic in order
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

__device__ __forceinline__ float wave_maxf(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// an entry whose source id lies outside [0, n_src) takes no part: score -inf, weight 0
__device__ __forceinline__ bool src_ok(int u, int64_t n_src) {
    return u >= 0 && int64_t(u) < n_src;
}

// the workgroup's maximum of its lanes' m into wgmax[blockIdx.x]: every workgroup, every call
__device__ __forceinline__ void store_wg_max(float m, float* __restrict__ wgmax) {
    __shared__ float smax[kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    m = wave_maxf(m);
    if (lane == 0) smax[wave] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        float b = smax[0];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) b = fmaxf(b, smax[w]);
        wgmax[blockIdx.x] = b;
    }
}

// The second forward launch of both operators. Every wave folds the workgroup maxima (a maximum
// does not depend on the order), then takes rows: the row's denominators in entry order, a in
// place of s in the buffer, out[v] = sum_e a[e,h] ft[idx_e,h,:] in entry order (64 entries in LDS
// at a time), exact zeros for a row without entries.
__device__ __forceinline__ void ns_softmax_aggregate(
    const int32_t* __restrict__ ptr, const int32_t* __restrict__ idx, const float* __restrict__ ft,
    const float* __restrict__ wgmax, int n_wg, int64_t n_rows, int64_t n_src, int H, int C,
    float* __restrict__ a, float* __restrict__ out) {
    __shared__ float sa_[kWaves][kChunk * kMaxHeads];
    __shared__ int su_[kWaves][kChunk];
    __shared__ float sden_[kWaves][kMaxHeads];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* sa = sa_[wave];
    int* su = su_[wave];
    float* sden = sden_[wave];
    float gmax = -INFINITY;
    for (int i = lane; i < n_wg; i += 64) gmax = fmaxf(gmax, wgmax[i]);
    gmax = wave_maxf(gmax);
    const int HC = H * C, nvec = HC >> 2;
    for (int64_t v = int64_t(blockIdx.x) * kWaves + wave; v < n_rows;
         v += int64_t(gridDim.x) * kWaves) {
        const int e0 = ptr[v], e1 = ptr[v + 1];
        float* orow = out + v * HC;
        if (e1 <= e0) {                        // a padded row: exact zeros
            for (int c = lane; c < nvec; c += 64)
                *reinterpret_cast<float4*>(orow + 4 * c) = make_float4(0.f, 0.f, 0.f, 0.f);
            continue;
        }
        wave_lds_sync();                       // the previous row's reads of sden are done
        if (lane < H) {                        // the row's denominators, in entry order
            float den = 0.f;
            for (int e = e0; e < e1; ++e) {
                const float sv = a[int64_t(e) * H + lane];
                den += sv == -INFINITY ? 0.f : expf(sv - gmax);
            }
            sden[lane] = den;
        }
        for (int t0 = 0; t0 < nvec; t0 += 64) {
            const int c4 = t0 + lane;
            const bool active = c4 < nvec;
            const int h = active ? (4 * c4) / C : 0;
            const bool last = t0 + 64 >= nvec;     // this pass replaces s by a in the buffer
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int cb = e0; cb < e1; cb += kChunk) {
                const int nc = min(kChunk, e1 - cb);
                wave_lds_sync();               // sden written; the previous chunk read
                for (int i = lane; i < nc * H; i += 64) {
                    const int j = i / H, hh = i - j * H;
                    const int64_t at = int64_t(cb + j) * H + hh;
                    // (rows wider than 64 vectors take several passes: all but the last leave s
                    // in the buffer and form the same a from it again)
                    const float sv = a[at];
                    const float w = (sv == -INFINITY ? 0.f : expf(sv - gmax)) /
                                    (sden[hh] + 1e-16f);
                    if (last) a[at] = w;
                    sa[i] = w;
                }
                for (int j = lane; j < nc; j += 64) {
                    const int u = idx[cb + j];
                    su[j] = src_ok(u, n_src) ? u : -1;
                }
                wave_lds_sync();
                if (active) {
#pragma unroll 4
                    for (int j = 0; j < nc; ++j) {
                        const int u = su[j];
                        if (u < 0) continue;
                        const float w = sa[j * H + h];
                        const float4 x = *reinterpret_cast<const float4*>(
                            ft + int64_t(u) * HC + 4 * c4);
                        acc.x = fmaf(w, x.x, acc.x);
                        acc.y = fmaf(w, x.y, acc.y);
                        acc.z = fmaf(w, x.z, acc.z);
                        acc.w = fmaf(w, x.w, acc.w);
                    }
                }
            }
            if (active) *reinterpret_cast<float4*>(orow + 4 * c4) = acc;
        }
    }
}

// What the two backwards' row passes share (ns_gat_bwd_body, ns_gatv2_bwd_body): a wave's view of
// one row, 64 entries at a time. xt is the message table (ft / xs), with_rel whether rel is read.
// In LDS: sa [kChunk * H] a; sg [kChunk * H] ga, which pass 2 overwrites with gl / gs; su [kChunk]
// the source id, -1 for an entry that takes no part; sr [kChunk] the relation; sD [H].
struct NsRow {
    const int32_t* idx;
    const uint8_t* rel;
    const float *xt, *a;
    int64_t n_src;
    int H, C;
    bool with_rel;
    float *sa, *sg;
    int *su, *sr;
    float* sD;

    // the chunk [cb, cb + nc) of the row whose gy is gyr: ids, a and ga into LDS
    __device__ __forceinline__ void fill(const float* gyr, int cb, int nc) const {
        const int lane = threadIdx.x & 63, HC = H * C;
        wave_lds_sync();
        for (int j = lane; j < nc; j += 64) {
            const int u = idx[cb + j];
            su[j] = src_ok(u, n_src) ? u : -1;
            sr[j] = with_rel ? int(rel[cb + j]) : 0;
        }
        for (int i = lane; i < nc * H; i += 64) {
            const int j = i / H, hh = i - j * H;
            const int u = idx[cb + j];
            float d = 0.f, w = 0.f;
            if (src_ok(u, n_src)) {
                w = a[int64_t(cb + j) * H + hh];
                const float4* gp = reinterpret_cast<const float4*>(gyr + hh * C);
                const float4* xp = reinterpret_cast<const float4*>(xt + int64_t(u) * HC + hh * C);
                for (int c = 0; c < (C >> 2); ++c) {
                    const float4 g = gp[c], x = xp[c];
                    d = fmaf(g.x, x.x, d);
                    d = fmaf(g.y, x.y, d);
                    d = fmaf(g.z, x.z, d);
                    d = fmaf(g.w, x.w, d);
                }
            }
            sa[i] = w;
            sg[i] = d;
        }
        wave_lds_sync();
    }

    // pass 1 over the row [e0, e1): D[h] = sum a ga in entry order into sD. Returns `one`: the
    // row is a single chunk, which pass 2 then finds in LDS.
    __device__ __forceinline__ bool pass1(const float* gyr, int e0, int e1) const {
        const int lane = threadIdx.x & 63;
        const bool one = e1 - e0 <= kChunk;
        float D = 0.f;
        for (int cb = e0; cb < e1; cb += kChunk) {
            const int nc = min(kChunk, e1 - cb);
            fill(gyr, cb, nc);
            if (lane < H)
                for (int j = 0; j < nc; ++j) D = fmaf(sa[j * H + lane], sg[j * H + lane], D);
        }
        if (lane < H) sD[lane] = D;
        return one;
    }
};

__device__ __forceinline__ NsRow ns_row(const int32_t* idx, const uint8_t* rel, bool with_rel,
                                        const float* xt, const float* a, int64_t n_src, int H,
                                        int C) {
    __shared__ float sa_[kWaves][kChunk * kMaxHeads];
    __shared__ float sg_[kWaves][kChunk * kMaxHeads];
    __shared__ int su_[kWaves][kChunk];
    __shared__ int sr_[kWaves][kChunk];
    __shared__ float sD_[kWaves][kMaxHeads];
    const int wave = threadIdx.x >> 6;
    return {idx, rel, xt, a, n_src, H, C, with_rel, sa_[wave], sg_[wave], su_[wave], sr_[wave],
            sD_[wave]};
}

// the workgroup's per-wave relation bins [kWaves][W] (dynamic LDS): zeroed before the rows ...
__device__ __forceinline__ void ns_bins_zero(float* bins_, int W) {
    for (int i = threadIdx.x; i < kWaves * W; i += kBlock) bins_[i] = 0.f;
    __syncthreads();
}

// ... and added in wave order into the workgroup's slab row after them
__device__ __forceinline__ void ns_bins_store(const float* bins_, int W, float* slab) {
    __syncthreads();
    for (int i = threadIdx.x; i < W; i += kBlock) {
        float t = bins_[i];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) t += bins_[w * W + i];
        slab[int64_t(blockIdx.x) * W + i] = t;
    }
}

inline int ns_gat_shape_rc(int32_t H, int32_t C) {
    if (H < 1 || H > kMaxHeads || C < 4 || C > 512 || (C & 3)) return REGNN_EUNSUPPORTED;
    return REGNN_OK;
}

inline int ns_gat_grid(int64_t cap_dst) {
    const int64_t g = (cap_dst + kWaves - 1) / kWaves;
    return int(g < 1 ? 1 : g < REGNN_NS_GAT_WORK_FLOATS ? g : REGNN_NS_GAT_WORK_FLOATS);
}

}  // namespace
}  // namespace regnn
