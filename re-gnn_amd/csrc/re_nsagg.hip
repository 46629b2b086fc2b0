// Typed block aggregation of raw input rows: layer 0 of the neighbour-sampled REGNN at any hidden
// width (mag/regnn_ns.py:300-346 with the reference default hidden 512, mag/regnn_ns.py:43).
//
// The reference projects every sampled node's raw row through its type's Linear (group_input,
// mag/regnn_ns.py:300-326: ~280 k rows x 128 -> hidden per step at fan-out [25, 20]) and then
// through the first conv's weight (mag/regnn_layers.py:102) before the mean aggregation. Both
// maps are linear, so for target row v of layer 0's block
//     a_v = inv_v sum_e tab[r_e] (x_e W_t(e)^T + b_t(e)) W_0 + bias
//         = inv_v sum_t (S_vt W_t^T + w_vt b_t) W_0 + bias,
//     S_vt = sum_{e in v, type(src_e) = t} tab[r_e] x_src_e,   w_vt = sum_{same e} tab[r_e],
// and the projections run over the ~13 k target rows only. This file forms S and w from the raw
// input tables (the gather: each sampled edge reads its source's raw K-float row once) and, in
// the backward, the relation-table gradient
//     d tab[r] = sum_{e: r_e = r} (<x_src_e, gS_v,t(e)> + gw_v,t(e)).
// The GEMMs (S W_c, its two backward products) stay on hipBLASLt.
//
// One forward and one backward body; the tables' widths are their compile-time policy: one K for
// every type (typed_agg_kernel / _bwd_kernel, K in {64, 128}) or one K_t per type
// (typed_agg_kt_kernel / _kt_bwd_kernel, widest K_t in {64, 128, 256}); one host launch function
// per direction.
#include "regnn_common.h"

namespace regnn {
namespace nsagg {

constexpr int kMT = REGNN_NSM_MAX_TYPES;   // node types

template <int N>
__device__ __forceinline__ const float* pick_tab(const Tabs& t, int i) {
    const float* r = t.p[0];
#pragma unroll
    for (int k = 1; k < N; ++k)
        if (i == k) r = t.p[k];
    return r;
}

// one edge's metadata, formed by one lane of the row's group (its four dependent loads run in
// parallel over the row's edges) and broadcast to the group: source type, source row in its
// type's table, tab[r_e] (tab may be null), relation id
// (e_type / e_off: the sampler's per-edge source type and table row of a meta-only hop, read
// directly instead of through the local id, n_id, node type and local row)
struct EdgeSrc {
    const int32_t* idx; const int32_t* n_id; const int32_t* ntype; const int64_t* local;
    const int32_t* e_type; const int64_t* e_off;
};

template <int LPR>
__device__ __forceinline__ void edge_meta(const EdgeSrc& E, const uint8_t* rel, const float* tab,
                                          int e, int e1, int& t, int64_t& row, float& w, int& r) {
    t = 0; row = 0; w = 0.f; r = 0;
    if (e < e1) {
        r = rel[e];
        if (E.e_type) {
            t = E.e_type[e];
            row = E.e_off[e];
        } else {
            const int g = E.n_id[E.idx[e]];
            t = E.ntype[g];
            row = E.local[g];
        }
        w = tab ? tab[r] : 0.f;
    }
}

// The width policy of the two bodies below: kq(t) float4 per row of table t, cq(t) S_t's first
// float4 in an output row. With EqualWidths kq is the constant LPR: the `l < kq` predicates and the
// select chain fold away (load index rw * LPR + l, store index k * LPR + l, no widths among the
// kernel's arguments).
template <int LPR>
struct EqualWidths {               // every table 4 LPR floats wide: S row v is [T][K]
    __device__ __forceinline__ int kq(int) const { return LPR; }
    __device__ __forceinline__ int cq(int t) const { return t * LPR; }
};

// One input width per node type (feats_type 5: paper rows 256 wide, the others 128): tables of
// widths K_t in {64, 128, 256}, S row v is [S_0 (K_0) | S_1 (K_1) | ..], S_t at column c_t =
// sum_{u < t} K_u. LPR = KM / 4 lanes per row for the widest table KM; an edge of type t is read by
// the group's first K_t / 4 lanes (one float4 each), the others sit the load out and add zeros to
// an accumulator that is never stored.
struct Widths {
    int kq[kMT];               // K_t / 4
    int cq[kMT];               // c_t / 4
};

template <int NT>
struct TypeWidths {
    const Widths& W;
    // a select chain over the NT widths (a dynamically indexed kernel argument goes to scratch)
    __device__ __forceinline__ int kq(int t) const {
        int r = W.kq[0];
#pragma unroll
        for (int k = 1; k < NT; ++k)
            if (t == k) r = W.kq[k];
        return r;
    }
    __device__ __forceinline__ int cq(int t) const { return W.cq[t]; }     // t: an unrolled index
};

// S [n_rows][sum K_t] (row stride lds floats), w [n_rows][T] (row stride ldw). LPR lanes per row,
// 64 / LPR rows per wave. Lane l keeps columns 4 l .. 4 l + 3 of every S_t, summed by fmaf in
// entry order: the two policies give the same bits where all K_t = 4 LPR.
// XT: the tables' storage type (fp32, or bf16: a lane's four columns are one 8-byte load, widened
// exactly; the sums are then those of the widened tables, bit for bit).
template <int LPR, int NT, typename XT = float, class WP>
__device__ __forceinline__ void
typed_agg_rows(const WP& Wd, const int32_t* __restrict__ ptr, const EdgeSrc& E,
               const uint8_t* __restrict__ rel, const float* __restrict__ tab, const Tabs& xt,
               int T, int64_t n_rows, float* __restrict__ S, float* __restrict__ wsum,
               int64_t lds, int64_t ldw) {
    constexpr int RPW = 64 / LPR;
    constexpr int UN = 4;
    const int lane = threadIdx.x & 63, l = lane % LPR, gl = lane - l;
    const int64_t rows_per_block = int64_t(kBlock / 64) * RPW;
    for (int64_t v0 = int64_t(blockIdx.x) * rows_per_block; v0 < n_rows;
         v0 += int64_t(gridDim.x) * rows_per_block) {
        const int64_t v = v0 + (threadIdx.x >> 6) * RPW + lane / LPR;
        if (v >= n_rows) continue;
        float4 acc[NT];
        float ws[NT];
#pragma unroll
        for (int k = 0; k < NT; ++k) {
            acc[k] = make_float4(0.f, 0.f, 0.f, 0.f);
            ws[k] = 0.f;
        }
        const int e0 = ptr[v], e1 = ptr[v + 1];
        for (int c = e0; c < e1; c += LPR) {
            int mt, mr;
            int64_t mrow;
            float mw;
            edge_meta<LPR>(E, rel, tab, c + l, e1, mt, mrow, mw, mr);
            const int m = min(LPR, e1 - c);
            for (int j = 0; j < m; j += UN) {
                float4 x[UN];
                int tt[UN];
                float ww[UN];
#pragma unroll
                for (int u = 0; u < UN; ++u) {
                    const int src = gl + min(j + u, m - 1);
                    tt[u] = __shfl(mt, src, 64);
                    const int64_t rw = __shfl(mrow, src, 64);
                    ww[u] = j + u < m ? __shfl(mw, src, 64) : 0.f;
                    const int kq = Wd.kq(tt[u]);
                    x[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (l < kq)
                        x[u] = row4(reinterpret_cast<const XT*>(pick_tab<NT>(xt, tt[u])),
                                    rw * kq + l);
                }
#pragma unroll
                for (int u = 0; u < UN; ++u) {
#pragma unroll
                    for (int k = 0; k < NT; ++k) {
                        if (tt[u] == k) {
                            acc[k].x = fmaf(ww[u], x[u].x, acc[k].x);
                            acc[k].y = fmaf(ww[u], x[u].y, acc[k].y);
                            acc[k].z = fmaf(ww[u], x[u].z, acc[k].z);
                            acc[k].w = fmaf(ww[u], x[u].w, acc[k].w);
                            ws[k] += ww[u];
                        }
                    }
                }
            }
        }
        float4* srow = reinterpret_cast<float4*>(S + v * lds);
#pragma unroll
        for (int k = 0; k < NT; ++k)
            if (k < T && l < Wd.kq(k)) srow[Wd.cq(k) + l] = acc[k];
        if (l < T) {
            float s = ws[0];
#pragma unroll
            for (int k = 1; k < NT; ++k)
                if (l == k) s = ws[k];
            wsum[v * ldw + l] = s;
        }
    }
}

template <int K, int NT>
__global__ void __launch_bounds__(kBlock)
typed_agg_kernel(const int32_t* __restrict__ ptr, EdgeSrc E, const uint8_t* __restrict__ rel,
                 const float* __restrict__ tab, Tabs xt, int T, int64_t n_rows,
                 float* __restrict__ S, float* __restrict__ wsum, int64_t lds, int64_t ldw) {
    typed_agg_rows<K / 4, NT>(EqualWidths<K / 4>{}, ptr, E, rel, tab, xt, T, n_rows, S, wsum, lds,
                              ldw);
}

template <int KM, int NT, typename XT = float>
__global__ void __launch_bounds__(kBlock)
typed_agg_kt_kernel(const int32_t* __restrict__ ptr, EdgeSrc E, const uint8_t* __restrict__ rel,
                    const float* __restrict__ tab, Tabs xt, Widths W, int T, int64_t n_rows,
                    float* __restrict__ S, float* __restrict__ wsum, int64_t lds, int64_t ldw) {
    typed_agg_rows<KM / 4, NT, XT>(TypeWidths<NT>{W}, ptr, E, rel, tab, xt, T, n_rows, S, wsum,
                                   lds, ldw);
}

// The relation bins of the backward kernels: one [256] row per row group in LDS, zeroed first ...
template <int NG>
__device__ __forceinline__ void bins_zero(float (&gbins)[NG][256]) {
    for (int i = threadIdx.x; i < NG * 256; i += kBlock) gbins[i >> 8][i & 255] = 0.f;
    __syncthreads();
}

// ... and summed in group order into the block's slab row [n_rel] after the rows
template <int NG>
__device__ __forceinline__ void bins_store(const float (&gbins)[NG][256], float* __restrict__ slab,
                                           int n_rel) {
    __syncthreads();
    for (int r = threadIdx.x; r < n_rel; r += kBlock) {
        float sr = 0.f;
        for (int k = 0; k < NG; ++k) sr += gbins[k][r];
        slab[int64_t(blockIdx.x) * n_rel + r] = sr;
    }
}

// d tab[r] = sum_e <x_src_e, gS[v, t_e]> + gw[v, t_e]: relation bins per row group in LDS (lane 0
// of the group adds its entries in order; the group rows summed in group order), one slab row
// [n_rel] per block (the caller reduces the slab in a fixed order): bitwise reproducible, no float
// atomics. The dot's butterfly runs over LPR lanes, with TypeWidths the lanes past K_t / 4 adding
// zeros: the per-type kernel's bits are its own, not the equal-width kernel's.
template <int LPR, int NT, typename XT = float, class WP>
__device__ __forceinline__ void
typed_agg_bwd_rows(const WP& Wd, const int32_t* __restrict__ ptr, const EdgeSrc& E,
                   const uint8_t* __restrict__ rel, const Tabs& xt, int T, int64_t n_rows,
                   const float* __restrict__ gS, const float* __restrict__ gw,
                   float* __restrict__ slab, int n_rel, int64_t lds, int64_t ldw) {
    constexpr int RPW = 64 / LPR;
    constexpr int UN = 4;
    constexpr int NG = kBlock / LPR;
    __shared__ float gbins[NG][256];
    bins_zero(gbins);
    const int lane = threadIdx.x & 63, l = lane % LPR, gl = lane - l;
    float* bins = gbins[threadIdx.x / LPR];
    const int64_t rows_per_block = int64_t(kBlock / 64) * RPW;
    for (int64_t v0 = int64_t(blockIdx.x) * rows_per_block; v0 < n_rows;
         v0 += int64_t(gridDim.x) * rows_per_block) {
        const int64_t v = v0 + (threadIdx.x >> 6) * RPW + lane / LPR;
        if (v >= n_rows) continue;
        const int e0 = ptr[v], e1 = ptr[v + 1];
        if (e0 == e1) continue;
        float4 g[NT];
        const float4* grow = reinterpret_cast<const float4*>(gS + v * lds);
#pragma unroll
        for (int k = 0; k < NT; ++k)
            g[k] = (k < T && l < Wd.kq(k)) ? grow[Wd.cq(k) + l] : make_float4(0.f, 0.f, 0.f, 0.f);
        const float gwl = l < T ? gw[v * ldw + l] : 0.f;
        for (int c = e0; c < e1; c += LPR) {
            int mt, mr;
            int64_t mrow;
            float mw;
            edge_meta<LPR>(E, rel, nullptr, c + l, e1, mt, mrow, mw, mr);
            (void)mw;
            const int m = min(LPR, e1 - c);
            for (int j = 0; j < m; j += UN) {
                float4 x[UN];
                int tt[UN], rr[UN];
#pragma unroll
                for (int u = 0; u < UN; ++u) {
                    const int src = gl + min(j + u, m - 1);
                    tt[u] = __shfl(mt, src, 64);
                    rr[u] = __shfl(mr, src, 64);
                    const int64_t rw = __shfl(mrow, src, 64);
                    const int kq = Wd.kq(tt[u]);
                    x[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (l < kq)
                        x[u] = row4(reinterpret_cast<const XT*>(pick_tab<NT>(xt, tt[u])),
                                    rw * kq + l);
                }
#pragma unroll
                for (int u = 0; u < UN; ++u) {
                    float4 gg = g[0];
#pragma unroll
                    for (int k = 1; k < NT; ++k)
                        if (tt[u] == k) gg = g[k];
                    // <x, gg>, fused in the order the compiler gave x.x gg.x + x.y gg.y + .. while
                    // the choice was its own: written out, so the bits no longer move with it
                    float d = fmaf(gg.w, x[u].w,
                                   fmaf(gg.z, x[u].z, fmaf(gg.x, x[u].x, gg.y * x[u].y)));
                    d = group_sum<LPR>(d);
                    const float b = __shfl(gwl, gl + tt[u], 64);
                    if (l == 0 && j + u < m) bins[rr[u]] += d + b;
                }
            }
        }
    }
    bins_store(gbins, slab, n_rel);
}

template <int K, int NT>
__global__ void __launch_bounds__(kBlock)
typed_agg_bwd_kernel(const int32_t* __restrict__ ptr, EdgeSrc E, const uint8_t* __restrict__ rel,
                     Tabs xt, int T, int64_t n_rows, const float* __restrict__ gS,
                     const float* __restrict__ gw, float* __restrict__ slab, int n_rel,
                     int64_t lds, int64_t ldw) {
    typed_agg_bwd_rows<K / 4, NT>(EqualWidths<K / 4>{}, ptr, E, rel, xt, T, n_rows, gS, gw, slab,
                                  n_rel, lds, ldw);
}

template <int KM, int NT, typename XT = float>
__global__ void __launch_bounds__(kBlock)
typed_agg_kt_bwd_kernel(const int32_t* __restrict__ ptr, EdgeSrc E,
                        const uint8_t* __restrict__ rel, Tabs xt, Widths W, int T, int64_t n_rows,
                        const float* __restrict__ gS, const float* __restrict__ gw,
                        float* __restrict__ slab, int n_rel, int64_t lds, int64_t ldw) {
    typed_agg_bwd_rows<KM / 4, NT, XT>(TypeWidths<NT>{W}, ptr, E, rel, xt, T, n_rows, gS, gw, slab,
                                       n_rel, lds, ldw);
}

// ---- layer 0 from the sampler's per-type input sums (relation slots) -------------------------
// With one relation per (target type, source type) pair (ogbn-mag's schema), the outer hop's
// sampler (regnn_ns_hop_typed_sums, on its own stream ahead of the model) forms the parameter-free
// parts: U[v][t] = the unweighted sum of row v's sampled input rows of source type t, cnt[v][t]
// their count, x_self[v] the self loop's row and the slots' relations u_rel[v][t] (-1: none),
// u_rel[v][T] = the self loop's. Layer 0's operand [S | w | 0] is then
//     S_vt = tab[r_vt] U_vt + [t = t_self(v)] tab[r_self] x_self(v),
//     w_vt = tab[r_vt] cnt_vt + [t = t_self(v)] tab[r_self]
// (agg0's formula, re_nsm2.hip) -- one read of contiguous sums per row instead of a gather of
// every sampled row on the model's critical path. 32 lanes per row (K = 128: a float4 each), two
// rows per wave. Rows in [n, the next multiple of 128) are written as zeros (the GEMMs' live-row
// tiles read them), rows past that are left alone (nothing reads them).
constexpr int kSlotK = 128;

template <int NT>
__global__ void __launch_bounds__(kBlock)
slot_agg_kernel(const int32_t* __restrict__ sizes, int hop, const float* __restrict__ U,
                const float* __restrict__ cnt, const float* __restrict__ xself,
                const int32_t* __restrict__ urel, const float* __restrict__ tab, int n_et, int T,
                int Tp, int64_t cap, float* __restrict__ out, int64_t ld) {
    const int n = sizes[hop];
    const int64_t lim = min(cap, (int64_t(n) + 127) / 128 * 128);
    const int l = threadIdx.x & 31;
    for (int64_t v = (int64_t(blockIdx.x) * kBlock + threadIdx.x) / 32; v < lim;
         v += int64_t(gridDim.x) * (kBlock / 32)) {
        float* o = out + v * ld;
        if (v >= n) {
#pragma unroll
            for (int t = 0; t < NT; ++t)
                if (t < T) *reinterpret_cast<float4*>(o + t * kSlotK + 4 * l) = make_float4(0.f, 0.f, 0.f, 0.f);
            if (l < Tp) o[T * kSlotK + l] = 0.f;
            continue;
        }
        const int32_t* ur = urel + v * (T + 1);
        const int rs = ur[T], ts = rs >= 0 ? rs - n_et : -1;
        const float ws = rs >= 0 ? tab[rs] : 0.f;
        const float4 xs = *reinterpret_cast<const float4*>(xself + v * kSlotK + 4 * l);
        float wl = 0.f;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            if (t >= T) continue;
            const int r = ur[t];
            const float wr = r >= 0 ? tab[r] : 0.f, wst = t == ts ? ws : 0.f;
            const float4 u = *reinterpret_cast<const float4*>(U + (v * T + t) * kSlotK + 4 * l);
            *reinterpret_cast<float4*>(o + t * kSlotK + 4 * l) =
                make_float4(fmaf(wst, xs.x, wr * u.x), fmaf(wst, xs.y, wr * u.y),
                            fmaf(wst, xs.z, wr * u.z), fmaf(wst, xs.w, wr * u.w));
            if (l == t) wl = fmaf(wr, cnt[v * T + t], wst);
        }
        if (l < Tp) o[T * kSlotK + l] = l < T ? wl : 0.f;
    }
}

// its relation-table gradient: d tab[r] = sum over (v, t) with r_vt = r of <U_vt, gS_vt> +
// cnt_vt gw_vt, and over v with r_self(v) = r of <x_self, gS_v,t_self> + gw_v,t_self. One slab
// row [n_rel] per block (launched with slab_rows blocks, 8 row groups each): each group adds its
// rows' terms into its own LDS bins in (t, then self) order, the groups summed in group order --
// bitwise reproducible; reduce the slab with regnn_rel_reduce.
template <int NT>
__global__ void __launch_bounds__(kBlock)
slot_agg_bwd_kernel(const int32_t* __restrict__ sizes, int hop, const float* __restrict__ U,
                    const float* __restrict__ cnt, const float* __restrict__ xself,
                    const int32_t* __restrict__ urel, const float* __restrict__ g, int64_t ld,
                    int n_et, int T, float* __restrict__ slab, int n_rel) {
    constexpr int NG = kBlock / 32;
    __shared__ float gbins[NG][256];
    bins_zero(gbins);
    const int n = sizes[hop];
    const int l = threadIdx.x & 31, grp = threadIdx.x / 32;
    float* bins = gbins[grp];
    for (int64_t v = (int64_t(blockIdx.x) * kBlock + threadIdx.x) / 32; v < n;
         v += int64_t(gridDim.x) * NG) {
        const int32_t* ur = urel + v * (T + 1);
        const int rs = ur[T], ts = rs >= 0 ? rs - n_et : -1;
        const float* gr = g + v * ld;
        const float4 xs = *reinterpret_cast<const float4*>(xself + v * kSlotK + 4 * l);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            if (t >= T) continue;
            const int r = ur[t];
            const float4 gs = *reinterpret_cast<const float4*>(gr + t * kSlotK + 4 * l);
            const float4 u = *reinterpret_cast<const float4*>(U + (v * T + t) * kSlotK + 4 * l);
            const float gw = gr[T * kSlotK + t];
            if (r >= 0) {
                const float d = group_sum<32>(u.x * gs.x + u.y * gs.y + u.z * gs.z + u.w * gs.w);
                if (l == 0) bins[r] += fmaf(cnt[v * T + t], gw, d);
            }
            if (t == ts) {
                const float d = group_sum<32>(xs.x * gs.x + xs.y * gs.y + xs.z * gs.z + xs.w * gs.w);
                if (l == 0) bins[rs] += d + gw;
            }
        }
    }
    bins_store(gbins, slab, n_rel);
}

// The two slot kernels over regnn_ns_hop_typed_sums_kt's outputs: one width K_t in {64, 128, 256}
// per type, U [cap][sum K_t] and the output's S part with type t at column sum_{u<t} K_u, x_self
// [cap][max K_t]. A lane takes kSlotP float4 columns of every per-type sum, column 4 l of each
// pass of kSlotK, and sits out the passes past a type's width. The widths come by value, a byte per
// type (every type index is an unrolled one: scalar shifts). Kernels of their own (slot_agg_kernel's
// scalar registers moved when its body became a width policy's: its text stays as it was); the
// formulas and their order are slot_agg_kernel's / _bwd_kernel's, so all K_t = 128 gives their bits.
constexpr int kSlotP = 2;          // 256 / kSlotK

struct SlotWidths {                // a byte per type
    uint32_t kq;                   // K_t / 4 (0 past the last type)
    uint32_t cq;                   // (sum_{u<t} K_u) / 4
    int sk, km;                    // sum K_t, max K_t
    __device__ __forceinline__ int k(int t) const { return int((kq >> (8 * t)) & 0xFFu) * 4; }
    __device__ __forceinline__ int col(int t) const { return int((cq >> (8 * t)) & 0xFFu) * 4; }
};

__device__ __forceinline__ float4 slot_load(bool on, const float* p) {
    return on ? *reinterpret_cast<const float4*>(p) : make_float4(0.f, 0.f, 0.f, 0.f);
}

template <int NT>
__global__ void __launch_bounds__(kBlock)
slot_agg_kt_kernel(const int32_t* __restrict__ sizes, int hop, const float* __restrict__ U,
                   const float* __restrict__ cnt, const float* __restrict__ xself,
                   const int32_t* __restrict__ urel, const float* __restrict__ tab, SlotWidths W,
                   int n_et, int T, int Tp, int64_t cap, float* __restrict__ out, int64_t ld) {
    const int n = sizes[hop];
    const int64_t lim = min(cap, (int64_t(n) + 127) / 128 * 128);
    const int l = threadIdx.x & 31;
    for (int64_t v = (int64_t(blockIdx.x) * kBlock + threadIdx.x) / 32; v < lim;
         v += int64_t(gridDim.x) * (kBlock / 32)) {
        float* o = out + v * ld;
        if (v >= n) {
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int p = 0; p < kSlotP; ++p)
                    if (t < T && p * kSlotK + 4 * l < W.k(t))
                        *reinterpret_cast<float4*>(o + W.col(t) + p * kSlotK + 4 * l) =
                            make_float4(0.f, 0.f, 0.f, 0.f);
            if (l < Tp) o[W.sk + l] = 0.f;
            continue;
        }
        const int32_t* ur = urel + v * (T + 1);
        const int rs = ur[T], ts = rs >= 0 ? rs - n_et : -1;
        const float ws = rs >= 0 ? tab[rs] : 0.f;
        float4 xs[kSlotP];
#pragma unroll
        for (int p = 0; p < kSlotP; ++p)
            xs[p] = slot_load(p * kSlotK + 4 * l < W.km, xself + v * W.km + p * kSlotK + 4 * l);
        float wl = 0.f;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            if (t >= T) continue;
            const int r = ur[t];
            const float wr = r >= 0 ? tab[r] : 0.f, wst = t == ts ? ws : 0.f;
#pragma unroll
            for (int p = 0; p < kSlotP; ++p) {
                const int c = p * kSlotK + 4 * l;
                if (c >= W.k(t)) continue;
                const float4 u = *reinterpret_cast<const float4*>(U + v * W.sk + W.col(t) + c);
                *reinterpret_cast<float4*>(o + W.col(t) + c) =
                    make_float4(fmaf(wst, xs[p].x, wr * u.x), fmaf(wst, xs[p].y, wr * u.y),
                                fmaf(wst, xs[p].z, wr * u.z), fmaf(wst, xs[p].w, wr * u.w));
            }
            if (l == t) wl = fmaf(wr, cnt[v * T + t], wst);
        }
        if (l < Tp) o[W.sk + l] = l < T ? wl : 0.f;
    }
}

// <a, b> over a lane's float4 columns. The first pass's four products are fused in the orders the
// compiler chose in slot_agg_bwd_kernel, read from its code: x first for <U, gS>, y first for
// <x_self, gS> (as typed_agg_bwd_rows' dot). Written out, so all K_t = 128 gives that kernel's bits
// whatever the compiler would choose here; the later passes' products are added after them
template <bool YFIRST>
__device__ __forceinline__ float slot_dot4(const float4& a, const float4& b) {
    const float d = YFIRST ? fmaf(a.x, b.x, a.y * b.y) : fmaf(a.y, b.y, a.x * b.x);
    return fmaf(a.w, b.w, fmaf(a.z, b.z, d));
}

template <bool YFIRST>
__device__ __forceinline__ float slot_dot(const float4 (&a)[kSlotP], const float4 (&b)[kSlotP]) {
    float d = slot_dot4<YFIRST>(a[0], b[0]);
#pragma unroll
    for (int p = 1; p < kSlotP; ++p) d += slot_dot4<YFIRST>(a[p], b[p]);
    return d;
}

template <int NT>
__global__ void __launch_bounds__(kBlock)
slot_agg_kt_bwd_kernel(const int32_t* __restrict__ sizes, int hop, const float* __restrict__ U,
                       const float* __restrict__ cnt, const float* __restrict__ xself,
                       const int32_t* __restrict__ urel, const float* __restrict__ g, int64_t ld,
                       SlotWidths W, int n_et, int T, float* __restrict__ slab, int n_rel) {
    constexpr int NG = kBlock / 32;
    __shared__ float gbins[NG][256];
    bins_zero(gbins);
    const int n = sizes[hop];
    const int l = threadIdx.x & 31, grp = threadIdx.x / 32;
    float* bins = gbins[grp];
    for (int64_t v = (int64_t(blockIdx.x) * kBlock + threadIdx.x) / 32; v < n;
         v += int64_t(gridDim.x) * NG) {
        const int32_t* ur = urel + v * (T + 1);
        const int rs = ur[T], ts = rs >= 0 ? rs - n_et : -1;
        const float* gr = g + v * ld;
        float4 xs[kSlotP];
#pragma unroll
        for (int p = 0; p < kSlotP; ++p)
            xs[p] = slot_load(p * kSlotK + 4 * l < W.km, xself + v * W.km + p * kSlotK + 4 * l);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            if (t >= T) continue;
            const int r = ur[t];
            float4 gs[kSlotP], u[kSlotP];
#pragma unroll
            for (int p = 0; p < kSlotP; ++p) {
                const int c = p * kSlotK + 4 * l;
                gs[p] = slot_load(c < W.k(t), gr + W.col(t) + c);
                u[p] = slot_load(c < W.k(t), U + v * W.sk + W.col(t) + c);
            }
            const float gw = gr[W.sk + t];
            if (r >= 0) {
                const float d = group_sum<32>(slot_dot<false>(u, gs));
                if (l == 0) bins[r] += fmaf(cnt[v * T + t], gw, d);
            }
            if (t == ts) {
                const float d = group_sum<32>(slot_dot<true>(xs, gs));
                if (l == 0) bins[rs] += d + gw;
            }
        }
    }
    bins_store(gbins, slab, n_rel);
}

// ---- the mean aggregation of a block in the strided layout (regnn_ns_hop strided = 1) --------
// row i's edges at slots [i S, i S + cnt[i]] (sampled ones in CSR order, the self loop last), the
// slot order the CSR layout keeps: y[i] = inv[i] sum_e tab[rel_e] x[idx_e] + bias for live rows
// i < sizes[0], bias for the others. One wave per row, LPR lanes x VPL float4 per lane, the
// row's entries loaded lane-parallel and its source rows UN at a time in flight.
template <int VPL>
__global__ void __launch_bounds__(kBlock)
strided_spmm_kernel(const int32_t* __restrict__ live, const int32_t* __restrict__ cnt, int S,
                    const int32_t* __restrict__ idx, const uint8_t* __restrict__ rel,
                    const float* __restrict__ tab, const float* __restrict__ inv,
                    const float* __restrict__ bias, const float* __restrict__ x,
                    float* __restrict__ y, int64_t n_rows, int F) {
    constexpr int UN = 8;
    const int lane = threadIdx.x & 63;
    const int n = live[0];
    const int nv = F / 4;
    for (int64_t i = (int64_t(blockIdx.x) * kBlock + threadIdx.x) / 64; i < n_rows;
         i += int64_t(gridDim.x) * (kBlock / 64)) {
        float4 acc[VPL];
#pragma unroll
        for (int q = 0; q < VPL; ++q) acc[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        const int m = i < n ? cnt[i] + 1 : 0;
        const int64_t base = i * S;
        const int my_u = lane < m ? idx[base + lane] : 0;
        const float my_w = lane < m ? (tab ? tab[rel[base + lane]] : 1.f) : 0.f;
        for (int j = 0; j < m; j += UN) {
            float4 xv[UN][VPL];
#pragma unroll
            for (int u = 0; u < UN; ++u) {
                const int uu = __shfl(my_u, min(j + u, m - 1), 64);
#pragma unroll
                for (int q = 0; q < VPL; ++q) {
                    const int c = lane + 64 * q;
                    xv[u][q] = c < nv ? reinterpret_cast<const float4*>(x + int64_t(uu) * F)[c]
                                      : make_float4(0.f, 0.f, 0.f, 0.f);
                }
            }
#pragma unroll
            for (int u = 0; u < UN; ++u) {
                if (j + u >= m) continue;
                const float w = __shfl(my_w, j + u, 64);
#pragma unroll
                for (int q = 0; q < VPL; ++q) {
                    acc[q].x = fmaf(w, xv[u][q].x, acc[q].x);
                    acc[q].y = fmaf(w, xv[u][q].y, acc[q].y);
                    acc[q].z = fmaf(w, xv[u][q].z, acc[q].z);
                    acc[q].w = fmaf(w, xv[u][q].w, acc[q].w);
                }
            }
        }
        const float iv = i < n ? inv[i] : 0.f;
#pragma unroll
        for (int q = 0; q < VPL; ++q) {
            const int c = lane + 64 * q;
            if (c >= nv) continue;
            float4 b = bias ? reinterpret_cast<const float4*>(bias)[c] : make_float4(0.f, 0.f, 0.f, 0.f);
            b.x = fmaf(iv, acc[q].x, b.x);
            b.y = fmaf(iv, acc[q].y, b.y);
            b.z = fmaf(iv, acc[q].z, b.z);
            b.w = fmaf(iv, acc[q].w, b.w);
            reinterpret_cast<float4*>(y + i * F)[c] = b;
        }
    }
}

}  // namespace nsagg
}  // namespace regnn

using namespace regnn;
using namespace regnn::nsagg;

// What the four entries share after their own pointer and range checks (E is theirs, edge_src):
// the tables, non-null and 16-byte aligned (the kernels read them with 16-byte loads); their
// widths, K_t[t] per type for the _kt entries (each in {64, 128, 256}: REGNN_EUNSUPPORTED
// otherwise) or, K_t null, K for every type (any K: the launch refuses what it has no kernel for);
// the S / gS operand `s`, 16-byte aligned, ld_s >= sum K_t and a multiple of 4, ld_w >= n_types.
// bf: the tables hold bf16 rows (the _dt entries; per-type widths only), carried as float pointers.
struct AggCall {
    const int32_t* ptr; EdgeSrc E; const uint8_t* rel; Tabs xt; Widths W;
    bool per_type, bf;
    int km, T;                 // the widest table (LPR = km / 4), node types
    int64_t n_rows, lds, ldw; hipStream_t stream;
};

static int agg_call(AggCall& c, const int32_t* ptr, const uint8_t* rel,
                    const void* const* tables, bool bf, int32_t n_types, const int32_t* K_t,
                    int32_t K, int64_t n_rows, const float* s, int64_t ld_s, int64_t ld_w,
                    hipStream_t stream) {
    c.ptr = ptr, c.rel = rel, c.xt = Tabs{}, c.W = Widths{}, c.per_type = K_t != nullptr, c.bf = bf;
    c.km = 0, c.T = n_types, c.n_rows = n_rows, c.lds = ld_s, c.ldw = ld_w, c.stream = stream;
    int64_t sk = 0;
    for (int t = 0; t < n_types; ++t) {
        const int k = K_t ? K_t[t] : K;
        if (K_t && k != 64 && k != 128 && k != 256) return REGNN_EUNSUPPORTED;
        if (!tables[t] || reinterpret_cast<uintptr_t>(tables[t]) % 16) return REGNN_EINVAL;
        c.xt.p[t] = static_cast<const float*>(tables[t]);
        c.W.kq[t] = k / 4;
        c.W.cq[t] = int(sk / 4);
        sk += k;
        if (k > c.km) c.km = k;
    }
    const bool ok = ld_s >= sk && ld_s % 4 == 0 && reinterpret_cast<uintptr_t>(s) % 16 == 0;
    return ok && ld_w >= n_types ? REGNN_OK : REGNN_EINVAL;
}

// One launch per direction. The per-type kernels are built for a widest table of 64, 128 and 256,
// the equal-width ones for 64 and 128 (an equal width of 256 is the _kt entries').
template <int KK, int N>
static int agg_fwd_at(const AggCall& c, const float* tab, float* S, float* wsum) {
    const int64_t rpb = int64_t(kBlock / 64) * (64 / (KK / 4));
    const dim3 grid(unsigned(std::min<int64_t>((c.n_rows + rpb - 1) / rpb, kMaxGrid)));
    if (c.bf)
        hipLaunchKernelGGL((typed_agg_kt_kernel<KK, N, bf16_t>), grid, dim3(kBlock), 0, c.stream,
                           c.ptr, c.E, c.rel, tab, c.xt, c.W, c.T, c.n_rows, S, wsum, c.lds, c.ldw);
    else if (c.per_type)
        hipLaunchKernelGGL((typed_agg_kt_kernel<KK, N>), grid, dim3(kBlock), 0, c.stream, c.ptr,
                           c.E, c.rel, tab, c.xt, c.W, c.T, c.n_rows, S, wsum, c.lds, c.ldw);
    else if constexpr (KK <= 128)
        hipLaunchKernelGGL((typed_agg_kernel<KK, N>), grid, dim3(kBlock), 0, c.stream, c.ptr, c.E,
                           c.rel, tab, c.xt, c.T, c.n_rows, S, wsum, c.lds, c.ldw);
    else return REGNN_EUNSUPPORTED;
    REGNN_LAUNCH_CHECK();
    return REGNN_OK;
}

template <int KK, int N>
static int agg_bwd_at(const AggCall& c, const float* gS, const float* gw, float* slab, int n_rel,
                      int slab_rows) {
    if (c.bf)
        hipLaunchKernelGGL((typed_agg_kt_bwd_kernel<KK, N, bf16_t>), dim3(unsigned(slab_rows)),
                           dim3(kBlock), 0, c.stream, c.ptr, c.E, c.rel, c.xt, c.W, c.T, c.n_rows,
                           gS, gw, slab, n_rel, c.lds, c.ldw);
    else if (c.per_type)
        hipLaunchKernelGGL((typed_agg_kt_bwd_kernel<KK, N>), dim3(unsigned(slab_rows)),
                           dim3(kBlock), 0, c.stream, c.ptr, c.E, c.rel, c.xt, c.W, c.T, c.n_rows,
                           gS, gw, slab, n_rel, c.lds, c.ldw);
    else if constexpr (KK <= 128)
        hipLaunchKernelGGL((typed_agg_bwd_kernel<KK, N>), dim3(unsigned(slab_rows)), dim3(kBlock),
                           0, c.stream, c.ptr, c.E, c.rel, c.xt, c.T, c.n_rows, gS, gw, slab,
                           n_rel, c.lds, c.ldw);
    else return REGNN_EUNSUPPORTED;
    REGNN_LAUNCH_CHECK();
    return REGNN_OK;
}

// (widest K, n_types <= 4 / <= 8) -> the instantiation
#define AGG_DISPATCH(AT, ...)                                                                  \
    if (c.km == 64) return c.T <= 4 ? AT<64, 4>(__VA_ARGS__) : AT<64, 8>(__VA_ARGS__);         \
    if (c.km == 128) return c.T <= 4 ? AT<128, 4>(__VA_ARGS__) : AT<128, 8>(__VA_ARGS__);      \
    if (c.km == 256) return c.T <= 4 ? AT<256, 4>(__VA_ARGS__) : AT<256, 8>(__VA_ARGS__);      \
    return REGNN_EUNSUPPORTED;

static int agg_fwd(const AggCall& c, const float* tab, float* S, float* wsum) {
    if (c.n_rows == 0) return REGNN_OK;
    AGG_DISPATCH(agg_fwd_at, c, tab, S, wsum)
}

// (no early return at n_rows == 0: the slab's rows are written, as zeros)
static int agg_bwd(const AggCall& c, const float* gS, const float* gw, float* slab, int n_rel,
                   int slab_rows) {
    AGG_DISPATCH(agg_bwd_at, c, gS, gw, slab, n_rel, slab_rows)
}
#undef AGG_DISPATCH

extern "C" {

static bool edge_src(const int32_t* idx, const int32_t* n_id, const int32_t* ntype,
                     const int64_t* local, const int32_t* e_type, const int64_t* e_off,
                     EdgeSrc& E) {
    E = EdgeSrc{idx, n_id, ntype, local, e_type, e_off};
    if (e_type || e_off) return e_type && e_off;
    return idx && n_id && ntype && local;
}

int regnn_ns_typed_agg(const int32_t* ptr, const int32_t* idx, const uint8_t* rel,
                       const float* rel_table, const int32_t* n_id, const int32_t* ntype,
                       const int64_t* local, const int32_t* e_type, const int64_t* e_off,
                       const float* const* tables, int32_t n_types, int32_t K, int64_t n_rows,
                       float* S, float* wsum, int64_t ld_s, int64_t ld_w, hipStream_t stream) {
    AggCall c;
    if (!ptr || !rel || !rel_table || !tables || !S || !wsum || n_types <= 0 || n_types > kMT ||
        n_rows < 0 || !edge_src(idx, n_id, ntype, local, e_type, e_off, c.E))
        return REGNN_EINVAL;
    int rc = agg_call(c, ptr, rel, reinterpret_cast<const void* const*>(tables), false, n_types,
                      nullptr, K, n_rows, S, ld_s, ld_w, stream);
    return rc ? rc : agg_fwd(c, rel_table, S, wsum);
}

int regnn_ns_typed_agg_bwd(const int32_t* ptr, const int32_t* idx, const uint8_t* rel,
                           const int32_t* n_id, const int32_t* ntype, const int64_t* local,
                           const int32_t* e_type, const int64_t* e_off,
                           const float* const* tables, int32_t n_types, int32_t K, int64_t n_rows,
                           const float* gS, const float* gw, int64_t ld_s, int64_t ld_w,
                           float* slab, int32_t n_rel, int32_t slab_rows, hipStream_t stream) {
    AggCall c;
    if (!ptr || !rel || !tables || !gS || !gw || !slab || n_types <= 0 || n_types > kMT ||
        n_rows < 0 || n_rel <= 0 || n_rel > 256 || slab_rows <= 0 ||
        !edge_src(idx, n_id, ntype, local, e_type, e_off, c.E))
        return REGNN_EINVAL;
    int rc = agg_call(c, ptr, rel, reinterpret_cast<const void* const*>(tables), false, n_types,
                      nullptr, K, n_rows, gS, ld_s, ld_w, stream);
    return rc ? rc : agg_bwd(c, gS, gw, slab, n_rel, slab_rows);
}

int regnn_ns_typed_agg_kt(const int32_t* ptr, const int32_t* idx, const uint8_t* rel,
                          const float* rel_table, const int32_t* n_id, const int32_t* ntype,
                          const int64_t* local, const int32_t* e_type, const int64_t* e_off,
                          const float* const* tables, int32_t n_types, const int32_t* K_t,
                          int64_t n_rows, float* S, float* wsum, int64_t ld_s, int64_t ld_w,
                          hipStream_t stream) {
    AggCall c;
    if (!ptr || !rel || !rel_table || !tables || !K_t || !S || !wsum || n_types <= 0 ||
        n_types > kMT || n_rows < 0 || !edge_src(idx, n_id, ntype, local, e_type, e_off, c.E))
        return REGNN_EINVAL;
    int rc = agg_call(c, ptr, rel, reinterpret_cast<const void* const*>(tables), false, n_types,
                      K_t, 0, n_rows, S, ld_s, ld_w, stream);
    return rc ? rc : agg_fwd(c, rel_table, S, wsum);
}

int regnn_ns_typed_agg_kt_bwd(const int32_t* ptr, const int32_t* idx, const uint8_t* rel,
                              const int32_t* n_id, const int32_t* ntype, const int64_t* local,
                              const int32_t* e_type, const int64_t* e_off,
                              const float* const* tables, int32_t n_types, const int32_t* K_t,
                              int64_t n_rows, const float* gS, const float* gw, int64_t ld_s,
                              int64_t ld_w, float* slab, int32_t n_rel, int32_t slab_rows,
                              hipStream_t stream) {
    AggCall c;
    if (!ptr || !rel || !tables || !K_t || !gS || !gw || !slab || n_types <= 0 ||
        n_types > kMT || n_rows < 0 || n_rel <= 0 || n_rel > 256 || slab_rows <= 0 ||
        !edge_src(idx, n_id, ntype, local, e_type, e_off, c.E))
        return REGNN_EINVAL;
    int rc = agg_call(c, ptr, rel, reinterpret_cast<const void* const*>(tables), false, n_types,
                      K_t, 0, n_rows, gS, ld_s, ld_w, stream);
    return rc ? rc : agg_bwd(c, gS, gw, slab, n_rel, slab_rows);
}

// the _kt entries with the tables' storage type: REGNN_F32 is the _kt entry itself, REGNN_BF16 its
// kernels reading bf16 rows (every other check is the _kt entry's)
int regnn_ns_typed_agg_dt(const int32_t* ptr, const int32_t* idx, const uint8_t* rel,
                          const float* rel_table, const int32_t* n_id, const int32_t* ntype,
                          const int64_t* local, const int32_t* e_type, const int64_t* e_off,
                          const void* const* tables, int32_t dtype, int32_t n_types,
                          const int32_t* K_t, int64_t n_rows, float* S, float* wsum, int64_t ld_s,
                          int64_t ld_w, hipStream_t stream) {
    if (dtype == REGNN_F32)
        return regnn_ns_typed_agg_kt(ptr, idx, rel, rel_table, n_id, ntype, local, e_type, e_off,
                                     reinterpret_cast<const float* const*>(tables), n_types, K_t,
                                     n_rows, S, wsum, ld_s, ld_w, stream);
    AggCall c;
    if (dtype != REGNN_BF16 || !ptr || !rel || !rel_table || !tables || !K_t || !S || !wsum ||
        n_types <= 0 || n_types > kMT || n_rows < 0 ||
        !edge_src(idx, n_id, ntype, local, e_type, e_off, c.E))
        return REGNN_EINVAL;
    int rc = agg_call(c, ptr, rel, tables, true, n_types, K_t, 0, n_rows, S, ld_s, ld_w, stream);
    return rc ? rc : agg_fwd(c, rel_table, S, wsum);
}

int regnn_ns_typed_agg_dt_bwd(const int32_t* ptr, const int32_t* idx, const uint8_t* rel,
                              const int32_t* n_id, const int32_t* ntype, const int64_t* local,
                              const int32_t* e_type, const int64_t* e_off,
                              const void* const* tables, int32_t dtype, int32_t n_types,
                              const int32_t* K_t, int64_t n_rows, const float* gS, const float* gw,
                              int64_t ld_s, int64_t ld_w, float* slab, int32_t n_rel,
                              int32_t slab_rows, hipStream_t stream) {
    if (dtype == REGNN_F32)
        return regnn_ns_typed_agg_kt_bwd(ptr, idx, rel, n_id, ntype, local, e_type, e_off,
                                         reinterpret_cast<const float* const*>(tables), n_types,
                                         K_t, n_rows, gS, gw, ld_s, ld_w, slab, n_rel, slab_rows,
                                         stream);
    AggCall c;
    if (dtype != REGNN_BF16 || !ptr || !rel || !tables || !K_t || !gS || !gw || !slab ||
        n_types <= 0 || n_types > kMT || n_rows < 0 || n_rel <= 0 || n_rel > 256 ||
        slab_rows <= 0 || !edge_src(idx, n_id, ntype, local, e_type, e_off, c.E))
        return REGNN_EINVAL;
    int rc = agg_call(c, ptr, rel, tables, true, n_types, K_t, 0, n_rows, gS, ld_s, ld_w, stream);
    return rc ? rc : agg_bwd(c, gS, gw, slab, n_rel, slab_rows);
}

int regnn_ns_spmm_strided_fwd(const int32_t* live, const int32_t* cnt, int32_t stride,
                              const int32_t* idx, const uint8_t* rel, const float* rel_table,
                              const float* inv, const float* bias, const float* x, float* y,
                              int64_t n_rows, int32_t F, hipStream_t stream) {
    if (!live || !cnt || !idx || !inv || !x || !y || (rel_table && !rel) || n_rows < 0 ||
        stride < 1 || stride > 64 || F <= 0 || F % 4)
        return REGNN_EINVAL;
    if (reinterpret_cast<uintptr_t>(x) % 16 || reinterpret_cast<uintptr_t>(y) % 16 ||
        (bias && reinterpret_cast<uintptr_t>(bias) % 16))
        return REGNN_EINVAL;
    if (n_rows == 0) return REGNN_OK;
    int64_t grid = (n_rows + kBlock / 64 - 1) / (kBlock / 64);
    if (grid > kMaxGrid) grid = kMaxGrid;
    const int vpl = (F / 4 + 63) / 64;
#define SSP_CASE(V)                                                                             \
    if (vpl <= V) {                                                                             \
        hipLaunchKernelGGL((strided_spmm_kernel<V>), dim3(unsigned(grid)), dim3(kBlock), 0,     \
                           stream, live, cnt, stride, idx, rel, rel_table, inv, bias, x, y,     \
                           n_rows, F);                                                          \
        REGNN_LAUNCH_CHECK();                                                                   \
        return REGNN_OK;                                                                        \
    }
    SSP_CASE(1) SSP_CASE(2) SSP_CASE(4)
#undef SSP_CASE
    return REGNN_EUNSUPPORTED;
}

// What the slot entries share: K for every type (widths NULL; K = kSlotK and <= 4 types or
// REGNN_EUNSUPPORTED) or one width per type, each 64 / 128 / 256 (the _kt entries)
static int slot_widths(int32_t n_types, int32_t K, const int32_t* widths, SlotWidths& W) {
    W = SlotWidths{};
    if ((!widths && K != kSlotK) || n_types > 4) return REGNN_EUNSUPPORTED;
    for (int t = 0; t < n_types; ++t) {
        const int k = widths ? widths[t] : K;
        if (k != 64 && k != 128 && k != 256) return REGNN_EUNSUPPORTED;
        W.kq |= uint32_t(k / 4) << (8 * t);
        W.cq |= uint32_t(W.sk / 4) << (8 * t);
        W.sk += k;
        W.km = std::max(W.km, k);
    }
    return REGNN_OK;
}

static int slot_agg_call(const int32_t* sizes, int32_t hop, const float* U, const float* cnt,
                         const float* x_self, const int32_t* u_rel, const float* rel_table,
                         int32_t n_et, int32_t n_types, int32_t K, const int32_t* widths,
                         int64_t cap, float* out, int64_t ld, hipStream_t stream) {
    if (!sizes || !U || !cnt || !x_self || !u_rel || !rel_table || !out || hop < 0 || hop > 7 ||
        n_et < 0 || n_types < 1 || cap < 0)
        return REGNN_EINVAL;
    SlotWidths W;
    if (int rc = slot_widths(n_types, K, widths, W)) return rc;
    const int Tp = (n_types + 3) & ~3;
    if (ld < int64_t(W.sk) + Tp || ld % 4 || reinterpret_cast<uintptr_t>(out) % 16 ||
        reinterpret_cast<uintptr_t>(U) % 16 || reinterpret_cast<uintptr_t>(x_self) % 16)
        return REGNN_EINVAL;
    if (cap == 0) return REGNN_OK;
    int64_t grid = (cap + kBlock / 32 - 1) / (kBlock / 32);
    if (grid > kMaxGrid) grid = kMaxGrid;
    if (widths)
        hipLaunchKernelGGL((slot_agg_kt_kernel<4>), dim3(unsigned(grid)), dim3(kBlock), 0, stream,
                           sizes, hop, U, cnt, x_self, u_rel, rel_table, W, n_et, n_types, Tp,
                           cap, out, ld);
    else
        hipLaunchKernelGGL((slot_agg_kernel<4>), dim3(unsigned(grid)), dim3(kBlock), 0, stream,
                           sizes, hop, U, cnt, x_self, u_rel, rel_table, n_et, n_types, Tp, cap,
                           out, ld);
    REGNN_LAUNCH_CHECK();
    return REGNN_OK;
}

static int slot_agg_bwd_call(const int32_t* sizes, int32_t hop, const float* U, const float* cnt,
                             const float* x_self, const int32_t* u_rel, const float* g,
                             int64_t ld, int32_t n_et, int32_t n_types, int32_t K,
                             const int32_t* widths, float* slab, int32_t n_rel,
                             int32_t slab_rows, hipStream_t stream) {
    if (!sizes || !U || !cnt || !x_self || !u_rel || !g || !slab || hop < 0 || hop > 7 ||
        n_et < 0 || n_types < 1 || n_rel <= 0 || n_rel > 256 || slab_rows <= 0)
        return REGNN_EINVAL;
    SlotWidths W;
    if (int rc = slot_widths(n_types, K, widths, W)) return rc;
    if (ld < int64_t(W.sk) + n_types || ld % 4 || reinterpret_cast<uintptr_t>(g) % 16 ||
        reinterpret_cast<uintptr_t>(U) % 16 || reinterpret_cast<uintptr_t>(x_self) % 16)
        return REGNN_EINVAL;
    if (widths)
        hipLaunchKernelGGL((slot_agg_kt_bwd_kernel<4>), dim3(unsigned(slab_rows)), dim3(kBlock),
                           0, stream, sizes, hop, U, cnt, x_self, u_rel, g, ld, W, n_et, n_types,
                           slab, n_rel);
    else
        hipLaunchKernelGGL((slot_agg_bwd_kernel<4>), dim3(unsigned(slab_rows)), dim3(kBlock), 0,
                           stream, sizes, hop, U, cnt, x_self, u_rel, g, ld, n_et, n_types, slab,
                           n_rel);
    REGNN_LAUNCH_CHECK();
    return REGNN_OK;
}

int regnn_ns_slot_agg(const int32_t* sizes, int32_t hop, const float* U, const float* cnt,
                      const float* x_self, const int32_t* u_rel, const float* rel_table,
                      int32_t n_et, int32_t n_types, int32_t K, int64_t cap, float* out,
                      int64_t ld, hipStream_t stream) {
    return slot_agg_call(sizes, hop, U, cnt, x_self, u_rel, rel_table, n_et, n_types, K, nullptr,
                         cap, out, ld, stream);
}

int regnn_ns_slot_agg_bwd(const int32_t* sizes, int32_t hop, const float* U, const float* cnt,
                          const float* x_self, const int32_t* u_rel, const float* g, int64_t ld,
                          int32_t n_et, int32_t n_types, int32_t K, float* slab, int32_t n_rel,
                          int32_t slab_rows, hipStream_t stream) {
    return slot_agg_bwd_call(sizes, hop, U, cnt, x_self, u_rel, g, ld, n_et, n_types, K, nullptr,
                             slab, n_rel, slab_rows, stream);
}

int regnn_ns_slot_agg_kt(const int32_t* sizes, int32_t hop, const float* U, const float* cnt,
                         const float* x_self, const int32_t* u_rel, const float* rel_table,
                         int32_t n_et, int32_t n_types, const int32_t* widths, int64_t cap,
                         float* out, int64_t ld, hipStream_t stream) {
    if (!widths) return REGNN_EINVAL;
    return slot_agg_call(sizes, hop, U, cnt, x_self, u_rel, rel_table, n_et, n_types, 0, widths,
                         cap, out, ld, stream);
}

int regnn_ns_slot_agg_bwd_kt(const int32_t* sizes, int32_t hop, const float* U, const float* cnt,
                             const float* x_self, const int32_t* u_rel, const float* g,
                             int64_t ld, int32_t n_et, int32_t n_types, const int32_t* widths,
                             float* slab, int32_t n_rel, int32_t slab_rows, hipStream_t stream) {
    if (!widths) return REGNN_EINVAL;
    return slot_agg_bwd_call(sizes, hop, U, cnt, x_self, u_rel, g, ld, n_et, n_types, 0, widths,
                             slab, n_rel, slab_rows, stream);
}

}  // extern "C"
