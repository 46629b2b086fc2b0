// The strided transposed index's second half (regnn_ns_hop strided, ABI 48): once every source's
// entry count (csc_cnt) and every slot's rank inside its source's segment (csc_rank) are final --
// ns_csc_rank_kernel wrote them in an earlier launch -- a workgroup needs nothing from any other:
// each one loads all the counts, forms their exclusive prefix in LDS by itself and places its own
// 1024 slots at prefix[source] + rank. Workgroup 0 also writes csc_ptr, the hub list and the
// piece table, the values and layout ns_csc_kernel (re_ns.hip) writes. No ticket, no flag, no
// wait: the only ordering is the launch boundary before it. Runs as its own launch
// (ns_csc_place_kernel, re_ns.hip) or as extra workgroups of the two-layer step's head launch
// (re_nsm2.hip), whose next launch (the gather) is the index's first reader.
#pragma once
#include "regnn_common.h"

namespace regnn {

constexpr int kCscPlaceT = 1024;           // threads, and slots placed, per workgroup
constexpr int kCscPlaceMax = 32768;        // sources <= slots <= this (kCscMax)
constexpr int kCscPlaceShort = 16;         // a source with more entries is a hub row (kCscShort)
constexpr int kCscPlaceUN = 8;             // counts requested per thread per round

struct CscPlaceArgs {
    const int32_t* sizes; int hop, cap_e, stride;   // stride: slots per target row (k + 1)
    const int32_t* cnt; const int32_t* rank;
    const int32_t* blk_idx; const uint8_t* blk_rel;
    int32_t* csc_ptr; int32_t* csc_ent; int32_t* csc_long;
};

// dynamic LDS: 2 x 16 wave totals (64 ints reserved), then one int per possible source
__host__ __device__ inline size_t csc_place_lds(int cap_e) {
    return (size_t(cap_e) + 64) * sizeof(int);
}
inline int csc_place_blocks(int cap_e) { return (cap_e + kCscPlaceT - 1) / kCscPlaceT; }

// workgroup `wg` of ceil(cap_e / 1024), 1024 threads; lds: csc_place_lds(cap_e) bytes
__device__ __forceinline__ void csc_scan_place(const CscPlaceArgs& A, int wg,
                                               int* __restrict__ lds) {
    constexpr int T = kCscPlaceT, NW = T / 64;
    int* sw = lds;                         // [2][NW] wave totals: entries; hub rows | pieces << 16
    int* pre = lds + 64;                   // [n] the counts, then their exclusive prefix
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int n = min(A.sizes[A.hop + 1], A.cap_e);
    // the slot's own words first: nothing below waits for them before the placement
    const int bp = wg * T + tid;
    int lid = -1, rank = 0, rel = 0;
    if (bp < A.cap_e) {
        lid = A.blk_idx[bp];               // -1: an empty slot of the strided layout
        rank = A.rank[bp];
        rel = int(A.blk_rel[bp]);
    }
    // every count, coalesced, kCscPlaceUN requests per thread in flight (one round up to 8 k
    // sources)
    for (int j0 = 0; j0 * T < n; j0 += kCscPlaceUN) {
        int v[kCscPlaceUN];
#pragma unroll
        for (int j = 0; j < kCscPlaceUN; ++j) {
            const int i = (j0 + j) * T + tid;
            v[j] = i < n ? A.cnt[i] : 0;
        }
#pragma unroll
        for (int j = 0; j < kCscPlaceUN; ++j) {
            const int i = (j0 + j) * T + tid;
            if (i < n) pre[i] = v[j];
        }
    }
    __syncthreads();
    // thread t scans the Q consecutive counts from t Q (Q odd: the lanes' LDS words fall in
    // different banks)
    const int Q = ((n + T - 1) / T) | 1, i0 = tid * Q;
    // hub rows (<= 1928) and pieces (<= 1960) of a whole block fit 16 bits each: one packed word
    int s = 0, lp = 0;
    for (int q = 0; q < Q; ++q) {
        const int c = i0 + q < n ? pre[i0 + q] : 0;
        s += c;
        lp += c > kCscPlaceShort ? 1 + (((c + REGNN_CSC_PIECE - 1) / REGNN_CSC_PIECE) << 16) : 0;
    }
    int xs = s, xlp = lp;                  // inclusive wave scans
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int ys = __shfl_up(xs, o, 64), ylp = __shfl_up(xlp, o, 64);
        if (lane >= o) {
            xs += ys;
            xlp += ylp;
        }
    }
    if (lane == 63) {
        sw[w] = xs;
        sw[NW + w] = xlp;
    }
    __syncthreads();
    int off = xs - s, olp = xlp - lp, ts = 0, tlp = 0;
#pragma unroll 4
    for (int u = 0; u < NW; ++u) {
        const int a = sw[u], b = sw[NW + u];
        if (u < w) {
            off += a;
            olp += b;
        }
        ts += a;
        tlp += b;
    }
    int loff = olp & 0xFFFF, poff = olp >> 16;
    const int tl = tlp & 0xFFFF, tp = tlp >> 16;
    int4* pieces = reinterpret_cast<int4*>(A.csc_long + REGNN_CSC_LONG_TAB);
    for (int q = 0; q < Q; ++q) {
        const int i = i0 + q;
        if (i >= n) break;
        const int c = pre[i];
        pre[i] = off;
        // hub rows ascending, each cut into pieces (counts that sum to <= cap_e stay inside both
        // tables; the bounds only keep a caller's inconsistent counts from writing past them)
        if (wg == 0 && c > kCscPlaceShort && loff < REGNN_CSC_LONG_CAP) {
            const int li = loff++;
            A.csc_long[1 + li] = i;
            const int npc = (c + REGNN_CSC_PIECE - 1) / REGNN_CSC_PIECE;
            for (int k = 0; k < npc && poff < REGNN_CSC_LONG_MAXPIECE; ++k, ++poff)
                pieces[poff] = make_int4(i, off + k * REGNN_CSC_PIECE,
                                         min(REGNN_CSC_PIECE, c - k * REGNN_CSC_PIECE),
                                         (li << 16) | (k << 8) | npc);
        }
        off += c;
    }
    __syncthreads();
    if (lid >= 0 && lid < n) {
        const int at = pre[lid] + rank;
        if (uint32_t(at) < uint32_t(A.cap_e)) A.csc_ent[at] = ((bp / A.stride) << 8) | rel;
    }
    if (wg == 0) {
        for (int i = tid; i < n; i += T) A.csc_ptr[i] = pre[i];
        if (tid == 0) {
            A.csc_ptr[n] = ts;
            A.csc_long[0] = tl;
            A.csc_long[REGNN_CSC_LONG_NPIECE] = tp;
        }
    }
}

}  // namespace regnn
