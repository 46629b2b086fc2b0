// The canonical transposed index of one device-sampled CSR block (regnn_ns_block_tidx): per source
// u its live entries' CSR positions, ascending -- the stable sort of the live entries by source --
// with each slot's target row, and the table of long segments cut into pieces. What the gather
// form of the block attention backwards walks (re_nsgat_src.h). A pure function of the block: no
// float, no order-dependent result, no workgroup waiting on another, no host size; every grid is
// sized by a capacity and every slot a reader takes is rewritten by every call.
//
//   clear      the per-source counts (hipMemsetAsync over the build's own scratch)
//   launch 1   tidx_count_kernel  a wave per row: integer atomics, counts do not depend on order
//   launch 2-4 the exclusive scan of the counts (and of the rows' piece counts) in three launches
//              over tiles of 1024 sources, none waiting on another workgroup: tidx_tile_kernel
//              (each tile's sums), tidx_tile_scan_kernel (ONE workgroup scans the tiles' sums),
//              tidx_emit_kernel (each tile again with its offset: t_ptr, the cursors back to
//              zero, the piece table -- sources ascending, a row's pieces consecutive)
//   launch 5   tidx_place_kernel  a wave per row: slots by an atomic cursor into the scratch (the
//                                 order inside a segment is run-dependent HERE and nowhere later)
//   launch 6   tidx_rank_kernel   a thread per slot: its rank among its segment's positions (a
//                                 count: order-free), the entry and its row written at that rank
#include "regnn_common.h"

namespace regnn {
namespace {

constexpr int kChunkT = REGNN_NS_TIDX_CHUNK;
constexpr int kTile = 4 * kBlock;                          // sources per tile of the scan
constexpr int64_t kMaxCap = 0x7ffffffe;                     // int32 ids and slots
constexpr int64_t kMaxPiecesOfRow = 0xffff;                 // the piece word's 16-bit fields

__device__ __forceinline__ bool live_src(int u, int64_t n_src) {
    return u >= 0 && int64_t(u) < n_src;
}

// row v's entries [e0, e1), clamped to the entry capacity
__device__ __forceinline__ void row_range(const int32_t* __restrict__ ptr, int64_t v, int cap_e,
                                          int& e0, int& e1) {
    e0 = max(0, min(ptr[v], cap_e));
    e1 = max(e0, min(ptr[v + 1], cap_e));
}

__global__ void __launch_bounds__(kBlock)
tidx_count_kernel(const int32_t* __restrict__ ptr, const int32_t* __restrict__ idx,
                  int64_t cap_dst, int64_t n_src, int cap_e, int32_t* __restrict__ cnt) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t v = int64_t(blockIdx.x) * (kBlock / 64) + wave; v < cap_dst;
         v += int64_t(gridDim.x) * (kBlock / 64)) {
        int e0, e1;
        row_range(ptr, v, cap_e, e0, e1);
        for (int e = e0 + lane; e < e1; e += 64) {
            const int u = idx[e];
            if (live_src(u, n_src)) atomicAdd(cnt + u, 1);
        }
    }
}

__device__ __forceinline__ int pieces_of(int n) {
    return n > kChunkT ? (n + kChunkT - 1) / kChunkT : 0;
}

// (n, p) summed over the workgroup's threads before this one, and over all of them
__device__ __forceinline__ void block_scan2(int n, int p, int& en, int& ep, int& tn, int& tp) {
    __shared__ int wn[kBlock / 64];
    __shared__ int wp[kBlock / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int in = n, ip = p;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int a = __shfl_up(in, o, 64), b = __shfl_up(ip, o, 64);
        if (lane >= o) {
            in += a;
            ip += b;
        }
    }
    if (lane == 63) {
        wn[wave] = in;
        wp[wave] = ip;
    }
    __syncthreads();
    int bn = 0, bp = 0;
    tn = tp = 0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) {
        if (w < wave) {
            bn += wn[w];
            bp += wp[w];
        }
        tn += wn[w];
        tp += wp[w];
    }
    en = bn + in - n;
    ep = bp + ip - p;
    __syncthreads();                                        // wn / wp may be written again
}

// The scan in three launches over tiles of kTile sources (four consecutive ones per thread): the
// tiles' sums, ONE workgroup scanning those, then each tile again with its offset.
__global__ void __launch_bounds__(kBlock)
tidx_tile_kernel(const int32_t* __restrict__ cnt, int64_t cap_src, int64_t n_tiles,
                 int32_t* __restrict__ tiles) {
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t u0 = tile * kTile + 4 * threadIdx.x;
        int n = 0, p = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = u0 + k < cap_src ? cnt[u0 + k] : 0;
            n += c;
            p += pieces_of(c);
        }
        int en, ep, tn, tp;
        block_scan2(n, p, en, ep, tn, tp);
        if (threadIdx.x == 0) {
            tiles[2 * tile] = tn;
            tiles[2 * tile + 1] = tp;
        }
    }
}

__global__ void __launch_bounds__(kBlock)
tidx_tile_scan_kernel(int32_t* __restrict__ tiles, int64_t n_tiles, int64_t cap_src,
                      int32_t* __restrict__ t_ptr, int32_t* __restrict__ t_long, int max_pieces) {
    int cn = 0, cp = 0;                                     // the tiles before this round
    for (int64_t base = 0; base < n_tiles; base += kBlock) {
        const int64_t i = base + threadIdx.x;
        const int n = i < n_tiles ? tiles[2 * i] : 0, p = i < n_tiles ? tiles[2 * i + 1] : 0;
        int en, ep, tn, tp;
        block_scan2(n, p, en, ep, tn, tp);
        if (i < n_tiles) {
            tiles[2 * i] = cn + en;
            tiles[2 * i + 1] = cp + ep;
        }
        cn += tn;
        cp += tp;
    }
    if (threadIdx.x == 0) {
        t_ptr[cap_src] = cn;
        t_long[0] = min(cp, max_pieces);
        t_long[1] = 0;                                      // the long rows: counted by the emit
        t_long[2] = REGNN_NS_TIDX_CHUNK;
        t_long[3] = 0;
    }
}

__global__ void __launch_bounds__(kBlock)
tidx_emit_kernel(int32_t* __restrict__ cnt, int64_t cap_src, int64_t n_tiles,
                 const int32_t* __restrict__ tiles, int32_t* __restrict__ t_ptr,
                 int32_t* __restrict__ t_long, int max_pieces) {
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t u0 = tile * kTile + 4 * threadIdx.x;
        int c[4], n = 0, p = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            c[k] = u0 + k < cap_src ? cnt[u0 + k] : 0;
            n += c[k];
            p += pieces_of(c[k]);
        }
        int en, ep, tn, tp;
        block_scan2(n, p, en, ep, tn, tp);
        int at = tiles[2 * tile] + en, pc = tiles[2 * tile + 1] + ep, rows = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t u = u0 + k;
            if (u >= cap_src) break;
            t_ptr[u] = at;
            cnt[u] = 0;                                     // the placement's cursor
            const int np = pieces_of(c[k]);
            for (int i = 0; i < np; ++i) {
                if (pc + i >= max_pieces) break;            // (cannot happen: the bound is exact)
                int32_t* q = t_long + 4 + 4 * (pc + i);
                q[0] = int(u);
                q[1] = at + i * kChunkT;
                q[2] = min(kChunkT, c[k] - i * kChunkT);
                q[3] = (i << 16) | np;
            }
            rows += np > 0;
            at += c[k];
            pc += np;
        }
        if (rows) atomicAdd(t_long + 1, rows);              // an integer count: order-free
    }
}

__global__ void __launch_bounds__(kBlock)
tidx_place_kernel(const int32_t* __restrict__ ptr, const int32_t* __restrict__ idx,
                  const int32_t* __restrict__ t_ptr, int64_t cap_dst, int64_t n_src, int cap_e,
                  int32_t* __restrict__ cursor, int32_t* __restrict__ tmp_pos,
                  int32_t* __restrict__ tmp_row) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t v = int64_t(blockIdx.x) * (kBlock / 64) + wave; v < cap_dst;
         v += int64_t(gridDim.x) * (kBlock / 64)) {
        int e0, e1;
        row_range(ptr, v, cap_e, e0, e1);
        for (int e = e0 + lane; e < e1; e += 64) {
            const int u = idx[e];
            if (!live_src(u, n_src)) continue;
            const int s = t_ptr[u] + atomicAdd(cursor + u, 1);
            if (s < 0 || s >= cap_e) continue;              // (a block whose rows overlap)
            tmp_pos[s] = e;
            tmp_row[s] = int(v);
        }
    }
}

// A thread per placed slot: rank = how many of its segment's positions are smaller (the positions
// of a segment are distinct), so the segment comes out ascending whatever order it was placed in.
__global__ void __launch_bounds__(kBlock)
tidx_rank_kernel(const int32_t* __restrict__ idx, const int32_t* __restrict__ t_ptr,
                 const int32_t* __restrict__ tmp_pos, const int32_t* __restrict__ tmp_row,
                 int64_t cap_src, int cap_e, int32_t* __restrict__ t_pos,
                 int32_t* __restrict__ t_row) {
    const int n_live = min(t_ptr[cap_src], cap_e);
    for (int64_t s = int64_t(blockIdx.x) * kBlock + threadIdx.x; s < n_live;
         s += int64_t(gridDim.x) * kBlock) {
        const int e = tmp_pos[s];
        if (e < 0 || e >= cap_e) continue;
        const int u = idx[e];
        if (u < 0 || int64_t(u) >= cap_src) continue;
        const int s0 = t_ptr[u], s1 = min(t_ptr[u + 1], n_live);
        int rank = 0;
        for (int j = s0; j < s1; ++j) rank += tmp_pos[j] < e;
        if (s0 < 0 || s0 + rank >= cap_e) continue;         // (a block whose rows overlap)
        t_pos[s0 + rank] = e;
        t_row[s0 + rank] = tmp_row[s];
    }
}

inline int64_t max_pieces(int64_t cap_e) {
    // a long row holds more than CHUNK entries and its pieces are ceil(n / CHUNK) <= n / CHUNK + 1
    return 2 * (cap_e / kChunkT) + 2;
}

}  // namespace
}  // namespace regnn

using namespace regnn;

extern "C" int64_t regnn_ns_tidx_long_ints(int64_t cap_e) {
    return cap_e < 0 ? 0 : 4 + 4 * max_pieces(cap_e);
}

extern "C" int64_t regnn_ns_tidx_work_ints(int64_t cap_src, int64_t cap_e) {
    // the counts / cursors, the slots as placed (position, row), the scan's tiles (sum, pieces)
    return cap_src < 0 || cap_e < 0 ? 0 : cap_src + 2 * cap_e + 2 * (cap_src / kTile + 1);
}

extern "C" int regnn_ns_block_tidx(const int32_t* ptr, const int32_t* idx, int64_t cap_dst,
                                   int64_t n_src, int64_t cap_src, int64_t cap_e, int32_t* t_ptr,
                                   int32_t* t_pos, int32_t* t_row, int32_t* t_long,
                                   int64_t long_ints, int32_t* work, int64_t work_ints,
                                   hipStream_t stream) {
    if (!ptr || !idx || !t_ptr || !t_pos || !t_row || !t_long || !work || cap_dst < 0 ||
        n_src < 0 || cap_src < 0 || cap_e < 0 || long_ints < 0 || work_ints < 0 || n_src > cap_src)
        return REGNN_EINVAL;
    if (cap_dst > kMaxCap || cap_src > kMaxCap || cap_e > kMaxCap ||
        cap_e / kChunkT + 1 > kMaxPiecesOfRow)
        return REGNN_EUNSUPPORTED;
    if (long_ints < regnn_ns_tidx_long_ints(cap_e) ||
        work_ints < regnn_ns_tidx_work_ints(cap_src, cap_e))
        return REGNN_EUNSUPPORTED;
    int32_t* cnt = work;
    int32_t* tmp_pos = work + cap_src;
    int32_t* tmp_row = tmp_pos + cap_e;
    if (cap_src > 0 && hipMemsetAsync(cnt, 0, size_t(cap_src) * sizeof(int32_t), stream) != hipSuccess)
        return REGNN_ELAUNCH;
    const int rows_grid = grid_for(cap_dst, kBlock / 64);
    if (cap_dst > 0 && cap_e > 0) {
        hipLaunchKernelGGL(tidx_count_kernel, dim3(rows_grid), dim3(kBlock), 0, stream, ptr, idx,
                           cap_dst, n_src, int(cap_e), cnt);
        REGNN_LAUNCH_CHECK();
    }
    const int64_t n_tiles = (cap_src + kTile - 1) / kTile;
    int32_t* tiles = tmp_row + cap_e;
    if (n_tiles > 0) {
        hipLaunchKernelGGL(tidx_tile_kernel, dim3(grid_for(n_tiles, 1)), dim3(kBlock), 0, stream,
                           static_cast<const int32_t*>(cnt), cap_src, n_tiles, tiles);
        REGNN_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(tidx_tile_scan_kernel, dim3(1), dim3(kBlock), 0, stream, tiles, n_tiles,
                       cap_src, t_ptr, t_long, int(max_pieces(cap_e)));
    REGNN_LAUNCH_CHECK();
    if (n_tiles > 0) {
        hipLaunchKernelGGL(tidx_emit_kernel, dim3(grid_for(n_tiles, 1)), dim3(kBlock), 0, stream,
                           cnt, cap_src, n_tiles, static_cast<const int32_t*>(tiles), t_ptr, t_long,
                           int(max_pieces(cap_e)));
        REGNN_LAUNCH_CHECK();
    }
    if (cap_dst == 0 || cap_e == 0) return REGNN_OK;
    hipLaunchKernelGGL(tidx_place_kernel, dim3(rows_grid), dim3(kBlock), 0, stream, ptr, idx,
                       static_cast<const int32_t*>(t_ptr), cap_dst, n_src, int(cap_e), cnt, tmp_pos,
                       tmp_row);
    REGNN_LAUNCH_CHECK();
    hipLaunchKernelGGL(tidx_rank_kernel, dim3(grid_for(cap_e, kBlock)), dim3(kBlock), 0, stream,
                       idx, static_cast<const int32_t*>(t_ptr),
                       static_cast<const int32_t*>(tmp_pos), static_cast<const int32_t*>(tmp_row),
                       cap_src, int(cap_e), t_pos, t_row);
    REGNN_LAUNCH_CHECK();
    return REGNN_OK;
}
