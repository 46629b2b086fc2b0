// A canonical order for a sampled block's transposed index (regnn_ns_hop csc_*: per local source
// u, csc_ent[csc_ptr[u] .. csc_ptr[u+1]) = its edges' target row << 8 | relation). The builds
// place a source's entries in the order an integer atomic cursor hands out, which differs from
// run to run. The fused step's consumer sums exact fixed-point integers over a segment, so it
// does not care; the module path's gather (regnn_ns_spmm_bwd_csc) sums floats in entry order, so
// its gradients differed in their last bits between two runs of one batch. This pass writes every
// segment sorted by entry value into a second buffer: the same index, one order on every run.
#include "regnn_common.h"

namespace regnn {
namespace nscsort {

// One wave per source, grid-stride over the n = sizes[size_idx] live sources. Every entry's
// place is its rank: the entries below it, and its equals before it (a stable rank sort; equal
// entries are interchangeable). Segments of <= 64 entries rank through lane shuffles, longer ones
// (a source cited by many of the batch's targets) by a pass over the segment per entry, each
// lane taking every 64th entry. Out of place: nothing is read that this launch writes.
__global__ void __launch_bounds__(kBlock)
csc_sort_kernel(const int32_t* __restrict__ sizes, int size_idx, const int32_t* __restrict__ ptr,
                const int32_t* __restrict__ ent, int32_t* __restrict__ out, int cap_src,
                int cap_e) {
    const int lane = threadIdx.x & 63;
    const int n = min(sizes[size_idx], cap_src);
    for (int u = (blockIdx.x * kBlock + threadIdx.x) >> 6; u < n;
         u += (gridDim.x * kBlock) >> 6) {
        const int p0 = ptr[u], p1 = ptr[u + 1];
        if (p0 < 0 || p1 > cap_e || p1 <= p0) continue;        // wave-uniform
        const int len = p1 - p0;
        if (len <= 64) {
            const int e = lane < len ? ent[p0 + lane] : 0x7fffffff;
            int rank = 0;
            for (int j = 0; j < len; ++j) {
                const int o = __shfl(e, j, 64);
                rank += (o < e || (o == e && j < lane)) ? 1 : 0;
            }
            if (lane < len) out[p0 + rank] = e;
        } else {
            for (int i = lane; i < len; i += 64) {
                const int e = ent[p0 + i];
                int rank = 0;
                for (int j = 0; j < len; ++j) {
                    const int o = ent[p0 + j];
                    rank += (o < e || (o == e && j < i)) ? 1 : 0;
                }
                out[p0 + rank] = e;
            }
        }
    }
}

}  // namespace nscsort
}  // namespace regnn

using namespace regnn;

extern "C" {

int regnn_ns_csc_sort(const int32_t* sizes, int32_t size_idx, const int32_t* csc_ptr,
                      const int32_t* csc_ent, int32_t* csc_sorted, int32_t cap_src,
                      int32_t cap_e, hipStream_t stream) {
    if (!sizes || !csc_ptr || !csc_ent || !csc_sorted || csc_ent == csc_sorted || size_idx < 0 ||
        size_idx > 15 || cap_src < 0 || cap_e < 0)
        return REGNN_EINVAL;
    if (cap_src == 0 || cap_e == 0) return REGNN_OK;
    const int waves = kBlock / 64;
    int64_t grid = (int64_t(cap_src) + waves - 1) / waves;
    if (grid > kMaxGrid) grid = kMaxGrid;
    hipLaunchKernelGGL(nscsort::csc_sort_kernel, dim3(unsigned(grid)), dim3(kBlock), 0, stream,
                       sizes, size_idx, csc_ptr, csc_ent, csc_sorted, cap_src, cap_e);
    REGNN_LAUNCH_CHECK();
    return REGNN_OK;
}

}  // extern "C"
