// The NS model's per-layer epilogue with BatchNorm (mag/regnn_layers.py:64-65,134-135 with
// --use_bn, then mag/regnn_ns.py:341-343), training mode, over the LIVE rows of a capacity-sized
// sampled block: the counterpart of re_wide.hip's LayerNorm pair.
//
//   a[v] = rs[v] x[v] + bias (+ res[v])                       v < live   (stored centred on row 0)
//   mean_c, var_c over the live rows (biased var for normalising)
//   y[v] = dropout(relu(gamma (a[v] - mean) rsqrt(var + eps) + beta))   v < live;  0 for v >= live
//   running_mean / running_var (unbiased) / num_batches_tracked updated where live >= 2
//
// The live count is a device int32 (null: n) read by every kernel; every grid is sized from n,
// so a captured graph replays with whatever count the sampler wrote. No atomics, the same bits on
// every run:
//   forward   1. bn_part:  a written; per block (count, column mean, column M2 about the block's
//                          own mean: a second pass over the block's rows of a) -> slab row
//             2. bn_merge: the slab rows merged per column in block order (Chan et al.'s
//                          pairwise update: never E[a^2] - mean^2; 8 segments of consecutive
//                          rows, then the segments in order), writes mean / rstd and the
//                          running buffers
//             3. bn_norm:  y; zeros past the live rows
//   backward  1. bn_bpart: per-block column sums of gy' and gy' xhat -> slab row
//             2. bn_bmerge: the slab rows summed in block order -> g_beta | g_gamma
//             3. bn_bwd:   ga = gamma rstd (gy' - g_beta / live - xhat g_gamma / live),
//                          gx = rs ga, gres = ga; zeros past the live rows
// act = 0: the norm alone (no relu, no dropout), for a caller that applies them itself.
// (the conv bias's gradient sum_v ga is exactly 0 under batch norm: the caller returns zeros)
//
// Rows of H fp32, H % 4 == 0, 4 <= H <= 1024. H in {64, 128, 256, 512, 1024}: re_wide.hip's
// (LPR, VPL) tiers. Any other width: the generic tier (LPR = 0), H / 4 lanes per row, one vector
// per lane, the first 256 - 256 % (H / 4) threads of a block active.
#include "re_nsm_common.h"

namespace regnn {
namespace widebn {
using namespace regnn::nsm;

constexpr int kSlabRowsMax = 512;
constexpr int kMergeCols = 64, kMergeSegs = 8;     // the merge launches: 512 threads

struct BnArgs {
    int64_t n; int H;
    const float* x; const float* rs; const float* bias; const float* res;
    const float* gamma; const float* beta;
    const int64_t* state; int layer; Drop drop;
    bool relu;                                         // act: relu (and dropout) after the norm
    float* a; float* stats; float* y;                  // forward outputs (stats [2][H]: mean, rstd)
    const float* a_in; const float* stats_in;          // backward inputs
    const float* gy; float* gx; float* gres;           // backward
    float* slab; int slab_rows; float* sums;           // sums [2][H]: g_beta, g_gamma
    float* rmean; float* rvar; int64_t* nbt; float eps, mom;
    const int32_t* live;                               // the live row count (may be null: n)
};

__device__ __forceinline__ int64_t bn_rows(const BnArgs& A) {
    return A.live ? max(int64_t(0), min(A.n, int64_t(*A.live))) : A.n;
}

// a thread's place: lane l of row group g; the generic tier (LPR 0) sizes both from H
template <int LPR>
struct Geo {
    int lpr, rpb, l, g;
    bool on;
    __device__ __forceinline__ explicit Geo(int H) {
        lpr = LPR ? LPR : H / 4;
        const int act = LPR ? kBlock : kBlock - kBlock % lpr;
        rpb = act / lpr;
        on = int(threadIdx.x) < act;
        l = threadIdx.x % lpr;
        g = threadIdx.x / lpr;
    }
};

__device__ __forceinline__ void drop4(uint32_t key, const Drop& d, int64_t row, int nvec, int vec,
                                      float (&m)[4]) {
    m[0] = m[1] = m[2] = m[3] = 1.f;
    if (!d.on) return;
    if (d.b8) drop_apply<4, 8>(key, d.thresh, d.scale, row, nvec, vec, m);
    else drop_apply<4, 16>(key, d.thresh, d.scale, row, nvec, vec, m);
}

__device__ __forceinline__ void ld4(const float* p, float (&v)[4]) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}

__device__ __forceinline__ void st4(float* p, const float (&v)[4]) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}

// The rows are stored centred on row 0 (the "pivot", per column): a[v] = (rs[v] x[v] + res[v]) -
// (rs[0] x[0] + res[0]), the difference formed in fp64 and rounded once, and so is the mean in
// stats. Column means far from 0 (|mean| >> std) then cost no precision: a, the mean and xhat
// carry rounding errors relative to the spread of a column, not to its offset.
__device__ __forceinline__ double bn_pivot(float rs0, float x0, float b, float r0) {
    return fma(double(rs0), double(x0), double(b) + double(r0));
}

// forward 1: a, and this block's (count, mean, M2) per column. slab row: [H mean | H M2 | count]
template <int LPR, int VPL>
__global__ void __launch_bounds__(kBlock) bn_part_kernel(BnArgs A) {
    __shared__ float red[1024 * VPL];                  // [rpb][H] row-group partials
    __shared__ float bmean[256 * 4 * VPL];             // the block's column means (>= H floats)
    __shared__ int cnts[kBlock];
    const Geo<LPR> G(A.H);
    const int H = A.H;
    const int64_t n = bn_rows(A);
    const int64_t step = int64_t(gridDim.x) * G.rpb;
    float s[VPL][4];
    double sh[VPL][4];                                 // bias - pivot (row 0 of rs x + bias + res)
#pragma unroll
    for (int j = 0; j < VPL; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k) s[j][k] = 0.f;
    int cnt = 0;
    if (G.on) {
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
            const int c = 4 * (G.l + G.lpr * j);
            float x0[4], r0[4] = {0.f, 0.f, 0.f, 0.f};
            ld4(A.x + c, x0);
            if (A.res) ld4(A.res + c, r0);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                sh[j][k] = -bn_pivot(A.rs ? A.rs[0] : 1.f, x0[k], 0.f, r0[k]);
        }
        for (int64_t v = int64_t(blockIdx.x) * G.rpb + G.g; v < n; v += step) {
            const float sc = A.rs ? A.rs[v] : 1.f;
#pragma unroll
            for (int j = 0; j < VPL; ++j) {
                const int c = 4 * (G.l + G.lpr * j);
                float x[4], r[4] = {0.f, 0.f, 0.f, 0.f}, a[4];
                ld4(A.x + v * H + c, x);
                if (A.res) ld4(A.res + v * H + c, r);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    // (the bias cancels against the pivot's: it moves no centred value)
                    a[k] = float(fma(double(sc), double(x[k]), double(r[k]) + sh[j][k]));
                    s[j][k] += a[k];
                }
                st4(A.a + v * H + c, a);
            }
            ++cnt;
        }
#pragma unroll
        for (int j = 0; j < VPL; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) red[G.g * H + 4 * (G.l + G.lpr * j) + k] = s[j][k];
        if (G.l == 0) cnts[G.g] = cnt;
    }
    __syncthreads();
    int bcnt = 0;
    for (int r = 0; r < G.rpb; ++r) bcnt += cnts[r];
    float* row = A.slab + int64_t(blockIdx.x) * 3 * H;
    for (int e = threadIdx.x; e < H; e += kBlock) {
        float t = 0.f;
        for (int r = 0; r < G.rpb; ++r) t += red[r * H + e];          // group order
        const float m = bcnt > 0 ? t / float(bcnt) : 0.f;
        bmean[e] = m;
        row[e] = m;
    }
    if (threadIdx.x == 0) row[2 * H] = float(bcnt);
    __syncthreads();
    // the squares about the block's own mean: every thread reads back the elements it wrote
    if (G.on) {
        float bm[VPL][4];
#pragma unroll
        for (int j = 0; j < VPL; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                bm[j][k] = bmean[4 * (G.l + G.lpr * j) + k];
                s[j][k] = 0.f;
            }
        for (int64_t v = int64_t(blockIdx.x) * G.rpb + G.g; v < n; v += step) {
#pragma unroll
            for (int j = 0; j < VPL; ++j) {
                float a[4];
                ld4(A.a + v * H + 4 * (G.l + G.lpr * j), a);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float d = a[k] - bm[j][k];
                    s[j][k] = fmaf(d, d, s[j][k]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < VPL; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) red[G.g * H + 4 * (G.l + G.lpr * j) + k] = s[j][k];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < H; e += kBlock) {
        float t = 0.f;
        for (int r = 0; r < G.rpb; ++r) t += red[r * H + e];
        row[H + e] = t;
    }
}

// One Chan et al. update: (N, mean, M2) <- (N, mean, M2) + (nb, mb, qb); an empty part changes
// nothing. (nb / Nn by the fast reciprocal: a weight in [0, 1] with ~1 ulp of error)
__device__ __forceinline__ void chan(float& N, float& mean, float& M2, float nb, float mb,
                                     float qb) {
    if (nb > 0.f) {
        const float Nn = N + nb, d = mb - mean, w = __fdividef(nb, Nn);
        mean = fmaf(d, w, mean);
        M2 += qb + d * d * (N * w);
        N = Nn;
    }
}

// forward 2: the slab rows merged in block order, in a fixed two-level shape: thread (column,
// segment) merges its segment of consecutive slab rows in order, then segment 0's thread merges
// the kMergeSegs segment results in segment order (one sequential chain over 512 rows is ~8x the
// latency of this)
__global__ void __launch_bounds__(kMergeCols * kMergeSegs) bn_merge_kernel(BnArgs A) {
    __shared__ float sN[kMergeSegs][kMergeCols], sM[kMergeSegs][kMergeCols],
        sQ[kMergeSegs][kMergeCols];
    const int tc = threadIdx.x % kMergeCols, sg = threadIdx.x / kMergeCols;
    const int c = blockIdx.x * kMergeCols + tc;
    const int H = A.H;
    const int per = (A.slab_rows + kMergeSegs - 1) / kMergeSegs;
    const int b0 = min(sg * per, A.slab_rows), b1 = min(b0 + per, A.slab_rows);
    float N = 0.f, mean = 0.f, M2 = 0.f;
    if (c < H) {
        int b = b0;
        for (; b + 4 <= b1; b += 4) {                  // four rows' loads in flight
            float nb[4], mb[4], qb[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float* row = A.slab + int64_t(b + u) * 3 * H;
                nb[u] = row[2 * H]; mb[u] = row[c]; qb[u] = row[H + c];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) chan(N, mean, M2, nb[u], mb[u], qb[u]);
        }
        for (; b < b1; ++b) {
            const float* row = A.slab + int64_t(b) * 3 * H;
            chan(N, mean, M2, row[2 * H], row[c], row[H + c]);
        }
    }
    sN[sg][tc] = N; sM[sg][tc] = mean; sQ[sg][tc] = M2;
    __syncthreads();
    if (sg != 0 || c >= H) return;
    for (int q = 1; q < kMergeSegs; ++q) chan(N, mean, M2, sN[q][tc], sM[q][tc], sQ[q][tc]);
    // fewer than 2 live rows: the variance is defined as 0 and the running buffers stay
    const float var = N >= 2.f ? M2 / N : 0.f;
    A.stats[c] = mean;                                 // relative to the pivot, as a is
    A.stats[H + c] = rsqrtf(var + A.eps);
    if (N >= 2.f) {
        const double pv = bn_pivot(A.rs ? A.rs[0] : 1.f, A.x[c], A.bias ? A.bias[c] : 0.f,
                                   A.res ? A.res[c] : 0.f);
        A.rmean[c] = (1.f - A.mom) * A.rmean[c] + A.mom * float(pv + double(mean));
        A.rvar[c] = (1.f - A.mom) * A.rvar[c] + A.mom * (M2 / (N - 1.f));
        if (c == 0 && A.nbt) A.nbt[0] += 1;
    }
}

// the pre-activation of one element, formed the same way forward and backward (its sign is the
// relu's mask)
__device__ __forceinline__ float bn_pre(float a, float mean, float rstd, float gw, float gb,
                                        float& xh) {
    xh = (a - mean) * rstd;
    return fmaf(xh, gw, gb);
}

template <int LPR, int VPL>
struct Cols {                                          // a thread's per-column constants
    float mean[VPL][4], rstd[VPL][4], gw[VPL][4], gb[VPL][4];
    __device__ __forceinline__ void load(const Geo<LPR>& G, const float* stats, const float* gamma,
                                         const float* beta, int H) {
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
            const int c = 4 * (G.l + G.lpr * j);
            ld4(stats + c, mean[j]);
            ld4(stats + H + c, rstd[j]);
            ld4(gamma + c, gw[j]);
            ld4(beta + c, gb[j]);
        }
    }
};

// forward 3: y over the live rows, zeros past them
template <int LPR, int VPL>
__global__ void __launch_bounds__(kBlock) bn_norm_kernel(BnArgs A) {
    const Geo<LPR> G(A.H);
    if (!G.on) return;
    const int H = A.H, nvec = H / 4;
    const uint32_t key = A.drop.on ? layer_key(A.state, A.layer) : 0u;
    Cols<LPR, VPL> C;
    C.load(G, A.stats, A.gamma, A.beta, H);
    const int64_t n = bn_rows(A);
    const int64_t step = int64_t(gridDim.x) * G.rpb;
    for (int64_t v = int64_t(blockIdx.x) * G.rpb + G.g; v < A.n; v += step) {
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
            const int vec = G.l + G.lpr * j;
            float o[4] = {0.f, 0.f, 0.f, 0.f};
            if (v < n) {
                float a[4], m[4];
                ld4(A.a + v * H + 4 * vec, a);
                drop4(key, A.drop, v, nvec, vec, m);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float xh;
                    const float yv = bn_pre(a[k], C.mean[j][k], C.rstd[j][k], C.gw[j][k], C.gb[j][k], xh);
                    o[k] = (A.relu ? fmaxf(yv, 0.f) : yv) * m[k];
                }
            }
            st4(A.y + v * H + 4 * vec, o);
        }
    }
}

// backward 1: slab row per block: [H sum gy' | H sum gy' xhat | unused]
template <int LPR, int VPL>
__global__ void __launch_bounds__(kBlock) bn_bpart_kernel(BnArgs A) {
    __shared__ float red[2 * 1024 * VPL];              // [rpb][2 H]
    const Geo<LPR> G(A.H);
    const int H = A.H, nvec = H / 4;
    const uint32_t key = A.drop.on ? layer_key(A.state, A.layer) : 0u;
    const int64_t n = bn_rows(A);
    const int64_t step = int64_t(gridDim.x) * G.rpb;
    if (G.on) {
        Cols<LPR, VPL> C;
        C.load(G, A.stats_in, A.gamma, A.beta, H);
        float pb[VPL][4], pw[VPL][4];
#pragma unroll
        for (int j = 0; j < VPL; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) pb[j][k] = pw[j][k] = 0.f;
        for (int64_t v = int64_t(blockIdx.x) * G.rpb + G.g; v < n; v += step) {
#pragma unroll
            for (int j = 0; j < VPL; ++j) {
                const int vec = G.l + G.lpr * j;
                float a[4], g[4], m[4];
                ld4(A.a_in + v * H + 4 * vec, a);
                ld4(A.gy + v * H + 4 * vec, g);
                drop4(key, A.drop, v, nvec, vec, m);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float xh;
                    const float yv = bn_pre(a[k], C.mean[j][k], C.rstd[j][k], C.gw[j][k], C.gb[j][k], xh);
                    const float gyv = (yv > 0.f || !A.relu) ? g[k] * m[k] : 0.f;
                    pb[j][k] += gyv;
                    pw[j][k] = fmaf(gyv, xh, pw[j][k]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < VPL; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int c = 4 * (G.l + G.lpr * j) + k;
                red[G.g * 2 * H + c] = pb[j][k];
                red[G.g * 2 * H + H + c] = pw[j][k];
            }
    }
    __syncthreads();
    float* row = A.slab + int64_t(blockIdx.x) * 3 * H;
    for (int e = threadIdx.x; e < 2 * H; e += kBlock) {
        float t = 0.f;
        for (int r = 0; r < G.rpb; ++r) t += red[r * 2 * H + e];      // group order
        row[e] = t;
    }
}

// backward 2: sums[e] = sum over the slab rows, e < 2 H, in bn_merge's fixed two-level order
__global__ void __launch_bounds__(kMergeCols * kMergeSegs) bn_bmerge_kernel(BnArgs A) {
    __shared__ float sT[kMergeSegs][kMergeCols];
    const int tc = threadIdx.x % kMergeCols, sg = threadIdx.x / kMergeCols;
    const int e = blockIdx.x * kMergeCols + tc;
    const int H = A.H;
    const int per = (A.slab_rows + kMergeSegs - 1) / kMergeSegs;
    const int b0 = min(sg * per, A.slab_rows), b1 = min(b0 + per, A.slab_rows);
    float t = 0.f;
    if (e < 2 * H) {
#pragma unroll 8
        for (int b = b0; b < b1; ++b) t += A.slab[int64_t(b) * 3 * H + e];
    }
    sT[sg][tc] = t;
    __syncthreads();
    if (sg != 0 || e >= 2 * H) return;
    for (int q = 1; q < kMergeSegs; ++q) t += sT[q][tc];
    A.sums[e] = t;
}

// backward 3: ga; gx = rs ga, gres = ga over the live rows, zeros past them
template <int LPR, int VPL>
__global__ void __launch_bounds__(kBlock) bn_bwd_kernel(BnArgs A) {
    const Geo<LPR> G(A.H);
    if (!G.on) return;
    const int H = A.H, nvec = H / 4;
    const uint32_t key = A.drop.on ? layer_key(A.state, A.layer) : 0u;
    Cols<LPR, VPL> C;
    C.load(G, A.stats_in, A.gamma, A.beta, H);
    const int64_t n = bn_rows(A);
    const float inv = n > 0 ? 1.f / float(n) : 0.f;
    float mb[VPL][4], mw[VPL][4];                      // g_beta / live, g_gamma / live
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        const int c = 4 * (G.l + G.lpr * j);
        ld4(A.sums + c, mb[j]);
        ld4(A.sums + H + c, mw[j]);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            mb[j][k] *= inv;
            mw[j][k] *= inv;
        }
    }
    const int64_t step = int64_t(gridDim.x) * G.rpb;
    for (int64_t v = int64_t(blockIdx.x) * G.rpb + G.g; v < A.n; v += step) {
        const bool lv = v < n;
        const float sc = (lv && A.rs) ? A.rs[v] : 1.f;
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
            const int vec = G.l + G.lpr * j;
            float ga[4] = {0.f, 0.f, 0.f, 0.f}, gx[4] = {0.f, 0.f, 0.f, 0.f};
            if (lv) {
                float a[4], g[4], m[4];
                ld4(A.a_in + v * H + 4 * vec, a);
                ld4(A.gy + v * H + 4 * vec, g);
                drop4(key, A.drop, v, nvec, vec, m);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float xh;
                    const float yv = bn_pre(a[k], C.mean[j][k], C.rstd[j][k], C.gw[j][k], C.gb[j][k], xh);
                    const float gyv = (yv > 0.f || !A.relu) ? g[k] * m[k] : 0.f;
                    ga[k] = C.gw[j][k] * C.rstd[j][k] * (gyv - mb[j][k] - xh * mw[j][k]);
                    gx[k] = sc * ga[k];
                }
            }
            st4(A.gx + v * H + 4 * vec, gx);
            if (A.gres) st4(A.gres + v * H + 4 * vec, ga);
        }
    }
}

}  // namespace widebn
}  // namespace regnn

using namespace regnn;
using namespace regnn::widebn;

namespace {

bool bn_width_ok(int H) { return H >= 4 && H <= 1024 && H % 4 == 0; }

bool bn_tier(int H) { return H == 64 || H == 128 || H == 256 || H == 512 || H == 1024; }

// rows per block of the row kernels
int bn_rpb(int H) {
    if (bn_tier(H)) return kBlock / (H >= 256 ? 64 : H / 4);
    const int lpr = H / 4;
    return (kBlock - kBlock % lpr) / lpr;
}

enum BnKernel { kPart, kNorm, kBPart, kBwd };

template <int LPR, int VPL>
void bn_launch_t(BnKernel which, const BnArgs& A, int blocks, hipStream_t stream) {
    switch (which) {
    case kPart:
        hipLaunchKernelGGL((bn_part_kernel<LPR, VPL>), dim3(blocks), dim3(kBlock), 0, stream, A);
        break;
    case kNorm:
        hipLaunchKernelGGL((bn_norm_kernel<LPR, VPL>), dim3(blocks), dim3(kBlock), 0, stream, A);
        break;
    case kBPart:
        hipLaunchKernelGGL((bn_bpart_kernel<LPR, VPL>), dim3(blocks), dim3(kBlock), 0, stream, A);
        break;
    case kBwd:
        hipLaunchKernelGGL((bn_bwd_kernel<LPR, VPL>), dim3(blocks), dim3(kBlock), 0, stream, A);
        break;
    }
}

int bn_launch(BnKernel which, const BnArgs& A, int blocks, hipStream_t stream) {
    switch (A.H) {
    case 64: bn_launch_t<16, 1>(which, A, blocks, stream); break;
    case 128: bn_launch_t<32, 1>(which, A, blocks, stream); break;
    case 256: bn_launch_t<64, 1>(which, A, blocks, stream); break;
    case 512: bn_launch_t<64, 2>(which, A, blocks, stream); break;
    case 1024: bn_launch_t<64, 4>(which, A, blocks, stream); break;
    default: bn_launch_t<0, 1>(which, A, blocks, stream); break;
    }
    REGNN_LAUNCH_CHECK();
    return REGNN_OK;
}

int bn_row_grid(int64_t n, int H) {
    const int rpb = bn_rpb(H);
    int64_t blocks = (n + rpb - 1) / rpb;
    if (blocks > kMaxGrid) blocks = kMaxGrid;
    return int(blocks < 1 ? 1 : blocks);
}

bool aligned(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

}  // namespace

extern "C" {

int64_t regnn_wide_bn_slab_rows(int64_t n, int32_t H) {
    if (!bn_width_ok(H)) return 1;
    const int rpb = bn_rpb(H);
    int64_t blocks = (n + rpb - 1) / rpb;
    if (blocks > kSlabRowsMax) blocks = kSlabRowsMax;
    return blocks < 1 ? 1 : blocks;
}

int regnn_wide_bn_fwd(int64_t n, int32_t H, const float* x, const float* rs, const float* bias,
                      const float* res, const float* gamma, const float* beta,
                      const int64_t* state, int32_t layer, float p_drop, float* a, float* stats,
                      float* y, float* slab, const int32_t* live, float* running_mean,
                      float* running_var, int64_t* num_batches_tracked, float eps, float momentum,
                      int32_t act, hipStream_t stream) {
    if (n < 0 || !x || !gamma || !beta || !a || !stats || !y || !slab || !running_mean ||
        !running_var || !(p_drop >= 0.f && p_drop < 1.f) || (p_drop > 0.f && !state) ||
        !(eps > 0.f) || !(momentum >= 0.f && momentum <= 1.f) || (!act && p_drop > 0.f))
        return REGNN_EINVAL;
    if (!bn_width_ok(H)) return REGNN_EUNSUPPORTED;
    if (n == 0) return REGNN_OK;
    if (!aligned(x) || !aligned(a) || !aligned(y) || !aligned(stats) || (res && !aligned(res)) ||
        (bias && !aligned(bias)) || !aligned(gamma) || !aligned(beta))
        return REGNN_EUNSUPPORTED;
    BnArgs A{};
    A.n = n; A.H = H; A.x = x; A.rs = rs; A.bias = bias; A.res = res; A.gamma = gamma; A.beta = beta;
    A.state = state; A.layer = layer; A.drop = make_drop(p_drop);
    A.a = a; A.stats = stats; A.y = y; A.slab = slab; A.live = live;
    A.slab_rows = int(regnn_wide_bn_slab_rows(n, H));
    A.rmean = running_mean; A.rvar = running_var; A.nbt = num_batches_tracked;
    A.eps = eps; A.mom = momentum; A.relu = act != 0;
    int rc = bn_launch(kPart, A, A.slab_rows, stream);
    if (rc != REGNN_OK) return rc;
    hipLaunchKernelGGL(bn_merge_kernel, dim3((H + kMergeCols - 1) / kMergeCols),
                       dim3(kMergeCols * kMergeSegs),
                       0, stream, A);
    REGNN_LAUNCH_CHECK();
    return bn_launch(kNorm, A, bn_row_grid(n, H), stream);
}

int regnn_wide_bn_bwd(int64_t n, int32_t H, const float* gy, const float* a, const float* stats,
                      const float* rs, const float* gamma, const float* beta,
                      const int64_t* state, int32_t layer, float p_drop, float* gx, float* gres,
                      float* slab, float* sums, const int32_t* live, int32_t act,
                      hipStream_t stream) {
    if (n < 0 || !gy || !a || !stats || !gamma || !beta || !gx || !slab || !sums ||
        !(p_drop >= 0.f && p_drop < 1.f) || (p_drop > 0.f && !state) || (!act && p_drop > 0.f))
        return REGNN_EINVAL;
    if (!bn_width_ok(H)) return REGNN_EUNSUPPORTED;
    if (!aligned(gy) || !aligned(a) || !aligned(gx) || !aligned(stats) || !aligned(sums) ||
        (gres && !aligned(gres)) || !aligned(gamma) || !aligned(beta))
        return REGNN_EUNSUPPORTED;
    BnArgs A{};
    A.n = n; A.H = H; A.gy = gy; A.a_in = a; A.stats_in = stats; A.rs = rs; A.gamma = gamma;
    A.beta = beta; A.state = state; A.layer = layer; A.drop = make_drop(p_drop);
    A.gx = gx; A.gres = gres; A.slab = slab; A.sums = sums; A.live = live; A.relu = act != 0;
    A.slab_rows = int(regnn_wide_bn_slab_rows(n, H));
    if (n == 0) A.slab_rows = 0;                       // no rows: zero sums, nothing else to write
    else if (int rc = bn_launch(kBPart, A, A.slab_rows, stream); rc != REGNN_OK) return rc;
    hipLaunchKernelGGL(bn_bmerge_kernel, dim3((2 * H + kMergeCols - 1) / kMergeCols),
                       dim3(kMergeCols * kMergeSegs), 0, stream, A);
    REGNN_LAUNCH_CHECK();
    return n == 0 ? REGNN_OK : bn_launch(kBwd, A, bn_row_grid(n, H), stream);
}

}  // extern "C"
