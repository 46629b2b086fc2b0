// Host build of the thread-per-(destination, head) GAT kernels of re_gat.hip (head counts that
// are no power of two <= 32): gat_softmax_fwd_generic, gat_softmax_bwd_generic and
// segment_sum_generic, for test_cpu_gat_generic_host.py. The kernels' own source text (cut out of
// re_gat.hip into gat_generic_kernels.inc, the LDS declaration replaced by the global `bins`)
// runs with one std::thread per GPU thread of a block and a std::barrier as __syncthreads; the
// blocks of the grid run one after another. Outputs are compared with a direct double-precision
// computation: the attention a per edge; gs per edge, ger per (destination, head) and the
// relation table's gradient summed over the slab rows; the permuted segment sums. The grid is
// capped low so that the grid-stride loops run. Exit status 0 = every case matches.
#include <algorithm>
#include <barrier>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <thread>
#include <vector>

constexpr int kBlock = 256;
struct Dim { int x; };
static thread_local Dim threadIdx;
static Dim blockIdx, gridDim;
static std::barrier<>* g_barrier;
static float* bins;                       // the block's LDS: [n_rel][kBlock]
#define __global__
#define __host__
#define __device__
#define __launch_bounds__(x)
#define __restrict__
#define __syncthreads() g_barrier->arrive_and_wait()
#define __expf expf
static inline float lrelu(float x, float slope) { return x > 0.f ? x : x * slope; }
#include "gat_generic_kernels.inc"

// run `kernel` (a callable without arguments) as `grid` blocks of kBlock threads
template <typename K>
static void launch(int grid, K kernel) {
    gridDim.x = grid;
    for (int b = 0; b < grid; ++b) {
        blockIdx.x = b;
        std::barrier<> bar(kBlock);
        g_barrier = &bar;
        std::vector<std::thread> threads;
        for (int t = 0; t < kBlock; ++t)
            threads.emplace_back([&, t] {
                threadIdx.x = t;
                kernel();
            });
        for (auto& t : threads) t.join();
    }
}

static int capped_grid(int64_t units, int per_block, int cap) {
    int64_t g = (units + per_block - 1) / per_block;
    if (g < 1) g = 1;
    return int(g < cap ? g : cap);
}

struct Case { int n_seg, H, n_rel, grid_cap; };

int main() {
    std::mt19937 rng(1);
    const float slope = 0.2f;
    // H = 3, 5, 6, 12: 256 % H != 0 (the refusal this kernel had); 64: divides the block;
    // 300: wider than the block (no slab); n_rel = 64: the LDS limit; grid 1: one block strides
    for (Case c : {Case{700, 3, 7, 4}, Case{500, 5, 7, 3}, Case{300, 12, 64, 2}, Case{100, 6, 1, 100},
                   Case{64, 12, 7, 1}, Case{40, 64, 3, 2}, Case{10, 300, 2, 2}, Case{1, 3, 2, 5}}) {
        const int H = c.H, n_rel = c.n_rel;
        std::vector<int32_t> ptr(c.n_seg + 1, 0);
        for (int v = 0; v < c.n_seg; ++v) ptr[v + 1] = ptr[v] + int(rng() % 9);   // degree 0..8
        const int E = ptr.back();
        std::vector<int32_t> idx(E);
        std::vector<uint8_t> rel(E);
        for (int k = 0; k < E; ++k) {
            idx[k] = int32_t(rng() % c.n_seg);
            rel[k] = uint8_t(rng() % n_rel);
        }
        auto rnd = [&](size_t n) {
            std::vector<float> v(n);
            for (auto& x : v) x = (int(rng() % 2001) - 1000) / 1000.f;
            return v;
        };
        auto ee = rnd(size_t(n_rel) * H), el = rnd(size_t(c.n_seg) * H), er = rnd(size_t(c.n_seg) * H);
        auto ga = rnd(size_t(E) * H);
        const int64_t total = int64_t(c.n_seg) * H;
        // forward: a = softmax over each destination's in-edges, as regnn_gat_softmax_fwd launches
        std::vector<float> a(size_t(E) * H, NAN);
        launch(capped_grid(total, kBlock, c.grid_cap), [&] {
            gat_softmax_fwd_generic(ptr.data(), idx.data(), rel.data(), ee.data(), el.data(),
                                    er.data(), c.n_seg, H, slope, a.data());
        });
        double worst_a = 0.0;
        for (int v = 0; v < c.n_seg; ++v)
            for (int h = 0; h < H; ++h) {
                double m = -INFINITY, sum = 0.0;
                std::vector<double> z;
                for (int k = ptr[v]; k < ptr[v + 1]; ++k) {
                    float sc = el[size_t(idx[k]) * H + h] + er[size_t(v) * H + h];
                    sc += ee[rel[k] * H + h];
                    z.push_back(lrelu(sc, slope));
                    m = std::fmax(m, z.back());
                }
                for (double x : z) sum += std::exp(x - m);
                for (int k = ptr[v]; k < ptr[v + 1]; ++k)
                    worst_a = std::fmax(worst_a, std::fabs(std::exp(z[k - ptr[v]] - m) / sum -
                                                           a[size_t(k) * H + h]));
            }
        // backward, as regnn_gat_softmax_bwd launches it
        const bool use_slab = H <= kBlock;
        const int act = gat_generic_act(H);
        const int grid = capped_grid(total, act, c.grid_cap);
        std::vector<float> gs(size_t(E) * H, NAN), ger(size_t(c.n_seg) * H, NAN);
        std::vector<float> slab(size_t(grid) * n_rel * H, NAN), lds(size_t(n_rel) * kBlock, NAN);
        bins = lds.data();
        launch(grid, [&] {
            gat_softmax_bwd_generic(ptr.data(), idx.data(), rel.data(), ee.data(), el.data(),
                                    er.data(), a.data(), ga.data(), c.n_seg, H, slope, gs.data(),
                                    ger.data(), use_slab ? slab.data() : nullptr, n_rel);
        });
        // segment sums of permuted rows (the backward's d el over the transposed index)
        std::vector<int32_t> perm(E);
        for (int k = 0; k < E; ++k) perm[k] = k;
        std::shuffle(perm.begin(), perm.end(), rng);
        std::vector<float> ssum(size_t(c.n_seg) * H, NAN);
        launch(capped_grid(total, kBlock, c.grid_cap), [&] {
            segment_sum_generic(ptr.data(), perm.data(), ga.data(), c.n_seg, H, ssum.data());
        });
        double worst_sum = 0.0;
        for (int v = 0; v < c.n_seg; ++v)
            for (int h = 0; h < H; ++h) {
                double acc = 0.0;
                for (int k = ptr[v]; k < ptr[v + 1]; ++k) acc += ga[size_t(perm[k]) * H + h];
                worst_sum = std::fmax(worst_sum, std::fabs(acc - ssum[size_t(v) * H + h]));
            }
        double worst = 0.0, worst_tab = 0.0;
        std::vector<double> tab(size_t(n_rel) * H, 0.0);
        for (int v = 0; v < c.n_seg; ++v)
            for (int h = 0; h < H; ++h) {
                double dot = 0.0, gsum = 0.0;
                for (int k = ptr[v]; k < ptr[v + 1]; ++k)
                    dot += double(a[size_t(k) * H + h]) * ga[size_t(k) * H + h];
                for (int k = ptr[v]; k < ptr[v + 1]; ++k) {
                    float s = el[size_t(idx[k]) * H + h] + er[size_t(v) * H + h];
                    s += ee[rel[k] * H + h];            // the score's sign as the kernel's fp32 takes it
                    double gz = a[size_t(k) * H + h] * (ga[size_t(k) * H + h] - dot);
                    if (!(s > 0.f)) gz *= slope;
                    worst = std::fmax(worst, std::fabs(gz - gs[size_t(k) * H + h]));
                    gsum += gz;
                    tab[rel[k] * H + h] += gz;
                }
                worst = std::fmax(worst, std::fabs(gsum - ger[size_t(v) * H + h]));
            }
        if (use_slab)
            for (int i = 0; i < n_rel * H; ++i) {
                double s = 0.0;
                for (int b = 0; b < grid; ++b) s += slab[size_t(b) * n_rel * H + i];
                worst_tab = std::fmax(worst_tab, std::fabs(s - tab[i]));
            }
        std::printf("n_seg %d H %d n_rel %d grid %d: a err %.2e  gs/ger err %.2e  g_tab err %.2e  "
                    "segment sum err %.2e\n", c.n_seg, H, n_rel, grid, worst_a, worst, worst_tab,
                    worst_sum);
        // a <= 1, |ga| <= 1, degree <= 8: |gz| <= 2, sums of <= 8 (ger, segment sums) or a few
        // thousand (g_tab) such terms; fp32 against double leaves ~1e-6 and ~1e-5. A wrong head
        // or a lost or doubled term is an error of order 0.1 to 1. NaN (an unwritten output)
        // fails the comparison.
        if (!(worst_a < 1e-5) || !(worst < 1e-4) || !(worst_tab < 1e-3) || !(worst_sum < 1e-4)) {
            std::puts("MISMATCH");
            return 1;
        }
    }
    std::puts("ok");
    return 0;
}
