// kernels_norm.hip -- per-unit norms of the difference of two grids
// (stencil_diff_norms, the convergence check of stencil_iterate_until;
// DESIGN.md §5.6).  No reference counterpart: the reference runs a fixed
// number of sweeps (src/stencil/stencil.cpp:23-57).
//
// For every slow-axis unit u in [begin, end) (a plane in 3D, a row in 2D):
//   max_abs[u] = max |d|,  sum_sq[u] = sum d*d,  d = double(a) - double(b)
// over the unit's interior cells.  A streaming read of both grids:
//
//  * Mapping.  The 256 lanes of a workgroup form LX x RY with LX = the power
//    of two that covers a row's 16-B vectors (at most 256) and RY = 256 / LX
//    rows.  A "trip" is one 16-B load per lane and grid: RY rows x LX vectors.
//    A unit is nrow_iters x nx_iters trips (row groups outer, x inner), cut
//    into `chunks` contiguous runs of trips, one workgroup per run.  A lane
//    issues 4 trips' loads from both grids (8 x 16 B in flight) before it
//    uses the first.  Interior x = 0 of every row is 128-B aligned and the
//    pitch a multiple of 128 B, so every vector is aligned and
//    inside its row; the lanes of the vector that holds the row's end mask
//    x >= nx.  Ghost cells, row padding and the tail pad are never loaded
//    into the result.  Plain loads: the next sweep reads both grids again.
//  * Determinism.  LX, RY, the trips and the chunks depend on the layout
//    alone; a lane adds its cells in trip order, the wave combines by a fixed
//    xor-shuffle tree, the four waves through LDS in wave order, and a second
//    tiny launch combines a unit's chunk partials in ascending chunk order.
//    No atomics, no hand-off between workgroups, nothing that depends on the
//    CU count, the stream or timing: equal grids give equal bits.
//  * NaN.  Max drops NaNs (v_max_f64), the sum does not, and a sum of squares
//    (terms >= 0 or +inf) is NaN only if some d is: the combine launch sets
//    both outputs of a unit to NaN when its sum is NaN.
#include <cmath>
#include <limits>

#include "common.hpp"

namespace stencil {
namespace {

typedef float norm_f32x4 __attribute__((ext_vector_type(4)));
typedef double norm_f64x2 __attribute__((ext_vector_type(2)));
template <typename T>
struct VecOf;
template <>
struct VecOf<float> {
    typedef norm_f32x4 type;
};
template <>
struct VecOf<double> {
    typedef norm_f64x2 type;
};

constexpr int kNormThreads = 256;
constexpr int kNormUnroll = 4;        // trips whose loads a lane has in flight
constexpr int64_t kNormChunkTrips = 16;  // trips per workgroup aimed at ...
constexpr int kNormMaxChunks = 32;       // ... up to this many chunks per unit
constexpr int64_t kNormMaxBlocks = int64_t(1) << 22;  // workgroups per launch

struct NormPlan {
    int lx_log2;         // lanes along x = 1 << lx_log2
    int nx_iters;        // trips along x per row group
    int64_t nrow_iters;  // row groups of RY rows per unit
    int chunks;          // workgroups (partials) per unit
};

NormPlan norm_plan(const stencil_layout& l) {
    const int64_t vw = l.prob.dtype == STENCIL_F32 ? 4 : 2;
    const int64_t vpr = (l.prob.nx + vw - 1) / vw;  // 16-B vectors per row
    NormPlan p{};
    while (p.lx_log2 < 8 && (int64_t(1) << p.lx_log2) < vpr) ++p.lx_log2;
    const int64_t lx = int64_t(1) << p.lx_log2, ry = kNormThreads / lx;
    const int64_t rows = l.prob.dims == 3 ? l.prob.ny : 1;
    p.nx_iters = int(std::max<int64_t>(1, (vpr + lx - 1) / lx));
    p.nrow_iters = (rows + ry - 1) / ry;
    const int64_t trips = p.nrow_iters * p.nx_iters;
    p.chunks = int(std::min<int64_t>(kNormMaxChunks, std::max<int64_t>(1, (trips + kNormChunkTrips - 1) / kNormChunkTrips)));
    return p;
}

template <typename T>
__global__ void __launch_bounds__(kNormThreads)
    diff_norm_kernel(const T* __restrict__ a, const T* __restrict__ b, Geom g, int dims, int64_t first_unit,
                     NormPlan p, double* __restrict__ part) {
    typedef typename VecOf<T>::type V;
    constexpr int VW = int(sizeof(V) / sizeof(T));
    __shared__ double red_max[kNormThreads / 64], red_sum[kNormThreads / 64];
    const int64_t u_rel = blockIdx.x / unsigned(p.chunks);
    const int c = int(blockIdx.x % unsigned(p.chunks));
    const int lx = 1 << p.lx_log2, ry = kNormThreads >> p.lx_log2;
    const int tx = int(threadIdx.x) & (lx - 1), ty = int(threadIdx.x) >> p.lx_log2;
    const int64_t rows = dims == 3 ? g.ny : 1;
    const int64_t unit = first_unit + u_rel;
    const int64_t base = g.origin + (dims == 3 ? unit * g.plane : unit * g.row);
    const int64_t trips = p.nrow_iters * p.nx_iters;
    const int64_t t0 = trips * c / p.chunks, t1 = trips * (c + 1) / p.chunks;
    int64_t ri = t0 / p.nx_iters;  // the trip's row group and x step, kept incrementally
    int xi = int(t0 - ri * p.nx_iters);
    double m = 0.0, s = 0.0;
    for (int64_t t = t0; t < t1; t += kNormUnroll) {
        V va[kNormUnroll], vb[kNormUnroll];
        int64_t xs[kNormUnroll];
#pragma unroll
        for (int k = 0; k < kNormUnroll; ++k) {
            const int64_t y = ri * ry + ty;
            const int64_t x = (int64_t(xi) * lx + tx) * VW;
            const bool ok = t + k < t1 && y < rows && x < g.nx;
            xs[k] = ok ? x : g.nx;  // g.nx: every element masked
            va[k] = V(0);
            vb[k] = V(0);
            if (ok) {
                const int64_t off = base + y * g.row + x;
                va[k] = *reinterpret_cast<const V*>(a + off);
                vb[k] = *reinterpret_cast<const V*>(b + off);
            }
            if (++xi == p.nx_iters) {
                xi = 0;
                ++ri;
            }
        }
#pragma unroll
        for (int k = 0; k < kNormUnroll; ++k) {
#pragma unroll
            for (int j = 0; j < VW; ++j) {
                double d = double(va[k][j]) - double(vb[k][j]);
                d = xs[k] + j < g.nx ? d : 0.0;
                m = fmax(m, fabs(d));
                s += d * d;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        m = fmax(m, __shfl_xor(m, o));
        s += __shfl_xor(s, o);
    }
    const int wave = int(threadIdx.x) >> 6;
    if ((threadIdx.x & 63) == 0) {
        red_max[wave] = m;
        red_sum[wave] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kNormThreads / 64; ++w) {
            m = fmax(m, red_max[w]);
            s += red_sum[w];
        }
        part[2 * int64_t(blockIdx.x)] = m;
        part[2 * int64_t(blockIdx.x) + 1] = s;
    }
}

// One lane per unit: its chunk partials in ascending chunk order, NaN made
// sticky for both outputs.
__global__ void __launch_bounds__(64) combine_norm_kernel(const double* __restrict__ part, int chunks, int64_t units,
                                                          double* __restrict__ max_abs, double* __restrict__ sum_sq) {
    const int64_t u = int64_t(blockIdx.x) * 64 + threadIdx.x;
    if (u >= units) return;
    double m = 0.0, s = 0.0;
    for (int c = 0; c < chunks; ++c) {
        m = fmax(m, part[2 * (u * chunks + c)]);
        s += part[2 * (u * chunks + c) + 1];
    }
    if (s != s) m = s = std::numeric_limits<double>::quiet_NaN();
    max_abs[u] = m;
    sum_sq[u] = s;
}

}  // namespace

int64_t diff_norms_workspace_bytes(const stencil_layout& l, int64_t units) {
    const NormPlan p = norm_plan(l);
    const int64_t batch = std::min(units, std::max<int64_t>(1, kNormMaxBlocks / p.chunks));
    return (2 * units + 2 * batch * p.chunks) * int64_t(sizeof(double));
}

// Kernel launches launch_diff_norms makes for `units` units: a norm and a
// combine launch per batch (host only).
int64_t diff_norms_launches(const stencil_layout& l, int64_t units) {
    if (units <= 0) return 0;
    const NormPlan p = norm_plan(l);
    const int64_t batch = std::min(units, std::max<int64_t>(1, kNormMaxBlocks / p.chunks));
    return 2 * ((units + batch - 1) / batch);
}

int launch_diff_norms(const stencil_layout& l, const void* a, const void* b, int64_t begin, int64_t end, double* scratch,
                      hipStream_t s) {
    const int64_t units = end - begin;
    if (units <= 0) return STENCIL_OK;
    if ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15)
        return set_error(STENCIL_EINVAL, "grids must be 16-byte aligned");
    const NormPlan p = norm_plan(l);
    const Geom g = geom_of(l);
    const int64_t batch = std::min(units, std::max<int64_t>(1, kNormMaxBlocks / p.chunks));
    double* max_abs = scratch;
    double* sum_sq = scratch + units;
    double* part = scratch + 2 * units;
    // launches on one stream run in order, so every batch reuses `part`
    for (int64_t u0 = 0; u0 < units; u0 += batch) {
        const int64_t n = std::min(batch, units - u0);
        const dim3 grid(unsigned(n * p.chunks));
        if (l.prob.dtype == STENCIL_F32)
            hipLaunchKernelGGL(diff_norm_kernel<float>, grid, dim3(kNormThreads), 0, s, static_cast<const float*>(a),
                               static_cast<const float*>(b), g, l.prob.dims, begin + u0, p, part);
        else
            hipLaunchKernelGGL(diff_norm_kernel<double>, grid, dim3(kNormThreads), 0, s, static_cast<const double*>(a),
                               static_cast<const double*>(b), g, l.prob.dims, begin + u0, p, part);
        STENCIL_LAUNCH_CHECK();
        hipLaunchKernelGGL(combine_norm_kernel, dim3(unsigned((n + 63) / 64)), dim3(64), 0, s, part, p.chunks, n,
                           max_abs + u0, sum_sq + u0);
        STENCIL_LAUNCH_CHECK();
    }
    return STENCIL_OK;
}

}  // namespace stencil
