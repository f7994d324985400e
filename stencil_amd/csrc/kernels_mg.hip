// kernels_mg.hip -- geometric multigrid for the 7-point Poisson solve on one
// GPU (include/stencil_hip.h "Geometric multigrid"): the
// transfer kernels between a fine grid and its vertex-centred coarsening, the
// residual norms, and the V-cycle driver (stencil_mg_*) on top of the relaxed
// sweeps of stencil_iterate_relax.  No reference counterpart: the reference
// runs a fixed number of plain sweeps (src/stencil/stencil.cpp:23-57).
//
// Every value is a sequence of separately rounded IEEE operations in the
// grid's type (the library is compiled with -ffp-contract=off): the results
// depend on the data alone, never on the tiling, the march or timing.
//
//  * restrict_residual_kernel.  A workgroup of 256 lanes owns a tile of
//    kMgTX x kMgTY coarse cells and a run of kMgZRun coarse planes and marches
//    the 2 n + 1 fine planes under them upward.  The fine tile with its ring
//    ((2 TX + 3) x (2 TY + 3) cells of u) is dealt over the lanes, kMgCells
//    cells each; a lane keeps its cells' planes z - 1, z, z + 1 in registers
//    (as sweep_source1 does), so u is read once per cell and plane.  Per fine
//    plane: the lanes put plane z of u into LDS, compute the residual of their
//    interior cells from it (x / y neighbours from LDS, z neighbours from
//    registers, g from memory) and put it into a second LDS tile; then lane
//    (X, Y) takes the x-then-y full weighting P(z) of its coarse cell from
//    that tile.  Two registers hold P(2Z) and P(2Z + 1) until P(2Z + 2)
//    arrives; P(2Z + 2) is the next coarse plane's first term.  The residual
//    never reaches global memory.  Neighbouring tiles recompute their shared
//    fine row / column, neighbouring z-runs their shared fine plane.  No
//    atomics, no hand-off between workgroups; the only stores are interior
//    cells of coarse planes [cbegin, cend).
//  * prolong_add_kernel.  One fine cell per lane, 64-lane rows along x: the
//    x-interpolation at the four (y, z) coarse corners, then y, then z; an odd
//    index is a copy of its coarse cell (a select, never 0.5 * (e + e)).  e is
//    an eighth of the traffic and comes from cache; u is read and written once.
//  * residual_norm_kernel.  stencil_diff_norms' reduction (kernels_norm.hip:
//    lane sums in trip order, a fixed xor-shuffle tree, waves through LDS in
//    wave order, chunk partials combined in ascending order by a second tiny
//    launch that makes NaN sticky) over the residual device function the
//    restriction uses; r is not stored.
#include <cmath>
#include <cstring>
#include <limits>
#include <new>
#include <vector>

#include "common.hpp"

struct stencil_mg {
    struct Level {
        stencil_layout lay{};
        void* field[2] = {nullptr, nullptr};  // ping-pong grids of the relaxed jobs
        void* src = nullptr;
        int cur = 0;  // the grid that holds the level's field
    };
    std::vector<Level> lv;
};

namespace stencil {
namespace {

constexpr int kMgTX = 32, kMgTY = 8;  // coarse cells per workgroup tile
constexpr int kMgThreads = kMgTX * kMgTY;
constexpr int kMgZRun = 8;                                  // coarse planes per workgroup
constexpr int kMgUW = 2 * kMgTX + 3, kMgUH = 2 * kMgTY + 3;  // the tile of u, ring included
constexpr int kMgRW = 2 * kMgTX + 1, kMgRH = 2 * kMgTY + 1;  // the tile of residuals
constexpr int kMgCells = (kMgUW * kMgUH + kMgThreads - 1) / kMgThreads;  // cells of u per lane

// r(c) = fl(J(c) - u(c)), J = fl(fl(sum6 * avg) + g): the `d` of the relaxed sweep (kernels_source.hip)
template <typename T>
__device__ __forceinline__ T mg_residual(T xm, T xp, T ym, T yp, T zm, T zp, T c, T g, T avg) {
    T sum = T(0);
    sum += xm;
    sum += xp;
    sum += ym;
    sum += yp;
    sum += zm;
    sum += zp;
    const T avged = sum * avg;  // rounded here
    const T j = avged + g;
    return j - c;
}

// The 1-D full-weighting operator: fl(fl(lo + hi) + fl(mid + mid))
template <typename T>
__device__ __forceinline__ T mg_weigh(T lo, T mid, T hi) {
    const T ends = lo + hi;
    const T twice = mid + mid;
    return ends + twice;
}

template <typename T>
__global__ void __launch_bounds__(kMgThreads)
    restrict_residual_kernel(const T* __restrict__ u, const T* __restrict__ g, T* __restrict__ gc, Geom gf, Geom gcs,
                             int64_t cbegin, int64_t cend, T avg) {
    __shared__ T su[kMgUH * kMgUW];
    __shared__ T sr[kMgRH * kMgRW];
    const int tid = int(threadIdx.x);
    const int64_t X0 = int64_t(blockIdx.x) * kMgTX, Y0 = int64_t(blockIdx.y) * kMgTY;
    const int64_t Z0 = cbegin + int64_t(blockIdx.z) * kMgZRun;
    const int64_t Z1 = Z0 + kMgZRun < cend ? Z0 + kMgZRun : cend;
    // tile-local (tx, ty) of u is fine cell (2 X0 - 1 + tx, 2 Y0 - 1 + ty)
    int64_t off[kMgCells];
    int ri[kMgCells];    // the cell's slot in the residual tile, -1: a ring cell
    bool ok[kMgCells];   // inside the ghost-padded plane: loaded
    bool own[kMgCells];  // an interior fine cell: has a residual
#pragma unroll
    for (int k = 0; k < kMgCells; ++k) {
        const int i = tid + k * kMgThreads;
        const int ty = i / kMgUW, tx = i - ty * kMgUW;
        const int64_t fx = 2 * X0 - 1 + tx, fy = 2 * Y0 - 1 + ty;
        const bool live = i < kMgUW * kMgUH;
        const bool inner = live && tx >= 1 && tx <= kMgRW && ty >= 1 && ty <= kMgRH;
        ok[k] = live && fx <= gf.nx && fy <= gf.ny;
        own[k] = inner && fx < gf.nx && fy < gf.ny;
        ri[k] = inner ? (ty - 1) * kMgRW + (tx - 1) : -1;
        off[k] = gf.origin + fy * gf.row + fx;
    }
    const int cx = tid % kMgTX, cy = tid / kMgTX;
    const int64_t X = X0 + cx, Y = Y0 + cy;
    const bool stores = X < gcs.nx && Y < gcs.ny;
    const int64_t zf0 = 2 * Z0, zf1 = 2 * Z1;  // fine planes zf0 .. zf1, both ends included
    T zm[kMgCells], c[kMgCells];
#pragma unroll
    for (int k = 0; k < kMgCells; ++k) {
        zm[k] = ok[k] ? u[off[k] + (zf0 - 1) * gf.plane] : T(0);
        c[k] = ok[k] ? u[off[k] + zf0 * gf.plane] : T(0);
    }
    T p0 = T(0), p1 = T(0);  // P(2Z), P(2Z + 1) of the coarse plane being gathered
    for (int64_t z = zf0; z <= zf1; ++z) {
        T zp[kMgCells], gv[kMgCells];
#pragma unroll
        for (int k = 0; k < kMgCells; ++k) {
            zp[k] = ok[k] ? u[off[k] + (z + 1) * gf.plane] : T(0);
            gv[k] = own[k] ? g[off[k] + z * gf.plane] : T(0);
        }
#pragma unroll
        for (int k = 0; k < kMgCells; ++k) {
            const int i = tid + k * kMgThreads;
            if (i < kMgUW * kMgUH) su[i] = c[k];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kMgCells; ++k) {
            const int i = tid + k * kMgThreads;
            if (ri[k] >= 0)
                sr[ri[k]] = own[k] ? mg_residual(su[i - 1], su[i + 1], su[i - kMgUW], su[i + kMgUW], zm[k], zp[k], c[k],
                                                 gv[k], avg)
                                   : T(0);
        }
        __syncthreads();
        // x, then y, at the lane's coarse cell: fine rows 2 cy .. 2 cy + 2, columns 2 cx .. 2 cx + 2 of the tile
        const T* row = sr + (2 * cy) * kMgRW + 2 * cx;
        const T a0 = mg_weigh(row[0], row[1], row[2]);
        const T a1 = mg_weigh(row[kMgRW], row[kMgRW + 1], row[kMgRW + 2]);
        const T a2 = mg_weigh(row[2 * kMgRW], row[2 * kMgRW + 1], row[2 * kMgRW + 2]);
        const T p = mg_weigh(a0, a1, a2);
        const int64_t rel = z - zf0;
        if (rel & 1) {
            p1 = p;
        } else {
            if (rel > 0 && stores) {
                const int64_t Z = Z0 + rel / 2 - 1;
                gc[gcs.origin + Z * gcs.plane + Y * gcs.row + X] = T(0.0625) * mg_weigh(p0, p1, p);
            }
            p0 = p;
        }
#pragma unroll
        for (int k = 0; k < kMgCells; ++k) {
            zm[k] = c[k];
            c[k] = zp[k];
        }
    }
}

constexpr int kPX = 64, kPY = 4;
constexpr int kProlongChunk = 4;  // fine planes per workgroup

// The two coarse cells of fine index i along one axis: odd i is a copy of (i - 1) / 2 (lo == hi), even i
// the mean of i / 2 - 1 and i / 2 (-1 and m: ghost cells)
__device__ __forceinline__ void mg_pair(int64_t i, int64_t* lo, int64_t* hi) {
    *lo = (i & 1) ? (i - 1) / 2 : i / 2 - 1;
    *hi = (i & 1) ? *lo : i / 2;
}

template <typename T>
__global__ void __launch_bounds__(kPX * kPY)
    prolong_add_kernel(const T* __restrict__ e, T* __restrict__ u, Geom gcs, Geom gf, int64_t begin, int64_t end) {
    const int64_t x = int64_t(blockIdx.x) * kPX + threadIdx.x;
    const int64_t y = int64_t(blockIdx.y) * kPY + threadIdx.y;
    if (x >= gf.nx || y >= gf.ny) return;
    const int64_t za = begin + int64_t(blockIdx.z) * kProlongChunk;
    const int64_t zb = za + kProlongChunk < end ? za + kProlongChunk : end;
    int64_t xl, xh, yl, yh;
    mg_pair(x, &xl, &xh);
    mg_pair(y, &yl, &yh);
    const bool xodd = x & 1, yodd = y & 1;
    const int64_t rl = gcs.origin + yl * gcs.row, rh = gcs.origin + yh * gcs.row;
    int64_t idx = gf.origin + za * gf.plane + y * gf.row + x;
    // x, then y, within coarse plane zc; an odd x loads its one coarse cell twice (xl == xh) and selects the
    // copy.  The parities of y and z are the same for a whole wave (a wave is one row of lanes), so an odd y or
    // z can skip its second corner's loads without divergence.  fp64 does (kSkip: 0.70 against 0.90 ms at 511^3);
    // fp32, whose lanes move half the bytes and wait on latency, not bandwidth, is faster with all eight loads
    // issued at once and the copies selected (0.31 against 0.54 ms): DESIGN.md 5.9.  The values are the same.
    constexpr bool kSkip = sizeof(T) == 8;
    auto in_plane = [&](int64_t zc) -> T {
        const int64_t pl = zc * gcs.plane;
        const T a = e[pl + rl + xl], b = e[pl + rl + xh];
        const T ab = a + b;
        const T lo = xodd ? a : T(0.5) * ab;
        if (kSkip && yodd) return lo;
        const T c = e[pl + rh + xl], d = e[pl + rh + xh];
        const T cd = c + d;
        const T hi = xodd ? c : T(0.5) * cd;
        const T lh = lo + hi;
        return yodd ? lo : T(0.5) * lh;
    };
    for (int64_t z = za; z < zb; ++z, idx += gf.plane) {
        int64_t zl, zh;
        mg_pair(z, &zl, &zh);
        const bool zodd = z & 1;
        T p = in_plane(zl);
        if (!kSkip || !zodd) {
            const T s = p + in_plane(zh);
            p = zodd ? p : T(0.5) * s;
        }
        u[idx] = u[idx] + p;
    }
}

// ---- full multigrid: the coarse problems and the cubic prolongation ----

constexpr int kSrcCells = (kMgRW * kMgRH + kMgThreads - 1) / kMgThreads;  // cells of g per lane and fine plane

// g_c = fl(0.0625 * A_z(A_y(A_x(g)))): restrict_residual_kernel's march with g in the residual's place.  The
// fine tile has no ring (the weighting of interior coarse cells touches interior fine cells only); plane z + 1
// is fetched into registers while plane z is weighed, and the two LDS tiles alternate, so a plane costs one
// barrier.  Stores: interior cells of coarse planes [cbegin, cend).
template <typename T>
__global__ void __launch_bounds__(kMgThreads)
    restrict_source_kernel(const T* __restrict__ g, T* __restrict__ gc, Geom gf, Geom gcs, int64_t cbegin, int64_t cend) {
    __shared__ T sg[2][kMgRH * kMgRW];
    const int tid = int(threadIdx.x);
    const int64_t X0 = int64_t(blockIdx.x) * kMgTX, Y0 = int64_t(blockIdx.y) * kMgTY;
    const int64_t Z0 = cbegin + int64_t(blockIdx.z) * kMgZRun;
    const int64_t Z1 = Z0 + kMgZRun < cend ? Z0 + kMgZRun : cend;
    // tile-local (tx, ty) is fine cell (2 X0 + tx, 2 Y0 + ty)
    int64_t off[kSrcCells];
    bool ok[kSrcCells];  // an interior fine cell: loaded
#pragma unroll
    for (int k = 0; k < kSrcCells; ++k) {
        const int i = tid + k * kMgThreads;
        const int ty = i / kMgRW, tx = i - ty * kMgRW;
        const int64_t fx = 2 * X0 + tx, fy = 2 * Y0 + ty;
        ok[k] = i < kMgRW * kMgRH && fx < gf.nx && fy < gf.ny;
        off[k] = gf.origin + fy * gf.row + fx;
    }
    const int cx = tid % kMgTX, cy = tid / kMgTX;
    const int64_t X = X0 + cx, Y = Y0 + cy;
    const bool stores = X < gcs.nx && Y < gcs.ny;
    const int64_t zf0 = 2 * Z0, zf1 = 2 * Z1;  // fine planes zf0 .. zf1, both ends included (zf1 <= nz - 1)
    T v[kSrcCells];
#pragma unroll
    for (int k = 0; k < kSrcCells; ++k) v[k] = ok[k] ? g[off[k] + zf0 * gf.plane] : T(0);
    T p0 = T(0), p1 = T(0);  // P(2Z), P(2Z + 1) of the coarse plane being gathered
    for (int64_t z = zf0; z <= zf1; ++z) {
        const int64_t rel = z - zf0;
        T* s = sg[rel & 1];
#pragma unroll
        for (int k = 0; k < kSrcCells; ++k) {
            const int i = tid + k * kMgThreads;
            if (i < kMgRW * kMgRH) s[i] = v[k];
        }
        if (z < zf1) {
#pragma unroll
            for (int k = 0; k < kSrcCells; ++k) v[k] = ok[k] ? g[off[k] + (z + 1) * gf.plane] : T(0);
        }
        __syncthreads();
        const T* row = s + (2 * cy) * kMgRW + 2 * cx;
        const T a0 = mg_weigh(row[0], row[1], row[2]);
        const T a1 = mg_weigh(row[kMgRW], row[kMgRW + 1], row[kMgRW + 2]);
        const T a2 = mg_weigh(row[2 * kMgRW], row[2 * kMgRW + 1], row[2 * kMgRW + 2]);
        const T p = mg_weigh(a0, a1, a2);
        if (rel & 1) {
            p1 = p;
        } else {
            if (rel > 0 && stores) {
                const int64_t Z = Z0 + rel / 2 - 1;
                gc[gcs.origin + Z * gcs.plane + Y * gcs.row + X] = T(0.0625) * mg_weigh(p0, p1, p);
            }
            p0 = p;
        }
    }
}

constexpr int kInjThreads = 256;

// The shell of the coarse ghost-padded box, one cell per lane: the two ghost planes whole, then per interior
// plane the two ghost rows whole and the two ghost cells of every interior row.
inline int64_t shell_cells(const Geom& c) {
    return 2 * (c.ny + 2) * (c.nx + 2) + c.nz * (2 * (c.nx + 2) + 2 * c.ny);
}

// Coarse shell cell (X, Y, Z) = fine ghost-shell cell (2X+1, 2Y+1, 2Z+1), into c0 and (if given) c1
template <typename T>
__global__ void __launch_bounds__(kInjThreads)
    inject_ghosts_kernel(const T* __restrict__ u, T* __restrict__ c0, T* __restrict__ c1, Geom gf, Geom gcs, int64_t total) {
    int64_t t = int64_t(blockIdx.x) * kInjThreads + threadIdx.x;
    if (t >= total) return;
    const int64_t W = gcs.nx + 2, area = W * (gcs.ny + 2), ring = 2 * W + 2 * gcs.ny;
    int64_t X, Y, Z;
    if (t < 2 * area) {
        Z = t < area ? -1 : gcs.nz;
        const int64_t r = t < area ? t : t - area;
        Y = r / W - 1;
        X = r % W - 1;
    } else {
        t -= 2 * area;
        Z = t / ring;
        int64_t r = t % ring;
        if (r < 2 * W) {
            Y = r < W ? -1 : gcs.ny;
            X = (r < W ? r : r - W) - 1;
        } else {
            r -= 2 * W;
            Y = r / 2;
            X = (r & 1) ? gcs.nx : -1;
        }
    }
    const T v = u[gf.origin + (2 * Z + 1) * gf.plane + (2 * Y + 1) * gf.row + (2 * X + 1)];
    const int64_t ci = gcs.origin + Z * gcs.plane + Y * gcs.row + X;
    c0[ci] = v;
    if (c1) c1[ci] = v;
}

constexpr int kCubicChunk = 16;  // fine planes per workgroup

// Fine index i along an axis of coarse extent m, in PADDED coarse indices (P = coarse index + 1, 0 .. m + 1):
// the four nodes P = s .. s + 3 (clamped to m + 1 where m = 1 has only three) and what to make of them.
// s = clamp(i / 2 - 1, 0, m - 2) never decreases with i, so a march along the axis keeps a sliding window.
template <typename T>
struct CubicAx {
    int64_t s;
    T w0, w1, w2, w3;  // the cubic's integer weights
    bool copy;         // odd i: node 1 (hi: node 2) exactly
    bool lin;          // even i, m = 1: the mean of nodes 0, 1 (hi: 1, 2)
    bool hi;
};

template <typename T>
__device__ __forceinline__ CubicAx<T> cubic_ax(int64_t i, int64_t m) {
    CubicAx<T> a;
    const int64_t k = i >> 1, top = m >= 2 ? m - 2 : 0;
    const int64_t lo = k - 1 > 0 ? k - 1 : 0;
    a.s = lo < top ? lo : top;
    a.copy = i & 1;
    a.lin = !a.copy && m == 1;
    a.hi = a.copy ? k + 1 - a.s == 2 : k == 1;
    const bool first = k == 0, last = k == m;
    a.w0 = first ? T(5) : last ? T(1) : T(-1);
    a.w1 = first ? T(15) : last ? T(-5) : T(9);
    a.w2 = first ? T(-5) : last ? T(15) : T(9);
    a.w3 = first ? T(1) : last ? T(5) : T(-1);
    return a;
}

// fl(0.0625 * fl( fl(fl(w0 p0) + fl(w1 p1)) + fl(fl(w2 p2) + fl(w3 p3)) )), or the copy, or the mean: selects,
// no branch on the arithmetic
template <typename T>
__device__ __forceinline__ T cubic_apply(T p0, T p1, T p2, T p3, const CubicAx<T>& a) {
    const T t0 = a.w0 * p0, t1 = a.w1 * p1, t2 = a.w2 * p2, t3 = a.w3 * p3;
    const T left = t0 + t1, right = t2 + t3;
    const T sum = left + right;
    const T cub = T(0.0625) * sum;
    const T la = a.hi ? p1 : p0, lb = a.hi ? p2 : p1;
    const T pair = la + lb;
    const T mean = T(0.5) * pair;
    return a.copy ? lb : a.lin ? mean : cub;
}

// u = the cubic prolongation of e at the interior cells of fine planes [begin, end): prolong_add_kernel's shape
// (one fine cell per lane, a wave is one row, so the parities of y and z are wave-uniform and an odd y takes
// one coarse row instead of four).  A lane marches kCubicChunk fine planes upward and keeps the in-plane
// values of the four coarse planes of its z window in registers; the window moves up by at most one coarse
// plane per fine plane.  e comes from cache, u is written once and never read.
template <typename T>
__global__ void __launch_bounds__(kPX * kPY)
    prolong_cubic_kernel(const T* __restrict__ e, T* __restrict__ u, Geom gcs, Geom gf, int64_t begin, int64_t end) {
    const int64_t x = int64_t(blockIdx.x) * kPX + threadIdx.x;
    const int64_t y = int64_t(blockIdx.y) * kPY + threadIdx.y;
    if (x >= gf.nx || y >= gf.ny) return;
    const int64_t za = begin + int64_t(blockIdx.z) * kCubicChunk;
    const int64_t zb = za + kCubicChunk < end ? za + kCubicChunk : end;
    const CubicAx<T> ax = cubic_ax<T>(x, gcs.nx), ay = cubic_ax<T>(y, gcs.ny);
    const int64_t px = gcs.nx + 1, py = gcs.ny + 1, pz = gcs.nz + 1;  // the last padded index per axis
    const T* corner = e + (gcs.origin - gcs.plane - gcs.row - 1);    // padded (0, 0, 0)
    int64_t xo[4], yo[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        xo[j] = ax.s + j < px ? ax.s + j : px;
        yo[j] = (ay.s + j < py ? ay.s + j : py) * gcs.row;
    }
    auto in_row = [&](const T* r) -> T { return cubic_apply(r[xo[0]], r[xo[1]], r[xo[2]], r[xo[3]], ax); };
    auto in_plane = [&](int64_t P) -> T {
        const T* pl = corner + (P < pz ? P : pz) * gcs.plane;
        if (ay.copy) return in_row(pl + yo[ay.hi ? 2 : 1]);
        return cubic_apply(in_row(pl + yo[0]), in_row(pl + yo[1]), in_row(pl + yo[2]), in_row(pl + yo[3]), ay);
    };
    int64_t cur = cubic_ax<T>(za, gcs.nz).s;
    T q0 = in_plane(cur), q1 = in_plane(cur + 1), q2 = in_plane(cur + 2), q3 = in_plane(cur + 3);
    int64_t idx = gf.origin + za * gf.plane + y * gf.row + x;
    for (int64_t z = za; z < zb; ++z, idx += gf.plane) {
        const CubicAx<T> az = cubic_ax<T>(z, gcs.nz);
        if (az.s != cur) {  // one coarse plane up
            cur = az.s;
            q0 = q1;
            q1 = q2;
            q2 = q3;
            q3 = in_plane(cur + 3);
        }
        u[idx] = cubic_apply(q0, q1, q2, q3, az);
    }
}

constexpr int kRnThreads = 256, kRnX = 64, kRnY = kRnThreads / kRnX;
constexpr int64_t kRnChunkTrips = 16;  // trips per workgroup aimed at ...
constexpr int kRnMaxChunks = 32;       // ... up to this many chunks per plane
constexpr int64_t kRnMaxBlocks = int64_t(1) << 22;  // workgroups per launch

struct RnPlan {
    int nx_iters;        // trips along x per row group
    int64_t nrow_iters;  // row groups of kRnY rows per plane
    int chunks;          // workgroups (partials) per plane
};

RnPlan rn_plan(const stencil_layout& l) {
    RnPlan p{};
    p.nx_iters = int(std::max<int64_t>(1, (l.prob.nx + kRnX - 1) / kRnX));
    p.nrow_iters = (l.prob.ny + kRnY - 1) / kRnY;
    const int64_t trips = p.nrow_iters * p.nx_iters;
    p.chunks = int(std::min<int64_t>(kRnMaxChunks, std::max<int64_t>(1, (trips + kRnChunkTrips - 1) / kRnChunkTrips)));
    return p;
}

template <typename T>
__global__ void __launch_bounds__(kRnThreads)
    residual_norm_kernel(const T* __restrict__ u, const T* __restrict__ g, Geom gf, int64_t first_plane, RnPlan p, T avg,
                         double* __restrict__ part) {
    __shared__ double red_max[kRnThreads / 64], red_sum[kRnThreads / 64];
    const int64_t z = first_plane + blockIdx.x / unsigned(p.chunks);
    const int c = int(blockIdx.x % unsigned(p.chunks));
    const int tx = int(threadIdx.x) & (kRnX - 1), ty = int(threadIdx.x) / kRnX;
    const int64_t trips = p.nrow_iters * p.nx_iters;
    const int64_t t0 = trips * c / p.chunks, t1 = trips * (c + 1) / p.chunks;
    int64_t ri = t0 / p.nx_iters;
    int xi = int(t0 - ri * p.nx_iters);
    double m = 0.0, s = 0.0;
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t y = ri * kRnY + ty;
        const int64_t x = int64_t(xi) * kRnX + tx;
        if (y < gf.ny && x < gf.nx) {
            const int64_t idx = gf.origin + z * gf.plane + y * gf.row + x;
            const T r = mg_residual(u[idx - 1], u[idx + 1], u[idx - gf.row], u[idx + gf.row], u[idx - gf.plane],
                                    u[idx + gf.plane], u[idx], g[idx], avg);
            const double d = double(r);
            m = fmax(m, fabs(d));
            s += d * d;
        }
        if (++xi == p.nx_iters) {
            xi = 0;
            ++ri;
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
        for (int w = 1; w < kRnThreads / 64; ++w) {
            m = fmax(m, red_max[w]);
            s += red_sum[w];
        }
        part[2 * int64_t(blockIdx.x)] = m;
        part[2 * int64_t(blockIdx.x) + 1] = s;
    }
}

// One lane per plane: its chunk partials in ascending chunk order, NaN made sticky for both outputs
// (kernels_norm.hip's combine)
__global__ void __launch_bounds__(64) residual_combine_kernel(const double* __restrict__ part, int chunks, int64_t units,
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

inline hipStream_t as_stream(void* s) { return static_cast<hipStream_t>(s); }

int64_t rn_workspace_bytes(const stencil_layout& l, int64_t units) {
    const RnPlan p = rn_plan(l);
    const int64_t batch = std::min(units, std::max<int64_t>(1, kRnMaxBlocks / p.chunks));
    return (2 * units + 2 * batch * p.chunks) * int64_t(sizeof(double));
}

// Per-plane residual norms of planes [begin, end) into scratch[0 .. n) (maxima) and scratch[n .. 2n) (sums)
template <typename T>
int launch_rn(const stencil_layout& l, const void* u, const void* g, int64_t begin, int64_t end, double* scratch,
              hipStream_t s) {
    const int64_t units = end - begin;
    if (units <= 0) return STENCIL_OK;
    const RnPlan p = rn_plan(l);
    const Geom gf = geom_of(l);
    const int64_t batch = std::min(units, std::max<int64_t>(1, kRnMaxBlocks / p.chunks));
    double* part = scratch + 2 * units;
    for (int64_t u0 = 0; u0 < units; u0 += batch) {
        const int64_t n = std::min(batch, units - u0);
        hipLaunchKernelGGL(residual_norm_kernel<T>, dim3(unsigned(n * p.chunks)), dim3(kRnThreads), 0, s,
                           static_cast<const T*>(u), static_cast<const T*>(g), gf, begin + u0, p, avg_weight<T>(l.prob),
                           part);
        STENCIL_LAUNCH_CHECK();
        hipLaunchKernelGGL(residual_combine_kernel, dim3(unsigned((n + 63) / 64)), dim3(64), 0, s, part, p.chunks, n,
                           scratch + u0, scratch + units + u0);
        STENCIL_LAUNCH_CHECK();
    }
    return STENCIL_OK;
}

constexpr int64_t kRestrictSpan = int64_t(65535) * kMgZRun;      // coarse planes per launch (grid z limit)
constexpr int64_t kProlongSpan = int64_t(65535) * kProlongChunk;  // fine planes per launch

int64_t restrict_launches(int64_t planes) { return planes <= 0 ? 0 : (planes + kRestrictSpan - 1) / kRestrictSpan; }
int64_t prolong_launches(int64_t planes) { return planes <= 0 ? 0 : (planes + kProlongSpan - 1) / kProlongSpan; }

template <typename T>
int launch_restrict(const stencil_layout& lf, const void* u, const void* g, const stencil_layout& lc, void* gc,
                    int64_t cbegin, int64_t cend, hipStream_t s) {
    const Geom gf = geom_of(lf), gcs = geom_of(lc);
    if (cend <= cbegin || gcs.nx <= 0 || gcs.ny <= 0) return STENCIL_OK;
    const int64_t gx = (gcs.nx + kMgTX - 1) / kMgTX, gy = (gcs.ny + kMgTY - 1) / kMgTY;
    if (gy > 65535 || gx > (int64_t(1) << 31) - 1) return set_error(STENCIL_EINVAL, "grid too large for the restriction");
    for (int64_t z0 = cbegin; z0 < cend; z0 += kRestrictSpan) {
        const int64_t z1 = std::min(cend, z0 + kRestrictSpan);
        const unsigned gz = unsigned((z1 - z0 + kMgZRun - 1) / kMgZRun);
        hipLaunchKernelGGL(restrict_residual_kernel<T>, dim3(unsigned(gx), unsigned(gy), gz), dim3(kMgThreads), 0, s,
                           static_cast<const T*>(u), static_cast<const T*>(g), static_cast<T*>(gc), gf, gcs, z0, z1,
                           avg_weight<T>(lf.prob));
        STENCIL_LAUNCH_CHECK();
    }
    return STENCIL_OK;
}

template <typename T>
int launch_prolong(const stencil_layout& lc, const void* e, const stencil_layout& lf, void* u, int64_t begin, int64_t end,
                   hipStream_t s) {
    const Geom gf = geom_of(lf), gcs = geom_of(lc);
    if (end <= begin || gf.nx <= 0 || gf.ny <= 0) return STENCIL_OK;
    const int64_t gx = (gf.nx + kPX - 1) / kPX, gy = (gf.ny + kPY - 1) / kPY;
    if (gy > 65535 || gx > (int64_t(1) << 31) - 1) return set_error(STENCIL_EINVAL, "grid too large for the prolongation");
    for (int64_t z0 = begin; z0 < end; z0 += kProlongSpan) {
        const int64_t z1 = std::min(end, z0 + kProlongSpan);
        const unsigned gz = unsigned((z1 - z0 + kProlongChunk - 1) / kProlongChunk);
        hipLaunchKernelGGL(prolong_add_kernel<T>, dim3(unsigned(gx), unsigned(gy), gz), dim3(kPX, kPY, 1), 0, s,
                           static_cast<const T*>(e), static_cast<T*>(u), gcs, gf, z0, z1);
        STENCIL_LAUNCH_CHECK();
    }
    return STENCIL_OK;
}

constexpr int64_t kCubicSpan = int64_t(65535) * kCubicChunk;  // fine planes per launch
int64_t cubic_launches(int64_t planes) { return planes <= 0 ? 0 : (planes + kCubicSpan - 1) / kCubicSpan; }

template <typename T>
int launch_restrict_source(const stencil_layout& lf, const void* g, const stencil_layout& lc, void* gc, int64_t cbegin,
                           int64_t cend, hipStream_t s) {
    const Geom gf = geom_of(lf), gcs = geom_of(lc);
    if (cend <= cbegin || gcs.nx <= 0 || gcs.ny <= 0) return STENCIL_OK;
    const int64_t gx = (gcs.nx + kMgTX - 1) / kMgTX, gy = (gcs.ny + kMgTY - 1) / kMgTY;
    if (gy > 65535 || gx > (int64_t(1) << 31) - 1) return set_error(STENCIL_EINVAL, "grid too large for the restriction");
    for (int64_t z0 = cbegin; z0 < cend; z0 += kRestrictSpan) {
        const int64_t z1 = std::min(cend, z0 + kRestrictSpan);
        const unsigned gz = unsigned((z1 - z0 + kMgZRun - 1) / kMgZRun);
        hipLaunchKernelGGL(restrict_source_kernel<T>, dim3(unsigned(gx), unsigned(gy), gz), dim3(kMgThreads), 0, s,
                           static_cast<const T*>(g), static_cast<T*>(gc), gf, gcs, z0, z1);
        STENCIL_LAUNCH_CHECK();
    }
    return STENCIL_OK;
}

// uc1: a second coarse grid that takes the same cells in the same launch, or NULL
template <typename T>
int launch_inject(const stencil_layout& lf, const void* u, const stencil_layout& lc, void* uc0, void* uc1, hipStream_t s) {
    const Geom gf = geom_of(lf), gcs = geom_of(lc);
    const int64_t total = shell_cells(gcs);
    const int64_t blocks = (total + kInjThreads - 1) / kInjThreads;
    if (blocks > (int64_t(1) << 31) - 1) return set_error(STENCIL_EINVAL, "grid too large for the ghost injection");
    hipLaunchKernelGGL(inject_ghosts_kernel<T>, dim3(unsigned(blocks)), dim3(kInjThreads), 0, s, static_cast<const T*>(u),
                       static_cast<T*>(uc0), static_cast<T*>(uc1), gf, gcs, total);
    STENCIL_LAUNCH_CHECK();
    return STENCIL_OK;
}

template <typename T>
int launch_prolong_cubic(const stencil_layout& lc, const void* e, const stencil_layout& lf, void* u, int64_t begin,
                         int64_t end, hipStream_t s) {
    const Geom gf = geom_of(lf), gcs = geom_of(lc);
    if (end <= begin || gf.nx <= 0 || gf.ny <= 0) return STENCIL_OK;
    const int64_t gx = (gf.nx + kPX - 1) / kPX, gy = (gf.ny + kPY - 1) / kPY;
    if (gy > 65535 || gx > (int64_t(1) << 31) - 1) return set_error(STENCIL_EINVAL, "grid too large for the prolongation");
    for (int64_t z0 = begin; z0 < end; z0 += kCubicSpan) {
        const int64_t z1 = std::min(end, z0 + kCubicSpan);
        const unsigned gz = unsigned((z1 - z0 + kCubicChunk - 1) / kCubicChunk);
        hipLaunchKernelGGL(prolong_cubic_kernel<T>, dim3(unsigned(gx), unsigned(gy), gz), dim3(kPX, kPY, 1), 0, s,
                           static_cast<const T*>(e), static_cast<T*>(u), gcs, gf, z0, z1);
        STENCIL_LAUNCH_CHECK();
    }
    return STENCIL_OK;
}

// ---- argument checks (all host only: they fire before a device is touched) ----

// The scope of stencil_sweepk_source; the message names what rules a problem out.
int check_mg_problem(const stencil_problem* p) {
    stencil_layout tmp;
    if (int rc = stencil_layout_init(p, &tmp)) return rc;  // NULL and malformed problems
    if (p->dims != 3) return set_error(STENCIL_EUNSUPPORTED, "multigrid: 3D grids only (got dims = %d)", p->dims);
    if (p->shape != STENCIL_STAR) return set_error(STENCIL_EUNSUPPORTED, "multigrid: the 7-point star only, not the box");
    if (p->radius != 1) return set_error(STENCIL_EUNSUPPORTED, "multigrid: radius 1 only (got %d)", p->radius);
    if (p->order != STENCIL_ORDER_NAIVE) return set_error(STENCIL_EUNSUPPORTED, "multigrid: the naive sum order only, not DMA");
    if (p->flags != 0) return set_error(STENCIL_EUNSUPPORTED, "multigrid: layouts without halo flags only (got %d)", p->flags);
    if (p->kernel != STENCIL_KERNEL_AUTO && p->kernel != STENCIL_KERNEL_TEMPORALK)
        return set_error(STENCIL_EUNSUPPORTED, "multigrid: kernel AUTO or TEMPORALK only (got %d)", p->kernel);
    return STENCIL_OK;
}

bool coarsenable(const stencil_problem& p) {
    return p.nx >= 3 && p.ny >= 3 && p.nz >= 3 && (p.nx & 1) && (p.ny & 1) && (p.nz & 1);
}

stencil_problem coarsened(const stencil_problem& p) {
    stencil_problem c = p;
    c.nx = (p.nx - 1) / 2;
    c.ny = (p.ny - 1) / 2;
    c.nz = (p.nz - 1) / 2;
    return c;
}

// A layout in scope whose geometry is stencil_layout_init's for its problem (the kernels trust it)
int check_mg_layout(const stencil_layout* l, const char* what) {
    if (!l) return set_error(STENCIL_EINVAL, "null %s layout", what);
    if (int rc = check_mg_problem(&l->prob)) return rc;
    stencil_layout want;
    if (int rc = stencil_layout_init(&l->prob, &want)) return rc;
    if (l->row != want.row || l->plane != want.plane || l->planes != want.planes || l->zghost != want.zghost ||
        l->rows != want.rows || l->origin != want.origin || l->elems != want.elems || l->bytes != want.bytes)
        return set_error(STENCIL_EINVAL, "the %s layout is not stencil_layout_init's for its problem", what);
    return STENCIL_OK;
}

// lf and lc in scope, of one dtype, lc the coarsening of lf
int check_mg_pair(const stencil_layout* lf, const stencil_layout* lc) {
    if (int rc = check_mg_layout(lf, "fine")) return rc;
    if (int rc = check_mg_layout(lc, "coarse")) return rc;
    if (lf->prob.dtype != lc->prob.dtype)
        return set_error(STENCIL_EINVAL, "the fine and the coarse grid differ in dtype (%d and %d)", lf->prob.dtype,
                         lc->prob.dtype);
    const stencil_problem want = coarsened(lf->prob);
    if (!coarsenable(lf->prob) || lc->prob.nx != want.nx || lc->prob.ny != want.ny || lc->prob.nz != want.nz)
        return set_error(STENCIL_EINVAL,
                         "the coarse layout (%lld x %lld x %lld) is not the coarsening of the fine one (%lld x %lld x %lld: "
                         "odd extents n >= 3 coarsen to (n - 1) / 2)",
                         (long long)lc->prob.nx, (long long)lc->prob.ny, (long long)lc->prob.nz, (long long)lf->prob.nx,
                         (long long)lf->prob.ny, (long long)lf->prob.nz);
    return STENCIL_OK;
}

int check_mg_params(const stencil_mg_params* p) {
    if (!p) return set_error(STENCIL_EINVAL, "null multigrid parameters");
    if (!p->omegas) return set_error(STENCIL_EINVAL, "null weights (omegas)");
    if (p->period == 0) return set_error(STENCIL_EINVAL, "the schedule's period must be at least 1");
    for (uint32_t i = 0; i < p->period; ++i)
        if (!std::isfinite(p->omegas[i]))
            return set_error(STENCIL_EINVAL, "weight %u of the schedule is not a finite number", i);
    return STENCIL_OK;
}

// The most levels of `fine`: coarsen while every extent is odd and >= 3
int max_levels(const stencil_problem& fine) {
    int n = 1;
    for (stencil_problem p = fine; coarsenable(p); p = coarsened(p)) ++n;
    return n;
}

// The shapes the relaxed job's launches take (kernels_strip.hip, kernels_source.hip): a plane below 4 GiB,
// fewer than 2^30 planes, at most 65535 groups of 4 rows
bool relax_job_runs(const stencil_layout& l) {
    const int64_t es = l.prob.dtype == STENCIL_F32 ? 4 : 8;
    return (l.plane + l.row + 64) * es < (int64_t(1) << 32) && l.prob.nz + 2 * kSourceSteps < (int64_t(1) << 30) &&
           (l.prob.ny + 3) / 4 <= 65535;
}

// Resolve `levels` (0: as many as there are) for `fine` and lay every level out; refuses a count the
// problem does not have and a level the relaxed job cannot run.
int mg_levels(const stencil_problem* fine, int32_t levels, std::vector<stencil_layout>* out) {
    if (int rc = check_mg_problem(fine)) return rc;
    const int most = max_levels(*fine);
    if (levels < 0 || levels > most)
        return set_error(STENCIL_EINVAL,
                         "levels = %d: a %lld x %lld x %lld grid has 1 .. %d (every extent odd and >= 3 to coarsen; 0 = all)",
                         levels, (long long)fine->nx, (long long)fine->ny, (long long)fine->nz, most);
    const int n = levels == 0 ? most : levels;
    stencil_problem p = *fine;
    for (int i = 0; i < n; ++i) {
        stencil_layout l;
        if (int rc = stencil_layout_init(&p, &l)) return rc;
        if (!relax_job_runs(l))
            return set_error(STENCIL_EUNSUPPORTED,
                             "multigrid: %d levels: level %d (%lld x %lld x %lld) is a shape the relaxed sweeps cannot run",
                             n, i, (long long)p.nx, (long long)p.ny, (long long)p.nz);
        out->push_back(l);
        p = coarsened(p);
    }
    return STENCIL_OK;
}

struct MgScratch {  // stream-ordered device scratch of the norm kernels
    double* dev = nullptr;
    hipStream_t s = nullptr;
    ~MgScratch() {
        if (dev) (void)hipFreeAsync(dev, s);
    }
};

// The per-plane residual norms of planes [begin, end) into host[0 .. n) (maxima) and host[n .. 2n) (sums);
// blocks until they have arrived.
int residual_norms_to_host(const stencil_layout& l, const void* u, const void* g, int64_t begin, int64_t end, double* host,
                           hipStream_t s) {
    const int64_t n = end - begin;
    if (n <= 0) {
        STENCIL_HIP_CHECK(hipStreamSynchronize(s));
        return STENCIL_OK;
    }
    MgScratch sc;
    sc.s = s;
    STENCIL_HIP_CHECK(hipMallocAsync(reinterpret_cast<void**>(&sc.dev), size_t(rn_workspace_bytes(l, n)), s));
    const int rc = l.prob.dtype == STENCIL_F32 ? launch_rn<float>(l, u, g, begin, end, sc.dev, s)
                                               : launch_rn<double>(l, u, g, begin, end, sc.dev, s);
    if (rc) return rc;
    STENCIL_HIP_CHECK(hipMemcpyAsync(host, sc.dev, size_t(2 * n) * sizeof(double), hipMemcpyDeviceToHost, s));
    STENCIL_HIP_CHECK(hipStreamSynchronize(s));
    return STENCIL_OK;
}

// stencil_diff_norms' scalar norm of per-plane values
double mg_scalar_norm(const double* host, int64_t n, int32_t norm) {
    double m = 0.0, s = 0.0;
    bool nan = false;
    for (int64_t u = 0; u < n; ++u) {
        nan = nan || host[u] != host[u];
        m = std::max(m, host[u]);
        s += host[n + u];
    }
    if (nan) return std::numeric_limits<double>::quiet_NaN();
    return norm == STENCIL_NORM_MAX ? m : std::sqrt(s);
}

int mg_restrict(const stencil_layout& lf, const void* u, const void* g, const stencil_layout& lc, void* gc, int64_t cbegin,
                int64_t cend, hipStream_t s) {
    return lf.prob.dtype == STENCIL_F32 ? launch_restrict<float>(lf, u, g, lc, gc, cbegin, cend, s)
                                        : launch_restrict<double>(lf, u, g, lc, gc, cbegin, cend, s);
}

int mg_prolong(const stencil_layout& lc, const void* e, const stencil_layout& lf, void* u, int64_t begin, int64_t end,
               hipStream_t s) {
    return lf.prob.dtype == STENCIL_F32 ? launch_prolong<float>(lc, e, lf, u, begin, end, s)
                                        : launch_prolong<double>(lc, e, lf, u, begin, end, s);
}

// `sweeps` relaxed sweeps on a level: stencil_iterate_relax's job from the level's field, phase 0
int mg_smooth(stencil_mg::Level& v, uint32_t sweeps, const stencil_mg_params& p, void* stream) {
    if (sweeps == 0) return STENCIL_OK;
    int fin = 0;
    if (int rc = stencil_iterate_relax(&v.lay, v.field[v.cur], v.field[v.cur ^ 1], v.src, sweeps, p.omegas, p.period, 0,
                                       stream, &fin, nullptr))
        return rc;
    if (fin) v.cur ^= 1;
    return STENCIL_OK;
}

int mg_cycle(stencil_mg* mg, size_t level, const stencil_mg_params& p, void* stream) {
    stencil_mg::Level& v = mg->lv[level];
    if (level + 1 == mg->lv.size()) return mg_smooth(v, p.coarse_sweeps, p, stream);
    stencil_mg::Level& c = mg->lv[level + 1];
    hipStream_t s = as_stream(stream);
    if (int rc = mg_smooth(v, p.pre, p, stream)) return rc;
    if (int rc = mg_restrict(v.lay, v.field[v.cur], v.src, c.lay, c.src, 0, c.lay.prob.nz, s)) return rc;
    // the coarse error starts from zero, ghost cells included (the other grid's ghost cells are zero since
    // creation: no sweep stores to a ghost cell)
    STENCIL_HIP_CHECK(hipMemsetAsync(c.field[c.cur], 0, size_t(c.lay.bytes), s));
    if (int rc = mg_cycle(mg, level + 1, p, stream)) return rc;
    if (int rc = mg_prolong(c.lay, c.field[c.cur], v.lay, v.field[v.cur], 0, v.lay.prob.nz, s)) return rc;
    return mg_smooth(v, p.post, p, stream);
}

int mg_restrict_source(const stencil_layout& lf, const void* g, const stencil_layout& lc, void* gc, int64_t cbegin,
                       int64_t cend, hipStream_t s) {
    return lf.prob.dtype == STENCIL_F32 ? launch_restrict_source<float>(lf, g, lc, gc, cbegin, cend, s)
                                        : launch_restrict_source<double>(lf, g, lc, gc, cbegin, cend, s);
}

int mg_inject(const stencil_layout& lf, const void* u, const stencil_layout& lc, void* uc0, void* uc1, hipStream_t s) {
    return lf.prob.dtype == STENCIL_F32 ? launch_inject<float>(lf, u, lc, uc0, uc1, s)
                                        : launch_inject<double>(lf, u, lc, uc0, uc1, s);
}

int mg_prolong_cubic(const stencil_layout& lc, const void* e, const stencil_layout& lf, void* u, int64_t begin, int64_t end,
                     hipStream_t s) {
    return lf.prob.dtype == STENCIL_F32 ? launch_prolong_cubic<float>(lc, e, lf, u, begin, end, s)
                                        : launch_prolong_cubic<double>(lc, e, lf, u, begin, end, s);
}

// Both field grids of a level to zero, ghost cells included
int mg_zero_fields(stencil_mg::Level& v, hipStream_t s) {
    STENCIL_HIP_CHECK(hipMemsetAsync(v.field[0], 0, size_t(v.lay.bytes), s));
    STENCIL_HIP_CHECK(hipMemsetAsync(v.field[1], 0, size_t(v.lay.bytes), s));
    return STENCIL_OK;
}

// The full multigrid pass (include/stencil_hip.h "Full multigrid")
int mg_fmg(stencil_mg* mg, const stencil_mg_params& p, uint32_t cycles, void* stream) {
    hipStream_t s = as_stream(stream);
    const size_t L = mg->lv.size();
    // 1. the coarse problems: sources, and the Dirichlet data in both field grids
    for (size_t l = 0; l + 1 < L; ++l) {
        stencil_mg::Level &f = mg->lv[l], &c = mg->lv[l + 1];
        if (int rc = mg_restrict_source(f.lay, f.src, c.lay, c.src, 0, c.lay.prob.nz, s)) return rc;
        if (int rc = mg_zero_fields(c, s)) return rc;
        if (int rc = mg_inject(f.lay, f.field[f.cur], c.lay, c.field[0], c.field[1], s)) return rc;
    }
    // 2. the coarsest level from a zero interior
    stencil_mg::Level& last = mg->lv[L - 1];
    if (L == 1) {  // the caller's ghost cells stay: the interior alone is zeroed, plane by plane
        const stencil_layout& lay = last.lay;
        const size_t es = lay.prob.dtype == STENCIL_F32 ? 4 : 8;
        char* base = static_cast<char*>(last.field[last.cur]) + size_t(lay.origin) * es;
        for (int64_t z = 0; z < lay.prob.nz; ++z)
            STENCIL_HIP_CHECK(hipMemset2DAsync(base + size_t(z * lay.plane) * es, size_t(lay.row) * es, 0,
                                               size_t(lay.prob.nx) * es, size_t(lay.prob.ny), s));
    }
    if (int rc = mg_smooth(last, p.coarse_sweeps, p, stream)) return rc;
    // 3. upward: the cubic prolongation as the starting guess, then `cycles` V-cycles from that level.  The
    // coarse level goes back to zero in BOTH grids first: mg_cycle zeroes field[cur] alone and relies on the
    // other grid's ghost cells being zero, which the injection of step 1 broke.
    for (size_t l = L - 1; l-- > 0;) {
        stencil_mg::Level &f = mg->lv[l], &c = mg->lv[l + 1];
        if (int rc = mg_prolong_cubic(c.lay, c.field[c.cur], f.lay, f.field[f.cur], 0, f.lay.prob.nz, s)) return rc;
        if (int rc = mg_zero_fields(c, s)) return rc;
        for (uint32_t i = 0; i < cycles; ++i)
            if (int rc = mg_cycle(mg, l, p, stream)) return rc;
    }
    return STENCIL_OK;
}

// The kernel launches of one V-cycle started at level `from` (stencil_mg_plan's count for from = 0)
int cycle_launches(const std::vector<stencil_layout>& lays, size_t from, const stencil_mg_params& p, int64_t* total) {
    for (size_t i = from; i < lays.size(); ++i) {
        const bool coarsest = i + 1 == lays.size();
        const uint32_t runs[2] = {coarsest ? p.coarse_sweeps : p.pre, coarsest ? 0u : p.post};
        for (uint32_t sweeps : runs) {
            int64_t n = 0;
            if (int rc = stencil_relax_plan(&lays[i], sweeps, &n, nullptr)) return rc;
            *total += n;
        }
        if (!coarsest) *total += restrict_launches(lays[i + 1].prob.nz) + prolong_launches(lays[i].prob.nz);
    }
    return STENCIL_OK;
}

void mg_release(stencil_mg* mg) {
    for (auto& v : mg->lv) {
        if (v.field[0]) (void)hipFree(v.field[0]);
        if (v.field[1]) (void)hipFree(v.field[1]);
        if (v.src) (void)hipFree(v.src);
    }
    delete mg;
}

}  // namespace
}  // namespace stencil

using namespace stencil;

extern "C" {

int stencil_coarsen_problem(const stencil_problem* fine, stencil_problem* coarse) {
    if (int rc = check_mg_problem(fine)) return rc;
    if (!coarse) return set_error(STENCIL_EINVAL, "null coarse problem");
    if (!coarsenable(*fine))
        return set_error(STENCIL_EINVAL, "a %lld x %lld x %lld grid does not coarsen: every extent must be odd and >= 3",
                         (long long)fine->nx, (long long)fine->ny, (long long)fine->nz);
    *coarse = coarsened(*fine);
    clear_error();
    return STENCIL_OK;
}

int stencil_residual_norms(const stencil_layout* l, const void* u, const void* src, int64_t begin, int64_t end,
                           double* max_abs, double* sum_sq, void* stream) {
    if (int rc = check_mg_layout(l, "grid's")) return rc;
    if (!u || !src || u == src) return set_error(STENCIL_EINVAL, "need two distinct grids (the field and the source)");
    if (!max_abs && !sum_sq) return set_error(STENCIL_EINVAL, "need max_abs or sum_sq");
    if (begin < 0 || end > l->prob.nz || begin > end)
        return set_error(STENCIL_EINVAL, "plane range [%lld, %lld) out of bounds [0, %lld)", (long long)begin, (long long)end,
                         (long long)l->prob.nz);
    const int64_t n = end - begin;
    std::vector<double> host(size_t(2 * n));
    if (int rc = residual_norms_to_host(*l, u, src, begin, end, host.data(), as_stream(stream))) return rc;
    if (max_abs) std::copy_n(host.data(), n, max_abs);
    if (sum_sq) std::copy_n(host.data() + n, n, sum_sq);
    clear_error();
    return STENCIL_OK;
}

int stencil_restrict_residual(const stencil_layout* lf, const void* u, const void* src, const stencil_layout* lc,
                              void* coarse_src, int64_t cbegin, int64_t cend, void* stream) {
    if (int rc = check_mg_pair(lf, lc)) return rc;
    if (!u || !src || !coarse_src) return set_error(STENCIL_EINVAL, "null grid");
    if (u == src || u == coarse_src || src == coarse_src)
        return set_error(STENCIL_EINVAL, "the field, the source and the coarse source must be three distinct grids");
    if (cbegin < 0 || cend > lc->prob.nz || cbegin > cend)
        return set_error(STENCIL_EINVAL, "coarse plane range [%lld, %lld) out of bounds [0, %lld)", (long long)cbegin,
                         (long long)cend, (long long)lc->prob.nz);
    const int rc = mg_restrict(*lf, u, src, *lc, coarse_src, cbegin, cend, as_stream(stream));
    if (rc == STENCIL_OK) clear_error();
    return rc;
}

int stencil_prolong_add(const stencil_layout* lc, const void* e, const stencil_layout* lf, void* u, int64_t begin,
                        int64_t end, void* stream) {
    if (int rc = check_mg_pair(lf, lc)) return rc;
    if (!e || !u) return set_error(STENCIL_EINVAL, "null grid");
    if (e == u) return set_error(STENCIL_EINVAL, "the coarse and the fine grid must be distinct");
    if (begin < 0 || end > lf->prob.nz || begin > end)
        return set_error(STENCIL_EINVAL, "fine plane range [%lld, %lld) out of bounds [0, %lld)", (long long)begin,
                         (long long)end, (long long)lf->prob.nz);
    const int rc = mg_prolong(*lc, e, *lf, u, begin, end, as_stream(stream));
    if (rc == STENCIL_OK) clear_error();
    return rc;
}

int stencil_mg_create(const stencil_problem* fine, int32_t levels, stencil_mg** mg) {
    if (!mg) return set_error(STENCIL_EINVAL, "null out pointer");
    *mg = nullptr;
    std::vector<stencil_layout> lays;
    if (int rc = mg_levels(fine, levels, &lays)) return rc;
    stencil_mg* m = new (std::nothrow) stencil_mg;
    if (!m) return set_error(STENCIL_ENOMEM, "out of host memory");
    m->lv.resize(lays.size());
    for (size_t i = 0; i < lays.size(); ++i) {
        stencil_mg::Level& v = m->lv[i];
        v.lay = lays[i];
        void** grids[3] = {&v.field[0], &v.field[1], &v.src};
        for (void** g : grids) {
            int rc = stencil_alloc(&v.lay, g);
            if (rc == STENCIL_OK && hipMemset(*g, 0, size_t(v.lay.bytes) + 256) != hipSuccess)
                rc = set_error(STENCIL_EHIP, "zeroing a multigrid level failed");
            if (rc) {
                mg_release(m);
                return rc;
            }
        }
    }
    *mg = m;
    clear_error();
    return STENCIL_OK;
}

int stencil_mg_destroy(stencil_mg* mg) {
    if (!mg) return STENCIL_OK;
    mg_release(mg);
    return STENCIL_OK;
}

int stencil_mg_levels(const stencil_mg* mg, int32_t* levels) {
    if (!mg || !levels) return set_error(STENCIL_EINVAL, "null hierarchy or out pointer");
    *levels = int32_t(mg->lv.size());
    return STENCIL_OK;
}

int stencil_mg_level(const stencil_mg* mg, int32_t level, stencil_layout* out, void** field, void** source) {
    if (!mg) return set_error(STENCIL_EINVAL, "null hierarchy");
    if (level < 0 || size_t(level) >= mg->lv.size())
        return set_error(STENCIL_EINVAL, "level %d of a hierarchy of %zu", level, mg->lv.size());
    const stencil_mg::Level& v = mg->lv[size_t(level)];
    if (out) *out = v.lay;
    if (field) *field = v.field[v.cur];
    if (source) *source = v.src;
    return STENCIL_OK;
}

int stencil_mg_upload(stencil_mg* mg, const void* field, const void* source, int64_t host_row, int64_t host_rows,
                      void* stream) {
    if (!mg) return set_error(STENCIL_EINVAL, "null hierarchy");
    if (!field && !source) return set_error(STENCIL_EINVAL, "need a field or a source array");
    stencil_mg::Level& v = mg->lv[0];
    if (field) {
        // both grids: the relaxed jobs ping-pong between them and need the field's ghost cells in each
        if (int rc = stencil_upload(&v.lay, v.field[0], field, host_row, host_rows, stream)) return rc;
        if (int rc = stencil_upload(&v.lay, v.field[1], field, host_row, host_rows, stream)) return rc;
    }
    if (source)
        if (int rc = stencil_upload(&v.lay, v.src, source, host_row, host_rows, stream)) return rc;
    clear_error();
    return STENCIL_OK;
}

int stencil_mg_download(const stencil_mg* mg, void* field, void* source, int64_t host_row, int64_t host_rows,
                        void* stream) {
    if (!mg) return set_error(STENCIL_EINVAL, "null hierarchy");
    if (!field && !source) return set_error(STENCIL_EINVAL, "need a field or a source array");
    const stencil_mg::Level& v = mg->lv[0];
    if (field)
        if (int rc = stencil_download(&v.lay, v.field[v.cur], field, host_row, host_rows, stream)) return rc;
    if (source)
        if (int rc = stencil_download(&v.lay, v.src, source, host_row, host_rows, stream)) return rc;
    clear_error();
    return STENCIL_OK;
}

int stencil_mg_vcycle(stencil_mg* mg, const stencil_mg_params* params, void* stream) {
    if (!mg) return set_error(STENCIL_EINVAL, "null hierarchy");
    if (int rc = check_mg_params(params)) return rc;
    if (int rc = mg_cycle(mg, 0, *params, stream)) return rc;
    clear_error();
    return STENCIL_OK;
}

int stencil_mg_solve(stencil_mg* mg, const stencil_mg_params* params, uint32_t max_cycles, uint32_t check_every,
                     int32_t norm, double tol, void* stream, uint32_t* cycles_done, double* last_norm, int* converged,
                     float* elapsed_ms) {
    if (!mg) return set_error(STENCIL_EINVAL, "null hierarchy");
    if (int rc = check_mg_params(params)) return rc;
    if (check_every == 0) return set_error(STENCIL_EINVAL, "check_every must be at least 1");
    if (!(tol >= 0.0)) return set_error(STENCIL_EINVAL, "tol must be a number >= 0");
    if (norm != STENCIL_NORM_MAX && norm != STENCIL_NORM_L2) return set_error(STENCIL_EINVAL, "bad norm %d", norm);
    hipStream_t s = as_stream(stream);
    struct Events {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ~Events() {
            if (e0) (void)hipEventDestroy(e0);
            if (e1) (void)hipEventDestroy(e1);
        }
    } ev;
    stencil_mg::Level& v = mg->lv[0];
    const int64_t n = v.lay.prob.nz;
    std::vector<double> host(size_t(2 * n));
    uint32_t done = 0;
    int conv = 0;
    double last = std::numeric_limits<double>::infinity();
    if (max_cycles > 0 && elapsed_ms) {
        STENCIL_HIP_CHECK(hipEventCreate(&ev.e0));
        STENCIL_HIP_CHECK(hipEventCreate(&ev.e1));
        STENCIL_HIP_CHECK(hipEventRecord(ev.e0, s));
    }
    while (done < max_cycles) {
        const uint32_t block = std::min(check_every, max_cycles - done);
        for (uint32_t i = 0; i < block; ++i)
            if (int rc = mg_cycle(mg, 0, *params, stream)) return rc;
        done += block;
        if (int rc = residual_norms_to_host(v.lay, v.field[v.cur], v.src, 0, n, host.data(), s)) return rc;
        last = mg_scalar_norm(host.data(), n, norm);
        if (last <= tol) {
            conv = 1;
            break;
        }
        if (last != last) break;
    }
    if (elapsed_ms) {
        *elapsed_ms = 0.f;
        if (ev.e0) {
            STENCIL_HIP_CHECK(hipEventRecord(ev.e1, s));
            STENCIL_HIP_CHECK(hipEventSynchronize(ev.e1));
            STENCIL_HIP_CHECK(hipEventElapsedTime(elapsed_ms, ev.e0, ev.e1));
        }
    }
    if (cycles_done) *cycles_done = done;
    if (last_norm) *last_norm = last;
    if (converged) *converged = conv;
    clear_error();
    return STENCIL_OK;
}

int stencil_mg_plan(const stencil_problem* fine, int32_t levels, const stencil_mg_params* params, int64_t* launches,
                    int32_t* levels_out) {
    std::vector<stencil_layout> lays;
    if (int rc = mg_levels(fine, levels, &lays)) return rc;
    if (int rc = check_mg_params(params)) return rc;
    int64_t total = 0;
    if (int rc = cycle_launches(lays, 0, *params, &total)) return rc;
    if (launches) *launches = total;
    if (levels_out) *levels_out = int32_t(lays.size());
    clear_error();
    return STENCIL_OK;
}

int stencil_restrict_source(const stencil_layout* lf, const void* src, const stencil_layout* lc, void* coarse_src,
                            int64_t cbegin, int64_t cend, void* stream) {
    if (int rc = check_mg_pair(lf, lc)) return rc;
    if (!src || !coarse_src) return set_error(STENCIL_EINVAL, "null grid");
    if (src == coarse_src) return set_error(STENCIL_EINVAL, "the source and the coarse source must be distinct grids");
    if (cbegin < 0 || cend > lc->prob.nz || cbegin > cend)
        return set_error(STENCIL_EINVAL, "coarse plane range [%lld, %lld) out of bounds [0, %lld)", (long long)cbegin,
                         (long long)cend, (long long)lc->prob.nz);
    const int rc = mg_restrict_source(*lf, src, *lc, coarse_src, cbegin, cend, as_stream(stream));
    if (rc == STENCIL_OK) clear_error();
    return rc;
}

int stencil_inject_ghosts(const stencil_layout* lf, const void* u, const stencil_layout* lc, void* uc, void* stream) {
    if (int rc = check_mg_pair(lf, lc)) return rc;
    if (!u || !uc) return set_error(STENCIL_EINVAL, "null grid");
    if (u == uc) return set_error(STENCIL_EINVAL, "the fine and the coarse grid must be distinct");
    const int rc = mg_inject(*lf, u, *lc, uc, nullptr, as_stream(stream));
    if (rc == STENCIL_OK) clear_error();
    return rc;
}

int stencil_prolong_cubic(const stencil_layout* lc, const void* e, const stencil_layout* lf, void* u, int64_t begin,
                          int64_t end, void* stream) {
    if (int rc = check_mg_pair(lf, lc)) return rc;
    if (!e || !u) return set_error(STENCIL_EINVAL, "null grid");
    if (e == u) return set_error(STENCIL_EINVAL, "the coarse and the fine grid must be distinct");
    if (begin < 0 || end > lf->prob.nz || begin > end)
        return set_error(STENCIL_EINVAL, "fine plane range [%lld, %lld) out of bounds [0, %lld)", (long long)begin,
                         (long long)end, (long long)lf->prob.nz);
    const int rc = mg_prolong_cubic(*lc, e, *lf, u, begin, end, as_stream(stream));
    if (rc == STENCIL_OK) clear_error();
    return rc;
}

int stencil_mg_fmg(stencil_mg* mg, const stencil_mg_params* params, uint32_t cycles, void* stream) {
    if (!mg) return set_error(STENCIL_EINVAL, "null hierarchy");
    if (int rc = check_mg_params(params)) return rc;
    if (int rc = mg_fmg(mg, *params, cycles, stream)) return rc;
    clear_error();
    return STENCIL_OK;
}

int stencil_mg_fmg_plan(const stencil_problem* fine, int32_t levels, const stencil_mg_params* params, uint32_t cycles,
                        int64_t* launches, int32_t* levels_out) {
    std::vector<stencil_layout> lays;
    if (int rc = mg_levels(fine, levels, &lays)) return rc;
    if (int rc = check_mg_params(params)) return rc;
    int64_t total = 0, n = 0;
    if (int rc = stencil_relax_plan(&lays.back(), params->coarse_sweeps, &n, nullptr)) return rc;
    total += n;
    for (size_t l = 0; l + 1 < lays.size(); ++l) {
        total += restrict_launches(lays[l + 1].prob.nz) + 1 + cubic_launches(lays[l].prob.nz);
        int64_t one = 0;
        if (int rc = cycle_launches(lays, l, *params, &one)) return rc;
        total += int64_t(cycles) * one;
    }
    if (launches) *launches = total;
    if (levels_out) *levels_out = int32_t(lays.size());
    clear_error();
    return STENCIL_OK;
}

}  // extern "C"
