// kernels_source.hip -- one sweep of the 3D 7-point star (r = 1, naive order)
// with a source term: out(c) = fl(fl(sum6(in, c) * avg) + src(c)) at every
// interior cell of planes [begin, end).  The remainder of a
// source job (fewer sweeps than the fused launches of kernels_strip_source.hip
// take) and the single sweep before stencil_iterate_until_source's check.
//
// One cell column per lane, 64-lane rows along x, marched over a chunk of
// planes: the centre column's three planes stay in registers, the x / y
// neighbours are re-reads served by L1 / L2 (as kernels_direct.hip).  The sum
// is the plain sweep's (0 + x- + x+ + y- + y+ + z- + z+) * avg, rounded, and
// the source is added with a rounding of its own: the library is compiled with
// -ffp-contract=off, so the two never become one fma.  Only interior cells of
// `src` are read.
#include "common.hpp"

namespace stencil {
namespace {

constexpr int kSX = 64, kSY = 4;
constexpr int kSourceChunk = 16;  // planes per workgroup

template <typename T>
__global__ void __launch_bounds__(kSX * kSY)
    sweep_source1(const T* __restrict__ in, T* __restrict__ out, const T* __restrict__ src, Geom g, int64_t begin,
                  int64_t end, T avg) {
    const int64_t x = int64_t(blockIdx.x) * kSX + threadIdx.x;
    const int64_t y = int64_t(blockIdx.y) * kSY + threadIdx.y;
    if (x >= g.nx || y >= g.ny) return;
    const int64_t za = begin + int64_t(blockIdx.z) * kSourceChunk;
    const int64_t zb = za + kSourceChunk < end ? za + kSourceChunk : end;
    int64_t idx = g.origin + za * g.plane + y * g.row + x;
    T zm = in[idx - g.plane], c = in[idx];
    for (int64_t z = za; z < zb; ++z, idx += g.plane) {
        const T zp = in[idx + g.plane];
        T sum = T(0);
        sum += in[idx - 1];
        sum += in[idx + 1];
        sum += in[idx - g.row];
        sum += in[idx + g.row];
        sum += zm;
        sum += zp;
        const T avged = sum * avg;  // rounded here
        out[idx] = avged + src[idx];
        zm = c;
        c = zp;
    }
}

// The relaxed sibling (stencil_sweepk_relax and, on slab layouts, stencil_sweepk_relax_halo with steps = 1: a
// relaxed job's remainder of one, the sweep before stencil_iterate_until_relax's and stencil_slab_run_until_relax's
// check; a single sweep reads a halo side's planes of `in` and advances none): the same march and the same value J, then
// out(c) = fl(in(c) + fl(w * fl(J - in(c)))) -- the subtract, the multiply and the add each rounded.
template <typename T>
__global__ void __launch_bounds__(kSX * kSY)
    sweep_relax1(const T* __restrict__ in, T* __restrict__ out, const T* __restrict__ src, Geom g, int64_t begin,
                 int64_t end, T avg, T w) {
    const int64_t x = int64_t(blockIdx.x) * kSX + threadIdx.x;
    const int64_t y = int64_t(blockIdx.y) * kSY + threadIdx.y;
    if (x >= g.nx || y >= g.ny) return;
    const int64_t za = begin + int64_t(blockIdx.z) * kSourceChunk;
    const int64_t zb = za + kSourceChunk < end ? za + kSourceChunk : end;
    int64_t idx = g.origin + za * g.plane + y * g.row + x;
    T zm = in[idx - g.plane], c = in[idx];
    for (int64_t z = za; z < zb; ++z, idx += g.plane) {
        const T zp = in[idx + g.plane];
        T sum = T(0);
        sum += in[idx - 1];
        sum += in[idx + 1];
        sum += in[idx - g.row];
        sum += in[idx + g.row];
        sum += zm;
        sum += zp;
        const T avged = sum * avg;  // rounded here
        const T j = avged + src[idx];
        const T d = j - c;
        const T wd = w * d;
        out[idx] = c + wd;
        zm = c;
        c = zp;
    }
}

template <typename T>
int launch_s1(const stencil_layout& l, const void* in, void* out, const void* src, int64_t begin, int64_t end,
              hipStream_t s) {
    const Geom g = geom_of(l);
    const int64_t n = end - begin;
    if (n <= 0 || g.nx <= 0 || g.ny <= 0) return STENCIL_OK;
    const unsigned gx = unsigned((g.nx + kSX - 1) / kSX), gy = unsigned((g.ny + kSY - 1) / kSY);
    if ((g.ny + kSY - 1) / kSY > 65535) return set_error(STENCIL_EINVAL, "grid too tall for the source sweep");
    constexpr int64_t kSpan = int64_t(65535) * kSourceChunk;  // planes per launch (grid z limit)
    for (int64_t z0 = begin; z0 < end; z0 += kSpan) {
        const int64_t z1 = std::min(end, z0 + kSpan);
        const unsigned gz = unsigned((z1 - z0 + kSourceChunk - 1) / kSourceChunk);
        hipLaunchKernelGGL(sweep_source1<T>, dim3(gx, gy, gz), dim3(kSX, kSY, 1), 0, s, static_cast<const T*>(in),
                           static_cast<T*>(out), static_cast<const T*>(src), g, z0, z1, avg_weight<T>(l.prob));
        STENCIL_LAUNCH_CHECK();
    }
    return STENCIL_OK;
}

template <typename T>
int launch_r1(const stencil_layout& l, const void* in, void* out, const void* src, int64_t begin, int64_t end, double omega,
              hipStream_t s) {
    const Geom g = geom_of(l);
    const int64_t n = end - begin;
    if (n <= 0 || g.nx <= 0 || g.ny <= 0) return STENCIL_OK;
    const unsigned gx = unsigned((g.nx + kSX - 1) / kSX), gy = unsigned((g.ny + kSY - 1) / kSY);
    if ((g.ny + kSY - 1) / kSY > 65535) return set_error(STENCIL_EINVAL, "grid too tall for the relaxed sweep");
    constexpr int64_t kSpan = int64_t(65535) * kSourceChunk;  // planes per launch (grid z limit)
    for (int64_t z0 = begin; z0 < end; z0 += kSpan) {
        const int64_t z1 = std::min(end, z0 + kSpan);
        const unsigned gz = unsigned((z1 - z0 + kSourceChunk - 1) / kSourceChunk);
        hipLaunchKernelGGL(sweep_relax1<T>, dim3(gx, gy, gz), dim3(kSX, kSY, 1), 0, s, static_cast<const T*>(in),
                           static_cast<T*>(out), static_cast<const T*>(src), g, z0, z1, avg_weight<T>(l.prob), T(omega));
        STENCIL_LAUNCH_CHECK();
    }
    return STENCIL_OK;
}

}  // namespace

int launch_source1(const stencil_layout& l, const void* in, void* out, const void* src, int64_t begin, int64_t end,
                   hipStream_t s) {
    if (!temporal2_supports(l.prob))
        return set_error(STENCIL_EUNSUPPORTED, "source sweeps cover the 3D r=1 naive 7-point star only");
    return l.prob.dtype == STENCIL_F32 ? launch_s1<float>(l, in, out, src, begin, end, s)
                                       : launch_s1<double>(l, in, out, src, begin, end, s);
}

int launch_relax1(const stencil_layout& l, const void* in, void* out, const void* src, int64_t begin, int64_t end,
                  double omega, hipStream_t s) {
    if (!temporal2_supports(l.prob))
        return set_error(STENCIL_EUNSUPPORTED, "relaxed sweeps cover the 3D r=1 naive 7-point star only");
    return l.prob.dtype == STENCIL_F32 ? launch_r1<float>(l, in, out, src, begin, end, omega, s)
                                       : launch_r1<double>(l, in, out, src, begin, end, omega, s);
}

}  // namespace stencil
