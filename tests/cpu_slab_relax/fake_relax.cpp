// fake_relax.cpp -- TEST INFRASTRUCTURE ONLY: slab_core.hpp's relaxed rounds
// (run_relax / relax_round_form, beside set_source / run_source / run) on the
// CPU fake device of tests/cpu_slab_source/, so that real send / recv between
// slabs runs under `pytest -m "not gpu"` at world 2 and 3.
//
// This one translation unit includes tests/cpu_slab_source/fake_source.cpp
// unchanged (its fake_slab_* and fake_source_* exports come along: the library
// is self-contained) and derives a device that adds the relaxed launches.
// sweepk_relax is `k` times: one oracle sweep of the extracted sub-grid, the
// add of the source, then the relaxation's three separately rounded operations
// (the difference, its weighting, the sum) on every non-ghost cell of that
// sub-grid -- fake_source.cpp's construction, so stage s is right on planes
// [-(k - s), nz + k - s) of a halo side and every advanced halo cell takes the
// source of its own plane and the stage's weight: stencil_sweepk_relax_halo's
// definition.  Built with -ffp-contract=off: no operation pair becomes an fma.
#include "../cpu_slab_source/fake_source.cpp"

namespace stencil {

namespace fake {
int64_t g_relax_sweeps = 0, g_relax_signal_sweeps = 0;
}  // namespace fake

struct FakeRelaxDev : FakeSourceDev {
    template <typename T>
    static int relax_t(const stencil_layout* l, const T* in, T* out, const T* rhs, int64_t b, int64_t e, int k,
                       const double* omegas) {
        const stencil_problem& p = l->prob;
        const int64_t r = p.radius, zg = l->zghost, n = p.nz;
        const int64_t lo_bound = (p.flags & STENCIL_HALO_LO) ? -zg : -r;
        const int64_t hi_bound = (p.flags & STENCIL_HALO_HI) ? n + zg : n + r;
        const int64_t zlo = std::max(b - int64_t(k) * r, lo_bound), zhi = std::min(e + int64_t(k) * r, hi_bound);
        oracle_problem op{};
        op.dims = 3;
        op.dtype = p.dtype == STENCIL_F64 ? ORACLE_F64 : ORACLE_F32;
        op.shape = ORACLE_STAR;
        op.radius = int32_t(r);
        op.order = ORACLE_ORDER_NAIVE;
        op.nx = p.nx;
        op.ny = p.ny;
        op.nz = (zhi - zlo) - 2 * r;
        if (op.nz < e - b)
            return set_error(STENCIL_EINVAL, "fake relaxed sweep: range [%lld, %lld) beyond the readable planes",
                             (long long)b, (long long)e);
        const int64_t sx = p.nx + 2 * r, sy = p.ny + 2 * r;
        std::vector<T> A(size_t(sx * sy * (zhi - zlo))), B;
        for (int64_t z = zlo; z < zhi; ++z)
            for (int64_t y = -r; y < p.ny + r; ++y)
                std::memcpy(&A[size_t(((z - zlo) * sy + (y + r)) * sx)], in + l->origin + z * l->plane + y * l->row - r,
                            size_t(sx) * sizeof(T));
        B = A;
        std::vector<T>* cur = &A;
        std::vector<T>* nxt = &B;
        for (int s = 0; s < k; ++s) {
            const int in_b = oracle_run(&op, 1, cur->data(), nxt->data(), 1);
            if (in_b != 1) return set_error(STENCIL_EINVAL, "fake relaxed sweep: oracle error %d", in_b);
            const T w = T(omegas[s]);  // rounded once to the grid's type
            for (int64_t z = zlo + r; z < zhi - r; ++z)
                for (int64_t y = 0; y < p.ny; ++y) {
                    const size_t at = size_t(((z - zlo) * sy + (y + r)) * sx + r);
                    T* d = &(*nxt)[at];
                    const T* c = &(*cur)[at];
                    const T* g = rhs + l->origin + z * l->plane + y * l->row;
                    for (int64_t x = 0; x < p.nx; ++x) {
                        const T j = d[x] + g[x];  // the source sweep's value
                        const T diff = j - c[x];
                        const T wd = w * diff;
                        d[x] = c[x] + wd;
                    }
                }
            std::swap(cur, nxt);
        }
        for (int64_t z = b; z < e; ++z)
            for (int64_t y = 0; y < p.ny; ++y)
                std::memcpy(out + l->origin + z * l->plane + y * l->row, &(*cur)[size_t(((z - zlo) * sy + (y + r)) * sx + r)],
                            size_t(p.nx) * sizeof(T));
        return STENCIL_OK;
    }
    static int sweepk_relax(const stencil_layout* l, const void* in, void* out, const void* src, int64_t b, int64_t e,
                            int k, const double* w, Stream) {
        if (b < 0 || e > l->prob.nz || b > e || k < 1 || k > STENCIL_SOURCE_MAX_STEPS || !src || !w)
            return set_error(STENCIL_EINVAL, "fake relaxed sweep: bad range, steps, source or weights");
        for (int i = 0; i < k; ++i)
            if (!std::isfinite(w[i])) return set_error(STENCIL_EINVAL, "fake relaxed sweep: weight %d is not finite", i);
        if ((l->prob.flags & (STENCIL_HALO_LO | STENCIL_HALO_HI)) && l->zghost < k)
            return set_error(STENCIL_EINVAL, "fake relaxed sweep: %d steps need halo >= %d", k, k);
        {
            std::lock_guard<std::mutex> lk(fake::g_stat_mu);
            ++fake::g_relax_sweeps;
        }
        if (b == e) return STENCIL_OK;
        return l->prob.dtype == STENCIL_F64 ? relax_t(l, static_cast<const double*>(in), static_cast<double*>(out),
                                                      static_cast<const double*>(src), b, e, k, w)
                                            : relax_t(l, static_cast<const float*>(in), static_cast<float*>(out),
                                                      static_cast<const float*>(src), b, e, k, w);
    }
    // the fake has no CUs: FAKE_SLAB_RELAX_GATE=0 makes a gated job's relaxed launches ungated
    static bool relax_halo_gate(const stencil_layout&, int, bool) {
        const char* v = std::getenv("FAKE_SLAB_RELAX_GATE");
        return !(v && *v && std::atoi(v) == 0);
    }
    static int sweepk_signal_relax(const stencil_layout* l, const void* in, void* out, const void* src, int64_t b,
                                   int64_t e, int k, const double* w, uint32_t* counters, uint64_t*, int* nsig, Stream s) {
        if (k < 3 || e - b < k) return set_error(STENCIL_EINVAL, "fake signalled relaxed sweep: steps 3..4, >= steps planes");
        if (int rc = sweepk_relax(l, in, out, src, b, e, k, w, s)) return rc;
        {
            std::lock_guard<std::mutex> lk(fake::g_stat_mu);
            ++fake::g_relax_signal_sweeps;
        }
        counters[0] += 1;
        counters[1] += 1;
        *nsig = 1;
        return STENCIL_OK;
    }
    static int sweepk_signal_relax_gated(const stencil_layout* l, const void* in, void* out, const void* src, int64_t b,
                                         int64_t e, int k, const double* w, uint32_t* counters, uint64_t* fsig,
                                         uint32_t need, uint32_t*, int* nsig, Stream s) {
        {
            std::lock_guard<std::mutex> lk(fake::g_stat_mu);
            ++fake::g_gated;
            if (int32_t(counters[3] - need) < 0 || counters[3] != need) ++fake::g_gate_bad;
        }
        return sweepk_signal_relax(l, in, out, src, b, e, k, w, counters, fsig, nsig, s);
    }
};

}  // namespace stencil

struct fake_relax_job : stencil::slab::Job<stencil::FakeRelaxDev> {};

using stencil::FakeRelaxDev;

extern "C" {

// the plain and the source calls a relaxed job needs, on Job<FakeRelaxDev>
int fake_relax_create2(const stencil_problem* g, int32_t n, const int32_t* devs, int32_t ex, int32_t flags, int64_t margin,
                       fake_relax_job** job) {
    return core::create<FakeRelaxDev>(g, n, devs, ex, flags, margin, job);
}
int fake_relax_create_rank2(const stencil_problem* g, int32_t nranks, int32_t rank, int32_t dev, const void* id,
                            int64_t id_bytes, int32_t flags, int64_t margin, fake_relax_job** job) {
    return core::create_rank<FakeRelaxDev>(g, nranks, rank, dev, id, id_bytes, flags, margin, job);
}
int fake_relax_destroy(fake_relax_job* job) {
    core::release<FakeRelaxDev>(job);
    return STENCIL_OK;
}
int fake_relax_info(const fake_relax_job* job, int32_t slab, int64_t* first, int64_t* planes, int32_t* dev, int32_t* k) {
    return core::info<FakeRelaxDev>(job, slab, first, planes, dev, k);
}
int fake_relax_fill_initial(fake_relax_job* job, int32_t kind, uint64_t seed) {
    return core::fill_initial<FakeRelaxDev>(job, kind, seed);
}
int fake_relax_upload(fake_relax_job* job, const void* host, int64_t row, int64_t rows) {
    return core::upload<FakeRelaxDev>(job, host, row, rows);
}
int fake_relax_download(fake_relax_job* job, void* host, int64_t row, int64_t rows) {
    return core::download<FakeRelaxDev>(job, host, row, rows);
}
int fake_relax_run(fake_relax_job* job, uint32_t iterations, float* ms) {
    return core::run<FakeRelaxDev>(job, iterations, ms);
}
int fake_relax_round_form(const fake_relax_job* job, int32_t* form) {
    return core::round_form<FakeRelaxDev>(job, form);
}
int fake_relax_round_info(const fake_relax_job* job, int32_t* form, int32_t* gated, int32_t* confined) {
    return core::round_info<FakeRelaxDev>(job, form, gated, confined);
}
int fake_relax_set_source(fake_relax_job* job, const void* host, int64_t row, int64_t rows) {
    return core::set_source<FakeRelaxDev>(job, host, row, rows);
}
int fake_relax_run_source(fake_relax_job* job, uint32_t iterations, float* ms) {
    return core::run_source<FakeRelaxDev>(job, iterations, ms);
}
int fake_relax_source_plan(const stencil_problem* g, uint32_t iterations, int64_t* rounds, int32_t* steps) {
    return core::source_plan<FakeRelaxDev>(g, iterations, rounds, steps);
}
int fake_relax_source_round_form(const fake_relax_job* job, int32_t* form) {
    return core::source_round_form<FakeRelaxDev>(job, form);
}

// the relaxed calls (stencil_slab_*_relax)
int fake_relax_run_relax(fake_relax_job* job, uint32_t iterations, const double* omegas, uint32_t period, uint32_t phase,
                         float* ms) {
    return core::run_relax<FakeRelaxDev>(job, iterations, omegas, period, phase, ms);
}
// (stencil_slab_run_until_relax is not here: its check runs kernels only the product has)
int fake_relax_relax_plan(const stencil_problem* g, uint32_t iterations, int64_t* rounds, int32_t* steps) {
    return core::source_plan<FakeRelaxDev>(g, iterations, rounds, steps);
}
int fake_relax_relax_round_form(const fake_relax_job* job, int32_t* form) {
    return core::relax_round_form<FakeRelaxDev>(job, form);
}

// {relaxed launches, of them face-signalled, source launches, of them face-signalled, plain launches, sends,
//  recvs, peer copies, gated launches, gate numbering violations}
void fake_relax_stats(int64_t* out10, int32_t reset) {
    std::lock_guard<std::mutex> lk(stencil::fake::g_stat_mu);
    out10[0] = stencil::fake::g_relax_sweeps;
    out10[1] = stencil::fake::g_relax_signal_sweeps;
    out10[2] = stencil::fake::g_source_sweeps;
    out10[3] = stencil::fake::g_source_signal_sweeps;
    out10[4] = stencil::fake::g_sweeps;
    out10[5] = stencil::fake::g_sends;
    out10[6] = stencil::fake::g_recvs;
    out10[7] = stencil::fake::g_peer_copies;
    out10[8] = stencil::fake::g_gated;
    out10[9] = stencil::fake::g_gate_bad;
    if (reset) {
        stencil::fake::g_relax_sweeps = stencil::fake::g_relax_signal_sweeps = 0;
        stencil::fake::g_source_sweeps = stencil::fake::g_source_signal_sweeps = 0;
        stencil::fake::g_sweeps = stencil::fake::g_signal_sweeps = 0;
        stencil::fake::g_sends = stencil::fake::g_recvs = stencil::fake::g_peer_copies = 0;
        stencil::fake::g_gated = stencil::fake::g_gate_bad = stencil::fake::g_xdone = 0;
    }
}

}  // extern "C"
