// fake_source.cpp -- TEST INFRASTRUCTURE ONLY: slab_core.hpp's source rounds
// (set_source / run_source / source_plan / source_round_form) on the CPU fake
// device of tests/cpu_slab/, so that real send / recv between slabs runs under
// `pytest -m "not gpu"` at world 2 and 3.
//
// This one translation unit includes tests/cpu_slab/fake_dev.cpp unchanged (its
// fake_slab_* exports come along: the library is self-contained) and derives a
// device that adds the source launches.  sweepk_source is `k` times one oracle
// sweep of the extracted sub-grid followed by the add of the source on every
// non-ghost cell of that sub-grid: the sub-grid reaches k planes beyond the
// range on a halo side, its outermost planes are its ghost planes, so stage s
// is right on planes [-(k - s), nz + k - s) there and every advanced halo cell
// gets the source of its own plane -- stencil_sweepk_source_halo's definition.
#include "../cpu_slab/fake_dev.cpp"

namespace stencil {

namespace fake {
int64_t g_source_sweeps = 0, g_source_signal_sweeps = 0;
bool g_source_signal = true;
}  // namespace fake

struct FakeSourceDev : FakeDev {
    template <typename T>
    static int source_t(const stencil_layout* l, const T* in, T* out, const T* rhs, int64_t b, int64_t e, int k) {
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
            return set_error(STENCIL_EINVAL, "fake source sweep: range [%lld, %lld) beyond the readable planes",
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
            // one sweep cur -> nxt (oracle_run leaves an odd count's result in its second buffer)
            const int in_b = oracle_run(&op, 1, cur->data(), nxt->data(), 1);
            if (in_b != 1) return set_error(STENCIL_EINVAL, "fake source sweep: oracle error %d", in_b);
            for (int64_t z = zlo + r; z < zhi - r; ++z)
                for (int64_t y = 0; y < p.ny; ++y) {
                    T* d = &(*nxt)[size_t(((z - zlo) * sy + (y + r)) * sx + r)];
                    const T* g = rhs + l->origin + z * l->plane + y * l->row;
                    for (int64_t x = 0; x < p.nx; ++x) d[x] = d[x] + g[x];  // a rounding of its own (-ffp-contract=off)
                }
            std::swap(cur, nxt);
        }
        for (int64_t z = b; z < e; ++z)
            for (int64_t y = 0; y < p.ny; ++y)
                std::memcpy(out + l->origin + z * l->plane + y * l->row, &(*cur)[size_t(((z - zlo) * sy + (y + r)) * sx + r)],
                            size_t(p.nx) * sizeof(T));
        return STENCIL_OK;
    }
    static int sweepk_source(const stencil_layout* l, const void* in, void* out, const void* src, int64_t b, int64_t e,
                             int k, Stream) {
        if (b < 0 || e > l->prob.nz || b > e || k < 1 || k > STENCIL_SOURCE_MAX_STEPS || !src)
            return set_error(STENCIL_EINVAL, "fake source sweep: bad range, steps or source");
        if ((l->prob.flags & (STENCIL_HALO_LO | STENCIL_HALO_HI)) && l->zghost < k)
            return set_error(STENCIL_EINVAL, "fake source sweep: %d steps need halo >= %d", k, k);
        {
            std::lock_guard<std::mutex> lk(fake::g_stat_mu);
            ++fake::g_source_sweeps;
        }
        if (b == e) return STENCIL_OK;
        return l->prob.dtype == STENCIL_F64 ? source_t(l, static_cast<const double*>(in), static_cast<double*>(out),
                                                       static_cast<const double*>(src), b, e, k)
                                            : source_t(l, static_cast<const float*>(in), static_cast<float*>(out),
                                                       static_cast<const float*>(src), b, e, k);
    }
    static bool source_signal_enabled() { return fake::g_source_signal; }
    // the fake has no CUs: FAKE_SLAB_SOURCE_GATE=0 makes a gated job's source launches ungated
    static bool source_halo_gate(const stencil_layout&, int, bool) {
        const char* v = std::getenv("FAKE_SLAB_SOURCE_GATE");
        return !(v && *v && std::atoi(v) == 0);
    }
    static int sweepk_signal_source(const stencil_layout* l, const void* in, void* out, const void* src, int64_t b,
                                    int64_t e, int k, uint32_t* counters, uint64_t*, int* nsig, Stream s) {
        if (k < 3 || e - b < k) return set_error(STENCIL_EINVAL, "fake signalled source sweep: steps 3..4, >= steps planes");
        if (int rc = sweepk_source(l, in, out, src, b, e, k, s)) return rc;
        {
            std::lock_guard<std::mutex> lk(fake::g_stat_mu);
            ++fake::g_source_signal_sweeps;
        }
        counters[0] += 1;
        counters[1] += 1;
        *nsig = 1;
        return STENCIL_OK;
    }
    static int sweepk_signal_source_gated(const stencil_layout* l, const void* in, void* out, const void* src, int64_t b,
                                          int64_t e, int k, uint32_t* counters, uint64_t* fsig, uint32_t need, uint32_t*,
                                          int* nsig, Stream s) {
        {
            std::lock_guard<std::mutex> lk(fake::g_stat_mu);
            ++fake::g_gated;
            if (int32_t(counters[3] - need) < 0 || counters[3] != need) ++fake::g_gate_bad;
        }
        return sweepk_signal_source(l, in, out, src, b, e, k, counters, fsig, nsig, s);
    }
};

}  // namespace stencil

struct fake_source_job : stencil::slab::Job<stencil::FakeSourceDev> {};

using stencil::FakeSourceDev;

extern "C" {

// the plain calls a source job needs, on Job<FakeSourceDev>
int fake_source_create2(const stencil_problem* g, int32_t n, const int32_t* devs, int32_t ex, int32_t flags,
                       int64_t margin, fake_source_job** job) {
    return core::create<FakeSourceDev>(g, n, devs, ex, flags, margin, job);
}
int fake_source_create_rank2(const stencil_problem* g, int32_t nranks, int32_t rank, int32_t dev, const void* id,
                            int64_t id_bytes, int32_t flags, int64_t margin, fake_source_job** job) {
    return core::create_rank<FakeSourceDev>(g, nranks, rank, dev, id, id_bytes, flags, margin, job);
}
int fake_source_destroy(fake_source_job* job) {
    core::release<FakeSourceDev>(job);
    return STENCIL_OK;
}
int fake_source_info(const fake_source_job* job, int32_t slab, int64_t* first, int64_t* planes, int32_t* dev, int32_t* k) {
    return core::info<FakeSourceDev>(job, slab, first, planes, dev, k);
}
int fake_source_fill_initial(fake_source_job* job, int32_t kind, uint64_t seed) {
    return core::fill_initial<FakeSourceDev>(job, kind, seed);
}
int fake_source_upload(fake_source_job* job, const void* host, int64_t row, int64_t rows) {
    return core::upload<FakeSourceDev>(job, host, row, rows);
}
int fake_source_download(fake_source_job* job, void* host, int64_t row, int64_t rows) {
    return core::download<FakeSourceDev>(job, host, row, rows);
}
int fake_source_run(fake_source_job* job, uint32_t iterations, float* ms) {
    return core::run<FakeSourceDev>(job, iterations, ms);
}
int fake_source_round_form(const fake_source_job* job, int32_t* form) {
    return core::round_form<FakeSourceDev>(job, form);
}
int fake_source_round_info(const fake_source_job* job, int32_t* form, int32_t* gated, int32_t* confined) {
    return core::round_info<FakeSourceDev>(job, form, gated, confined);
}

// the source calls (stencil_slab_*_source)
int fake_source_set_source(fake_source_job* job, const void* host, int64_t row, int64_t rows) {
    return core::set_source<FakeSourceDev>(job, host, row, rows);
}
int fake_source_run_source(fake_source_job* job, uint32_t iterations, float* ms) {
    return core::run_source<FakeSourceDev>(job, iterations, ms);
}
int fake_source_source_plan(const stencil_problem* g, uint32_t iterations, int64_t* rounds, int32_t* steps) {
    return core::source_plan<FakeSourceDev>(g, iterations, rounds, steps);
}
int fake_source_source_round_form(const fake_source_job* job, int32_t* form) {
    return core::source_round_form<FakeSourceDev>(job, form);
}

void fake_source_set_source_signal(int32_t on) { stencil::fake::g_source_signal = on != 0; }
// {source launches, of them face-signalled, plain launches, sends, recvs, peer copies, gated launches,
//  gate numbering violations}
void fake_source_stats(int64_t* out8, int32_t reset) {
    std::lock_guard<std::mutex> lk(stencil::fake::g_stat_mu);
    out8[0] = stencil::fake::g_source_sweeps;
    out8[1] = stencil::fake::g_source_signal_sweeps;
    out8[2] = stencil::fake::g_sweeps;
    out8[3] = stencil::fake::g_sends;
    out8[4] = stencil::fake::g_recvs;
    out8[5] = stencil::fake::g_peer_copies;
    out8[6] = stencil::fake::g_gated;
    out8[7] = stencil::fake::g_gate_bad;
    if (reset) {
        stencil::fake::g_source_sweeps = stencil::fake::g_source_signal_sweeps = 0;
        stencil::fake::g_sweeps = stencil::fake::g_signal_sweeps = 0;
        stencil::fake::g_sends = stencil::fake::g_recvs = stencil::fake::g_peer_copies = 0;
        stencil::fake::g_gated = stencil::fake::g_gate_bad = stencil::fake::g_xdone = 0;
    }
}

}  // extern "C"
