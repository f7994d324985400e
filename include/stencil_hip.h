/*
 * stencil_hip.h -- the C-ABI boundary of the MI355X stencil engine
 * (libstencil_hip.so, built from the .hip sources in stencil_amd/csrc for gfx950).
 *
 * Plain C: pointers, sizes and opaque stream handles only (a stream is a
 * hipStream_t passed as void*; NULL = the default stream).  No HIP, torch or
 * C++ types cross this boundary; the host CLI (stencil_amd/csrc/host) is
 * compiled with plain g++ against this header alone.
 *
 * Two layers:
 *
 *  1. The reference's own kernel ABI, layout-compatible and name-identical
 *     (drop-in for src/stencil/slave/stencil_slave.hpp:13-46):
 *        void stencil_iterate_dma(StencilArguments*);                 (:28)
 *        void stencil_iterate_dma_static_unroll(StencilArguments*);   (:33)
 *        void stencil_iterate_dma_slave_pack(StencilArguments*);      (:41)
 *        void stencil_iterate_rma(StencilArguments*);                 (:44)
 *     In the reference these run on the 64 CPEs via
 *     athread_spawn(SLAVE_FUN(fn), &args); athread_join()
 *     (src/stencil/stencil.cpp:34-53).  Here the call runs the whole job on
 *     the current GPU and returns when the parity-selected host buffer holds
 *     the result.  Arithmetic order follows each reference variant so results
 *     are bit-identical to what that variant computes.
 *
 *  2. The native engine API (device-resident grids, fp32/fp64, 2D/3D, star
 *     and box shapes, any radius, slab sweeps for multi-GPU).  The reference
 *     has no counterpart; it generalises Stencil::run
 *     (src/stencil/stencil.cpp:23-57) and BoundaryMatrix
 *     (include/stencil/boundary_matrix.hpp:31-238).
 *
 * Errors: native calls return STENCIL_OK (0) or a negative STENCIL_E* code;
 * stencil_last_error_message() describes the most recent failure on the
 * calling thread.  The reference-ABI entry points return void like the
 * reference (stencil_slave.hpp:26-46) and report through
 * stencil_last_error() (0 = success).
 */
#ifndef STENCIL_HIP_H
#define STENCIL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ errors */
#define STENCIL_OK 0
#define STENCIL_EINVAL (-1)      /* bad argument / unsupported combination */
#define STENCIL_EHIP (-2)        /* a HIP runtime call failed */
#define STENCIL_ENOMEM (-3)      /* device allocation failed */
#define STENCIL_ENODEV (-4)      /* no usable gfx950 device */
#define STENCIL_EUNSUPPORTED (-5)
#define STENCIL_ETIMEOUT (-6)      /* a slab job's device wait passed its deadline (a peer stopped answering) */

const char* stencil_strerror(int code);
const char* stencil_last_error_message(void);
int stencil_last_error(void);
/* 0 in libstencil_hip.so (the product: AUTO's plan, the environment knobs
 * below only); 1 in libstencil_hip_debug.so, which also reads the experiment
 * knobs (STENCIL_*_CFG workgroup shapes, forced z-chunks and kernel families)
 * the shape-sweep tests and A/B tools use.  Documented knobs, read by both:
 * STENCIL_TK_STEPS (3..5) / STENCIL_BOX_STEPS (3, 4) fused sweeps per launch,
 * STENCIL_TK_PACK / STENCIL_BOXK_PACK (0 equal z-chunks, 1 measured choice,
 * 2 the model's), STENCIL_SLAB_SIGNAL=0 (slab rounds without face signals),
 * STENCIL_SLAB_CPWAIT=1 (face-signalled slab rounds wait for the faces in the
 * command processor, hipStreamWaitValue64, instead of a polling wait kernel),
 * STENCIL_SLAB_SERIAL=1 (every full slab round as one plain launch, then the
 * exchange: nothing runs beside the launch), STENCIL_SLAB_XCU=c (default 1:
 * a face-signalled job whose launch takes several rounds of workgroups runs
 * its exchange confined to c CUs of every XCD and its launches off them;
 * 0 = never confined) and STENCIL_SLAB_XCU_EXCL=0 (the launches may use the
 * exchange's CUs too),
 * STENCIL_SLAB_PLACEMENTS=n (default 1 = the first allocation; n > 1: a
 * two-grid slab tries n placements of its grids at creation and keeps the
 * fastest -- the same launch runs 4-8 % apart in short bursts depending on
 * the grids' physical pages, 0.8 % over C2's 1000 sweeps.  Cost at
 * stencil_slab_create*: up to n candidate grid pairs allocated at once,
 * within a quarter of the free HBM, and about 6 timed K-step launches per
 * candidate; bench.py opts in with its --placements, default 16),
 * STENCIL_SLAB_TIMEOUT_MS (a slab job's deadline for any device wait,
 * default 60000: stencil_slab_set_timeout), STENCIL_SLAB_ROLLING_OVERLAP=0
 * (rolling slab rounds exchange after the pass instead of beside it),
 * STENCIL_SLAB_STAGED=0 (slabs whose launch takes several rounds of
 * workgroups run face-signalled rounds instead of staged ones),
 * STENCIL_SLAB_GATE=0 (face-signalled rounds wait for the exchange stream's
 * event before each launch instead of gating the launch's halo-reading
 * workgroups on the exchange-completion word: stencil_slab_round_info),
 * STENCIL_SLAB_SOURCE_SIGNAL=0 (the full source rounds of a face-signalled
 * slab job, stencil_slab_run_source, take the boundary + interior form instead
 * of one face-signalled source launch: stencil_slab_source_round_form; the
 * same knob governs the relaxed rounds, stencil_slab_run_relax:
 * stencil_slab_relax_round_form),
 * STENCIL_UNTIL_FUSED=0 (stencil_iterate_until checks every block with a
 * single sweep and stencil_diff_norms' kernels instead of the checking K-step
 * launch, stencil_sweepk_update_max: the A/B lever and the fallback). */
int stencil_debug_knobs(void);

/* --------------------------------------------- 1. reference-compatible ABI */

/* Layout-identical to detail::BoundaryMatrix<float,false>
 * (include/stencil/boundary_matrix.hpp:225-237 field order, LP64: 40 bytes). */
typedef struct StencilMatrixView {
    size_t actual_width;      /* width + 2*boundary_width  (_actual_width)  */
    size_t actual_height;     /* height + 2*boundary_height (_actual_height) */
    unsigned boundary_width;  /* _boundary_width  (= radius) */
    unsigned boundary_height; /* _boundary_height (= radius) */
    size_t data_stride;       /* _data_stride, elements per row */
    float* data;              /* _data, row-major incl. ghost ring, HOST memory */
} StencilMatrixView;

/* Layout-identical to struct Arguments (stencil_slave.hpp:13-24): 88 bytes. */
typedef struct StencilArguments {
    unsigned block_size; /* accepted for compatibility; the GPU picks its own tiling */
    unsigned iterations;
    StencilMatrixView input;  /* both buffers hold the initial grid + ghosts */
    StencilMatrixView output; /* final grid: output if iterations odd, else input */
} StencilArguments;

void stencil_iterate_dma(StencilArguments* args);
void stencil_iterate_dma_static_unroll(StencilArguments* args);
void stencil_iterate_dma_slave_pack(StencilArguments* args);
void stencil_iterate_rma(StencilArguments* args);

/* ------------------------------------------------------ 2. native engine */

enum { STENCIL_F32 = 0, STENCIL_F64 = 1 };
enum { STENCIL_STAR = 0, STENCIL_BOX = 1 };
/* Sum order. NAIVE = Stencil::check_result (stencil.cpp:104-125) and
 * DMAStaticUnroll; DMA = stencil_dma.cpp (r=1: 431-444, r>1: 636-650).
 * DMA order exists for 2D star only. */
enum { STENCIL_ORDER_NAIVE = 0, STENCIL_ORDER_DMA = 1 };
/* Kernel family. AUTO picks the fastest one that supports the problem. */
enum {
    STENCIL_KERNEL_AUTO = 0,
    STENCIL_KERNEL_DIRECT = 1,    /* one cell per lane, neighbours via L1/L2 */
    STENCIL_KERNEL_ZMARCH = 2,    /* 2.5D: LDS plane + z register queue */
    STENCIL_KERNEL_TEMPORAL2 = 3, /* ZMARCH with 2 fused time steps per launch */
    STENCIL_KERNEL_TEMPORALK = 4, /* 3D 7-point star: K = 3..5 fused steps per launch
                                     (K = env STENCIL_TK_STEPS, default 4) */
    STENCIL_KERNEL_PERSISTENT = 5 /* 2D star r <= 2: the whole job in one launch, one
                                     resident workgroup per tile, K-cell rings exchanged
                                     through the grid with neighbour-only flags every
                                     K sweeps (K = env STENCIL_TB2DP_K, default 8/r);
                                     grids whose tiles do not all fit at once use
                                     TEMPORAL2 */
};
enum { STENCIL_INIT_REFERENCE = 0, STENCIL_INIT_RANDOM = 1 };
/* stencil_problem.flags: which z faces of this grid are halos filled by a
 * neighbouring slab (multi-GPU) rather than Dirichlet ghosts.  Only the fused
 * two-step kernel cares: it must advance halo planes to t+1, and must keep
 * Dirichlet ghost planes fixed. */
enum { STENCIL_HALO_LO = 1, STENCIL_HALO_HI = 2 };

typedef struct stencil_problem {
    int32_t dims;   /* 2 or 3 */
    int32_t dtype;  /* STENCIL_F32 / STENCIL_F64 */
    int32_t shape;  /* STENCIL_STAR / STENCIL_BOX */
    int32_t radius; /* >= 1 (reference -r) */
    int32_t order;  /* STENCIL_ORDER_* */
    int32_t kernel; /* STENCIL_KERNEL_* */
    int32_t halo;   /* 3D: ghost planes per z side, >= radius (0 = radius); 2 for fused slabs */
    int32_t flags;  /* STENCIL_HALO_* */
    int64_t nx, ny, nz; /* interior extents (reference: width = height = -s); nz = 1 for 2D */
} stencil_problem;

/* Device layout: x fastest, ghost ring of width `radius` on x and y and of
 * `zghost` planes on z (3D), rows padded so interior x = 0 of every row is
 * 128-byte aligned.
 * Element (x, y, z) of the interior (ghosts at -r..-1 and n..n+r-1) is at
 *   base[origin + z*plane + y*row + x]    (z = 0 for 2D). */
typedef struct stencil_layout {
    stencil_problem prob;
    int64_t row;    /* elements between consecutive rows (y) */
    int64_t plane;  /* elements between consecutive planes (z); rows*row */
    int64_t planes; /* allocated planes (nz + 2*zghost for 3D, 1 for 2D) */
    int64_t zghost; /* ghost/halo planes per z side (3D; 0 for 2D) */
    int64_t rows;   /* allocated rows per plane (ny + 2r) */
    int64_t origin; /* element offset of interior (0,0,0) */
    int64_t elems;  /* elements to allocate */
    int64_t bytes;  /* elems * sizeof(element) */
} stencil_layout;

int stencil_layout_init(const stencil_problem* prob, stencil_layout* out);

/* Extent of the slow axis (z for 3D, y for 2D): sweeps and slabs range over it. */
int64_t stencil_slow_extent(const stencil_layout* l);

int stencil_device_count(int* count);
int stencil_set_device(int device);
int stencil_synchronize(void* stream);
int stencil_alloc(const stencil_layout* l, void** dev);
int stencil_free(void* dev);

/* Initial condition on the device (interior + ghosts), see DESIGN.md §Init:
 * REFERENCE = stencil.cpp:190-207 (x-ghosts 1, every other cell 0);
 * RANDOM    = interior splitmix64(seed + linear index) in [0,1). */
int stencil_fill_initial(const stencil_layout* l, void* dev, int init_kind, uint64_t seed,
                         void* stream);

/* Host <-> device copies of the whole ghost-padded grid. The host array is
 * dense: row stride host_row elements, host_rows rows per plane (the
 * reference's BoundaryMatrix has host_row = n + 2r). Asynchronous on
 * `stream` (host memory should be pinned for true overlap). */
int stencil_upload(const stencil_layout* l, void* dev, const void* host, int64_t host_row,
                   int64_t host_rows, void* stream);
int stencil_download(const stencil_layout* l, const void* dev, void* host, int64_t host_row,
                     int64_t host_rows, void* stream);
/* Copy `count` planes (slow-axis units, ghost rows/planes included, indices
 * relative to the interior: -g .. n+g-1 with g = zghost in 3D, radius in 2D)
 * between two device grids. */
int stencil_copy_planes(const stencil_layout* l, const void* src, int64_t src_first,
                        void* dst, int64_t dst_first, int64_t count, void* stream);

/* One Jacobi sweep out = S(in) over slow-axis interior indices [begin, end).
 * Ghost cells are read, never written. */
int stencil_sweep(const stencil_layout* l, const void* in, void* out, int64_t begin, int64_t end,
                  void* stream);

/* Two fused sweeps (TEMPORAL2 family): out = S(S(in)) on [begin, end), using
 * `in`'s ghost/halo planes (2r deep) for the redundant halo compute. `out`
 * must differ from `in`; no scratch grid is needed. */
int stencil_sweep2(const stencil_layout* l, const void* in, void* out, int64_t begin, int64_t end,
                   void* stream);

/* K fused sweeps, out = S^K(in) on [begin, end): steps 1 = stencil_sweep,
 * 2 = stencil_sweep2, 3..5 = the TEMPORALK kernel (3D 7-point star), 3..4 =
 * the K-step box kernel (3D 27-point box; kernels_boxk.hip, which also serves
 * the box's 2-step sweep2).
 * With HALO_LO/HI flags the grid needs halo >= steps. */
int stencil_sweepk(const stencil_layout* l, const void* in, void* out, int64_t begin, int64_t end,
                   int32_t steps, void* stream);

/* Launch geometry of stencil_sweepk's K-step kernel (3D r=1 7-point star,
 * steps 3..5) on [begin, end), computed as the launch would, without
 * launching: workgroups, planes per z-chunk (0 = balanced shares) and
 * whether the packed longest-first chunk schedule is used (it is built and
 * uploaded on first use).  Queries the current device. */
int stencil_sweepk_geometry(const stencil_layout* l, int64_t begin, int64_t end, int32_t steps, int64_t* workgroups,
                            int32_t* zchunk, int32_t* packed);

/* stencil_sweepk's K-step launch of the 3D r=1 naive 7-point star (steps
 * 3..5; other steps STENCIL_EINVAL, other problems STENCIL_EUNSUPPORTED) that
 * also reports the size of its LAST sweep's update: the launch raises
 * *update_max_bits -- 8 bytes of DEVICE memory holding a double's bit pattern,
 * zeroed by the caller -- to
 *   max |double(u^K) - double(u^(K-1))|
 * over exactly the cells it stores (the interior cells of planes [begin, end);
 * never a ghost cell, a plane outside the range or a slab-halo plane the
 * launch advances on the way).  The lane that stores a cell of u^K holds that
 * cell's u^(K-1) in registers, so the value costs no memory traffic: each
 * workgroup combines its lanes and issues at most one 64-bit atomic max on the
 * bit pattern (non-negative doubles order as unsigned integers).  A maximum
 * does not depend on the order it is taken in: the value is bit for bit the
 * maximum of stencil_diff_norms' max_abs for the two grids.  If any such
 * difference is NaN (inf - inf included) the word ends as a NaN pattern (they
 * sort above +inf).  The word accumulates over launches; the launch is
 * asynchronous on `stream`.  `out` is bitwise stencil_sweepk's.  NULL word:
 * STENCIL_EINVAL. */
int stencil_sweepk_update_max(const stencil_layout* l, const void* in, void* out, int64_t begin, int64_t end,
                              int32_t steps, uint64_t* update_max_bits, void* stream);

/* Multi-GPU slabs: stencil_sweepk over [begin, end) (3D 7-point star, steps
 * 3..5; 27-point box, steps 2..4) as ONE launch whose workgroups add 1 to counters[0] as soon as the
 * low face planes [begin, begin+steps) are stored and to counters[1] for
 * [end-steps, end) (the last z-chunk marches downward, so both faces come
 * first); *signals_per_face = adds per face per launch.  counters: two
 * uint32 in device memory, zeroed by the caller, accumulating over launches.
 * face_signal (optional, from stencil_face_signal_create): the workgroup
 * that completes a face's count for this launch also adds 1 to it, so it
 * grows by 2 per launch once both faces are stored.
 * stencil_wait_counters queues on `stream` a one-lane kernel that returns
 * when counters[0] >= target_lo and counters[1] >= target_hi -- what is
 * queued behind it (the halo send) waits for the faces, not for the whole
 * launch.  After 10 s it sets *timeout_flag and returns instead; a wait that
 * finds *timeout_flag already set returns at once (a lost peer costs one
 * timeout, and the slab job's run() reports it).
 * stencil_wait_face_signal queues the same wait on the command processor
 * (hipStreamWaitValue64, *face_signal >= target): no kernel, no timeout. */
int stencil_sweepk_signal(const stencil_layout* l, const void* in, void* out, int64_t begin, int64_t end,
                          int32_t steps, uint32_t* counters, uint64_t* face_signal, int32_t* signals_per_face,
                          void* stream);
int stencil_wait_counters(const uint32_t* counters, uint32_t target_lo, uint32_t target_hi, uint32_t* timeout_flag,
                          void* stream);
/* The halo-gated form (the 7-point star only; the box: STENCIL_EUNSUPPORTED):
 * as stencil_sweepk_signal, and the workgroups whose z range reaches a halo
 * plane (z < 0 with STENCIL_HALO_LO, z >= nz with STENCIL_HALO_HI) first wait
 * until counters[3] >= gate_need (uint32, wrap-safe), until *release_flag != 0
 * (host-coherent, as stencil_wait_counters' timeout flag; may be NULL), or
 * 10 s (then they set *release_flag and go on with stale halos: the caller
 * must treat the launch as failed).  A slab round then queues its launch right behind the previous
 * round's launch, with no event wait for the exchange that fills its halos
 * (DESIGN.md §7): the halo planes are the only bytes that exchange writes.
 * stencil_exchange_done queues on `stream` (behind the exchange's transfers)
 * one lane storing counters[3] = value. */
int stencil_sweepk_signal_gated(const stencil_layout* l, const void* in, void* out, int64_t begin, int64_t end,
                                int32_t steps, uint32_t* counters, uint64_t* face_signal, uint32_t gate_need,
                                uint32_t* release_flag, int32_t* signals_per_face, void* stream);
int stencil_exchange_done(uint32_t* counters, uint32_t value, void* stream);
/* The face-signalled launches that also report their update (the checking
 * round of a face-signalled slab job, stencil_slab_run_until): `out`, the
 * counters and the face signal are exactly stencil_sweepk_signal's (the gated
 * form: stencil_sweepk_signal_gated's, halo gate included), and the launch
 * raises *update_max_bits exactly as stencil_sweepk_update_max does -- the same
 * per-cell condition (the store's own), up- and down-marching chunks alike, so
 * the word is bit for bit that call's for the same range.  The 7-point star,
 * r = 1, naive order, steps 3..5: other steps and a NULL word are
 * STENCIL_EINVAL, other problems (the box included) STENCIL_EUNSUPPORTED.  A
 * range shorter than `steps` planes is STENCIL_EINVAL here (such a launch
 * signals one face only).  fp32 and fp64 steps = 4 run 6-row
 * strips (the plain checking launch's remedy): the same sums, no scratch. */
int stencil_sweepk_signal_update_max(const stencil_layout* l, const void* in, void* out, int64_t begin, int64_t end,
                                     int32_t steps, uint32_t* counters, uint64_t* face_signal,
                                     uint64_t* update_max_bits, int32_t* signals_per_face, void* stream);
int stencil_sweepk_signal_update_max_gated(const stencil_layout* l, const void* in, void* out, int64_t begin,
                                           int64_t end, int32_t steps, uint32_t* counters, uint64_t* face_signal,
                                           uint64_t* update_max_bits, uint32_t gate_need, uint32_t* release_flag,
                                           int32_t* signals_per_face, void* stream);
/* face signals: 8 bytes of HIP signal memory (hipExtMallocWithFlags,
 * hipMallocSignalMemory) holding a uint64 count */
int stencil_face_signal_create(uint64_t** face_signal);
int stencil_face_signal_destroy(uint64_t* face_signal);
int stencil_face_signal_reset(uint64_t* face_signal, void* stream);   /* queued: *face_signal = 0 */
int stencil_face_signal_read(const uint64_t* face_signal, uint64_t* value);  /* synchronous */
int stencil_wait_face_signal(const uint64_t* face_signal, uint64_t target, void* stream);

/* Whole job: `iterations` ping-pong sweeps starting from grid `a` (grid `b`
 * must hold the same ghosts). *final_in_b = 1 when the result is in `b`, 0
 * when in `a`.  The grids swap once per LAUNCH: with one sweep per launch
 * that is the parity rule (stencil.cpp:88-92,134: `b` when iterations is
 * odd); a job of K-step launches ends wherever its launch count leaves it
 * (23 sweeps of a 2D r = 1 job end in `a`), so read the flag.
 * With prob.kernel == TEMPORAL2, pairs of iterations run as one launch;
 * with TEMPORALK, K-tuples (remainder as a pair and/or a single sweep).
 * If elapsed_ms is non-NULL the call brackets its launches with hipEvents on
 * `stream`, synchronises, and stores the elapsed device time. */
int stencil_iterate(const stencil_layout* l, void* a, void* b, uint32_t iterations, void* stream,
                    int* final_in_b, float* elapsed_ms);

/* Settle stencil_iterate's one-time, per-shape choices before a timed run:
 * the first fused launch of the job (K-step 7-point star or box) from `a`
 * into `b`, which on a shape's first use times the packed and equal z-chunk
 * grids (blocking once) and keeps the faster.  `a` is not changed; `b` is
 * overwritten (its ghost cells are not).  Then the same launch again for
 * about 25 ms of device time (at most 2048 launches): after the GPU has idled
 * its clock needs that long to settle (the first launches run up to 1.45x
 * slower), so a timed run that follows measures the settled state.  2D jobs
 * of K-step launches settle the same way (they have no per-shape choice).
 * Blocks the host once.  A no-op for jobs without a K-step launch.  No
 * reference counterpart (the reference has no per-shape state). */
int stencil_prepare(const stencil_layout* l, const void* a, void* b, void* stream);
/* The same, reporting what ran before the caller's timed region: the kernel
 * launches (the schedule trial's included) and their device time, estimated
 * from the one timed settle launch. */
int stencil_prepare2(const stencil_layout* l, const void* a, void* b, void* stream, int64_t* settle_launches,
                     float* settle_ms);

/* One resident grid instead of two (3D, no slab flags): for jobs whose two
 * ping-pong grids do not fit the GPU -- BASELINE config 3, 4096^3 fp32, is
 * 2 x 279 GB; one grid plus a few hundred spare planes fits 288 GiB.  The
 * reference swaps two owner buffers every sweep (src/stencil/stencil.cpp:
 * 14-21, 88-92; include/stencil/boundary_matrix.hpp:59); here a pass of K
 * fused sweeps writes plane z of the new grid into the slot D planes below
 * (down pass) or back (up pass), in launches over z-ranges of D - K*r planes
 * ordered so that no launch writes a slot any later read needs (D >= K*r + 1;
 * K = the sweeps of one pass, r = the radius).  Results
 * are bitwise those of stencil_iterate.
 *   allocation: stencil_rolling_bytes(l, D, &bytes, &K) bytes at `base`;
 *   the grid at home (position 0) is the layout's grid at base + D*plane*esz,
 *   shifted (position 1) at base.  Fill / upload the home grid as usual,
 *   then stencil_rolling_init_margin copies its top ghost plane into the D
 *   spare slots (the x/y ghost ring must be the same in every plane and the
 *   z ghost planes alike, as in the reference initial condition).
 *   stencil_rolling_iterate: `iterations` sweeps from *position (updated);
 *   launches = kernel launches issued; elapsed_ms as stencil_iterate. */
int stencil_rolling_bytes(const stencil_layout* l, int64_t shift_planes, int64_t* bytes, int32_t* sweeps_per_pass);
int stencil_rolling_init_margin(const stencil_layout* l, void* base, int64_t shift_planes, void* stream);
int stencil_rolling_iterate(const stencil_layout* l, void* base, int64_t shift_planes, uint32_t iterations,
                            int32_t* position, void* stream, int64_t* launches, float* elapsed_ms);

/* The dispatcher model behind the packed z-chunk schedule, on the host (no
 * GPU needed): `tiles` x-y tiles of `planes` planes on `slots` one-workgroup
 * CU slots, `fill` planes of pipeline fill per chunk (2K for the 7-point
 * K-step kernel, 3K for the box), equal chunks of `zchunk` planes as the
 * alternative.  Returns the simulated makespans (plane steps) of the equal
 * chunks and of the best packed grid, and the packed grid's workgroups (0 when
 * it would not be used: it must beat equal chunks by 2 %).  stencil_iterate
 * then times both grids on a shape's first launch (STENCIL_TK_PACK=1). */
int stencil_pack_plan(int64_t tiles, int64_t planes, int32_t fill, int32_t slots, int32_t zchunk,
                      int64_t* equal_steps, int64_t* packed_steps, int64_t* workgroups);
/* The packed grid itself (host only): {tile, first plane, planes} per
 * workgroup in dispatch order, for a tile grid `tiles_x` wide; xcd_width > 0
 * reorders every generation of equal chunks into XCD patches of that width
 * (the dispatcher deals workgroup i to XCD i % 8); -1: the width with the most
 * same-XCD x/y neighbour tiles, as long jobs (>= 256 sweeps per call of
 * stencil_iterate / stencil_slab_run) launch it.  Writes at most
 * `capacity` triples into `table` (may be NULL) and the count to
 * *workgroups (0: no packed grid). */
int stencil_pack_table(int64_t tiles, int64_t tiles_x, int64_t planes, int32_t fill, int32_t slots, int32_t zchunk,
                       int32_t xcd_width, int32_t* table, int64_t capacity, int64_t* workgroups);
/* The packed grid of the fp64 K = 4 strip's sliver mode (host only), where the
 * last tile column -- at most 8 columns wide -- runs as sliver workgroups of
 * four tile rows each: for an nx x ny plane of `planes` planes on `slots`
 * workgroup slots, geometry[0..3] = tile columns, tile rows, main (full-width)
 * tiles and schedule tiles (main + sliver workgroups; both 0 where the mode is
 * off: one tile column, a last column wider than 8, more than 2 tiles per
 * slot, more schedule tiles than slots).  The mode runs only with this table:
 * where it is empty (fewer than 8 planes) the launch is the plain tile grid's.  The table is stencil_pack_table's for that tile count: tile < main
 * is main tile (tile % (columns - 1), tile / (columns - 1)), tile >= main
 * sliver workgroup tile - main (tile rows 4j .. 4j + 3 of the last column).
 * The main tiles take chunks of Lc planes, the sliver workgroups of
 * ceil(Lc / 2) (they take longer per plane); Lc is the model's best among the
 * tables whose full chunks fit the slots at once, or chunk_planes when that is
 * > 0 (as STENCIL_TK_PACK_LC).  xcd_width as stencil_pack_table's, the patches
 * over the main tiles. */
int stencil_sliver_table(int64_t nx, int64_t ny, int64_t planes, int32_t slots, int32_t chunk_planes,
                         int32_t xcd_width, int64_t* geometry, int32_t* table, int64_t capacity, int64_t* workgroups);

/* Launch plan of stencil_iterate for `iterations`: number of kernel launches
 * and the kernel family AUTO resolves to. */
int stencil_plan(const stencil_layout* l, uint32_t iterations, int64_t* launches,
                 int32_t* kernel);

/* Device-side checksums of the interior: per-plane sums (double, ascending
 * x, y order within the plane) written to `plane_sums` (slow_extent
 * entries, device or host pointer) -- the "checksum of checksums" used by
 * the full-size property tests. */
int stencil_plane_sums(const stencil_layout* l, const void* dev, double* plane_sums_host,
                       void* stream);

/* Convergence-controlled runs.  The reference runs a fixed count
 * (stencil.cpp:23-57); a Jacobi solver is normally driven until the update
 * falls below a tolerance.
 *
 * stencil_diff_norms: for two grids of one layout and every slow-axis unit u
 * in [begin, end) (a plane in 3D, a row in 2D),
 *   max_abs[u - begin] = max |d|,  sum_sq[u - begin] = sum d*d,
 *   d = double(a) - double(b), over the unit's interior cells only
 * (kernels_norm.hip: one streaming read of both grids; the result depends on
 * the layout and the data alone, never on the device, the stream or timing).
 * If any d of a unit is NaN both outputs of that unit are NaN; infinities
 * propagate.  max_abs / sum_sq: end - begin doubles each, HOST arrays, either
 * may be NULL (not both).  Queued on `stream`, then synchronises it.  The
 * scalar norm of the pair is, for STENCIL_NORM_MAX, the maximum of max_abs,
 * and for STENCIL_NORM_L2 the square root of the sum of sum_sq taken in
 * ascending unit order on the host; NaN if any unit is NaN.
 *
 * stencil_iterate_until: sweeps from grid `a` (as stencil_iterate) in blocks of
 * min(check_every, max_iterations - done), each followed by the scalar norm of
 * u^n - u^(n-1).  STENCIL_NORM_MAX on a job of K-step 7-point launches
 * (stencil_plan: TEMPORALK), blocks of at least K sweeps: block - K sweeps by
 * stencil_iterate's own plan, then ONE checking K-step launch
 * (stencil_sweepk_update_max) whose 8-byte maximum is zeroed before it on the
 * stream and copied back after it -- no extra sweep, no pass over the grids.
 * Every other block (shorter ones, STENCIL_NORM_L2, the box, 2D, r > 1, forced
 * kernel families; every block with STENCIL_UNTIL_FUSED=0): block - 1 sweeps
 * by stencil_iterate's own plan, then ONE single sweep, so that the two grids
 * hold u^(n-1) and u^n (a K-step launch leaves u^n and u^(n-K)), then
 * stencil_diff_norms' kernels.  Both forms give the same sweep counts, norms
 * (bit for bit) and final grid; which buffer holds it may differ, so read
 * *final_in_b.  stencil_until_plan (host only, no device needed) reports the
 * kernel launches of one block of `block` sweeps, its check included, and
 * whether that check rides in the block's last launch.
 * Stops with *converged = 1 when norm <= tol,
 * with *converged = 0 when the norm is NaN or max_iterations sweeps are done
 * (a final block shorter than check_every is checked too).  Not converging is
 * a result, not an error: STENCIL_OK either way.  max_iterations = 0:
 * *iterations_done = 0, *converged = 0, *last_norm = +inf.  The grid
 * *final_in_b names is bitwise stencil_iterate's after *iterations_done
 * sweeps.  *elapsed_ms (optional): hipEvent time from the first launch to the
 * completion of the last check.  Blocks the host once per check.
 * STENCIL_EINVAL: check_every = 0, tol < 0 or NaN, an unknown norm, a == b or
 * NULL grids; diff_norms: begin < 0, end > slow extent, begin > end;
 * until_plan: block = 0, an unknown norm. */
enum { STENCIL_NORM_MAX = 0, STENCIL_NORM_L2 = 1 };
int stencil_diff_norms(const stencil_layout* l, const void* a, const void* b, int64_t begin, int64_t end,
                       double* max_abs, double* sum_sq, void* stream);
int stencil_iterate_until(const stencil_layout* l, void* a, void* b, uint32_t max_iterations,
                          uint32_t check_every, int32_t norm, double tol, void* stream,
                          uint32_t* iterations_done, int* final_in_b, double* last_norm,
                          int* converged, float* elapsed_ms);
int stencil_until_plan(const stencil_layout* l, uint32_t block, int32_t norm, int64_t* launches,
                       int32_t* fused_check);

/* Sweeps with a source term (Poisson's right-hand side, a heat source, a
 * multigrid smoother): u' = S(u) + g.  Scope: the 3D 7-point star, r = 1,
 * naive order, fp32 / fp64, layouts with flags == 0, kernel AUTO or TEMPORALK.
 * `src` is a device grid of the SAME layout as the field (stencil_alloc,
 * stencil_upload); only its interior cells have meaning, the caller scales it
 * (g = h^2 / 6 f for the 7-point Laplacian).  One source sweep over planes
 * [begin, end) stores, at every interior cell c of those planes,
 *   out(c) = fl( fl( sum6(in, c) * avg ) + src(c) )
 * with sum6 and avg the plain sweep's (0 + x- + x+ + y- + y+ + z- + z+): the
 * multiply is rounded, then the source is added and rounded again -- never one
 * fma.  A launch of `steps` sweeps is bitwise `steps` such sweeps (ghost cells
 * keep their input value in between and get no source).  It stores the
 * interior cells of [begin, end) of `out` and nothing else, never stores to
 * `in` or `src`, and no value of a `src` ghost cell, padding or tail-pad
 * element reaches a result.
 *
 * stencil_sweepk_source: steps in 1 .. STENCIL_SOURCE_MAX_STEPS; 2, 3 and 4 are
 * the K-step strip kernel with its source option (one extra read stream per
 * launch: 24 B per cell and launch in fp64 instead of 16), 1 a single sweep.
 * stencil_iterate_source: stencil_iterate with the source -- ping-pong from
 * `a` in launches of STENCIL_SOURCE_MAX_STEPS sweeps, the remainder as one
 * shorter launch; read *final_in_b.  stencil_source_plan (host only, no
 * device): the kernel launches of that job and the sweeps of its fused launch.
 * stencil_iterate_until_source: stencil_iterate_until's stopping rule,
 * arguments, outputs and edge cases on source sweeps, always with the un-fused
 * check: block - 1 sweeps by stencil_iterate_source's plan, one single source
 * sweep, then stencil_diff_norms' kernels.
 * STENCIL_EINVAL: NULL src; src equal to in, out, a or b; a == b or NULL
 * grids; a bad range; steps outside 1 .. STENCIL_SOURCE_MAX_STEPS;
 * check_every = 0; tol < 0 or NaN; an unknown norm.  STENCIL_EUNSUPPORTED
 * (the message names the restriction): 2D, the box, r > 1, the DMA order,
 * halo flags, a forced kernel family other than AUTO or TEMPORALK. */
#define STENCIL_SOURCE_MAX_STEPS 4
int stencil_sweepk_source(const stencil_layout* l, const void* in, void* out, const void* src,
                          int64_t begin, int64_t end, int32_t steps, void* stream);
int stencil_iterate_source(const stencil_layout* l, void* a, void* b, const void* src, uint32_t iterations,
                           void* stream, int* final_in_b, float* elapsed_ms);
int stencil_source_plan(const stencil_layout* l, uint32_t iterations, int64_t* launches, int32_t* steps);
int stencil_iterate_until_source(const stencil_layout* l, void* a, void* b, const void* src,
                                 uint32_t max_iterations, uint32_t check_every, int32_t norm, double tol,
                                 void* stream, uint32_t* iterations_done, int* final_in_b,
                                 double* last_norm, int* converged, float* elapsed_ms);

/* Source launches on slab layouts (the launches of stencil_slab_run_source).
 * stencil_sweepk_source_halo is stencil_sweepk_source for layouts that may
 * carry STENCIL_HALO_LO / STENCIL_HALO_HI: `src` has the same layout, halo
 * planes included.  With flags it needs halo >= steps (as stencil_sweepk);
 * with flags == 0 it is bitwise stencil_sweepk_source.  On a halo side the
 * launch advances the halo planes on chip, as the plain kernel does: stage s
 * of K = steps is computed for planes [-(K - s), nz + K - s) there, and each
 * advanced halo cell gets `src` of its own plane.  The launch therefore reads
 * `src` on planes [begin - (K - 1), end + K - 1), clipped to
 * [-(K - 1), nz + K - 1) on a halo side and to [0, nz) on a Dirichlet side: no
 * value of src's planes -K or nz + K - 1, of its x/y ghost ring or padding, or
 * of its z ghost planes on a Dirichlet side reaches a result.  It stores the
 * interior cells of [begin, end) of `out` and nothing else.  steps = 1 reads
 * the halo planes of `in` and advances none.
 *   stencil_sweepk_signal_source / _gated: stencil_sweepk_signal / _gated with
 * the source (steps 3 or 4): `out` is bitwise stencil_sweepk_source_halo's,
 * the face counters, the face signal and the halo gate are exactly
 * stencil_sweepk_signal's.  The strips are narrower than the plain source
 * launch's where the signalling code needs the registers (K = 4: 4 rows per
 * strip instead of 5), so *signals_per_face differs from the plain launch's.
 * STENCIL_EINVAL: as stencil_sweepk_source; signalled: steps other than 3 or
 * 4, NULL counters, a range shorter than `steps` planes; halo < steps on a
 * layout with halo flags.  STENCIL_EUNSUPPORTED: as stencil_sweepk_source,
 * but for the halo flags. */
int stencil_sweepk_source_halo(const stencil_layout* l, const void* in, void* out, const void* src,
                               int64_t begin, int64_t end, int32_t steps, void* stream);
int stencil_sweepk_signal_source(const stencil_layout* l, const void* in, void* out, const void* src,
                                 int64_t begin, int64_t end, int32_t steps, uint32_t* counters,
                                 uint64_t* face_signal, int32_t* signals_per_face, void* stream);
int stencil_sweepk_signal_source_gated(const stencil_layout* l, const void* in, void* out, const void* src,
                                       int64_t begin, int64_t end, int32_t steps, uint32_t* counters,
                                       uint64_t* face_signal, uint32_t gate_need, uint32_t* release_flag,
                                       int32_t* signals_per_face, void* stream);

/* Relaxed source sweeps: damped Jacobi, and Chebyshev or scheduled-relaxation
 * Jacobi when the weights cycle through a schedule.  Scope, grids and the
 * stores rule are stencil_sweepk_source's (3D 7-point star, r = 1, naive
 * order, fp32 / fp64, flags == 0, kernel AUTO or TEMPORALK; `src` a device grid
 * of the field's layout, for a plain smoother a grid of zeros).  One relaxed
 * sweep with the weight omega stores, at every interior cell c of its planes,
 *   J   = fl( fl( sum6(in, c) * avg ) + src(c) )    the source sweep's value
 *   d   = fl( J - in(c) )
 *   out = fl( in(c) + fl( w * d ) )                 w = omega rounded once to
 *                                                   the grid's type
 * four roundings after the multiply, never an fma.  Ghost cells keep their
 * value and get neither source nor relaxation.  A launch of `steps` sweeps with
 * the weights omegas[0 .. steps) is bitwise `steps` such sweeps in order.
 * omega = 1 is NOT promised to equal the source sweep: fl(c + fl(J - c))
 * differs from J in some cells (where J - c is inexact).
 *
 * stencil_sweepk_relax: steps in 1 .. STENCIL_SOURCE_MAX_STEPS; 2, 3 and 4 are
 * the K-step strip kernel with its relaxation option (the weights travel as
 * kernel arguments: no device buffer, no copy), 1 a single relaxed sweep.
 * `omegas` is a host array of `steps` doubles.
 * stencil_iterate_relax: ping-pong from `a` by stencil_iterate_source's plan
 * (stencil_relax_plan, host only, equals stencil_source_plan); sweep i of the
 * job (0-based) takes omegas[(phase + i) % period], so a caller continues a
 * schedule across calls by passing the sweeps done so far as `phase`.
 * stencil_iterate_until_relax: stencil_iterate_until_source's stopping rule,
 * outputs and edge cases (max_iterations = 0, a NaN norm), always the un-fused
 * check: block - 1 sweeps by the plan, one single relaxed sweep, then
 * stencil_diff_norms' kernels; the schedule index runs on across blocks.  The
 * norm is that of u^n - u^(n-1), which contains sweep n's weight: make
 * check_every a multiple of `period`, so that every check sees the same weight.
 * stencil_chebyshev_weights (host only): the Chebyshev schedule of `period`
 * = P weights for the Dirichlet problem of p's extents,
 *   rho = (cos(pi/(nx+1)) + cos(pi/(ny+1)) + cos(pi/(nz+1))) / 3,
 *   omega_j = 1 / (1 - rho cos(pi (2j + 1) / (2P))),  j = 0 .. P-1,
 * returned in the Lebedev-Finogenov order (perm_1 = [0]; perm_2m is perm_m with
 * every entry p replaced by the pair p, 2m - 1 - p: P = 4 gives j = 0, 3, 1, 2),
 * which keeps the intermediate error bounded -- in ascending j a long schedule
 * overflows in fp32.  P is a power of two in 1 .. 64; *spectral_radius
 * (optional) = rho.
 * STENCIL_EINVAL: everything stencil_sweepk_source / stencil_iterate_source /
 * stencil_iterate_until_source reject; NULL omegas; period == 0; a weight that
 * is NaN or infinite; a period of stencil_chebyshev_weights that is not a power
 * of two in 1 .. 64.  STENCIL_EUNSUPPORTED (the message names the restriction):
 * as stencil_sweepk_source, halo flags included. */
int stencil_sweepk_relax(const stencil_layout* l, const void* in, void* out, const void* src,
                         int64_t begin, int64_t end, int32_t steps, const double* omegas, void* stream);
int stencil_iterate_relax(const stencil_layout* l, void* a, void* b, const void* src, uint32_t iterations,
                          const double* omegas, uint32_t period, uint32_t phase, void* stream,
                          int* final_in_b, float* elapsed_ms);
int stencil_iterate_until_relax(const stencil_layout* l, void* a, void* b, const void* src,
                                uint32_t max_iterations, uint32_t check_every, int32_t norm, double tol,
                                const double* omegas, uint32_t period, uint32_t phase, void* stream,
                                uint32_t* iterations_done, int* final_in_b, double* last_norm,
                                int* converged, float* elapsed_ms);
int stencil_relax_plan(const stencil_layout* l, uint32_t iterations, int64_t* launches, int32_t* steps);
int stencil_chebyshev_weights(const stencil_problem* p, int32_t period, double* omegas,
                              double* spectral_radius);

/* Relaxed launches on slab layouts (the launches of stencil_slab_run_relax).
 * stencil_sweepk_relax_halo is stencil_sweepk_relax for layouts that may carry
 * STENCIL_HALO_LO / STENCIL_HALO_HI, exactly as stencil_sweepk_source_halo is
 * to stencil_sweepk_source: with flags it needs halo >= steps, with flags == 0
 * it is bitwise stencil_sweepk_relax (which itself keeps refusing halo flags).
 * On a halo side stage s of K = steps is computed for planes
 * [-(K - s), nz + K - s); each advanced halo cell takes `src` of its own plane
 * and the stage's weight, omegas[s - 1] rounded once to the grid's type.  The
 * reads of `src` are those documented for stencil_sweepk_source_halo.  It
 * stores the interior cells of [begin, end) of `out` and nothing else.
 * steps = 1 reads the halo planes of `in` and advances none.
 *   stencil_sweepk_signal_relax / _gated: stencil_sweepk_signal_source /
 * _gated with the weights (steps 3 or 4): `out` is bitwise
 * stencil_sweepk_relax_halo's; the counters, the face signal and the halo gate
 * are exactly stencil_sweepk_signal_source's.  Stage s applies omegas[s - 1]
 * whichever way a chunk is marched.  The rows per strip are the signalled
 * source launch's (6 at K = 3, 4 at K = 4), so *signals_per_face equals that
 * launch's.
 * STENCIL_EINVAL: as stencil_sweepk_source_halo / stencil_sweepk_signal_source
 * (in their order), then NULL omegas or a weight that is NaN or infinite.
 * STENCIL_EUNSUPPORTED: as stencil_sweepk_source_halo. */
int stencil_sweepk_relax_halo(const stencil_layout* l, const void* in, void* out, const void* src,
                              int64_t begin, int64_t end, int32_t steps, const double* omegas, void* stream);
int stencil_sweepk_signal_relax(const stencil_layout* l, const void* in, void* out, const void* src,
                                int64_t begin, int64_t end, int32_t steps, const double* omegas,
                                uint32_t* counters, uint64_t* face_signal, int32_t* signals_per_face,
                                void* stream);
int stencil_sweepk_signal_relax_gated(const stencil_layout* l, const void* in, void* out, const void* src,
                                      int64_t begin, int64_t end, int32_t steps, const double* omegas,
                                      uint32_t* counters, uint64_t* face_signal, uint32_t gate_need,
                                      uint32_t* release_flag, int32_t* signals_per_face, void* stream);

/* Geometric multigrid for the 7-point Poisson solve on one GPU (DESIGN.md
 * §5.9; kernels_mg.hip): the relaxed sweeps above are the smoother, the calls
 * below compute residuals, move them between a fine grid and its coarsening,
 * and run V-cycles.  Scope everywhere: stencil_sweepk_source's (3D 7-point
 * star, r = 1, naive order, fp32 / fp64, flags == 0, kernel AUTO or TEMPORALK).
 * Every formula is a sequence of separately rounded IEEE operations in the
 * grid's type T, never an fma: results are bit for bit defined by the data.
 *
 * Coarsening is vertex-centred: a fine problem with odd interior extents
 * nx, ny, nz >= 3 has the coarse problem ((nx-1)/2, (ny-1)/2, (nz-1)/2), and
 * coarse interior cell (X, Y, Z) sits on fine interior cell (2X+1, 2Y+1, 2Z+1).
 * The coarse grid has its own stencil_layout (stencil_layout_init of the coarse
 * problem; its pitch and origin are unrelated to the fine grid's).
 *
 * Residual, in the library's scaling r = (h^2 / 6) (f + Laplace_h u): at every
 * interior cell c
 *   r(c) = fl( J(c) - u(c) ),  J(c) = fl( fl( sum6(u, c) * avg ) + g(c) )
 * -- exactly the `d` of the relaxed sweep.  It reads u's ghost ring and g's
 * interior; no residual of a ghost cell exists.
 *
 * Restricted residual (the coarse problem's source): the coarse error equation
 * is e = S(e) + g_c with g_c = 4 R(r), R the 27-point full weighting, taken
 * separably.  The 1-D operator along an axis is
 *   A(X) = fl( fl( v(i-1) + v(i+1) ) + fl( v(i) + v(i) ) ),  i = 2X + 1,
 * applied along x to r, then along y to that, then along z; then
 * g_c = fl( 0.0625 * that ).  Every fine index touched (2X .. 2X+2) is interior.
 *
 * Prolongation and correction: trilinear and separable, x, then y, then z.
 * Along an axis fine index i odd takes coarse cell (i-1)/2 EXACTLY (a copy, not
 * 0.5 (e + e), which differs for huge values); i even takes
 * fl( 0.5 * fl( e(i/2 - 1) + e(i/2) ) ), coarse indices -1 and m being e's ghost
 * cells (the ghost ring's edges and corners included).  Then
 * u(c) = fl( u(c) + p(c) ), in place, at interior cells only.
 *
 * stencil_coarsen_problem (host only): *coarse = the coarsening of *fine.
 * STENCIL_EINVAL: an even extent or an extent < 3, NULL arguments;
 * STENCIL_EUNSUPPORTED outside the scope (the message names the restriction).
 *
 * stencil_residual_norms: stencil_diff_norms' outputs, argument rules,
 * determinism and NaN rule for d = double(r(c)), per plane of [begin, end):
 * max_abs[z - begin] = max |d|, sum_sq[z - begin] = sum d*d over the plane's
 * interior cells.  r is not stored.  This is the stopping criterion of a
 * multigrid solve (the update norm of the *_until calls means nothing across
 * cycles).
 *
 * stencil_restrict_residual: reads u and src (= g) on the fine layout lf,
 * stores g_c at the interior cells of coarse planes [cbegin, cend) of
 * coarse_src (layout lc) and nothing else; the residual never reaches memory.
 * stencil_prolong_add: u += P(e) at the interior cells of fine planes
 * [begin, end), in place; never stores to a ghost cell, to padding or to e.
 * STENCIL_EINVAL for both: lc is not the coarsening of lf (or either is not
 * stencil_layout_init's layout of its problem), a dtype mismatch, NULL grids,
 * aliased grids, a bad range.
 *
 * The hierarchy, stencil_mg: levels 0 (fine) .. L-1, each with two field grids
 * (the relaxed jobs ping-pong) and a source grid, allocated zeroed on the
 * current device.  stencil_mg_create: levels = 0 coarsens while every extent is
 * odd and >= 3; a count above that is STENCIL_EINVAL; a level whose shape the
 * relaxed job cannot run refuses the count with STENCIL_EUNSUPPORTED and a
 * message (nothing is ever launched on such a shape).  stencil_mg_level: the
 * level's layout, the grid that CURRENTLY holds its field, its source grid
 * (each output optional).  stencil_mg_upload / stencil_mg_download move the
 * fine field and / or the fine source (either may be NULL, not both) as dense
 * ghost-padded host arrays, as stencil_upload does; the field's ghost cells are
 * the Dirichlet data.
 *
 * stencil_mg_vcycle: one V-cycle.  The coarsest level runs coarse_sweeps
 * relaxed sweeps.  Every other level l: `pre` relaxed sweeps; the restricted
 * residual into level l+1's source; level l+1's field set to zero, ghost cells
 * included; the cycle on level l+1; prolong-add into level l; `post` relaxed
 * sweeps.  Every smoothing run is stencil_iterate_relax's job on that level's
 * layout with omegas[i % period] for its sweep i (phase 0 in every run).  A
 * fixed sequence of bitwise-defined operations: the result is bitwise defined.
 * stencil_mg_solve: cycles in blocks of min(check_every, max_cycles - done),
 * each followed by the scalar norm (stencil_diff_norms' rule: STENCIL_NORM_MAX
 * or STENCIL_NORM_L2) of the fine stencil_residual_norms; stopping rule and edge
 * cases are stencil_iterate_until's (*converged = 1 when norm <= tol; 0 when
 * the norm is NaN or max_cycles are done; max_cycles = 0: *cycles_done = 0,
 * *converged = 0, *last_norm = +inf; not converging is STENCIL_OK).
 * STENCIL_EINVAL: NULL hierarchy or params, NULL omegas, period = 0, a weight
 * that is NaN or infinite, check_every = 0, tol < 0 or NaN, an unknown norm.
 * stencil_mg_plan (host only, no device): the kernel launches of one cycle --
 * stencil_relax_plan of every smoothing run plus one restriction and one
 * prolongation launch per level but the coarsest (the zero fill is a memset) --
 * and the level count `levels` resolves to.
 * All argument errors fire before a device is touched. */
typedef struct stencil_mg stencil_mg;
typedef struct stencil_mg_params {
    uint32_t pre;            /* relaxed sweeps before the coarse-grid correction */
    uint32_t post;           /* ... and after it */
    uint32_t coarse_sweeps;  /* relaxed sweeps on the coarsest level */
    uint32_t period;         /* weights in `omegas` */
    const double* omegas;    /* host array; sweep i of every smoothing run takes omegas[i % period] */
} stencil_mg_params;
int stencil_coarsen_problem(const stencil_problem* fine, stencil_problem* coarse);
int stencil_residual_norms(const stencil_layout* l, const void* u, const void* src, int64_t begin, int64_t end,
                           double* max_abs, double* sum_sq, void* stream);
int stencil_restrict_residual(const stencil_layout* lf, const void* u, const void* src, const stencil_layout* lc,
                              void* coarse_src, int64_t cbegin, int64_t cend, void* stream);
int stencil_prolong_add(const stencil_layout* lc, const void* e, const stencil_layout* lf, void* u, int64_t begin,
                        int64_t end, void* stream);
int stencil_mg_create(const stencil_problem* fine, int32_t levels, stencil_mg** mg);
int stencil_mg_destroy(stencil_mg* mg);
int stencil_mg_levels(const stencil_mg* mg, int32_t* levels);
int stencil_mg_level(const stencil_mg* mg, int32_t level, stencil_layout* out, void** field, void** source);
int stencil_mg_upload(stencil_mg* mg, const void* field, const void* source, int64_t host_row, int64_t host_rows,
                      void* stream);
int stencil_mg_download(const stencil_mg* mg, void* field, void* source, int64_t host_row, int64_t host_rows,
                        void* stream);
int stencil_mg_vcycle(stencil_mg* mg, const stencil_mg_params* params, void* stream);
int stencil_mg_solve(stencil_mg* mg, const stencil_mg_params* params, uint32_t max_cycles, uint32_t check_every,
                     int32_t norm, double tol, void* stream, uint32_t* cycles_done, double* last_norm, int* converged,
                     float* elapsed_ms);
int stencil_mg_plan(const stencil_problem* fine, int32_t levels, const stencil_mg_params* params, int64_t* launches,
                    int32_t* levels_out);

/* Full multigrid (FMG) start-up of the same solve: the
 * problem is solved on the coarsest level, the solution interpolated one level
 * up as the starting guess, a few V-cycles run there, and so on up to the fine
 * level -- the solution down to discretization accuracy in one pass, whatever
 * the fine field held.  Scope, indices and rounding rules are those above: every
 * operation is rounded separately in T and is never an fma.  A fine extent
 * n = 2m + 1 has the coarse extent m; ghost cells are index -1 and n on the
 * fine grid, -1 and m on the coarse grid; coarse cell X sits on fine 2X + 1, so
 * coarse ghost -1 sits on fine ghost -1 and coarse ghost m on fine ghost n.
 *
 * Coarse source: g_c = fl( 0.0625 * A_z(A_y(A_x(g))) ), the 1-D operator A
 * above applied to g's interior directly (= 4 R(g): g = h^2 f / 6 and the
 * coarse h is 2h).  Interior cells only.
 *
 * Coarse Dirichlet data: every cell (X, Y, Z) of the coarse ghost shell -- the
 * padded (mz+2)(my+2)(mx+2) box minus its interior, edges and corners included
 * -- is an exact copy of the fine ghost-shell cell (2X+1, 2Y+1, 2Z+1).
 *
 * Cubic prolongation (a set, not an add): separable, x, then y, then z; the x
 * pass runs over every coarse row, ghost rows and planes included.  Along an
 * axis with the coarse line c(-1 .. m), fine index i odd takes c((i-1)/2)
 * exactly.  Fine index i even, k = i/2:
 *   m = 1:   fl( 0.5 * fl( c(k-1) + c(k) ) );
 *   m >= 2:  four consecutive nodes p0..p3 with exact integer weights w0..w3,
 *            k = 0:      c(-1 .. 2),     ( 5, 15, -5,  1)
 *            k = m:      c(m-3 .. m),    ( 1, -5, 15,  5)
 *            otherwise:  c(k-2 .. k+1),  (-1,  9,  9, -1)
 *            value = fl( 0.0625 * fl( fl( fl(w0 p0) + fl(w1 p1) )
 *                                   + fl( fl(w2 p2) + fl(w3 p3) ) ) ).
 * It READS THE EDGES AND CORNERS of the coarse ghost ring (fine cell (0, 0, z)
 * uses coarse (-1, -1, .)), cells no sweep ever reads: a caller of
 * stencil_mg_fmg must supply them in the fine field's ghost shell -- they are
 * the boundary data on the domain's edges.
 *
 * stencil_restrict_source: g_c of src (layout lf) into the interior cells of
 * coarse planes [cbegin, cend) of coarse_src (layout lc), nothing else.
 * stencil_inject_ghosts: the coarse Dirichlet data of u (lf) into the shell
 * cells of uc (lc), nothing else: no interior cell, no row padding.
 * stencil_prolong_cubic: the cubic prolongation of e (lc) stored at the interior
 * cells of fine planes [begin, end) of u (lf), nothing else; u is not read.
 * Argument rules of all three: stencil_restrict_residual's / stencil_prolong_add's
 * (STENCIL_EINVAL: lc is not the coarsening of lf, a layout that is not
 * stencil_layout_init's, a dtype mismatch, NULL grids, aliased grids, a bad
 * range).  No atomics; results do not depend on tiling or timing.
 *
 * stencil_mg_fmg: the pass on a hierarchy of L levels.
 *   1. For l = 0 .. L-2: level l+1's source = the coarse source of level l's
 *      source; both field grids of level l+1 zeroed; level l's field ghost
 *      shell injected into both field grids of level l+1.  Level 0's ghost
 *      shell is the caller's; level 0's interior is ignored and overwritten.
 *   2. Level L-1: coarse_sweeps relaxed sweeps from its zero interior (L = 1:
 *      the whole pass, on level 0 with its interior zeroed first).
 *   3. For l = L-2 .. 0: level l's interior = the cubic prolongation of level
 *      l+1's field; both field grids of level l+1 zeroed entirely (so that later
 *      V-cycles find the zero ghost cells they rely on); `cycles` V-cycles
 *      started at level l (stencil_mg_vcycle's recursion from that level; it
 *      overwrites only sources of levels > l, which are consumed).  cycles = 0
 *      is allowed.
 * After the pass the field and the source of every level are bitwise defined,
 * and every level >= 1 has zero ghost cells in both grids, as after creation.
 * STENCIL_EINVAL as stencil_mg_vcycle.
 * stencil_mg_fmg_plan (host only): the kernel launches of the pass -- per level
 * but the coarsest one source restriction, one injection and one cubic
 * prolongation, stencil_relax_plan of the coarsest run, and `cycles` times the
 * launches of a V-cycle started at each level l < L-1 (stencil_mg_plan's count
 * from that level down); memsets are not counted -- and the level count.
 * All argument errors fire before a device is touched. */
int stencil_restrict_source(const stencil_layout* lf, const void* src, const stencil_layout* lc, void* coarse_src,
                            int64_t cbegin, int64_t cend, void* stream);
int stencil_inject_ghosts(const stencil_layout* lf, const void* u, const stencil_layout* lc, void* uc, void* stream);
int stencil_prolong_cubic(const stencil_layout* lc, const void* e, const stencil_layout* lf, void* u, int64_t begin,
                          int64_t end, void* stream);
int stencil_mg_fmg(stencil_mg* mg, const stencil_mg_params* params, uint32_t cycles, void* stream);
int stencil_mg_fmg_plan(const stencil_problem* fine, int32_t levels, const stencil_mg_params* params, uint32_t cycles,
                        int64_t* launches, int32_t* levels_out);

/* A plain device copy kernel (read n bytes, write n bytes) used by bench.py to
 * calibrate attainable HBM bandwidth on the box. */
int stencil_copy_bandwidth(void* dst, const void* src, int64_t bytes, int reps, void* stream,
                           float* elapsed_ms);

/* ------------------------------------------------ 3. multi-GPU z-slab jobs
 *
 * The reference runs its whole decomposed job behind one call: 64 CPEs own
 * 8x8 blocks and exchange halo strips every iteration (athread_spawn/join,
 * src/stencil/stencil.cpp:34-53; stencil_dma.cpp:236-247, stencil_rma.cpp:
 * 198-255).  A slab job does the same across GPUs from ONE host thread: the
 * global 3D grid is cut into contiguous z-slabs (remainder planes to the
 * lowest slabs), slab i lives on devices[i] with K ghost planes per shared
 * face (K = the sweeps stencil_iterate fuses into one launch for `global`),
 * and every round of K fused sweeps exchanges K whole planes with each
 * neighbour: the boundary planes first on a high-priority stream with the
 * exchange behind them, the interior on a second stream.  Results are bitwise
 * those of one grid.  Exchange: RCCL ncclSend/ncclRecv (ncclCommInitAll over
 * the devices, one slab per GPU; librccl is loaded on first use) or device
 * copies (hipMemcpyPeerAsync; slabs may share a GPU).  PERIODIC joins the
 * two z ends into a ring (a rehearsal mode: one slab exchanges with itself). */
enum { STENCIL_EXCHANGE_RCCL = 0, STENCIL_EXCHANGE_COPY = 1 };
/* PERIODIC: the z ends form a ring.  ROLLING: each slab keeps ONE resident
 * grid plus a margin of spare planes instead of two grids (the scheme of
 * stencil_rolling_*, per slab): a round is a pass of ceil(n / S) z-range
 * launches (S = margin - K*radius), then the exchange -- for slabs whose two
 * grids do not fit one GPU, e.g. the north star's 4096^3 fp64 on 2 GPUs (one
 * 278 GB grid each).  Bitwise the two-grid job; no face-signalled rounds.
 * No sweep writes a ghost cell, and a pass lands each plane in a slot whose
 * x/y ghost ring came from another plane, so a ROLLING job needs the same
 * x/y ghost ring in every plane and equal bottom ghost planes (the reference
 * initial condition has both): stencil_slab_upload checks a host grid for
 * this and returns STENCIL_EINVAL otherwise. */
enum { STENCIL_SLAB_PERIODIC = 1, STENCIL_SLAB_ROLLING = 2 };
typedef struct stencil_slab_job stencil_slab_job;

/* global: a 3D problem with halo = 0 and flags = 0; devices: ngpus ordinals
 * (NULL = 0 .. ngpus-1).  Every slab must own at least K planes. */
int stencil_slab_create(const stencil_problem* global, int32_t ngpus, const int32_t* devices, int32_t exchange,
                        int32_t flags, stencil_slab_job** job);
/* The same with the rolling margin: margin_planes > 0 spare planes per slab
 * (at least K*radius + 1), 0 = as deep as each device's free memory allows
 * beside its grid (less a 4 GiB reserve for RCCL), at most 512.  Ignored
 * without STENCIL_SLAB_ROLLING. */
int stencil_slab_create2(const stencil_problem* global, int32_t ngpus, const int32_t* devices, int32_t exchange,
                         int32_t flags, int64_t margin_planes, stencil_slab_job** job);
/* Rank mode: one process per GPU, as the reference's MPI-style launch and
 * torch.distributed.run give it.  Rank 0 makes an RCCL id
 * (stencil_slab_unique_id, STENCIL_SLAB_ID_BYTES bytes) and hands it to every
 * rank by its own channel (a torch.distributed broadcast, MPI_Bcast, a file);
 * each rank then calls stencil_slab_create_rank with the same global problem
 * and builds only its slab (z split as above, slab = rank) on `device`, joined
 * by ncclCommInitRank -- a collective: every rank must call it (a rank that
 * does not within STENCIL_SLAB_TIMEOUT_MS fails the others' calls with
 * STENCIL_ETIMEOUT; RCCL's bootstrap thread for the abandoned attempt then
 * stays blocked until the process exits).  The job then
 * holds ONE slab (stencil_slab_info slab 0) and every call below is
 * per-rank and collective over the ranks (run: every rank the same
 * iterations).  Host arrays keep the global shape: upload reads and download /
 * plane_sums write only this rank's planes (download: plus the global ghost
 * planes at the two ends).  Exchange is always RCCL. */
enum { STENCIL_SLAB_ID_BYTES = 128 };
int stencil_slab_unique_id(void* id, int64_t bytes);
int stencil_slab_create_rank(const stencil_problem* global, int32_t nranks, int32_t rank, int32_t device,
                             const void* id, int64_t id_bytes, int32_t flags, stencil_slab_job** job);
int stencil_slab_create_rank2(const stencil_problem* global, int32_t nranks, int32_t rank, int32_t device,
                              const void* id, int64_t id_bytes, int32_t flags, int64_t margin_planes,
                              stencil_slab_job** job);
int stencil_slab_destroy(stencil_slab_job* job);
int stencil_slab_info(const stencil_slab_job* job, int32_t slab, int64_t* first_plane, int64_t* planes,
                      int32_t* device, int32_t* sweeps_per_round);
/* Rolling slabs: the margin (0: two grids per slab) and the most z-range
 * launches one pass makes on a slab of this process. */
int stencil_slab_rolling_info(const stencil_slab_job* job, int64_t* margin_planes, int64_t* launches_per_pass);
/* Initial condition of the global grid (global linear indices for the random
 * interior, as stencil_fill_initial on one grid), halos exchanged. */
int stencil_slab_fill_initial(stencil_slab_job* job, int32_t init_kind, uint64_t seed);
/* The global grid from / to a dense host array with ghosts (x fastest,
 * host_row elements per row, host_rows rows per plane, nz + 2r planes).
 * ROLLING jobs: see the ghost-ring condition above. */
int stencil_slab_upload(stencil_slab_job* job, const void* host, int64_t host_row, int64_t host_rows);
int stencil_slab_download(stencil_slab_job* job, void* host, int64_t host_row, int64_t host_rows);
/* `iterations` sweeps of the whole job (rounds of K, the remainder as one
 * shorter round); synchronous.  elapsed_ms: host wall time of the rounds,
 * all devices synchronised at both ends. */
int stencil_slab_run(stencil_slab_job* job, uint32_t iterations, float* elapsed_ms);
/* Sweeps until the update is small: stencil_iterate_until's stopping rule on a
 * slab job.  Blocks of min(check_every, max_iterations - done) sweeps, each
 * followed by the norm (STENCIL_NORM_MAX / STENCIL_NORM_L2) of u^n - u^(n-1)
 * over the whole global interior; stops with *converged = 1 when norm <= tol,
 * with 0 on a NaN norm or at the cap (a shorter last block is checked too);
 * max_iterations = 0: 0 sweeps, not converged, norm +inf.  STENCIL_OK either
 * way.  Afterwards the job is in the state stencil_slab_run(*iterations_done)
 * would leave.
 *   Check in the launch (max norm, rounds of K = 3..5 7-point strip launches,
 * block >= K, STENCIL_UNTIL_FUSED not 0): block - K sweeps as stencil_slab_run
 * issues them, then one checking round of K sweeps -- a face-signalled job's
 * round with stencil_sweepk_signal_update_max (gated when the job is), every
 * other two-grid job's boundary + interior round with
 * stencil_sweepk_update_max -- raising one 8-byte word per slab, zeroed in
 * stream order before the round and copied back after it; the norm is the
 * maximum of the slabs' bit patterns (a NaN pattern wins).
 *   Otherwise (L2, the box, blocks shorter than K, other families,
 * STENCIL_UNTIL_FUSED=0): block - 1 sweeps, one round of a single sweep, then
 * stencil_diff_norms' kernels per slab over its own planes; the maximum, or
 * the per-plane sums added in ascending global plane order.  A plane's values
 * depend on nx, ny and the row pitch alone, so both norms are bit for bit the
 * single grid's.
 *   Every host wait goes through the job's deadline (stencil_slab_set_timeout).
 * STENCIL_EINVAL: NULL job, check_every = 0, tol < 0 or NaN, unknown norm.
 * STENCIL_EUNSUPPORTED: STENCIL_SLAB_ROLLING jobs (one grid: u^(n-1) is gone)
 * and rank-mode jobs (the check would need an all-reduce over the ranks).
 * elapsed_ms: host wall time of rounds and checks, as stencil_slab_run.
 * stencil_slab_until_plan (host only, no device): the rounds of one block of
 * `block` sweeps, its checking round included -- fused (block-K)/K rounded up
 * + 1, un-fused (block-1)/K rounded up + 1, K as stencil_plan resolves it --
 * and whether the check rides in the launch.  STENCIL_EINVAL: block = 0,
 * unknown norm, a problem that is not a valid slab global. */
int stencil_slab_run_until(stencil_slab_job* job, uint32_t max_iterations, uint32_t check_every, int32_t norm,
                           double tol, uint32_t* iterations_done, double* last_norm, int* converged,
                           float* elapsed_ms);
int stencil_slab_until_plan(const stencil_problem* global, uint32_t block, int32_t norm, int64_t* rounds,
                            int32_t* fused_check);
/* Source terms across the slabs: u' = S(u) + g on the whole global grid
 * (Poisson solves over GPUs).  Scope: two-grid jobs of the 3D 7-point star,
 * r = 1, naive order, kernel AUTO or TEMPORALK.
 *   stencil_slab_set_source: `host` has the global shape, as
 * stencil_slab_upload takes it; only its interior cells have meaning.  The
 * first call allocates one source grid per slab (STENCIL_ENOMEM if one does
 * not fit: nothing is kept and the job stays usable); afterwards each slab's
 * source grid holds its planes and, in the halo planes of each shared face,
 * the neighbouring slab's (wrapped with STENCIL_SLAB_PERIODIC), filled by one
 * exchange of the source grids.  Rank mode reads only the rank's planes.  A
 * second call replaces the values.
 *   stencil_slab_run_source: stencil_slab_run with the source.  Rounds take
 * Ks = min(K, STENCIL_SOURCE_MAX_STEPS) sweeps, the remainder as one shorter
 * round; the halo depth stays K.  Results are bitwise those of
 * stencil_iterate_source on one grid, and it may alternate freely with
 * stencil_slab_run.  A full round of a face-signalled job with Ks = K is one
 * stencil_sweepk_signal_source launch per slab -- gated when the job is and
 * the launch's own tiles meet the gate's rule, else waiting for the exchange's
 * event -- unless STENCIL_SLAB_SOURCE_SIGNAL=0 or the job waits for its faces
 * in the command processor (STENCIL_SLAB_CPWAIT=1).  Every other round --
 * staged jobs' (their tuning state is not touched), remainders, Ks < K, slabs
 * sharing a GPU -- is boundary + interior launches of
 * stencil_sweepk_source_halo, or one launch with STENCIL_SLAB_SERIAL=1.
 * stencil_slab_source_round_form reports a full source round's form
 * (STENCIL_SLAB_FORM_SIGNALLED, _BOUNDARY_INTERIOR or _SERIAL).
 *   stencil_slab_run_until_source: stencil_slab_run_until's arguments,
 * stopping rule and edge cases on source rounds, always with the un-fused
 * check: block - 1 source sweeps as run_source issues them, one round of a
 * single source sweep, then stencil_diff_norms' kernels per slab, reduced as
 * stencil_slab_run_until's un-fused check.  Counts, norms (bit for bit) and
 * grid equal stencil_iterate_until_source's on one grid.
 *   stencil_slab_source_plan (host only): *rounds = ceil(iterations / Ks),
 * *steps = Ks.
 * STENCIL_EINVAL: NULL arguments, a host array that is too small, run*_source
 * before set_source, run_until's argument errors.  STENCIL_EUNSUPPORTED (the
 * message names the restriction): STENCIL_SLAB_ROLLING jobs (one resident
 * grid), anything but the 3D r = 1 naive 7-point star; run_until_source in
 * rank mode.  Every host wait goes through the job's deadline. */
int stencil_slab_set_source(stencil_slab_job* job, const void* host, int64_t host_row, int64_t host_rows);
int stencil_slab_run_source(stencil_slab_job* job, uint32_t iterations, float* elapsed_ms);
int stencil_slab_run_until_source(stencil_slab_job* job, uint32_t max_iterations, uint32_t check_every,
                                  int32_t norm, double tol, uint32_t* iterations_done, double* last_norm,
                                  int* converged, float* elapsed_ms);
int stencil_slab_source_plan(const stencil_problem* global, uint32_t iterations, int64_t* rounds, int32_t* steps);
int stencil_slab_source_round_form(const stencil_slab_job* job, int32_t* form);
/* Relaxed sweeps in slab jobs: u' = u + w (S(u) + g - u) with a weight per
 * sweep (damped Jacobi; Chebyshev Jacobi with a schedule) across the slabs.
 * Scope: that of the source rounds -- two-grid jobs of the 3D 7-point star,
 * r = 1, naive order, kernel AUTO or TEMPORALK, fp32 / fp64, slab mode (slabs
 * may share a GPU) and rank mode, STENCIL_SLAB_PERIODIC allowed.  The grid g is
 * stencil_slab_set_source's; for a plain smoother it is a grid of zeros.
 *   stencil_slab_run_relax: stencil_slab_run_source with weights.  `omegas` is
 * a host array of `period` doubles; sweep i of the call (0-based) takes
 * omegas[(phase + i) % period], so a caller continues a schedule across calls
 * by passing the sweeps done so far as `phase`.  Rounds take
 * Ks = min(K, STENCIL_SOURCE_MAX_STEPS) sweeps, the remainder as one shorter
 * round; the halo depth stays K; all slabs of a round take the same weights,
 * which travel as launch arguments (nothing is uploaded per round).  Results
 * are bitwise those of stencil_iterate_relax on one grid, and it alternates
 * freely with stencil_slab_run and stencil_slab_run_source.  The form of a
 * full relaxed round follows the source round's rule: one
 * stencil_sweepk_signal_relax launch per slab where the job's rounds are
 * face-signalled, Ks = K >= 3, the job does not wait for its faces in the
 * command processor (STENCIL_SLAB_CPWAIT=1) and STENCIL_SLAB_SOURCE_SIGNAL is
 * not 0 -- the one knob governs source and relaxed rounds alike -- gated when
 * the job is and the relaxed launch's own tiles meet the gate's rule (decided
 * once per job, apart from the source rounds' decision).  Every other round --
 * staged jobs', remainders, Ks < K (K = 5 jobs), slabs sharing a GPU -- is
 * boundary + interior launches of stencil_sweepk_relax_halo, or one launch
 * with STENCIL_SLAB_SERIAL=1.  stencil_slab_relax_round_form reports a full
 * relaxed round's form (STENCIL_SLAB_FORM_SIGNALLED, _BOUNDARY_INTERIOR or
 * _SERIAL).
 *   stencil_slab_run_until_relax: stencil_slab_run_until's arguments, stopping
 * rule and edge cases on relaxed rounds, always with the un-fused check:
 * block - 1 relaxed sweeps as run_relax issues them, one round of a single
 * relaxed sweep, then stencil_diff_norms' kernels per slab.  The schedule
 * index runs on across blocks and the checking sweep takes its own weight.
 * Counts, norms (bit for bit) and grid equal stencil_iterate_until_relax's on
 * one grid.
 *   stencil_slab_relax_plan (host only) equals stencil_slab_source_plan.
 * STENCIL_EINVAL: a NULL job or omegas, period == 0, a weight that is NaN or
 * infinite, run*_relax before stencil_slab_set_source (the message names
 * set_source), run_until's argument errors.  STENCIL_EUNSUPPORTED (the message
 * names the restriction): STENCIL_SLAB_ROLLING jobs, anything but the 3D r = 1
 * naive 7-point star; run_until_relax in rank mode.  A refused call leaves the
 * job usable.  Every host wait goes through the job's deadline. */
int stencil_slab_run_relax(stencil_slab_job* job, uint32_t iterations, const double* omegas, uint32_t period,
                           uint32_t phase, float* elapsed_ms);
int stencil_slab_run_until_relax(stencil_slab_job* job, uint32_t max_iterations, uint32_t check_every,
                                 int32_t norm, double tol, const double* omegas, uint32_t period,
                                 uint32_t phase, uint32_t* iterations_done, double* last_norm, int* converged,
                                 float* elapsed_ms);
int stencil_slab_relax_plan(const stencil_problem* global, uint32_t iterations, int64_t* rounds, int32_t* steps);
int stencil_slab_relax_round_form(const stencil_slab_job* job, int32_t* form);
/* Per-plane interior sums of the current global grid (nz doubles, host). */
int stencil_slab_plane_sums(stencil_slab_job* job, double* sums);
/* Kernel timing for roofline figures: with timing on, every round records
 * hipEvents around slab 0's compute launch (the whole slab in face-signalled
 * rounds, its interior launch in boundary + interior rounds, the pass's
 * z-range launches in rolling rounds) on that launch's stream.  kernel_time
 * synchronises and returns the summed device time, the spans timed, the
 * interior cells one span covers and whether the rounds are face-signalled
 * (1) or not (0); stencil_slab_round_form gives the form (a staged round's
 * span is its face launches and its middle launch).  Enabling (or
 * disabling) drops earlier records. */
int stencil_slab_kernel_timing(stencil_slab_job* job, int32_t enable);
int stencil_slab_kernel_time(stencil_slab_job* job, float* total_ms, int64_t* launches, int64_t* cells_per_launch,
                             int32_t* signalled);
/* With kernel timing on, every timed round also records its exchange on slab
 * 0's exchange stream: from the end of what precedes the transfers there (the
 * face wait of a face-signalled round; a rolling round's face launches) to
 * the end of the RCCL send/recv (or copies).  exchange_time synchronises and
 * returns the summed transfer time, the part of it that ran while the same
 * round's timed launch span ran (the overlap the round form is for; ~0 for
 * serial rounds), and the exchanges counted.  Over xGMI this is the wire
 * time of K planes per shared face plus RCCL's own latency. */
int stencil_slab_exchange_time(stencil_slab_job* job, float* transfer_ms, float* beside_ms, int64_t* exchanges);
/* The form of the job's full rounds (kernel_time's `signalled` is 1 for
 * face-signalled rounds, 0 otherwise). */
enum {
    STENCIL_SLAB_FORM_BOUNDARY_INTERIOR = 0, /* boundary planes on one stream, the interior on another */
    STENCIL_SLAB_FORM_SIGNALLED = 1,         /* one face-signalled launch, the exchange as the faces land */
    STENCIL_SLAB_FORM_ROLLING = 2,           /* one grid + a margin: a pass of z-range launches */
    STENCIL_SLAB_FORM_SERIAL = 3,            /* one launch of the whole slab, then the exchange */
    STENCIL_SLAB_FORM_STAGED = 4             /* the face quarters, then the middle beside the exchange */
};
int stencil_slab_round_form(const stencil_slab_job* job, int32_t* form);
/* How the job's full rounds run beyond their form (each output may be NULL):
 * *gated = 1 when face-signalled launches gate their halo-reading workgroups
 * on the exchange-completion word instead of waiting for the exchange stream
 * (stencil_sweepk_signal_gated; STENCIL_SLAB_GATE=0: never), *confined = 1
 * when the exchange runs on a few CUs of its own (STENCIL_SLAB_XCU). */
int stencil_slab_round_info(const stencil_slab_job* job, int32_t* form, int32_t* gated, int32_t* confined);
/* The exchange's CU budget (staged rounds with a confined exchange, slab 0):
 * CUs per XCD in use, the alternative budget the tuning rounds tried (0:
 * none; STENCIL_SLAB_XCU_ALT, default 4), and the timed tuning round with the
 * default (STENCIL_SLAB_XCU) and with the alternative budget, ms (0: not run:
 * the alternative is tried only when the exchange ran at least 0.8x as long
 * as the middle launch beside it).  The faster is kept (the alternative only
 * when 2 % faster); the face span is then tuned from that round. */
int stencil_slab_exchange_budget(const stencil_slab_job* job, int32_t* cus, int32_t* alt_cus, float* round_ms,
                                 float* alt_round_ms);
/* Bounded-time failure.  Every wait of the job for its devices (the end of
 * run(), fill, upload, download, plane sums, and -- while run() issues
 * rounds -- the exchange of the round kInflight = 8 rounds back) gives up
 * after `timeout_ms` (default 60000, or the STENCIL_SLAB_TIMEOUT_MS knob at
 * creation); so does an asynchronous RCCL error, polled meanwhile
 * (ncclCommGetAsyncError).  The job then aborts its communicators
 * (ncclCommAbort: RCCL's kernels waiting for a peer that stopped posting
 * return), releases its queued face waits, and the call returns
 * STENCIL_ETIMEOUT (or the error); every later call on the job fails, and
 * stencil_slab_destroy frees it.  The reference has no counterpart: its
 * never-waited reply (stencil_rma.cpp:334-338) hangs instead. */
int stencil_slab_set_timeout(stencil_slab_job* job, int64_t timeout_ms);

#ifdef __cplusplus
}
#endif

#endif /* STENCIL_HIP_H */
