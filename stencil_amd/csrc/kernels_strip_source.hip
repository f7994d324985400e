// kernels_strip_source.hip -- the 7-point strip kernel (kernels_strip.hip) with
// its source option (SRC): the shapes of stencil_sweepk_source's fused
// launches (on slab layouts too: stencil_sweepk_source_halo) and of the
// face-signalled source launches (SRC + SIG: stencil_sweepk_signal_source), a
// translation unit of their own so the plain shapes' build is what it was.
// Same sums as the plain kernel, then the source added with a rounding of its
// own.
#define STRIP_SOURCE_TU
#include "kernels_strip.hip"
