// kernels_strip_relax.hip -- the 7-point strip kernel (kernels_strip.hip) with
// its source and relaxation options (SRC + RLX): the shapes of
// stencil_sweepk_relax's fused launches, a translation unit of their own so
// every other shape's build is what it was.  Each sweep is the source sweep's
// value J relaxed by the sweep's own weight, u' = u + w (J - u), in four
// roundings after the multiply and never an fma.
#define STRIP_RELAX_TU
#include "kernels_strip.hip"
