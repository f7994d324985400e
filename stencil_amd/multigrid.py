"""Geometric multigrid for the 7-point Poisson solve on one GPU (stencil_mg_*,
stencil_restrict_residual, stencil_prolong_add, stencil_residual_norms:
include/stencil_hip.h, csrc/kernels_mg.hip), and its full
multigrid start-up (stencil_mg_fmg, stencil_restrict_source,
stencil_inject_ghosts, stencil_prolong_cubic: DESIGN.md §5.10).

`PoissonMultigrid` owns a hierarchy of vertex-centred coarsenings -- odd
extents n >= 3 coarsen to (n - 1) / 2 -- and runs V-cycles whose smoother is
the relaxed sweep of JacobiEngine.iterate_relax.  The module functions
`coarsen`, `restrict_residual`, `prolong_add` and `residual_norms` run the
transfer kernels on JacobiEngine grids; `restrict_source`, `inject_ghosts` and
`prolong_cubic` those of the full multigrid pass (`PoissonMultigrid.fmg`).
Everything is bitwise defined (tests/mg_ref.py and tests/fmg_ref.py state it in
numpy).
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .engine import _NP_DTYPE, _TORCH_DTYPE, JacobiEngine, StencilSpec, UntilResult, _stream_handle

# kernels_mg.hip's restriction tile: coarse cells per workgroup in x and y, coarse planes per z-run
RESTRICT_TILE = (32, 8)
RESTRICT_ZRUN = 8
# the smoother of the issue's measurements: V(2,2), damped Jacobi with omega = 6/7, 8 sweeps on the coarsest level
DEFAULT_OMEGAS = (6.0 / 7.0,)


def _ptr(t: torch.Tensor) -> ctypes.c_void_p:
    return ctypes.c_void_p(t.data_ptr())


def _params(pre: int, post: int, coarse_sweeps: int, omegas):
    """(stencil_mg_params, the array it points into -- keep both alive)."""
    w = [float(x) for x in (omegas if hasattr(omegas, "__len__") else [omegas])]
    arr = (ctypes.c_double * max(1, len(w)))(*w)
    return _lib.MgParams(pre, post, coarse_sweeps, len(w), arr if w else None), arr


def coarsen_problem(prob: _lib.Problem, lib=None) -> _lib.Problem:
    """The coarse problem of `prob` (stencil_coarsen_problem, host only)."""
    lib = lib if lib is not None else _lib.load()
    out = _lib.Problem()
    _lib.check(lib.stencil_coarsen_problem(ctypes.byref(prob), ctypes.byref(out)), "stencil_coarsen_problem", lib=lib)
    return out


def coarsen(fine: JacobiEngine) -> JacobiEngine:
    """A JacobiEngine for the coarsening of `fine`'s problem, on its device."""
    c = coarsen_problem(fine.prob, fine.lib)
    return JacobiEngine(fine.spec, int(c.nx), int(c.ny), int(c.nz), device=fine.device)


def restrict_residual(fine: JacobiEngine, u: torch.Tensor, src: torch.Tensor, coarse: JacobiEngine,
                      coarse_src: torch.Tensor, cbegin: int = 0, cend: int | None = None, stream=None) -> None:
    """coarse_src = 4 R(r) on coarse planes [cbegin, cend), r the residual of
    the field `u` with the source `src` on the fine grid
    (stencil_restrict_residual); the residual is never stored."""
    cend = int(coarse.prob.nz) if cend is None else cend
    _lib.check(fine.lib.stencil_restrict_residual(ctypes.byref(fine.layout), _ptr(u), _ptr(src),
                                                  ctypes.byref(coarse.layout), _ptr(coarse_src), cbegin, cend,
                                                  _stream_handle(stream)), "stencil_restrict_residual", lib=fine.lib)


def prolong_add(coarse: JacobiEngine, e: torch.Tensor, fine: JacobiEngine, u: torch.Tensor, begin: int = 0,
                end: int | None = None, stream=None) -> None:
    """u += P(e) on fine planes [begin, end), in place (stencil_prolong_add);
    e's ghost ring is read, edges and corners included."""
    end = int(fine.prob.nz) if end is None else end
    _lib.check(fine.lib.stencil_prolong_add(ctypes.byref(coarse.layout), _ptr(e), ctypes.byref(fine.layout), _ptr(u),
                                            begin, end, _stream_handle(stream)), "stencil_prolong_add", lib=fine.lib)


def restrict_source(fine: JacobiEngine, src: torch.Tensor, coarse: JacobiEngine, coarse_src: torch.Tensor,
                    cbegin: int = 0, cend: int | None = None, stream=None) -> None:
    """coarse_src = 4 R(src) on coarse planes [cbegin, cend): the coarse
    problem's source of the full multigrid pass (stencil_restrict_source)."""
    cend = int(coarse.prob.nz) if cend is None else cend
    _lib.check(fine.lib.stencil_restrict_source(ctypes.byref(fine.layout), _ptr(src), ctypes.byref(coarse.layout),
                                                _ptr(coarse_src), cbegin, cend, _stream_handle(stream)),
               "stencil_restrict_source", lib=fine.lib)


def inject_ghosts(fine: JacobiEngine, u: torch.Tensor, coarse: JacobiEngine, uc: torch.Tensor, stream=None) -> None:
    """uc's ghost shell (edges and corners included) = the cells of u's ghost
    shell it sits on: the coarse problem's Dirichlet data (stencil_inject_ghosts)."""
    _lib.check(fine.lib.stencil_inject_ghosts(ctypes.byref(fine.layout), _ptr(u), ctypes.byref(coarse.layout), _ptr(uc),
                                              _stream_handle(stream)), "stencil_inject_ghosts", lib=fine.lib)


def prolong_cubic(coarse: JacobiEngine, e: torch.Tensor, fine: JacobiEngine, u: torch.Tensor, begin: int = 0,
                  end: int | None = None, stream=None) -> None:
    """u = the cubic prolongation of e on fine planes [begin, end) -- a set,
    not an add (stencil_prolong_cubic); e's ghost ring is read, edges and
    corners included."""
    end = int(fine.prob.nz) if end is None else end
    _lib.check(fine.lib.stencil_prolong_cubic(ctypes.byref(coarse.layout), _ptr(e), ctypes.byref(fine.layout), _ptr(u),
                                              begin, end, _stream_handle(stream)), "stencil_prolong_cubic", lib=fine.lib)


def _residual_norms(lib, layout, u_ptr, src_ptr, begin, end, stream):
    n = max(0, end - begin)
    max_abs, sum_sq = np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.float64)
    dp = ctypes.POINTER(ctypes.c_double)
    _lib.check(lib.stencil_residual_norms(ctypes.byref(layout), u_ptr, src_ptr, begin, end, max_abs.ctypes.data_as(dp),
                                          sum_sq.ctypes.data_as(dp), _stream_handle(stream)),
               "stencil_residual_norms", lib=lib)
    return max_abs, sum_sq


def residual_norms(e: JacobiEngine, u: torch.Tensor, src: torch.Tensor, begin: int = 0, end: int | None = None,
                   stream=None):
    """Per-plane (max |r|, sum r^2) of the residual over planes [begin, end),
    in double (stencil_residual_norms); two numpy float64 arrays."""
    end = int(e.prob.nz) if end is None else end
    return _residual_norms(e.lib, e.layout, _ptr(u), _ptr(src), begin, end, stream)


def _scalar_norm(max_abs: np.ndarray, sum_sq: np.ndarray, norm: str) -> float:
    """stencil_diff_norms' scalar norm of per-plane values."""
    kind = _lib.NORM_NAMES[norm]
    if np.isnan(max_abs).any():
        return float("nan")
    if kind == _lib.NORM_MAX:
        return float(max_abs.max()) if max_abs.size else 0.0
    total = 0.0
    for v in sum_sq:
        total += float(v)
    return float(np.sqrt(total))


def mg_plan(spec: StencilSpec, nx: int, ny: int, nz: int, levels: int = 0, pre: int = 2, post: int = 2,
            coarse_sweeps: int = 8, omegas=DEFAULT_OMEGAS, lib=None) -> dict:
    """One V-cycle as kernel launches, and the level count `levels` resolves
    to (stencil_mg_plan; host only, no device)."""
    lib = lib if lib is not None else _lib.load()
    prob = spec.problem(nx, ny, nz)
    par, _keep = _params(pre, post, coarse_sweeps, omegas)
    launches, nlev = ctypes.c_int64(0), ctypes.c_int32(0)
    _lib.check(lib.stencil_mg_plan(ctypes.byref(prob), levels, ctypes.byref(par), ctypes.byref(launches),
                                   ctypes.byref(nlev)), "stencil_mg_plan", lib=lib)
    return {"launches": int(launches.value), "levels": int(nlev.value)}


def fmg_plan(spec: StencilSpec, nx: int, ny: int, nz: int, levels: int = 0, cycles: int = 2, pre: int = 2, post: int = 2,
             coarse_sweeps: int = 8, omegas=DEFAULT_OMEGAS, lib=None) -> dict:
    """One full multigrid pass as kernel launches (memsets not counted), and
    the level count (stencil_mg_fmg_plan; host only, no device)."""
    lib = lib if lib is not None else _lib.load()
    prob = spec.problem(nx, ny, nz)
    par, _keep = _params(pre, post, coarse_sweeps, omegas)
    launches, nlev = ctypes.c_int64(0), ctypes.c_int32(0)
    _lib.check(lib.stencil_mg_fmg_plan(ctypes.byref(prob), levels, ctypes.byref(par), cycles, ctypes.byref(launches),
                                       ctypes.byref(nlev)), "stencil_mg_fmg_plan", lib=lib)
    return {"launches": int(launches.value), "levels": int(nlev.value)}


class _DeviceMemory:
    """A device allocation of the library's as torch sees it (the CUDA array interface)."""

    def __init__(self, ptr: int, count: int, np_dtype):
        self.__cuda_array_interface__ = {"shape": (count,), "typestr": np.dtype(np_dtype).str, "data": (ptr, False),
                                         "version": 2, "strides": None}


@dataclass(frozen=True)
class MgLevel:
    """One level of a hierarchy: its layout and flat tensors over the grid that
    currently holds its field and over its source grid (the library's memory:
    valid until the hierarchy is closed; `field` until the next cycle)."""
    layout: _lib.Layout
    field: torch.Tensor
    source: torch.Tensor

    @property
    def shape(self):
        p = self.layout.prob
        return int(p.nx), int(p.ny), int(p.nz)

    def interior(self, grid: torch.Tensor) -> torch.Tensor:
        """Strided (nz, ny, nx) view of the interior."""
        p, lay = self.layout.prob, self.layout
        return grid.as_strided((p.nz, p.ny, p.nx), (lay.plane, lay.row, 1), grid.storage_offset() + lay.origin)

    def with_ghosts(self, grid: torch.Tensor) -> torch.Tensor:
        """Strided view of interior + ghost ring, the oracle's dense shape."""
        p, lay = self.layout.prob, self.layout
        corner = grid.storage_offset() + lay.origin - lay.plane - lay.row - 1
        return grid.as_strided((p.nz + 2, p.ny + 2, p.nx + 2), (lay.plane, lay.row, 1), corner)

    def to_numpy(self, grid: torch.Tensor) -> np.ndarray:
        torch.cuda.synchronize(grid.device)
        return self.with_ghosts(grid).cpu().numpy().copy()


class PoissonMultigrid:
    """A multigrid hierarchy for u = S(u) + g on an nx x ny x nz grid (odd
    extents coarsen; `levels` = 0: as many levels as the extents give)."""

    def __init__(self, spec: StencilSpec, nx: int, ny: int, nz: int, levels: int = 0, device: int | torch.device = 0):
        self.lib = _lib.load()
        self.spec = spec
        self.shape = (nx, ny, nz)
        self.prob = spec.problem(nx, ny, nz)
        self.device = torch.device("cuda", device) if isinstance(device, int) else device
        self.torch_dtype = _TORCH_DTYPE[self.prob.dtype]
        self.np_dtype = _NP_DTYPE[self.prob.dtype]
        self.mg = None
        mg = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.stencil_mg_create(ctypes.byref(self.prob), levels, ctypes.byref(mg)), "stencil_mg_create",
                       lib=self.lib)
        self.mg = mg
        n = ctypes.c_int32(0)
        _lib.check(self.lib.stencil_mg_levels(self.mg, ctypes.byref(n)), "stencil_mg_levels", lib=self.lib)
        self.levels = int(n.value)

    def close(self) -> None:
        if self.mg:
            self.lib.stencil_mg_destroy(self.mg)
            self.mg = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ data
    def _padded(self, dense, what: str) -> np.ndarray:
        nx, ny, nz = self.shape
        inner, padded = (nz, ny, nx), (nz + 2, ny + 2, nx + 2)
        a = dense.detach().cpu().numpy() if isinstance(dense, torch.Tensor) else np.asarray(dense)
        if a.shape == padded:
            return np.ascontiguousarray(a, dtype=self.np_dtype)
        if a.shape != inner:
            raise ValueError(f"{what} of shape {a.shape}: expected {inner} or {padded}")
        out = np.zeros(padded, dtype=self.np_dtype)
        out[1:-1, 1:-1, 1:-1] = a
        return out

    def _upload(self, field, source, stream) -> None:
        keep = [a for a in (field, source) if a is not None]
        with torch.cuda.device(self.device):
            _lib.check(self.lib.stencil_mg_upload(self.mg, field.ctypes.data if field is not None else None,
                                                  source.ctypes.data if source is not None else None,
                                                  keep[0].shape[2], keep[0].shape[1], _stream_handle(stream)),
                       "stencil_mg_upload", lib=self.lib)
            _lib.check(self.lib.stencil_synchronize(_stream_handle(stream)), "stencil_synchronize", lib=self.lib)

    def set_field(self, dense, stream=None) -> None:
        """The fine field: a dense ghost-padded (nz + 2, ny + 2, nx + 2) array
        (its ghost cells are the Dirichlet data), or the (nz, ny, nx) interior
        inside zero ghost cells."""
        self._upload(self._padded(dense, "field"), None, stream)

    def set_source(self, dense, stream=None) -> None:
        """The fine source g, scaled by the caller (g = h^2 / 6 f): (nz, ny, nx)
        or ghost-padded (the ghost cells have no meaning)."""
        self._upload(None, self._padded(dense, "source"), stream)

    def download(self, stream=None) -> np.ndarray:
        """The fine field, dense with ghosts (the oracle's layout)."""
        nx, ny, nz = self.shape
        out = np.zeros((nz + 2, ny + 2, nx + 2), dtype=self.np_dtype)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.stencil_mg_download(self.mg, out.ctypes.data, None, nx + 2, ny + 2,
                                                    _stream_handle(stream)), "stencil_mg_download", lib=self.lib)
            _lib.check(self.lib.stencil_synchronize(_stream_handle(stream)), "stencil_synchronize", lib=self.lib)
        return out

    def level(self, i: int) -> MgLevel:
        """Level i (0 = fine): its layout and tensors over its grids."""
        lay = _lib.Layout()
        field, source = ctypes.c_void_p(), ctypes.c_void_p()
        _lib.check(self.lib.stencil_mg_level(self.mg, i, ctypes.byref(lay), ctypes.byref(field), ctypes.byref(source)),
                   "stencil_mg_level", lib=self.lib)
        count = int(lay.elems) + 256 // self.spec.elem_bytes  # tail pad, as stencil_alloc
        grids = [torch.as_tensor(_DeviceMemory(p.value, count, self.np_dtype), device=self.device)
                 for p in (field, source)]
        return MgLevel(lay, grids[0], grids[1])

    # ---------------------------------------------------------------- cycles
    def vcycle(self, pre: int = 2, post: int = 2, coarse_sweeps: int = 8, omegas=DEFAULT_OMEGAS, cycles: int = 1,
               stream=None) -> None:
        """`cycles` V(pre, post) cycles (stencil_mg_vcycle): sweep i of every
        smoothing run is relaxed by omegas[i % len(omegas)]."""
        par, _keep = _params(pre, post, coarse_sweeps, omegas)
        with torch.cuda.device(self.device):
            for _ in range(cycles):
                _lib.check(self.lib.stencil_mg_vcycle(self.mg, ctypes.byref(par), _stream_handle(stream)),
                           "stencil_mg_vcycle", lib=self.lib)

    def fmg(self, cycles: int = 2, pre: int = 2, post: int = 2, coarse_sweeps: int = 8, omegas=DEFAULT_OMEGAS,
            stream=None) -> None:
        """One full multigrid pass (stencil_mg_fmg): the coarsest problem
        solved, then per level upward the cubic prolongation as the starting
        guess and `cycles` V(pre, post) cycles.  The fine field's interior is
        ignored and overwritten; its ghost shell is the Dirichlet data, EDGES
        AND CORNERS INCLUDED (the prolongation reads them)."""
        par, _keep = _params(pre, post, coarse_sweeps, omegas)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.stencil_mg_fmg(self.mg, ctypes.byref(par), cycles, _stream_handle(stream)),
                       "stencil_mg_fmg", lib=self.lib)

    def fmg_plan(self, cycles: int = 2, pre: int = 2, post: int = 2, coarse_sweeps: int = 8,
                 omegas=DEFAULT_OMEGAS) -> dict:
        """One full multigrid pass as kernel launches (stencil_mg_fmg_plan)."""
        return fmg_plan(self.spec, *self.shape, levels=self.levels, cycles=cycles, pre=pre, post=post,
                        coarse_sweeps=coarse_sweeps, omegas=omegas, lib=self.lib)

    def solve(self, tol: float, max_cycles: int, check_every: int = 1, norm: str = "max", pre: int = 2, post: int = 2,
              coarse_sweeps: int = 8, omegas=DEFAULT_OMEGAS, stream=None, timed: bool = False) -> UntilResult:
        """V-cycles until the fine residual's norm is <= tol, checked every
        `check_every` cycles and after the last one, at most `max_cycles`
        (stencil_mg_solve).  `iterations` of the result counts cycles; `grid`
        is level(0).field."""
        par, _keep = _params(pre, post, coarse_sweeps, omegas)
        done, conv = ctypes.c_uint32(0), ctypes.c_int(0)
        last, ms = ctypes.c_double(0.0), ctypes.c_float(0.0)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.stencil_mg_solve(self.mg, ctypes.byref(par), max_cycles, check_every,
                                                 _lib.NORM_NAMES[norm], tol, _stream_handle(stream), ctypes.byref(done),
                                                 ctypes.byref(last), ctypes.byref(conv),
                                                 ctypes.byref(ms) if timed else None), "stencil_mg_solve", lib=self.lib)
        return UntilResult(self.level(0).field, int(done.value), bool(conv.value), float(last.value),
                           ms.value if timed else None)

    def residual_norms(self, begin: int = 0, end: int | None = None, stream=None):
        """Per-plane (max |r|, sum r^2) of the fine residual (stencil_residual_norms)."""
        lay = _lib.Layout()
        field, source = ctypes.c_void_p(), ctypes.c_void_p()
        _lib.check(self.lib.stencil_mg_level(self.mg, 0, ctypes.byref(lay), ctypes.byref(field), ctypes.byref(source)),
                   "stencil_mg_level", lib=self.lib)
        end = self.shape[2] if end is None else end
        with torch.cuda.device(self.device):
            return _residual_norms(self.lib, lay, field, source, begin, end, stream)

    def residual_norm(self, norm: str = "max", stream=None) -> float:
        """The scalar norm of the fine residual: "max" or "l2" (the per-plane
        sums added in ascending order); NaN if any plane is NaN."""
        return _scalar_norm(*self.residual_norms(stream=stream), norm)

    def plan(self, pre: int = 2, post: int = 2, coarse_sweeps: int = 8, omegas=DEFAULT_OMEGAS) -> dict:
        """One cycle as kernel launches (stencil_mg_plan)."""
        return mg_plan(self.spec, *self.shape, levels=self.levels, pre=pre, post=post, coarse_sweeps=coarse_sweeps,
                       omegas=omegas, lib=self.lib)
