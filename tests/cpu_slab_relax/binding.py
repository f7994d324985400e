"""ctypes binding of tests/cpu_slab_relax/libslab_fake_relax.so -- TEST
INFRASTRUCTURE ONLY.

The library runs csrc/slab_core.hpp's relaxed rounds (stencil_slab_run_relax,
...) beside its source and plain rounds on the CPU fake device of
tests/cpu_slab_source/ extended by a relaxed sweep (fake_relax.cpp).  `load()`
returns an object with the product's stencil_slab_* names, so
stencil_amd.engine.SlabJob(..., lib=load()) drives it unchanged.
stencil_slab_run_until_relax is not here: its check runs kernels only the
product has (as stencil_slab_run_until_source).
"""
from __future__ import annotations

import ctypes
import os

from stencil_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "libslab_fake_relax.so")
# the stencil_slab_* names the library exports as fake_relax_*
PLAIN = ("create2", "create_rank2", "destroy", "info", "fill_initial", "upload", "download", "run", "round_form",
         "round_info")
SOURCE = ("set_source", "run_source", "source_plan", "source_round_form")
RELAX = ("run_relax", "relax_plan", "relax_round_form")
STATS = ("relax_sweeps", "relax_signal_sweeps", "source_sweeps", "source_signal_sweeps", "plain_sweeps", "sends",
         "recvs", "peer_copies", "gated", "gate_violations")

_cached = None


class FakeRelaxLib:
    def __init__(self, cdll: ctypes.CDLL):
        self._cdll = cdll
        sigs = {**_lib.signatures(), **_lib.slab_source_signatures(), **_lib.slab_relax_signatures()}
        for short in PLAIN + SOURCE + RELAX:
            name = "stencil_slab_" + short
            fn = getattr(cdll, "fake_relax_" + short)
            fn.restype, fn.argtypes = sigs[name]
            setattr(self, name, fn)
        res, args = sigs["stencil_slab_unique_id"]
        cdll.fake_slab_unique_id.restype, cdll.fake_slab_unique_id.argtypes = res, args
        self.stencil_slab_unique_id = cdll.fake_slab_unique_id
        cdll.fake_slab_last_error_message.restype = ctypes.c_char_p
        cdll.fake_slab_set_k.argtypes = [ctypes.c_int32]
        cdll.fake_slab_set_signal.argtypes = [ctypes.c_int32]
        cdll.fake_source_set_source_signal.argtypes = [ctypes.c_int32]
        cdll.fake_relax_stats.argtypes = [ctypes.POINTER(ctypes.c_int64), ctypes.c_int32]

    # what _lib.check calls on failure
    def stencil_last_error_message(self):
        return self._cdll.fake_slab_last_error_message()

    @staticmethod
    def stencil_strerror(code):
        return b"fake slab error %d" % code

    # test knobs of the fake device
    def set_k(self, k: int) -> None:
        """Sweeps per round (0: the library's own rule)."""
        self._cdll.fake_slab_set_k(k)

    def set_signal(self, on: bool) -> None:
        self._cdll.fake_slab_set_signal(1 if on else 0)

    def set_source_signal(self, on: bool) -> None:
        """STENCIL_SLAB_SOURCE_SIGNAL of the fake device (source and relaxed rounds alike)."""
        self._cdll.fake_source_set_source_signal(1 if on else 0)

    def stats(self, reset: bool = False) -> dict:
        out = (ctypes.c_int64 * len(STATS))()
        self._cdll.fake_relax_stats(out, 1 if reset else 0)
        return dict(zip(STATS, list(out)))


def available() -> bool:
    return os.path.exists(PATH)


def load() -> FakeRelaxLib:
    global _cached
    if _cached is None:
        if not available():
            raise ImportError(f"{PATH} is missing: run `make` (Makefile target {os.path.relpath(PATH, os.path.dirname(os.path.dirname(HERE)))})")
        _cached = FakeRelaxLib(ctypes.CDLL(PATH))
    return _cached
