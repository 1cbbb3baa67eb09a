"""ctypes binding of libovl.so (the C ABI declared in include/ovl.h).

The library is built in-tree by ``csrc/Makefile`` (``__graft_entry__.build()``)
into ``genome-assembly-using-overlap-graphs_amd/build/libovl.so``.  There is no
CPU fallback: if the library is missing or no GPU is visible the engine
raises ``OvlError`` (the host forms -- ``ovl_remove_cycles`` and the ``*_host`` functions of
``stages.py`` -- need neither a context nor a GPU).  ctypes releases the GIL for the
duration of each call.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
import threading

PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(PKG_ROOT, "build", "libovl.so")
CSRC = os.path.join(PKG_ROOT, "csrc")

ABI_VERSION = 4

OVL_OK = 0
ERRORS = {
    -1: "OVL_E_ARG", -2: "OVL_E_HIP", -3: "OVL_E_OOM", -4: "OVL_E_UNSUPPORTED",
    -5: "OVL_E_RANGE", -6: "OVL_E_STATE", -7: "OVL_E_INDEX", -8: "OVL_E_INTERNAL",
}
KERNELS = {0: "none", 1: "ungapped", 2: "dp", 3: "banded"}
BAND_FORMS = {-1: "none", 0: "strip", 1: "rows", 2: "fast", 3: "diag", 4: "lane"}

# name -> (restype, argtypes); mirrors include/ovl.h exactly
_P = ctypes.c_void_p
_i32 = ctypes.c_int32
_i64 = ctypes.c_int64
_pi32 = ctypes.POINTER(ctypes.c_int32)
_pi64 = ctypes.POINTER(ctypes.c_int64)
_pf64 = ctypes.POINTER(ctypes.c_double)
SIGNATURES = {
    "ovl_version": (ctypes.c_int, []),
    "ovl_device_count": (ctypes.c_int, [_pi32]),
    "ovl_create": (ctypes.c_int, [_i32, ctypes.POINTER(_P)]),
    "ovl_create_on_devices": (ctypes.c_int, [_P, _i32, ctypes.POINTER(_P)]),
    "ovl_ctx_devices": (ctypes.c_int, [_P, _P, _i32, _pi32]),
    "ovl_destroy": (ctypes.c_int, [_P]),
    "ovl_host_alloc": (ctypes.c_int, [_i64, ctypes.POINTER(_P)]),
    "ovl_host_free": (ctypes.c_int, [_P]),
    "ovl_host_register": (ctypes.c_int, [_P, _i64]),
    "ovl_host_unregister": (ctypes.c_int, [_P]),
    "ovl_host_pool": (ctypes.c_int, [_pi32, _pi32, _pi32, _pi32]),
    "ovl_host_pool_rule": (ctypes.c_int32, [_i32, _i32, _i32]),
    "ovl_set_timing": (ctypes.c_int, [_P, _i32]),
    "ovl_last_timing": (ctypes.c_int, [_P, _pf64, _pf64]),
    "ovl_last_launches": (ctypes.c_int, [_P, _i32, _P, _P, _P, _P, _pi32]),
    "ovl_last_transfer": (ctypes.c_int, [_P, _pi64, _pi64]),
    "ovl_last_pair_list": (ctypes.c_int, [_P, _pi64, _pi64]),
    "ovl_last_results": (ctypes.c_int, [_P, _pi64, _pi64, _pi64]),
    "ovl_last_error": (ctypes.c_char_p, [_P]),
    "ovl_score_pairs": (ctypes.c_int, [_P, _P, _P, _i32, _P, _P, _i64, _i32, _i32, _i64, _i32, _P, _P]),
    "ovl_set_reads": (ctypes.c_int, [_P, _P, _P, _i32]),
    "ovl_reads_info": (ctypes.c_int, [_P, _pi32, _pi32, _pi32, _pi64]),
    "ovl_plan": (ctypes.c_int, [_P, _i32, _i32, _i64, _i32, _pi32]),
    "ovl_last_score_form": (ctypes.c_int, [_P] + [_pi32] * 11),
    "ovl_score_host": (ctypes.c_int, [_P, _P, _P, _i64, _i32, _i32, _i64, _i32, _P, _P]),
    "ovl_score_device": (ctypes.c_int, [_P, _P, _P, _i64, _i32, _i32, _i64, _i32, _P, _P, _P]),
    "ovl_check_device_errors": (ctypes.c_int, [_P]),
    "ovl_align_one": (ctypes.c_int, [_P, _i32, _i32, _i32, _i32, _i64, _pi32, _pi32, _P]),
    "ovl_candidates": (ctypes.c_int, [_P, _i32, _pi64]),
    "ovl_seed_candidates": (ctypes.c_int, [_P, _i32, _pi64]),
    "ovl_seed_offsets_copy": (ctypes.c_int, [_P, _P]),
    "ovl_last_seed_timing": (ctypes.c_int, [_P] + [_pf64] * 4),
    "ovl_candidates_copy": (ctypes.c_int, [_P, _P, _P]),
    "ovl_candidates_device": (ctypes.c_int, [_P, ctypes.POINTER(_P), ctypes.POINTER(_P), _pi64]),
    "ovl_score_candidates": (ctypes.c_int, [_P, _i32, _i32, _i64, _i32, _P, _P]),
    "ovl_score_candidates_range": (ctypes.c_int, [_P, _i64, _i64, _i32, _i32, _i64, _i32, _P, _P]),
    "ovl_candidates_shards": (ctypes.c_int, [_P, _i32, _P]),
    "ovl_quiesce": (ctypes.c_int, [_P]),
    "ovl_devices_for": (ctypes.c_int, [_P, _i64, _pi32]),
    "ovl_resident_stats": (ctypes.c_int, [_P, _pi32, _pi64, _pi64, _pi32]),
    "ovl_local_align": (ctypes.c_int, [_P, _P, _i32, _P, _i32, _i32, _i32, _i64, _pi32, _pi32, _pi32, _pi32,
                                       _pi32, _P, _i64, _pi64]),
    "ovl_local_align_batch": (ctypes.c_int, [_P, _P, _P, _i32, _P, _i32, _P, _P, _i32, _i32, _i64, _P, _P, _P, _P,
                                             _P, _P, _P, _P]),
    "ovl_last_local_batch": (ctypes.c_int, [_P, _pi32, _pi32, _pi32]),
    "ovl_remove_cycles": (ctypes.c_int, [_P, _P, _P, _i32, _P, _pi64]),
    "ovl_remove_cycles_stream": (ctypes.c_int, [_P, _P, _P, _i32, _P, _pi64, _P, _P, _P]),
    "ovl_transitive_reduce": (ctypes.c_int, [_P, _P, _P, _P, _i32, _P, _pi64]),
    "ovl_transitive_reduce_host": (ctypes.c_int, [_P, _P, _P, _i32, _P, _pi64]),
    "ovl_last_transitive": (ctypes.c_int, [_P, _pi32, _pi32, _pi64]),
    "ovl_reach_reduce": (ctypes.c_int, [_P, _P, _P, _i32, _P, _pi64, _P]),
    "ovl_reach_reduce_host": (ctypes.c_int, [_P, _P, _i32, _P, _pi64, _P]),
    "ovl_last_reach": (ctypes.c_int, [_P, _pi32, _pi32, _pi32]),
    "ovl_read_best": (ctypes.c_int, [_P, _P, _P, _i32, _P, _P, _i32, _i32, _i32, _i32, _i64, _P, _P, _P, _P, _P, _P,
                                     _P]),
    "ovl_read_best_host": (ctypes.c_int, [_P, _P, _i32, _P, _P, _i32, _i32, _i32, _i32, _i64, _P, _P, _P, _P, _P, _P,
                                          _P]),
    "ovl_last_read_best": (ctypes.c_int, [_P, _pi64, _pi64, _pi32]),
    "ovl_consensus": (ctypes.c_int, [_P, _P, _P, _i32, _P, _P, _i32, _P, _i32, _i32, _i32, _i64, _i32, _P, _P, _pi64,
                                     _pi64, _P]),
    "ovl_consensus_host": (ctypes.c_int, [_P, _P, _i32, _P, _P, _i32, _P, _i32, _i32, _i32, _i64, _i32, _P, _P, _pi64,
                                          _pi64, _P]),
    "ovl_last_consensus": (ctypes.c_int, [_P, _pi64, _pi64, _pi64, _pi32]),
    "ovl_last_consensus_timing": (ctypes.c_int, [_P, _pf64, _pf64, _pf64]),
    "ovl_consensus_placed": (ctypes.c_int, [_P, _P, _P, _i32, _P, _P, _P, _i32, _P, _P, _i32, _i32, _i32, _i64, _i32,
                                            _i32, _i32, _P, _P, _pi64, _pi64, _pi64, _pi32, _P]),
    "ovl_consensus_placed_host": (ctypes.c_int, [_P, _P, _i32, _P, _P, _P, _i32, _P, _P, _i32, _i32, _i32, _i64, _i32,
                                                 _i32, _i32, _P, _P, _pi64, _pi64, _pi64, _pi32, _P]),
    "ovl_last_consensus_placed": (ctypes.c_int, [_P, _pi64, _pi64, _pi64, _pi32, _pi32]),
    "ovl_last_consensus_placed_timing": (ctypes.c_int, [_P, _pf64, _pf64]),
    "ovl_layout_host": (ctypes.c_int, [_P, _P, _i32, _P, _P, _P, _P, _i64, _i32, _i32, _P, _P, _P, _P, _P, _P, _P,
                                       _pi32]),
    "ovl_layout": (ctypes.c_int, [_P, _P, _P, _i32, _P, _P, _P, _P, _i64, _i32, _i32, _P, _P, _P, _P, _P, _P, _P,
                                  _pi32]),
    "ovl_layout_candidates": (ctypes.c_int, [_P, _i32, _i32, _i64, _i32, _i32, _i32, _P, _P, _P, _P, _P, _P, _P,
                                             _pi32]),
    "ovl_last_layout": (ctypes.c_int, [_P, _pi64, _pi64, _pi32, _pi64]),
    "ovl_last_layout_timing": (ctypes.c_int, [_P] + [_pf64] * 4),
    "ovl_kmer_spectrum_host": (ctypes.c_int, [_P, _P, _i32, _i32, _P, _P, _i64, _pi64]),
    "ovl_correct_reads_host": (ctypes.c_int, [_P, _P, _i32, _i32, _i32, _P, _P, _P]),
    "ovl_kmer_spectrum": (ctypes.c_int, [_P, _P, _P, _i32, _i32, _P, _P, _i64, _pi64]),
    "ovl_correct_reads": (ctypes.c_int, [_P, _P, _P, _i32, _i32, _i32, _P, _P, _P]),
    "ovl_last_correct_timing": (ctypes.c_int, [_P] + [_pf64] * 4),
    "ovl_unitigs_host": (ctypes.c_int, [_P, _P, _i32, _P, _i32, _P, _P, _P, _P, _P, _P, _P, _P, _pi32, _pi64, _pi64,
                                        _pi32]),
    "ovl_unitigs": (ctypes.c_int, [_P, _P, _P, _i32, _P, _i32, _P, _P, _P, _P, _P, _P, _P, _P, _pi32, _pi64, _pi64,
                                   _pi32]),
    "ovl_unitigs_candidates": (ctypes.c_int, [_P, _P, _P, _i32, _i32, _i32, _i64, _i32, _P, _P, _P, _P, _pi32, _pi64,
                                              _pi64, _pi32]),
    "ovl_unitigs_edges_copy": (ctypes.c_int, [_P, _P, _P, _P, _P]),
    "ovl_unitigs_walk_host": (ctypes.c_int, [_P, _P, _i32, _P, _P, _pi32, _pi32]),
    "ovl_last_unitigs": (ctypes.c_int, [_P, _pi64, _pi64, _pi32, _pi32]),
    "ovl_last_unitigs_timing": (ctypes.c_int, [_P] + [_pf64] * 4),
}


class OvlError(RuntimeError):
    """A libovl call failed (or the library / GPU is unavailable)."""

    def __init__(self, code: int, msg: str):
        super().__init__(f"{ERRORS.get(code, code)}: {msg}")
        self.code = code


_lock = threading.Lock()
_lib = None


def build(force: bool = False) -> str:
    """Compile libovl.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    if force or not os.path.exists(LIB_PATH):
        subprocess.run(["make", "-s", "-C", CSRC], check=True)
    return LIB_PATH


def _share_torch_hip_runtime() -> None:
    """Load torch's HIP runtime first when torch is installed.

    torch's libc10_hip needs ``libamdhip64.so`` from torch/lib, while libovl needs the
    soname ``libamdhip64.so.7``.  Loaded in that order both resolve to torch's copy; the
    other order maps a second runtime, and the later one sees no GPU.  Only the import
    happens here (no device is touched).
    """
    try:
        import torch  # noqa: F401
    except ImportError:
        pass


def load():
    """Load and type libovl.so; raises OvlError if it is absent.

    OVL_LIB_PATH may point at another build of the same library (the diagnostic
    trace build, build/trace/libovl.so); it is never a CPU implementation.
    """
    global _lib
    with _lock:
        if _lib is None:
            path = os.environ.get("OVL_LIB_PATH") or LIB_PATH
            if not os.path.exists(path):
                raise OvlError(-2, f"{path} not built: run __graft_entry__.build() "
                                   "(make -C genome-assembly-using-overlap-graphs_amd/csrc)")
            _share_torch_hip_runtime()
            lib = ctypes.CDLL(path)
            for name, (res, args) in SIGNATURES.items():
                fn = getattr(lib, name)
                fn.restype = res
                fn.argtypes = args
            v = lib.ovl_version()
            if v != ABI_VERSION:
                raise OvlError(-1, f"libovl ABI {v} != expected {ABI_VERSION}")
            _lib = lib
        return _lib


def last_error(ctx=None) -> str:
    msg = load().ovl_last_error(ctx)
    return msg.decode("utf-8", "replace") if msg else ""


def check(rc: int, ctx=None) -> None:
    if rc != OVL_OK:
        raise OvlError(rc, last_error(ctx))


def _ptr(a) -> ctypes.c_void_p:
    """The data pointer of a numpy array."""
    return ctypes.c_void_p(a.ctypes.data)


def read_out(fn, *head, ctx=None) -> tuple:
    """Call ``fn(*head, &x0, &x1, ...)``, a scalar ``x`` per argument type left in ``fn.argtypes`` (each a POINTER to
    a simple type, as ``SIGNATURES`` spells it), and return the values: ``int`` for c_int32 / c_int64, ``float`` for
    c_double.  Errors are read from ``ctx``."""
    types = fn.argtypes[len(head):]
    if not all(issubclass(t, ctypes._Pointer) and issubclass(t._type_, ctypes._SimpleCData) for t in types):
        raise TypeError(f"{fn.__name__}: the arguments after the first {len(head)} are not all pointers to scalars")
    outs = [t._type_() for t in types]
    check(fn(*head, *[ctypes.byref(x) for x in outs]), ctx)
    return tuple(x.value for x in outs)
