"""ctypes binding of libcolbert_hip.so (include/colbert_hip.h).  There is no CPU fallback: if the
library is missing, or there is no GPU, calls raise -- loudly."""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
# COLBERT_HIP_LIB: another build of the same library (e.g. a parent commit's build, `make SUF=_old`)
LIB_PATH = os.environ.get("COLBERT_HIP_LIB") or os.path.join(CSRC, "libcolbert_hip.so")
HEADER = os.path.normpath(os.path.join(_HERE, "..", "include", "colbert_hip.h"))


class ColBERTError(RuntimeError):
    code = -1


class DimensionMismatch(ColBERTError):
    code = 1


class DomainError(ColBERTError):
    code = 2


class BoundsError(ColBERTError):
    code = 3


class ArgumentError(ColBERTError):
    code = 4


class HipError(ColBERTError):
    code = 10


class Unsupported(ColBERTError):
    code = 11


class OutOfMemory(ColBERTError):
    code = 12


_ERRORS = {c.code: c for c in (DimensionMismatch, DomainError, BoundsError, ArgumentError, HipError,
                               Unsupported, OutOfMemory)}


def build(force: bool = False, jobs: int = 3) -> str:
    """Compile libcolbert_hip.so for gfx950 with hipcc (colbert.jl_amd/csrc/Makefile)."""
    cmd = ["make", "-C", CSRC, f"-j{jobs}"]
    if force:
        cmd.append("-B")
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL)
    return LIB_PATH


def declared_symbols() -> list[str]:
    """Every function name include/colbert_hip.h declares."""
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(clb_[a-z0-9_]+)\s*\(", text)))


class SearchRequest(C.Structure):
    """clb_search_request (include/colbert_hip.h), field for field: what a search call carries besides queries, sizes and outputs."""
    _fields_ = [("struct_bytes", C.c_int64), ("filters", C.POINTER(C.c_void_p)), ("scope", C.c_int), ("pad_short", C.c_int),
                ("grouping", C.c_void_p), ("per_group", C.c_int64), ("group_base", C.c_int64), ("prior", C.c_void_p),
                ("prior_weight", C.c_float), ("list_prior", C.c_void_p), ("after_scores", C.c_void_p), ("after_pids", C.c_void_p),
                ("list_pids", C.c_void_p), ("list_lens", C.c_void_p), ("list_stride", C.c_int64), ("list_scores", C.c_void_p)]


_entries = {}


def request_entry(name: str):
    """One of the four entry points that take a SearchRequest (every search of this package goes through them), resolved once."""
    fn = _entries.get(name)
    if fn is None:
        fn = getattr(lib(), name, None)
        if fn is None:
            raise ColBERTError(f"{LIB_PATH} lacks {name}: a library built before the search request entry points cannot be "
                               "driven by this package (COLBERT_HIP_LIB) -- drive it from its own checkout")
        _entries[name] = fn
    return fn


_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ColBERTError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(there is no CPU fallback)")
        # One HIP runtime per process: PyTorch wheels bundle their own libamdhip64.so.7 (same SONAME as the
        # system one this library links against).  Whichever is loaded first serves both; torch cannot
        # initialise on top of the system copy, so when torch is installed it is imported first.
        if os.environ.get("COLBERT_HIP_NO_TORCH") != "1":
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
        l = C.CDLL(LIB_PATH)
        l.clb_version.restype = C.c_char_p
        l.clb_last_error.restype = C.c_char_p
        l.clb_searcher_device_bytes.restype = C.c_int64
        l.clb_packed_topk_bytes.restype = C.c_int64
        l.clb_comm_unique_id_bytes.restype = C.c_int64
        l.clb_kmeans_shard_block_bytes.restype = C.c_int64
        l.clb_filter_count.restype = C.c_int64
        l.clb_grouping_count.restype = C.c_int64
        l.clb_grouping_count.argtypes = [C.c_void_p]
        l.clb_grouping_create.restype = C.c_int
        l.clb_grouping_create.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_void_p)]
        l.clb_grouping_destroy.argtypes = [C.c_void_p]
        l.clb_search_batch_grouped.restype = C.c_int
        l.clb_search_batch_grouped.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64,
                                               C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                               C.c_void_p]
        l.clb_search_batch_grouped_device_slot.restype = C.c_int
        l.clb_search_batch_grouped_device_slot.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_int64,
                                                           C.c_int64, C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_void_p,
                                                           C.c_void_p, C.c_void_p, C.c_void_p]
        if hasattr(l, "clb_search_batch_grouped_hits"):        # (absent from a COLBERT_HIP_LIB build of an earlier commit)
            l.clb_search_batch_grouped_hits.restype = C.c_int
            l.clb_search_batch_grouped_hits.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64,
                                                        C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_void_p,
                                                        C.c_void_p, C.c_void_p]
            l.clb_search_batch_grouped_hits_device_slot.restype = C.c_int
            l.clb_search_batch_grouped_hits_device_slot.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_int64,
                                                                    C.c_int64, C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_int64,
                                                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        if hasattr(l, "clb_prior_create"):                     # (absent from a COLBERT_HIP_LIB build of an earlier commit)
            l.clb_prior_create.restype = C.c_int
            l.clb_prior_create.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_void_p)]
            l.clb_prior_create_device.restype = C.c_int
            l.clb_prior_create_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_void_p)]
            l.clb_prior_max_abs.restype = C.c_float
            l.clb_prior_max_abs.argtypes = [C.c_void_p]
            l.clb_prior_destroy.restype = C.c_int
            l.clb_prior_destroy.argtypes = [C.c_void_p]
            l.clb_search_batch_prior.restype = C.c_int
            l.clb_search_batch_prior.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64,
                                                 C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_int,
                                                 C.c_void_p, C.c_void_p, C.c_void_p]
            l.clb_search_batch_prior_device_slot.restype = C.c_int
            l.clb_search_batch_prior_device_slot.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_int64,
                                                             C.c_int64, C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_void_p,
                                                             C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        if hasattr(l, "clb_filter_combine"):                   # (absent from a COLBERT_HIP_LIB build of an earlier commit)
            l.clb_filter_combine.restype = C.c_int
            l.clb_filter_combine.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.c_int64, C.POINTER(C.c_void_p)]
            l.clb_filter_create_range.restype = C.c_int
            l.clb_filter_create_range.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_int, C.POINTER(C.c_void_p)]
            l.clb_filter_extend.restype = C.c_int
            l.clb_filter_extend.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
            l.clb_filter_bitmap.restype = C.c_int
            l.clb_filter_bitmap.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        if hasattr(l, "clb_search_batch_after"):               # (absent from a COLBERT_HIP_LIB build of an earlier commit)
            l.clb_search_batch_after.restype = C.c_int
            l.clb_search_batch_after.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64,
                                                 C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_void_p]
            l.clb_search_batch_after_device_slot.restype = C.c_int
            l.clb_search_batch_after_device_slot.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_int64,
                                                             C.c_int64, C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_void_p,
                                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        l.clb_searcher_generation.restype = C.c_int64
        l.clb_searcher_num_docs.restype = C.c_int64
        l.clb_searcher_num_embeddings.restype = C.c_int64
        l.clb_searcher_remove.restype = C.c_int
        l.clb_searcher_remove.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
        l.clb_searcher_update.restype = C.c_int
        l.clb_searcher_update.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                          C.POINTER(C.c_int64)]
        l.clb_searcher_update_device.restype = C.c_int
        l.clb_searcher_update_device.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.POINTER(C.c_int64)]
        l.clb_filter_create_pids_global.restype = C.c_int
        l.clb_filter_create_pids_global.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
        l.clb_search_shard_phase1_filtered_slot.restype = C.c_int
        l.clb_search_shard_phase1_filtered_slot.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64,
                                                            C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_void_p]
        vp, i64_, ci = C.c_void_p, C.c_int64, C.c_int
        l.clb_search_shard_phase1_grouped_slot.restype = ci
        l.clb_search_shard_phase1_grouped_slot.argtypes = [vp, ci, vp, i64_, i64_, i64_, i64_, C.POINTER(vp), ci, vp, i64_, vp, vp, vp]
        l.clb_search_shard_phase2_grouped_slot.restype = ci
        l.clb_search_shard_phase2_grouped_slot.argtypes = [vp, ci, vp, i64_, i64_, i64_, i64_, vp, vp, i64_, vp, i64_, vp, vp, vp,
                                                           vp, vp, vp]
        l.clb_search_result_groups_slot.restype = ci
        l.clb_search_result_groups_slot.argtypes = [vp, ci, vp, i64_, vp, i64_, i64_, vp, vp, vp]
        l.clb_debug_group_tau_device.restype = ci
        l.clb_debug_group_tau_device.argtypes = [vp, vp, i64_, i64_, i64_, vp, vp]
        if hasattr(l, "clb_search_shard_phase1_prior_slot"):   # (absent from a COLBERT_HIP_LIB build of an earlier commit)
            l.clb_search_shard_phase1_prior_slot.restype = ci
            l.clb_search_shard_phase1_prior_slot.argtypes = [vp, ci, vp, i64_, i64_, i64_, i64_, C.POINTER(vp), ci, vp, i64_, vp,
                                                             C.c_float, vp, vp, vp, vp]
            l.clb_search_shard_phase2_prior_slot.restype = ci
            l.clb_search_shard_phase2_prior_slot.argtypes = [vp, ci, vp, i64_, i64_, i64_, i64_, vp, vp, vp, i64_, vp, i64_, vp,
                                                             C.c_float, vp, vp, vp, vp, vp, vp]
            l.clb_debug_prior_tau_device.restype = ci
            l.clb_debug_prior_tau_device.argtypes = [vp, vp, vp, vp, i64_, i64_, i64_, vp, vp]
        if hasattr(l, "clb_search_batch_request"):              # (absent from a COLBERT_HIP_LIB build of an earlier commit: request_entry)
            rq = C.POINTER(SearchRequest)
            l.clb_search_batch_request.restype = ci
            l.clb_search_batch_request.argtypes = [vp, vp, i64_, i64_, i64_, i64_, rq, vp, vp, vp]
            l.clb_search_batch_request_device_slot.restype = ci
            l.clb_search_batch_request_device_slot.argtypes = [vp, ci, vp, i64_, i64_, i64_, i64_, rq, vp, vp, vp, vp]
            l.clb_search_shard_phase1_request_slot.restype = ci
            l.clb_search_shard_phase1_request_slot.argtypes = [vp, ci, vp, i64_, i64_, i64_, i64_, rq, vp, vp, vp, vp]
            l.clb_search_shard_phase2_request_slot.restype = ci
            l.clb_search_shard_phase2_request_slot.argtypes = [vp, ci, vp, i64_, i64_, i64_, i64_, rq, vp, vp, vp, i64_, vp, vp, vp,
                                                               vp, vp, vp]
        if hasattr(l, "clb_search_batch_listed"):               # (absent from a COLBERT_HIP_LIB build of an earlier commit)
            l.clb_search_batch_listed.restype = ci
            l.clb_search_batch_listed.argtypes = [vp, vp, i64_, i64_, i64_, i64_, vp, vp, i64_, vp, vp, vp, vp]
            l.clb_search_batch_listed_device_slot.restype = ci
            l.clb_search_batch_listed_device_slot.argtypes = [vp, ci, vp, i64_, i64_, i64_, i64_, vp, vp, i64_, vp, vp, vp, vp, vp]
        if hasattr(l, "clb_search_batch_listed_prior"):         # (likewise)
            l.clb_search_batch_listed_prior.restype = ci
            l.clb_search_batch_listed_prior.argtypes = [vp, vp, i64_, i64_, i64_, i64_, vp, vp, i64_, vp, C.c_float, vp, vp, vp, vp]
            l.clb_search_batch_listed_prior_device_slot.restype = ci
            l.clb_search_batch_listed_prior_device_slot.argtypes = [vp, ci, vp, i64_, i64_, i64_, i64_, vp, vp, i64_, vp, C.c_float,
                                                                    vp, vp, vp, vp, vp]
        l.clb_merge_topk_grouped_device.restype = ci
        l.clb_merge_topk_grouped_device.argtypes = [ci, vp, vp, vp, i64_, i64_, i64_, vp, vp, vp, vp, vp, vp]
        l.clb_packed_grouped_bytes.restype = i64_
        l.clb_packed_grouped_bytes.argtypes = [i64_, i64_]
        l.clb_merge_topk_grouped_packed_device.restype = ci
        l.clb_merge_topk_grouped_packed_device.argtypes = [ci, vp, i64_, i64_, i64_, vp, vp, vp, vp]
        if hasattr(l, "clb_debug_nearest"):
            l.clb_debug_nearest_scratch_create.restype = ci
            l.clb_debug_nearest_scratch_create.argtypes = [ci, C.POINTER(vp)]
            l.clb_debug_nearest_scratch_destroy.restype = ci
            l.clb_debug_nearest_scratch_destroy.argtypes = [vp]
            l.clb_debug_nearest.restype = ci
            l.clb_debug_nearest.argtypes = [ci, ci, ci, i64_, vp, i64_, vp, i64_, vp, vp, vp, vp, vp, vp]
        _lib = l
    return _lib


def measure_copy_rate(device: int = 0, nbytes: int = 1 << 30, reps: int = 5) -> float:
    """GB/s (read + written) of a device-to-device copy of `nbytes` on `device`, now (clb_measure_copy_rate)."""
    out = C.c_double(0.0)
    check(lib().clb_measure_copy_rate(C.c_int(device), C.c_int64(nbytes), C.c_int(reps), C.byref(out)))
    return float(out.value)


def measure_read_rate(device: int = 0, nbytes: int = 1 << 30, reps: int = 5) -> float:
    """GB/s of a read-only sweep over `nbytes` on `device`, now (clb_measure_read_rate)."""
    out = C.c_double(0.0)
    check(lib().clb_measure_read_rate(C.c_int(device), C.c_int64(nbytes), C.c_int(reps), C.byref(out)))
    return float(out.value)


def check(rc: int) -> None:
    if rc != 0:
        msg = lib().clb_last_error().decode(errors="replace")
        raise _ERRORS.get(rc, ColBERTError)(msg or f"libcolbert_hip error {rc}")


def fptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def colmajor(a, dtype) -> np.ndarray:
    """A numpy array laid out like the Julia Array of the same shape (column-major, dense)."""
    return np.asfortranarray(np.asarray(a, dtype=dtype))


i64 = C.c_int64
