"""ctypes binding of the C ABI in include/spmv_abi.h (libspmv_hip.so).

This is the Python-side twin of the cgo/ctypes stub shown in INTEGRATION.md: it declares every
entry point of the header, turns negative status codes into exceptions and wraps the opaque
handles in small classes.  There is no fallback of any kind: if the shared library is missing or
no GPU is visible, loading / context creation raises.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np

_PKG = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ.get("SPMV_HIP_SO") or _PKG / "lib" / "libspmv_hip.so")  # override: A/B against another build

FMT_COO, FMT_CSR, FMT_CSC, FMT_ELL, FMT_DIA, FMT_BSR, FMT_CSR_F32 = 0, 1, 2, 3, 4, 5, 6
CSR_AUTO, CSR_VECTOR, CSR_LDSWIN, CSR_SCALAR, CSR_PANEL, CSR_TWOPHASE, CSR_SEGSCAN, CSR_SPLIT, CSR_ELL = 0, 1, 2, 3, 4, 5, 6, 7, 8
AMG_RESTRICT_FUSED, AMG_RESTRICT_UNFUSED, AMG_PROLONG_FUSED, AMG_PROLONG_UNFUSED = 0, 1, 2, 3  # spmv_amg_transfer_timed
PRECOND_NONE, PRECOND_JACOBI, PRECOND_SYMGS, PRECOND_ILU0, PRECOND_CHEBYSHEV, PRECOND_AMG = 0, 1, 2, 3, 4, 5
PRECOND_FSAI = 6
TRSV_LOWER, TRSV_UPPER, TRSV_UNIT, TRSV_TRANSPOSE = 0, 1, 2, 4  # spmv_trsv_*'s flags
REFINE_CG, REFINE_BICGSTAB = 0, 1  # spmv_refine's inner solver
FSAI_MAX_ROW = 64  # SPMV_FSAI_MAX_ROW: the cap on the pattern columns of a row of G
SPGEMM_AUTO, SPGEMM_ROWS, SPGEMM_SORT = 0, 1, 2  # spmv_spgemm's method
FLAG_DPP_REDUCE, FLAG_XCD_REMAP = 1, 2

_i32p = C.POINTER(C.c_int32)
_i64p = C.POINTER(C.c_int64)
_f64p = C.POINTER(C.c_double)
_vp = C.c_void_p


class MatInfo(C.Structure):
    _fields_ = [
        ("format", C.c_int32),
        ("nrow", C.c_int32),
        ("ncol", C.c_int32),
        ("ell_k", C.c_int32),
        ("nnz", C.c_int64),
        ("row_begin", C.c_int64),
        ("max_row_nnz", C.c_int32),
        ("kernel", C.c_int32),
        ("lanes_per_row", C.c_int32),
        ("sorted_rows", C.c_int32),
        ("device_bytes", C.c_int64),
    ]


# name -> (restype, argtypes).  Kept in one table so tests can check it against the header.
SIGNATURES = {
    "spmv_abi_version": (C.c_int, []),
    "spmv_last_error": (C.c_char_p, []),
    "spmv_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "spmv_ctx_create": (C.c_int, [C.c_int, C.POINTER(_vp)]),
    "spmv_ctx_create_on_stream": (C.c_int, [C.c_int, _vp, C.POINTER(_vp)]),
    "spmv_ctx_destroy": (C.c_int, [_vp]),
    "spmv_sync": (C.c_int, [_vp]),
    "spmv_ctx_mem_info": (C.c_int, [_vp, _i64p, _i64p]),
    "spmv_ctx_device": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "spmv_ctx_get_param": (C.c_int, [_vp, C.c_char_p, _i64p]),
    "spmv_vec_create": (C.c_int, [_vp, C.c_int64, C.POINTER(_vp)]),
    "spmv_vec_wrap_device": (C.c_int, [_vp, C.c_int64, _vp, C.POINTER(_vp)]),
    "spmv_vec_destroy": (C.c_int, [_vp]),
    "spmv_vec_size": (C.c_int, [_vp, _i64p]),
    "spmv_vec_device_ptr": (C.c_int, [_vp, C.POINTER(_vp)]),
    "spmv_vec_upload": (C.c_int, [_vp, C.c_int64, C.c_int64, _vp]),
    "spmv_vec_download": (C.c_int, [_vp, C.c_int64, C.c_int64, _vp]),
    "spmv_vec_fill": (C.c_int, [_vp, C.c_double]),
    "spmv_vec_copy": (C.c_int, [_vp, C.c_int64, _vp, C.c_int64, C.c_int64]),
    "spmv_comm_create": (C.c_int, [C.POINTER(_vp), C.c_int32, C.POINTER(_vp)]),
    "spmv_comm_destroy": (None, [_vp]),
    "spmv_comm_backend": (C.c_char_p, [_vp]),
    "spmv_comm_allgather": (C.c_int, [_vp, C.POINTER(_vp), _i64p]),
    "spmv_csr_upload": (C.c_int, [_vp, C.c_int32, C.c_int32, _vp, _vp, _vp, C.POINTER(_vp)]),
    "spmv_csr_wrap_device": (C.c_int, [_vp, C.c_int32, C.c_int32, _vp, _vp, _vp, C.POINTER(_vp)]),
    "spmv_csr_upload_shard": (C.c_int, [_vp, C.c_int64, C.c_int64, C.c_int32, _vp, _vp, _vp, C.POINTER(_vp)]),
    "spmv_coo_upload": (C.c_int, [_vp, C.c_int32, C.c_int32, C.c_int64, _vp, _vp, _vp, C.POINTER(_vp)]),
    "spmv_coo_wrap_device": (C.c_int, [_vp, C.c_int32, C.c_int32, C.c_int64, _vp, _vp, _vp, C.POINTER(_vp)]),
    "spmv_ell_upload": (C.c_int, [_vp, C.c_int32, C.c_int32, C.c_int32, C.c_int64, _vp, _vp, C.POINTER(_vp)]),
    "spmv_ell_wrap_device": (C.c_int, [_vp, C.c_int32, C.c_int32, C.c_int32, C.c_int64, _vp, _vp, C.POINTER(_vp)]),
    "spmv_csc_upload": (C.c_int, [_vp, C.c_int32, C.c_int32, _vp, _vp, _vp, C.POINTER(_vp)]),
    "spmv_dia_upload": (C.c_int, [_vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, C.POINTER(_vp)]),
    "spmv_mat_destroy": (C.c_int, [_vp]),
    "spmv_mat_get_info": (C.c_int, [_vp, C.POINTER(MatInfo)]),
    "spmv_mat_validate": (C.c_int, [_vp]),
    "spmv_mat_set_kernel": (C.c_int, [_vp, C.c_int32, C.c_int32]),
    "spmv_mat_set_flags": (C.c_int, [_vp, C.c_uint32]),
    "spmv_mat_set_param": (C.c_int, [_vp, C.c_char_p, C.c_int64]),
    "spmv_mat_get_param": (C.c_int, [_vp, C.c_char_p, _i64p]),
    "spmv_mat_get_plan": (C.c_int, [_vp, _vp, _i64p]),
    "spmv_mat_set_plan": (C.c_int, [_vp, _vp, C.c_int64]),
    "spmv_ctx_set_plan": (C.c_int, [_vp, _vp, C.c_int64]),
    "spmv_plan_check": (C.c_int, [_vp, C.c_int64, _i32p, _i32p, _i32p]),
    "spmv_mat_download": (C.c_int, [_vp, _vp, _vp, _vp]),
    "spmv_mat_device_ptrs": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]),
    "spmv_apply": (C.c_int, [_vp, _vp, _vp, _vp]),
    "spmv_apply_timed": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int32, _f64p]),
    "spmv_apply_multi": (C.c_int, [_vp, _vp, C.c_int32, _vp, _vp, C.c_int32]),
    "spmv_apply_multi_timed": (C.c_int, [_vp, _vp, C.c_int32, _vp, _vp, C.c_int32, C.c_int32, _f64p]),
    "spmv_sddmm": (C.c_int, [_vp, _vp, C.c_int32, C.c_double, _vp, _vp, C.c_double, _vp]),
    "spmv_sddmm_timed": (C.c_int, [_vp, _vp, C.c_int32, C.c_double, _vp, _vp, C.c_double, _vp, C.c_int32, _f64p]),
    "spmv_csr_with_values": (C.c_int, [_vp, _vp, _vp, C.POINTER(_vp)]),
    "spmv_apply_transpose": (C.c_int, [_vp, _vp, _vp, _vp]),
    "spmv_apply_transpose_timed": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int32, _f64p]),
    "spmv_mat_transpose_setup": (C.c_int, [_vp]),
    "spmv_dot": (C.c_int, [_vp, _vp, _vp, _f64p]),
    "spmv_axpby": (C.c_int, [_vp, C.c_double, _vp, C.c_double, _vp, _vp]),
    "spmv_apply_dot": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int32, _vp, _f64p]),
    "spmv_cg_multi": (C.c_int, [_vp, _vp, C.c_int32, _vp, _vp, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.POINTER(C.c_int32), _f64p]),
    "spmv_cg": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.POINTER(C.c_int32), _f64p]),
    "spmv_cgls": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int32, C.c_double, C.c_int32, C.c_double, C.POINTER(C.c_int32), _f64p, _f64p]),
    "spmv_bicgstab": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.POINTER(C.c_int32), _f64p]),
    "spmv_gmres": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.POINTER(C.c_int32), _f64p]),
    "spmv_minres": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_double, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.POINTER(C.c_int32), _f64p]),
    "spmv_block_gram": (C.c_int, [_vp, C.c_int64, C.c_int32, _vp, C.c_int64, C.c_int32, _vp, C.c_int64, _f64p]),
    "spmv_block_combine": (C.c_int, [_vp, C.c_int64, C.c_int32, _vp, C.c_int64, C.c_int32, _f64p, _vp, C.c_int64]),
    "spmv_lobpcg": (C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, C.c_int32, C.c_double, C.c_int32, _f64p, _f64p, C.POINTER(C.c_int32)]),
    "spmv_symgs": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int32]),
    "spmv_symgs_setup": (C.c_int, [_vp, _vp]),
    "spmv_symgs_order": (C.c_int, [_vp, _vp, _i32p]),
    "spmv_ilu0_setup": (C.c_int, [_vp, _vp]),
    "spmv_ilu0_solve": (C.c_int, [_vp, _vp, _vp, _vp]),
    "spmv_ilu0_factors": (C.c_int, [_vp, _vp, _f64p]),
    "spmv_ilu0_order": (C.c_int, [_vp, _vp, _i32p]),
    "spmv_trsv_setup": (C.c_int, [_vp, _vp, C.c_uint32]),
    "spmv_trsv_solve": (C.c_int, [_vp, _vp, C.c_uint32, _vp, _vp]),
    "spmv_trsv_solve_multi": (C.c_int, [_vp, _vp, C.c_uint32, C.c_int32, _vp, _vp]),
    "spmv_trsv_info": (C.c_int, [_vp, C.c_uint32, _i32p, _i32p, _i32p, _i64p]),
    "spmv_chebyshev_coefficients": (C.c_int, [C.c_int32, C.c_double, C.c_double, _f64p, _f64p, _f64p]),
    "spmv_lanczos": (C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_uint64, _f64p, _f64p, _f64p, _f64p, _i32p]),
    "spmv_chebyshev_setup": (C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_double, C.c_double]),
    "spmv_chebyshev_info": (C.c_int, [_vp, _i32p, _i32p, _f64p, _f64p]),
    "spmv_chebyshev_solve": (C.c_int, [_vp, _vp, _vp, _vp]),
    "spmv_chebyshev": (C.c_int, [_vp, _vp, _vp, _vp]),
    "spmv_amg_setup": (C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double]),
    "spmv_amg_info": (C.c_int, [_vp, _i32p, _i64p, _i64p]),
    "spmv_amg_level": (C.c_int, [_vp, _vp, C.c_int32, _i32p, _i32p, _i32p, _f64p]),
    "spmv_amg_solve": (C.c_int, [_vp, _vp, _vp, _vp]),
    "spmv_amg_setup_smoothed": (C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double]),
    "spmv_amg_prolongator": (C.c_int, [_vp, _vp, C.c_int32, _i64p, _i32p, _i32p, _f64p]),
    "spmv_amg_transfer_timed": (C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, C.c_int32, _f64p]),
    "spmv_fsai_setup": (C.c_int, [_vp, _vp, C.c_int32]),
    "spmv_fsai_solve": (C.c_int, [_vp, _vp, _vp, _vp]),
    "spmv_fsai_info": (C.c_int, [_vp, _i32p, _i64p, _i32p]),
    "spmv_fsai_factor": (C.c_int, [_vp, _vp, _i64p, _i32p, _i32p, _f64p]),
    "spmv_spgemm": (C.c_int, [_vp, _vp, _vp, C.c_int32, C.POINTER(_vp)]),
    "spmv_csr_transpose": (C.c_int, [_vp, _vp, C.POINTER(_vp)]),
    "spmv_perm_create": (C.c_int, [_vp, C.c_int64, _i32p, C.POINTER(_vp)]),
    "spmv_perm_rcm": (C.c_int, [_vp, _vp, C.POINTER(_vp)]),
    "spmv_perm_download": (C.c_int, [_vp, _i32p, _i32p]),
    "spmv_perm_info": (C.c_int, [_vp, C.c_char_p, _i64p]),
    "spmv_perm_destroy": (C.c_int, [_vp]),
    "spmv_csr_permute": (C.c_int, [_vp, _vp, _vp, _vp, C.POINTER(_vp)]),
    "spmv_vec_permute": (C.c_int, [_vp, _vp, C.c_int32, _vp, _vp]),
    "spmv_csr_bandwidth": (C.c_int, [_vp, _vp, _i64p, _i64p]),
    "spmv_coo_to_csr": (C.c_int, [_vp, _vp, C.POINTER(_vp)]),
    "spmv_coo_to_ell": (C.c_int, [_vp, _vp, C.POINTER(_vp)]),
    "spmv_csr_to_ell": (C.c_int, [_vp, _vp, C.POINTER(_vp)]),
    "spmv_bsr_upload": (C.c_int, [_vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, C.POINTER(_vp)]),
    "spmv_bsr_wrap_device": (C.c_int, [_vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, C.POINTER(_vp)]),
    "spmv_csr_to_bsr": (C.c_int, [_vp, _vp, C.c_int32, C.POINTER(_vp)]),
    "spmv_bsr_to_csr": (C.c_int, [_vp, _vp, C.c_int32, C.POINTER(_vp)]),
    "spmv_csr_to_f32": (C.c_int, [_vp, _vp, C.POINTER(_vp)]),
    "spmv_csr_f32_upload": (C.c_int, [_vp, C.c_int32, C.c_int32, _vp, _vp, _vp, C.POINTER(_vp)]),
    "spmv_f32_to_csr": (C.c_int, [_vp, _vp, C.POINTER(_vp)]),
    "spmv_f32_info": (C.c_int, [_vp, _i64p, _i64p, _f64p]),
    "spmv_refine": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double,
                              C.POINTER(C.c_int32), C.POINTER(C.c_int32), _f64p]),
    "spmv_csr_split_columns": (C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.POINTER(_vp), C.POINTER(_vp)]),
    "spmv_partition_rows": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, _i64p, _i64p]),
    "spmv_partition_rows_balanced": (C.c_int, [C.c_int64, _vp, C.c_int32, _vp]),
    "spmv_gen_csr_uniform": (C.c_int, [_vp, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.POINTER(_vp)]),
    "spmv_gen_ell_banded": (C.c_int, [_vp, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.POINTER(_vp)]),
    "spmv_gen_dia_banded": (C.c_int, [_vp, C.c_int32, C.c_int32, C.c_uint64, C.POINTER(_vp)]),
    "spmv_gen_coo_powerlaw": (C.c_int, [_vp, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.POINTER(_vp)]),
    "spmv_gen_coo_powerlaw_sorted": (C.c_int, [_vp, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.POINTER(_vp)]),
    "spmv_mat_partition_rows": (C.c_int, [_vp, C.c_int32, C.c_int32, _vp]),
    "spmv_ctx_xcd_round_robin": (C.c_int, [_vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "spmv_apply_host": (C.c_int, [_vp, _vp, _vp, _vp]),
    "spmv_csr_extract_rows": (C.c_int, [_vp, _vp, C.c_int64, C.c_int64, C.POINTER(_vp)]),
    "spmv_gen_vec_uniform": (C.c_int, [_vp, _vp, C.c_int64, C.c_uint64]),
}


class SpmvError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"libspmv_hip status {code}: {message}")
        self.code = code


_lib = None


def load(path: os.PathLike | None = None) -> C.CDLL:
    """Load libspmv_hip.so (once) and declare every prototype.  Raises if the library is absent."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = Path(path) if path else LIB_PATH
    if not p.exists():
        raise FileNotFoundError(
            f"{p} not found: build the HIP engine first (make engine, or __graft_entry__.build()). "
            "There is no CPU fallback."
        )
    lib = C.CDLL(str(p))
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the library does not export the symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _check(rc: int) -> None:
    if rc != 0:
        raise SpmvError(rc, load().spmv_last_error().decode("utf-8", "replace"))


def _host(a, dtype) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=dtype)


def _ptr(a) -> int | None:
    """address of a numpy array / torch tensor / raw int; None passes NULL"""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data
    if hasattr(a, "data_ptr"):
        return a.data_ptr()
    return int(a)


def device_count() -> int:
    n = C.c_int(0)
    rc = load().spmv_device_count(C.byref(n))
    return n.value if rc == 0 else 0


def plan_check(plan: bytes) -> tuple[int, int, int]:
    """(root format, root kernel, number of nodes) of a plan blob, or SpmvError with the reason; needs no device (spmv_plan_check)"""
    f, k, n = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    _check(load().spmv_plan_check(plan, len(plan), C.byref(f), C.byref(k), C.byref(n)))
    return f.value, k.value, n.value


def chebyshev_coefficients(degree: int, lmin: float, lmax: float) -> tuple[float, np.ndarray, np.ndarray]:
    """(c0, c1[degree], c2[degree]) of the Chebyshev polynomial on [lmin, lmax] as the engine computes them on the host
    (spmv_chebyshev_coefficients); needs no device"""
    c0, c1, c2 = C.c_double(0.0), np.zeros(max(int(degree), 1)), np.zeros(max(int(degree), 1))
    _check(load().spmv_chebyshev_coefficients(degree, lmin, lmax, C.byref(c0), c1.ctypes.data_as(_f64p), c2.ctypes.data_as(_f64p)))
    return c0.value, c1[:degree], c2[:degree]


def partition_rows(nrow: int, nparts: int, part: int) -> tuple[int, int]:
    """Equal rows per part, last part takes the remainder (reference src/mat_vec.cpp:233,245-246)."""
    b, e = C.c_int64(), C.c_int64()
    _check(load().spmv_partition_rows(nrow, nparts, part, C.byref(b), C.byref(e)))
    return b.value, e.value


def partition_rows_balanced(row_ptr64, nparts: int) -> np.ndarray:
    rp = _host(row_ptr64, np.int64)
    bounds = np.zeros(nparts + 1, dtype=np.int64)
    _check(load().spmv_partition_rows_balanced(len(rp) - 1, rp.ctypes.data, nparts, bounds.ctypes.data))
    return bounds


class Context:
    """One HIP device + one stream (spmv_ctx)."""

    def __init__(self, device: int = 0, stream: int | None = None):
        self._lib = load()
        h = _vp()
        if stream is None:
            _check(self._lib.spmv_ctx_create(device, C.byref(h)))
        else:
            _check(self._lib.spmv_ctx_create_on_stream(device, _vp(stream), C.byref(h)))
        self.h = h
        self.device = device

    def close(self):
        if getattr(self, "h", None):
            self._lib.spmv_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        _check(self._lib.spmv_sync(self.h))

    def apply_host(self, A: "Matrix", x_host: np.ndarray, y_host: np.ndarray) -> None:
        """y_host += A * x_host with HOST arrays (float64, contiguous), synchronous: the reference's call shape in one entry point"""
        if x_host.dtype != np.float64 or y_host.dtype != np.float64 or not x_host.flags.c_contiguous or not y_host.flags.c_contiguous:
            raise ValueError("apply_host: float64 contiguous arrays")
        i = A.info
        if x_host.size != i.ncol or y_host.size != i.nrow:
            raise ValueError(f"apply_host: x has {x_host.size} entries (ncol {i.ncol}), y {y_host.size} (nrow {i.nrow})")
        _check(self._lib.spmv_apply_host(self.h, A.h, x_host.ctypes.data, y_host.ctypes.data))

    def get_param(self, name: str) -> int:
        """what the context found out about its platform (spmv_ctx_get_param): "host_stores", "xcd_round_robin", ..."""
        v = C.c_int64(0)
        _check(self._lib.spmv_ctx_get_param(self.h, name.encode(), C.byref(v)))
        return v.value

    def set_plan(self, plan: bytes | None) -> None:
        """handles of the plan's format created on this context from now on take `plan` instead of selecting; None clears it"""
        if plan is None:
            _check(self._lib.spmv_ctx_set_plan(self.h, None, 0))
        else:
            _check(self._lib.spmv_ctx_set_plan(self.h, plan, len(plan)))

    def xcd_round_robin(self) -> tuple[int, int]:
        """(1 / 0 / -1, distinct XCD ids seen): the start-up probe of workgroup placement (spmv_ctx_xcd_round_robin)"""
        rr, seen = C.c_int32(0), C.c_int32(0)
        _check(self._lib.spmv_ctx_xcd_round_robin(self.h, C.byref(rr), C.byref(seen)))
        return rr.value, seen.value

    # ---- vectors
    def vector(self, n: int) -> "Vector":
        h = _vp()
        _check(self._lib.spmv_vec_create(self.h, n, C.byref(h)))
        return Vector(self, h, n)

    def vector_from(self, host) -> "Vector":
        a = _host(host, np.float64)
        v = self.vector(a.size)
        v.upload(a)
        return v

    def wrap_vector(self, dev, n: int | None = None) -> "Vector":
        """borrow device memory (torch tensor or raw pointer)"""
        if n is None:
            n = dev.numel()
        h = _vp()
        _check(self._lib.spmv_vec_wrap_device(self.h, n, _vp(_ptr(dev)), C.byref(h)))
        v = Vector(self, h, n)
        v._keep = dev
        return v

    # ---- matrices from host arrays
    def csr(self, nrow, ncol, row_ptr, col, val) -> "Matrix":
        rp, c, v = _host(row_ptr, np.int32), _host(col, np.int32), _host(val, np.float64)
        h = _vp()
        _check(self._lib.spmv_csr_upload(self.h, nrow, ncol, _ptr(rp), _ptr(c), _ptr(v), C.byref(h)))
        return Matrix(self, h)

    def csr_shard(self, row_begin, row_end, ncol, row_ptr64, col, val) -> "Matrix":
        rp, c, v = _host(row_ptr64, np.int64), _host(col, np.int32), _host(val, np.float64)
        h = _vp()
        _check(self._lib.spmv_csr_upload_shard(self.h, row_begin, row_end, ncol, _ptr(rp), _ptr(c), _ptr(v), C.byref(h)))
        return Matrix(self, h)

    def coo(self, nrow, ncol, row, col, val) -> "Matrix":
        r, c, v = _host(row, np.int32), _host(col, np.int32), _host(val, np.float64)
        h = _vp()
        _check(self._lib.spmv_coo_upload(self.h, nrow, ncol, r.size, _ptr(r), _ptr(c), _ptr(v), C.byref(h)))
        return Matrix(self, h)

    def ell(self, nrow, ncol, k, nnz, col, val) -> "Matrix":
        c, v = _host(col, np.int32), _host(val, np.float64)
        h = _vp()
        _check(self._lib.spmv_ell_upload(self.h, nrow, ncol, k, nnz, _ptr(c), _ptr(v), C.byref(h)))
        return Matrix(self, h)

    def bsr(self, nrow, ncol, bs, brow_ptr, bcol, val) -> "Matrix":
        """block CSR (spmv_bsr_upload): blocks of bs x bs values, row-major inside a block; nrow, ncol are scalar dimensions"""
        rp, c, v = _host(brow_ptr, np.int32), _host(bcol, np.int32), _host(val, np.float64)
        h = _vp()
        _check(self._lib.spmv_bsr_upload(self.h, nrow, ncol, bs, _ptr(rp), _ptr(c), _ptr(v), C.byref(h)))
        return Matrix(self, h)

    def csr_f32(self, nrow, ncol, row_ptr, col, val) -> "Matrix":
        """CSR with single-precision value storage (spmv_csr_f32_upload): val is taken as float32; packed on the device"""
        rp, c, v = _host(row_ptr, np.int32), _host(col, np.int32), _host(val, np.float32)
        h = _vp()
        _check(self._lib.spmv_csr_f32_upload(self.h, nrow, ncol, _ptr(rp), _ptr(c), _ptr(v), C.byref(h)))
        return Matrix(self, h)

    def csc(self, nrow, ncol, col_ptr, row, val) -> "Matrix":
        cp, r, v = _host(col_ptr, np.int32), _host(row, np.int32), _host(val, np.float64)
        h = _vp()
        _check(self._lib.spmv_csc_upload(self.h, nrow, ncol, _ptr(cp), _ptr(r), _ptr(v), C.byref(h)))
        return Matrix(self, h)

    def dia(self, nrow, ncol, offsets, val) -> "Matrix":
        o, v = _host(offsets, np.int32), _host(val, np.float64)
        h = _vp()
        _check(self._lib.spmv_dia_upload(self.h, nrow, ncol, o.size, _ptr(o), _ptr(v), C.byref(h)))
        return Matrix(self, h)

    # ---- matrices borrowing device memory
    def wrap_csr(self, nrow, ncol, d_row_ptr, d_col, d_val) -> "Matrix":
        h = _vp()
        _check(self._lib.spmv_csr_wrap_device(self.h, nrow, ncol, _ptr(d_row_ptr), _ptr(d_col), _ptr(d_val), C.byref(h)))
        m = Matrix(self, h)
        m._keep = (d_row_ptr, d_col, d_val)
        return m

    def wrap_bsr(self, nrow, ncol, bs, d_brow_ptr, d_bcol, d_val) -> "Matrix":
        h = _vp()
        _check(self._lib.spmv_bsr_wrap_device(self.h, nrow, ncol, bs, _ptr(d_brow_ptr), _ptr(d_bcol), _ptr(d_val), C.byref(h)))
        m = Matrix(self, h)
        m._keep = (d_brow_ptr, d_bcol, d_val)
        return m

    def wrap_coo(self, nrow, ncol, nnz, d_row, d_col, d_val) -> "Matrix":
        h = _vp()
        _check(self._lib.spmv_coo_wrap_device(self.h, nrow, ncol, nnz, _ptr(d_row), _ptr(d_col), _ptr(d_val), C.byref(h)))
        m = Matrix(self, h)
        m._keep = (d_row, d_col, d_val)
        return m

    def wrap_ell(self, nrow, ncol, k, nnz, d_col, d_val) -> "Matrix":
        h = _vp()
        _check(self._lib.spmv_ell_wrap_device(self.h, nrow, ncol, k, nnz, _ptr(d_col), _ptr(d_val), C.byref(h)))
        m = Matrix(self, h)
        m._keep = (d_col, d_val)
        return m

    # ---- generators
    def gen_csr_uniform(self, row_begin, row_end, ncol, k, band=0, seed=1) -> "Matrix":
        h = _vp()
        _check(self._lib.spmv_gen_csr_uniform(self.h, row_begin, row_end, ncol, k, band, seed, C.byref(h)))
        return Matrix(self, h)

    def gen_ell_banded(self, nrow, ncol, k, seed=1) -> "Matrix":
        h = _vp()
        _check(self._lib.spmv_gen_ell_banded(self.h, nrow, ncol, k, seed, C.byref(h)))
        return Matrix(self, h)

    def gen_dia_banded(self, nrow, k, seed=1) -> "Matrix":
        h = _vp()
        _check(self._lib.spmv_gen_dia_banded(self.h, nrow, k, seed, C.byref(h)))
        return Matrix(self, h)

    def gen_coo_powerlaw(self, nrow, ncol, max_len=4096, seed=1, sorted_by_length=False) -> "Matrix":
        """row-sorted COO with power-law row lengths; sorted_by_length: the lengths at the distribution's quantiles, longest first"""
        h = _vp()
        fn = self._lib.spmv_gen_coo_powerlaw_sorted if sorted_by_length else self._lib.spmv_gen_coo_powerlaw
        _check(fn(self.h, nrow, ncol, max_len, seed, C.byref(h)))
        return Matrix(self, h)

    def extract_rows(self, csr: "Matrix", row_begin: int, row_end: int) -> "Matrix":
        """rows [row_begin, row_end) of a device-resident CSR handle (of any context) as a shard on THIS context"""
        h = _vp()
        _check(self._lib.spmv_csr_extract_rows(self.h, csr.h, row_begin, row_end, C.byref(h)))
        return Matrix(self, h)

    def gen_vector(self, n, index_offset=0, seed=1) -> "Vector":
        v = self.vector(n)
        _check(self._lib.spmv_gen_vec_uniform(self.h, v.h, index_offset, seed))
        return v

    # ---- ops
    def apply(self, A: "Matrix", x: "Vector", y: "Vector") -> None:
        """y += A*x, asynchronous on the context's stream"""
        _check(self._lib.spmv_apply(self.h, A.h, x.h, y.h))

    def apply_timed(self, A: "Matrix", x: "Vector", y: "Vector", reps: int) -> float:
        ms = C.c_double(0.0)
        _check(self._lib.spmv_apply_timed(self.h, A.h, x.h, y.h, reps, C.byref(ms)))
        return ms.value

    def apply_multi(self, A: "Matrix", X: "Vector", Y: "Vector", k: int, overwrite: bool = False) -> None:
        """Y += A*X (Y = A*X with overwrite) for k vectors at once, asynchronous.  X and Y are row-major (ncol, k) and (nrow, k):
        Vectors of ncol*k and nrow*k entries, e.g. wrap_vector of C-contiguous torch tensors.  CSR and ELL handles; column c of Y
        is bit-identical to the oracle's fma flavour on column c of X"""
        _check(self._lib.spmv_apply_multi(self.h, A.h, k, X.h, Y.h, 1 if overwrite else 0))

    def apply_multi_timed(self, A: "Matrix", X: "Vector", Y: "Vector", k: int, reps: int, overwrite: bool = False) -> float:
        """`reps` back-to-back apply_multi between two device events; mean milliseconds per product"""
        ms = C.c_double(0.0)
        _check(self._lib.spmv_apply_multi_timed(self.h, A.h, k, X.h, Y.h, 1 if overwrite else 0, reps, C.byref(ms)))
        return ms.value

    def sddmm(self, A: "Matrix", U: "Vector", V: "Vector", k: int, out: "Vector", alpha: float = 1.0, beta: float = 0.0) -> None:
        """out[e] = alpha * U[row(e), :] . V[col(e), :] + beta * out[e] for every stored entry e of the CSR handle A (spmv_sddmm),
        asynchronous.  A gives the pattern only; U and V are row-major (nrow, k) and (ncol, k) as apply_multi's, out has nnz entries
        in A's entry order.  beta = 0: out is not read"""
        _check(self._lib.spmv_sddmm(self.h, A.h, k, alpha, U.h, V.h, beta, out.h))

    def sddmm_timed(self, A: "Matrix", U: "Vector", V: "Vector", k: int, out: "Vector", reps: int, alpha: float = 1.0, beta: float = 0.0) -> float:
        """`reps` back-to-back sddmm between two device events; mean milliseconds per call"""
        ms = C.c_double(0.0)
        _check(self._lib.spmv_sddmm_timed(self.h, A.h, k, alpha, U.h, V.h, beta, out.h, reps, C.byref(ms)))
        return ms.value

    def csr_with_values(self, A: "Matrix", values: "Vector") -> "Matrix":
        """a CSR handle over A's row_ptr / col_ind and `values`' storage (spmv_csr_with_values): nothing is copied, A and the vector
        are kept alive by the new handle's Python object"""
        h = _vp()
        _check(self._lib.spmv_csr_with_values(self.h, A.h, values.h, C.byref(h)))
        m = Matrix(self, h)
        m._keep = (A, values)
        return m

    def apply_transpose(self, A: "Matrix", x: "Vector", y: "Vector") -> None:
        """y += A^T x, asynchronous: x has nrow entries (a shard: its rows), y ncol.  The first call builds the handle's transposed
        state (Matrix.transpose_setup); the forward state, its kernel and its plan stay as they were"""
        _check(self._lib.spmv_apply_transpose(self.h, A.h, x.h, y.h))

    def apply_transpose_timed(self, A: "Matrix", x: "Vector", y: "Vector", reps: int) -> float:
        """`reps` back-to-back apply_transpose between two device events (set-up, if due, before them); mean milliseconds"""
        ms = C.c_double(0.0)
        _check(self._lib.spmv_apply_transpose_timed(self.h, A.h, x.h, y.h, reps, C.byref(ms)))
        return ms.value

    def dot(self, x: "Vector", y: "Vector") -> float:
        r = C.c_double(0.0)
        _check(self._lib.spmv_dot(self.h, x.h, y.h, C.byref(r)))
        return r.value

    def axpby(self, alpha: float, x: "Vector", beta: float, y: "Vector", w: "Vector") -> None:
        _check(self._lib.spmv_axpby(self.h, alpha, x.h, beta, y.h, w.h))

    def mem_info(self) -> tuple[int, int]:
        """(free, total) device memory in bytes"""
        f, t = C.c_int64(0), C.c_int64(0)
        _check(self._lib.spmv_ctx_mem_info(self.h, C.byref(f), C.byref(t)))
        return f.value, t.value

    def apply_dot(self, A: "Matrix", x: "Vector", y: "Vector", w: "Vector", overwrite: bool = False) -> float:
        """y = A*x (overwrite) or y += A*x; returns w . y of the updated y (fused into the product where possible)"""
        d = C.c_double(0.0)
        _check(self._lib.spmv_apply_dot(self.h, A.h, x.h, y.h, 1 if overwrite else 0, w.h, C.byref(d)))
        return d.value

    def symgs(self, A: "Matrix", b: "Vector", x: "Vector", sweeps: int = 1) -> None:
        """`sweeps` symmetric Gauss-Seidel sweeps on A x = b, x updated in place (CSR handle holding the whole square
        matrix; the first call analyses it).  Sweep order: A.set_param("symgs_order", 1 multicolour (default) | 0 rows)"""
        _check(self._lib.spmv_symgs(self.h, A.h, b.h, x.h, sweeps))

    def symgs_order(self, A: "Matrix"):
        """sets the handle up if need be and returns order[k] = the k-th row of a forward sweep"""
        _check(self._lib.spmv_symgs_setup(self.h, A.h))
        out = np.zeros(A.info.nrow, dtype=np.int32)
        _check(self._lib.spmv_symgs_order(self.h, A.h, out.ctypes.data_as(_i32p)))
        return out

    def ilu0_setup(self, A: "Matrix") -> None:
        """ILU(0) of a CSR handle holding the whole square matrix, on the device: order, symbolic and numeric set-up (synchronous,
        idempotent).  Sweep order: A.set_param("ilu0_order", 1 multicolour (default) | 0 rows)"""
        _check(self._lib.spmv_ilu0_setup(self.h, A.h))

    def ilu0_solve(self, A: "Matrix", r: "Vector", z: "Vector") -> None:
        """z = U^-1 L^-1 r with the ILU(0) factors of A (set up on first use), asynchronous; r and z must not overlap"""
        _check(self._lib.spmv_ilu0_solve(self.h, A.h, r.h, z.h))

    def ilu0_factors(self, A: "Matrix") -> np.ndarray:
        """the factor values aligned to the handle's own CSR entries, as an in-place csrilu0 would leave them (l_ik below the
        diagonal in sweep order, u_ij on and above it; of duplicates the first stored one carries the value, the others 0.0)"""
        out = np.zeros(A.info.nnz, dtype=np.float64)
        _check(self._lib.spmv_ilu0_factors(self.h, A.h, out.ctypes.data_as(_f64p)))
        return out

    def ilu0_order(self, A: "Matrix") -> np.ndarray:
        """sets the handle up if need be and returns order[k] = the k-th row of the ILU(0) sweep"""
        out = np.zeros(A.info.nrow, dtype=np.int32)
        _check(self._lib.spmv_ilu0_order(self.h, A.h, out.ctypes.data_as(_i32p)))
        return out

    def trsv_setup(self, A: "Matrix", flags: int = TRSV_LOWER) -> None:
        """analyses the triangle of a square CSR handle that `flags` selects (TRSV_LOWER | TRSV_UPPER, + TRSV_TRANSPOSE): a working
        copy, its levels and launch schedule (synchronous, idempotent; one analysis per uplo and transpose, shared by UNIT and
        non-UNIT solves).  Without TRSV_UNIT a missing, zero or non-finite diagonal entry raises, naming the row"""
        _check(self._lib.spmv_trsv_setup(self.h, A.h, flags))

    def trsv_solve(self, A: "Matrix", b: "Vector", x: "Vector", flags: int = TRSV_LOWER) -> None:
        """x = op(T)^-1 b with the selected triangle of A plus the diagonal (TRSV_UNIT: a unit diagonal), set up on first use,
        asynchronous; entries of the other triangle are ignored.  b and x may be the same vector, else they must not overlap"""
        _check(self._lib.spmv_trsv_solve(self.h, A.h, flags, b.h, x.h))

    def trsv_solve_multi(self, A: "Matrix", B: "Vector", X: "Vector", k: int, flags: int = TRSV_LOWER) -> None:
        """the same for k right-hand sides (1 .. 64) in the launches of one solve; B and X row-major (nrow, k) as apply_multi's.
        Column c has the bits of a k = 1 solve of that column; B and X may be the same vector"""
        _check(self._lib.spmv_trsv_solve_multi(self.h, A.h, flags, k, B.h, X.h))

    def trsv_info(self, A: "Matrix", flags: int = TRSV_LOWER) -> dict:
        """{levels, lanes, launches, bytes} of the analysis `flags` selects: dependency levels, lanes per row and launches of one
        trsv_solve, device bytes; raises where the handle has no such analysis"""
        lv, ln, la, by = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int64(0)
        _check(self._lib.spmv_trsv_info(A.h, flags, C.byref(lv), C.byref(ln), C.byref(la), C.byref(by)))
        return dict(levels=lv.value, lanes=ln.value, launches=la.value, bytes=by.value)

    def lanczos(self, A: "Matrix", steps: int, scaled: bool = False, seed: int = 1):
        """`steps` (1 .. 64) Lanczos steps without reorthogonalisation on a symmetric handle (scaled: on diag(sqrt s) A diag(sqrt s),
        s_i = 1 / a_ii of a CSR handle) from gen_vector(seed) normalised, synchronous.  Returns (ritz_min, ritz_max, alpha, beta,
        steps_done): the extreme eigenvalues of the tridiagonal matrix and its coefficients alpha_j, beta_{j+1}, j < steps_done
        (fewer than `steps` where an invariant subspace ended the run)"""
        lo, hi, done = C.c_double(0.0), C.c_double(0.0), C.c_int32(0)
        alpha, beta = np.zeros(max(int(steps), 1)), np.zeros(max(int(steps), 1))
        _check(self._lib.spmv_lanczos(self.h, A.h, 1 if scaled else 0, steps, seed, C.byref(lo), C.byref(hi), alpha.ctypes.data_as(_f64p),
                                      beta.ctypes.data_as(_f64p), C.byref(done)))
        return lo.value, hi.value, alpha[: done.value], beta[: done.value], done.value

    def chebyshev_setup(self, A: "Matrix", degree: int = 4, scaled: bool = True, lmin: float = 0.0, lmax: float = 0.0) -> None:
        """the Chebyshev polynomial preconditioner of degree `degree` (products per application) on [lmin, lmax] for diag(s) A, s_i =
        1 / a_ii where scaled (a CSR handle), synchronous; replaces earlier state.  lmax = 0: the row bound of a CSR handle (and 1.05
        times Lanczos' largest Ritz value where A.set_param("cheby_lanczos_steps", m > 0)); lmin = 0: lmax / "cheby_ratio" (30)"""
        _check(self._lib.spmv_chebyshev_setup(self.h, A.h, degree, 1 if scaled else 0, lmin, lmax))

    def chebyshev_info(self, A: "Matrix") -> tuple[int, bool, float, float]:
        """(degree, scaled, lmin, lmax) of the handle's Chebyshev state; degree 0: not set up"""
        d, s, lo, hi = C.c_int32(0), C.c_int32(0), C.c_double(0.0), C.c_double(0.0)
        _check(self._lib.spmv_chebyshev_info(A.h, C.byref(d), C.byref(s), C.byref(lo), C.byref(hi)))
        return d.value, bool(s.value), lo.value, hi.value

    def chebyshev_solve(self, A: "Matrix", r: "Vector", z: "Vector") -> None:
        """z = M^-1 r with the handle's Chebyshev polynomial (chebyshev_setup first), asynchronous; r and z must not overlap"""
        _check(self._lib.spmv_chebyshev_solve(self.h, A.h, r.h, z.h))

    def chebyshev(self, A: "Matrix", b: "Vector", x: "Vector") -> None:
        """one smoothing step x += M^-1 (b - A x) with the handle's Chebyshev polynomial (chebyshev_setup first), asynchronous"""
        _check(self._lib.spmv_chebyshev(self.h, A.h, b.h, x.h))

    def amg_setup(self, A: "Matrix", max_levels: int = 0, coarse_max: int = 0, smooth_degree: int = 0, strength: float = 0.0,
                  overcorrection: float = 0.0) -> None:
        """aggregation AMG on a CSR handle (spmv_amg_setup), synchronous; replaces earlier state and the handle's Chebyshev state (the
        smoother of level 0).  0 takes the default: 16 levels, a dense coarsest solve from 256 rows down, smoothing degree 2, every
        stored entry a neighbour, overcorrection 1.5"""
        _check(self._lib.spmv_amg_setup(self.h, A.h, max_levels, coarse_max, smooth_degree, strength, overcorrection))

    def amg_setup_smoothed(self, A: "Matrix", max_levels: int = 0, coarse_max: int = 0, smooth_degree: int = 0, strength: float = 0.0,
                           overcorrection: float = 0.0, prolong_damping: float = 0.0) -> None:
        """smoothed-aggregation AMG on a CSR handle (spmv_amg_setup_smoothed), synchronous; replaces earlier AMG state as amg_setup
        does.  0 takes the default: those of amg_setup but overcorrection 1.0, and prolong_damping 4/3"""
        _check(self._lib.spmv_amg_setup_smoothed(self.h, A.h, max_levels, coarse_max, smooth_degree, strength, overcorrection, prolong_damping))

    def amg_prolongator(self, A: "Matrix", level: int):
        """(row_ptr, col, val) of the smoothed prolongator P of one level on the host (rows[level] x rows[level + 1])"""
        levels, rows, _ = self.amg_info(A)
        nnz = C.c_int64(0)
        _check(self._lib.spmv_amg_prolongator(self.h, A.h, level, C.byref(nnz), None, None, None))
        n, e = int(rows[level]), nnz.value
        rp, cc, cv = np.zeros(n + 1, dtype=np.int32), np.zeros(e, dtype=np.int32), np.zeros(e, dtype=np.float64)
        _check(self._lib.spmv_amg_prolongator(self.h, A.h, level, C.byref(nnz), rp.ctypes.data_as(_i32p), cc.ctypes.data_as(_i32p),
                                              cv.ctypes.data_as(_f64p)))
        return rp, cc, cv

    def amg_transfer_timed(self, A: "Matrix", level: int, what: int, v: "Vector", reps: int, lanes: int = 0) -> float:
        """milliseconds of one restriction (what AMG_RESTRICT_FUSED / AMG_RESTRICT_UNFUSED; v: its right-hand side) or prolongation
        (AMG_PROLONG_FUSED / AMG_PROLONG_UNFUSED; v: the x it adds into) of one level of a smoothed state (spmv_amg_transfer_timed)"""
        ms = C.c_double(0.0)
        _check(self._lib.spmv_amg_transfer_timed(self.h, A.h, level, what, lanes, v.h, reps, C.byref(ms)))
        return ms.value

    def amg_info(self, A: "Matrix") -> tuple[int, np.ndarray, np.ndarray]:
        """(levels, rows per level, entries per level) of the handle's hierarchy"""
        levels, rows, nnz = C.c_int32(0), np.zeros(32, dtype=np.int64), np.zeros(32, dtype=np.int64)
        _check(self._lib.spmv_amg_info(A.h, C.byref(levels), rows.ctypes.data_as(_i64p), nnz.ctypes.data_as(_i64p)))
        return levels.value, rows[: levels.value], nnz[: levels.value]

    def amg_level(self, A: "Matrix", level: int):
        """(agg, row_ptr, col, val) of one level on the host: the aggregate of every row (None on the coarsest level) and the level's
        operator as CSR"""
        levels, rows, nnz = self.amg_info(A)
        if not 0 <= level < levels:
            raise SpmvError(-1, f"amg_level: level={level}, the hierarchy has {levels}")
        n, e = int(rows[level]), int(nnz[level])
        agg = np.zeros(n, dtype=np.int32) if level + 1 < levels else None
        rp, cc, cv = np.zeros(n + 1, dtype=np.int32), np.zeros(e, dtype=np.int32), np.zeros(e, dtype=np.float64)
        _check(self._lib.spmv_amg_level(self.h, A.h, level, agg.ctypes.data_as(_i32p) if agg is not None else None, rp.ctypes.data_as(_i32p),
                                        cc.ctypes.data_as(_i32p), cv.ctypes.data_as(_f64p)))
        return agg, rp, cc, cv

    def amg_solve(self, A: "Matrix", r: "Vector", z: "Vector") -> None:
        """z = B r, one V(1,1) cycle of the handle's hierarchy (amg_setup first), asynchronous; r and z must not overlap"""
        _check(self._lib.spmv_amg_solve(self.h, A.h, r.h, z.h))

    def fsai_setup(self, A: "Matrix", level: int = 0) -> None:
        """FSAI of a symmetric positive definite CSR handle (spmv_fsai_setup), synchronous; replaces earlier state: the lower-triangular
        G with G A G^T ~ I on the pattern of tril(A^level), level 1 .. 3 (0: the handle's "fsai_level", default 1); a row of more than
        FSAI_MAX_ROW pattern columns is refused"""
        _check(self._lib.spmv_fsai_setup(self.h, A.h, level))

    def fsai_solve(self, A: "Matrix", r: "Vector", z: "Vector") -> None:
        """z = G^T (G r) with the handle's FSAI factor (fsai_setup first): two products, asynchronous; r and z must not overlap"""
        _check(self._lib.spmv_fsai_solve(self.h, A.h, r.h, z.h))

    def fsai_info(self, A: "Matrix") -> tuple[int, int, int]:
        """(level, entries of G, pattern columns of its longest row) of the handle's FSAI state"""
        level, nnz, longest = C.c_int32(0), C.c_int64(0), C.c_int32(0)
        _check(self._lib.spmv_fsai_info(A.h, C.byref(level), C.byref(nnz), C.byref(longest)))
        return level.value, nnz.value, longest.value

    def fsai_factor(self, A: "Matrix"):
        """(row_ptr, col, val) of the FSAI factor G on the host: lower triangular, columns ascending, the diagonal last in its row"""
        nnz = C.c_int64(0)
        _check(self._lib.spmv_fsai_factor(self.h, A.h, C.byref(nnz), None, None, None))
        n, e = A.info.nrow, nnz.value
        rp, cc, cv = np.zeros(n + 1, dtype=np.int32), np.zeros(e, dtype=np.int32), np.zeros(e, dtype=np.float64)
        _check(self._lib.spmv_fsai_factor(self.h, A.h, C.byref(nnz), rp.ctypes.data_as(_i32p), cc.ctypes.data_as(_i32p), cv.ctypes.data_as(_f64p)))
        return rp, cc, cv

    def cg(self, A: "Matrix", b: "Vector", x: "Vector", max_iter: int = 1000, rel_tol: float = 1e-8, check_every: int = 1,
           jacobi: bool = False, symgs: bool = False, precond: int | None = None):
        """conjugate gradients on the device from the x passed in (jacobi: diagonal preconditioner, symgs: one symmetric
        Gauss-Seidel sweep per iteration; CSR handles); returns (iterations, ||r|| / ||b||).  precond, if given, is passed as it
        is (PRECOND_*; PRECOND_ILU0: the ILU(0) factors of a CSR handle, set up on first use; PRECOND_CHEBYSHEV: the handle's Chebyshev
        polynomial, set up on first use with the defaults unless chebyshev_setup was called; PRECOND_AMG: one cycle of the handle's
        aggregation AMG hierarchy, likewise unless amg_setup was called; PRECOND_FSAI: the handle's FSAI factor, likewise unless
        fsai_setup was called)"""
        it, res = C.c_int32(0), C.c_double(0.0)
        pc = precond if precond is not None else (PRECOND_SYMGS if symgs else (PRECOND_JACOBI if jacobi else PRECOND_NONE))
        _check(self._lib.spmv_cg(self.h, A.h, b.h, x.h, max_iter, rel_tol, check_every, pc, C.byref(it), C.byref(res)))
        return it.value, res.value

    def cg_multi(self, A: "Matrix", B: "Vector", X: "Vector", k: int, max_iter: int = 1000, rel_tol: float = 1e-8, check_every: int = 1,
                 jacobi: bool = False, precond: int | None = None):
        """k independent conjugate-gradient solves A x_c = b_c in one loop, from the X passed in.  B and X are row-major (nrow, k):
        Vectors of nrow*k entries.  CSR and ELL handles; jacobi: the diagonal preconditioner (CSR).  Columns that have converged are
        frozen.  Returns (iters: np.int32[k], rel_resid: np.float64[k]) per column.  precond, if given, is passed as it is (PRECOND_*)"""
        it, res = np.zeros(max(int(k), 1), dtype=np.int32), np.zeros(max(int(k), 1), dtype=np.float64)
        pc = precond if precond is not None else (PRECOND_JACOBI if jacobi else PRECOND_NONE)
        _check(self._lib.spmv_cg_multi(self.h, A.h, k, B.h, X.h, max_iter, rel_tol, check_every, pc, it.ctypes.data_as(C.POINTER(C.c_int32)),
                                       res.ctypes.data_as(_f64p)))
        return it[:k], res[:k]

    def cgls(self, A: "Matrix", b: "Vector", x: "Vector", max_iter: int = 1000, rel_tol: float = 1e-8, check_every: int = 1,
             damp: float = 0.0):
        """least squares min ||b - A x||^2 + damp^2 ||x||^2 by CGLS on the device, from the x passed in: any format, any shape (b has
        nrow entries, x ncol).  The first call builds the handle's transposed state.  Stops at ||A^T r - damp^2 x|| <= rel_tol *
        ||A^T b||; returns (iterations, ||A^T r - damp^2 x|| / ||A^T b||, ||r|| / ||b||)"""
        it, nres, res = C.c_int32(0), C.c_double(0.0), C.c_double(0.0)
        _check(self._lib.spmv_cgls(self.h, A.h, b.h, x.h, max_iter, rel_tol, check_every, damp, C.byref(it), C.byref(nres), C.byref(res)))
        return it.value, nres.value, res.value

    def bicgstab(self, A: "Matrix", b: "Vector", x: "Vector", max_iter: int = 1000, rel_tol: float = 1e-8, check_every: int = 1,
                 precond: int = 0):
        """A x = b for a square, not necessarily symmetric A by right-preconditioned BiCGSTAB on the device, from the x passed in: any
        format, two forward products per iteration, no transposed state.  precond: any PRECOND_* that the library's table of preconditioners
        (csrc/precond.hip) does not refuse for this solver, on the handles its row takes; two applications per iteration.
        Stops at ||r|| <= rel_tol * ||b||; returns (iterations, ||r|| / ||b||)"""
        it, res = C.c_int32(0), C.c_double(0.0)
        _check(self._lib.spmv_bicgstab(self.h, A.h, b.h, x.h, max_iter, rel_tol, check_every, precond, C.byref(it), C.byref(res)))
        return it.value, res.value

    def gmres(self, A: "Matrix", b: "Vector", x: "Vector", restart: int = 30, max_iter: int = 1000, rel_tol: float = 1e-8, check_every: int = 1,
              precond: int = 0):
        """A x = b for a square, not necessarily symmetric A by right-preconditioned restarted GMRES(restart) on the device, from the x
        passed in: any format, one forward product and one preconditioner application per iteration, classical Gram-Schmidt twice
        against a basis of restart + 1 work vectors (restart: 1 .. 64; 0: 30).  precond: any PRECOND_* that the library's table of
        preconditioners (csrc/precond.hip) does not refuse for this solver, on the handles its row takes.  Does not break down where BiCGSTAB does; stagnation
        (GMRES(1) on a rotation) is no error.  Stops at ||r|| <= rel_tol * ||b||; returns (iterations, ||r|| / ||b||)"""
        it, res = C.c_int32(0), C.c_double(0.0)
        _check(self._lib.spmv_gmres(self.h, A.h, b.h, x.h, restart, max_iter, rel_tol, check_every, precond, C.byref(it), C.byref(res)))
        return it.value, res.value

    def minres(self, A: "Matrix", b: "Vector", x: "Vector", shift: float = 0.0, P: "Matrix | None" = None, max_iter: int = 1000,
               rel_tol: float = 1e-8, check_every: int = 1, precond: int = 0):
        """(A - shift I) x = b for a square symmetric A that need not be positive definite, by preconditioned MINRES on the device, from
        the x passed in: any format, one forward product and one preconditioner application per iteration, no breakdown, a residual that
        never grows.  P: the handle the preconditioner is built from and kept in (None: A) - it must be symmetric positive definite, which
        one built from an indefinite A is not.  precond: PRECOND_NONE, PRECOND_JACOBI, PRECOND_CHEBYSHEV, PRECOND_AMG or PRECOND_FSAI.
        Stops at phibar <= rel_tol * sqrt(b.M^-1 b), phibar the residual's M^-1 norm (the 2-norm without a preconditioner); returns
        (iterations, phibar / sqrt(b.M^-1 b))"""
        it, res = C.c_int32(0), C.c_double(0.0)
        _check(self._lib.spmv_minres(self.h, A.h, P.h if P is not None else None, b.h, x.h, shift, max_iter, rel_tol, check_every, precond,
                                     C.byref(it), C.byref(res)))
        return it.value, res.value

    def refine(self, A: "Matrix", A_lo: "Matrix", b: "Vector", x: "Vector", solver: int = REFINE_CG, precond: int = PRECOND_NONE, max_outer: int = 20,
               inner_max_iter: int = 1000, inner_tol: float = 1e-4, rel_tol: float = 1e-12):
        """iterative refinement (spmv_refine) from the x passed in: r = b - A x in fp64 with A, the correction from `solver`
        (REFINE_CG / REFINE_BICGSTAB, `precond` as that solver takes it) on A_lo - a format-6 copy of A is the intended use - to
        inner_tol, x += d; stops at ||r|| <= rel_tol ||b||, after max_outer steps, or where a step does not reduce ||r|| (x goes
        back to the best iterate).  Returns (outer steps, inner iterations in all, ||b - A x|| / ||b||)"""
        outer, inner, res = C.c_int32(0), C.c_int32(0), C.c_double(0.0)
        _check(self._lib.spmv_refine(self.h, A.h, A_lo.h, b.h, x.h, solver, precond, max_outer, inner_max_iter, inner_tol, rel_tol, C.byref(outer),
                                     C.byref(inner), C.byref(res)))
        return outer.value, inner.value, res.value

    def block_gram(self, n: int, p: int, U: "Vector", ldu: int, q: int, V: "Vector", ldv: int) -> np.ndarray:
        """G = U^T V (p, q) of two column-major blocks (column c at c * ld, ld >= n; rows n .. ld - 1 are padding that is never
        touched), synchronous; 1 <= p, q <= 96.  Deterministic, and exactly symmetric where U and V are the same block"""
        G = np.zeros((max(int(p), 0), max(int(q), 0)), dtype=np.float64)
        buf = G if G.size else np.zeros(1)
        _check(self._lib.spmv_block_gram(self.h, n, p, U.h, ldu, q, V.h, ldv, buf.ctypes.data_as(_f64p)))
        return G

    def block_combine(self, n: int, p: int, S: "Vector", lds: int, q: int, Cm, Out: "Vector", ldo: int) -> None:
        """Out[i, :] = S[i, :] Cm for every row of a column-major block, Cm (p, q) on the host, asynchronous; every output is
        fma(S[i][k], Cm[k][j], .) from 0.0 in ascending k.  Out may be S itself (same start, same ld)"""
        c = _host(Cm, np.float64)
        if c.shape != (p, q):
            raise ValueError(f"block_combine: Cm has shape {c.shape}, not ({p}, {q})")
        _check(self._lib.spmv_block_combine(self.h, n, p, S.h, lds, q, c.ctypes.data_as(_f64p), Out.h, ldo))

    def lobpcg(self, A: "Matrix", X: "Vector", k: int, nev: int | None = None, largest: bool = False, max_iter: int = 500, tol: float = 1e-8,
               precond: int | None = None):
        """the nev (default k) smallest - largest: largest - eigenvalues of a symmetric A and their vectors by LOBPCG with a block of
        k <= 16 vectors, synchronous.  X: nrow * k entries, column-major; holds the start block (gen_vector(nrow * k)) and receives
        the unit vectors.  precond: as for gmres, by the same table (None: PRECOND_NONE), applied column by column; it must be positive definite.
        Stops when resid_j = ||A x_j - theta_j x_j|| <= tol for the first nev columns, or after max_iter iterations (no error).
        Returns (theta[k], resid[k], iterations)"""
        theta, resid, it = np.zeros(max(int(k), 1)), np.zeros(max(int(k), 1)), C.c_int32(0)
        _check(self._lib.spmv_lobpcg(self.h, A.h, k, k if nev is None else nev, 1 if largest else 0, X.h, max_iter, tol, 0 if precond is None else precond,
                                     theta.ctypes.data_as(_f64p), resid.ctypes.data_as(_f64p), C.byref(it)))
        return theta[:k], resid[:k], it.value

    def spgemm(self, A: "Matrix", B: "Matrix", method: int = 0) -> "Matrix":
        """C = A B for two CSR handles (spmv_spgemm), synchronous: a structural pattern with ascending columns, every value its
        products added left to right in stored order.  method: SPGEMM_AUTO, SPGEMM_ROWS (rows in LDS) or SPGEMM_SORT (global sort)"""
        h = _vp()
        _check(self._lib.spmv_spgemm(self.h, A.h, B.h, method, C.byref(h)))
        return Matrix(self, h)

    def csr_transpose(self, A: "Matrix") -> "Matrix":
        """A^T as a CSR handle of its own (spmv_csr_transpose), synchronous: rows ascending inside a row, duplicates kept in order"""
        h = _vp()
        _check(self._lib.spmv_csr_transpose(self.h, A.h, C.byref(h)))
        return Matrix(self, h)

    # ---- reordering
    def perm(self, order) -> "Perm":
        """the permutation order[k] = the old index that takes new position k (spmv_perm_create): uploaded, checked and inverted on
        the device; anything that is not a permutation of 0 .. n-1 raises, naming the smallest offending position"""
        o = _host(order, np.int32)
        h = _vp()
        _check(self._lib.spmv_perm_create(self.h, o.size, o.ctypes.data_as(_i32p) if o.size else None, C.byref(h)))
        return Perm(self, h, o.size)

    def perm_rcm(self, A: "Matrix") -> "Perm":
        """the reverse Cuthill-McKee ordering of a square CSR handle's graph (the pattern of A + A^T), computed on the device
        (spmv_perm_rcm), synchronous; a fixed permutation: every run returns the same integers"""
        h = _vp()
        _check(self._lib.spmv_perm_rcm(self.h, A.h, C.byref(h)))
        return Perm(self, h, A.info.nrow)

    def csr_permute(self, A: "Matrix", rows: "Perm | None" = None, cols: "Perm | None" = None) -> "Matrix":
        """B[k][l] = A[rows.order[k]][cols.order[l]] as a CSR handle of its own (spmv_csr_permute), synchronous: ascending columns
        inside a row, duplicates kept in stored order, values bit for bit; None is the identity"""
        h = _vp()
        _check(self._lib.spmv_csr_permute(self.h, A.h, rows.h if rows is not None else None, cols.h if cols is not None else None, C.byref(h)))
        return Matrix(self, h)

    def vec_permute(self, p: "Perm", src: "Vector", dst: "Vector", back: bool = False) -> None:
        """dst[k] = src[order[k]] (back: dst[order[k]] = src[k]) in one launch, asynchronous; src and dst must not overlap"""
        _check(self._lib.spmv_vec_permute(self.h, p.h, 1 if back else 0, src.h, dst.h))

    def csr_bandwidth(self, A: "Matrix") -> tuple[int, int]:
        """(bandwidth, profile) of a CSR handle: max |i - j| over its entries, and the sum over its non-empty rows of max(0, i - min j)"""
        b, q = C.c_int64(0), C.c_int64(0)
        _check(self._lib.spmv_csr_bandwidth(self.h, A.h, C.byref(b), C.byref(q)))
        return b.value, q.value

    def coo_to_csr(self, coo: "Matrix") -> "Matrix":
        h = _vp()
        _check(self._lib.spmv_coo_to_csr(self.h, coo.h, C.byref(h)))
        return Matrix(self, h)

    def csr_split_columns(self, csr: "Matrix", col_begin: int, col_end: int):
        """(inside, outside): entries with a column in [col_begin, col_end) rebased to 0, and the rest with global columns"""
        a, b = _vp(), _vp()
        _check(self._lib.spmv_csr_split_columns(self.h, csr.h, col_begin, col_end, C.byref(a), C.byref(b)))
        return Matrix(self, a), Matrix(self, b)

    def coo_to_ell(self, coo: "Matrix") -> "Matrix":
        h = _vp()
        _check(self._lib.spmv_coo_to_ell(self.h, coo.h, C.byref(h)))
        return Matrix(self, h)

    def csr_to_ell(self, csr: "Matrix") -> "Matrix":
        h = _vp()
        _check(self._lib.spmv_csr_to_ell(self.h, csr.h, C.byref(h)))
        return Matrix(self, h)

    def csr_to_bsr(self, A: "Matrix", bs: int) -> "Matrix":
        """the BSR handle of a CSR handle (spmv_csr_to_bsr), on the device: block columns ascending, duplicates added in stored order"""
        h = _vp()
        _check(self._lib.spmv_csr_to_bsr(self.h, A.h, bs, C.byref(h)))
        return Matrix(self, h)

    def csr_to_f32(self, A: "Matrix") -> "Matrix":
        """the format-6 handle of a CSR handle (spmv_csr_to_f32), on the device: every value rounded to float, nearest-even; what the
        rounding did is Matrix.f32_info.  A value that is not finite or rounds to +-inf: SpmvError (SPMV_ERR_INVALID)"""
        h = _vp()
        _check(self._lib.spmv_csr_to_f32(self.h, A.h, C.byref(h)))
        return Matrix(self, h)

    def f32_to_csr(self, A: "Matrix") -> "Matrix":
        """the fp64 CSR handle of a format-6 handle's widened values (spmv_f32_to_csr): exact"""
        h = _vp()
        _check(self._lib.spmv_f32_to_csr(self.h, A.h, C.byref(h)))
        return Matrix(self, h)

    def bsr_to_csr(self, A: "Matrix", drop_zeros: bool = True) -> "Matrix":
        """the CSR handle of a BSR handle (spmv_bsr_to_csr), on the device: the positions inside nrow x ncol, columns ascending"""
        h = _vp()
        _check(self._lib.spmv_bsr_to_csr(self.h, A.h, 1 if drop_zeros else 0, C.byref(h)))
        return Matrix(self, h)


class Comm:
    """exchange between several contexts of this process (spmv_comm_*): the x all-gather of the sharded drivers"""

    def __init__(self, ctxs):
        self.ctxs = list(ctxs)
        self._lib = self.ctxs[0]._lib
        arr = (_vp * len(self.ctxs))(*[c.h for c in self.ctxs])
        self.h = _vp()
        _check(self._lib.spmv_comm_create(arr, len(self.ctxs), C.byref(self.h)))

    def __del__(self):
        try:
            if self.h:
                self._lib.spmv_comm_destroy(self.h)
        except Exception:
            pass
        self.h = None

    @property
    def backend(self) -> str:
        return self._lib.spmv_comm_backend(self.h).decode()

    def allgather(self, vecs, offsets) -> None:
        n = len(self.ctxs)
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        # the C side reads vecs[0..n) and offsets[0..n]: a short array would be read out of bounds on the host
        if len(vecs) != n or off.ndim != 1 or off.size != n + 1:
            raise ValueError(f"Comm.allgather: {n} participants need {n} vectors and {n + 1} offsets, got {len(vecs)} and {off.size}")
        arr = (_vp * n)(*[v.h for v in vecs])
        _check(self._lib.spmv_comm_allgather(self.h, arr, off.ctypes.data_as(_i64p)))


class Perm:
    """a permutation on the device (spmv_perm): order[k] is the old index that takes new position k, inverse[order[k]] = k"""

    def __init__(self, ctx: Context, h, n: int):
        self.ctx, self.h, self.n = ctx, h, n

    def __del__(self):
        try:
            if self.h and self.ctx.h:
                self.ctx._lib.spmv_perm_destroy(self.h)
        except Exception:
            pass
        self.h = None

    def download(self) -> tuple[np.ndarray, np.ndarray]:
        """(order, inverse) on the host"""
        o, i = np.zeros(self.n, dtype=np.int32), np.zeros(self.n, dtype=np.int32)
        if self.n:
            _check(self.ctx._lib.spmv_perm_download(self.h, o.ctypes.data_as(_i32p), i.ctypes.data_as(_i32p)))
        return o, i

    def info(self, name: str) -> int:
        """one counter by name (spmv_perm_info): "n", and what perm_rcm did - "rcm_isolated", "rcm_components", "rcm_levels", "rcm_bfs",
        "rcm_launches", "rcm_transient_bytes" (0 for a permutation made by perm)"""
        v = C.c_int64(0)
        _check(self.ctx._lib.spmv_perm_info(self.h, name.encode(), C.byref(v)))
        return v.value


class Vector:
    def __init__(self, ctx: Context, h, n: int):
        self.ctx, self.h, self.n = ctx, h, n
        self._keep = None

    def __del__(self):
        try:
            if self.h and self.ctx.h:
                self.ctx._lib.spmv_vec_destroy(self.h)
        except Exception:
            pass
        self.h = None

    def upload(self, host, offset: int = 0) -> None:
        a = _host(host, np.float64)
        _check(self.ctx._lib.spmv_vec_upload(self.h, offset, a.size, _ptr(a)))

    def download(self, offset: int = 0, n: int | None = None) -> np.ndarray:
        n = self.n - offset if n is None else n
        out = np.empty(n, dtype=np.float64)
        _check(self.ctx._lib.spmv_vec_download(self.h, offset, n, _ptr(out)))
        return out

    def fill(self, a: float) -> None:
        _check(self.ctx._lib.spmv_vec_fill(self.h, a))

    def copy_from(self, src: "Vector", n: int, dst_offset: int = 0, src_offset: int = 0) -> None:
        _check(self.ctx._lib.spmv_vec_copy(self.h, dst_offset, src.h, src_offset, n))

    @property
    def device_ptr(self) -> int:
        p = _vp()
        _check(self.ctx._lib.spmv_vec_device_ptr(self.h, C.byref(p)))
        return p.value or 0


class Matrix:
    def __init__(self, ctx: Context, h):
        self.ctx, self.h = ctx, h
        self._keep = None

    def __del__(self):
        try:
            if self.h and self.ctx.h:
                self.ctx._lib.spmv_mat_destroy(self.h)
        except Exception:
            pass
        self.h = None

    def validate(self) -> None:
        """raise SpmvError if an index is out of range or an offset array is inconsistent"""
        _check(self.ctx._lib.spmv_mat_validate(self.h))

    @property
    def info(self) -> MatInfo:
        i = MatInfo()
        _check(self.ctx._lib.spmv_mat_get_info(self.h, C.byref(i)))
        return i

    def set_kernel(self, kernel: int, lanes_per_row: int = 0) -> None:
        _check(self.ctx._lib.spmv_mat_set_kernel(self.h, kernel, lanes_per_row))

    def set_param(self, name: str, value: int) -> None:
        _check(self.ctx._lib.spmv_mat_set_param(self.h, name.encode(), value))

    def get_param(self, name: str) -> int:
        v = C.c_int64(0)
        _check(self.ctx._lib.spmv_mat_get_param(self.h, name.encode(), C.byref(v)))
        return v.value

    def transpose_setup(self) -> None:
        """build the handle's transposed state now (spmv_mat_transpose_setup): synchronous, idempotent"""
        _check(self.ctx._lib.spmv_mat_transpose_setup(self.h))

    def get_plan(self) -> bytes:
        """the handle's set-up decisions (kernel, layout, tuned parameters; its copies' too) as a POD blob (spmv_mat_get_plan)"""
        n = C.c_int64(0)
        _check(self.ctx._lib.spmv_mat_get_plan(self.h, None, C.byref(n)))
        buf = C.create_string_buffer(n.value)
        _check(self.ctx._lib.spmv_mat_get_plan(self.h, buf, C.byref(n)))
        return buf.raw[: n.value]

    def set_plan(self, plan: bytes) -> None:
        """build exactly the kernel and layout of `plan` (from get_plan of a handle of the same format), no timing launch"""
        _check(self.ctx._lib.spmv_mat_set_plan(self.h, plan, len(plan)))

    def f32_info(self) -> tuple[int, int, float]:
        """(values that changed, nonzero values that became zero or subnormal, largest relative change among the others) of the
        rounding that made this format-6 handle (spmv_f32_info); zeros for an uploaded one"""
        inexact, underflow, rel = C.c_int64(0), C.c_int64(0), C.c_double(0.0)
        _check(self.ctx._lib.spmv_f32_info(self.h, C.byref(inexact), C.byref(underflow), C.byref(rel)))
        return inexact.value, underflow.value, rel.value

    def set_flags(self, flags: int) -> None:
        _check(self.ctx._lib.spmv_mat_set_flags(self.h, flags))

    def partition_rows(self, nparts: int, balance_entries: bool = False) -> np.ndarray:
        """bounds[nparts + 1] of a row partition of this handle (columns for CSC): equal rows (the reference's split) or by entries"""
        bounds = np.zeros(nparts + 1, dtype=np.int64)
        _check(self.ctx._lib.spmv_mat_partition_rows(self.h, nparts, 1 if balance_entries else 0, bounds.ctypes.data))
        return bounds

    def download(self):
        """(a, b, v) host copies; see spmv_mat_download for which array is which per format"""
        i = self.info
        fmt = i.format
        if fmt == FMT_CSR or fmt == FMT_CSR_F32:  # (format 6: the columns and the values widened to double, out of the packed stream)
            na, nb, nv = i.nrow + 1, i.nnz, i.nnz
        elif fmt == FMT_COO:
            na = nb = nv = i.nnz
        elif fmt == FMT_ELL:
            na, nb, nv = 0, i.nrow * i.ell_k, i.nrow * i.ell_k
        elif fmt == FMT_CSC:
            na, nb, nv = i.ncol + 1, i.nnz, i.nnz
        elif fmt == FMT_BSR:  # block row pointer, block columns, nnzb * bs * bs values (ell_k holds bs)
            na, nb, nv = -(-i.nrow // i.ell_k) + 1, i.nnz // (i.ell_k * i.ell_k), i.nnz
        else:
            na, nb, nv = i.ell_k, 0, i.nrow * i.ell_k
        a = np.empty(na, dtype=np.int32)
        b = np.empty(nb, dtype=np.int32)
        v = np.empty(nv, dtype=np.float64)
        _check(self.ctx._lib.spmv_mat_download(self.h, _ptr(a) if na else None, _ptr(b) if nb else None, _ptr(v) if nv else None))
        return a, b, v
