"""CPU-side checks of the sampled dense-dense product (spmv_sddmm, spmv_sddmm_timed, spmv_csr_with_values): the header declares
them, the library exports them, the Python bindings have them, their null-argument checks run before any device use, and the
no-scratch gate names the new kernels."""
import ctypes as C
import fnmatch
import inspect
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
ENTRY_POINTS = ("spmv_sddmm", "spmv_sddmm_timed", "spmv_csr_with_values")


def test_header_library_and_bindings_agree(pkg):
    lib = pkg.capi.load()
    header = (ROOT / "include" / "spmv_abi.h").read_text()
    for name in ENTRY_POINTS:
        assert re.search(rf"\bint {name}\(", header), f"include/spmv_abi.h does not declare {name}"
        assert hasattr(lib, name), f"libspmv_hip.so does not export {name}"
        assert name in pkg.capi.SIGNATURES
    sig = pkg.capi.SIGNATURES
    vp = C.c_void_p
    assert sig["spmv_sddmm"] == (C.c_int, [vp, vp, C.c_int32, C.c_double, vp, vp, C.c_double, vp])
    assert sig["spmv_sddmm_timed"] == (C.c_int, [vp, vp, C.c_int32, C.c_double, vp, vp, C.c_double, vp, C.c_int32, C.POINTER(C.c_double)])
    restype, argtypes = sig["spmv_csr_with_values"]
    assert restype is C.c_int and len(argtypes) == 4 and argtypes[:3] == [vp, vp, vp]
    assert re.search(r"#define SPMV_ABI_VERSION 1\b", header) and lib.spmv_abi_version() == 1
    # the order contract is written down where the other products' contracts are
    doc = header[header.index("spmv_sddmm:"):header.index("int spmv_sddmm(")]
    assert "Order of the additions" in doc and "depends on k alone" in doc and "never read" in doc


def test_null_arguments_are_refused_without_a_device(pkg):
    lib = pkg.capi.load()
    ms, h = C.c_double(-1.0), C.c_void_p()
    calls = {
        "spmv_sddmm": lambda: lib.spmv_sddmm(None, None, 4, 1.0, None, None, 0.0, None),
        "spmv_sddmm_timed": lambda: lib.spmv_sddmm_timed(None, None, 4, 1.0, None, None, 0.0, None, 3, C.byref(ms)),
        "spmv_csr_with_values": lambda: lib.spmv_csr_with_values(None, None, None, C.byref(h)),
    }
    for name, call in calls.items():
        assert call() == -1, name
        err = lib.spmv_last_error()
        assert name.replace("_timed", "").encode() in err and b"null" in err, (name, err)
    assert ms.value == -1.0 and not h.value


def test_context_and_operator_have_the_methods(pkg):
    ctx = pkg.capi.Context
    for name, head in (("sddmm", ["self", "A", "U", "V", "k", "out", "alpha", "beta"]),
                       ("sddmm_timed", ["self", "A", "U", "V", "k", "out", "reps", "alpha", "beta"]),
                       ("csr_with_values", ["self", "A", "values"])):
        fn = getattr(ctx, name, None)
        assert callable(fn), name
        params = inspect.signature(fn).parameters
        assert list(params) == head, (name, list(params))
        if "alpha" in params:
            assert params["alpha"].default == 1.0 and params["beta"].default == 0.0
    source = (ROOT / "arm-spmv_amd" / "torch_ops.py").read_text()
    assert re.search(r"def sddmm\(self, U: torch\.Tensor, V: torch\.Tensor\)", source)
    assert re.search(r"def spmv\(op: SparseOperator, x: torch\.Tensor, values: torch\.Tensor \| None = None\)", source)
    assert re.search(r"def spmm\(op: SparseOperator, X: torch\.Tensor, values: torch\.Tensor \| None = None\)", source)


def test_the_no_scratch_gate_names_the_new_kernels():
    """every __global__ kernel that csrc/kernels_sddmm.hip defines matches a pattern of tools/hot_kernels.txt that names it (not the catch-all)"""
    source = (ROOT / "arm-spmv_amd" / "csrc" / "kernels_sddmm.hip").read_text()
    kernels = re.findall(r"__global__[^;{]*?void\s+(\w+)\s*\(", source)
    assert len(kernels) >= 2 and {"sddmm_kernel", "sddmm_k1_kernel"} <= set(kernels), kernels
    patterns = [line.split("#")[0].strip() for line in (ROOT / "tools" / "hot_kernels.txt").read_text().splitlines()]
    patterns = [p for p in patterns if p.startswith("sddmm_")]
    assert len(patterns) >= len(kernels), patterns
    for k in kernels:
        assert any(fnmatch.fnmatch(k, p) or fnmatch.fnmatch(k + "<16>", p) for p in patterns), (k, patterns)


def test_the_settings_header_is_a_build_dependency():
    assert "$(CSRC)/sddmm_settings.hpp" in (ROOT / "Makefile").read_text()
