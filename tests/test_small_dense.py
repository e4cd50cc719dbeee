"""The small dense host routines of spmv_lobpcg (csrc/small_dense.hpp: cyclic Jacobi, Cholesky with its smallest pivot, the triangular
inverse, the generalised symmetric problem) are pure host arithmetic: compiled with g++ and held to their bounds by
tests/small_dense_check.cpp, in the manner of the spgemm_settings check - once plainly, once under the address and undefined-behaviour
sanitizers (a stand-alone program with its own main)."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def _build_and_run(tmp_path, name, flags):
    if not shutil.which("g++"):
        pytest.skip("no g++ here")
    exe = tmp_path / name
    subprocess.run(["g++", *flags, "-std=c++17", f"-I{ROOT / 'arm-spmv_amd' / 'csrc'}", str(ROOT / "tests" / "small_dense_check.cpp"), "-o", str(exe)],
                   check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and " 0 violations" in r.stdout, r.stdout + r.stderr
    assert "16 orders up to 144" in r.stdout
    return r


def test_eigen_cholesky_inverse_and_generalised_problem_meet_their_bounds(tmp_path):
    _build_and_run(tmp_path, "small_dense_check", ["-O2", "-ffp-contract=off"])


def test_the_same_program_is_clean_under_address_and_undefined_sanitizers(tmp_path):
    r = _build_and_run(tmp_path, "small_dense_check_san", ["-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
