"""csrc/csr_f32_settings.hpp on the host: the packed entry word, the classification of a double under rounding to float, the lane
counts and the grid of the single-precision-storage product, walked by tests/csr_f32_settings_check.cpp under g++.  No GPU."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "arm-spmv_amd" / "csrc"


def test_the_entry_word_the_classification_and_the_grid_of_the_settings_header(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++ here")
    exe = tmp_path / "csr_f32_settings_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", f"-I{CSRC}", str(ROOT / "tests" / "csr_f32_settings_check.cpp"), "-o", str(exe)], check=True,
                   timeout=120)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and " 0 violations" in r.stdout, r.stdout + r.stderr
    assert int(r.stdout.split()[0]) > 6000, r.stdout  # (seven lane counts x 301 row counts x three checks, and the rest)


def test_the_kernel_file_takes_its_arithmetic_from_the_header():
    text = (CSRC / "kernels_csr_f32.hip").read_text()
    for name in ("f32_entry_col", "f32_entry_value", "csr_f32_grid", "csr_f32_rows_per_workgroup", "csr_f32_lanes_valid", "csr_f32_lanes_that_fit"):
        assert name + "(" in text, name
    code = re.sub(r"//[^\n]*", "", text)
    assert "atomicAdd" not in code and "unsafeAtomicAdd" not in code  # no atomic add on y (the fused dot's slot_add is wave.hpp's)
    assert "group_sum<LPR, false>" in code and "load_stream(ent" in code and "int64_t       j" in code  # the lanes' join, ONE load per entry, 64-bit offsets
    assert "csr_vector_kernel" not in code  # a kernel of its own, not an instance of the fp64 one
    conv = (CSRC / "convert_f32.hip").read_text()
    for name in ("f32_classify", "f32_pack", "f32_changed", "f32_rel_change", "f32_entry_col", "f32_entry_value"):
        assert name + "(" in conv, name
    hot = (ROOT / "tools" / "hot_kernels.txt").read_text()
    assert "csr_f32_kernel<*" in hot
    assert "csr_f32_settings.hpp" in (ROOT / "Makefile").read_text()


def test_the_fp64_row_parallel_kernel_is_as_it_was():
    """the format is a kernel of its own: csr_vector_kernel keeps its three template parameters and its two loads per entry"""
    text = (CSRC / "kernels_csr.hip").read_text()
    assert "template <int LPR, bool USE_DPP, bool XCD_REMAP>\n__global__ __launch_bounds__(kBlock) void csr_vector_kernel(" in text
    assert "const int    c0 = load_stream(col + j);" in text and "const double v0 = load_stream(val + j);" in text
