"""csrc/bsr_settings.hpp on the host: the lane map, the reduction's partners, the lanes per block row and the grid of the block CSR
product, walked by tests/bsr_settings_check.cpp under g++.  No GPU."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def test_the_lane_map_the_reduction_and_the_grid_of_the_settings_header(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++ here")
    exe = tmp_path / "bsr_settings_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT / 'arm-spmv_amd' / 'csrc'}", str(ROOT / "tests" / "bsr_settings_check.cpp"), "-o", str(exe)],
                   check=True, timeout=120)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and " 0 violations" in r.stdout, r.stdout + r.stderr
    assert int(r.stdout.split()[0]) > 10000, r.stdout


def test_the_kernel_file_takes_its_arithmetic_from_the_header():
    text = (ROOT / "arm-spmv_amd" / "csrc" / "kernels_bsr.hip").read_text()
    for name in ("bsr_lane_map", "bsr_first_row", "bsr_value_offset", "bsr_half", "bsr_grid", "bsr_pick_lanes", "bsr_lanes_valid"):
        assert name + "(" in text, name
    assert "atomicAdd" not in text and "unsafeAtomicAdd" not in text  # no atomics on y
    hot = (ROOT / "tools" / "hot_kernels.txt").read_text()
    assert "bsr_vector_kernel<*" in hot
