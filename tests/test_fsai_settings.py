"""The FSAI row kernel's lane classes, LDS sizes and packed-triangle offsets (csrc/fsai_settings.hpp, used by csrc/fsai.hip) are pure
host arithmetic: compiled with g++ and held to their properties by tests/fsai_settings_check.cpp, in the manner of the other
*_settings checks."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def test_lane_classes_lds_sizes_and_triangle_offsets(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++ here")
    exe = tmp_path / "fsai_settings_check"
    subprocess.run(["g++", "-O2", "-std=c++17", f"-I{ROOT / 'arm-spmv_amd' / 'csrc'}", str(ROOT / "tests" / "fsai_settings_check.cpp"), "-o", str(exe)],
                   check=True, timeout=120)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and " 0 violations" in r.stdout, r.stdout + r.stderr
    assert "5 class edges" in r.stdout and "cap 64" in r.stdout
