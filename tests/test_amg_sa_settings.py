"""The lanes a row of R or P takes in the smoothed-aggregation cycle (csrc/amg_sa_settings.hpp, used by csrc/amg.hip) are pure host
arithmetic: compiled with g++ and held to their properties by tests/amg_sa_settings_check.cpp, in the manner of the spgemm_settings
check."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def test_the_lane_rule_is_the_largest_power_of_two_below_half_the_mean_row(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++ here")
    exe = tmp_path / "amg_sa_settings_check"
    subprocess.run(["g++", "-O2", "-std=c++17", f"-I{ROOT / 'arm-spmv_amd' / 'csrc'}", str(ROOT / "tests" / "amg_sa_settings_check.cpp"), "-o", str(exe)],
                   check=True, timeout=120)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and " 0 violations" in r.stdout, r.stdout + r.stderr
    assert "103 named row lengths" in r.stdout
