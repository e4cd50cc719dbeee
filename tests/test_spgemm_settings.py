"""spmv_spgemm's row classes (csrc/spgemm_settings.hpp, used by csrc/spgemm.hip) are pure host arithmetic: compiled with g++ and held
to their properties by tests/spgemm_settings_check.cpp, in the manner of the split_rows and ell_settings checks."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def test_row_classes_are_total_monotone_fit_lds_and_have_the_stated_edges(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++ here")
    exe = tmp_path / "spgemm_settings_check"
    subprocess.run(["g++", "-O2", "-std=c++17", f"-I{ROOT / 'arm-spmv_amd' / 'csrc'}", str(ROOT / "tests" / "spgemm_settings_check.cpp"), "-o", str(exe)],
                   check=True, timeout=120)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and " 0 violations" in r.stdout, r.stdout + r.stderr
    assert "3 class edges" in r.stdout
