"""The sampled product's division of the entries among runs, chunks, lane groups and steps, and of the columns among a group's lanes
(csrc/sddmm_settings.hpp, used by csrc/kernels_sddmm.hip) is pure host arithmetic: compiled with g++ and held to its properties by
tests/sddmm_settings_check.cpp, in the manner of the other *_settings checks."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def settings():
    """the integer constants of the header by name"""
    text = (ROOT / "arm-spmv_amd" / "csrc" / "sddmm_settings.hpp").read_text()
    out = {}
    for name, expr in re.findall(r"constexpr int (kSddmm\w+)\s*=\s*([^;]+);", text):
        out[name] = int(eval(expr, {"__builtins__": {}}))  # (products of literals)
    return out


def test_every_entry_and_column_has_one_owner(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++ here")
    exe = tmp_path / "sddmm_settings_check"
    subprocess.run(["g++", "-O2", "-std=c++17", f"-I{ROOT / 'arm-spmv_amd' / 'csrc'}", str(ROOT / "tests" / "sddmm_settings_check.cpp"), "-o", str(exe)],
                   check=True, timeout=120)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and " 0 violations" in r.stdout, r.stdout + r.stderr
    s = settings()
    assert f"7 lane classes, run {s['kSddmmRun']}, cap {s['kSddmmMaxGrid']}" in r.stdout and "k up to 64" in r.stdout


def test_constants_the_tests_rely_on():
    s = settings()
    assert s["kSddmmMaxK"] == 64 and s["kSddmmWave"] == 64 and s["kSddmmChunk"] == 64
    assert s["kSddmmRun"] % s["kSddmmChunk"] == 0 and s["kSddmmBlock"] % s["kSddmmWave"] == 0
    # one trip of the full grid stays within a few million entries, so that the second trip can be tested quickly
    assert s["kSddmmMaxGrid"] * (s["kSddmmBlock"] // s["kSddmmWave"]) * s["kSddmmRun"] <= 4 * 2**20
