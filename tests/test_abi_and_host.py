"""CPU-side checks of the boundary: the shared library loads, exports every symbol the header declares, the
ctypes table matches the header, and the engine refuses to run without a GPU instead of falling back."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "spmv_abi.h").read_text()


def declared_symbols():
    body = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    return sorted(set(re.findall(r"\b(spmv_[a-z0-9_]+)\s*\(", body)))


def test_library_exports_every_declared_symbol(pkg):
    lib = pkg.capi.load()
    names = declared_symbols()
    assert len(names) >= 40
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/spmv_abi.h but not exported by libspmv_hip.so"


def test_ctypes_table_covers_the_header(pkg):
    assert sorted(pkg.capi.SIGNATURES) == declared_symbols()
    assert pkg.capi.load().spmv_abi_version() == 1


def test_mat_info_layout_matches_header(pkg):
    fields = re.search(r"typedef struct spmv_mat_info\s*\{(.*?)\}\s*spmv_mat_info;", HEADER, re.S).group(1)
    names = re.findall(r"int(?:32|64)_t\s+(\w+);", fields)
    assert names == [f[0] for f in pkg.capi.MatInfo._fields_]
    assert C.sizeof(pkg.capi.MatInfo) == 56


def test_no_gpu_means_loud_failure_not_fallback(pkg):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(pkg.capi.SpmvError) as e:
        pkg.capi.Context(0)
    assert e.value.code == -2 and "no CPU fallback" in str(e.value)


def test_partition_rows_host_arithmetic(pkg, orc):
    import oracle_lib as ol

    capi = pkg.capi
    for nrow, parts in ((10, 4), (3, 8), (80_000_000, 8), (10_000_001, 7), (0, 3)):
        got = [capi.partition_rows(nrow, parts, p) for p in range(parts)]
        assert got == [ol.partition_rows(orc, nrow, parts, p) for p in range(parts)]
        assert got[0][0] == 0 and got[-1][1] == nrow
        assert all(got[i][1] == got[i + 1][0] for i in range(parts - 1))
    with pytest.raises(capi.SpmvError):
        capi.partition_rows(10, 0, 0)
    # nnz-balanced split of a skewed matrix: every part within one row of its share
    lens = np.array([1] * 1000 + [4096] + [1] * 1000 + [300] * 10, dtype=np.int64)
    rp = np.concatenate(([0], np.cumsum(lens)))
    b = capi.partition_rows_balanced(rp, 4)
    assert b[0] == 0 and b[-1] == len(lens) and np.all(np.diff(b) >= 0)
    share = rp[b[1:]] - rp[b[:-1]]
    assert share.sum() == rp[-1] and share.max() <= rp[-1] / 4 + 4096


def test_balanced_partition_takes_the_nearest_row_boundary(pkg):
    """spmv_partition_rows_balanced: boundary p = the row boundary whose offset lies nearest to p / nparts of the entries (ties go
    to the later one), monotone, rows never split - against a plain numpy restatement on random and adversarial offsets"""
    capi = pkg.capi
    rng = np.random.default_rng(77)
    cases_ = []
    for _ in range(40):
        nrow = int(rng.integers(1, 400))
        kind = rng.integers(0, 4)
        lens = (rng.integers(0, 50, nrow) if kind == 0 else np.where(rng.random(nrow) < 0.05, rng.integers(1000, 5000, nrow), rng.integers(0, 3, nrow))
                if kind == 1 else np.zeros(nrow, np.int64) if kind == 2 else np.sort(rng.integers(0, 200, nrow))[::-1])
        cases_.append(np.concatenate(([0], np.cumsum(lens))).astype(np.int64))
    cases_.append(np.array([0, 0, 0, 10, 10, 10], np.int64))  # every entry in one row
    cases_.append(np.array([5, 7, 9, 11], np.int64))          # offsets that do not start at 0 (a slice of a larger array)
    for rp in cases_:
        nrow = len(rp) - 1
        for parts in (1, 2, 3, 8, 13):
            got = capi.partition_rows_balanced(rp, parts)
            want = [0]
            nnz = int(rp[-1] - rp[0])
            for p in range(1, parts):
                target = int(rp[0]) + (nnz * p) // parts
                r = int(np.searchsorted(rp, target, side="left"))
                r = min(r, nrow)
                if r > 0 and target - int(rp[r - 1]) < int(rp[r]) - target:
                    r -= 1
                want.append(max(r, want[-1]))
            want.append(nrow)
            assert list(got) == want, (rp[:12], parts, list(got), want)
            assert got[0] == 0 and got[-1] == nrow and np.all(np.diff(got) >= 0)


def test_synth_generators_are_index_addressable(pkg):
    s = pkg.synth
    rp, c, v = s.csr_uniform(0, 1000, 5000, 8, seed=3)
    rp2, c2, v2 = s.csr_uniform(400, 600, 5000, 8, seed=3)
    assert np.array_equal(c[400 * 8:600 * 8], c2) and np.array_equal(v[400 * 8:600 * 8], v2)
    assert rp2[0] == 0 and rp2[-1] == 200 * 8
    assert c.min() >= 0 and c.max() < 5000 and v.min() >= -1 and v.max() < 1
    _, cb, _ = s.csr_uniform(0, 1000, 5000, 8, band=64, seed=3)
    d = (cb.reshape(1000, 8).astype(np.int64) - np.arange(1000)[:, None]) % 5000
    assert np.all((d < 32) | (d >= 5000 - 32))
    assert np.array_equal(s.vec_uniform(100, 50, 9), s.vec_uniform(150, 0, 9)[50:])
    ln = s.powerlaw_lengths(200_000, 4096, seed=1)
    assert ln.min() >= 8 and ln.max() == 4096 and 40 < ln.mean() < 80
    r, cc, vv = s.coo_powerlaw(2000, 3000, 4096, seed=1)
    assert np.all(np.diff(r) >= 0) and len(r) == s.powerlaw_lengths(2000, 4096, 1).sum()
    # the same distribution at its quantiles: rows sorted by length, the longest first (positional skew for the partition tests)
    ls = s.powerlaw_lengths(200_000, 4096, seed=1, sorted_by_length=True)
    assert np.all(np.diff(ls) <= 0) and ls[0] == 4096 and ls[-1] == 8 and abs(ls.mean() - ln.mean()) < 2.0
    rs, cs, vs = s.coo_powerlaw(2000, 3000, 4096, seed=1, sorted_by_length=True)
    assert np.all(np.diff(rs) >= 0) and len(rs) == s.powerlaw_lengths(2000, 4096, 1, True).sum() and cs.max() < 3000
    # known answers pin the generator itself (splitmix64 reference values)
    assert int(s.splitmix64(np.array([0], dtype=np.uint64))[0]) == 0xE220A8397B1DCDAF
    assert int(s.splitmix64(np.array([1], dtype=np.uint64))[0]) == 0x910A2DEC89025CC1


def test_no_kernel_of_the_engine_uses_scratch(tmp_path):
    """`make engine` is gated by tools/kernel_resources.py --check tools/hot_kernels.txt: a kernel of the engine that spills a
    register or uses scratch memory fails the build (round 3 shipped a spilling expand kernel whose documentation said it
    did not).  The same check over the objects of the build that was just loaded; a list whose pattern matches no kernel
    (a renamed kernel) must fail too."""
    import glob
    import subprocess
    import sys

    objs = sorted(glob.glob(str(ROOT / "build" / "obj" / "*.o")))
    if not objs:
        pytest.skip("no object files here (the library travelled without its build directory)")
    tool = str(ROOT / "tools" / "kernel_resources.py")
    r = subprocess.run([sys.executable, tool, "--check", str(ROOT / "tools" / "hot_kernels.txt")] + objs, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "none uses scratch" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    n = int(r.stdout.strip().splitlines()[-1].split()[2])
    assert n >= 300  # every kernel the engine defines (rocPRIM's are excluded by name)
    bad = tmp_path / "patterns.txt"
    bad.write_text("csr_panel_pp_kernel<*\nno_such_kernel_anywhere*\n")
    r = subprocess.run([sys.executable, tool, "--check", str(bad)] + objs, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "matched no kernel" in r.stderr


def test_placement_spread_arithmetic_holds_for_every_fp32_time(tmp_path):
    """`twophase_placement_spread` (csrc/placement_math.hpp, used by tp_choose_pieces) is exactly 1000 when the search keeps
    the pieces as built and >= 1000 whenever the kept configuration is the faster one - for EVERY positive fp32 time, not for
    the draw of one run (round 4 truncated (1000.0f * t) / t: 999 for 11.8 % of the times between 0.3 and 2 ms, and the GPU
    parity suite asserts >= 1000).  tests/placement_math_check.cpp walks all 2.1e9 normal floats in ~2 s."""
    import shutil
    import subprocess

    if not shutil.which("g++"):
        pytest.skip("no g++ here")
    exe = tmp_path / "placement_math_check"
    subprocess.run(["g++", "-O2", "-std=c++17", f"-I{ROOT / 'arm-spmv_amd' / 'csrc'}", str(ROOT / "tests" / "placement_math_check.cpp"), "-o", str(exe)],
                   check=True, timeout=120)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    words = r.stdout.split()
    assert int(words[1]) > 2_000_000_000 and words[3] == "0" and words[5] == "0"
    assert int(words[7]) > 1_000_000  # the old form really had the hole this test closes


def test_panel_row_groups_cover_the_rows_and_ask_for_a_finer_cut_only_when_skewed(tmp_path):
    """The panel layout's row groups (csrc/panel_groups.hpp, used by csr_panel_build): every cut covers all rows once under the
    LDS cap of 20000 rows; the busiest-CU figure is what a direct count gives; a profile of many light rows and one heavy
    stretch (the shape of an R-MAT graph's row lengths: round 5) leaves the single round of 256 groups far from even
    and asks for a trial of more rounds, a uniform profile does not.  tests/panel_groups_check.cpp, 300 cuts."""
    import shutil
    import subprocess

    if not shutil.which("g++"):
        pytest.skip("no g++ here")
    exe = tmp_path / "panel_groups_check"
    subprocess.run(["g++", "-O2", "-std=c++17", f"-I{ROOT / 'arm-spmv_amd' / 'csrc'}", str(ROOT / "tests" / "panel_groups_check.cpp"), "-o", str(exe)],
                   check=True, timeout=120)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and " 0 violations" in r.stdout, r.stdout + r.stderr
    assert "uniform: trial of 0" in r.stdout


def test_split_virtual_rows_hold_every_entry_once_in_order(tmp_path):
    """Kernel SPLIT, mode 2 (csrc/split_rows.hpp, used by csr_split_build): a long row's entries are dealt out to V = ceil(len / 64)
    virtual rows, entry k to row k mod V at position k / V.  tests/split_rows_check.cpp: the dealing is a bijection, keeps the
    order inside every virtual row, balances their lengths to within one, and parts neighbouring entries."""
    import shutil
    import subprocess

    if not shutil.which("g++"):
        pytest.skip("no g++ here")
    exe = tmp_path / "split_rows_check"
    subprocess.run(["g++", "-O2", "-std=c++17", f"-I{ROOT / 'arm-spmv_amd' / 'csrc'}", str(ROOT / "tests" / "split_rows_check.cpp"), "-o", str(exe)],
                   check=True, timeout=120)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and " 0 violations" in r.stdout, r.stdout + r.stderr


def test_panel_launch_settings_are_what_launch_and_plan_computed_and_always_instantiated(tmp_path):
    """The panel kernel's chunk size, load order and barrier (csrc/panel_settings.hpp: panel_effective, called by panel_launch
    and by the plan's collect) for every request and every build-time trial result that can reach a launch: equal to the
    expressions the two sites held separately (restated in tests/panel_settings_check.cpp), always one of the instantiated
    combinations, and - on the values include/spmv_abi.h documents - equal to what spmv_mat_get_param reports."""
    import shutil
    import subprocess

    if not shutil.which("g++"):
        pytest.skip("no g++ here")
    exe = tmp_path / "panel_settings_check"
    subprocess.run(["g++", "-O2", "-std=c++17", f"-I{ROOT / 'arm-spmv_amd' / 'csrc'}", str(ROOT / "tests" / "panel_settings_check.cpp"), "-o", str(exe)],
                   check=True, timeout=120)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    words = r.stdout.replace(",", "").split()
    assert r.returncode == 0, r.stdout + r.stderr
    assert int(words[1]) == 34 * 4 * 6 * 3 * 10 * 4  # every combination of the ranges above
    assert words[3] == "0" and words[5] == "0"  # differences from the two sites; results outside the instantiated set
    assert int(words[8]) == 5 * 4 * 4 * 3 * 5 * 4 and words[10] == "0"  # documented requests: get_param reports what runs


def test_ell_launch_settings_are_what_the_product_decided_and_always_instantiated(tmp_path):
    """What a product of an ELL handle launches (csrc/ell_settings.hpp: ell_effective, called by ell_own_apply) for every variant,
    lanes_per_row, flag, row parity, alignment, set of copies in memory, window size and padding mark: equal to the nested
    conditions and launch macros ell_own_apply held before (restated in tests/ell_settings_check.cpp) and always one of the
    instantiated kernels - the fall-through of variant 3 without its copy, the 5120-double window cap and unroll 8 on the one-row
    path included."""
    import shutil
    import subprocess

    if not shutil.which("g++"):
        pytest.skip("no g++ here")
    exe = tmp_path / "ell_settings_check"
    subprocess.run(["g++", "-O2", "-std=c++17", f"-I{ROOT / 'arm-spmv_amd' / 'csrc'}", str(ROOT / "tests" / "ell_settings_check.cpp"), "-o", str(exe)],
                   check=True, timeout=120)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    words = r.stdout.replace(",", "").split()
    assert r.returncode == 0, r.stdout + r.stderr
    # variants x lanes_per_row x (flag, parity, 3 alignments, descriptors, mask, tiles, DIA-order copy, padding mark) x window sizes
    assert int(words[1]) == 4 * 8 * 2 ** 10 * 4
    assert words[3] == "0" and words[5] == "0"  # differences from ell_own_apply as it stood; results outside the instantiated set
    paths = [int(w) for w in words[-4:]]
    assert sum(paths) == int(words[1]) and min(paths) > 0  # every path is reached: DIA order, diagonal slots, columns, one row


def test_plan_blobs_are_checked_without_a_device(pkg):
    """spmv_plan_check: the validation spmv_mat_set_plan / spmv_ctx_set_plan run on a blob, callable anywhere (a plan received
    from another rank, read from a file).  A node is 32 four-byte fields: format, kernel, lanes, flags, 9 panel fields, 2 split,
    2 two-phase, 2 ELL, COO bins, 3 child indices (-1: none), 9 reserved; children come after their parent."""
    import struct

    capi = pkg.capi

    def node(fmt, kernel, lanes=0, children=(-1, -1, -1), **kw):
        f = [0] * 32
        f[0], f[1], f[2] = fmt, kernel, lanes
        f[12] = kw.get("rounds", 1)
        f[14] = kw.get("split_mode", 0)
        f[17] = kw.get("ell_variant", 0)
        f[19] = kw.get("bins", 0)
        f[20], f[21], f[22] = children
        return struct.pack("<32i", *f)

    def blob(*nodes, magic=0x4E4C5053, version=1, nbytes=None, count=None):
        body = b"".join(nodes)
        return struct.pack("<IIII", magic, version, 16 + len(body) if nbytes is None else nbytes, len(nodes) if count is None else count) + body

    one = blob(node(capi.FMT_CSR, capi.CSR_PANEL, 8))
    assert capi.plan_check(one) == (capi.FMT_CSR, capi.CSR_PANEL, 1)
    # a COO handle that runs from its row-grouped copy, which runs the long-row split in virtual-row mode: four nodes
    tree = blob(node(capi.FMT_COO, capi.CSR_PANEL, children=(1, -1, -1)), node(capi.FMT_CSR, capi.CSR_SPLIT, children=(2, 3, -1), split_mode=2),
                node(capi.FMT_CSR, capi.CSR_PANEL), node(capi.FMT_CSR, capi.CSR_VECTOR, 16))
    assert capi.plan_check(tree) == (capi.FMT_COO, capi.CSR_PANEL, 4)
    assert capi.plan_check(blob(node(capi.FMT_CSR, capi.CSR_ELL, children=(-1, -1, 1)), node(capi.FMT_ELL, capi.CSR_VECTOR, ell_variant=3))) == (capi.FMT_CSR, capi.CSR_ELL, 2)
    bad = {
        "empty": b"", "header only": one[:16], "truncated": one[:-4], "magic": blob(node(1, 1), magic=0x12345678), "version": blob(node(1, 1), version=2),
        "byte count": blob(node(1, 1), nbytes=999), "node count": blob(node(1, 1), count=2), "no nodes": blob(count=0),
        "too many nodes": blob(*[node(1, 1)] * 65), "format": blob(node(7, 1)), "kernel": blob(node(1, 9)), "negative kernel": blob(node(1, -1)),
        "lanes not a power of two": blob(node(1, 1, 3)), "lanes beyond a wavefront": blob(node(1, 1, 128)),
        "child points at itself": blob(node(0, 4, children=(0, -1, -1))), "child points backwards": blob(node(1, 7, children=(1, -1, -1)), node(1, 7, children=(0, -1, -1))),
        "child out of range": blob(node(0, 4, children=(5, -1, -1)), node(1, 1)), "row-grouped copy that is not CSR": blob(node(0, 4, children=(1, -1, -1)), node(3, 1)),
        "ELL copy that is not ELL": blob(node(1, 8, children=(-1, -1, 1)), node(1, 1)), "split mode": blob(node(1, 7, split_mode=3)),
        "ELL variant": blob(node(3, 1, ell_variant=4)), "COO bins": blob(node(0, 1, bins=9)), "rounds": blob(node(1, 4, rounds=17)),
    }
    for what, b in bad.items():
        with pytest.raises(capi.SpmvError, match="plan") as e:
            capi.plan_check(b)
        assert e.value.code == -1, what  # SPMV_ERR_INVALID
    # an unaligned buffer: the library copies the nodes out before it reads a field
    raw = bytearray(b"\x00" + tree)
    view = (C.c_char * len(tree)).from_buffer(raw, 1)
    f, k, n = C.c_int32(), C.c_int32(), C.c_int32()
    assert capi.load().spmv_plan_check(C.addressof(view), len(tree), C.byref(f), C.byref(k), C.byref(n)) == 0 and n.value == 4
