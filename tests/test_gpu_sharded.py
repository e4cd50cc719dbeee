"""The sharded solver step on real shards (`pytest -m gpu`): dist.HipShardOps beyond world 1.

tests/child_sharded_cg.py runs HipShardOps at world 1 only: the shard starts at row 0, owns every column, its outside part is
empty and the block the Gauss-Seidel sweep works on is the whole matrix.  Here
  * child_sharded_ops.py calls every method of HipShardOps on rank r's shard of a world of 1, 2, 3 and 8 (and of 8 ranks
    over 5 rows: seven ranks without rows), in one process, against the integer references of tests/sharded_ref.py bit for
    bit (tests/test_sharded_ref.py shows on the CPU that every sum involved is exact in any order);
  * child_sharded_ranks.py runs dist.cg_sharded - plain, overlapped, preconditioned - and the transposed exchange
    (product_transpose + reduce_transposed) on three ranks over gloo, all on this one GPU.
Children, because torch must initialise its HIP runtime BEFORE the engine's library is loaded and this process has long
loaded the engine.  Each is started once, with a time limit, and stops at its first failed check.

What turns each check red (the first group is asserted on the CPU in test_sharded_ref.py::test_a_broken_result_differs_from_the_reference):
  q_own / the dot of product_dot     the rows or the direction slice of another rank (lo swapped for 0); any dropped or doubled term
  begin_local + finish_remote_dot    the outside part overwriting q (or adding nothing): q_out alone and q_in alone differ from
                                     q; the outside part reading one of the rank's own columns: they are all poison
  the downloaded parts of the split  the rebase dropped from the twin (col + lo != col for lo > 0); the order inside a row changed
                                     (the twin is checked entry by entry); row_begin: lo swapped for 0 in `lo - c0`
  product_transpose and its sum      one rank's partial left out; x_own read on an empty row (poison); partial_full not zeroed (NaN)
  the sweep                          the other sequence, or the block cut one row off: 1e4 times the gate away
  empty ranks                        any error raised ends the child with a nonzero exit
  cg_sharded, three ranks            a p_full read before the exchange has landed, or a slice of another rank, changes the
                                     iterates: the counts, the agreement of the ranks bit for bit, the true residual through
                                     the oracle's product; the preconditioned twin sweeps in the engine's sequence, so a
                                     block cut from the wrong rows moves the count (15 at world 3, 8 on the whole matrix)
  reduce_transposed                  split sizes taken from the row bounds under the ragged column bounds (they differ), a
                                     partial added twice or not at all: every entry of y0 + A^T x is exact
Measured on an MI355X: 24 / 25 iterations plain and overlapped at n = 6001 / 6000 (single device: 24 / 25), 15 with the block
sweep in either order (the oracle twin: 15), solutions within 6e-16 relative; each test 2 - 6 s of wall time."""
import socket
import subprocess
import sys
from pathlib import Path

import pytest

import sharded_ref as sr

pytestmark = pytest.mark.gpu
TESTS = Path(__file__).resolve().parent


@pytest.mark.parametrize("n,world", sr.OPS_CASES, ids=lambda v: str(v))
def test_every_ranks_local_operations_on_its_own_shard(n, world):
    """product_dot under four kernels, the column split and its row_begin bookkeeping, begin_local + finish_remote_dot,
    product_transpose, the block sweep in both orders, axpby and dot: rank by rank, shards built with csr_shard and with
    extract_rows, exact inputs with poison wherever nothing reads, NaN in every output beforehand"""
    r = subprocess.run([sys.executable, str(TESTS / "child_sharded_ops.py"), str(world), str(n)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and f"SHARDED_OPS_OK world={world} n={n}" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
    assert "SHARDED_OPS_FAIL" not in r.stdout
    assert "product_dot={" in r.stdout and "panel:" in r.stdout.split("product_dot={")[1].split("}")[0]


def test_three_ranks_over_gloo_on_one_gpu():
    """cg_sharded with the engine as local operations at world 3 (ragged and equal slices; plain, overlapped, preconditioned in
    both sweep orders) and the transposed exchange with CUDA tensors over gloo"""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "3", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), str(TESTS / "child_sharded_ranks.py")], capture_output=True, text=True, timeout=420)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "SHARDED_RANKS_OK world=3" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
    assert "SHARDED_RANKS_FAIL" not in r.stdout
