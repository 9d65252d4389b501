"""The sparse sharded job (python -m drep_amd.distributed --sparse under
torch.distributed.run) rehearsed on one MI355X: 1, 3 and 8 ranks share the GPU
over gloo, the shared-hash screen forced on, and the root's stored pair list,
linkage and primary Cdb must equal the dense one-rank job's: the list is the
non-zero part of its condensed counts, Z and Cdb are the same bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

from drep_amd.store import load_condensed, load_primary_linkage, load_sparse

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, L = 240, 300_000


def _run(world, out, port, sparse):
    """One launch under its own time limit (as tests/test_gpu_dist.py::_run)."""
    env = dict(os.environ, DREPHIP_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1", DREPHIP_AP_SCREEN="1")
    if not sparse:
        env["DREPHIP_SEGMENT_POISON"] = "1"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
           "--master-addr", "127.0.0.1", "--master-port", str(port), "-m", "drep_amd.distributed",
           "--genomes", str(N), "--genome-bp", str(L), "--family-size", "20", "--sketch", "1000",
           "--out", out] + (["--sparse"] if sparse else [])
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])


@pytest.mark.timeout(900)
def test_sparse_sharded_job_matches_dense(tmp_path):
    dense = _run(1, str(tmp_path / "dense"), 29811, sparse=False)
    assert dense["n_gpus"] == 1 and "sparse" not in dense
    cm = load_condensed(str(tmp_path / "dense"), mmap=False)
    pl = load_primary_linkage(str(tmp_path / "dense"))
    cdb = pd.read_csv(tmp_path / "dense" / "primary_Cdb.csv")
    ii, jj = np.triu_indices(N, 1)
    k = np.asarray(cm.common) > 0
    want = (ii[k].astype(np.uint32), jj[k].astype(np.uint32), np.asarray(cm.common)[k], np.asarray(cm.denom)[k])
    assert N < k.sum() < len(k) and dense["primary_clusters"] > 1
    for world, port in ((1, 29821), (3, 29831), (8, 29841)):
        d = str(tmp_path / ("s%d" % world))
        res = _run(world, d, port, sparse=True)
        assert res["n_gpus"] == world and res["sparse"] is True and res["pairs_listed"] == int(k.sum())
        assert "gather_pairs_s" in res["times"] and "gather_segments_s" not in res["times"]
        assert not os.path.exists(os.path.join(d, "MASH_files", "condensed"))
        sm = load_sparse(d, mmap=False)
        for name, g, e in zip(("i", "j", "common", "denom"), (sm.i, sm.j, sm.common, sm.denom), want):
            assert np.array_equal(np.asarray(g), e), (world, name)
        assert np.array_equal(sm.nhash, cm.nhash)
        assert np.array_equal(load_primary_linkage(d)["linkage"], pl["linkage"]), world
        assert pd.read_csv(os.path.join(d, "primary_Cdb.csv")).equals(cdb), world
        ranks = res["ranks"]
        assert [r["rank"] for r in ranks] == list(range(world))
        assert sum(r["pairs"] for r in ranks) == res["pairs_listed"]
        for r in ranks:
            if r["rows"][0] < min(r["rows"][1], N - 1):                 # a rank with rows
                st = r["sparse_stats"]
                assert st["direct"] > 0 and st["fallback"] == 0 and st["direct"] == r["pairs"], (world, r)
                assert st["blocks"] >= 1 and r["screen_used"]
            assert r["peak_device_bytes"] >= r["sparse_stats"]["scratch_bytes"] > 0
