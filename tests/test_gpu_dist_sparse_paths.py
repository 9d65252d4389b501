"""The other routes of the sparse sharded job's all-pairs stage
(distributed.allpairs_sparse_rows_sharded), 3 gloo ranks sharing one MI355X:
the sharded screen's dense verdict (the plain sparse call with the screen off:
the compaction fallback) and DREPHIP_SCREEN_SHARD=0 (every rank groups all
entries itself: the plain sparse call, direct).  The stored list must equal the
oracle's pairs with common > 0 of the oracle's sketches."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from drep_amd.store import load_sparse

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, L = 240, 300_000


def _run(world, out, port, **extra):
    # auto mode screens from 100 genomes on, so that the verdict is taken at this N
    env = dict(os.environ, DREPHIP_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1", DREPHIP_SCREEN_MIN_N="100", **extra)
    env.pop("DREPHIP_AP_SCREEN", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
           "--master-addr", "127.0.0.1", "--master-port", str(port), "-m", "drep_amd.distributed",
           "--genomes", str(N), "--genome-bp", str(L), "--family-size", "20", "--sketch", "1000",
           "--out", out, "--sparse"]
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])


@pytest.mark.timeout(700)
def test_sparse_sharded_job_dense_verdict_and_unsharded_screen(tmp_path):
    h, nh = oracle.sketch_synth(0, N, L, seed=0xD2E9, family_size=20, threads=8)
    oc, od = oracle.allpairs(h, nh, 1000, threads=8)
    ii, jj = np.triu_indices(N, 1)
    k = oc > 0
    want = (ii[k].astype(np.uint32), jj[k].astype(np.uint32), oc[k], od[k])
    # a pair check priced at 10^9 probes: every set is "dense"
    for name, port, extra, route in (("verdict", 29851, {"DREPHIP_SCREEN_RATIO": "1e9"}, "fallback"),
                                     ("flat", 29861, {"DREPHIP_SCREEN_SHARD": "0"}, "direct")):
        d = str(tmp_path / name)
        res = _run(3, d, port, **extra)
        assert res["n_gpus"] == 3 and res["sparse"] is True and res["pairs_listed"] == int(k.sum())
        sm = load_sparse(d, mmap=False)
        assert np.array_equal(sm.nhash, nh)
        for what, g, e in zip(("i", "j", "common", "denom"), (sm.i, sm.j, sm.common, sm.denom), want):
            assert np.array_equal(np.asarray(g), e), (name, what)
        other = "direct" if route == "fallback" else "fallback"
        for r in res["ranks"]:
            st = r["sparse_stats"]
            assert st[route] == r["pairs"] > 0 and st[other] == 0, (name, r)
            assert r["screen_used"] == (route == "direct")
