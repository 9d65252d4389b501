"""Ward's method in the host model of the GPU chain's launch protocol
(tools/chain_sim.py), and the places that must keep refusing it: ward has no
sparse form.  No GPU."""
import os
import sys

import numpy as np
import pytest
import scipy.cluster.hierarchy as sch
from scipy.spatial.distance import squareform

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import chain_sim  # noqa: E402


def ward_input(kind, n, seed=0):
    """Condensed distances of the kinds tests/test_gpu.py's linkage test uses."""
    rng = np.random.default_rng(n * 31 + seed)
    m = n * (n - 1) // 2
    if kind == "ties":
        vals = np.array([0.0, 0.00243596, 0.0157245, 0.0157245, 0.05, 0.1, 0.243761, 1.0, 1.0, 1.0])
        return vals[rng.integers(0, len(vals), m)]
    if kind == "fewvals":
        return np.array([0.1, 0.3, 0.7])[rng.integers(0, 3, m)]
    if kind == "mash":
        fam = rng.integers(0, max(1, n // 40), n)
        iu = np.triu_indices(n, 1)
        same = fam[iu[0]] == fam[iu[1]]
        y = np.ones(m)
        y[same] = np.round(rng.random(int(same.sum())) * 0.2, 3)
        return y
    if kind == "equal":
        return np.full(m, 0.5)
    if kind == "zero":
        return np.zeros(m)
    raise ValueError(kind)


@pytest.mark.parametrize("policy", ["r4", "r5"])
@pytest.mark.parametrize("kind,n", [("ties", 17), ("ties", 257), ("mash", 300), ("fewvals", 200), ("equal", 64),
                                    ("zero", 50)])
def test_chain_sim_ward_equals_scipy(kind, n, policy):
    """The launch protocol with ward's update -- ni, the other cluster's size,
    and dxy, the merged (or speculated) pair's distance, handed to Sim.lw --
    gives scipy's Z bit for bit, under both speculation policies."""
    y = ward_input(kind, n)
    Zs = sch.linkage(y, "ward")
    assert not np.isnan(Zs).any()
    sim = chain_sim.Sim(squareform(y).astype(np.float64), policy=policy, method="ward")
    Z = sim.run()
    assert Z.shape == Zs.shape
    assert np.array_equal(Z, Zs), np.argwhere(Z != Zs)[:5]
    assert sim.stats["launches"] >= n - 1


def test_chain_sim_refuses_unknown_method():
    D = squareform(ward_input("ties", 5))
    with pytest.raises(ValueError, match="method"):
        chain_sim.Sim(D, method="centroid").run()


def test_chain_sim_other_methods_unchanged():
    """complete / average / weighted ignore ward's two further operands."""
    y = ward_input("ties", 65)
    for method in ("complete", "average", "weighted"):
        Z = chain_sim.Sim(squareform(y).astype(np.float64), policy="r5", method=method).run()
        assert np.array_equal(Z, sch.linkage(y, method)), method


def test_sparse_forms_refuse_ward():
    from drep_amd import _lib
    from drep_amd.d_cluster import (GPU_DENSE_LINKAGE_METHODS, GPU_LINKAGE_METHODS, SparseMash,
                                    cluster_mash_sparse)
    assert "ward" in GPU_DENSE_LINKAGE_METHODS and "ward" not in GPU_LINKAGE_METHODS
    assert _lib.DENSE_LINK_METHODS["ward"] == 5 and "ward" not in _lib.LINK_METHODS
    with pytest.raises(KeyError):
        _lib.linkage_sparse(4, [0], [1], [0.5], "ward")
    sm = SparseMash(names=["a", "b", "c"], locations=["a", "b", "c"], i=np.array([0], np.uint32),
                    j=np.array([1], np.uint32), common=np.array([500], np.uint16), denom=np.array([1000], np.uint16),
                    nhash=np.full(3, 1000, np.uint32), length=np.full(3, 10 ** 6, np.uint64), s=1000)
    with pytest.raises(ValueError, match="clusterAlg"):
        cluster_mash_sparse(sm, clusterAlg="ward", P_ani=0.9)


def test_c_api_refuses_ward_without_a_sparse_form():
    """drephip_linkage_sparse (host only) refuses ward, saying why; the other
    refused codes keep the pinned sentence."""
    from drep_amd import _lib
    lib = _lib.lib()
    i, j, v = np.array([0], np.uint32), np.array([1], np.uint32), np.array([0.5])
    Z = np.zeros(12)
    assert lib.drephip_linkage_sparse(4, 1, i, j, v, 5, Z) != 0
    assert "ward has no sparse form" in lib.drephip_last_error().decode()
    assert lib.drephip_linkage_sparse(4, 1, i, j, v, 3, Z) != 0
    assert "linkage method must be single, complete, average or weighted" in lib.drephip_last_error().decode()


def test_distributed_parser_refuses_sparse_ward(capsys):
    from drep_amd import distributed
    a = distributed.parse_args(["--method", "ward", "--genomes", "10"])
    assert a.method == "ward" and not a.sparse
    assert distributed.parse_args(["--sparse", "--method", "average"]).sparse
    with pytest.raises(SystemExit) as e:
        distributed.parse_args(["--sparse", "--method", "ward"])
    assert e.value.code == 2
    assert "ward has no sparse form" in capsys.readouterr().err
