"""Ward's method on the dense GPU chain (drephip_linkage*, method 5): Z equal
to scipy.cluster.hierarchy.linkage(y, "ward") bit for bit at every grid
variant of the chain-step kernel, the paths it may and may not take, the
refusal of negative distances, and the counts path of cluster_mash_condensed."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.cluster.hierarchy as sch
from scipy.spatial.distance import squareform

import oracle
from drep_amd import _lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 1000


def ward_input(kind, n):
    """The input kinds of tests/test_gpu.py::test_gpu_linkage_matches_scipy."""
    rng = np.random.default_rng(n * 31 + 4)
    m = n * (n - 1) // 2
    if kind == "ties":
        vals = np.array([0.0, 0.00243596, 0.0157245, 0.0157245, 0.05, 0.1, 0.243761, 1.0, 1.0, 1.0])
        return vals[rng.integers(0, len(vals), m)]
    if kind == "cont":
        return rng.random(m)
    if kind == "fewvals":
        return np.array([0.1, 0.3, 0.7])[rng.integers(0, 3, m)]
    if kind == "mash":
        fam = rng.integers(0, max(1, n // 40), n)
        iu = np.triu_indices(n, 1)
        same = fam[iu[0]] == fam[iu[1]]
        y = np.ones(m)
        y[same] = np.round(rng.random(int(same.sum())) * 0.2, 3)
        return y
    if kind == "above1":
        return rng.random(m) * 1.5
    if kind == "negative":
        return rng.random(m) - 0.3
    if kind == "zero":
        return np.zeros(m)
    return np.full(m, 0.5)                                   # equal


def run_dense(y, env, per_lane=None):
    if per_lane is not None:
        os.environ["DREPHIP_LINK_PER_LANE"] = per_lane
    os.environ.update(env)
    try:
        with _lib.Context(0, 21, S, 42) as ctx:
            ctx.set_linkage_path(ctx.LINK_DENSE)
            Z = ctx.linkage(y, "ward")
            assert not ctx.linkage_info()["sparse"]
            assert ctx.linkage_launches() >= len(Z)
    finally:
        for k in ["DREPHIP_LINK_PER_LANE"] + list(env):
            os.environ.pop(k, None)
    return Z


@pytest.mark.parametrize("n,kind", [(2, "ties"), (3, "ties"), (17, "ties"), (257, "ties"), (2100, "ties"),
                                    (300, "cont"), (64, "equal"), (400, "fewvals"), (1500, "mash"), (700, "above1"),
                                    (300, "zero"), (4500, "mash")])
def test_gpu_ward_matches_scipy(n, kind):
    """Bit identity with scipy at the variants of the existing linkage test:
    the default grid (one-wave workgroups), 128/256-lane workgroups at 1, 4 and
    16 entries per lane, one-wave workgroups at 2 and 8, compactions down to 4
    active clusters with short graph batches polled after each, and the
    speculation on (default), without the known-merge launches, and off.  The
    n = 4500 case (the one-wave grid spans several passes) runs the default
    variant only."""
    y = ward_input(kind, n)
    Zs = sch.linkage(y, method="ward")
    assert not np.isnan(Zs).any()
    variants = [(None, {})]
    if n < 4500:
        variants += [("4", {}), ("1", {}), ("16", {}), ("2", {"DREPHIP_LINK_WG": "64"}),
                     ("8", {"DREPHIP_LINK_WG": "64"}), (None, {"DREPHIP_LINK_WG": "512"}),
                     (None, {"DREPHIP_LINK_SPEC": "0"}), (None, {"DREPHIP_LINK_SPEC": "1"}),
                     (None, {"DREPHIP_LINK_COMPACT_MIN": "4", "DREPHIP_LINK_BATCH": "16", "DREPHIP_LINK_POLL": "1"}),
                     (None, {"DREPHIP_LINK_COMPACT_MIN": "4", "DREPHIP_LINK_BATCH": "6", "DREPHIP_LINK_POLL": "1"}),
                     ("2", {"DREPHIP_LINK_COMPACT_MIN": "4", "DREPHIP_LINK_BATCH": "10", "DREPHIP_LINK_POLL": "1"})]
    for per_lane, env in variants:
        Z = run_dense(y, env, per_lane)
        assert Z.shape == Zs.shape
        assert np.array_equal(Z, Zs), (per_lane, env, np.argwhere(Z != Zs)[:5])


def test_gpu_ward_paths():
    """Ward has no sparse form: the automatic choice takes the dense chain even
    where every other method would go sparse (mash), and a forced sparse path is
    refused."""
    y = ward_input("mash", 1500)
    Zs = sch.linkage(y, method="ward")
    with _lib.Context(0, 21, S, 42) as ctx:
        Z = ctx.linkage(y, "average")
        assert ctx.linkage_info()["sparse"]                  # (the input does have a sparse form)
        Z = ctx.linkage(y, "ward")
        assert not ctx.linkage_info()["sparse"]
        assert np.array_equal(Z, Zs)
        ctx.set_linkage_path(ctx.LINK_SPARSE)
        with pytest.raises(_lib.DrepHipError, match="sparse"):
            ctx.linkage(y, "ward")
        ctx.set_linkage_path(ctx.LINK_AUTO)
        M = squareform(y).astype(np.float32)
        assert np.array_equal(ctx.linkage_square(M, "ward"), sch.linkage(squareform(M.astype(np.float64)), "ward"))


def test_gpu_ward_refuses_negative_distances():
    """scipy's ward gives NaN rows on negative distances; the GPU refuses them
    (found by the kernels that build the matrix), and the drop-in
    cluster_mash_database falls back to scipy, NaNs included."""
    import pandas as pd
    from drep_amd.d_cluster import cluster_mash_database
    n = 300
    y = ward_input("negative", n)
    assert (y < 0).any()
    M = squareform(y).astype(np.float32)
    with _lib.Context(0, 21, S, 42) as ctx:
        with pytest.raises(_lib.DrepHipError, match="distances >= 0"):
            ctx.linkage(y, "ward")
        with pytest.raises(_lib.DrepHipError, match="distances >= 0"):
            ctx.linkage_square(M, "ward")
        ctx.set_linkage_path(ctx.LINK_DENSE)
        with pytest.raises(_lib.DrepHipError, match="distances >= 0"):
            ctx.linkage(y, "ward")
        # (the other methods take negative values, as scipy does)
        assert np.array_equal(ctx.linkage(y, "average"), sch.linkage(y, "average"))
        assert np.array_equal(ctx.linkage_square(M, "complete"),
                              sch.linkage(squareform(M.astype(np.float64)), "complete"))
    # the drop-in on the same values: dist = 1 - similarity in float32, as the reference computes it
    names = ["g%03d.fa" % i for i in range(n)]
    g1, g2 = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    sim = (np.float32(1) - M).astype(np.float32)
    db = pd.DataFrame({"genome1": np.array(names)[g1.ravel()], "genome2": np.array(names)[g2.ravel()],
                       "similarity": sim.ravel()})
    # The linkage step of the drop-in returns scipy's Z, NaNs included.  (The
    # whole cluster_mash_database cannot return it: Z's first merges are at the
    # negative distances themselves, and scipy's fcluster, the next step of
    # the reference too, refuses a Z with negative distances -- so the drop-in
    # must raise what the reference path raises.)
    from drep_amd.d_cluster import _square_linkage
    z_ref = sch.linkage(squareform(M.astype(np.float64)), method="ward")
    assert np.isnan(z_ref).any()
    for MM in (M, M.astype(np.float64)):                   # drephip_linkage_square, squareform + drephip_linkage
        z_gpu = _square_linkage(MM, "ward", 0)
        assert np.array_equal(z_gpu, z_ref, equal_nan=True)
    errs = []
    for gpu in (None, 0):
        with pytest.raises(ValueError) as e:
            cluster_mash_database(db.copy(), clusterAlg="ward", P_ani=0.9, gpu=gpu)
        errs.append(str(e.value))
    assert errs[0] == errs[1] and "negative distances" in errs[0]


def test_cluster_mash_database_ward_gpu_equals_host():
    """The drop-in on an Mdb-shaped table: ward on the GPU gives the host
    path's Z, linkage_db and Cdb."""
    import pandas as pd
    from drep_amd.d_cluster import cluster_mash_database
    n = 300
    M = squareform(ward_input("mash", n)).astype(np.float32)
    names = np.array(["g%03d.fa" % i for i in range(n)])
    g1, g2 = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    db = pd.DataFrame({"genome1": names[g1.ravel()], "genome2": names[g2.ravel()],
                       "similarity": (np.float32(1) - M).ravel()})
    cdb_cpu, (z_cpu, ldb_cpu, _) = cluster_mash_database(db.copy(), clusterAlg="ward", P_ani=0.9, gpu=None)
    cdb_gpu, (z_gpu, ldb_gpu, _) = cluster_mash_database(db.copy(), clusterAlg="ward", P_ani=0.9, gpu=0)
    assert np.array_equal(z_gpu, z_cpu) and ldb_gpu.equals(ldb_cpu) and cdb_gpu.equals(cdb_cpu)
    assert cdb_gpu["primary_cluster"].nunique() > 1


def test_gpu_ward_refuses_negative_table_value(ctx1000):
    """The counts form: a negative value in the distance table is refused for
    ward by the matrix build, and taken by the other methods."""
    import torch
    from drep_amd.d_cluster import linkage_tables
    n = 40
    rng = np.random.default_rng(3)
    common = rng.integers(1, 900, n * (n - 1) // 2).astype(np.uint16)
    common[5] = 7
    d_c = torch.from_numpy(common.view(np.int16)).cuda()
    perm = np.arange(n, dtype=np.uint32)
    lut, off = linkage_tables(np.array([S]), S)
    st = torch.cuda.current_stream().cuda_stream
    ctx1000.set_linkage_path(ctx1000.LINK_AUTO)
    Z = ctx1000.linkage_counts_device(d_c.data_ptr(), None, n, perm, lut, off, "ward", st)
    assert np.array_equal(Z, sch.linkage(lut[common], "ward"))
    bad = lut.copy()
    bad[off[S] + 7] = -0.25
    with pytest.raises(_lib.DrepHipError, match="distances >= 0"):
        ctx1000.linkage_counts_device(d_c.data_ptr(), None, n, perm, bad, off, "ward", st)
    ctx1000.set_linkage_path(ctx1000.LINK_DENSE)
    Z = ctx1000.linkage_counts_device(d_c.data_ptr(), None, n, perm, bad, off, "average", st)
    ctx1000.set_linkage_path(ctx1000.LINK_AUTO)
    assert np.array_equal(Z, sch.linkage(bad[common], "average"))


@pytest.fixture(scope="module")
def family():
    return oracle.sketch_synth(0, 160, 400_000, seed=5, family_size=20, threads=8)


def test_cluster_mash_condensed_ward_runs_on_the_gpu(family, ctx1000, monkeypatch):
    """cluster_mash_condensed sends ward to the GPU chain (it used to fall back
    to host scipy silently): the reference path's Z and Cdb, names shuffled, and
    a launch count that proves the chain ran."""
    from drep_amd import d_cluster
    from drep_amd.d_cluster import CondensedMash, cluster_mash_condensed
    h, nh = family
    N = len(nh)
    c, d = ctx1000.allpairs(h, nh)
    rng = np.random.default_rng(5)
    names = ["g%04d.fna" % i for i in rng.permutation(N)]
    cm = CondensedMash(names, names, c, d, nh, np.full(N, 400_000, np.uint64), S)
    launches = []

    class Counting(_lib.Context):
        def close(self):
            if getattr(self, "_h", None):
                launches.append(self.linkage_launches())
            super().close()

    cdb_cpu, (z_cpu, _, _) = cluster_mash_condensed(cm, clusterAlg="ward", P_ani=0.95, gpu=None)
    monkeypatch.setattr(d_cluster._lib, "Context", Counting)
    cdb_gpu, (z_gpu, _, _) = cluster_mash_condensed(cm, clusterAlg="ward", P_ani=0.95, gpu=0)
    assert launches and launches[-1] >= N - 1
    assert np.array_equal(z_gpu, z_cpu)
    assert cdb_gpu.equals(cdb_cpu)
    assert cdb_gpu["primary_cluster"].nunique() > 1


def test_gpu_ward_compaction_runs(capfd, monkeypatch):
    """As test_gpu_linkage_compaction_runs: the matrix is compacted while the
    ward chain runs, not with DREPHIP_LINK_COMPACT=0, and Z is scipy's both times."""
    n = 3000
    rng = np.random.default_rng(7)
    fam = rng.integers(0, 60, n)
    iu = np.triu_indices(n, 1)
    y = np.where(fam[iu[0]] == fam[iu[1]], np.round(rng.random(len(iu[0])) * 0.2, 3), 1.0)
    Zs = sch.linkage(y, method="ward")
    monkeypatch.setenv("DREPHIP_DEBUG", "1")
    monkeypatch.setenv("DREPHIP_LINK_BATCH", "32")
    monkeypatch.setenv("DREPHIP_LINK_POLL", "1")
    monkeypatch.setenv("DREPHIP_LINK_COMPACT_MIN", "100")
    capfd.readouterr()
    with _lib.Context(0, 21, S, 42) as ctx:
        ctx.set_linkage_path(ctx.LINK_DENSE)
        Z = ctx.linkage(y, "ward")
    err = capfd.readouterr().err
    assert int(re.search(r"compactions (\d+)", err).group(1)) >= 1, err[-500:]
    assert np.array_equal(Z, Zs), np.argwhere(Z != Zs)[:5]
    monkeypatch.setenv("DREPHIP_LINK_COMPACT", "0")
    capfd.readouterr()
    with _lib.Context(0, 21, S, 42) as ctx:
        ctx.set_linkage_path(ctx.LINK_DENSE)
        Z = ctx.linkage(y, "ward")
    assert "compactions 0" in capfd.readouterr().err
    assert np.array_equal(Z, Zs)


@pytest.mark.parametrize("order", ["even", "odd"])
def test_ward_adverse_workgroup_order(order):
    """tools/linkage_adverse.py on ward alone, under the builds whose even (odd)
    workgroups sleep before their loads (tests/test_gpu.py::
    test_linkage_adverse_workgroup_order): ward's further operands -- D[x][y],
    D[A][B], the sizes of A, B, W -- must be the previous launch's too."""
    lib = os.path.join(ROOT, "drep_amd", "lib_ab", "adverse_" + order, "libdrephip.so")
    if not os.path.exists(lib):
        pytest.skip("adverse-order build missing (run __graft_entry__.build())")
    env = dict(os.environ, DREPHIP_LIB=lib, DREPHIP_LINK_BATCH="32", DREPHIP_LINK_POLL="1",
               DREPHIP_LINK_COMPACT_MIN="100")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "linkage_adverse.py"), "ward"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert "DREPHIP_LK_ADVERSE=%d" % (1 if order == "even" else 2) in res["build"].get("extra", "")
    assert [(c["n"], c["method"], c["wg"]) for c in res["cases"]] == \
        [(300, "ward", "64"), (300, "ward", "256"), (3000, "ward", "64"), (3000, "ward", "256")]
    bad = [c for c in res["cases"] if not c["equal"]]
    assert not bad, bad
