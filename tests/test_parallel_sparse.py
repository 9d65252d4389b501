"""The sparse sharded job's plumbing on CPU with gloo: the gather of the ranks'
pair lists (parallel.gather_pair_lists) and drep_amd.distributed.
run_sharded_sparse with oracle stand-ins for the HIP stages -- the root's list
equals the oracle's pairs with common > 0, and its Z and Cdb equal
cluster_mash_condensed of the oracle's counts bit for bit (reference chain
drep/d_cluster.py:170-185)."""
import os
import socket

import numpy as np
import pytest

S = 1000


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _list_of(rank, world):
    """Rank's list of the gather test: rank 1 holds none, the last rank many."""
    n = 0 if rank == 1 else (50_000 + rank if rank == world - 1 else 7 + rank)
    a = np.arange(n * 4, dtype=np.int64).reshape(n, 4) * (rank + 3) % 2_000_000_011
    return a.astype(np.int32)


def _gworker(rank, world, port, root, out_dir):
    import torch
    import torch.distributed as dist
    from drep_amd import parallel
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    mine = _list_of(rank, world)
    # room past n is ignored
    rec = torch.from_numpy(np.concatenate([mine, np.full((3, 4), -7, np.int32)]))
    full = parallel.gather_pair_lists(rec, len(mine), root=root)
    assert (full is not None) == (rank == root)
    if full is not None:
        np.save(os.path.join(out_dir, "full.npy"), full.numpy())
    # every list empty
    none = parallel.gather_pair_lists(torch.empty((0, 4), dtype=torch.int32), 0, root=root)
    assert (none is not None) == (rank == root) and (none is None or tuple(none.shape) == (0, 4))
    with pytest.raises(ValueError):
        parallel.gather_pair_lists(torch.empty((2, 3), dtype=torch.int32), 2, root=root)
    dist.destroy_process_group()


@pytest.mark.parametrize("world,root", [(2, 0), (3, 0), (3, 2)])
def test_gloo_gather_pair_lists(tmp_path, world, root):
    import torch.multiprocessing as mp
    mp.start_processes(_gworker, args=(world, _free_port(), root, str(tmp_path)), nprocs=world, join=True,
                       start_method="spawn")
    want = np.concatenate([_list_of(r, world) for r in range(world)])
    got = np.load(os.path.join(tmp_path, "full.npy"))
    assert got.dtype == np.int32 and np.array_equal(got, want)


def _sketches(N, how):
    import oracle
    h, nh = oracle.sketch_synth(0, N, 60_000, seed=4, family_size=5, s=S, threads=2)
    if how == "partial":                     # genomes 5, 6, 7 keep a partial sketch
        for g in (5, 6, 7):
            h[g, 100 + g:] = np.iinfo(np.uint64).max
            nh[g] = 100 + g
    else:                                    # genomes 3 and 17 have no k-mer at all
        for g in (3, 17):
            h[g, :] = np.iinfo(np.uint64).max
            nh[g] = 0
    return h, nh


def _worker_sparse(rank, world, port, N, out_dir, how):
    """One rank of run_sharded_sparse: the oracle's sketches and merge stand in
    for the HIP stages; the sharding, the all-gather, the gather of the lists
    and the root's clustering are the product code."""
    import torch
    import torch.distributed as dist
    import oracle
    from drep_amd import distributed as D
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    names = D.synthetic_names(N)
    allh, alln = _sketches(N, how)

    def sketch_fn(p):
        loc_h = torch.full((p.nmax, S), -1, dtype=torch.int64)
        loc_n = torch.zeros(p.nmax, dtype=torch.int32)
        if p.g1 > p.g0:
            loc_h[:p.g1 - p.g0] = torch.from_numpy(allh[p.g0:p.g1].view(np.int64).copy())
            loc_n[:p.g1 - p.g0] = torch.from_numpy(alln[p.g0:p.g1].view(np.int32).copy())
        return loc_h, loc_n

    def sparse_fn(H, NH, p):
        if not p.seg_len:
            return torch.empty((0, 4), dtype=torch.int32), 0
        Hn, Nn = H.numpy().view(np.uint64), NH.numpy().view(np.uint32)
        r1 = min(p.r1, N - 1)
        c, d = oracle.allpairs(Hn, Nn, S, r0=p.r0, r1=r1, threads=1)
        c, d = c[:p.seg_len], d[:p.seg_len]
        i = np.concatenate([np.full(N - 1 - r, r) for r in range(p.r0, r1)])
        j = np.concatenate([np.arange(r + 1, N) for r in range(p.r0, r1)])
        k = c > 0
        rec = np.stack([i[k], j[k], c[k].astype(np.int64), d[k].astype(np.int64)], axis=1).astype(np.int32)
        return torch.from_numpy(rec), int(k.sum())

    res = D.run_sharded_sparse(N, names, S, sketch_fn, sparse_fn, "average", 0.9)
    assert set(res["times"]) >= {"sketch_s", "allgather_s", "allpairs_s", "gather_pairs_s"}
    if rank == 0:
        assert "common" not in res and "denom" not in res            # no condensed tensor
        np.save(os.path.join(out_dir, "Z.npy"), res["linkage"])
        np.save(os.path.join(out_dir, "pairs.npy"), res["pairs"].numpy())
        res["Cdb"].to_csv(os.path.join(out_dir, "Cdb.csv"), index=False)
    else:
        assert "Cdb" not in res
    dist.destroy_process_group()


@pytest.mark.parametrize("world,how", [(2, "partial"), (3, "partial"), (3, "empty")])
def test_gloo_sparse_sharded_clustering_matches_condensed(tmp_path, world, how):
    import pandas as pd
    import torch.multiprocessing as mp
    import oracle
    from drep_amd import distributed as D
    from drep_amd.d_cluster import CondensedMash, cluster_mash_condensed
    N = 29
    mp.start_processes(_worker_sparse, args=(world, _free_port(), N, str(tmp_path), how), nprocs=world, join=True,
                       start_method="spawn")
    h, nh = _sketches(N, how)
    want_c, want_d = oracle.allpairs(h, nh, S)
    ii, jj = np.triu_indices(N, 1)
    k = want_c > 0
    want = np.stack([ii[k], jj[k], want_c[k].astype(np.int64), want_d[k].astype(np.int64)], axis=1).astype(np.int32)
    assert len(want) > N and (want_d[k] < S).any() == (how == "partial")
    assert np.array_equal(np.load(os.path.join(tmp_path, "pairs.npy")), want)
    names = D.synthetic_names(N)
    cm = CondensedMash(names, names, want_c, want_d, nh, np.zeros(N, np.uint64), S)
    cdb, (Z, _, _) = cluster_mash_condensed(cm, clusterAlg="average", P_ani=0.9, gpu=None)
    assert np.array_equal(np.load(os.path.join(tmp_path, "Z.npy")), Z)
    got = pd.read_csv(os.path.join(tmp_path, "Cdb.csv"))
    assert got["genome"].tolist() == cdb["genome"].tolist()
    assert got["primary_cluster"].tolist() == cdb["primary_cluster"].tolist()
    assert cdb["primary_cluster"].nunique() > 1
