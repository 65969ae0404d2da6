"""Spectral clustering without a GPU: the file format of umhsnerf/cluster.py and its refusals, k-means++ on the host, the Lloyd update,
and the float64 Lloyd helper of tests/cluster_f64.py that the GPU test is judged against."""
import numpy as np
import pytest
import torch

import cluster_f64 as CF

WL = [400.0 + 10.0 * i for i in range(8)]


def _clusters(metric="angle", K=3):
    from umhsnerf.cluster import SpectralClusters

    rng = np.random.default_rng(4)
    return SpectralClusters(rng.random((K, 8)) + 0.1, metric, WL, counts=np.arange(K) * 10, objective=1.25)


@pytest.mark.parametrize("metric", ["angle", "euclidean"])
def test_file_round_trip_and_the_same_clusters_give_the_same_bytes(metric, tmp_path):
    from umhsnerf.cluster import SpectralClusters

    c = _clusters(metric)
    c.save(tmp_path / "a.npz")
    c.save(tmp_path / "b.npz")
    assert (tmp_path / "a.npz").read_bytes() == (tmp_path / "b.npz").read_bytes()
    with np.load(tmp_path / "a.npz", allow_pickle=False) as f:
        assert sorted(f.files) == ["colors", "counts", "metric", "names", "objective", "spectra", "wavelengths"]
        assert [str(n) for n in f["names"]] == ["cluster_0", "cluster_1", "cluster_2"] and str(f["metric"]) == metric
    back = SpectralClusters.load(tmp_path / "a.npz", WL)
    assert np.array_equal(back.centres, c.centres) and back.metric == metric and back.wavelengths == WL
    assert np.array_equal(back.counts, c.counts) and np.array_equal(back.colors, c.colors) and back.objective == 1.25
    assert len(back) == 3 and back.bands == 8
    # what the kernel takes: unit rows rounded once, or the centres rounded once
    d = back.device_centres()
    assert d.dtype == torch.float32 and tuple(d.shape) == (3, 8)
    if metric == "angle":
        assert bool(((d.double().norm(dim=1) - 1).abs() < 1e-6).all())
    else:
        assert torch.equal(d, torch.from_numpy(c.centres).float())


def test_default_colours_are_the_class_palette_and_an_angle_file_loads_as_a_spectral_library(tmp_path):
    from umhsnerf.library import SpectralLibrary
    from umhsnerf.umhs_model import CLASS_COLORS

    c = _clusters("angle", K=17)
    palette = CLASS_COLORS.numpy()
    assert np.array_equal(c.colors, palette[np.arange(17) % len(palette)])
    c.save(tmp_path / "angle.npz")
    lib = SpectralLibrary.load(tmp_path / "angle.npz", WL)
    assert lib.names == c.names and np.array_equal(lib.spectra, c.centres) and np.array_equal(lib.colors, c.colors)
    assert torch.equal(lib.unit(), c.device_centres())


def test_refusals(tmp_path):
    from umhsnerf import cluster
    from umhsnerf.cluster import SpectralClusters

    c = _clusters()
    c.save(tmp_path / "c.npz")
    with pytest.raises(ValueError, match="bands"):
        SpectralClusters.load(tmp_path / "c.npz", WL[:-1])
    with pytest.raises(ValueError, match="wavelengths are not the scene's"):
        SpectralClusters.load(tmp_path / "c.npz", [w + 1.0 for w in WL])
    np.savez(tmp_path / "short.npz", spectra=c.centres)
    with pytest.raises(ValueError, match="no array named"):
        SpectralClusters.load(tmp_path / "short.npz", WL)
    with pytest.raises(ValueError, match="1..64 clusters"):
        SpectralClusters(np.ones((65, 8)), "angle", WL)
    with pytest.raises(ValueError, match="1..256 bands"):
        SpectralClusters(np.ones((3, 257)), "angle", list(range(257)))
    with pytest.raises(ValueError, match="metric"):
        SpectralClusters(np.ones((3, 8)), "manhattan", WL)
    with pytest.raises(ValueError, match="finite"):
        SpectralClusters(np.zeros((3, 8)), "angle", WL)
    frames = [torch.rand(50, 8)]
    with pytest.raises(ValueError, match="1..64"):
        cluster.fit(frames, 65, "angle")
    with pytest.raises(ValueError, match="metric"):
        cluster.fit(frames, 3, "manhattan")
    with pytest.raises(ValueError, match="the model has 5 endmembers, --clusters asks for 3"):
        cluster.fit(frames, 3, "angle", "endmembers", endmembers=torch.rand(5, 8))
    with pytest.raises(ValueError, match="needs the model's learnt endmembers"):
        cluster.fit(frames, 3, "angle", "endmembers")
    with pytest.raises(ValueError, match="init must be"):
        cluster.fit(frames, 3, "angle", "random")
    with pytest.raises(ValueError, match=r"\[K,B\]"):
        cluster.fit(frames, 3, "angle", np.ones((4, 8)))
    with pytest.raises(ValueError, match="cluster outputs need fitted clusters; pass --clusters FILE"):
        cluster.requested_without_clusters(["rgb", "cluster_pred"], None)
    cluster.requested_without_clusters(["rgb", "cluster_pred"], "c.npz")
    cluster.requested_without_clusters(["rgb"], None)


@pytest.mark.parametrize("metric", ["angle", "euclidean"])
def test_kmeanspp_is_deterministic_per_seed_and_draws_rows_of_the_subsample(metric):
    from umhsnerf import cluster

    data = CF.planted(4000, 8, 3, metric)
    frames = [(data["frames"][0], None), (data["frames"][1], torch.ones(data["frames"][1].shape[0])), data["frames"][2]]
    rows = cluster.subsample(frames, seed=5)
    assert rows.dtype == np.float64 and rows.shape == (4000, 8) and np.array_equal(rows, data["x"].double().numpy())
    few = cluster.subsample(frames, seed=5, limit=300)
    assert few.shape == (300, 8) and np.array_equal(few, cluster.subsample(frames, seed=5, limit=300))
    assert not np.array_equal(few, cluster.subsample(frames, seed=6, limit=300))
    # rows that are empty, not finite or masked out are never drawn
    x = data["frames"][0].clone()
    x[0], x[1, 3], x[2, 0] = 0.0, float("nan"), float("inf")
    mask = torch.ones(x.shape[0])
    mask[3] = 0.5
    assert np.array_equal(cluster.subsample([(x, mask)], seed=0), x[4:].double().numpy())
    a, b = cluster.kmeanspp(rows, 3, metric, seed=1), cluster.kmeanspp(rows, 3, metric, seed=1)
    assert np.array_equal(a, b) and a.shape == (3, 8)
    assert not np.array_equal(a, cluster.kmeanspp(rows, 3, metric, seed=2))
    assert all((rows == c).all(1).any() for c in a)
    # D^2 sampling puts the three centres into the three planted clusters far more often than uniform draws would (2 in 9)
    hits = 0
    for seed in range(20):
        c = cluster.kmeanspp(rows, 3, metric, seed)
        truth = {int(data["truth"][int(np.nonzero((rows == row).all(1))[0][0])]) for row in c}
        hits += len(truth) == 3
    assert hits >= 15, hits


@pytest.mark.parametrize("metric", ["angle", "euclidean"])
def test_the_update_keeps_the_centre_of_an_empty_cluster(metric):
    from umhsnerf import cluster

    centres = np.array([[1.0, 0.0], [0.0, 1.0], [3.0, 4.0]])
    acc = np.array([5.0, 0.1, 2.0, 0.0, 3.0, 2.0, 2.0, 0.0, 0.0, 3.0, 6.0])
    new, empty = cluster.update(centres, acc, metric)
    assert empty == 1 and np.array_equal(new[1], centres[1])
    want = [[2.0, 2.0], [3.0, 6.0]]
    for got, s, n in zip(new[[0, 2]], want, (2.0, 3.0)):
        np.testing.assert_allclose(got, np.asarray(s) / (np.linalg.norm(s) if metric == "angle" else n), rtol=1e-15)
    mine, _ = CF.update_centres(torch.from_numpy(centres), torch.from_numpy(acc), 3, 2, metric)
    assert np.array_equal(mine.numpy(), new)


@pytest.mark.parametrize("metric", ["angle", "euclidean"])
def test_the_float64_lloyd_helper_is_monotone_and_recovers_the_planted_partition(metric):
    from umhsnerf import cluster

    shape = (4000, 8, 3)
    data = CF.planted(*shape, metric)
    seed = CF.FIT_CASES[shape][metric]
    init = torch.from_numpy(cluster.kmeanspp(cluster.subsample(data["frames"], seed), 3, metric, seed))
    run = CF.lloyd(data["frames"], init, metric, torch.float64)
    o = run["objective"]
    assert len(o) >= 2 and all(b <= a for a, b in zip(o[:-1], o[1:])), o
    assert CF.partition_agreement(run["labels"], data["truth"], 3) >= 0.99
    # from a poor start too: rows of one planted cluster only
    poor = data["x"][data["truth"] == 0][:3].double()
    slow = CF.lloyd(data["frames"], poor, metric, torch.float64, tolerance=0.0)["objective"]
    assert len(slow) >= 3 and all(b <= a * (1 + 1e-12) for a, b in zip(slow[:-1], slow[1:])), slow
