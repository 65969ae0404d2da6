"""Spectral clustering on the GPU: csrc/umhs_cluster.hip per row and per sum against float64 (tests/cluster_f64.py), ``cluster.fit``
against the float64 Lloyd run from the same initial centres on planted data, the outputs of ``UMHSModel.spectral_clusters_context`` on
a small trained pipeline over the labelled scene of tests/test_hip_seg.py (three steps at 1024 rays, 20 x 28 path frames), and
``--clusters`` / ``python -m umhsnerf.cluster`` on the command lines."""
import json
import os

import numpy as np
import pytest
import torch

import cluster_f64 as CF
import rays_f64 as RF

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_WORST = {}


def _report(key, report):
    _WORST[key] = report
    with open(os.path.join(RF.report_dir(ROOT), "cluster_f64.json"), "w") as f:
        json.dump(_WORST, f, indent=1)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


# ------------------------------------------------------------------------------------------------------------------------------ #
# kernel
# ------------------------------------------------------------------------------------------------------------------------------ #
def _step(p, x=None, rows=slice(None), mask=None, acc="new", want_label=True, want_score=True):
    """ops.cluster_step of the problem's rows -> {"label", "score", "acc"} on the device."""
    from umhsnerf import ops

    K, B = p["K"], p["B"]
    if isinstance(acc, str):
        acc = torch.zeros(2 + K + K * B, dtype=torch.float64, device=DEV)
    image = ops.library_prepare(p["centres"].to(DEV))
    x = p["x"].to(DEV)[rows] if x is None else x
    label, score = ops.cluster_step(x, image, K, p["metric"], None if p["h"] is None else p["h"].to(DEV), None if mask is None else mask.to(DEV),
                                    acc, want_label, want_score)
    return {"label": label, "score": score, "acc": acc}


@pytest.mark.parametrize("metric", list(CF.METRICS))
@pytest.mark.parametrize("c", CF.CASES + [CF.BOUNDARY_CASE], ids=CF.case_id)
def test_step_is_within_the_bounds_of_float64_and_repeats_bit_for_bit(c, metric):
    p, r64 = CF.reference(*c, metric)
    out = _step(p)
    report = {}
    fails = CF.check_step(p, out, r64, report=report)
    print(CF.case_id(c), metric, {k: round(v, 3) for k, v in report.items()})
    _report(f"step {CF.case_id(c)} {metric}", report)
    assert not fails, fails
    again = _step(p)
    assert all(_same_bits(out[k], again[k]) for k in ("label", "score", "acc"))
    # assigning alone gives the same labels and scores
    alone = _step(p, acc=None)
    assert _same_bits(out["label"], alone["label"]) and _same_bits(out["score"], alone["score"])
    if c[0] == 0:  # R = 0 returns OK and leaves acc as it was
        kept = torch.arange(2 + c[2] + c[2] * c[1], dtype=torch.float64, device=DEV)
        assert _same_bits(_step(p, acc=kept.clone())["acc"], kept)


@pytest.mark.parametrize("c", [c for c in CF.CASES if c[0] > 0], ids=CF.case_id)
def test_angle_labels_and_scores_are_the_first_slot_of_library_match_bit_for_bit(c):
    from umhsnerf import ops

    p, _ = CF.reference(*c, "angle")
    out = _step(p, acc=None)
    index, cos = ops.library_match(p["x"].to(DEV), ops.library_prepare(p["centres"].to(DEV)), p["K"])
    assert _same_bits(out["label"], index[:, 0].contiguous()) and _same_bits(out["score"], cos[:, 0].contiguous())


@pytest.mark.parametrize("metric", list(CF.METRICS))
def test_a_call_split_at_a_multiple_of_the_chunk_leaves_the_same_bits(metric):
    from umhsnerf import ops

    assert ops.cluster_chunk() == CF.CHUNK == 1024
    p, r64 = CF.reference(2100, 141, 64, metric)
    whole = _step(p)
    for at in (1024, 2048):
        acc = _step(p, rows=slice(0, at))["acc"]
        acc = _step(p, rows=slice(at, None), acc=acc)["acc"]
        assert _same_bits(acc, whole["acc"]), at
    a = _step(p, rows=slice(0, 1000))
    b = _step(p, rows=slice(1000, None), acc=a["acc"])
    out = {"label": torch.cat([a["label"], b["label"]]), "score": torch.cat([a["score"], b["score"]]), "acc": b["acc"]}
    assert _same_bits(out["label"], whole["label"]) and _same_bits(out["score"], whole["score"])
    assert not CF.check_step(p, out, r64)


@pytest.mark.parametrize("metric", list(CF.METRICS))
def test_strided_and_unaligned_rows_give_the_same_bits_and_nothing_past_a_row_or_an_output_is_touched(metric):
    from umhsnerf import _hip, ops

    p, _ = CF.reference(1100, 31, 6, metric)
    R, B, K = p["R"], p["B"], p["K"]
    want = _step(p)
    wide = torch.full((R, B + 3), float("nan"), device=DEV)  # NaN in the columns past B: reading one would invalidate the row
    wide[:, :B] = p["x"].to(DEV)
    flat = torch.full((R * (B + 3) + 1,), float("nan"), device=DEV)
    off = flat[1:].view(R, B + 3)
    off[:, :B] = p["x"].to(DEV)
    assert off.data_ptr() % 16 == 4
    for x in (wide[:, :B], off[:, :B]):
        got = _step(p, x=x)
        assert all(_same_bits(want[k], got[k]) for k in ("label", "score", "acc"))
    # every output inside guards
    n = 2 + K + K * B
    acc = torch.full((8 + n + 8,), -7.0, dtype=torch.float64, device=DEV)
    acc[8:-8].zero_()
    label = torch.full((16 + R + 16,), -7, dtype=torch.int32, device=DEV)
    score = torch.full((16 + R + 16,), -7.0, device=DEV)
    x, image = p["x"].to(DEV), ops.library_prepare(p["centres"].to(DEV))
    h = None if p["h"] is None else p["h"].to(DEV)
    lib = _hip.lib()
    ws = torch.empty(int(lib.umhs_cluster_workspace_bytes(R, K, B)), dtype=torch.uint8, device=DEV)
    _hip.check(lib.umhs_cluster_step(_hip.ptr(x), B, R, None, _hip.ptr(image), _hip.ptr(h), K, B, CF.METRICS[metric],
                                     _hip.C.c_void_p(label.data_ptr() + 64), _hip.C.c_void_p(score.data_ptr() + 64),
                                     _hip.C.c_void_p(acc.data_ptr() + 64), _hip.ptr(ws), ws.numel(), _hip.stream()), "umhs_cluster_step")
    assert _same_bits(label[16:-16], want["label"]) and _same_bits(score[16:-16], want["score"]) and _same_bits(acc[8:-8], want["acc"])
    for guard in (label[:16], label[-16:], score[:16], score[-16:], acc[:8], acc[-8:]):
        assert bool((guard == -7).all())
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.cluster_step(p["x"], image, K, metric, h)


@pytest.mark.parametrize("metric", list(CF.METRICS))
def test_a_mask_at_exactly_one_half_is_left_out_and_dead_rows_add_nothing(metric):
    p, r64 = CF.reference(1100, 31, 6, metric)
    R = p["R"]
    mask = torch.ones(R)
    mask[::7] = 0.5
    mask[1::7] = 0.0
    mask[2::7] = 0.5000001
    out = _step(p, mask=mask)
    dead = p["dead"] | (mask <= 0.5)
    report = {}
    assert not CF.check_step(p, out, r64, dead=dead, report=report), report
    assert int((out["label"].cpu()[~dead] >= 0).sum()) == int((~dead).sum()) == int(out["acc"][0])
    # the rows left alive keep their bits
    plain = _step(p)
    live = (~dead).to(DEV)
    assert torch.equal(out["label"][live], plain["label"][live]) and torch.equal(out["score"][live], plain["score"][live])
    # NaN, Inf and all-zero rows give (-1, 0) and add nothing: the same acc with those rows' values replaced and masked out
    x = p["x"].clone()
    x[p["dead"]] = 1e30
    a = torch.ones(R)
    a[p["dead"]] = 0.5
    other = _step(p, x=x.to(DEV), mask=a)
    assert all(_same_bits(plain[k], other[k]) for k in ("label", "score", "acc"))
    assert int(p["dead"].sum()) >= 4 and bool((plain["label"].cpu()[p["dead"]] == -1).all()) and bool((plain["score"].cpu()[p["dead"]] == 0).all())


@pytest.mark.parametrize("metric", list(CF.METRICS))
def test_every_combination_of_absent_outputs(metric):
    p, _ = CF.reference(300, 31, 17, metric)
    want = _step(p)
    for want_label in (True, False):
        for want_score in (True, False):
            for acc in ("new", None):
                got = _step(p, acc=acc, want_label=want_label, want_score=want_score)
                assert (got["label"] is None) == (not want_label) and (got["score"] is None) == (not want_score)
                assert want_label is False or _same_bits(got["label"], want["label"])
                assert want_score is False or _same_bits(got["score"], want["score"])
                assert acc is None or _same_bits(got["acc"], want["acc"])


def test_every_error_of_the_header():
    from umhsnerf import _hip, ops

    lib, C = _hip.lib(), _hip.C
    R, B, K = 40, 5, 3
    x = torch.rand(R, B, device=DEV)
    image = ops.library_prepare(torch.rand(K, B, device=DEV))
    h = torch.rand(K, device=DEV)
    acc = torch.zeros(2 + K + K * B, dtype=torch.float64, device=DEV)
    label, score = torch.empty(R, dtype=torch.int32, device=DEV), torch.empty(R, device=DEV)
    ws = torch.empty(int(lib.umhs_cluster_workspace_bytes(R, K, B)), dtype=torch.uint8, device=DEV)
    assert ws.numel() == (2 + K + K * B) * 4 and lib.umhs_cluster_workspace_bytes(600 * 1024, K, B) == 512 * (2 + K + K * B) * 4
    assert lib.umhs_cluster_workspace_bytes(0, K, B) == 0 == lib.umhs_cluster_workspace_bytes(R, 65, B) == lib.umhs_cluster_workspace_bytes(R, K, 257)

    def call(x=x, stride=B, R=R, image=image, h=h, K=K, B=B, metric=1, acc=acc, ws=ws, ws_bytes=None):
        return lib.umhs_cluster_step(_hip.ptr(x), stride, R, None, _hip.ptr(image), _hip.ptr(h), K, B, metric, _hip.ptr(label), _hip.ptr(score),
                                     _hip.ptr(acc), _hip.ptr(ws), (ws.numel() if ws is not None else 0) if ws_bytes is None else ws_bytes,
                                     _hip.stream())

    ARG, UNSUPPORTED = -1, -2  # UMHS_ERR_ARG, UMHS_ERR_UNSUPPORTED
    assert call() == 0
    for bad in (dict(K=0), dict(B=0), dict(R=-1), dict(stride=B - 1), dict(metric=2), dict(metric=-1)):
        assert call(**bad) == ARG, bad
    assert call(B=257, stride=257) == UNSUPPORTED and call(K=65) == UNSUPPORTED
    assert call(K=65, metric=7) == ARG  # (bad arguments come before the limits)
    assert call(R=0, x=None, image=None, h=None, acc=acc, ws=None) == 0  # R == 0: OK whatever the pointers
    assert call(x=None) == ARG and call(image=None) == ARG
    assert call(h=None) == ARG and call(h=None, metric=0) == 0
    assert call(ws=None) == ARG and call(ws_bytes=ws.numel() - 1) == ARG
    assert call(acc=None, ws=None) == 0  # assigning alone needs no workspace
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="limits"):
        ops.cluster_step(x, image, 65, "angle")
    with pytest.raises(ValueError, match="metric"):
        ops.cluster_step(x, image, K, "manhattan")
    with pytest.raises(ValueError, match="half_norm"):
        ops.cluster_step(x, image, K, "euclidean")
    with pytest.raises(ValueError, match="acc must be"):
        ops.cluster_step(x, image, K, "angle", acc=acc[:-1])
    with pytest.raises(ValueError, match="does not belong"):
        ops.cluster_step(x, image, K + 40, "angle")
    with pytest.raises(ValueError, match="one value per row"):
        ops.cluster_step(x, image, K, "angle", mask=torch.ones(R - 1, device=DEV))


# ------------------------------------------------------------------------------------------------------------------------------ #
# the fit
# ------------------------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("metric", list(CF.METRICS))
@pytest.mark.parametrize("shape", list(CF.FIT_CASES), ids=CF.case_id)
def test_fit_follows_the_float64_lloyd_run_from_the_same_initial_centres(shape, metric, tmp_path):
    from umhsnerf import cluster

    R, B, K = shape
    seed = CF.FIT_CASES[shape][metric]
    data = CF.planted(R, B, K, metric)
    frames = [f.to(DEV) for f in data["frames"]]
    init = cluster.kmeanspp(cluster.subsample(frames, seed), K, metric, seed)
    assert np.array_equal(init, cluster.kmeanspp(cluster.subsample(data["frames"], seed), K, metric, seed))  # host or device: the same rows
    r64 = CF.lloyd(data["frames"], torch.from_numpy(init), metric, torch.float64)
    recovered = CF.partition_agreement(r64["labels"], data["truth"], K)
    print(CF.case_id(shape), metric, "float64 Lloyd recovers", recovered, "in", len(r64["objective"]), "iterations")
    assert recovered >= 0.99  # (a condition on the float64 run alone)
    clusters, log = cluster.fit(frames, K, metric, "kmeans++", seed=seed)
    explicit, log2 = cluster.fit(frames, K, metric, init, seed=seed)
    assert np.array_equal(clusters.centres, explicit.centres) and log == log2
    assert log["converged"] and log["empty"] == 0 and log["valid"] == R and log["iterations"] == len(log["objective"]) <= len(r64["objective"])
    assert all(sum(c) == R for c in log["counts"]) and clusters.counts.tolist() == log["counts"][-1]
    # labels: every row outside the float64 tied set, at the float64 run's final centres
    label, _ = clusters.assign(torch.cat(frames))
    final = CF.ref64(data["x"], clusters.device_centres(), CF.half_norm(clusters.device_centres()) if metric == "euclidean" else None, metric,
                     torch.zeros(R, dtype=torch.bool))
    tied = CF.tied_set(final["val"], final["mag"])
    assert bool(tied.gather(1, label.cpu().long()[:, None]).all())
    decided = tied.sum(1) == 1
    assert float(decided.float().mean()) > 0.99 and torch.equal(label.cpu().long()[decided], r64["labels"][decided])
    ratio = CF.centre_ratio(torch.from_numpy(clusters.centres), r64["centres"])
    margin = CF.objective_margin(metric, R)
    rises = [b - a * (1 + margin[0]) - margin[1] for a, b in zip(log["objective"][:-1], log["objective"][1:])]
    print("centres", round(ratio, 3), "u; objective", log["objective"])
    _report(f"fit {CF.case_id(shape)} {metric}", {"centres": ratio, "recovered": recovered, "iterations": log["iterations"]})
    assert ratio <= CF.K_CENTRE and all(r <= 0 for r in rises)
    # the same seed and the same data give the same bytes
    clusters.save(tmp_path / "a.npz")
    cluster.fit(frames, K, metric, "kmeans++", seed=seed)[0].save(tmp_path / "b.npz")
    assert (tmp_path / "a.npz").read_bytes() == (tmp_path / "b.npz").read_bytes()


@pytest.mark.parametrize("metric", list(CF.METRICS))
def test_an_empty_cluster_keeps_its_centre_and_is_reported(metric):
    from umhsnerf import cluster

    p, r64 = CF.reference(*CF.EMPTY_CASE, metric)
    x = p["x"].to(DEV)
    clusters, log = cluster.fit([x], p["K"], metric, p["centres"].double().numpy(), iterations=1)
    counts = np.asarray(log["counts"][0])
    empty = counts == 0
    assert log["empty"] == int(empty.sum()) >= 4 and log["valid"] == int((~p["dead"]).sum()) == int(counts.sum())
    assert np.array_equal(clusters.centres[empty], p["centres"].double().numpy()[empty])
    assert not np.array_equal(clusters.centres[~empty], p["centres"].double().numpy()[~empty])
    with pytest.raises(ValueError, match="no valid spectrum"):
        cluster.fit([torch.zeros(50, p["B"], device=DEV)], 3, metric, p["centres"][:3].double().numpy())


# ------------------------------------------------------------------------------------------------------------------------------ #
# model
# ------------------------------------------------------------------------------------------------------------------------------ #
NAMES = ("cluster_raw", "cluster_pred", "cluster_score")
H, W, FOVS = 20, 28, (50.0, 75.0, 50.0)
BASE_FLAGS = ["--num-classes", "3", "--temperature", "0.4", "--background-color", "black"]
CROP = {"crop_center": [0.1, -0.05, 0.2], "crop_scale": [0.9, 0.6, 1.2], "crop_rot": [0.3, -0.2, 0.5], "crop_bg_color": {"r": 38, "g": 120, "b": 255}}


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """The labelled scene of tests/test_hip_seg.py (6 train / 2 eval frames of 24x32, 8 bands, label images of 4 labels) with captured
    cubes that follow the labels -- one smooth spectrum per label plus noise -- a pipeline trained for three steps, its checkpoint, a
    camera path of three 20x28 frames, and clusters fitted on the captured training stack."""
    from library_f64 import make_library
    from test_hip_distortion import _look_at_origin
    from test_hip_seg import _labels, _scene
    from umhsnerf import cluster
    from umhsnerf.data.umhs_datamanager import UMHSDataManager, UMHSDataManagerConfig
    from umhsnerf.data.umhs_dataparser import UMHSDataParserConfig
    from umhsnerf.render import load_camera_path
    from umhsnerf.umhs_model import UMHSConfig
    from umhsnerf.umhs_pipeline import UMHSPipeline

    root = tmp_path_factory.mktemp("cluster")
    torch.manual_seed(0)
    scene = root / "scene"
    scene.mkdir()
    meta = _scene(scene)
    g = torch.Generator().manual_seed(31)
    E = make_library(4, 8, g)
    for k, fr in enumerate(meta["frames"]):
        lab = torch.from_numpy(_labels(24, 32, k).astype(np.int64))
        x = E[lab.clamp(max=3)] + 0.01 * torch.randn(24, 32, 8, generator=g)
        np.save(scene / fr["hyperspectral_file_path"], x.float().numpy())
    dm = UMHSDataManager(UMHSDataManagerConfig(dataparser=UMHSDataParserConfig(data=scene), train_num_rays_per_batch=1024), device=DEV,
                         num_classes=3, seed=9)
    cfg = UMHSConfig(method="rgb+spectral", pred_specular=False, temperature=0.4, background_color="black")
    pipe = UMHSPipeline.from_packed_samples(cfg, DEV, metadata={"wavelengths": meta["wavelengths"], "num_classes": 3}, seed=2, datamanager=dm)
    for step in range(3):
        pipe.get_train_loss_dict(step)
    torch.cuda.synchronize()
    pipe._ahead = None
    pipe.eval()
    torch.save({"step": 3, "pipeline": pipe.state_dict()}, root / "step-000000003.ckpt")
    rng = np.random.default_rng(11)
    path = {"camera_type": "perspective", "render_height": H, "render_width": W, "fps": 24, "seconds": 0.125,
            "camera_path": [{"camera_to_world": _look_at_origin(rng).reshape(-1).tolist(), "fov": fov, "aspect": W / H} for fov in FOVS]}
    (root / "path.json").write_text(json.dumps(path))
    cameras, _ = load_camera_path(path, device=DEV)
    wl = [float(w) for w in meta["wavelengths"]]
    stack = dm.train_split.hs_image
    clusters, log = cluster.fit([stack[i].to(DEV).float() for i in range(stack.shape[0])], 4, "angle", seed=0, wavelengths=wl)
    clusters.save(root / "clusters.npz")
    return dict(root=root, scene=scene, pipe=pipe, cameras=cameras, wl=wl, clusters=clusters, log=log, stack=stack)


def _frame(world, clusters=None, camera=1, output_names=None, crop=False):
    from umhsnerf.render import parse_crop

    model = world["pipe"].model
    if crop:  # (the untrained scene is opaque everywhere: a crop box leaves rays that accumulate nothing)
        rb = world["cameras"].generate_rays(camera, keep_shape=True, obb_box=parse_crop(CROP)["obb"], near_floor=model.config.near_plane)
    else:
        rb = world["cameras"].generate_rays(camera, keep_shape=True)
    with model.spectral_clusters_context(clusters):
        return model.get_outputs_for_camera_ray_bundle(rb, output_names=output_names)


def test_outside_the_context_nothing_changes_and_inside_only_the_asked_for_keys_are_added(world):
    plain = _frame(world)
    assert int(plain["num_samples_per_ray"].sum()) > 0 and not any(k in plain for k in NAMES)
    got = _frame(world, world["clusters"])
    assert [k for k in got if k not in NAMES] == list(plain) and all(k in got for k in NAMES)
    for k in plain:
        assert torch.equal(got[k], plain[k]), k
    assert {k: tuple(got[k].shape) for k in NAMES} == {"cluster_raw": (H, W, 1), "cluster_pred": (H, W, 3), "cluster_score": (H, W, 1)}
    # computed only when asked for
    some = _frame(world, world["clusters"], output_names=["rgb", "depth"])
    assert sorted(some) == ["depth", "rgb"]
    some = _frame(world, world["clusters"], output_names=["cluster_pred"])
    assert sorted(some) == ["cluster_pred"] and torch.equal(some["cluster_pred"], got["cluster_pred"])
    assert world["pipe"].model._spectral_clusters is None


def test_the_outputs_are_frame_outputs_of_the_frames_own_spectral_and_empty_pixels_are_minus_one_black_zero(world):
    clusters = world["clusters"]
    seen = 0
    for metric_clusters in (clusters, type(clusters)(clusters.centres, "euclidean", world["wl"])):
        for crop in (False, True):
            got = _frame(world, metric_clusters, crop=crop)
            want = metric_clusters.frame_outputs(got["spectral"], got["accumulation"])
            assert sorted(want) == sorted(NAMES)
            for k in NAMES:
                assert torch.equal(got[k], want[k]), k
            empty = got["accumulation"][..., 0] <= 0.5
            seen += int(empty.sum())
            assert bool((got["cluster_raw"][empty] == -1).all()) and bool((got["cluster_pred"][empty] == 0).all())
            assert bool((got["cluster_score"][empty] == 0).all())
            # by hand, from the op: the rendered pixels
            label, score = metric_clusters.assign(got["spectral"].reshape(-1, 8))
            rendered = ~empty.reshape(-1)
            assert torch.equal(got["cluster_raw"].reshape(-1)[rendered], label.float()[rendered])
            assert torch.equal(got["cluster_score"].reshape(-1)[rendered], score[rendered])
            colors = torch.from_numpy(metric_clusters.colors).to(DEV)
            at = got["cluster_raw"].reshape(-1).long()
            assert torch.equal(got["cluster_pred"].reshape(-1, 3)[at >= 0], colors[at[at >= 0]])
    assert seen > 100


def test_under_material_edits_the_edited_scene_is_classified(world):
    from umhsnerf.materials import load_material_edits

    model, clusters = world["pipe"].model, world["clusters"]
    edits = load_material_edits({"materials": [{"material": 2, "spectrum": [0.9, 0.05, 0.7, 0.1, 0.6, 0.2, 0.8, 0.3]}]}, 3, 8, False)
    rb = world["cameras"].generate_rays(1, keep_shape=True)
    with model.material_edits_context(edits), model.spectral_clusters_context(clusters):
        got = model.get_outputs_for_camera_ray_bundle(rb)
    plain = _frame(world, clusters)
    assert not torch.equal(got["spectral"], plain["spectral"])
    want = clusters.frame_outputs(got["spectral"], got["accumulation"])
    for k in NAMES:
        assert torch.equal(got[k], want[k]), k
    assert not torch.equal(got["cluster_score"], plain["cluster_score"])


def test_refusals_and_the_state_after_an_exception(world):
    from umhsnerf.cluster import SpectralClusters
    from umhsnerf.umhs_model import UMHSConfig, UMHSModel

    model, clusters = world["pipe"].model, world["clusters"]
    rgb = UMHSModel(UMHSConfig(method="rgb", background_color="black"), metadata={"wavelengths": world["wl"], "num_classes": 3}, seed=1)
    with pytest.raises(NotImplementedError, match="spectral method"):
        with rgb.spectral_clusters_context(clusters):
            pass
    rb = world["cameras"].generate_rays(0, keep_shape=True)
    model.train()
    try:
        with pytest.raises(NotImplementedError, match="model.eval"):
            with model.spectral_clusters_context(clusters):
                model.get_outputs_for_camera_ray_bundle(rb)
    finally:
        model.eval()
    assert model._spectral_clusters is None
    with pytest.raises(KeyError):
        with model.spectral_clusters_context(clusters):
            assert model._spectral_clusters is clusters
            raise KeyError("inside")
    assert model._spectral_clusters is None
    with pytest.raises(ValueError, match="wavelengths"):
        with model.spectral_clusters_context(SpectralClusters(np.ones((2, 5)), "angle", [1.0, 2.0, 3.0, 4.0, 5.0])):
            pass


# ------------------------------------------------------------------------------------------------------------------------------ #
# command lines
# ------------------------------------------------------------------------------------------------------------------------------ #
def _model_flags(world):
    return ["--data", str(world["scene"]), "--checkpoint", str(world["root"] / "step-000000003.ckpt"), *BASE_FLAGS]


def test_fit_then_render_dataset_with_the_clusters_and_classify_the_captured_frames(world, capsys):
    from PIL import Image

    from umhsnerf import cluster, render

    root = world["root"]
    got = cluster.main(["fit", *_model_flags(world), "--source", "captured", "--split", "train", "--clusters", "4", "--metric", "angle",
                        "--output", str(root / "cli.npz")])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0]) == got
    log = world["log"]
    assert got["clusters"] == 4 and got["bands"] == 8 and got["valid"] == log["valid"] == world["stack"][..., 0].numel()
    assert got["iterations"] == log["iterations"] and got["converged"] and got["counts"] == log["counts"][-1]
    assert (root / "cli.npz").read_bytes() == (root / "clusters.npz").read_bytes()  # the same seed and data: the same bytes
    rendered = cluster.main(["fit", *_model_flags(world), "--source", "rendered", "--split", "train", "--clusters", "3", "--metric",
                             "euclidean", "--init", "endmembers", "--iterations", "3", "--output", str(root / "rendered.npz")])
    capsys.readouterr()
    assert 2 <= rendered["valid"] <= got["valid"] and rendered["clusters"] == 3 and rendered["iterations"] <= 3
    with pytest.raises(ValueError, match="the model has 3 endmembers, --clusters asks for 4"):
        cluster.main(["fit", *_model_flags(world), "--clusters", "4", "--init", "endmembers", "--output", str(root / "no.npz")])
    out = render.main(["dataset", *_model_flags(world), "--split", "test", "--output-path", str(root / "ds"), "--clusters",
                       str(root / "cli.npz"), "--rendered-output-names", "cluster_pred", "cluster_raw"])
    capsys.readouterr()
    assert out["frames"] >= 1 and out["files"] == 2 * out["frames"] and out["clusters"] == str(root / "cli.npz")
    for name in ("cluster_pred", "cluster_raw"):
        files = sorted((root / "ds" / "test" / name).glob("*.png"))
        assert len(files) == out["frames"]
        assert np.asarray(Image.open(files[0])).shape[2] == 3
    with pytest.raises(ValueError, match="pass --clusters FILE"):
        render.main(["dataset", *_model_flags(world), "--output-path", str(root / "no"), "--rendered-output-names", "cluster_pred"])
    assert world["pipe"].model._spectral_clusters is None
    # the captured frames, classified
    summary = cluster.main(["captured", *_model_flags(world), "--split", "train", "--clusters-file", str(root / "cli.npz"), "--output-path",
                            str(root / "captured")])
    capsys.readouterr()
    files = sorted((root / "captured").glob("*_cluster.npy"))
    assert len(files) == summary["frames"] == world["stack"].shape[0] and summary["invalid_pixels"] == [0] * len(files)
    first = np.load(files[0])
    assert first.shape == (24, 32) and first.dtype == np.int32 and first.min() >= 0 and first.max() <= 3
    assert abs(sum(c["share"] for c in summary["clusters"]) - 1.0) < 1e-9 and json.loads((root / "captured" / "summary.json").read_text())["frames"] == len(files)


def test_eval_with_the_clusters_prints_the_new_keys_and_scores_the_k_means_baseline(world, capsys):
    from umhsnerf import eval as umhs_eval

    got = umhs_eval.main([*_model_flags(world), "--clusters", str(world["root"] / "clusters.npz")])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0]) == got and "psnr" in got and "seg_acc" in got
    for key in ("cluster_top", "cluster_agreement", "cluster_model_agreement", "cluster_seg_acc", "cluster_seg_miou", "cluster_seg_iou_0"):
        assert key in got, key
    assert 0 <= got["cluster_agreement"] <= 1 and 0 <= got["cluster_model_agreement"] <= 1
    assert len(got["cluster_top"]) >= 1 and sum(c["share"] for c in got["cluster_top"]) <= 1.0 + 1e-9
    # the captured cubes follow the labels (one spectrum per label, 1 % noise): k-means of them is a near-perfect segmentation
    assert got["cluster_seg_acc"] > 0.95 and got["cluster_seg_miou"] > 0.9
