"""Segmentation scoring on the GPU: ``umhs_seg_confusion`` (``ops.seg_confusion``) against ``torch.bincount`` on the CPU
(tests/seg_ref.py), and the layers above it -- ``UMHSDataManager.eval_images`` and ``UMHSPipeline.get_average_eval_image_metrics`` on a
scene on disk whose frames carry ``seg_file_path``, with the stacks on the device and in host memory.

Counts are integers: every comparison of a table is ``torch.equal``.  The shapes are the smallest at which the kernel can go wrong:
0, 1, 63, 64, 65 pixels (around one wave), 5x7 and 37x29 (no multiple of 4, 64 or 256: scalar head and tail around the 16-byte quads),
256x256 (64 workgroups), 2^20 (every workgroup of the capped grid, one step each) and 2^20 + 4,099 (a second, partly empty step);
2^20 pixels in one bin for contention and the 64-bit global add; label pointers at byte offsets 1, 2, 3 of an aligned word; float
pointers off the 16-byte boundary, and two that do not share an alignment (the scalar path)."""
import functools
import json

import numpy as np
import pytest
import torch

import seg_ref as SR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

PIXELS = [0, 1, 63, 64, 65, 5 * 7, 37 * 29, 256 * 256]
TABLES = [(1, 1), (4, 3), (6, 7), (16, 32)]


@functools.lru_cache(maxsize=None)
def _case(n, C, L):
    """(seg_raw, accumulation, labels, reference table) of one shape, computed once on the CPU and never modified."""
    raw, acc, lab = SR.case(n, C, L)
    return raw, acc, lab, SR.confusion(raw, acc, lab, C, L)


@pytest.mark.parametrize("C, L", TABLES)
@pytest.mark.parametrize("n", PIXELS)
def test_table_equals_bincount(n, C, L):
    from umhsnerf import ops

    raw, acc, lab, want = _case(n, C, L)
    if n >= 64:
        assert bool((acc == 0.5).any()) and bool((lab == 255).any())
    got = ops.seg_confusion(raw.to(DEV), acc.to(DEV), lab.to(DEV), C, L)
    assert got.dtype == torch.int64 and got.shape == (C + 1, L) and got.is_cuda
    assert torch.equal(got.cpu(), want)
    assert int(want.sum()) == int(((lab != 255) & (lab < L)).sum())  # every kept label is counted exactly once
    if n == 37 * 29:  # any shape with the same number of elements
        again = ops.seg_confusion(raw.to(DEV).view(37, 29, 1), acc.to(DEV).view(37, 29), lab.to(DEV).view(37, 29), C, L)
        assert torch.equal(again, got)


@pytest.mark.parametrize("n", [37 * 29, 4096 + 5])
def test_table_does_not_depend_on_where_the_buffers_start(n):
    """Labels at byte offsets 1, 2, 3 of an aligned word (the quads' label bytes then come from two words), the float streams at 4, 8
    and 12 bytes off a 16-byte boundary (a scalar head in front of the quads), and float streams that differ in alignment (no quads)."""
    from umhsnerf import ops

    C, L = 6, 7
    raw, acc, lab, want = _case(n, C, L)
    for shift in (1, 2, 3):
        buf = torch.full((n + 64,), 3, dtype=torch.uint8, device=DEV)  # valid labels all around: none may leak in
        view = buf[shift : shift + n]
        view.copy_(lab)
        assert view.data_ptr() % 4 == shift
        assert torch.equal(ops.seg_confusion(raw.to(DEV), acc.to(DEV), view, C, L).cpu(), want), shift
    for shift_raw, shift_acc in ((1, 1), (2, 2), (3, 3), (0, 1), (3, 2)):
        fr, fa = torch.zeros(n + 8, device=DEV), torch.ones(n + 8, device=DEV)
        vr, va = fr[shift_raw : shift_raw + n], fa[shift_acc : shift_acc + n]
        vr.copy_(raw), va.copy_(acc)
        assert vr.data_ptr() % 16 == 4 * shift_raw and va.data_ptr() % 16 == 4 * shift_acc
        lv = torch.full((n + 64,), 3, dtype=torch.uint8, device=DEV)[3 : 3 + n]
        lv.copy_(lab)
        assert torch.equal(ops.seg_confusion(vr, va, lv, C, L).cpu(), want), (shift_raw, shift_acc)


def test_more_pixels_than_one_step_of_the_capped_grid():
    """1,024 workgroups x 1,024 pixels is one step of the whole grid: beyond 2^20 pixels workgroups take a second, partly empty one."""
    from umhsnerf import ops

    n, C, L = (1 << 20) + 4096 + 3, 6, 7
    raw, acc, lab, want = _case(n, C, L)
    assert torch.equal(ops.seg_confusion(raw.to(DEV), acc.to(DEV), lab.to(DEV), C, L).cpu(), want)
    shifted = torch.zeros(n + 4, dtype=torch.uint8, device=DEV)[1 : 1 + n]
    shifted.copy_(lab)
    assert torch.equal(ops.seg_confusion(raw.to(DEV), acc.to(DEV), shifted, C, L).cpu(), want)


def test_pixels_that_are_not_scored_never_reach_the_table():
    from umhsnerf import ops

    C, L = 4, 3
    nan = float("nan")
    #                     kept  kept   >=L   ignore  NaN   -1     C    2.5   NaN acc  acc 0.5  unrendered junk raw
    raw = torch.tensor([1.0,  3.0,   0.0,  0.0,   nan,  -1.0,  4.0,  2.5,  2.0,     2.0,     nan,  -7.0, 1e9] * 70)
    acc = torch.tensor([0.9,  0.51,  0.9,  0.9,   0.9,  0.9,   0.9,  0.9,  nan,     0.5,     0.1,  0.2,  0.0] * 70)
    lab = torch.tensor([0,    2,     3,    255,   1,    1,     1,    1,    2,       1,       0,    1,    2] * 70, dtype=torch.uint8)
    want = torch.zeros(C + 1, L, dtype=torch.int64)
    want[1, 0] = want[3, 2] = 70
    want[C, 2], want[C, 1], want[C, 0] = 70 + 70, 70 + 70, 70  # NaN accumulation, 0.5, and the three unrendered pixels whatever seg_raw is
    assert torch.equal(SR.confusion(raw, acc, lab, C, L), want)
    guarded = torch.zeros(C + 3, L, dtype=torch.int64, device=DEV)  # one guard row in front and one behind
    out = ops.seg_confusion(raw.to(DEV), acc.to(DEV), lab.to(DEV), C, L, out=guarded[1 : C + 2])
    assert out.data_ptr() == guarded[1].data_ptr() and torch.equal(out.cpu(), want)
    assert not bool(guarded[0].any()) and not bool(guarded[-1].any())
    # ignore_label = -1: label 255 is a label like any other, and here >= L
    assert torch.equal(ops.seg_confusion(raw.to(DEV), acc.to(DEV), lab.to(DEV), C, L, ignore_label=-1).cpu(), want)
    # another ignore label: label 0 goes, 255 is >= L
    want0 = want.clone()
    want0[:, 0] = 0
    assert torch.equal(ops.seg_confusion(raw.to(DEV), acc.to(DEV), lab.to(DEV), C, L, ignore_label=0).cpu(), want0)


def test_calls_accumulate_into_out():
    from umhsnerf import ops

    C, L = 6, 7
    a, b = _case(37 * 29, C, L), _case(256 * 256, C, L)
    dev = lambda c: [t.to(DEV) for t in c[:3]]
    out = ops.seg_confusion(*dev(a), C, L)
    assert torch.equal(out.cpu(), a[3])
    same = ops.seg_confusion(*dev(b), C, L, out=out)
    assert same is out and torch.equal(out.cpu(), a[3] + b[3])
    fresh = ops.seg_confusion(*dev(b), C, L)
    assert fresh is not out and torch.equal(fresh.cpu(), b[3])
    with pytest.raises(ValueError, match="out must be"):
        ops.seg_confusion(*dev(a), C, L, out=torch.zeros(C, L, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="differ in size"):
        ops.seg_confusion(dev(a)[0], dev(a)[1], dev(b)[2], C, L)
    with pytest.raises(RuntimeError, match="shape not supported"):
        ops.seg_confusion(*dev(a), 17, L)


def test_one_bin_takes_every_pixel_and_the_global_add_is_64_bit():
    from umhsnerf import ops

    n, C, L = 1 << 20, 16, 32
    raw, acc = torch.full((n,), 5.0, device=DEV), torch.ones(n, device=DEV)
    lab = torch.full((n,), 9, dtype=torch.uint8, device=DEV)
    want = torch.zeros(C + 1, L, dtype=torch.int64)
    want[5, 9] = n
    assert torch.equal(ops.seg_confusion(raw, acc, lab, C, L).cpu(), want)
    out = torch.zeros(C + 1, L, dtype=torch.int64, device=DEV)
    out[5, 9] = 1 << 33
    ops.seg_confusion(raw, acc, lab, C, L, out=out)
    want[5, 9] = (1 << 33) + n
    assert torch.equal(out.cpu(), want)


# ---- the model's own outputs -------------------------------------------------------------------------------------------------------
def _labels(Hs, Ws, k):
    """A label image of flat regions: vertical bands of labels 0..3 shifted by ``k``, a strip of the ignore label on top."""
    s = ((np.arange(Ws)[None, :] + 3 * k) // 8 % 4).astype(np.uint8) * np.ones((Hs, 1), np.uint8)
    s[:2] = 255
    return s


def _scene(root, with_labels=True, Hs=24, Ws=32, B=8):
    """The ``make_scene`` recipe of tests/test_hip_distortion.py (6 train / 2 eval frames of 24x32, 8 bands) plus a label file per frame;
    the cubes are rewritten with a spectrum that varies over the frame (a constant one has no SSIM: its data range is 0)."""
    from test_hip_distortion import make_scene

    meta = make_scene(root, B=B, Hs=Hs, Ws=Ws)
    rng = np.random.default_rng(5)
    for fr in meta["frames"]:
        np.save(root / fr["hyperspectral_file_path"], (0.2 + 0.6 * rng.random((Hs, Ws, B))).astype(np.float32))
    if with_labels:
        (root / "seg").mkdir()
        for k, fr in enumerate(meta["frames"]):
            name = "seg/" + fr["file_path"].replace("/", "_")
            np.save(root / name, _labels(Hs, Ws, k))
            fr["seg_file_path"] = name
        (root / "transforms.json").write_text(json.dumps(meta))
    return meta


def _datamanager(root, on_gpu=True, seed=1):
    from umhsnerf.data.umhs_datamanager import UMHSDataManager, UMHSDataManagerConfig
    from umhsnerf.data.umhs_dataparser import UMHSDataParserConfig

    return UMHSDataManager(UMHSDataManagerConfig(dataparser=UMHSDataParserConfig(data=root), train_num_rays_per_batch=1024, images_on_gpu=on_gpu),
                           device=DEV, num_classes=3, seed=seed)


def _pipeline(root, meta, on_gpu=True, train_steps=0):
    """(pipeline, its data manager).  ``train_steps``: so many training steps first, drawn from a data manager of their own -- the one
    returned has then drawn nothing yet, like a second ``_datamanager(root, on_gpu)``."""
    from umhsnerf.umhs_model import UMHSConfig
    from umhsnerf.umhs_pipeline import UMHSPipeline

    cfg = UMHSConfig(method="rgb+spectral", pred_specular=True, temperature=0.4, background_color="black")
    pipe = UMHSPipeline.from_packed_samples(cfg, DEV, metadata={"wavelengths": meta["wavelengths"], "num_classes": 3}, seed=2,
                                            datamanager=_datamanager(root, on_gpu, seed=9))
    for step in range(train_steps):
        pipe.get_train_loss_dict(step)
    torch.cuda.synchronize()
    pipe._ahead = None  # (a batch drawn one step ahead belongs to the training data manager)
    pipe.datamanager = _datamanager(root, on_gpu)
    return pipe, pipe.datamanager


def test_table_of_a_models_own_outputs(tmp_path):
    """``seg_raw`` / ``accumulation`` as ``get_outputs_for_camera_ray_bundle`` returns them for a 24x32 frame of a fresh spectral model."""
    from umhsnerf import ops

    pipe, dm = _pipeline(tmp_path, _scene(tmp_path))
    pipe.eval()
    cam, batch = next(iter(dm.eval_images()))
    out = pipe.model.get_outputs_for_camera_ray_bundle(cam)
    C, L = 3, dm.eval_split.seg_num_labels
    assert L == 4 and out["seg_raw"].shape == (24, 32, 1) and batch["seg_image"].shape == (24, 32) and batch["seg_image"].dtype == torch.uint8
    got = ops.seg_confusion(out["seg_raw"], out["accumulation"], batch["seg_image"], C, L)
    raw, acc, lab = out["seg_raw"].cpu().reshape(-1), out["accumulation"].cpu().reshape(-1), batch["seg_image"].cpu().reshape(-1).long()
    row = torch.where(acc > 0.5, raw.long(), torch.full_like(lab, C))
    keep = lab != 255
    want = torch.bincount((row * L + lab)[keep], minlength=(C + 1) * L).view(C + 1, L)
    assert torch.equal(got.cpu(), want) and int(want.sum()) == 22 * 32


@pytest.mark.parametrize("on_gpu", [True, False])
def test_whole_eval_split_once_in_order_and_scored(tmp_path, on_gpu):
    from umhsnerf.utils.seg_metrics import seg_scores

    meta = _scene(tmp_path)
    pipe, dm = _pipeline(tmp_path, meta, on_gpu, train_steps=40)  # (trained a little: a fresh model renders nothing at all)
    twin = _datamanager(tmp_path, on_gpu)  # the same data manager, never iterated
    assert dm.eval_split.seg.is_cuda == on_gpu and dm.eval_split.seg.shape == (2, 24, 32) and dm.train_split.seg.shape == (6, 24, 32)
    assert "seg_image" not in dm.next_train(0)[1] and "seg_image" not in twin.next_train(0)[1]  # training batches never carry labels
    item = dm.eval_dataset[1]["seg_image"]
    assert item.shape == (24, 32) and item.dtype == torch.uint8 and torch.equal(item, dm.eval_split.seg[1])

    frames = dm.eval_images()
    assert len(frames) == 2 == len(dm.fixed_indices_eval_dataloader)
    cursor = dm._eval_cursor
    seen = list(frames)
    assert len(seen) == 2 and dm._eval_cursor == cursor
    for i, (cam, batch) in enumerate(seen):  # in order, and what next_eval_image hands out
        cam2, batch2 = twin.next_eval_image(i)
        assert batch["image_idx"] == i == batch2["image_idx"] and cam.origins.shape == (24, 32, 3)
        assert torch.equal(cam.origins, cam2.origins) and torch.equal(cam.directions, cam2.directions)
        for key in ("image", "hs_image", "seg_image"):
            assert batch[key].is_cuda and torch.equal(batch[key], batch2[key]), key
        assert batch["seg_image"].shape == (24, 32) and batch["seg_image"].dtype == torch.uint8
    # the labels are those of the eval frames' files, in the split's (sorted) order
    names = dm.train_dataparser_outputs.metadata["seg_filenames"]
    assert len(names) == 6 and torch.equal(dm.train_split.seg[0].cpu(), torch.from_numpy(np.load(names[0])))

    # one frame at a time, by hand
    pipe.eval()
    singles, tables, kept = [], [], 0
    for cam, batch in dm.eval_images():
        out = pipe.model.get_outputs_for_camera_ray_bundle(cam)
        singles.append(pipe.model.get_image_metrics_and_images(out, batch)[0])
        tables.append(SR.confusion(out["seg_raw"], out["accumulation"], batch["seg_image"], 3, 4))
        kept += int((batch["seg_image"] != 255).sum())
        if batch["image_idx"] == 0:
            raw0 = out["seg_raw"].cpu()
    pipe.train()

    assert pipe.last_seg_eval is None
    result = pipe.get_average_eval_image_metrics(get_std=True, output_path=tmp_path / "renders")
    assert pipe.model.training and pipe.training
    for key in ("psnr", "ssim", "psnr_spectral", "ssim_spectral", "sam_spectral", "rmse_spectral"):
        values = np.array([m[key] for m in singles], dtype=np.float64)
        print(key, result[key], values.mean(), result[key + "_std"])
        assert result[key] == pytest.approx(values.mean(), rel=1e-12, abs=0.0), key
        assert result[key + "_std"] == pytest.approx(values.std(ddof=1), rel=1e-9, abs=1e-300), key
    assert result["fps"] > 0 and result["num_rays_per_sec"] > 0 and "fps_std" in result
    # the split's segmentation scores: from ONE table over both frames
    counts = pipe.last_seg_eval["counts"]
    assert torch.equal(counts, tables[0] + tables[1]) and int(counts.sum()) == kept == 2 * 22 * 32
    ref = SR.scores(counts.numpy(), pipe.last_seg_eval["assignment"])
    assert pipe.last_seg_eval["assignment"] == seg_scores(counts)["assignment"]
    assert set(ref) == {"seg_acc", "seg_miou", "seg_iou_0", "seg_iou_1", "seg_iou_2", "seg_iou_3"}
    for key, value in ref.items():
        assert result[key] == value and key + "_std" not in result, key
    assert "assignment" not in result and all(isinstance(v, float) for v in result.values())
    print("rendered share", float((counts[:3].sum() / counts.sum())), "scores", {k: result[k] for k in ref})
    # the files
    from PIL import Image

    for idx in (0, 1):
        for key in ("img", "accumulation", "depth", "se_per_pixel"):
            assert (tmp_path / "renders" / f"eval_{key}_{idx:04d}.png").exists(), (key, idx)
        assert (tmp_path / "renders" / f"seg_pred_{idx:04d}.png").exists()
    back = np.array(Image.open(tmp_path / "renders" / "seg_raw_0000.png"))
    assert back.dtype == np.uint8 and back.shape == (24, 32) and np.array_equal(back, raw0[..., 0].numpy().astype(np.uint8))
    assert np.array(Image.open(tmp_path / "renders" / "seg_pred_0000.png")).shape == (24, 32, 3)
    assert np.array(Image.open(tmp_path / "renders" / "eval_img_0000.png")).shape == (24, 64, 3)

    # nothing above moved the cursor or the generator: the next training batch has the bits it has without any of it
    assert dm._eval_cursor == cursor
    (ra, ba), (rb, bb) = dm.next_train(1), twin.next_train(1)
    assert torch.equal(ba["indices"], bb["indices"]) and torch.equal(ba["image"], bb["image"]) and torch.equal(ba["hs_image"], bb["hs_image"])
    assert torch.equal(ra.origins, rb.origins) and torch.equal(ra.directions, rb.directions)


def test_a_scene_without_labels_is_evaluated_without_the_new_kernel(tmp_path, monkeypatch):
    from umhsnerf import ops

    meta = _scene(tmp_path, with_labels=False)
    pipe, dm = _pipeline(tmp_path, meta)
    assert dm.eval_split.seg is None and dm.train_split.seg is None and "seg_image" not in next(iter(dm.eval_images()))[1]
    assert "seg_image" not in dm.eval_dataset[0] and "seg_image" not in dm.next_eval_image(0)[1]

    def refuse(*a, **k):
        raise AssertionError("umhs_seg_confusion must not be launched for a scene without labels")

    monkeypatch.setattr(ops, "seg_confusion", refuse)
    result = pipe.get_average_eval_image_metrics(output_path=tmp_path / "renders")
    assert pipe.last_seg_eval is None and not any(k.startswith("seg_") for k in result) and not any(k.endswith("_std") for k in result)
    assert {"psnr", "ssim", "psnr_spectral", "ssim_spectral", "sam_spectral", "rmse_spectral", "fps", "num_rays_per_sec"} <= set(result)
    from PIL import Image

    pipe.eval()
    cam, _ = next(iter(dm.eval_images()))
    raw0 = pipe.model.get_outputs_for_camera_ray_bundle(cam)["seg_raw"].cpu()
    pipe.train()
    back = np.array(Image.open(tmp_path / "renders" / "seg_raw_0000.png"))  # the model's labels are still written
    assert np.array_equal(back, raw0[..., 0].numpy().astype(np.uint8))


def test_a_model_that_segments_perfectly_scores_one_and_the_permutation_is_recovered():
    """Endmembers = C well-separated rows; the rendered spectrum of a pixel with label k is endmember perm[k]: the epilogue's ``seg_raw``
    is then perm[label], and the scores must say so."""
    from umhsnerf import _hip, ops
    from umhsnerf.utils.seg_metrics import seg_scores

    C, B, Hs, Ws = 4, 8, 24, 32
    from umhsnerf.umhs_model import UMHSConfig, UMHSModel

    model = UMHSModel(UMHSConfig(method="rgb+spectral", background_color="black"), metadata={"wavelengths": [420 + 30 * k for k in range(B)],
                                                                                            "num_classes": C}, seed=0).to(DEV)
    E = torch.full((C, B), 0.05)
    for c in range(C):
        E[c, 2 * c : 2 * c + 2] = 0.9
    with torch.no_grad():
        model.field.endmembers.copy_(E.to(DEV))
    perm = [2, 0, 3, 1]  # label k is rendered as cluster perm[k]
    lab = torch.from_numpy(_labels(Hs, Ws, 0)).reshape(-1)
    spectra = E[torch.tensor(perm)][lab.clamp(max=3).long()].to(DEV).contiguous()
    R = Hs * Ws
    acc = torch.ones(R, device=DEV)
    mm = ops.tmid_minmax(torch.ones(4, device=DEV), torch.full((4,), 2.0, device=DEV))
    _, _, _, seg_raw, _ = ops.ray_epilogue_fwd(spectra, _hip.f32c(model.converter.transform_matrix), model.field.endmembers.detach().contiguous(), acc,
                                               torch.full((R,), 1.5, device=DEV), mm, _hip.f32c(model.class_colors), 0.2)
    counts = ops.seg_confusion(seg_raw, acc, lab.to(DEV), C, 4).cpu()
    sc = seg_scores(counts)
    assert sc["assignment"] == perm and sc["seg_acc"] == 1.0 == sc["seg_miou"] and all(sc[f"seg_iou_{k}"] == 1.0 for k in range(4))
    assert int(counts.sum()) == 22 * 32 and int(counts[C].sum()) == 0


def test_the_eval_entry_point_loads_a_checkpoint_and_prints_one_json_line(tmp_path, capsys):
    """``python -m umhsnerf.eval`` in process: a Trainer-style checkpoint of a briefly trained pipeline, evaluated by a pipeline the entry
    point builds itself, gives the numbers the trained pipeline gives."""
    from umhsnerf import eval as umhs_eval

    scene = tmp_path / "scene"
    pipe, _ = _pipeline(scene, _scene(scene), train_steps=40)
    want = pipe.get_average_eval_image_metrics(get_std=True)
    torch.save({"step": 40, "pipeline": pipe.state_dict()}, tmp_path / "step-000000040.ckpt")
    capsys.readouterr()
    got = umhs_eval.main(["--data", str(scene), "--checkpoint", str(tmp_path / "step-000000040.ckpt"), "--output-path", str(tmp_path / "out"),
                          "--num-classes", "3", "--pred-specular", "--temperature", "0.4", "--background-color", "black"])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0]) == got
    assert set(got) == set(want) and "seg_miou" in got and "psnr_std" in got
    for key in want:
        if key not in ("fps", "num_rays_per_sec", "fps_std", "num_rays_per_sec_std"):  # (wall-clock)
            assert got[key] == want[key], key
    assert (tmp_path / "out" / "seg_raw_0001.png").exists() and (tmp_path / "out" / "eval_img_0000.png").exists()
