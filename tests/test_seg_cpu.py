"""Segmentation scoring without a GPU: ``seg_file_path`` through the parser and ``load_seg`` through the dataset, the assignment and the
scores of ``umhsnerf.utils.seg_metrics`` against scipy and the float64 restatement (tests/seg_ref.py), and the argument checks of
``umhs_seg_confusion`` (nothing is launched).  Counts and matched totals are integers and compared with ``==``."""
import ctypes
import json

import numpy as np
import pytest
import torch

import seg_ref as SR
from test_hip_distortion import make_scene
from umhsnerf.data.umhs_dataparser import UMHSDataParserConfig
from umhsnerf.data.utils.hs_dataloader import HyperspectralDataset, load_seg
from umhsnerf.utils.seg_metrics import match_clusters, seg_scores

H, W = 24, 32


def _add_labels(root, which=lambda i, fr: True, array=None, seed=1):
    """Adds ``seg_file_path`` (seg/<split>_<name>.npy; labels 0..4 and some 255) to the frames of the scene that ``which`` picks."""
    meta = json.loads((root / "transforms.json").read_text())
    rng = np.random.default_rng(seed)
    (root / "seg").mkdir(exist_ok=True)
    labels = {}
    for i, fr in enumerate(meta["frames"]):
        if which(i, fr):
            s = rng.integers(0, 5, (H, W)).astype(np.uint8) if array is None else array
            if array is None:
                s[rng.random((H, W)) < 0.1] = 255
            name = "seg/" + fr["file_path"].replace("/", "_")
            np.save(root / name, s)
            fr["seg_file_path"] = name
            labels[fr["file_path"]] = s
    (root / "transforms.json").write_text(json.dumps(meta))
    return labels


def test_parser_and_dataset_carry_the_label_images_in_split_order(tmp_path):
    make_scene(tmp_path)
    labels = _add_labels(tmp_path)
    parser = UMHSDataParserConfig(data=tmp_path).setup()
    assert parser.config.seg_ignore_label == 255
    for split, n in (("train", 6), ("val", 2)):
        out = parser.get_dataparser_outputs(split)
        names = out.metadata["seg_filenames"]
        assert len(names) == n == len(out.image_filenames)
        for img, seg in zip(out.image_filenames, names):  # the same frames, in the same (sorted) order
            assert seg == tmp_path / "seg" / f"{img.parent.name}_{img.name}"
        ds = HyperspectralDataset(out)
        assert ds.seg.dtype == torch.uint8 and ds.seg.shape == (n, H, W) and ds.seg_num_labels == 5
        for i, img in enumerate(out.image_filenames):
            np.testing.assert_array_equal(ds.seg[i].numpy(), labels[f"{img.parent.name}/{img.name}"])


def test_a_scene_without_labels_parses_as_before_and_labels_on_some_frames_are_refused(tmp_path):
    make_scene(tmp_path)
    out = UMHSDataParserConfig(data=tmp_path).setup().get_dataparser_outputs("train")
    assert out.metadata["seg_filenames"] is None and out.mask_filenames is None
    ds = HyperspectralDataset(out)
    assert ds.seg is None and ds.mask is None and ds.image.shape == (6, H, W, 4) and ds.hs_image.shape == (6, H, W, 8)
    _add_labels(tmp_path, which=lambda i, fr: i != 3)
    with pytest.raises(AssertionError, match="seg_file_path"):
        UMHSDataParserConfig(data=tmp_path).setup().get_dataparser_outputs("train")


@pytest.mark.parametrize("bad, match", [
    (np.zeros((H, W, 1), np.uint8), "one channel"),
    (np.zeros((H, W + 1), np.uint8), "the frames are"),
    (np.arange(H * W, dtype=np.uint8).reshape(H, W) % 33, "32 labels"),  # 33 distinct labels, 0..32
    (np.zeros((H, W), np.float32), "integers"),
    (np.full((H, W), 256, np.int32), "0..255"),
])
def test_a_bad_label_file_is_a_value_error_that_names_the_file(tmp_path, bad, match):
    make_scene(tmp_path)
    _add_labels(tmp_path, array=bad)
    out = UMHSDataParserConfig(data=tmp_path).setup().get_dataparser_outputs("val")
    with pytest.raises(ValueError, match=match) as err:
        HyperspectralDataset(out)
    assert str(out.metadata["seg_filenames"][0]) in str(err.value)


def test_npy_and_png_labels_load_alike_and_the_ignore_label_does_not_count(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    s = (np.arange(H * W).reshape(H, W) % 7).astype(np.uint8)
    s[0, :5] = 255
    np.save(tmp_path / "s.npy", s)
    Image.fromarray(s).save(tmp_path / "s.png")
    np.save(tmp_path / "wide.npy", s.astype(np.int64))
    for name in ("s.npy", "s.png", "wide.npy"):
        got = load_seg(tmp_path / name)
        assert got.dtype == torch.uint8 and torch.equal(got, torch.from_numpy(s)), name
    from umhsnerf.data.utils.hs_dataloader import seg_num_labels

    assert seg_num_labels(torch.from_numpy(s)) == 7 and seg_num_labels(torch.from_numpy(s), ignore_label=-1) == 256
    assert seg_num_labels(torch.from_numpy(s), ignore_label=6) == 256 and seg_num_labels(torch.full((2, 2), 255, dtype=torch.uint8)) == 0


# ---- assignment and scores ---------------------------------------------------------------------------------------------------------
def _tables():
    rng = np.random.default_rng(11)
    out = {f"{p}x{k}": rng.integers(0, 10**6, (p, k)) for p, k in ((1, 1), (2, 5), (5, 2), (7, 4), (17, 32))}
    zc = rng.integers(0, 10**6, (6, 7))
    zc[:, 3] = 0
    zr = rng.integers(0, 10**6, (6, 7))
    zr[2, :] = 0
    out["zero_column"], out["zero_row"] = zc, zr
    return out


@pytest.mark.parametrize("name", ["1x1", "2x5", "5x2", "7x4", "17x32", "zero_column", "zero_row"])
def test_assignment_and_scores_equal_scipy_and_the_float64_restatement(name):
    counts = _tables()[name]
    want, want_total = SR.scipy_assignment(counts)
    got = match_clusters(torch.from_numpy(counts))
    pairs = [(p, k) for k, p in enumerate(got) if p >= 0]
    assert len(pairs) == min(counts.shape) and len({p for p, _ in pairs}) == len(pairs)  # injective, min(P, K) pairs
    assert sum(int(counts[p, k]) for p, k in pairs) == want_total  # exact: integers
    if name in ("1x1", "2x5", "5x2", "7x4"):  # small enough to enumerate: the optimum is unique (entries drawn from [0, 10^6)), so the
        # assignments themselves must agree
        optima, best = SR.brute_force(counts)
        assert best == want_total and len(optima) == 1
        assert got == optima[0] == want
    sc = seg_scores(counts)
    assert sc["assignment"] == got
    ref = SR.scores(counts, got)
    assert set(sc) == set(ref) | {"assignment"} and len([k for k in sc if k.startswith("seg_iou_")]) == counts.shape[1]
    for key, value in ref.items():
        assert sc[key] == value, key  # the same float64 divisions
    # under scipy's assignment the matched total, hence seg_acc, is the same
    assert sc["seg_acc"] == SR.scores(counts, want)["seg_acc"]
    if name == "zero_column":
        assert sc["seg_iou_3"] == 0.0 and sc["seg_miou"] == sum(sc[f"seg_iou_{k}"] for k in range(7) if k != 3) / 6


def test_a_hand_made_table():
    """Rows: clusters 0 and 1 and "nothing rendered"; columns: labels 0 (background), 1, 2.  Cluster 1 is label 1's (40 of its 50
    pixels), cluster 0 is label 2's, and the background pairs with the empty row."""
    counts = [[5, 10, 30],
              [0, 40, 5],
              [60, 0, 0]]
    assert match_clusters(counts) == [2, 1, 0]  # 60 + 40 + 30 = 130: every other choice is smaller (e.g. 5 + 40 + 0, 60 + 10 + 5)
    sc = seg_scores(torch.tensor(counts))
    assert sc["assignment"] == [2, 1, 0]
    assert sc["seg_acc"] == 130 / 150
    assert sc["seg_iou_0"] == 60 / (60 + 65 - 60) and sc["seg_iou_1"] == 40 / (45 + 50 - 40) and sc["seg_iou_2"] == 30 / (45 + 35 - 30)
    assert sc["seg_miou"] == (60 / 65 + 40 / 55 + 30 / 50) / 3
    assert seg_scores(torch.zeros(3, 3, dtype=torch.int64)) == {} and seg_scores([[0, 0]]) == {}
    # more labels than rows: a label is left without a row, scores 0 and still counts in the mean
    sc = seg_scores([[7, 3, 0]])
    assert sc["assignment"] == [0, -1, -1] and sc["seg_iou_1"] == 0.0 and sc["seg_miou"] == (7 / 10 + 0.0) / 2 and sc["seg_acc"] == 0.7


# ---- the C entry -------------------------------------------------------------------------------------------------------------------
def test_seg_confusion_argument_errors_come_back_before_any_launch(built_library):
    from umhsnerf import _hip

    lib = _hip.lib()
    ARG, UNSUP = -1, -2
    d = ctypes.c_void_p(4096)  # never dereferenced
    call = lambda **kw: lib.umhs_seg_confusion(*[kw.get(k, v) for k, v in dict(
        raw=d, acc=d, labels=d, n=64, C=6, L=7, ignore=255, counts=d, stream=None).items()])
    for missing in ("raw", "acc", "labels", "counts"):
        assert call(**{missing: None}) == ARG, missing
    assert call(n=-1) == ARG and call(C=0) == ARG and call(L=-3) == ARG
    assert call(C=17) == UNSUP and call(L=33) == UNSUP
    assert call(n=0) == 0 and call(n=0, C=16, L=32) == 0


def test_the_wrapper_has_no_cpu_path():
    from umhsnerf import ops

    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.seg_confusion(torch.zeros(4), torch.ones(4), torch.zeros(4, dtype=torch.uint8), 2, 2)
