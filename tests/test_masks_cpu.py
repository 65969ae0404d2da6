"""Masks without a GPU: ``mask_path`` through the parser, ``load_mask`` / ``mask_color`` through the dataset, the argument checks of the
new exports (nothing is launched), and the properties of the CPU restatement (tests/mask_ref.py) the kernels are held to bit for bit."""
import ctypes
import json

import numpy as np
import pytest
import torch

import mask_ref as MR
from test_data_cpu import make_scene
from umhsnerf.data.umhs_dataparser import UMHSDataParserConfig
from umhsnerf.data.utils.hs_dataloader import HyperspectralDataset, load_mask

H, W = 6, 8


def _add_masks(root, which=lambda i, fr: True, writer=None, rgb_only=False, seed=1):
    """Adds ``mask_path`` (masks/<split>_<name>.npy, random 50 % of 255) to the frames of test_data_cpu.make_scene that ``which`` picks."""
    meta = json.loads((root / "transforms.json").read_text())
    rng = np.random.default_rng(seed)
    (root / "masks").mkdir(exist_ok=True)
    masks = {}
    for i, fr in enumerate(meta["frames"]):
        m = ((rng.random((H, W)) < 0.5) * 255).astype(np.uint8)
        m[0, 0], m[-1, -1] = 255, 0  # both kinds of pixel in every mask
        if rgb_only:
            np.save(root / fr["file_path"], np.load(root / fr["file_path"])[:, :, :3])
        if which(i, fr):
            name = "masks/" + fr["file_path"].replace("/", "_")
            fr["mask_path"] = (writer or (lambda p, a: np.save(p, a) or p))(root / name, m).relative_to(root).as_posix()
            masks[fr["file_path"]] = m
    (root / "transforms.json").write_text(json.dumps(meta))
    return masks


def test_parser_passes_mask_filenames_in_split_order(tmp_path):
    make_scene(tmp_path)
    _add_masks(tmp_path)
    parser = UMHSDataParserConfig(data=tmp_path, mask_color=(1.0, 0.0, 1.0)).setup()
    for split, n in (("train", 5), ("val", 2)):
        out = parser.get_dataparser_outputs(split)
        assert len(out.mask_filenames) == n == len(out.image_filenames)
        for img, msk in zip(out.image_filenames, out.mask_filenames):  # the same frames, in the same (sorted) order
            assert msk == tmp_path / "masks" / f"{img.parent.name}_{img.name}"
        assert out.metadata["mask_color"] == (1.0, 0.0, 1.0)


def test_parser_without_masks_and_with_masks_on_some_frames(tmp_path):
    make_scene(tmp_path)
    out = UMHSDataParserConfig(data=tmp_path).setup().get_dataparser_outputs("train")
    assert out.mask_filenames is None and "mask_color" in out.metadata and out.metadata["mask_color"] is None
    assert HyperspectralDataset(out).mask is None
    _add_masks(tmp_path, which=lambda i, fr: i != 3)
    with pytest.raises(AssertionError, match="mask"):
        UMHSDataParserConfig(data=tmp_path).setup().get_dataparser_outputs("train")


def test_npy_and_png_masks_give_the_same_stack(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    a, b = tmp_path / "npy", tmp_path / "png"
    for root in (a, b):
        root.mkdir()
        make_scene(root)

    def png(path, arr):
        path = path.with_suffix(".png")
        Image.fromarray(arr).save(path)  # uint8 H x W: mode "L"
        return path

    masks = _add_masks(a)
    _add_masks(b, writer=png)
    outs = [UMHSDataParserConfig(data=r).setup().get_dataparser_outputs("train") for r in (a, b)]
    assert all(p.suffix == ".png" for p in outs[1].mask_filenames)
    da, db = (HyperspectralDataset(o) for o in outs)
    assert da.mask.dtype == torch.uint8 and da.mask.shape == (5, H, W) and torch.equal(da.mask, db.mask)
    for i, p in enumerate(outs[0].image_filenames):
        np.testing.assert_array_equal(da.mask[i].numpy(), masks[f"train/{p.name}"])
    assert torch.equal(da.image, HyperspectralDataset(UMHSDataParserConfig(data=a).setup().get_dataparser_outputs("train")).image)


def test_load_mask_takes_one_channel_and_any_non_zero_value(tmp_path):
    m = np.zeros((H, W), dtype=np.uint8)
    m[1, 2], m[3, 4], m[5, 6] = 255, 1, 7
    np.save(tmp_path / "m.npy", m)
    got = load_mask(tmp_path / "m.npy")
    assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), m)  # uint8 values are kept: the sampler asks != 0
    np.save(tmp_path / "b.npy", m != 0)
    np.save(tmp_path / "f.npy", m.astype(np.float32) / 255.0)  # 1/255 must not truncate to "unset"
    for name in ("b.npy", "f.npy"):
        got = load_mask(tmp_path / name)
        assert got.dtype == torch.uint8 and np.array_equal(got.numpy() != 0, m != 0)
    np.save(tmp_path / "c3.npy", np.repeat(m[:, :, None], 3, axis=2))
    with pytest.raises(ValueError, match="one channel"):
        load_mask(tmp_path / "c3.npy")
    np.save(tmp_path / "c1.npy", m[:, :, None])
    with pytest.raises(ValueError, match="one channel"):
        load_mask(tmp_path / "c1.npy")


def test_three_channel_and_wrong_size_masks_are_refused_by_the_dataset(tmp_path):
    for sub, bad in (("rgb", lambda m: np.repeat(m[:, :, None], 3, axis=2)), ("size", lambda m: m[:, :-1])):
        root = tmp_path / sub
        root.mkdir()
        make_scene(root)
        _add_masks(root)
        out = UMHSDataParserConfig(data=root).setup().get_dataparser_outputs("train")
        np.save(out.mask_filenames[2], bad(np.load(out.mask_filenames[2])))
        with pytest.raises(ValueError, match="mask"):
            HyperspectralDataset(out)


def test_mask_color_rewrites_rgb_outside_the_mask_only(tmp_path):
    make_scene(tmp_path)
    _add_masks(tmp_path, rgb_only=True)
    plain = HyperspectralDataset(UMHSDataParserConfig(data=tmp_path).setup().get_dataparser_outputs("train"))
    ds = HyperspectralDataset(UMHSDataParserConfig(data=tmp_path, mask_color=(1, 0, 1)).setup().get_dataparser_outputs("train"))
    inside = ds.mask != 0
    assert 0 < int(inside.sum()) < inside.numel() and ds.image.shape == (5, H, W, 3) and ds.image.is_contiguous()
    assert torch.equal(ds.image[inside], plain.image[inside])
    assert torch.equal(ds.image[~inside], torch.tensor([1.0, 0.0, 1.0]).expand(int((~inside).sum()), 3))
    assert not torch.equal(ds.image, plain.image)
    assert torch.equal(ds.hs_image, plain.hs_image) and torch.equal(ds.mask, plain.mask)  # hs_image and the mask are untouched


def test_mask_color_on_an_rgba_stack_is_refused(tmp_path):
    make_scene(tmp_path)  # its frames are RGBA
    _add_masks(tmp_path)
    assert HyperspectralDataset(UMHSDataParserConfig(data=tmp_path).setup().get_dataparser_outputs("train")).image.shape[-1] == 4
    with pytest.raises(ValueError, match="mask_color"):
        HyperspectralDataset(UMHSDataParserConfig(data=tmp_path, mask_color=(1, 0, 1)).setup().get_dataparser_outputs("train"))


def test_datamanager_config_and_split_signature():
    import inspect

    from umhsnerf.data.umhs_datamanager import ResidentSplit, UMHSDataManagerConfig

    assert UMHSDataManagerConfig().ignore_mask is False
    params = list(inspect.signature(ResidentSplit.__init__).parameters)
    assert params == ["self", "cameras", "image", "hs_image", "device", "on_gpu", "mask"]  # mask last: splits are built positionally


def test_argument_errors_of_the_mask_exports_are_reported_before_anything_is_launched(built_library):
    """In the style of test_cabi_cpu.test_argument_errors_are_reported_before_anything_is_launched: no HIP call is made."""
    from umhsnerf import _hip

    lib = _hip.lib()
    ARG, UNSUP = -1, -2
    d = ctypes.c_void_p(4096)  # never dereferenced
    masked = lambda u=d, R=8, n=3, w=8, off=d, lst=d, out=d: lib.umhs_pixel_indices_masked(u, R, n, w, off, lst, out, None)
    for missing in ("u", "off", "lst", "out"):
        assert masked(**{missing: None}) == ARG, missing
    assert masked(R=-1) == ARG and masked(n=0) == ARG and masked(w=0) == ARG
    assert masked(R=0) == 0 and lib.umhs_pixel_indices_masked(None, 0, 3, 8, None, None, None, None) == 0  # nothing to do
    count = lambda m=d, n=2, px=48, c=d: lib.umhs_mask_count(m, n, px, c, None)
    assert count(m=None) == ARG and count(c=None) == ARG and count(n=-1) == ARG and count(px=0) == ARG
    assert count(n=0) == 0 and lib.umhs_mask_count(None, 0, 48, None, None) == 0
    assert count(px=(1 << 24) + 1) == UNSUP  # ids are int32 and a rank comes from one float32 uniform
    compact = lambda m=d, n=2, px=48, o=d, lst=d, cap=10: lib.umhs_mask_compact(m, n, px, o, lst, cap, None)
    assert compact(m=None) == ARG and compact(o=None) == ARG and compact(lst=None) == ARG and compact(cap=-1) == ARG and compact(px=0) == ARG
    assert compact(n=0) == 0 and compact(px=(1 << 24) + 1) == UNSUP
    # chunks per image: a function of H*W alone, enough for an image that starts at any byte of a 16-byte granule
    assert lib.umhs_mask_chunks(0) == 0 and lib.umhs_mask_chunks(1) == 1 and lib.umhs_mask_chunks(4096 - 15) == 1
    assert lib.umhs_mask_chunks(4096 - 14) == 2 and lib.umhs_mask_chunks(1 << 24) == 4097


def test_ops_refuse_host_tensors_and_wrong_types():
    from umhsnerf import ops

    with pytest.raises(ValueError, match="uint8"):
        ops.mask_lists(torch.ones(2, 4, 4))
    with pytest.raises(ValueError, match="uint8"):
        ops.mask_lists(torch.ones(4, 4, dtype=torch.uint8))
    off, lst = MR.mask_lists(MR.case_d())
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.pixel_indices_masked(torch.rand(4, 3), off, lst, 1)
    with pytest.raises(ValueError, match="int64"):
        ops.pixel_indices_masked(torch.rand(4, 3), off.to(torch.int32), lst, 1)


# ---- the restatement itself ----------------------------------------------------------------------------------------------------
def test_restated_lists_are_the_nonzero_order():
    m = MR.case_a()
    off, lst = MR.mask_lists(m)
    assert off.dtype == torch.int64 and lst.dtype == torch.int32 and off[0] == 0 and int(off[-1]) == lst.numel() == int((m != 0).sum())
    cnt = (off[1:] - off[:-1]).tolist()
    assert cnt[0] == 0 and cnt[2] == 1 and cnt[3] == 37 * 53 and cnt[4] == 0 and 0.2 * 1961 < cnt[1] < 0.4 * 1961
    assert int(lst[off[2]]) == 37 * 53 - 1  # the very last pixel of image 2
    for i in range(5):
        ids = lst[off[i] : off[i + 1]].long()
        assert bool((ids[1:] > ids[:-1]).all()) and bool((m[i].view(-1)[ids] != 0).all())


def test_restated_draw_is_uniform_over_the_set_pixels_of_case_a():
    m = MR.case_a()
    off, lst = MR.mask_lists(m)
    u = torch.rand(200_000, 3, generator=torch.Generator().manual_seed(0))
    rows = MR.pixel_indices_masked(u, off, lst, 53)
    assert rows.dtype == torch.int64 and rows.shape == (200_000, 3)
    assert bool((m[rows[:, 0], rows[:, 1], rows[:, 2]] != 0).all())  # every pick lies inside the mask
    assert set(rows[:, 0].unique().tolist()) == {1, 2, 3}  # images 0 and 4 are empty: never chosen
    hit = torch.zeros_like(m, dtype=torch.bool)
    hit[rows[:, 0], rows[:, 1], rows[:, 2]] = True
    assert torch.equal(hit, m != 0)  # every set pixel is hit (200,000 draws over ~2,550 pixels)
    # uniform over the pixels, not over the images: image 3 (all set) gets its share of M
    share = float((rows[:, 0] == 3).float().mean())
    assert abs(share - 1961 / int(off[-1])) < 0.01
    # column 2 is unused
    u2 = u.clone()
    u2[:, 2] = 0.25
    assert torch.equal(MR.pixel_indices_masked(u2, off, lst, 53), rows)


def test_restated_draw_clamps_at_one_and_handles_the_crafted_rows():
    for name in ("a", "b", "d"):
        m = MR.CASES[name]()
        n, h, w = m.shape
        off, lst = MR.mask_lists(m)
        rows = MR.pixel_indices_masked(MR.crafted_rows(), off, lst, w)
        first = torch.nonzero(m.view(-1))[0, 0]
        last = torch.nonzero(m.view(-1))[-1, 0]
        as_row = lambda f: [int(f) // (h * w), int(f) % (h * w) // w, int(f) % w]
        assert rows[0].tolist() == as_row(first)  # u = 0: the first set pixel of the stack
        assert rows[1].tolist() == as_row(last)  # u = 1.0 clamps to the last set pixel
        assert bool((m[rows[:, 0], rows[:, 1], rows[:, 2]] != 0).all())
        i_last, i_first = rows[3, 0], rows[4, 0]  # (1.0, 0): first pixel of the last non-empty image; (0, 1.0): last of the first
        assert rows[3].tolist() == [int(i_last)] + as_row(lst[off[i_last]])[1:] and int(i_last) == as_row(last)[0]
        assert rows[4].tolist() == [int(i_first)] + as_row(lst[off[i_first + 1] - 1])[1:] and int(i_first) == as_row(first)[0]
    assert MR.pixel_indices_masked(torch.zeros(0, 3), off, lst, 1).shape == (0, 3)
