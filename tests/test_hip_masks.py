"""Masked training frames on the GPU: ``umhs_mask_count`` / ``umhs_mask_compact`` (``ops.mask_lists``) and ``umhs_pixel_indices_masked``
against the CPU restatement (tests/mask_ref.py), and the layers above them -- ``ResidentSplit`` / ``UMHSDataManager`` with the stacks on
the device and in host memory, and training from a ``transforms.json`` whose frames carry ``mask_path``.

No tolerance anywhere: the lists are integers and every product of the draw is one float32 multiplication, so the kernels must give
the restatement's bits.  The cases (mask_ref.CASES) are the smallest shapes at which the kernels can go wrong:
  (a) n=5, 37x53: H*W odd (images start off the 16-byte granules the kernels load), no multiple of 64, empty first and last images, a
      single set pixel at the very end of an image, values 255 / 7 / 1;
  (b) n=3, 64x64: an image is exactly one chunk of 4,096 pixels; first and last pixel of every image set;
  (c) n=6, 2048x2048: M = 20,971,519 > 2^24 and odd, so (float)M rounds; an empty image inside the stack; 1,024 chunks per image;
  (d) n=1, 1x1."""
import functools
import json

import numpy as np
import pytest
import torch

import mask_ref as MR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def _ref(name):
    """(mask, off, list, uniform rows, restated indices) of a case, computed once on the CPU and never modified."""
    m = MR.CASES[name]()
    off, lst = MR.mask_lists(m)
    u = MR.uniform_rows()
    return m, off, lst, u, MR.pixel_indices_masked(u, off, lst, m.shape[2])


@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_lists_equal_the_restatement_fed_whole_and_frame_by_frame(name):
    from umhsnerf import ops

    m, off, lst, _, _ = _ref(name)
    got_off, got_lst = ops.mask_lists(m.to(DEV))
    assert got_off.dtype == torch.int64 and got_lst.dtype == torch.int32 and got_off.is_cuda and got_lst.is_cuda
    assert torch.equal(got_off.cpu(), off) and torch.equal(got_lst.cpu(), lst)
    host_off, host_lst = ops.mask_lists(m, device=DEV)  # from host memory: one frame on the device at a time
    assert host_lst.is_cuda and torch.equal(host_off, got_off) and torch.equal(host_lst, got_lst)


@pytest.mark.parametrize("shift", [1, 7, 16, 21])
def test_lists_do_not_depend_on_where_the_stack_starts(shift):
    """The chunks are cut on the 16-byte granules of the address space: the same stack at another alignment gives the same lists."""
    from umhsnerf import ops

    m, off, lst, _, _ = _ref("a")
    buf = torch.full((m.numel() + 64,), 255, dtype=torch.uint8, device=DEV)  # set bytes all around the stack: none may leak in
    view = buf[shift : shift + m.numel()].view(m.shape)
    view.copy_(m)
    assert view.data_ptr() % 16 == shift % 16
    got_off, got_lst = ops.mask_lists(view)
    assert torch.equal(got_off.cpu(), off) and torch.equal(got_lst.cpu(), lst)


@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_draw_equals_the_restatement(name):
    from umhsnerf import ops

    m, off, lst, u, want = _ref(name)
    w = m.shape[2]
    d_off, d_lst = off.to(DEV), lst.to(DEV)
    got = ops.pixel_indices_masked(u.to(DEV), d_off, d_lst, w)
    assert u.shape[0] == 200_005 and u.shape[0] % 256 != 0 and got.dtype == torch.int64 and got.shape == (200_005, 3)
    rows = got.cpu()
    assert torch.equal(rows, want)
    # independently of the restatement: every row is a set pixel of the mask
    assert bool((m[rows[:, 0], rows[:, 1], rows[:, 2]] != 0).all())
    one = ops.pixel_indices_masked(u[:1].to(DEV), d_off, d_lst, w)
    assert one.shape == (1, 3) and torch.equal(one.cpu(), want[:1])
    none = ops.pixel_indices_masked(u[:0].to(DEV), d_off, d_lst, w)
    assert none.shape == (0, 3) and none.dtype == torch.int64
    if name == "a":
        hit = torch.zeros_like(m, dtype=torch.bool)
        hit[rows[:, 0], rows[:, 1], rows[:, 2]] = True
        assert torch.equal(hit, m != 0)  # every set pixel is hit, and images 0 and 4 (empty) never
    if name == "c":
        assert int(off[-1]) == 20_971_519 and float(torch.tensor(int(off[-1])).float()) != int(off[-1])  # (float)M rounds here
        assert 1 not in rows[:, 0].unique().tolist()


# ---- ResidentSplit / UMHSDataManager --------------------------------------------------------------------------------------------
def _split(on_gpu=True, mask="rect", n=4, Hs=24, Ws=32, B=8, seed=3):
    """tests/test_hip_data.py's cameras on a sphere looking at the origin; ``mask``: "rect" (an off-centre rectangle per frame, frame 2
    empty), "zero", or None."""
    from umhsnerf.data.umhs_datamanager import ResidentSplit
    from umhsnerf.data.umhs_dataparser import Cameras

    g = torch.Generator().manual_seed(seed)
    pos = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1) * 0.9
    z = torch.nn.functional.normalize(pos, dim=-1)
    x = torch.nn.functional.normalize(torch.linalg.cross(torch.tensor([[0.0, 0, 1]]).expand(n, 3), z), dim=-1)
    y = torch.linalg.cross(z, x)
    c2w = torch.stack([x, y, z, pos], -1).contiguous()
    cams = Cameras(c2w, torch.full((n,), 30.0), torch.full((n,), 30.0), torch.full((n,), Ws / 2), torch.full((n,), Hs / 2), Hs, Ws)
    hs = torch.rand(n, Hs, Ws, B, generator=g)
    rgb = torch.rand(n, Hs, Ws, 3, generator=g)
    m = None
    if mask is not None:
        m = torch.zeros(n, Hs, Ws, dtype=torch.uint8)
        if mask == "rect":
            for i in range(n):
                if i != 2:
                    m[i, 3 + i : 15 + i, 5 : 20 + 2 * i] = 255
    return ResidentSplit(cams, rgb, hs, DEV, on_gpu=on_gpu, mask=m), rgb, hs, m


@pytest.mark.parametrize("on_gpu", [True, False])
def test_datamanager_draws_inside_the_mask(on_gpu):
    from umhsnerf import ops
    from umhsnerf.data.umhs_datamanager import UMHSDataManager, UMHSDataManagerConfig

    split, rgb, hs, m = _split(on_gpu)
    assert split.mask.is_cuda == on_gpu and split.mask.dtype == torch.uint8 and split.mask_off.is_cuda and split.mask_list.is_cuda
    off, lst = MR.mask_lists(m)
    assert torch.equal(split.mask_off.cpu(), off) and torch.equal(split.mask_list.cpu(), lst)
    cfg = lambda **kw: UMHSDataManagerConfig(train_num_rays_per_batch=1000, eval_num_rays_per_batch=500, images_on_gpu=on_gpu, **kw)
    dm = UMHSDataManager(cfg(), device=DEV, seed=5, train=split)
    rb, batch = dm.next_train(0)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(5)
    u = torch.rand((1000, 3), device=DEV, generator=gen)  # the same block the unmasked sampler draws
    idx = MR.pixel_indices_masked(u.cpu(), off, lst, 32)
    assert torch.equal(batch["indices"].cpu(), idx) and batch["indices"].is_cuda
    assert bool((m[idx[:, 0], idx[:, 1], idx[:, 2]] != 0).all()) and 2 not in idx[:, 0].tolist()
    assert torch.equal(batch["image"].cpu(), rgb[idx[:, 0], idx[:, 1], idx[:, 2]])
    assert torch.equal(batch["hs_image"].cpu(), hs[idx[:, 0], idx[:, 1], idx[:, 2]])
    o, d, area, nrm = ops.raygen(batch["indices"], split.c2w, split.intrinsics, want_area=True, want_norm=True)
    assert torch.equal(rb.origins, o) and torch.equal(rb.directions, d) and torch.equal(rb.pixel_area, area)
    assert torch.equal(rb.metadata["directions_norm"], nrm) and torch.equal(rb.camera_indices, batch["indices"][:, :1])
    if on_gpu:  # the masked path adds no host sync to next_train (torch's sync debug mode raises on one)
        torch.cuda.set_sync_debug_mode("error")
        try:
            dm.next_train(1)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    # next_eval follows the mask of the split it draws from; next_eval_image carries the mask
    ev = dm.next_eval(0)[1]["indices"].cpu()
    assert ev.shape == (500, 3) and bool((m[ev[:, 0], ev[:, 1], ev[:, 2]] != 0).all())
    for i in range(3):
        cam, full = dm.next_eval_image(i)
        assert full["mask"].shape == (24, 32, 1) and full["mask"].dtype == torch.bool and full["mask"].is_cuda
        assert torch.equal(full["mask"][..., 0].cpu(), m[i] != 0) and cam.directions.shape == (24, 32, 3)
    item = dm.train_dataset[1]
    assert item["mask"].shape == (24, 32, 1) and item["mask"].dtype == torch.bool and torch.equal(item["mask"][..., 0].cpu(), m[1] != 0)


def test_both_residencies_give_the_same_masked_batches():
    from umhsnerf.data.umhs_datamanager import UMHSDataManager, UMHSDataManagerConfig

    a, b = _split(True)[0], _split(False)[0]
    assert torch.equal(a.mask_off, b.mask_off) and torch.equal(a.mask_list, b.mask_list) and not b.mask.is_cuda
    dma = UMHSDataManager(UMHSDataManagerConfig(train_num_rays_per_batch=777), device=DEV, seed=4, train=a)
    dmb = UMHSDataManager(UMHSDataManagerConfig(train_num_rays_per_batch=777, images_on_gpu=False), device=DEV, seed=4, train=b)
    for step in range(3):
        (ra, ba), (rb, bb) = dma.next_train(step), dmb.next_train(step)
        assert torch.equal(ba["indices"], bb["indices"]) and torch.equal(ra.directions, rb.directions)
        assert torch.equal(ba["image"], bb["image"]) and torch.equal(ba["hs_image"], bb["hs_image"])


@pytest.mark.parametrize("on_gpu", [True, False])
def test_ignore_mask_reproduces_the_unmasked_split(on_gpu):
    from umhsnerf.data.umhs_datamanager import UMHSDataManager, UMHSDataManagerConfig

    masked, plain = _split(on_gpu)[0], _split(on_gpu, mask=None)[0]
    assert plain.mask is None and plain.mask_list is None
    mk = lambda split, **kw: UMHSDataManager(UMHSDataManagerConfig(train_num_rays_per_batch=1000, images_on_gpu=on_gpu, **kw), device=DEV,
                                             seed=5, train=split)
    dm_ignored, dm_plain, dm_masked = mk(masked, ignore_mask=True), mk(plain), mk(masked)
    for step in range(2):
        a, b, c = dm_ignored.next_train(step)[1], dm_plain.next_train(step)[1], dm_masked.next_train(step)[1]
        assert torch.equal(a["indices"], b["indices"]) and torch.equal(a["image"], b["image"]) and torch.equal(a["hs_image"], b["hs_image"])
        assert not torch.equal(a["indices"], c["indices"])
    assert torch.equal(dm_ignored.next_eval(0)[1]["indices"], dm_plain.next_eval(0)[1]["indices"])
    assert "mask" in dm_ignored.next_eval_image(0)[1] and "mask" not in dm_plain.next_eval_image(0)[1]  # still loaded


@pytest.mark.parametrize("on_gpu", [True, False])
def test_an_all_zero_mask_is_refused_when_the_split_is_built(on_gpu):
    with pytest.raises(ValueError, match="no pixel"):
        _split(on_gpu, mask="zero")
    from umhsnerf.data.umhs_datamanager import ResidentSplit

    good = _split(on_gpu, mask=None)[0]
    with pytest.raises(ValueError, match="mask must be"):
        ResidentSplit(good.cameras, good.image, good.hs_image, DEV, on_gpu=on_gpu, mask=torch.ones(4, 24, 31, dtype=torch.uint8))


# ---- on disk ---------------------------------------------------------------------------------------------------------------------
def _masked_scene(root, B=8, Hs=24, Ws=32):
    """The ``make_scene`` recipe of tests/test_hip_distortion.py plus an off-centre rectangle mask per frame (.npy, 255 inside); the
    cubes hold 0.6 inside the mask and 0.0 outside, so a batch row drawn outside a mask shows."""
    from test_hip_distortion import make_scene

    meta = make_scene(root, B=B, Hs=Hs, Ws=Ws)
    (root / "masks").mkdir()
    for k, fr in enumerate(meta["frames"]):
        m = np.zeros((Hs, Ws), dtype=np.uint8)
        m[2 + k : 14 + k, 4 + 2 * k : 18 + 2 * k] = 255
        name = "masks/" + fr["file_path"].replace("/", "_")
        np.save(root / name, m)
        fr["mask_path"] = name
        np.save(root / fr["hyperspectral_file_path"], np.where(m[:, :, None] != 0, np.float32(0.6), np.float32(0.0)) * np.ones((1, 1, B), np.float32))
    (root / "transforms.json").write_text(json.dumps(meta))
    return meta


@pytest.mark.parametrize("on_gpu", [True, False])
def test_batches_from_a_masked_scene_on_disk_stay_inside_the_masks(tmp_path, on_gpu):
    from umhsnerf.data.umhs_datamanager import UMHSDataManager, UMHSDataManagerConfig
    from umhsnerf.data.umhs_dataparser import UMHSDataParserConfig

    _masked_scene(tmp_path)
    mk = lambda **kw: UMHSDataManager(UMHSDataManagerConfig(dataparser=UMHSDataParserConfig(data=tmp_path), train_num_rays_per_batch=2048,
                                                            images_on_gpu=on_gpu, **kw), device=DEV, num_classes=3, seed=1)
    dm = mk()
    assert dm.train_split.mask.shape == (6, 24, 32) and dm.eval_split.mask.shape == (2, 24, 32) and dm.train_split.mask.is_cuda == on_gpu
    assert int(dm.train_split.mask_off[-1]) == 6 * 12 * 14 and int(dm.eval_split.mask_off[-1]) == 2 * 12 * 14
    for step in range(20):
        _, batch = dm.next_train(step)
        assert batch["hs_image"].shape == (2048, 8) and bool((batch["hs_image"] == 0.6).all()), step  # EVERY row lies inside a mask
    assert bool((dm.next_eval(0)[1]["hs_image"] == 0.6).all())
    _, full = dm.next_eval_image(0)
    assert torch.equal(full["mask"][..., 0], full["hs_image"][..., 0] == 0.6)
    outside = mk(ignore_mask=True).next_train(0)[1]["hs_image"]  # and without the masks the same scene does show its outside
    assert bool((outside == 0.0).any()) and bool((outside == 0.6).any())


def test_training_from_a_masked_scene_on_disk_reduces_the_loss(tmp_path):
    """As test_hip_distortion.test_training_from_a_distorted_scene_on_disk_reduces_the_loss asserts for its scene."""
    from umhsnerf.data.umhs_datamanager import UMHSDataManager, UMHSDataManagerConfig
    from umhsnerf.data.umhs_dataparser import UMHSDataParserConfig
    from umhsnerf.umhs_model import UMHSConfig
    from umhsnerf.umhs_pipeline import UMHSPipeline

    torch.manual_seed(0)
    B = 8
    meta = _masked_scene(tmp_path, B=B)
    dm = UMHSDataManager(UMHSDataManagerConfig(dataparser=UMHSDataParserConfig(data=tmp_path), train_num_rays_per_batch=2048), device=DEV,
                         num_classes=3, seed=1)
    cfg = UMHSConfig(method="rgb+spectral", pred_specular=True, temperature=0.4, background_color="black")
    pipe = UMHSPipeline.from_packed_samples(cfg, DEV, metadata={"wavelengths": meta["wavelengths"], "num_classes": 3}, seed=2, datamanager=dm)
    split = dm.train_split
    with torch.no_grad():  # a self-consistent target: rgb = converter(hs)
        split.image = pipe.model.converter(split.hs_image.view(-1, B)).view(*split.hs_image.shape[:3], 3).contiguous()
    losses = []
    for step in range(80):
        _, loss_dict, metrics = pipe.get_train_loss_dict(step)
        losses.append(float(sum(loss_dict.values()).detach()))
    assert np.isfinite(losses).all() and np.mean(losses[-10:]) < 0.5 * np.mean(losses[:5]), (losses[:5], losses[-10:])
