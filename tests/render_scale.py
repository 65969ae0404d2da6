"""Whole-frame renders at frame scale against a float64 oracle: the scene, the frames, the selected rays, their float64 truth and the
comparator (plain helper module, no tests in it).

Used by tests/test_hip_render_scale.py (``UMHSModel.get_outputs_for_camera_ray_bundle`` on the GPU: three chunks, every heads workgroup
looping) and tests/test_render_scale_cpu.py (the comparator passes the float32 oracle and rejects planted chunk-loop and tile faults).

STATE.  Oracle parameters as tests/test_hip_fullsize.py::_bench_state makes them (``T.FieldParams``, table U(+-0.5), density bias
+1.5), loaded into a ``UMHSPipeline.from_packed_samples`` model through ``reference_state_dict()``: the oracle owns the same numbers.

SCENE.  A ball (centre (0.15, -0.4, 0.55), radius 0.34) and a slab ([-0.7, 0.8] x [-1, -0.75] x [0.2, 0.9]) written by hand into level
0 of the occupancy grid (a cell is occupied when its centre is inside either); nothing is trained.  One pinhole camera at (0, 0, 3)
looking down -z, 40 degrees vertical field of view, 259 x 254 pixels = 2 x 32768 + 250 rays (250 % 64 = 58), step 0.006:
  chunk 0  rays     0 .. 32767   rows 0 .. 126: above the ball, no sample; the sampler hands out its one fake sample
  chunk 1  rays 32768 .. 65535   the ball (mean chord 0.45 = 76 samples, nearer than the slab: the chunks clip depth to different ranges) and the upper rows of the slab: > 8 x 65,536 samples
  chunk 2  rays 65536 .. 65785   250 rays of the last row: through the slab at 20 degrees, ~110 samples per ray
``assert_shape`` holds a frame to all of it, so that a drift of the scene fails loudly instead of thinning the coverage.
What the frame does NOT do: chunk 2 holds longer rays but, with 250 of them, far fewer samples than chunk 1, and the workspace slots
are sized by samples and rays -- they are re-grown once in the frame (from the fake sample's to chunk 1's) and never by the partial
chunk.  A slot re-grown between two chunks that both hold samples is not covered here.

FRAMES.  On the GPU a frame's samples are ``model.sample(chunk)`` -- the deterministic eval march of the forward itself.  Without a GPU
``analytic_march`` stands in: the same step through the exact ball and slab (not their voxelisation), enough to give the CPU test a
frame of the same shape.  Either way a ``Frame`` is a list of ``Chunk``s holding rays, packed samples and optional per-ray planes.

SELECTION (``select``): the first and last ray of every chunk (= both sides of every chunk border); every ray whose samples straddle
a multiple of 65,536 samples of its chunk (where a heads workgroup's loop iteration changes) and the ray after it; the longest ray; rays
with 0 and with 1 sample; a seeded random remainder (half of it among the rays that have samples) up to 256.

TRUTH (``truth``): ``T.model_outputs`` on the selected rays' packed samples, chunk by chunk, with the chunk's own [min, max] of t_mid
as the depth clip range (the clip is per launch, in the reference and here).  ``decided``: a ray's label counts when the float64 top-2
gap of seg_probs is above 1e-3 and its accumulation is more than 1e-3 from the 0.5 threshold seg_raw multiplies by (as much a tie as
the gap); at least 98 % of the selected rays with samples must be decided -- on the oracle alone (``assert_labels_cap``).

COMPARATOR (``compare``): the model-level tolerances of tests/model_golden.py -- ``GPU_OUT_MAX`` (1e-4 of the tensor's maximum) and
``GPU_OUT_ELEM`` (rtol 1e-4, atol 1e-6 per element); num_samples_per_ray and decided labels exact.  ``Report`` collects every figure
(worst |diff| / tolerance) and writes them to ``render_scale.json`` in ``rays_f64.report_dir()``."""
from __future__ import annotations

import contextlib
import json
import math
import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

import model_golden as MG
from oracle import torch_ref as T

W, H = 259, 254
CHUNK = 32768
TILE = 65536  # 256 workgroups x 256 samples: one iteration of umhs_field_heads_fwd's persistent loop
STEP = 0.006
FOV = 40.0
CAMERA = (0.0, 0.0, 3.0)
BALL = ((0.15, -0.4, 0.55), 0.34)
SLAB = (-0.7, -1.0, 0.2, 0.8, -0.75, 0.9)
CROP = {"center": (0.1, -0.6, 0.35), "scale": (1.3, 0.9, 1.3)}  # an axis-aligned box that cuts the ball and the slab
NEAR_FLOOR = 0.05
N_SELECT = 256
GAP = 1e-3
EXACT = ("seg_raw", "seg_pred", "num_samples_per_ray")
SKIP = ("weights",)  # per sample, not per ray

# mode -> (method, pred_specular, C, B, temperature, parameter seed)
# (the seeds: the first of 40 .. 79 with which 98 % of the selected rays have a decided label -- with random endmembers every ray of a
# frame renders much the same mixture, so a seed decides nearly all labels or nearly none; 55 gives 99.4 %, 49 gives 98.8 %)
STATES = {"spec_b31": ("rgb+spectral", True, 6, 31, 0.4, 55), "nospec_b141": ("spectral", False, 4, 141, 0.7, 49),
          "rgb": ("rgb", False, 5, 21, 0.4, 42)}


@contextlib.contextmanager
def threads():
    """At most 16 CPU threads for the oracles while active; the process's setting comes back afterwards."""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    before = torch.get_num_threads()
    torch.set_num_threads(max(1, min(n, 16)))
    try:
        yield
    finally:
        torch.set_num_threads(before)


# ------------------------------------------------------------------------------------------------------------------------------ #
# state
# ------------------------------------------------------------------------------------------------------------------------------ #
def make_params(state: str) -> T.FieldParams:
    """tests/test_hip_fullsize.py::_bench_state for one of STATES."""
    method, spec, C, B, _, seed = STATES[state]
    p = T.FieldParams(C, B, spec, method, table_scale=0.5, seed=seed)
    with torch.no_grad():
        p.base_b[1][0] += 1.5
    return p


def bands_of(state: str) -> List[float]:
    return [float(b) for b in np.linspace(400, 700, STATES[state][3])]


def class_colors() -> torch.Tensor:
    from umhsnerf.umhs_model import CLASS_COLORS

    return CLASS_COLORS.clone()


def make_pipeline(state: str, p: T.FieldParams, device):
    from umhsnerf.umhs_model import UMHSConfig
    from umhsnerf.umhs_pipeline import UMHSPipeline

    method, spec, C, _, temp, _ = STATES[state]
    cfg = UMHSConfig(method=method, pred_specular=spec, temperature=temp, render_step_size=STEP, cone_angle=0.0)
    pipe = UMHSPipeline.from_packed_samples(cfg, torch.device(device), metadata={"wavelengths": bands_of(state), "num_classes": C}, seed=3)
    pipe.model.field.load_state_dict(p.reference_state_dict())
    write_grid(pipe.model)
    pipe.model.eval()
    return pipe


# ------------------------------------------------------------------------------------------------------------------------------ #
# scene
# ------------------------------------------------------------------------------------------------------------------------------ #
def occupancy(res: int) -> torch.Tensor:
    """Level 0 of the grid over [-1, 1]^3, bool [res, res, res] indexed (x, y, z): cells whose centre is in the ball or the slab."""
    c = (torch.arange(res, dtype=torch.float64) + 0.5) * (2.0 / res) - 1.0
    x, y, z = torch.meshgrid(c, c, c, indexing="ij")
    (bx, by, bz), r = BALL
    ball = (x - bx) ** 2 + (y - by) ** 2 + (z - bz) ** 2 < r * r
    x0, y0, z0, x1, y1, z1 = SLAB
    slab = (x > x0) & (x < x1) & (y > y0) & (y < y1) & (z > z0) & (z < z1)
    return ball | slab


def write_grid(model) -> None:
    grid = model.sampler.occupancy_grid
    assert grid._roi == [-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]
    b = torch.zeros_like(grid.binaries)
    b[0] = occupancy(grid.res).to(b.device)
    grid.binaries = b
    grid.occs.fill_(0.0)
    grid.occs[: grid.cells_per_lvl] = b[0].flatten().float()


def camera_path() -> dict:
    x, y, z = CAMERA
    return {"render_height": H, "render_width": W, "camera_type": "perspective",
            "camera_path": [{"camera_to_world": [1, 0, 0, x, 0, 1, 0, y, 0, 0, 1, z, 0, 0, 0, 1], "fov": FOV}]}


def cpu_rays():
    """The frame's rays without a GPU (``T.generate_rays`` with the intrinsics ``render.load_camera_path`` gives) -> origins, directions [H W, 3]."""
    focal = (H / 2.0) / math.tan(FOV * math.pi / 360.0)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    idx = torch.stack([torch.zeros_like(yy), yy, xx], -1).reshape(-1, 3)
    c2w = torch.tensor([[1, 0, 0, CAMERA[0]], [0, 1, 0, CAMERA[1]], [0, 0, 1, CAMERA[2]]], dtype=torch.float32)[None]
    o, d, _, _ = T.generate_rays(idx, c2w, torch.tensor([[focal, focal, W / 2.0, H / 2.0]], dtype=torch.float32))
    return o.contiguous(), d.contiguous()


def _box_interval(o, d, lo, hi):
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / d
        a, b = (lo - o) * inv, (hi - o) * inv
    a, b = np.where(np.isnan(a), -np.inf, a), np.where(np.isnan(b), np.inf, b)
    return np.minimum(a, b).max(1), np.maximum(a, b).min(1)


def cpu_crop_planes(o, d):
    """Per-ray entry into (floored at NEAR_FLOOR) and exit from CROP, both 1e10 on a miss, [R,1] float32 (what the ray generator gives)."""
    o64, d64 = o.double().numpy(), d.double().numpy()
    c, s = np.asarray(CROP["center"]), np.asarray(CROP["scale"])
    ta, tb = _box_interval(o64, d64, c - s / 2, c + s / 2)
    ta = np.maximum(ta, NEAR_FLOOR)
    miss = ~(ta < tb)
    near, far = np.where(miss, 1e10, ta), np.where(miss, 1e10, tb)
    return torch.from_numpy(near).float()[:, None], torch.from_numpy(far).float()[:, None]


def analytic_march(o: torch.Tensor, d: torch.Tensor, nears=None, fars=None):
    """The stand-in march: per ray, samples [t, t + STEP) from the entry into the exact ball / slab while the mid-point lies before the
    exit, the two objects in order along the ray, inside [nears, fars] where given -> (ray_indices, t0, t1) packed, float32 times."""
    o64, d64 = o.double().numpy(), d.double().numpy()
    R = o64.shape[0]
    near = np.full(R, NEAR_FLOOR) if nears is None else nears.double().numpy().reshape(-1)
    far = np.full(R, 1e3) if fars is None else fars.double().numpy().reshape(-1)
    (cx, cy, cz), r = BALL
    oc = o64 - np.array([cx, cy, cz])
    b, c = (oc * d64).sum(1), (oc * oc).sum(1) - r * r
    disc = b * b - c
    root = np.sqrt(np.maximum(disc, 0.0))
    ball = (np.where(disc > 0, -b - root, np.inf), np.where(disc > 0, -b + root, -np.inf))
    slab = _box_interval(o64, d64, np.array(SLAB[:3]), np.array(SLAB[3:]))
    ri, t0 = [], []
    order = ball[0] <= slab[0]
    for first in (True, False):  # the nearer object of every ray, then the farther one
        ta = np.where(order == first, ball[0], slab[0])
        tb = np.where(order == first, ball[1], slab[1])
        ta, tb = np.maximum(ta, near), np.minimum(tb, far)
        n = np.where(tb > ta, np.ceil((tb - ta) / STEP - 0.5), 0).astype(np.int64)
        n = np.maximum(n, 0)
        rays = np.repeat(np.arange(R), n)
        k = np.arange(n.sum()) - np.repeat(np.cumsum(n) - n, n)
        ri.append(rays)
        t0.append(np.where(np.isfinite(ta), ta, 0.0)[rays] + k * STEP)
    ri, t0 = np.concatenate(ri), np.concatenate(t0)
    keep = np.lexsort((t0, ri))
    ri, t0 = ri[keep], t0[keep].astype(np.float32)
    return torch.from_numpy(ri), torch.from_numpy(t0), torch.from_numpy((t0 + np.float32(STEP)).astype(np.float32))


# ------------------------------------------------------------------------------------------------------------------------------ #
# frames
# ------------------------------------------------------------------------------------------------------------------------------ #
@dataclass
class Chunk:
    r0: int  # first ray of the chunk in the frame
    o: torch.Tensor  # [R,3] the chunk's rays (CPU, float32)
    d: torch.Tensor
    ri: torch.Tensor  # [n] int64, chunk-local
    t0: torch.Tensor  # [n] float32
    t1: torch.Tensor
    fake: bool = False  # no sample survived: ``ri, t0, t1`` are the sampler's one fake sample (ray 0, t = 1 .. 1)
    nears: Optional[torch.Tensor] = None
    fars: Optional[torch.Tensor] = None
    pinfo: torch.Tensor = field(init=False)

    def __post_init__(self):
        self.pinfo = T.pack_info(self.ri, self.R)

    @property
    def R(self) -> int:
        return self.o.shape[0]

    @property
    def n(self) -> int:
        return int(self.ri.numel())

    @property
    def counts(self) -> torch.Tensor:
        return self.pinfo[:, 1]

    def clip_range(self, dtype=torch.float64):
        mid = (self.t0.to(dtype) + self.t1.to(dtype)) / 2
        return (mid.min(), mid.max()) if mid.numel() else (torch.zeros((), dtype=dtype), torch.zeros((), dtype=dtype))


def make_chunk(r0, o, d, ri, t0, t1, nears=None, fars=None, fake: bool = False) -> Chunk:
    """A chunk from what a march gave; an empty march becomes nerfstudio's one fake sample, as ``VolumetricSampler.forward`` makes it
    (``fake``: the march was the model's own, and that sample is in ``ri, t0, t1`` already)."""
    if ri.numel() == 0:
        fake = True
        ri, t0, t1 = torch.zeros(1, dtype=torch.int64), torch.ones(1), torch.ones(1)
    return Chunk(r0, o.float().cpu(), d.float().cpu(), ri.long().cpu(), t0.float().cpu().reshape(-1), t1.float().cpu().reshape(-1), fake,
                 None if nears is None else nears.float().cpu(), None if fars is None else fars.float().cpu())


@dataclass
class Frame:
    chunks: List[Chunk]

    @property
    def R(self) -> int:
        return sum(c.R for c in self.chunks)

    @property
    def counts(self) -> torch.Tensor:
        return torch.cat([c.counts for c in self.chunks])

    def chunk_of(self, ray: int) -> int:
        return next(i for i, c in enumerate(self.chunks) if c.r0 <= ray < c.r0 + c.R)


def cpu_frame(crop: bool = False, planes_from: Optional[Dict[int, int]] = None, planes_shift: Optional[Dict[int, int]] = None) -> Frame:
    """The frame through ``analytic_march``.  ``planes_from`` {chunk: other chunk}: march that chunk inside the OTHER chunk's
    nears / fars rows; ``planes_shift`` {chunk: rays}: inside its own rows moved by that many rays (planted faults of the chunk
    loop's slicing)."""
    o, d = cpu_rays()
    nears, fars = cpu_crop_planes(o, d) if crop else (None, None)
    chunks = []
    for i, r0 in enumerate(range(0, o.shape[0], CHUNK)):
        sl = slice(r0, r0 + CHUNK)
        nf = (None, None)
        if crop:
            j = (planes_from or {}).get(i, i)
            k, a = o[sl].shape[0], j * CHUNK + (planes_shift or {}).get(i, 0)
            nf = (nears[a: a + k], fars[a: a + k])
        chunks.append(make_chunk(r0, o[sl], d[sl], *analytic_march(o[sl], d[sl], *nf), *nf))
    return Frame(chunks)


def model_frame(model, bundle) -> Frame:
    """The frame as the model samples it: ``model.sample`` of every chunk of ``bundle`` (a [H,W] RayBundle on the model's device),
    sliced as ``_camera_ray_bundle_outputs`` slices it."""
    from umhsnerf._ns_compat import RayBundle

    o, d = bundle.origins.reshape(-1, 3), bundle.directions.reshape(-1, 3)
    planes = bundle.nears is not None and bundle.fars is not None
    nears, fars = (bundle.nears.reshape(-1, 1), bundle.fars.reshape(-1, 1)) if planes else (None, None)
    chunks = []
    with torch.no_grad():
        for r0 in range(0, o.shape[0], CHUNK):
            sl = slice(r0, r0 + CHUNK)
            rb = RayBundle(origins=o[sl], directions=d[sl])
            if planes:
                rb.nears, rb.fars = nears[sl], fars[sl]
            rs, ri = model.sample(rb)
            fr = rs.frustums
            fake = model.sampler.last_packed_info is None  # VolumetricSampler's "one fake sample" branch
            ch = make_chunk(r0, o[sl], d[sl], ri, fr.starts, fr.ends, nears[sl] if planes else None, fars[sl] if planes else None, fake)
            assert not fake or (ch.n == 1 and float(ch.t0[0]) == float(ch.t1[0]) == 1.0 and int(ch.ri[0]) == 0)
            chunks.append(ch)
    return Frame(chunks)


def shape_facts(frame: Frame) -> Dict:
    c = frame.chunks
    hit = [ch.counts[ch.counts > 0] if not ch.fake else ch.counts[:0] for ch in c]
    return {"rays": [ch.R for ch in c], "samples": [0 if ch.fake else ch.n for ch in c],
            "hit_rays": [int(h.numel()) for h in hit], "samples_per_hit_ray": [float(h.double().mean()) if h.numel() else 0.0 for h in hit],
            "longest_ray": [int(ch.counts.max()) for ch in c], "heads_loop_iterations": [-(-ch.n // TILE) for ch in c]}


def assert_shape(frame: Frame) -> Dict:
    """The coverage claims of the module docstring, asserted on the frame itself -> ``shape_facts``."""
    f, c = shape_facts(frame), frame.chunks
    assert frame.R == H * W == 2 * CHUNK + 250 and [ch.R for ch in c] == [CHUNK, CHUNK, 250], f
    r = c[2].R
    assert 0 < r < CHUNK and r % 64 != 0
    assert c[0].fake and c[0].n == 1 and not c[1].fake and not c[2].fake, f  # chunk 0 takes the sampler's fake-sample branch
    assert c[1].n > 8 * TILE, f  # every heads workgroup loops at least 8 times
    assert c[1].n > 8 * c[0].n, f  # every workspace slot is re-grown once, from chunk 0's one sample to chunk 1 (not again: see SCENE)
    assert f["samples_per_hit_ray"][2] > f["samples_per_hit_ray"][1], f  # the partial chunk holds the longer rays
    assert 64 <= f["samples_per_hit_ray"][1] <= 128 and 64 <= f["samples_per_hit_ray"][2] <= 128, f
    for ch in c[1:]:
        assert int((ch.counts == 0).sum()) > 0, f
    assert any(int((ch.counts == 1).sum()) > 0 for ch in c[1:]), f
    assert max(f["longest_ray"]) < 1024, f
    return f


# ------------------------------------------------------------------------------------------------------------------------------ #
# selection
# ------------------------------------------------------------------------------------------------------------------------------ #
def straddlers(ch: Chunk) -> torch.Tensor:
    """Chunk-local rays whose samples lie on both sides of a multiple of TILE samples of the chunk's packed order."""
    s, c = ch.pinfo[:, 0], ch.pinfo[:, 1]
    return torch.nonzero((c > 0) & (s // TILE != (s + c - 1).clamp(min=0) // TILE)).reshape(-1)


def select(frame: Frame, seed: int = 0, n: int = N_SELECT) -> Dict[str, List[int]]:
    """-> {kind: global ray indices}; ``selected(kinds)`` is their sorted union."""
    kinds: Dict[str, List[int]] = {"first_of_chunk": [], "last_of_chunk": [], "straddle": [], "after_straddle": [], "longest": [],
                                   "zero": [], "one": []}
    counts = frame.counts
    for ch in frame.chunks:
        kinds["first_of_chunk"].append(ch.r0)
        kinds["last_of_chunk"].append(ch.r0 + ch.R - 1)
        if ch.fake:
            continue
        st = straddlers(ch)
        kinds["straddle"] += [ch.r0 + int(r) for r in st]
        kinds["after_straddle"] += [ch.r0 + int(r) + 1 for r in st if int(r) + 1 < ch.R]
        kinds["zero"] += [ch.r0 + int(r) for r in torch.nonzero(ch.counts == 0).reshape(-1)[:2]]
        kinds["one"] += [ch.r0 + int(r) for r in torch.nonzero(ch.counts == 1).reshape(-1)[:2]]
    live = torch.cat([ch.counts if not ch.fake else torch.zeros_like(ch.counts) for ch in frame.chunks])
    kinds["longest"].append(int(live.argmax()))
    g = torch.Generator().manual_seed(seed)
    taken = set(sum(kinds.values(), []))
    hit = torch.nonzero(live > 0).reshape(-1)
    rest = max(0, n - len(taken))
    draw = [int(hit[i]) for i in torch.randperm(hit.numel(), generator=g)[: rest // 2 + 64]]
    draw += [int(i) for i in torch.randperm(frame.R, generator=g)[: rest + 64]]
    kinds["random"] = []
    a, b = draw[: rest // 2 + 64], draw[rest // 2 + 64:]
    for r in [x for pair in zip(a, b) for x in pair]:  # alternate: one among the rays with samples, one anywhere, until n are taken
        if len(taken) >= n:
            break
        if r not in taken:
            taken.add(r)
            kinds["random"].append(r)
    assert counts.numel() == frame.R
    return kinds


def selected(kinds: Dict[str, List[int]]) -> List[int]:
    return sorted(set(sum(kinds.values(), [])))


def assert_selection(frame: Frame, kinds: Dict[str, List[int]]) -> None:
    """Every kind of ray the module docstring lists is there."""
    counts, c = frame.counts, frame.chunks
    assert len(kinds["first_of_chunk"]) == len(kinds["last_of_chunk"]) == 3
    borders = {CHUNK - 1, CHUNK, 2 * CHUNK - 1, 2 * CHUNK, 0, frame.R - 1}
    assert borders <= set(selected(kinds))
    # (a multiple of TILE may fall between two rays: then no ray straddles it)
    assert len(kinds["straddle"]) >= max(8, (c[1].n - 1) // TILE - 2) and kinds["after_straddle"], kinds["straddle"]
    for r in kinds["straddle"]:
        ch = c[frame.chunk_of(r)]
        s, k = (int(v) for v in ch.pinfo[r - ch.r0])
        assert s // TILE < (s + k - 1) // TILE
    assert all(int(counts[r]) == 0 for r in kinds["zero"]) and len(kinds["zero"]) >= 2
    assert all(int(counts[r]) == 1 for r in kinds["one"]) and len(kinds["one"]) >= 1
    assert int(counts[kinds["longest"][0]]) == max(int(ch.counts.max()) for ch in c)
    assert len(kinds["random"]) >= 64 and len(selected(kinds)) >= min(N_SELECT, 200)


# ------------------------------------------------------------------------------------------------------------------------------ #
# truth
# ------------------------------------------------------------------------------------------------------------------------------ #
def gather_rays(ch: Chunk, local: Sequence[int]):
    """The packed samples of the chunk-local rays ``local`` (in that order) -> (origins, directions [N,3], t0, t1 [N], ray ids 0..k-1 [N])."""
    local = torch.as_tensor(list(local), dtype=torch.int64)
    cnt = ch.pinfo[local, 1]
    idx = torch.repeat_interleave(ch.pinfo[local, 0], cnt) + (torch.arange(int(cnt.sum())) - torch.repeat_interleave(cnt.cumsum(0) - cnt, cnt))
    ri = torch.repeat_interleave(torch.arange(local.numel()), cnt)
    rays = local[ri]
    return ch.o[rays], ch.d[rays], ch.t0[idx], ch.t1[idx], ri, idx


def truth(p: T.FieldParams, frame: Frame, rays: Sequence[int], state: str, dtype=torch.float64, clip_from: Optional[Dict[int, int]] = None,
          render=None) -> Dict[str, torch.Tensor]:
    """``T.model_outputs`` in ``dtype`` on the rays ``rays`` (global, ascending) of the frame, chunk by chunk with the chunk's own depth
    clip range -> {key: [len(rays), ...]}.  ``p`` must be of that dtype.  ``clip_from`` {chunk: other chunk}: clip that chunk's depth
    with the OTHER chunk's range (a planted fault).  ``render(chunk, o, d, t0, t1, ri, k, idx, clip)``: another oracle of the same
    signature of results (the edited / regional renders of tests/material_f64.py and tests/region_f64.py, normals)."""
    assert list(rays) == sorted(rays)
    temp, M, colors = STATES[state][4], T.colour_matrix(bands_of(state)), class_colors()
    outs: Dict[str, List[torch.Tensor]] = {}
    for i, ch in enumerate(frame.chunks):
        local = [r - ch.r0 for r in rays if ch.r0 <= r < ch.r0 + ch.R]
        if not local:
            continue
        k = len(local)
        if int(ch.counts[torch.as_tensor(local)].sum()) < 2:  # (the oracles squeeze a batch of one sample and take no empty one: the chunk's
            local = local + [int(ch.counts.argmax())] * 2  # longest ray rides along, twice for the fake sample's sake; its rows are dropped)
        o, d, t0, t1, ri, idx = gather_rays(ch, local)
        clip = frame.chunks[(clip_from or {}).get(i, i)].clip_range(dtype)
        with torch.no_grad():
            if render is not None:
                out = render(ch, o, d, t0, t1, ri, len(local), idx, clip)
            else:
                out = T.model_outputs(p, o.to(dtype), d.to(dtype), t0.to(dtype)[:, None], t1.to(dtype)[:, None], ri, len(local), temp,
                                      M.to(dtype), depth_clip_range=clip, class_colors=colors.to(dtype))
        for key, v in out.items():
            if key not in SKIP and torch.is_tensor(v) and v.shape[:1] == (len(local),):
                outs.setdefault(key, []).append(v.detach().reshape(len(local), -1)[:k])
    return {k: torch.cat(v) for k, v in outs.items()}


def decided(t64: Dict[str, torch.Tensor]) -> torch.Tensor:
    """Rays whose label is decided (module docstring), bool [k]."""
    top = t64["seg_probs"].double().topk(2, dim=1).values
    return ((top[:, 0] - top[:, 1]) > GAP) & ((t64["accumulation"].double().reshape(-1) - 0.5).abs() > GAP)


def assert_labels_cap(t64: Dict[str, torch.Tensor]) -> float:
    live = t64["num_samples_per_ray"].reshape(-1) > 0
    share = float(decided(t64)[live].double().mean())
    assert share >= 0.98, f"only {share:.3f} of the selected rays with samples have a decided label"
    return share


# ------------------------------------------------------------------------------------------------------------------------------ #
# comparator
# ------------------------------------------------------------------------------------------------------------------------------ #
class Report:
    """Worst |diff| / tolerance per (mode, check, tensor), written to ``render_scale.json`` of the run-output directory; ``check``
    collects instead of stopping at the first miss (``MG.Report``'s pattern)."""

    def __init__(self, mode: str, what: str):
        self.mode, self.what, self.figures, self.misses, self.checked = mode, what, {}, [], set()

    def check(self, name: str, r: float, note: str = ""):
        self.figures[name] = max(r, self.figures.get(name, 0.0))
        self.checked.add(name)
        if not r <= 1.0:
            self.misses.append(f"{name}: {r:.3g} x its tolerance{note}")

    def note(self, name: str, value):
        self.figures[name] = value

    @property
    def worst(self) -> float:
        return max([self.figures[k] for k in self.checked] or [0.0])

    def finish(self, root: str, strict: bool = True):
        import rays_f64

        path = os.path.join(rays_f64.report_dir(root), "render_scale.json")
        try:
            with open(path) as f:
                doc = json.load(f)
        except (OSError, ValueError):
            doc = {}
        doc.setdefault(self.mode, {})[self.what] = self.figures
        with open(path, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
        print(f"{self.mode} / {self.what}: " + ", ".join(f"{k} {v:.3g}" if isinstance(v, float) else f"{k} {v}" for k, v in self.figures.items()))
        if strict:
            assert not self.misses, f"{self.mode} / {self.what}:\n  " + "\n  ".join(self.misses)


def compare(r: Report, got: Dict[str, torch.Tensor], want: Dict[str, torch.Tensor], labels_ok: Optional[torch.Tensor] = None,
            keys: Optional[Sequence[str]] = None, rows: Optional[torch.Tensor] = None, prefix: str = "") -> None:
    """``got`` against ``want`` (row for row) into ``r``: every key of ``want`` (or ``keys``) within GPU_OUT_MAX of the tensor's maximum and
    within GPU_OUT_ELEM per element; num_samples_per_ray exact; seg_raw / seg_pred exact on the rows ``labels_ok``.  ``rows``: only these."""
    for k in (keys if keys is not None else want.keys()):
        if k in SKIP:
            continue
        if k not in got:
            r.check(f"{prefix}{k} (present)", MG.INF)
            continue
        w = want[k].detach().cpu().double()
        g = got[k].detach().cpu().double().reshape(w.shape[0], -1) if got[k].numel() == w.numel() else got[k].detach().cpu().double()
        w = w.reshape(w.shape[0], -1)
        if g.shape != w.shape:
            r.check(f"{prefix}{k} (shape)", MG.INF, f" ({tuple(g.shape)} against {tuple(w.shape)})")
            continue
        if rows is not None:
            g, w = g[rows], w[rows]
        if k in EXACT:
            ok = labels_ok if (k != "num_samples_per_ray" and labels_ok is not None) else torch.ones(w.shape[0], dtype=torch.bool)
            if rows is not None and k != "num_samples_per_ray" and labels_ok is not None:
                ok = labels_ok[rows]
            r.check(f"{prefix}{k} (exact)", 0.0 if torch.equal(g[ok], w[ok]) else MG.INF, f" ({int((g[ok] != w[ok]).any(1).sum())} rows differ)")
        else:
            r.check(f"{prefix}{k} / max", MG.max_ratio(g, w, MG.GPU_OUT_MAX))
            r.check(f"{prefix}{k} / element", MG.ratio(g, w, **MG.GPU_OUT_ELEM))


def rows_of(outputs: Dict[str, torch.Tensor], rays: Sequence[int]) -> Dict[str, torch.Tensor]:
    """The rows ``rays`` of a frame's outputs ([H,W,...] or [R,...]) -> {key: [len(rays), ...]} on the CPU."""
    idx = torch.as_tensor(list(rays), dtype=torch.int64)
    out = {}
    for k, v in outputs.items():
        if torch.is_tensor(v) and v.numel() and v.numel() % (H * W) == 0 and k not in SKIP:
            out[k] = v.reshape(H * W, -1)[idx.to(v.device)].cpu()
    return out
