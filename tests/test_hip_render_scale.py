"""Whole-frame renders at frame scale: ``UMHSModel.get_outputs_for_camera_ray_bundle`` over three chunks -- one empty (the sampler's
fake-sample branch), one past 8 x 65,536 samples (every workgroup of umhs_field_heads_fwd loops), one partial with longer rays --
against the chunk loop restated with ``model.forward`` (bit for bit), against a float64 oracle on ~256 selected rays, and against the
same rays rendered in launches of at most 65,536 samples (no heads workgroup loops there: the regime tests/test_hip_field_variants.py
holds to float64).  Scene, selection, oracle and comparator: tests/render_scale.py; its planted faults: tests/test_render_scale_cpu.py.

Modes: spec_b31 (rgb+spectral, specular head, C=6, B=31), nospec_b141 (spectral, C=4, B=141), normals (spec_b31 naming "normals"),
edit (spec_b31 under a dictionary edit and a density edit), regions (spec_b31 under a regional edit), crop (spec_b31 inside a crop
box: per-ray nears / fars), rgb (method "rgb").  And, apart from the modes, the two-launch forward of tests/test_hip_field_variants.py
taken to the looping regime on its own (70,001 and 8 x 65,536 + 4,097 samples), and one chunk at the size production renders: 32,768
rays through an all-occupied grid, 19.8 M samples (level-major features past 2^31 bytes, the [n,16] base rows past 2^30).

Every figure (worst |diff| / tolerance per mode, check and tensor; the chunks' sample counts) goes to ``render_scale.json`` in the
run-output directory."""
import contextlib
import copy
import os

import numpy as np
import pytest
import torch

import field_f64 as F
import material_f64 as MF
import model_golden as MG
import normals_f64 as NF
import region_f64 as RF
import render_scale as RS
from oracle import torch_ref as T

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ["spec_b31", "nospec_b141", "normals", "edit", "regions", "crop", "rgb"]
STATE_OF = {"nospec_b141": "nospec_b141", "rgb": "rgb"}  # every other mode renders the spec_b31 model
BASE = ["accumulation", "depth", "spectral", "spectral2", "specular", "rgb", "num_samples_per_ray", "abundances", "seg_probs", "seg_raw",
        "seg_pred"]
OVERRIDE = (0.25, 0.5, 0.75)
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _threads():
    with RS.threads():
        yield


def _edit_doc(mode):
    """edit: a recoloured material, a dimmed one, a thinned one and a specular gain; regions: another edit inside a box through the
    ball's left half (material 1 removed, material 3 brightened) on top of a top-level density edit."""
    g = torch.Generator().manual_seed(5)
    spectrum = [round(float(v), 4) for v in torch.rand(31, generator=g)]
    top = {"materials": [{"material": 2, "spectrum": spectrum}, {"material": 0, "gain": 0.4}, {"material": 1, "density": 0.25}], "specular_gain": 0.5}
    if mode == "edit":
        return top
    (bx, by, bz), r = RS.BALL
    box = {"center": [bx - 0.2, by, bz], "rotation": [0.0, 0.0, 0.3], "scale": [0.4, 1.0, 1.0]}
    return {"materials": [{"material": 4, "density": 0.5}, {"material": 0, "gain": 0.4}],
            "regions": [{"box": box, "materials": [{"material": 1, "density": 0.0}, {"material": 3, "gain": 2.0}], "specular_gain": 0.5}]}


def _state(state):
    if ("state", state) not in _CACHE:
        p = RS.make_params(state)
        p64 = copy.deepcopy(p).double()
        p64.scalings = p64.scalings.double()
        _CACHE[("state", state)] = {"state": state, "p": p, "p64": p64, "pipe": RS.make_pipeline(state, p, DEV)}
    return _CACHE[("state", state)]


def _bundle(model, crop):
    from umhsnerf import export
    from umhsnerf.render import load_camera_path

    key = ("bundle", crop)
    if key not in _CACHE:
        cams, meta = load_camera_path(RS.camera_path(), device=DEV)
        assert (meta["render_height"], meta["render_width"]) == (RS.H, RS.W)
        if crop:
            obb = export.obb_from_params(RS.CROP["center"], (0.0, 0.0, 0.0), RS.CROP["scale"])
            _CACHE[key] = cams.generate_rays(0, keep_shape=True, obb_box=obb, near_floor=RS.NEAR_FLOOR)
        else:
            _CACHE[key] = cams.generate_rays(0, keep_shape=True)
    return _CACHE[key]


@contextlib.contextmanager
def _normals(model, on):
    before, model._normals_requested = model._normals_requested, model._normals_requested or on
    try:
        yield
    finally:
        model._normals_requested = before


def _world(mode):
    """Per mode, once: the model, the frame's bundle, the context it renders under, the full render and the frame's own samples."""
    if mode in _CACHE:
        return _CACHE[mode]
    from umhsnerf.materials import load_material_edits

    st = _state(STATE_OF.get(mode, "spec_b31"))
    model = st["pipe"].model
    assert model.config.near_plane == RS.NEAR_FLOOR and max(int(model.config.eval_num_rays_per_chunk), 32768) == RS.CHUNK
    bundle = _bundle(model, mode == "crop")
    edits = load_material_edits(_edit_doc(mode), 6, 31, True) if mode in ("edit", "regions") else None
    if edits is not None:
        assert edits.edits_dictionary and edits.edits_density and bool(edits.regions) == (mode == "regions")
    ctx = (lambda: model.material_edits_context(edits)) if edits is not None else contextlib.nullcontext
    names = [k for k in BASE if st["state"] == "spec_b31" or k in ("rgb", "accumulation", "depth", "num_samples_per_ray")] + ["normals"] \
        if mode == "normals" else None
    with ctx():
        full = model.get_outputs_for_camera_ray_bundle(bundle, output_names=names)
    frame = RS.model_frame(model, bundle)
    torch.cuda.synchronize()
    w = _CACHE[mode] = dict(st, mode=mode, model=model, bundle=bundle, ctx=ctx, names=names, edits=edits, full=full, frame=frame,
                            facts=RS.assert_shape(frame))
    return w


def _chunk_bundles(bundle):
    from umhsnerf._ns_compat import RayBundle

    o, d = bundle.origins.reshape(-1, 3), bundle.directions.reshape(-1, 3)
    out = []
    for i in range(0, o.shape[0], RS.CHUNK):
        rb = RayBundle(origins=o[i:i + RS.CHUNK], directions=d[i:i + RS.CHUNK])
        if bundle.nears is not None:
            rb.nears, rb.fars = bundle.nears.reshape(-1, 1)[i:i + RS.CHUNK], bundle.fars.reshape(-1, 1)[i:i + RS.CHUNK]
        out.append(rb)
    return out


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)))


# ------------------------------------------------------------------------------------------------------------------------------ #
# (a) the chunk loop, exactly
# ------------------------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("mode", MODES)
def test_the_frame_is_the_concatenation_of_its_chunks_forwards(mode):
    w = _world(mode)
    model, bundle, full, names = w["model"], w["bundle"], w["full"], w["names"]
    r = RS.Report(mode, "a: chunk loop")
    chunks = _chunk_bundles(bundle)
    assert [len(c) for c in chunks] == [RS.CHUNK, RS.CHUNK, 250]
    with torch.no_grad(), w["ctx"](), _normals(model, mode == "normals"):
        parts = [model.forward(rb) for rb in chunks]
    keys = [k for k, v in parts[1].items() if torch.is_tensor(v) and v.shape[:1] == (RS.CHUNK,) and (names is None or k in names)]
    r.check("key set", 0.0 if set(full) == set(keys) else MG.INF, f" ({sorted(set(full) ^ set(keys))})")
    assert {"rgb", "depth", "accumulation", "num_samples_per_ray"} <= set(keys) and ("normals" in keys) == (mode == "normals")
    for k in keys:
        want = torch.cat([p[k] for p in parts]).view(RS.H, RS.W, -1)
        r.check(f"{k} (bits)", 0.0 if k in full and _same_bits(full[k], want) else MG.INF)
    with w["ctx"]():
        two = model.get_outputs_for_camera_ray_bundle(bundle, output_names=["rgb", "depth"])
        again = model.get_outputs_for_camera_ray_bundle(bundle, output_names=names)
    r.check("output_names=[rgb, depth]: nothing else", 0.0 if set(two) == {"rgb", "depth"} else MG.INF, f" ({sorted(two)})")
    for k in ("rgb", "depth"):
        r.check(f"output_names=[rgb, depth]: {k} (bits)", 0.0 if _same_bits(two[k], full[k]) else MG.INF)
    r.check("a second render gives the same bits", 0.0 if set(again) == set(full) and all(_same_bits(again[k], full[k]) for k in full) else MG.INF)
    # the background override: method rgb composites over it inside every chunk; the spectral methods get the term added to the frame
    colour = torch.tensor(OVERRIDE, device=DEV)
    with w["ctx"](), model.background_color_override_context(OVERRIDE):
        over = model.get_outputs_for_camera_ray_bundle(bundle, output_names=["rgb"])
        if mode == "rgb":
            with torch.no_grad():
                want = torch.cat([model.forward(rb)["rgb"] for rb in chunks]).view(RS.H, RS.W, 3)
    if mode != "rgb":
        want = full["rgb"] + colour * (1.0 - full["accumulation"])
    r.check("background override: only rgb", 0.0 if set(over) == {"rgb"} else MG.INF, f" ({sorted(over)})")
    r.check("background override: rgb (bits)", 0.0 if _same_bits(over["rgb"], want) else MG.INF)
    assert float((over["rgb"] - full["rgb"]).abs().max()) > 0.1  # (the empty chunk shows the colour)
    r.finish(ROOT)


# ------------------------------------------------------------------------------------------------------------------------------ #
# (b) the selected rays against float64
# ------------------------------------------------------------------------------------------------------------------------------ #
def _positions(w, o, d, t0, t1):
    """The model-frame positions of samples as the render computes them (float32, on the device)."""
    from umhsnerf import ops

    return ops.positions_fwd(o.to(DEV).contiguous(), d.to(DEV).contiguous(), t0.to(DEV).contiguous(), t1.to(DEV).contiguous(),
                             w["model"].field._spec())


def _edited_oracle(w):
    """``render`` of RS.truth for the modes edit / regions: tests/material_f64.edited_render / tests/region_f64.regional_render in
    float64 on the same samples (regions: with the layers of the float32 membership of the render's own positions), the depth
    clipped to the chunk's range instead of the call's.  The region layers come from ``ops.positions_fwd`` -- the code under test: a
    fault of the positions kernel would move both sides' layers together.  It is the plain modes that hold that kernel, through
    ``T.model_outputs`` from the raw origins, directions and times."""
    model, edits, p64, state = w["model"], w["edits"], w["p64"], w["state"]
    E = model.field.endmembers.detach()
    temp, M = RS.STATES[state][4], T.colour_matrix(RS.bands_of(state))

    def render(ch, o, d, t0, t1, ri, k, idx, clip):
        if w["mode"] == "edit":
            out = MF.edited_render(p64, edits.dictionary(E), edits.density_gain("cpu"), edits.specular_gain, o, d, t0, t1, ri, k, temp, M)
        else:
            wpos = _positions(w, o, d, t0, t1)[0].cpu().numpy()
            layer = torch.from_numpy(RF.classify32(wpos, edits.region_table()).astype(np.int64))
            w.setdefault("layers", set()).update(int(v) for v in layer.unique())
            out = RF.regional_render(p64, edits.dictionaries(E), edits.density_gains("cpu"), edits.specular_gains("cpu"), layer, o, d, t0, t1,
                                     ri, k, temp, M)
        t0c, t1c = t0.double()[:, None], t1.double()[:, None]
        out["depth"] = T.render_depth_expected(out["weights"], t0c, t1c, ri, k, clip)
        out["num_samples_per_ray"] = T.pack_info(ri, k)[:, 1]
        out.pop("unedited_spectral")
        return out

    return render


def _normals_truth(w, rays, t64w):
    """Float64 normals of the selected rays: tests/normals_f64.evaluate (steps 1-6) on the samples' positions as the render computes
    them, and step 7 (``ray_normals64``) under the float64 oracle's own weights.  The positions (pos01, world position, selector) are
    ``ops.positions_fwd``'s, so this truth is not independent of that kernel; the plain modes hold it (see ``_edited_oracle``)."""
    p, frame = w["p"], w["frame"]
    nw = NF.Weights(p.hash_table.detach(), p.base_w[0].detach(), p.base_b[0].detach(), p.base_w[1].detach(), p.base_b[1].detach(), p.log2_T)
    rows = []
    for ch in frame.chunks:
        local = [r - ch.r0 for r in rays if ch.r0 <= r < ch.r0 + ch.R]
        if not local:
            continue
        o, d, t0, t1, ri, _ = RS.gather_rays(ch, local)
        if ri.numel() == 0:
            rows.append(np.full((len(local), 3), 0.5))
            continue
        wpos, pos01, sel = (t.cpu() for t in _positions(w, o, d, t0, t1))
        n64 = NF.evaluate(nw, pos01, wpos, sel, True, (-1.0,) * 3 + (1.0,) * 3)["normal"]
        rows.append(NF.ray_normals64(t64w[ch.r0][: ri.numel()], n64, T.pack_info(ri, len(local)))[0])
    return torch.from_numpy(np.concatenate(rows))


@pytest.mark.parametrize("mode", MODES)
def test_the_selected_rays_match_float64(mode):
    w = _world(mode)
    frame, full, state = w["frame"], w["full"], w["state"]
    r = RS.Report(mode, "b: float64")
    r.note("chunks", w["facts"])
    # the frame's samples are the forward's own: the same deterministic march
    r.check("num_samples_per_ray of every ray (exact)", 0.0 if torch.equal(full["num_samples_per_ray"].reshape(-1).cpu(), frame.counts) else MG.INF)
    kinds = RS.select(frame, seed=0)
    RS.assert_selection(frame, kinds)
    rays = RS.selected(kinds)
    r.note("selected", {k: len(v) for k, v in kinds.items()})
    weights = {}

    def keep_weights(ch, o, d, t0, t1, ri, k, idx, clip):  # the plain oracle, its per-sample weights kept for step 7 of the normals
        dt = torch.float64
        out = T.model_outputs(w["p64"], o.to(dt), d.to(dt), t0.to(dt)[:, None], t1.to(dt)[:, None], ri, k, RS.STATES[state][4],
                              T.colour_matrix(RS.bands_of(state)).to(dt), depth_clip_range=clip, class_colors=RS.class_colors().to(dt))
        weights[ch.r0] = out["weights"].reshape(-1)
        return out

    render = _edited_oracle(w) if mode in ("edit", "regions") else (keep_weights if mode == "normals" else None)
    t64 = RS.truth(w["p64"], frame, rays, state, render=render)
    ok = None
    if "seg_probs" in t64:
        r.note("decided labels", RS.assert_labels_cap(t64))
        ok = RS.decided(t64)
    got = RS.rows_of(full, rays)
    RS.compare(r, got, t64, ok)
    if mode == "regions":
        assert w["layers"] == {0, 1}, w["layers"]  # both the top-level edit and the region's are seen
    if mode == "normals":
        RS.compare(r, got, {"normals": _normals_truth(w, rays, weights)})
    r.finish(ROOT)


# ------------------------------------------------------------------------------------------------------------------------------ #
# (c) every ray of the chunks with samples against launches that do not loop
# ------------------------------------------------------------------------------------------------------------------------------ #
def _ray_cuts(pinfo, limit, lo=0, hi=None):
    """Ray ranges [r0, r1) covering the rays [lo, hi) (default: all), whole rays only, each with at most ``limit`` samples (greedy)."""
    hi = pinfo.shape[0] if hi is None else hi
    ends = (pinfo[:, 0] + pinfo[:, 1]).tolist()
    cuts, r0, base = [], lo, int(pinfo[lo, 0])
    while r0 < hi:
        r1 = r0
        while r1 < hi and ends[r1] - base <= limit:
            r1 += 1
        assert r1 > r0
        cuts.append((r0, r1))
        r0, base = r1, ends[r1 - 1]
    return cuts


def _small_launches(r, w, mode, fr, ri, pinfo, flat, keys, row0=0, lo=0, hi=None):
    """The rays [lo, hi) of a chunk (samples ``fr`` / ``ri`` on the device, ``pinfo`` on the host; its first ray is row ``row0`` of
    ``flat``, the frame's outputs as [rays, -1]) rendered again in launches of at most TILE samples and compared into ``r`` -> the
    number of launches.  Method rgb clips the depth inside its own path: there both sides are clipped once more with the small
    launch's (narrower) range."""
    from umhsnerf._ns_compat import packed_ray_samples

    model, launches = w["model"], 0
    for r0, r1 in _ray_cuts(pinfo, RS.TILE, lo, hi):
        a, b = int(pinfo[r0, 0]), int(pinfo[r1 - 1, 0] + pinfo[r1 - 1, 1])
        assert 0 < b - a <= RS.TILE
        launches += 1
        sub = packed_ray_samples(fr.origins[a:b].contiguous(), fr.directions[a:b].contiguous(), fr.starts[a:b].contiguous(),
                                 fr.ends[a:b].contiguous())
        sub_info = (pinfo[r0:r1] - torch.tensor([a, 0])).to(DEV).contiguous()
        with torch.no_grad(), w["ctx"](), _normals(model, mode == "normals"):
            out = model.get_outputs_from_samples(sub, (ri[a:b] - r0).contiguous(), r1 - r0, packed_info=sub_info)
        want = {k: flat[k][row0 + r0: row0 + r1] for k in keys}
        if mode == "rgb":
            mid = (fr.starts[a:b] + fr.ends[a:b]) / 2
            want["depth"] = want["depth"].clamp(float(mid.min()), float(mid.max()))
        ok = None
        if "seg_probs" in want:  # labels: where the frame's own top-2 gap and accumulation are clear of a tie
            top = want["seg_probs"].topk(2, dim=1).values
            ok = (((top[:, 0] - top[:, 1]) > RS.GAP) & ((want["accumulation"].reshape(-1) - 0.5).abs() > RS.GAP)).cpu()
        RS.compare(r, {k: out[k] for k in keys}, want, ok)
    return launches


@pytest.mark.parametrize("mode", MODES)
def test_every_ray_matches_launches_of_at_most_65536_samples(mode, monkeypatch):
    from umhsnerf import ops

    w = _world(mode)
    model, full, frame = w["model"], w["full"], w["frame"]
    r = RS.Report(mode, "c: small launches")
    keys = [k for k in BASE + ["normals"] if k in full]
    flat = {k: full[k].reshape(RS.H * RS.W, -1) for k in keys}
    launches = 0
    tmid = ops.tmid_minmax
    for ci, rb in list(enumerate(_chunk_bundles(w["bundle"])))[1:]:
        ch = frame.chunks[ci]
        with torch.no_grad():
            rs, ri = model.sample(rb)
        fr = rs.frustums
        pinfo = T.pack_info(ri.cpu(), len(rb))
        assert torch.equal(pinfo, ch.pinfo)
        # the depth clip is per launch: the small launches of a spectral method clip with the chunk's range, as the frame did
        mm = tmid(fr.starts.reshape(-1).contiguous(), fr.ends.reshape(-1).contiguous())
        monkeypatch.setattr(ops, "tmid_minmax", lambda *a, **k: mm)
        launches += _small_launches(r, w, mode, fr, ri, pinfo, flat, keys, row0=ch.r0)
        monkeypatch.setattr(ops, "tmid_minmax", tmid)
    r.note("launches", launches)
    assert launches >= 10
    r.finish(ROOT)


# ------------------------------------------------------------------------------------------------------------------------------ #
# the heads loop alone
# ------------------------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("n,seed", [(70001, 7), (8 * 65536 + 4097, 8)])
def test_two_launch_forward_past_256_workgroups_of_256_samples(n, seed):
    """``hip.two_launch()`` of tests/test_hip_field_variants.py where umhs_field_heads_fwd's grid is capped and every workgroup loops
    (the next tile prefetched, the per-16-sample head / tail partials joined by the finish kernel), against ``F.oracle_per_ray`` in
    float64 with that file's own comparators.  70,001 samples: every sample and ray.  8 x 65,536 + 4,097: the rays that straddle a
    multiple of 65,536 samples, their neighbours and 64 seeded random rays (the oracle is separable per sample)."""
    from field_hip import Hip, _logits

    case = F.make_case(4, 48, True, 0.55, n, seed=seed)
    hip = Hip(case)
    base, w, ho = hip.two_launch()
    torch.cuda.synchronize()
    pinfo = case.packed_info()
    s, c = pinfo[:, 0], pinfo[:, 1]
    straddle = torch.nonzero((c > 0) & (s // RS.TILE != (s + c - 1).clamp(min=0) // RS.TILE)).reshape(-1)
    assert straddle.numel() >= (n - 1) // RS.TILE - 1 and -(-n // 256) > 256  # (a boundary may fall between two rays)
    if n <= 100000:
        rays = torch.arange(case.R)
    else:
        g = torch.Generator().manual_seed(seed)
        near = torch.cat([straddle - 1, straddle, straddle + 1]).clamp(0, case.R - 1)
        rays = torch.unique(torch.cat([near, torch.randperm(case.R, generator=g)[:64], torch.tensor([0, case.R - 2, case.R - 1])]))
    cnt = c[rays]
    idx = torch.repeat_interleave(s[rays], cnt) + (torch.arange(int(cnt.sum())) - torch.repeat_interleave(cnt.cumsum(0) - cnt, cnt))
    sub = copy.copy(case)
    sub.n, sub.counts = int(idx.numel()), cnt
    sub.enc, sub.wpos, sub.dirs, sub.sel, sub.t0, sub.t1 = (t[idx] for t in (case.enc, case.wpos, case.dirs, case.sel, case.t0, case.t1))
    p64 = copy.deepcopy(case.p).double()
    with torch.no_grad():
        o64 = F.field_forward(p64, sub.enc.double(), sub.wpos.double(), sub.dirs.double(), sub.sel.double(), case.temp)
    rep, mode = {}, f"heads loop n={n}"
    fails = F.check_forward({k: v[idx.to(DEV)] for k, v in base.items() if k in ("sigma", "sigma_raw", "emb")}, o64, ["sigma", "sigma_raw", "emb"],
                            rep, "base.")
    fails += F.check_values("heads.abundances", ho["abundances"][idx.to(DEV)], o64["abundances"], rep)
    fails += F.check_values("heads.feat_logits", _logits(ho, case)[idx.to(DEV)], o64["feat_logits"], rep)
    per_ray = F.oracle_per_ray(sub, o64, weights=w.cpu().double()[idx])
    comp = dict(zip(["spectral", "spectral2", "specular"], ho["comp"]), abundances=ho["comp_abundances"])
    fails += F.check_forward({k: v[rays.to(DEV)] for k, v in comp.items()}, per_ray, list(per_ray), rep, "rays.")
    r = RS.Report(mode, "float64")
    for k, v in rep.items():
        r.note(k, v)
    r.note("rays", int(rays.numel()))
    r.note("straddling rays", int(straddle.numel()))
    r.finish(ROOT)
    assert not fails, "; ".join(fails[:12])


# ------------------------------------------------------------------------------------------------------------------------------ #
# one chunk at the size production renders (a test of its own: it can be removed without touching the others)
# ------------------------------------------------------------------------------------------------------------------------------ #
PRODUCTION_STEP = 0.02  # 11 .. 14.3 units from the near plane to the far side of the coarsest grid level: 550 .. 715 samples per ray


def _production_selection(ch, n_enc_boundary, seed=0, n=RS.N_SELECT):
    """-> {kind: rays} of the one chunk: its first and last ray; every eighth ray that straddles a multiple of TILE samples and the ray
    after it; the rays around sample 2^24 (where the [n,16] base rows pass 2^30 bytes) and around the sample at which the level-major
    features pass 2^31 bytes; the longest ray; a seeded random remainder."""
    s, c = ch.pinfo[:, 0].contiguous(), ch.pinfo[:, 1]
    holder = lambda i: int(torch.searchsorted(s, torch.tensor(i), right=True)) - 1
    st = [int(x) for x in RS.straddlers(ch)][::8]
    kinds = {"first_of_chunk": [0], "last_of_chunk": [ch.R - 1], "straddle": st, "after_straddle": [x + 1 for x in st if x + 1 < ch.R],
             "base16_2^30_bytes": [x for x in range(holder(1 << 24) - 1, holder(1 << 24) + 2) if 0 <= x < ch.R],
             "enc_2^31_bytes": [x for x in range(holder(n_enc_boundary) - 1, holder(n_enc_boundary) + 2) if 0 <= x < ch.R],
             "longest": [int(c.argmax())]}
    taken = set(sum(kinds.values(), []))
    g = torch.Generator().manual_seed(seed)
    kinds["random"] = []
    for x in torch.randperm(ch.R, generator=g).tolist():
        if len(taken) >= n:
            break
        if x not in taken:
            taken.add(x)
            kinds["random"].append(x)
    return kinds


def test_one_production_chunk_of_two_to_the_24_samples(monkeypatch):
    """A single chunk of 32,768 rays through an all-occupied grid with 550+ samples each -- the "32 k rays x 529 samples" of
    umhs_model.py: at least 2^24 samples, so the level-major features pass 2^31 bytes and the [n,16] base rows 2^30 bytes.  About 256
    selected rays against float64 and 2,048 rays (the first 512, 512 around sample 2^24, the last 1,024) against launches of at most
    65,536 samples, with the comparator and the tolerances of the modes above."""
    from umhsnerf import ops
    from umhsnerf.render import load_camera_path

    st = _state("spec_b31")
    model = st["pipe"].model
    grid = model.sampler.occupancy_grid
    before = (grid.binaries, grid.occs.clone(), model.config.render_step_size)
    w = dict(st, mode="production", model=model, ctx=contextlib.nullcontext)
    r = RS.Report("production", "one chunk of 2^24 samples")
    try:
        grid.mark_all_occupied()
        model.config.render_step_size = PRODUCTION_STEP
        path = dict(RS.camera_path(), render_height=128, render_width=256)
        cams, _ = load_camera_path(path, device=DEV)
        bundle = cams.generate_rays(0, keep_shape=True)
        assert bundle.origins.numel() // 3 == RS.CHUNK
        full = model.get_outputs_for_camera_ray_bundle(bundle, output_names=BASE)
        frame = RS.model_frame(model, bundle)
        torch.cuda.synchronize()
        (ch,) = frame.chunks
        n = ch.n
        assert n >= 1 << 24 and n * 32 * 4 > 1 << 31 and n * 16 * 4 > 1 << 30 and int(ch.counts.min()) >= 512, n
        assert int(ch.counts.max()) <= 1024  # (one pass of the march: its scratch row holds a ray)
        r.note("samples", n)
        r.note("samples per ray (min, max)", [int(ch.counts.min()), int(ch.counts.max())])
        r.note("heads_loop_iterations", -(-n // RS.TILE))
        r.check("num_samples_per_ray of every ray (exact)", 0.0 if torch.equal(full["num_samples_per_ray"].reshape(-1).cpu(), ch.counts) else MG.INF)
        level, sample = divmod(1 << 28, n)  # element (level, sample, 0) of the [16, n, 2] features lies 2^31 bytes in
        assert 0 < level < 16
        kinds = _production_selection(ch, sample)
        rays = RS.selected(kinds)
        assert 200 <= len(rays) <= RS.N_SELECT + 8 and kinds["base16_2^30_bytes"] and kinds["enc_2^31_bytes"] and len(kinds["straddle"]) >= 30
        r.note("selected", {k: len(v) for k, v in kinds.items()})
        t64 = RS.truth(st["p64"], frame, rays, "spec_b31")
        r.note("decided labels", RS.assert_labels_cap(t64))
        flat = {k: full[k].reshape(RS.CHUNK, -1) for k in BASE}
        RS.compare(r, {k: v[torch.as_tensor(rays, device=DEV)].cpu() for k, v in flat.items()}, t64, RS.decided(t64), prefix="float64: ")
        # small launches
        with torch.no_grad():
            rs, ri = model.sample(_only_chunk(bundle))
        fr = rs.frustums
        mm = ops.tmid_minmax(fr.starts.reshape(-1).contiguous(), fr.ends.reshape(-1).contiguous())
        monkeypatch.setattr(ops, "tmid_minmax", lambda *a, **k: mm)
        mid = int(torch.searchsorted(ch.pinfo[:, 0].contiguous(), torch.tensor(1 << 24), right=True)) - 1
        launches = 0
        for lo, hi in ((0, 512), (mid - 256, mid + 256), (RS.CHUNK - 1024, RS.CHUNK)):
            sub = RS.Report("production", "scratch")
            launches += _small_launches(sub, w, "production", fr, ri, ch.pinfo, flat, BASE, lo=lo, hi=hi)
            for k, v in sub.figures.items():
                r.check(f"small launches: {k}", v)
        r.note("launches", launches)
        assert launches >= 16
    finally:
        monkeypatch.undo()
        grid.binaries, model.config.render_step_size = before[0], before[2]
        grid.occs.copy_(before[1])
    r.finish(ROOT)


def _only_chunk(bundle):
    """The frame's one chunk as ``_camera_ray_bundle_outputs`` hands it to the forward."""
    (rb,) = _chunk_bundles(bundle)
    return rb
