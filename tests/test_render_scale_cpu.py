"""The frame-scale comparator of tests/render_scale.py without a GPU: it passes the float32 oracle on the selected rays of the
three-chunk frame and rejects, one by one, the faults a chunk loop or a persistent tile loop can make.

The frame here is ``RS.cpu_frame()`` (``analytic_march`` through the exact ball and slab); its shape is held by ``RS.assert_shape``
as the GPU frame's is.  Every fault is planted into the float32 oracle's rows, so what the comparator sees is a faithful render with
exactly one thing wrong.  How far above tolerance each fault lands (worst |diff| / tolerance over the report; "inf": an exact quantity
or a shape differs), measured here and asserted >= 10:

  spec_b31     tile_removed 3.3e+03 | tile_to_neighbour 3.3e+03 (on the neighbour's own row) | chunk2_shifted inf (values alone 9.2e+03) |
               chunk1_clip_of_chunk2 4.0e+02 | chunk1_planes_of_chunk0 inf | chunk1_planes_one_row_up inf (values alone 9.3e+03) |
               last_chunk_truncated inf (values alone 1.0e+04)
  nospec_b141  tile_removed 3.6e+03 | tile_to_neighbour 3.6e+03 | chunk2_shifted inf (9.0e+03) | chunk1_clip_of_chunk2 4.0e+02 |
               chunk1_planes_of_chunk0 inf | chunk1_planes_one_row_up inf (8.9e+03) | last_chunk_truncated inf (1.0e+04)

(chunk1_planes_of_chunk0 empties chunk 1 -- chunk 0's planes are all misses -- so only the sample counts speak; chunk1_planes_one_row_up
leaves it about as full as before and is caught by the values too.)
(removing 16 of a ray's 64 .. 128 samples moves the ray by a good share of its value: three orders of magnitude above 1e-4).  The
float32 oracle itself sits at 0.016 x the tolerance."""
import copy

import pytest
import torch

import model_golden as MG
import render_scale as RS

STATES = ["spec_b31", "nospec_b141"]
FAULTS = ["tile_removed", "tile_to_neighbour", "chunk2_shifted", "chunk1_clip_of_chunk2", "chunk1_planes_of_chunk0", "chunk1_planes_one_row_up",
          "last_chunk_truncated"]
VALUE_KEYS = ("spectral", "accumulation", "depth", "rgb", "abundances")


@pytest.fixture(scope="module", autouse=True)
def _threads():
    with RS.threads():
        yield


@pytest.fixture(scope="module")
def frames():
    plain, crop = RS.cpu_frame(), RS.cpu_frame(crop=True)
    return {"plain": plain, "crop": crop, "facts": RS.assert_shape(plain), "crop_facts": RS.assert_shape(crop)}


@pytest.fixture(scope="module", params=STATES)
def world(request, frames):
    """Per state: the parameters in both precisions, the selection and both oracles' rows on the plain and the cropped frame (computed
    once, never modified: every test copies what it changes)."""
    state = request.param
    p = RS.make_params(state)
    p64 = copy.deepcopy(p).double()
    p64.scalings = p64.scalings.double()
    w = {"state": state, "p": p, "p64": p64}
    for name in ("plain", "crop"):
        kinds = RS.select(frames[name], seed=0)
        RS.assert_selection(frames[name], kinds)
        rays = RS.selected(kinds)
        w[name] = {"frame": frames[name], "kinds": kinds, "rays": rays, "t64": RS.truth(p64, frames[name], rays, state),
                   "t32": RS.truth(p, frames[name], rays, state, torch.float32)}
    return w


def test_the_frames_have_the_shape_the_gpu_test_relies_on(frames):
    for facts in (frames["facts"], frames["crop_facts"]):
        print(facts)
        assert facts["heads_loop_iterations"][1] >= 9 and facts["samples"][0] == 0


def test_the_selection_holds_every_kind_of_ray(world):
    for name in ("plain", "crop"):
        s = world[name]
        print(world["state"], name, {k: len(v) for k, v in s["kinds"].items()}, len(s["rays"]))
        assert 200 <= len(s["rays"]) <= RS.N_SELECT + 40
        nspr = s["t64"]["num_samples_per_ray"].reshape(-1)
        assert torch.equal(nspr, s["frame"].counts[torch.as_tensor(s["rays"])])
        assert int((nspr == 0).sum()) >= 2 and int((nspr == 1).sum()) >= 1


def test_the_labels_cap_holds_on_the_oracle_alone(world):
    for name in ("plain", "crop"):
        share = RS.assert_labels_cap(world[name]["t64"])
        print(world["state"], name, f"{share:.3f} of the selected rays with samples have a decided label")


def test_the_float32_oracle_passes_the_comparator(world):
    for name in ("plain", "crop"):
        s = world[name]
        r = RS.Report(world["state"], f"cpu float32 oracle ({name})")
        RS.compare(r, s["t32"], s["t64"], RS.decided(s["t64"]))
        print(world["state"], name, f"worst {r.worst:.3g}")
        assert not r.misses, r.misses
        assert r.worst <= 0.25  # (a float32 evaluation of 100 samples per ray: well inside 1e-4)


def _tile_contribution(w, frame, ray, dtype=torch.float32):
    """What the 16 samples [k, k + 16) of ``ray`` that hold its TILE boundary add to its ``spectral``: the difference of the ray rendered
    up to k + 16 and up to k samples (the weights of the earlier samples do not depend on the later ones)."""
    ch = frame.chunks[frame.chunk_of(ray)]
    s, c = (int(v) for v in ch.pinfo[ray - ch.r0])
    cut = ((s + c - 1) // RS.TILE) * RS.TILE - s  # the ray's first sample of the next loop iteration
    k = min(max(cut - 8, 0), c - 16)
    assert c >= 32 and 0 <= k and k + 16 <= c
    parts = []
    for m in (k, k + 16):
        sub = RS.Chunk(ch.r0, ch.o, ch.d, torch.full((m,), ray - ch.r0), ch.t0[s:s + m], ch.t1[s:s + m])
        parts.append(RS.truth(w["p"], RS.Frame([sub]), [ray], w["state"], dtype)["spectral"][0])
    return parts[1] - parts[0]


def _plant(w, fault):
    """-> (got rows, the set they are compared on, rows that must show the fault or None)."""
    side = w["crop" if fault.startswith("chunk1_planes") else "plain"]
    frame, rays, state = side["frame"], side["rays"], w["state"]
    got = {k: v.clone() for k, v in side["t32"].items()}
    row = {r: i for i, r in enumerate(rays)}
    at = None
    if fault in ("tile_removed", "tile_to_neighbour"):
        ray = next(r for r in side["kinds"]["straddle"] if int(frame.counts[r]) >= 32 and r + 1 in row)
        c = _tile_contribution(w, frame, ray)
        got["spectral"][row[ray]] -= c
        at = torch.tensor([row[ray]])
        if fault == "tile_to_neighbour":
            got["spectral"][row[ray + 1]] += c
            at = torch.tensor([row[ray + 1]])
    elif fault == "chunk2_shifted":  # row i of chunk 2 holds ray i - 1
        mine = [r for r in rays if r >= 2 * RS.CHUNK]
        shifted = RS.truth(w["p"], frame, [r - 1 for r in mine], state, torch.float32)
        for k in got:
            got[k][[row[r] for r in mine]] = shifted[k]
    elif fault == "chunk1_clip_of_chunk2":
        got = RS.truth(w["p"], frame, rays, state, torch.float32, clip_from={1: 2})
    elif fault == "chunk1_planes_of_chunk0":
        got = RS.truth(w["p"], RS.cpu_frame(crop=True, planes_from={1: 0}), rays, state, torch.float32)
    elif fault == "chunk1_planes_one_row_up":  # chunk 1 marches inside the planes of the pixels one image row above its own: not empty
        wrong = RS.cpu_frame(crop=True, planes_shift={1: -RS.W})
        assert wrong.chunks[1].n > 8 * RS.TILE
        got = RS.truth(w["p"], wrong, rays, state, torch.float32)
    elif fault == "last_chunk_truncated":  # the rays past the last multiple of 64 of the partial chunk are never written
        lost = [row[r] for r in rays if r >= 2 * RS.CHUNK + (250 // 64) * 64]
        assert lost and row[frame.R - 1] in lost
        for k in got:
            got[k][lost] = 0
    return got, side, at


@pytest.mark.parametrize("fault", FAULTS)
def test_the_comparator_rejects_a_planted_fault(world, fault):
    got, side, at = _plant(world, fault)
    r = RS.Report(world["state"], f"cpu fault {fault}")
    RS.compare(r, got, side["t64"], RS.decided(side["t64"]), rows=at)
    values = RS.Report(world["state"], "values alone")
    RS.compare(values, got, side["t64"], keys=[k for k in VALUE_KEYS if k in got], rows=at)
    print(f"{world['state']} {fault}: {r.worst:.3g} x tolerance (values alone {values.worst:.3g})")
    assert r.misses and r.worst >= 10.0, (fault, r.figures)
    if fault != "chunk1_planes_of_chunk0":  # (there the sample counts themselves differ: an exact quantity)
        assert values.worst >= 10.0 and values.worst != MG.INF, (fault, values.figures)
