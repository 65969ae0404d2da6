"""umhs_density_normals (csrc/umhs_normals.hip) against the float64 oracle of tests/normals_f64.py, element by element: g01, grad and
the normal of every committed case (its docstring lists them: N = 1, 63, 64, 65, 257, 3077; log2_T 12, 13 and 19; the edge set,
scattered, rays; the contraction inside, outside, one float either side of 1 and on exact ties; an anisotropic box with points outside
it; every hidden unit inactive; sigma_raw beyond +-15).  The world-position cases take pos01 and sel from umhs_positions_fwd itself:
those bits define the cell.  Every output sits between guard floats and holds NaN before the launch.  The features passed in and the
features gathered in the kernel must give identical bits, and so must outputs requested singly and together.  The kernel's own worst
ratios go to normals_f64.json in NF.report_dir()."""
import ctypes as C
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import normals_f64 as NF

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = {}
GUARD = 16
SENTINEL = -12345.5


@pytest.fixture(scope="module", autouse=True)
def _write_report():
    yield
    worst = {k: max((r.get(k, 0.0) for r in REPORT.values()), default=0.0) for k in ("g01", "grad", "normal")}
    with open(os.path.join(NF.report_dir(ROOT), "normals_f64.json"), "w") as f:
        json.dump({"K": {"g01": NF.K_G01, "grad": NF.K_GRAD}, "worst": worst, "cases": REPORT}, f, indent=1)


def _mods():
    from umhsnerf import _hip, ops

    return ops, _hip


def _gpu_positions(wpos, contraction, aabb):
    ops, _ = _mods()
    spec = SimpleNamespace(contraction=contraction, aabb=tuple(aabb))
    _, pos01, sel = ops.positions_fwd(None, None, None, None, spec, world_pos_in=wpos.to(DEV).contiguous())
    return pos01.cpu(), sel.cpu()


def _case(name, weights=None):
    mode = NF.CASES[name][3]
    return NF.case(name, positions_fn=_gpu_positions if mode != "direct" else None, weights=weights)


def _launch(c, want, enc=None):
    """The C entry point itself, every requested output inside a buffer with GUARD sentinel floats on either side -> {name: [N,3] cpu}."""
    ops, _hip = _mods()
    w, n = c.weights, c.n
    d = lambda t: t.to(DEV).contiguous()
    ins = [d(c.pos01), d(c.wpos), d(c.sel), d(w.table), ops.hash_scalings().to(DEV), d(w.w0), d(w.b0), d(w.w1), d(w.b1)]
    bufs = {k: torch.full((3 * n + 2 * GUARD,), SENTINEL, device=DEV) for k in want}
    for b in bufs.values():
        b[GUARD:GUARD + 3 * n] = float("nan")
    out = lambda k: C.c_void_p(bufs[k].data_ptr() + 4 * GUARD) if k in bufs else None
    aabb = (C.c_float * 6)(*c.aabb)
    _hip.check(_hip.lib().umhs_density_normals(
        _hip.ptr(ins[0]), _hip.ptr(ins[1]), _hip.ptr(ins[2]), _hip.ptr(enc), _hip.ptr(ins[3]), _hip.ptr(ins[4]), w.log2_T, _hip.ptr(ins[5]),
        _hip.ptr(ins[6]), _hip.ptr(ins[7]), _hip.ptr(ins[8]), int(c.contraction), aabb, n, out("grad"), out("normal"), out("g01"),
        _hip.stream()), "umhs_density_normals")
    torch.cuda.synchronize()
    res = {}
    for k, b in bufs.items():
        h = b.cpu()
        assert (h[:GUARD] == SENTINEL).all() and (h[GUARD + 3 * n:] == SENTINEL).all(), f"{c.name} {k}: a guard float was written"
        res[k] = h[GUARD:GUARD + 3 * n].view(n, 3).clone()
        assert torch.isfinite(res[k]).all(), f"{c.name} {k}: an element was not written (or is not finite)"
    return res


def _same_bits(a, b):
    return bool((a.view(torch.int32) == b.view(torch.int32)).all())


@pytest.mark.parametrize("name", list(NF.CASES))
def test_every_element_against_float64(name):
    ops, _ = _mods()
    c = _case(name)
    r64 = c.run(np.float64)
    got = _launch(c, ("g01", "grad", "normal"))
    fails = NF.check_all(name, got, r64, REPORT)
    print(f"{name}: N {c.n}, worst ratios {REPORT[name]}")
    # the features passed in (the render path's level-major gather) against the features gathered in the kernel: the same bits
    enc = ops.hashgrid_fwd(c.pos01.to(DEV), c.weights.table.to(DEV), ops.hash_scalings().to(DEV), c.weights.log2_T, True)
    with_enc = _launch(c, ("g01", "grad", "normal"), enc=enc)
    for k in got:
        if not _same_bits(got[k], with_enc[k]):
            fails.append(f"{name} {k}: enc passed in and enc gathered in the kernel differ in bits")
    # requested singly against together: the same bits
    for k in ("g01", "grad", "normal"):
        if not _same_bits(got[k], _launch(c, (k,))[k]):
            fails.append(f"{name} {k}: requested alone differs in bits from requested together")
    if NF.CASES[name][4] == "inactive":
        assert (got["grad"] == 0).all() and (got["normal"] == 0).all() and (got["g01"] == 0).all()
    assert not fails, "\n".join(fails)


def test_teeth_cases_have_teeth_on_the_gpu_run_too():
    for name in NF.TEETH_CASES:
        r64 = _case(name).run(np.float64)
        teeth, _, _ = NF.teeth_mask(r64)
        assert teeth.sum() >= 0.9 * r64["live"].sum()


def _spectral_flat(w):
    """The weights of a case in a UMHSField parameter layout (4 classes, 8 bands) -> (spec-like, flat on the device)."""
    ops, _ = _mods()
    L = ops.FieldLayout(4, 8, False, w.log2_T)
    flat = torch.zeros(L.total)
    for key, t in (("encoder.hash_table", w.table), ("mlp.layers.0.weight", w.w0), ("mlp.layers.0.bias", w.b0),
                   ("mlp.layers.1.weight", w.w1), ("mlp.layers.1.bias", w.b1)):
        L.view(flat, "mlp_base." + key).copy_(t)
    return L, flat.to(DEV)


@pytest.mark.parametrize("name", ["contract13", "box13"])
def test_ops_density_normals_through_a_field_layout(name):
    ops, _ = _mods()
    c = _case(name)
    L, flat = _spectral_flat(c.weights)
    spec = ops.FieldSpec(L, 0.5, c.contraction, tuple(c.aabb), scalings=ops.hash_scalings().to(DEV))
    wpos, pos01, sel = ops.positions_fwd(None, None, None, None, spec, world_pos_in=c.wpos.to(DEV))
    assert _same_bits(pos01.cpu(), c.pos01) and _same_bits(sel.cpu(), c.sel)
    direct = _launch(c, ("g01", "grad", "normal"))
    out = ops.density_normals(spec, flat, pos01, wpos, sel, want=("grad", "normal", "g01"))
    assert set(out) == {"grad", "normal", "g01"}
    for k, v in out.items():
        assert v.shape == (c.n, 3) and _same_bits(v.cpu(), direct[k])
    only = ops.density_normals(spec, flat, pos01, wpos, sel)
    assert list(only) == ["normal"] and _same_bits(only["normal"].cpu(), direct["normal"])
    enc = ops.hashgrid_fwd(pos01, L.view(flat, "mlp_base.encoder.hash_table"), spec.scalings, L.log2_hashmap_size, True)
    assert _same_bits(ops.density_normals(spec, flat, pos01, wpos, sel, enc=enc)["normal"].cpu(), direct["normal"])
    with pytest.raises(ValueError):
        ops.density_normals(spec, flat, pos01, wpos, sel, want=("normals",))
    with pytest.raises(ValueError):
        ops.density_normals(spec, flat, pos01, wpos, sel, enc=enc[:, :-1])


def test_the_rgb_fields_weights_through_the_same_entry_point():
    """UMHSRGBField has the same mlp_base: its own (seeded) weights, its table scaled up to the cases' magnitude, the contract13 positions."""
    ops, _ = _mods()
    from umhsnerf.umhs_field_rgb import UMHSRGBField

    f = UMHSRGBField(aabb=torch.tensor([[-1.0, -1, -1], [1, 1, 1]]), log2_hashmap_size=13, seed=5)
    with torch.no_grad():
        f.layout.view(f.flat, "mlp_base.encoder.hash_table").mul_(100.0)
    v = {k: t.detach().clone() for k, t in f.named_views().items()}
    w = NF.Weights(v["mlp_base.encoder.hash_table"], v["mlp_base.mlp.layers.0.weight"], v["mlp_base.mlp.layers.0.bias"],
                   v["mlp_base.mlp.layers.1.weight"], v["mlp_base.mlp.layers.1.bias"], 13)
    c = _case("contract13", weights=w)
    r64 = c.run(np.float64)
    margin = (np.abs(r64["h"]) / (NF.U * r64["mag_h"])).min()
    assert margin >= NF.KINK, f"a hidden unit sits {margin:.3g} u mag_h from the ReLU kink: choose another seed"
    f = f.to(DEV)
    spec = f.normals_spec()
    wpos, pos01, sel = ops.positions_fwd(None, None, None, None, f._geom(), world_pos_in=c.wpos.to(DEV))
    assert _same_bits(pos01.cpu(), c.pos01)
    got = {k: t.cpu() for k, t in ops.density_normals(spec, f.flat.detach(), pos01, wpos, sel, want=("g01", "grad", "normal")).items()}
    fails = NF.check_all("rgb_contract13", got, r64, REPORT)
    assert not fails, "\n".join(fails)
    direct = _launch(c, ("normal",))
    assert _same_bits(direct["normal"], got["normal"])
