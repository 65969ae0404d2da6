"""CPU checks of tests/normals_f64.py: the comparators pass the float32 model of csrc/umhs_normals.hip and reject planted faults, K and
the teeth condition are measured, the float64 oracle agrees with finite differences of float64 oracle/torch_ref.field_density, and the
host surface of the feature (C ABI table, --normal-method, PLY header) is what the documents say."""
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "unsupervised-hyperspectral-nerf_amd"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import hash_f64 as H  # noqa: E402
import normals_f64 as NF  # noqa: E402
from oracle import torch_ref as T  # noqa: E402


def _model_outputs(c, fault=None):
    r = c.run(np.float32, fault)
    return {k: np.ascontiguousarray(r[k], dtype=np.float32) for k in ("g01", "grad", "normal")}


def test_comparators_pass_the_float32_model_and_K_holds():
    worst = {"g01": 0.0, "grad": 0.0}
    report = {}
    for name in NF.CASES:
        c = NF.case(name)
        r64, outs = c.run(np.float64), _model_outputs(c)
        fails = NF.check_all(name, outs, r64, report)
        assert not fails, "\n".join(fails)
        for k in worst:
            worst[k] = max(worst[k], report[name][k])
        print(f"{name}: N {c.n}, live {int(r64['live'].sum())}, worst g01 {report[name]['g01']:.2f} grad {report[name]['grad']:.2f} "
              f"normal {report[name]['normal']:.3f} of its bound, teeth {report[name]['teeth']:.3f}")
    print(f"worst over all cases: g01 {worst['g01']:.2f} u mag, grad {worst['grad']:.2f} u mag -> K {NF.k_from(worst['g01']):g} / {NF.k_from(worst['grad']):g}")
    assert 4 * worst["g01"] <= NF.K_G01 and NF.K_G01 == NF.k_from(worst["g01"])
    assert 4 * worst["grad"] <= NF.K_GRAD and NF.K_GRAD == NF.k_from(worst["grad"])
    assert abs(worst["g01"] - NF.WORST_G01) < 0.01 and abs(worst["grad"] - NF.WORST_GRAD) < 0.01  # the docstring quotes what is measured


def test_teeth_condition_from_the_float64_run_alone():
    for name in NF.TEETH_CASES:
        r64 = NF.case(name).run(np.float64)
        teeth, _, gn = NF.teeth_mask(r64)
        share = teeth.sum() / r64["live"].sum()
        print(f"{name}: teeth {share:.4f}, |g01| median {np.median(np.linalg.norm(r64['g01'], axis=1)):.2f}, |grad| median {np.median(gn):.3g}")
        assert share >= 0.9


def test_cases_stay_clear_of_the_relu_kink():
    for name in NF.CASES:
        c = NF.case(name)
        r = c.run(np.float64)
        margin = (np.abs(r["h"]) / (NF.U * r["mag_h"])).min()
        print(f"{name}: smallest |h| / (u mag_h) = {margin:.3g}")
        assert margin >= NF.KINK
        assert ((c.run(np.float32)["h"] > 0) == (r["h"] > 0)).all()


def test_special_cases_are_what_they_claim():
    r = NF.case("inactive12").run(np.float64)
    assert (r["h"] < 0).all() and (r["q"] == 0).all() and (r["grad"] == 0).all() and (r["normal"] == 0).all()
    m = _model_outputs(NF.case("inactive12"))
    assert (m["grad"] == 0).all() and (m["normal"] == 0).all()
    assert (NF.case("sigma_hi13").run(np.float64)["sigma"] > 15).all() and (NF.case("sigma_lo13").run(np.float64)["sigma"] < -15).all()
    box = NF.case("box13")
    dead = box.sel == 0
    assert 10 < int(dead.sum()) < box.n // 2 and (box.pos01[dead] == 0).all()
    c = NF.case("contract13")
    m = c.wpos.abs().amax(1)
    one = np.float32(1)
    for v in (np.nextafter(one, np.float32(0)), one, np.nextafter(one, np.float32(2))):
        assert int((m == float(v)).sum()) >= 4
    srt = c.wpos.abs().sort(dim=1, descending=True).values
    assert int(((srt[:, 0] == srt[:, 1]) & (srt[:, 0] >= 1)).sum()) >= 4  # exact ties of the maximum, outside the unit box
    assert int((m < 1).sum()) > 50 and int((m > 1).sum()) > 50 and (c.sel == 1).all()
    e = NF.case("edges13_65")
    geo = H.geometry(e.pos01, H.ALL_LEVELS, 13)
    assert geo.eq.sum(-1).max() == 3 and (geo.eq.sum(-1) == 1).any() and (geo.eq.sum(-1) == 2).any()


def test_tie_of_the_maximum_goes_to_the_lowest_index():
    """x = (1.5, 1.5, 0.3): with k = 0 the rank-one term lands on component 0; an evaluation that picks k = 1 fails the rule."""
    c = NF.case("contract13")
    r64 = c.run(np.float64)
    i = int(((c.wpos[:, 0] == 1.5) & (c.wpos[:, 1] == 1.5)).nonzero()[0])
    x = c.wpos[i].double().numpy()
    g = r64["g01"][i]
    m = 1.5
    s, t = 2 / m - 1 / m**2, -2 / m**2 + 2 / m**3
    want = np.array([s * g[0] + t * (x @ g), s * g[1], s * g[2]]) / 4 * np.exp(np.clip(r64["sigma"][i], -15, 15))
    assert np.allclose(r64["grad"][i], want, rtol=1e-12, atol=0)
    other = np.array([s * g[0], s * g[1] + t * (x @ g), s * g[2]]) / 4 * np.exp(np.clip(r64["sigma"][i], -15, 15))
    wrong = r64["grad"].copy()
    wrong[i] = other
    assert NF.check_vec("tie", "grad", wrong.astype(np.float32), r64["grad"], r64["mag_grad"], NF.K_GRAD)


@pytest.mark.parametrize("fault,name", [("sign", "scattered12"), ("scale", "scattered12"), ("swap_x", "rays13"), ("relu", "scattered12"),
                                        ("rank_one", "contract13"), ("quarter", "contract13"), ("extent", "box13"), ("clamp", "sigma_hi13")])
def test_planted_faults_are_rejected(fault, name):
    c = NF.case(name)
    r64 = c.run(np.float64)
    for dt in (np.float32, np.float64):
        r = c.run(dt, fault)
        outs = {k: np.ascontiguousarray(r[k], dtype=np.float32) for k in ("g01", "grad", "normal")}
        fails = NF.check_all(name, outs, r64)
        assert fails, f"fault {fault} passed on {name}"
        # the direction-only faults must show in the normal as well, the magnitude-only ones in grad
        if fault in ("sign", "swap_x", "relu", "rank_one"):
            assert NF.check_normal(name, outs["normal"], r64), f"fault {fault}: the normal comparator saw nothing"
        assert NF.check_vec(name, "grad", outs["grad"], r64["grad"], r64["mag_grad"], NF.K_GRAD), f"fault {fault}: grad passed"


def test_another_precision_for_the_cell_is_the_wrong_truth():
    """Measured here: against the float32-defined cell a float32 evaluation of g01 is a few u away; against a
    genuine float64 pos01 * scale it is orders of magnitude further (recorded, and asserted only as 'at least 100 x worse')."""
    c = NF.case("scattered12")
    r64, r32 = c.run(np.float64), c.run(np.float32)
    gn = np.linalg.norm(r64["g01"], axis=1)
    rel = np.linalg.norm(r32["g01"] - r64["g01"], axis=1) / (NF.U * gn)
    # float64 product: the reference expression in float64 through autograd
    w = c.weights
    x = c.pos01.double().requires_grad_()
    enc = T.hash_encode(x, w.table.double(), T.hash_scalings(), w.log2_T)
    h = torch.relu(enc @ w.w0.double().T + w.b0.double())
    (g,) = torch.autograd.grad((h @ w.w1[0].double() + w.b1[0].double()).sum(), x)
    rel_wrong = np.linalg.norm(r32["g01"] - g.numpy(), axis=1) / (NF.U * gn)
    dn = np.abs(r32["normal"] - r64["normal"]).max()
    print(f"float32 g01 vs float64, float32-defined cell: median {np.median(rel):.1f} u, max {rel.max():.1f} u of |g01|; normals within {dn:.2e}")
    print(f"float32 g01 vs a float64 pos01 * scale:        median {np.median(rel_wrong):.0f} u, max {rel_wrong.max():.0f} u of |g01|")
    assert np.median(rel_wrong) > 100 * np.median(rel)


# ---- finite differences of float64 torch_ref.field_density ------------------------------------------------------------------------
FD_STEP = 1e-6


def _fd_points(mode: str, n: int, log2_T: int):
    """float32 world positions whose pos01 sits well inside a cell on every level and axis (offset in [0.01, 0.99]).  "box" and
    "inside": pos01 = m / 4096 with m < 4096, so that pos01 * scale_l (scale_l < 2048, an integer) is EXACT in float32 -- the float32
    cell the oracle is defined by and float64 torch_ref then agree on every offset, and the world position maps onto it exactly (box
    extents 2, 4, 2; inside the unit box pos01 = (x + 2) / 4).  "outside": random points with 1.2 < |x|inf < 6."""
    g = torch.Generator().manual_seed(9100 + len(mode))
    if mode == "outside":
        d = torch.nn.functional.normalize(torch.randn(40 * n, 3, generator=g), dim=-1)
        w = (d * (1.2 + 4.8 * torch.rand(40 * n, 1, generator=g))).float()
        w = w[w.abs().amax(1) > 1.2]
        pos01, _ = NF.positions_model(w, True, NF.UNIT_BOX)
    else:
        lo, hi = (1024 + 64, 3072 - 64) if mode == "inside" else (64, 4096 - 64)
        pos01 = torch.randint(lo, hi, (40 * n, 3), generator=g).float() / 4096.0
        if mode == "inside":
            w = pos01 * 4.0 - 2.0
        else:
            a, b = torch.tensor(NF.BOX[:3]), torch.tensor(NF.BOX[3:])
            w = a + pos01 * (b - a)
    off = H.geometry(pos01, H.ALL_LEVELS, log2_T).off
    ok = torch.from_numpy(((off >= 0.01) & (off <= 0.99)).all(axis=(1, 2)))
    return w[ok][:n].contiguous()


@pytest.mark.parametrize("mode", ["box", "inside", "outside"])
def test_oracle_agrees_with_finite_differences_of_float64_field_density(mode):
    """Central differences, step 1e-6 in world space, of float64 torch_ref.field_density against the oracle's grad.
    Tolerance, per component, in units of the oracle's envelope mag_grad (plus 1e-9 |density| / step for the difference's own rounding):
      box, inside   1e-6.  Inside a cell the encoding is LINEAR along each axis, so along a world axis sigma_raw is linear and the
                    density is exp of a linear function: the second-order term is (step sigma')^2 / 6 <= (1e-6 x 300)^2 / 6 ~ 1.5e-8
                    of the derivative; the float32 cell is the float64 cell here (exact products), so nothing else differs.
      outside       2e-3.  The oracle's cell is defined by the float32 pos01 of umhs_positions_fwd, float64 field_density contracts
                    in float64: the offsets differ by up to scale x (a few ulp of pos01) ~ 2047 x 4 x 6e-8 = 5e-4 of a cell, and a
                    blend derivative is bilinear in the other two offsets, so it moves by at most twice that share of its envelope;
                    the curvature of the contraction adds (step x scale / 4)^2 / 6 ~ 4e-8.
    Points where a hidden unit changes sign within the step (a kink of the ReLU inside the difference) are left out."""
    log2_T, n = 12, 48
    contraction = mode != "box"
    p = T.FieldParams(4, 8, False, log2_hashmap_size=log2_T, table_scale=NF.TABLE_SCALE, seed=11, dtype=torch.float64)
    w = NF.Weights(p.hash_table.detach().float(), p.base_w[0].detach().float(), p.base_b[0].detach().float(), p.base_w[1].detach().float(),
                   p.base_b[1].detach().float(), log2_T)
    assert (w.table.double() == p.hash_table.detach()).all()  # (the float64 parameters are float32 values)
    wpos = _fd_points(mode, n, log2_T)
    assert wpos.shape[0] == n
    aabb = NF.UNIT_BOX if contraction else NF.BOX
    pos01, sel = NF.positions_model(wpos, contraction, aabb)
    assert (sel == 1).all()
    r64 = NF.evaluate(w, pos01, wpos, sel, contraction, aabb, np.float64)
    aabb_t = torch.tensor(aabb, dtype=torch.float64).view(2, 3)
    z3, z1 = torch.zeros(n, 3, dtype=torch.float64), torch.zeros(n, 1, dtype=torch.float64)

    def density_and_mask(x):
        with torch.no_grad():
            d = T.field_density(p, x, z3, z1, z1, contraction, aabb_t)[0][:, 0]
            pos = (T.scene_contraction_linf(x) + 2.0) / 4.0 if contraction else (x - aabb_t[0]) / (aabb_t[1] - aabb_t[0])
            h = T.hash_encode(pos, p.hash_table, p.scalings, log2_T) @ p.base_w[0].T + p.base_b[0]
        return d.numpy(), (h > 0).numpy()

    x0 = wpos.double()
    d0, m0 = density_and_mask(x0)
    fd, smooth = np.zeros((n, 3)), np.ones(n, bool)
    for a in range(3):
        e = torch.zeros(3, dtype=torch.float64)
        e[a] = FD_STEP
        dp, mp = density_and_mask(x0 + e)
        dm, mm = density_and_mask(x0 - e)
        fd[:, a] = (dp - dm) / (2 * FD_STEP)
        smooth &= (mp == m0).all(1) & (mm == m0).all(1)
    assert smooth.sum() >= n - 4
    tol = (1e-6 if mode != "outside" else 2e-3) * r64["mag_grad"] + 1e-9 * np.abs(d0)[:, None] / FD_STEP
    err = np.abs(fd - r64["grad"])
    print(f"{mode}: {int(smooth.sum())} of {n} points, worst |fd - grad| / tol = {(err / tol)[smooth].max():.3g}, "
          f"worst relative to |grad| = {(np.linalg.norm(err, axis=1) / np.linalg.norm(r64['grad'], axis=1))[smooth].max():.3g}")
    assert (err <= tol)[smooth].all()


# ---- the host surface -----------------------------------------------------------------------------------------------------------------
def test_c_abi_has_the_symbol_and_the_version_stays_11():
    from umhsnerf import _hip, build

    assert "umhs_density_normals" in _hip.SIGNATURES and len(_hip.SIGNATURES["umhs_density_normals"][1]) == 18
    assert _hip.ABI_VERSION == 11 and "umhs_normals.hip" in build.SOURCES
    with open(os.path.join(ROOT, "include", "umhs_hip.h")) as f:
        header = f.read()
    assert re.search(r"#define UMHS_ABI_VERSION 11\b", header)
    decl = re.search(r"int umhs_density_normals\(([^;]*)\);", header)
    assert decl and len(decl.group(1).split(",")) == 18


def test_normal_method_argument_parsing(capsys):
    from umhsnerf import export

    base = ["pointcloud", "--data", "d", "--checkpoint", "c", "--output-dir", "o"]
    assert getattr(export.parse_args(base), "normal_method", "none") == "none"  # (not in the namespace unless given)
    assert export.parse_args(base + ["--normal-method", "analytic"]).normal_method == "analytic"
    for refused in ("open3d", "model_output"):
        with pytest.raises(SystemExit):
            export.parse_args(base + ["--normal-method", refused])
        assert "analytic" in capsys.readouterr().err
    with pytest.raises(ValueError, match="analytic"):
        export.export_pointcloud(None, "o", normal_method="open3d")


def test_ply_header_with_and_without_normals():
    from umhsnerf import export

    plain = export.ply_header(5, 3).decode().split("\n")
    assert plain == export.ply_header(5, 3, False).decode().split("\n") and not any("nx" in ln for ln in plain)
    with_n = export.ply_header(5, 3, True).decode().split("\n")
    i = with_n.index("property float z")
    assert with_n[i + 1:i + 4] == ["property float nx", "property float ny", "property float nz"] and with_n[i + 4] == "property uchar red"
    assert [ln for ln in with_n if ln not in ("property float nx", "property float ny", "property float nz")] == plain
    table = torch.arange(2 * 20, dtype=torch.uint8).view(2, 20)
    n = torch.tensor([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])
    rows = export.rows_with_normals(table, n)
    assert rows.shape == (2, 32) and (rows[:, :12] == table[:, :12]).all() and (rows[:, 24:] == table[:, 12:]).all()
    assert (rows[:, 12:24].contiguous().view(torch.float32) == n).all()
    world = np.array([[0.0, -2.0, 0.0, 5.0], [2.0, 0.0, 0.0, 6.0], [0.0, 0.0, 2.0, 7.0]], dtype=np.float32)  # a rotation x 2 and a shift
    assert torch.allclose(export.world_frame_normals(n, world), torch.tensor([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0]]))
