"""VCA endmember initialisation without a GPU: the float64 restatement against the fixtures recorded from the reference's own
vca.py (tests/golden/make_golden_vca.py), the package's host-side half against the restatement, the error behaviour of the new C
entries, and the field's ``endmember_init`` / ``load_vca`` precedence."""
import ctypes
import os

import numpy as np
import pytest
import torch

from vca_f64 import F64Passes, draws_from_seed, vca_f64

CUBES = ["b31", "b128", "b141", "b31_low"]
RUNS = ["b31", "b128", "b141"]  # the cubes the reference runs on; on b31_low (below its SNR threshold) it raises


def _fixture(golden_dir, name):
    g = np.load(os.path.join(golden_dir, f"g6_vca_{name}.npz"))
    cube = g["cube"]
    return g, cube.reshape(-1, cube.shape[-1]), int(g["num_classes"]), g["draws"]


@pytest.mark.parametrize("name", RUNS)
def test_restatement_reproduces_the_reference(golden_dir, name):
    g, rows, R, draws = _fixture(golden_dir, name)
    assert rows.dtype == np.float32 and str(g["raised_f32"]) == "" and str(g["raised_f64"]) == ""
    assert np.array_equal(draws, draws_from_seed(R, 1234))
    Ae, idx, info = vca_f64(rows.T, R, draws)
    assert info["branch"] == "projective" and info["snr"] > info["snr_th"] + 15
    assert np.array_equal(idx, g["indice_f64"]) and np.array_equal(idx, g["indice_f32"])
    assert np.max(np.abs(Ae - g["Ae_f64"])) <= 1e-9
    d_ref = float(g["d_ref"])
    assert d_ref == np.max(np.abs(g["Ae_f32"] - g["Ae_f64"])) and 0 < d_ref < 1e-3


def test_reference_raises_below_its_snr_threshold(golden_dir):
    """hs_dataloader.py:57-58 swallows this and the field starts from randn; the restatement takes the published branch."""
    g, rows, R, draws = _fixture(golden_dir, "b31_low")
    assert str(g["raised_f32"]) == "UnboundLocalError" == str(g["raised_f64"]) and "Ae_f64" not in g.files
    Ae, idx, info = vca_f64(rows.T, R, draws)
    assert info["branch"] == "affine" and info["snr"] < info["snr_th"] - 5
    assert len(set(idx.tolist())) == R and np.isfinite(Ae).all()


@pytest.mark.parametrize("name", CUBES)
def test_host_half_matches_the_restatement(golden_dir, name):
    """vca_plan / vca_select / vca_finish on float64 NumPy passes: the basis and SNR come from the moments alone there."""
    from umhsnerf.data.utils import vca as V

    _, rows, R, draws = _fixture(golden_dir, name)
    Ae, idx, info = vca_f64(rows.T, R, draws)
    passes = F64Passes(rows)
    plan = V.vca_plan(*passes.moments(), R)
    assert plan["branch"] == info["branch"] and abs(plan["snr"] - info["snr"]) < 1e-6 and plan["snr_th"] == info["snr_th"]
    got = V.vca_select(plan, draws, passes.argmax, passes.project(plan))
    assert np.array_equal(got, idx)
    assert np.max(np.abs(V.vca_finish(plan, passes.pixels(got)) - Ae.T)) <= 1e-9
    E, i2, inf = V.run_vca(F64Passes(rows), R, draws)
    assert E.dtype == torch.float32 and tuple(E.shape) == (R, rows.shape[1]) and i2.dtype == torch.int64
    assert np.array_equal(i2.numpy(), idx) and inf["branch"] == info["branch"] and set(inf) == {"snr", "snr_th", "branch"}
    assert np.array_equal(V.reference_draws(R, 1234), draws)
    with pytest.raises(ValueError):
        V.vca_plan(*passes.moments(), 16)


def test_vca_entries_report_argument_errors_before_anything_is_launched():
    """As test_argument_errors_are_reported_before_anything_is_launched: host-side checks only, so this runs without a GPU."""
    from umhsnerf import _hip

    lib = _hip.lib()
    ARG, UNSUP, WS = -1, -2, -3
    d = ctypes.c_void_p(4096)  # never dereferenced
    big = 1 << 40
    assert lib.umhs_vca_rows_per_partial() >= 8
    mom = lambda rows=d, n=100, b=31, s=d, S=d, ws=d, wsb=big: lib.umhs_vca_moments(rows, n, b, 0, s, S, ws, wsb, None)
    assert mom(rows=None) == ARG and mom(s=None) == ARG and mom(S=None) == ARG and mom(n=-1) == ARG and mom(b=0) == ARG
    assert mom(n=0) == 0 and mom(n=0, rows=None) == 0
    assert mom(b=257) == UNSUP
    need = lib.umhs_vca_moments_workspace_bytes(100, 31)
    assert need > 0 and lib.umhs_vca_moments_workspace_bytes(100, 257) == 0
    assert mom(ws=None) == WS and mom(wsb=need - 1) == WS
    f16 = (ctypes.c_float * 16)()
    proj = lambda rows=d, n=100, b=31, basis=d, mean=d, r=6, aff=1, y=d, mx=d, ws=d, wsb=big: lib.umhs_vca_project(
        rows, n, b, basis, mean, r, aff, y, mx, ws, wsb, None)
    assert proj(rows=None) == ARG and proj(basis=None) == ARG and proj(y=None) == ARG and proj(n=-1) == ARG and proj(r=0) == ARG
    assert proj(mean=None) == ARG and proj(mx=None) == ARG  # the affine form needs both
    assert proj(n=0) == 0
    assert proj(b=257) == UNSUP and proj(r=16) == UNSUP
    assert proj(ws=None) == WS and proj(wsb=lib.umhs_vca_project_workspace_bytes(100) - 1) == WS
    am = lambda y=d, n=100, f=f16, idx=d, row=d, ws=d, wsb=big: lib.umhs_vca_argmax(y, n, f, 0.0, idx, row, None, ws, wsb, None)
    assert am(y=None) == ARG and am(f=None) == ARG and am(idx=None) == ARG and am(row=None) == ARG and am(n=-1) == ARG
    assert am(y=ctypes.c_void_p(4100)) == ARG  # rows of y are read as float4
    assert am(n=0) == 0
    assert am(ws=None) == WS and am(wsb=lib.umhs_vca_argmax_workspace_bytes(100) - 1) == WS


def _field(**kw):
    from umhsnerf.umhs_field import UMHSField

    return UMHSField(aabb=[[-1, -1, -1], [1, 1, 1]], num_images=1, wavelengths=31, num_classes=6, method="rgb+spectral",
                     log2_hashmap_size=12, seed=3, **kw)


def test_field_takes_endmember_init_under_load_vca(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)  # no vca.npy here
    E = torch.rand(6, 31, generator=torch.Generator().manual_seed(0))
    plain = _field()
    assert torch.equal(_field(load_vca=True, endmember_init=E).endmembers.detach(), E)
    # load_vca off: the argument is ignored and the whole buffer is the one of a field built without it
    assert torch.equal(_field(load_vca=False, endmember_init=E).flat.detach(), plain.flat.detach())
    # on: everything but the endmembers is unchanged (the randn draw stays in the generator's sequence)
    on = _field(load_vca=True, endmember_init=E)
    off = on.layout.offset("endmembers")
    assert torch.equal(on.flat.detach()[:off], plain.flat.detach()[:off])
    assert torch.equal(_field(load_vca=True).flat.detach(), plain.flat.detach())  # nothing to load: randn, as before
    with pytest.raises(ValueError):
        _field(load_vca=True, endmember_init=E[:5])
    # an existing vca.npy in the working directory still wins
    F = np.random.RandomState(1).rand(6, 31).astype(np.float32)
    np.save(tmp_path / "vca.npy", F)
    assert torch.equal(_field(load_vca=True, endmember_init=E).endmembers.detach(), torch.from_numpy(F))
    assert torch.equal(_field(load_vca=False, endmember_init=E).flat.detach(), plain.flat.detach())
