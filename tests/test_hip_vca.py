"""VCA endmember initialisation on the GPU: the three kernels of csrc/umhs_vca.hip against float64, the whole initialiser against
the fixtures recorded from the reference's vca.py and against the float64 restatement (tests/vca_f64.py), resident and
host-resident stacks, and ``load_vca`` through the pipeline."""
import os

import numpy as np
import pytest
import torch

from vca_f64 import draws_from_seed, make_cube, vca_f64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24  # unit roundoff of fp32


def _fixture(golden_dir, name):
    g = np.load(os.path.join(golden_dir, f"g6_vca_{name}.npz"))
    return g, g["cube"], int(g["num_classes"]), g["draws"]


def _d_ref(golden_dir, bands):
    return float(np.load(os.path.join(golden_dir, f"g6_vca_b{bands}.npz"))["d_ref"])


# ---- 5: moments ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [3, 21, 31, 128, 141, 256])
@pytest.mark.parametrize("N", [1, 63, 1000, 262144 + 17])
def test_moments_match_float64_within_the_fp32_dot_product_bound(B, N):
    """Every fp32 partial is an fmaf chain over K rows (exact products, one rounding per addition) and the partials meet in
    float64, so the error of an entry is at most that of an fp32 dot product of length K: (K + 2) 2^-24 sum |terms|."""
    from umhsnerf import ops

    K = ops.vca_rows_per_partial()
    g = torch.Generator().manual_seed(1000 * B + N % 997)
    rows = torch.randn(N, B, generator=g)
    r64 = rows.double()
    s_ref, S_ref = r64.sum(0), r64.T @ r64
    s_abs, S_abs = r64.abs().sum(0), r64.abs().T @ r64.abs()
    d = rows.to(DEV)
    s, S = ops.vca_moments(d)
    assert s.dtype == S.dtype == torch.float64 and tuple(S.shape) == (B, B)
    es, eS = ((s.cpu() - s_ref).abs() / s_abs).max().item(), ((S.cpu() - S_ref).abs() / S_abs).max().item()
    print(f"moments B={B} N={N}: max error / sum|terms| = {es / U:.2f} u (sum), {eS / U:.2f} u (S); bound {(K + 2)} u")
    assert ((s.cpu() - s_ref).abs() <= (K + 2) * U * s_abs).all()
    assert ((S.cpu() - S_ref).abs() <= (K + 2) * U * S_abs).all()
    assert torch.equal(S, S.T)
    s2, S2 = ops.vca_moments(d)
    assert torch.equal(s, s2) and torch.equal(S, S2)  # bitwise from run to run
    if N > 1:  # two halves fed with accumulate = the whole, to float64 rounding (the fp32 partials are cut elsewhere)
        h = N // 2
        sa, Sa = ops.vca_moments(d[:h])
        sb, Sb = ops.vca_moments(d[h:], sa, Sa)
        assert sb is sa and Sb is Sa
        assert ((sa.cpu() - s_ref).abs() <= (K + 2) * U * s_abs).all() and ((Sa.cpu() - S_ref).abs() <= (K + 2) * U * S_abs).all()
        if h % K == 0:  # cut on a partial's boundary: the same fp32 partials, added in float64 in another grouping
            assert ((Sa - S).abs() <= 1e-12 * S_abs.to(DEV)).all() and ((sa - s).abs() <= 1e-12 * s_abs.to(DEV)).all()


def test_moments_of_aligned_halves_equal_the_whole_to_float64_rounding():
    from umhsnerf import ops

    K = ops.vca_rows_per_partial()
    rows = torch.rand(40 * K, 141, generator=torch.Generator().manual_seed(5)).to(DEV)
    s, S = ops.vca_moments(rows)
    sa, Sa = ops.vca_moments(rows[: 20 * K])
    ops.vca_moments(rows[20 * K :], sa, Sa)
    assert ((Sa - S).abs() <= 1e-13 * S.abs()).all() and ((sa - s).abs() <= 1e-13 * s.abs()).all()


# ---- 6: projection and arg-max --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,R,N", [(3, 3, 50), (31, 6, 4097), (141, 4, 20001), (256, 15, 9000)])
def test_projection_matches_float64(B, R, N):
    """x_k is an fp32 dot product of length B (fmaf chain per lane, then a tree over the lanes): |dx_k| <= (B + 2) u sum_b |y_b w_bk|.
    Projective form y_k = x_k / (x_15 + 1e-6): the quotient inherits (|dx_k| + |y_k| |dx_15|) / den plus two roundings (the
    addition of 1e-6 and the division)."""
    from umhsnerf import ops

    g = torch.Generator().manual_seed(B + N)
    rows = torch.rand(N, B, generator=g)
    basis = torch.zeros(B, 16)
    basis[:, :R] = torch.randn(B, R, generator=g) / B ** 0.5
    basis[:, 15] = torch.rand(B, generator=g) * 0.5 + 0.5  # a denominator well away from zero
    r64, b64 = rows.double(), basis.double()
    x = r64 @ b64
    tol_x = (B + 2) * U * (r64.abs() @ b64.abs())
    den = x[:, 15:16] + 1e-6
    y_ref = x / den
    y_ref[:, 15] = 0
    tol = (tol_x + y_ref.abs() * tol_x[:, 15:16]) / den * (1 + 1e-3) + 4 * U * y_ref.abs()
    y, mx = ops.vca_project(rows.to(DEV), basis.to(DEV), R)
    assert mx is None and tuple(y.shape) == (N, 16)
    err = (y.cpu().double() - y_ref).abs()
    print(f"project B={B}: max error / tolerance {float((err / tol.clamp_min(1e-300))[:, :R].max()):.3f}")
    assert (err <= tol).all() and (y[:, R:] == 0).all()
    # affine form: x = basis^T (row - mean); the subtraction rounds once more
    mean = rows.mean(0)
    basis[:, 15] = 0
    b64 = basis.double()
    c64 = (rows - mean).double()  # the fp32 difference the kernel forms, exactly
    xa = c64 @ b64
    tol_a = (B + 2) * U * (c64.abs() @ b64.abs())
    ya, mx = ops.vca_project(rows.to(DEV), basis.to(DEV), R, mean=mean.to(DEV))
    assert ((ya.cpu().double() - xa).abs() <= tol_a).all()
    sq = (ya.double() ** 2).sum(1).max().item()  # 16 products and a 6-level tree in fp32: at most 8 roundings on the way
    assert abs(float(mx) - sq) <= 8 * U * sq
    assert abs(float(mx) - float((xa ** 2).sum(1).max())) <= 1e-4 * sq
    out = torch.full((N + 2, 16), 7.0, device=DEV)
    ops.vca_project(rows.to(DEV), basis.to(DEV), R, mean=mean.to(DEV), out=out[1 : N + 1])
    assert torch.equal(out[1 : N + 1], ya) and (out[0] == 7).all() and (out[-1] == 7).all()  # nothing outside its rows


@pytest.mark.parametrize("N", [1, 777, 300001])
def test_argmax_matches_float64_and_the_lowest_index_wins_a_tie(N):
    from umhsnerf import ops

    g = torch.Generator().manual_seed(N)
    y = torch.randn(N, 16, generator=g)
    y[:, 9:] = 0
    f = torch.randn(16, generator=g)
    bias = 0.25
    p = (2 * N) // 3
    y[p] *= 8  # a clear winner unless its own |v| is tiny; asserted on the float64 side below
    v = (bias + y.double() @ f.double()).abs()
    top = torch.sort(v).values[-2:]
    if N > 1:
        assert (top[1] - top[0]) / top[1] > 1e-3
    want = int(torch.argmax(v))
    idx, row, val = ops.vca_argmax(y.to(DEV), f.tolist(), bias)
    assert idx.dtype == torch.int64 and int(idx) == want
    assert torch.equal(row.cpu(), y[want])
    assert abs(float(val) - float(v[want])) <= 18 * U * float(abs(bias) + y[want].double().abs() @ f.double().abs())
    # ties: a copy of the winner behind it, then also one in front
    back = torch.cat([y, y[want : want + 1]])
    assert int(ops.vca_argmax(back.to(DEV), f.tolist(), bias)[0]) == want
    both = torch.cat([y[want : want + 1], y, y[want : want + 1]])
    assert int(ops.vca_argmax(both.to(DEV), f.tolist(), bias)[0]) == 0
    many = y[want : want + 1].repeat(70000, 1)  # equal values in every thread, wave and block
    many[:5] = 0  # |v| = |bias| there
    assert float(v[want]) > 2 * abs(bias)
    assert int(ops.vca_argmax(many.to(DEV), f.tolist(), bias)[0]) == 5


# ---- 7: the fixture cubes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["b31", "b128", "b141"])
def test_endmembers_of_the_fixture_cubes_are_the_references(golden_dir, name):
    """Same pixels as the reference; endmembers within twice the reference's own fp32 distance from its float64 run (our fp32
    operations are not in its order)."""
    from umhsnerf.data.utils.vca import vca_endmembers

    g, cube, R, draws = _fixture(golden_dir, name)
    E, idx, info = vca_endmembers(torch.from_numpy(cube).to(DEV), R, draws=draws)
    assert info["branch"] == "projective" and info["snr"] > info["snr_th"]
    assert np.array_equal(idx.numpy(), g["indice_f64"]) and np.array_equal(idx.numpy(), g["indice_f32"])
    dist, d_ref = float(np.max(np.abs(E.numpy().astype(np.float64) - g["Ae_f64"].T))), float(g["d_ref"])
    print(f"vca {name}: max|E_gpu - Ae_f64| = {dist:.3e}, d_ref = {d_ref:.3e}")
    assert dist <= 2 * d_ref + 1e-6
    E2, idx2, _ = vca_endmembers(torch.from_numpy(cube), R, draws=draws, device=DEV)  # host-resident input: same bits
    assert torch.equal(E, E2) and torch.equal(idx, idx2)


def test_endmembers_below_the_snr_threshold_match_the_restatement(golden_dir):
    from umhsnerf.data.utils.vca import vca_endmembers

    g, cube, R, draws = _fixture(golden_dir, "b31_low")
    Ae, want, ref = vca_f64(cube.reshape(-1, cube.shape[-1]).T, R, draws)
    E, idx, info = vca_endmembers(torch.from_numpy(cube).to(DEV), R, draws=draws)
    assert info["branch"] == "affine" == ref["branch"] and abs(info["snr"] - ref["snr"]) < 1e-3
    assert np.array_equal(idx.numpy(), want)
    dist, d_ref = float(np.max(np.abs(E.numpy().astype(np.float64) - Ae.T))), _d_ref(golden_dir, 31)
    print(f"vca b31_low: max|E_gpu - E_f64| = {dist:.3e}, d_ref (b31) = {d_ref:.3e}")
    assert dist <= 2 * d_ref + 1e-6


# ---- 8: stacks ----------------------------------------------------------------------------------------------------------------------
def _cams(n, H, W):
    from umhsnerf.data.umhs_dataparser import Cameras

    g = torch.Generator().manual_seed(n)
    pos = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1) * 0.9
    z = torch.nn.functional.normalize(pos, dim=-1)
    x = torch.nn.functional.normalize(torch.linalg.cross(torch.tensor([[0.0, 0, 1]]).expand(n, 3), z), dim=-1)
    c2w = torch.stack([x, torch.linalg.cross(z, x), z, pos], -1).contiguous()
    return Cameras(c2w, torch.full((n,), 30.0), torch.full((n,), 30.0), torch.full((n,), W / 2), torch.full((n,), H / 2), H, W)


def _split(stack, on_gpu=True):
    from umhsnerf.data.umhs_datamanager import ResidentSplit

    n, H, W, _ = stack.shape
    rgb = torch.rand(n, H, W, 3, generator=torch.Generator().manual_seed(0))
    return ResidentSplit(_cams(n, H, W), rgb, torch.from_numpy(stack), DEV, on_gpu=on_gpu)


@pytest.mark.parametrize("shape,B,R,seed", [((4, 64, 64), 31, 6, 7), ((3, 48, 48), 141, 4, 8), ((2, 64, 64), 128, 9, 9)])
def test_whole_stack_first_frame_and_host_resident_stack(golden_dir, shape, B, R, seed):
    from umhsnerf.data.utils.vca import vca_endmembers

    stack = make_cube(shape, B, R, 40.0, seed)
    draws = draws_from_seed(R, 1234)
    Ae, want, ref = vca_f64(stack.reshape(-1, B).T, R, draws)
    print(f"stack {shape} B={B}: smallest arg-max margin {ref['margins'].min():.3e}, branch {ref['branch']}")
    assert ref["margins"].min() >= 1e-3  # fp32 cannot pick another pixel
    split = _split(stack)
    E, idx, info = split.vca_endmembers(R, num_images=None, draws=draws)
    assert info["branch"] == ref["branch"] and np.array_equal(idx.numpy(), want)
    dist, d_ref = float(np.max(np.abs(E.numpy().astype(np.float64) - Ae.T))), _d_ref(golden_dir, B)
    print(f"stack {shape} B={B}: max|E_gpu - E_f64| = {dist:.3e}, d_ref = {d_ref:.3e}")
    assert dist <= 2 * d_ref + 1e-6
    E0, idx0, _ = split.vca_endmembers(R, draws=draws)  # num_images=1: frame 0, as the reference's dataset
    F0, fidx0, _ = vca_endmembers(torch.from_numpy(stack[0]).to(DEV), R, draws=draws)
    assert torch.equal(E0, F0) and torch.equal(idx0, fidx0) and int(idx0.max()) < shape[1] * shape[2]
    host = _split(stack, on_gpu=False)
    assert not host.hs_image.is_cuda
    Eh, idxh, _ = host.vca_endmembers(R, num_images=None, draws=draws)
    assert torch.equal(Eh, E) and torch.equal(idxh, idx)
    Eh0, idxh0, _ = host.vca_endmembers(R, draws=draws)
    assert torch.equal(Eh0, E0) and torch.equal(idxh0, idx0)
    with pytest.raises(ValueError):
        split.vca_endmembers(R, num_images=shape[0] + 1)


# ---- 9: through the pipeline -----------------------------------------------------------------------------------------------------
def test_load_vca_through_the_pipeline(tmp_path, monkeypatch):
    from umhsnerf.data.umhs_datamanager import UMHSDataManager, UMHSDataManagerConfig
    from umhsnerf.data.utils import vca as V
    from umhsnerf.umhs_model import UMHSConfig, UMHSModel
    from umhsnerf.umhs_pipeline import UMHSPipeline

    monkeypatch.chdir(tmp_path)  # no vca.npy in the working directory
    torch.manual_seed(0)
    n, H, W, B, C = 4, 32, 32, 31, 6
    stack = make_cube((n, H, W), B, C, 40.0, 11)
    split = _split(stack)
    meta = {"wavelengths": list(np.linspace(420, 680, B)), "num_classes": C}
    mk = lambda: UMHSDataManager(UMHSDataManagerConfig(train_num_rays_per_batch=1024), device=DEV, seed=1, train=split)
    cfg = lambda on: UMHSConfig(method="rgb+spectral", pred_specular=True, temperature=0.4, background_color="black", load_vca=on)
    pipe = UMHSPipeline.from_packed_samples(cfg(True), DEV, metadata=meta, seed=2, datamanager=mk())
    E, idx, info = split.vca_endmembers(C)
    assert torch.equal(pipe.model.field.endmembers.detach().cpu(), E) and info["branch"] in ("projective", "affine")
    assert not os.path.exists("vca.npy")  # nothing is written
    # every row is a pixel of frame 0 projected onto the basis of frame 0
    rows0 = stack[0].reshape(-1, B).astype(np.float64)
    assert int(idx.max()) < H * W
    plan = V.vca_plan(rows0.sum(0), rows0.T @ rows0, H * W, C)
    assert plan["branch"] == info["branch"]
    assert np.max(np.abs(V.vca_finish(plan, rows0[idx.numpy()]) - E.numpy())) < 1e-4
    # off: the parameters of the seed, VCA or not
    off = UMHSPipeline.from_packed_samples(cfg(False), DEV, metadata=meta, seed=2, datamanager=mk())
    plain = UMHSModel(cfg(False), metadata=meta, seed=2)
    assert torch.equal(off.model.field.flat.detach().cpu(), plain.field.flat.detach())
    o = plain.field.layout.offset("endmembers")
    assert torch.equal(pipe.model.field.flat.detach().cpu()[:o], plain.field.flat.detach()[:o])
    assert not torch.equal(off.model.field.endmembers.detach().cpu(), E)
    with torch.no_grad():
        split.image = pipe.model.converter(split.hs_image.view(-1, B)).view(n, H, W, 3).contiguous()
    losses = []
    for step in range(5):
        _, loss_dict, _ = pipe.get_train_loss_dict(step)
        losses.append(float(sum(loss_dict.values()).detach()))
    assert np.isfinite(losses).all(), losses
