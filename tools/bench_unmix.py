"""Spectral unmixing: ``ops.unmix`` (csrc/umhs_unmix.hip) against a copy of its bytes, the product alone, a torch projected-gradient
composition and scipy on the host; and what ``--unmix model`` adds to a rendered frame (not bench.py: that measures the training step).
GPU box.  Records, not gates.

Kernel (device events, warm, median and min of ROUNDS >= 5, the variants alternated inside one process), at 921,600 rows (one
1280 x 720 frame) x (31 bands, 6 endmembers), (128, 9) and (141, 16); endmembers of tests/unmix_f64.py's synthetic builder; two row
mixes: ``interior`` (Dirichlet mixtures, noise 0.001: one solve per row) and ``constrained`` (mixtures pushed outside the simplex, noise
0.01: several constraints active); both modes:
  unmix_<mix>_<mode>_b<B>_k<K>_ms   the kernel, abundances and residual
  copy_b<B>_k<K>_ms                 a device copy of the bytes it reads and writes (R B 4 read, R (K + 1) 4 written)
  project_b<B>_k<K>_ms              ``ops.spectral_project`` at the same (K, B), P = K with the score: the product b = E x alone
  torch_pg_<mode>_b<B>_k<K>_ms      projected gradient in torch at a fixed 200 iterations on [R,K] tensors (NNLS: clamp; FCLS: the
                                    sort-based projection onto the simplex); its distance from the kernel's abundances is recorded
  scipy_nnls_b<B>_k<K>_ms           ``scipy.optimize.nnls`` over a 10,000-row sample on 16 host threads, scaled to 921,600 rows
  solves_* / capped_*               the mean and the largest number of solves per row, the rows stopped at the cap
Model (bench.py's ``sampler_scene`` after 300 steps; one 1280 x 720 camera, rays generated outside the clock), alternated in one run:
  frame_720_plain_ms / frame_720_unmix_ms   ``rgb`` alone, and ``rgb unmix_pred unmix_residual`` under ``unmixing_context``
Prints one JSON line and writes it to --out (default profiles/unmix/bench_unmix.json)."""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "unsupervised-hyperspectral-nerf_amd"), os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))]
import numpy as np
import torch

import bench
import unmix_f64 as UF
from bench_material import _cameras, alternate
from umhsnerf import ops
from umhsnerf.unmix import Unmixer

DEV = torch.device("cuda", 0)
ROUNDS, ROWS = 7, 1280 * 720
SHAPES = ((31, 6), (128, 9), (141, 16))
PG_ITERATIONS, SCIPY_ROWS, HOST_THREADS = 200, 10000, 16
MODES = (("nnls", 0), ("fcls", 1))


def rows_of(E, mix, g):
    K = E.shape[0]
    a = torch.distributions.Dirichlet(torch.ones(K)).sample((ROWS,))
    if mix == "constrained":
        a = a + 0.6 * torch.randn(ROWS, K, generator=g) / K ** 0.5
        a = a + (1.0 - a.sum(1, keepdim=True)) / K
    return (a @ E + (0.001 if mix == "interior" else 0.01) * torch.randn(ROWS, E.shape[1], generator=g)).float().to(DEV)


def simplex_projection(v):
    u, _ = torch.sort(v, dim=1, descending=True)
    css = u.cumsum(1) - 1.0
    k = torch.arange(1, v.shape[1] + 1, device=v.device, dtype=v.dtype)
    rho = ((u - css / k) > 0).sum(1, keepdim=True)
    return (v - css.gather(1, rho - 1) / rho.to(v.dtype)).clamp_min(0.0)


def torch_pg(x, E, G, step, mode):
    b = x @ E.T
    a = torch.full_like(b, 1.0 / E.shape[0] if mode else 0.0)
    for _ in range(PG_ITERATIONS):
        a = a - step * (a @ G - b)
        a = simplex_projection(a) if mode else a.clamp_min(0.0)
    return a


def scipy_part(E, x):
    from scipy.optimize import nnls

    A, rows = E.double().numpy().T.copy(), x[:SCIPY_ROWS].double().cpu().numpy()
    chunks = np.array_split(rows, HOST_THREADS)
    t0 = time.perf_counter()
    with ThreadPoolExecutor(HOST_THREADS) as pool:
        list(pool.map(lambda c: [nnls(A, r) for r in c], chunks))
    return (time.perf_counter() - t0) * 1e3 * ROWS / SCIPY_ROWS


def kernel_part(rounds):
    g = torch.Generator().manual_seed(5)
    torch.manual_seed(5)
    res = {"rows": ROWS}
    for B, K in SHAPES:
        tag = f"b{B}_k{K}"
        E = torch.from_numpy(UF.synthetic_endmembers(K, B))
        Ed, G = E.to(DEV), torch.from_numpy(UF.gram32(E.numpy())).to(DEV)
        image = ops.library_prepare(Ed)
        step = 1.0 / float(torch.linalg.eigvalsh(G.double().cpu())[-1])
        n = (ROWS * B * 4 + ROWS * (K + 1) * 4) // 8
        src, dst = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
        zero = torch.zeros(B, device=DEV)
        xs = {mix: rows_of(E, mix, g) for mix in ("interior", "constrained")}
        variants = {f"copy_{tag}_ms": lambda: dst.copy_(src), f"project_{tag}_ms": lambda: ops.spectral_project(xs["interior"], zero, image, K, K)}
        for mix, x in xs.items():
            for name, mode in MODES:
                variants[f"unmix_{mix}_{name}_{tag}_ms"] = lambda x=x, mode=mode: ops.unmix(x, image, G, K, mode)
        for name, mode in MODES:
            variants[f"torch_pg_{name}_{tag}_ms"] = lambda mode=mode: torch_pg(xs["constrained"], Ed, G, step, mode)
        res.update(alternate(variants, rounds, reps=1, warm=2))
        res[f"bytes_{tag}"] = n * 8
        res[f"cond_e_{tag}"] = float(np.linalg.cond(E.double().numpy()))
        for mix, x in xs.items():
            for name, mode in MODES:
                a, _, status = ops.unmix(x, image, G, K, mode, want_status=True)
                ok = status > 0
                res[f"solves_{mix}_{name}_{tag}"] = [float(status[ok].float().mean()), int(status.max())]
                res[f"capped_{mix}_{name}_{tag}"] = int((status == -2).sum())
                res[f"unmix_{mix}_{name}_{tag}_over_copy"] = res[f"unmix_{mix}_{name}_{tag}_ms"]["median"] / res[f"copy_{tag}_ms"]["median"]
                if mix == "constrained":  # a record of how far 200 projected-gradient iterations are from the optimum
                    res[f"torch_pg_{name}_{tag}_vs_kernel"] = float((torch_pg(x, Ed, G, step, mode) - a).abs().max())
                    res[f"torch_pg_{name}_{tag}_over_kernel"] = res[f"torch_pg_{name}_{tag}_ms"]["median"] / res[f"unmix_{mix}_{name}_{tag}_ms"]["median"]
        res[f"scipy_nnls_{tag}_ms"] = scipy_part(E, xs["constrained"])
        del xs, src, dst
    return res


def model_part(rounds, pipe):
    model = pipe.model.eval()
    rays = _cameras(720, 1280).generate_rays(0, keep_shape=True)
    try:
        unmixer = Unmixer.from_model(model)
    except ValueError as e:  # (endmembers too close to dependent after this little training: the guard's message is the record)
        pipe.model.train()
        return {"refused": str(e)}

    def frame(u, names):
        with model.unmixing_context(u):
            return model.get_outputs_for_camera_ray_bundle(rays, output_names=names)

    res = alternate({"frame_720_plain_ms": lambda: frame(None, ["rgb"]),
                     "frame_720_unmix_ms": lambda: frame(unmixer, ["rgb", "unmix_pred", "unmix_residual"])}, rounds, reps=1, warm=2)
    plain, with_unmix = res["frame_720_plain_ms"]["median"], res["frame_720_unmix_ms"]["median"]
    out = frame(unmixer, ["spectral"])
    _, _, status = unmixer.unmix(out["spectral"], False, True)
    res.update(bands=unmixer.bands, endmembers=len(unmixer), cond=unmixer.conditioning["cond"], frame_720_unmix_minus_plain_ms=with_unmix - plain,
               frame_720_unmix_share=(with_unmix - plain) / with_unmix, mean_solves=float(status[status > 0].float().mean()),
               capped=int((status == -2).sum()))
    pipe.model.train()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unmix", "bench_unmix.json"))
    ap.add_argument("--rounds", type=int, default=ROUNDS)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: nothing here is measured without one"
    rounds = max(args.rounds, 5)
    kernel = kernel_part(rounds)
    pipe, _ = bench.sampler_scene(bench.C2, DEV)
    res = {"bench": "unmix", "device": torch.cuda.get_device_name(0), "rounds": rounds, "kernel": kernel, "model": model_part(rounds, pipe)}
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
