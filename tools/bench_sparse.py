"""Sparse unmixing: ``ops.sparse_unmix`` (csrc/umhs_sparse.hip) against the arithmetic of its iteration at the fp32-MFMA rate, the same
iteration composed in torch, and a copy of its bytes; and what ``sparse_pred`` adds to a rendered frame (not bench.py: that measures the
training step).  GPU box.  Records, not gates.

Kernel (device events, warm, median and min of ROUNDS >= 5, the variants alternated inside one process), at 921,600 rows (one
1280 x 720 frame) x (31 bands, 32 entries), (128, 64) and (141, 128); libraries of the recipe of tests/sparse_f64.py (31 x 32 has more
entries than bands: no singular-value floor there); lambda 1e-3, epsilon 1e-4, 400 iterations, mu auto; two row mixes: ``interior`` (two
entries, noise 0.001) and ``mixed`` (three entries, noise 0.01):
  sparse_<mix>_b<B>_l<L>_ms        the kernel, abundances and residual and status
  sparse_<mix>_b<B>_l<L>_nores_ms  the kernel, abundances alone
  iterations_<mix>_*               [mean per row, largest, mean over the 32-row tiles of a tile's largest (what a wave pays)]; a capped
                                   row counts max_iterations; capped_<mix>_*: the rows stopped there
  mfma_<mix>_*_ms                  (a) 2 L^2 iterations R FLOP (iterations: the per-row mean) at the fp32-MFMA rate MEASURED in this run,
                                   mfma_measured_TFLOPs: ``ops.library_match`` of the same rows' worth of work at 256 bands x 4096 entries,
                                   2 R B L over its time; mfma_guide_<mix>_*_ms: the same FLOP at the 157.3 TFLOP/s of the guide
  mfma_tiles_<mix>_*_ms            the FLOP the kernel issues: 2 (32 T)^2 x the tile's largest iteration count, at the measured rate
  torch_<mix>_*_ms                 (b) the iteration in torch (matmul + elementwise on [R,L] tensors) at round(mean iterations), no stopping
  copy_b<B>_l<L>_ms                (c) a device copy of the bytes read and written (R B 4 read, R (L + 2) 4 written)
Model (bench.py's ``sampler_scene`` after 300 steps; one 1280 x 720 camera, rays generated outside the clock), alternated in one run:
  frame_720_plain_ms / frame_720_sparse_ms   ``rgb`` alone, and ``rgb sparse_pred`` under ``sparse_unmixing_context`` with a 128-entry library
Prints one JSON line and writes it to --out (default profiles/sparse/bench_sparse.json)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "unsupervised-hyperspectral-nerf_amd"), os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))]
import numpy as np
import torch

import bench
import sparse_f64 as SF
from bench_material import _cameras, alternate
from umhsnerf import ops
from umhsnerf.library import SpectralLibrary
from umhsnerf.sparse import SparseUnmixer

DEV = torch.device("cuda", 0)
ROUNDS, ROWS = 7, 1280 * 720
SHAPES = ((31, 32), (128, 64), (141, 128))
MIXES = (("interior", 2, 0.001), ("mixed", 3, 0.01))
MFMA_GUIDE_TFLOPS = 157.3
MATCH_BANDS, MATCH_ENTRIES = 256, 4096


def bench_library(L, B, seed=1):
    """float32 [L,B]: tests/sparse_f64.py's synthetic library; with more entries than bands the same smooth spectra, no floor."""
    if L <= B:
        return SF.synthetic_library(L, B, seed)
    g = np.random.default_rng(100 * seed + 7 * L + B)
    p = (np.arange(B) + 0.5) / B
    A = g.uniform(0.1, 0.3, (L, 1)) + 0.15 * g.uniform(0.0, 1.0, (L, B))
    for _ in range(2):
        A = A + g.uniform(0.2, 0.6, (L, 1)) * np.exp(-0.5 * ((p[None, :] - g.uniform(0.0, 1.0, (L, 1))) / g.uniform(0.05, 0.2, (L, 1))) ** 2)
    return np.ascontiguousarray(A.astype(np.float32))


def rows_of(A, entries, sigma, g):
    L, B = A.shape
    a = torch.zeros(ROWS, L)
    a.scatter_(1, torch.randint(L, (ROWS, entries), generator=g), 0.2 + 0.8 * torch.rand(ROWS, entries, generator=g))
    return (a @ torch.from_numpy(A) + sigma * torch.randn(ROWS, B, generator=g)).float().to(DEV)


def torch_admm(x, Q, M, theta, iterations):
    c = x @ Q.T
    tau = theta * x.square().sum(1, keepdim=True).sqrt()
    z, d = torch.zeros_like(c), torch.zeros_like(c)
    for _ in range(iterations):
        t = torch.addmm(c, z - d, M.T) + d
        z = (t - tau).clamp_min(0.0)
        d = t - z
    return z


def measured_mfma_tflops(rounds):
    g = torch.Generator().manual_seed(3)
    unit = torch.nn.functional.normalize(torch.rand(MATCH_ENTRIES, MATCH_BANDS, generator=g), dim=1).to(DEV)
    image, x = ops.library_prepare(unit), torch.rand(ROWS, MATCH_BANDS, generator=g).to(DEV)
    t = alternate({"match": lambda: ops.library_match(x, image, MATCH_ENTRIES)}, rounds, reps=1, warm=2)["match"]
    return 2.0 * ROWS * MATCH_BANDS * MATCH_ENTRIES / t["median"] / 1e9, t


def kernel_part(rounds):
    g = torch.Generator().manual_seed(5)
    res = {"rows": ROWS, "lambda": SF.LAMBDA, "epsilon": SF.EPSILON, "max_iterations": SF.MAX_ITERATIONS}
    rate, res["match_b256_l4096_ms"] = measured_mfma_tflops(rounds)
    res["mfma_measured_TFLOPs"], res["mfma_guide_TFLOPs"] = rate, MFMA_GUIDE_TFLOPS
    for B, L in SHAPES:
        tag = f"b{B}_l{L}"
        A = bench_library(L, B)
        mu = SF.auto_mu(A)
        operands = ops.sparse_prepare(torch.from_numpy(A).to(DEV), SF.LAMBDA, mu)
        P = SF.prepare(A, SF.LAMBDA, mu)
        Q, M = torch.from_numpy(P["Q32"]).to(DEV), torch.from_numpy(P["M32"]).to(DEV)
        n = (ROWS * B * 4 + ROWS * (L + 2) * 4) // 8
        src, dst = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
        xs = {mix: rows_of(A, entries, sigma, g) for mix, entries, sigma in MIXES}
        counts = {}
        for mix, x in xs.items():
            _, _, status = ops.sparse_unmix(x, operands, SF.EPSILON, SF.MAX_ITERATIONS, False, True)
            it = torch.where(status == -2, torch.full_like(status, SF.MAX_ITERATIONS), status.clamp_min(0)).float()
            tiles = torch.nn.functional.pad(it, (0, (-ROWS) % 32)).view(-1, 32).max(1).values
            counts[mix] = (float(it.mean()), int(it.max()), float(tiles.mean()))
            res[f"iterations_{mix}_{tag}"] = list(counts[mix])
            res[f"capped_{mix}_{tag}"] = int((status == -2).sum())
        variants = {f"copy_{tag}_ms": lambda: dst.copy_(src)}
        for mix, x in xs.items():
            variants[f"sparse_{mix}_{tag}_ms"] = lambda x=x: ops.sparse_unmix(x, operands, SF.EPSILON, SF.MAX_ITERATIONS, True, True)
            variants[f"sparse_{mix}_{tag}_nores_ms"] = lambda x=x: ops.sparse_unmix(x, operands, SF.EPSILON, SF.MAX_ITERATIONS, False, False)
            variants[f"torch_{mix}_{tag}_ms"] = lambda x=x, k=int(round(counts[mix][0])): torch_admm(x, Q, M, operands.theta, k)
        res.update(alternate(variants, rounds, reps=1, warm=2))
        res[f"bytes_{tag}"], res[f"cond_a_{tag}"], res[f"mu_{tag}"] = n * 8, float(np.linalg.cond(A.astype(np.float64))), mu
        T = (L + 31) // 32
        for mix in xs:
            mean, _, tile = counts[mix]
            kernel = res[f"sparse_{mix}_{tag}_ms"]["median"]
            res[f"mfma_{mix}_{tag}_ms"] = 2.0 * L * L * mean * ROWS / (rate * 1e12) * 1e3
            res[f"mfma_guide_{mix}_{tag}_ms"] = 2.0 * L * L * mean * ROWS / (MFMA_GUIDE_TFLOPS * 1e12) * 1e3
            res[f"mfma_tiles_{mix}_{tag}_ms"] = 2.0 * (32 * T) ** 2 * tile * ROWS / (rate * 1e12) * 1e3
            res[f"sparse_{mix}_{tag}_over_mfma"] = kernel / res[f"mfma_{mix}_{tag}_ms"]
            res[f"sparse_{mix}_{tag}_over_mfma_tiles"] = kernel / res[f"mfma_tiles_{mix}_{tag}_ms"]
            res[f"torch_{mix}_{tag}_over_sparse"] = res[f"torch_{mix}_{tag}_ms"]["median"] / kernel
            res[f"sparse_{mix}_{tag}_over_copy"] = kernel / res[f"copy_{tag}_ms"]["median"]
        del xs, src, dst
    return res


def model_part(rounds, pipe):
    model = pipe.model.eval()
    rays = _cameras(720, 1280).generate_rays(0, keep_shape=True)
    wl = [float(w) for w in model.kwargs["wavelengths"]]
    B = len(wl)
    L = 128
    library = SpectralLibrary([f"entry_{k}" for k in range(L)], bench_library(L, B).astype(np.float64), wl)
    unmixer = SparseUnmixer(library)

    def frame(u, names):
        with model.sparse_unmixing_context(u):
            return model.get_outputs_for_camera_ray_bundle(rays, output_names=names)

    res = alternate({"frame_720_plain_ms": lambda: frame(None, ["rgb"]),
                     "frame_720_sparse_ms": lambda: frame(unmixer, ["rgb", "sparse_pred"])}, rounds, reps=1, warm=2)
    plain, with_sparse = res["frame_720_plain_ms"]["median"], res["frame_720_sparse_ms"]["median"]
    out = frame(unmixer, ["spectral"])
    _, _, status = unmixer.unmix(out["spectral"], False, True)
    ok = status > 0
    res.update(bands=B, entries=L, frame_720_sparse_minus_plain_ms=with_sparse - plain, frame_720_sparse_share=(with_sparse - plain) / with_sparse,
               mean_iterations=float(status[ok].float().mean()) if bool(ok.any()) else None, capped=int((status == -2).sum()),
               invalid=int((status == -1).sum()))
    pipe.model.train()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse", "bench_sparse.json"))
    ap.add_argument("--rounds", type=int, default=ROUNDS)
    ap.add_argument("--no-model", action="store_true", help="the kernel part alone")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: nothing here is measured without one"
    rounds = max(args.rounds, 5)
    res = {"bench": "sparse", "device": torch.cuda.get_device_name(0), "rounds": rounds, "kernel": kernel_part(rounds)}
    if not args.no_model:
        pipe, _ = bench.sampler_scene(bench.C2, DEV)
        res["model"] = model_part(rounds, pipe)
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
