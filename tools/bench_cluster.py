"""Spectral clustering: ``ops.cluster_step`` (csrc/umhs_cluster.hip) with and without the accumulator against the torch composition it
replaces, a copy of its bytes and the matrix-core time of its products; and one Lloyd iteration over the captured stack of bench.py's
synthetic scene with the cost of its one host read (not bench.py: that measures the training step).  GPU box.  Records, not gates.

Kernels (device events, warm, median and min of ROUNDS >= 5, the variants alternated inside one process), at 921,600 rows (one
1280 x 720 frame), (B, K) = (31, 6), (31, 64), (128, 16), (141, 64), both metrics:
  step_<m>_b<B>_k<K>_ms / assign_<m>_b<B>_k<K>_ms   the kernel with ``acc`` (assign + sums, two launches per 512 chunks) and without (one launch)
  torch_<m>_b<B>_k<K>_ms                            ``normalize`` (angle) + ``matmul`` + ``argmax`` + ``index_add_`` of the member vectors
  copy_b<B>_k<K>_ms                                 a device copy of the bytes the step reads and writes (R B 4 read, R 8 written, the chunk
                                                    partials written and read once)
  mfma_b<B>_k<K>_ms                                 4 R K B / 157.3 TFLOP/s (the distances and the one-hot sums): arithmetic, not a run
Lloyd (bench.py's ``sampler_scene`` captured stack, 6 x 64 x 64 x 31, K = 6, angle), alternated in one run:
  lloyd_iteration_ms   ``cluster_step`` of every frame into one accumulator, the host read and the float64 update (wall clock)
  lloyd_device_ms      the launches alone (device events);  lloyd_host_read_ms  the accumulator's ``.cpu()`` alone (wall clock)
Prints one JSON line and writes it to --out (default profiles/cluster/bench_cluster.json)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "unsupervised-hyperspectral-nerf_amd"), os.path.dirname(os.path.abspath(__file__))]
import torch

import bench
from bench_material import alternate, device_ms, stats
from umhsnerf import cluster, ops

DEV = torch.device("cuda", 0)
ROUNDS, ROWS = 7, 1280 * 720
SHAPES = ((31, 6), (31, 64), (128, 16), (141, 64))
MFMA_F32_TFLOPS = 157.3


def kernel_part(rounds):
    g = torch.Generator().manual_seed(5)
    res = {"rows": ROWS}
    for B, K in SHAPES:
        centres = torch.rand(K, B, generator=g) * 0.9 + 0.05
        x = ((0.5 + torch.rand(ROWS, 1, generator=g)) * (centres[torch.randint(0, K, (ROWS,), generator=g)]
                                                          + 0.02 * torch.randn(ROWS, B, generator=g))).to(DEV)
        n_acc = 2 + K + K * B
        nbytes = ROWS * B * 4 + ROWS * 8 + 2 * -(-ROWS // ops.cluster_chunk()) * n_acc * 4
        src, dst = torch.empty(nbytes // 8, device=DEV), torch.empty(nbytes // 8, device=DEV)
        tag = f"b{B}_k{K}"
        variants = {f"copy_{tag}_ms": lambda: dst.copy_(src)}
        compare = {}
        for metric in ("angle", "euclidean"):
            c = (centres / centres.norm(dim=1, keepdim=True) if metric == "angle" else centres).to(DEV).contiguous()
            image = ops.library_prepare(c)
            half = (c.double().pow(2).sum(1) / 2).float() if metric == "euclidean" else None
            acc = torch.zeros(n_acc, dtype=torch.float64, device=DEV)

            def torch_step(c=c, half=half, metric=metric):
                v = torch.nn.functional.normalize(x, dim=1) if metric == "angle" else x
                val = v @ c.T if metric == "angle" else x @ c.T - half
                label = val.argmax(1)
                return label, torch.zeros(K, B, device=DEV).index_add_(0, label, v)

            variants[f"step_{metric}_{tag}_ms"] = lambda image=image, half=half, acc=acc, metric=metric: ops.cluster_step(x, image, K, metric, half, acc=acc)
            variants[f"assign_{metric}_{tag}_ms"] = lambda image=image, half=half, metric=metric: ops.cluster_step(x, image, K, metric, half)
            variants[f"torch_{metric}_{tag}_ms"] = torch_step
            compare[metric] = (image, half, torch_step)
        res.update(alternate(variants, rounds, reps=2, warm=2))
        res[f"mfma_{tag}_ms"] = 4.0 * ROWS * K * B / (MFMA_F32_TFLOPS * 1e12) * 1e3
        res[f"bytes_{tag}"] = nbytes
        for metric, (image, half, torch_step) in compare.items():
            mine = res[f"step_{metric}_{tag}_ms"]["median"]
            res[f"step_{metric}_{tag}_over_copy"] = mine / res[f"copy_{tag}_ms"]["median"]
            res[f"step_{metric}_{tag}_over_mfma"] = mine / res[f"mfma_{tag}_ms"]
            res[f"assign_{metric}_{tag}_over_copy"] = res[f"assign_{metric}_{tag}_ms"]["median"] / res[f"copy_{tag}_ms"]["median"]
            res[f"torch_{metric}_{tag}_over_step"] = res[f"torch_{metric}_{tag}_ms"]["median"] / mine
            # a record that both looked at the same thing: the share of equal labels, the largest relative difference of the sums
            acc = torch.zeros(n_acc, dtype=torch.float64, device=DEV)
            label, _ = ops.cluster_step(x, image, K, metric, half, acc=acc)
            want_label, want_sums = torch_step()
            res[f"labels_{metric}_{tag}_vs_torch"] = float((label.long() == want_label).float().mean())
            res[f"sums_{metric}_{tag}_vs_torch"] = float((acc[2 + K:].view(K, B) - want_sums.double()).abs().max() / want_sums.abs().max())
        del x, src, dst
    return res


def lloyd_part(rounds, pipe):
    stack = pipe.datamanager.train_split.hs_image
    wl = [float(w) for w in pipe.model.kwargs["wavelengths"]]
    g = torch.Generator().manual_seed(7)
    frames = [(stack[i].to(DEV).float() * (0.5 + torch.rand(*stack.shape[1:3], 1, generator=g).to(DEV))).contiguous() for i in range(stack.shape[0])]
    K, B = 6, stack.shape[-1]
    init = torch.rand(K, B, generator=g).double().numpy() + 0.05
    clusters = cluster.SpectralClusters(init, "angle", wl)
    acc = torch.zeros(2 + K + K * B, dtype=torch.float64, device=DEV)

    def launches():
        acc.zero_()
        for f in frames:
            clusters.step(f, None, acc, want_label=False, want_score=False)

    def wall(fn, reps=5):
        torch.cuda.synchronize()
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) * 1e3)
        return t

    def iteration():
        launches()
        cluster.update(clusters.centres, acc.cpu().numpy(), "angle")

    launches()
    res = {"frames": len(frames), "rows": int(sum(f[..., 0].numel() for f in frames)), "bands": B, "clusters": K}
    device, whole, read = [], [], []
    for _ in range(rounds):
        device.append(device_ms(launches, reps=2))
        whole += wall(iteration, reps=2)
        read += wall(lambda: acc.cpu(), reps=2)
    res.update(lloyd_device_ms=stats(device), lloyd_iteration_ms=stats(whole), lloyd_host_read_ms=stats(read))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster", "bench_cluster.json"))
    ap.add_argument("--rounds", type=int, default=ROUNDS)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: nothing here is measured without one"
    rounds = max(args.rounds, 5)
    kernel = kernel_part(rounds)
    pipe, _ = bench.sampler_scene(bench.C2, DEV, warm=0)
    res = {"bench": "cluster", "device": torch.cuda.get_device_name(0), "rounds": rounds, "kernel": kernel, "lloyd": lloyd_part(rounds, pipe)}
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
