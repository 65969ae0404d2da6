"""Camera-path rendering, stage by stage (not bench.py: that measures the training step).  GPU box.

Model: C2-shaped (31 bands, 6 classes, pred_specular): bench.py's ``sampler_scene`` -- 300 training steps on its synthetic target, so
that the occupancy grid has settled and a ray keeps what ``eval_image`` measures.  (A randomly initialised model is no yardstick here:
its grid is empty, the march keeps 3e-5 samples per ray and "renders" 50 M rays/s of background.)  Paths: 8 cameras on a circle
around the target, the training cameras' distance and field of view, at 256 x 256 and at 1280 x 720.  Panel sets: ``rgb + abundances_0..5`` (all six abundances of C2) and ``wv_0..wv_20`` (21 panels: two
launches of the compose kernel and a join, see render.compose_frame).

Per (size, panel set), per frame:
  render_ms   rays + get_outputs_for_camera_ray_bundle(output_names=base tensors), host clock around a device synchronise
  compose_ms  render.compose_frame (the HIP kernel), device events over REPS repetitions; compose_GBps = bytes the algorithm moves
              (3 bytes stored per pixel and panel + 4 bytes read per channel read) over that time; store_GBps = the stored bytes alone
  torch_ms    the same frame composed by torch ops on the device (the nerfstudio way: column copy, clip, long(), gather, cat, x255,
              cast), device events; ``torch_equal`` says whether its bytes equal the kernel's
  memcpy_ms   a plain device-to-device copy of the frame's bytes: the ceiling of the store side
  d2h_ms      frame -> pinned host buffer, device events
  encode_ms   PIL PNG encode + write of one frame on ONE thread, host clock
  fps         render_camera_path end to end (4 encoder threads), all 8 frames, files written; fps_torch the same loop composing with
              the torch ops
Prints one JSON line and writes it to --out.  ``--compose-only`` runs just the two compositions (REPS each, per size and panel set) and
prints nothing measured: it is the command to put under ``rocprofv3 --kernel-trace --stats`` for the kernels' own times (the event
timings above include the host's issue time, which bounds small frames)."""
import argparse
import json
import math
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "unsupervised-hyperspectral-nerf_amd")]
import numpy as np
import torch

import bench
from umhsnerf import ops, render
from umhsnerf.utils import colormaps

DEV = torch.device("cuda", 0)
B, C, FRAMES, REPS = 31, 6, 8, 20
PANEL_SETS = {"rgb+abundances": ["rgb"] + [f"abundances_{i}" for i in range(C)], "wv_0..20": [f"wv_{i}" for i in range(21)]}


def camera_path(height, width, n=FRAMES, radius=0.8, fov=2 * math.degrees(math.atan(32.0 / 30.0))):
    cams = []
    for k in range(n):
        a = 2 * math.pi * k / n
        pos = np.array([radius * math.cos(a), radius * math.sin(a), 0.4])
        z = pos / np.linalg.norm(pos)  # the camera looks down -z, at the origin
        x = np.cross([0.0, 0.0, 1.0], z)
        x /= np.linalg.norm(x)
        m = np.eye(4)
        m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, np.cross(z, x), z, pos
        cams.append({"camera_to_world": m.reshape(-1).tolist(), "fov": fov, "aspect": width / height})
    return {"camera_type": "perspective", "render_height": height, "render_width": width, "camera_path": cams, "fps": 24, "seconds": n / 24}


def torch_compose(outputs, names, colormap_options=None, depth_near_plane=None, depth_far_plane=None, out=None):
    """include/umhs_hip.h's arithmetic with torch ops, panel by panel (RGB and SCALAR without normalize: what the panel sets here use)."""
    lut = colormaps.device_table("default", DEV)
    panels = []
    for name in names:
        t, ch, kind = render.resolve_output(outputs, name)
        if kind == ops.PANEL_RGB:
            panels.append(t)
        else:
            v = t[..., ch].clip(0, 1)
            v = torch.nan_to_num(v, nan=0.0)
            panels.append(lut[(v * 255).long()])
    frame = torch.cat(panels, dim=1)
    return ((frame * 255) + 0.5).clamp(0, 255).nan_to_num(nan=0.0).to(torch.uint8)


def device_ms(fn, reps=REPS):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="256x256,1280x720")
    ap.add_argument("--compose-only", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: nothing here is measured without one"
    assert (bench.C2["B"], bench.C2["C"]) == (B, C)
    pipe, _ = bench.sampler_scene(bench.C2, DEV)
    pipe.eval()
    model, rows = pipe.model, []
    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        cameras, _ = render.load_camera_path(camera_path(H, W), device=DEV)
        for set_name, names in PANEL_SETS.items():
            keys = render.source_keys(names) + ["num_samples_per_ray"]
            with torch.no_grad():
                def rendered(i):
                    return model.get_outputs_for_camera_ray_bundle(cameras.generate_rays(i), output_names=keys)

                rendered(0)  # warm up this shape
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(FRAMES):
                    outputs = rendered(i)
                torch.cuda.synchronize()
                render_ms = (time.perf_counter() - t0) / FRAMES * 1e3
                frame = render.compose_frame(outputs, names)
                compose_ms = device_ms(lambda: render.compose_frame(outputs, names, out=frame))
                tframe = torch_compose(outputs, names)
                torch_ms = device_ms(lambda: torch_compose(outputs, names))
                if args.compose_only:
                    continue
                other = torch.empty_like(frame)
                memcpy_ms = device_ms(lambda: other.copy_(frame))
                pinned = torch.empty(frame.shape, dtype=torch.uint8).pin_memory()
                d2h_ms = device_ms(lambda: pinned.copy_(frame, non_blocking=True))
                torch.cuda.synchronize()
                host = pinned.numpy().copy()
                with tempfile.TemporaryDirectory() as tmp:
                    t0 = time.perf_counter()
                    render._encode(host, os.path.join(tmp, "frame.png"), "png", 100)
                    encode_ms = (time.perf_counter() - t0) * 1e3
                    png_bytes = os.path.getsize(os.path.join(tmp, "frame.png"))
                    res = render.render_camera_path(pipe, cameras, os.path.join(tmp, "hip"), names)
                    res_torch = render.render_camera_path(pipe, cameras, os.path.join(tmp, "torch"), names, compose_fn=torch_compose)
            stored = frame.numel()
            read = 4 * H * W * sum(3 if n == "rgb" else 1 for n in names)
            rows.append({"size": f"{W}x{H}", "panels": set_name, "n_panels": len(names), "frame_bytes": stored, "png_bytes": png_bytes,
                         "render_ms": render_ms, "rays_per_s": H * W / render_ms * 1e3,
                         "samples_per_ray": float(outputs["num_samples_per_ray"].float().mean()) if "num_samples_per_ray" in outputs else None, "compose_ms": compose_ms, "torch_ms": torch_ms,
                         "torch_equal": bool(torch.equal(frame, tframe)), "memcpy_ms": memcpy_ms, "d2h_ms": d2h_ms, "encode_ms": encode_ms,
                         "compose_GBps": (stored + read) / compose_ms / 1e6, "store_GBps": stored / compose_ms / 1e6,
                         "memcpy_GBps": stored / memcpy_ms / 1e6, "fps": res["fps"], "fps_torch": res_torch["fps"]})
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    if args.compose_only:
        return
    result = {"bench": "render", "model": {"bands": B, "classes": C, "pred_specular": True}, "frames": FRAMES, "reps": REPS,
              "device": torch.cuda.get_device_name(0), "rows": rows}
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
