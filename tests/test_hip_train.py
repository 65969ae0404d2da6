"""The stand-alone trainer end to end on the GPU: ``python -m umhsnerf.train`` as a child process (run directory, checkpoints, log,
``eval --load-config``), bit-exact resume, evaluation and gradient logging that leave the trajectory alone, the logged gradient norms
against torch, flag parsing, the non-finite stop, and a 2-rank run.

Scene and model: the ``make_scene`` recipe of tests/test_hip_distortion.py (24 x 32 frames of 8 bands), 3 classes, ``pred_specular``, 1024
rays per batch, ``background_color black``; a 2^14-slot hash table keeps the checkpoints at 6 MB.  Every child process has its own
timeout; a child that fails ends the test."""
import json
import math
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

import stats_f64 as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "unsupervised-hyperspectral-nerf_amd")
ENV = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, ROOT]))
MODEL = ["--pipeline.num_classes", "3", "--pipeline.model.method", "rgb+spectral", "--pipeline.model.pred-specular", "True",
         "--pipeline.model.temperature", "0.4", "--pipeline.model.background-color", "black", "--pipeline.model.log2_hashmap_size", "14",
         "--pipeline.datamanager.train-num-rays-per-batch", "1024", "--pipeline.datamanager.eval-num-rays-per-batch", "256",
         "--machine.seed", "7", "--vis", "none"]
NO_EVAL = ["--steps-per-eval-batch", "0", "--steps-per-eval-image", "0", "--steps-per-eval-all-images", "0"]


def _child(module, args, timeout=240):
    r = subprocess.run([sys.executable, "-m", module, *map(str, args)], env=ENV, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, f"{module} {args}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    return r


def _train(root, name, steps, extra=(), timeout=240):
    """One child run -> its run directory ``root/name/umhsnerf/t``."""
    _child("umhsnerf.train", ["--data", root / "scene", "--output-dir", root, "--experiment-name", name, "--timestamp", "t",
                              "--max-num-iterations", steps, *MODEL, *extra], timeout)
    return root / name / "umhsnerf" / "t"


def _tensors(obj, prefix=""):
    if torch.is_tensor(obj):
        yield prefix, obj
    elif isinstance(obj, dict):
        for k, v in obj.items():
            yield from _tensors(v, f"{prefix}/{k}")
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            yield from _tensors(v, f"{prefix}/{i}")


def _same_bits(a, b, keys=("pipeline", "optimizers")):
    for key in keys:
        ta, tb = dict(_tensors(a[key])), dict(_tensors(b[key]))
        assert ta.keys() == tb.keys() and len(ta) >= 2, key
        for k in ta:
            assert ta[k].dtype == tb[k].dtype and ta[k].shape == tb[k].shape, (key, k)
            assert torch.equal(ta[k].cpu().contiguous().view(torch.uint8), tb[k].cpu().contiguous().view(torch.uint8)), (key, k)
    if "optimizers" in keys:
        sa, sb = a["optimizers"]["fields"]["state"], b["optimizers"]["fields"]["state"]
        assert [s["step"] for s in sa.values()] == [s["step"] for s in sb.values()]


def _load(run, step):
    return torch.load(run / "nerfstudio_models" / f"step-{step:09d}.ckpt", map_location="cpu", weights_only=False)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """The scene and the reference run: 6 steps in one child, a save every 3, prefetch on as usual, evaluation only after the last step."""
    from test_hip_distortion import make_scene

    root = tmp_path_factory.mktemp("train")
    make_scene(root / "scene", B=8)
    run = _train(root, "six", 6, ["--steps-per-save", "3"])
    return dict(root=root, run=run, six=_load(run, 6))


def test_a_run_leaves_config_checkpoints_and_log_and_eval_reads_its_config(world):
    run = world["run"]
    cfg = json.loads((run / "config.json").read_text())
    assert cfg["pipeline"]["model"]["pred_specular"] is True and cfg["pipeline"]["num_classes"] == 3 and cfg["max_num_iterations"] == 6
    assert cfg["derived"]["wavelengths"] == [420.0 + 30 * k for k in range(8)] and cfg["derived"]["num_classes"] == 3
    assert Path(cfg["data"]) == world["root"] / "scene" and cfg["pipeline"]["datamanager"]["train_num_rays_per_batch"] == 1024
    assert sorted(p.name for p in (run / "nerfstudio_models").iterdir()) == ["step-000000003.ckpt", "step-000000006.ckpt"]
    ck = world["six"]
    assert ck["step"] == 6 and set(ck) == {"step", "pipeline", "optimizers", "schedulers", "scalers", "umhs_trainer"}
    assert ck["schedulers"] == {} and ck["scalers"] is None and len(ck["umhs_trainer"]["ranks"]) == 1
    assert set(ck["umhs_trainer"]["ranks"][0]) == {"device_rng", "cpu_rng", "datamanager"}
    assert ck["umhs_trainer"]["ranks"][0]["datamanager"]["train_count"] == 6
    assert [s["step"] for s in ck["optimizers"]["fields"]["state"].values()] == [6]
    assert ck["optimizers"]["fields"]["param_groups"][0]["max_steps"] == 6
    rows = [json.loads(line) for line in (run / "log.jsonl").read_text().splitlines()]
    assert rows[0]["event"] == "config" and rows[0]["config"] == cfg
    assert rows[-1]["event"] == "done" and rows[-1]["step"] == 6 and len(rows[-1]["checkpoints"]) == 2
    logged = [r for r in rows if "Train Loss" in r]
    assert [r["step"] for r in logged] == [0] and math.isfinite(logged[0]["Train Loss"]) and logged[0]["learning_rate/fields"] == pytest.approx(2e-2, rel=1e-12)
    assert {"Train Loss Dict/spectral_loss", "Train Loss Dict/rgb_loss", "Train Metrics Dict/psnr", "Train Metrics Dict/psnr_spectral",
            "Train Metrics Dict/num_samples_per_batch"} <= set(logged[0])
    final_eval = [r for r in rows if r.get("event") == "eval"]
    assert len(final_eval) == 1 and final_eval[0]["step"] == 6
    assert math.isfinite(final_eval[0]["Eval Images Metrics Dict (all images)/psnr"])
    # eval reads the run: scene, model flags (3 classes, specular, the small table) and the latest checkpoint come from config.json
    out = _child("umhsnerf.eval", ["--load-config", run / "config.json"]).stdout.strip().splitlines()[-1]
    metrics = json.loads(out)
    assert {"psnr", "psnr_spectral"} <= set(metrics) and all(math.isfinite(v) for v in metrics.values())
    assert metrics["psnr"] == pytest.approx(final_eval[0]["Eval Images Metrics Dict (all images)/psnr"], rel=1e-4)


def test_resume_is_bit_exact(world):
    root = world["root"]
    first = _train(root, "three", 3, ["--optimizers.fields.scheduler.max-steps", "6"])  # (the learning-rate schedule of the 6-step run)
    assert [p.name for p in (first / "nerfstudio_models").iterdir()] == ["step-000000003.ckpt"]
    _same_bits(_load(first, 3), _load(world["run"], 3))  # (the single run saved at 3 too, with prefetch held back for that step only)
    second = _train(root, "three-more", 6, ["--load-dir", first / "nerfstudio_models"])
    assert [p.name for p in (second / "nerfstudio_models").iterdir()] == ["step-000000006.ckpt"]
    resumed = _load(second, 6)
    _same_bits(resumed, world["six"])
    a, b = resumed["umhs_trainer"]["ranks"][0], world["six"]["umhs_trainer"]["ranks"][0]
    assert torch.equal(a["device_rng"], b["device_rng"]) and torch.equal(a["datamanager"]["generator"], b["datamanager"]["generator"])
    rows = [json.loads(line) for line in (second / "log.jsonl").read_text().splitlines()]
    assert rows[0]["start_step"] == 3 and rows[-1]["event"] == "done"


def test_evaluation_between_steps_does_not_move_the_trajectory(world):
    run = _train(world["root"], "with-eval", 6, ["--steps-per-eval-batch", "2", "--steps-per-eval-image", "2", "--steps-per-save", "3"])
    _same_bits(_load(run, 6), world["six"])
    rows = [json.loads(line) for line in (run / "log.jsonl").read_text().splitlines()]
    evals = [r for r in rows if r.get("event") == "eval"]
    assert [r["step"] for r in evals] == [2, 4, 6]
    assert all(math.isfinite(r["Eval Loss Dict/spectral_loss"]) and math.isfinite(r["Eval Images Metrics/psnr"]) for r in evals)
    off = _train(world["root"], "no-eval", 6, NO_EVAL)
    _same_bits(_load(off, 6), world["six"])


def _trainer(world, extra=()):
    from umhsnerf.train import Trainer, parse_flags

    return Trainer(parse_flags(["--data", str(world["root"] / "scene"), "--output-dir", str(world["root"]), "--experiment-name", "in-process",
                                "--max-num-iterations", "6", *MODEL, *NO_EVAL, *extra]))


def test_gradient_logging_leaves_the_trajectory_alone_and_matches_torch(world):
    trainer = _trainer(world, ["--log-gradients", "True", "--logging-steps", "2"])
    layout, flat = trainer.field.layout, trainer.field.flat
    checked = False
    for step in range(6):
        _, loss_dict, metrics = trainer.train_step(step)
        if step == 2:
            trainer.flush_logs(wait=True)
            row, grad = trainer.last_row, flat.grad.detach().clone()
            assert row["step"] == 2 and row["Gradients/non_finite"] == 0
            total, largest = 0.0, 0.0
            for name in layout.entries:
                view = layout.view(grad, name)
                want, got = float(view.double().norm()), row[f"Gradients/field.{name}"]
                n = view.numel()
                # sqrt halves the relative error of the sums (the kernel's chain; torch's float64 sum, at worst one chain of n), and
                # each side rounds its square root once
                bound = (0.5 * (S.gamma(S.chain_length(n)) + S.gamma(n)) + 3 * S.U) * want
                print(f"{name}: |logged - torch| = {abs(got - want):.3e}, bound {bound:.3e}, norm {want:.3e}")
                assert abs(got - want) <= bound, (name, got, want, bound)
                total, largest = total + got, max(largest, float(view.abs().max()))
            assert row["Gradients/Total"] == total and row["Gradients/max_abs"] == largest and total > 0
            assert sum(k.startswith("Gradients/field.") for k in row) == len(layout.entries)
            checked = True
    assert checked
    trainer.flush_logs(wait=True)
    torch.cuda.synchronize()
    here = {"pipeline": trainer.pipeline.state_dict(), "optimizers": {"fields": trainer.optimizer.state_dict()}}
    _same_bits(here, world["six"])  # logged at steps 0, 2, 4 with the fused Adam arm withheld: the same bits as the plain run
    # a non-finite gradient value, set by hand in front of the logging call: the row is written, then the run ends
    with torch.no_grad():
        flat.grad[layout.offset("endmembers") + 1] = float("nan")
    with pytest.raises(FloatingPointError, match=r"step 6: 1 non-finite gradient value\(s\) in field\.endmembers"):
        trainer.log_step(6, loss_dict, metrics, wait=True)
    assert trainer.last_row["step"] == 6 and trainer.last_row["Gradients/non_finite"] == 1
    with torch.no_grad():
        flat.grad[layout.offset("endmembers") + 1] = 0.0
        keep = flat.data[5].clone()
        flat.data[5] = float("inf")
    with pytest.raises(FloatingPointError, match=r"non-finite parameter value\(s\) in field\.mlp_base\.encoder\.hash_table"):
        trainer.log_step(7, loss_dict, metrics, wait=True)
    with torch.no_grad():
        flat.data[5] = keep


def test_the_reference_scripts_flags_parse_into_the_right_fields(world):
    from umhsnerf.train import Trainer, parse_flags

    argv = ["umhsnerf", "--steps_per_save", "1000", "--save-only-latest-checkpoint", "False", "--machine.seed", "42", "--machine.num-devices", "4",
            "--log-gradients", "True", "--log_gradients", "True", "--gradient-accumulation_steps", "3", "--pipeline.num_classes", "6",
            "--pipeline.num-classes", "6", "--pipeline.model.far-plane", "1000", "--pipeline.model.near_plane", "0.05",
            "--pipeline.model.background-color", "last_sample", "--pipeline.model.spectral_loss_weight", "5.0",
            "--pipeline.model.temperature", "0.4", "--pipeline.model.pred_dino", "False", "--pipeline.model.pred-specular", "True",
            "--pipeline.model.load_vca", "True", "--pipeline.model.implementation", "tcnn", "--pipeline.datamanager.images-on-gpu", "False",
            "--pipeline.datamanager.patch-size", "1", "--pipeline.datamanager.train-num-rays-per-batch", "4096",
            "--pipeline.datamanager.eval_num_rays_per_batch", "256", "--pipeline.model.method", "rgb+spectral", "--data", "data/processed/hotdog",
            "--experiment-name", "hotdog t0.4 k6", "--max-num-iterations", "100000", "--vis", "viewer+wandb", "--viewer.websocket-port", "7007",
            "--viewer.max-num-display-images", "1", "--pipeline.datamanager.dataparser.eval-mode", "interval", "--load-step", "2000",
            "--pipeline.model.grid_resolution", "64", "--pipeline.datamanager.dataparser.downscale-factor", "2"]
    c = parse_flags(argv)
    m, dm = c.pipeline.model, c.pipeline.datamanager
    assert (c.steps_per_save, c.save_only_latest_checkpoint, c.machine.seed, c.machine.num_devices) == (1000, False, 42, 4)
    assert c.log_gradients is True and c.gradient_accumulation_steps == 3 == c.pipeline.gradient_accumulation_steps
    assert c.pipeline.num_classes == 6 and (m.far_plane, m.near_plane, m.background_color) == (1000.0, 0.05, "last_sample")
    assert (m.spectral_loss_weight, m.temperature, m.pred_dino, m.pred_specular, m.load_vca, m.method) == (5.0, 0.4, False, True, True, "rgb+spectral")
    assert m.implementation == "torch" and m.grid_resolution == 64  # --pipeline.model.implementation is accepted and ignored
    assert (dm.images_on_gpu, dm.patch_size, dm.train_num_rays_per_batch, dm.eval_num_rays_per_batch) == (False, 1, 4096, 256)
    assert dm.dataparser.data == Path("data/processed/hotdog") == c.data and dm.dataparser.eval_mode == "interval" and dm.dataparser.downscale_factor == 2
    assert (c.experiment_name, c.max_num_iterations, c.vis, c.load_step) == ("hotdog t0.4 k6", 100000, "viewer+wandb", 2000)
    assert c.viewer == {"websocket_port": "7007", "max_num_display_images": "1"}
    d = parse_flags([])  # defaults
    assert (d.output_dir, d.max_num_iterations, d.steps_per_save, d.save_only_latest_checkpoint) == (Path("outputs"), 30000, 2000, False)
    assert (d.steps_per_eval_batch, d.steps_per_eval_image, d.steps_per_eval_all_images, d.logging_steps, d.log_gradients) == (500, 500, 25000, 10, False)
    assert d.pipeline.datamanager.train_num_rays_per_batch == 9216 * 4 and d.pipeline.model.eval_num_rays_per_chunk == 512
    for bad in (["--pipeline.model.no-such-field", "1"], ["--pipeline.model.method", "cmyk"], ["--max-num-iterations", "many"], ["stray"]):
        with pytest.raises(SystemExit):
            parse_flags(bad)
    # settings the package refuses keep raising their own errors
    scene = ["--data", str(world["root"] / "scene"), *MODEL]
    with pytest.raises(NotImplementedError, match="pred_dino"):
        Trainer(parse_flags([*scene, "--pipeline.model.pred_dino", "True"]))
    with pytest.raises(NotImplementedError, match="patch_size"):
        Trainer(parse_flags([*scene, "--pipeline.datamanager.patch-size", "2"]))
    with pytest.raises(NotImplementedError, match="use_appearance_embedding"):
        Trainer(parse_flags([*scene, "--pipeline.model.use-appearance-embedding", "False"]))


def test_save_only_latest_checkpoint_removes_the_older_files(world):
    run = _train(world["root"], "latest", 6, ["--steps-per-save", "2", "--save-only-latest-checkpoint", "True", *NO_EVAL])
    assert [p.name for p in (run / "nerfstudio_models").iterdir()] == ["step-000000006.ckpt"]
    _same_bits(_load(run, 6), world["six"])


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs")
def test_two_ranks_write_one_reproducible_checkpoint(world):
    runs = [_train(world["root"], f"two-ranks-{i}", 4, ["--machine.num-devices", "2", *NO_EVAL], timeout=300) for i in range(2)]
    for run in runs:
        assert [p.name for p in (run / "nerfstudio_models").iterdir()] == ["step-000000004.ckpt"]
    a, b = (_load(run, 4) for run in runs)
    assert len(a["umhs_trainer"]["ranks"]) == 2 and a["umhs_trainer"]["world_size"] == 2
    assert not torch.equal(a["umhs_trainer"]["ranks"][0]["datamanager"]["generator"], a["umhs_trainer"]["ranks"][1]["datamanager"]["generator"])
    _same_bits(a, b, keys=("pipeline",))
