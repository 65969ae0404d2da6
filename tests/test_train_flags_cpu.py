"""CPU checks of the stand-alone trainer's command line (``umhsnerf.train.parse_flags``: flags generated from the config dataclasses) and
of ``--load-config`` for the commands that read a checkpoint (no GPU: nothing is built or loaded)."""
import dataclasses
import json
from pathlib import Path

import pytest


def test_every_config_field_is_a_flag_and_both_spellings_parse():
    from umhsnerf.data.umhs_datamanager import UMHSDataManagerConfig
    from umhsnerf.data.umhs_dataparser import UMHSDataParserConfig
    from umhsnerf.train import TrainerConfig, flag_table, parse_flags
    from umhsnerf.umhs_model import UMHSConfig
    from umhsnerf.umhs_pipeline import UMHSPipelineConfig

    table = flag_table(TrainerConfig())
    for prefix, cls in (("pipeline.", UMHSPipelineConfig), ("pipeline.model.", UMHSConfig), ("pipeline.datamanager.", UMHSDataManagerConfig),
                        ("pipeline.datamanager.dataparser.", UMHSDataParserConfig)):
        for f in dataclasses.fields(cls):
            if not f.name.startswith("_") and f.name not in ("datamanager", "model", "dataparser"):
                assert prefix + f.name in table, prefix + f.name
    a = parse_flags(["--pipeline.model.near_plane", "0.1", "--pipeline.datamanager.train_num_rays_per_batch", "2048", "--steps_per_save", "7"])
    b = parse_flags(["--pipeline.model.near-plane=0.1", "--pipeline.datamanager.train-num-rays-per-batch", "2048", "--steps-per-save", "7"])
    for c in (a, b):
        assert (c.pipeline.model.near_plane, c.pipeline.datamanager.train_num_rays_per_batch, c.steps_per_save) == (0.1, 2048, 7)
    c = parse_flags(["--log-gradients", "--pipeline.model.render-step-size", "0.01", "--pipeline.model.collider-params", "None",
                     "--pipeline.datamanager.dataparser.mask-color", "(1.0, 0.0, 0.0)", "--pipeline.model.implementation", "tcnn",
                     "--viewer.websocket-port", "7007", "--vis", "viewer+wandb", "--pipeline.model.pred_dino", "False"])
    assert c.log_gradients is True and c.pipeline.model.render_step_size == 0.01 and c.pipeline.model.collider_params is None
    assert c.pipeline.datamanager.dataparser.mask_color == (1.0, 0.0, 0.0) and c.pipeline.model.implementation == "torch"
    assert c.viewer == {"websocket_port": "7007"} and c.vis == "viewer+wandb" and c.pipeline.model.pred_dino is False
    for bad in (["--pipeline.model.temperature"], ["--no-such-flag", "1"], ["--pipeline.model.background-color", "green"], ["--log-gradients", "maybe"]):
        with pytest.raises(SystemExit):
            parse_flags(bad)


def test_vis_backends_outside_the_package_are_named_once():
    from umhsnerf.train import _vis_notice

    assert _vis_notice("none") is None
    assert "viewer, wandb" in _vis_notice("viewer+wandb") and "log.jsonl" in _vis_notice("tensorboard")


def _fake_run(tmp_path, **model):
    from umhsnerf.train import config_to_dict, parse_flags

    run = tmp_path / "exp" / "umhsnerf" / "t"
    (run / "nerfstudio_models").mkdir(parents=True)
    for step in (2000, 10000, 4000):
        (run / "nerfstudio_models" / f"step-{step:09d}.ckpt").write_bytes(b"")
    c = parse_flags(["--data", "scenes/hotdog", "--pipeline.num-classes", "6", "--pipeline.model.method", "rgb+spectral",
                     "--pipeline.model.pred-specular", "True", "--pipeline.model.temperature", "0.4", "--pipeline.model.log2-hashmap-size", "17",
                     "--pipeline.datamanager.images-on-gpu", "False", "--pipeline.datamanager.dataparser.eval-mode", "interval"])
    d = config_to_dict(c)
    json.dumps(d)  # every value is a JSON value
    (run / "config.json").write_text(json.dumps(d))
    return run


def test_load_config_supplies_scene_model_flags_and_latest_checkpoint(tmp_path, capsys):
    import argparse

    from umhsnerf import eval as E, export, render

    run = _fake_run(tmp_path)
    ap = argparse.ArgumentParser()
    E.add_model_arguments(ap)
    a = ap.parse_args(["--load-config", str(run / "config.json")])
    assert a.data == "scenes/hotdog" and a.checkpoint == str(run / "nerfstudio_models" / "step-000010000.ckpt")
    assert (a.method, a.num_classes, a.pred_specular, a.temperature, a.log2_hashmap_size) == ("rgb+spectral", 6, True, 0.4, 17)
    assert (a.eval_mode, a.images_on_gpu, a.background_color, a.seg_ignore_label) == ("interval", False, "random", 255)
    # explicit flags override the file, on either side of --load-config
    ap = argparse.ArgumentParser()
    E.add_model_arguments(ap)
    a = ap.parse_args(["--temperature", "0.7", "--load-config", str(run / "config.json"), "--checkpoint", "other.ckpt", "--num-classes", "4"])
    assert (a.temperature, a.checkpoint, a.num_classes, a.data, a.log2_hashmap_size) == (0.7, "other.ckpt", 4, "scenes/hotdog", 17)
    # the subcommands of render and export take it too
    r = render.parse_args(["dataset", "--load-config", str(run / "config.json"), "--output-path", "out"])
    assert r.data == "scenes/hotdog" and r.num_classes == 6 and r.checkpoint.endswith("step-000010000.ckpt")
    x = export.parse_args(["pointcloud", "--load-config", str(run / "config.json"), "--output-dir", "out", "--num-classes", "5"])
    assert x.data == "scenes/hotdog" and x.num_classes == 5 and x.pred_specular is True
    # without the flag nothing changes: --data and --checkpoint stay required, and the namespace has no new key
    ap = argparse.ArgumentParser()
    E.add_model_arguments(ap)
    with pytest.raises(SystemExit):
        ap.parse_args(["--checkpoint", "step.ckpt"])
    assert "--data" in capsys.readouterr().err
    plain = ap.parse_args(["--data", "s", "--checkpoint", "c"])
    assert "load_config" not in vars(plain) and plain.num_classes == 5 and plain.pred_specular is False
    # a run directory without checkpoints, or a missing file, is an argument error
    empty = tmp_path / "empty"
    empty.mkdir()
    (empty / "config.json").write_text((run / "config.json").read_text())
    for bad in (empty / "config.json", tmp_path / "nowhere.json"):
        ap = argparse.ArgumentParser()
        E.add_model_arguments(ap)
        with pytest.raises(SystemExit):
            ap.parse_args(["--load-config", str(bad)])
        assert "--load-config" in capsys.readouterr().err
