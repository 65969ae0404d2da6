"""CPU checks of umhsnerf/materials.py (the edit model and its file format) and of the --material-edits flag of the command lines."""
import json
import math

import numpy as np
import pytest
import torch

from umhsnerf.materials import MaterialEdits, load_material_edits

C, B = 4, 5
SPEC = [0.1, 0.2, 0.3, 0.4, 0.5]


def _load(d, pred_specular=True):
    return load_material_edits(d, C, B, pred_specular)


def test_the_documented_file_loads(tmp_path):
    np.save(tmp_path / "pigment.npy", np.asarray(SPEC, dtype=np.float32)[::-1].copy())
    doc = {"materials": [{"material": 2, "spectrum": SPEC}, {"material": 0, "from_material": 1, "gain": 0.5},
                         {"material": 1, "density": 0.0}, {"material": 3, "spectrum_file": "pigment.npy"}], "specular_gain": 1.0}
    (tmp_path / "edits.json").write_text(json.dumps(doc))
    e = load_material_edits(tmp_path / "edits.json", C, B, True)  # spectrum_file is relative to the JSON, not to the working directory
    assert isinstance(e, MaterialEdits) and (e.n_classes, e.n_bands, e.pred_specular) == (C, B, True)
    assert e.gains == (0.5, 1.0, 1.0, 1.0) and e.densities == (1.0, 0.0, 1.0, 1.0) and e.specular_gain == 1.0
    assert e.edits_density and e.edits_dictionary and not e.is_identity
    assert e.spectra[0] == 1 and e.spectra[1] is None and e.spectra[2] == tuple(SPEC)
    assert e.spectra[3] == tuple(float(v) for v in np.asarray(SPEC, dtype=np.float32)[::-1])
    assert load_material_edits(str(tmp_path / "edits.json"), C, B, True) == e
    with pytest.raises(Exception):  # immutable
        e.gains = (1.0,) * C
    with pytest.raises(ValueError, match=r"entry 3 \(material 3\).*cannot read spectrum_file"):
        _load(doc)  # the dict form resolves against the working directory, where there is no pigment.npy


def test_identity_files():
    for doc in ({}, {"materials": []}, {"materials": [{"material": 1}], "specular_gain": 1.0},
                {"materials": [{"material": 0, "gain": 1.0, "density": 1}]}):
        e = _load(doc)
        assert e.is_identity and not e.edits_density and not e.edits_dictionary
    assert MaterialEdits.identity(C, B, False).is_identity
    assert not _load({"materials": [{"material": 0, "from_material": 0}]}).is_identity  # a spectrum was named: not judged by value
    assert _load({"materials": [{"material": 0, "density": 0.5}]}).edits_density
    assert not _load({"specular_gain": 0.5}).is_identity


@pytest.mark.parametrize("doc,words", [
    ({"material": []}, "unknown keys ['material'] in the file"),
    ({"materials": [{"material": 0, "colour": 1}]}, "entry 0: unknown keys ['colour']"),
    ({"materials": [{"material": 1}, {"material": 4}]}, "entry 1: material 4 is outside 0..3"),
    ({"materials": [{"material": -1}]}, "entry 0: material -1 is outside 0..3"),
    ({"materials": [{"gain": 2.0}]}, "entry 0: material None is outside 0..3"),
    ({"materials": [{"material": 2, "gain": 2.0}, {"material": 2}]}, "entry 1 (material 2): material 2 is listed twice"),
    ({"materials": [{"material": 2, "spectrum": SPEC[:4]}]}, "entry 0 (material 2): the spectrum has 4 values, the model has 5 bands"),
    ({"materials": [{"material": 2, "spectrum": SPEC[:4] + [float("nan")]}]}, "entry 0 (material 2): the spectrum holds a non-finite value"),
    ({"materials": [{"material": 2, "spectrum": SPEC[:4] + [float("inf")]}]}, "non-finite value"),
    ({"materials": [{"material": 2, "spectrum": SPEC, "from_material": 1}]}, "entry 0 (material 2): spectrum and from_material exclude each other"),
    ({"materials": [{"material": 2, "from_material": 1, "spectrum_file": "x.npy"}]}, "from_material and spectrum_file exclude each other"),
    ({"materials": [{"material": 2, "from_material": 7}]}, "entry 0 (material 2): from_material 7 is outside 0..3"),
    ({"materials": [{"material": 0}, {"material": 2, "gain": -0.5}]}, "entry 1 (material 2): gain -0.5 must be a finite number >= 0"),
    ({"materials": [{"material": 2, "gain": float("inf")}]}, "gain inf must be a finite number >= 0"),
    ({"materials": [{"material": 2, "density": -1}]}, "entry 0 (material 2): density -1 must be a finite number >= 0"),
    ({"materials": [{"material": 2, "density": float("nan")}]}, "density nan must be a finite number >= 0"),
    ({"specular_gain": -1.0}, "specular_gain -1.0 must be a finite number >= 0"),
    ({"specular_gain": float("nan")}, "specular_gain nan must be a finite number >= 0"),
])
def test_refusals_name_the_entry_and_the_reason(doc, words):
    with pytest.raises(ValueError) as e:
        _load(doc)
    assert words in str(e.value), str(e.value)


def test_specular_gain_needs_the_specular_head():
    assert _load({"specular_gain": 0.5}, pred_specular=True).specular_gain == 0.5
    assert _load({"specular_gain": 1.0}, pred_specular=False).is_identity
    with pytest.raises(ValueError, match="specular_gain 0.5 needs a model with the specular head"):
        _load({"specular_gain": 0.5}, pred_specular=False)


def test_spectrum_file_refusals(tmp_path):
    np.save(tmp_path / "two_d.npy", np.zeros((1, B), dtype=np.float32))
    np.save(tmp_path / "ints.npy", np.zeros(B, dtype=np.int64))
    np.save(tmp_path / "short.npy", np.zeros(B - 1, dtype=np.float64))
    for name, words in (("two_d.npy", "1-D float array"), ("ints.npy", "1-D float array"), ("short.npy", "has 4 values"),
                        ("missing.npy", "cannot read spectrum_file")):
        (tmp_path / "e.json").write_text(json.dumps({"materials": [{"material": 1, "spectrum_file": name}]}))
        with pytest.raises(ValueError, match=words):
            load_material_edits(tmp_path / "e.json", C, B, False)
    (tmp_path / "bad.json").write_text("{not json")
    with pytest.raises(ValueError, match="is not JSON"):
        load_material_edits(tmp_path / "bad.json", C, B, False)


def test_dictionary_is_one_float32_product_per_element_and_from_material_copies_the_unedited_row():
    g = torch.Generator().manual_seed(3)
    E = torch.rand(C, B, generator=g)
    spec = [0.1 * (i + 1) + 1e-3 for i in range(B)]
    e = _load({"materials": [{"material": 0, "from_material": 1, "gain": 0.3}, {"material": 1, "spectrum": spec, "gain": 1.7},
                             {"material": 3, "gain": 0.0}]})
    got = e.dictionary(E)
    assert got.dtype == torch.float32 and got.shape == (C, B) and got.is_contiguous() and got.device == E.device
    Ep = E.double().clone()
    Ep[0] = E[1].double()  # the UNEDITED row 1, although row 1 is itself replaced
    Ep[1] = torch.tensor(spec, dtype=torch.float32).double()
    gains = torch.tensor([0.3, 1.7, 1.0, 0.0], dtype=torch.float32).double()
    want = (gains[:, None] * Ep).float()  # float64 product of float32 factors, rounded once: the float32 product
    assert torch.equal(got, want)
    assert torch.equal(got[2], E[2]) and bool((got[3] == 0).all())
    assert torch.equal(MaterialEdits.identity(C, B, True).dictionary(E), E)
    assert torch.equal(e.density_gain("cpu"), torch.ones(C))
    with pytest.raises(ValueError, match=r"built for a \[4,5\] dictionary"):
        e.dictionary(torch.rand(C, B + 1))
    assert not math.isnan(float(got.sum()))


def test_the_flag_parses_on_all_five_subcommands():
    from umhsnerf import export, render

    base = ["--data", "scene", "--checkpoint", "step.ckpt"]
    for sub, extra in (("camera-path", ["--camera-path-filename", "p.json"]), ("dataset", []), ("interpolate", [])):
        common = [sub, *base, "--output-path", "out", *extra]
        assert render.parse_args(common).material_edits is None
        assert render.parse_args([*common, "--material-edits", "edits.json"]).material_edits == "edits.json"
    for sub in ("pointcloud", "tsdf"):
        common = [sub, *base, "--output-dir", "out"]
        assert getattr(export.parse_args(common), "material_edits", None) is None
        assert export.parse_args([*common, "--material-edits", "edits.json"]).material_edits == "edits.json"
