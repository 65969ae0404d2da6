"""The field-variant comparators (tests/field_f64.py) have the power to see the bugs they are there for: fed the float32 oracle's own
results in place of the kernels', they pass them; with a planted fault they reject every cell the fault applies to.

Faults: (1) the last sample of a ragged tail tile missing from the outputs and from dW; (2) band B-1 of a partial band tile replaced by
band B-2, or its d_spectral column ignored; (3) endmember C-1 missing from the mixing; (4) every dW entry scaled by 1 - 2^-17 (a
truncating bf16 split: the slope check at the large-n cell must see it); (5) the directional head's gradient zeroed with the specular
head on.  Cells: a plain backward, a folded backward (compositing backward in the loss), the two-launch forward's per-ray sums, and a
plain backward at 16,385 samples (past 256 workgroups x 64 samples, the size of the GPU table's large rows)."""
import copy

import pytest
import torch

import field_f64 as F

CELLS = {
    "plain_C4_B17_spec_n37": dict(C=4, B=17, spec=True, temp=0.7, n=37, kind="plain"),
    "folded_C3_B40_spec_n100": dict(C=3, B=40, spec=True, temp=1.5, n=100, kind="composited"),
    "rays_C9_B31_spec_n90": dict(C=9, B=31, spec=True, temp=0.4, n=90, kind="rays"),
    "plain_C2_B5_nospec_n16385": dict(C=2, B=5, spec=False, temp=0.8, n=16385, kind="plain", large=True),
}
_cache = {}


def _cell(name):
    if name not in _cache:
        torch.set_num_threads(max(1, min(torch.get_num_threads(), 16)))
        c = CELLS[name]
        case = F.make_case(c["C"], c["B"], c["spec"], c["temp"], c["n"], seed=11)
        d = {"case": case}
        d["p32"], d["p64"] = F.oracle_pair(case, "plain")
        if c["kind"] == "composited":
            d["b32"], d["b64"] = F.oracle_pair(case, "composited", grad_scaling=True)
        else:
            d["b32"], d["b64"] = d["p32"], d["p64"]
        if c["kind"] == "rays":
            d["w32"] = F.T.render_weight_from_density(case.t0, case.t1, d["p32"]["out"]["sigma"], case.packed_info())[0]
        _cache[name] = d
    return CELLS[name], _cache[name]


def _oracle32(name, p=None, **kw):
    """The float32 oracle of a cell again, with a fault planted through its inputs."""
    c, d = _cell(name)
    case = d["case"]
    p = case.p if p is None else p
    if c["kind"] == "composited":
        return F.oracle_composited(p, case, torch.float32, grad_scaling=True, **kw)
    return F.oracle_plain(p, case, torch.float32, **kw)


def _judge_fwd(name, out32=None, drop_last=False):
    """The forward comparators of a cell (per-sample outputs; in the "rays" cell also the per-ray sums) with the "kernel" outputs given
    (default: the clean float32 oracle)."""
    c, d = _cell(name)
    case = d["case"]
    out32 = d["p32"]["out"] if out32 is None else out32
    fails = F.check_forward(out32, d["p64"]["out"], F.fwd_keys(case.spec))
    if c["kind"] == "rays":
        w = d["w32"].clone()
        if drop_last:
            w[-1] = 0
        got = F.oracle_per_ray(case, out32, weights=w)
        fails += F.check_forward(got, F.oracle_per_ray(case, d["p64"]["out"], weights=d["w32"].double()), list(got), prefix="rays.")
    return fails


def _judge_bwd(name, back32=None):
    c, d = _cell(name)
    back32 = d["b32"] if back32 is None else back32
    return F.check_backward(back32, d["b32"], d["b64"], large=c.get("large", False))


@pytest.mark.parametrize("name", list(CELLS))
def test_the_float32_oracle_passes_its_own_comparators(name):
    c, d = _cell(name)
    assert not _judge_fwd(name)
    if c["kind"] != "rays":
        assert not _judge_bwd(name)
    assert d["case"].extra["inert"] <= max(2, 0.03 * d["case"].n)


def _fault_cases():
    out = []
    for name, c in CELLS.items():
        fs = ["last_sample", "endmember"]
        if c["B"] % 16 and c["B"] >= 2:
            fs.append("band")
        if c.get("large"):
            fs.append("dw_scaled")
        if c["spec"] and c["kind"] != "rays":
            fs.append("directional")
        out += [pytest.param(name, f, id=f"{name}-{f}") for f in fs]
    return out


@pytest.mark.parametrize("name,fault", _fault_cases())
def test_a_planted_fault_is_rejected(name, fault):
    """Each half of a fault on its own: the faulted forward outputs are rejected by the forward comparators, the faulted gradients by
    the backward comparators (no cell where one half would pass on the other's strength)."""
    c, d = _cell(name)
    case = d["case"]
    B, C = case.B, case.C
    clean = d["p32"]["out"]
    bwd = c["kind"] != "rays"
    if fault == "last_sample":
        out = {k: v.clone() for k, v in clean.items()}
        for v in out.values():
            v[-1] = 0
        assert _judge_fwd(name, out, drop_last=True), "outputs without the last sample passed"
        if bwd:
            assert _judge_bwd(name, _oracle32(name, drop_last=True)), "dW without the last sample passed"
    elif fault == "band":
        out = {k: v.clone() for k, v in clean.items()}
        for k in ("spectral", "spectral2", "specular"):
            if k in out:
                out[k][:, B - 1] = out[k][:, B - 2]
        assert _judge_fwd(name, out), "band B-1 = band B-2 passed"
        if bwd:
            assert _judge_bwd(name, _oracle32(name, zero_band=B - 1)), "the ignored d_spectral column of band B-1 passed"
    elif fault == "endmember":
        p = copy.deepcopy(case.p)
        with torch.no_grad():
            p.endmembers[C - 1] = 0
        assert _judge_fwd(name, F.oracle_plain(p, case, torch.float32, with_grads=False)["out"]), "mixing without endmember C-1 passed"
        if bwd:
            assert _judge_bwd(name, _oracle32(name, p=p)), "gradients without endmember C-1 passed"
    elif fault == "dw_scaled":
        back = copy.deepcopy(d["b32"])
        for k, g in back["grads"].items():
            if "_w." in k or k == "endmembers":
                g.mul_(1 - 2.0 ** -17)
        fails = _judge_bwd(name, back)
        assert any("slope" in m for m in fails), fails  # (the slope check sees it, whatever else does)
    elif fault == "directional":
        back = copy.deepcopy(d["b32"])
        for k, g in back["grads"].items():
            if k.startswith("dir_"):
                g.zero_()
        assert _judge_bwd(name, back), "a zeroed directional-head gradient passed"


@pytest.mark.parametrize("C,B,spec,n", [(4, 17, True, 37), (1, 40, False, 20), (9, 31, True, 5)])
def test_the_restated_field_outputs_are_the_oracles(C, B, spec, n):
    """field_f64.field_forward restates oracle/torch_ref.field_outputs only for its shapes at one sample or one band: elsewhere the same
    numbers, bit for bit."""
    case = F.make_case(C, B, spec, 0.6, n, seed=2)
    p = case.p
    mine = F.field_forward(p, case.enc, case.wpos, case.dirs, case.sel, case.temp)
    ref = F.T.field_outputs(p, case.wpos, case.dirs, torch.zeros(n, 1), torch.zeros(n, 1), mine["emb"], case.temp)
    for k in ("spectral", "abundances") + (("spectral2", "specular") if spec else ()):
        assert torch.equal(mine[k], ref[k].reshape(mine[k].shape)), k
