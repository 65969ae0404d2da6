"""The multiresolution hash grid (csrc/umhs_hash.h, umhs_hashgrid.hip, umhs_hashgrid_part.h: umhs_hashgrid_fwd / _fwd_count,
umhs_enc_gather, umhs_hashgrid_bwd in its atomic and its partitioned form, _bwd_prepare / _bwd_prepare_counted / _bwd_apply /
_bwd_apply_adam) against a float64 oracle: every element of the encoding, every slot of the table gradient.  Cases, oracle, rules and
the constants K are tests/hash_f64.py's (its docstring says which case reaches which path of the kernels);
tests/test_hash_f64_bounds_cpu.py shows that the comparators reject planted faults.

Every output buffer holds NaN, garbage or a known prior before the launch, so an element a kernel never writes -- or one it should
not have written -- fails.  Figures measured on the way go to hash_f64.json in HF.report_dir(): per case, path and level the worst
ratio (to be held against K), the teeth share and the number of elements whose bits differ from float32 (forward: from
torch_ref.hash_encode, asserted zero; backward: from the float32 / int64 model of the partitioned path, reported; the Adam step in
the reduce's epilogue: from the replay of tests/adam_f64.py, asserted zero, beside its float64 envelope ratios)."""
import json
import os

import pytest
import torch

import adam_f64 as AF
import hash_f64 as HF

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = {"forward": {}, "backward": {}, "fused adam": {}}
ADAM_BUFFERS = ("table", "exp_avg", "exp_avg_sq")
NAN = float("nan")
_fwd_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _write_report():
    yield
    summary = {"forward worst": 0.0, "forward not bit-equal": 0, "partitioned backward worst": 0.0, "atomic backward worst": 0.0,
               "backward not bit-equal to the model": 0, "teeth": {}, "fused adam worst": 0.0, "fused adam not bit-equal to the replay": 0}
    for r in REPORT["fused adam"].values():
        summary["fused adam worst"] = max(summary["fused adam worst"], r["p_worst"], r["m_worst"], r["v_worst"])
        summary["fused adam not bit-equal to the replay"] += r["p_bits_differ"] + r["m_bits_differ"] + r["v_bits_differ"]
    for case, variants in REPORT["forward"].items():
        for v in variants.values():
            summary["forward worst"] = max(summary["forward worst"], max(v["worst"]))
            summary["forward not bit-equal"] += sum(v["not_bit_equal"] or [])
    for case, paths in REPORT["backward"].items():
        for p, rep in paths.items():
            key = "atomic backward worst" if p.startswith("atomic") else "partitioned backward worst"
            summary[key] = max(summary[key], max(r["worst"] for r in rep))
            summary["backward not bit-equal to the model"] += sum(r.get("not_bit_equal", 0) for r in rep)
            if p == "onecall/overwrite":
                summary["teeth"][case] = HF.teeth_share(rep)
    with open(os.path.join(HF.report_dir(ROOT), "hash_f64.json"), "w") as f:
        json.dump({"K": {"forward": HF.K_F, "partitioned backward": HF.K_B, "atomic backward": HF.K_A}, "summary": summary, **REPORT}, f, indent=1)


def _mods():
    from umhsnerf import _hip, ops

    return ops, _hip


def _sc():
    return HF.T.hash_scalings().to(DEV)


# ------------------------------------------------------------------------------------------------------------------------------ #
# forward
# ------------------------------------------------------------------------------------------------------------------------------ #
def _fwd_case(name):
    if name not in _fwd_cache:
        kind, log2_T, n = HF.FWD_CASES[name]
        x, table = HF.positions(kind, n), HF.fwd_table(log2_T)
        geo = HF.geometry(x, HF.ALL_LEVELS, log2_T)
        r64, mag = HF.forward_oracle(geo, table)
        r32 = HF.T.hash_encode(x, table, HF.T.hash_scalings(), log2_T).view(-1, 16, 2)
        _fwd_cache[name] = (log2_T, x, table, r64, mag, r32)
    return _fwd_cache[name]


@pytest.mark.parametrize("name", list(HF.FWD_CASES))
def test_forward_every_element_against_float64_and_the_float32_bits(name):
    ops, _hip = _mods()
    log2_T, x, table, r64, mag, r32 = _fwd_case(name)
    n = x.shape[0]
    xd, td, sc = x.to(DEV), table.to(DEV), _sc()
    rep = REPORT["forward"].setdefault(name, {})
    fails = []
    full = lambda *s: torch.full(s, NAN, device=DEV, dtype=torch.float32)
    # level-major and row-major
    enc = ops.hashgrid_fwd(xd, td, sc, log2_T, True, out=full(16, n, 2))
    fails += HF.check_forward("level_major", enc.permute(1, 0, 2), r64, mag, r32, rep)
    enc = ops.hashgrid_fwd(xd, td, sc, log2_T, False, out=full(n, 32))
    fails += HF.check_forward("row_major", enc.view(n, 16, 2), r64, mag, r32, rep)
    # the forward that also takes the backward's histogram
    enc = ops.hashgrid_fwd_count(xd, td, sc, log2_T)
    assert enc is not None
    fails += HF.check_forward("fwd_count", enc.permute(1, 0, 2), r64, mag, r32, rep)
    # a row-major buffer with the odd row stride 33: the scalar store path of both kernels; column 32 keeps its bits
    lib = _hip.lib()
    buf = full(n, 33)
    _hip.check(lib.umhs_hashgrid_fwd(ops.ptr(xd), ops.ptr(td), ops.ptr(sc), n, 16, log2_T, ops.ptr(buf), 33, 2, _hip.stream()), "umhs_hashgrid_fwd")
    fails += HF.check_forward("stride33", buf[:, :32].reshape(n, 16, 2), r64, mag, r32, rep)
    assert bool(torch.isnan(buf[:, 32]).all())
    nbytes = lib.umhs_hashgrid_bwd_workspace_bytes(n, 16, log2_T)
    ws = ops._workspace(nbytes, xd.device, ops.WS_HASH_BWD)
    buf = full(n, 33)
    _hip.check(lib.umhs_hashgrid_fwd_count(ops.ptr(xd), ops.ptr(td), ops.ptr(sc), n, 16, log2_T, ops.ptr(buf), 33, 2, ops.ptr(ws), ws.numel(),
                                           _hip.stream()), "umhs_hashgrid_fwd_count")
    fails += HF.check_forward("fwd_count_stride33", buf[:, :32].reshape(n, 16, 2), r64, mag, r32, rep)
    assert bool(torch.isnan(buf[:, 32]).all())
    # part = (offset, count) into a pre-filled buffer: the other rows keep their bits
    off = n // 3
    cnt = max(1, n - off - 1)
    before = torch.rand(16, n, 2, generator=torch.Generator().manual_seed(2)).to(DEV)
    buf = before.clone()
    ops.hashgrid_fwd(xd, td, sc, log2_T, True, out=buf, part=(off, cnt))
    sl = slice(off, off + cnt)
    fails += HF.check_forward("part", buf[:, sl].permute(1, 0, 2), r64[sl], mag[sl], r32[sl], rep)
    keep = torch.ones(n, dtype=torch.bool, device=DEV)
    keep[sl] = False
    assert torch.equal(buf[:, keep].view(torch.int32), before[:, keep].view(torch.int32)), "rows outside the part changed"
    assert not fails, fails


@pytest.mark.parametrize("m,n", [(1, 5), (300, 257), (257, 1)])
def test_enc_gather_is_bit_exact_and_clamps(m, n):
    ops, _ = _mods()
    g = torch.Generator().manual_seed(31 + m)
    enc = torch.randn(16, m, 2, generator=g)
    idx = torch.randint(0, m, (n,), generator=g)
    idx[0] = -3  # clamped to 0
    idx[-1] = m + 2  # clamped to m - 1
    if n > 4:
        idx[1], idx[2], idx[3] = -(2 ** 40), m, 2 ** 40
    got = ops.enc_gather(enc.to(DEV), idx.to(DEV)).cpu()
    want = enc[:, idx.clamp(0, m - 1)]
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------------------ #
# backward
# ------------------------------------------------------------------------------------------------------------------------------ #
PATHS = ("atomic", "onecall", "prepare_apply", "count_apply", "groups", "adam")


def _check_fused_adam(key, adam, before, d_table, Tn, levels):
    """The Adam step in the epilogue of the bucket reduce (``step4`` in csrc/umhs_hashgrid_part.h) under the rules of tests/adam_f64.py:
    the levels ``levels`` = [l0, l1) of table, exp_avg and exp_avg_sq against the replay (bits) and the float64 oracle (envelope) of one
    update from ``before`` with g = the d_table this very launch wrote, grad_scale 1, no clamp; every other level keeps its bits in
    all three buffers."""
    l0, l1 = levels
    part = lambda t: t.view(16, Tn, 2)[l0:l1].reshape(-1)
    host = lambda t: part(t).cpu().numpy()
    case = AF.Case(key, *(host(before[k]) for k in ADAM_BUFFERS), host(d_table), AF.Hyper(adam["lr"], *adam["betas"], adam["eps"], adam["step"]))
    fails = AF.check(*(part(adam[k]) for k in ADAM_BUFFERS), case, REPORT["fused adam"])
    keep = torch.ones(16, dtype=torch.bool)
    keep[l0:l1] = False
    for k in ADAM_BUFFERS:
        if bool(keep.any()) and not torch.equal(adam[k].view(16, Tn, 2)[keep].view(torch.int32), before[k].view(16, Tn, 2)[keep].view(torch.int32)):
            fails.append(f"{key}: {k} changed in a level outside [{l0}, {l1})")
    return fails


def _launch(path, c, x, sc, d_enc, d_table, overwrite, table=None, adam=None):
    ops, _ = _mods()
    lb, lc = c.levels[0], len(c.levels)
    ops._release(x.device, ops.WS_HASH_BWD)
    kw = dict(level_begin=lb, level_count=lc)
    if path in ("atomic", "onecall"):
        ops.hashgrid_bwd(x, d_enc, sc, c.log2_T, d_table, True, method="atomic" if path == "atomic" else "partition", overwrite=overwrite, **kw)
    elif path == "prepare_apply":
        assert ops.hashgrid_bwd_prepare(x, sc, c.log2_T, lb, lc)
        ops.hashgrid_bwd_apply(x, d_enc, sc, c.log2_T, d_table, True, overwrite=overwrite, ws_range=(lb, lc), **kw)
    elif path == "count_apply":  # the histogram of ALL levels from the forward's launch; the case's levels applied out of it
        assert ops.hashgrid_fwd_count(x, table, sc, c.log2_T) is not None
        assert ops.hashgrid_bwd_prepare_counted(x, sc, c.log2_T)
        ops.hashgrid_bwd_apply(x, d_enc, sc, c.log2_T, d_table, True, overwrite=overwrite, ws_range=(0, 16), **kw)
    elif path == "groups":  # level groups of 4 (of 2 in the four-level case) out of one prepare
        assert ops.hashgrid_bwd_prepare(x, sc, c.log2_T, lb, lc)
        step = 4 if lc == 16 else 2
        for l0 in range(lb, lb + lc, step):
            ops.hashgrid_bwd_apply(x, d_enc, sc, c.log2_T, d_table, True, overwrite=overwrite, level_begin=l0, level_count=step, ws_range=(lb, lc))
    elif path == "adam":
        assert overwrite and ops.hashgrid_bwd_prepare(x, sc, c.log2_T, lb, lc)
        ops.hashgrid_bwd_apply(x, d_enc, sc, c.log2_T, d_table, True, overwrite=True, ws_range=(lb, lc), adam=adam, **kw)
    ops._release(x.device, ops.WS_HASH_BWD)


@pytest.mark.parametrize("name", list(HF.BWD_CASES))
def test_backward_every_slot_on_every_path(name):
    """Every path on the case, overwriting garbage and accumulating onto a non-zero table; the partitioned paths twice (bit equality
    run to run); the levels outside the case's range keep their bits."""
    c = HF.bwd_case(name)
    n, Tn = c.x.shape[0], 1 << c.log2_T
    lb, lc = c.levels[0], len(c.levels)
    x, sc = c.x.to(DEV), _sc()
    d_enc = torch.zeros(16, n, 2)
    d_enc[lb:lb + lc] = c.grads.permute(1, 0, 2)
    d_enc = d_enc.to(DEV)
    orc = [o.to(DEV) for o in c.oracle]
    g = torch.Generator().manual_seed(77)
    prior = ((torch.rand(16 * Tn, 2, generator=g) - 0.5) * 1e-3).to(DEV)
    table = HF.fwd_table(c.log2_T).to(DEV)
    garbage = torch.full((16 * Tn, 2), 123.0, device=DEV)
    models = {gm: HF.partition_model(c.geo, c.grads, gm).to(DEV) for gm in (True, False)}
    rep = REPORT["backward"].setdefault(name, {})
    fails = []
    lv = lambda t: t.view(16, Tn, 2)[lb:lb + lc]
    outside = torch.ones(16, dtype=torch.bool)
    outside[lb:lb + lc] = False
    for path in PATHS:
        kind = "atomic" if path == "atomic" else "partition"
        adam = None
        if path == "adam":  # the seventh step, from moments that are alive: m of both signs, v >= 0
            adam = dict(table=table.clone(), exp_avg=((torch.rand(16 * Tn, 2, generator=g) - 0.5) * 2e-3).to(DEV),
                        exp_avg_sq=(torch.rand(16 * Tn, 2, generator=g) * 1e-6).to(DEV), lr=1e-2, betas=(0.9, 0.99), eps=1e-15, step=7,
                        level_begin=lb + lc // 2)
            adam_before = {k: adam[k].clone() for k in ADAM_BUFFERS}
        # overwrite onto garbage
        d_table = garbage.clone()
        _launch(path, c, x, sc, d_enc, d_table, True, table, adam)
        key = f"{path}/overwrite"
        fails += HF.check_backward(f"{name}/{key}", lv(d_table), orc, kind, report=rep)
        rep[key] = rep.pop(f"{name}/{key}")
        if kind == "partition":
            ne = (lv(d_table).view(torch.int32) != models[path == "onecall"].view(torch.int32)).sum(dim=(1, 2)).tolist()
            for r, k in zip(rep[key], ne):
                r["not_bit_equal"] = int(k)
        if bool(outside.any()):
            assert bool((d_table.view(16, Tn, 2)[outside] == 123.0).all()), f"{key}: levels outside the range were written"
        if path in ("onecall", "prepare_apply"):
            again = garbage.clone()
            _launch(path, c, x, sc, d_enc, again, True, table)
            assert torch.equal(again.view(torch.int32), d_table.view(torch.int32)), f"{key}: not bitwise reproducible"
        if path == "adam":
            assert not torch.equal(adam["table"], table)  # the step was taken; its arithmetic, element by element:
            updated = (adam["level_begin"], lb + lc)
            fails += _check_fused_adam(name, adam, adam_before, d_table, Tn, updated)
            if n <= 2:  # no record lands in most slabs (all but one of a 2^13 level here): zero gradient, and they still step
                still = d_table.view(16, Tn, 2)[updated[0]:updated[1]] == 0
                moved = lambda k: (adam[k] != adam_before[k]).view(16, Tn, 2)[updated[0]:updated[1]]
                assert float(still.float().mean()) > 0.99 and bool(moved("exp_avg")[still].all()) and float(moved("table")[still].float().mean()) > 0.99
            if n <= 128:  # a non-finite gradient on the last level: its slabs with records are NaN in the gradient and in all three buffers
                bad = d_enc.clone()
                bad[lb + lc - 1, 0, 0] = NAN
                nan_table = garbage.clone()
                for k in ADAM_BUFFERS:
                    adam[k].copy_(adam_before[k])
                _launch(path, c, x, sc, bad, nan_table, True, table, adam)
                fails += _check_fused_adam(f"{name}/nan", adam, adam_before, nan_table, Tn, updated)
                last = lambda t: t.view(16, Tn, 2)[lb + lc - 1]
                hit = torch.isnan(last(nan_table))
                assert bool(hit.any()) and all(bool(torch.isnan(last(adam[k])[hit]).all()) for k in ADAM_BUFFERS)
            continue
        # accumulate onto a non-zero table
        d_table = prior.clone()
        _launch(path, c, x, sc, d_enc, d_table, False, table)
        key = f"{path}/accumulate"
        fails += HF.check_backward(f"{name}/{key}", lv(d_table), orc, kind, prior=lv(prior), report=rep)
        rep[key] = rep.pop(f"{name}/{key}")
        if bool(outside.any()):
            assert torch.equal(d_table.view(16, Tn, 2)[outside].view(torch.int32), prior.view(16, Tn, 2)[outside].view(torch.int32)), key
    assert not fails, fails
    if name in HF.TEETH_CASES:
        assert HF.teeth_share(rep["onecall/overwrite"]) >= 0.9


@pytest.mark.parametrize("strides", ["even", "odd"])
@pytest.mark.parametrize("name", ["rays13", "edges13"])
def test_backward_from_a_gradient_view_that_starts_one_float_into_its_storage(name, strides):
    """d_enc 4 bytes off an 8-byte boundary, level-major with even strides (2, 2 N) and row-major with the odd row stride 33: hb_load's
    scalar gradient load (and the atomic kernel's)."""
    ops, _hip = _mods()
    lib = _hip.lib()
    c = HF.bwd_case(name)
    n, Tn = c.x.shape[0], 1 << c.log2_T
    x, sc = c.x.to(DEV), _sc()
    orc = [o.to(DEV) for o in c.oracle]
    if strides == "even":
        store = torch.full((16 * n * 2 + 1,), NAN, device=DEV)
        view, sn, sl = torch.as_strided(store, (16, n, 2), (2 * n, 2, 1), 1), 2, 2 * n
        view.copy_(c.grads.permute(1, 0, 2))
    else:
        store = torch.full((n * 33 + 1,), NAN, device=DEV)
        view, sn, sl = torch.as_strided(store, (n, 16, 2), (33, 2, 1), 1), 33, 2
        view.copy_(c.grads)
    d_ptr = store.data_ptr() + 4
    assert d_ptr % 8 == 4
    nbytes = lib.umhs_hashgrid_bwd_workspace_bytes(n, 16, c.log2_T)
    ops._release(x.device, ops.WS_HASH_BWD)
    ws = ops._workspace(nbytes, x.device, ops.WS_HASH_BWD)
    rep = REPORT["backward"].setdefault(f"{name}/view+1/{strides}", {})
    fails = []
    for path in ("atomic", "onecall", "prepare_apply"):
        d_table = torch.full((16 * Tn, 2), 123.0, device=DEV)
        if path == "prepare_apply":
            _hip.check(lib.umhs_hashgrid_bwd_prepare(ops.ptr(x), ops.ptr(sc), n, 0, 16, c.log2_T, ops.ptr(ws), ws.numel(), _hip.stream()), "prepare")
            _hip.check(lib.umhs_hashgrid_bwd_apply(ops.ptr(x), d_ptr, sn, sl, ops.ptr(sc), n, 0, 16, 0, 16, c.log2_T, ops.ptr(d_table), 1, ops.ptr(ws),
                                                   ws.numel(), _hip.stream()), "apply")
        else:
            w = None if path == "atomic" else ws
            _hip.check(lib.umhs_hashgrid_bwd(ops.ptr(x), d_ptr, sn, sl, ops.ptr(sc), n, 0, 16, c.log2_T, ops.ptr(d_table), 1, ops.ptr(w),
                                             w.numel() if w is not None else 0, _hip.stream()), "umhs_hashgrid_bwd")
        key = f"{path}/overwrite"
        fails += HF.check_backward(key, d_table.view(16, Tn, 2), orc, "atomic" if path == "atomic" else "partition", report=rep)
    assert not fails, fails
