"""The hash-grid comparators (tests/hash_f64.py) have the power to see the bugs they are there for: fed the float32 model of the
kernels' own arithmetic in place of the kernels' results, every case passes (this run is also where K_f, K_b and K_a are measured and
where the teeth condition and the fixed-point quantum are held); with a fault planted in the model, every case the fault applies to
fails.  A float32 emulation of hb_fixed is swept over both signs and binades -40..5 and its worst error, in units of the fixed-point
quantum, is asserted: E_FIX, the figure the per-slot rule and the comment in csrc/umhs_hashgrid_part.h quote.

Faults: (1) the partner slot of a pair record formed with k one too small; (2) ox and 1 - ox swapped in a pair record; (3) an integer
x coordinate giving its weight to slot floor + 1; (4) a run's first sample lost where the run crosses a 16-lane row; (5) the records of
a bucket past its 4096th (5a) and past its 8192nd (5b) dropped; (6) the other half of the 16-byte pair taken for odd slot indices in
the forward; (7) the offsets of buckets >= 64 missing the first scan round's carry; (8) the fixed-point scale 20 bits too coarse;
(9) overwrite mode leaving an untouched slot's stale value; (10) the slab of a level group applied one level off."""
import math

import numpy as np
import pytest
import torch

import hash_f64 as HF

_cache = {}
WORST = {}


def _stats(name):
    _model(name, False)
    return _cache[("stats", name)]


def _model(name, grad_mask, exact=False, fault=None, contract=True):
    key = ("model", name, grad_mask, exact, fault, contract)
    if key not in _cache:
        torch.set_num_threads(max(1, min(torch.get_num_threads(), 8)))  # (small tensors: a wide thread pool only costs)
        c = HF.bwd_case(name)
        st = {}
        _cache[key] = HF.partition_model(c.geo, c.grads, grad_mask, exact=exact, fault=fault, stats=st, contract=contract)
        if fault is None and not exact and not grad_mask and contract:
            _cache[("stats", name)] = st
    return _cache[key]


def _atomic(name):
    if ("atomic", name) not in _cache:
        c = HF.bwd_case(name)
        _cache[("atomic", name)] = HF.atomic_model(c.geo, c.grads)
    return _cache[("atomic", name)]


def _fwd(name):
    if ("fwd", name) not in _cache:
        kind, log2_T, n = HF.FWD_CASES[name]
        x, table = HF.positions(kind, n), HF.fwd_table(log2_T)
        geo = HF.geometry(x, HF.ALL_LEVELS, log2_T)
        r64, mag = HF.forward_oracle(geo, table)
        r32 = HF.T.hash_encode(x, table, HF.T.hash_scalings(), log2_T).view(-1, 16, 2)
        _cache[("fwd", name)] = (geo, table, r64, mag, r32)
    return _cache[("fwd", name)]


def _note(family, worst):
    WORST[family] = max(WORST.get(family, 0.0), worst)


def _measure_backward(name):
    c = HF.bwd_case(name)
    for gm in (True, False):
        rep = {}
        assert not HF.check_backward("exact", _model(name, gm, exact=True), c.oracle, "partition", report=rep)
        _note("partitioned backward", max(r["worst"] for r in rep["exact"]))
    rep = {}
    assert not HF.check_backward("atomic", _atomic(name), c.oracle, "atomic", report=rep)
    _note("atomic backward", max(r["worst"] for r in rep["atomic"]))


# ------------------------------------------------------------------------------------------------------------------------------ #
# the clean model passes; K, teeth, quantum
# ------------------------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("name", list(HF.BWD_CASES))
def test_the_float32_model_passes_the_backward_comparators(name):
    c = HF.bwd_case(name)
    prior = (torch.rand(len(c.levels), 1 << c.log2_T, 2, generator=torch.Generator().manual_seed(1)) - 0.5) * 1e-3
    for gm in (True, False):
        rep = {}
        m = _model(name, gm)
        fails = HF.check_backward("overwrite", m, c.oracle, "partition", report=rep)
        if not gm:  # hb_fixed's remainder as the source spells it instead of as compiled (one fma): the rule holds for both
            fails += HF.check_backward("as written", _model(name, gm, contract=False), c.oracle, "partition")
        fails += HF.check_backward("accumulate", prior + m, c.oracle, "partition", prior=prior)
        assert not fails, fails
        if name in HF.TEETH_CASES:
            assert HF.teeth_share(rep["overwrite"]) >= 0.9, HF.teeth_share(rep["overwrite"])
    _measure_backward(name)
    a = _atomic(name)
    assert not HF.check_backward("atomic accumulate", prior + a, c.oracle, "atomic", prior=prior)
    print(name, {k: round(v, 3) for k, v in WORST.items()}, "teeth", round(HF.teeth_share(rep["overwrite"]), 3))


@pytest.mark.parametrize("name", list(HF.FWD_CASES))
def test_the_float32_reference_passes_the_forward_comparators(name):
    """float32 hash_encode against the float64 oracle, and the numpy copy of the kernel's tree against hash_encode bit for bit."""
    geo, table, r64, mag, r32 = _fwd(name)
    rep = {}
    assert not HF.check_forward("ref32", r32, r64, mag, r32, rep)
    assert not HF.check_forward("model", HF.forward_model(geo, table), r64, mag, r32)
    _note("forward", max(rep["ref32"]["worst"]))
    assert min(rep["ref32"]["teeth"]) >= 0.9


def test_k_leaves_the_float32_model_a_factor_of_four_and_is_at_least_8():
    """K per family = max(8, 4 x the worst ratio of the float32 model, rounded up to a power of two).  (Runs the clean cases it needs.)"""
    for name in HF.BWD_CASES:
        _measure_backward(name)
    for name in HF.FWD_CASES:
        rep = {}
        geo, table, r64, mag, r32 = _fwd(name)
        HF.check_forward("ref32", r32, r64, mag, r32, rep)
        _note("forward", max(rep["ref32"]["worst"]))
    have = {"forward": HF.K_F, "partitioned backward": HF.K_B, "atomic backward": HF.K_A}
    print({f: round(w, 3) for f, w in WORST.items()}, have)
    assert set(WORST) == set(have)
    for f, k in have.items():
        assert k >= 8 and math.log2(k) == int(math.log2(k)) and 4 * WORST[f] <= k, (f, WORST[f], k)
        assert k == max(8.0, 2.0 ** math.ceil(math.log2(4 * WORST[f]))), (f, WORST[f], k)


def test_hb_fixed_rounds_negative_addends_by_up_to_128_units():
    """hi = (int)floorf(x), lo = saturating (uint32)((x - floorf(x)) * 2^32) against floor(x * 2^32), 2000 values per binade and sign."""
    g = np.random.default_rng(3)
    worst = {1: 0.0, -1: 0.0}
    saturated = 0
    for b in range(-40, 6):
        m = (1 + g.random(2000)).astype(np.float32)
        for sign in (1, -1):
            x = (sign * np.ldexp(m, b)).astype(np.float32)
            truth = np.floor(x.astype(np.float64) * 4294967296.0)  # exact: 24 significant bits, scaled by a power of two
            got = HF.hb_fixed_model(x)
            err = np.abs(got.astype(np.float64) - truth)  # (|values| < 2^38: exact in float64)
            worst[sign] = max(worst[sign], float(err.max()))
            saturated += int(((x - np.floor(x)).astype(np.float32) == 1.0).sum())
    print("hb_fixed worst error in units:", worst, "remainders that rounded to 1.0f:", saturated)
    assert worst[1] < 1.0  # positive addends: the floor alone
    assert 64.0 < worst[-1] <= HF.E_FIX == 128.0  # negative addends in (-1, 0): half the float32 spacing below 1, in units of 2^-32
    assert saturated > 0  # the conversion of 2^32 is reached: the emulation saturates it, as v_cvt_u32_f32 does
    # the two examples of the record: -7.8 units become -1, -197 units become -256
    ex = HF.hb_fixed_model(np.array([-7.8 / 4294967296.0, -197.0 / 4294967296.0], np.float32))
    assert ex.tolist() == [-1, -256]


@pytest.mark.parametrize("name", list(HF.BWD_CASES))
def test_the_quantum_bounds_what_the_fixed_point_costs(name):
    """|fixed-point model - exactly accumulated model| <= n_s Q + one float32 rounding, per slot component: Q is an upper bound of the
    unit the reduce pass really uses, times hb_fixed's 128."""
    c = HF.bwd_case(name)
    worst = 0.0
    for gm in (False,):
        # (the remainder as written: both runs then start from the same rounded products and differ by the fixed point alone)
        fx, ex = _model(name, gm, contract=False), _model(name, gm, exact=True)
        for li, o in enumerate(c.oracle):
            d = (fx[li][o.slots].double() - ex[li][o.slots].double()).abs()
            bound = o.cnt * o.q[:, None] + 2 * HF.U * o.ref.abs() + HF.U * HF.TINY
            worst = max(worst, float((d / bound).max()))
    print(name, "worst |fixed - exact| / (n_s Q + 2 u |ref|):", worst)
    assert worst <= 1.0


def test_the_cases_reach_the_paths_the_docstring_names():
    st = _stats("scattered12")
    assert all(v["max_bucket_records"] > 8192 and v["nb"] == 1 and v["merged_records"] == 0 for v in st.values())
    st = _stats("rays13")
    assert st[0]["merged_records"] > 0 and st[0]["crossing_runs"] > 0 and st[15]["merged_records"] == 0
    assert HF.bwd_case("rays13").x.shape[0] == 3072 + 5
    assert _stats("threshold13")[0]["nonhead_per_wave"] == [15, 16]
    assert _stats("threshold13")[0]["merged_records"] > 0
    st = _stats("edges13")
    assert all(v["eqx_solo"] > 0 for v in st.values()) and set(range(11)) <= set(st[15]["pair_k"]) and 15 in st[15]["pair_k"]
    assert _stats("scattered19")[15]["nb"] == 64 and _stats("scattered19")[15]["buckets_used"] == 64
    st = _stats("scattered20")
    assert all(v["nb"] == 128 and v["high_buckets"] > 0 for v in st.values())
    # the one-call form drops the zero-gradient samples and breaks runs there: other records, same sums within the rule
    a, b = _model("rays13", True), _model("rays13", False)
    assert not torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------------------------ #
# planted faults
# ------------------------------------------------------------------------------------------------------------------------------ #
def _applies(name, fault):
    st = _stats(name)
    if fault in (1, 2):
        return any(v["odd_floor_pairs"] > 0 for v in st.values()) if fault == 1 else True
    if fault == 3:
        return any(v["eqx_solo"] > 0 for v in st.values())
    if fault == 4:
        return any(v["crossing_runs"] > 0 for v in st.values())
    if fault == "5a":
        return any(v["max_bucket_records"] > 4096 for v in st.values())
    if fault == "5b":
        return any(v["max_bucket_records"] > 8192 for v in st.values())
    if fault == 7:
        return any(v["high_buckets"] > 0 for v in st.values())
    if fault == 8:  # needs a slot whose whole gradient lies far below the level maximum: every case with more than one sample
        return HF.bwd_case(name).x.shape[0] > 1
    if fault == 9:
        return True
    if fault == 10:
        return len(HF.bwd_case(name).levels) == 16
    raise KeyError(fault)


MODEL_FAULTS = (1, 2, 3, 4, "5a", "5b", 7, 8)
# which case each fault must apply to at the least (so that no fault is vacuous)
MUST_APPLY = {1: "one_cell13", 2: "tiny13", 3: "edges13", 4: "rays13", "5a": "rays13", "5b": "scattered12", 7: "scattered20", 8: "tiny13",
              9: "one_cell13", 10: "scattered19"}


@pytest.mark.parametrize("fault", list(MUST_APPLY), ids=lambda f: f"fault{f}")
@pytest.mark.parametrize("name", list(HF.BWD_CASES))
def test_planted_backward_faults_are_rejected(name, fault):
    applies = _applies(name, fault)
    if MUST_APPLY[fault] == name:
        assert applies
    if not applies:
        return  # (the fault changes nothing in this case: nothing to reject)
    c = HF.bwd_case(name)
    if fault in MODEL_FAULTS:
        bad = _model(name, False, fault=fault)
        prior = None
    elif fault == 9:
        bad = _model(name, False).clone()
        li = len(c.levels) - 1
        free = torch.ones(1 << c.log2_T, dtype=torch.bool)
        free[c.oracle[li].slots] = False
        bad[li, int(free.nonzero()[0]), 1] = 123.0
        prior = None
    else:
        m = _model(name, False)
        bad = m.clone()
        bad[4:8] = m[3:7]  # the second group of four levels lands one level up
        prior = None
    assert not torch.equal(bad, _model(name, False)), "the fault must change the model's result"
    fails = HF.check_backward("fault", bad, c.oracle, "partition", prior=prior)
    assert fails, f"fault {fault} passes in {name}"


@pytest.mark.parametrize("name", list(HF.FWD_CASES))
def test_planted_forward_fault_is_rejected(name):
    geo, table, r64, mag, r32 = _fwd(name)
    bad = HF.forward_model(geo, table, fault=6)
    assert not torch.equal(bad, r32)
    rep = {}
    fails = HF.check_forward("fault6", bad, r64, mag, None, rep)  # (the float64 rule alone must see it)
    assert fails, name
