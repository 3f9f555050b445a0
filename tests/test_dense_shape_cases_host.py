"""What the case table of tests/dense_shape_cases.py claims about itself, asserted on the CPU: a failure of test_zzz_dense_shapes_gpu.py is then never the table's or the
reference's fault.  Every (family group, boundary) pair and every template instantiation the table must hold is claimed by a case; every case's family follows from the
restated launcher predicates in the launchers' order of trial; every constant and tuning default the predicates cite equals the value parsed out of csrc/; and the
derived quantities the cases rely on -- waves per tile, k-steps per wave, split-K slab lengths, row splits and scratch bytes -- are what the cases say they are."""
import numpy as np
import pytest

import conv_shape_cases as cc
import dense_shape_cases as dc
from hip_helpers import DT, rounded


def test_constants_are_the_sources():
    h = dc.source_constants()
    assert h["GEMM_BM"] == dc.GEMM_BM == cc.GEMM_BM
    assert (h["WG_F32"], h["WG_BF16"], h["WG_X3"]) == (dc.WGRAD_BP["f32"], dc.WGRAD_BP["bf16"], dc.WGRAD_BP["x3"])
    assert h["G2_OOB"] == dc.G2_OOB
    assert h["SMALLM_MAX_M"] == dc.SMALLM_MAX_M and h["SMALLM_TILE"] == [dc.SMALLM_TILE] * 2 and h["SMALLM_KSTEP"] == dc.SMALLM_KSTEP and h["SMALLM_WAVES"] == dc.SMALLM_WAVES
    assert tuple(h["TALLK_N"]) == dc.TALLK_N and h["TALLK_GROUP"] == dc.TALLK_GROUP and h["TALLK_ROWS"] == dc.TALLK_ROWS and 1 << h["TALLK_STEP"] == h["TALLK_KMOD"] == 16
    assert [1 << b for b in h["TALLK_MAX"]] == [dc.TALLK_MAX_BYTES] * 2
    assert h["SPLITK_BK"] == [dc.SPLITK_BK["bf16"], dc.SPLITK_BK["f32"]] and dc.SPLITK_BK["x3"] == dc.SPLITK_BK["f32"] and h["SPLITK_STAGE"] == 128
    assert h["DWG_PRED"] == [dc.DWG_TILE] * 4 + [dc.DWG_MIN_TILES] and h["DWG_TILE"] == [dc.DWG_TILE] * 2 and h["DWG_ROWS"] == dc.DWG_ROWS
    assert h["DWGS_PRED"] == [16, 16, dc.DWGS_TILE, dc.DWGS_TILE, dc.DWGS_MAX_KN] and h["DWGS_TILE"] == [dc.DWGS_TILE] * 2
    assert h["DWGS_DEPTH"] == dc.DWGS_DEPTH and 1 << h["DWGS_STEP"] == dc.DWGS_STEP and h["DWGS_WSPLIT"] == [dc.DWGS_STEP, 2, 2]
    assert h["WIDE_ROWS"] == 64 and h["DENSE_TARGET_KEY"] == 11
    for key, v in dc.DEFAULTS.items():
        assert h["DEFAULTS"][key] == v, (key, h["DEFAULTS"][key], v)
    for name, v in dc.ENV_DEFAULTS.items():
        assert h["ENV_DEFAULTS"][name] == v, (name, h["ENV_DEFAULTS"][name], v)


def test_case_lists_have_fixed_lengths():
    assert len(dc.CASES) == 103 and [c.id for c in dc.CASES] == list(range(103))
    assert dict(dc.N_CASES) == {"dense_smallm": 8, "tallk": 9, "gemm2": 21, "gen1": 14, "dwg": 7, "dwgs": 13, "gen1w": 17, "pair": 5, "refused": 9}
    assert len(set(dc.case_id(c) for c in dc.CASES)) == len(dc.CASES)
    assert all(c.entry in dc.ENTRIES and c.dt in DT and c.why and c.layout in (0, 1) and c.nsplit >= 1 for c in dc.CASES)


@pytest.mark.parametrize("group", sorted(dc.REQUIRED))
def test_every_family_boundary_pair_is_claimed(group):
    have = set()
    for c in dc.CASES:
        if dc.group_of(c.family) == group:
            have |= set(c.tags)
    missing = set(dc.REQUIRED[group].split()) - have
    assert not missing, (group, sorted(missing))


def test_every_family_and_instantiation_has_a_case():
    fams = set(c.family for c in dc.CASES)
    assert not [i for i in dc.INSTANTIATIONS if i not in fams]
    assert set(dc.group_of(f) for f in fams) == set(dc.REQUIRED)
    # the instantiation no key reaches (dwg_kernel<4>) and the knobs' fall-backs: the child-process steps
    landed = [set(dc.family_of(c, env)[0] for c in dc.env_cases(i)) for i, (env, _, _) in enumerate(dc.ENV_STEPS)]
    assert "dwg.4" in landed[0] and any(f.startswith("gemm2.") for f in landed[0]) and any(f.startswith("gen1.") for f in landed[0])
    assert landed[1] == {"gen1.n32.splitk", "gen1.n64.splitk", "gen1.n128.splitk", "gen1w.128.single"}
    for i, (env, prefixes, allowed) in enumerate(dc.ENV_STEPS):
        cases = dc.env_cases(i)
        assert landed[i] <= set(allowed), landed[i] - set(allowed)
        for p in prefixes:                                 # every case of the families the knob switches off runs again
            assert [c.id for c in cases if c.family.startswith(p)] == [c.id for c in dc.CASES if c.family.startswith(p) and (p != "gemm2." or c.nsplit > 1)], p


@pytest.mark.parametrize("c", dc.CASES, ids=dc.case_id)
def test_claimed_family_and_sizes_follow_from_the_predicates(c):
    fam, plan = dc.family_of(c)
    assert fam == c.family
    o = c.opt
    for key in ("steps", "last", "ws", "ns", "grid", "stages", "splits", "wave_steps"):
        if key in o:
            assert list(np.atleast_1d(plan[key])) == list(np.atleast_1d(o[key])), (key, plan[key], o[key])
    if fam.startswith("refused"):
        assert "refused" in c.tags and plan is None
    if "falls_through" in c.tags:
        assert not fam.startswith(("dense_smallm", "tallk", "dwg.", "dwgs.")) and fam != "pair"
    if c.entry == "fwd" and c.dt == "bf16":
        assert c.K % 8 == 0 or fam.startswith("refused")
    kn = dc.knobs_of(c)
    for tag, (key, val) in {"key0_off": (0, 0), "key22_off": (22, 0), "key11_16": (11, 16), "key11_1": (11, 1), "key11_1024": (11, 1024), "auto_small_grid": (17, 0)}.items():
        if tag in c.tags:
            assert kn[key] == val


def test_sizes_sit_on_the_edges_they_cite():
    def one(prefix, *tags):
        got = [c for c in dc.CASES if c.family.startswith(prefix) and set(tags) <= set(c.tags)]
        assert got, (prefix, tags)
        return got
    # dense_smallm: both sides of M = 256, a half-filled last step, waves without a step, tails inside a tile
    assert [c.M for c in one("dense_smallm", "m_at")] == [dc.SMALLM_MAX_M] and [c.M for c in one("gen1", "m_past", "falls_through")] == [dc.SMALLM_MAX_M + 1]
    assert all(c.K % 8 == 4 for c in one("dense_smallm", "k_mod8_4")) and all(c.K < 32 for c in one("dense_smallm", "k_below_32"))
    assert all(0 in dc.smallm_wave_steps(c.K) for c in one("dense_smallm", "idle_waves"))
    assert all(len(set(dc.smallm_wave_steps(c.K))) > 1 and 0 not in dc.smallm_wave_steps(c.K) for c in one("dense_smallm", "uneven_waves"))
    assert all(c.M % 32 for c in one("dense_smallm", "m_tail")) and all(c.N % 32 for c in one("dense_smallm", "n_tail"))
    assert all(c.opt.get("relu") and not c.opt.get("mask") for c in one("dense_smallm", "relu_nomask"))
    # tall-K: every instantiation; step counts below, at and past one and two request groups; clamped rows
    g = dc.TALLK_GROUP
    assert sorted(set(dc.family_of(c)[1]["steps"] for c in dc.by_family("tallk"))) == [g - 1, g, g + 1, 2 * g - 1, 2 * g, 2 * g + 1]
    assert sorted(set(c.M for c in dc.by_family("tallk"))) == [1, 31, 32, 33, 64, 96, 112, 160]
    for c in dc.by_family("tallk"):
        p = dc.family_of(c)[1]
        assert p["len"] * c.nsplit == c.K and p["grid"][1] * p["kp"] == c.nsplit
    # gemm2 split-K: whole stages per split, a last slab of some stages plus 16 bytes, the stage fall-back, the empty slab
    for c in one("gemm2", "last_slab_short"):
        p = dc.family_of(c)[1]
        assert (p["len"] * cc.esz(c.dt)) % 128 == 0 and 0 < p["last"] < p["len"] and p["len"] * (c.nsplit - 1) + p["last"] == c.K
    assert sorted((p["last"] * cc.esz(c.dt)) % 128 for c in one("gemm2", "last_slab_short") for p in [dc.family_of(c)[1]]).count(16) >= 3
    for c in one("gen1", "stage_fallback"):
        assert c.layout == 1 and (dc.family_of(c)[1]["len"] * cc.esz(c.dt)) % 128 != 0 and dc.knobs_of(c)[0] == 1
    for c in one("refused", "empty_slab"):
        assert dc.splitk_len(c.dt, c.K, c.nsplit)[1] <= 0 and dc.splitk_len(c.dt, c.K, c.nsplit - 1)[1] > 0
    # gemm2 tiles: rows below / at / past a tile, nk on both sides of 6
    assert sorted(c.M for c in one("gemm2.128x64", "nk_at")) == [127, 128, 129] and sorted(c.M for c in one("gemm2.256x32", "t256x32") if c.nsplit == 1) == [256, 257]
    assert all(cc.ceil_div(c.K * cc.esz(c.dt), 128) == 6 for c in one("gemm2", "nk_at")) and all(cc.ceil_div(c.K * cc.esz(c.dt), 128) < 6 and c.tune[20] >= 3 for c in one("gemm2", "nk_below"))
    assert sorted(c.N for c in one("gen1.n", "n_at") + one("gen1.n", "n_past")) == [32, 33, 64, 65]
    # dwg: the early return, both tile orders, the ring's fill levels
    for c in one("dwg", "early_return"):
        p = dc.family_of(c)[1]
        assert p["grid"][1] > 0 and (p["KT"] * p["NT"]) % 8
    assert all(dc.family_of(c)[1]["NT"] > dc.family_of(c)[1]["KT"] and c.M % dc.DWG_ROWS for c in one("dwg", "nt_major", "ragged_stage"))
    assert [c.M for c in one("dwg", "m_below_stage")] == [7] and all(c.M <= 100 for c in dc.by_family("dwg."))
    nst = dc.ENV_DEFAULTS["MI355_DWG_NST"]
    assert [dc.family_of(c)[1]["stages"] for c in one("dwg", "stages_nst_minus_1") + one("dwg", "stages_nst") + one("dwg", "stages_past_nst")] == [nst - 1, nst, nst + 1]
    assert [dc.family_of(c)[1]["stages"] for c in one("dwg", "stages_nst4_minus_1") + one("dwg", "stages_nst4")] == [3, 4]
    c = one("gen1w", "tiles_255")[0]
    assert (c.K // dc.DWG_TILE) * (c.N // dc.DWG_TILE) == dc.DWG_MIN_TILES - 1 and c.opt["overwrite"]
    # dwgs: the row counts of every wave count (the two-wave ones are 64, 96, 160, 224), groups and tails against the depth, the K N limit from both sides
    assert sorted(set(c.M for c in dc.by_family("dwgs.") if dc.dwgs_wsplit(c.M) == 2)) == [64, 96, 160, 224]
    assert sorted(set(c.M for c in dc.by_family("dwgs.") if dc.dwgs_wsplit(c.M) == 1)) == [16, 32, 112] and sorted(set(c.M for c in dc.by_family("dwgs.") if dc.dwgs_wsplit(c.M) == 4)) == [128, 256, 320]
    assert [dc.dwgs_wsplit(m) for m in (512, 16, 48, 80, 2048, 32)] == [4, 1, 1, 1, 4, 1]         # (the row counts test_ops_gpu.py ran before this table existed: no two-wave launch)
    for c in dc.by_family("dwgs."):
        p = dc.family_of(c)[1]
        assert p["ws"] * p["ns"] * dc.DWGS_STEP == c.M
        for t, want in (("tail_1", 1), ("tail_3", 3), ("whole_group", 0)):
            if t in c.tags:
                assert p["ns"] % dc.DWGS_DEPTH == want and p["ns"] >= dc.DWGS_DEPTH
    assert [c.K * c.N for c in one("dwgs", "kn_at") + one("gen1w", "kn_past")] == [dc.DWGS_MAX_KN, dc.DWGS_MAX_KN + 64 * 512]
    # first-generation filter gradient: 64 / 65 / 61 result rows, the target block count, row splits and scratch bytes
    assert [dc.family_of(c)[1]["Kce"] for c in one("gen1w", "kce_64") + one("gen1w", "kce_65") + one("gen1w", "kce_61")] == [64, 65, 61]
    assert [dc.family_of(c)[1]["splits"] for c in one("gen1w", "key11_16") + one("gen1w", "key11_1") + one("gen1w", "key11_1024")] == [16, 1, 9]
    for c in dc.by_family("gen1w"):
        kn, p = dc.knobs_of(c), dc.family_of(c)[1]
        if c.opt.get("scratch") == "exact" and p["splits"] > 1:       # what mi_gemm_wgrad_scratch_bytes returns covers the launch's slabs, with or without the bias row
            assert dc.scratch_bytes(c.dt, c.M, c.K, c.N, kn) >= p["slab_bytes"] == p["splits"] * cc.ceil_div(p["Kce"] * c.N, 4) * 16
        if "m_tail" in c.tags:
            assert c.M % p["mps"]
    for c in one("refused", "overwrite_short_scratch"):
        need = dc.gen1w_plan(c.dt, c.M, c.K, c.N, c.opt.get("dbias"), dc.knobs_of(c))["slab_bytes"]
        assert dc.scratch_given(c, dc.knobs_of(c)) == need - 16
    for c in dc.by_family("pair"):
        plans = dc.family_of(c)[1]["plans"]
        assert (c.family == "pair") == (c.dt == "bf16" and all(p["wide"] for p in plans) and not dc.dwgs_ok(c.dt, c.M, c.K, c.N, dc.knobs_of(c)))


@pytest.mark.parametrize("c", [c for c in dc.CASES if c.K * c.N <= 1 << 20 and not c.family.startswith("refused")], ids=dc.case_id)
def test_references_are_finite_and_masks_are_planted(c):
    d, r = dc.reference(c)
    for name, v in r.items():
        assert np.isfinite(v).all() and np.abs(v).max() > 0, name
    if c.entry == "fwd" and c.opt.get("mask") and c.M * c.N >= 3:
        m = rounded(d["mask"], DT[c.dt][1]).numpy().reshape(-1)
        assert m[0] == 0.0 and m[1] < 0 and m[2] > 0 and r["out"].reshape(-1)[0] == 0 and r["out"].reshape(-1)[1] == 0
    if c.entry == "fwd" and c.nsplit > 1:
        assert r["slabs"].shape == (c.nsplit, c.M, c.N) and np.allclose(r["slabs"].sum(0), r["out"], rtol=1e-12, atol=1e-12)
        rs = dc.slab_ranges(c)
        assert rs[0][0] == 0 and rs[-1][1] == c.K and all(a[1] == b[0] for a, b in zip(rs, rs[1:])) and all(lo < hi for lo, hi in rs)
    if c.entry == "fwd" and c.opt.get("relu") and c.M * c.N >= 64:
        assert (r["out"] == 0).any() and (r["out"] > 0).any()
