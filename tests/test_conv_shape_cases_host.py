"""What the case table of tests/conv_shape_cases.py claims about itself, asserted on the CPU: a failure of test_x_conv_shapes_gpu.py is then never the table's or the
reference's fault.  Every (family, boundary) pair the table must hold is claimed by a case; every case's family follows from the restated launcher predicates in the
launchers' order of trial; the lists have fixed lengths; every reference is finite with a non-zero scale; every mask carries its planted 0.0 and negative value; and
every derived size equals the constant it cites -- the constants are parsed out of the headers, so a changed tile size fails here instead of moving a case off its edge."""
import numpy as np
import pytest

import conv_shape_cases as cc
from hip_helpers import DT, rounded

SMALL = [c for c in cc.CASES if c.B <= 16]


def test_constants_are_the_headers():
    h = cc.header_constants()
    assert h["TC_BMT"] == cc.TC_BMT and h["TC_MAXHALO"] == cc.TC_MAXHALO and h["SMALL_TILE"] == [cc.TC_BMT_SMALL, cc.TC_MAXHALO_SMALL]
    assert h["TW_BP"] == cc.TW_BP and h["GN_BMT"] == cc.GN_BMT and h["GEMM_BM"] == cc.GEMM_BM
    assert h["NW_BP"] == cc.NW_BP and h["NW_SLAB"][0] * h["NW_SLAB"][1] + h["NW_SLAB"][2] == cc.NW_SLAB
    assert (h["WG_F32"], h["WG_BF16"], h["WG_X3"]) == (cc.WGRAD_BP["f32"], cc.WGRAD_BP["bf16"], cc.WGRAD_BP["x3"])
    assert h["RW_MAXHALO"] == [cc.RW_MAXHALO[2], cc.RW_MAXHALO[3]]
    assert h["RC_MAXHALO"] == [cc.RC_MAXHALO[(4, 1)], cc.RC_MAXHALO[(4, 2)], cc.RC_MAXHALO[(5, 1)]]
    assert h["GEN1_WGRAD_TARGET"] == cc.GEN1_WGRAD_TARGET
    assert h["NW_CUS"] * h["NW_WAVES"] == cc.NW_GRID_WAVES
    for key, v in cc.DEFAULTS.items():                     # the knobs' defaults as tuning.hip's table holds them: a changed default moves the split counts and scratch sizes
        assert h["DEFAULTS"][key] == v, (key, h["DEFAULTS"][key], v)


def test_case_lists_have_fixed_lengths():
    assert len(cc.CASES) == 197 and [c.id for c in cc.CASES] == list(range(197))
    assert dict(cc.N_CASES) == {"tapconv.conv": 26, "tapconv.gather": 22, "gemm2.conv": 12, "gemm2.gather": 7, "gen1": 23, "tapwgrad.conv": 13, "tapwgrad.gather4": 11,
                                "tapwgrad.gather5": 9, "rwconv.gather": 28, "rwconv.conv": 4, "narrow_conv": 14, "narrow_wgrad": 10, "gather_narrow": 11, "refused": 7}
    assert len(set(cc.case_id(c) for c in cc.CASES)) == len(cc.CASES)
    assert all(c.entry in cc.ENTRIES and c.dt in DT and c.why for c in cc.CASES)


@pytest.mark.parametrize("family", sorted(cc.REQUIRED))
def test_every_family_boundary_pair_is_claimed(family):
    have = set()
    for c in cc.CASES:
        if c.family.split(":")[0] == family:
            have |= set(c.tags)
    missing = set(cc.REQUIRED[family].split()) - have
    assert not missing, (family, sorted(missing))


@pytest.mark.parametrize("c", cc.CASES, ids=cc.case_id)
def test_claimed_family_and_sizes_follow_from_the_predicates(c):
    fam, plan = cc.family_of(c)
    assert fam == c.family
    o = c.opt
    for key in ("MP", "halo", "tile", "GW", "utap", "splits", "capped", "nkb", "direct", "lean", "path"):
        if key in o:
            if key in ("halo", "GW") and key not in plan:            # a shape that fell through: the slot grid of the launcher that refused it
                form, B, ih, iw, ci, oh, ow, n = cc.tap_args(c)
                t, gh, gw, halo = cc.slot_grid(form, c.k, oh, ow)
                assert {"halo": halo, "GW": gw}[key] == o[key], (key, halo, gw, o[key])
                continue
            assert plan[key] == o[key], (key, plan[key], o[key])
    # the tuning a case sets is the tuning its tags speak of
    if "small" in c.tags:
        assert c.tune[5] == 2 and c.dt == "bf16"
    if c.family.startswith("refused"):
        assert "refused" in c.tags and plan is None
    if "falls_through" in c.tags:                          # the kernel the shape sits next to refuses it with the same tuning: switching every OTHER specialised family off changes nothing
        first = {"tapconv.gather": ("rwconv",), "tapconv.conv": ("rwconv",), "gemm2.gather": ("tapconv", "rwconv"), "gemm2.conv": ("tapconv", "rwconv"),
                 "gen1": ("tapconv", "tapwgrad", "narrow", "rwconv", "gemm2")}[fam]
        kn = cc.knobs_of(c)
        assert (kn[13] == 2 and "rwconv" in first) or (kn[1] >= 1 and "tapconv" in first) or (kn[3] and "tapwgrad" in first) or (kn[4] and "narrow" in first), "no first choice was switched on"


def test_sizes_sit_on_the_edges_they_cite():
    def one(fam, *tags):
        got = [c for c in cc.CASES if c.family == fam and set(tags) <= set(c.tags)]
        assert got, (fam, tags)
        return got
    for fam in ("tapconv.conv", "tapconv.gather"):
        for small, bmt, maxhalo in ((False, cc.TC_BMT, cc.TC_MAXHALO), (True, cc.TC_BMT_SMALL, cc.TC_MAXHALO_SMALL)):
            sel = (lambda c: ("small" in c.tags) == small)
            mp = {t: [cc.family_of(c)[1]["MP"] for c in one(fam, t) if sel(c)] for t in ("mp_below", "mp_at", "mp_past")}
            assert mp["mp_below"] and all(bmt - 2 <= m < bmt for m in mp["mp_below"])          # (bmt - 1 is prime for both tiles' neighbours 255 = 3 x 5 x 17 / 127: 126 is the nearest grid)
            assert mp["mp_at"] and all(m == bmt for m in mp["mp_at"])
            assert mp["mp_past"] and all(bmt < m <= bmt + 2 for m in mp["mp_past"])
            at = [cc.family_of(c)[1] for c in one(fam, "halo_at") if sel(c)]
            if fam == "tapconv.gather" or small:
                assert at and all(p["halo"] == maxhalo and p["tile"] == ("small" if small else "big") for p in at)
    past = [cc.family_of(c) for c in cc.CASES if "halo_past" in c.tags and "small" not in c.tags and c.tune.get(13, 0) == 0]
    assert sorted(c.opt["halo"] for c in cc.CASES if "halo_past" in c.tags and "small" not in c.tags and "halo" in c.opt) == [cc.TC_MAXHALO + 1, cc.TC_MAXHALO + 2]
    assert past and all(f == "gemm2.gather" for f, _ in past)
    for c in one("tapconv.conv", "small", "halo_past") + one("tapconv.gather", "small", "halo_past"):
        p = cc.family_of(c)[1]
        assert p["halo"] == cc.TC_MAXHALO_SMALL + 1 and p["tile"] == "big"
    # ragged stages: KC is no multiple of the 128-byte stage; below one stage: KC < the stage
    for c in cc.CASES:
        if c.family.startswith("tapconv"):
            p = cc.family_of(c)[1]
            chs = 128 // cc.esz(c.dt)
            if "ragged_stage" in c.tags:
                assert p["KC"] > chs and p["KC"] % chs
            if "kc_below_stage" in c.tags:
                assert p["KC"] < chs
            if "n_ragged" in c.tags:
                assert p["NE"] % p["BNE"]
    # register-weight kernels: both sides of GW > 32 / GW > 16 and of the halo limits
    gw = sorted(set(c.opt["GW"] for c in cc.CASES if c.family == "rwconv.gather" and "wide" not in c.tags))
    assert gw == [33, cc.RW_MAXHALO[2] - 1] and cc.RW_MAXHALO[3] == 2 * 47 + 2
    assert sorted(set(c.opt["GW"] for c in cc.CASES if "refused" in c.tags and "GW" in c.opt and c.entry == "deconv.fwd")) == [32, 48]
    assert [cc.family_of(c)[1]["halo"] for c in one("rwconv.conv", "halo_at")] == [cc.RC_MAXHALO[(4, 1)], cc.RC_MAXHALO[(4, 2)], cc.RC_MAXHALO[(5, 1)]]
    assert [c.opt["GW"] for c in one("rwconv.conv", "gw_17")] == [17] and [c.opt["GW"] for c in one("tapconv.conv", "gw_16")] == [16]
    # filter gradients: positions against TW_BP, the rounded-up grid, the k = 6 fall-through, the pixels-per-wave cap
    mp = {t: cc.family_of(one("tapwgrad.conv", t)[0])[1]["MP"] for t in ("mp_below", "mp_at", "mp_past")}
    assert mp["mp_below"] == cc.TW_BP - 2 and mp["mp_at"] == cc.TW_BP and mp["mp_past"] == cc.TW_BP + 1
    for c in one("tapwgrad.conv", "grid_rounds_up") + one("tapwgrad.gather4", "grid_rounds_up"):
        p = cc.family_of(c)[1]
        assert p["splits"] > 1 and p["grid_splits"] > p["splits"]
    for c in one("tapwgrad.conv", "one_split"):
        assert cc.family_of(c)[1]["splits"] == 1 and c.tune[9] == 16
    c = one("gen1", "k6_gather")[0]
    assert cc.tapwgrad_plan("gather", c.B, c.IH, c.IW, c.C, *cc.out_hw(c), c.N, 5, cc.knobs_of(c), True) is not None        # (the same layer at k = 5 is taken: 36 > 32 pairs is what refuses k = 6)
    for c in one("narrow_wgrad", "ppw_cap"):
        p = cc.family_of(c)[1]
        OH, OW = cc.out_hw(c)
        ohw, M = OH * OW, c.B * OH * OW
        uncapped = -(-(-(-M // cc.NW_GRID_WAVES)) // cc.NW_BP) * cc.NW_BP
        assert p["capped"] and p["ppw"] == 2 * ohw // cc.NW_BP * cc.NW_BP and ohw % cc.NW_BP != 0 and uncapped > 2 * ohw
        frames = lambda ppw: max((min(M, w * ppw + ppw) - 1) // ohw - (w * ppw) // ohw + 1 for w in range(-(-M // ppw)))
        assert frames(p["ppw"]) == 3                       # a capped wave range straddles the three frames the kernel looks up ...
        assert frames(uncapped) == 4                       # ... and without the cap some range would reach a fourth
        assert c.B * c.IH * c.IW * c.C <= 3 * 1000 * 1000  # 2.5 MB as camera bytes
    for c in one("narrow_wgrad", "ohw_16"):
        assert np.prod(cc.out_hw(c)) == cc.NW_BP
    assert np.prod(cc.out_hw(one("gen1", "ohw_15")[0])) == cc.NW_BP - 1
    assert [int(np.prod(cc.out_hw(c))) for c in one("narrow_conv", "ohw_32") + one("narrow_conv", "ohw_33") + one("gen1", "ohw_31")] == [32, 33, 31]
    assert cc.family_of(one("narrow_conv", "m_below")[0])[1]["M"] < 128 < cc.family_of(one("narrow_conv", "m_past")[0])[1]["M"]
    # gemm2: nk on both sides of 6, gen-1 wgrad: rows on both sides of 64 and of BP
    for c in one("gemm2.conv", "nk_at"):
        assert -(-cc.family_of(c)[1]["K"] * cc.esz(c.dt) // 128) == 6
    for c in one("gemm2.conv", "nk_below"):
        assert -(-cc.family_of(c)[1]["K"] * cc.esz(c.dt) // 128) < 6 and c.tune[20] >= 3
    for c in one("gen1", "wgrad", "m_below_bp"):
        assert cc.family_of(c)[1]["mps"] == cc.WGRAD_BP[c.dt] and cc.family_of(c)[1]["M"] < cc.WGRAD_BP[c.dt] and cc.family_of(c)[1]["splits"] == 1
    assert sorted(c.dt for c in one("gen1", "wgrad", "m_below_bp")) == ["bf16", "f32", "x3"]
    assert [c.k * c.k * c.C for c in one("gen1", "kc_below_64") + one("gen1", "kc_at_64") + one("gen1", "kc_above_64")] == [48, 64, 128]


@pytest.mark.parametrize("c", SMALL, ids=cc.case_id)
def test_references_are_finite_and_masks_are_planted(c):
    d = cc.make_inputs(c)
    td = DT[c.dt][1]
    m = rounded(d["mask"], td).numpy().reshape(-1)
    assert m[0] == 0.0 and m[1] < 0 and m[2] > 0
    if c.family.startswith("refused"):
        return
    r = cc.reference(c, d)
    for name in ("out", "dw", "db"):
        if name in r:
            assert np.isfinite(r[name]).all() and np.abs(r[name]).max() > 0, name
    if c.entry.endswith(".dgrad") and c.opt.get("mask", True):
        open_ = cc.reference(c._replace(opt=dict(c.opt, mask=False)), d)["out"].reshape(-1)
        assert open_[0] != 0 and open_[1] != 0 and r["out"].reshape(-1)[0] == 0 and r["out"].reshape(-1)[1] == 0          # the planted elements decide something
    if "larger_input" in c.tags:
        un = cc.unreached(c)
        assert un.any() and (r["out"][:, un] == 0).all() and np.abs(r["out"][:, ~un]).max() > 0
    if c.entry.endswith(".wgrad"):
        assert r["dw_scale"] > 0 and r["db_scale"] > 0
    if c.opt.get("idx"):
        assert len(set(d["idx"].tolist())) < c.B and d["idx"].max() < c.opt["nframes"]
