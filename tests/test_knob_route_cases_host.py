"""What tests/knob_route_cases.py claims, asserted on the CPU: the ledger partitions the table of csrc/tuning.hip, every file it names really sets the knob, no
value DESIGN.md section 7 names for a knob is left unrun, every step's stated route is what the restated gates of vae_engine_cases.route() give under the step's
knobs, and the layer-op cases under keys 12, 14, 15 and 19 reach the family they state.  A knob added to the table without a test fails here."""
import re

import pytest

import conv_shape_cases as cc
import knob_route_cases as kc
import vae_engine_cases as vc

ROWS = kc.table_rows()


def test_the_table_is_parsed_whole():
    text = open(kc.TUNING_HIP).read()
    assert len(ROWS) == len(re.findall(r"\{K_\w+, (?:nullptr|\"MI355_\w+\"), (?:NOKEY|\d+), ", text)) >= 59
    assert len({r.knob for r in ROWS}) == len(ROWS)
    assert [r.key for r in ROWS if r.key is not None] == list(range(27))                      # the keyed rows come first, the enumerator is the key
    h = cc.header_constants()["DEFAULTS"]
    assert all(h[r.key] == r.default for r in ROWS if r.key is not None)                       # the same defaults conv_shape_cases.py parses
    # every environment name of the table has its line in DESIGN.md section 7, and the section names no row the table lacks
    design = kc.design_rows()
    assert set(design) == {r.knob for r in ROWS}, set(design) ^ {r.knob for r in ROWS}


def test_every_row_is_in_exactly_one_list():
    in_steps = set()
    for s in kc.STEPS.values():
        in_steps |= set(kc.knobs_of_step(s, ROWS))
    lists = {"STEPS": in_steps, "COVERED_ELSEWHERE": set(kc.COVERED_ELSEWHERE), "EXEMPT": set(kc.EXEMPT)}
    known = {r.knob for r in ROWS}
    for name, members in lists.items():
        assert members <= known, (name, members - known)
    for r in ROWS:
        where = [name for name, members in lists.items() if r.knob in members]
        if r.knob in kc.EXEMPT_IN_PART:
            assert where == ["STEPS", "EXEMPT"], (r.knob, where)
        elif "EXEMPT" in where or not where:
            assert where == ["EXEMPT"], "%s: %s" % (r.knob, where or "in no list: a knob without a test")
        # (a knob may be run by a step here AND pinned by another file: the two lists are then both right; what may not happen is a row in neither)
    assert kc.EXEMPT_IN_PART == {"key23"}


def test_exempt_holds_only_the_rows_the_ledger_may_exempt():
    assert set(kc.EXEMPT) == {"key2", "key23", "key25", "MI355_ARES_DBG", "MI355_RWCONV_DBG", "key8", "MI355_PPO_PAD", "MI355_DEBUG_GUARDS"}
    by = {r.knob: r for r in ROWS}
    assert by["key8"].set == "S_IGNORED" and by["MI355_DEBUG_GUARDS"].parse == "P_OFF_PER_CALL"
    for k in ("key2", "key23", "key25", "MI355_ARES_DBG", "MI355_RWCONV_DBG"):
        assert "TIMING" in kc.design_rows()[k], k


@pytest.mark.parametrize("knob", sorted(kc.COVERED_ELSEWHERE))
def test_files_named_as_covering_a_knob_set_it(knob):
    (row,) = [r for r in ROWS if r.knob == knob]
    for fname, where, vals in kc.COVERED_ELSEWHERE[knob]:
        assert where and vals and row.default not in vals, (knob, fname)
        if knob == "MI355_TAPCONV":                          # environment only, stored as key 1 = -1: the file pins that key
            (row1,) = [r for r in ROWS if r.key == 1]
            assert kc.file_sets_knob(fname, row1._replace(env=None))
            continue
        assert kc.file_sets_knob(fname, row), (knob, fname)
    # a file that does not mention the knob is caught
    assert not kc.file_sets_knob("philox_ref.py", row)


def test_no_named_value_is_left_unrun():
    run = kc.values_run(ROWS)
    design = kc.design_rows()
    for knob, pat in kc.NAMED_IN_TEXT.items():
        assert re.search(pat, design[knob]), (knob, design[knob])                              # NAMED is what the section's line says
    assert set(kc.NAMED) == set(kc.NAMED_IN_TEXT)
    missing = {}
    for r in ROWS:
        if r.knob in kc.EXEMPT and r.knob not in kc.EXEMPT_IN_PART:
            continue
        need = kc.named_values(r) if r.knob not in kc.EXEMPT_IN_PART else set()
        if need - run.get(r.knob, set()):
            missing[r.knob] = sorted(need - run.get(r.knob, set()))
    assert not missing, missing
    # the issue's examples
    assert {0, 1, 2} <= run["MI355_RWCONV_CONV"] and {5, 6} <= run["MI355_NW_DEPTH"] and {1, 2, 3} <= run["MI355_ARES_CFG"]
    by = {r.knob: r for r in ROWS}
    assert kc.named_values(by["MI355_RWCONV_CONV"]) == {0, 1, 2} and kc.named_values(by["MI355_TW_LDEC"]) == {1, 2, 3} and kc.named_values(by["MI355_ENCHEAD"]) == {0}


def test_the_steps_are_the_ones_the_work_set_out():
    ids = set(kc.STEPS)
    assert {"enc12_0", "enc12_ring_0", "enc12_c2_0", "enc12_ring_c2_0", "enchead_0", "relu_bits_0", "narrow_0", "dectail_0", "dectail_edge_0", "ares_0", "ares_mid_0",
            "ares_cfg_1", "ares_cfg_2", "ares_cfg_3", "rwconv_2_ares_mid_0", "rwconv_0", "rwconv_wide_0", "slab_bf16_0", "bwd_streams_0", "dp_open_join_0",
            "dp_open_join_0_bwd_streams_0", "latent_split_1", "latent_split_5", "latent_split_32", "reduce_ry_cap_1", "reduce_ry_cap_64", "gemm2_remap3_0", "nw_waves_4",
            "key12_0", "key14_0", "key15_0", "key15_1", "key15_2", "key19_5", "key19_6", "enc12_forms", "ppo_streams_1"} <= ids
    for s in kc.ENGINE_STEPS:
        assert s.runs and all(cid in (1, 7, 8) for _, cid, _ in s.runs), s.id                  # existing cases only
        assert all(k.startswith("MI355_") for k in s.env)
    guards = {s.id for s in kc.ENGINE_STEPS if s.guards}
    assert guards == {"enc12_0", "narrow_0", "relu_bits_0", "dectail_0", "ares_0", "ares_mid_0", "latent_split_1", "latent_split_5", "latent_split_32"}
    # the decoder tail's edge = 0 form: the same tiling on every legal model (deconv3's output side 8 e + 15 is odd), another one at the op level where IH is a multiple of 8
    DT_TY, DT_TX = 8, 16
    assert "constexpr int DT_TY = %d" % DT_TY in open(cc.CSRC + "/dectail_tile.hpp").read() and "DT_TX = %d" % DT_TX in open(cc.CSRC + "/dectail_tile.hpp").read()
    for c in vc.CASES:
        h3, w3, _ = vc.geom(c)["dec"][3]
        assert -(-h3 // DT_TY) == -(-(h3 + 1) // DT_TY) and -(-w3 // DT_TX) == -(-(w3 + 1) // DT_TX), c.id
    changed = [(B, IH, IW) for B, IH, IW in kc.DECTAIL_EDGE_OP_SHAPES if -(-IH // DT_TY) != -(-(IH + 1) // DT_TY) or -(-IW // DT_TX) != -(-(IW + 1) // DT_TX)]
    assert changed == [(2, 8, 15), (1, 16, 33)] and all((3 * (2 * IW + 2)) % 4 == 0 for _, _, IW in kc.DECTAIL_EDGE_OP_SHAPES)
    assert {s.id for s in kc.STEPS.values() if s.digest == "equal"} == {"enc12_ring_0", "enc12_c2_0", "enc12_ring_c2_0", "ares_cfg_1", "ares_cfg_2", "ares_cfg_3", "bwd_streams_0", "dectail_edge_0",
                                                                      "dp_open_join_0", "dp_open_join_0_bwd_streams_0", "gemm2_remap3_0", "ppo_streams_1", "ppo_streams_1_fused_0"}
    # the tensors a digest-equal step may still move: the one-queue backward's own reduce kernels for the fused tail and the fused head backward, bf16 only
    assert set(kc.DIGEST_EXCEPT) == {"bwd_streams_0", "dp_open_join_0_bwd_streams_0"}
    for exc in kc.DIGEST_EXCEPT.values():
        assert exc == {"bf16": ("vae/decoder/deconv4/kernel", "vae/encoder/conv1/kernel", "vae/encoder/conv1/bias")}
    src = open(cc.CSRC + "/conv_ops.hip").read() + open(cc.CSRC + "/enchead.hip").read() + open(cc.CSRC + "/vae_engine.hip").read()
    assert "if (small_of(ctx)) return mi_reduce_slabs((hipStream_t)stream, (const float*)scratch, (long long)DT_SLAB, n_partial, (long long)DT_SLAB, dw, 0, ctx->small);" in src
    assert "MI_LAUNCH(enchead_reduce_kernel, dim3(49), dim3(1024), 0, st, (const float*)q.slabs, nblocks, dw1, db1);" in src
    assert "MiWgradCtx cx = {defer ? &tiled : nullptr, (fork && part != 0 && W.scratch_tail_bytes > 0 && e->tm.mode != 1) ? &side_sums : nullptr, 0, 1};" in src


def test_ppo_reference_trunk_cases():
    import ppo_shape_cases as pc
    assert kc.PPO_REF_TRUNK["A3-33"] == pc.ENGINE_CASES["A3-33"] and sorted(v[3] for v in kc.PPO_REF_TRUNK.values()) == [5, 33]
    for name, args in kc.PPO_REF_TRUNK.items():
        assert (args[0], args[2]) == pc.REF and args[1] == 3, name
    c = pc.build(*kc.PPO_REF_TRUNK["R3-5"])
    assert pc.conditions_met(c.cond), c.cond
    assert pc.PER_LAYER_CASES == ["C100-5", "C100-77", "C67-5", "C67-77"]
    assert {s.id for s in kc.ENGINE_STEPS if s.dp} == {"bwd_streams_0", "dp_open_join_0", "dp_open_join_0_bwd_streams_0"}
    assert [s.id for s in kc.ENGINE_STEPS if s.slab == "fp32"] == ["slab_bf16_0"]
    # uint8 tables need the narrow kernels; the steps whose knob acts on camera bytes only ask for them
    assert all(u8 is False for _, _, u8 in kc.STEPS["narrow_0"].runs)
    for i in ("enc12_ring_0", "enc12_c2_0", "enc12_ring_c2_0", "enchead_0"):
        assert all(u8 is True for _, _, u8 in kc.STEPS[i].runs), i


@pytest.mark.parametrize("sid", [s.id for s in kc.ENGINE_STEPS])
def test_stated_route_is_the_gates_under_the_steps_knobs(sid):
    s = kc.STEPS[sid]
    assert not kc.route_failures(s)
    for precision, cid, _ in s.runs:
        want, base = kc.stated_route(s, precision, cid)
        assert vc.route_tuple(base) == (vc.STATED_BF16 if precision == "bf16" else vc.STATED_F32)[cid]         # the default is the row's written-down route
        assert (want != base) == bool(s.route.get((precision, cid))), (sid, precision, cid)


def test_route_defaults_are_todays_behaviour():
    for c in vc.CASES + [vc.Z12]:
        for p in vc.PRECISIONS:
            for training in (True, False):
                a = vc.route(c, p, training=training)
                assert a == vc.route(c, p, training=training, env={}) == vc.route(c, p, training=training, env={"MI355_BWD_STREAMS": "0", "MI355_LATENT_SPLIT": "16", "MI355_ENC12": "1"})
                assert a == vc.route(c, p, training=training, env={"MI355_LATENT_SPLIT": "33"}) == vc.route(c, p, training=training, env={"LATENT_SPLIT": 0})   # out of range: the default
    assert vc.route_knobs({"MI355_ENC12": "00", "ARES": 2, "MI355_DECTAIL": ""}) == dict(vc.ROUTE_KNOBS, ENC12=0)            # P_ON: off only for a first character '0'
    r = kc.table_rows()
    by = {x.knob: x for x in r}
    for name, default in vc.ROUTE_KNOBS.items():
        assert by["MI355_" + name].default == default and by["MI355_" + name].parse == ("P_RANGE" if name == "LATENT_SPLIT" else "P_ON"), name
    assert (by["MI355_LATENT_SPLIT"].lo, by["MI355_LATENT_SPLIT"].hi) == (1, 32)


def test_route_restates_the_sources_gates():
    """The knob terms of route() next to the source lines they restate: a gate that gains or loses a knob fails here."""
    src = {n: open(cc.CSRC + "/" + n).read() for n in ("enc12.hip", "enchead.hip", "ares.hip", "conv_ops.hip", "vae_engine.hip")}
    assert "return knob(K_ENC12) && knob(K_NARROW) && dtype == MI_BF16" in src["enc12.hip"]
    assert "if (!knob(K_ENCHEAD) || !knob(K_NARROW) || dtype != MI_BF16 || !bits_act1" in src["enchead.hip"]
    assert "if (!knob(K_ARES) || dtype != MI_BF16" in src["ares.hip"] and "if (!knob(K_ARES_MID)) return MI_OK;" in src["ares.hip"]
    assert "const bool ok = knob(K_ARES) && d.dtype == MI_BF16" in src["vae_engine.hip"]
    assert "const bool tail_try = knob(K_DECTAIL) && want_grad" in src["vae_engine.hip"]
    assert "if (!knob(K_DECTAIL) || !knob(K_NARROW) || dtype != MI_BF16 || Cin != 32 || Cout != 3" in src["conv_ops.hip"]
    assert "if (!knob(K_NARROW) || mask || 4 * N > 32" in src["conv_ops.hip"]                    # try_gather_narrow: the loss epilogue
    assert "if (!knob(K_NARROW) || Cout != 32 || KH != KW || KH > 4) return 0;" in src["conv_ops.hip"]      # try_narrow_conv
    assert src["vae_engine.hip"].count("knob(K_RELU_BITS)") == 3
    assert "if (ns > knob(K_LATENT_SPLIT)) ns = knob(K_LATENT_SPLIT);" in src["vae_engine.hip"]


def test_a_misstated_step_fails():
    """Deliberately wrong statements of a step's route are caught: MI355_ENCHEAD=0 claiming a fused head backward; MI355_ENC12=0 claiming that the head backward
    falls back too; MI355_NARROW=0 forgetting the decoder tail; a claimed change that is the default; MI355_LATENT_SPLIT=5 claiming 5 slices on the smallest model."""
    s = kc.STEPS["enchead_0"]
    assert not kc.route_failures(s)
    bad = kc.route_failures(s, route={})                     # "nothing changes": the head backward stays fused
    assert {b[3] for b in bad} == {"head_bwd", "pair_launch"} and all("'fused'" in b[4] or "True" in b[4] for b in bad), bad
    bad = kc.route_failures(kc.STEPS["enc12_0"], route={("bf16", 7): {"enc_head": "two launches", "head_bwd": "layer ops", "pair_launch": False}})
    assert {b[3] for b in bad} == {"head_bwd", "pair_launch"}, bad
    narrow = kc.STEPS["narrow_0"]
    forgot = {k: {f: v for f, v in d.items() if f not in ("tail", "stream_mask")} for k, d in narrow.route.items()}
    assert {b[3] for b in kc.route_failures(narrow, route=forgot)} == {"tail", "stream_mask"}
    bad = kc.route_failures(kc.STEPS["ares_cfg_1"], route={("bf16", 7): {"ares": "on+mid"}})
    assert len(bad) == 1 and "is the default" in bad[0][4], bad
    ls = kc.STEPS["latent_split_5"]
    wrong = dict(ls.route)
    wrong[("bf16", 1)] = {"ns_heads": 5, "ns_dz": 5}
    assert {(b[1], b[2], b[3]) for b in kc.route_failures(ls, route=wrong)} == {("bf16", 1, "ns_heads"), ("bf16", 1, "ns_dz")}


OP_CASES = [(sid, c) for sid, cases in kc.KNOB_OP_CASES.items() for c in cases]


@pytest.mark.parametrize("sid,c", OP_CASES, ids=["%s-%s" % (sid, kc.op_case_id(c)) for sid, c in OP_CASES])
def test_layer_op_cases_reach_the_family_they_state(sid, c):
    fam, plan = cc.family_of(c)
    assert fam == c.family
    (base,) = [b for b in cc.CASES if b.id == c.id]
    key, value = (int(x) for x in sid[3:].split("_"))
    assert cc.knobs_of(c)[key] == value != cc.header_constants()["DEFAULTS"][key] and {k: v for k, v in c.tune.items() if k != key} == {k: v for k, v in base.tune.items() if k != key}
    assert (c.entry, c.dt, c.B, c.IH, c.IW, c.C, c.N, c.k, c.opt) == (base.entry, base.dt, base.B, base.IH, base.IW, base.C, base.N, base.k, base.opt)      # no new shape
    if key == 14:                                           # at the default these take the class-wave kernel: k = 5, C = 64, NE = 4 N = 128, slabs
        assert c.k == 5 and c.C == 64 and 4 * c.N == 128 and plan["slabs_possible"] and plan["splits"] > 1 and c.opt["scratch"] == "exact"
    if key == 12:
        assert c.entry.endswith(".dgrad") and c.opt.get("mask", True)
    if key == 19:
        assert c.opt["frames"] == "u8" and c.opt["dbias"] and (c.k, c.C, c.N) == (4, 3, 32)
    if key == 15:
        assert base.family == "rwconv.conv" and (fam == "rwconv.conv") == (c.k == 5 and value >= 1 or c.k == 4 and c.C == 32 and c.entry == "conv.fwd" and value >= 2)


def test_layer_op_case_lists():
    n = {sid: len(cases) for sid, cases in kc.KNOB_OP_CASES.items()}
    assert n == {"key14_0": 3, "key12_0": len([c for c in cc.CASES if c.family.startswith("tapconv") and "mask" in c.tags]), "key15_0": 4, "key15_1": 4, "key15_2": 4,
                 "key19_5": 2, "key19_6": 2}, n
    assert n["key12_0"] >= 6
    fams = lambda sid: sorted(c.family for c in kc.KNOB_OP_CASES[sid])      # noqa: E731
    assert fams("key15_0") == ["tapconv.conv"] * 4 and fams("key15_1").count("rwconv.conv") == 1 and fams("key15_2").count("rwconv.conv") == 3
    # one uint8 case below a wave range's worth of pixels per wave, one whose ranges are capped at three frames
    plans = [cc.family_of(c)[1] for c in kc.KNOB_OP_CASES["key19_5"]]
    assert sorted(p["capped"] for p in plans) == [False, True] and min(p["nwave"] for p in plans) < 12 < max(p["nwave"] for p in plans)
    assert list(kc.ENC12_FORMS.values()) == [4096, 4096 | 8192, 4096 | 16384, 4096 | 8192 | 16384]
