"""The ledger of the tuning knobs (csrc/tuning.hip) and the steps of test_zzzzzzzzzzzz_knob_routes_gpu.py (test infrastructure; imports no GPU): every row of the
table is run off its default by a step below (STEPS), by another test file (COVERED_ELSEWHERE), or is exempt for a stated reason (EXEMPT).
test_knob_route_cases_host.py asserts that the three lists partition the table -- a knob added tomorrow without a test fails there -- and that every step's stated
route is what vae_engine_cases.route() gives under the step's knobs.

A knob's id is its environment name, or `key<N>` for a row that has none.

A step = one setting of one or more knobs and what runs under it:
  kind 'engine'  a child process (tests/knob_route_worker.py) started with the step's environment: the ConvVAE engine on existing cases of vae_engine_cases.py;
  kind 'op'      in the test's own process, dispatch pinned with mi_set_tuning: layer-op cases (KNOB_OP_CASES below, shapes of conv_shape_cases.py) or the four
                 product forms of the fused encoder head;
  kind 'ppo'     a child process: the PPO per-layer step on two streams.
`route` states, per (precision, case), the fields of vae_engine_cases.route() the step CHANGES and their new values; every other field keeps its default value.
`digest`: 'equal' -- the child's SHA-256 of (losses, gradient buffer, parameters after Adam) equals the default process's, asserted: the knob moves work between
queues or blocks and changes no kernel's accumulation order and no reduction's (the reason names the source lines); 'bound' -- another kernel or another order of
sums: the float64 bound stands alone (whether the digest happened to be equal is printed, not asserted)."""
import collections
import os
import re

import conv_shape_cases as cc
import vae_engine_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TUNING_HIP = os.path.join(cc.CSRC, "tuning.hip")
DESIGN_MD = os.path.join(ROOT, "DESIGN.md")
TESTS = os.path.join(ROOT, "tests")

Row = collections.namedtuple("Row", "knob enum env key default parse set lo hi")


def table_rows(text=None):
    """The rows of tuning.hip's table, in order: Row(knob id, enumerator, environment name or None, key or None, default, parse rule, set rule, lo, hi)."""
    text = open(TUNING_HIP).read() if text is None else text
    body = text[text.index("constexpr Row rows[K_COUNT] = {"):text.index("constexpr bool rows_in_enum_order()")]
    rows = []
    for m in re.finditer(r"^\s*\{(K_\w+), (nullptr|\"\w+\"), (NOKEY|\d+), (-?\d+), (P_\w+)(?:, (S_\w+))?(?:, (-?\w+), (-?\w+))?\}", body, flags=re.M):
        enum, env, key, default, parse, set_, lo, hi = m.groups()
        env = None if env == "nullptr" else env.strip('"')
        key = None if key == "NOKEY" else int(key)
        num = lambda v: None if v is None else (2 ** 31 - 1 if v == "MAXI" else int(v))      # noqa: E731
        rows.append(Row(env or "key%d" % key, enum, env, key, int(default), parse, set_ or "S_NONE", num(lo), num(hi)))
    n_lines = len(re.findall(r"^\s*\{K_\w+,", body, flags=re.M))
    assert len(rows) == n_lines, (len(rows), n_lines)       # a row the pattern does not understand must not drop out of the ledger silently
    return rows


def design_rows(text=None):
    """{knob id: the 'what it selects' text of its line in DESIGN.md section 7} (a line that names several knobs gives each of them its text)."""
    text = open(DESIGN_MD).read() if text is None else text
    sec = text[text.index("## 7. Knobs"):]
    sec = sec[:sec.index("Read by the Python side")]
    out = {}
    for line in sec.splitlines():
        cells = [c.strip() for c in line.strip().strip("|").split("|")]
        if len(cells) != 4 or cells[0] in ("environment", "---"):
            continue
        names = re.findall(r"`(MI355_\w+)`", cells[0])
        if not names:
            names = ["key%d" % int(cells[1])]
        for n in names:
            out[n] = cells[3]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# the non-default values DESIGN.md section 7 names
# ---------------------------------------------------------------------------------------------------------------------------------------
# Written down per knob where section 7 lists values in words; the host test checks each against the section's text (NAMED_IN_TEXT: a pattern the line must hold).
NAMED = {
    "MI355_TAPCONV_MINBLOCKS": (-1,), "key5": (1, 2), "key10": (4, 8), "MI355_GEMM2_TILE": (0, 1, 3), "MI355_NW_DEPTH": (5, 6), "MI355_GEMM2_STAGES": (3, 4),
    "MI355_X3_TAPWGRAD": (0, 2), "MI355_DWG_NST": (4,), "MI355_ARES_CFG": (1, 2, 3),
}
NAMED_IN_TEXT = {
    "MI355_TAPCONV_MINBLOCKS": r"-1 \(any negative", "key5": r"1 big .*2 small", "key10": r"\(4 / 8 / 12\)", "MI355_GEMM2_TILE": r"0 auto .*1 always 64 x 64.*3 always 128 x 128",
    "MI355_NW_DEPTH": r"\(3 / 5 / 6\)", "MI355_GEMM2_STAGES": r"\(2 / 3 / 4\)", "MI355_X3_TAPWGRAD": r"0 off, 1 conv2 / conv3, 2 every", "MI355_DWG_NST": r"4 for exactly 4",
    "MI355_ARES_CFG": r"bit 0 conv, bit 1 gather",
}


def named_values(row):
    """The non-default values a row's knob must be run at: the other side of an on / off switch, every value of a range of at most four (keys 13, 15, 24), and NAMED."""
    vals = set(NAMED.get(row.knob, ()))
    if row.parse in ("P_ON", "P_OFF", "P_OFF_PER_CALL") or row.set == "S_BOOL":
        vals.add(1 - row.default)
    if row.lo is not None and row.hi is not None and row.hi - row.lo <= 3:
        vals |= set(range(row.lo, row.hi + 1))
    vals.discard(row.default)
    return vals


# ---------------------------------------------------------------------------------------------------------------------------------------
# EXEMPT: rows no test runs off their default, and why
# ---------------------------------------------------------------------------------------------------------------------------------------
EXEMPT = {
    "key2": "timing mask of the filter-gradient / tapconv kernels: results are wrong by construction",
    "key23": "timing mask of the fused encoder-head forward kernel: wrong by construction without bit 4096 (with it -- pick a product form -- the step enc12_forms runs it)",
    "key25": "timing mask of the decoder tail: wrong by construction",
    "MI355_ARES_DBG": "timing mask of the activation-resident kernels: wrong by construction",
    "MI355_RWCONV_DBG": "timing variants of the deconv3-forward register-weight kernel: wrong by construction",
    "key8": "removed knob: the key answers 0 and changes nothing",
    "MI355_PPO_PAD": "read only by probe builds (-DMI355_PPO_PAD_PROBE)",
    "MI355_DEBUG_GUARDS": "the guard mode itself: the guard tests and this file's guard steps run under it",
}
EXEMPT_IN_PART = {"key23"}      # exempt as a timing mask, run by a step as the form selector (bit 4096): the one row that is in two lists

# ---------------------------------------------------------------------------------------------------------------------------------------
# COVERED_ELSEWHERE: knob -> [(test file, case / test that sets it off its default, values)]
# ---------------------------------------------------------------------------------------------------------------------------------------
COVERED_ELSEWHERE = {
    "MI355_GEMM2": [("conv_shape_cases.py", "GENERATIONS['gen1'] (key 0 = 0): every first-generation case of test_x_conv_shapes_gpu.py", (0,))],
    "MI355_TAPCONV_MINBLOCKS": [("conv_shape_cases.py", "GENERATIONS['gen1'] / GEMM2 (key 1 = -1), 'newest' (key 1 = 1)", (-1, 1))],
    "MI355_TAPCONV": [("conv_shape_cases.py", "stored as key 1 = -1 (tuning.hip fill_from_environment; parse: test_tuning_host.py): GENERATIONS['gen1'] / GEMM2", (0,))],
    "MI355_TAPWGRAD": [("conv_shape_cases.py", "GENERATIONS['gen1'] (key 3 = 0)", (0,))],
    "MI355_NARROW": [("conv_shape_cases.py", "GENERATIONS['gen1'] (key 4 = 0)", (0,))],
    "key5": [("conv_shape_cases.py", "TAP_BIG (key 5 = 1), TAP_SMALL (key 5 = 2)", (1, 2))],
    "key6": [("conv_shape_cases.py", "tune(TAP_BIG, k6=0): lds_epilogue cases", (0,))],
    "key7": [("conv_shape_cases.py", "tune(TW, k9=64, k7=0): pair_layout cases", (0,))],
    "key9": [("conv_shape_cases.py", "tune(TW, k9=16 | 64)", (16, 64))],
    "key10": [("conv_shape_cases.py", "tune(NAR, k10=4 | 8): waves4 / waves8 cases", (4, 8))],
    "MI355_DENSE_WGRAD_BLOCKS": [("dense_shape_cases.py", "k11=1 | 16 | 1024", (1, 16, 1024))],
    "MI355_RWCONV": [("conv_shape_cases.py", "GENERATIONS['rwconv'] (key 13 = 2), 'gen1' / 'newest' (key 13 = 0)", (0, 2))],
    "MI355_RWCONV_BLOCKS": [("conv_shape_cases.py", "tune(GENERATIONS['rwconv'], k16=1 | 2)", (1, 2))],
    "MI355_GEMM2_TILE": [("conv_shape_cases.py", "tune(GEMM2, k17=1 | 3)", (1, 3)), ("dense_shape_cases.py", "k17=0 | 1 | 3", (0, 1, 3))],
    "key18": [("conv_shape_cases.py", "tune(TW, k9=64, k18=1): slab_bf16 cases", (1,))],
    "MI355_GEMM2_STAGES": [("conv_shape_cases.py", "tune(GEMM2, k20=3 | 4)", (3, 4))],
    "MI355_X3_TAPWGRAD": [("conv_shape_cases.py", "tune(TW, k9=64, k21=2): x3_split", (2,)), ("test_ops_gpu.py", "mi_set_tuning(21, 2); key 21 = 0: every split-storage case of GENERATIONS['gen1']", (0, 2))],
    "MI355_DWGS": [("test_ops_gpu.py", "mi_set_tuning(22, 0)", (0,))],
    "MI355_TW_LDEC": [("test_x_conv_shapes_gpu.py", "the `decodes` cases: mi_set_tuning(24, mode) for mode in (0, 3)", (3,)),
                      ("test_ops_gpu.py", "test of the per-wave DMA-row decode: mi_set_tuning(24, mode), modes 1, 2, 3", (1, 2, 3))],
    "MI355_DECTAIL_SPLIT5": [("test_ops_gpu.py", "mi_set_tuning(26, mode)", (1,))],
    "MI355_GEMM2_SPLITK": [("test_zzz_dense_shapes_gpu.py", "dense_knob_worker.py child with MI355_GEMM2_SPLITK=0", (0,))],
    "MI355_NARROW_LEAN": [("test_x_conv_shapes_gpu.py", "narrow_lean_worker.py child with MI355_NARROW_LEAN=0", (0,))],
    "MI355_TALLK": [("test_zzz_dense_shapes_gpu.py", "dense_knob_worker.py child with MI355_TALLK=0", (0,))],
    "MI355_DWG": [("test_zzz_dense_shapes_gpu.py", "dense_knob_worker.py child with MI355_DWG=0", (0,))],
    "MI355_DWG_NST": [("test_zzz_dense_shapes_gpu.py", "dense_knob_worker.py child with MI355_DWG_NST=4", (4,))],
    "MI355_REPARAM_WIDE": [("test_w_vae_elementwise_gpu.py", "reparam_wide_worker.py child with MI355_REPARAM_WIDE=1", (1,))],
    "MI355_PPO_FUSED": [("test_j_ppo_bf16x3_gpu.py", "child with MI355_PPO_FUSED=0", (0,))],
    "MI355_MLP_STREAMS": [("test_zzzzzzzz_mlp_engine_shapes_gpu.py", "mlp_engine_worker.py child with MI355_MLP_STREAMS=0", (0,))],
}


def file_sets_knob(fname, row):
    """A test file really sets the knob: it holds the knob's environment name, a mi_set_tuning(key, ..) call, a k<key>= preset of conv_shape_cases.tune(), or an entry
    `key: value` / `(key, value)` of a preset that Tuning() hands to mi_set_tuning (GENERATIONS of conv_shape_cases.py, the pairs of test_ops_gpu.py)."""
    text = open(os.path.join(TESTS, fname)).read()
    if row.env and re.search(r"\b%s\b" % row.env, text):
        return True
    if row.key is None:
        return False
    k = row.key
    pats = (r"mi_set_tuning\(%d, " % k, r"\bk%d=-?\d" % k, r"[{,] ?%d: -?\d+[,}]" % k, r"\(\(?%d, -?\w+\)" % k)
    return any(re.search(p, text) for p in pats)


# ---------------------------------------------------------------------------------------------------------------------------------------
# layer-op cases under keys 12, 14, 15 and 19 (test_zzzzzzzzzzzz_knob_routes_gpu.py runs them with test_x_conv_shapes_gpu.py's own runners and bounds).
# Each is an EXISTING case of conv_shape_cases.CASES (same shape, seed and reference) under one more tune(..) preset; `family` is what the predicates give under it.
# ---------------------------------------------------------------------------------------------------------------------------------------
def _one(family, *tags, **opt):
    got = [c for c in cc.CASES if c.family == family and set(tags) <= set(c.tags) and all(c.opt.get(k) == v for k, v in opt.items())]
    assert got, (family, tags, opt)
    return got


def _retuned(c, family, **kw):
    return c._replace(tune=cc.tune(c.tune, **kw), family=family)


KNOB_OP_CASES = collections.OrderedDict()      # step id -> [Case]
# key 14 = 0: the k = 5 filter gradient of 64 -> 32 channels on the pair layout instead of the class-wave kernel (conv_ops.hip: K_TAPWGRAD_CW && KH == 5 && C == 64 && slabs):
# the cases that take the class-wave kernel at the default are the C = 64 ones with slabs (several splits, scratch exact)
KNOB_OP_CASES["key14_0"] = [_retuned(c, "tapwgrad.gather5", k14=0) for c in _one("tapwgrad.gather5") if c.C == 64 and c.opt.get("scratch") == "exact" and not c.opt.get("slab_bf16")]
# key 12 = 0: tapconv without the mask-line prefetch, on every masked tapconv case
KNOB_OP_CASES["key12_0"] = [_retuned(c, c.family, k12=0) for c in cc.CASES if c.family.startswith("tapconv") and "mask" in c.tags]
# key 15 = 0, 1, 2 on the register-weight conv-form cases: 0 none of them, 1 the k = 5 layer, 2 also 32 -> 64 k = 4; the rest falls to tapconv
_RC = _one("rwconv.conv")


def _rc_family(c, on):
    wide = (c.C, c.N) == (64, 128) or (c.entry == "deconv.dgrad" and (c.N, c.C) == (64, 128))
    taken = (c.k == 5 and on >= 1) or (c.k == 4 and not wide and on >= 2) or (c.k == 4 and wide and on >= 3)
    return "rwconv.conv" if taken else "tapconv.conv"


for _on in (0, 1, 2):
    KNOB_OP_CASES["key15_%d" % _on] = [_retuned(c, _rc_family(c, _on), k15=_on) for c in _RC]
# key 19 = 5, 6: narrow_wgrad_kernel<unsigned char, 3, 1, 12, DEPTH> on the uint8 filter-gradient cases (4 x 4 x 3 -> 32 with dbias): one below a wave range
# (3 x 16 pixels) and the 5900-frame one whose ranges are capped at three frames
_NW_U8 = [c for c in _one("narrow_wgrad", "frames_u8") if c.opt.get("dbias")]
for _depth in (5, 6):
    KNOB_OP_CASES["key19_%d" % _depth] = [_retuned(c, "narrow_wgrad", k19=_depth) for c in _NW_U8]


def op_case_id(c):
    return "%03d-%s-%s-%s" % (c.id, c.entry, "_".join(c.tags[:2]), "_".join("k%d=%d" % kv for kv in sorted(c.tune.items()) if kv[0] in (12, 14, 15, 19)))


# the four product forms of the fused encoder head on camera bytes, picked in-process by key 23 = 4096 | 8192 ring | 16384 pipelined conv2 (enc12.hip)
ENC12_FORMS = collections.OrderedDict([("compiler-scheduled", 4096), ("ring", 4096 | 8192), ("c2 asked without ring", 4096 | 16384), ("ring + c2", 4096 | 8192 | 16384)])
ENC12_BATCHES = (1, 2, 3, 5)

# ---------------------------------------------------------------------------------------------------------------------------------------
# STEPS
# ---------------------------------------------------------------------------------------------------------------------------------------
Step = collections.namedtuple("Step", "id kind env keys runs route guards digest dp slab extra why")
ALL3, BF16 = ("fp32", "bf16x3", "bf16"), ("bf16",)
STEPS = collections.OrderedDict()


def step(id_, env=None, runs=(), route=None, guards=False, digest="bound", dp=False, slab="bf16", keys=None, kind="engine", extra=(), why=""):
    """runs: ((precision, case id, u8), ..) -- u8: None (the helper's own rule: cases 1 and 7 also run on uint8 tables), True, or False (float tables only)."""
    assert id_ not in STEPS and digest in ("equal", "bound") and why
    env = {("MI355_" + k): str(v) for k, v in (env or {}).items()}
    if guards:
        env["MI355_DEBUG_GUARDS"] = "1"
    STEPS[id_] = Step(id_, kind, env, dict(keys or {}), tuple(runs), dict(route or {}), guards, digest, dp, slab, tuple(extra), why)


def runs(precisions, cases, u8=None):
    return tuple((p, c, u8) for p in precisions for c in cases)


HEAD_OPS = {"head_bwd": "layer ops", "pair_launch": False}
step("enc12_0", {"ENC12": 0}, runs(BF16, (7,)), {("bf16", 7): {"enc_head": "two launches"}}, guards=True,
     why="conv1 and conv2 as two launches, the head backward still fused (conv1's narrow kernel writes the bit words); the engine sizes has_act1 by the same knob")
for _id, _env in (("enc12_ring_0", {"ENC12_RING": 0}), ("enc12_c2_0", {"ENC12_C2": 0}), ("enc12_ring_c2_0", {"ENC12_RING": 0, "ENC12_C2": 0})):
    step(_id, _env, runs(BF16, (7,), u8=True), digest="equal",
         why="training forms of enc12_fwd_kernel on camera bytes: the knobs schedule the frame loads and conv2's LDS reads (enc12_tile.hpp), every MFMA keeps its operands and "
             "its place in the k loop; act1 and the bit words are stated bitwise by enc12.hip, act2 follows from the unchanged loop order")
step("enchead_0", {"ENCHEAD": 0}, runs(BF16, (7,), u8=True), {("bf16", 7): dict(HEAD_OPS)}, extra=("nw_depth",),
     why="head backward as layer ops: conv1's filter gradient on narrow_wgrad_kernel -- on uint8 tables the <unsigned char, 3, 1, 12> forms, key 19 = 3, 5, 6 in turn "
         "(DEPTH moves the prefetch distance; steps past a wave's range add zeros: the three are bitwise equal)")
step("relu_bits_0", {"RELU_BITS": 0}, runs(BF16, (7, 1)), {("bf16", 7): dict(HEAD_OPS, bits1=False), ("bf16", 1): dict(HEAD_OPS, bits1=False)}, guards=True,
     why="no ReLU bit words: the input gradients read the activations as masks, the head backward (which needs the words) runs as layer ops")
_NARROW_OFF = dict(HEAD_OPS, conv1="general", bits1=False, tail="plain", stream_mask=5)
step("narrow_0", {"NARROW": 0}, runs(BF16, (7, 1), u8=False), {("bf16", 7): dict(_NARROW_OFF, enc_head="two launches"), ("bf16", 1): dict(_NARROW_OFF)}, guards=True,
     why="the narrow kernels off: conv1 general, no fused head either way, no fused tail and no loss epilogue -- deconv4, the unfused loss, the chunked finalisation "
         "(float tables: uint8 tables need the narrow kernels)")
step("dectail_0", {"DECTAIL": 0}, runs(BF16, (7,)), {("bf16", 7): {"tail": "epilogue", "stream_mask": 5}}, guards=True,
     why="no fused decoder tail: deconv4 with the loss epilogue, dlogits stored, backward from deconv4; read by tail_try and by mi_deconv2d_tail_fused")
step("dectail_edge_0", {"DECTAIL_EDGE": 0}, runs(BF16, (7, 1)), digest="equal", extra=("dectail_edge_op",),
     why="the decoder tail tiled over the slot grid (edge = 0, conv_ops.hip tiles_y / tiles_x over IH + 1 / IW + 1 instead of IH / IW).  In the ENGINE the two forms "
         "coincide: deconv3's output is (8 e + 15) pixels a side for a frame side of 16 e + 32, never a multiple of the 8 x 16 tile, so both count the same tiles and the "
         "last slot row / column falls inside the last tile either way -- the digest is the default's.  The distinct tiling (IH a multiple of 8: one more tile row, "
         "which holds the last slot row alone) runs at the op level in the same child (DECTAIL_EDGE_OP_SHAPES)")
DECTAIL_EDGE_OP_SHAPES = ((2, 8, 15), (1, 16, 33), (2, 7, 15))      # (B, IH, IW) of test_decoder_tail_fused_equals_the_three_ops: IH = 8, 16 change the tiling, 7 does not (IW must be odd)
step("ares_0", {"ARES": 0}, runs(BF16, (7,)), {("bf16", 7): {"ares": "off"}}, guards=True,
     why="the general tile kernels for conv4 / deconv1; read by ares_eligible (the fragment-ordered copies) and by mi_ares_conv")
step("ares_mid_0", {"ARES_MID": 0}, runs(BF16, (7,)), {("bf16", 7): {"ares": "on"}}, guards=True, extra=("ares_mid_op",),
     why="the mid layers (deconv2 forward, conv3's input gradient) stay on the register-weight kernels: mi_ares_conv form 2 launches nothing and writes nothing")
for _v in (1, 2, 3):
    step("ares_cfg_%d" % _v, {"ARES_CFG": _v}, runs(BF16, (7,)), digest="equal", extra=("ares_op",),
         why="frames per block of the activation-resident kernels (bit 0: ares_conv_kernel<2, 2>, bit 1: ares_gather_kernel<8, 1>): a frame's rows move to another block; "
             "each block walks all 16 taps from tap0 = (b >> 4) & 15 / o0 = (b >> 5) & 7 (ares_tile.hpp), which is 0 for every block while the batch has at most 8 "
             "frame groups -- at batch 3 the order of every sum is the default's")
step("rwconv_2_ares_mid_0", {"RWCONV": 2, "ARES_MID": 0}, runs(BF16, (7,)), {("bf16", 7): {"ares": "on"}},
     why="the mid layers on the register-weight kernels whenever eligible (batch 3 is far below the auto threshold): another kernel, bound only")
step("rwconv_0", {"RWCONV": 0}, runs(BF16, (7,)), why="no register-weight kernel anywhere: tapconv / gemm2 for conv2, conv3, deconv2, deconv3 and their input gradients")
step("rwconv_wide_0", {"RWCONV_WIDE": 0, "RWCONV": 2}, runs(BF16, (7,)), why="the 128 -> 64 channel layers stay on tapconv while the narrower ones take the register-weight kernels")
step("slab_bf16_0", {"SLAB_BF16": 0}, runs(BF16, (7, 1)), slab="fp32",
     why="fp32 partial-sum slabs in the bf16 engine's backward pass: the filter / bias gradient rows take the layer ops' bound, not the bf16-slab allowance")
step("bwd_streams_0", {"BWD_STREAMS": 0}, runs(ALL3, (7, 1)), digest="equal", dp=True,
     why="the one-queue backward (vae_engine.hip: fork = false, defer = false, every layer on scratch region 0, each slab sum behind its own kernel, no pair launch): "
         "the same kernels on the same operands; every split count is a function of the shape")
step("dp_open_join_0", {"DP_OPEN_JOIN": 0}, runs(ALL3, (7, 1)), digest="equal", dp=True, why="the closed joins of the data-parallel step: events only")
step("dp_open_join_0_bwd_streams_0", {"DP_OPEN_JOIN": 0, "BWD_STREAMS": 0}, runs(ALL3, (7, 1)), digest="equal", dp=True, why="both: the data-parallel step on one queue")


def _ls_route(v, ns17, ns1_f32, ns1_bf16):
    """LATENT_SPLIT = v: (ns_heads, ns_dz) of cases 7 and 8 (flat 6144 / 10240: both take the cap itself), of case 1 (flat 256: 16 fp32 K blocks, 8 bf16 ones)."""
    out = {}
    for p in ALL3:
        for cid in (7, 8):
            out[(p, cid)] = {"ns_heads": ns17, "ns_dz": ns17} if ns17 != 16 else {}
        n1, d1 = (ns1_bf16, 8) if p == "bf16" else (ns1_f32, 16)
        out[(p, 1)] = {"ns_heads": n1, "ns_dz": n1} if n1 != d1 else {}
    return out


step("latent_split_1", {"LATENT_SPLIT": 1}, runs(ALL3, (1, 7, 8)), _ls_route(1, 1, 1, 1), guards=True, why="one K slice: the latent layers' sums unsplit; the slab regions are sized by it")
step("latent_split_5", {"LATENT_SPLIT": 5}, runs(ALL3, (1, 7, 8)), _ls_route(5, 5, 4, 4), guards=True,
     why="an odd cap: 5 slices of 6144 / 10240; case 1 (K = 256) has 4, the most whose slices each own a K block of the rounded-up length")
step("latent_split_32", {"LATENT_SPLIT": 32}, runs(ALL3, (1, 7, 8)), _ls_route(32, 32, 16, 8), guards=True, why="the cap of round 4: 32 slices where K allows (case 1 keeps its 16 / 8)")
for _v in (1, 64):
    step("reduce_ry_cap_%d" % _v, {"REDUCE_RY_CAP": _v}, runs(("bf16", "bf16x3"), (7,)),
         why="slab-reduce chains per element (conv_ops.hip: ry doubles up to the cap): another grouping of the slabs of one element, another order of sums")
step("gemm2_remap3_0", {"GEMM2_REMAP3": 0}, runs(BF16, (7, 1)), digest="equal", why="dense layers on gemm2: the numbering of the blocks over the XCDs (q.remap3); every block computes the same tile")
step("nw_waves_4", {"NW_WAVES": 4}, runs(BF16, (7, 1)), why="narrow_wgrad's grid sized for 4 waves per CU (no narrow_wgrad launch on the default route of these cases: the next step has one)")
step("nw_waves_4_enchead_0", {"NW_WAVES": 4, "ENCHEAD": 0}, runs(BF16, (7, 1)), {("bf16", 7): dict(HEAD_OPS), ("bf16", 1): dict(HEAD_OPS)},
     why="conv1's filter gradient on narrow_wgrad_kernel with 1024 wave ranges instead of 3072: other pixels per wave, other slabs, another order of sums")
# ---- in-process op steps ----
for _id in KNOB_OP_CASES:
    _k, _v = _id[3:].split("_")
    step(_id, keys={int(_k): int(_v)}, kind="op", why="layer-op cases of conv_shape_cases.py under key %s = %s (KNOB_OP_CASES)" % (_k, _v))
step("enc12_forms", keys={23: 4096}, kind="op", why="key 23 with bit 4096 picks a product form of the fused encoder head by mask (ENC12_FORMS): all four on camera bytes")
# ---- PPO ----
# the reference trunk 67 -> 500 / 300 -> 3 actions on the per-layer path (MI355_PPO_FUSED=0), at M = 5 and 33: name -> arguments of ppo_shape_cases.build.  A3-33 is the
# existing case; R3-5 is the same trunk at M = 5, its seed the first whose float64 reference meets ppo_shape_cases.conditions_met (test_knob_route_cases_host.py)
PPO_REF_TRUNK = collections.OrderedDict([("R3-5", (67, 3, (500, 300), 5, 27, 0.0173)), ("A3-33", (67, 3, (500, 300), 33, 9, 0.0173))])
step("ppo_streams_1", {"PPO_STREAMS": 1}, kind="ppo", digest="equal",
     why="the per-layer PPO step's backward on two streams (ppo_engine.hip, the knob's only reader): the same kernels, the value and policy branches on two queues")
step("ppo_streams_1_fused_0", {"PPO_STREAMS": 1, "PPO_FUSED": 0}, kind="ppo", digest="equal", extra=("ref_trunk",),
     why="the same on the reference trunk, which takes the per-layer path only with the fused step switched off; compared with the one-stream child ppo_fused_0")
step("ppo_fused_0", {"PPO_FUSED": 0}, kind="ppo", extra=("ref_trunk",), why="the one-stream per-layer step on the reference trunk: the other side of ppo_streams_1_fused_0's digests")

ENGINE_STEPS = [s for s in STEPS.values() if s.kind == "engine"]
# Tensors a digest-equal step may still move, per precision, because the SOURCE shows another order of sums for them.  The one-queue backward hands its calls no list of
# small sums (vae_engine.hip: cx.small is NULL unless the pass forks), so the per-block partial sums of the fused decoder tail and of the fused encoder-head backward go
# through dectail_reduce_kernel / enchead_reduce_kernel (32 thread rows, every 32nd slab each) instead of reduce_small_fused_kernel's lanes (conv_ops.hip
# mi_deconv2d_tail_reduce_ctx, enchead.hip): deconv4's filter gradient and conv1's filter and bias gradient, in the bf16 engine only.
_ONE_QUEUE = {"bf16": ("vae/decoder/deconv4/kernel", "vae/encoder/conv1/kernel", "vae/encoder/conv1/bias")}
DIGEST_EXCEPT = {"bwd_streams_0": _ONE_QUEUE, "dp_open_join_0_bwd_streams_0": _ONE_QUEUE}


def knobs_of_step(s, rows=None):
    """{knob id: value} a step sets off its default (MI355_DEBUG_GUARDS, the guard mode, is not a knob under test)."""
    rows = table_rows() if rows is None else rows
    by_env, by_key = {r.env: r for r in rows if r.env}, {r.key: r for r in rows if r.key is not None}
    out = {}
    for name, v in s.env.items():
        if name != "MI355_DEBUG_GUARDS":
            out[by_env[name].knob] = int(v)
    for k, v in s.keys.items():
        out[by_key[k].knob] = v
    if "nw_depth" in s.extra:
        out["MI355_NW_DEPTH"] = (5, 6)
    return out


def values_run(rows=None):
    """{knob id: set of non-default values STEPS and COVERED_ELSEWHERE run it at}."""
    rows = table_rows() if rows is None else rows
    default = {r.knob: r.default for r in rows}
    out = collections.defaultdict(set)
    for s in STEPS.values():
        for knob, v in knobs_of_step(s, rows).items():
            out[knob] |= set(v if isinstance(v, tuple) else (v,))
    for knob, places in COVERED_ELSEWHERE.items():
        for _, _, vals in places:
            out[knob] |= set(vals)
    return {k: {v for v in vs if v != default[k]} for k, vs in out.items()}


def stated_route(s, precision, cid, route=None):
    """(route under the step's knobs as the step STATES it, default route): the default route with the step's stated changes laid over it."""
    c = vc.by_id(cid)
    mb = vc.CREATE_BATCH.get(cid, 128)
    base = vc.route(c, precision, max_batch=mb)
    want = dict(base)
    want.update((s.route if route is None else route).get((precision, cid), {}))
    return want, base


def route_failures(s, route=None):
    """What test_knob_route_cases_host.py asserts of a step's route statement, as a list of failures: the stated route is route(c, precision, env = the step's) field
    by field, and every field the step claims to change differs from the default."""
    bad = []
    for precision, cid, _ in s.runs:
        want, base = stated_route(s, precision, cid, route)
        got = vc.route(vc.by_id(cid), precision, max_batch=vc.CREATE_BATCH.get(cid, 128), env=s.env)
        for k in got:
            if got[k] != want[k]:
                bad.append((s.id, precision, cid, k, "stated %r, the gates give %r" % (want[k], got[k])))
        for k, v in (s.route if route is None else route).get((precision, cid), {}).items():
            if base[k] == v:
                bad.append((s.id, precision, cid, k, "claimed as a change, but %r is the default" % (v,)))
    return bad
