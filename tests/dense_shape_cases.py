"""Cases, float64 references and dispatch predicates for test_zzz_dense_shapes_gpu.py (test infrastructure; imports no GPU): the dense entry points mi_gemm_bias_act and
mi_gemm_wgrad / _ws / _bias_ws / _bias_set / _bias_pair_ws (csrc/conv_ops.hip) OFF the shapes of the three models, at the edges of the launchers' predicates.

A case = one entry ("fwd", "wgrad", "pair"), one storage type, the shape a [M, K], W [K, N] (layout 0) or [N, K] (layout 1), dy [M, N], the split count, the epilogue /
gradient options, the mi_set_tuning settings that pin the dispatch, the kernel family it is meant to reach and the boundary it probes (tags + words).

The predicates below restate the launchers' SHAPE conditions and nothing else (fresh allocations are 16-byte aligned); family_of() applies them in the launchers' order of
trial.  test_dense_shape_cases_host.py asserts that every case's claimed family follows from them and that every constant equals the value parsed out of csrc/.

Families:  dense_smallm | tallk.<N / 32> | gemm2.<BM>x<BN>s<stages>[.splitk] | gen1.n<32|64|128>[.splitk]            (mi_gemm_bias_act, in this order of trial)
           dwg.<stages> | dwgs.<store|add>.w<waves> | gen1w.<64|128>.<single|slabs|atomics>                          (mi_gemm_wgrad_bias_set, in this order of trial)
           pair | pair.two_calls                                                                                    (mi_gemm_wgrad_bias_pair_ws)
           refused:<why>                                                                                            (an error, nothing launched)"""
import collections
import os
import re

import numpy as np

import conv_shape_cases as cc
from conv_shape_cases import ceil_div, esz, gemm2_tile, gen1_wgrad_plan
from hip_helpers import DT, rounded

CSRC = cc.CSRC

# ---------------------------------------------------------------------------------------------------------------------------------------
# constants the cases cite (test_dense_shape_cases_host.py compares them with csrc/)
# ---------------------------------------------------------------------------------------------------------------------------------------
GEMM_BM = 128                            # gemm_tile.hpp: rows per first-generation block
WGRAD_BP = cc.WGRAD_BP                   # wgrad_tile.hpp WgradCfg<T>::BP: rows per first-generation filter-gradient step
SMALLM_MAX_M = 256                       # mi_gemm_bias_act: dense_smallm_kernel takes M <= 256
SMALLM_TILE, SMALLM_KSTEP, SMALLM_WAVES = 32, 8, 4        # gemm2_tile.hpp: 32 x 32 output tile, 8 k per step, four waves split the steps
TALLK_N = (32, 64, 128)                  # mi_gemm_bias_act: the tall-K kernel's output widths
TALLK_GROUP, TALLK_ROWS = 6, 32          # tallk_tile.hpp: k16-steps requested together; rows per block
TALLK_MAX_BYTES = 1 << 30
DWG_TILE, DWG_MIN_TILES, DWG_ROWS = 128, 256, 32          # mi_gemm_wgrad_bias_set / dwg_tile.hpp
DWGS_TILE, DWGS_MAX_KN, DWGS_DEPTH, DWGS_STEP = 64, 262144, 4, 16      # dwgs_eligible / dwgs_tile.hpp
G2_OOB = 0x40000000                      # gemm2_tile.hpp: every tensor a descriptor covers is shorter
SPLITK_BK = {"f32": 16, "bf16": 32, "x3": 16}            # mi_gemm_bias_act: a split's length is a multiple of this many k
ENV_DEFAULTS = {"MI355_TALLK": 1, "MI355_GEMM2_SPLITK": 1, "MI355_DWG": 1, "MI355_DWG_NST": 3}       # knobs the environment alone reaches (read when the library loads)


def source_constants():
    """The same constants parsed out of csrc/: {name: value}."""
    out = {}

    def grab(fname, pats):
        text = open(os.path.join(CSRC, fname)).read()
        for name, pat in pats.items():
            m = re.search(pat, text)
            assert m, (fname, name)
            out[name] = [int(g, 0) for g in m.groups()] if len(m.groups()) > 1 else int(m.group(1), 0)

    grab("gemm_tile.hpp", {"GEMM_BM": r"constexpr int GEMM_BM = (\d+);"})
    grab("wgrad_tile.hpp", {"WG_F32": r"WgradCfg<float>\s*\{ static constexpr int BP = (\d+);", "WG_BF16": r"WgradCfg<bf16_t>\s*\{ static constexpr int BP = (\d+);",
                            "WG_X3": r"WgradCfg<split_t>\s*\{ static constexpr int BP = (\d+);"})
    grab("gemm2_tile.hpp", {"G2_OOB": r"constexpr uint32_t G2_OOB = (0x[0-9a-fA-F]+)u;", "SMALLM_KSTEP": r"const int ksteps = \(p\.K \+ 7\) / (\d+);",
                            "SMALLM_WAVES": r"const int per = \(ksteps \+ 3\) / (\d+);", "SMALLM_TILE": r"const int n0 = blockIdx\.x \* (\d+), m0 = blockIdx\.y \* (\d+);"})
    grab("tallk_tile.hpp", {"TALLK_GROUP": r"constexpr int U = (\d+);", "TALLK_ROWS": r"const int m0 = blockIdx\.x \* (\d+),", "TALLK_STEP": r"const int steps = p\.len >> (\d+);"})
    grab("dwg_tile.hpp", {"DWG_ROWS": r"constexpr int DWG_ROWS = (\d+);", "DWG_TILE": r"const int k0 = kt \* (\d+), n0 = nt \* (\d+);"})
    grab("dwgs_tile.hpp", {"DWGS_DEPTH": r"constexpr int DWGS_DEPTH = (\d+);", "DWGS_TILE": r"const int k0 = kt \* (\d+), n0 = nt \* (\d+);", "DWGS_STEP": r"const int ns = \(p\.M >> (\d+)\) / ws;"})
    grab("conv_ops.hip", {
        "SMALLM_MAX_M": r"nsplit <= 1 && !mask && M <= (\d+) && K % 4 == 0 && knob\(K_GEMM2\)",
        "TALLK_N": r"knob\(K_TALLK\) && \(N == (\d+) \|\| N == (\d+) \|\| N == (\d+)\)",
        "TALLK_KMOD": r"K % \(nsplit \* (\d+)\) == 0",
        "TALLK_MAX": r"\(long long\)M \* K \* 2 < \(1ll << (\d+)\) && \(long long\)N \* K \* 2 < \(1ll << (\d+)\)",
        "SPLITK_BK": r"const int bk = dtype == MI_BF16 \? (\d+) : (\d+);",
        "SPLITK_STAGE": r"\(p\.ksplit_len \* esz_of\(dtype\)\) % (\d+) != 0",
        "DWG_PRED": r"K % (\d+) == 0 && N % (\d+) == 0 && \(long long\)\(K / (\d+)\) \* \(N / (\d+)\) >= (\d+)",
        "DWGS_PRED": r"M >= (\d+) && M % (\d+) == 0 && K % (\d+) == 0 && N % (\d+) == 0 && \(long long\)K \* N <= (\d+)",
        "DWGS_WSPLIT": r"const int steps = M / (\d+);\s*if \(steps % 4 == 0 && steps / 4 >= (\d+)\) return 4;\s*if \(steps % 2 == 0 && steps / 2 >= (\d+)\) return 2;",
        "WIDE_ROWS": r"const bool wide = Kce > (\d+);"})
    assert "launch_wgrad((hipStream_t)stream, dtype, 0, p, knob(K_DENSE_WGRAD_BLOCKS), scratch, scratch_bytes, overwrite, ctx)" in open(os.path.join(CSRC, "conv_ops.hip")).read()
    text = open(os.path.join(CSRC, "tuning.hip")).read()
    out["DEFAULTS"] = {int(m.group(1)): int(m.group(2)) for m in re.finditer(r"^\s*\{K_\w+, (?:nullptr|\"\w+\"), (\d+), (-?\d+), P_", text, flags=re.M)}
    out["ENV_DEFAULTS"] = {m.group(1): int(m.group(2)) for m in re.finditer(r"^\s*\{K_\w+, \"(MI355_\w+)\", NOKEY, (-?\d+), P_", text, flags=re.M)}
    out["DENSE_TARGET_KEY"] = int(re.search(r"\{K_DENSE_WGRAD_BLOCKS, \"MI355_DENSE_WGRAD_BLOCKS\", (\d+), (\d+),", text).group(1))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# tuning presets (mi_set_tuning keys; csrc/tuning.hip).  DEFAULTS = what a fresh process holds for the keys the dense launchers read.
# ---------------------------------------------------------------------------------------------------------------------------------------
DEFAULTS = {0: 1, 11: 256, 17: 2, 20: 2, 22: 1}
AUTO = {}
NO_GEMM2 = {0: 0}
NO_DWGS = {22: 0}


def tune(base=None, **kw):
    d = dict(base or {})
    d.update({int(k[1:]): v for k, v in kw.items()})
    return d


def knobs_of(case):
    d = dict(cc.DEFAULTS)
    d.update(DEFAULTS)
    d.update(case.tune)
    return d


Case = collections.namedtuple("Case", "id entry dt M K N layout nsplit tune family tags why opt")
ENTRIES = ("fwd", "wgrad", "pair")


# ---------------------------------------------------------------------------------------------------------------------------------------
# predicates, one per family
# ---------------------------------------------------------------------------------------------------------------------------------------
def smallm_ok(dt, M, K, layout, nsplit, mask, kn):
    """mi_gemm_bias_act, first trial: dense_smallm_kernel."""
    return dt == "f32" and layout == 0 and nsplit <= 1 and not mask and M <= SMALLM_MAX_M and K % 4 == 0 and bool(kn[0])


def smallm_wave_steps(K):
    """k-steps of 8 each of the four waves owns: [steps of wave 0, .., wave 3]."""
    ksteps = ceil_div(K, SMALLM_KSTEP)
    per = ceil_div(ksteps, SMALLM_WAVES)
    return [max(0, min(ksteps, w * per + per) - w * per) for w in range(SMALLM_WAVES)]


def tallk_plan(dt, M, K, N, layout, nsplit, raw, env):
    """mi_gemm_bias_act, second trial: None or {nt, kp, len, steps, grid}.  raw: fp32 slabs wanted, no bias / ReLU / mask."""
    if not (dt == "bf16" and layout == 1 and nsplit > 1 and raw and env["MI355_TALLK"] and N in TALLK_N and K % (nsplit * 16) == 0):
        return None
    if M * K * 2 >= TALLK_MAX_BYTES or N * K * 2 >= TALLK_MAX_BYTES:
        return None
    nt = N // 32
    kp = 4 // nt
    if nsplit % kp:
        return None
    ln = K // nsplit
    return {"nt": nt, "kp": kp, "len": ln, "steps": ln // 16, "grid": (ceil_div(M, TALLK_ROWS), nsplit // kp)}


def splitk_len(dt, K, nsplit):
    """mi_gemm_bias_act: (length of a split, length of the last split); the last is <= 0 when the call is refused (an empty slab)."""
    bk = SPLITK_BK[dt]
    ln = ceil_div(ceil_div(K, nsplit), bk) * bk
    return ln, K - ln * (nsplit - 1)


def gemm2_dense_ok(dt, nsplit, ln, kn, env):
    """try_conv_form_gemm2 on a dense layer (one position per row, stride 1: neither the register-weight nor the tap kernels are asked)."""
    if nsplit > 1 and (not env["MI355_GEMM2_SPLITK"] or (ln * esz(dt)) % 128):
        return False
    return bool(kn[0])


def dwg_ok(dt, M, K, N, overwrite, env):
    """mi_gemm_wgrad_bias_set, first trial: dwg_kernel."""
    return bool(overwrite and env["MI355_DWG"] and dt == "bf16" and M >= 1 and K % DWG_TILE == 0 and N % DWG_TILE == 0 and (K // DWG_TILE) * (N // DWG_TILE) >= DWG_MIN_TILES and
                0 < M * K * 2 < G2_OOB and 0 < M * N * 2 < G2_OOB)


def dwgs_ok(dt, M, K, N, kn):
    """dwgs_eligible."""
    return bool(kn[22] and dt == "bf16" and M >= 16 and M % 16 == 0 and K % DWGS_TILE == 0 and N % DWGS_TILE == 0 and K * N <= DWGS_MAX_KN and M * K < 1 << 31 and M * N < 1 << 31)


def dwgs_wsplit(M):
    """Waves per 64 x 64 tile: each wave keeps at least two load rounds."""
    steps = M // DWGS_STEP
    if steps % 4 == 0 and steps // 4 >= 2:
        return 4
    if steps % 2 == 0 and steps // 2 >= 2:
        return 2
    return 1


def tile_grid(KT, NT):
    """(blocks launched, blocks that return at once) of the XCD-contiguous tile numbering of dwg_kernel / dwgs_kernel."""
    T = KT * NT
    blocks = ceil_div(T, 8) * 8
    return blocks, blocks - T


def gen1w_plan(dt, M, K, N, dbias, kn):
    """prepare_wgrad on a dense layer: gen1_wgrad_plan over the result's rows incl. the bias row, with tuning key 11 as the target block count."""
    kce = K + (1 if dbias else 0)
    return dict(gen1_wgrad_plan(dt, M, kce, N, kn[11]), Kce=kce)


def scratch_bytes(dt, M, K, N, kn):
    """What mi_gemm_wgrad_scratch_bytes must return: the slabs of the launch WITH a bias row; 0 for a single row split."""
    p = gen1_wgrad_plan(dt, M, K + 1, N, kn[11])
    return p["slab_bytes"] if p["splits"] > 1 else 0


def scratch_given(c, kn):
    """Bytes of scratch the case hands over: 'none' 0 | 'exact' mi_gemm_wgrad_scratch_bytes | 'need' the launch's own slabs, to the byte | 'short' 16 bytes less than those."""
    mode = c.opt.get("scratch", "none")
    if mode == "none":
        return 0
    if mode == "exact":
        return scratch_bytes(c.dt, c.M, c.K, c.N, kn)
    need = gen1w_plan(c.dt, c.M, c.K, c.N, c.opt.get("dbias"), kn)["slab_bytes"]
    return need if mode == "need" else need - 16


def wgrad_family(dt, M, K, N, dbias, overwrite, given, kn, env):
    """mi_gemm_wgrad_bias_set's order of trial -> (family, plan)."""
    if dwg_ok(dt, M, K, N, overwrite, env):
        kt, nt = K // DWG_TILE, N // DWG_TILE
        return "dwg.%d" % env["MI355_DWG_NST"], {"KT": kt, "NT": nt, "grid": tile_grid(kt, nt), "stages": ceil_div(M, DWG_ROWS)}
    if dwgs_ok(dt, M, K, N, kn):
        ws = dwgs_wsplit(M)
        kt, nt = K // DWGS_TILE, N // DWGS_TILE
        return "dwgs.%s.w%d" % ("store" if overwrite else "add", ws), {"ws": ws, "ns": M // DWGS_STEP // ws, "KT": kt, "NT": nt, "grid": tile_grid(kt, nt)}
    if K % (8 if dt == "bf16" else 4):
        return "refused:K not a vector multiple", None
    p = gen1w_plan(dt, M, K, N, dbias, kn)
    slabs = p["splits"] > 1 and given >= p["slab_bytes"]
    if overwrite and p["splits"] > 1 and not slabs:
        return "refused:overwrite needs scratch", None
    mode = "single" if p["splits"] == 1 else ("slabs" if slabs else "atomics")
    return "gen1w.%d.%s" % (128 if p["wide"] else 64, mode), p


def family_of(c, env=None):
    """-> (family, plan): the kernel family the entry point's order of trial ends in, with the launch's derived sizes.  env: the environment-only knobs."""
    env = dict(ENV_DEFAULTS, **(env or {}))
    kn = knobs_of(c)
    o = c.opt
    dt, M, K, N = c.dt, c.M, c.K, c.N
    if c.entry == "fwd":
        bias, relu, mask, out_f32 = o.get("bias", False), o.get("relu", False), o.get("mask", False), o.get("out_f32", False)
        if smallm_ok(dt, M, K, c.layout, c.nsplit, mask, kn):
            return "dense_smallm", {"wave_steps": smallm_wave_steps(K), "grid": (ceil_div(N, SMALLM_TILE), ceil_div(M, SMALLM_TILE))}
        raw = out_f32 and not bias and not relu and not mask
        p = tallk_plan(dt, M, K, N, c.layout, c.nsplit, raw, env)
        if p:
            return "tallk.%d" % p["nt"], p
        if K % (8 if dt == "bf16" else 4):
            return "refused:K not a vector multiple", None
        ln, last, gz = 0, 0, 1
        if c.nsplit > 1:
            if not raw:
                return "refused:split-K writes raw fp32 slabs only", None
            ln, last = splitk_len(dt, K, c.nsplit)
            if last <= 0:
                return "refused:empty slab", None
            gz = c.nsplit
        sfx = ".splitk" if c.nsplit > 1 else ""
        plan = {"len": ln, "last": last}
        if c.layout == 1 and gemm2_dense_ok(dt, c.nsplit, ln, kn, env):
            t = gemm2_tile(N, M, gz, K, dt, kn)
            return "gemm2.%dx%ds%d%s" % (t + (sfx,)), dict(plan, tile=t)
        return "gen1.n%d%s" % (32 if N <= 32 else (64 if N <= 64 else 128), sfx), plan
    if c.entry == "wgrad":
        return wgrad_family(dt, M, K, N, o.get("dbias"), o.get("overwrite"), scratch_given(c, kn), kn, env)
    # pair: both problems on the first-generation kernel's bf16 128-row form, or the two single calls
    probs = [(M, K, N, o.get("dbias", True)), tuple(o["second"]) + (o.get("dbias1", True),)]
    ok = dt == "bf16"
    for (m, k, n, db) in probs:
        if not ok:
            break
        if dwgs_ok(dt, m, k, n, kn) or k % 8 or not gen1w_plan(dt, m, k, n, db, kn)["wide"]:
            ok = False
    return ("pair" if ok else "pair.two_calls"), {"plans": [gen1w_plan(dt, m, k, n, db, kn) for (m, k, n, db) in probs]}


# ---------------------------------------------------------------------------------------------------------------------------------------
# inputs and float64 references
# ---------------------------------------------------------------------------------------------------------------------------------------
def make_inputs(c):
    """numpy float32 inputs of a case, from the case's own fixed seed.  Pair cases: the second problem's arrays carry the suffix 1."""
    rng = np.random.RandomState(5000 + c.id)

    def one(M, K, N):
        d = {"a": rng.randn(M, K).astype(np.float32), "w": (rng.randn(K, N) / np.sqrt(K)).astype(np.float32), "b": rng.randn(N).astype(np.float32),
             "mask": cc.plant(rng.randn(M, N).astype(np.float32)) if M * N >= 3 else -np.ones((M, N), np.float32), "dy": rng.randn(M, N).astype(np.float32),
             "dw0": (0.25 * rng.randn(K, N)).astype(np.float32), "db0": (0.25 * rng.randn(N)).astype(np.float32)}
        return d
    d = one(c.M, c.K, c.N)
    if c.entry == "pair":
        d.update({k + "1": v for k, v in one(*c.opt["second"]).items()})
    return d


def slab_ranges(c, env=None):
    """Split-K: the k range [lo, hi) of every slab as the family the case reaches cuts it."""
    fam, plan = family_of(c, env)
    if fam.startswith("tallk"):
        return [(s * plan["len"], (s + 1) * plan["len"]) for s in range(c.nsplit)]
    return [(s * plan["len"], min(c.K, (s + 1) * plan["len"])) for s in range(c.nsplit)]


def reference_fwd(c, d, env=None):
    """{'out': [M, N]} or, split-K, {'out': the unsplit product, 'slabs': [nsplit, M, N]}: float64 on the values the kernel reads."""
    td = DT[c.dt][1]
    o = c.opt
    a, w = rounded(d["a"], td).numpy(), rounded(d["w"], td).numpy()
    y = a @ w
    if c.nsplit > 1:
        return {"out": y, "slabs": np.stack([a[:, lo:hi] @ w[lo:hi] for lo, hi in slab_ranges(c, env)])}
    if o.get("bias"):
        y = y + d["b"].astype(np.float64)
    if o.get("relu"):
        y = np.maximum(y, 0.0)
    if o.get("mask"):
        y = y * (rounded(d["mask"], td).numpy() > 0)
    return {"out": y}


def reference_wgrad(dt, a, dy):
    """(dw [K, N], db [N]) float64: a^T dy and the column sums of dy, on the values the kernel reads."""
    td = DT[dt][1]
    ar, dyr = rounded(a, td).numpy(), rounded(dy, td).numpy()
    return ar.T @ dyr, dyr.sum(0)


_REFS = {}


def reference(c, env=None):
    """(inputs, reference) of a case, computed once and shared (callers leave both unchanged)."""
    key = (c.id, tuple(sorted((env or {}).items())))
    if key not in _REFS:
        d = make_inputs(c)
        if c.entry == "fwd":
            r = reference_fwd(c, d, env)
        elif c.entry == "wgrad":
            dw, db = reference_wgrad(c.dt, d["a"], d["dy"])
            r = {"dw": dw, "db": db}
        else:
            dw, db = reference_wgrad(c.dt, d["a"], d["dy"])
            dw1, db1 = reference_wgrad(c.dt, d["a1"], d["dy1"])
            r = {"dw": dw, "db": db, "dw1": dw1, "db1": db1}
        _REFS[key] = (d, r)
    return _REFS[key]


# ---------------------------------------------------------------------------------------------------------------------------------------
# the case table.  Nothing searches: every shape is written down with the derivation of its size.
# ---------------------------------------------------------------------------------------------------------------------------------------
CASES = []


def add(entry, dt, M, K, N, layout, nsplit, tune_, family, tags, why, **opt):
    CASES.append(Case(len(CASES), entry, dt, M, K, N, layout, nsplit, tune_, family, tuple(tags.split()), why, opt))


RAW = dict(out_f32=True)
EPI = dict(bias=True, relu=True, mask=True)

# ---- dense_smallm_kernel: fp32, W [K, N], no mask, M <= 256, K % 4 == 0; a block = one 32 x 32 tile, the four waves take ceil(ksteps / 4) steps of 8 k each --------------
add("fwd", "f32", 256, 36, 40, 0, 1, AUTO, "dense_smallm", "m_at k_mod8_4 n_tail relu_nomask", "M = 256, the last row count the kernel takes; K = 36 = 4 steps and a half-filled fifth; N = 40 = a tile and 8; bias + ReLU, no mask", bias=True, relu=True)
add("fwd", "f32", 257, 36, 40, 0, 1, AUTO, "gen1.n64", "m_past falls_through", "M = 257: one row past the predicate, the first-generation kernel (W [K, N] never takes gemm2)", bias=True, relu=True)
add("fwd", "f32", 255, 36, 40, 0, 1, AUTO, "dense_smallm", "m_below m_tail k_mod8_4", "M = 255: the last tile holds 31 rows", bias=True)
add("fwd", "f32", 1, 4, 1, 0, 1, AUTO, "dense_smallm", "k_below_32 m1 n1 idle_waves", "one row, one column, K = 4: a single half-filled step, waves 1 - 3 own none", bias=True, relu=True, wave_steps=[1, 0, 0, 0])
add("fwd", "f32", 33, 20, 33, 0, 1, AUTO, "dense_smallm", "k_below_32 m_tail n_tail relu_nomask no_bias idle_waves k_mod8_4", "K = 20 = 3 steps (the third half filled): wave 3 owns none; M = N = 33: a second tile of one row / column; ReLU without bias or mask", relu=True, wave_steps=[1, 1, 1, 0])
add("fwd", "f32", 31, 300, 31, 0, 1, AUTO, "dense_smallm", "m_tail n_tail k_mod8_4 uneven_waves", "M = N = 31 inside one tile; K = 300 = 38 steps: 10 / 10 / 10 / 8 per wave, the last half filled", bias=True, wave_steps=[10, 10, 10, 8])
add("fwd", "f32", 32, 64, 32, 0, 1, AUTO, "dense_smallm", "full_tile relu_nomask", "exactly one full tile, K = 64 = two steps per wave; the PPO layer form (bias + ReLU)", bias=True, relu=True, wave_steps=[2, 2, 2, 2])
add("fwd", "f32", 64, 44, 96, 0, 1, AUTO, "dense_smallm", "several_blocks k_mod8_4 relu_nomask", "2 x 3 tiles; K = 44 (K % 8 == 4)", bias=True, relu=True)
add("fwd", "f32", 32, 28, 32, 0, 1, AUTO, "dense_smallm", "k_below_32 k_mod8_4 plain", "K = 28 = 4 steps, one per wave, the last half filled; no bias, no ReLU", wave_steps=[1, 1, 1, 1])
add("fwd", "f32", 32, 64, 32, 0, 1, AUTO, "gen1.n32", "mask falls_through", "the same layer with a ReluGrad mask: not the small-M kernel's", **EPI)
add("fwd", "f32", 32, 64, 32, 0, 1, NO_GEMM2, "gen1.n32", "key0_off falls_through", "key 0 = 0 switches the small-M kernel off with gemm2", bias=True, relu=True)
add("fwd", "x3", 32, 64, 40, 0, 1, AUTO, "gen1.n64", "x3 small_m falls_through", "split storage is not the small-M kernel's (fp32 only)", bias=True, relu=True)
add("fwd", "f32", 32, 64, 40, 1, 1, AUTO, "gemm2.128x64s2", "layout1 small_m falls_through f32", "fp32 with W [N, K]: not the small-M kernel's, gemm2 takes it", bias=True, relu=True)
add("fwd", "f32", 32, 6, 40, 0, 1, AUTO, "refused:K not a vector multiple", "refused k_vector", "K = 6: neither the small-M kernel (K % 4) nor the tile kernels (16-byte vectors)", bias=True)
add("fwd", "bf16", 32, 12, 40, 1, 1, AUTO, "refused:K not a vector multiple", "refused k_vector", "bf16 K = 12: not a multiple of 8", bias=True)

# ---- tallk_kernel<N / 32>: bf16, W [N, K], raw fp32 slabs, N in {32, 64, 128}, K % (16 nsplit) == 0, nsplit % (4 / (N / 32)) == 0; steps = K / nsplit / 16 in groups of six -----
add("fwd", "bf16", 33, 448, 32, 1, 4, AUTO, "tallk.1", "nt1 steps_7 m_tail", "N = 32 (four K sub-slices per block): 448 / 4 / 16 = 7 steps = one group and one; M = 33: a second block of one row (31 clamped)", steps=7, **RAW)
add("fwd", "bf16", 32, 384, 32, 1, 4, AUTO, "tallk.1", "nt1 steps_6 m_at", "6 steps = exactly one group; M = 32 = one block", steps=6, **RAW)
add("fwd", "bf16", 31, 768, 32, 1, 8, AUTO, "tallk.1", "nt1 steps_6 m_below two_slices", "8 slabs = two blocks along K of four sub-slices; 6 steps; M = 31", steps=6, **RAW)
add("fwd", "bf16", 1, 160, 64, 1, 2, AUTO, "tallk.2", "nt2 steps_5 m1", "N = 64 (two sub-slices per block): 5 steps; one row: 31 lanes clamp to it", steps=5, **RAW)
add("fwd", "bf16", 64, 1248, 64, 1, 6, AUTO, "tallk.2", "nt2 steps_13 m_at", "6 slabs of 13 steps = two groups and one; M = 64 = two full blocks", steps=13, **RAW)
add("fwd", "bf16", 96, 192, 64, 1, 2, AUTO, "tallk.2", "nt2 steps_6 m_at", "6 steps; M = 96", steps=6, **RAW)
add("fwd", "bf16", 112, 352, 128, 1, 2, AUTO, "tallk.4", "nt4 steps_11 m_tail", "N = 128 (one K slice per block): 11 steps = one group and five; M = 112 = 3.5 blocks", steps=11, **RAW)
add("fwd", "bf16", 160, 288, 128, 1, 3, AUTO, "tallk.4", "nt4 steps_6 m_at odd_nsplit", "three slabs of 6 steps; M = 160 = five blocks", steps=6, **RAW)
add("fwd", "bf16", 33, 16 * 2 * 12, 128, 1, 2, AUTO, "tallk.4", "nt4 steps_12 m_tail", "12 steps = two whole groups; M = 33", steps=12, **RAW)
add("fwd", "bf16", 33, 256, 32, 1, 2, AUTO, "gemm2.256x32s2.splitk", "nsplit_not_kp falls_through t256x32", "N = 32 needs nsplit % 4 == 0: two slabs go to gemm2's split-K (len 128 = two stages)", **RAW)
add("fwd", "bf16", 33, 176, 64, 1, 2, AUTO, "gen1.n64.splitk", "k_not_16nsplit stage_fallback falls_through", "K = 176 is no multiple of 32: not tall-K; len = 96 elements = 192 bytes is no whole stage: not gemm2 either", **RAW)
add("fwd", "bf16", 33, 384, 96, 1, 2, AUTO, "gemm2.128x64s2.splitk", "n96 falls_through", "N = 96 is not a tall-K width: gemm2 split-K on two 64-wide column blocks (len 192 = three stages)", **RAW)
add("fwd", "f32", 33, 512, 32, 1, 4, AUTO, "gemm2.256x32s2.splitk", "tallk_shape_f32 falls_through t256x32 f32", "a tall-K shape in fp32: gemm2 split-K (len 128 k = four stages)", **RAW)

# ---- gemm2 split-K (W [N, K]): len = ceil(ceil(K / nsplit) / bk) bk must be whole 128-byte stages ---------------------------------------------------------------------
add("fwd", "bf16", 33, 328, 64, 1, 3, AUTO, "gemm2.128x64s2.splitk", "last_slab_short t128x64", "len = 128; the last slab holds 328 - 256 = 72 k = 128 bytes plus 16", last=72, **RAW)
add("fwd", "f32", 33, 100, 40, 1, 2, AUTO, "gemm2.128x64s2.splitk", "last_slab_short f32 n_tail", "fp32: len = 64; the last slab holds 36 k = 128 bytes plus 16", last=36, **RAW)
add("fwd", "x3", 129, 100, 72, 1, 2, tune(k17=1), "gemm2.64x64s2.splitk", "last_slab_short x3 t64x64 m_past", "split storage on 64 x 64 tiles (key 17 = 1); M = 129", last=36, **RAW)
add("fwd", "bf16", 130, 904, 136, 1, 3, tune(k17=3, k20=3), "gemm2.128x128s3.splitk", "last_slab_short t128x128 stages3 m_past n_tail", "128 x 128 tiles, three stages: len = 320 = five stages, the last slab 264 k = four stages and 16 bytes; M = 130, N = 136", last=264, **RAW)
add("fwd", "bf16", 33, 1000, 40, 1, 2, tune(k20=4), "gemm2.128x64s4.splitk", "stages4 last_slab_short", "four LDS stages: len = 512 = eight stages, the last slab 488 k = 7.6 stages", last=488, **RAW)
add("fwd", "f32", 33, 96, 40, 1, 2, AUTO, "gen1.n64.splitk", "stage_fallback f32 falls_through", "fp32 len = 48 k = 192 bytes: no whole stage, the first-generation kernel", **RAW)
add("fwd", "bf16", 33, 64, 40, 1, 3, AUTO, "refused:empty slab", "refused empty_slab", "K = 64 in three slabs of 32: the third would be empty", **RAW)
add("fwd", "f32", 33, 32, 40, 0, 3, AUTO, "refused:empty slab", "refused empty_slab layout0", "fp32 K = 32 in three slabs of 16", **RAW)
add("fwd", "bf16", 33, 256, 40, 1, 2, AUTO, "refused:split-K writes raw fp32 slabs only", "refused splitk_epilogue", "split-K with a bias", bias=True, out_f32=True)
add("fwd", "bf16", 33, 256, 40, 1, 2, AUTO, "refused:split-K writes raw fp32 slabs only", "refused splitk_epilogue", "split-K into the storage type", )
add("fwd", "bf16", 33, 328, 64, 0, 3, AUTO, "gen1.n64.splitk", "layout0 last_slab_short", "W [K, N] can only take the first-generation kernel: the same ragged split", last=72, **RAW)
add("fwd", "bf16", 33, 328, 64, 1, 3, NO_GEMM2, "gen1.n64.splitk", "key0_off last_slab_short", "key 0 = 0: the first-generation kernel on K-contiguous weights", last=72, **RAW)

# ---- gemm2 tiles without split (W [N, K]): 256 x 32 | 128 x 64 (2 / 3 / 4 stages from nk >= 6) | 64 x 64 | 128 x 128 (2 / 3 stages) ------------------------------------------
add("fwd", "bf16", 257, 200, 24, 1, 1, AUTO, "gemm2.256x32s2", "t256x32 m_past n_tail ragged_k", "M = 257 = a 256-row tile and one; N = 24; K = 200 = 3.125 stages", **EPI)
add("fwd", "bf16", 256, 200, 32, 1, 1, AUTO, "gemm2.256x32s2", "t256x32 m_at n_at", "M = 256, N = 32 exactly", bias=True, relu=True)
add("fwd", "bf16", 255, 64, 33, 1, 1, AUTO, "gemm2.128x64s2", "t128x64 m_below n_past", "N = 33: the first width past the 32-wide tile; M = 255", bias=True, out_f32=True)
add("fwd", "bf16", 127, 384, 64, 1, 1, tune(k20=2), "gemm2.128x64s2", "t128x64 stages2 nk_at m_below n_at", "nk = 6, two stages; M = 127, N = 64", **EPI)
add("fwd", "bf16", 128, 384, 40, 1, 1, tune(k20=3), "gemm2.128x64s3", "t128x64 stages3 nk_at m_at", "nk = 6: three stages; M = 128", **EPI)
add("fwd", "bf16", 129, 384, 40, 1, 1, tune(k20=4), "gemm2.128x64s4", "t128x64 stages4 nk_at m_past", "nk = 6: four stages; M = 129", **EPI)
add("fwd", "bf16", 129, 320, 40, 1, 1, tune(k20=4), "gemm2.128x64s2", "t128x64 nk_below", "K = 320: nk = 5 < 6 keeps two stages whatever key 20 says", **EPI)
add("fwd", "f32", 36, 72, 72, 1, 1, tune(k17=1), "gemm2.64x64s2", "t64x64 f32 m_tail n_tail", "64 x 64 tiles (key 17 = 1): M = 36, N = 72", **EPI)
add("fwd", "bf16", 65, 72, 65, 1, 1, tune(k17=0), "gemm2.64x64s2", "t64x64 auto_small_grid m_past n_past", "key 17 = 0: a grid below 512 blocks takes 64 x 64 tiles; M = N = 65", **EPI)
add("fwd", "x3", 130, 108, 136, 1, 1, tune(k17=3, k20=3), "gemm2.128x128s2", "t128x128 nk_below x3 n_tail m_past", "128 x 128 tiles: K = 108 x 4 bytes = 3.4 stages: two stages although key 20 asks for three", **EPI)
add("fwd", "bf16", 130, 384, 136, 1, 1, tune(k17=3, k20=3), "gemm2.128x128s3", "t128x128 stages3 n_tail", "128 x 128 tiles, nk = 6: three stages", **EPI)
add("fwd", "bf16", 130, 384, 72, 1, 1, tune(k17=2), "gemm2.128x64s2", "t128x64 two_columns", "N = 72 on 128 x 64 tiles: two column blocks", bias=True, out_f32=True)

# ---- first-generation gemm_kernel (W [K, N], or key 0 = 0): 128 rows x 32 | 64 | 128 columns ----------------------------------------------------------------------------
add("fwd", "bf16", 129, 72, 32, 0, 1, AUTO, "gen1.n32", "gemm_n32 n_at m_past", "N = 32; M = 129", **EPI)
add("fwd", "bf16", 127, 72, 33, 0, 1, AUTO, "gen1.n64", "gemm_n64 n_past m_below", "N = 33; M = 127", **EPI)
add("fwd", "x3", 128, 76, 64, 0, 1, AUTO, "gen1.n64", "gemm_n64 n_at m_at x3", "N = 64, M = 128; split storage, K = 76", **EPI)
add("fwd", "f32", 300, 76, 65, 0, 1, AUTO, "gen1.n128", "gemm_n128 n_past f32", "N = 65: the 128-wide tile; fp32 past the small-M kernel (M = 300)", bias=True, relu=True)
add("fwd", "bf16", 33, 72, 136, 0, 1, AUTO, "gen1.n128", "gemm_n128 two_columns out_f32", "N = 136: two 128-wide column blocks; fp32 output from bf16 storage", bias=True, out_f32=True)
add("fwd", "bf16", 33, 72, 30, 0, 1, AUTO, "gen1.n32", "gemm_n32 n_unaligned", "N = 30: the rows of W [K, N] are no whole vectors", **EPI)

# ---- dwg_kernel<3> (MI355_DWG_NST = 4 in the child process): bf16, storing form, K % 128 == N % 128 == 0, >= 256 tiles; stages of 32 rows ------------------------------------
add("wgrad", "bf16", 33, 128 * 257, 128, 0, 1, AUTO, "dwg.3", "early_return kt_major ragged_stage", "257 x 1 tiles on a grid of 264: seven blocks return at once; M = 33: a second stage of one row", overwrite=True, dbias=True, grid=(264, 7), twice=True)
add("wgrad", "bf16", 40, 128, 128 * 256, 0, 1, AUTO, "dwg.3", "nt_major ragged_stage", "1 x 256 tiles (NT > KT: n-major numbering); M = 40: a ragged second stage", overwrite=True, dbias=True, grid=(256, 0), twice=True)
add("wgrad", "bf16", 7, 2048, 2048, 0, 1, AUTO, "dwg.3", "m_below_stage", "16 x 16 tiles; M = 7: a single stage, 25 of its rows out of range", overwrite=True, dbias=True, grid=(256, 0))
add("wgrad", "bf16", 1, 128, 128 * 256, 0, 1, AUTO, "dwg.3", "m1 nt_major no_dbias", "one row, no bias gradient", overwrite=True, grid=(256, 0))
add("wgrad", "bf16", 64, 2048, 2048, 0, 1, AUTO, "dwg.3", "stages_nst_minus_1", "M = 64 = two full stages = NST - 1 of the three-stage ring", overwrite=True, dbias=True, stages=2)
add("wgrad", "bf16", 96, 2048, 2048, 0, 1, AUTO, "dwg.3", "stages_nst stages_nst4_minus_1", "M = 96 = three full stages = NST (and NST - 1 of the four-stage ring)", overwrite=True, dbias=True, stages=3, twice=True)
add("wgrad", "bf16", 100, 2048, 2048, 0, 1, AUTO, "dwg.3", "stages_past_nst stages_nst4 ragged_stage", "M = 100 = four stages, the last of 4 rows: the ring wraps (NST = 3) / is exactly full (NST = 4)", overwrite=True, dbias=True, stages=4)
add("wgrad", "bf16", 16, 128 * 255, 128, 0, 1, AUTO, "gen1w.128.single", "tiles_255 falls_through", "255 tiles: one short of the tile kernel; K N is past the one-wave kernel's limit too: the first-generation kernel, one row split, plain stores", overwrite=True, dbias=True)
add("wgrad", "bf16", 33, 2048, 2048, 0, 1, AUTO, "gen1w.128.single", "adding_form falls_through", "the tile kernel only stores: the adding form of the same shape is the first-generation kernel's (M = 33 is not the one-wave kernel's)", dbias=True)

# ---- dwgs_kernel<store | add> with 1 / 2 / 4 waves per 64 x 64 tile: bf16, M % 16 == 0, K % 64 == N % 64 == 0, K N <= 262144 -------------------------------------------------
# waves: steps = M / 16; four if steps % 4 == 0 and steps >= 8, else two if steps % 2 == 0 and steps >= 4, else one.  Per wave ns = steps / waves load rounds, DWGS_DEPTH = 4 in flight
add("wgrad", "bf16", 16, 64, 64, 0, 1, AUTO, "dwgs.store.w1", "w1 ns_1 one_tile early_return", "M = 16: one step; one tile on a grid of eight: seven blocks return at once", overwrite=True, dbias=True, ws=1, ns=1, grid=(8, 7))
add("wgrad", "bf16", 32, 128, 192, 0, 1, AUTO, "dwgs.add.w1", "w1 ns_2 nt_major", "M = 32: two steps do not split (a wave keeps two rounds); 2 x 3 tiles, n-major", dbias=True, ws=1, ns=2)
add("wgrad", "bf16", 112, 192, 64, 0, 1, AUTO, "dwgs.store.w1", "w1 ns_7 tail_3 kt_major", "M = 112: seven steps = one group of four and a tail of three; 3 x 1 tiles", overwrite=True, dbias=True, ws=1, ns=7)
add("wgrad", "bf16", 64, 128, 192, 0, 1, AUTO, "dwgs.store.w2", "w2 ns_2 hand_over", "M = 64: two waves of two steps (less than the depth: tail steps only); wave 0 stores its tile to LDS, wave 1 adds and stores", overwrite=True, dbias=True, ws=2, ns=2, twice=True)
add("wgrad", "bf16", 64, 128, 192, 0, 1, AUTO, "dwgs.add.w2", "w2 ns_2 hand_over", "the adding form of the same", dbias=True, ws=2, ns=2, twice=True)
add("wgrad", "bf16", 96, 64, 64, 0, 1, AUTO, "dwgs.store.w2", "w2 ns_3 one_tile", "M = 96: two waves of three steps", overwrite=True, dbias=True, ws=2, ns=3)
add("wgrad", "bf16", 96, 64, 64, 0, 1, AUTO, "dwgs.add.w2", "w2 ns_3 no_dbias", "adding form without the bias row", ws=2, ns=3)
add("wgrad", "bf16", 160, 192, 128, 0, 1, AUTO, "dwgs.store.w2", "w2 ns_5 tail_1", "M = 160: two waves of five steps = one group and a tail of one", overwrite=True, dbias=True, ws=2, ns=5)
add("wgrad", "bf16", 224, 64, 192, 0, 1, AUTO, "dwgs.add.w2", "w2 ns_7 tail_3", "M = 224: two waves of seven steps", dbias=True, ws=2, ns=7)
add("wgrad", "bf16", 128, 128, 64, 0, 1, AUTO, "dwgs.store.w4", "w4 ns_2", "M = 128: eight steps, four waves of two", overwrite=True, dbias=True, ws=4, ns=2, twice=True)
add("wgrad", "bf16", 256, 64, 128, 0, 1, AUTO, "dwgs.add.w4", "w4 ns_4 whole_group", "M = 256: four waves of four steps = exactly one group", dbias=True, ws=4, ns=4)
add("wgrad", "bf16", 320, 64, 64, 0, 1, AUTO, "dwgs.store.w4", "w4 ns_5 tail_1 no_dbias", "M = 320: four waves of five steps; no bias row", overwrite=True, ws=4, ns=5)
add("wgrad", "bf16", 64, 512, 512, 0, 1, AUTO, "dwgs.store.w2", "w2 kn_at", "K N = 262144: the largest result the kernel takes (64 tiles)", overwrite=True, dbias=True, ws=2, ns=2)
add("wgrad", "bf16", 64, 512, 576, 0, 1, AUTO, "gen1w.128.single", "kn_past falls_through", "K N = 294912: past the limit; 513 rows in five 128-row blocks x nine column blocks: one row split, plain stores", overwrite=True, dbias=True)
add("wgrad", "bf16", 8, 64, 64, 0, 1, AUTO, "gen1w.128.single", "m_below_16 falls_through", "M = 8 < 16: the first-generation kernel (65 rows with the bias row)", dbias=True)
add("wgrad", "bf16", 24, 64, 64, 0, 1, AUTO, "gen1w.64.single", "m_not_16 falls_through", "M = 24 is no multiple of 16; no bias row: 64 rows", )
add("wgrad", "bf16", 64, 128, 192, 0, 1, NO_DWGS, "gen1w.128.single", "key22_off falls_through", "key 22 = 0: the first-generation kernel on the two-wave shape (M = 64 = one step of 64 rows: one row split)", dbias=True, scratch="exact", splits=1)

# ---- first-generation wgrad_kernel: 64 rows per block up to 64 result rows (incl. the bias row), else 128; row splits = key 11 / blocks, in multiples of BP rows ---------------
add("wgrad", "f32", 40, 64, 40, 0, 1, AUTO, "gen1w.64.slabs", "kce_64 rows64", "K = 64 without a bias row: the 64-row kernel; M = 40 in three splits of 16", scratch="exact", splits=3, twice=True)
add("wgrad", "f32", 40, 64, 40, 0, 1, AUTO, "gen1w.128.slabs", "kce_65 rows128 dbias", "the same with a bias row: 65 result rows flip to the 128-row kernel", scratch="exact", dbias=True, splits=3, twice=True)
add("wgrad", "f32", 40, 60, 40, 0, 1, AUTO, "gen1w.64.slabs", "kce_61 rows64 dbias", "K = 60 with a bias row: 61 rows stay on the 64-row kernel", scratch="exact", dbias=True, splits=3)
add("wgrad", "f32", 512, 72, 40, 0, 1, AUTO, "refused:overwrite needs scratch", "refused overwrite_no_scratch", "storing form, 32 row splits, no scratch", overwrite=True, dbias=True)
add("wgrad", "f32", 512, 72, 40, 0, 1, AUTO, "refused:overwrite needs scratch", "refused overwrite_short_scratch", "storing form with 16 bytes less scratch than the slabs take", overwrite=True, dbias=True, scratch="short")
add("wgrad", "f32", 512, 72, 40, 0, 1, AUTO, "gen1w.128.slabs", "overwrite slabs dbias", "storing form through the storing ordered sum", overwrite=True, dbias=True, scratch="exact", splits=32, twice=True)
add("wgrad", "f32", 512, 72, 40, 0, 1, AUTO, "gen1w.128.atomics", "scratch_short dbias", "adding form with 16 bytes less: atomics", dbias=True, scratch="short", splits=32)
add("wgrad", "f32", 512, 72, 40, 0, 1, tune(k11=16), "gen1w.128.slabs", "key11_16 dbias", "key 11 = 16: 16 row splits of 32", dbias=True, scratch="exact", splits=16)
add("wgrad", "f32", 512, 72, 40, 0, 1, tune(k11=1), "gen1w.128.single", "key11_1 overwrite", "key 11 = 1: one row split, plain stores need no scratch", overwrite=True, dbias=True, splits=1)
add("wgrad", "bf16", 520, 72, 40, 0, 1, tune(k11=1024), "gen1w.128.slabs", "key11_1024 bf16 m_tail", "key 11 = 1024 on bf16 (64 rows per step): nine splits, the last of 8 rows", dbias=True, scratch="exact", splits=9)
add("wgrad", "x3", 40, 76, 24, 0, 1, AUTO, "gen1w.128.slabs", "x3 m_tail", "split storage (32 rows per step): two splits, the second of 8 rows", dbias=True, scratch="exact", splits=2)
add("wgrad", "f32", 12, 72, 40, 0, 1, AUTO, "gen1w.128.single", "m_below_bp", "M = 12 < 16 rows of a step", dbias=True, scratch="exact", splits=1)
add("wgrad", "bf16", 40, 8, 24, 0, 1, AUTO, "gen1w.64.single", "k8 no_scratch", "K = 8: one vector per row", dbias=True, splits=1)
add("wgrad", "f32", 40, 6, 24, 0, 1, AUTO, "refused:K not a vector multiple", "refused k_vector", "K = 6", dbias=True)

# ---- wgrad_pair_kernel: two bf16 problems, both on the 128-row first-generation form ------------------------------------------------------------------------------------
add("pair", "bf16", 40, 72, 136, 0, 1, AUTO, "pair", "off_model scratch", "[40, 72]^T [40, 136] and [40, 136]^T [40, 24] as one launch, slabs for both", second=(40, 136, 24), scratch="exact")
add("pair", "bf16", 130, 64, 40, 0, 1, AUTO, "pair", "kce_65 different_m scratch", "K = 64 with its bias row = 65 rows: the 128-row form; the two problems have different row counts", second=(72, 200, 72), scratch="exact")
add("pair", "bf16", 130, 64, 40, 0, 1, AUTO, "pair.two_calls", "kce_64 falls_through", "the same without problem 0's bias row: 64 rows, the 64-row form: two calls", second=(72, 200, 72), scratch="exact", dbias=False)
add("pair", "bf16", 128, 64, 64, 0, 1, AUTO, "pair.two_calls", "dwgs_eligible falls_through", "problem 0 is the one-wave kernel's (four waves per tile: another summation order than the first-generation kernel's two row splits): two calls", second=(40, 72, 40), scratch="exact")
add("pair", "f32", 40, 72, 136, 0, 1, AUTO, "pair.two_calls", "f32 falls_through", "fp32: two calls", second=(40, 136, 24), scratch="exact")

assert [c.id for c in CASES] == list(range(len(CASES)))


def group_of(family):
    return family.split(":")[0].split(".")[0]


N_CASES = collections.Counter(group_of(c.family) for c in CASES)

# every (family group, boundary tag) pair the table must hold at least once
REQUIRED = {
    "dense_smallm": "m_at m_below k_mod8_4 k_below_32 idle_waves uneven_waves m_tail n_tail m1 n1 relu_nomask no_bias plain full_tile several_blocks",
    "tallk": "nt1 nt2 nt4 steps_5 steps_6 steps_7 steps_11 steps_12 steps_13 m1 m_below m_at m_tail two_slices odd_nsplit",
    "gemm2": "t256x32 t128x64 t64x64 t128x128 stages2 stages3 stages4 nk_at nk_below last_slab_short nsplit_not_kp n96 m_below m_at m_past n_at n_past n_tail f32 x3 auto_small_grid two_columns",
    "gen1": "m_past mask key0_off stage_fallback k_not_16nsplit layout0 last_slab_short gemm_n32 gemm_n64 gemm_n128 n_at n_past n_unaligned x3 f32 out_f32",
    "dwg": "early_return kt_major nt_major ragged_stage m_below_stage m1 no_dbias stages_nst_minus_1 stages_nst stages_past_nst stages_nst4_minus_1 stages_nst4",
    "dwgs": "w1 w2 w4 ns_1 ns_2 ns_3 ns_4 ns_5 ns_7 tail_1 tail_3 whole_group hand_over one_tile early_return nt_major kt_major no_dbias kn_at",
    "gen1w": "tiles_255 adding_form kn_past m_below_16 m_not_16 key22_off kce_64 kce_65 kce_61 overwrite slabs scratch_short key11_16 key11_1 key11_1024 x3 bf16 m_below_bp m_tail k8",
    "pair": "off_model kce_65 different_m kce_64 dwgs_eligible f32",
    "refused": "k_vector empty_slab splitk_epilogue overwrite_no_scratch overwrite_short_scratch",
}

# every kernel family and template instantiation a key can reach (dwg.4 and the knob fall-backs: ENV_STEPS below, in a child process)
INSTANTIATIONS = ("dense_smallm", "tallk.1", "tallk.2", "tallk.4",
                  "gemm2.256x32s2", "gemm2.128x64s2", "gemm2.128x64s3", "gemm2.128x64s4", "gemm2.64x64s2", "gemm2.128x128s2", "gemm2.128x128s3",
                  "gemm2.256x32s2.splitk", "gemm2.128x64s2.splitk", "gemm2.128x64s4.splitk", "gemm2.64x64s2.splitk", "gemm2.128x128s3.splitk",
                  "gen1.n32", "gen1.n64", "gen1.n128", "gen1.n64.splitk",
                  "dwg.3", "dwgs.store.w1", "dwgs.store.w2", "dwgs.store.w4", "dwgs.add.w1", "dwgs.add.w2", "dwgs.add.w4",
                  "gen1w.64.single", "gen1w.64.slabs", "gen1w.128.single", "gen1w.128.slabs", "gen1w.128.atomics", "pair", "pair.two_calls")

# the environment-only knobs, two child processes (the knobs of a step are independent of each other): {variable: value}, the family prefix whose cases run again, and the
# families those cases must land in
ENV_STEPS = (
    ({"MI355_TALLK": 0, "MI355_DWG_NST": 4}, ("tallk.", "dwg."), ("gemm2.256x32s2.splitk", "gemm2.128x64s2.splitk", "gemm2.128x128s2.splitk", "gen1.n32.splitk", "gen1.n64.splitk", "gen1.n128.splitk", "dwg.4")),
    ({"MI355_GEMM2_SPLITK": 0, "MI355_DWG": 0}, ("gemm2.", "dwg."), ("gen1.n32.splitk", "gen1.n64.splitk", "gen1.n128.splitk", "gen1w.128.single")),
)


def env_cases(step):
    """The cases a step of ENV_STEPS runs again: those whose family under the DEFAULT environment starts with one of the step's prefixes and changes under the step's."""
    env, prefixes, _ = ENV_STEPS[step]
    out = []
    for c in CASES:
        if c.family.startswith(prefixes) and (family_of(c, env)[0] != c.family):
            out.append(c)
    return out


def by_family(prefix):
    return [c for c in CASES if c.family.startswith(prefix)]


def case_id(c):
    return "%s-%03d-%s-%s" % (c.family.split(":")[0], c.id, c.dt, "_".join(c.tags[:3]))
