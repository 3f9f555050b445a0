"""Cases, float64 references and dispatch predicates for test_x_conv_shapes_gpu.py (test infrastructure; imports no GPU): the conv / deconv layer-op entry points
OFF the nine layer geometries of the ConvVAE, at the edges of the launchers' predicates (csrc/conv_ops.hip, csrc/rwconv.hip).

A case = one entry point, one storage type, one shape, the mi_set_tuning settings that pin the dispatch, the kernel family it is meant to reach and the boundary it
probes (tags + words).  The shape of a case is always the FORWARD layer's: x [B, IH, IW, C] -> y [B, OH, OW, N], kernel size k, stride 2, VALID --
conv.*: OH = (IH - k) // 2 + 1, kernel HWIO [k, k, C, N];  deconv.*: OH = (IH - 1) * 2 + k, kernel [k, k, N, C].

The predicates below (one per family) restate the launchers' SHAPE conditions and nothing else (fresh allocations are 16-byte aligned); family_of() applies them in the
launchers' order of trial.  test_conv_shape_cases_host.py asserts that every case's claimed family follows from them and that every derived size equals the constant
it cites (parsed out of the headers)."""
import collections
import math
import os
import re

import numpy as np
import torch
import torch.nn.functional as F

from hip_helpers import DT, rounded

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "carla-ppo_amd", "csrc")

# ---------------------------------------------------------------------------------------------------------------------------------------
# constants the cases cite (test_conv_shape_cases_host.py compares them with the headers)
# ---------------------------------------------------------------------------------------------------------------------------------------
TC_BMT, TC_BMT_SMALL = 256, 128          # tapconv_tile.hpp TC_BMT; the small tile of launch_tapconv_t (conv_ops.hip)
TC_MAXHALO, TC_MAXHALO_SMALL = 96, 48
TW_BP = 128                              # tapwgrad_tile.hpp: positions per step
GN_BMT = 128                             # narrow_tile.hpp: positions per gather_narrow block
GEMM_BM = 128                            # gemm_tile.hpp
NW_BP, NW_SLAB = 16, 64 * 32 + 32        # narrow_tile.hpp: pixels per narrow_wgrad wave step, floats per block slab
NW_GRID_WAVES = 256 * 12                 # try_narrow_wgrad: one wave range per resident wave (256 CUs x MI355_NW_WAVES = 12)
RW_MAXHALO = {2: 48, 3: 96}              # rwconv.hip RwCfg<TAPS>::MAXHALO
RC_MAXHALO = {(4, 1): 48, (4, 2): 32, (5, 1): 96}      # rwconv.hip RcCfg<KH, CK>::MAXHALO
WGRAD_BP = {"f32": 16, "bf16": 64, "x3": 32}            # wgrad_tile.hpp WgradCfg<T>::BP
GEN1_WGRAD_TARGET = 1024                 # launch_wgrad's target block count at the layer-op entry points


def header_constants():
    """The same constants parsed out of the sources: {name: int}."""
    out = {}

    def grab(fname, pats):
        text = open(os.path.join(CSRC, fname)).read()
        for name, pat in pats.items():
            m = re.search(pat, text)
            assert m, (fname, name)
            out[name] = [int(g) for g in m.groups()] if len(m.groups()) > 1 else int(m.group(1))

    grab("tapconv_tile.hpp", {"TC_BMT": r"constexpr int TC_BMT = (\d+);", "TC_MAXHALO": r"constexpr int TC_MAXHALO = (\d+);"})
    grab("tapwgrad_tile.hpp", {"TW_BP": r"constexpr int TW_BP = (\d+);"})
    grab("narrow_tile.hpp", {"GN_BMT": r"constexpr int GN_BMT = (\d+);", "NW_BP": r"constexpr int NW_BP = (\d+);", "NW_SLAB": r"constexpr int NW_SLAB = (\d+) \* (\d+) \+ (\d+);"})
    grab("gemm_tile.hpp", {"GEMM_BM": r"constexpr int GEMM_BM = (\d+);"})
    grab("wgrad_tile.hpp", {"WG_F32": r"WgradCfg<float>\s*\{ static constexpr int BP = (\d+);", "WG_BF16": r"WgradCfg<bf16_t>\s*\{ static constexpr int BP = (\d+);",
                            "WG_X3": r"WgradCfg<split_t>\s*\{ static constexpr int BP = (\d+);"})
    grab("rwconv.hip", {"RW_MAXHALO": r"static constexpr int MAXHALO = TAPS == 2 \? (\d+) : (\d+);",
                        "RC_MAXHALO": r"static constexpr int MAXHALO = TAPS == 2 \? \(CK == 1 \? (\d+) : (\d+)\) : (\d+);"})
    grab("conv_ops.hip", {"NW_CUS": r"long long nwave = (\d+)ll \* knob\(K_NW_WAVES\);", "SMALL_TILE": r"launch_tapconv_v<T, MODE, TAPS, (\d+), (\d+)>\(st, q\) : launch_tapconv_v<T, MODE, TAPS, TC_BMT, TC_MAXHALO>",
                          "GEN1_WGRAD_TARGET": r"return launch_wgrad\(\(hipStream_t\)stream, dtype, x_is_f32, p, (\d+), scratch, scratch_bytes, 0, ctx\);"})
    text = open(os.path.join(CSRC, "tuning.hip")).read()
    out["NW_WAVES"] = int(re.search(r"\{K_NW_WAVES, \"MI355_NW_WAVES\", NOKEY, (\d+),", text).group(1))
    out["DEFAULTS"] = {int(m.group(1)): int(m.group(2)) for m in re.finditer(r"^\s*\{K_\w+, (?:nullptr|\"\w+\"), (\d+), (-?\d+), P_", text, flags=re.M)}
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# tuning presets (mi_set_tuning keys; csrc/tuning.hip).  DEFAULTS = what a fresh process holds.
# ---------------------------------------------------------------------------------------------------------------------------------------
DEFAULTS = {0: 1, 1: 300, 3: 1, 4: 1, 5: 0, 6: 1, 7: 1, 9: 256, 10: 12, 13: 1, 14: 1, 15: 3, 16: 0, 17: 2, 18: 0, 20: 2, 21: 1, 24: 0}
GENERATIONS = {"gen1": {0: 0, 1: -1, 3: 0, 4: 0, 13: 0}, "newest": {0: 1, 1: 1, 3: 1, 4: 1, 13: 0}, "rwconv": {0: 1, 1: 1, 3: 1, 4: 1, 13: 2, 15: 3, 16: 1}}
GEN1 = GENERATIONS["gen1"]
NEW = GENERATIONS["newest"]
TAP_BIG = {**NEW, 5: 1}
TAP_SMALL = {**NEW, 5: 2}
GEMM2 = {**NEW, 1: -1}


def tune(base, **kw):
    d = dict(base)
    d.update({int(k[1:]): v for k, v in kw.items()})
    return d


def knobs_of(case):
    d = dict(DEFAULTS)
    d.update(case.tune)
    return d


Case = collections.namedtuple("Case", "id entry dt B IH IW C N k tune family tags why opt")
ENTRIES = ("conv.fwd", "conv.dgrad", "conv.wgrad", "deconv.fwd", "deconv.dgrad", "deconv.wgrad")


def out_hw(c):
    if c.entry.startswith("conv."):
        return (c.IH - c.k) // 2 + 1, (c.IW - c.k) // 2 + 1
    return (c.IH - 1) * 2 + c.k, (c.IW - 1) * 2 + c.k


def esz(dt):
    return 2 if dt == "bf16" else 4


def ceil_div(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the slot grid of the raw-staged kernels (tapconv_tile.hpp): form "conv" = conv fwd / deconv dgrad, "gather" = deconv fwd / conv dgrad.
# The arguments are the TAP kernel's: a [B, ih, iw, c] -> out [B, oh, ow, n].
# ---------------------------------------------------------------------------------------------------------------------------------------
def slot_grid(form, k, oh, ow):
    t = (k + 1) // 2
    if form == "conv":
        gh, gw = oh + t - 1, ow + t - 1
    else:
        gh, gw = (oh + 1) // 2 + t - 1, (ow + 1) // 2 + t - 1
    return t, gh, gw, (t - 1) * gw + t - 1


def tap_args(c):
    """(form, B, ih, iw, c, oh, ow, n) as the forward / input-gradient launchers see the case."""
    OH, OW = out_hw(c)
    if c.entry == "conv.fwd":
        return "conv", c.B, c.IH, c.IW, c.C, OH, OW, c.N
    if c.entry == "deconv.dgrad":
        return "conv", c.B, OH, OW, c.N, c.IH, c.IW, c.C
    if c.entry == "deconv.fwd":
        return "gather", c.B, c.IH, c.IW, c.C, OH, OW, c.N
    if c.entry == "conv.dgrad":
        return "gather", c.B, OH, OW, c.N, c.IH, c.IW, c.C
    raise ValueError(c.entry)


def tapconv_plan(form, dt, B, ih, iw, c, oh, ow, n, k, ldb, kn):
    """try_tapconv: None (not eligible) or {tile, MP, halo, NE, BNE, KC, direct}."""
    mb = kn[1]
    e = esz(dt)
    if mb < 0 or k < 3 or k > 6:
        return None
    if (c * e) % 16 or (n * e) % 16 or B * oh * ow * n >= 1 << 31:
        return None
    t, gh, gw, halo = slot_grid(form, k, oh, ow)
    if form == "conv":
        if (ldb * e) % 16 or ldb < k * k * c:
            return None
        if t == 3 and mb > 1:
            return None
        kc, ne = 4 * c, n
    else:
        if n % 32:
            return None
        kc, ne = c, 4 * n
    if halo > TC_MAXHALO:
        return None
    mp = B * gh * gw
    bne = 128 if ne >= 128 else 64
    gy = ceil_div(ne, bne)
    blocks = ceil_div(mp, TC_BMT) * gy
    if blocks < mb:
        return None
    auto_small = 300 <= blocks <= 1000 and gy <= 2
    small = halo <= TC_MAXHALO_SMALL and dt == "bf16" and (kn[5] == 2 or (kn[5] == 0 and auto_small))
    return {"tile": "small" if small else "big", "MP": mp, "halo": halo, "NE": ne, "BNE": bne, "KC": kc, "GW": gw, "direct": bool(kn[6]) and n % 32 == 0}


def rwconv_gather_ok(dt, B, ih, iw, c, oh, ow, n, k, relu, mask, kn):
    """mi_try_rwconv_gather (the entry points of this file never ask for bit words)."""
    ck = 2 if (c == 128 and n == 64 and k == 4) else 1
    if dt != "bf16" or c != 64 * ck or n != 32 * ck or k not in (4, 5):
        return False
    t, gh, gw, halo = slot_grid("gather", k, oh, ow)
    if halo > RW_MAXHALO[t] or (ck == 1 and gw <= 32):
        return False
    mp = B * gh * gw
    if kn[13] == 0 or (kn[13] == 1 and mp < 75000):
        return False
    return not (ck == 2 and relu and mask)


def rwconv_conv_ok(dt, B, ih, iw, c, oh, ow, n, k, ldb, kn):
    """mi_try_rwconv_conv."""
    ck = 2 if (c == 64 and n == 128) else 1
    on = kn[15]
    if not on or kn[13] == 0 or dt != "bf16" or c != 32 * ck or n != 64 * ck:
        return False
    if not ((k == 5 and ck == 1) or (k == 4 and ck == 1 and on >= 2) or (k == 4 and ck == 2 and on >= 3)):
        return False
    if oh != (ih - k) // 2 + 1 or ow != (iw - k) // 2 + 1 or ldb % 8 or ldb < k * k * c:
        return False
    t, gh, gw, halo = slot_grid("conv", k, oh, ow)
    if halo > RC_MAXHALO[(k, ck)] or gw <= 16:
        return False
    return not (kn[13] == 1 and B * gh * gw < 75000)


def gather_narrow_ok(dt, B, ih, iw, c, oh, ow, n, k, mask, kn):
    """try_gather_narrow (plain form: an output tensor, no fused loss)."""
    if not kn[4] or mask or 4 * n > 32 or k < 3 or k > 6:
        return False
    pa = c * esz(dt)
    if pa not in (64, 128) or (2 * n * esz(dt)) % 4:
        return False
    if slot_grid("gather", k, oh, ow)[3] > TC_MAXHALO:
        return False
    return dt == "bf16" or pa == 128


def narrow_conv_ok(dt, src, B, ih, iw, cs, k, cout, kn):
    """try_narrow_conv; src: 'bf16' | 'f32' | 'u8' | 'x3' (the source tensor's element type)."""
    if not kn[4] or cout != 32 or k > 4:
        return False
    run, K = k * cs, k * k * cs
    if run % 4 or K > 48:
        return False
    if dt == "f32" and src != "f32":
        return False
    if dt == "x3" and src not in ("f32", "x3"):
        return False
    if dt == "bf16" and src == "x3":
        return False
    ssz = {"u8": 1, "f32": 4, "x3": 4, "bf16": 2}[src]
    if (iw * cs * ssz) % (2 * ssz) or (ih * iw * cs * ssz) % (2 * ssz):
        return False
    if (K * esz(dt)) % 16:
        return False
    oh, ow = (ih - k) // 2 + 1, (iw - k) // 2 + 1
    return oh * ow >= 32


def narrow_wgrad_plan(dt, src, B, ih, iw, cs, oh, ow, nwide, k, kn):
    """try_narrow_wgrad: None or {ppw, capped, nwave, blocks, nwv}.  src: 'bf16' | 'f32' | 'u8'."""
    if not kn[4] or dt != "bf16":
        return None
    run = k * cs
    if nwide != 32 or k > 4 or run > 12 or run % 4 or k * run > 64:
        return None
    nsz = {"u8": 1, "f32": 4, "bf16": 2}[src]
    if (iw * cs * nsz) % (2 * nsz) or (ih * iw * cs * nsz) % (2 * nsz):
        return None
    M = B * oh * ow
    if M >= 1 << 26:
        return None
    ppw = ceil_div(ceil_div(M, NW_GRID_WAVES), NW_BP) * NW_BP
    if oh * ow < NW_BP:
        return None
    capped = ppw > 2 * oh * ow
    if capped:
        ppw = 2 * oh * ow // NW_BP * NW_BP
    nwave = ceil_div(M, ppw)
    nwv = 12 if (src == "u8" or kn[10] >= 12) else (8 if kn[10] >= 8 else 4)
    return {"ppw": ppw, "capped": capped, "nwave": nwave, "nwv": nwv, "blocks": ceil_div(nwave, nwv)}


def tapwgrad_plan(form, B, ih, iw, c, oh, ow, n, k, kn, dbias):
    """try_tapwgrad on bf16 tensors a [B, ih, iw, c] (slot side), d [B, oh, ow, n]: None (not eligible: shape, or more than 32 live (tap, tile) pairs) or the launch's
    plan {family, MP, splits, grid_splits, gy, npairs, slab_bytes, bias_bytes, bias_slabs_possible}."""
    if not kn[3] or k < 3 or k > 6 or c % 8 or n % 8:
        return None
    taps = (k + 1) // 2
    if form == "conv":
        if taps != 2 or (4 * c) % 128 or n % 64:
            return None
        kc, ne, kcb, neb = 4 * c, n, 128, 64
    else:
        kc, ne = c, 4 * n
        if taps == 2:
            if c % 128 or n % 64:
                return None
            kcb, neb = 128, 64
        else:
            if c % 64 or n != 32:
                return None
            kcb, neb = 64, 128
    t, gh, gw, halo = slot_grid(form, k, oh, ow)
    if halo > TC_MAXHALO:
        return None
    mp = B * gh * gw
    gy = (kc // kcb) * (ne // neb)
    npairs = 0
    for tap in range(taps * taps):
        for nt in range(neb // 32):
            valid = True
            if form == "gather" and neb == 4 * n:
                ta, tb = tap // taps, tap % taps
                valid = (nt >> 1) + 2 * (taps - 1 - ta) < k and (nt & 1) + 2 * (taps - 1 - tb) < k
            if valid:
                if npairs >= 32:
                    return None
                npairs += 1
    splits = max(1, kn[9] // gy)
    pps = ceil_div(ceil_div(mp, splits), TW_BP) * TW_BP
    splits = ceil_div(mp, pps)
    slab_floats = gy * npairs * (4 if taps == 2 else 2) * 1024
    slab_bytes = ceil_div(splits * slab_floats * (2 if kn[18] else 4), 256) * 256
    split_layout = bool(kn[7]) and taps == 2 and npairs == 8
    bias_bytes = splits * (2 if split_layout else 1) * ne * 4 if dbias else 0
    fam = "tapwgrad.conv" if form == "conv" else ("tapwgrad.gather4" if taps == 2 else "tapwgrad.gather5")
    return {"family": fam, "MP": mp, "splits": splits, "grid_splits": ceil_div(splits, 8) * 8, "gy": gy, "npairs": npairs, "nkb": kc // kcb,
            "slab_bytes": slab_bytes, "bias_bytes": bias_bytes, "slabs_possible": splits > 1 and (not dbias or n <= 256), "split_layout": split_layout}


def gen1_conv_ok(dt, in_f32, ih, iw, c, k):
    """conv_form_gemm / launch_wgrad, first-generation kernels: 'plain' | 'merged' | None (MI_ERR_SHAPE)."""
    v = 4 if (dt != "bf16" or in_f32) else 8
    if c % v == 0:
        return "plain"
    if (k * c) % 4 == 0 and (iw * c) % 2 == 0 and (ih * iw * c) % 2 == 0:
        return "merged"
    return None


def gen1_wgrad_plan(dt, M, Kc, N, target=GEN1_WGRAD_TARGET):
    """wgrad_splits / prepare_wgrad: {splits, mps, slab_bytes, wide}.  target: the launch's target block count (the layer-op entry points' 1024; the dense entry
    points pass tuning key 11)."""
    bp = WGRAD_BP[dt]
    gx, gy = (ceil_div(Kc, 128) if Kc > 64 else 1), ceil_div(N, 64)
    splits = max(1, target // (gx * gy))
    mps = max(bp, ceil_div(ceil_div(M, splits), bp) * bp)
    splits = ceil_div(M, mps)
    return {"splits": splits, "mps": mps, "wide": Kc > 64, "slab_bytes": splits * ceil_div(Kc * N, 4) * 4 * 4}


def gemm2_tile(N, M_grid, gz, K, dt, kn):
    """launch_gemm2_tiles: (BM, BN, stages)."""
    nk = ceil_div(K * esz(dt), 128)
    st64 = kn[20] if nk >= 6 else 2
    st64 = 4 if st64 >= 4 else (3 if st64 == 3 else 2)
    if N <= 32:
        return (256, 32, 2)
    if N <= 64:
        return (128, 64, st64)
    if kn[17] == 1 or (kn[17] == 0 and ceil_div(M_grid, 128) * ceil_div(N, 64) * gz < 512):
        return (64, 64, 2)
    gx = ceil_div(M_grid, 128)
    if kn[17] == 3 or gx * ceil_div(N, 128) * gz >= 384:
        return (128, 128, 3 if (kn[17] == 3 and kn[20] >= 3 and nk >= 6) else 2)
    return (128, 64, st64)


def family_of(c):
    """-> (family, plan): the kernel family the entry point's order of trial ends in for this case, with the launch's derived sizes where a predicate computes them.
    'refused:<why>' = the entry point returns an error and launches nothing."""
    kn = knobs_of(c)
    o = c.opt
    OH, OW = out_hw(c)
    dt, k = c.dt, c.k
    if c.entry in ("conv.fwd", "deconv.dgrad"):
        form, B, ih, iw, ci, oh, ow, n = tap_args(c)
        wT = o.get("wT", 1)
        frames = o.get("frames") if c.entry == "conv.fwd" else None
        src = {"u8": "u8", "f32": "f32", "bf16": "bf16", None: "f32" if dt == "f32" else dt}[frames]
        if wT and narrow_conv_ok(dt, src, B, ih, iw, ci, k, n, kn):
            return "narrow_conv", {"M": B * oh * ow, "lean": dt == "bf16" and k == 4 and k * ci == 12 and c.entry == "conv.fwd" and o.get("bias", True) and o.get("relu", True)}
        if frames == "u8":
            return "refused:uint8 frames off the narrow kernel", None
        in_f32 = frames == "f32"
        K = k * k * ci
        if wT and not (in_f32 and dt != "f32") and not o.get("idx"):
            if rwconv_conv_ok(dt, B, ih, iw, ci, oh, ow, n, k, K, kn):
                return "rwconv.conv", {"GW": slot_grid("conv", k, oh, ow)[2], "halo": slot_grid("conv", k, oh, ow)[3]}
            p = tapconv_plan("conv", dt, B, ih, iw, ci, oh, ow, n, k, K, kn)
            if p:
                return "tapconv.conv", p
            if kn[0] and (ci * esz(dt)) % 16 == 0 and (K * esz(dt)) % 16 == 0:
                return "gemm2.conv", {"tile": gemm2_tile(n, B * oh * ow, 1, K, dt, kn), "M": B * oh * ow, "K": K}
        g = gen1_conv_ok(dt, in_f32, ih, iw, ci, k)
        if g is None:
            return "refused:merged path", None
        return "gen1", {"path": g, "M": B * oh * ow, "BN": 32 if n <= 32 else (64 if n <= 64 else 128)}
    if c.entry in ("deconv.fwd", "conv.dgrad"):
        form, B, ih, iw, ci, oh, ow, n = tap_args(c)
        mask = c.entry == "conv.dgrad" and o.get("mask", True)
        relu = c.entry == "deconv.fwd" and o.get("relu", True)
        if ci % (8 if dt == "bf16" else 4):
            return "refused:deconv C not a vector multiple", None
        if k < 2:
            return "refused:k < 2", None
        if gather_narrow_ok(dt, B, ih, iw, ci, oh, ow, n, k, mask, kn):
            return "gather_narrow", {"MP": B * slot_grid("gather", k, oh, ow)[1] * slot_grid("gather", k, oh, ow)[2]}
        if rwconv_gather_ok(dt, B, ih, iw, ci, oh, ow, n, k, relu, mask, kn):
            return "rwconv.gather", {"GW": slot_grid("gather", k, oh, ow)[2], "halo": slot_grid("gather", k, oh, ow)[3]}
        p = tapconv_plan("gather", dt, B, ih, iw, ci, oh, ow, n, k, 0, kn)
        if p:
            return "tapconv.gather", p
        maxM = B * ((oh + 1) // 2) * ((ow + 1) // 2)
        if kn[0] and n > 32 and (ci * esz(dt)) % 16 == 0 and k <= 6:
            return "gemm2.gather", {"tile": gemm2_tile(n, maxM, 4, ((k + 1) // 2) ** 2 * ci, dt, kn), "utap": (ci * esz(dt)) % 128 == 0, "maxM": maxM}
        return "gen1", {"path": "gather", "M": maxM, "BN": 32 if n <= 32 else (64 if n <= 64 else 128)}
    # ---- filter gradients ----
    dbias = bool(o.get("dbias"))
    scratch = o.get("scratch", "none")
    if c.entry == "conv.wgrad":
        frames = o.get("frames")
        src = {"u8": "u8", "f32": "f32", "bf16": "bf16", None: "f32" if dt == "f32" else "bf16"}[frames]
        nw = narrow_wgrad_plan(dt, src, c.B, c.IH, c.IW, c.C, OH, OW, c.N, k, kn)
        if nw:
            return "narrow_wgrad", nw
        if frames == "u8":
            return "refused:uint8 frames off the narrow kernel", None
        form, a, d = "conv", (c.IH, c.IW, c.C), (OH, OW, c.N)
        tap_allowed = not o.get("idx") and not frames
        big, Cbig = (c.IH, c.IW), c.C
        small_n = c.N
        in_f32 = frames == "f32"
    else:
        nw = None if dbias else narrow_wgrad_plan(dt, "bf16", c.B, OH, OW, c.N, c.IH, c.IW, c.C, k, kn)
        if nw:
            return "narrow_wgrad", nw
        form, a, d = "gather", (c.IH, c.IW, c.C), (OH, OW, c.N)
        tap_allowed = True
        big, Cbig = (OH, OW), c.N
        small_n = c.C
        in_f32 = False
    if tap_allowed:
        if dt == "bf16":
            p = tapwgrad_plan(form, c.B, a[0], a[1], a[2], d[0], d[1], d[2], k, kn, dbias)
            if p:
                return p["family"], p
        elif dt == "x3" and kn[21] and scratch in ("big",) and (k + 1) // 2 == 2:
            c2, n2 = 2 * a[2], 2 * d[2]
            shape_ok = ((8 * a[2]) % 128 == 0 and n2 % 64 == 0) if form == "conv" else (c2 % 128 == 0 and n2 % 64 == 0)
            if shape_ok and (kn[21] == 2 or (form == "conv" and a[2] * d[2] <= 64 * 128)):
                p = tapwgrad_plan(form, c.B, a[0], a[1], c2, d[0], d[1], n2, k, kn, dbias)
                if p:
                    return p["family"], dict(p, x3=True)
    g = gen1_conv_ok(dt, in_f32, big[0], big[1], Cbig, k)
    if g is None:
        return "refused:merged path", None
    M = c.B * (OH * OW if c.entry == "conv.wgrad" else c.IH * c.IW)
    return "gen1", dict(gen1_wgrad_plan(dt, M, k * k * Cbig, small_n), path=g, M=M)


# ---------------------------------------------------------------------------------------------------------------------------------------
# inputs and float64 references
# ---------------------------------------------------------------------------------------------------------------------------------------
def _nchw(a):
    return a.permute(0, 3, 1, 2)


def _nhwc(a):
    return a.permute(0, 2, 3, 1).contiguous()


def plant(mask):
    """An exact 0.0 and a negative value in every mask: `> 0`, not `>= 0`, is what passes."""
    f = mask.reshape(-1)
    f[0] = 0.0
    f[1] = -abs(f[1]) - 0.5
    if f.size > 2:
        f[2] = abs(f[2]) + 0.5
    return mask


def make_inputs(c):
    """numpy float32 (uint8 for camera-byte frames) inputs of a case, from the case's own fixed seed."""
    rng = np.random.RandomState(1000 + c.id)
    OH, OW = out_hw(c)
    k, o = c.k, c.opt
    d = {}
    nfr = o.get("nframes", c.B)
    if o.get("frames") == "u8":
        d["x_u8"] = rng.randint(0, 256, (nfr, c.IH, c.IW, c.C)).astype(np.uint8)
        d["x"] = d["x_u8"].astype(np.float32) / np.float32(255.0)
    else:
        d["x"] = rng.randn(nfr, c.IH, c.IW, c.C).astype(np.float32)
    d["idx"] = (np.arange(c.B, dtype=np.int32)[::-1].copy() if o["idx"] == "reversed" else np.array(o["idx"], np.int32)) if o.get("idx") else None
    if c.entry.startswith("conv."):
        d["w"] = (rng.randn(k, k, c.C, c.N) / np.sqrt(k * k * c.C)).astype(np.float32)             # HWIO
    else:
        d["w"] = (rng.randn(k, k, c.N, c.C) / np.sqrt(k * k * c.C / 4)).astype(np.float32)         # [kh, kw, out, in]
    d["b"] = (0.1 * rng.randn(c.N)).astype(np.float32)
    d["dy"] = rng.randn(c.B, OH, OW, c.N).astype(np.float32)
    d["mask"] = plant(rng.randn(c.B, c.IH, c.IW, c.C).astype(np.float32))
    d["dw0"] = (0.25 * rng.randn(*d["w"].shape)).astype(np.float32)                                # the filter / bias gradient buffers start non-zero: the call accumulates
    d["db0"] = (0.25 * rng.randn(c.N)).astype(np.float32)
    return d


def reference(c, d):
    """float64 statements of the case's op on the values the kernel reads: {'out'} (fwd, dgrad) or {'dw', 'db', 'dw_scale', 'db_scale'} (wgrad), numpy float64."""
    td = DT[c.dt][1]
    o = c.opt
    x = d["x"][d["idx"]] if d["idx"] is not None else d["x"][:c.B]
    xr = rounded(x, td).requires_grad_(True)
    wr = rounded(d["w"], td).requires_grad_(True)
    conv = c.entry.startswith("conv.")
    if conv:
        y = F.conv2d(_nchw(xr), wr.permute(3, 2, 0, 1), None, stride=2)
    else:
        y = F.conv_transpose2d(_nchw(xr), wr.permute(3, 2, 0, 1), None, stride=2)
    if c.entry.endswith(".fwd"):
        if o.get("bias", True):
            y = y + torch.from_numpy(d["b"]).double().reshape(1, -1, 1, 1)
        if o.get("relu", True):
            y = F.relu(y)
        return {"out": _nhwc(y).detach().numpy()}
    dyr = rounded(d["dy"], td)
    y.backward(_nchw(dyr))
    if c.entry.endswith(".dgrad"):
        g = xr.grad
        if o.get("mask", True):
            g = g * (rounded(d["mask"], td) > 0)
        return {"out": g.numpy()}
    dw = wr.grad.numpy()
    db = dyr.sum((0, 1, 2)).numpy()
    return {"dw": d["dw0"].astype(np.float64) + dw, "db": d["db0"].astype(np.float64) + db, "dw_scale": float(np.abs(dw).max()), "db_scale": float(np.abs(db).max())}


def unreached(c):
    """conv.dgrad: boolean [IH, IW] of the input pixels no VALID stride-2 window reaches (their gradient is an exact zero)."""
    OH, OW = out_hw(c)
    m = np.ones((c.IH, c.IW), bool)
    m[:2 * (OH - 1) + c.k, :2 * (OW - 1) + c.k] = False
    return m


# ---------------------------------------------------------------------------------------------------------------------------------------
# the case table.  Nothing searches: every shape is written down with the derivation of its size.
# ---------------------------------------------------------------------------------------------------------------------------------------
CASES = []


def add(entry, dt, B, IH, IW, C, N, k, tune_, family, tags, why, **opt):
    CASES.append(Case(len(CASES), entry, dt, B, IH, IW, C, N, k, tune_, family, tuple(tags.split()), why, opt))


# ---- tapconv, conv form (conv.fwd on K-contiguous weights, deconv.dgrad): slot grid GH x GW = (OH + T - 1) x (OW + T - 1), T = (k + 1) // 2, KC = 4 C ----------------
# channel stages are 128 bytes: 64 bf16 / 32 fp32 channels of the 4 C per slot
add("conv.fwd", "bf16", 2, 7, 9, 8, 40, 3, TAP_BIG, "tapconv.conv", "k3 kc_below_stage n_ragged", "k = 3 on the 2 x 2-tap kernel (kernel row / column 3 does not exist); KC = 32 < 64; N = 40 in a 64-wide tile")
add("conv.fwd", "bf16", 2, 8, 10, 24, 72, 4, TAP_BIG, "tapconv.conv", "k4 ragged_stage n_ragged", "KC = 96 = 1.5 stages; N = 72 = one 64-wide tile and 8")
add("conv.fwd", "f32", 2, 9, 11, 12, 136, 5, TAP_BIG, "tapconv.conv", "k5 ragged_stage n_ragged f32", "k = 5 on the 3 x 3-tap kernel; KC = 48 = 1.5 fp32 stages; N = 136 = one 128-wide tile and 8")
add("conv.fwd", "x3", 2, 10, 12, 20, 40, 6, TAP_BIG, "tapconv.conv", "k6 ragged_stage n_ragged x3", "k = 6 fills all 3 x 3 taps; KC = 80 = 2.5 split stages")
add("conv.fwd", "bf16", 2, 8, 10, 40, 64, 4, TAP_BIG, "tapconv.conv", "ragged_stage", "KC = 160 = 2.5 stages (an odd number of stages: the two-slice loop ends on its first half)")
add("conv.fwd", "bf16", 1, 8, 10, 72, 64, 4, TAP_BIG, "tapconv.conv", "ragged_stage", "KC = 288 = 4.5 stages")
add("conv.fwd", "f32", 2, 8, 10, 4, 64, 4, TAP_BIG, "tapconv.conv", "kc_below_stage f32", "KC = 16 < 32 fp32 channels")
add("deconv.dgrad", "x3", 2, 3, 4, 64, 12, 4, TAP_BIG, "tapconv.conv", "ragged_stage x3 mask", "deconv input gradient = conv form over dy [B, 8, 10, 12]: KC = 48 = 1.5 stages, ReluGrad mask")
add("deconv.dgrad", "bf16", 2, 3, 4, 40, 8, 3, TAP_BIG, "tapconv.conv", "k3 kc_below_stage n_ragged mask", "k = 3 deconv input gradient: dy [B, 7, 9, 8], KC = 32, 40 outputs, mask")
add("deconv.dgrad", "f32", 1, 3, 4, 136, 12, 5, TAP_BIG, "tapconv.conv", "k5 ragged_stage n_ragged f32 mask", "k = 5 deconv input gradient: dy [B, 9, 11, 12], 136 outputs, mask")
# MP = B GH GW against the 256-position tile (k = 4: GH = OH + 1, GW = OW + 1): 255 = 3 x 5 x 17, 256 = 2 x 8 x 16; 257 is prime (no grid has it): 258 = 3 x 2 x 43
add("conv.fwd", "bf16", 3, 10, 34, 8, 64, 4, TAP_BIG, "tapconv.conv", "mp_below", "MP = 3 x 5 x 17 = 255 = TC_BMT - 1", MP=255)
add("conv.fwd", "bf16", 2, 16, 32, 8, 64, 4, TAP_BIG, "tapconv.conv", "mp_at", "MP = 2 x 8 x 16 = 256 = TC_BMT", MP=256)
add("conv.fwd", "bf16", 3, 4, 86, 8, 64, 4, TAP_BIG, "tapconv.conv", "mp_past", "MP = 3 x 2 x 43 = 258: the second block holds two positions (257 is prime)", MP=258)
# the small tile (bf16, key 5 = 2): 126 = 3 x 6 x 7, 128 = 2 x 8 x 8, 129 = 1 x 3 x 43 (127 is prime)
add("conv.fwd", "bf16", 3, 12, 14, 8, 64, 4, TAP_SMALL, "tapconv.conv", "small mp_below", "small tile, MP = 3 x 6 x 7 = 126", MP=126, tile="small")
add("conv.fwd", "bf16", 2, 16, 16, 8, 64, 4, TAP_SMALL, "tapconv.conv", "small mp_at", "small tile, MP = 2 x 8 x 8 = 128", MP=128, tile="small")
add("conv.fwd", "bf16", 1, 6, 86, 8, 64, 4, TAP_SMALL, "tapconv.conv", "small mp_past", "small tile, MP = 3 x 43 = 129, halo 44", MP=129, tile="small")
# small tile halo: k = 4 conv form halo = GW + 1 = OW + 2: 48 at OW = 46 (IW = 94), 49 at OW = 47 (IW = 96) -> the big tile
add("conv.fwd", "bf16", 1, 4, 94, 8, 64, 4, TAP_SMALL, "tapconv.conv", "small halo_at", "small tile at its halo limit: GW = 47, halo 48", halo=48, tile="small")
add("conv.fwd", "bf16", 1, 4, 96, 8, 64, 4, TAP_SMALL, "tapconv.conv", "small halo_past", "halo 49: the launcher takes the big tile although key 5 asks for the small one", halo=49, tile="big")
# odd (IH - k): the last input row / column is read by no window
add("conv.fwd", "bf16", 2, 9, 10, 8, 64, 4, TAP_BIG, "tapconv.conv", "odd_h", "IH - k = 5 odd")
add("conv.fwd", "f32", 2, 8, 11, 4, 32, 4, TAP_BIG, "tapconv.conv", "odd_w f32", "IW - k = 7 odd")
add("conv.fwd", "x3", 2, 9, 11, 4, 32, 4, TAP_BIG, "tapconv.conv", "odd_hw x3", "both odd")
add("conv.fwd", "bf16", 2, 8, 10, 24, 64, 4, tune(TAP_BIG, k6=0), "tapconv.conv", "lds_epilogue ragged_stage", "the LDS-staged epilogue (key 6 = 0)", direct=False)
add("conv.fwd", "bf16", 2, 8, 10, 24, 64, 4, TAP_BIG, "tapconv.conv", "direct_epilogue ragged_stage", "the register epilogue on the same shape", direct=True)

# ---- tapconv, gather form (deconv.fwd, conv.dgrad): slot = input pixel, GH x GW = ((OH + 1) // 2 + T - 1) x ((OW + 1) // 2 + T - 1), KC = C, NE = 4 N, N % 32 == 0 ----
add("deconv.fwd", "bf16", 2, 2, 3, 8, 32, 3, TAP_BIG, "tapconv.gather", "k3 kc_below_stage n32", "k = 3: the odd parity classes own one tap per axis; KC = 8")
add("deconv.fwd", "bf16", 2, 2, 3, 24, 96, 4, TAP_BIG, "tapconv.gather", "k4 kc_below_stage n96", "N = 96: NE = 384 = three 128-wide tiles")
add("deconv.fwd", "f32", 2, 2, 3, 40, 32, 5, TAP_BIG, "tapconv.gather", "k5 ragged_stage n32 f32", "k = 5 with one parity class per 32-wide tile (the {0,3} | {1,2} wave split); KC = 40 = 1.25 fp32 stages")
add("deconv.fwd", "x3", 2, 2, 3, 20, 32, 6, TAP_BIG, "tapconv.gather", "k6 kc_below_stage n32 x3", "k = 6: every class owns all 3 x 3 taps")
add("deconv.fwd", "bf16", 2, 2, 3, 72, 64, 5, TAP_BIG, "tapconv.gather", "k5 ragged_stage", "k = 5, N = 64 (two classes per 128-wide tile); KC = 72 = 1.125 stages")
add("conv.dgrad", "bf16", 2, 9, 11, 32, 24, 4, TAP_BIG, "tapconv.gather", "k4 larger_input mask kc_below_stage", "conv input gradient into [9, 11]: the windows reach 8 x 10, row 8 and column 10 are exact zeros; mask")
add("conv.dgrad", "f32", 2, 9, 11, 32, 12, 5, TAP_BIG, "tapconv.gather", "k5 mask f32 kc_below_stage", "k = 5 conv input gradient, mask")
add("conv.dgrad", "x3", 2, 8, 11, 32, 20, 3, TAP_BIG, "tapconv.gather", "k3 larger_input mask x3", "k = 3 conv input gradient into [8, 11]: windows reach 7 x 11")
# halo = GW + 1 (k = 4, GW = IW + 2) | 2 GW + 2 (k = 5, GW = IW + 4) against TC_MAXHALO = 96
add("deconv.fwd", "bf16", 1, 1, 93, 8, 64, 4, TAP_BIG, "tapconv.gather", "halo_at", "k = 4: GW = 95, halo 96 = TC_MAXHALO", halo=96)
add("deconv.fwd", "bf16", 1, 1, 94, 8, 64, 4, TAP_BIG, "gemm2.gather", "halo_past falls_through", "k = 4: halo 97: tapconv refuses, gemm2 takes it", halo=97)
add("deconv.fwd", "bf16", 1, 1, 43, 8, 64, 5, TAP_BIG, "tapconv.gather", "halo_at k5", "k = 5: GW = 47, halo 96", halo=96)
add("deconv.fwd", "bf16", 1, 1, 44, 8, 64, 5, TAP_BIG, "gemm2.gather", "halo_past k5 falls_through", "k = 5: GW = 48, halo 98: gemm2", halo=98)
add("deconv.fwd", "bf16", 1, 1, 45, 8, 32, 4, TAP_SMALL, "tapconv.gather", "small halo_at", "small tile: GW = 47, halo 48", halo=48, tile="small")
add("deconv.fwd", "bf16", 1, 1, 46, 8, 32, 4, TAP_SMALL, "tapconv.gather", "small halo_past", "halo 49: the big tile", halo=49, tile="big")
# MP = B (IH + 2) (IW + 2) for k = 4: 255 = 3 x 5 x 17, 256 = 2 x 8 x 16, 258 = 2 x 3 x 43; small tile 126 = 3 x 6 x 7, 128 = 2 x 8 x 8, 129 = 1 x 3 x 43
add("deconv.fwd", "bf16", 3, 3, 15, 8, 32, 4, TAP_BIG, "tapconv.gather", "mp_below", "MP = 255", MP=255)
add("deconv.fwd", "bf16", 2, 6, 14, 8, 32, 4, TAP_BIG, "tapconv.gather", "mp_at", "MP = 256", MP=256)
add("deconv.fwd", "bf16", 2, 1, 41, 8, 32, 4, TAP_BIG, "tapconv.gather", "mp_past", "MP = 258", MP=258)
add("deconv.fwd", "bf16", 3, 4, 5, 8, 32, 4, TAP_SMALL, "tapconv.gather", "small mp_below", "small tile, MP = 126", MP=126, tile="small")
add("deconv.fwd", "bf16", 2, 6, 6, 8, 32, 4, TAP_SMALL, "tapconv.gather", "small mp_at", "small tile, MP = 128", MP=128, tile="small")
add("deconv.fwd", "bf16", 1, 1, 41, 8, 32, 4, TAP_SMALL, "tapconv.gather", "small mp_past", "small tile, MP = 129", MP=129, tile="small")
add("deconv.fwd", "bf16", 2, 2, 3, 24, 32, 4, tune(TAP_BIG, k6=0), "tapconv.gather", "lds_epilogue", "the LDS-staged epilogue (key 6 = 0)", direct=False)

# ---- gemm2 (key 1 = -1): conv form M = B OH OW, K = k k C; gather form per parity class ---------------------------------------------------------------------------
add("conv.fwd", "bf16", 3, 8, 10, 24, 24, 4, GEMM2, "gemm2.conv", "t256x32 ragged_m ragged_n ragged_k", "256 x 32 tile: M = 36, N = 24, K = 384 bytes 768 = 6 stages", tile=(256, 32, 2))
add("conv.fwd", "bf16", 3, 16, 20, 24, 40, 4, tune(GEMM2, k20=2), "gemm2.conv", "t128x64 stages2 nk_at ragged_m ragged_n", "128 x 64, nk = 6, two stages: M = 189", tile=(128, 64, 2))
add("conv.fwd", "bf16", 3, 16, 20, 24, 40, 4, tune(GEMM2, k20=3), "gemm2.conv", "t128x64 stages3 nk_at", "nk = 6: three stages", tile=(128, 64, 3))
add("conv.fwd", "bf16", 3, 16, 20, 24, 40, 4, tune(GEMM2, k20=4), "gemm2.conv", "t128x64 stages4 nk_at", "nk = 6: four stages", tile=(128, 64, 4))
add("conv.fwd", "bf16", 3, 16, 20, 16, 40, 4, tune(GEMM2, k20=4), "gemm2.conv", "t128x64 nk_below", "K = 256: nk = 4 < 6 keeps two stages whatever key 20 says", tile=(128, 64, 2))
add("conv.fwd", "bf16", 3, 16, 20, 8, 40, 5, tune(GEMM2, k20=3), "gemm2.conv", "t128x64 ragged_k k5", "k = 5: K = 200 elements = 3.125 stages", tile=(128, 64, 2))
add("conv.fwd", "f32", 3, 8, 10, 12, 72, 4, tune(GEMM2, k17=1), "gemm2.conv", "t64x64 ragged_m ragged_n f32", "64 x 64 tiles (key 17 = 1): M = 36, N = 72", tile=(64, 64, 2))
add("conv.fwd", "x3", 3, 16, 20, 12, 136, 3, tune(GEMM2, k17=3, k20=3), "gemm2.conv", "t128x128 nk_below ragged_n x3 k3", "128 x 128 tiles: K = 108 x 4 bytes = 3.4 stages -> nk = 4 < 6: two stages although key 20 asks for three", tile=(128, 128, 2))
add("conv.fwd", "bf16", 3, 16, 20, 24, 136, 4, tune(GEMM2, k17=3, k20=3), "gemm2.conv", "t128x128 stages3 ragged_n", "128 x 128 tiles, nk = 6: three stages", tile=(128, 128, 3))
add("conv.fwd", "bf16", 3, 16, 20, 24, 72, 4, tune(GEMM2, k17=2), "gemm2.conv", "t128x64 two_columns", "N > 64 on 128 x 64 tiles: two column blocks", tile=(128, 64, 2))
add("deconv.dgrad", "bf16", 2, 3, 4, 72, 24, 6, GEMM2, "gemm2.conv", "k6 mask ragged_n", "k = 6 deconv input gradient on gemm2, mask", tile=(128, 64, 2))
add("deconv.fwd", "bf16", 2, 3, 5, 64, 40, 4, GEMM2, "gemm2.gather", "utap_on n33_64", "C = 64 bf16 = 128 bytes: UTAP; N = 40", utap=True)
add("deconv.fwd", "bf16", 2, 3, 5, 24, 40, 4, GEMM2, "gemm2.gather", "utap_off n33_64", "C = 24: no UTAP", utap=False)
add("deconv.fwd", "f32", 2, 3, 5, 32, 136, 5, tune(GEMM2, k17=3), "gemm2.gather", "utap_on n_above_128 f32 k5", "fp32 C = 32 = 128 bytes; N = 136 on 128 x 128 tiles; k = 5", utap=True)
add("deconv.fwd", "x3", 2, 3, 5, 12, 136, 3, tune(GEMM2, k17=1), "gemm2.gather", "utap_off n_above_128 x3 k3", "k = 3, 64 x 64 tiles", utap=False)
add("conv.dgrad", "bf16", 2, 9, 11, 40, 24, 6, GEMM2, "gemm2.gather", "k6 mask larger_input", "k = 6 conv input gradient (gather N = 40) into [9, 11]: windows reach 8 x 10", utap=False)

# ---- first-generation kernels (GENERATIONS['gen1']) --------------------------------------------------------------------------------------------------------------
add("conv.fwd", "f32", 3, 8, 10, 4, 24, 4, GEN1, "gen1", "gemm_n32 ragged", "gemm_kernel BN = 32, N = 24, M = 36", wT=0, also_wT=True)
add("conv.fwd", "bf16", 3, 16, 20, 8, 40, 4, GEN1, "gen1", "gemm_n64 ragged", "BN = 64, N = 40, M = 189", wT=0, also_wT=True)
add("conv.fwd", "x3", 3, 16, 20, 4, 72, 4, GEN1, "gen1", "gemm_n128 ragged", "BN = 128, N = 72", wT=0, also_wT=True)
add("conv.fwd", "f32", 3, 8, 12, 1, 24, 4, GEN1, "gen1", "merged c1 odd_ow", "merged path, C = 1, OW = 5", wT=0, path="merged")
add("conv.fwd", "bf16", 3, 8, 12, 2, 40, 4, GEN1, "gen1", "merged c2 odd_ow", "merged path, C = 2 bf16 (4-byte vectors)", wT=0, path="merged")
add("conv.fwd", "x3", 3, 8, 12, 3, 24, 4, GEN1, "gen1", "merged c3 odd_ow", "merged path, C = 3 split storage", wT=0, path="merged")
add("conv.fwd", "bf16", 3, 8, 12, 3, 24, 4, GEN1, "gen1", "merged c3 frames_f32 repeated_idx", "fp32 frames read by the bf16 kernel through frame_idx = [2, 0, 2]", wT=0, frames="f32", nframes=4, idx=[2, 0, 2], path="merged")
add("conv.fwd", "x3", 3, 8, 12, 4, 40, 4, GEN1, "gen1", "frames_f32 repeated_idx", "fp32 frames read by the split kernel, C = 4 (plain path), frame_idx = [3, 3, 1]", wT=0, frames="f32", nframes=4, idx=[3, 3, 1], path="plain")
add("deconv.fwd", "bf16", 2, 3, 5, 8, 24, 4, GEN1, "gen1", "gather gemm_n32 ragged", "gather form on gemm_kernel, N = 24")
add("conv.dgrad", "f32", 2, 10, 12, 40, 12, 5, GEN1, "gen1", "gather gemm_n64 ragged mask larger_input k5", "k = 5 conv input gradient (gather N = 40)")
add("deconv.dgrad", "x3", 2, 3, 4, 72, 12, 4, GEN1, "gen1", "gemm_n128 ragged mask", "deconv input gradient, 72 outputs, plain weights", wT=0)
# wgrad_kernel: rows Kc = k k C of the big tensor (64 | 128 per block), splits of mps rows (multiples of BP = 16 / 64 / 32)
add("conv.wgrad", "f32", 1, 8, 10, 3, 40, 4, GEN1, "gen1", "wgrad kc_below_64 one_split m_below_bp merged", "Kc = 48, M = 12 < BP = 16: one split (scratch given, unused)", scratch="big", splits=1)
add("conv.wgrad", "f32", 3, 16, 20, 4, 40, 4, GEN1, "gen1", "wgrad kc_at_64 several_splits scratch", "Kc = 64, M = 189: 12 splits of 16 rows, slabs + ordered sum", scratch="exact", splits=12, twice=True)
add("conv.wgrad", "f32", 3, 16, 20, 4, 40, 4, GEN1, "gen1", "wgrad several_splits scratch_short", "256 bytes less scratch than the slabs need: atomics", scratch="short", splits=12)
add("conv.wgrad", "f32", 3, 16, 20, 8, 40, 4, GEN1, "gen1", "wgrad kc_above_64 several_splits no_scratch dbias", "Kc = 128: 128 rows per block; no scratch; bias gradient by the column sums", scratch="none", splits=12, dbias=True)
add("conv.wgrad", "bf16", 1, 8, 22, 8, 72, 4, GEN1, "gen1", "wgrad m_below_bp bf16", "M = 30 < BP = 64, N = 72", scratch="none", splits=1)
add("conv.wgrad", "x3", 3, 8, 12, 3, 24, 4, GEN1, "gen1", "wgrad merged x3 two_splits", "M = 3 x 3 x 5 = 45: two splits of 32 rows, merged C = 3", scratch="exact", splits=2)
add("conv.wgrad", "x3", 1, 8, 12, 3, 24, 4, GEN1, "gen1", "wgrad merged x3 m_below_bp", "M = 15 < BP = 32 (split storage)", scratch="none", splits=1)
add("deconv.wgrad", "bf16", 2, 3, 5, 8, 24, 4, GEN1, "gen1", "wgrad deconv", "deconv filter gradient on wgrad_kernel: big tensor dy [2, 8, 12, 24], M = 30", scratch="none", splits=1)

# ---- tapwgrad (bf16; split storage through try_tapwgrad_split with key 21 = 2) ----------------------------------------------------------------------------------------
TW = dict(NEW)
# conv form, k = 4: GH x GW = (OH + 1) x (OW + 1); MP against TW_BP = 128: 126 = 3 x 6 x 7, 128 = 2 x 8 x 8, 129 = 1 x 3 x 43
add("conv.wgrad", "bf16", 3, 12, 14, 32, 64, 4, tune(TW, k9=16), "tapwgrad.conv", "mp_below one_split scratch_unused dbias", "MP = 126: one split, no slabs although scratch was given", scratch="big", dbias=True, MP=126, splits=1)
add("conv.wgrad", "bf16", 2, 16, 16, 32, 64, 4, tune(TW, k9=16), "tapwgrad.conv", "mp_at one_split", "MP = 128: one step exactly", scratch="none", MP=128, splits=1)
add("conv.wgrad", "bf16", 1, 6, 86, 32, 64, 4, tune(TW, k9=64), "tapwgrad.conv", "mp_past scratch_exact dbias two_runs", "MP = 129: two splits (the second holds one position); scratch exactly slab + bias bytes", scratch="exact", dbias=True, MP=129, splits=2, twice=True)
add("conv.wgrad", "bf16", 1, 6, 86, 32, 64, 4, tune(TW, k9=64), "tapwgrad.conv", "scratch_short dbias", "256 bytes less: atomics", scratch="short", dbias=True, MP=129, splits=2)
add("conv.wgrad", "bf16", 1, 6, 86, 32, 64, 4, tune(TW, k9=64), "tapwgrad.conv", "scratch_off8 dbias", "scratch offset by 8 bytes: atomics", scratch="off8", dbias=True, MP=129, splits=2)
add("conv.wgrad", "bf16", 1, 6, 86, 32, 64, 4, tune(TW, k9=64), "tapwgrad.conv", "no_dbias same_dw", "without dbias: the same dW bit for bit", scratch="exact", MP=129, splits=2, same_as_dbias=True)
# 9 splits on a grid rounded up to 16: key 9 = 64, gy = 1 -> 64 splits asked, MP = 3 x 16 x 22 = 1056 -> 17 -> 128 positions per split, 9 splits -> 16 x gy blocks, 7 idle
add("conv.wgrad", "bf16", 3, 32, 44, 32, 64, 4, tune(TW, k9=64), "tapwgrad.conv", "grid_rounds_up scratch_exact dbias decodes", "MP = 1056: 9 splits on a grid of 16: seven idle blocks", scratch="exact", dbias=True, MP=1056, splits=9, decodes=True, twice=True)
add("conv.wgrad", "bf16", 3, 32, 44, 32, 64, 4, tune(TW, k9=64, k7=0), "tapwgrad.conv", "pair_layout scratch_exact dbias decodes", "the pair layout (key 7 = 0) on the same shape", scratch="exact", dbias=True, MP=1056, splits=9, decodes=True)
add("conv.wgrad", "bf16", 3, 32, 44, 32, 64, 4, tune(TW, k9=64, k18=1), "tapwgrad.conv", "slab_bf16", "bf16 slabs (key 18): held to the bound of test_bf16_partial_sum_slabs_error_bound_at_batch_512", scratch="exact", dbias=True, MP=1056, splits=9, slab_bf16=True)
add("conv.wgrad", "bf16", 3, 16, 20, 32, 320, 4, tune(TW, k9=64), "tapwgrad.conv", "n320_dbias", "N = 320 > 256 with dbias: gy = 5, MP = 3 x 8 x 10 = 240 in 2 splits, but no bias_part, so no slabs either: atomics", scratch="big", dbias=True, splits=2, MP=240)
add("conv.wgrad", "bf16", 3, 16, 20, 96, 192, 4, tune(TW, k9=64), "tapwgrad.conv", "c96_n192 scratch_exact dbias", "C = 96 (KC = 384 = 3 row blocks), N = 192 (3 column blocks): gy = 9", scratch="exact", dbias=True, twice=True)
add("conv.wgrad", "bf16", 3, 21, 25, 32, 64, 3, tune(TW, k9=64), "tapwgrad.conv", "k3 scratch_exact dbias", "k = 3 conv form (MP = 3 x 11 x 13 = 429, 4 splits): kernel row / column 3 of the 2 x 2-tap result does not exist", scratch="exact", dbias=True, MP=429, splits=4)
add("conv.wgrad", "x3", 3, 32, 44, 16, 32, 4, tune(TW, k9=64, k21=2), "tapwgrad.conv", "x3_split", "split storage on the doubled-channel bf16 kernel (C' = 32, N' = 64) + fold", scratch="big", dbias=True, x3=True)
# gather form
add("deconv.wgrad", "bf16", 3, 1, 2, 256, 128, 4, tune(TW, k9=64), "tapwgrad.gather4", "c256_n128_1x2 scratch_exact dbias", "C = 256, N = 128 at a 1 x 2 image: MP = 3 x 3 x 4 = 36, one split", scratch="big", dbias=True, splits=1)
add("deconv.wgrad", "bf16", 3, 5, 19, 128, 64, 4, tune(TW, k9=64), "tapwgrad.gather4", "grid_rounds_up scratch_exact dbias decodes two_runs", "MP = 3 x 7 x 21 = 441: gy = 4, 16 splits asked -> pps = 128 -> 4 splits on a grid of 8", scratch="exact", dbias=True, MP=441, splits=4, decodes=True, twice=True)
add("deconv.wgrad", "bf16", 3, 5, 19, 128, 64, 3, tune(TW, k9=64), "tapwgrad.gather4", "k3 scratch_exact dbias", "k = 3 gather form", scratch="exact", dbias=True)
add("deconv.wgrad", "bf16", 3, 5, 19, 128, 32, 5, tune(TW, k9=64), "tapwgrad.gather5", "k5_c128 scratch_exact dbias decodes", "k = 5, C = 128: the pair-layout kernel with nkb = 2 (the class-wave kernel is C = 64 only)", scratch="exact", dbias=True, nkb=2, decodes=True)
add("deconv.wgrad", "bf16", 3, 5, 19, 64, 32, 5, tune(TW, k9=64), "tapwgrad.gather5", "k5_c64_off_shape scratch_exact dbias decodes two_runs", "k = 5, C = 64 off the model's 18 x 38: the class-wave kernel", scratch="exact", dbias=True, nkb=1, decodes=True, twice=True)
# gather k = 4: MP = B (IH + 2) (IW + 2): 126 = 3 x 6 x 7, 128 = 2 x 8 x 8, 129 = 1 x 3 x 43;  gather k = 5: MP = B (IH + 4) (IW + 4), both factors >= 5: 126 = 3 x 6 x 7,
# 128 = 2 x 8 x 8, 129 = 3 x 43 has no such grid: 130 = 2 x 5 x 13
add("deconv.wgrad", "bf16", 3, 4, 5, 128, 64, 4, tune(TW, k9=16), "tapwgrad.gather4", "mp_below one_split dbias", "MP = 126, one split", scratch="big", dbias=True, MP=126, splits=1)
add("deconv.wgrad", "bf16", 2, 6, 6, 128, 64, 4, tune(TW, k9=16), "tapwgrad.gather4", "mp_at one_split", "MP = 128", scratch="none", MP=128, splits=1)
add("deconv.wgrad", "bf16", 1, 1, 41, 128, 64, 4, tune(TW, k9=64), "tapwgrad.gather4", "mp_past scratch_exact dbias two_runs", "MP = 129: two splits", scratch="exact", dbias=True, MP=129, splits=2, twice=True)
add("deconv.wgrad", "bf16", 3, 5, 19, 128, 64, 4, tune(TW, k9=64), "tapwgrad.gather4", "scratch_short dbias", "256 bytes less: atomics", scratch="short", dbias=True, MP=441, splits=4)
add("deconv.wgrad", "bf16", 3, 5, 19, 128, 64, 4, tune(TW, k9=64), "tapwgrad.gather4", "scratch_off8 dbias", "scratch offset by 8: atomics", scratch="off8", dbias=True, MP=441, splits=4)
add("deconv.wgrad", "bf16", 3, 5, 19, 128, 64, 4, tune(TW, k9=64), "tapwgrad.gather4", "no_dbias same_dw", "without dbias: the same dW", scratch="exact", MP=441, splits=4, same_as_dbias=True)
add("deconv.wgrad", "bf16", 3, 5, 19, 128, 64, 4, tune(TW, k9=64, k7=0), "tapwgrad.gather4", "pair_layout scratch_exact dbias decodes", "8 pairs: the pair layout (key 7 = 0)", scratch="exact", dbias=True, MP=441, splits=4, decodes=True)
add("deconv.wgrad", "bf16", 3, 5, 19, 128, 64, 4, tune(TW, k9=64, k18=1), "tapwgrad.gather4", "slab_bf16", "bf16 slabs", scratch="exact", dbias=True, MP=441, splits=4, slab_bf16=True)
add("deconv.wgrad", "bf16", 3, 2, 3, 64, 32, 5, tune(TW, k9=16), "tapwgrad.gather5", "mp_below one_split dbias", "k = 5: MP = 126, one split: no slabs, the pair-layout kernel", scratch="big", dbias=True, MP=126, splits=1)
add("deconv.wgrad", "bf16", 2, 4, 4, 64, 32, 5, tune(TW, k9=16), "tapwgrad.gather5", "mp_at one_split", "k = 5: MP = 128", scratch="none", MP=128, splits=1)
add("deconv.wgrad", "bf16", 2, 1, 9, 64, 32, 5, tune(TW, k9=64), "tapwgrad.gather5", "mp_past scratch_exact dbias two_runs", "k = 5: MP = 130: two splits", scratch="exact", dbias=True, MP=130, splits=2, twice=True)
add("deconv.wgrad", "bf16", 3, 5, 19, 64, 32, 5, tune(TW, k9=64), "tapwgrad.gather5", "scratch_short dbias", "k = 5, 256 bytes less: atomics on the pair-layout kernel", scratch="short", dbias=True, MP=621, splits=5)
add("deconv.wgrad", "bf16", 3, 5, 19, 64, 32, 5, tune(TW, k9=64), "tapwgrad.gather5", "scratch_off8 dbias", "k = 5, scratch offset by 8", scratch="off8", dbias=True, MP=621, splits=5)
add("deconv.wgrad", "bf16", 3, 5, 19, 64, 32, 5, tune(TW, k9=64), "tapwgrad.gather5", "no_dbias same_dw", "k = 5 without dbias: the same dW", scratch="exact", MP=621, splits=5, same_as_dbias=True)
add("deconv.wgrad", "bf16", 3, 5, 19, 64, 32, 5, tune(TW, k9=64, k18=1), "tapwgrad.gather5", "slab_bf16", "k = 5, bf16 slabs", scratch="exact", dbias=True, MP=621, splits=5, slab_bf16=True)
add("deconv.wgrad", "bf16", 3, 5, 19, 64, 32, 6, tune(TW, k9=64), "gen1", "k6_gather falls_through", "k = 6: 36 live pairs, try_tapwgrad returns 0: the first-generation kernel", scratch="big", dbias=True)

# ---- rwconv (key 13 = 2) --------------------------------------------------------------------------------------------------------------------------------------------
for blocks in (0, 1, 2):
    RW = tune(GENERATIONS["rwconv"], k16=blocks)
    # gather form 64 -> 32: k = 4 GW = IW + 2, k = 5 GW = IW + 4; taken for 32 < GW <= 47
    add("deconv.fwd", "bf16", 2, 2, 31, 64, 32, 4, RW, "rwconv.gather", "gw_33 k4", "k = 4, GW = 33: just above the incremental slot decode's limit", GW=33)
    add("deconv.fwd", "bf16", 2, 2, 45, 64, 32, 4, RW, "rwconv.gather", "gw_47 k4", "k = 4, GW = 47: halo 48 = MAXHALO", GW=47)
    add("deconv.fwd", "bf16", 2, 2, 29, 64, 32, 5, RW, "rwconv.gather", "gw_33 k5", "k = 5, GW = 33", GW=33)
    add("conv.dgrad", "bf16", 2, 7, 89, 32, 64, 5, RW, "rwconv.gather", "gw_47 k5 mask", "k = 5 conv input gradient, dy [2, 2, 43, 64]: GW = 47, halo 96 = MAXHALO; mask", GW=47)
    add("conv.dgrad", "bf16", 2, 6, 64, 32, 64, 4, RW, "rwconv.gather", "gw_33 k4 mask", "k = 4 conv input gradient, dy [2, 2, 31, 64]: GW = 33; mask", GW=33)
    add("deconv.fwd", "bf16", 2, 3, 1, 128, 64, 4, RW, "rwconv.gather", "wide iw_1", "128 -> 64, IW = 1: GW = 3", GW=3)
    add("deconv.fwd", "bf16", 2, 2, 45, 128, 64, 4, RW, "rwconv.gather", "wide gw_47", "128 -> 64, GW = 47: halo 48", GW=47)
    add("conv.dgrad", "bf16", 2, 6, 92, 64, 128, 4, RW, "rwconv.gather", "wide gw_47 mask", "128 -> 64 as conv3's input gradient, dy [2, 2, 45, 128]; mask", GW=47)
RW = tune(GENERATIONS["rwconv"], k16=1)
add("conv.dgrad", "bf16", 2, 6, 92, 32, 64, 4, RW, "rwconv.gather", "gw_47 k4 mask", "k = 4 conv input gradient, dy [2, 2, 45, 64]: GW = 47, halo 48; mask", GW=47)
add("conv.dgrad", "bf16", 2, 8, 4, 64, 128, 4, RW, "rwconv.gather", "wide iw_1 mask", "128 -> 64 as an input gradient, dy [2, 3, 1, 128]: GW = 3; mask", GW=3)
add("deconv.fwd", "bf16", 2, 2, 43, 64, 32, 5, RW, "rwconv.gather", "gw_47 k5 relu", "k = 5 forward with bias + ReLU at GW = 47", GW=47)
add("conv.dgrad", "bf16", 2, 7, 61, 32, 64, 5, RW, "rwconv.gather", "gw_33 k5 mask", "k = 5 conv input gradient, dy [2, 2, 29, 64]: GW = 33; mask", GW=33)
add("deconv.fwd", "bf16", 2, 2, 30, 64, 32, 4, RW, "tapconv.gather", "gw_32 refused k4 falls_through", "k = 4, GW = 32: refused, tapconv takes it", GW=32)
add("deconv.fwd", "bf16", 2, 2, 46, 64, 32, 4, RW, "tapconv.gather", "gw_48 refused k4 falls_through", "k = 4, GW = 48: halo 49 refused", GW=48)
add("deconv.fwd", "bf16", 2, 2, 28, 64, 32, 5, RW, "tapconv.gather", "gw_32 refused k5 falls_through", "k = 5, GW = 32", GW=32)
add("deconv.fwd", "bf16", 2, 2, 44, 64, 32, 5, RW, "gen1", "gw_48 refused k5 falls_through", "k = 5, GW = 48: halo 98 is past tapconv's limit too, and N = 32 is not gemm2's: the first-generation kernel", GW=48)
# conv form (test_conv_form_register_weight_kernel_walks_runs_of_chunks moves the image size): GW = OW + T - 1 must exceed 16; halo limits 48 / 32 / 96
add("conv.fwd", "bf16", 2, 10, 35, 32, 64, 4, RW, "rwconv.conv", "gw_17", "32 -> 64, k = 4: OW = 16, GW = 17", GW=17)
add("conv.fwd", "bf16", 2, 10, 33, 32, 64, 4, RW, "tapconv.conv", "gw_16 refused falls_through", "GW = 16: refused, tapconv", GW=16)
add("conv.fwd", "bf16", 2, 6, 94, 32, 64, 4, RW, "rwconv.conv", "halo_at", "k = 4: GW = 47, halo 48", GW=47)
add("conv.fwd", "bf16", 2, 6, 96, 32, 64, 4, RW, "tapconv.conv", "halo_past refused falls_through", "k = 4: GW = 48, halo 49", GW=48)
add("deconv.dgrad", "bf16", 2, 3, 30, 128, 64, 4, RW, "rwconv.conv", "wide halo_at mask", "64 -> 128 as a deconv input gradient over dy [2, 8, 62, 64]: GW = 31, halo 32; mask", GW=31)
add("conv.fwd", "bf16", 2, 8, 64, 64, 128, 4, RW, "tapconv.conv", "wide halo_past refused falls_through", "64 -> 128: GW = 32, halo 33", GW=32)
add("conv.fwd", "bf16", 2, 9, 93, 32, 64, 5, RW, "rwconv.conv", "k5 halo_at", "k = 5: OW = 45, GW = 47, halo 96", GW=47)
add("conv.fwd", "bf16", 2, 9, 95, 32, 64, 5, RW, "gemm2.conv", "k5 halo_past refused falls_through", "k = 5: GW = 48, halo 98: past tapconv's limit too: gemm2", GW=48)

# ---- narrow kernels (key 4 = 1) -------------------------------------------------------------------------------------------------------------------------------------
NAR = dict(NEW)
# narrow_conv: Cs -> 32 channels, k k Cs <= 48, (k Cs) % 4 == 0; OH OW >= 32; 128 pixels per block
add("conv.fwd", "bf16", 2, 16, 18, 1, 32, 4, NAR, "narrow_conv", "cs1_k4 m_below", "Cs = 1: OH OW = 7 x 8 = 56, M = 112 < 128")
add("conv.fwd", "bf16", 3, 16, 16, 2, 32, 4, NAR, "narrow_conv", "cs2_k4 m_past", "Cs = 2: M = 3 x 49 = 147 = 128 + 19")
add("conv.fwd", "bf16", 1, 14, 22, 3, 32, 4, NAR, "narrow_conv", "cs3_k4 lean one_frame", "Cs = 3 (the lean form): one frame of OH OW = 6 x 10 = 60 pixels, half a block", lean=True)
add("conv.fwd", "bf16", 3, 10, 18, 3, 32, 4, NAR, "narrow_conv", "cs3_k4 lean ohw_32", "OH OW = 4 x 8 = 32 exactly: a wave's 32 pixels are one frame", lean=True)
add("conv.fwd", "bf16", 4, 8, 24, 3, 32, 4, NAR, "narrow_conv", "cs3_k4 lean ohw_33", "OH OW = 3 x 11 = 33: every wave but the first crosses a frame", lean=True)
add("conv.fwd", "bf16", 3, 4, 64, 3, 32, 4, NAR, "gen1", "ohw_31 refused falls_through", "OH OW = 1 x 31 = 31 < 32: refused; K-contiguous weights, C = 3: tapconv and gemm2 need 16-byte pixels: the merged first-generation path", path="merged")
add("conv.fwd", "bf16", 3, 10, 18, 2, 32, 2, NAR, "narrow_conv", "cs2_k2", "Cs = 2, k = 2: OH OW = 5 x 9 = 45")
add("conv.fwd", "f32", 3, 11, 19, 4, 32, 3, NAR, "narrow_conv", "cs4_k3 f32", "fp32, Cs = 4, k = 3: K = 36, OH OW = 5 x 9 = 45")
add("conv.fwd", "x3", 3, 10, 18, 3, 32, 4, NAR, "narrow_conv", "cs3_k4 x3", "split storage source")
add("conv.fwd", "bf16", 3, 10, 18, 3, 32, 4, NAR, "narrow_conv", "frames_u8 repeated_idx lean", "camera bytes through frame_idx = [2, 0, 2]", frames="u8", nframes=4, idx=[2, 0, 2], lean=True)
add("conv.fwd", "bf16", 3, 10, 18, 3, 32, 4, NAR, "narrow_conv", "frames_f32 repeated_idx lean", "fp32 frames through frame_idx", frames="f32", nframes=4, idx=[1, 1, 3], lean=True)
add("conv.fwd", "bf16", 3, 10, 18, 3, 32, 4, NAR, "narrow_conv", "frames_bf16 repeated_idx lean", "bf16 frames through frame_idx = [3, 0, 3]", frames="bf16", nframes=4, idx=[3, 0, 3], lean=True)
add("conv.fwd", "x3", 3, 10, 18, 1, 32, 4, NAR, "narrow_conv", "frames_f32 repeated_idx x3 cs1", "fp32 frames read by the split kernel", frames="f32", nframes=4, idx=[3, 0, 3])
add("deconv.dgrad", "bf16", 3, 4, 8, 32, 3, 4, NAR, "narrow_conv", "cs3_k4 mask", "deconv4's input gradient off its shape: dy [3, 10, 18, 3], mask (first-generation form: a tensor mask is not the lean form's)", lean=False)
add("deconv.dgrad", "f32", 3, 4, 8, 32, 1, 4, NAR, "narrow_conv", "cs1_k4 mask f32", "fp32, one logit channel")
# narrow_wgrad: OH OW >= 16
add("conv.wgrad", "bf16", 3, 8, 12, 3, 32, 4, tune(NAR, k10=12), "gen1", "ohw_15 refused falls_through wgrad merged", "OH OW = 3 x 5 = 15 < NW_BP: refused; C = 3 is not tapwgrad's: the merged first-generation kernel", scratch="big", dbias=True, path="merged")
add("conv.wgrad", "bf16", 3, 10, 10, 3, 32, 4, tune(NAR, k10=12), "narrow_wgrad", "cs3_k4 ohw_16 waves12 scratch dbias two_runs", "OH OW = 4 x 4 = 16 = NW_BP", scratch="big", dbias=True, twice=True)
add("conv.wgrad", "bf16", 3, 10, 10, 1, 32, 4, tune(NAR, k10=8), "narrow_wgrad", "cs1_k4 waves8 no_scratch", "Cs = 1, eight waves per block, atomics", scratch="none")
add("conv.wgrad", "bf16", 3, 10, 10, 2, 32, 4, tune(NAR, k10=4), "narrow_wgrad", "cs2_k4 waves4 scratch dbias", "Cs = 2, four waves per block", scratch="big", dbias=True)
add("conv.wgrad", "bf16", 3, 10, 10, 2, 32, 2, tune(NAR, k10=4), "narrow_wgrad", "cs2_k2 scratch", "Cs = 2, k = 2: OH OW = 25", scratch="big")
add("conv.wgrad", "bf16", 3, 10, 10, 3, 32, 4, NAR, "narrow_wgrad", "frames_u8 repeated_idx dbias scratch", "camera bytes through frame_idx", scratch="big", dbias=True, frames="u8", nframes=4, idx=[2, 0, 2])
add("conv.wgrad", "bf16", 3, 10, 10, 3, 32, 4, NAR, "narrow_wgrad", "frames_f32 repeated_idx no_scratch", "fp32 frames through frame_idx", scratch="none", frames="f32", nframes=4, idx=[1, 1, 3])
add("conv.wgrad", "bf16", 3, 10, 10, 3, 32, 4, NAR, "narrow_wgrad", "frames_bf16 repeated_idx scratch dbias", "bf16 frames through frame_idx", scratch="big", dbias=True, frames="bf16", nframes=4, idx=[3, 0, 3])
add("deconv.wgrad", "bf16", 3, 4, 4, 32, 3, 4, NAR, "narrow_wgrad", "deconv cs3_k4 scratch", "deconv4's filter gradient off its shape: narrow side dy [3, 10, 10, 3]", scratch="big")
# the ppw cap: pixels per wave = ceil(M / 3072) rounded up to 16, capped at 2 OH OW rounded DOWN to 16.  OH OW must be no multiple of 16, or every wave range is
# frame-aligned and the cap decides nothing: frames of 12 x 12 x 3 give OH OW = 25, cap 48; uncapped 64 needs ceil(M / 3072) > 48, M > 147456 = 5898.2 frames: B = 5900
# (M = 147500: 49 -> 64 uncapped).  A capped range of 48 pixels straddles three frames (e.g. pixels 24 .. 71), an uncapped one of 64 four (pixels 64 .. 127 = frames 2 .. 5):
# the kernel looks up three.  2.5 MB as camera bytes.
add("conv.wgrad", "bf16", 5900, 12, 12, 3, 32, 4, NAR, "narrow_wgrad", "ppw_cap scratch dbias", "B = 5900 tiny frames: the cap of 2 OH OW pixels per wave (three frames per wave range) bites", scratch="big", dbias=True, capped=True)
add("conv.wgrad", "bf16", 5900, 12, 12, 3, 32, 4, NAR, "narrow_wgrad", "ppw_cap frames_u8 dbias", "the same through camera bytes and a frame index that walks backwards", scratch="big", dbias=True, capped=True, frames="u8", nframes=5900, idx="reversed")
# gather_narrow: N <= 8 outputs, 64- or 128-byte pixels, no mask
for n_, k_, iw_ in ((1, 3, 5), (2, 4, 6), (3, 5, 5), (5, 6, 6), (8, 4, 5)):
    add("deconv.fwd", "bf16", 2, 3, iw_, 32, n_, k_, NAR, "gather_narrow", "n%d k%d c32 %s" % (n_, k_, "odd_ow" if (2 * iw_ - 2 + k_) % 2 else "even_ow"), "bf16 C = 32 (64-byte pixels), N = %d, k = %d" % (n_, k_))
add("deconv.fwd", "bf16", 2, 3, 5, 64, 3, 4, NAR, "gather_narrow", "n3 k4 c64", "bf16 C = 64: the CPR = 8 instantiation")
add("deconv.fwd", "bf16", 2, 3, 5, 64, 5, 5, NAR, "gather_narrow", "n5 k5 c64 odd_ow", "bf16 C = 64, generic stores, k = 5")
add("deconv.fwd", "f32", 2, 3, 5, 32, 3, 4, NAR, "gather_narrow", "n3 k4 f32", "fp32 C = 32")
add("deconv.fwd", "x3", 2, 3, 5, 32, 2, 5, NAR, "gather_narrow", "n2 k5 x3 odd_ow", "split storage C = 32")
add("deconv.fwd", "bf16", 3, 6, 18, 32, 3, 4, NAR, "gather_narrow", "n3 k4 mp_past", "MP = 3 x 8 x 20 = 480: four blocks of 128, the last ragged")
add("conv.dgrad", "bf16", 2, 8, 12, 3, 32, 4, NAR, "gather_narrow", "n3 k4 conv_dgrad", "conv1's input gradient (no mask): dy [2, 3, 5, 32] -> [2, 8, 12, 3]", mask=False)

# ---- refusals: MiError, nothing written -----------------------------------------------------------------------------------------------------------------------------
add("conv.fwd", "f32", 2, 8, 11, 1, 24, 4, GEN1, "refused:merged path", "refused odd_iwc", "merged path with odd IW C = 11", wT=0)
add("conv.fwd", "bf16", 2, 8, 11, 3, 24, 4, GEN1, "refused:merged path", "refused odd_iwc", "merged path with odd IW C = 33 (bf16)", wT=0)
add("conv.wgrad", "x3", 2, 8, 11, 3, 24, 4, GEN1, "refused:merged path", "refused odd_iwc wgrad", "filter gradient, merged path, odd IW C", scratch="none")
add("deconv.fwd", "bf16", 2, 3, 5, 12, 24, 4, NEW, "refused:deconv C not a vector multiple", "refused deconv_c", "deconv with C = 12 bf16 (not a multiple of 8)")
add("conv.dgrad", "f32", 2, 8, 12, 8, 6, 4, NEW, "refused:deconv C not a vector multiple", "refused deconv_c", "conv input gradient with N = 6 fp32 (not a multiple of 4)")
add("conv.fwd", "bf16", 2, 10, 18, 4, 32, 4, NAR, "refused:uint8 frames off the narrow kernel", "refused u8_off_narrow", "camera bytes with Cs = 4, k = 4: K = 64 > 48 is not the narrow kernel's", frames="u8")
add("conv.wgrad", "bf16", 2, 10, 18, 4, 32, 4, NAR, "refused:uint8 frames off the narrow kernel", "refused u8_off_narrow wgrad", "camera bytes, run = 16 > 12", frames="u8", scratch="none")

N_CASES = collections.Counter(c.family.split(":")[0] for c in CASES)

# every (family, boundary tag) pair the table must hold at least once (test_conv_shape_cases_host.py)
REQUIRED = {
    "tapconv.conv": "k3 k4 k5 k6 ragged_stage kc_below_stage n_ragged mp_below mp_at mp_past small halo_at halo_past odd_h odd_w odd_hw lds_epilogue direct_epilogue f32 x3 mask",
    "tapconv.gather": "k3 k4 k5 k6 ragged_stage kc_below_stage n32 n96 mp_below mp_at mp_past small halo_at halo_past larger_input lds_epilogue f32 x3 mask gw_32 gw_48",
    "gemm2.conv": "t256x32 t128x64 t64x64 t128x128 stages2 stages3 stages4 nk_at nk_below ragged_m ragged_n ragged_k f32 x3 k6",
    "gemm2.gather": "utap_on utap_off n33_64 n_above_128 halo_past k3 k5 k6 f32 x3",
    "gen1": "gemm_n32 gemm_n64 gemm_n128 merged c1 c2 c3 odd_ow frames_f32 repeated_idx wgrad kc_below_64 kc_at_64 kc_above_64 m_below_bp one_split several_splits scratch scratch_short no_scratch k6_gather",
    "tapwgrad.conv": "mp_below mp_at mp_past one_split scratch_exact scratch_short scratch_off8 no_dbias dbias n320_dbias grid_rounds_up c96_n192 k3 pair_layout decodes slab_bf16 x3_split",
    "tapwgrad.gather4": "c256_n128_1x2 grid_rounds_up k3 decodes mp_below mp_at mp_past one_split scratch_exact scratch_short scratch_off8 no_dbias pair_layout slab_bf16",
    "tapwgrad.gather5": "k5_c128 k5_c64_off_shape mp_below mp_at mp_past one_split scratch_exact scratch_short scratch_off8 no_dbias slab_bf16",
    "rwconv.gather": "gw_33 gw_47 k4 k5 wide iw_1 mask relu",
    "rwconv.conv": "gw_17 halo_at wide k5",
    "narrow_conv": "cs1_k4 cs2_k4 cs3_k4 cs2_k2 cs4_k3 m_below m_past ohw_32 ohw_33 lean frames_u8 frames_f32 frames_bf16 x3 f32 mask",
    "narrow_wgrad": "cs1_k4 cs2_k4 cs3_k4 cs2_k2 ohw_16 ppw_cap waves4 waves8 waves12 scratch no_scratch frames_u8 frames_f32 frames_bf16 deconv",
    "gather_narrow": "n1 n2 n3 n5 n8 k3 k4 k5 k6 c32 c64 f32 x3 odd_ow even_ow mp_past",
    "refused": "odd_iwc deconv_c u8_off_narrow",
}


def by_family(prefix):
    return [c for c in CASES if c.family.split(":")[0].startswith(prefix)]


def case_id(c):
    return "%s-%03d-%s-%s-%s" % (c.family.split(":")[0], c.id, c.entry, c.dt, "_".join(c.tags[:3]))
