"""What the calls through the head-level kernels of csrc/ppo_fused.hip cost (profiles/r34_behaviour_cloning.md, profiles/r35_ppo_head_helpers.md): interleaved windows
of the plain one-call PPO step (mi_ppo_train_step with a cached log pi_old, two windows: its own run-to-run spread), mi_ppo_clone_step with returns and policy-only
in both kinds, and mi_ppo_train_step_kl with value clipping, at M = 32 and M = 2048 (fp32, 67 inputs, 2 actions); at M = 2048 also one window each of
mi_ppo_update_stats_idx, mi_ppo_kl_stats_idx and mi_ppo_logp_old.  In the same rounds: the step with a demonstration term (mi_ppo_train_step_demo, this build
only: the parent has no such entry) at (M_p, M_d) = (32, 32) and (2048, 256), and the plain step followed by the policy-only clone step on the same M_d rows -- the
two calls, two chains and two optimiser steps the one-chain step replaces (profiles/r36_demonstration_term.md).  One process, device events, a warm-up of 100 calls, nine rounds per variant; median / min / max
of the rounds in us per call.  With --parent-lib PATH every variant also runs from ANOTHER build of the library (the parent commit's libmi355_carla.so) in the same
process and the same rounds, on an engine of its own with the same parameters, and each variant of this build is compared with the SAME variant of that one: the
entry points have the same prototypes in both.

    python tools/clone_latency.py [--parent-lib PATH] [OUT_DIR]      # default out/: writes clone_latency.json there and prints the table

Expectations (recorded, not enforced): no variant exceeds its twin from the other build by more than the allowance, the larger of 2 % and the plain step's own
spread; the clone step with returns stays within the allowance of the plain step, and policy-only below it; the demonstration step is faster than the two calls by
more than the allowance (summary: one_chain_pays).

Dual clip (profiles/r42_dual_clip.md): this build's plain step also runs on a second engine of this build with mi_ppo_set_dual_clip(3) on -- the column
`plain_dual_clip`, the same rows, so no sample is dual-clipped and the kernel's extra compare and multiply are all that differs -- and with a parent library
the parent's plain step gets its second window too: summary.plain_vs_parent holds this build's plain step (setting off) minus the parent's, the parent's own
difference between its two windows, and whether the first stays within twice the second."""
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "carla-ppo_amd"), ROOT):
    sys.path.insert(0, p)
from mi355 import lib as milib  # noqa: E402
from mi355.init import init_ppo  # noqa: E402
from mi355.ppo_device import N_KL_STATS, N_STATS, PpoDevice  # noqa: E402

argv = sys.argv[1:]
PARENT = None
if "--parent-lib" in argv:
    i = argv.index("--parent-lib")
    PARENT = argv[i + 1]
    del argv[i:i + 2]
OUT = argv[0] if argv else os.path.join(ROOT, "out")

dev = torch.device("cuda", 0)
rng = np.random.RandomState(0)
A, DIN, MAXB = 2, 67, 2048 + 256                        # (the largest demonstration step: 2048 + 256 rows)
M_DEMO = {32: 32, 2048: 256}
low, high = np.array([-1.0, 0.0], np.float32), np.array([1.0, 1.0], np.float32)
d = PpoDevice(DIN, A, low, high, 0.2, 1.0, 0.01, max_batch=MAXB)
th = init_ppo(1, DIN, A, 0.4)
d.load_params(th, {k.replace("policy/", "policy_old/", 1): (v + 0.01 * rng.standard_normal(v.shape)).astype(np.float32) for k, v in th.items()})
up = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)      # noqa: E731
p = milib.ptr
ADAM = (1e-6, 0.9, 0.999, 1e-8)


class Build:
    """The measured entries of one build of the library on one engine, called through the raw C prototypes (the same Python work per call for both builds)."""

    NAMES = ("mi_ppo_workspace_bytes", "mi_ppo_create", "mi_ppo_destroy", "mi_ppo_train_step", "mi_ppo_clone_step", "mi_ppo_train_step_kl",
             "mi_ppo_update_stats_idx", "mi_ppo_kl_stats_idx", "mi_ppo_logp_old")

    def __init__(self, path=None, dual_clip=None):
        """path None: this tree's library on d's engine; else another build, on an engine of its own (buffers, workspace) holding d's parameters.  dual_clip: this
        tree's library on an engine of its own with mi_ppo_set_dual_clip(dual_clip) on."""
        self.path = path
        self.own = path is not None or dual_clip is not None
        if not self.own:
            self.cdll, self.handle, self.bufs = d.L.cdll, d.handle, [d.params, d.params_old, d.grads, d.adam_m, d.adam_v]
        else:
            self.cdll = ctypes.CDLL(path) if path is not None else d.L.cdll
            protos = milib.parse_header()
            for name in self.NAMES if path is not None else ():      # (prototypes of this tree's header: the same in both builds)
                fn = getattr(self.cdll, name)
                fn.restype, fn.argtypes = milib._CTYPES[protos[name][0]], [milib._CTYPES[t] for t, _ in protos[name][1]]
            desc = d._desc(MAXB)
            nbytes = int(self.cdll.mi_ppo_workspace_bytes(ctypes.byref(desc)))
            self.bufs = [x.clone() for x in (d.params, d.params_old, d.grads, d.adam_m, d.adam_v)]
            self.ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
            self.handle = self.cdll.mi_ppo_create(ctypes.byref(desc), *[p(x) for x in self.bufs], p(self.ws), nbytes, low.ctypes.data, high.ctypes.data)
            if not self.handle:
                raise RuntimeError("mi_ppo_create failed in " + (path or "this build"))
            if dual_clip is not None and self.cdll.mi_ppo_set_dual_clip(self.handle, ctypes.c_float(dual_clip)) != 0:
                raise RuntimeError("mi_ppo_set_dual_clip failed")
        self.state = [x.clone() for x in self.bufs]

    def restore(self):
        for x, y in zip(self.bufs, self.state):
            x.copy_(y)

    def call(self, name, *args):
        rc = getattr(self.cdll, name)(self.handle, *args)
        if rc != 0:
            raise RuntimeError("%s failed (%d) in %s" % (name, rc, self.path or "this build"))

    def close(self):
        if self.own:
            self.cdll.mi_ppo_destroy(self.handle)

    def plain(self, t, M):
        st = d.stream()
        return lambda: self.call("mi_ppo_train_step", st, p(t["s"]), p(t["a"]), p(t["R"]), p(t["adv"]), p(t["lp"]), M, 1.0 / M, 1.0, *ADAM)

    def variants(self, t, M, with_stats):
        """name -> call, on the tensors t."""
        st, a = d.stream(), (M, 1.0 / M, 1.0)
        kinds = {k: milib.clone_kind(k, "clone_latency") for k in ("nll", "mse")}
        plain = lambda: self.call("mi_ppo_train_step", st, p(t["s"]), p(t["a"]), p(t["R"]), p(t["adv"]), p(t["lp"]), *a, *ADAM)      # noqa: E731
        clone = lambda R, kind: lambda: self.call("mi_ppo_clone_step", None, st, p(t["s"]), p(t["a"]), p(R), kinds[kind], None, M, *a, 1, *ADAM)      # noqa: E731
        v = {"plain_a": plain,
             "clone_returns_nll": clone(t["R"], "nll"), "clone_policy_only_nll": clone(None, "nll"),
             "kl_vclip": lambda: self.call("mi_ppo_train_step_kl", None, st, p(t["s"]), p(t["a"]), p(t["R"]), p(t["adv"]), p(t["lp"]), p(t["mo"]), 0.7, p(t["vo"]), 0.2,
                                           None, M, *a, 1, *ADAM),
             "plain_b": plain,
             "clone_returns_mse": clone(t["R"], "mse"), "clone_policy_only_mse": clone(None, "mse")}
        Md = M_DEMO[M]
        clone_demo = lambda: self.call("mi_ppo_clone_step", None, st, p(t["ds"]), p(t["da"]), None, kinds["nll"], None, Md, Md, 1.0 / Md, 1.0, 1, *ADAM)      # noqa: E731
        v["plain_then_clone"] = lambda: (plain(), clone_demo())
        if self.path is None:                                # (the new entry: this build only)
            v["demo"] = lambda: self.call("mi_ppo_train_step_demo", None, st, p(t["s"]), p(t["a"]), p(t["R"]), p(t["adv"]), p(t["lp"]), None, 0, 0.0, None, 0.0, None, M, M,
                                          p(t["ds"]), p(t["da"]), None, Md, Md, 0, 0.5, 1.0 / Md, 1.0 / M, 1.0, 1, *ADAM)
        if with_stats:
            v["update_stats"] = lambda: self.call("mi_ppo_update_stats_idx", st, p(t["s"]), p(t["a"]), p(t["R"]), p(t["lp"]), p(t["rows"]), M, M, 0, p(t["scratch"]),
                                                  p(t["stats"]), None, None)
            v["kl_stats"] = lambda: self.call("mi_ppo_kl_stats_idx", st, p(t["s"]), p(t["mo"]), p(t["rows"]), M, M, 0, p(t["kl_scratch"]), p(t["kl_stats"]))
            v["logp_old"] = lambda: self.call("mi_ppo_logp_old", st, p(t["s"]), p(t["a"]), M, p(t["lp_out"]))
        return v


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters          # us per call


def ab(variants, iters, rounds=9, warm=100):
    for fn in variants.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            t[k].append(window(fn, iters))
    return {k: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v))) for k, v in t.items()}


this = Build()
dual = Build(dual_clip=3.0)
other = Build(PARENT) if PARENT else None
out = {"parent_lib": bool(PARENT)}
for M, iters in ((32, 2000), (2048, 300)):
    t = {"s": up(0.5 * rng.standard_normal((M, DIN))), "a": up(rng.uniform(0, 1, (M, A))), "R": up(rng.standard_normal(M)), "adv": up(rng.standard_normal(M)),
         "vo": up(rng.standard_normal(M)), "lp": torch.empty(M, device=dev), "mo": torch.empty(M, A, device=dev), "lp_out": torch.empty(M, device=dev),
         "rows": torch.arange(M, device=dev, dtype=torch.int32), "stats": torch.zeros(N_STATS, device=dev, dtype=torch.float64),
         "scratch": torch.zeros(d.stats_scratch_doubles(M), device=dev, dtype=torch.float64), "kl_stats": torch.zeros(N_KL_STATS, device=dev, dtype=torch.float64),
         "kl_scratch": torch.zeros(d.kl_stats_scratch_doubles(M), device=dev, dtype=torch.float64),
         "ds": up(0.5 * rng.standard_normal((M_DEMO[M], DIN))), "da": up(rng.uniform(0, 1, (M_DEMO[M], A)))}
    d.old_policy_cache(t["s"], t["a"], M, t["lp"], t["mo"])
    variants = dict(this.variants(t, M, M == 2048))
    variants["plain_dual_clip"] = dual.plain(t, M)
    if other is not None:                                    # the twins, interleaved with this build's windows
        variants.update({k + "_parent": fn for k, fn in other.variants(t, M, M == 2048).items()})
    res = ab(variants, iters)
    base = res["plain_a_parent" if other is not None else "plain_a"]["median"]
    spread = abs(res["plain_a"]["median"] - res["plain_b"]["median"]) / base
    spread = max(spread, max((res[k]["max"] - res[k]["min"]) / res[k]["median"] for k in ("plain_a", "plain_b")))
    allow = max(0.02, spread)
    res["summary"] = {"baseline": "plain_a_parent" if other is not None else "plain_a", "baseline_us": base, "plain_spread": spread, "allowance": allow,
                      "with_returns_over_plain": {k: res["clone_returns_" + k]["median"] / base - 1.0 for k in ("nll", "mse")},
                      "policy_only_over_plain": {k: res["clone_policy_only_" + k]["median"] / base - 1.0 for k in ("nll", "mse")}}
    res["summary"]["with_returns_within_allowance"] = all(v <= allow for v in res["summary"]["with_returns_over_plain"].values())
    res["summary"]["policy_only_below_plain"] = all(v < 0 for v in res["summary"]["policy_only_over_plain"].values())
    two = res["plain_then_clone"]["median"]
    res["summary"]["demo_rows"] = M_DEMO[M]
    res["summary"]["demo_over_plain"] = res["demo"]["median"] / res["plain_a"]["median"] - 1.0
    res["summary"]["demo_over_two_calls"] = res["demo"]["median"] / two - 1.0
    res["summary"]["one_chain_pays"] = bool(res["demo"]["median"] < two * (1.0 - allow))
    if other is not None:
        over = {k: res[k]["median"] / res[k + "_parent"]["median"] - 1.0 for k in variants if not k.endswith("_parent") and k not in ("demo", "plain_dual_clip")}
        res["summary"]["over_parent_twin"] = over
        res["summary"]["all_within_allowance_of_parent"] = all(v <= allow for v in over.values())
        # the timing condition of profiles/r42_dual_clip.md: both windows of each build together (the mean of the two medians), in us
        mine, theirs = (0.5 * (res["plain_a" + x]["median"] + res["plain_b" + x]["median"]) for x in ("", "_parent"))
        parent_diff = abs(res["plain_a_parent"]["median"] - res["plain_b_parent"]["median"])
        res["summary"]["plain_vs_parent"] = {"this_minus_parent_us": mine - theirs, "parent_two_runs_differ_us": parent_diff,
                                             "within_twice_the_parents_difference": bool(mine - theirs <= 2.0 * parent_diff)}
    res["summary"]["dual_clip_over_plain"] = res["plain_dual_clip"]["median"] / (0.5 * (res["plain_a"]["median"] + res["plain_b"]["median"])) - 1.0
    out["step_M%d" % M] = res
    this.restore()
    dual.restore()
    if other is not None:
        other.restore()

os.makedirs(OUT, exist_ok=True)
json.dump(out, open(os.path.join(OUT, "clone_latency.json"), "w"), indent=1)
for k, v in out.items():
    if not isinstance(v, dict):
        continue
    print(k)
    for kk, vv in v.items():
        print("   %-28s %s" % (kk, "median %9.2f us  min %9.2f  max %9.2f" % (vv["median"], vv["min"], vv["max"]) if "median" in vv else json.dumps(vv)))
if other is not None:
    other.close()
dual.close()
d.close()
