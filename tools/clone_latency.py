"""What a behaviour-cloning step costs (profiles/r34_behaviour_cloning.md): interleaved windows of mi_ppo_clone_step with returns and policy-only against the plain
one-call PPO step (mi_ppo_train_step with a cached log pi_old) at M = 32 and M = 2048 (fp32, 67 inputs, 2 actions) -- one process, device events, a warm-up, nine
rounds per variant; median / min / max of the rounds in us per call.  Two windows of the plain step per round give its own run-to-run spread.  With
--parent-lib PATH the plain step also runs from ANOTHER build of the library (the parent commit's libmi355_carla.so) in the same process and the same rounds, on an
engine of its own with the same parameters: the plain step's entry points have the same prototypes in both.

    python tools/clone_latency.py [--parent-lib PATH] [OUT_DIR]      # default out/: writes clone_latency.json there and prints the table

Expectations (recorded, not enforced): the step with returns is the same chain with fewer gathers and should not exceed the plain step by more than the larger of
2 % and the plain step's own spread; policy-only should be below the plain step."""
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
from mi355.ppo_device import PpoDevice  # noqa: E402

argv = sys.argv[1:]
PARENT = None
if "--parent-lib" in argv:
    i = argv.index("--parent-lib")
    PARENT = argv[i + 1]
    del argv[i:i + 2]
OUT = argv[0] if argv else os.path.join(ROOT, "out")

dev = torch.device("cuda", 0)
rng = np.random.RandomState(0)
A, DIN, MAXB = 2, 67, 2048
low, high = np.array([-1.0, 0.0], np.float32), np.array([1.0, 1.0], np.float32)
d = PpoDevice(DIN, A, low, high, 0.2, 1.0, 0.01, max_batch=MAXB)
th = init_ppo(1, DIN, A, 0.4)
d.load_params(th, {k.replace("policy/", "policy_old/", 1): (v + 0.01 * rng.standard_normal(v.shape)).astype(np.float32) for k, v in th.items()})
up = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)      # noqa: E731


class OtherBuild:
    """The plain step of another build of the library: an engine of its own (buffers, workspace) holding d's parameters."""

    NAMES = ("mi_ppo_workspace_bytes", "mi_ppo_create", "mi_ppo_destroy", "mi_ppo_train_step")

    def __init__(self, path):
        self.cdll = ctypes.CDLL(path)
        protos = milib.parse_header()
        for name in self.NAMES:                              # (prototypes of this tree's header: these four are the same in both builds)
            fn = getattr(self.cdll, name)
            fn.restype, fn.argtypes = milib._CTYPES[protos[name][0]], [milib._CTYPES[t] for t, _ in protos[name][1]]
        desc = d._desc(MAXB)
        nbytes = int(self.cdll.mi_ppo_workspace_bytes(ctypes.byref(desc)))
        self.bufs = [x.clone() for x in (d.params, d.params_old, d.grads, d.adam_m, d.adam_v)]
        self.ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
        p = milib.ptr
        self.handle = self.cdll.mi_ppo_create(ctypes.byref(desc), *[p(x) for x in self.bufs], p(self.ws), nbytes, low.ctypes.data, high.ctypes.data)
        if not self.handle:
            raise RuntimeError("mi_ppo_create failed in " + path)

    def train_step(self, s, a, R, adv, lp, M, inv_m, gs, alpha):
        p = milib.ptr
        rc = self.cdll.mi_ppo_train_step(self.handle, d.stream(), p(s), p(a), p(R), p(adv), p(lp), M, inv_m, gs, alpha, 0.9, 0.999, 1e-8)
        if rc != 0:
            raise RuntimeError("mi_ppo_train_step failed in the other build (%d)" % rc)


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


other = OtherBuild(PARENT) if PARENT else None
out = {"parent_lib": bool(PARENT)}
state = [x.clone() for x in (d.params, d.adam_m, d.adam_v)]
for M, iters in ((32, 2000), (2048, 300)):
    s, a = up(0.5 * rng.standard_normal((M, DIN))), up(rng.uniform(0, 1, (M, A)))
    R, adv = up(rng.standard_normal(M)), up(rng.standard_normal(M))
    lp = torch.empty(M, device=dev)
    d.logp_old(s, a, M, lp)
    args = (M, 1.0 / M, 1.0, 1e-6)
    variants = {
        "plain_a": lambda: d.train_step(s, a, R, adv, *args, logp_old=lp),
        "clone_returns_nll": lambda: d.clone_step(None, s, a, R, "nll", None, *args),
        "clone_policy_only_nll": lambda: d.clone_step(None, s, a, None, "nll", None, *args),
        "plain_b": lambda: d.train_step(s, a, R, adv, *args, logp_old=lp),
        "clone_returns_mse": lambda: d.clone_step(None, s, a, R, "mse", None, *args),
        "clone_policy_only_mse": lambda: d.clone_step(None, s, a, None, "mse", None, *args),
    }
    if other is not None:
        variants["plain_parent"] = lambda: other.train_step(s, a, R, adv, lp, *args)
    res = ab(variants, iters)
    base = res["plain_parent" if other is not None else "plain_a"]["median"]
    spread = abs(res["plain_a"]["median"] - res["plain_b"]["median"]) / base
    spread = max(spread, max((res[k]["max"] - res[k]["min"]) / res[k]["median"] for k in ("plain_a", "plain_b")))
    allow = max(0.02, spread)
    res["summary"] = {"baseline": "plain_parent" if other is not None else "plain_a", "baseline_us": base, "plain_spread": spread, "allowance": allow,
                      "with_returns_over_plain": {k: res["clone_returns_" + k]["median"] / base - 1.0 for k in ("nll", "mse")},
                      "policy_only_over_plain": {k: res["clone_policy_only_" + k]["median"] / base - 1.0 for k in ("nll", "mse")}}
    res["summary"]["with_returns_within_allowance"] = all(v <= allow for v in res["summary"]["with_returns_over_plain"].values())
    res["summary"]["policy_only_below_plain"] = all(v < 0 for v in res["summary"]["policy_only_over_plain"].values())
    out["step_M%d" % M] = res
    for x, y in zip((d.params, d.adam_m, d.adam_v), state):
        x.copy_(y)

os.makedirs(OUT, exist_ok=True)
json.dump(out, open(os.path.join(OUT, "clone_latency.json"), "w"), indent=1)
for k, v in out.items():
    if not isinstance(v, dict):
        continue
    print(k)
    for kk, vv in v.items():
        print("   %-24s %s" % (kk, "median %9.2f us  min %9.2f  max %9.2f" % (vv["median"], vv["min"], vv["max"]) if "median" in vv else json.dumps(vv)))
if other is not None:
    other.cdll.mi_ppo_destroy(other.handle)
d.close()
