"""What the adaptive KL penalty costs (profiles/r24_kl_penalty.md): interleaved windows of the plain and the penalised one-call PPO step at M = 32 and 2048 (fp32),
mi_ppo_old_policy_cache against mi_ppo_logp_old at 4096 rows, and the kl_stats pass over 1024 x 128 rows against the diagnostics pass -- one process, device events,
a warm-up, nine rounds per variant; median / min / max of the rounds in us per call.  Two windows of the plain step per round give its own spread.

    python tools/ppo_kl_penalty_bench.py [OUT_DIR]      # default out/: writes kl_cost.json there and prints the table"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "carla-ppo_amd"), ROOT):
    sys.path.insert(0, p)
from mi355.ppo_device import PpoDevice, N_KL_STATS, N_STATS  # noqa: E402

dev = torch.device("cuda", 0)
rng = np.random.RandomState(0)
A, DIN = 2, 67
low, high = np.array([-1.0, 0.0], np.float32), np.array([1.0, 1.0], np.float32)
d = PpoDevice(DIN, A, low, high, 0.2, 1.0, 0.01, max_batch=4096)
from mi355.init import init_ppo  # noqa: E402
th = init_ppo(1, DIN, A, 0.4)
old = {k.replace("policy/", "policy_old/", 1): (v + 0.01 * rng.standard_normal(v.shape)).astype(np.float32) for k, v in th.items()}
d.load_params(th, old)
up = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)      # noqa: E731


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


out = {}
state = [x.clone() for x in (d.params, d.adam_m, d.adam_v)]
for M, iters in ((32, 2000), (2048, 300)):
    s, a = up(0.5 * rng.standard_normal((M, DIN))), up(rng.uniform(0, 1, (M, A)))
    R, adv = up(rng.standard_normal(M)), up(rng.standard_normal(M))
    lp, mo = torch.empty(M, device=dev), torch.empty(M, A, device=dev)
    d.old_policy_cache(s, a, M, lp, mo)
    args = (M, 1.0 / M, 1.0, 1e-6)
    variants = {
        "plain_a": lambda: d.train_step(s, a, R, adv, *args, logp_old=lp),
        "kl": lambda: d.train_step_kl(None, s, a, R, adv, lp, mo, 0.7, None, *args),
        "plain_b": lambda: d.train_step(s, a, R, adv, *args, logp_old=lp),
        "kl_no_cache": lambda: d.train_step_kl(None, s, a, R, adv, None, None, 0.7, None, *args),
        "plain_no_cache": lambda: d.train_step(s, a, R, adv, *args),
    }
    out["step_M%d" % M] = ab(variants, iters)
    for x, y in zip((d.params, d.adam_m, d.adam_v), state):
        x.copy_(y)

M = 4096
s, a = up(0.5 * rng.standard_normal((M, DIN))), up(rng.uniform(0, 1, (M, A)))
lp, mo = torch.empty(M, device=dev), torch.empty(M, A, device=dev)
out["cache_M4096"] = ab({"logp_old_a": lambda: d.logp_old(s, a, M, lp), "old_policy_cache": lambda: d.old_policy_cache(s, a, M, lp, mo),
                         "logp_old_b": lambda: d.logp_old(s, a, M, lp)}, 300)

E, T = 1024, 128
n = E * T
S, Act, Ret = up(0.5 * rng.standard_normal((n, DIN))), up(rng.uniform(0, 1, (n, A))), up(rng.standard_normal(n))
LP, MO = torch.empty(n, device=dev), torch.empty(n, A, device=dev)
for lo in range(0, n, 4096):
    d.old_policy_cache(S[lo:lo + 4096], Act[lo:lo + 4096], 4096, LP[lo:lo + 4096], MO[lo:lo + 4096])
rows = torch.arange(n, dtype=torch.int32, device=dev)
ks, kscr = torch.zeros(N_KL_STATS, dtype=torch.float64, device=dev), torch.zeros(d.kl_stats_scratch_doubles(4096), dtype=torch.float64, device=dev)
us, uscr = torch.zeros(N_STATS, dtype=torch.float64, device=dev), torch.zeros(d.stats_scratch_doubles(4096), dtype=torch.float64, device=dev)


def kl_pass():
    for lo in range(0, n, 4096):
        d.kl_stats(S, MO, rows[lo:lo + 4096], 4096, ks, kscr, accumulate=lo > 0)


def diag_pass():
    for lo in range(0, n, 4096):
        d.update_stats(S, Act, Ret, LP, rows[lo:lo + 4096], 4096, us, uscr, accumulate=lo > 0)


out["stats_1024x128"] = ab({"kl_stats_a": kl_pass, "update_stats": diag_pass, "kl_stats_b": kl_pass}, 10, rounds=7, warm=3)
out["stats_1024x128"]["kl_sums"] = ks.cpu().numpy().tolist()
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "out")
os.makedirs(OUT, exist_ok=True)
json.dump(out, open(os.path.join(OUT, "kl_cost.json"), "w"), indent=1)
for k, v in out.items():
    print(k)
    for kk, vv in v.items():
        print("   %-18s %s" % (kk, vv if not isinstance(vv, dict) else "median %9.2f us  min %9.2f  max %9.2f" % (vv["median"], vv["min"], vv["max"])))
d.close()
