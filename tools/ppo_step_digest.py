"""Bit-for-bit digest of the PPO minibatch-step entries (profiles/r25_ppo_step_routes.md): every entry x {contiguous tensors, table rows} x M in (5, 33, 256, 257)
x gradient-norm limit in (None, 0.5, inf) x {fp32, bf16x3} on the reference shape (67 -> 500 / 300, 2 actions) with seeded inputs.  A cell starts from the same
parameters, zero optimiser state and a gradient buffer of 4.25, runs three consecutive steps and prints one JSON line: the CRC-32C (mi_crc32c over the host copy) of
params, m, v, the gradient buffer, losses, kl_losses, grad_clip and value_head_grad[:M].  Two builds compute the same steps iff their outputs are the same text.

    python tools/ppo_step_digest.py [--time-limit 300] > digest.jsonl      # one process, no retries; the alarm ends a run that takes longer"""
import argparse
import ctypes
import json
import os
import signal
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "carla-ppo_amd"), ROOT):
    sys.path.insert(0, p)
from mi355 import lib as milib  # noqa: E402
from mi355.init import init_ppo  # noqa: E402
from mi355.ppo_device import PpoDevice  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--time-limit", type=int, default=300, help="seconds; the process is ended by SIGALRM behind it")
args = ap.parse_args()
signal.alarm(args.time_limit)

DIN, A, MAXB, STEPS = 67, 2, 320, 3
MS, LIMITS = (5, 33, 256, 257), (None, 0.5, float("inf"))
ALPHA, EPS_V, BETA, FILL = 1e-3, 0.2, 0.7, 4.25
L = milib.get()
dev = torch.device("cuda", 0)
low, high = np.array([-1.0, 0.0], np.float32), np.array([1.0, 1.0], np.float32)
hcomm, comm_log = ctypes.c_void_p(), np.zeros((64, 4), np.int64)
L.mi_comm_init_recording(ctypes.addressof(hcomm), 0, 1, comm_log.ctypes.data, 64)


def crc(t):
    b = t.detach().cpu().contiguous().numpy().tobytes()
    return int(L.mi_crc32c(0, b, len(b))) & 0xffffffff


for precision in ("fp32", "bf16x3"):
    rng = np.random.RandomState(25)
    d = PpoDevice(DIN, A, low, high, 0.2, 1.0, 0.01, max_batch=MAXB, precision=precision)
    th = init_ppo(1, DIN, A, 0.4)
    d.load_params(th, {k.replace("policy/", "policy_old/", 1): (v + 0.02 * rng.standard_normal(v.shape)).astype(np.float32) for k, v in th.items()})
    d.kl_losses.zero_()                                  # (workspace no step but train_step_kl writes)
    start = [x.clone() for x in (d.params, d.adam_m, d.adam_v)]
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)      # noqa: E731
    for M in MS:
        flat = {"s": up(0.5 * rng.standard_normal((M, DIN))), "a": up(rng.uniform(0, 1, (M, A))), "R": up(rng.standard_normal(M)), "adv": up(rng.standard_normal(M)),
                "vo": up(rng.standard_normal(M)), "lp": torch.empty(M, device=dev), "mo": torch.empty(M, A, device=dev)}
        d.old_policy_cache(flat["s"], flat["a"], M, flat["lp"], flat["mo"])
        n = 2 * M + 3
        rows = torch.from_numpy(rng.permutation(n)[:M].astype(np.int32)).to(dev)
        tab = {}
        for k, x in flat.items():
            tab[k] = up(0.5 * rng.standard_normal((n,) + tuple(x.shape[1:])))
            tab[k][rows.long()] = x
        a = (M, 1.0 / M, 1.0, ALPHA)
        adam = lambda: d.apply_adam(ALPHA)      # noqa: E731
        for form, t, r in (("contiguous", flat, None), ("rows", tab, rows)):
            data = (t["s"], t["a"], t["R"], t["adv"])
            vclip = lambda comm, **kw: d.train_step_vclip(comm, *data, t["lp"], t["vo"], EPS_V, r, *a, **kw)      # noqa: E731
            kl = lambda comm, **kw: d.train_step_kl(comm, *data, t["lp"], t["mo"], BETA, r, *a, old_values=t["vo"], clip_range_vf=EPS_V, **kw)      # noqa: E731
            entries = [("dp", lambda: d.train_step_dp(hcomm, *data, t["lp"], r, *a)), ("dp_no_cache", lambda: d.train_step_dp(hcomm, *data, None, r, *a)),
                       ("vclip", lambda: vclip(None)), ("vclip_comm", lambda: vclip(hcomm)), ("vclip_adam0", lambda: (vclip(None, adam=False), adam())),
                       ("vclip_comm_adam0", lambda: (vclip(hcomm, adam=False), adam())),
                       ("kl", lambda: kl(None)), ("kl_comm", lambda: kl(hcomm)), ("kl_adam0", lambda: (kl(None, adam=False), adam())),
                       ("kl_no_cache", lambda: d.train_step_kl(None, *data, None, None, BETA, r, *a))]
            entries += [("vclip_gradients", lambda: vclip(None, adam=False)), ("kl_gradients", lambda: kl(None, adam=False))]      # the buffer before Adam zeroes it
            if r is None:
                fb = lambda: d.forward_backward(*data, M, 1.0 / M, 1.0)      # noqa: E731
                entries += [("forward_backward_gradients", fb), ("forward_backward", lambda: (fb(), adam())),
                            ("train_step", lambda: d.train_step(*data, *a, logp_old=t["lp"])), ("train_step_no_cache", lambda: d.train_step(*data, *a))]
            else:
                entries += [("train_step_idx", lambda: d.train_step_idx(*data, t["lp"], r, *a)), ("train_step_idx_no_cache", lambda: d.train_step_idx(*data, None, r, *a))]
            for limit in LIMITS:
                d.set_max_grad_norm(limit)
                for name, step in entries:
                    for x, y in zip((d.params, d.adam_m, d.adam_v), start):
                        x.copy_(y)
                    d.grads.fill_(FILL)
                    for _ in range(STEPS):
                        step()
                    out = {"cell": "%s %s M=%d limit=%s %s" % (precision, form, M, limit, name)}
                    for key, x in (("params", d.params), ("m", d.adam_m), ("v", d.adam_v), ("grads", d.grads), ("losses", d.losses), ("kl_losses", d.kl_losses),
                                   ("grad_clip", d.grad_clip), ("value_head_grad", d.value_head_grad[:M])):
                        out[key] = "%08x" % crc(x)
                    print(json.dumps(out), flush=True)
    d.close()
L.mi_comm_destroy(hcomm)
