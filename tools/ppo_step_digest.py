"""Bit-for-bit digest of the PPO entries that run the kernels of csrc/ppo_fused.hip (profiles/r25_ppo_step_routes.md, profiles/r35_ppo_head_helpers.md), with seeded
inputs, on two shapes: the reference's (67 -> 500 / 300, 2 actions: the NA = 2 instantiations) and the small one of the cloning tests (5 -> 36 / 20, 3 actions: the
NA = 8 instantiations).  Two builds compute the same thing iff their outputs are the same text.

Step cells: every minibatch-step entry x {contiguous tensors, table rows} x M in (5, 33, 256, 257) x gradient-norm limit in (None, 0.5, inf) x {fp32, bf16x3}; at
M = 5 and 33 also clone_step over {nll, mse} x {with returns, policy only} x {adam 1, adam 0}.  A cell starts from the same parameters, zero optimiser state and a
gradient buffer of 4.25, runs three consecutive steps and prints one JSON line: the CRC-32C (mi_crc32c over the host copy) of params, m, v, the gradient buffer,
losses, kl_losses, grad_clip and value_head_grad[:M].  At M = 5, 33 and 257 also the step with a demonstration term (train_step_demo) with M_DEMO = 7 demonstration
rows drawn from a stream of their own (the inputs of every other cell are those they were): plain "nll", KL + value clip "mse", on the recording communicator, and
adam 0; those cells also print demo_losses and value_head_grad[:M + M_DEMO].

Head cells, at M = 5 (the wave-per-sample predict kernel) and 33, per precision: old_policy_cache (both outputs), logp_old, update_stats (the sums and the two
optional tables), kl_stats, predict sampled with given noise and greedy, logp_idx (the policy net alone: contiguous, and through the row list into a table); one
JSON line each with the CRC-32C of every output.  (The two logp_idx cells come last and draw nothing from the input streams: every other cell is the line it was.)

    python tools/ppo_step_digest.py [--time-limit 600] > digest.jsonl      # one process, no retries; the alarm ends a run that takes longer
    MI355_LIB=<another build's library> python tools/ppo_step_digest.py    # the same cells from that build (the C ABI has to be this tree's)"""
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
from mi355.ppo_device import N_KL_STATS, N_STATS, PpoDevice  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--time-limit", type=int, default=600, help="seconds; the process is ended by SIGALRM behind it")
args = ap.parse_args()
signal.alarm(args.time_limit)

MAXB, STEPS = 320, 3
SHAPES = (("A2", 67, 2, (500, 300)), ("A3", 5, 3, (36, 20)))
MS, HEAD_MS, LIMITS = (5, 33, 256, 257), (5, 33), (None, 0.5, float("inf"))
DEMO_MS, M_DEMO = (5, 33, 257), 7
ALPHA, EPS_V, BETA, FILL = 1e-3, 0.2, 0.7, 4.25
L = milib.get()
dev = torch.device("cuda", 0)
hcomm, comm_log = ctypes.c_void_p(), np.zeros((64, 4), np.int64)
L.mi_comm_init_recording(ctypes.addressof(hcomm), 0, 1, comm_log.ctypes.data, 64)


def crc(t):
    b = t.detach().cpu().contiguous().numpy().tobytes()
    return int(L.mi_crc32c(0, b, len(b))) & 0xffffffff


def emit(cell, named):
    out = {"cell": cell}
    for key, x in named:
        out[key] = "%08x" % crc(x)
    print(json.dumps(out), flush=True)


def head_cells(d, tag, M, A, flat, tab, rows):
    """The forward-only entries under the start parameters: every output starts from a fill, so that an entry left unwritten shows."""
    f32 = lambda *shape: torch.full(shape, FILL, device=dev)      # noqa: E731
    f64 = lambda n: torch.full((n,), FILL, device=dev, dtype=torch.float64)      # noqa: E731
    n = tab["s"].shape[0]
    lp, mo = f32(M), f32(M, A)
    d.old_policy_cache(flat["s"], flat["a"], M, lp, mo)
    emit("%s M=%d old_policy_cache" % (tag, M), (("logp", lp), ("mean", mo)))
    lp2 = f32(M)
    d.logp_old(flat["s"], flat["a"], M, lp2)
    emit("%s M=%d logp_old" % (tag, M), (("logp", lp2),))
    for acc in (False, True):
        stats, scratch, lpn, val = f64(N_STATS), f64(d.stats_scratch_doubles(M)), f32(n), f32(n)
        d.update_stats(tab["s"], tab["a"], tab["R"], tab["lp"], rows, M, stats, scratch, accumulate=acc, logp_new_out=lpn, value_out=val)
        emit("%s M=%d update_stats accumulate=%d" % (tag, M, acc), (("stats", stats), ("logp_new", lpn), ("value", val)))
        stats, scratch = f64(N_KL_STATS), f64(d.kl_stats_scratch_doubles(M))
        d.kl_stats(tab["s"], tab["mo"], rows, M, stats, scratch, accumulate=acc)
        emit("%s M=%d kl_stats accumulate=%d" % (tag, M, acc), (("stats", stats),))
    for greedy in (0, 1):
        act, val = f32(M, A), f32(M)
        d.predict(flat["s"], M, flat["noise"], greedy, act, val)
        emit("%s M=%d predict greedy=%d" % (tag, M, greedy), (("action", act), ("value", val)))
    lpc, lpt = f32(M), f32(n)
    d.logp_idx(flat["s"], flat["a"], None, M, lpc)
    emit("%s M=%d logp_idx contiguous" % (tag, M), (("logp", lpc),))
    d.logp_idx(tab["s"], tab["a"], rows, M, lpt)
    emit("%s M=%d logp_idx rows" % (tag, M), (("logp", lpt),))


for shape, DIN, A, HIDDEN in SHAPES:
    low = np.array([-1.0, 0.0, -0.5][:A], np.float32)
    high = np.array([1.0, 1.0, 0.75][:A], np.float32)
    for precision in ("fp32", "bf16x3"):
        rng = np.random.RandomState(25)
        drng = np.random.RandomState(36)                     # the demonstration rows: a stream of their own
        d = PpoDevice(DIN, A, low, high, 0.2, 1.0, 0.01, hidden=HIDDEN, max_batch=MAXB, precision=precision)
        th = init_ppo(1, DIN, A, 0.4, hidden=HIDDEN)
        d.load_params(th, {k.replace("policy/", "policy_old/", 1): (v + 0.02 * rng.standard_normal(v.shape)).astype(np.float32) for k, v in th.items()})
        d.kl_losses.zero_()                                  # (workspace no step but train_step_kl writes)
        start = [x.clone() for x in (d.params, d.adam_m, d.adam_v)]
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)      # noqa: E731
        tag = "%s %s" % (shape, precision)
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
            if M in HEAD_MS:
                flat["noise"] = up(rng.standard_normal((M, A)))
                d.params.copy_(start[0])
                head_cells(d, tag, M, A, flat, tab, rows)
            dflat = {"ds": up(0.5 * drng.standard_normal((M_DEMO, DIN))), "da": up(drng.uniform(0, 1, (M_DEMO, A)))}
            drows = torch.from_numpy(drng.permutation(2 * M_DEMO + 3)[:M_DEMO].astype(np.int32)).to(dev)
            dtab = {}
            for k, x in dflat.items():
                dtab[k] = up(0.5 * drng.standard_normal((2 * M_DEMO + 3,) + tuple(x.shape[1:])))
                dtab[k][drows.long()] = x
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
                if M in HEAD_MS:
                    for kind in ("nll", "mse"):
                        for what, R in (("returns", t["R"]), ("policy_only", None)):
                            for on in (True, False):
                                entries.append(("clone_%s_%s_adam%d" % (kind, what, on),
                                                lambda kind=kind, R=R, on=on: d.clone_step(None, t["s"], t["a"], R, kind, r, *a, adam=on)))
                demo_entries = []
                if M in DEMO_MS:
                    dt, dr = (dflat, None) if r is None else (dtab, drows)
                    demo = lambda comm, kind, klc, vo, **kw: d.train_step_demo(comm, *data, t["lp"], t["mo"] if klc is not None else None, klc, r, M, dt["ds"], dt["da"], dr,      # noqa: E731
                                                                               M_DEMO, kind, 0.5, 1.0 / M_DEMO, 1.0 / M, 1.0, ALPHA, old_values=vo, clip_range_vf=EPS_V, **kw)
                    demo_entries = [("demo_nll", lambda: demo(None, "nll", None, None)), ("demo_kl_vclip_mse", lambda: demo(None, "mse", BETA, t["vo"])),
                                    ("demo_comm", lambda: demo(hcomm, "nll", None, None)), ("demo_gradients", lambda: demo(None, "nll", BETA, t["vo"], adam=False))]

                def run(cells, named):
                    for limit in LIMITS:
                        d.set_max_grad_norm(limit)
                        for name, step in cells:
                            for x, y in zip((d.params, d.adam_m, d.adam_v), start):
                                x.copy_(y)
                            d.grads.fill_(FILL)
                            for _ in range(STEPS):
                                step()
                            emit("%s %s M=%d limit=%s %s" % (tag, form, M, limit, name), named())
                common = lambda: (("params", d.params), ("m", d.adam_m), ("v", d.adam_v), ("grads", d.grads), ("losses", d.losses), ("kl_losses", d.kl_losses),      # noqa: E731
                                  ("grad_clip", d.grad_clip))
                run(entries, lambda: common() + (("value_head_grad", d.value_head_grad[:M]),))
                # the demonstration cells behind the others, and the workspace a later cell may show unwritten (the last norm, the KL floats, dv) put back behind them: the
                # text of every other cell is what it is without them
                carried = [x.clone() for x in (d.grad_clip, d.kl_losses, d.losses, d.value_head_grad)]
                run(demo_entries, lambda: common() + (("demo_losses", d.demo_losses), ("value_head_grad", d.value_head_grad[:M + M_DEMO])))
                for x, y in zip((d.grad_clip, d.kl_losses, d.losses, d.value_head_grad), carried):
                    x.copy_(y)
                d.set_max_grad_norm(None)
        d.close()
L.mi_comm_destroy(hcomm)
