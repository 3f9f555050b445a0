"""Each minibatch-step entry takes the route its form calls for (csrc/ppo_engine.hip): the in-tile Adam iff the optimiser is wanted, there is no communicator,
M <= 256 and clipping by the global norm is off; else the fused chain into the flat gradient buffer, the all-reduce where a communicator is given, mi_ppo_apply_adam.

One fused-range engine (max_batch 320) per shape of tests/kl_penalty_cases.py -- the reference's 67 -> 500 / 300 with 2 actions and 5 -> 36 / 20 with 3 -- in fp32 and
bf16x3; M in (33, 257) and the limit in (None, inf): the smallest settings on each side of both conditions (33: two loss blocks; 257: two row chunks and the ordered
slab sum; inf takes the flat route and scales nothing).  Everything is compared bitwise; nothing here needs a reference.
  flat route     the one-call entry == the same entry with adam = False (the plain forms without log pi_old: forward_backward) followed by apply_adam, and the
                 gradient buffer was written;
  in-tile route  the gradient buffer still holds the 4.25 it was filled with: the in-tile update writes none."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import kl_penalty_cases as kc  # noqa: E402
import ppo_shape_cases as pc  # noqa: E402
from rollout_gpu_common import bitwise  # noqa: E402

ALPHA, EPS_V, BETA, FILL = 1e-4, 0.2, 0.7, 4.25
MS, LIMITS = (33, 257), (None, float("inf"))
GRID = [(s, p, M, lim) for s in kc.SHAPES for p in ("fp32", "bf16x3") for M in MS for lim in LIMITS]


class Problem:
    pass


class Rig:
    """One engine per (shape, precision) and its problem per M: contiguous tensors, the same samples as shuffled rows of tables of 2 M + 3 rows, the old policy's cache."""

    def __init__(self, shape, precision):
        import torch
        from mi355.ppo_device import PpoDevice
        self.din, self.A, self.hidden, _, _ = kc.SHAPES[shape]
        self.shape = shape
        low, high = pc.bounds(self.A)
        self.d = PpoDevice(self.din, self.A, low, high, pc.EPS, pc.VALUE_SCALE, pc.ENTROPY_SCALE, hidden=self.hidden, max_batch=320, precision=precision)
        assert self.d.fused_ok()
        self.used = torch.zeros(self.d.n_flat, dtype=torch.bool, device=self.d.device)
        for _, (o_, s_) in self.d.layout.items():
            self.used[o_:o_ + s_] = True
        self.problems = {}

    def up(self, x):
        import torch
        return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(self.d.device)

    def problem(self, M):
        import torch
        if M in self.problems:
            return self.problems[M]
        d, A = self.d, self.A
        q = Problem()
        q.M = M
        c = kc.build(self.shape, M)
        d.load_params(c.theta, pc.old_names(c.theta_old))
        d.adam_m.zero_(); d.adam_v.zero_()
        q.state0 = [x.clone() for x in (d.params, d.adam_m, d.adam_v, d.params_old)]
        rng = np.random.RandomState(700 + M)
        flat = {"s": self.up(c.s), "a": self.up(c.a), "R": self.up(c.R), "adv": self.up(c.adv), "vo": self.up(c.R + 0.3 * rng.standard_normal(M)),
                "lp": torch.empty(M, device=d.device), "mo": torch.empty(M, A, device=d.device)}
        d.old_policy_cache(flat["s"], flat["a"], M, flat["lp"], flat["mo"])
        n = 2 * M + 3
        q.rows = torch.from_numpy(rng.permutation(n)[:M].astype(np.int32)).to(d.device)
        tab = {}
        for k, x in flat.items():                                                    # lp / mo / vo: NaN in every row the index does not name
            shape_k = (n,) + tuple(x.shape[1:])
            tab[k] = self.up(0.5 * rng.standard_normal(shape_k)) if k in ("s", "a", "R", "adv") else torch.full(shape_k, float("nan"), device=d.device)
            tab[k][q.rows.long()] = x
        q.flat, q.tab = flat, tab
        self.problems[M] = q
        return q

    def run(self, q, limit, *calls):
        """The calls in order from the problem's start state with the gradient buffer at FILL -> [params, m, v, losses, kl_losses], the gradient buffer."""
        d = self.d
        for x, y in zip((d.params, d.adam_m, d.adam_v, d.params_old), q.state0):
            x.copy_(y)
        d.grads.fill_(FILL)
        d.set_max_grad_norm(limit)
        for f in calls:
            f()
        return [x.clone() for x in (d.params, d.adam_m, d.adam_v, d.losses, d.kl_losses)], d.grads.clone()


@pytest.fixture(scope="module")
def rigs():
    made = {}

    def get(shape, precision):
        if (shape, precision) not in made:
            made[(shape, precision)] = Rig(shape, precision)
        return made[(shape, precision)]
    yield get
    for r in made.values():
        r.d.close()


@pytest.fixture(scope="module")
def recording_comm():
    from mi355 import lib as milib
    L = milib.get()
    hcomm, log = ctypes.c_void_p(), np.zeros((256, 4), np.int64)
    L.mi_comm_init_recording(ctypes.addressof(hcomm), 0, 1, log.ctypes.data, 256)
    yield hcomm
    L.mi_comm_destroy(hcomm)


@pytest.mark.parametrize("shape,precision,M,limit", GRID)
def test_each_entry_takes_the_route_its_form_calls_for(rigs, recording_comm, shape, precision, M, limit):
    r = rigs(shape, precision)
    q, d = r.problem(M), r.d
    a = (M, 1.0 / M, 1.0, ALPHA)
    in_tile = M <= 256 and limit is None                                             # ... of a call without a communicator
    adam = lambda: d.apply_adam(ALPHA)      # noqa: E731
    written = lambda g: bool((g[r.used] != FILL).any())      # noqa: E731
    untouched = lambda g: bool((g == FILL).all())      # noqa: E731
    for form in ("flat", "rows"):
        t, rows = (q.flat, None) if form == "flat" else (q.tab, q.rows)
        data = (t["s"], t["a"], t["R"], t["adv"])
        tag = (shape, precision, M, limit, form)
        # the two entries with an adam argument, with and without the cache / old values, alone and on the recording communicator
        entries = {
            "vclip": lambda comm, **kw: d.train_step_vclip(comm, *data, t["lp"], t["vo"], EPS_V, rows, *a, **kw),
            "vclip_no_cache": lambda comm, **kw: d.train_step_vclip(comm, *data, None, t["vo"], EPS_V, rows, *a, **kw),
            "kl": lambda comm, **kw: d.train_step_kl(comm, *data, t["lp"], t["mo"], BETA, rows, *a, **kw),
            "kl_vclip_no_cache": lambda comm, **kw: d.train_step_kl(comm, *data, None, None, BETA, rows, *a, old_values=t["vo"], clip_range_vf=EPS_V, **kw),
        }
        for name, entry in entries.items():
            two_calls, g2 = r.run(q, limit, lambda: entry(None, adam=False), adam)
            assert written(g2), (tag, name)
            for comm in (None, recording_comm):
                one_call, g1 = r.run(q, limit, lambda: entry(comm))
                if comm is None and in_tile:
                    assert untouched(g1), (tag, name)
                    assert not bitwise(one_call[:3], q.state0[:3]), (tag, name)      # (it did train)
                else:
                    assert bitwise(one_call, two_calls) and bitwise(g1, g2), (tag, name, comm is not None)
        # the plain forms without log pi_old: forward_backward (contiguous tensors only), then apply_adam
        if form == "flat":
            two_calls, g2 = r.run(q, limit, lambda: d.forward_backward(*data, M, 1.0 / M, 1.0), adam)
            assert written(g2), tag
            one_call, g1 = r.run(q, limit, lambda: d.train_step(*data, *a))
            dp, gd = r.run(q, limit, lambda: d.train_step_dp(recording_comm, *data, None, None, *a))
            cached, gc = r.run(q, limit, lambda: d.train_step(*data, *a, logp_old=t["lp"]))
        else:
            two_calls, g2 = r.run(q, limit, lambda: d.train_step_dp(recording_comm, *data, None, rows, *a))
            one_call, g1 = r.run(q, limit, lambda: d.train_step_idx(*data, None, rows, *a))
            dp, gd = two_calls, g2
            cached, gc = r.run(q, limit, lambda: d.train_step_idx(*data, t["lp"], rows, *a))
        assert written(gd), tag                                                      # a communicator: the flat route at every M
        if form == "flat":
            assert bitwise(dp, two_calls) and bitwise(gd, g2), tag
        if in_tile:
            assert untouched(g1) and untouched(gc), tag
            assert not bitwise(one_call[:3], q.state0[:3]) and not bitwise(cached[:3], q.state0[:3]), tag
        else:
            assert bitwise(one_call, two_calls) and bitwise(g1, g2), tag
            with_comm, gw = r.run(q, limit, lambda: d.train_step_dp(recording_comm, *data, t["lp"], rows, *a))
            assert bitwise(cached, with_comm) and bitwise(gc, gw), tag
    d.set_max_grad_norm(None)
