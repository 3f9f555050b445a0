"""CPU-only characterisation of PPO._step_resident / _step_rows / _kl_step: WHICH device call a minibatch step becomes, with which arguments, for every combination of
world, form, option, cached log pi_old, the two environment switches and fused_ok().  The device is a stub that records (method name, arguments, keywords) of every
step call; mi355.dist's world_size / rank / mi_comm / all_reduce_sum are replaced, the all-reduce logging into the same list.  fused_ok() is a question, not a step: it
is answered from the cell and only counted (at most once per step).  Every cell runs two consecutive steps and pins either the ordered log of both and the two beta
powers afterwards, or the exception's type and full text with the log empty and the powers untouched.  expected() spells the table out of its parts, independently
of ppo.py.  Also: the null-handle refusal of the four C entries that look at their handle right behind it."""
import ctypes
import itertools

import numpy as np
import pytest

from oracle import ppo_oracle as po

B1, B2, EPS = 0.9, 0.999, 1e-8
N_ROWS, M_LOCAL, DIN, A = 9, 4, 67, 2
VALUE_CLIP, KL_COEF, HANDLE = 0.2, 0.5, 0xC0FFEE
WORLDS = ("w1", "w2_comm", "w2_no_comm", "w2_host_loop")
# fronts: "resident" = _step_resident, "rows" = _step_rows, "kl_flat" / "kl_rows" = _kl_step without / with rows; the options each can express are in CELLS below
# option -> (value_clip set, KL penalty on, mean_old given, old values given)
OPTIONS = {"plain": (False, False, False, False), "vclip": (True, False, False, True), "old_values_without_vclip": (False, False, False, True),
           "kl_mean": (False, True, True, False), "kl_no_mean": (False, True, False, False), "kl_vclip_mean": (True, True, True, True),
           "kl_vclip_no_mean": (True, True, False, True), "kl_old_values_without_vclip": (False, True, True, True)}
# what each front can be asked: _step_resident takes no old values (value_clip set changes nothing there) and _step_rows no mean_old; _kl_step is the rollout buffers' entry
CELLS = [("resident", o) for o in ("plain", "vclip", "kl_mean", "kl_no_mean")] + \
        [("rows", o) for o in ("plain", "vclip", "old_values_without_vclip", "kl_no_mean", "kl_vclip_no_mean", "kl_old_values_without_vclip")] + \
        [("kl_flat", o) for o in ("kl_mean", "kl_no_mean", "kl_vclip_mean", "kl_vclip_no_mean", "kl_old_values_without_vclip")] + \
        [("kl_rows", o) for o in ("kl_mean", "kl_no_mean", "kl_vclip_mean", "kl_vclip_no_mean", "kl_old_values_without_vclip")]
KL_TEXT = ("PPO: the KL penalty needs the fused one-call step (this policy's shape is outside the fused kernels' range, "
           "MI355_PPO_FUSED=0 / MI355_PPO_IDX=0, or data parallel without the library's communicator)")
VCLIP_TEXT = ("PPO._step_rows: value clipping needs the fused one-call step (this policy's shape is outside the fused kernels' range, "
              "MI355_PPO_FUSED=0 / MI355_PPO_IDX=0, or data parallel without the library's communicator)")
OFF_TEXT = "PPO.%s: old values were passed but value clipping is off (set_value_clip)"


class _Comm:
    handle = HANDLE


class StubDev:
    """Records every step call; tensors it was built with are logged by name, any other tensor by its values."""

    def __init__(self, log, names):
        import torch
        self.log, self.names, self.ok, self.asked = log, names, True, 0
        self.grads = torch.zeros(4)
        names[id(self.grads)] = "grads"

    def fused_ok(self):
        self.asked += 1
        return self.ok

    def __getattr__(self, name):
        if name not in ("train_step", "train_step_idx", "train_step_dp", "train_step_vclip", "train_step_kl", "forward_backward", "apply_adam"):
            raise AttributeError(name)

        def call(*args, **kw):
            self.log.append((name, tuple(seen(self.names, x) for x in args), {k: seen(self.names, v) for k, v in kw.items()}))
        return call


def seen(names, x):
    import torch
    if isinstance(x, torch.Tensor):
        return names.get(id(x)) or ("tensor", str(x.dtype), tuple(x.shape), x.is_contiguous(), x.reshape(-1).tolist())
    return x


@pytest.fixture()
def rig(tmp_path, monkeypatch):
    import torch
    from mi355 import dist as midist
    from ppo import PPO
    for k in ("MI355_PPO_KL_COEF", "MI355_PPO_MAX_GRAD_NORM", "MI355_DP_SKIP_ALLREDUCE", "MI355_DP_HOST_LOOP", "MI355_PPO_FUSED", "MI355_PPO_IDX"):
        monkeypatch.delenv(k, raising=False)
    m = PPO(np.array([DIN]), po.ActionSpace(), learning_rate=3e-4, lr_decay=0.998, model_dir=str(tmp_path), seed=1)
    m.episode_counter = 3                                                            # a learning rate that has decayed
    g = torch.Generator().manual_seed(7)
    t = {"s": torch.randn(N_ROWS, DIN, generator=g), "a": torch.randn(N_ROWS, A, generator=g), "r": torch.randn(N_ROWS, generator=g),
         "adv": torch.randn(N_ROWS, generator=g), "logp": torch.randn(N_ROWS, generator=g), "mean": torch.randn(N_ROWS, A, generator=g),
         "vold": torch.randn(N_ROWS, generator=g), "rows": torch.tensor([7, 2, 5, 0], dtype=torch.int32)}
    log = []
    names = {id(v): k for k, v in t.items()}
    m.dev = StubDev(log, names)
    monkeypatch.setattr(midist, "rank", lambda: 0)
    monkeypatch.setattr(midist, "all_reduce_sum", lambda x, async_op=False: log.append(("all_reduce_sum", (seen(names, x),), {})))
    return m, t, log, midist


def set_world(monkeypatch, midist, world):
    monkeypatch.setattr(midist, "world_size", lambda: 1 if world == "w1" else 2)
    monkeypatch.setattr(midist, "mi_comm", lambda: _Comm if world in ("w2_comm", "w2_host_loop") else None)
    if world == "w2_host_loop":
        monkeypatch.setenv("MI355_DP_HOST_LOOP", "1")
    else:
        monkeypatch.delenv("MI355_DP_HOST_LOOP", raising=False)


def alpha_of(lr, b1p, b2p):
    one = np.float32(1.0)
    return np.float32(np.float32(lr) * np.sqrt(one - np.float32(b2p), dtype=np.float32) / (one - np.float32(b1p)))


def gathered(t, name):
    x = t[name][t["rows"].long()].contiguous()
    return ("tensor", str(x.dtype), tuple(x.shape), True, x.reshape(-1).tolist())


def expected(t, world, front, option, logp, fused, idx, ok, lr, b1p, b2p):
    """-> ("raise", type, text) or ("log", [entries]) of ONE step from the beta powers given."""
    value_clip, kl, mean, old_values = OPTIONS[option]
    W = 1 if world == "w1" else 2
    comm = HANDLE if world == "w2_comm" else None                                    # the host loop switch and a process group without the library communicator: none
    rows = front in ("rows", "kl_rows")
    m_global = M_LOCAL * W
    scale = (M_LOCAL, 1.0 / m_global, M_LOCAL / float(m_global))
    adam = (alpha_of(lr, b1p, b2p), B1, B2, EPS)
    data = ("s", "a", "r", "adv")
    lp = "logp" if logp else None
    if old_values and not value_clip:
        return ("raise", ValueError, OFF_TEXT % ("_step_rows" if front == "rows" else "_kl_step"))
    if kl:
        one_call = fused and (not rows or idx) and ok
        if not one_call or (W > 1 and comm is None):
            return ("raise", ValueError, KL_TEXT)
        if not mean:
            lp = None                                                                # without the old means the cached log pi_old is dropped
        return ("log", [("train_step_kl", (comm,) + data + (lp, "mean" if mean else None, KL_COEF, "rows" if rows else None) + scale + adam,
                         {"old_values": "vold" if old_values else None, "clip_range_vf": VALUE_CLIP if old_values else None})])
    if front == "rows":
        if old_values:
            if not (fused and idx and ok) or (W > 1 and comm is None):
                return ("raise", ValueError, VCLIP_TEXT)
            return ("log", [("train_step_vclip", (comm,) + data + (lp, "vold", VALUE_CLIP, "rows") + scale + adam, {})])
        if fused and idx and ok and W == 1:
            return ("log", [("train_step_idx", data + (lp, "rows") + scale + adam, {})])
        if fused and idx and ok and comm is not None:
            return ("log", [("train_step_dp", (comm,) + data + (lp, "rows") + scale + adam, {})])
        data = tuple(gathered(t, k) for k in data)                                   # the rows are gathered on the host and the contiguous form takes over
        lp = gathered(t, "logp") if logp else None
    if W == 1 and fused:                                                             # (fused_ok() is not asked: the C entry falls back by itself)
        return ("log", [("train_step", data + scale + adam, {"logp_old": lp})])
    if comm is not None:                                                             # (even with MI355_PPO_FUSED=0)
        return ("log", [("train_step_dp", (comm,) + data + (lp, None) + scale + adam, {})])
    out = [("forward_backward", data + scale, {})]                                   # (the cached log pi_old is not used)
    if W > 1:
        out.append(("all_reduce_sum", ("grads",), {}))
    return ("log", out + [("apply_adam", adam, {})])


def call(m, t, front, option, logp):
    _, _, mean, old_values = OPTIONS[option]
    W = 2 if m._world != "w1" else 1
    lp, mo, vo = t["logp"] if logp else None, t["mean"] if mean else None, t["vold"] if old_values else None
    if front == "resident":
        kw = {"mean_old": mo} if mean else {}
        return m._step_resident(t["s"], t["a"], t["r"], t["adv"], M_LOCAL, M_LOCAL * W, logp_old=lp, **kw)
    if front == "rows":
        kw = {"old_values_all": vo} if old_values else {}
        return m._step_rows(t["s"], t["a"], t["r"], t["adv"], lp, t["rows"], M_LOCAL, M_LOCAL * W, **kw)
    kw = {"old_values": vo} if old_values else {}
    return m._kl_step(t["s"], t["a"], t["r"], t["adv"], lp, mo, t["rows"] if front == "kl_rows" else None, M_LOCAL, M_LOCAL * W, **kw)


def same(got, want):
    """Equal entry by entry; numbers compare by value AND type family (a float32 alpha is not a float)."""
    if isinstance(want, (tuple, list)):
        return isinstance(got, (tuple, list)) and len(got) == len(want) and all(same(g, w) for g, w in zip(got, want))
    if isinstance(want, dict):
        return isinstance(got, dict) and sorted(got) == sorted(want) and all(same(got[k], want[k]) for k in want)
    if isinstance(want, np.float32):
        return isinstance(got, np.float32) and got.tobytes() == want.tobytes()
    return type(got) is type(want) and got == want


@pytest.mark.parametrize("front,option", CELLS, ids=["%s-%s" % c for c in CELLS])
@pytest.mark.parametrize("world", WORLDS)
def test_every_cell_of_the_dispatch(rig, monkeypatch, world, front, option):
    m, t, log, midist = rig
    set_world(monkeypatch, midist, world)
    m._world = world
    value_clip, kl, _, _ = OPTIONS[option]
    m.value_clip = VALUE_CLIP if value_clip else None
    m.kl_penalty = KL_COEF if kl else None
    lr = m.current_learning_rate()
    for logp, fused, idx, ok in itertools.product((True, False), (True, False), (True, False), (True, False)):
        for name, on in (("MI355_PPO_FUSED", fused), ("MI355_PPO_IDX", idx)):
            if on:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, "0")
        tag = (world, front, option, logp, fused, idx, ok)
        m.dev.ok = ok
        m.beta1_power, m.beta2_power = np.float32(B1), np.float32(B2)
        del log[:]
        b1p, b2p, want_log = m.beta1_power, m.beta2_power, []
        for step in range(2):
            want = expected(t, world, front, option, logp, fused, idx, ok, lr, b1p, b2p)
            m.dev.asked = 0
            if want[0] == "raise":
                with pytest.raises(want[1]) as info:
                    call(m, t, front, option, logp)
                assert str(info.value) == want[2], tag
            else:
                assert call(m, t, front, option, logp) is None, tag
                want_log += want[1]
                b1p, b2p = np.float32(b1p * np.float32(B1)), np.float32(b2p * np.float32(B2))
            assert m.dev.asked <= 1, tag
        assert same(log, want_log), (tag, log, want_log)
        assert same((m.beta1_power, m.beta2_power), (b1p, b2p)), tag              # once per step that ran, in fp32; a refused step leaves them


def test_the_grid_is_the_one_described():
    """4 worlds x 20 (front, option) pairs x 16 switch settings, two steps each; both refusals, every device call and the host gather occur."""
    import torch
    t = {k: torch.zeros(N_ROWS, *s) for k, s in (("s", (DIN,)), ("a", (A,)), ("r", ()), ("adv", ()), ("logp", ()))}
    t["rows"] = torch.tensor([7, 2, 5, 0], dtype=torch.int32)
    kinds = set()
    n = 0
    for world, (front, option) in itertools.product(WORLDS, CELLS):
        for logp, fused, idx, ok in itertools.product((True, False), repeat=4):
            want = expected(t, world, front, option, logp, fused, idx, ok, np.float32(3e-4), np.float32(B1), np.float32(B2))
            kinds.add(want[2] if want[0] == "raise" else tuple(e[0] for e in want[1]))
            n += 1
    assert n == 4 * 20 * 16
    assert kinds == {KL_TEXT, VCLIP_TEXT, OFF_TEXT % "_step_rows", OFF_TEXT % "_kl_step", ("train_step",), ("train_step_idx",), ("train_step_dp",), ("train_step_vclip",),
                     ("train_step_kl",), ("forward_backward", "apply_adam"), ("forward_backward", "all_reduce_sum", "apply_adam")}


def test_null_handle_of_the_four_entries_that_read_the_engine_next():
    """mi_ppo_train_step / _idx / _dp / mi_ppo_forward_backward look at e->d.max_batch right behind the null check, so a dummy handle reaches nothing further: the
    walk of their host-checkable errors is the null-handle code and text (the _vclip / _kl walks are in test_value_clip_host.py / test_kl_penalty_host.py)."""
    from mi355 import lib as milib
    protos = milib.parse_header()
    cdll = ctypes.CDLL(milib.LIB_PATH)
    cdll.mi_last_error.restype = ctypes.c_char_p
    for name in ("mi_ppo_train_step", "mi_ppo_train_step_idx", "mi_ppo_train_step_dp", "mi_ppo_forward_backward"):
        fn = getattr(cdll, name)
        fn.restype = ctypes.c_int
        fn.argtypes = [milib._CTYPES[t] for t, _ in protos[name][1]]
        args = [None if t is ctypes.c_void_p else 1 for t in fn.argtypes]
        assert fn(*args) == -4 and cdll.mi_last_error() == b"ppo engine: null handle", name      # MI_ERR_STATE
