"""The rollout step on the MlpVAE encoder, as far as a machine without a GPU can check it: the three C entries exist with the header's prototypes, the scratch
size is the documented layout and needs no handle, every argument error of both entries comes back before any launch with the entry's own name in front, and
rollout.py sends an "mlp" device to the new entries and everything else to the ones it always called."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "carla-ppo_amd"))

NEW = ("mi_mlp_rollout_workspace_bytes", "mi_mlp_rollout_step_batch", "mi_mlp_rollout_value_batch")


def desc(S, enc, z, dec=(8,), dtype=0, max_batch=4):
    from mi355 import lib as milib
    d = milib.MiMlpVaeDesc()
    d.dtype, d.max_batch, d.source_size, d.target_size, d.z_dim, d.n_enc, d.n_dec = dtype, max_batch, S, S, z, len(enc), len(dec)
    for i, h in enumerate(enc):
        d.enc[i] = h
    for i, h in enumerate(dec):
        d.dec[i] = h
    d.loss_kind, d.with_optimizer, d.beta, d.kl_tolerance = 0, 0, 1.0, 0.0
    return d


def test_the_three_entries_are_exported_with_the_headers_prototypes():
    from mi355 import lib as milib
    L = milib.get()
    protos = milib.parse_header()
    for name in NEW:
        assert name in protos and hasattr(L.cdll, name), name
    assert L.mi_abi_version() == 7
    ret, args = protos["mi_mlp_rollout_workspace_bytes"]
    assert ret == "long long" and [a[0] for a in args] == ["const MiMlpVaeDesc*", "int"]
    ret, args = protos["mi_mlp_rollout_step_batch"]
    assert ret == "int" and [a[1] for a in args] == ["mlp_h", "ppo_h", "stream", "frames_u8", "measurements", "n_meas", "noise", "greedy", "n", "scratch", "scratch_bytes", "out",
                                                    "obs_mean", "obs_inv_std", "obs_clip", "nstate", "table_rows", "n_table_rows", "tab_states", "tab_raw_states", "tab_actions",
                                                    "tab_values"]
    ret, args = protos["mi_mlp_rollout_value_batch"]
    assert ret == "int" and [a[1] for a in args] == ["mlp_h", "ppo_h", "stream", "frames_u8", "measurements", "n_meas", "n", "scratch", "scratch_bytes", "out", "obs_mean",
                                                    "obs_inv_std", "obs_clip", "nstate", "table_rows", "n_table_rows", "tab_final_values"]
    # the arguments of the ConvVAE's normalised entries, under the same names: the Python side passes one tuple to either
    assert [a[1] for a in protos["mi_mlp_rollout_step_batch"][1][2:]] == [a[1] for a in protos["mi_rollout_step_batch_norm"][1][2:]]
    assert [a[1] for a in protos["mi_mlp_rollout_value_batch"][1][2:]] == [a[1] for a in protos["mi_rollout_value_batch_norm"][1][2:]]


@pytest.mark.parametrize("S,enc,z", [(38400, (512, 256), 64), (72, (36,), 8), (264, (132, 20, 12, 8), 8)])
def test_workspace_bytes_is_the_documented_layout_and_needs_no_handle(S, enc, z):
    """raw sums [n][enc[0]] | .. | [n][enc[-1]] | raw means [n][z], fp32: 4 n (sum(enc) + z) bytes."""
    from mi355 import lib as milib
    L = milib.get()
    d = desc(S, enc, z)
    for n in (1, 2, 31, 32, 33, 64, 65, 1024):
        assert L.mi_mlp_rollout_workspace_bytes(ctypes.byref(d), n) == 4 * n * (sum(enc) + z), n
    for dt in (0, 1):                                                                 # the step reads the fp32 master weights whatever the storage type
        if dt == 0 or all(v % 8 == 0 for v in (S, z) + enc):
            assert L.mi_mlp_rollout_workspace_bytes(ctypes.byref(desc(S, enc, z, dtype=dt)), 3) == 12 * (sum(enc) + z)


def test_workspace_bytes_refuses_bad_counts_and_bad_descs():
    from mi355 import lib as milib
    L = milib.get()
    err = L.cdll.mi_last_error
    good = desc(72, (36,), 8)
    for n in (0, -1, 1025):
        assert L.mi_mlp_rollout_workspace_bytes(ctypes.byref(good), n) == -1 and err().startswith(b"mi_mlp_rollout_workspace_bytes: 1 <= n_envs <= MI_ROLLOUT_MAX_ENVS"), n
    for bad in (desc(70, (36,), 8), desc(72, (34,), 8), desc(72, (36,), 6), desc(72, (), 8), desc(72, (36,), 8, dtype=2), desc(72, (36,), 8, dtype=1)):
        assert L.mi_mlp_rollout_workspace_bytes(ctypes.byref(bad), 4) == -2 and err().startswith(b"mi_mlp_rollout_workspace_bytes: unsupported sizes")
        assert L.mi_mlpvae_param_floats(ctypes.byref(bad)) == -1                      # the engine refuses the same descs
    assert L.mi_mlp_rollout_workspace_bytes(None, 4) == -2


def test_every_argument_error_before_any_launch():
    """No check needs a device and every one runs before the first launch: the dummy host buffers are never written.  Each message starts with the entry's name."""
    from mi355 import lib as milib
    L = milib.get()
    buf = (ctypes.c_double * 64)()
    base = ctypes.addressof(buf)
    base += -base % 16
    p, odd, odd2 = ctypes.c_void_p(base), ctypes.c_void_p(base + 4), ctypes.c_void_p(base + 2)
    err = L.cdll.mi_last_error
    flt = ctypes.c_float

    def step(mlp=p, ppo=p, frames=p, meas=p, noise=None, greedy=1, n=4, scratch=p, out=p, mean=p, inv=p, clip=10.0, nstate=p, rows=p, n_rows=8, ts=p, tr=p, ta=p, tv=p):
        return L.cdll.mi_mlp_rollout_step_batch(mlp, ppo, None, frames, meas, 3, noise, greedy, n, scratch, 0, out, mean, inv, flt(clip), nstate, rows, n_rows, ts, tr, ta, tv)
    me = b"mi_mlp_rollout_step_batch: "
    for h in ("mlp", "ppo"):
        assert step(**{h: None}) == -4 and err() == me + b"null handle", h
    for kw in (dict(frames=None), dict(out=None), dict(scratch=None), dict(meas=None), dict(greedy=0)):
        assert step(**kw) == -1 and err() == me + b"missing buffers", kw
    for kw in (dict(ts=None), dict(tr=None), dict(ta=None), dict(tv=None), dict(n_rows=0)):
        assert step(**kw) == -1 and err() == me + b"missing tables", kw
    for name in ("inv", "nstate"):
        assert step(**{name: None}) == -1 and err().startswith(me + b"missing obs_mean / obs_inv_std / nstate"), name
    assert step(nstate=odd) == -1 and err().startswith(me + b"nstate must be 16-byte aligned")
    for bad in (0.0, -2.0, float("nan")):
        assert step(clip=bad) == -1 and err().startswith(me + b"obs_clip"), bad
    # obs_mean NULL = not normalised: what belongs to it must be NULL too
    for kw in (dict(), dict(inv=None), dict(inv=None, nstate=None), dict(inv=None, tr=None)):
        assert step(mean=None, **kw) == -1 and err().startswith(me + b"obs_inv_std, nstate and tab_raw_states are NULL where obs_mean is"), kw
    plain = dict(mean=None, inv=None, nstate=None, tr=None)
    assert step(ts=None, **plain) == -1 and err() == me + b"missing tables"            # the recording step without normalisation still needs its three tables
    for bad in (0, -1, 1025):
        assert step(n=bad, **plain) == -1 and err().startswith(me + b"1 <= n <= MI_ROLLOUT_MAX_ENVS"), bad
        assert step(n=bad, clip=float("inf")) == -1 and err().startswith(me + b"1 <= n <= MI_ROLLOUT_MAX_ENVS"), bad        # +inf is a valid clip: the next check answers
    # table_rows NULL records nothing and reads no table: the call gets as far as the range of n
    assert step(rows=None, ts=None, ta=None, tv=None, n=0, **plain) == -1 and err().startswith(me + b"1 <= n <= MI_ROLLOUT_MAX_ENVS")
    assert step(frames=odd2, **plain) == -1 and err().startswith(me + b"the frames must be 4-byte aligned")
    assert step(scratch=odd, **plain) == -1 and err().startswith(me + b"the scratch must be 16-byte aligned")

    def value(mlp=p, ppo=p, frames=p, meas=p, n=4, scratch=p, out=p, mean=p, inv=p, clip=10.0, nstate=p, rows=p, n_rows=8, tf=p):
        return L.cdll.mi_mlp_rollout_value_batch(mlp, ppo, None, frames, meas, 3, n, scratch, 0, out, mean, inv, flt(clip), nstate, rows, n_rows, tf)
    me = b"mi_mlp_rollout_value_batch: "
    for h in ("mlp", "ppo"):
        assert value(**{h: None}) == -4 and err() == me + b"null handle", h
    for kw in (dict(frames=None), dict(out=None), dict(scratch=None), dict(meas=None)):
        assert value(**kw) == -1 and err() == me + b"missing buffers", kw
    for kw in (dict(tf=None), dict(n_rows=0)):
        assert value(**kw) == -1 and err() == me + b"missing tables", kw
    for name in ("inv", "nstate"):
        assert value(**{name: None}) == -1 and err().startswith(me + b"missing obs_mean / obs_inv_std / nstate"), name
    assert value(nstate=odd) == -1 and err().startswith(me + b"nstate must be 16-byte aligned")
    for bad in (0.0, float("nan")):
        assert value(clip=bad) == -1 and err().startswith(me + b"obs_clip"), bad
    assert value(mean=None) == -1 and err().startswith(me + b"obs_inv_std, nstate and tab_raw_states are NULL where obs_mean is")
    plain = dict(mean=None, inv=None, nstate=None)
    for bad in (0, 1025):
        assert value(n=bad, **plain) == -1 and err().startswith(me + b"1 <= n <= MI_ROLLOUT_MAX_ENVS"), bad
    assert value(rows=None, tf=None, n=0, **plain) == -1 and err().startswith(me + b"1 <= n <= MI_ROLLOUT_MAX_ENVS")      # table_rows may be NULL here too
    assert value(frames=odd2, **plain) == -1 and err().startswith(me + b"the frames must be 4-byte aligned")
    assert value(scratch=odd, **plain) == -1 and err().startswith(me + b"the scratch must be 16-byte aligned")

    # a short scratch: the size comes from the engine, so this check needs a real MlpVAE handle -- which mi_mlpvae_create makes on the host alone (it only keeps
    # the pointers it is given).  The check comes before anything reads the PPO handle.
    d = desc(72, (36,), 8)
    ws = (ctypes.c_char * 512)()
    wbase = ctypes.addressof(ws)
    wbase += -wbase % 256
    need_ws = L.mi_mlpvae_workspace_bytes(ctypes.byref(d))
    h = L.cdll.mi_mlpvae_create(ctypes.byref(d), p, None, None, None, None, p, ctypes.c_void_p(wbase), ctypes.c_longlong(max(need_ws, 1 << 20)))
    assert h
    try:
        need = L.mi_mlp_rollout_workspace_bytes(ctypes.byref(d), 4)
        assert need == 4 * 4 * 44
        rc = L.cdll.mi_mlp_rollout_step_batch(h, p, None, p, p, 3, None, 1, 4, p, ctypes.c_longlong(need - 1), p, None, None, flt(0.0), None, None, 0, None, None, None, None)
        assert rc == -1 and err().startswith(b"mi_mlp_rollout_step_batch: scratch too small (mi_mlp_rollout_workspace_bytes)")
        rc = L.cdll.mi_mlp_rollout_value_batch(h, p, None, p, p, 3, 4, p, ctypes.c_longlong(need - 1), p, None, None, flt(0.0), None, None, 0, None)
        assert rc == -1 and err().startswith(b"mi_mlp_rollout_value_batch: scratch too small (mi_mlp_rollout_workspace_bytes)")
    finally:
        L.mi_mlpvae_destroy(h)
    assert all(x == 0.0 for x in buf)
    # the neighbours keep their messages, and never look at the handle
    assert L.cdll.mi_rollout_step_batch(p, p, None, None, p, 3, None, 1, 4, p, 0, p) == -1 and err() == b"mi_rollout_step_batch: missing buffers"
    assert L.cdll.mi_rollout_value_batch_rec(p, p, None, p, p, 3, 4, p, 0, p, None, 8, p) == -1 and err() == b"mi_rollout_value_batch_rec: missing tables"


# ---- which entries the step classes call: a stub library that records names, CPU tensors in place of the pinned / device ones ----
class StubLib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("mi_"):
            raise AttributeError(name)

        def entry(*args):
            self.calls.append((name, len(args), args))
            return 0
        return entry


def stub_buffer(monkeypatch, kind, E=3, T=4):
    import torch
    import rollout
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: types.SimpleNamespace(cuda_stream=0, synchronize=lambda: None))
    s = object.__new__(rollout._RecordingStep)
    s.L, s.num_envs, s.z_dim, s.A, s.n_meas, s.frame_bytes, s.io, s.device = StubLib(), E, 4, 2, 3, 12, "pinned", "cpu"
    s._rng, s._obs_norm, s.row = np.random.Generator(np.random.Philox(1)), None, 2 + 1 + 4
    if kind is not None:
        s._kind = kind
    s._f_off = (E * s.frame_bytes + 15) // 16 * 16
    s.h_in, s.h_out = torch.zeros(s._f_off + 4 * E * (s.n_meas + s.A + 1), dtype=torch.uint8), torch.zeros(E * s.row)
    s.d_in = s.d_out = None
    s._in_np = s.h_in.numpy()
    s._f_np, s._i_np = s._in_np[s._f_off:].view(np.float32), s._in_np[s._f_off:].view(np.int32)
    s._out_np = s.h_out.numpy().reshape(E, s.row)
    s.scratch, s.scratch_bytes = torch.zeros(16, dtype=torch.uint8), 16
    s.vae = s.ppo = types.SimpleNamespace(dev=types.SimpleNamespace(handle=1))
    b = object.__new__(rollout.ContinuousRolloutBuffer)
    b.rows, b._step, b.L, b.device, b.num_envs, b.horizon, b.n_table_rows = rollout.SegmentedRows(E, T), s, s.L, "cpu", E, T, E * (T + 1)
    b.states, b.actions = torch.zeros(b.n_table_rows, 7), torch.zeros(b.n_table_rows, 2)
    b.values, b.final_values = torch.zeros(b.n_table_rows), torch.zeros(b.n_table_rows)
    b._obs_norm = b.raw_states = None
    return b, s


def collect(b, E):
    frames, meas = np.zeros((E, 2, 2, 3), np.uint8), np.zeros((E, 3))
    b.rows.reset()
    b.step(frames, meas)
    b.outcome(np.zeros(E), np.zeros(E, bool))
    b.truncate(frames[:1], meas[:1], env_ids=[0])
    b.bootstrap(frames[1:], meas[1:], env_ids=np.arange(1, E))


def test_an_mlp_device_goes_to_the_new_entries_and_nothing_else_does(monkeypatch):
    import torch
    import rollout
    from mi355 import lib as milib
    protos = milib.parse_header()
    n_step, n_value = len(protos["mi_mlp_rollout_step_batch"][1]), len(protos["mi_mlp_rollout_value_batch"][1])
    assert (n_step, n_value) == (22, 17)
    b, s = stub_buffer(monkeypatch, "mlp")
    collect(b, 3)
    s(np.zeros((2, 2, 2, 3), np.uint8), np.zeros((2, 3)), greedy=True)
    assert [c[:2] for c in s.L.calls] == [("mi_mlp_rollout_step_batch", n_step), ("mi_mlp_rollout_value_batch", n_value), ("mi_mlp_rollout_step_batch", n_step),
                                          ("mi_mlp_rollout_step_batch", n_step)]
    rec, val, _, plain = [c[2] for c in s.L.calls]
    assert rec[12:16] == (None, None, 0.0, None) and rec[16] is not None and rec[17] == b.n_table_rows and rec[19] is None          # not normalised; recording, no raw table
    assert rec[18] == b.states.data_ptr() and rec[20] == b.actions.data_ptr() and rec[21] == b.values.data_ptr()
    assert val[10:14] == (None, None, 0.0, None) and val[15] == b.n_table_rows and val[16] == b.final_values.data_ptr()
    assert plain[12:] == (None, None, 0.0, None, None, 0, None, None, None, None)                                                  # the evaluation step: nothing recorded
    # with observation normalisation on: the same two entries, the statistics and both tables filled in
    del s.L.calls[:]
    on = rollout._obs_norm_tensors("cpu", 7, 3)
    on.update(rollout.observation_normalization_settings())
    b._obs_norm = s._obs_norm = on
    b.raw_states = torch.zeros_like(b.states)
    collect(b, 3)
    s(np.zeros((2, 2, 2, 3), np.uint8), np.zeros((2, 3)), greedy=True)
    assert [c[:2] for c in s.L.calls] == [("mi_mlp_rollout_step_batch", n_step), ("mi_mlp_rollout_value_batch", n_value), ("mi_mlp_rollout_step_batch", n_step),
                                          ("mi_mlp_rollout_step_batch", n_step)]
    rec, val, _, plain = [c[2] for c in s.L.calls]
    norm = (on["mean32"].data_ptr(), on["inv32"].data_ptr(), on["clip"], on["nstate"].data_ptr())
    assert rec[12:16] == norm and rec[18] == b.states.data_ptr() and rec[19] == b.raw_states.data_ptr()
    assert val[10:14] == norm and plain[12:16] == norm and plain[16:] == (None, 0, None, None, None, None)
    # a conv device, and a fake without the attribute at all, call what they always called
    for kind in ("conv", None):
        b, s = stub_buffer(monkeypatch, kind)
        collect(b, 3)
        s(np.zeros((2, 2, 2, 3), np.uint8), np.zeros((2, 3)), greedy=True)
        assert [c[:2] for c in s.L.calls] == [("mi_rollout_step_batch_rec", 17), ("mi_rollout_value_batch_rec", 13), ("mi_rollout_step_batch_rec", 17), ("mi_rollout_step_batch", 12)], kind


class FakeDev:
    source_shape = (2, 2, 3)
    device = "cpu"
    handle = 1

    def __init__(self, kind):
        self.L = StubLib()
        if kind is not None:
            self.rollout_kind = kind


class FakeModel:
    z_dim, num_actions, input_dim, seed = 4, 2, 7, 0

    def __init__(self, kind=None):
        self.dev = FakeDev(kind)

    def _need_dev(self):
        return self.dev


def test_setup_reads_the_kind_and_the_single_frame_step_refuses_an_mlp_encoder():
    import rollout
    for kind, want in ((None, "conv"), ("conv", "conv"), ("mlp", "mlp")):
        s = object.__new__(rollout.BatchedRolloutStep)
        s._setup("BatchedRolloutStep", FakeModel(kind), FakeModel(), None, "pinned")
        assert s._kind == want
    s = object.__new__(rollout.BatchedRolloutStep)
    with pytest.raises(ValueError, match="unknown encoder kind"):
        s._setup("BatchedRolloutStep", FakeModel("tcn"), FakeModel(), None, "pinned")
    vae = FakeModel("mlp")
    with pytest.raises(ValueError, match=r"RolloutStep: .*BatchedRolloutStep\(vae, ppo, num_envs=1\)"):
        rollout.RolloutStep(vae, FakeModel())
    assert vae.dev.L.calls == []                                                     # before anything reaches C
    from mi355.mlp_vae_device import MlpVaeDevice
    from mi355.vae_device import VaeDevice
    assert MlpVaeDevice.rollout_kind == "mlp" and getattr(VaeDevice, "rollout_kind", "conv") == "conv"
