"""Latent stacking on the GPU: rollout_stack_kernel behind both encoder chains (mi_rollout_step_batch_stack / mi_rollout_value_batch_stack and their mi_mlp_ forms),
BatchedRolloutStep / RolloutBuffer / ContinuousRolloutBuffer built by stacked(.., latent_stack=k).

The stacking itself is copying, so the assertions are bitwise and do not depend on the encoders' split-K atomics: the expected row of a call is assembled on the host
(tests/latent_stack_cases.py) from the latent THAT call returned and the latents the EARLIER calls returned.  The only tolerances are the project's own:
actions rtol 1e-4 / atol 1e-5 and values rel 1e-4 / abs 1e-5 against oracle.ppo_oracle (float64 parameters of the same values, fed the device's stacked state), 1e-5
between two device paths (both end in fp32 atomics), 1 fp32 ulp for the normalised table against normalize_observations(raw_states).

Encoders: the MlpVAE 72 -> (36,) -> 8 on (4, 6, 3) frames for z_dim = 8, the ConvVAE of rollout_gpu_common at z_dim = 64.  Shapes: latent_stack_cases.KERNEL_SHAPES.
The first thing the module does is to look for the new symbols: on a tree without the feature every test fails there, before any device call."""
import copy
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "carla-ppo_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import latent_stack_cases as lc  # noqa: E402
from oracle import ppo_oracle as po  # noqa: E402
from oracle import vae_oracle as vo  # noqa: E402
from rollout_gpu_common import SENTINEL, bitwise, flat_state, make_vae, vae_params  # noqa: E402

pytestmark = pytest.mark.gpu

MLP_SRC, MLP_ENC, MLP_Z = (4, 6, 3), (36,), 8
HP = dict(learning_rate=1e-4, lr_decay=1.0, epsilon=0.2, value_scale=1.0, entropy_scale=0.01, initial_std=1.0)
PAD = 8                                                                              # sentinels behind every buffer the kernel writes


class World:
    def __init__(self, tmp):
        self.tmp, self._vaes, self.count = tmp, {}, 0

    def vae(self, z_dim):
        if z_dim not in self._vaes:
            if z_dim == MLP_Z:
                from vae.models import MlpVAE
                rng = np.random.RandomState(21)
                p = vo.init_mlp_vae_params(3, z_dim=MLP_Z, source_shape=MLP_SRC, target_shape=MLP_SRC, encoder_sizes=MLP_ENC, decoder_sizes=(8,))
                for k in p:
                    if k.endswith("bias"):
                        p[k] = (0.05 * rng.standard_normal(p[k].shape)).astype(np.float32)
                v = MlpVAE(np.array(MLP_SRC), encoder_sizes=MLP_ENC, decoder_sizes=(8,), z_dim=MLP_Z, model_dir=str(self.tmp / "mlp_vae"), precision="fp32", training=False)
                v.set_weights(p)
                v.init_session(init_logging=False)
            else:
                assert z_dim == 64
                v = make_vae(self.tmp / "conv_vae", vae_params())
            self._vaes[z_dim] = v
        return self._vaes[z_dim]

    def frames(self, rng, z_dim, n):
        return rng.randint(0, 256, (n,) + (MLP_SRC if z_dim == MLP_Z else (80, 160, 3)), dtype=np.uint8)

    def pair(self, din, n_act=2, seed=2):
        """An oracle / device policy pair with the same weights (N(0, 0.05) biases), wide inputs on."""
        import ppo_shape_cases as pc
        from ppo import PPO
        space = po.ActionSpace() if n_act == 2 else po.ActionSpace(*pc.bounds(n_act))
        o = po.OraclePPO([din], space, seed=seed, **HP)
        rng = np.random.RandomState(40 + n_act)
        for k in o.params:
            if k.endswith("bias"):
                o.params[k] = (0.05 * rng.standard_normal(o.params[k].shape)).astype(np.float32)
        self.count += 1
        m = PPO(np.array([din]), space, model_dir=str(self.tmp / ("ppo_%d" % self.count)), seed=seed, **HP)
        m.set_weights(o.params)
        m.set_wide_inputs()
        m.init_session(init_logging=False)
        assert m.dev.fused_ok() == (din <= 1024)
        return o, m


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    from mi355 import lib as milib
    L = milib.get()
    for name in ("mi_rollout_step_batch_stack", "mi_rollout_value_batch_stack", "mi_mlp_rollout_step_batch_stack", "mi_mlp_rollout_value_batch_stack"):
        assert hasattr(L.cdll, name), "the library has no stacked rollout step: " + name
    return World(tmp_path_factory.mktemp("latent_stack"))


def measurements(rng, n, n_meas):
    base = np.stack([rng.uniform(-1, 1, n), rng.uniform(0, 1, n), rng.uniform(0, 30, n)] + [rng.uniform(-2, 2, n) for _ in range(max(0, n_meas - 3))], axis=1)
    return np.ascontiguousarray(base[:, :n_meas])


def padded(t, value=SENTINEL):
    """-> (a tensor of t's shape and contents that is the head of a larger one, the PAD floats behind it)."""
    import torch
    big = torch.full((t.numel() + PAD,), value, dtype=t.dtype, device=t.device)
    big[:t.numel()] = t.reshape(-1)
    return big[:t.numel()].view(t.shape), big[t.numel():]


def pads_intact(pads):
    return all(bool((p == SENTINEL).all()) for p in pads)


def check_oracle(o, got, greedy, noise, tag):
    """actions rtol 1e-4 / atol 1e-5, values rel 1e-4 / abs 1e-5 against OraclePPO.predict of the device's own stacked state."""
    a, v, states = got
    a_o, v_o = o.predict(states, greedy=greedy, noise=None if greedy else noise)
    a_o, v_o = np.asarray(a_o).reshape(a.shape), np.asarray(v_o).reshape(v.shape)
    print("%s: actions max abs %.3e, values max abs %.3e" % (tag, np.abs(a - a_o).max(), np.abs(v - v_o).max()))
    assert np.allclose(a, a_o, rtol=1e-4, atol=1e-5), (tag, a, a_o)
    for e in range(len(v)):
        assert float(v[e]) == pytest.approx(float(v_o[e]), rel=1e-4, abs=1e-5), (tag, e)


def f32(states):
    x = np.asarray(states).astype(np.float32)
    assert np.array_equal(x.astype(np.float64), states)                              # the returned float64 state is the exact widening of fp32 values
    return x


# ------------------------------------------------------------------------------------------------------------------------------------ the kernel
def pad_outputs(s):
    """PAD sentinels behind the step's output buffer(s): h_out (pinned; out rows | older latents) and, with io = "device", d_out -> the pads."""
    import torch
    n = s.h_out.numel()
    big = torch.full((n + PAD,), SENTINEL, dtype=torch.float32).pin_memory()
    s.h_out = big[:n]
    s._out_np = s.h_out.numpy()[:s.num_envs * s.row].reshape(s.num_envs, s.row)
    s._older_np = s.h_out.numpy()[s.num_envs * s.row:]
    pads = [big[n:]]
    if s.d_out is not None:
        s.d_out, pad = padded(torch.full_like(s.d_out, SENTINEL))
        pads.append(pad)
    return pads


@pytest.mark.parametrize("io", ["pinned", "device"])
@pytest.mark.parametrize("n_act", [2, 3])
@pytest.mark.parametrize("z_dim,k,n_meas", lc.KERNEL_SHAPES, ids=["din%d" % lc.din_of(*s) for s in lc.KERNEL_SHAPES])
def test_kernel_sequence_sentinels_value_call_and_recording(world, z_dim, k, n_meas, n_act, io):
    import torch
    from rollout import ContinuousRolloutBuffer
    din = lc.din_of(z_dim, k, n_meas)
    o, m = world.pair(din, n_act)
    vae = world.vae(z_dim)
    E, T, LANES = 4, 7, 3                                                            # lane 3 is never named: its history, output rows and table rows are sentinels
    buf = ContinuousRolloutBuffer.stacked(vae, m, E, T, k, seed=3, io=io)
    s = buf._step
    assert (s.d_out is not None) == (io == "device")
    assert s.k == k and s.n_meas == n_meas and tuple(s.history.shape) == (E, k - 1, z_dim) and s.fresh.all() and tuple(buf.states.shape) == (E * (T + 1), din)
    rng = np.random.RandomState(100 + din + n_act)
    pads = []
    for name in ("states", "actions", "values", "final_values"):
        t, pad = padded(torch.full_like(getattr(buf, name), SENTINEL))
        setattr(buf, name, t)
        pads.append(pad)
    s.sstate, pad = padded(torch.full_like(s.sstate, SENTINEL))
    pads.append(pad)
    pads += pad_outputs(s)                                                           # eight sentinels behind the output region too

    def sequence(tag):
        """Six calls on three lanes from a known history -> the latents every call returned.  Every relation asserted is to the latents the calls themselves return."""
        known = np.random.RandomState(7).standard_normal((E, k - 1, z_dim)).astype(np.float32)
        known[3] = np.nan                                                            # the unnamed lane
        hist_t, hist_pad = padded(torch.from_numpy(known).to(s.device))
        s.history = hist_t
        s.fresh[:] = [False, True, False, True]                                      # lanes 0 and 2 continue from the known history, lane 1 starts an episode
        host = lc.HostStack(E, k, z_dim)
        host.hist, host.fresh = known.copy(), s.fresh.copy()
        for t in (buf.states, buf.actions, buf.values, buf.final_values):
            t.fill_(SENTINEL)
        seq_rng = np.random.RandomState(11)
        written = np.zeros(E * (T + 1), bool)
        latents = []
        plan = [([0, 1, 2], False, True), ([2, 0], False, True), ([0, 1, 2], False, True), ([1], False, False), ([0, 1, 2], True, True), ([2, 1, 0], False, True)]
        for c, (lanes, greedy, record) in enumerate(plan):
            lanes = np.array(lanes)
            n = len(lanes)
            if c == 2:                                                               # lane 0 restarts; what its history held must not reach the row and must be gone afterwards
                s.restart([0])
                host.restart([0])
                s.history[0].fill_(float("nan"))
                torch.cuda.synchronize()
            f, ms = world.frames(seq_rng, z_dim, n), measurements(seq_rng, n, n_meas)
            nz = seq_rng.standard_normal((n, n_act)).astype(np.float32)
            rows = (lanes * (T + 1) + c).astype(np.int32) if record else None
            before = [t.clone() for t in (buf.states, buf.actions, buf.values)]
            s.h_out.fill_(SENTINEL)                                                  # (io = "pinned": the kernels store straight into it)
            if s.d_out is not None:
                s.d_out.fill_(SENTINEL)
            s.sstate.fill_(SENTINEL)
            torch.cuda.synchronize()
            fresh_in = s.fresh[lanes].copy()
            got = s.record(*s.check(f, ms, greedy, nz), greedy, rows, buf.states, buf.actions, buf.values, None, lanes=lanes)
            a, v, states = got
            assert states.shape == (n, din) and states.dtype == np.float64 and a.shape == (n, n_act) and v.shape == (n,), (tag, c)
            st32 = f32(states)
            z_ret = st32[:, :z_dim]
            latents.append(z_ret)
            want = host.call(lanes, z_ret, ms)
            assert np.array_equal(st32.view(np.int32), want.view(np.int32)), (tag, c)                  # bitwise the host assembly, measurements included
            for e in range(n):
                if fresh_in[e]:                                                      # a first step repeats its own latent k times
                    assert np.array_equal(st32[e, :k * z_dim].reshape(k, z_dim), np.broadcast_to(z_ret[e], (k, z_dim))), (tag, c, e)
            assert np.isfinite(st32).all(), (tag, c)
            hist = s.history.cpu().numpy()
            assert np.array_equal(hist[:LANES].view(np.int32), host.hist[:LANES].view(np.int32)), (tag, c)
            assert np.isnan(hist[3]).all() and np.array_equal(hist[3].view(np.int32), known[3].view(np.int32)), (tag, c)     # the unnamed lane: NaN, where it was
            assert not s.fresh[lanes].any() and s.fresh[3]
            check_oracle(o, got, greedy, nz, "%s call %d" % (tag, c))
            # what the call recorded
            tabs = [t.cpu().numpy() for t in (buf.states, buf.actions, buf.values)]
            if record:
                assert np.array_equal(tabs[0][rows].view(np.int32), st32.view(np.int32)) and np.array_equal(tabs[1][rows], a) and np.array_equal(tabs[2][rows], v), (tag, c)
                written[rows] = True
            for now, was in zip(tabs, before):
                other = np.ones(len(now), bool)
                if record:
                    other[rows] = False
                assert np.array_equal(now[other], was.cpu().numpy()[other]), (tag, c)                  # table_rows NULL: nothing at all
            assert (tabs[2][~written] == np.float32(SENTINEL)).all() and (tabs[0][~written] == np.float32(SENTINEL)).all(), (tag, c)
            # behind what the call wrote: output rows >= n, the older latents of rows >= n, the sstate rows >= n, every pad
            assert (s._out_np[n:] == np.float32(SENTINEL)).all() and (s._older_np[n * (k - 1) * z_dim:] == np.float32(SENTINEL)).all(), (tag, c)
            if s.d_out is not None:                                                  # the device twin: rows >= n of both regions
                d = s.d_out.cpu().numpy()
                assert (d[n * s.row:s._older_off] == np.float32(SENTINEL)).all() and (d[s._older_off + n * (k - 1) * z_dim:] == np.float32(SENTINEL)).all(), (tag, c)
            assert bool((s.sstate[n:] == SENTINEL).all()) and pads_intact(pads + [hist_pad]), (tag, c)
            assert np.array_equal(s.sstate[:n].cpu().numpy().view(np.int32), want.view(np.int32)), (tag, c)
        return latents, host, hist_pad

    lat1, host, hist_pad = sequence("first")
    # ---- the bootstrap call and the value-only entry: nothing moves; the recording step's value for the same frame and history
    lanes = np.array([1, 2, 0])
    f, ms = world.frames(rng, z_dim, 3), measurements(rng, 3, n_meas)
    hist0, fresh0 = s.history.clone(), s.fresh.copy()
    rows = (lanes * (T + 1) + 6).astype(np.int32)
    boot = s.record(*s.check(f, ms, True, None), True, rows, buf.states, buf.actions, buf.values, None, lanes=lanes, advance=False)
    assert bitwise(s.history, hist0) and np.array_equal(s.fresh, fresh0)
    want = lc.stack_rows(host.hist, lanes, host.fresh[lanes], f32(boot[2])[:, :z_dim], ms)
    assert np.array_equal(f32(boot[2]).view(np.int32), want.view(np.int32))
    assert np.array_equal(buf.states.cpu().numpy()[rows].view(np.int32), want.view(np.int32)) and np.array_equal(buf.values.cpu().numpy()[rows], boot[1])
    check_oracle(o, boot, True, None, "bootstrap")
    fv_rows = (lanes * (T + 1) + 5).astype(np.int32)
    vv = s.record_value_lanes(*s.check(f, ms, True, None)[:3], fv_rows, buf.final_values, lanes)
    assert bitwise(s.history, hist0) and np.array_equal(s.fresh, fresh0)
    fv = buf.final_values.cpu().numpy()
    assert np.array_equal(fv[fv_rows], vv) and (np.delete(fv, fv_rows) == np.float32(SENTINEL)).all()
    stepped = s.record(*s.check(f, ms, True, None), True, None, lanes=lanes)
    assert not bitwise(s.history, hist0)
    print("value-only against the recording step: max |diff| %.3e; bootstrap: %.3e" % (np.abs(vv - stepped[1]).max(), np.abs(boot[1] - stepped[1]).max()))
    assert np.allclose(vv, stepped[1], rtol=1e-5, atol=1e-5) and np.allclose(boot[1], stepped[1], rtol=1e-5, atol=1e-5)
    v_o = np.asarray(o.predict(stepped[2], greedy=True)[1]).reshape(-1)
    for e in range(3):
        assert float(vv[e]) == pytest.approx(float(v_o[e]), rel=1e-4, abs=1e-5), e
    assert pads_intact(pads + [hist_pad])
    # ---- call to call: the same sequence again stands in the same relation to ITS returned latents (sequence() asserts that); the latents agree to 1e-5
    lat2, _, hist_pad2 = sequence("second")
    for x, y in zip(lat1, lat2):
        assert np.allclose(x, y, rtol=1e-5, atol=1e-5)
    assert pads_intact(pads + [hist_pad2])


@pytest.mark.parametrize("n_act", [2, 3])
@pytest.mark.parametrize("z_dim,k,n_meas", lc.KERNEL_SHAPES, ids=["din%d" % lc.din_of(*s) for s in lc.KERNEL_SHAPES])
def test_kernel_with_observation_normalisation(world, z_dim, k, n_meas, n_act):
    """Synthetic well-conditioned statistics: raw_states is bitwise the returned state, states within 1 fp32 ulp of normalize_observations(raw_states), actions and
    values within the oracle bounds of the oracle fed the NORMALISED device rows; the history still advances on the RAW latents.  The value-only entry with the
    statistics on leaves the history bitwise and is within 1e-5 of the recording step's value for the same frame and history.  Fresh statistics and clip = inf: the
    two tables are equal."""
    from rollout import ContinuousRolloutBuffer, normalize_observations
    din = lc.din_of(z_dim, k, n_meas)
    o, m = world.pair(din, n_act)
    E, T = 5, 4
    rng = np.random.RandomState(51 + din + n_act)
    buf = ContinuousRolloutBuffer.stacked(world.vae(z_dim), m, E, T, k, seed=3)
    buf.set_observation_normalization(clip=2.5, epsilon=1e-8)
    sd = buf.observation_normalization_state()
    assert sd["z_dim"] == k * z_dim
    buf.load_observation_normalization_state(dict(sd, count=100.0, mean=rng.uniform(-0.5, 0.5, din), m2=100.0 * rng.uniform(0.2, 4.0, din)))
    sd = buf.observation_normalization_state()
    host = lc.HostStack(E, k, z_dim)
    buf.reset()

    def check_step(t, f, ms, greedy):
        nz = rng.standard_normal((E, n_act)).astype(np.float32)
        a, v, states = buf.step(f, ms, greedy=greedy, noise=nz)
        buf.outcome(np.zeros(E), np.zeros(E, bool))
        st32 = f32(states)
        assert np.array_equal(st32.view(np.int32), host.call(np.arange(E), st32[:, :z_dim], ms).view(np.int32)), t
        rows = np.arange(E) * (T + 1) + t
        raw, nrm = buf.raw_states.cpu().numpy()[rows], buf.states.cpu().numpy()[rows]
        assert np.array_equal(raw.view(np.int32), st32.view(np.int32)), t
        want = normalize_observations(raw, sd)
        ulp = np.spacing(np.abs(want).astype(np.float32))
        assert (np.abs(nrm.astype(np.float64) - want.astype(np.float64)) <= ulp).all() and np.abs(nrm).max() <= np.float32(2.5), t
        assert np.array_equal(buf._step.sstate[:E].cpu().numpy().view(np.int32), nrm.view(np.int32)), t          # what trunk layer 1 read is what was recorded
        assert np.array_equal(buf.history.cpu().numpy().view(np.int32), host.hist.view(np.int32)), t
        assert np.array_equal(buf.actions.cpu().numpy()[rows], a) and np.array_equal(buf.values.cpu().numpy()[rows], v), t
        check_oracle(o, (a, v, nrm.astype(np.float64)), greedy, nz, "normalised din %d A %d step %d" % (din, n_act, t))
        return v

    for t in range(2):
        check_step(t, world.frames(rng, z_dim, E), measurements(rng, E, n_meas), t == 1)
    # the value-only entry with the statistics on: the history is read and never advanced
    f, ms = world.frames(rng, z_dim, E), measurements(rng, E, n_meas)
    s = buf._step
    hist0, fresh0, tabs0 = buf.history.clone(), s.fresh.copy(), [x.clone() for x in (buf.states, buf.raw_states, buf.actions, buf.values)]
    fv_rows = (np.arange(E) * (T + 1) + 1).astype(np.int32)
    vv = s.record_value_lanes(*s.check(f, ms, True, None)[:3], fv_rows, buf.final_values, np.arange(E))
    assert bitwise(buf.history, hist0) and np.array_equal(s.fresh, fresh0) and bitwise([buf.states, buf.raw_states, buf.actions, buf.values], tabs0)
    assert np.array_equal(buf.final_values.cpu().numpy()[fv_rows], vv)
    v_step = check_step(2, f, ms, True)
    print("normalised value-only against the recording step: max |diff| %.3e" % np.abs(vv - v_step).max())
    assert np.allclose(vv, v_step, rtol=1e-5, atol=1e-5)
    # fresh statistics and clip = inf: the identity
    buf2 = ContinuousRolloutBuffer.stacked(world.vae(z_dim), m, E, T, k, seed=3)
    buf2.set_observation_normalization(clip=float("inf"))
    buf2.reset()
    _, _, states2 = buf2.step(f, ms)
    rows = np.arange(E) * (T + 1)
    assert np.array_equal(buf2.states.cpu().numpy()[rows].view(np.int32), buf2.raw_states.cpu().numpy()[rows].view(np.int32))
    assert np.array_equal(buf2.raw_states.cpu().numpy()[rows].view(np.int32), f32(states2).view(np.int32))


def test_shape_refusals_through_the_c_abi_write_nothing(world):
    """k z_dim + n_meas != din (MI_ERR_SHAPE) on the MlpVAE chain, and din = 1028 > 1024 on the ConvVAE chain: the output buffer, the history and sstate keep their
    contents, and the good call goes through."""
    import torch
    from rollout import BatchedRolloutStep
    z_dim, k, n_meas = 8, 3, 5
    _, m = world.pair(lc.din_of(z_dim, k, n_meas))
    vae = world.vae(z_dim)
    step = BatchedRolloutStep.stacked(vae, m, 4, k, seed=3)
    rng = np.random.RandomState(95)
    f, ms = world.frames(rng, z_dim, 4), measurements(rng, 4, n_meas)
    step.step(f, ms, greedy=True)                                                     # fills the input buffer: lanes and flags behind the measurements and the noise
    L = step.L
    base = step.h_in.data_ptr()
    fptr = base + step._f_off
    iptr = fptr + 4 * 4 * (n_meas + step.A)
    good = dict(mlp_h=vae.dev.handle, ppo_h=m.dev.handle, stream=torch.cuda.current_stream().cuda_stream, frames_u8=base, measurements=fptr, n_meas=n_meas, noise=None, greedy=1,
                n=4, scratch=step.scratch.data_ptr(), scratch_bytes=step.scratch_bytes, out=step.h_out.data_ptr(), obs_mean=None, obs_inv_std=None, obs_clip=0.0, table_rows=None,
                n_table_rows=0, tab_states=None, tab_raw_states=None, tab_actions=None, tab_values=None, latent_stack=k, hist=step.history.data_ptr(), n_lanes=4, lanes=iptr,
                first=iptr + 16, advance=1, sstate=step.sstate.data_ptr(), older_out=step.h_out.data_ptr() + 4 * step._older_off)
    names = [a[1] for a in L.protos["mi_mlp_rollout_step_batch_stack"][1]]
    raw = lambda **kw: L.cdll.mi_mlp_rollout_step_batch_stack(*[dict(good, **kw)[key] for key in names])      # noqa: E731
    err = L.cdll.mi_last_error
    me = b"mi_mlp_rollout_step_batch_stack: "
    step.h_out.fill_(SENTINEL)
    step.sstate.fill_(SENTINEL)
    step.history.fill_(SENTINEL)
    hist0 = step.history.clone()
    for kw in (dict(n_meas=n_meas - 1), dict(n_meas=n_meas + 1), dict(latent_stack=k - 1), dict(latent_stack=k + 1)):
        assert raw(**kw) == -2 and err() == me + b"latent_stack x z_dim + measurements must equal the policy's input size", kw
    assert raw(latent_stack=1) == -1 and err() == me + b"2 <= latent_stack <= MI_ROLLOUT_MAX_STACK"
    torch.cuda.synchronize()
    assert (step.h_out.numpy() == np.float32(SENTINEL)).all() and bool((step.sstate == SENTINEL).all()) and bitwise(step.history, hist0)
    assert raw() == 0
    torch.cuda.synchronize()
    assert (step.h_out.numpy()[:4 * step.row] != np.float32(SENTINEL)).all() and not bitwise(step.history, hist0)
    # more than 1024 inputs: 16 latents of 64 and 4 measurements.  The Python classes refuse such a step, so the buffers come from a plain step on the same policy
    z_dim, k, n_meas = 64, 16, 4
    din = lc.din_of(z_dim, k, n_meas)
    _, m = world.pair(din)
    vae = world.vae(z_dim)
    plain = BatchedRolloutStep(vae, m, 2, seed=3)
    assert plain.n_meas == din - z_dim
    hist = torch.full((2, k - 1, z_dim), SENTINEL, device=plain.device)
    sstate = torch.full((2, din), SENTINEL, device=plain.device)
    ints = torch.zeros(4, dtype=torch.int32, device=plain.device)
    older = torch.full((2, (k - 1) * z_dim), SENTINEL, device=plain.device)
    plain.h_out.fill_(SENTINEL)
    base = plain.h_in.data_ptr()
    rc = L.cdll.mi_rollout_step_batch_stack(vae.dev.handle, m.dev.handle, torch.cuda.current_stream().cuda_stream, base, base + plain._f_off, n_meas, None, 1, 2, plain.scratch.data_ptr(),
                                            plain.scratch_bytes, plain.h_out.data_ptr(), None, None, 0.0, None, 0, None, None, None, None, k, hist.data_ptr(), 2, ints.data_ptr(),
                                            ints.data_ptr() + 8, 1, sstate.data_ptr(), older.data_ptr())
    assert rc == -2 and err() == b"mi_rollout_step_batch_stack: at most 1024 inputs"
    torch.cuda.synchronize()
    assert (plain.h_out.numpy() == np.float32(SENTINEL)).all() and all(bool((t == SENTINEL).all()) for t in (hist, sstate, older))


# ------------------------------------------------------------------------------------------------------------------------------------ the buffers
def collect(world, buf, host, rng, z_dim, n_meas, continuous, expected, feed=None):
    """One collection: every lane steps until its row is full (RolloutBuffer: or done); dones in mid-lane, and with `continuous` one truncation.  `expected` takes
    {table row: the host assembly of that row}; `host` advances with the latents the calls return.  feed: the observations of every lane's first step (the bootstrap
    observation of the collection before).  -> the bootstrap observations."""
    E, T = buf.num_envs, buf.horizon
    buf.reset()
    live, t = np.arange(E), 0
    while len(live):
        n = len(live)
        f, ms = world.frames(rng, z_dim, n), measurements(rng, n, n_meas)
        if t == 0 and feed is not None:
            f, ms = feed[0][live], feed[1][live]
        nz = rng.standard_normal((n, 2)).astype(np.float32)
        rows = buf.rows._base[live] + buf.rows.lengths[live]
        _, _, states = buf.step(f, ms, env_ids=live, noise=nz)
        st32 = f32(states)
        want = host.call(live, st32[:, :z_dim], ms)
        assert np.array_equal(st32.view(np.int32), want.view(np.int32)), t
        for r, w in zip(rows, want):
            expected[int(r)] = w
        # lane 1 ends an episode in mid-lane; lane 0 behind its last step but one -- the continuous buffer's at its very last step, which leaves that lane fresh
        dones = np.array([(e == 1 and t == 1) or (e == 0 and t == (T - 1 if continuous else T - 2)) for e in live])
        buf.outcome(rng.uniform(0, 1, n), dones, env_ids=live)
        host.restart(live[dones])
        if continuous and t == 2 and 2 in live:                                      # lane 2 is truncated behind its third step: valued on its history, then fresh
            fin = world.frames(rng, z_dim, 1), measurements(rng, 1, n_meas)
            hist0 = buf.history.clone()
            v = buf.truncate(fin[0], fin[1], env_ids=np.array([2]))
            assert bitwise(buf.history, hist0) and np.isfinite(v).all()
            host.restart([2])
        t += 1
        live = live[buf.lengths[live] < T] if continuous else live[~dones & (buf.lengths[live] < T)]
    need = buf.rows.needs_bootstrap() if continuous else buf.rows.stepped()
    f, ms = world.frames(rng, z_dim, E), measurements(rng, E, n_meas)
    if len(need):
        rows = buf.rows._base[need] + buf.rows.lengths[need]
        hist0, fresh0 = buf.history.clone(), buf._step.fresh.copy()
        _, _, states = buf.bootstrap(f[need], ms[need], env_ids=need)
        assert bitwise(buf.history, hist0) and np.array_equal(buf._step.fresh, fresh0)      # not advanced: the observation is stepped again
        st32 = f32(states)
        want = host.call(need, st32[:, :z_dim], ms[need], advance=False)
        assert np.array_equal(st32.view(np.int32), want.view(np.int32))
        for r, w in zip(rows, want):
            expected[int(r)] = w                                                     # the bootstrap slot holds the stacked row of the bootstrap observation
    assert np.array_equal(buf._step.fresh, host.fresh) and np.array_equal(buf.history.cpu().numpy().view(np.int32), host.hist.view(np.int32))
    return f, ms


def check_tables(buf, expected):
    tab = buf.states.cpu().numpy()
    for r, w in expected.items():
        assert np.array_equal(tab[r].view(np.int32), w.view(np.int32)), r


def twin_update(world, buf, m1, din, mode, epochs, batch, seed):
    """The host loop of the same device calls on a twin policy fed this buffer's tables (the pattern of test_s / test_y / test_zzzzz): parameters, Adam slots and
    theta_old bitwise."""
    import torch
    from ppo import ADAM_BETA1, ADAM_BETA2, ADAM_EPSILON, _adam_alpha
    _, m2 = world.pair(din)
    d = m2.dev
    m2.update_old_policy()
    valid = buf.rows.valid_rows()
    lp, mo = torch.zeros_like(buf.logp_old), None
    if mode == "kl":
        mo = torch.zeros(buf.n_table_rows, 2, device=buf.device)
        d.old_policy_cache(buf.states, buf.actions, buf.n_table_rows, lp, mo)
    else:
        d.logp_old(buf.states, buf.actions, buf.n_table_rows, lp)
    idx = torch.from_numpy(valid).to(buf.device).long()
    assert bitwise(lp[idx], buf.logp_old[idx])
    np.random.seed(seed)
    b1, b2 = np.float32(ADAM_BETA1), np.float32(ADAM_BETA2)
    for _ in range(epochs):
        order = np.arange(len(valid))
        np.random.shuffle(order)
        perm = torch.from_numpy(valid[order]).to(buf.device)
        for i in range(0, len(valid), batch):
            mb = perm[i:i + batch]
            n = int(mb.numel())
            tail = (mb, n, 1.0 / n, 1.0, _adam_alpha(m2.current_learning_rate(), b1, b2), ADAM_BETA1, ADAM_BETA2, ADAM_EPSILON)
            if mode == "kl":
                d.train_step_kl(None, buf.states, buf.actions, buf.returns, buf.advantages, lp, mo, 0.5, *tail)
            elif mode == "vclip":
                d.train_step_vclip(None, buf.states, buf.actions, buf.returns, buf.advantages, lp, buf.values, 0.2, *tail)
            else:
                d.train_step_idx(buf.states, buf.actions, buf.returns, buf.advantages, lp, *tail)
            b1, b2 = np.float32(b1 * np.float32(ADAM_BETA1)), np.float32(b2 * np.float32(ADAM_BETA2))
    assert bitwise(flat_state(m1), flat_state(m2)), mode
    assert not bitwise(m1.dev.params, m1.dev.params_old)


def run_buffer_case(world, continuous, E, T, k, z_dim, modes):
    from rollout import ContinuousRolloutBuffer, RolloutBuffer
    cls = ContinuousRolloutBuffer if continuous else RolloutBuffer
    n_meas, epochs, batch, seed = 3, 2, 8, 5
    din = lc.din_of(z_dim, k, n_meas)
    vae = world.vae(z_dim)
    for mode in modes:
        _, m1 = world.pair(din)
        if mode == "vclip":
            m1.set_value_clip(0.2)
        if mode == "kl":
            m1.set_kl_penalty(0.5)
        buf = cls.stacked(vae, m1, E, T, k, seed=3)
        host = lc.HostStack(E, k, z_dim)
        rng = np.random.RandomState(300 + E + k)
        expected = {}
        boot = collect(world, buf, host, rng, z_dim, n_meas, continuous, expected)
        check_tables(buf, expected)
        np.random.seed(seed)
        out = buf.update_with_diagnostics(num_epochs=epochs, batch_size=batch) if mode == "diag" else buf.update(num_epochs=epochs, batch_size=batch)
        assert len(out["losses"]) == epochs * -(-out["samples"] // batch) and all(np.isfinite(list(rec.values())).all() for rec in out["losses"])
        if mode == "diag":
            assert out["epochs_run"] == epochs
        if mode == "kl":
            assert out["kl_coef"] == 0.5 and np.isfinite(out["kl"]["kl"])
        check_tables(buf, expected)                                                  # the update reads the table and writes none of it
        twin_update(world, buf, m1, din, mode, epochs, batch, seed)
        if mode != "plain":
            continue
        # ---- the second collection: reset() keeps history and flags; the bootstrap observation is stepped again
        state = buf.history_state()
        host2 = copy.deepcopy(host)
        rng_state = rng.get_state()
        expected2 = {}
        collect(world, buf, host, rng, z_dim, n_meas, continuous, expected2, feed=boot)
        check_tables(buf, expected2)
        first_rows = buf.rows._base.astype(np.int64)
        carried = ~state["fresh"]
        assert carried.any() and (~carried).any()                                    # some lanes continue their episode, some start one
        tab = buf.states.cpu().numpy()[first_rows]
        for e in range(E):
            old = tab[e, z_dim:k * z_dim].reshape(k - 1, z_dim)
            src = state["history"][e] if carried[e] else np.broadcast_to(tab[e, :z_dim], (k - 1, z_dim))
            assert np.array_equal(old.view(np.int32), np.ascontiguousarray(src).view(np.int32)), e
        # ---- the state round trip into a fresh buffer: the same collection stands in the same relation to the carried history
        other = cls.stacked(vae, m1, E, T, k, seed=3)
        other.load_history_state(state)
        assert bitwise(other.history, buf._step.history.new_tensor(state["history"])) and np.array_equal(other._step.fresh, state["fresh"])
        rng.set_state(rng_state)
        expected3 = {}
        collect(world, other, host2, rng, z_dim, n_meas, continuous, expected3, feed=boot)
        check_tables(other, expected3)
        tab3 = other.states.cpu().numpy()[first_rows]
        assert np.array_equal(tab3[:, z_dim:k * z_dim][carried].view(np.int32), tab[:, z_dim:k * z_dim][carried].view(np.int32))
        assert np.allclose(tab3, tab, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("k", lc.BUFFER_STACKS)
@pytest.mark.parametrize("E,T", lc.BUFFER_SHAPES)
@pytest.mark.parametrize("continuous", [False, True], ids=["RolloutBuffer", "ContinuousRolloutBuffer"])
@pytest.mark.parametrize("mode", ["plain", "diag", "vclip", "kl"])
def test_buffers_on_the_mlp_encoder(world, continuous, E, T, k, mode):
    run_buffer_case(world, continuous, E, T, k, MLP_Z, [mode])


@pytest.mark.parametrize("continuous", [False, True], ids=["RolloutBuffer", "ContinuousRolloutBuffer"])
def test_buffers_on_the_conv_encoder(world, continuous):
    """(E, T) = (3, 5), k = 2: 131 inputs, the fused kernels' wide range."""
    run_buffer_case(world, continuous, 3, 5, 2, 64, ["plain"])


def test_buffer_observation_normalisation_merges_every_column(world):
    """update() merges din columns; normalize_latents=False leaves the first k z_dim columns at mean 0 / inv_std 1."""
    from rollout import ContinuousRolloutBuffer, observation_normalization_fp32, observation_normalization_state_checked
    E, T, k, z_dim, n_meas = 3, 5, 2, MLP_Z, 3
    din = lc.din_of(z_dim, k, n_meas)
    _, m = world.pair(din)
    buf = ContinuousRolloutBuffer.stacked(world.vae(z_dim), m, E, T, k, seed=3)
    buf.set_observation_normalization(clip=10.0, normalize_latents=False)
    host = lc.HostStack(E, k, z_dim)
    expected = {}
    collect(world, buf, host, np.random.RandomState(77), z_dim, n_meas, True, expected)
    raw = buf.raw_states.cpu().numpy()
    for r, w in expected.items():
        assert np.array_equal(raw[r].view(np.int32), w.view(np.int32)), r
    np.random.seed(5)
    out = buf.update(num_epochs=1, batch_size=8)
    rms = out["observation_rms"]
    valid = buf.rows.valid_rows()
    assert rms["count"] == len(valid) == E * T and rms["mean"].shape == (din,) and rms["var"].shape == (din,)
    assert np.allclose(rms["mean"], raw[valid].astype(np.float64).mean(axis=0), rtol=1e-9, atol=1e-12)
    assert np.allclose(rms["var"], raw[valid].astype(np.float64).var(axis=0), rtol=1e-9, atol=1e-12)
    sd = buf.observation_normalization_state()
    assert sd["z_dim"] == k * z_dim
    mean32, inv32 = buf._obs_norm["mean32"].cpu().numpy(), buf._obs_norm["inv32"].cpu().numpy()
    assert (mean32[:k * z_dim] == 0).all() and (inv32[:k * z_dim] == 1).all() and (mean32[k * z_dim:] != 0).all() and (inv32[k * z_dim:] != 1).all()
    want = observation_normalization_fp32(observation_normalization_state_checked(sd, din))
    assert np.array_equal(mean32, want[0]) and np.allclose(inv32, want[1], rtol=1e-6)
