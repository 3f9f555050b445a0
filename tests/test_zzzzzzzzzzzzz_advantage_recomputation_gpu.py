"""Advantage recomputation on the GPU: mi_ppo_values_idx (csrc/ppo_fused.hip, ppo_values_head_kernel) against float64 and against itself, PPO.values(), and
RolloutBuffer / ContinuousRolloutBuffer.set_advantage_recomputation against a host loop on a twin policy.

The value pass: the policies and row counts of tests/advantage_recomputation_cases.py, held to its bound (rel 1e-4 / abs 1e-5, the project's bound for values; the
fp32 twin of the reference stays inside it on the CPU: tests/test_advantage_recomputation_host.py) in both precision modes -- bf16x3 by the project's rule, the
larger of that bound and 4 x the fp32 mode's own distance, should the bound be exceeded (printed if it is).  Everything else here is bitwise.

The buffers: an update with the setting on is compared, bit for bit, with host_loop() -- the first finish call, the cache of log pi_old, and per epoch the refresh
(PpoDevice.values_idx, then the finish call on the refreshed table) and the policy's own minibatch step per shuffled minibatch -- driven on a twin policy from a copy
of the tables the device collected (two collections of the same frames need not agree in their last bit: the encoder's split-K sums are fp32 atomics)."""
import copy
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "carla-ppo_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import advantage_recomputation_cases as ac  # noqa: E402
from oracle import ppo_oracle as po  # noqa: E402
from oracle import vae_oracle as vo  # noqa: E402
from rollout_gpu_common import SENTINEL, bitwise, flat_state, make_pair  # noqa: E402

pytestmark = pytest.mark.gpu

PAD = 8
GAMMA, LAM = 0.99, 0.95


def padded(t, value=SENTINEL):
    import torch
    big = torch.full((t.numel() + PAD,), value, dtype=t.dtype, device=t.device)
    big[:t.numel()] = t.reshape(-1)
    return big[:t.numel()].view(t.shape), big[t.numel():]


def same_bits(x, y):
    return np.array_equal(np.asarray(x, np.float32).view(np.int32), np.asarray(y, np.float32).view(np.int32))


# ---------------------------------------------------------------------------------------------------------------------------------------- the value pass
_DEV = {}


def device(name, precision="fp32", max_batch=320):
    """The PpoDevice of policy `name` in this precision mode and at this max_batch, created once per module (theta_old = theta)."""
    from mi355.ppo_device import PpoDevice
    key = (name, precision, max_batch)
    if key not in _DEV:
        pol = ac.policy(name)
        d = PpoDevice(pol["input_dim"], pol["A"], pol["low"], pol["high"], ac.EPS, ac.VALUE_SCALE, ac.ENTROPY_SCALE, hidden=pol["hidden"], max_batch=max_batch,
                      precision=precision, wide_inputs=pol["wide"])
        d.load_params(pol["theta"], {k.replace("policy/", "policy_old/", 1): v for k, v in pol["theta"].items()})
        assert d.fused_ok()
        _DEV[key] = d
    return _DEV[key]


def run_values(d, s, rows=None, n_rows=None, out=None):
    """values_idx on host states -> (the out table with its PAD sentinels behind it, host).  rows: the table has n_rows rows of NaN and rows[i] holds s[i]."""
    import torch
    M = len(s)
    if rows is None:
        table, idx, n = torch.from_numpy(s).to(d.device), None, M
    else:
        n = n_rows
        host = np.full((n, s.shape[1]), np.nan, np.float32)
        host[rows] = s
        table, idx = torch.from_numpy(host).to(d.device), torch.from_numpy(np.asarray(rows, np.int32)).to(d.device)
    full = torch.full((n + PAD,), float("nan"), device=d.device)
    full[n:] = SENTINEL
    d.values_idx(table, idx, M, full[:n] if out is None else out)
    torch.cuda.synchronize()
    return full.cpu().numpy()


def row_list(M, seed=0):
    """M distinct rows, shuffled, of a table of 2 M + 3 rows."""
    n = 2 * M + 3
    return np.random.RandomState(50 + M + seed).permutation(n)[:M].astype(np.int32), n


_FP32_DISTANCE = {}


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("name", list(ac.POLICIES))
def test_values_against_float64(name, precision):
    """Contiguous, and through a row list into a larger table with NaN in every state row the list does not name; entries of the output no row names keep their NaN."""
    if precision == "bf16x3" and name not in _FP32_DISTANCE:
        test_values_against_float64(name, "fp32")
    d, pol, worst = device(name, precision), ac.policy(name), 0.0
    for M in ac.ROW_COUNTS:
        s = ac.states(name, M)
        ref = ac.value64(pol["theta"], s)
        got = run_values(d, s)
        assert np.all(got[M:] == SENTINEL)
        d_c = ac.distance(got[:M], ref)
        rows, n = row_list(M)
        tab = run_values(d, s, rows, n)
        assert np.all(tab[n:] == SENTINEL)
        other = np.ones(n, bool)
        other[rows] = False
        assert np.isnan(tab[:n][other]).all(), (name, M)
        d_l = ac.distance(tab[rows], ref)
        print("%s %s M=%d: contiguous %.3e, row list %.3e of the bound (max |v| %.3f)" % (name, precision, M, d_c, d_l, np.abs(ref).max()))
        worst = max(worst, d_c, d_l)
    limit = 1.0
    if precision == "fp32":
        _FP32_DISTANCE[name] = worst
    elif worst > 1.0:
        limit = max(1.0, 4.0 * _FP32_DISTANCE[name])
        print("%s bf16x3 exceeds rel 1e-4 / abs 1e-5 (%.3e of it): held to max(that, 4 x the fp32 mode's %.3e)" % (name, worst, _FP32_DISTANCE[name]))
    assert worst <= limit, (name, precision, worst, limit)


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("name", list(ac.POLICIES))
def test_values_are_bitwise_the_statistics_pass_and_themselves(name, precision):
    """value_out of mi_ppo_update_stats_idx on the same rows and parameters; the row-list form against the contiguous form on the gathered rows; two runs."""
    import torch
    from mi355.ppo_device import N_STATS
    d, pol = device(name, precision), ac.policy(name)
    for M in (5, 33, 257):
        s = ac.states(name, M, seed=1)
        rows, n = row_list(M, seed=1)
        tab = run_values(d, s, rows, n)
        again = run_values(d, s, rows, n)
        assert same_bits(tab[rows], again[rows]), (name, M, "two runs")
        assert same_bits(tab[rows], run_values(d, s)[:M]), (name, M, "row list against contiguous")
        host = np.zeros((n, pol["input_dim"]), np.float32)                           # (the statistics pass reads actions / returns / logp_old of the named rows)
        host[rows] = s
        dev = d.device
        v_out = torch.full((n,), float("nan"), device=dev)
        d.update_stats(torch.from_numpy(host).to(dev), torch.zeros(n, pol["A"], device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev),
                       torch.from_numpy(rows).to(dev), M, torch.zeros(N_STATS, dtype=torch.float64, device=dev),
                       torch.zeros(d.stats_scratch_doubles(M), dtype=torch.float64, device=dev), value_out=v_out)
        assert same_bits(tab[rows], v_out.cpu().numpy()[rows]), (name, precision, M, "value_out of update_stats")


@pytest.mark.parametrize("M", [64, 65, 200])
def test_the_chunk_loop(M):
    """An engine of max_batch = 64 against one of max_batch = 256 on the same rows: whole chunks, a partial last chunk, and the row list cut at chunk borders."""
    small, big = device("ref2", max_batch=64), device("ref2", max_batch=256)
    assert small.max_batch == 64 and big.max_batch == 256
    s = ac.states("ref2", M, seed=2)
    a, b = run_values(small, s), run_values(big, s)
    assert same_bits(a, b) and np.all(a[M:] == SENTINEL) and not np.isnan(a[:M]).any()
    rows, n = row_list(M, seed=2)
    a, b = run_values(small, s, rows, n), run_values(big, s, rows, n)
    assert same_bits(a[rows], b[rows]) and np.array_equal(np.isnan(a), np.isnan(b)) and np.isnan(a[:n]).sum() == n - M
    assert small.max_batch == 64                                                     # the engine was not grown


def test_skipped_rows_sentinels_and_what_is_not_written():
    import torch
    d, pol, M = device("small3"), ac.policy("small3"), 37
    dev = d.device
    s = ac.states("small3", M, seed=3)
    rows, n = row_list(M, seed=3)
    clean = run_values(d, s, rows, n)
    bad = rows.copy()
    bad[[0, 17, 36]] = (-1, n, n + 5)                                                # outside the table: nothing is stored for them, wherever the clamped load went
    d.grads.normal_()
    d.adam_m.normal_()
    d.adam_v.uniform_()
    d.losses.fill_(3.25)
    state = [t.clone() for t in (d.params, d.params_old, d.adam_m, d.adam_v, d.grads, d.losses)]
    host = np.full((n, pol["input_dim"]), np.nan, np.float32)
    host[rows] = s
    full = torch.full((n + PAD,), float("nan"), device=dev)
    full[n:] = SENTINEL
    d.values_idx(torch.from_numpy(host).to(dev), torch.from_numpy(bad).to(dev), M, full[:n])
    got = full.cpu().numpy()
    keep = np.ones(M, bool)
    keep[[0, 17, 36]] = False
    assert same_bits(got[rows[keep]], clean[rows[keep]])                             # the others are unaffected
    assert np.isnan(got[rows[~keep]]).all()                                          # the rows the bad entries replaced were never named
    assert np.isnan(got[:n]).sum() == n - keep.sum() and np.all(got[n:] == SENTINEL)
    assert bitwise([d.params, d.params_old, d.adam_m, d.adam_v, d.grads, d.losses], state)
    d.grads.zero_()
    d.adam_m.zero_()
    d.adam_v.zero_()


def test_a_refused_call_writes_nothing():
    import torch
    from mi355 import lib as milib
    from mi355.ppo_device import PpoDevice
    d, pol = device("small3"), ac.policy("small3")
    dev, p = d.device, milib.ptr
    table = torch.from_numpy(ac.states("small3", 8)).to(dev)
    out = torch.full((8 + PAD,), SENTINEL, device=dev)
    cdll = d.L.cdll
    for kw in (dict(M=0), dict(n_rows=0), dict(states=None), dict(out=None), dict(M=9)):
        a = dict(states=p(table), n_rows=8, M=8, out=p(out))
        a.update(kw)
        assert cdll.mi_ppo_values_idx(d.handle, None, a["states"], None, a["n_rows"], a["M"], a["out"]) == -1, kw
        assert cdll.mi_last_error().startswith(b"mi_ppo_values_idx: "), kw
    # an engine outside the fused range: MI_ERR_SHAPE, through the binding a MiError
    low, high = ac.bounds(3)
    off = PpoDevice(100, 3, low, high, ac.EPS, ac.VALUE_SCALE, ac.ENTROPY_SCALE, hidden=(64, 64), max_batch=32)
    assert not off.fused_ok()
    wide = torch.zeros(8, 100, device=dev)
    assert cdll.mi_ppo_values_idx(off.handle, None, p(wide), None, 8, 8, p(out)) == -2 and cdll.mi_last_error().startswith(b"mi_ppo_values_idx: needs the fused kernels")
    with pytest.raises(milib.MiError, match="needs the fused kernels"):
        off.values_idx(wide, None, 8, out[:8])
    off.close()
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


def test_ppo_values(tmp_path):
    """PPO.values() against predict(greedy=True)'s values, host and device states; on a policy outside the fused range it IS that call's value half."""
    import torch
    _, m = make_pair(tmp_path / "a")
    s = ac.states("ref2", 41, seed=4)
    _, v_ref = m.predict(s, greedy=True)
    v = m.values(s)
    assert v.dtype == np.float32 and v.shape == (41,)
    print("PPO.values against predict: max |difference| %.3e" % np.abs(v - v_ref).max())
    assert np.allclose(v, v_ref, rtol=1e-4, atol=1e-5)
    assert same_bits(m.values(torch.from_numpy(s).to(m.dev.device)), v)
    assert m.values(s[0]).shape == (1,) and same_bits(m.values(s[0]), m.values(s[:1]))
    mb = m.dev.max_batch
    big = np.tile(s, (mb // 41 + 2, 1))                                              # more rows than the engine's max_batch: the entry's own chunk loop
    assert len(big) > mb and same_bits(m.values(big)[:41], v) and m.dev.max_batch == mb
    _, w = make_pair(tmp_path / "b", input_dim=100)
    assert not w.dev.fused_ok()
    s = (0.5 * np.random.RandomState(3).standard_normal((9, 100))).astype(np.float32)
    assert same_bits(w.values(s), w.predict(s, greedy=True)[1])


# ---------------------------------------------------------------------------------------------------------------------------------------- the buffers
Z, K_MEAS, SRC = 16, 3, (4, 6, 3)


@pytest.fixture(scope="module")
def vae(tmp_path_factory):
    from vae.models import MlpVAE
    rng = np.random.RandomState(21)
    p = vo.init_mlp_vae_params(3, z_dim=Z, source_shape=SRC, target_shape=SRC, encoder_sizes=(36,), decoder_sizes=(8,))
    for k in p:
        if k.endswith("bias"):
            p[k] = (0.05 * rng.standard_normal(p[k].shape)).astype(np.float32)
    v = MlpVAE(np.array(SRC), encoder_sizes=(36,), decoder_sizes=(8,), z_dim=Z, model_dir=str(tmp_path_factory.mktemp("recompute_vae")), precision="fp32", training=False)
    v.set_weights(p)
    v.init_session(init_logging=False)
    return v


def env_inputs(rng, n):
    frames = rng.randint(0, 256, (n,) + SRC, dtype=np.uint8)
    meas = np.stack([rng.uniform(-1, 1, n), rng.uniform(0, 1, n), rng.uniform(0, 30, n)], axis=1)
    return frames, meas, rng.standard_normal((n, 2)).astype(np.float32)


def collect(buf, seed, continuous):
    """Ragged lanes: lane 2 takes T - 1 steps.  RolloutBuffer: lane 1 reports done at its step 1 and ends there.  ContinuousRolloutBuffer: lane 1 reports done at its
    step 1 and goes on, lane 0 is truncated at its step 2 (mid-lane), lane 2 at its last step (the lane's end: it needs no bootstrap)."""
    rng = np.random.RandomState(seed)
    E, T = buf.num_envs, buf.horizon
    buf.reset()
    for t in range(T):
        f, ms, nz = env_inputs(rng, E)
        ff, fms, _ = env_inputs(rng, E)
        live = np.array([e for e in range(E) if buf.rows.state[e] == buf.rows.OPEN and not (e == 2 and t >= T - 1)])
        buf.step(f[live], ms[live], env_ids=live, noise=nz[live])
        dones = np.zeros(E, bool)
        dones[1] = t == 1
        buf.outcome(rng.uniform(0, 1, E)[live], dones[live], env_ids=live)
        if continuous:
            cut = np.array([e for e, at in ((0, 2), (2, T - 2)) if at == t])
            if len(cut):
                buf.truncate(ff[cut], fms[cut], env_ids=cut)
    f, ms, _ = env_inputs(rng, E)
    need = buf.rows.needs_bootstrap() if continuous else buf.rows.stepped()
    buf.bootstrap(f[need], ms[need], env_ids=need)
    assert buf.lengths[2] == T - 1 and (continuous or buf.lengths[1] == 2)
    if continuous:
        assert buf.rows.truncs.sum() == 2 and buf.rows.truncs[0, 2] and buf.rows.truncs[2, T - 2] and 2 not in need
    return buf.rows.valid_rows()


def buffer_class(continuous):
    import rollout
    return rollout.ContinuousRolloutBuffer if continuous else rollout.RolloutBuffer


def make(vae, tmp, continuous, E, T, recompute, stack=1, pad=False, **hp):
    """-> (buffer, policy, the sentinels behind its new tables)."""
    import torch
    _, m = make_pair(tmp, input_dim=stack * Z + K_MEAS, **hp)
    assert m.dev.fused_ok()
    buf = buffer_class(continuous).stacked(vae, m, E, T, stack, seed=3)
    pads = []
    if recompute:
        buf.set_advantage_recomputation(True)
        if pad:
            buf.values_now, p = padded(torch.zeros(buf.n_table_rows, device=buf.device))
            pads.append(p)
            for attr in ("final_states", "_final_actions", "final_values_now") if continuous else ():
                t, p = padded(getattr(buf, attr))
                setattr(buf, attr, t)
                pads.append(p)
    return buf, m, pads


def copy_collection(src, dst):
    """dst's tables and book-keeping become src's, bit for bit."""
    for attr in ("states", "actions", "values", "final_values"):
        if getattr(src, attr, None) is not None:
            getattr(dst, attr).copy_(getattr(src, attr))
    dst.rows = copy.deepcopy(src.rows)


def refresh_rows(B, continuous):
    """The rows a refresh values: the recorded steps and the bootstrap slot of every non-empty lane whose last step neither reported done nor was truncated
    (RolloutBuffer: of every non-empty lane -- its finish call reads the slot under the terminal mask)."""
    lengths, T1 = B.rows.lengths, B.horizon + 1
    boot = [e * T1 + lengths[e] for e in range(B.num_envs) if lengths[e] > 0 and not (continuous and B.rows._last_done()[e])]
    return np.concatenate([B.rows.valid_rows(), np.asarray(boot, np.int32)]).astype(np.int32)


def finish_call(B, continuous, r, d, normalize="segment"):
    """-> finish(values table, final values table, f64 [3, E, T]): the buffer's finish call, spelled here."""
    import torch
    from mi355 import lib as milib
    E, T, dev, L = B.num_envs, B.horizon, B.device, B.L
    st = torch.cuda.current_stream(dev).cuda_stream
    if not continuous:
        ln = torch.from_numpy(B.rows.lengths.copy()).to(dev)
        return lambda v, fv, f64: L.mi_rollout_finish(st, v.data_ptr(), r.data_ptr(), d.data_ptr(), ln.data_ptr(), E, T, GAMMA, LAM, B.returns.data_ptr(),
                                                      B.advantages.data_ptr(), f64[0].data_ptr(), f64[1].data_ptr(), f64[2].data_ptr())
    segs = B.rows.segments()
    desc = torch.from_numpy(np.stack([segs[:, 0] * (T + 1) + segs[:, 1], segs[:, 2], B.rows.segment_truncated()]).astype(np.int32)).to(dev)
    assert B.rows.truncs.any()
    batch = normalize == "batch"
    scratch = torch.empty(int(L.mi_rollout_finish_segments_scratch_doubles(len(segs))), dtype=torch.float64, device=dev) if batch else None
    return lambda v, fv, f64: L.mi_rollout_finish_segments_boot(st, v.data_ptr(), r.data_ptr(), d.data_ptr(), desc[0].data_ptr(), desc[1].data_ptr(), len(segs), E, T,
                                                                GAMMA, LAM, 1 if batch else 0, milib.ptr(scratch), B.returns.data_ptr(), B.advantages.data_ptr(),
                                                                f64[0].data_ptr(), f64[1].data_ptr(), f64[2].data_ptr(), fv.data_ptr(), desc[2].data_ptr())


def host_loop(B, m, continuous, epochs, batch, final_states=None, vclip=False, klp=False, mbn=None, reward_scaling=False, v_old_is_values_now=False):
    """The update with a refresh, by hand on twin policy `m` from buffer B's tables (B has the setting off) -> dict(values_now, final_values_now, f64 of the first
    finish, f64 of the last refresh, recomputed)."""
    import rollout
    import torch
    E, T, dev, d, L = B.num_envs, B.horizon, B.device, m.dev, B.L
    st = torch.cuda.current_stream(dev).cuda_stream
    valid, lengths = B.rows.valid_rows(), B.rows.lengths.copy()
    n_valid = len(valid)
    nan3 = lambda: torch.full((3, E, T), float("nan"), dtype=torch.float64, device=dev)      # noqa: E731
    r, dn = torch.from_numpy(B.rows.rewards).to(dev), torch.from_numpy(B.rows.dones).to(dev)
    if reward_scaling:
        u = types.SimpleNamespace(clock=rollout._StageClock(None, dev), lengths=lengths, st=st)
        r = B._scale_rewards(u, B._reward_scaling, r, dn, GAMMA, B.rows.truncs.copy() if continuous else None)[1]
    finish = finish_call(B, continuous, r, dn)
    first = nan3()
    finish(B.values, getattr(B, "final_values", None), first)
    m.update_old_policy()
    lp = B._cache_logp_old(valid, klp)
    values_now = B.values.clone()
    fv_now = B.final_values.clone() if continuous else None
    rows = torch.from_numpy(refresh_rows(B, continuous)).to(dev)
    if continuous:
        e_t, t_t = np.nonzero(B.rows.truncs)
        trunc_rows = torch.from_numpy((e_t * (T + 1) + t_t).astype(np.int32)).to(dev)
    cur, last, recomputed = first, None, 0
    table = torch.zeros(B.n_table_rows, device=dev) if mbn is not None else None
    stats = torch.zeros(3 * -(-n_valid // batch), dtype=torch.float64, device=dev) if mbn is not None else None
    for epoch in range(epochs):
        if epoch > 0:
            d.values_idx(B.states, rows, int(rows.numel()), values_now)
            if continuous:
                d.values_idx(final_states, trunc_rows, int(trunc_rows.numel()), fv_now)
            last = nan3()
            finish(values_now, fv_now, last)
            cur, recomputed = last, recomputed + 1
        idx = np.arange(n_valid)
        np.random.shuffle(idx)
        perm = torch.from_numpy(valid[idx]).to(dev)
        adv = B.advantages
        if mbn is not None:
            L.mi_ppo_minibatch_advantages(st, cur[0].data_ptr(), perm.data_ptr(), n_valid, batch, E, T, mbn, table.data_ptr(), stats.data_ptr())
            adv = table
        v_old = (values_now if v_old_is_values_now else B.values) if vclip else None
        for i in range(0, n_valid, batch):
            mb = perm[i:i + batch]
            n = int(mb.numel())
            if klp:
                m._kl_step(B.states, B.actions, B.returns, adv, lp, B.mean_old, mb, n, n, old_values=v_old)
            else:
                m._step_rows(B.states, B.actions, B.returns, adv, lp, mb, n, n, **({} if v_old is None else {"old_values_all": v_old}))
            m.train_step_counter += 1
    torch.cuda.synchronize()
    return dict(values_now=values_now, final_values_now=fv_now, first=first.cpu().numpy(), last=None if last is None else last.cpu().numpy(), recomputed=recomputed)


def check_refreshed_against_the_oracle(buf, out, continuous):
    """refreshed_returns / refreshed_raw_advantages are, bitwise, oracle.ppo_oracle.compute_gae per lane / per segment fed refreshed_values, the refreshed bootstrap
    slot and, where truncated, refreshed_final_values -- the assertion of the existing buffer tests on the refreshed tables."""
    E, T = buf.num_envs, buf.horizon
    v_now = buf.values_now.view(E, T + 1).cpu().numpy()
    rec = np.arange(T)[None, :] < buf.rows.lengths[:, None]
    assert same_bits(out["refreshed_values"][rec], v_now[:, :T][rec]) and np.isnan(out["refreshed_values"][~rec]).all()
    segs = buf.rows.segments() if continuous else [(e, 0, int(buf.rows.lengths[e])) for e in range(E) if buf.rows.lengths[e] > 0]
    for e, first, n in segs:
        last, sl = first + n - 1, slice(first, first + n)
        done = buf.rows.dones[e, last] != 0
        if continuous and buf.rows.truncs[e, last]:
            boot = float(out["refreshed_final_values"][e, last])
        else:
            boot = 0.0 if (continuous and done) else float(v_now[e, first + n])
        raw = po.compute_gae(buf.rows.rewards[e, sl], out["refreshed_values"][e, sl].astype(np.float64), boot, buf.rows.dones[e, sl], GAMMA, LAM)
        ret, _ = po.returns_and_normalized_advantages(raw, out["refreshed_values"][e, sl].astype(np.float64))
        assert np.array_equal(out["refreshed_raw_advantages"][e, sl], raw) and np.array_equal(out["refreshed_returns"][e, sl], ret), (e, first, n)
    for k in ("refreshed_returns", "refreshed_advantages", "refreshed_raw_advantages"):
        assert out[k].dtype == np.float64 and np.isnan(out[k][~rec]).all() and not np.isnan(out[k][rec]).any(), k


SHAPES = [(3, 5, 4), (5, 20, 7)]                                                     # E, T, batch size (a partial last minibatch at both)
CLASSES = pytest.mark.parametrize("continuous", [False, True], ids=["RolloutBuffer", "ContinuousRolloutBuffer"])


@pytest.mark.parametrize("E,T,batch", SHAPES)
@CLASSES
def test_one_epoch_with_the_setting_on_is_the_setting_off(vae, tmp_path, continuous, E, T, batch):
    A, m_a, _ = make(vae, tmp_path / "a", continuous, E, T, True)
    C, m_c, _ = make(vae, tmp_path / "c", continuous, E, T, False)
    valid = collect(A, 71 + E, continuous)
    assert len(valid) % batch != 0
    copy_collection(A, C)
    np.random.seed(5)
    out_a = A.update(GAMMA, LAM, num_epochs=1, batch_size=batch)
    np.random.seed(5)
    out_c = C.update(GAMMA, LAM, num_epochs=1, batch_size=batch)
    assert bitwise(flat_state(m_a), flat_state(m_c)) and out_a["losses"] == out_c["losses"]
    for k in ("returns", "advantages", "raw_advantages", "values"):
        assert np.array_equal(out_a[k], out_c[k], equal_nan=True), k
    assert bitwise([A.returns, A.advantages], [C.returns, C.advantages])
    assert out_a["recomputed_epochs"] == 0 and "refreshed_values" not in out_a and "recomputed_epochs" not in out_c


@pytest.mark.parametrize("E,T,batch", SHAPES)
@CLASSES
def test_three_epochs_are_the_host_loop(vae, tmp_path, continuous, E, T, batch):
    import torch
    A, m_a, pads = make(vae, tmp_path / "a", continuous, E, T, True, pad=True)
    B, m_b, _ = make(vae, tmp_path / "b", continuous, E, T, False)
    C, m_c, _ = make(vae, tmp_path / "c", continuous, E, T, False)
    collect(A, 71 + E, continuous)
    copy_collection(A, B)
    copy_collection(A, C)
    times = {}
    np.random.seed(5)
    out = A.update(GAMMA, LAM, num_epochs=3, batch_size=batch, stage_times=times)
    np.random.seed(5)
    ref = host_loop(B, m_b, continuous, 3, batch, final_states=getattr(A, "final_states", None))
    assert bitwise(flat_state(m_a), flat_state(m_b))
    assert out["recomputed_epochs"] == 2 == ref["recomputed"] and times["recompute"] > 0
    assert bitwise(A.values_now, ref["values_now"]) and bitwise([A.returns, A.advantages], [B.returns, B.advantages])
    for i, k in enumerate(("raw_advantages", "returns", "advantages")):
        assert np.array_equal(out[k], ref["first"][i], equal_nan=True) and np.array_equal(out["refreshed_" + k], ref["last"][i], equal_nan=True), k
    if continuous:
        assert bitwise(A.final_values_now, ref["final_values_now"]) and np.array_equal(np.isnan(out["refreshed_final_values"]), ~A.rows.truncs)
    check_refreshed_against_the_oracle(A, out, continuous)
    # what stays from collection time: a twin with the setting off returns the same
    np.random.seed(5)
    out_c = C.update(GAMMA, LAM, num_epochs=3, batch_size=batch)
    for k in ("values", "returns", "raw_advantages", "advantages") + (("final_values",) if continuous else ()):
        assert np.array_equal(out[k], out_c[k], equal_nan=True), k
    assert bitwise(A.values, C.values) and not bitwise(flat_state(m_a)[0], flat_state(m_c)[0])      # ... and the refresh changed what was learnt
    assert not np.array_equal(out["refreshed_values"], out["values"], equal_nan=True)
    torch.cuda.synchronize()
    assert pads and all(bool((p == SENTINEL).all()) for p in pads)


SETTINGS = ["value_clip", "minibatch_norm", "reward_scaling", "observation_norm", "kl_penalty", "latent_stack"]


@pytest.mark.parametrize("setting", SETTINGS)
def test_other_settings_are_their_host_loop(vae, tmp_path, setting):
    E, T, batch = 3, 5, 4
    stack = 2 if setting == "latent_stack" else 1
    A, m_a, _ = make(vae, tmp_path / "a", False, E, T, True, stack=stack)
    B, m_b, _ = make(vae, tmp_path / "b", False, E, T, False, stack=stack)
    kw = {}
    for buf, m in ((A, m_a), (B, m_b)):
        if setting == "value_clip":
            m.set_value_clip(0.02)
            kw = dict(vclip=True)
        elif setting == "minibatch_norm":
            buf.set_minibatch_normalization(ddof=1)
            kw = dict(mbn=1)
        elif setting == "reward_scaling":
            buf.set_reward_scaling(clip=5.0)
            kw = dict(reward_scaling=True)
        elif setting == "kl_penalty":
            m.set_kl_penalty(0.5)
            kw = dict(klp=True)
    if setting == "observation_norm":
        A.set_observation_normalization(clip=5.0)                                    # (B reads A's tables: the normalised rows)
    collect(A, 31, False)
    copy_collection(A, B)
    np.random.seed(7)
    out = A.update(GAMMA, LAM, num_epochs=3, batch_size=batch)
    np.random.seed(7)
    ref = host_loop(B, m_b, False, 3, batch, **kw)
    assert out["recomputed_epochs"] == 2
    assert bitwise(flat_state(m_a), flat_state(m_b)), setting
    assert bitwise(A.values_now, ref["values_now"]) and np.array_equal(out["refreshed_returns"], ref["last"][1], equal_nan=True)
    if setting == "value_clip":                                                      # V_old is the collection-time table: a loop that clips around values_now learns something else
        X, m_x, _ = make(vae, tmp_path / "x", False, E, T, False)
        m_x.set_value_clip(0.02)
        copy_collection(A, X)
        np.random.seed(7)
        host_loop(X, m_x, False, 3, batch, vclip=True, v_old_is_values_now=True)
        assert not bitwise(flat_state(m_a)[0], flat_state(m_x)[0])


def test_the_kl_stop_ends_the_refreshes_with_the_epochs(vae, tmp_path):
    """update_with_diagnostics with a target_kl between the KL of epoch 1 and that of epoch 2, read from a run without a target on a third policy.  The KL has to grow
    from epoch 1 to epoch 2 for such a target to exist: at 1e-3 twelve samples overshoot in epoch 1 (measured 0.047, 0.044, 0.015), so the learning rates are
    tried from 1e-4 downwards and the first at which it grows is used (printed)."""
    E, T, batch = 3, 5, 4
    for lr in (1e-4, 3e-5, 1e-5):
        P, m_p, _ = make(vae, tmp_path / ("p%g" % lr), False, E, T, True, learning_rate=lr)
        A, m_a, _ = make(vae, tmp_path / ("a%g" % lr), False, E, T, True, learning_rate=lr)
        B, m_b, _ = make(vae, tmp_path / ("b%g" % lr), False, E, T, False, learning_rate=lr)
        collect(A, 31, False)
        copy_collection(A, P)
        copy_collection(A, B)
        np.random.seed(7)
        probe = P.update_with_diagnostics(GAMMA, LAM, num_epochs=3, batch_size=batch)    # the KL of every epoch, to put the target between epochs 1 and 2
        kl = [e["approx_kl"] for e in probe["epochs"]]
        print("learning rate %g: approx_kl per epoch %s" % (lr, kl))
        if kl[0] < kl[1]:
            break
    assert probe["recomputed_epochs"] == 2 and kl[0] < kl[1], kl
    np.random.seed(7)
    out = A.update_with_diagnostics(GAMMA, LAM, num_epochs=3, batch_size=batch, target_kl=0.5 * (kl[0] + kl[1]))
    assert out["stopped_early"] and out["epochs_run"] == 2 and out["recomputed_epochs"] == 1
    assert out["epochs"] == probe["epochs"][:2]
    np.random.seed(7)
    ref = host_loop(B, m_b, False, 2, batch)
    assert bitwise(flat_state(m_a), flat_state(m_b)) and bitwise(A.values_now, ref["values_now"])


def test_truncate_with_the_setting_on_keeps_the_state_row(vae, tmp_path):
    """The recording call's value is the value-only call's within 1e-5 (both end in fp32 atomics), and final_states holds, bitwise, the state that call returned."""
    E, T = 3, 5
    A, m_a, _ = make(vae, tmp_path / "a", True, E, T, True)
    C, m_c, _ = make(vae, tmp_path / "c", True, E, T, False)
    rng = np.random.RandomState(17)
    f, ms, nz = env_inputs(rng, E)
    ff, fms, _ = env_inputs(rng, E)
    seen = []
    record = A._step.record
    A._step.record = lambda *a, **k: seen.append(record(*a, **k)) or seen[-1]
    for buf in (A, C):
        buf.reset()
        buf.step(f, ms, noise=nz)
        buf.outcome(np.ones(E), np.zeros(E, bool))
    cut = np.array([0, 2])
    v_on, v_off = A.truncate(ff[cut], fms[cut], env_ids=cut), C.truncate(ff[cut], fms[cut], env_ids=cut)
    assert v_on.dtype == np.float32 and v_on.shape == (2,)
    print("truncate(): recording call against the value-only call, max |difference| %.3e" % np.abs(v_on - v_off).max())
    assert np.allclose(v_on, v_off, rtol=0, atol=1e-5)
    _, values, states = seen[-1]
    rows = cut * (T + 1)
    got = A.final_states.cpu().numpy()
    assert same_bits(got[rows, :Z], states[:, :Z].astype(np.float32)) and same_bits(got[rows, Z:], fms[cut].astype(np.float32))
    assert same_bits(A.final_values.cpu().numpy()[rows], v_on) and same_bits(values, v_on)
    other = np.ones(len(got), bool)
    other[rows] = False
    assert not got[other].any() and not A.states.cpu().numpy()[rows + 1].any()      # nothing else was written: the lanes' next slots are still empty
    assert C.final_states is None


@CLASSES
def test_switching_the_setting_off_again(vae, tmp_path, continuous):
    E, T, batch = 3, 5, 4
    A, m_a, _ = make(vae, tmp_path / "a", continuous, E, T, True)
    C, m_c, _ = make(vae, tmp_path / "c", continuous, E, T, False)
    A.set_advantage_recomputation(False)
    assert A.values_now is None and (not continuous or A.final_states is None)
    collect(A, 9, continuous)
    with pytest.raises(ValueError, match="steps are recorded"):
        A.set_advantage_recomputation(True)
    copy_collection(A, C)
    np.random.seed(3)
    out_a = A.update(GAMMA, LAM, num_epochs=3, batch_size=batch)
    np.random.seed(3)
    out_c = C.update(GAMMA, LAM, num_epochs=3, batch_size=batch)
    assert bitwise(flat_state(m_a), flat_state(m_c)) and out_a["losses"] == out_c["losses"] and sorted(out_a) == sorted(out_c)
    assert A.values_now is None
