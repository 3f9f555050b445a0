"""Truncation in continuous collection (rollout.ContinuousRolloutBuffer.truncate: an episode that stops without being terminal and is followed by a reset in the same
lane).  mi_rollout_finish_segments_boot against the dense GAE / normalisation kernels on each segment alone with [v_0 .. v_{L-1}, v_final] (bitwise), against
mi_rollout_finish_segments where no segment is truncated (bitwise), and what it must not read; mi_rollout_value_batch_rec against the greedy batched step on the same
frames; the whole loop against the oracle's GAE, the trainer's loop and the oracle's update.  Set-up and tolerances are rollout_gpu_common.py's; the criteria of the
normalize = 1 case and of the end-to-end case are test_n_rollout_segments_gpu.py's (its batch-normalisation bound and its PARAM_REL_MEASURED rule)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import ppo_oracle as po  # noqa: E402
from rollout_gpu_common import SENTINEL, check_losses, inputs, make_pair, make_world, rel_err, tables  # noqa: E402

GAMMA, LAM = 0.99, 0.95
# lanes as lists of (length, how the segment ends): "t" truncated, "d" done, "o" open (a lane's last segment: it bootstraps from the slot behind it)
LANES = {
    7: [[(1, "t"), (2, "t"), (3, "d"), (1, "o")],          # a truncated segment of one step; a truncated segment followed by another episode; a done; an open tail
        [(4, "d"), (3, "t")],                              # truncated at the lane's last slot
        [(2, "o")]],                                       # stopped early
    130: [[(130, "t")],                                    # the lane-strided loops pass 64 twice; truncated at the lane's last slot
          [(1, "t"), (64, "t"), (40, "d"), (25, "o")]],
}


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    return make_world(tmp_path_factory, "rollout_truncation", policy=False)


def make_case(T):
    lanes = LANES[T]
    E = len(lanes)
    rng = np.random.RandomState(900 + T)
    case = dict(E=E, T=T, values=rng.standard_normal((E, T + 1)).astype(np.float32), final=rng.standard_normal((E, T + 1)).astype(np.float32),
                rewards=rng.uniform(-1, 1, (E, T)), dones=np.zeros((E, T)), segs=[])
    for e, lane in enumerate(lanes):
        s = 0
        for n, kind in lane:
            case["segs"].append((e, s, n, kind))
            s += n
            if kind == "d":
                case["dones"][e, s - 1] = 1.0
        assert s <= T
    return case


@pytest.fixture(scope="module")
def cases():
    """Per T: the case and, computed once, the dense kernels' result on every segment alone."""
    out = {}
    for T in LANES:
        case = make_case(T)
        out[T] = (case, expected(case))
    return out


def expected(case):
    """Per segment (raw advantages, returns, normalised advantages) of mi_gae_scan + mi_adv_normalize on that segment alone: the value behind the last step is v_final
    for a truncated segment, 0.0 behind a done, else the table slot."""
    import utils
    out = []
    for e, s, n, kind in case["segs"]:
        v = case["values"][e, s:s + n + 1].astype(np.float64)
        if kind == "t":
            v[n] = float(case["final"][e, s + n - 1])
        elif kind == "d":
            v[n] = 0.0
        raw, ret, adv = utils.compute_gae_batched(case["rewards"][e, s:s + n][None], v[None], case["dones"][e, s:s + n][None], GAMMA, LAM, normalize=True)
        out.append((raw[0], ret[0], adv[0]))
    return out


def run(case, normalize=0, boot=True, flags=None, values=None, final=None, dones=None):
    """-> (fp32 returns [E, T + 1], fp32 advantages [E, T + 1], fp64 [3, E, T] = raw advantages, returns, normalised advantages); everything starts as SENTINEL.
    boot False: mi_rollout_finish_segments on the same buffers."""
    import torch
    from mi355 import lib as milib
    L = milib.get()
    E, T, dev = case["E"], case["T"], "cuda"
    segs = case["segs"]
    desc = np.array([[e * (T + 1) + s, n, kind == "t"] for e, s, n, kind in segs], np.int32).T.copy()
    if flags is not None:
        desc[2] = flags
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)      # noqa: E731
    v_d, f_d = up((case["values"] if values is None else values).reshape(-1)), up((case["final"] if final is None else final).reshape(-1))
    r_d, d_d, desc_d = up(case["rewards"]), up(case["dones"] if dones is None else dones), up(desc)
    n_seg = len(segs)
    ret32, adv32 = torch.full((E * (T + 1),), SENTINEL, device=dev), torch.full((E * (T + 1),), SENTINEL, device=dev)
    f64 = torch.full((3, E, T), SENTINEL, dtype=torch.float64, device=dev)
    scratch = torch.zeros(int(L.mi_rollout_finish_segments_scratch_doubles(n_seg)), dtype=torch.float64, device=dev) if normalize else None
    args = (torch.cuda.current_stream().cuda_stream, v_d.data_ptr(), r_d.data_ptr(), d_d.data_ptr(), desc_d[0].data_ptr(), desc_d[1].data_ptr(), n_seg, E, T, GAMMA, LAM,
            normalize, milib.ptr(scratch), ret32.data_ptr(), adv32.data_ptr(), f64[0].data_ptr(), f64[1].data_ptr(), f64[2].data_ptr())
    if boot:
        L.mi_rollout_finish_segments_boot(*args, f_d.data_ptr(), desc_d[2].data_ptr())
    else:
        L.mi_rollout_finish_segments(*args)
    torch.cuda.synchronize()
    return ret32.cpu().numpy().reshape(E, T + 1), adv32.cpu().numpy().reshape(E, T + 1), f64.cpu().numpy()


def check(case, got, want, normalize, tag, skip=()):
    """normalize 0: every segment is bitwise `want` (fp32 tables and the three fp64 arrays).  normalize 1: raw advantages and returns bitwise; the normalised
    advantages at test_n_rollout_segments_gpu.py::test_batch_normalisation's criterion (1e-12 max|A_norm| of numpy's fp64 statistics over the concatenation; the fp32
    table is the fp64 result rounded).  Slots of no segment keep the sentinel."""
    ret32, adv32, (raw, ret, advn) = got
    m = np.zeros((case["E"], case["T"] + 1), bool)
    for i, ((e, s, n, _), (w_raw, w_ret, w_adv)) in enumerate(zip(case["segs"], want)):
        m[e, s:s + n] = True
        if i in skip:
            continue
        assert np.array_equal(raw[e, s:s + n], w_raw) and np.array_equal(ret[e, s:s + n], w_ret), (tag, i, e, s, n)
        assert np.array_equal(ret32[e, s:s + n], w_ret.astype(np.float32)), (tag, i, e, s, n)
        if normalize == 0:
            assert np.array_equal(advn[e, s:s + n], w_adv) and np.array_equal(adv32[e, s:s + n], w_adv.astype(np.float32)), (tag, i, e, s, n)
    assert np.all(ret32[~m] == SENTINEL) and np.all(adv32[~m] == SENTINEL) and all(np.all(x[~m[:, :-1]] == SENTINEL) for x in (raw, ret, advn)), tag
    if normalize == 1 and not skip:
        a = np.concatenate([w[0] for w in want])
        ref = (a - a.mean()) / (a.std() + 1e-8)
        mine = np.concatenate([advn[e, s:s + n] for e, s, n, _ in case["segs"]])
        mine32 = np.concatenate([adv32[e, s:s + n] for e, s, n, _ in case["segs"]])
        err = np.abs(mine - ref).max()
        print("\n%s: batch-normalised advantages against numpy: max |diff| = %.3e (bound %.3e)" % (tag, err, 1e-12 * np.abs(ref).max()))
        assert err <= 1e-12 * np.abs(ref).max(), tag
        ref32 = ref.astype(np.float32)
        assert np.all(np.abs(mine32.astype(np.float64) - ref32.astype(np.float64)) <= np.spacing(np.abs(ref32)).astype(np.float64)), tag
        assert np.array_equal(mine32, mine.astype(np.float32)), tag


def same(x, y):
    return all(np.array_equal(p, q) for p, q in zip(x, y))


@pytest.mark.parametrize("T", sorted(LANES))
@pytest.mark.parametrize("normalize", [0, 1])
def test_finish_with_a_bootstrap_source_matches_the_dense_kernels_segment_by_segment(cases, T, normalize):
    case, want = cases[T]
    kinds = [k for _, _, _, k in case["segs"]]
    assert {"t", "d", "o"} <= set(kinds) and any(n == 1 and k == "t" for _, _, n, k in case["segs"])
    assert any(k == "t" and s + n == T for _, s, n, k in case["segs"]) and any(k == "t" and s + n < T for _, s, n, k in case["segs"])
    got = run(case, normalize)
    check(case, got, want, normalize, (T, normalize))
    assert same(run(case, normalize), got)                                            # two runs are bitwise equal
    # no flag set: the old entry, bit for bit (the truncated segments then read the slot behind them, like any open segment)
    zeros = np.zeros(len(case["segs"]), np.int32)
    assert same(run(case, normalize, flags=zeros), run(case, normalize, boot=False))
    assert not same(run(case, normalize, flags=zeros), got)


@pytest.mark.parametrize("T", sorted(LANES))
def test_what_a_truncated_segment_must_not_read(cases, T):
    """NaN in the tab_values slot behind every truncated segment and in tab_final_values at every row no flag points to.  A segment whose OWN first value is NaN comes
    out NaN by the definition of delta_0, and the slot behind a truncated segment that another episode follows IS that episode's first value: so, as in
    test_n_rollout_segments_gpu.py::test_slots_behind_a_done_are_not_read, the NaNs behind segments go in in two passes (behind the even and behind the odd truncated
    segments of each lane; a slot that starts no segment in both).  Every truncated segment has a NaN behind it in one pass, and every segment is compared, bitwise
    to the clean run's expectation and NaN-free, in a pass in which its own values are intact."""
    case, want = cases[T]
    final = np.full_like(case["final"], np.nan)
    for e, s, n, kind in case["segs"]:
        if kind == "t":
            final[e, s + n - 1] = case["final"][e, s + n - 1]
    starts = {(e, s) for e, s, _, _ in case["segs"]}
    seen, compared = set(), set()
    for normalize in (0, 1):
        for parity in (0, 1):
            values = case["values"].copy()
            k_in_lane, poisoned = {}, set()
            for i, (e, s, n, kind) in enumerate(case["segs"]):
                if kind != "t":
                    continue
                k = k_in_lane[e] = k_in_lane.get(e, -1) + 1
                if k % 2 == parity or (e, s + n) not in starts:
                    values[e, s + n] = np.nan
                    poisoned.add((e, s + n))
                    seen.add(i)
            skip = {i for i, (e, s, _, _) in enumerate(case["segs"]) if (e, s) in poisoned}
            got = run(case, normalize, values=values, final=final)
            if normalize == 0:
                check(case, got, want, 0, (T, parity), skip=skip)
            for i, (e, s, n, _) in enumerate(case["segs"]):
                if i in skip:
                    continue
                compared.add(i)
                w_raw, w_ret, _ = want[i]
                assert np.array_equal(got[2][0][e, s:s + n], w_raw) and np.array_equal(got[2][1][e, s:s + n], w_ret), (normalize, parity, i)
                if normalize == 0 or not skip:
                    for x in (got[0][e, s:s + n], got[1][e, s:s + n], got[2][2][e, s:s + n]):
                        assert np.isfinite(x).all(), (normalize, parity, i)
                else:                                                               # batch statistics take in the skipped (NaN) segments' advantages: returns only
                    assert np.isfinite(got[0][e, s:s + n]).all(), (normalize, parity, i)
    assert seen == {i for i, sg in enumerate(case["segs"]) if sg[3] == "t"} and compared == set(range(len(case["segs"])))
    # one truncated segment against the same data finished as a done: the last step's return differs by gamma v_final (fp64 rounding: 1e-9 absolute at values and
    # rewards of order 1), and the done never reads v_final either
    i, (e, s, n, _) = next((i, sg) for i, sg in enumerate(case["segs"]) if sg[3] == "t" and sg[2] > 1)
    dones = case["dones"].copy()
    dones[e, s + n - 1] = 1.0
    flags = np.array([k == "t" for _, _, _, k in case["segs"]], np.int32)
    flags[i] = 0
    last = s + n - 1
    final_as_done = final.copy()
    final_as_done[e, last] = np.nan
    as_done = run(case, 0, flags=flags, dones=dones, final=final_as_done)
    trunc = run(case, 0)
    v_final = float(case["final"][e, last])
    assert abs((trunc[2][1][e, last] - as_done[2][1][e, last]) - GAMMA * v_final) <= 1e-9
    assert np.isfinite(as_done[2][1][e, s:s + n]).all() and abs(GAMMA * v_final) > 1e-3


def collect_steps(buf, rng, n_steps=1):
    for _ in range(n_steps):
        f, ms, nz = inputs(rng, buf.num_envs)
        buf.step(f, ms, noise=nz)
        buf.outcome(rng.uniform(0, 1, buf.num_envs), np.zeros(buf.num_envs, bool))


@pytest.mark.parametrize("io", ["pinned", "device"])
def test_value_only_call_matches_the_greedy_step_and_records_at_the_right_rows(world, tmp_path, io):
    """truncate() at n = 1, 3 and num_envs = 4: the values are the greedy BatchedRolloutStep's on the same frames at test_l_rollout_batch_gpu.py's tolerance between two
    calls on the same frames (rtol = atol = 1e-5: the split-K layers end in fp32 atomics), they sit in buf.final_values at the rows of the lanes' last counted steps,
    bitwise what the call returned, and every other row of it is still zero; the step's own tables are not touched."""
    from rollout import BatchedRolloutStep, ContinuousRolloutBuffer
    E, T = 4, 4
    _, m = make_pair(tmp_path / "m")
    buf = ContinuousRolloutBuffer(world["vae"], m, E, T, io=io)
    step = BatchedRolloutStep(world["vae"], m, E, io=io)
    assert buf.final_values.shape == (E * (T + 1),) and str(buf.final_values.dtype) == "torch.float32" and not bool(buf.final_values.any())
    rng = np.random.RandomState(471)
    buf.reset()
    want = np.zeros(E * (T + 1), np.float32)
    for t, ids in enumerate(([2], [3, 0, 1], None)):
        collect_steps(buf, rng)
        n = E if ids is None else len(ids)
        f, ms, _ = inputs(rng, n)
        before = tables(buf)
        got = buf.truncate(f, ms, env_ids=None if ids is None else np.array(ids))
        assert got.shape == (n,) and got.dtype == np.float32, (io, n)
        _, v_step, _ = step(f, ms, greedy=True)
        print("\nio=%s n=%d: value-only call against the greedy step: max |diff| = %.3e" % (io, n, np.abs(got - v_step).max()))
        assert np.allclose(got, v_step, rtol=1e-5, atol=1e-5), (io, n, got, v_step)
        rows = np.array(range(E) if ids is None else ids) * (T + 1) + t
        want[rows] = got
        assert np.array_equal(buf.final_values.cpu().numpy(), want), (io, n)         # the right rows, bitwise; every other row still zero
        for now, was in zip(tables(buf), before):
            assert np.array_equal(now, was), (io, n)
        assert np.argwhere(buf.rows.truncs).tolist() == sorted([e, s] for s, grp in enumerate(([2], [3, 0, 1], range(E))[:t + 1]) for e in grp)
    # a row outside the table records nothing (the step's rule); the values still come back
    f, ms, _ = inputs(rng, 3)
    got = buf._step.record_value(f, 3, ms, np.array([-1, E * (T + 1), 2 ** 31 - 1], np.int32), buf.final_values)
    assert np.allclose(got, step(f, ms, greedy=True)[1], rtol=1e-5, atol=1e-5) and np.array_equal(buf.final_values.cpu().numpy(), want)
    # the argument errors that need real handles: MI_ERR_ARG with a message, nothing launched
    L, s = buf.L, buf._step
    base = s.h_in.data_ptr()
    good = dict(vae_h=buf.vae.dev.handle, ppo_h=buf.ppo.dev.handle, stream=None, frames_u8=base, measurements=base + s._f_off, n_meas=s.n_meas, n=2,
                scratch=s.scratch.data_ptr(), scratch_bytes=s.scratch_bytes, out=s.h_out.data_ptr(), table_rows=base + s._f_off + 4 * 2 * s.n_meas, n_table_rows=E * (T + 1),
                tab_final_values=buf.final_values.data_ptr())
    names = [a[1] for a in L.protos["mi_rollout_value_batch_rec"][1]]
    call = lambda **kw: L.cdll.mi_rollout_value_batch_rec(*[dict(good, **kw)[k] for k in names])      # noqa: E731
    assert call(scratch_bytes=16) == -1 and L.cdll.mi_last_error().startswith(b"mi_rollout_value_batch_rec: scratch too small")
    assert call(n_meas=s.n_meas + 1) == -2 and L.cdll.mi_last_error().startswith(b"mi_rollout_value_batch_rec: z_dim + measurements")
    assert np.array_equal(buf.final_values.cpu().numpy(), want)
    # the misuse the buffer refuses on the host: an awaiting lane, and a lane whose last step is already truncated
    with pytest.raises(ValueError, match="already truncated"):
        buf.truncate(f[:1], ms[:1], env_ids=np.array([0]))
    assert np.array_equal(buf.final_values.cpu().numpy(), want)


def test_collect_with_truncations_update_matches_the_oracle_and_the_trainers_loop(world, tmp_path):
    """E = 4, T = 8: lane 0 truncated mid-lane and bootstrapped at its end, lane 1 a done and a truncation at the lane's last slot, lane 2 two truncations back to back
    and a done in its last slot, lane 3 nothing but its bootstrap.  update()'s fp64 returns and raw advantages are, bitwise (the criterion of
    test_n_rollout_segments_gpu.py's end-to-end case), oracle.ppo_oracle.compute_gae per segment on the returned values / final_values / bootstrap_values and the rewards;
    the parameters after the update against the PPO.train_step loop on the same samples at that test's rule (value net bitwise, the others within 4 x its measured
    figure for normalize="segment")."""
    import utils
    from rollout import ContinuousRolloutBuffer
    from test_n_rollout_segments_gpu import PARAM_REL_MEASURED, VALUE_NET
    seed, epochs, batch = 5, 3, 8
    E, T = 4, 8
    o, m_a = make_pair(tmp_path / "a")
    _, m_b = make_pair(tmp_path / "b")
    buf = ContinuousRolloutBuffer(world["vae"], m_a, E, T)
    done_at, trunc_at = {1: (5,), 2: (8,)}, {0: (3,), 1: (8,), 2: (1, 2)}
    rng = np.random.RandomState(571)
    buf.reset()
    returned = {}
    for t in range(1, T + 1):
        f, ms, nz = inputs(rng, E)
        buf.step(f, ms, noise=nz)
        buf.outcome(rng.uniform(0, 1, E), np.array([t in done_at.get(e, ()) for e in range(E)]))
        cut = np.array([e for e in range(E) if t in trunc_at.get(e, ())], np.int64)
        if len(cut):
            f, ms, _ = inputs(rng, len(cut))                                          # the stopped episodes' final observations
            for e, v in zip(cut, buf.truncate(f, ms, env_ids=cut)):
                returned[(int(e), t - 1)] = v
    need = buf.rows.needs_bootstrap()
    assert need.tolist() == [0, 3]
    f, ms, _ = inputs(rng, E)
    buf.bootstrap(f[need], ms[need], env_ids=need)
    valid = buf.rows.valid_rows()
    segs = buf.rows.segments()
    assert segs.tolist() == [[0, 0, 3], [0, 3, 5], [1, 0, 5], [1, 5, 3], [2, 0, 1], [2, 1, 1], [2, 2, 6], [3, 0, 8]]
    s_tab, a_tab, _ = tables(buf)
    np.random.seed(seed)
    out = buf.update(GAMMA, LAM, num_epochs=epochs, batch_size=batch)
    n_steps = epochs * (E * T // batch)
    assert out["samples"] == E * T and len(out["losses"]) == n_steps and np.array_equal(out["segments"], segs)
    assert out["segment_truncated"].tolist() == [1, 0, 0, 1, 1, 1, 0, 0] and out["segment_truncated"].dtype == np.int32
    assert np.isnan(out["bootstrap_values"]).tolist() == [False, True, True, False] and out["bootstrap_values"].dtype == np.float32
    fv = out["final_values"]
    assert fv.shape == (E, T) and fv.dtype == np.float32 and np.argwhere(~np.isnan(fv)).tolist() == [[0, 2], [1, 7], [2, 0], [2, 1]]
    for (e, t), v in returned.items():
        assert fv[e, t] == v                                                          # what truncate() returned
    for k in ("returns", "advantages", "raw_advantages", "values"):
        assert np.isfinite(out[k]).all(), k
    # the float64 recomputation, per segment, by the oracle's GAE from what update() returned
    rets, advs = [], []
    for (e, first, n), tr in zip(segs, out["segment_truncated"]):
        last = first + n - 1
        done = buf.rows.dones[e, last] != 0
        boot = float(fv[e, last]) if tr else 0.0 if done else float(out["bootstrap_values"][e])
        assert tr or done or first + n == T
        sl = slice(first, first + n)
        raw_o = po.compute_gae(buf.rows.rewards[e, sl], out["values"][e, sl].astype(np.float64), boot, buf.rows.dones[e, sl], GAMMA, LAM)
        ret_o, _ = po.returns_and_normalized_advantages(raw_o, out["values"][e, sl].astype(np.float64))
        print("\nsegment (%d, %d, %d) truncated=%d: max |raw - oracle| = %.3e, max |returns - oracle| = %.3e"
              % (e, first, n, tr, np.abs(out["raw_advantages"][e, sl] - raw_o).max(), np.abs(out["returns"][e, sl] - ret_o).max()))
        assert np.array_equal(out["raw_advantages"][e, sl], raw_o) and np.array_equal(out["returns"][e, sl], ret_o), (e, first, n)
        # the trainer's own statements (the dense kernels) for route B's samples, bitwise the update's as well
        adv = utils.compute_gae(buf.rows.rewards[e, sl], out["values"][e, sl], boot, buf.rows.dones[e, sl], GAMMA, LAM)
        ret, advn = utils.normalize_advantages(adv, out["values"][e, sl])
        assert np.array_equal(out["returns"][e, sl], ret) and np.array_equal(out["advantages"][e, sl], advn), (e, first, n)
        rets.append(ret)
        advs.append(advn)
    ret, adv = np.concatenate(rets), np.concatenate(advs)
    assert np.array_equal(buf.returns.cpu().numpy()[valid], ret.astype(np.float32)) and np.array_equal(buf.advantages.cpu().numpy()[valid], adv.astype(np.float32))
    s, a = s_tab[valid], a_tab[valid]
    m_b.update_old_policy()
    np.random.seed(seed)
    logs_b = [m_b.train_step(s[mb], a[mb], ret[mb], adv[mb]) for mb in po.minibatch_schedule(len(valid), batch, epochs)]
    o.update_old_policy()
    np.random.seed(seed)
    logs_o = [o.train(s[mb], a[mb], ret[mb], adv[mb]) for mb in po.minibatch_schedule(len(valid), batch, epochs)]
    check_losses(out["losses"], logs_o, "A against O")
    check_losses(out["losses"], logs_b, "A against B")
    pa, pb = m_a.dev.export_params(), m_b.dev.export_params()
    worst = max(rel_err(pa[name], pb[name]) for name in pa)
    print("\nparameters after the update, truncating buffer against PPO.train_step loop: max |diff| / tensor max = %.3e" % worst)
    for name in pa:
        print("  %-34s %.3e" % (name, rel_err(pa[name], pb[name])))
    assert any(name.startswith(VALUE_NET) for name in pa)
    for name in pa:
        if name.startswith(VALUE_NET):
            assert np.array_equal(pa[name], pb[name]), name
    assert worst <= 4 * PARAM_REL_MEASURED["segment"], worst
    # a second collection WITHOUT truncation on the same buffer takes the old entry: nothing of the first one's truncations is left
    buf.reset()
    assert not buf.rows.truncs.any()
    collect_steps(buf, rng, T)
    f, ms, _ = inputs(rng, E)
    buf.bootstrap(f, ms)
    out2 = buf.update(GAMMA, LAM, num_epochs=0)
    assert not out2["segment_truncated"].any() and np.isnan(out2["final_values"]).all() and out2["segments"].tolist() == [[e, 0, T] for e in range(E)]
