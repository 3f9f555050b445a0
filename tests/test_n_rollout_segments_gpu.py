"""Continuous collection (rollout.ContinuousRolloutBuffer: lanes that go on after a done; mi_rollout_finish_segments finishes them segment by segment) against the
dense GAE / normalisation kernels on each segment alone (bitwise), mi_rollout_finish where the two overlap (bitwise), numpy for the batch normalisation, the existing
RolloutBuffer on a collection both can hold (bitwise), the trainer's loop built from existing pieces and the oracle.  Set-up restated from
test_m_rollout_buffer_gpu.py (make_pair, vae_params, make_vae, inputs, tables, check_recorded, check_losses); tolerances are that file's for the update's losses
(test_e_c5_replay_gpu.py's)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import ppo_oracle as po  # noqa: E402
from rollout_gpu_common import SENTINEL, Z, check_losses, check_recorded, fill_tables, inputs, make_pair, make_world, rel_err, tables  # noqa: E402

GAMMA, LAM = 0.99, 0.95


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    return make_world(tmp_path_factory, "rollout_segments", policy=False)


# ---- the kernel ----------------------------------------------------------------------------------------------------------------------------------------------------

def layout(T):
    """Lanes as lists of (segment length, ends in a done): one segment per lane at test_m_rollout_buffer_gpu.py's lengths (a terminal at the end of every other one);
    lanes cut into segments of 1, 2, 3, 63, 64, 65 steps (those below T, over as many lanes as they take) and a remainder that ends at the horizon without a done; the same
    lanes with a done in their last slot; a lane stopped early behind a done; an empty lane."""
    lanes = [[(x, e % 2 == 0)] if x else [] for e, x in enumerate(x for x in (1, 2, 63, 64, 65, T, 0, T - 1, 3, 0, T, 1) if x <= T)]
    packed, cuts, used = [], [], 0                                                    # the cuts that fit in front of a remainder, in as many lanes as that takes
    for n in (1, 2, 3, 63, 64, 65):
        if n >= T:
            continue
        if used + n >= T:
            packed.append((cuts, used))
            cuts, used = [], 0
        cuts, used = cuts + [(n, True)], used + n
    packed.append((cuts, used))
    for cuts, used in packed:
        lanes.append(cuts + [(T - used, False)])
        lanes.append(cuts + [(T - used, True)])                                       # the lane's last slot is a done
    lanes.append([(1, True), (min(2, T - 2), False)])                                 # stopped early: T - 1 steps at most
    lanes.append([])
    return lanes


def make_case(T, seed, lanes=None):
    lanes = layout(T) if lanes is None else lanes
    E = len(lanes)
    rng = np.random.RandomState(seed)
    values = rng.standard_normal((E, T + 1)).astype(np.float32)
    rewards = rng.uniform(-1, 1, (E, T))
    dones = np.zeros((E, T))
    segs = []                                                                          # (lane, first slot, length, ends in a done)
    for e, lane in enumerate(lanes):
        s = 0
        for n, done in lane:
            segs.append((e, s, n, done))
            s += n
            if done:
                dones[e, s - 1] = 1.0
        assert s <= T
    return dict(E=E, T=T, values=values, rewards=rewards, dones=dones, segs=segs)


def descriptors(case):
    T = case["T"]
    return np.array([[e * (T + 1) + s, n] for e, s, n, _ in case["segs"]], np.int32).reshape(-1, 2)


def run_segments(case, desc=None, normalize=0, optional=True, values=None, alloc_lanes=None):
    """-> (fp32 returns [lanes, T + 1], fp32 advantages [lanes, T + 1], fp64 [3, lanes, T] = raw advantages, returns, normalised advantages or None); everything starts as
    SENTINEL.  alloc_lanes > E: tables and arrays larger than the num_envs the call is given."""
    import torch
    from mi355 import lib as milib
    L = milib.get()
    E, T = case["E"], case["T"]
    lanes = alloc_lanes or E
    desc = descriptors(case) if desc is None else np.asarray(desc, np.int32).reshape(-1, 2)
    pad = lambda x, fill: np.concatenate([x, np.full((lanes - E,) + x.shape[1:], fill, x.dtype)])      # noqa: E731
    dev = "cuda"
    v_d = torch.from_numpy(pad(case["values"] if values is None else values, 0).reshape(-1)).to(dev)
    r_d, d_d = torch.from_numpy(pad(case["rewards"], 0)).to(dev), torch.from_numpy(pad(case["dones"], 0)).to(dev)
    row_d, len_d = torch.from_numpy(desc[:, 0].copy()).to(dev), torch.from_numpy(desc[:, 1].copy()).to(dev)
    n_seg = len(desc)
    ret32, adv32 = torch.full((lanes * (T + 1),), SENTINEL, device=dev), torch.full((lanes * (T + 1),), SENTINEL, device=dev)
    f64 = torch.full((3, lanes, T), SENTINEL, dtype=torch.float64, device=dev)
    scratch = torch.zeros(int(L.mi_rollout_finish_segments_scratch_doubles(n_seg)), dtype=torch.float64, device=dev) if normalize else None
    st = torch.cuda.current_stream().cuda_stream
    L.mi_rollout_finish_segments(st, v_d.data_ptr(), r_d.data_ptr(), d_d.data_ptr(), row_d.data_ptr(), len_d.data_ptr(), n_seg, E, T, GAMMA, LAM, normalize,
                                 milib.ptr(scratch), ret32.data_ptr(), adv32.data_ptr(), f64[0].data_ptr() if optional or normalize else None,
                                 f64[1].data_ptr() if optional else None, f64[2].data_ptr() if optional else None)
    torch.cuda.synchronize()
    return ret32.cpu().numpy().reshape(lanes, T + 1), adv32.cpu().numpy().reshape(lanes, T + 1), f64.cpu().numpy()


def expected(case):
    """Per segment (raw advantages, returns, normalised advantages) of the dense kernels on that segment alone: the bootstrap value is 0.0 behind a done, else the table slot."""
    import utils
    out = []
    for e, s, n, done in case["segs"]:
        v = case["values"][e, s:s + n + 1].astype(np.float64)                         # (a slot behind the lane's last step exists: the table has T + 1)
        if done:
            v[n] = 0.0
        raw, ret, adv = utils.compute_gae_batched(case["rewards"][e, s:s + n][None], v[None], case["dones"][e, s:s + n][None], GAMMA, LAM, normalize=True)
        out.append((raw[0], ret[0], adv[0]))
    return out


def check_segments(case, got, want, tag, skip=()):
    """Every segment is bitwise `want`; slots of no segment (and of the segments in `skip`) are not looked at here."""
    ret32, adv32, (raw, ret, advn) = got
    for i, ((e, s, n, _), (w_raw, w_ret, w_adv)) in enumerate(zip(case["segs"], want)):
        if i in skip:
            continue
        assert np.array_equal(raw[e, s:s + n], w_raw), (tag, i, e, s, n)
        assert np.array_equal(ret[e, s:s + n], w_ret), (tag, i, e, s, n)
        assert np.array_equal(advn[e, s:s + n], w_adv), (tag, i, e, s, n)
        assert np.array_equal(ret32[e, s:s + n], w_ret.astype(np.float32)) and np.array_equal(adv32[e, s:s + n], w_adv.astype(np.float32)), (tag, i, e, s, n)


def covered(case, lanes=None):
    m = np.zeros((lanes or case["E"], case["T"] + 1), bool)
    for e, s, n, _ in case["segs"]:
        m[e, s:s + n] = True
    return m


def check_untouched(case, got, tag):
    ret32, adv32, f64 = got
    m = covered(case, ret32.shape[0])
    assert np.all(ret32[~m] == SENTINEL) and np.all(adv32[~m] == SENTINEL), tag
    for x in f64:
        assert np.all(x[~m[:, :-1]] == SENTINEL), tag


def same(x, y):
    return np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and np.array_equal(x[2], y[2])


@pytest.mark.parametrize("T", [4, 128, 1024])
def test_segment_kernel_matches_the_dense_kernels_segment_by_segment(T):
    case = make_case(T, 160 + T)
    assert any(len(lane) > 2 for lane in layout(T)) and sum(n for _, _, n, _ in case["segs"]) > 2 * T
    want = expected(case)
    got = run_segments(case)
    check_segments(case, got, want, T)
    check_untouched(case, got, T)                                                     # slots of no segment keep the sentinel
    for (e, s, n, _), (_, _, w_adv) in zip(case["segs"], want):
        if n == 1:
            assert got[2][2][e, s] == 0.0                                            # std 0: (A - mean) / (0 + 1e-8) = 0
    assert same(run_segments(case), got)                                              # two runs are bitwise equal
    bare = run_segments(case, optional=False)                                         # without the optional outputs the tables come out the same
    assert np.array_equal(bare[0], got[0]) and np.array_equal(bare[1], got[1]) and np.all(bare[2] == SENTINEL)


def test_slots_behind_a_done_are_not_read():
    """NaN in the slot behind a done-ended segment -- the next segment's first value, or the lane's bootstrap slot -- changes nothing in that segment.  A segment whose
    OWN first value is NaN comes out NaN by the definition of delta_0, so the NaNs go in in two passes (behind the even and behind the odd done-ended segments of each
    lane): every done-ended segment has a NaN behind it in one pass, and every segment is compared, bitwise and NaN-free, in a pass in which its own values are intact."""
    T = 128
    case = make_case(T, 77)
    want = expected(case)                                                             # from the intact values
    clean = run_segments(case)
    check_segments(case, clean, want, "clean")
    seen_nan_behind, compared = set(), set()
    for parity in (0, 1):
        values = case["values"].copy()
        k_in_lane, poisoned_rows = {}, set()
        for i, (e, s, n, done) in enumerate(case["segs"]):
            if not done:
                continue
            k = k_in_lane[e] = k_in_lane.get(e, -1) + 1
            if k % 2 == parity or s + n == T:                                         # the lane's bootstrap slot starts no segment: in both passes
                values[e, s + n] = np.nan
                poisoned_rows.add((e, s + n))
                seen_nan_behind.add(i)
        skip = {i for i, (e, s, n, _) in enumerate(case["segs"]) if (e, s) in poisoned_rows}
        got = run_segments(case, values=values)
        check_segments(case, got, want, ("pass", parity), skip=skip)
        for i, (e, s, n, _) in enumerate(case["segs"]):
            if i not in skip:
                compared.add(i)
                for x in (got[0][e, s:s + n], got[1][e, s:s + n], got[2][0][e, s:s + n], got[2][1][e, s:s + n], got[2][2][e, s:s + n]):
                    assert not np.isnan(x).any(), (parity, i)
        check_untouched(case, got, ("pass", parity))
    assert seen_nan_behind == {i for i, sg in enumerate(case["segs"]) if sg[3]} and compared == set(range(len(case["segs"])))


def test_one_segment_per_lane_equals_the_dense_finish():
    """Lanes that do not end in a done, and lanes that do with 0.0 in their bootstrap slot: mi_rollout_finish_segments is mi_rollout_finish, bitwise."""
    import torch
    from mi355 import lib as milib
    L = milib.get()
    T = 128
    lengths = np.array([1, 2, 63, 64, 65, T, 0, T - 1, 3, 0, T, 1], np.int32)
    case = make_case(T, 88, [[(int(x), e % 2 == 0)] if x else [] for e, x in enumerate(lengths)])
    E = case["E"]
    for e, s, n, done in case["segs"]:
        if done:
            case["values"][e, n] = 0.0
    got = run_segments(case)
    dev = "cuda"
    v_d, r_d, d_d, l_d = (torch.from_numpy(x).to(dev) for x in (case["values"].reshape(-1), case["rewards"], case["dones"], lengths))
    ret32, adv32 = torch.full((E * (T + 1),), SENTINEL, device=dev), torch.full((E * (T + 1),), SENTINEL, device=dev)
    f64 = torch.full((3, E, T), SENTINEL, dtype=torch.float64, device=dev)
    L.mi_rollout_finish(torch.cuda.current_stream().cuda_stream, v_d.data_ptr(), r_d.data_ptr(), d_d.data_ptr(), l_d.data_ptr(), E, T, GAMMA, LAM, ret32.data_ptr(),
                        adv32.data_ptr(), f64[0].data_ptr(), f64[1].data_ptr(), f64[2].data_ptr())
    assert same(got, (ret32.cpu().numpy().reshape(E, T + 1), adv32.cpu().numpy().reshape(E, T + 1), f64.cpu().numpy()))
    assert np.isfinite(got[2][2][covered(case)[:, :-1]]).all()


def test_bad_descriptors_are_not_executed():
    """Length 0, a negative length, a first slot plus length beyond T, a lane >= num_envs and a row number in a bootstrap slot leave every output at its sentinel; the good
    descriptors of the same call come out right.  Cannot fault: every pointer is valid and the tables hold two lanes more than the num_envs the call is given, so even a
    descriptor that were executed would stay inside them."""
    T = 16
    lanes = [[(5, True), (11, False)], [(16, True)], [(3, False)], [], [], [], []]     # lanes 3 .. 6 take the bad descriptors
    case = make_case(T, 99, lanes)
    E = case["E"]
    want = expected(case)
    T1 = T + 1
    bad = [[3 * T1 + 2, 0], [3 * T1 + 4, -3], [3 * T1 + 6, -2 ** 31], [4 * T1 + 14, 5], [4 * T1 + 0, T + 1], [5 * T1 + 1, T], [E * T1 + 3, 4], [(E + 1) * T1, 1],
           [5 * T1 + T, 1], [3 * T1 + T, 2]]
    good = descriptors(case)
    for normalize in (0, 1):
        for order in (np.concatenate([good, bad]), np.concatenate([bad, good]), np.concatenate([bad[:5], good[:2], bad[5:], good[2:]])):
            got = run_segments(case, desc=order, normalize=normalize, alloc_lanes=E + 2)
            check_untouched(case, got, (normalize, len(order)))                       # lanes 3 .. E + 1 and every uncovered slot of lanes 0 .. 2
            if normalize == 0:
                check_segments(case, got, want, "good among bad")
            else:
                for (e, s, n, _), (w_raw, w_ret, _) in zip(case["segs"], want):
                    assert np.array_equal(got[2][0][e, s:s + n], w_raw) and np.array_equal(got[2][1][e, s:s + n], w_ret), (e, s, n)
                a = np.concatenate([w[0] for w in want])                             # the bad ones add nothing to the sums or to the count: test_batch_normalisation's bound
                ref = (a - a.mean()) / (a.std() + 1e-8)
                mine = np.concatenate([got[2][2][e, s:s + n] for e, s, n, _ in case["segs"]])
                assert np.abs(mine - ref).max() <= 1e-12 * np.abs(ref).max()
    only_bad = run_segments(case, desc=bad, alloc_lanes=E + 2)
    assert all(np.all(x == SENTINEL) for x in (only_bad[0], only_bad[1], only_bad[2]))
    only_bad = run_segments(case, desc=bad, normalize=1, alloc_lanes=E + 2)
    assert all(np.all(x == SENTINEL) for x in (only_bad[0], only_bad[1], only_bad[2]))


@pytest.mark.parametrize("T", [4, 128, 1024])
def test_batch_normalisation(T):
    """normalize = 1: raw advantages and returns as with normalize = 0; the normalised advantages within 1e-12 max|A_norm| (n eps for n = 8192 steps; a CPU emulation of
    the lane-strided, butterfly, segment-order sum stayed below 5e-16 on 20 random cases) of numpy's fp64 statistics over the concatenation; fp32 table within 1 ulp."""
    case = make_case(T, 260 + T)
    total = sum(n for _, _, n, _ in case["segs"])
    assert 8 <= total <= 8192
    want = expected(case)
    got = run_segments(case, normalize=1)
    ret32, adv32, (raw, ret, advn) = got
    for (e, s, n, _), (w_raw, w_ret, _) in zip(case["segs"], want):
        assert np.array_equal(raw[e, s:s + n], w_raw) and np.array_equal(ret[e, s:s + n], w_ret) and np.array_equal(ret32[e, s:s + n], w_ret.astype(np.float32)), (e, s, n)
    check_untouched(case, got, T)
    a = np.concatenate([w[0] for w in want])
    assert a.std() > 0.1                                                              # rewards from uniform(-1, 1): far from 0
    ref = (a - a.mean()) / (a.std() + 1e-8)
    mine = np.concatenate([advn[e, s:s + n] for e, s, n, _ in case["segs"]])
    mine32 = np.concatenate([adv32[e, s:s + n] for e, s, n, _ in case["segs"]])
    err = np.abs(mine - ref).max()
    print("\nT = %d, %d steps in %d segments: max |A_norm - numpy| = %.3e (bound %.3e)" % (T, total, len(case["segs"]), err, 1e-12 * np.abs(ref).max()))
    assert err <= 1e-12 * np.abs(ref).max()
    ref32 = ref.astype(np.float32)
    assert np.all(np.abs(mine32.astype(np.float64) - ref32.astype(np.float64)) <= np.spacing(np.abs(ref32)).astype(np.float64))
    assert np.array_equal(mine32, mine.astype(np.float32))                            # the table is the fp64 result rounded
    assert same(run_segments(case, normalize=1), got)                                 # two runs are bitwise equal


# ---- the buffer ----------------------------------------------------------------------------------------------------------------------------------------------------

def collect(buf, rng, done_at, stop_at=None):
    """A continuous collection: every lane steps until it is full (or has taken stop_at[e] steps); lane e reports done at its steps done_at[e] (1-based) and goes on.
    Bootstraps the lanes that need it.  Returns the valid-row list."""
    E, T = buf.num_envs, buf.horizon
    stop_at = stop_at or {}
    buf.reset()
    while True:
        live = np.array([e for e in range(E) if buf.lengths[e] < min(T, stop_at.get(e, T))], np.int64)
        if not len(live):
            break
        f, ms, nz = inputs(rng, len(live))
        buf.step(f, ms, env_ids=live, noise=nz)
        dones = np.array([int(buf.lengths[e]) + 1 in done_at.get(int(e), ()) for e in live])
        buf.outcome(rng.uniform(0, 1, len(live)), dones, env_ids=live)
    need = buf.rows.needs_bootstrap()
    f, ms, _ = inputs(rng, E)
    buf.bootstrap(f[need], ms[need], env_ids=need)
    assert buf.bootstrap(None, None) is None                                          # nothing left that needs one: a no-op
    return buf.rows.valid_rows()


def host_samples(buf, valid, normalize):
    """The trainer's own statements on the tables read back: per SEGMENT compute_gae (bootstrap 0.0 behind a done, as train.py:172's value is masked by the terminal flag)
    + normalize_advantages; normalize = "batch": numpy's fp64 statistics over all samples.  Samples in the valid-row order."""
    import utils
    E, T = buf.num_envs, buf.horizon
    s, a, v = tables(buf)
    v = v.reshape(E, T + 1)
    rets, advs, raws = [], [], []
    for e, first, n in buf.rows.segments():
        done = buf.rows.dones[e, first + n - 1] != 0
        adv = utils.compute_gae(buf.rows.rewards[e, first:first + n], v[e, first:first + n], 0.0 if done else v[e, first + n], buf.rows.dones[e, first:first + n], GAMMA, LAM)
        ret, advn = utils.normalize_advantages(adv, v[e, first:first + n])
        rets.append(ret)
        advs.append(advn)
        raws.append(adv)
    raw = np.concatenate(raws)
    adv = np.concatenate(advs) if normalize == "segment" else (raw - raw.mean()) / (raw.std() + 1e-8)
    return s[valid], a[valid], np.concatenate(rets), adv


def test_buffer_equals_the_existing_buffer_where_they_overlap(world, tmp_path):
    """No lane is ended by a done (every lane ends at the horizon or is stopped early): a RolloutBuffer handed the same tables and rows trains to the same bits."""
    from rollout import ContinuousRolloutBuffer, RolloutBuffer
    E, T = 8, 16
    _, m_a = make_pair(tmp_path / "a")
    _, m_b = make_pair(tmp_path / "b")
    cb = ContinuousRolloutBuffer(world["vae"], m_a, E, T)
    valid = collect(cb, np.random.RandomState(171), {}, {2: 5, 6: 11})
    assert cb.lengths.tolist() == [16, 16, 5, 16, 16, 16, 11, 16] and cb.rows.segments().tolist() == [[e, 0, int(cb.lengths[e])] for e in range(E)]
    rb = RolloutBuffer(world["vae"], m_b, E, T)
    for dst, src in ((rb.states, cb.states), (rb.actions, cb.actions), (rb.values, cb.values)):
        dst.copy_(src)
    rb.rows.lengths[:], rb.rows.rewards[:], rb.rows.dones[:] = cb.rows.lengths, cb.rows.rewards, cb.rows.dones
    rb.rows.state[:] = rb.rows.CLOSED
    assert np.array_equal(rb.rows.valid_rows(), valid)
    np.random.seed(5)
    out_c = cb.update(GAMMA, LAM, num_epochs=3, batch_size=32)
    np.random.seed(5)
    out_r = rb.update(GAMMA, LAM, num_epochs=3, batch_size=32)
    assert out_c["samples"] == out_r["samples"] == 112 and len(out_c["losses"]) == 12
    assert out_c["losses"] == out_r["losses"]
    for k in ("raw_advantages", "returns", "advantages", "values", "bootstrap_values", "lengths"):
        assert np.array_equal(out_c[k], out_r[k], equal_nan=True), k
    for t_c, t_r in ((cb.returns, rb.returns), (cb.advantages, rb.advantages), (cb.logp_old, rb.logp_old)):
        assert np.array_equal(t_c.cpu().numpy()[valid], t_r.cpu().numpy()[valid])
    pa, pb = m_a.dev.export_params(), m_b.dev.export_params()
    for name in pa:
        assert np.array_equal(pa[name], pb[name]), name


# Parameters after the update, route A (the continuous buffer: cached log pi_old, gather inside the kernels) against route B (PPO.train_step per minibatch on the host's
# per-segment samples: in-step old-policy forward, rows gathered on the host), largest |difference| of a tensor relative to the tensor's max.  MEASURED on one MI355X
# against that loop: normalize="segment" 1.634e-06 (policy/action_logstd; policy/dense/bias 8.8e-07), normalize="batch" 4.479e-06 (policy/dense/bias, a tensor that starts
# at zero and is still small after 12 steps; the batch-normalised advantages themselves came out bitwise numpy's); the value net's six tensors came out bitwise equal both
# times.  Asserted with a factor of 4 as the margin for other boxes and library builds (test_m_rollout_buffer_gpu.py's rule).
PARAM_REL_MEASURED = {"segment": 1.634e-06, "batch": 4.479e-06}
VALUE_NET = ("policy/dense_2/", "policy/dense_3/", "policy/value/")


@pytest.mark.parametrize("normalize", ["segment", "batch"])
def test_update_with_mid_lane_dones_matches_the_trainers_loop_and_the_oracle(world, tmp_path, normalize):
    from rollout import ContinuousRolloutBuffer
    seed, epochs, batch = 5, 3, 32
    E, T = 8, 16
    o, m_a = make_pair(tmp_path / "a")
    _, m_b = make_pair(tmp_path / "b")
    buf = ContinuousRolloutBuffer(world["vae"], m_a, E, T)
    done_at = {1: (4,), 2: (1, 2, 9), 4: (16,), 5: (7, 16), 7: (15,)}                 # mid-lane, back to back, at a lane's end, one step before it
    valid = collect(buf, np.random.RandomState(271), done_at)
    assert buf.lengths.tolist() == [T] * E and len(valid) == 128
    segs = buf.rows.segments()
    assert segs.tolist() == [[0, 0, 16], [1, 0, 4], [1, 4, 12], [2, 0, 1], [2, 1, 1], [2, 2, 7], [2, 9, 7], [3, 0, 16], [4, 0, 16], [5, 0, 7], [5, 7, 9], [6, 0, 16],
                             [7, 0, 15], [7, 15, 1]]
    assert buf.rows.closed.tolist() == [True, True, True, True, False, False, True, True]      # lanes 4 and 5 end in a done: no bootstrap
    s, a, ret, adv = host_samples(buf, valid, normalize)
    np.random.seed(seed)
    times = {}
    out = buf.update(GAMMA, LAM, num_epochs=epochs, batch_size=batch, normalize=normalize, stage_times=times)
    n_steps = epochs * (128 // batch)
    assert out["samples"] == 128 and len(out["losses"]) == n_steps and out["lengths"].tolist() == [T] * E and np.array_equal(out["segments"], segs)
    assert sorted(times) == ["finish", "logp_old", "sgd"]
    assert np.isnan(out["bootstrap_values"]).tolist() == [False, False, False, False, True, True, False, False] and out["bootstrap_values"].dtype == np.float32
    assert not np.isnan(out["returns"]).any() and not np.isnan(out["advantages"]).any() and not np.isnan(out["values"]).any()
    # returns (and per-segment advantages) are the host statements', bit for bit
    assert np.array_equal(out["returns"].reshape(-1), ret)
    assert np.array_equal(buf.returns.cpu().numpy()[valid], ret.astype(np.float32))
    if normalize == "segment":
        assert np.array_equal(out["advantages"].reshape(-1), adv) and np.array_equal(buf.advantages.cpu().numpy()[valid], adv.astype(np.float32))
    else:
        err = np.abs(out["advantages"].reshape(-1) - adv).max()
        print("\nbatch-normalised advantages against numpy: max |diff| = %.3e (bound %.3e)" % (err, 1e-12 * np.abs(adv).max()))
        assert err <= 1e-12 * np.abs(adv).max()
        assert abs(out["advantages"].mean()) < 1e-12 and out["advantages"].std() == pytest.approx(1.0, abs=1e-6)
    # route B: the loop of train.py:193-207 on a second model with the same weights; route O: the oracle fed the same
    m_b.update_old_policy()
    np.random.seed(seed)
    logs_b = [m_b.train_step(s[mb], a[mb], ret[mb], adv[mb]) for mb in po.minibatch_schedule(len(valid), batch, epochs)]
    o.update_old_policy()
    np.random.seed(seed)
    logs_o = [o.train(s[mb], a[mb], ret[mb], adv[mb]) for mb in po.minibatch_schedule(len(valid), batch, epochs)]
    check_losses(out["losses"], logs_o, "A against O")
    check_losses(out["losses"], logs_b, "A against B")
    assert out["losses"][0]["prob_ratio"] == pytest.approx(1.0, abs=1e-5)
    assert m_a.get_train_step_idx() == m_b.get_train_step_idx() == n_steps
    pa, pb = m_a.dev.export_params(), m_b.dev.export_params()
    worst = max(rel_err(pa[name], pb[name]) for name in pa)
    print("\nparameters after the update (normalize=%s), continuous buffer against PPO.train_step loop: max |diff| / tensor max = %.3e" % (normalize, worst))
    for name in pa:
        print("  %-34s %.3e" % (name, rel_err(pa[name], pb[name])))
    assert any(name.startswith(VALUE_NET) for name in pa)
    for name in pa:
        if name.startswith(VALUE_NET):
            assert np.array_equal(pa[name], pb[name]), name                          # the returns are bitwise the host's and log pi_old does not enter
    assert worst <= 4 * PARAM_REL_MEASURED[normalize], worst


def test_recording_after_a_done_is_confined(world, tmp_path):
    """A step after a done records into slot lengths[e], bitwise what the call returned; every other table row is unchanged."""
    from rollout import ContinuousRolloutBuffer
    E, T = 5, 4
    _, m = make_pair(tmp_path / "m")
    buf = ContinuousRolloutBuffer(world["vae"], m, E, T)
    buf.reset()
    fill_tables(buf)
    rng = np.random.RandomState(371)
    done_at = {0: (1,), 2: (2,), 3: (1, 2, 3)}
    for t in range(T):
        f, ms, nz = inputs(rng, E)
        perm = rng.permutation(E)
        before = tables(buf)
        rows = perm * (T + 1) + buf.lengths[perm]
        assert rows.tolist() == (perm * (T + 1) + t).tolist()                         # a done moved no lane back to slot 0
        got = buf.step(f, ms, env_ids=perm, noise=nz)
        check_recorded(tables(buf), before, rows, got, ms, t)
        buf.outcome(rng.uniform(0, 1, E), np.array([t + 1 in done_at.get(int(e), ()) for e in perm]), env_ids=perm)
    assert buf.lengths.tolist() == [T] * E and buf.rows.needs_bootstrap().tolist() == [0, 1, 2, 3, 4]
    assert bool((buf.returns == SENTINEL).all()) and bool((buf.advantages == SENTINEL).all()) and bool((buf.logp_old == SENTINEL).all())
    f, ms, _ = inputs(rng, E)
    before = tables(buf)
    got = buf.bootstrap(f, ms)
    s, a, v = tables(buf)
    rows = np.arange(E) * (T + 1) + T
    assert np.array_equal(v[rows], got[1]) and np.array_equal(s[rows, :Z], got[2][:, :Z].astype(np.float32))
    other = np.ones(len(v), bool)
    other[rows] = False
    for now, was in zip((s, a, v), before):
        assert np.array_equal(now[other], was[other])
    np.random.seed(3)
    out = buf.update(num_epochs=1, batch_size=8)
    assert out["samples"] == E * T and len(out["segments"]) == 5 + 1 + 1 + 3
    # slots of no segment (the bootstrap slots) were not written by the finish
    assert bool((buf.returns[rows] == SENTINEL).all()) and bool((buf.advantages[rows] == SENTINEL).all())
    with pytest.raises(ValueError, match="normalize"):
        buf.update(normalize="lane")


def test_second_collection_after_reset_matches_a_fresh_buffer(world, tmp_path):
    """No state leaks from one collect -> update cycle into the next (mirrors test_m_rollout_buffer_gpu.py: the two models reach the second cycle through their own
    first cycles, whose collections end in fp32 atomics, so the comparison is at the update tolerances, not bitwise)."""
    from rollout import ContinuousRolloutBuffer
    E, T = 6, 8
    _, m1 = make_pair(tmp_path / "m1", learning_rate=1e-3)
    _, m2 = make_pair(tmp_path / "m2", learning_rate=1e-3)
    used, first = ContinuousRolloutBuffer(world["vae"], m1, E, T, seed=3), ContinuousRolloutBuffer(world["vae"], m2, E, T, seed=3)
    outs = []
    for buf, m in ((used, m1), (first, m2)):
        collect(buf, np.random.RandomState(81), {1: (3,), 4: (8,)})                    # cycle 1: every lane full
        np.random.seed(9)
        buf.update(num_epochs=1, batch_size=16)
        if buf is first:
            buf = ContinuousRolloutBuffer(world["vae"], m, E, T, seed=3)              # cycle 2 on a buffer that has seen nothing
        valid = collect(buf, np.random.RandomState(82), {0: (2, 5), 3: (5,), 5: (1, 8)}, {3: 5, 4: 1})      # other segments, shorter lanes: stale slots lie behind them
        assert buf.lengths.tolist() == [8, 8, 8, 5, 1, 8]
        np.random.seed(10)
        outs.append((buf.update(num_epochs=2, batch_size=16), valid))
    (a, va), (b, vb) = outs
    assert np.array_equal(va, vb) and np.array_equal(a["segments"], b["segments"]) and a["samples"] == b["samples"] == 38
    check_losses(a["losses"], b["losses"], "reused against fresh")
    assert np.array_equal(np.isnan(a["returns"]), np.isnan(b["returns"])) and np.array_equal(np.isnan(a["bootstrap_values"]), np.isnan(b["bootstrap_values"]))
    assert np.allclose(np.nan_to_num(a["returns"]), np.nan_to_num(b["returns"]), rtol=1e-4, atol=1e-4)
