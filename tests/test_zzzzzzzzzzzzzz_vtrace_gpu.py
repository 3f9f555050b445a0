"""V-trace on the GPU: mi_rollout_finish_vtrace (csrc/ppo_ops.hip) against the GAE finish entries (the identity), against the float64 references of
tests/vtrace_cases.py and against itself; mi_ppo_logp_idx (csrc/ppo_fused.hip, ppo_logp_head_kernel) against float64, against the statistics pass and the cache of
log pi_old, and against itself; and RolloutBuffer / ContinuousRolloutBuffer.set_vtrace against a host loop on a twin policy.  Run with -s for the measured distances.

Bounds.  weights_out against numpy's exp: 4 fp64 ulps (both libraries document at most 1 ulp for double exp, so the two lie within 2 ulps of each other; the bound
doubles that).  log pi against float64: 1e-4 of the sum of the absolute terms of log pi, sum_a z^2 / 2 + |logstd| + log(2 pi) / 2, the bound the clone and
demonstration tests hold clone_loss to (their cases files form the batch mean of the same terms; here it is per row), in both precision modes.  Everything else is
bitwise: the finish op's other outputs against reference (a) fed the device's own weights (the normalisation's sums in the finish kernels' documented order,
vtrace_cases.wave_sum), the fp32 tables against float32() of the fp64 outputs.

The buffers: an update with V-trace and recomputation on is compared, bit for bit, with vt_host_loop() -- the first (GAE) finish call, the cache of log pi_old, and
per epoch the refresh (PpoDevice.values_idx, PpoDevice.logp_idx, mi_rollout_finish_vtrace) and the policy's own minibatch step per shuffled minibatch -- on a twin
policy from a copy of the collected tables.  The collection helpers are those of the advantage-recomputation tests."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "carla-ppo_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import advantage_recomputation_cases as ac  # noqa: E402
import test_zzzzzzzzzzzzz_advantage_recomputation_gpu as rg  # noqa: E402  (helpers only: device(), make(), collect(), copy_collection(), finish_call(), ..)
import vtrace_cases as vc  # noqa: E402
from oracle import ppo_oracle as po  # noqa: E402
from oracle import vae_oracle as vo  # noqa: E402
from rollout_gpu_common import SENTINEL, bitwise, flat_state  # noqa: E402

pytestmark = pytest.mark.gpu

PAD = 8
GAMMA, LAM = rg.GAMMA, rg.LAM
MI_ERR_ARG = -1
IDS = vc.case_ids()
IDS_IDENTITY = [cid for cid in IDS if cid[2] in ((1.0, 1.0), (2.5, 1.5)) and cid[3] == 0]
same_bits = rg.same_bits


def same_bits64(x, y):
    return np.array_equal(np.asarray(x, np.float64).view(np.int64), np.asarray(y, np.float64).view(np.int64))


# ---------------------------------------------------------------------------------------------------------------------------------------- the finish op
OUT_F32, OUT_F64 = ("tab_returns", "tab_adv"), ("adv_raw", "returns", "adv_norm", "weights")


def lib():
    from mi355 import lib as milib
    return milib.get()


def outputs(E, T):
    """Every output filled with SENTINEL, PAD more behind it."""
    import torch
    out = {k: torch.full((E * (T + 1) + PAD,), SENTINEL, device="cuda") for k in OUT_F32}
    out.update({k: torch.full((E * T + PAD,), SENTINEL, dtype=torch.float64, device="cuda") for k in OUT_F64})
    return out


def host(out):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def run_vtrace(c, rbd, normalize, boot=True, **over):
    """mi_rollout_finish_vtrace on case c through the raw entry -> (return code, the outputs on the host, each with its PAD behind it).  over: tables (values,
    final_values, lp_now, lp_old, rewards, dones, seg_row, seg_len, seg_boot) or arguments (T, n_seg, num_envs, rho_bar, c_bar, normalize_arg, rbd_arg) replaced,
    `null`: names of pointer arguments passed as NULL."""
    import torch
    E, T = c["E"], c["T"]
    g = lambda k: np.ascontiguousarray(over.get(k, c[k]))      # noqa: E731
    dev = lambda a: torch.from_numpy(a).to("cuda")      # noqa: E731
    t = {k: dev(g(k).reshape(-1)) for k in ("values", "final_values", "lp_now", "lp_old", "rewards", "dones", "seg_row", "seg_len", "seg_boot")}
    n_seg = len(g("seg_row"))
    out = outputs(E, T)
    scratch = torch.full((2 * n_seg + 2 + PAD,), SENTINEL, dtype=torch.float64, device="cuda")
    null = set(over.get("null", ()))
    if not boot:
        null |= {"final_values", "seg_boot"}
    if normalize == 0:
        null |= {"scratch"}
    p = lambda name, tensor: None if name in null else tensor.data_ptr()      # noqa: E731
    rc = lib().cdll.mi_rollout_finish_vtrace(
        None, p("values", t["values"]), p("lp_now", t["lp_now"]), p("lp_old", t["lp_old"]), p("rewards", t["rewards"]), p("dones", t["dones"]),
        p("seg_row", t["seg_row"]), p("seg_len", t["seg_len"]), over.get("n_seg", n_seg), over.get("num_envs", E), over.get("T", T), c["gamma"], c["lam"],
        over.get("rho_bar", c["rho_bar"]), over.get("c_bar", c["c_bar"]), over.get("rbd_arg", rbd), over.get("normalize_arg", normalize), p("scratch", scratch),
        p("tab_returns", out["tab_returns"]), p("tab_adv", out["tab_adv"]), p("adv_raw", out["adv_raw"]), p("returns", out["returns"]), p("adv_norm", out["adv_norm"]),
        p("weights", out["weights"]), p("final_values", t["final_values"]), p("seg_boot", t["seg_boot"]))
    got = host(out)
    got["scratch_pad"] = scratch.cpu().numpy()[2 * n_seg + 2:]
    return rc, got


def run_gae(c, form, normalize, lens=None):
    """The existing entry on the same inputs: form "rows" (mi_rollout_finish, lens), "seg" (mi_rollout_finish_segments) or "boot" (.._boot)."""
    import torch
    E, T, L = c["E"], c["T"], lib()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to("cuda")      # noqa: E731
    v, fv, r, d = dev(c["values"]), dev(c["final_values"]), dev(c["rewards"]), dev(c["dones"])
    out = outputs(E, T)
    o = [out[k].data_ptr() for k in ("tab_returns", "tab_adv", "adv_raw", "returns", "adv_norm")]
    if form == "rows":
        ln = dev(np.asarray(lens, np.int32))
        L.mi_rollout_finish(None, v.data_ptr(), r.data_ptr(), d.data_ptr(), ln.data_ptr(), E, T, c["gamma"], c["lam"], *o)
    else:
        row, length, boot = dev(c["seg_row"]), dev(c["seg_len"]), dev(c["seg_boot"])
        n_seg = len(c["seg_row"])
        scratch = torch.empty(2 * n_seg + 2, dtype=torch.float64, device="cuda") if normalize else None
        args = (None, v.data_ptr(), r.data_ptr(), d.data_ptr(), row.data_ptr(), length.data_ptr(), n_seg, E, T, c["gamma"], c["lam"], normalize,
                None if scratch is None else scratch.data_ptr(), *o)
        if form == "seg":
            L.mi_rollout_finish_segments(*args)
        else:
            L.mi_rollout_finish_segments_boot(*args, fv.data_ptr(), boot.data_ptr())
    return host(out)


def rows_form(c):
    """Case c as mi_rollout_finish sees a buffer: one segment per lane from slot 0, ragged lengths (the last of three or more lanes empty), lane 0's last step
    terminal -- the slot behind it is read and masked."""
    E, T = c["E"], c["T"]
    lens = np.array([max(1, T - 2 * e) for e in range(E)], np.int32)
    if E >= 3:
        lens[E - 1] = 0
    d = dict(c)
    d["dones"] = c["dones"].copy()
    d["dones"][0, lens[0] - 1] = 1.0
    d["seg_row"] = (np.arange(E) * (T + 1)).astype(np.int32)
    d["seg_len"], d["seg_boot"] = lens.copy(), np.zeros(E, np.int32)
    return d, lens


@pytest.mark.parametrize("cid", IDS_IDENTITY, ids=vc.case_name)
def test_the_policy_has_not_moved_the_finish_is_the_gae_finish(cid):
    """tab_logp_now a bitwise copy of tab_logp_old, bars >= 1: every output is the matching GAE entry's, bit for bit, sentinels and unwritten slots included."""
    c = vc.case(cid)
    still = dict(lp_now=c["lp_old"].copy())
    names = ("tab_returns", "tab_adv", "adv_raw", "returns", "adv_norm")
    d, lens = rows_form(c)
    rc, got = run_vtrace(d, 1, 0, boot=False, **still)
    want = run_gae(d, "rows", 0, lens)
    assert rc == 0 and all(same_bits64(got[k], want[k]) if got[k].dtype == np.float64 else same_bits(got[k], want[k]) for k in names), (cid, "mi_rollout_finish")
    for normalize in (0, 1):
        for form, boot in (("seg", False), ("boot", True)):
            rc, got = run_vtrace(c, 0, normalize, boot=boot, **still)
            want = run_gae(c, form, normalize)
            for k in names:
                eq = same_bits64(got[k], want[k]) if got[k].dtype == np.float64 else same_bits(got[k], want[k])
                assert rc == 0 and eq, (cid, form, normalize, k)
    w = got["weights"][:c["E"] * c["T"]]
    assert np.all((w == 1.0) | (w == SENTINEL)) and (w == 1.0).sum() == sum(n for *_, n, _ in c["segs"])


def expected(c, got, rbd, normalize):
    """Reference (a) fed the device's own weights -> the reference dict and the mask of executed steps [E, T]."""
    E, T = c["E"], c["T"]
    w = np.zeros((E, T + 1))
    w[:, :T] = got["weights"][:E * T].reshape(E, T)
    ref = vc.reference(c, w, bool(rbd), normalize)
    return ref, ~np.isnan(ref["raw"])


@pytest.mark.parametrize("cid", IDS, ids=vc.case_name)
def test_the_finish_against_the_references(cid):
    c = vc.case(cid)
    E, T = c["E"], c["T"]
    w_np = vc.weights64(c)[:, :T]
    for rbd in (0, 1):
        for normalize in (0, 1):
            rc, got = run_vtrace(c, rbd, normalize)
            assert rc == 0
            ref, ex = expected(c, got, rbd, normalize)
            w = got["weights"][:E * T].reshape(E, T)
            ulps = float((np.abs(w[ex] - w_np[ex]) / np.spacing(w_np[ex])).max())
            assert ulps <= 4.0 and np.all(w[~ex] == SENTINEL), (cid, rbd, normalize, ulps)
            f64 = {k: got[k][:E * T].reshape(E, T) for k in ("adv_raw", "returns", "adv_norm")}
            dist = {}
            for k, r in (("adv_raw", "raw"), ("returns", "returns"), ("adv_norm", "adv")):
                dist[k] = float(np.abs(f64[k][ex] - ref[r][ex]).max() / max(np.abs(ref[r][ex]).max(), 1e-300))
            print("%s rbd=%d normalize=%d: weights %.2f ulps of numpy's exp; |device - reference (a)| / max: raw %.2e, returns %.2e, normalised %.2e"
                  % (vc.case_name(cid), rbd, normalize, ulps, dist["adv_raw"], dist["returns"], dist["adv_norm"]))
            for k, r in (("adv_raw", "raw"), ("returns", "returns"), ("adv_norm", "adv")):
                assert same_bits64(f64[k][ex], ref[r][ex]), (cid, rbd, normalize, k, dist[k])
                assert np.all(f64[k][~ex] == SENTINEL), (cid, k)                      # slots of no executed segment keep their sentinel
            tabs = {k: got[k][:E * (T + 1)].reshape(E, T + 1) for k in OUT_F32}
            assert same_bits(tabs["tab_returns"][:, :T][ex], f64["returns"][ex].astype(np.float32))
            assert same_bits(tabs["tab_adv"][:, :T][ex], f64["adv_norm"][ex].astype(np.float32))
            for k in OUT_F32:
                assert np.all(tabs[k][:, :T][~ex] == SENTINEL) and np.all(tabs[k][:, T] == SENTINEL), (cid, k)
            assert all(np.all(got[k][-PAD:] == SENTINEL) for k in OUT_F32 + OUT_F64) and np.all(got["scratch_pad"] == SENTINEL), (cid, "the sentinels behind the outputs")


def read_masks(c, rbd):
    """What an executed segment reads: value slots [E, T + 1], log-probability slots [E, T + 1], final-value slots [E, T + 1], steps [E, T]; and the value slots
    behind a terminal / a truncated segment that nothing reads."""
    E, T = c["E"], c["T"]
    v, lp, fv, st = np.zeros((E, T + 1), bool), np.zeros((E, T + 1), bool), np.zeros((E, T + 1), bool), np.zeros((E, T), bool)
    for e, s, n, kind in c["segs"]:
        v[e, s:s + n] = lp[e, s:s + n] = st[e, s:s + n] = True
        if kind == vc.TRUNCATED:
            fv[e, s + n - 1] = True
        elif kind == vc.OPEN or rbd:
            v[e, s + n] = True
    behind = {k: [(e, s + n) for e, s, n, kind in c["segs"] if kind == k and not v[e, s + n]] for k in (vc.TERMINAL, vc.TRUNCATED)}
    return v, lp, fv, st, behind


@pytest.mark.parametrize("cid", [(3, 5, (2.5, 1.5), 0), (5, 70, (2.5, 1.5), 0)], ids=vc.case_name)
def test_nan_where_nothing_is_read_changes_nothing_and_two_runs_agree(cid):
    c = vc.case(cid)
    names = OUT_F32 + OUT_F64
    for normalize in (0, 1):
        rc, clean = run_vtrace(c, 0, normalize)
        rc2, again = run_vtrace(c, 0, normalize)
        assert rc == 0 == rc2 and all(np.array_equal(clean[k], again[k]) for k in names), "two runs"
        v, lp, fv, st, behind = read_masks(c, 0)
        assert behind[vc.TERMINAL] and behind[vc.TRUNCATED]                         # a slot behind a done and one behind a truncated segment that no segment reads
        nan = lambda a, read: np.where(read, a, np.nan).astype(a.dtype)      # noqa: E731
        planted = dict(values=nan(c["values"], v), final_values=nan(c["final_values"], fv), lp_now=nan(c["lp_now"], lp), lp_old=nan(c["lp_old"], lp),
                       rewards=nan(c["rewards"], st), dones=nan(c["dones"], st))
        rc, got = run_vtrace(c, 0, normalize, **planted)
        assert rc == 0 and all(np.array_equal(clean[k], got[k]) for k in names), ("NaN in every slot that is not read", normalize)


def test_a_nan_in_a_read_log_probability_reaches_its_segment():
    """It is not masked by a bar: planted at the last step of a segment of two or more steps, every return of that segment and every raw advantage in front of that
    step is NaN; the other segments keep their bits (per-segment normalisation)."""
    c = vc.case((3, 5, (0.5, 0.0), 0))
    E, T = c["E"], c["T"]
    e, s, n, _ = next(seg for seg in c["segs"] if seg[2] >= 2)
    lp_now = c["lp_now"].copy()
    lp_now[e, s + n - 1] = np.nan
    rc, clean = run_vtrace(c, 0, 0)
    rc2, got = run_vtrace(c, 0, 0, lp_now=lp_now)
    assert rc == 0 == rc2
    ret, raw = got["returns"][:E * T].reshape(E, T), got["adv_raw"][:E * T].reshape(E, T)
    assert np.isnan(ret[e, s:s + n]).all() and np.isnan(raw[e, s:s + n - 1]).all() and np.isnan(got["weights"][:E * T].reshape(E, T)[e, s + n - 1])
    other = np.ones((E, T), bool)
    other[e, s:s + n] = False
    for k in OUT_F64:
        assert np.array_equal(got[k][:E * T].reshape(E, T)[other], clean[k][:E * T].reshape(E, T)[other]), k


def test_a_refused_finish_writes_nothing():
    c = vc.case((3, 5, (2.5, 1.5), 0))
    nan, inf = float("nan"), float("inf")
    refusals = [dict(T=0), dict(T=4097), dict(n_seg=0), dict(num_envs=0), dict(rho_bar=nan), dict(rho_bar=0.0), dict(rho_bar=-1.0), dict(c_bar=nan), dict(c_bar=-0.5),
                dict(null=("final_values",)), dict(null=("seg_boot",)), dict(normalize_arg=1, null=("scratch",))]
    refusals += [dict(null=(k,)) for k in ("values", "lp_now", "lp_old", "rewards", "dones", "seg_row", "seg_len", "tab_returns", "tab_adv")]
    for kw in refusals:
        rc, got = run_vtrace(c, 0, 1 if "normalize_arg" in kw else 0, **kw)
        assert rc == MI_ERR_ARG and lib().cdll.mi_last_error().startswith(b"mi_rollout_finish_vtrace: "), kw
        assert all(np.all(got[k] == SENTINEL) for k in OUT_F32 + OUT_F64) and np.all(got["scratch_pad"] == SENTINEL), kw
    rc, _ = run_vtrace(c, 0, 0, rho_bar=inf, c_bar=inf)                              # +inf is a valid bar
    assert rc == 0


# ---------------------------------------------------------------------------------------------------------------------------------------- mi_ppo_logp_idx
HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)


def logp64(pol, s, a):
    """log pi(a | s) in float64 from the float32 parameters, states and actions -> (log pi [n], the sum of the absolute terms [n])."""
    import torch
    th = {k: torch.from_numpy(v.astype(np.float64)) for k, v in pol["theta"].items()}
    with torch.no_grad():
        mean, ls, _ = po.policy_forward(th, torch.from_numpy(s.astype(np.float64)), pol["low"], pol["high"])
    mean, ls = mean.numpy(), np.broadcast_to(ls.numpy(), mean.shape)
    z = (a.astype(np.float64) - mean) / np.exp(ls)
    return (-0.5 * z * z - (HALF_LOG_2PI + ls)).sum(1), (0.5 * z * z + np.abs(ls) + HALF_LOG_2PI).sum(1)


def actions(name, s, seed=0):
    """The policy's own sampled actions at states s, clipped into the action range, float32 [n, A]."""
    import torch
    pol = ac.policy(name)
    th = {k: torch.from_numpy(v.astype(np.float64)) for k, v in pol["theta"].items()}
    with torch.no_grad():
        mean, ls, _ = po.policy_forward(th, torch.from_numpy(s.astype(np.float64)), pol["low"], pol["high"])
    noise = np.random.RandomState(600 + len(s) + seed).standard_normal(mean.shape)
    return np.clip(mean.numpy() + np.exp(ls.numpy()) * noise, pol["low"], pol["high"]).astype(np.float32)


def tables(d, s, a, rows, n_rows, fill=np.nan):
    """-> (states table, actions table, row list or None, n) on the device: with rows, tables of n_rows rows of `fill` whose row rows[i] holds s[i] / a[i]."""
    import torch
    if rows is None:
        return torch.from_numpy(s).to(d.device), torch.from_numpy(a).to(d.device), None, len(s)
    hs, ha = np.full((n_rows, s.shape[1]), fill, np.float32), np.full((n_rows, a.shape[1]), fill, np.float32)
    hs[rows], ha[rows] = s, a
    return torch.from_numpy(hs).to(d.device), torch.from_numpy(ha).to(d.device), torch.from_numpy(np.asarray(rows, np.int32)).to(d.device), n_rows


def run_logp(d, s, a, rows=None, n_rows=None):
    """logp_idx on host rows -> the out table (NaN to start with) with its PAD sentinels behind it, on the host."""
    import torch
    ts, ta, idx, n = tables(d, s, a, rows, n_rows)
    full = torch.full((n + PAD,), float("nan"), device=d.device)
    full[n:] = SENTINEL
    d.logp_idx(ts, ta, idx, len(s), full[:n])
    torch.cuda.synchronize()
    return full.cpu().numpy()


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("name", list(ac.POLICIES))
def test_logp_against_float64(name, precision):
    """Contiguous, and through a row list into larger tables with NaN in every row of `states` and `actions` the list does not name; entries of the output no row
    names keep their NaN."""
    d, pol, worst = rg.device(name, precision), ac.policy(name), 0.0
    for M in ac.ROW_COUNTS:
        s = ac.states(name, M)
        a = actions(name, s)
        ref, terms = logp64(pol, s, a)
        got = run_logp(d, s, a)
        assert np.all(got[M:] == SENTINEL)
        d_c = float((np.abs(got[:M] - ref) / (1e-4 * terms)).max())
        rows, n = rg.row_list(M)
        tab = run_logp(d, s, a, rows, n)
        other = np.ones(n, bool)
        other[rows] = False
        assert np.all(tab[n:] == SENTINEL) and np.isnan(tab[:n][other]).all() and not np.isnan(tab[rows]).any(), (name, M)
        d_l = float((np.abs(tab[rows] - ref) / (1e-4 * terms)).max())
        print("%s %s M=%d: contiguous %.3e, row list %.3e of the bound (1e-4 of the absolute terms, mean %.2f)" % (name, precision, M, d_c, d_l, terms.mean()))
        worst = max(worst, d_c, d_l)
    assert worst <= 1.0, (name, precision, worst)


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("name", list(ac.POLICIES))
def test_logp_is_bitwise_the_statistics_pass_the_cache_and_itself(name, precision):
    """logp_new_out of mi_ppo_update_stats_idx on the same rows and parameters; the cache of mi_ppo_logp_old (theta_old == theta: the devices of rg.device() load
    both from one set, which is what update_old_policy() leaves); the row-list form against the contiguous form; two runs."""
    import torch
    from mi355.ppo_device import N_STATS
    d, pol = rg.device(name, precision), ac.policy(name)
    assert bitwise(d.params, d.params_old)
    dev = d.device
    for M in (5, 33, 257):
        s = ac.states(name, M, seed=1)
        a = actions(name, s, seed=1)
        rows, n = rg.row_list(M, seed=1)
        tab = run_logp(d, s, a, rows, n)
        assert same_bits(tab[rows], run_logp(d, s, a, rows, n)[rows]), (name, M, "two runs")
        contiguous = run_logp(d, s, a)[:M]
        assert same_bits(tab[rows], contiguous), (name, M, "row list against contiguous")
        ts, ta, idx, _ = tables(d, s, a, rows, n, fill=0.0)                          # (the statistics pass reads returns / logp_old of the named rows)
        lp_out = torch.full((n,), float("nan"), device=dev)
        d.update_stats(ts, ta, torch.zeros(n, device=dev), torch.zeros(n, device=dev), idx, M, torch.zeros(N_STATS, dtype=torch.float64, device=dev),
                       torch.zeros(d.stats_scratch_doubles(M), dtype=torch.float64, device=dev), logp_new_out=lp_out)
        assert same_bits(tab[rows], lp_out.cpu().numpy()[rows]), (name, precision, M, "logp_new_out of update_stats")
        cache = torch.full((M,), float("nan"), device=dev)
        d.logp_old(torch.from_numpy(s).to(dev), torch.from_numpy(a).to(dev), M, cache)
        assert same_bits(contiguous, cache.cpu().numpy()), (name, precision, M, "the cache of logp_old")


@pytest.mark.parametrize("M", [64, 65, 200])
def test_the_chunk_loop_of_logp(M):
    """An engine of max_batch = 64 against one of max_batch = 256: whole chunks, a partial last chunk, and the row list cut at chunk borders."""
    small, big = rg.device("ref2", max_batch=64), rg.device("ref2", max_batch=256)
    assert small.max_batch == 64 and big.max_batch == 256
    s = ac.states("ref2", M, seed=2)
    a = actions("ref2", s, seed=2)
    x, y = run_logp(small, s, a), run_logp(big, s, a)
    assert same_bits(x, y) and np.all(x[M:] == SENTINEL) and not np.isnan(x[:M]).any()
    rows, n = rg.row_list(M, seed=2)
    x, y = run_logp(small, s, a, rows, n), run_logp(big, s, a, rows, n)
    assert same_bits(x[rows], y[rows]) and np.array_equal(np.isnan(x), np.isnan(y)) and np.isnan(x[:n]).sum() == n - M
    assert small.max_batch == 64                                                     # the engine was not grown


def test_logp_rows_outside_the_table_and_what_is_not_written():
    import torch
    d, M = rg.device("small3"), 37
    dev = d.device
    s = ac.states("small3", M, seed=3)
    a = actions("small3", s, seed=3)
    rows, n = rg.row_list(M, seed=3)
    clean = run_logp(d, s, a, rows, n)
    bad = rows.copy()
    bad[[0, 17, 36]] = (-1, n, n + 5)                                                # outside the table: nothing is stored for them, wherever the clamped loads went
    d.grads.normal_()
    d.adam_m.normal_()
    d.adam_v.uniform_()
    d.losses.fill_(3.25)
    state = [t.clone() for t in (d.params, d.params_old, d.adam_m, d.adam_v, d.grads, d.losses)]
    ts, ta, _, _ = tables(d, s, a, rows, n)
    full = torch.full((n + PAD,), float("nan"), device=dev)
    full[n:] = SENTINEL
    d.logp_idx(ts, ta, torch.from_numpy(bad).to(dev), M, full[:n])
    got = full.cpu().numpy()
    keep = np.ones(M, bool)
    keep[[0, 17, 36]] = False
    assert same_bits(got[rows[keep]], clean[rows[keep]]) and np.isnan(got[rows[~keep]]).all()
    assert np.isnan(got[:n]).sum() == n - keep.sum() and np.all(got[n:] == SENTINEL)
    assert bitwise([d.params, d.params_old, d.adam_m, d.adam_v, d.grads, d.losses], state)
    d.grads.zero_()
    d.adam_m.zero_()
    d.adam_v.zero_()


def test_a_refused_logp_call_writes_nothing():
    import torch
    from mi355 import lib as milib
    from mi355.ppo_device import PpoDevice
    d = rg.device("small3")
    dev, p = d.device, milib.ptr
    s = ac.states("small3", 8)
    table, acts = torch.from_numpy(s).to(dev), torch.from_numpy(actions("small3", s)).to(dev)
    out = torch.full((8 + PAD,), SENTINEL, device=dev)
    cdll = d.L.cdll
    for kw in (dict(M=0), dict(n_rows=0), dict(states=None), dict(actions=None), dict(out=None), dict(M=9)):
        x = dict(states=p(table), actions=p(acts), n_rows=8, M=8, out=p(out))
        x.update(kw)
        assert cdll.mi_ppo_logp_idx(d.handle, None, x["states"], x["actions"], None, x["n_rows"], x["M"], x["out"]) == -1, kw
        assert cdll.mi_last_error().startswith(b"mi_ppo_logp_idx: "), kw
    low, high = ac.bounds(3)
    off = PpoDevice(100, 3, low, high, ac.EPS, ac.VALUE_SCALE, ac.ENTROPY_SCALE, hidden=(64, 64), max_batch=32)      # outside the fused range: MI_ERR_SHAPE
    assert not off.fused_ok()
    wide, wa = torch.zeros(8, 100, device=dev), torch.zeros(8, 3, device=dev)
    assert cdll.mi_ppo_logp_idx(off.handle, None, p(wide), p(wa), None, 8, 8, p(out)) == -2 and cdll.mi_last_error().startswith(b"mi_ppo_logp_idx: needs the fused kernels")
    with pytest.raises(milib.MiError, match="needs the fused kernels"):
        off.logp_idx(wide, wa, None, 8, out[:8])
    off.close()
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


def test_ppo_log_probs(tmp_path):
    """PPO.log_probs() against float64, host and device inputs, one row, and more rows than the engine's max_batch."""
    import torch
    o, m = rg.make_pair(tmp_path / "a")
    s = ac.states("ref2", 41, seed=4)
    a = np.random.RandomState(8).uniform(-0.5, 0.5, (41, 2)).astype(np.float32)
    lp = m.log_probs(s, a)
    assert lp.dtype == np.float32 and lp.shape == (41,)
    th = {k: torch.from_numpy(np.asarray(v, np.float64)) for k, v in o.params.items()}
    space = po.ActionSpace()
    with torch.no_grad():
        mean, ls, _ = po.policy_forward(th, torch.from_numpy(s.astype(np.float64)), space.low, space.high)
    mean, ls = mean.numpy(), np.broadcast_to(ls.numpy(), mean.shape)
    z = (a.astype(np.float64) - mean) / np.exp(ls)
    ref, terms = (-0.5 * z * z - (HALF_LOG_2PI + ls)).sum(1), (0.5 * z * z + np.abs(ls) + HALF_LOG_2PI).sum(1)
    print("PPO.log_probs against float64: %.3e of the bound" % (np.abs(lp - ref) / (1e-4 * terms)).max())
    assert (np.abs(lp - ref) <= 1e-4 * terms).all()
    assert same_bits(m.log_probs(torch.from_numpy(s).to(m.dev.device), torch.from_numpy(a).to(m.dev.device)), lp)
    assert m.log_probs(s[0], a[0]).shape == (1,) and same_bits(m.log_probs(s[0], a[0]), lp[:1])
    mb = m.dev.max_batch
    reps = mb // 41 + 2
    assert same_bits(m.log_probs(np.tile(s, (reps, 1)), np.tile(a, (reps, 1)))[:41], lp) and m.dev.max_batch == mb
    with pytest.raises(ValueError, match="states and"):
        m.log_probs(s, a[:40])


# ---------------------------------------------------------------------------------------------------------------------------------------- the buffers
@pytest.fixture(scope="module")
def vae(tmp_path_factory):
    from vae.models import MlpVAE
    rng = np.random.RandomState(21)
    Z, SRC = rg.Z, rg.SRC
    p = vo.init_mlp_vae_params(3, z_dim=Z, source_shape=SRC, target_shape=SRC, encoder_sizes=(36,), decoder_sizes=(8,))
    for k in p:
        if k.endswith("bias"):
            p[k] = (0.05 * rng.standard_normal(p[k].shape)).astype(np.float32)
    v = MlpVAE(np.array(SRC), encoder_sizes=(36,), decoder_sizes=(8,), z_dim=Z, model_dir=str(tmp_path_factory.mktemp("vtrace_vae")), precision="fp32", training=False)
    v.set_weights(p)
    v.init_session(init_logging=False)
    return v


BARS = (1.02, 0.98)                                                                  # close to 1: three epochs at these sizes move the weights a few per cent and more, so both bars truncate (asserted below)


def make(vae, tmp, continuous, E, T, bars=BARS, recompute=True, **hp):
    """-> (buffer with recomputation and, with bars, V-trace on; its policy)."""
    buf, m, _ = rg.make(vae, tmp, continuous, E, T, recompute, **hp)
    if bars is not None:
        buf.set_vtrace(*bars)
    return buf, m


def vt_host_loop(B, m, continuous, epochs, batch, bars, final_states=None, vclip=False, mbn=None, normalize="segment"):
    """The update with V-trace refreshes, by hand on twin policy `m` from buffer B's tables (B has every setting of the refresh off) -> dict(values_now, logp_now,
    f64 of the first finish, f64 of the last refresh, weights of the last refresh, recomputed)."""
    import torch
    from mi355 import lib as milib
    E, T, dev, d, L = B.num_envs, B.horizon, B.device, m.dev, B.L
    st = torch.cuda.current_stream(dev).cuda_stream
    valid, lengths = B.rows.valid_rows(), B.rows.lengths.copy()
    n_valid = len(valid)
    nan3 = lambda: torch.full((3, E, T), float("nan"), dtype=torch.float64, device=dev)      # noqa: E731
    r, dn = torch.from_numpy(B.rows.rewards).to(dev), torch.from_numpy(B.rows.dones).to(dev)
    first = nan3()
    rg.finish_call(B, continuous, r, dn, normalize)(B.values, getattr(B, "final_values", None), first)
    m.update_old_policy()
    lp = B._cache_logp_old(valid, False)
    values_now, logp_now = B.values.clone(), torch.zeros(B.n_table_rows, device=dev)
    fv_now = B.final_values.clone() if continuous else None
    rows, valid_dev = torch.from_numpy(rg.refresh_rows(B, continuous)).to(dev), torch.from_numpy(valid).to(dev)
    if continuous:
        e_t, t_t = np.nonzero(B.rows.truncs)
        trunc_rows = torch.from_numpy((e_t * (T + 1) + t_t).astype(np.int32)).to(dev)
        segs = B.rows.segments()
        desc = np.stack([segs[:, 0] * (T + 1) + segs[:, 1], segs[:, 2], B.rows.segment_truncated()])
    else:
        lanes = np.nonzero(lengths > 0)[0]
        desc = np.stack([lanes * (T + 1), lengths[lanes], np.zeros(len(lanes))])
    desc = torch.from_numpy(desc.astype(np.int32)).to(dev)
    n_seg = int(desc.shape[1])
    batch_norm = normalize == "batch"
    scratch = torch.empty(2 * n_seg + 2, dtype=torch.float64, device=dev) if batch_norm else None
    weights = torch.full((E, T), float("nan"), dtype=torch.float64, device=dev)
    cur, last, recomputed = first, None, 0
    table = torch.zeros(B.n_table_rows, device=dev) if mbn is not None else None
    stats = torch.zeros(3 * -(-n_valid // batch), dtype=torch.float64, device=dev) if mbn is not None else None
    for epoch in range(epochs):
        if epoch > 0:
            d.values_idx(B.states, rows, int(rows.numel()), values_now)
            d.logp_idx(B.states, B.actions, valid_dev, n_valid, logp_now)
            if continuous:
                d.values_idx(final_states, trunc_rows, int(trunc_rows.numel()), fv_now)
            last = nan3()
            L.mi_rollout_finish_vtrace(st, values_now.data_ptr(), logp_now.data_ptr(), lp.data_ptr(), r.data_ptr(), dn.data_ptr(), desc[0].data_ptr(), desc[1].data_ptr(),
                                       n_seg, E, T, GAMMA, LAM, bars[0], bars[1], 0 if continuous else 1, 1 if batch_norm else 0, milib.ptr(scratch),
                                       B.returns.data_ptr(), B.advantages.data_ptr(), last[0].data_ptr(), last[1].data_ptr(), last[2].data_ptr(), weights.data_ptr(),
                                       fv_now.data_ptr() if continuous else None, desc[2].data_ptr() if continuous else None)
            cur, recomputed = last, recomputed + 1
        idx = np.arange(n_valid)
        np.random.shuffle(idx)
        perm = torch.from_numpy(valid[idx]).to(dev)
        adv = B.advantages
        if mbn is not None:
            L.mi_ppo_minibatch_advantages(st, cur[0].data_ptr(), perm.data_ptr(), n_valid, batch, E, T, mbn, table.data_ptr(), stats.data_ptr())
            adv = table
        for i in range(0, n_valid, batch):
            mb = perm[i:i + batch]
            n = int(mb.numel())
            m._step_rows(B.states, B.actions, B.returns, adv, lp, mb, n, n, **({"old_values_all": B.values} if vclip else {}))
            m.train_step_counter += 1
    torch.cuda.synchronize()
    return dict(values_now=values_now, logp_now=logp_now, first=first.cpu().numpy(), last=None if last is None else last.cpu().numpy(),
                weights=weights.cpu().numpy(), recomputed=recomputed)


SHAPES = rg.SHAPES                                                                   # (E, T, batch size) = (3, 5, 4), (5, 20, 7)
CLASSES = rg.CLASSES


def check_result(A, out, ref, bars):
    for i, k in enumerate(("raw_advantages", "returns", "advantages")):
        assert np.array_equal(out[k], ref["first"][i], equal_nan=True) and np.array_equal(out["refreshed_" + k], ref["last"][i], equal_nan=True), k
    w = out["refreshed_importance_weights"]
    rec = np.arange(A.horizon)[None, :] < A.rows.lengths[:, None]
    assert w.dtype == np.float64 and np.array_equal(w, ref["weights"], equal_nan=True) and np.isnan(w[~rec]).all() and not np.isnan(w[rec]).any()
    assert out["vtrace_rho_clip_fraction"] == float((w[rec] > bars[0]).mean()) and out["vtrace_c_clip_fraction"] == float((w[rec] > bars[1]).mean())


THREE_EPOCHS = [(c, E, T, b, "segment") for c in (False, True) for E, T, b in SHAPES] + [(True, 3, 5, 4, "batch")]      # normalize="batch": ContinuousRolloutBuffer, once


@pytest.mark.parametrize("continuous,E,T,batch,normalize", THREE_EPOCHS,
                         ids=["%s-%dx%d-%s" % ("ContinuousRolloutBuffer" if c else "RolloutBuffer", E, T, n) for c, E, T, _, n in THREE_EPOCHS])
def test_three_epochs_are_the_host_loop(vae, tmp_path, continuous, E, T, batch, normalize):
    import torch
    A, m_a = make(vae, tmp_path / "a", continuous, E, T)
    B, m_b = make(vae, tmp_path / "b", continuous, E, T, bars=None, recompute=False)
    A.logp_now, pad = rg.padded(torch.zeros(A.n_table_rows, device=A.device))
    rg.collect(A, 71 + E, continuous)
    rg.copy_collection(A, B)
    kw = dict(normalize=normalize) if continuous else {}
    np.random.seed(5)
    out = A.update(GAMMA, LAM, num_epochs=3, batch_size=batch, **kw)
    np.random.seed(5)
    ref = vt_host_loop(B, m_b, continuous, 3, batch, BARS, final_states=getattr(A, "final_states", None), **kw)
    assert bitwise(flat_state(m_a), flat_state(m_b)) and out["recomputed_epochs"] == 2 == ref["recomputed"]
    assert bitwise([A.values_now, A.logp_now, A.returns, A.advantages], [ref["values_now"], ref["logp_now"], B.returns, B.advantages])
    check_result(A, out, ref, BARS)
    w = out["refreshed_importance_weights"]
    print("%s %dx%d %s: weights of the last refresh in [%.4f, %.4f], clip fractions rho %.3f c %.3f"
          % (type(A).__name__, E, T, normalize, np.nanmin(w), np.nanmax(w), out["vtrace_rho_clip_fraction"], out["vtrace_c_clip_fraction"]))
    assert not np.all(w[~np.isnan(w)] == 1.0)                                        # the policy has moved
    assert out["vtrace_rho_clip_fraction"] > 0.0 and 0.0 < out["vtrace_c_clip_fraction"] < 1.0      # ... far enough for both bars to truncate, and not everywhere
    assert bool((pad == SENTINEL).all())


@pytest.mark.parametrize("E,T,batch", SHAPES)
@CLASSES
def test_one_epoch_is_the_setting_off(vae, tmp_path, continuous, E, T, batch):
    A, m_a = make(vae, tmp_path / "a", continuous, E, T)
    C, m_c = make(vae, tmp_path / "c", continuous, E, T, bars=None, recompute=False)
    rg.collect(A, 71 + E, continuous)
    rg.copy_collection(A, C)
    np.random.seed(5)
    out_a = A.update(GAMMA, LAM, num_epochs=1, batch_size=batch)
    np.random.seed(5)
    out_c = C.update(GAMMA, LAM, num_epochs=1, batch_size=batch)
    assert bitwise(flat_state(m_a), flat_state(m_c)) and out_a["losses"] == out_c["losses"]
    for k in ("returns", "advantages", "raw_advantages", "values"):
        assert np.array_equal(out_a[k], out_c[k], equal_nan=True), k
    assert bitwise([A.returns, A.advantages], [C.returns, C.advantages])
    assert out_a["recomputed_epochs"] == 0 and "refreshed_importance_weights" not in out_a and "vtrace_rho_clip_fraction" not in out_a


@pytest.mark.parametrize("E,T,batch", SHAPES)
@CLASSES
def test_at_learning_rate_zero_vtrace_is_recomputation_alone(vae, tmp_path, continuous, E, T, batch):
    """theta never moves, so log pi_theta is the cache bit for bit (the fifth contract of csrc/ppo_head.hpp), every weight is exactly 1.0 and, the bars being
    >= 1, the refreshed tables are those of the GAE refresh."""
    A, m_a = make(vae, tmp_path / "a", continuous, E, T, bars=(1.0, 1.0), learning_rate=0.0)
    C, m_c = make(vae, tmp_path / "c", continuous, E, T, bars=None, learning_rate=0.0)
    before = flat_state(m_a)[0]
    rg.collect(A, 71 + E, continuous)
    rg.copy_collection(A, C)
    if continuous:
        C.final_states.copy_(A.final_states)
    np.random.seed(5)
    out_a = A.update(GAMMA, LAM, num_epochs=3, batch_size=batch)
    np.random.seed(5)
    out_c = C.update(GAMMA, LAM, num_epochs=3, batch_size=batch)
    assert bitwise(flat_state(m_a)[0], before) and bitwise(flat_state(m_c)[0], before)
    assert out_a["recomputed_epochs"] == 2 == out_c["recomputed_epochs"]
    for k in ("refreshed_returns", "refreshed_raw_advantages", "refreshed_advantages", "refreshed_values"):
        assert np.array_equal(out_a[k], out_c[k], equal_nan=True), k
    w = out_a["refreshed_importance_weights"]
    assert np.all(w[~np.isnan(w)] == 1.0) and (~np.isnan(w)).sum() == A.rows.lengths.sum()
    assert out_a["vtrace_rho_clip_fraction"] == 0.0 == out_a["vtrace_c_clip_fraction"]
    assert bitwise([A.returns, A.advantages], [C.returns, C.advantages])


@pytest.mark.parametrize("setting", ["value_clip", "minibatch_norm"])
def test_other_settings_are_their_host_loop(vae, tmp_path, setting):
    E, T, batch = 3, 5, 4
    A, m_a = make(vae, tmp_path / "a", False, E, T)
    B, m_b = make(vae, tmp_path / "b", False, E, T, bars=None, recompute=False)
    kw = {}
    for buf, m in ((A, m_a), (B, m_b)):
        if setting == "value_clip":
            m.set_value_clip(0.02)
            kw = dict(vclip=True)
        else:
            buf.set_minibatch_normalization(ddof=1)
            kw = dict(mbn=1)
    rg.collect(A, 31, False)
    rg.copy_collection(A, B)
    np.random.seed(7)
    out = A.update(GAMMA, LAM, num_epochs=3, batch_size=batch)
    np.random.seed(7)
    ref = vt_host_loop(B, m_b, False, 3, batch, BARS, **kw)
    assert out["recomputed_epochs"] == 2 and bitwise(flat_state(m_a), flat_state(m_b)), setting
    assert bitwise([A.values_now, A.logp_now], [ref["values_now"], ref["logp_now"]])
    check_result(A, out, ref, BARS)


def test_diagnostics_with_a_kl_stop_are_the_host_loop(vae, tmp_path):
    """update_with_diagnostics with a target_kl between the KL of epoch 1 and that of epoch 2 (read from a run without a target on a third policy; the learning
    rates are tried from 1e-4 downwards until the KL grows from epoch 1 to epoch 2, as in the advantage-recomputation tests): two epochs, one refresh."""
    E, T, batch = 3, 5, 4
    for lr in (1e-4, 3e-5, 1e-5):
        P, m_p = make(vae, tmp_path / ("p%g" % lr), False, E, T, learning_rate=lr)
        A, m_a = make(vae, tmp_path / ("a%g" % lr), False, E, T, learning_rate=lr)
        B, m_b = make(vae, tmp_path / ("b%g" % lr), False, E, T, bars=None, recompute=False, learning_rate=lr)
        rg.collect(A, 31, False)
        rg.copy_collection(A, P)
        rg.copy_collection(A, B)
        np.random.seed(7)
        probe = P.update_with_diagnostics(GAMMA, LAM, num_epochs=3, batch_size=batch)
        kl = [e["approx_kl"] for e in probe["epochs"]]
        print("learning rate %g: approx_kl per epoch %s" % (lr, kl))
        if kl[0] < kl[1]:
            break
    assert probe["recomputed_epochs"] == 2 and kl[0] < kl[1], kl
    np.random.seed(7)
    out = A.update_with_diagnostics(GAMMA, LAM, num_epochs=3, batch_size=batch, target_kl=0.5 * (kl[0] + kl[1]))
    assert out["stopped_early"] and out["epochs_run"] == 2 and out["recomputed_epochs"] == 1 and out["epochs"] == probe["epochs"][:2]
    np.random.seed(7)
    ref = vt_host_loop(B, m_b, False, 2, batch, BARS)
    assert bitwise(flat_state(m_a), flat_state(m_b)) and bitwise([A.values_now, A.logp_now], [ref["values_now"], ref["logp_now"]])
    check_result(A, out, ref, BARS)


@CLASSES
def test_switching_vtrace_off_again(vae, tmp_path, continuous):
    E, T, batch = 3, 5, 4
    A, m_a = make(vae, tmp_path / "a", continuous, E, T)
    C, m_c = make(vae, tmp_path / "c", continuous, E, T, bars=None)
    A.set_vtrace(None)
    assert A._vtrace is None and A.logp_now is None
    rg.collect(A, 9, continuous)
    rg.copy_collection(A, C)
    if continuous:
        C.final_states.copy_(A.final_states)
    np.random.seed(3)
    out_a = A.update(GAMMA, LAM, num_epochs=3, batch_size=batch)
    np.random.seed(3)
    out_c = C.update(GAMMA, LAM, num_epochs=3, batch_size=batch)
    assert bitwise(flat_state(m_a), flat_state(m_c)) and out_a["losses"] == out_c["losses"] and sorted(out_a) == sorted(out_c)
    for k in ("refreshed_returns", "refreshed_advantages", "refreshed_raw_advantages", "refreshed_values"):
        assert np.array_equal(out_a[k], out_c[k], equal_nan=True), k
    assert A.logp_now is None and "refreshed_importance_weights" not in out_a


@CLASSES
def test_vtrace_without_recomputation_is_refused(vae, tmp_path, continuous):
    E, T = 3, 5
    A, m_a = make(vae, tmp_path / "a", continuous, E, T, recompute=False)
    for bad in (dict(rho_bar=0.0), dict(c_bar=-1.0), dict(rho_bar=float("nan")), dict(rho_bar=True)):
        with pytest.raises(ValueError, match="set_vtrace"):
            A.set_vtrace(**bad)
    assert A._vtrace == {"rho_bar": BARS[0], "c_bar": BARS[1]}
    rg.collect(A, 9, continuous)
    state = flat_state(m_a)
    tabs = [t.clone() for t in (A.states, A.actions, A.values, A.returns, A.advantages, A.logp_old)]
    with pytest.raises(ValueError, match="V-trace"):
        A.update(GAMMA, LAM, num_epochs=3, batch_size=4)
    assert bitwise(flat_state(m_a), state) and bitwise([A.states, A.actions, A.values, A.returns, A.advantages, A.logp_old], tabs)
    assert A.logp_now is None and A.values_now is None
