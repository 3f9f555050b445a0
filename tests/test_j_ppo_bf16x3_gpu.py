"""The split-bf16 ("bf16x3") precision mode of the PPO training step (mi_ppo_set_precision): the GEMM stages of the fused kernels on
v_mfma_f32_32x32x16_bf16 with fp32 operands split in registers.  Against the float64 oracle, with the fp32 oracle as the yardstick of what
fp32 arithmetic itself costs; bounds are written in each test."""
import ctypes
import os
import subprocess
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ppo_oracle as po  # noqa: E402
from oracle import vae_oracle as vo  # noqa: E402
from ppo import PPO, _adam_alpha  # noqa: E402
from mi355 import lib as milib  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HP = dict(learning_rate=1e-4, lr_decay=1.0, epsilon=0.2, value_scale=1.0, entropy_scale=0.01, initial_std=1.0)
KEYS = ("policy_loss", "value_loss", "entropy_loss", "loss", "ratio_mean")


def max_rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def model(tmp_path, precision, params, seed=2):
    m = PPO(np.array([67]), po.ActionSpace(), model_dir=str(tmp_path), seed=seed, precision=precision, **HP)
    m.set_weights(params)
    m.init_session(init_logging=False)
    return m


def near_kink(params, params_old, s, a, tau=1e-4, eps=0.2):
    """Samples at which the loss is not smooth within the split form's forward error (~1e-5 of each layer's max): a ReLU pre-activation of the policy or
    value trunk within tau x that layer's max |z| of zero, or a probability ratio within tau of a clip edge 1 +- eps.  On the other side of such a kink a
    sample's whole contribution to a gradient column switches on or off (the float64 emulation of this mode's forward puts one value-trunk unit across it
    in the M = 256 draw below): a discontinuity, not the arithmetic this file measures, so such samples are not drawn."""
    t = lambda p: {k: torch.from_numpy(np.asarray(v, np.float64)) for k, v in p.items()}      # noqa: E731
    th, tho, x = t(params), t(params_old), torch.from_numpy(s.astype(np.float64))
    bad = torch.zeros(len(s), dtype=torch.bool)
    for k1, k2 in (("policy/dense", "policy/dense_1"), ("policy/dense_2", "policy/dense_3")):
        z1 = x @ th[k1 + "/kernel"] + th[k1 + "/bias"]
        z2 = torch.relu(z1) @ th[k2 + "/kernel"] + th[k2 + "/bias"]
        for z in (z1, z2):
            bad |= (z.abs() < tau * z.abs().max()).any(1)
    sp = po.ActionSpace()
    mean, ls, _ = po.policy_forward(th, x, sp.low, sp.high)
    mean_o, ls_o, _ = po.policy_forward(tho, x, sp.low, sp.high, scope="policy_old")
    act = torch.from_numpy(a.astype(np.float64))
    r = torch.exp(po.normal_log_prob(act, mean, ls).sum(1) - po.normal_log_prob(act, mean_o, ls_o).sum(1))
    bad |= ((r - (1 + eps)).abs() < tau) | ((r - (1 - eps)).abs() < tau)
    return bad.numpy()


def problem(M, seed=2):
    """theta != theta_old (ratio != 1, some samples clipped), as in the fp32 fused-step test; the fp32 and float64 oracles on the same parameters;
    M samples away from the loss's kinks (near_kink)."""
    o = po.OraclePPO([67], po.ActionSpace(), seed=seed, **HP)
    init = {k: v.copy() for k, v in o.params.items()}
    rng = np.random.RandomState(5 + M)
    for k in o.params:
        o.params[k] = o.params[k] + (0.02 * rng.standard_normal(o.params[k].shape)).astype(np.float32)
    o64 = po.OraclePPO([67], po.ActionSpace(), seed=seed, dtype=torch.float64, **HP)
    o64.params = OrderedDict((k, v.copy()) for k, v in o.params.items())
    o64.params_old = OrderedDict((k, v.copy()) for k, v in o.params_old.items())
    n = 3 * M
    s = (0.5 * rng.standard_normal((n, 67))).astype(np.float32)
    a = np.stack([rng.uniform(-1, 1, n), rng.uniform(0, 1, n)], axis=1).astype(np.float32)
    R, A = rng.randn(n).astype(np.float32), rng.randn(n).astype(np.float32)
    keep = np.flatnonzero(~near_kink(o.params, o.params_old, s, a))[:M]
    assert len(keep) == M
    return o, o64, init, (s[keep], a[keep], R[keep], A[keep])


def setup(tmp_path, M, precision="bf16x3"):
    o, o64, init, (s, a, R, A) = problem(M)
    m = model(tmp_path, precision, init)
    m.dev.load_params(o.params)                          # theta only; theta_old stays the initial copy
    dt = (m._to_dev(s, (M, 67)), m._to_dev(a, (M, 2)), m._to_dev(R, (M,)), m._to_dev(A, (M,)))
    return o, o64, m, (s, a, R, A), dt


def used_mask(d):
    used = torch.zeros(d.n_flat, dtype=torch.bool, device=d.device)
    for _, (o_, s_) in d.layout.items():
        used[o_:o_ + s_] = True
    return used


@pytest.mark.parametrize("M", [32, 77, 256, 2048])
def test_bf16x3_gradient_pass_against_float64(tmp_path, M):
    """Five loss scalars within 1e-4 relative of float64; each of the 13 gradients within max(1e-3, 4 x the fp32 oracle's own distance from float64) of its
    tensor max.  At M = 2048 the mode is really taken: the gradients are not bitwise those of the fp32 mode."""
    o, o64, m, (s, a, R, A), (sd, ad, Rd, Ad) = setup(tmp_path, M)
    assert m.precision == "bf16x3" and m.dev.engine_precision() == milib.MI_BF16X3
    scal64, g64 = o64.loss_and_grads(s, a, R, A)
    _, g32 = o.loss_and_grads(s, a, R, A)
    d = m.dev
    d.forward_backward(sd, ad, Rd, Ad, M, 1.0 / M, 1.0)
    L = d.losses.cpu().numpy()
    g = d.export_grads()
    print("\nbf16x3 gradient pass, M = %d: loss scalars (relative to float64)" % M)
    for got, key in zip(L, KEYS):
        print("  %-13s %.3e" % (key, abs(got - scal64[key]) / max(abs(scal64[key]), 1e-30)))
        assert got == pytest.approx(scal64[key], rel=1e-4, abs=1e-6), (key, got, scal64[key])
    print("  gradient max error / tensor max (device bf16x3, fp32 oracle):")
    bad = {}
    for k in g64:
        e_d, e_o = max_rel(g[k], g64[k]), max_rel(g32[k], g64[k])
        print("  %-34s %.3e  %.3e" % (k, e_d, e_o))
        if e_d > max(1e-3, 4.0 * e_o):
            bad[k] = (e_d, e_o)
    assert not bad, bad
    if M == 2048:
        m32 = model(tmp_path / "fp32", "fp32", po.OraclePPO([67], po.ActionSpace(), seed=2, **HP).params)
        m32.dev.load_params(o.params)
        m32.dev.forward_backward(sd, ad, Rd, Ad, M, 1.0 / M, 1.0)
        used = used_mask(d)
        assert m32.dev.engine_precision() == milib.MI_F32
        assert not torch.equal(m32.dev.grads[used], d.grads[used])


def test_bf16x3_mode_survives_engine_growth(tmp_path):
    """ensure_batch() recreates the engine for a larger batch: the mode is applied to the new engine (and to the 2048-row gradient pass it runs)."""
    from mi355.ppo_device import PpoDevice
    o, o64, m, _, (sd, ad, Rd, Ad) = setup(tmp_path, 2048)
    sp = po.ActionSpace()
    d = PpoDevice(67, 2, sp.low, sp.high, 0.2, 1.0, 0.01, max_batch=32, precision="bf16x3")
    assert d.max_batch == 32 and d.engine_precision() == milib.MI_BF16X3
    d.params.copy_(m.dev.params)
    d.params_old.copy_(m.dev.params_old)
    d.ensure_batch(2048)
    assert d.max_batch >= 2048 and d.engine_precision() == milib.MI_BF16X3
    d.forward_backward(sd, ad, Rd, Ad, 2048, 1.0 / 2048, 1.0)
    m.dev.forward_backward(sd, ad, Rd, Ad, 2048, 1.0 / 2048, 1.0)
    used = used_mask(d)
    assert torch.equal(d.grads[used], m.dev.grads[used])
    # MI_BF16 has no PPO form; the refused call leaves the mode alone
    assert d.L.cdll.mi_ppo_set_precision(d.handle, milib.MI_BF16) == -1
    assert d.engine_precision() == milib.MI_BF16X3
    d.close()


@pytest.mark.parametrize("M", [77, 2048])
def test_bf16x3_gradient_pass_is_reproducible(tmp_path, M):
    """Two bf16x3 gradient passes are bitwise equal, garbage in the gradient buffer in between (no atomics: fixed-order slab sums above 256 rows)."""
    _, _, m, _, (sd, ad, Rd, Ad) = setup(tmp_path, M)
    d = m.dev
    d.forward_backward(sd, ad, Rd, Ad, M, 1.0 / M, 1.0)
    first = d.grads.clone()
    d.grads.fill_(4.25)
    d.forward_backward(sd, ad, Rd, Ad, M, 1.0 / M, 1.0)
    used = used_mask(d)
    assert torch.equal(d.grads[used], first[used])


@pytest.mark.parametrize("M", [32, 256, 2048])
def test_bf16x3_one_call_steps_match_the_oracle_adam(tmp_path, M):
    """train_step and train_step_idx against the oracle's TF-Adam on its own gradients: atol 2e-6 where |g| > 1e-3 of the tensor max, no element moves
    more than 1.01 lr; the step with the cached log pi_old (mi_ppo_logp_old, same mode) matches the step without it to 1e-7 wherever |g| > 1e-6.  (The
    cache's head sums in another order than the loss kernel's: log pi_old differs in the last bits, so does every gradient, and an element whose gradient
    is at Adam's epsilon scale, ~1e-8, can change sign and move by a few lr / 100 -- in either precision mode.)"""
    o, _, m, (s, a, R, A), (sd, ad, Rd, Ad) = setup(tmp_path, M)
    d = m.dev
    _, grads = o.loss_and_grads(s, a, R, A)
    before = {k: v.copy() for k, v in o.params.items()}
    want = {k: v.copy() for k, v in before.items()}
    adam = vo.AdamTF({k: v.shape for k, v in before.items()})
    adam.step(want, grads, 1e-4)
    alpha = _adam_alpha(1e-4, 0.9, 0.999)
    perm = np.random.RandomState(M).permutation(M)
    inv = torch.from_numpy(np.argsort(perm).astype(np.int32)).to(d.device)           # table row of minibatch sample i: the tables hold the samples permuted
    tables = [t[torch.from_numpy(perm).to(d.device)].contiguous() for t in (sd, ad, Rd, Ad)]
    results = {}
    for form in ("train_step", "train_step_idx", "cached"):
        d.load_params(before)
        d.adam_m.zero_(); d.adam_v.zero_()
        if form == "train_step":
            d.train_step(sd, ad, Rd, Ad, M, 1.0 / M, 1.0, alpha)
        elif form == "train_step_idx":
            d.train_step_idx(*tables, None, inv, M, 1.0 / M, 1.0, alpha)
        else:
            lp = torch.empty(M, device=d.device)
            d.logp_old(sd, ad, M, lp)
            d.train_step(sd, ad, Rd, Ad, M, 1.0 / M, 1.0, alpha, logp_old=lp)
        got = d.export_params()
        results[form] = got
        for k in want:
            sig = np.abs(grads[k]) > 1e-3 * np.abs(grads[k]).max()
            assert np.allclose(got[k][sig], want[k][sig], rtol=0, atol=2e-6), (form, k, float(np.abs(got[k][sig] - want[k][sig]).max()))
            assert np.abs(got[k] - before[k]).max() <= 1.01e-4, (form, k)
    for k in results["train_step"]:
        diff = np.abs(results["cached"][k] - results["train_step"][k])
        sig = np.abs(grads[k]) > 1e-6
        if (diff > 1e-7).any():
            print("  cached vs uncached, %s: %d elements > 1e-7 (max %.2e), largest |g| among them %.2e" % (k, int((diff > 1e-7).sum()), diff.max(), np.abs(grads[k])[diff > 1e-7].max()))
        assert (diff[sig] <= 1e-7).all(), k


@pytest.mark.parametrize("M", [77, 2048])
def test_bf16x3_data_parallel_form_leaves_the_single_rank_gradients(tmp_path, M):
    """train_step_dp at world size 1 on the recording communicator (the collective recorded, the buffer left alone) feeds Adam the gradient buffer of the
    single-rank gradient pass, bitwise.  The flat Adam clears that buffer, so it is read through what Adam made of it: from zero moments m = 0.1 g, and the
    parameters, moments of the one-call form equal those of the host sequence (gradient pass, then mi_ppo_apply_adam) bit for bit."""
    _, _, m, _, (sd, ad, Rd, Ad) = setup(tmp_path, M)
    d = m.dev
    start = d.params.clone()
    alpha = _adam_alpha(1e-4, 0.9, 0.999)
    d.adam_m.zero_(); d.adam_v.zero_()
    d.forward_backward(sd, ad, Rd, Ad, M, 1.0 / M, 1.0)
    d.apply_adam(alpha)
    want = (d.params.clone(), d.adam_m.clone(), d.adam_v.clone())
    d.params.copy_(start)
    d.adam_m.zero_(); d.adam_v.zero_()
    d.grads.fill_(-3.5)
    log = np.zeros((8, 4), np.int64)
    h = ctypes.c_void_p()
    d.L.mi_comm_init_recording(ctypes.addressof(h), 0, 1, log.ctypes.data, 8)
    try:
        d.train_step_dp(h, sd, ad, Rd, Ad, None, None, M, 1.0 / M, 1.0, alpha)
        torch.cuda.synchronize()
        assert d.L.mi_comm_recorded(h) >= 0                       # (a recording communicator: -1 would be a real one)
    finally:
        d.L.mi_comm_destroy(h)
    used = used_mask(d)
    for got, ref in zip((d.params, d.adam_m, d.adam_v), want):
        assert torch.equal(got[used], ref[used])
    assert bool((d.adam_m[used] != 0).any())


def _c3_update(m, s_arr, a_arr, returns, advantages, epochs=4):
    np.random.seed(0)
    m.update_old_policy()
    for mb in po.minibatch_schedule(128, 32, epochs):
        m.train(s_arr[mb], a_arr[mb], returns[mb], advantages[mb])
    return m.dev.export_params()


def test_bf16x3_c3_trajectory_no_further_from_float64_than_twice_fp32(tmp_path):
    """A C3-shaped update (horizon 128, 4 epochs x 4 minibatches of 32) in bf16x3 ends no further from the float64 oracle's trajectory than 2 x the fp32
    mode's distance (per-tensor RMS of the update error, floor 2e-4 of the update scale: the rule of the fp32 tests)."""
    o = po.OraclePPO([67], po.ActionSpace(), seed=2, **HP)
    p0 = {k: v.copy() for k, v in o.params.items()}
    rng = np.random.RandomState(7)
    T = 128
    s_arr = (0.5 * rng.standard_normal((T, 67))).astype(np.float32)
    s_arr[:, 64] = rng.uniform(-1, 1, T); s_arr[:, 65] = rng.uniform(0, 1, T); s_arr[:, 66] = rng.uniform(0, 30, T)
    a_arr = np.stack([rng.uniform(-1, 1, T), rng.uniform(0, 1, T)], axis=1).astype(np.float32)
    returns, advantages = rng.randn(T), rng.randn(T)
    advantages = (advantages - advantages.mean()) / (advantages.std() + 1e-8)
    got = {p: _c3_update(model(tmp_path / p, p, p0), s_arr, a_arr, returns, advantages) for p in ("fp32", "bf16x3")}
    # the float64 trajectory: losses, gradients and the Adam recurrence in float64 on the same minibatches
    ex = OrderedDict((k, v.astype(np.float64)) for k, v in p0.items())
    adam64 = po.AdamTF(OrderedDict((k, v.shape) for k, v in ex.items()), dtype=np.float64)
    ex_old = {k.replace("policy/", "policy_old/", 1): torch.from_numpy(v.copy()) for k, v in ex.items()}
    t64 = lambda x: torch.from_numpy(np.asarray(x, np.float32).astype(np.float64))     # noqa: E731
    np.random.seed(0)
    for mb in po.minibatch_schedule(T, 32, 4):
        pt = OrderedDict((k, torch.from_numpy(v.copy()).requires_grad_(True)) for k, v in ex.items())
        L64 = po.ppo_losses(pt, ex_old, t64(s_arr[mb]), t64(a_arr[mb]), t64(returns[mb]), t64(advantages[mb]), o.low, o.high, 0.2, 1.0, 0.01)
        L64["loss"].backward()
        adam64.step(ex, {k: v.grad.numpy() for k, v in pt.items()}, 1e-4)
    print("\nC3 update, RMS update error / max |update| vs the float64 trajectory (bf16x3, fp32):")
    for k in p0:
        upd_x = ex[k] - p0[k].astype(np.float64)
        scale = max(np.abs(upd_x).max(), 1e-12)
        e = {p: np.sqrt(np.mean(((got[p][k].astype(np.float64) - p0[k]) - upd_x) ** 2)) for p in got}
        print("  %-34s %.3e  %.3e" % (k, e["bf16x3"] / scale, e["fp32"] / scale))
        assert e["bf16x3"] <= 2.0 * e["fp32"] + 2e-4 * scale, (k, e["bf16x3"] / scale, e["fp32"] / scale)


def test_bf16x3_checkpoint_loads_into_an_fp32_model(tmp_path):
    """The precision is not part of a checkpoint: train in bf16x3, save(), load_latest_checkpoint() into an fp32 PPO -- identical parameters."""
    o = po.OraclePPO([67], po.ActionSpace(), seed=2, **HP)
    m = model(tmp_path / "run", "bf16x3", o.params)
    rng = np.random.RandomState(3)
    for _ in range(3):
        m.train((0.5 * rng.standard_normal((32, 67))).astype(np.float32), rng.uniform(0, 1, (32, 2)).astype(np.float32), rng.randn(32), rng.randn(32))
    m.save()
    m2 = PPO(np.array([67]), po.ActionSpace(), model_dir=str(tmp_path / "run"), seed=9, precision="fp32", **HP)
    m2.init_session(init_logging=False)
    assert m2.load_latest_checkpoint()
    assert m2.precision == "fp32" and m2.dev.engine_precision() == milib.MI_F32
    a, b = m.dev.export_params(), m2.dev.export_params()
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert m2.get_train_step_idx() == 3


def test_bf16x3_never_falls_back_to_fp32(tmp_path):
    """With the fused kernels switched off (MI355_PPO_FUSED=0, read once per process: a child process) init_session() of a bf16x3 PPO raises; fp32 still runs."""
    code = ("import sys, numpy as np\n"
            "sys.path[:0] = [%r, %r]\n"
            "from oracle import ppo_oracle as po\n"
            "from ppo import PPO\n"
            "from mi355 import lib as milib\n"
            "PPO(np.array([67]), po.ActionSpace(), model_dir=%r, seed=1, precision='fp32').init_session(init_logging=False)\n"
            "m = PPO(np.array([67]), po.ActionSpace(), model_dir=%r, seed=1, precision='bf16x3')\n"
            "try:\n"
            "    m.init_session(init_logging=False)\n"
            "except milib.MiError as e:\n"
            "    print('REFUSED', e); sys.exit(0)\n"
            "print('RAN'); sys.exit(3)\n") % (os.path.join(ROOT, "carla-ppo_amd"), ROOT, str(tmp_path / "a"), str(tmp_path / "b"))
    env = dict(os.environ, MI355_PPO_FUSED="0")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "REFUSED" in r.stdout and "fused kernels" in r.stdout, r.stdout
