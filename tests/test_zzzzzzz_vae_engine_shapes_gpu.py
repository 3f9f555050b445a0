"""The ConvVAE ENGINE (csrc/vae_engine.hip) against float64 OFF the one model every other test builds: nine geometries / latent widths / batches
(tests/vae_engine_cases.py) that take the host gates of run_encoder, run_decoder, mi_vae_forward, mi_vae_backward and the rollout entries down every branch.

A  one whole step of the fp32 and bf16x3 engines against the float64 oracle: losses 1e-4, posterior mean 1e-4 of max, all 22 gradient tensors 2e-4 (fp32) / 1e-2
   (bf16x3) of each tensor's max, parameters after Adam within 2e-6 of AdamTF on the device's own gradients where |g| > 1e-3 of max, encode / reconstruct / generate
   1e-4 of max, padding floats of the gradient buffer 0.
B  the bf16 engine: forward against the oracle's bf16-storage emulation, then every layer against the float64 statement of that one op on the engine's OWN stored
   tensors (mi_vae_buffer 20..60); uint8 frame tables bitwise the float tables.
C  identities: two runs bitwise, one-call step = forward + backward + Adam, backward in parts, the data-parallel step on a recording communicator, workspace guards
   (child process), inference-only engine bitwise the training engine.
D  z_dim = 12 (fp32 / bf16x3 only) through A's assertions.
E  the rollout step entries on another ConvVAE.

Every bound is the project's existing one for that quantity (README tolerance table) or stated in vae_engine_cases.py.  Measured deviations are printed (pytest -s)
as `MEASURE case precision | what | achieved | bound`: profiles/r30_vae_engine_shapes.md."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import vae_engine_cases as vc  # noqa: E402
from hip_helpers import split_decode  # noqa: E402
from mi355 import lib as milib  # noqa: E402
from oracle import vae_oracle as vo  # noqa: E402

PATTERN16, PATTERN32 = 0x4BAD, 0x4BAD4BAD      # what a stored-tensor region holds before a pass: a region still full of it was never written


def measure(c, precision, what, achieved, bound):
    fmt = lambda v: "/".join("%.3e" % x for x in v) if isinstance(v, tuple) else ("%.3e" % v if isinstance(v, float) else str(v))   # noqa: E731
    print("MEASURE case %d %s | %s | %s | %s" % (c.id, precision, what, fmt(achieved), fmt(bound)))


# ---------------------------------------------------------------------------------------------------------------------------------------
# engines: one per (case, precision, loss, mode), built once; every engine is released before the next precision's are built
# ---------------------------------------------------------------------------------------------------------------------------------------
class Zoo:
    def __init__(self, root):
        self.root, self.precision, self.models = root, None, {}

    def release(self):
        for m in self.models.values():
            m.dev.close()
        self.models.clear()
        torch.cuda.empty_cache()

    def get(self, c, precision, loss_fn="bce", kl_tolerance=0.0, training=True):
        from vae.models import ConvVAE
        if precision != self.precision:
            self.release()
            self.precision = precision
        key = (c.id, loss_fn, kl_tolerance, training)
        if key not in self.models:
            m = ConvVAE(np.array(vc.src_shape(c)), np.array(vc.tgt_shape(c)), z_dim=c.z, model_dir=str(self.root / ("%d_%s_%s_%d" % (c.id, precision, loss_fn, training))),
                        precision=precision, loss_fn=loss_fn, kl_tolerance=kl_tolerance, training=training, seed=0)
            m.set_weights(vc.params(c))
            if c.id in vc.CREATE_BATCH:                    # created small, grown by ensure_batch inside the first pass
                make = m._make_device
                m._make_device = lambda max_batch: make(vc.CREATE_BATCH[c.id])
            m.init_session(init_logging=False)
            self.models[key] = m
        return self.models[key]


@pytest.fixture(scope="module")
def zoo(tmp_path_factory):
    z = Zoo(tmp_path_factory.mktemp("vae_engine_shapes"))
    yield z
    z.release()


def reset(m, c):
    """Back to the case's parameters, zero Adam slots and gradient buffer, first-step bias corrections."""
    from vae.models import ADAM_BETA1, ADAM_BETA2
    dev = m.dev
    dev.load_params(vc.params(c))
    for t in (dev.grads, dev.adam_m, dev.adam_v):
        t.zero_()
    m.beta1_power, m.beta2_power = np.float32(ADAM_BETA1), np.float32(ADAM_BETA2)
    torch.cuda.synchronize()


def tables(m, c, u8=False):
    d = vc.inputs(c)
    dev = m.dev
    if u8:
        src = torch.from_numpy(d["src_u8"].reshape(c.B, -1)).to(dev.device)
        tgt = torch.from_numpy(d["tgt_u8"].reshape(c.B, -1)).to(dev.device)
    else:
        src = m._frames(d["src"], int(np.prod(vc.src_shape(c))), "src")
        tgt = m._frames(d["tgt"], dev.P, "tgt")
    return src, tgt, m._eps(c.B, d["eps"])


def _plant(t):
    if t is not None:
        (t.view(torch.int16).fill_(PATTERN16) if t.element_size() == 2 else t.view(torch.int32).fill_(PATTERN32))


def _untouched(t):
    v = t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)
    same = int((v == (PATTERN16 if t.element_size() == 2 else PATTERN32)).sum())
    assert same == v.numel() or same < 0.01 * v.numel(), (same, v.numel())      # a region is written whole or not at all
    return same == v.numel()


def _f64(t):
    if t is None:
        return None
    if t.dtype == torch.int32:
        return split_decode(t.cpu().numpy())
    return t.float().cpu().numpy().astype(np.float64)


def observed_route(m, c):
    """Which of the skippable stored tensors the last forward + backward wrote: (decoder tail, head backward)."""
    dev = m.dev
    logits, dlogits, g1 = (not _untouched(dev.stored("dec", 4, c.B))), (not _untouched(dev.stored("gdec", 4, c.B))), (not _untouched(dev.stored("gact", 1, c.B)))
    tail = "plain" if logits else ("epilogue" if dlogits else "fused")
    assert not (logits and not dlogits)
    return tail, ("layer ops" if g1 else "fused")


def run_step(m, c, u8=False, grab=False):
    """forward + backward(part 0) + Adam from the case's parameters.  -> dict(losses, mean, flat gradient buffer, gradients, parameters after, route[, stored])."""
    reset(m, c)
    dev, B = m.dev, c.B
    src, tgt, e = tables(m, c, u8)
    dev.ensure_batch(B)                                # (case 9: the engine grows here; the regions below belong to the engine that runs the pass)
    if dev.max_batch != B and c.id in vc.CREATE_BATCH:
        raise AssertionError("the engine of case %d was not re-created for batch %d" % (c.id, B))
    for name, i in (("dec", 4), ("gdec", 4), ("gact", 1)):
        _plant(dev.stored(name, i, B))
    dev.forward(src, tgt, None, B, 1.0 / B, e, 1, 1)
    out = {"losses": dev.losses.cpu().numpy().copy(), "mean": dev._view(1, B * c.z).cpu().numpy().reshape(B, c.z).copy()}
    dev.backward(src, None, e, 1.0 / B, 0)
    torch.cuda.synchronize()
    out["flat"] = dev.grads.cpu().numpy().copy()
    out["grads"] = dev._from_flat(out["flat"])
    out["route"] = observed_route(m, c)
    if grab:
        st = {"%s%d" % (n, i): _f64(dev.stored(n, i, B)) for n, idx in (("act", range(1, 5)), ("dec", range(5)), ("gact", range(1, 5)), ("gdec", range(5))) for i in idx}
        st["dheads"] = _f64(dev.stored("dheads", 0, B))
        st["z"] = _f64(dev._view(5, B * c.z, torch.bfloat16)).reshape(B, c.z)
        st["mean"], st["logvar"] = out["mean"].astype(np.float64), dev._view(2, B * c.z).cpu().numpy().reshape(B, c.z).astype(np.float64)
        out["stored"] = st
    m._adam_step()
    torch.cuda.synchronize()
    out["after"] = dev.export_params()
    out["slots"] = (dev.adam_m.cpu().numpy().copy(), dev.adam_v.cpu().numpy().copy())
    out["params_flat"] = dev.params.cpu().numpy().copy()
    return out


def infer(m, c):
    d, dev, B = vc.inputs(c), m.dev, c.B
    src = m._frames(d["src"], int(np.prod(vc.src_shape(c))), "src")
    mean, rec, gen = torch.empty(B, c.z, device=dev.device), torch.empty(B, dev.P, device=dev.device), torch.empty(B, dev.P, device=dev.device)
    dev.encode(src, None, B, mean)
    dev.reconstruct(src, None, B, None, 0, rec)
    dev.decode(torch.from_numpy(d["eps"]).to(dev.device), B, gen)
    torch.cuda.synchronize()
    return mean.cpu().numpy(), rec.cpu().numpy(), gen.cpu().numpy()


def check_step(m, c, precision, loss_fn="bce", kl_tolerance=0.0, env=None):
    """env: the tuning knobs this process runs under, off their defaults (vae_engine_cases.route; tests/knob_route_worker.py)."""
    ref = vc.reference(c, loss_fn=loss_fn, kl_tolerance=kl_tolerance)
    got = run_step(m, c)
    rows, bad = vc.step_report(ref, float(got["losses"][0]), float(got["losses"][1]), got["mean"], got["grads"], precision)
    tag = precision if loss_fn == "bce" else "%s %s" % (precision, loss_fn)
    for name, val, bound in rows[:3]:
        measure(c, tag, name, float(val), bound)
    worst = max((r for r in rows if r[0].startswith("grad ")), key=lambda r: r[1])
    measure(c, tag, "worst gradient: " + worst[0][5:], float(worst[1]), worst[2])
    # the route the host gates chose is the one the case's row states
    want = vc.route(c, precision, max_batch=m.dev.max_batch, env=env)
    measure(c, tag, "route (tail, head backward)", "%s, %s" % got["route"], "%s, %s" % (want["tail"], want["head_bwd"]))
    assert got["route"] == (want["tail"], want["head_bwd"]), (got["route"], want)
    assert not bad, bad
    # padding floats between the tensors of the flat gradient buffer stay 0
    used = np.zeros(m.dev.n_flat, bool)
    for o, s in m.dev.layout.values():
        used[o:o + s] = True
    assert (~used).sum() > 0 and not got["flat"][~used].any()
    # the optimiser half: AdamTF applied to the DEVICE's gradients
    adam = vc.adam_report(vc.params(c), got["grads"], got["after"])
    k = max(adam, key=adam.get)
    measure(c, tag, "Adam vs AdamTF on device gradients, worst: " + k, adam[k], vc.ADAM_BOUND)
    assert adam[k] <= vc.ADAM_BOUND, adam
    return got


# ---------------------------------------------------------------------------------------------------------------------------------------
# Part A (and D's GPU half: z_dim = 12)
# ---------------------------------------------------------------------------------------------------------------------------------------
A_RUNS = [(c.id, "bce") for c in vc.CASES] + [(vc.Z12.id, "bce")] + [(i, k) for i in vc.LOSS_KIND_CASES for k in ("bce_v2", "mse")]


@pytest.mark.parametrize("cid,loss_fn", A_RUNS)
@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_one_step_against_float64(zoo, precision, cid, loss_fn):
    """Part A (and, as case 10, Part D's z_dim = 12): forward losses, posterior mean, all 22 gradient tensors and the Adam update of one whole step against the float64
    oracle; bce_v2 / mse run with kl_tolerance > 0 on one fused-epilogue and one plain tail (cases 1, 5).  No tensor is exempt: the fp32 oracle alone is within 2.8e-6
    of float64 on every tensor of every case (test_vae_engine_cases_host.py)."""
    c = vc.by_id(cid)
    tol = 0.0 if loss_fn == "bce" else vc.KL_TOLERANCE[cid]
    check_step(zoo.get(c, precision, loss_fn, tol), c, precision, loss_fn, tol)


@pytest.mark.parametrize("cid", [c.id for c in vc.CASES] + [vc.Z12.id])
@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_inference_surface_against_float64(zoo, precision, cid):
    """encode, reconstruct(sample = False) and generate_from_latent: 1e-4 of max against the float64 oracle."""
    c = vc.by_id(cid)
    m = zoo.get(c, precision)
    reset(m, c)
    ref = vc.inference_reference(c)
    for what, got, want in zip(("encode", "reconstruct", "generate_from_latent"), infer(m, c), (ref["mean"], ref["recon"], ref["gen"])):
        err = vc.rel_err(got, want)
        measure(c, precision, what + " / max", err, 1e-4)
        assert err < 1e-4, (what, err)


# ---------------------------------------------------------------------------------------------------------------------------------------
# Part B: the bf16 engine
# ---------------------------------------------------------------------------------------------------------------------------------------
def _route_none(st, rt):
    """The regions a fused route skips hold nothing of this pass."""
    st = dict(st)
    if rt["tail"] != "plain":
        st["dec4"] = None
    if rt["tail"] == "fused":
        st["gdec4"] = None
    if rt["head_bwd"] == "fused":
        st["gact1"] = None
    return st


def bf16_layer_by_layer(zoo, cid, env=None, slab="bf16", u8=None):
    """The body of test_bf16_engine_layer_by_layer_on_its_own_stored_tensors.  env, slab: the tuning knobs the process runs under and the slab kind they give the
    backward pass (tests/knob_route_worker.py; the defaults are a process without knobs); u8: also run the step on uint8 frame tables (None: cases 1 and 7)."""
    c = vc.by_id(cid)
    m = zoo.get(c, "bf16")
    got = run_step(m, c, grab=True)
    rt = vc.route(c, "bf16", max_batch=m.dev.max_batch, env=env)
    measure(c, "bf16", "route (tail, head backward)", "%s, %s" % got["route"], "%s, %s" % (rt["tail"], rt["head_bwd"]))
    assert got["route"] == (rt["tail"], rt["head_bwd"]), (got["route"], rt)
    emul, exact = vc.reference(c, dtype="f32", storage="bf16"), vc.reference(c)
    d_recon, d_mean = abs(got["losses"][0] / emul.recon - 1), vc.rel_err(got["mean"], emul.mean)
    kl_bound = 1.25 * abs(emul.kl - exact.kl) + 5e-3 * abs(exact.kl)
    measure(c, "bf16", "reconstruction loss vs emulation", float(d_recon), 2e-3)
    measure(c, "bf16", "posterior mean / max vs emulation", d_mean, 3e-2)
    measure(c, "bf16", "|kl - float64|", float(abs(got["losses"][1] - exact.kl)), float(kl_bound))
    assert d_recon < 2e-3 and d_mean < 3e-2 and abs(got["losses"][1] - exact.kl) <= kl_bound, (d_recon, d_mean, got["losses"][1], exact.kl, emul.kl)
    R = vc.layer_report(c, _route_none(got["stored"], rt), got["grads"], vc.params(c), vc.inputs(c), rt, slab=slab)
    for name, how, val, bound in R.rows:
        measure(c, "bf16", "%s (%s)" % (name, how), val, bound)
    assert not R.bad, R.bad
    assert len(R.rows) >= 41
    if cid in vc.PART_B_U8_CASES if u8 is None else u8:
        assert m.dev.accepts_u8
        u8 = run_step(m, c, u8=True, grab=True)
        assert np.array_equal(u8["losses"], got["losses"]) and np.array_equal(u8["flat"], got["flat"]) and np.array_equal(u8["params_flat"], got["params_flat"])
        for k, v in _route_none(got["stored"], rt).items():
            if v is not None:
                assert np.array_equal(u8["stored"][k], v), k
    return got


@pytest.mark.parametrize("cid", vc.PART_B_CASES)
def test_bf16_engine_layer_by_layer_on_its_own_stored_tensors(zoo, cid):
    """Part B.  Forward against the oracle's bf16-storage emulation: reconstruction loss 2e-3, posterior mean 3e-2 of max, KL within 1.25 x |emulation - float64| +
    5e-3 |float64|.  (The bf16 engine's GRADIENTS are not compared with the oracle at these batch sizes: the emulation itself is 19 % - 67 % of deconv1's kernel
    gradient away from float64 -- ReLU flips behind the bottleneck with few samples to average them.)  Instead, after one forward + backward, every layer is held
    against the float64 statement of that ONE op on the engine's own stored inputs (vae_engine_cases.layer_report): forward outputs and input gradients 4e-3 rel +
    4e-3 of max, filter gradients 2e-3 rms / 1e-2 max of the tensor's max, bias gradients 1e-4 of max more.  Cases 1 and 7: uint8 frame tables give bitwise the
    float tables' losses, stored tensors and gradients (as test_uint8_frame_tables_in_the_bf16_engine asserts at the model's shape)."""
    bf16_layer_by_layer(zoo, cid)


# ---------------------------------------------------------------------------------------------------------------------------------------
# Part C: identities
# ---------------------------------------------------------------------------------------------------------------------------------------
def _same_step(a, b):
    return np.array_equal(a["params_flat"], b["params_flat"]) and np.array_equal(a["slots"][0], b["slots"][0]) and np.array_equal(a["slots"][1], b["slots"][1]) and \
        np.array_equal(a["losses"], b["losses"])


@pytest.mark.parametrize("cid", vc.PART_C_CASES)
@pytest.mark.parametrize("precision", list(vc.PRECISIONS))
def test_step_identities(zoo, precision, cid):
    """Two runs of a step from the same parameters are bitwise equal in parameters, Adam slots and losses -- what the README promises of every training path without fp32
    atomics; case 5 takes the unfused mi_bce_logits_fwd_bwd_bias, but with FOUR target channels its fused dbias (the one fp32-atomic sum of the engine) is off
    (fuse_b4), so the promise is the plain one there too.  mi_vae_train_step in one call is bitwise forward + backward(0) + Adam.  The backward pass in parts 1, 3, 4
    gives part 0's gradient buffer BITWISE (every filter / bias gradient sums its splits in an order that is a function of the shape alone), and
    mi_vae_train_step_dp on a recording communicator is BITWISE the host loop forward + parts + Adam, logging the buckets of mi_vae_dp_buckets."""
    from vae.models import adam_alpha, ADAM_BETA1, ADAM_BETA2, ADAM_EPSILON
    L = milib.get()
    c = vc.by_id(cid)
    m = zoo.get(c, precision)
    dev, B = m.dev, c.B
    first, second = run_step(m, c), run_step(m, c)
    assert _same_step(first, second) and np.array_equal(first["flat"], second["flat"])
    assert np.abs(first["flat"]).max() > 0
    alpha = adam_alpha(vc.LR, np.float32(ADAM_BETA1), np.float32(ADAM_BETA2))
    src, tgt, e = tables(m, c)

    def state():
        torch.cuda.synchronize()
        return {"params_flat": dev.params.cpu().numpy().copy(), "slots": (dev.adam_m.cpu().numpy().copy(), dev.adam_v.cpu().numpy().copy()), "losses": dev.losses.cpu().numpy().copy()}

    # one C call
    reset(m, c)
    dev.train_step(src, tgt, None, B, 1.0 / B, e, alpha, ADAM_BETA1, ADAM_BETA2, ADAM_EPSILON)
    assert _same_step(state(), first)
    # backward in parts against part 0
    reset(m, c)
    dev.forward(src, tgt, None, B, 1.0 / B, e, 1, 1)
    for part, lo, hi in dev.grad_buckets:
        dev.backward(src, None, e, 1.0 / B, part=part)
    torch.cuda.synchronize()
    parts = dev._from_flat(dev.grads.cpu().numpy())
    errs = {k: vc.rel_err(parts[k], first["grads"][k]) for k in parts}
    measure(c, precision, "backward in parts 1, 3, 4 vs part 0, worst gradient / max", max(errs.values()), 0.0)
    assert np.array_equal(dev.grads.cpu().numpy(), first["flat"]), {k: v for k, v in errs.items() if not np.array_equal(parts[k], first["grads"][k])}
    dev.apply_adam(alpha, ADAM_BETA1, ADAM_BETA2, ADAM_EPSILON)
    host_loop = state()
    # the data-parallel step as one C call on a recording communicator
    reset(m, c)
    log = np.zeros((16, 4), np.int64)
    h = ctypes.c_void_p()
    L.mi_comm_init_recording(ctypes.addressof(h), 0, 2, log.ctypes.data, 16)
    try:
        dev.train_step_dp(h, src, tgt, None, B, 1.0 / B, e, alpha, ADAM_BETA1, ADAM_BETA2, ADAM_EPSILON)
        dp = state()
        n = L.mi_comm_recorded(h)
    finally:
        L.mi_comm_destroy(h)
    assert _same_step(dp, host_loop)
    bk = np.zeros(9, np.int64)
    L.mi_vae_dp_buckets(ctypes.byref(dev._desc(dev.max_batch)), bk.ctypes.data)
    want = [(1, int(bk[3 * i + 2] - bk[3 * i + 1]), 1, dev.grads.data_ptr() + 4 * int(bk[3 * i + 1])) for i in range(3)] + [(5, 3, 0, 0)]
    assert [tuple(int(x) for x in r) for r in log[:n]] == want
    assert [int(bk[3 * i]) for i in range(3)] == [1, 3, 4] == [p for p, _, _ in dev.grad_buckets]


@pytest.mark.parametrize("cid", vc.PART_C_CASES)
@pytest.mark.parametrize("precision", list(vc.PRECISIONS))
def test_inference_only_engine_is_bitwise_the_training_engine(zoo, precision, cid):
    """encode / reconstruct / generate_from_latent of an engine created with training = False (slim workspace, no conv1 output behind a fused encoder head) are bitwise
    the training engine's, as test_k_vae_inference_gpu.py asserts at 80 x 160; its gradient regions do not exist."""
    c = vc.by_id(cid)
    mt = zoo.get(c, precision)
    reset(mt, c)
    want = infer(mt, c)
    mi = zoo.get(c, precision, training=False)
    assert mi.dev.workspace.numel() < mt.dev.workspace.numel() // 4
    got = infer(mi, c)
    for what, a, b in zip(("encode", "reconstruct", "generate_from_latent"), got, want):
        assert np.array_equal(a, b), what
    assert mi.dev.stored("gact", 1, c.B) is None and mi.dev.stored("gdec", 4, c.B) is None and mi.dev.stored("dheads", 0, c.B) is None
    assert mi.dev.stored("act", 2, c.B) is not None and mi.dev.stored("dec", 4, c.B) is not None


def guard_run(cid):
    """Runs in the child (tests/vae_engine_guard_worker.py, MI355_DEBUG_GUARDS=1): a training step, encode, reconstruct and generate per precision -> guard counts."""
    import tempfile
    import pathlib
    assert os.environ.get("MI355_DEBUG_GUARDS") == "1"
    c = vc.by_id(cid)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        z = Zoo(pathlib.Path(tmp))
        for precision in vc.PRECISIONS:
            m = z.get(c, precision)
            n0, bad0, _ = m.dev.check_guards()
            run_step(m, c)
            infer(m, c)
            n, bad, _ = m.dev.check_guards()
            out[precision] = [n0, bad0, n, bad, m.dev.L.cdll.mi_last_error().decode() if bad else ""]
        z.release()
    return out


@pytest.mark.parametrize("cid", [1, 8])
def test_workspace_guards_stay_intact(cid):
    """MI355_DEBUG_GUARDS=1 in a fresh child process: 256 guard bytes behind every workspace region; after a training step, encode, reconstruct and generate on the
    smallest model and on the widest one (case 8: flat 10240, 2 z = 256, batch 1), in all three precisions, every guard still holds its pattern."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "vae_engine_guard_worker.py")
    r = subprocess.run([sys.executable, worker, str(cid)], env=dict(os.environ, MI355_DEBUG_GUARDS="1"), capture_output=True, text=True, timeout=150)
    assert r.returncode == 0, "exit status %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    out = json.loads([line for line in r.stdout.splitlines() if line.startswith("{")][-1])
    assert set(out) == set(vc.PRECISIONS)
    for precision, (n0, bad0, n, bad, msg) in out.items():
        assert n0 >= 30 and n == n0 and bad0 == 0 and bad == 0, (precision, n0, bad0, n, bad, msg)


# ---------------------------------------------------------------------------------------------------------------------------------------
# Part E: the rollout step on another ConvVAE
# ---------------------------------------------------------------------------------------------------------------------------------------
SENT = -777.0


@pytest.mark.parametrize("cid", vc.ROLLOUT_CASES)
def test_rollout_entries_on_another_convvae(zoo, tmp_path, cid):
    """mi_rollout_step, mi_rollout_step_batch and mi_rollout_value_batch_rec on the smallest model and on 80 x 144 (W.roll_bytes, roll_env_floats() and the per-layer
    table of the step are built from the geometry): a policy of z_dim + 3 inputs and 2 actions, greedy and with given noise, n = 1 and 3 (33 on case 1), against
    OracleVAE.encode (float64) followed by the PPO oracle's predict at the bounds of test_l_rollout_batch_gpu.py: latents 1e-4 of the row's max, actions rtol 1e-4 /
    atol 1e-5, values rel 1e-4 / abs 1e-5.  Eight sentinel floats behind `out` and behind the scratch survive; the single-frame entry is within 1e-5 of row 0 of the
    batched one; a bf16 VAE gives the same answers (the step reads the fp32 masters) -- to 1e-5, not bitwise: the step's split-K layers add their raw sums with fp32
    atomics (rollout.hip), so two calls on the SAME engine already differ in the last bit; 1e-5 is what the project asks between two device paths of this step."""
    from rollout_gpu_common import make_pair
    L = milib.get()
    c = vc.by_id(cid)
    A, K, z = 2, 3, c.z
    o, pm = make_pair(tmp_path / "ppo", input_dim=z + K)
    rng = np.random.RandomState(300 + cid)
    N = 33 if cid == 1 else 3
    frames = rng.randint(0, 256, (N,) + vc.src_shape(c), dtype=np.uint8)
    meas = np.stack([rng.uniform(-1, 1, N), rng.uniform(0, 1, N), rng.uniform(0, 30, N)], axis=1).astype(np.float32)
    noise = rng.standard_normal((N, A)).astype(np.float32)
    ovae = vo.OracleVAE(vc.src_shape(c), vc.tgt_shape(c), z, params=vc.params(c), training=False, dtype=torch.float64)
    z_o = np.concatenate([ovae.encode(frames[i:i + 8].astype(np.float32) / np.float32(255.0)) for i in range(0, N, 8)])
    st = torch.cuda.current_stream().cuda_stream
    dev_of = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    row = A + 1 + z
    answers = {}
    for precision in ("fp32", "bf16"):
        vae = zoo.get(c, precision, training=False)
        vh, ph = vae.dev.handle, pm.dev.handle
        for n in ((1, 3, 33) if cid == 1 else (1, 3)):
            nbytes = int(L.mi_rollout_batch_workspace_bytes(vh, ph, n))
            assert nbytes > 0 and nbytes % 4 == 0
            scratch = torch.full((nbytes // 4 + 8,), SENT, device="cuda")
            f_d, m_d, z_d = dev_of(frames[:n]), dev_of(meas[:n]), dev_of(noise[:n])
            for greedy in (False, True):
                out = torch.full((n * row + 8,), SENT, device="cuda")
                L.mi_rollout_step_batch(vh, ph, st, f_d.data_ptr(), m_d.data_ptr(), K, None if greedy else z_d.data_ptr(), 1 if greedy else 0, n,
                                        scratch.data_ptr(), nbytes, out.data_ptr())
                torch.cuda.synchronize()
                got = out.cpu().numpy()
                assert (got[n * row:] == SENT).all() and (scratch[nbytes // 4:] == SENT).all().item(), (precision, n, greedy)
                got = got[:n * row].reshape(n, row)
                states = np.concatenate([z_o[:n], meas[:n]], 1)
                a_o, v_o = o.predict(states, greedy=greedy, noise=None if greedy else noise[:n])
                a_o, v_o = np.asarray(a_o).reshape(n, A), np.asarray(v_o).reshape(n)
                bad = vc.rollout_failures(got, z_o[:n], a_o, v_o, A)
                assert not bad, (precision, n, greedy, bad)
                answers[(precision, n, greedy)] = got
                if n == 3:
                    measure(c, precision, "rollout batch n = 3 greedy = %d: worst latent / row max" % greedy, max(vc.rel_err(got[r, A + 1:], z_o[r]) for r in range(n)), 1e-4)
                    measure(c, precision, "rollout batch n = 3 greedy = %d: worst |value - oracle|" % greedy, float(np.abs(got[:, A] - v_o).max()), "1e-4 rel + 1e-5")
                # the single-frame entry against row 0 of the batched one
                if n == 1:
                    one = torch.full((row + 8,), SENT, device="cuda")
                    L.mi_rollout_step(vh, ph, st, f_d.data_ptr(), m_d.data_ptr(), K, None if greedy else z_d.data_ptr(), 1 if greedy else 0, one.data_ptr())
                    torch.cuda.synchronize()
                    one = one.cpu().numpy()
                    assert (one[row:] == SENT).all()
                    assert np.allclose(one[:row], got[0], rtol=1e-5, atol=1e-5), (precision, greedy, one[:row], got[0])
            # the value-only entry: out [n], and the table rows it names
            vout = torch.full((n + 8,), SENT, device="cuda")
            tab = torch.full((2 * n + 8,), SENT, device="cuda")
            rows_d = dev_of(np.arange(n, dtype=np.int32) * 2)
            L.mi_rollout_value_batch_rec(vh, ph, st, f_d.data_ptr(), m_d.data_ptr(), K, n, scratch.data_ptr(), nbytes, vout.data_ptr(), rows_d.data_ptr(), 2 * n, tab.data_ptr())
            torch.cuda.synchronize()
            v, t = vout.cpu().numpy(), tab.cpu().numpy()
            assert (v[n:] == SENT).all() and (t[2 * n:] == SENT).all() and (t[1:2 * n:2] == SENT).all() and (scratch[nbytes // 4:] == SENT).all().item()
            assert np.array_equal(t[0:2 * n:2], v[:n])
            assert np.allclose(v[:n], answers[(precision, n, True)][:, A], rtol=1e-5, atol=1e-5), (precision, n)
    for key, got in answers.items():
        if key[0] == "bf16":
            assert np.allclose(got, answers[("fp32",) + key[1:]], rtol=1e-5, atol=1e-5), key


# ---------------------------------------------------------------------------------------------------------------------------------------
# Part B, the third unstored intermediate; the ordered bias rows of a one-split filter gradient
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_inference_form_of_the_fused_encoder_head_against_float64(zoo):
    """conv1's output behind the INFERENCE form of the fused encoder head (case 7, bf16: the one geometry the fused head takes): an inference-only engine has no region
    for it, encode() stores conv2's output alone, and that is held against the float64 two-stage statement from the frames with conv1's output rounded to bf16 as the
    training form stores it, at the bf16 bound 4e-3 rel + 4e-3 of max.  The training engine's encode() takes the same form (no backward pass follows) and stores the same bits."""
    c = vc.by_id(7)
    assert vc.route(c, "bf16", training=False)["enc_head"] == "fused"
    out = {}
    for training in (False, True):
        m = zoo.get(c, "bf16", training=training)
        if training:
            reset(m, c)
        dev = m.dev
        if not training:
            assert dev.stored("act", 1, c.B) is None
        else:
            _plant(dev.stored("act", 1, c.B))
        _plant(dev.stored("act", 2, c.B))
        infer(m, c)
        if training:
            assert _untouched(dev.stored("act", 1, c.B))     # the inference form ran: conv1's output never left the chip
        out[training] = _f64(dev.stored("act", 2, c.B))
    R = vc.encoder_head_inference_report(c, out[False], vc.params(c), vc.inputs(c))
    for name, how, val, bound in R.rows:
        measure(c, "bf16", "%s (%s)" % (name, how), val, bound)
    assert not R.bad, R.bad
    assert np.array_equal(out[False], out[True])


@pytest.mark.parametrize("case_no", [79, 97, 105])
def test_one_split_filter_gradient_sums_its_bias_rows_in_order(case_no):
    """What mi_vae_backward asks for in its own calls (the bias_rows field of the context it hands them) and a caller from outside switches on per thread
    (mi_tapwgrad_bias_rows, used here): a raw-staged filter gradient whose positions fit ONE split -- a small layer at a small
    batch; one case per kernel family of tests/conv_shape_cases.py -- has no slabs, but each bias element is still the sum of 2 - 8 partial sums (position halves, parity
    classes), which met in fp32 atomics: two runs of a small-batch step differed in the last bit.  Switched on: the partial rows go through the scratch and one ordered
    sum -- the bias gradient of three runs bitwise equal, dW and dbias inside the layer ops' bounds against float64 (1e-4 rel + 1e-4 of max; 1e-4 of max), the
    sentinels behind dW / dbias intact.  Switched off (every other caller's default) the scratch stays untouched."""
    import conv_shape_cases as cc
    import test_x_conv_shapes_gpu as tx
    L = milib.get()
    (c,) = [k for k in cc.CASES if k.id == case_no]
    fam, plan = cc.family_of(c)
    assert fam.startswith("tapwgrad") and plan["splits"] == 1 and c.opt.get("dbias") and c.opt.get("scratch") == "big", (fam, plan)
    d = cc.make_inputs(c)
    ref = cc.reference(c, d)
    with tx.Tuning(c.tune):
        off = tx.run_wgrad(c, d)
        prev = L.mi_tapwgrad_bias_rows(1)
        try:
            on = [tx.run_wgrad(c, d) for _ in range(3)]
        finally:
            assert L.mi_tapwgrad_bias_rows(prev) == 1
    assert prev == 0 and off["touched"] is False
    for r in on:
        assert r["touched"] is True and r["tails"]
        assert np.array_equal(r["db"], on[0]["db"])          # (dW is not asked: this test's buffers start non-zero, and the two position halves of a dW element then add in either order)
        tx.assert_close(r["dw"], ref["dw"], 1e-4, 1e-4 * ref["dw_scale"], "dw")
        tx.assert_close(r["db"], ref["db"], 0.0, 1e-4 * ref["db_scale"], "dbias")
