"""Every shipped non-default setting of the tuning knobs (csrc/tuning.hip) that no other test runs, against float64: the steps of
tests/knob_route_cases.py.

engine  the ConvVAE engine under each environment knob, one child process per step (the knobs are read when the library loads): existing cases 7, 1 and 8 of
        vae_engine_cases.py through the existing assertions at their existing bounds -- check_step (fp32 / bf16x3), the bf16 layer-by-layer report on the engine's own
        stored tensors (bf16; fp32-slab bounds under MI355_SLAB_BF16=0), the route the knob-aware gates of vae_engine_cases.route() predict, workspace guards where
        the engine sizes or carves by the knob, two runs bitwise, the one-call step bitwise forward + backward + Adam, the data-parallel identities where the knob
        touches the queues -- and a SHA-256 of (losses, gradient buffer, parameters after Adam) compared with the default process where the source says the knob
        changes no order of sums.
op      in this process, dispatch pinned with mi_set_tuning (restored in `finally`): layer-op cases of conv_shape_cases.py under keys 12, 14, 15 and 19 with
        test_x_conv_shapes_gpu.py's runners and bounds; the four product forms of the fused encoder head on camera bytes (key 23, bit 4096).
ppo     one child with MI355_PPO_STREAMS=1: the per-layer PPO step on two streams.
Measured figures are printed (pytest -s) as MEASURE lines: profiles/r38_knob_routes.md."""
import ctypes
import hashlib
import json
import os
import pathlib
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import conv_shape_cases as cc  # noqa: E402
import knob_route_cases as kc  # noqa: E402
import vae_engine_cases as vc  # noqa: E402
from mi355 import lib as milib  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str((a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def step_digest(got):
    """What a step leaves behind, as SHA-256s: 'all' -- the two losses, the flat gradient buffer, the parameters after Adam; 'losses'; one per gradient tensor."""
    out = {"all": digest(got["losses"], got["flat"], got["params_flat"]), "losses": digest(got["losses"])}
    out.update((k, digest(v)) for k, v in got["grads"].items())
    return out


ATOMIC_DBIAS = "vae/decoder/deconv4/bias"


def without(dev, flat, name):
    """A flat parameter-shaped buffer with one tensor's range zeroed."""
    o, n = dev.layout[name]
    flat = flat.copy()
    flat[o:o + n] = 0
    return flat


# ---------------------------------------------------------------------------------------------------------------------------------------
# bodies that run in the child (tests/knob_route_worker.py)
# ---------------------------------------------------------------------------------------------------------------------------------------
def one_call_identity(tz, m, c, first, rt):
    """Two runs of a step are bitwise equal, and mi_vae_train_step in one call is bitwise forward + backward + Adam (as test_step_identities asserts them).  The one
    exception the README's row makes: where the route takes the unfused loss pass mi_bce_logits_fwd_bwd_bias with its fused dbias (plain tail, at most three target
    channels), deconv4's bias gradient meets in fp32 atomics -- that tensor (gradient, parameter, Adam slots) is left out of the identity, and it alone."""
    from vae.models import adam_alpha, ADAM_BETA1, ADAM_BETA2, ADAM_EPSILON
    dev = m.dev
    atomic = rt["tail"] == "plain" and rt["fuse_b4"]
    cut = (lambda a: without(dev, a, ATOMIC_DBIAS)) if atomic else (lambda a: a)

    def same(a, b):
        return np.array_equal(cut(a["params_flat"]), cut(b["params_flat"])) and np.array_equal(cut(a["slots"][0]), cut(b["slots"][0])) and \
            np.array_equal(cut(a["slots"][1]), cut(b["slots"][1])) and np.array_equal(a["losses"], b["losses"])
    second = tz.run_step(m, c)
    assert same(first, second) and np.array_equal(cut(first["flat"]), cut(second["flat"])) and np.abs(first["flat"]).max() > 0, \
        sorted(k for k in first["grads"] if not np.array_equal(first["grads"][k], second["grads"][k]))
    tz.measure(c, "identity", "two runs bitwise equal" + (" (all but deconv4's bias gradient: fp32 atomics of the unfused loss pass)" if atomic else ""), "yes", "yes")
    alpha = adam_alpha(vc.LR, np.float32(ADAM_BETA1), np.float32(ADAM_BETA2))
    src, tgt, e = tz.tables(m, c)
    tz.reset(m, c)
    dev.train_step(src, tgt, None, c.B, 1.0 / c.B, e, alpha, ADAM_BETA1, ADAM_BETA2, ADAM_EPSILON)
    torch.cuda.synchronize()
    one = {"params_flat": dev.params.cpu().numpy().copy(), "slots": (dev.adam_m.cpu().numpy().copy(), dev.adam_v.cpu().numpy().copy()), "losses": dev.losses.cpu().numpy().copy()}
    assert same(one, first)


def ares_ops(s):
    """The activation-resident kernels at the op level under the step's MI355_ARES_CFG / MI355_ARES_MID: batches 1, 3, 5 and 9 leave frame groups of 2, 4 and 8 a
    ragged last group each."""
    import test_ops_gpu as to
    from hip_helpers import DT, P, alloc, dev, host, stream
    if "ares_op" in s.extra:
        for B in (1, 3, 5, 9):
            to.test_activation_resident_small_grid_layers(B)           # the three forms against float64 at hip_helpers.tols("bf16")
        return
    # MI355_ARES_MID=0: form 2 launches nothing and writes nothing (the engine then takes the layer ops); forms 0 and 1 still run
    L = milib.get()
    code, td = DT["bf16"]
    rng = np.random.RandomState(5)
    nb = int(L.mi_ares_weight_bytes())
    for B in (1, 3, 5, 9):
        launched = np.ones(1, np.int32)
        wfm = torch.empty(nb, device="cuda", dtype=torch.uint8)
        L.mi_ares_pack_weights(stream(), 2, P(dev((rng.randn(4, 4, 64, 128) / 16).astype(np.float32))), wfm.data_ptr())
        om = alloc(td, B * 18 * 38 * 64 + 8, fill=7.0)
        L.mi_ares_conv(stream(), code, 2, P(dev(rng.randn(B, 8, 18, 128).astype(np.float32), td)), B, wfm.data_ptr(), P(dev(np.zeros(64, np.float32))), 1, None, om.data_ptr(),
                       launched.ctypes.data)
        assert launched[0] == 0 and (host(om) == 7.0).all(), B
        for form, xshape, oshape in ((0, (B, 8, 18, 128), (B, 3, 8, 256)), (1, (B, 3, 8, 256), (B, 8, 18, 128))):
            wf = torch.empty(nb, device="cuda", dtype=torch.uint8)
            L.mi_ares_pack_weights(stream(), form, P(dev((rng.randn(4, 4, 128, 256) / 32).astype(np.float32))), wf.data_ptr())
            out = alloc(td, int(np.prod(oshape)), fill=7.0)
            L.mi_ares_conv(stream(), code, form, P(dev(rng.randn(*xshape).astype(np.float32), td)), B, wf.data_ptr(), None, 0, None, out.data_ptr(), launched.ctypes.data)
            assert launched[0] == 1, (B, form)


def engine_step_run(s):
    """One engine step of knob_route_cases.STEPS in THIS process (started with the step's environment) -> {'digests': {'precision/case': sha}, 'guards': {..}}."""
    import test_zzzzzzz_vae_engine_shapes_gpu as tz
    L = milib.get()
    out = {"step": s.id, "digests": {}, "guards": {}}
    with tempfile.TemporaryDirectory() as tmp:
        zoo = tz.Zoo(pathlib.Path(tmp))
        try:
            for precision, cid, u8 in s.runs:
                c = vc.by_id(cid)
                m = zoo.get(c, precision)
                tag = "%s/%d" % (precision, cid)
                if s.guards:
                    n0, bad0, _ = m.dev.check_guards()
                if precision == "bf16":
                    depths = (3, 5, 6) if "nw_depth" in s.extra else (None,)
                    seen = []
                    for depth in depths:                         # (key 19 acts on the uint8 run inside the helper, which must equal the float tables' run bitwise)
                        prev = L.mi_set_tuning(19, depth) if depth is not None else None
                        try:
                            got = tz.bf16_layer_by_layer(zoo, cid, env=s.env, slab=s.slab, u8=u8)
                        finally:
                            if depth is not None:
                                L.mi_set_tuning(19, prev)
                        seen.append(step_digest(got)["all"])
                    assert len(set(seen)) == 1, seen
                else:
                    got = tz.check_step(m, c, precision, env=s.env)
                out["digests"][tag] = step_digest(got)
                if s.dp:                                         # two runs, the one-call step, the backward in parts, train_step_dp on a recording communicator + its bucket log
                    tz.test_step_identities(zoo, precision, cid)
                else:
                    one_call_identity(tz, m, c, got, vc.route(c, precision, max_batch=m.dev.max_batch, env=s.env))
                if s.guards:
                    tz.infer(m, c)
                    n, bad, _ = m.dev.check_guards()
                    out["guards"][tag] = [n0, bad0, n, bad, L.cdll.mi_last_error().decode() if bad else ""]
                    assert n0 >= 30 and n == n0 and bad0 == 0 and bad == 0, (tag, out["guards"][tag])
        finally:
            zoo.release()
    if "ares_op" in s.extra or "ares_mid_op" in s.extra:
        ares_ops(s)
    if "dectail_edge_op" in s.extra:                         # mi_deconv2d_tail_fused with edge = 0 where that is another tiling: against the three separately validated ops
        import test_ops_gpu as to
        for B, IH, IW in kc.DECTAIL_EDGE_OP_SHAPES:
            for kind, u8 in ((0, True), (0, False), (1, True), (2, False)):
                to.test_decoder_tail_fused_equals_the_three_ops(kind, u8, B, IH, IW)
    return out


def ppo_digests(check, ref_trunk=False):
    """The per-layer PPO pass on ppo_shape_cases.PER_LAYER_CASES (ref_trunk: on knob_route_cases.PPO_REF_TRUNK, in a process with the fused step switched off): check --
    the gradient pass against float64 at test_r_ppo_shapes_gpu.py's bounds; then three train_steps from the case's parameters, twice, bitwise equal
    -> {case: SHA-256 of parameters, Adam slots and the five loss scalars}."""
    import ppo_shape_cases as pc
    import test_r_ppo_shapes_gpu as tr

    class PerLayerRig(tr.Rig):
        """tr.Rig on a case the per-layer path takes -- by its shape, or because MI355_PPO_FUSED=0."""

        def __init__(self, c):
            from mi355.ppo_device import PpoDevice
            self.c, self.fused = c, False
            self.d = d = PpoDevice(c.input_dim, c.A, c.low, c.high, pc.EPS, pc.VALUE_SCALE, pc.ENTROPY_SCALE, hidden=c.hidden, max_batch=320, precision="fp32")
            assert not d.fused_ok()
            up = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(d.device)      # noqa: E731
            self.s, self.a, self.R, self.adv = up(c.s), up(c.a), up(c.R), up(c.adv)
            self.reset()

    cases = {n: (lambda n=n: pc.build(*kc.PPO_REF_TRUNK[n])) for n in kc.PPO_REF_TRUNK} if ref_trunk else {n: (lambda n=n: pc.engine_case(n)) for n in pc.PER_LAYER_CASES}
    made, out = {}, {}

    def get(name, precision="fp32"):
        if name not in made:
            made[name] = PerLayerRig(cases[name]())
        made[name].reset()
        return made[name]
    try:
        for name in cases:
            if check:
                tr.test_gradient_pass_against_float64(get, name, "fp32")
            seen = []
            for _ in range(2):
                r = get(name)
                c, d = r.c, r.d
                for _ in range(3):
                    d.train_step(r.s, r.a, r.R, r.adv, c.M, 1.0 / c.M, 1.0, tr.ALPHA)
                torch.cuda.synchronize()
                # (the five loss scalars: the per-layer pass writes no action means / stds behind them -- those entries of the buffer are the fused kernels')
                seen.append(digest(d.params.cpu().numpy(), d.adam_m.cpu().numpy(), d.adam_v.cpu().numpy(), d.losses.cpu().numpy()[:5]))
            assert seen[0] == seen[1], name
            out[name] = seen[0]
    finally:
        for r in made.values():
            r.d.close()
    return out


def ppo_step_run(s):
    return {"step": s.id, "digests": ppo_digests(check=True, ref_trunk="ref_trunk" in s.extra)}


# ---------------------------------------------------------------------------------------------------------------------------------------
# the parent: children, the default process's digests
# ---------------------------------------------------------------------------------------------------------------------------------------
def run_child(s):
    knob_names = {r.env for r in kc.table_rows() if r.env}
    env = {k: v for k, v in os.environ.items() if k not in knob_names}
    env.update(s.env)
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "knob_route_worker.py"), s.id], env=env, capture_output=True, text=True, timeout=150)
    except subprocess.TimeoutExpired as e:
        pytest.exit("step %s: the child did not end within 150 s -- nothing more is started on this GPU\n%s" % (s.id, str(e.stderr or "")[-3000:]), returncode=3)
    if r.returncode in (-6, -11, 134, 139) or "illegal memory access" in r.stderr:      # an abort, a segmentation fault or a GPU fault: the session ends here
        pytest.exit("step %s: the child faulted (exit status %d) -- nothing more is started on this GPU\n%s" % (s.id, r.returncode, r.stderr[-6000:]), returncode=3)
    for line in r.stdout.splitlines():
        if line.startswith("MEASURE") or "(bound " in line:
            print("[%s] %s" % (s.id, line))
    assert r.returncode == 0, "exit status %d\n%s\n%s" % (r.returncode, r.stdout[-3000:], r.stderr[-6000:])
    out = json.loads([line for line in r.stdout.splitlines() if line.startswith("{")][-1])
    assert out["step"] == s.id
    return out


@pytest.fixture(scope="module")
def default_digests(tmp_path_factory):
    """{'precision/case': SHA-256} of the same step at default knobs, computed once, in this process, for every (precision, case) a digest-equal step runs."""
    import test_zzzzzzz_vae_engine_shapes_gpu as tz
    want = sorted({(p, cid) for s in kc.ENGINE_STEPS for p, cid, _ in s.runs}, key=lambda pc_: (vc.PRECISIONS.index(pc_[0]), pc_[1]))
    zoo = tz.Zoo(tmp_path_factory.mktemp("knob_routes_default"))
    out = {}
    try:
        for precision, cid in want:
            c = vc.by_id(cid)
            out["%s/%d" % (precision, cid)] = step_digest(tz.run_step(zoo.get(c, precision), c))
    finally:
        zoo.release()
    return out


@pytest.mark.parametrize("sid", [s.id for s in kc.ENGINE_STEPS])
def test_engine_under_knob(sid, default_digests):
    """One child per step: the engine under the step's knobs through the existing assertions (engine_step_run); then the digests against the default process --
    asserted equal where the step says `equal`, printed otherwise."""
    s = kc.STEPS[sid]
    out = run_child(s)
    assert set(out["digests"]) == {"%s/%d" % (p, cid) for p, cid, _ in s.runs}
    if s.guards:
        assert set(out["guards"]) == set(out["digests"])
    differ = {tag: sorted(k for k in d if k != "all" and d[k] != default_digests[tag][k]) for tag, d in out["digests"].items()}
    for tag in sorted(differ):
        what = "equal" if not differ[tag] else ("differs in " + ", ".join(differ[tag]) if len(differ[tag]) <= 5 else "differs in %d of 23" % len(differ[tag]))
        print("MEASURE knob %s %s | losses and the 22 gradient tensors vs the default process, bitwise | %s | %s" % (sid, tag, what, "equal" if s.digest == "equal" else "-"))
        assert (out["digests"][tag]["all"] == default_digests[tag]["all"]) == (not differ[tag]), (sid, tag)      # (the parameters after Adam follow the gradients)
    if s.digest == "equal":
        allowed = {tag: set(kc.DIGEST_EXCEPT.get(sid, {}).get(tag.split("/")[0], ())) for tag in differ}
        assert all(set(differ[tag]) <= allowed[tag] for tag in differ), (sid, differ)


def test_ppo_per_layer_step_on_two_streams():
    """MI355_PPO_STREAMS=1 in a child: the per-layer path's gradient pass against float64 at the bounds of test_r_ppo_shapes_gpu.py on every per-layer case; three
    train_steps, run twice, bitwise equal, and digest-equal to the one-stream run of this process (the same kernels on the same operands: the value side and the old
    policy's forward only move to a second queue)."""
    s = kc.STEPS["ppo_streams_1"]
    out = run_child(s)
    here = ppo_digests(check=False)
    assert set(out["digests"]) == set(here) and len(here) == 4
    for name in sorted(here):
        eq = out["digests"][name] == here[name]
        print("MEASURE knob %s %s | digest of (parameters, Adam slots, losses) after three steps vs one stream | %s | equal" % (s.id, name, "equal" if eq else "differs"))
    assert out["digests"] == here


def test_ppo_reference_trunk_per_layer_on_two_streams():
    """The reference trunk 67 -> 500 / 300 -> 3 takes the per-layer path only with MI355_PPO_FUSED=0, which this process cannot set any more: two children, one with
    MI355_PPO_STREAMS=1 as well.  M = 5 and 33: each child's gradient pass against float64 at test_r_ppo_shapes_gpu.py's bounds, two runs of three train_steps
    bitwise equal; the two children's digests equal."""
    two, one = run_child(kc.STEPS["ppo_streams_1_fused_0"]), run_child(kc.STEPS["ppo_fused_0"])
    assert set(two["digests"]) == set(one["digests"]) == set(kc.PPO_REF_TRUNK)
    for name in kc.PPO_REF_TRUNK:
        eq = two["digests"][name] == one["digests"][name]
        print("MEASURE knob ppo_streams_1_fused_0 %s | digest of (parameters, Adam slots, losses) after three steps vs one stream | %s | equal" % (name, "equal" if eq else "differs"))
    assert two["digests"] == one["digests"]


# ---------------------------------------------------------------------------------------------------------------------------------------
# op level, in this process
# ---------------------------------------------------------------------------------------------------------------------------------------
OP_CASES = [(sid, c) for sid, cases in kc.KNOB_OP_CASES.items() for c in cases]


@pytest.fixture(scope="module", autouse=True)
def _print_op_measurements():
    import test_x_conv_shapes_gpu as tx
    before = dict(tx.MEAS)                                  # (what test_x_conv_shapes_gpu.py's own tests noted in this process is theirs, and already printed)
    tx.MEAS.clear()
    yield
    for (section, what), (a, b) in sorted(tx.MEAS.items()):
        print("MEASURE op %s | %s | %s | %s" % (section, what, ("yes" if a else "no") if b == "flag" else "%.3g" % a, "-" if b in (None, "flag") else "%.3g" % b))
    tx.MEAS.update(before)


@pytest.mark.parametrize("sid,c", OP_CASES, ids=["%s-%s" % (sid, kc.op_case_id(c)) for sid, c in OP_CASES])
def test_layer_op_under_key(sid, c):
    """Keys 12, 14, 15 and 19 off their defaults on existing cases of conv_shape_cases.py, through test_x_conv_shapes_gpu.py's own tests (float64 reference, the
    case's bounds, sentinels, bitwise second runs).  Key 19 = 5 / 6: also bitwise the depth-3 kernel (the depth moves the prefetch distance; steps past a wave's
    range add zeros)."""
    import test_x_conv_shapes_gpu as tx
    if c.entry.endswith(".wgrad"):
        tx.test_filter_gradient(c)
    else:
        tx.test_forward_and_input_gradient(c)
    if sid.startswith("key19"):
        d = cc.make_inputs(c)
        with tx.Tuning(c.tune):
            deep = tx.run_wgrad(c, d)
        with tx.Tuning(cc.tune(c.tune, k19=3)):
            three = tx.run_wgrad(c, d)
        assert deep["touched"] and three["touched"]
        assert np.array_equal(deep["dw"], three["dw"]) and np.array_equal(deep["db"], three["db"])
    L = milib.get()
    key = int(sid[3:].split("_")[0])
    assert L.mi_set_tuning(key, cc.header_constants()["DEFAULTS"][key]) == cc.header_constants()["DEFAULTS"][key]      # the preset was restored


@pytest.mark.parametrize("with_idx", [True, False])
@pytest.mark.parametrize("B", kc.ENC12_BATCHES)
def test_fused_encoder_head_product_forms_on_camera_bytes(B, with_idx):
    """mi_conv2d_enc12_fwd on uint8 frames in each of the four product forms (key 23 = 4096 | 8192 ring | 16384 pipelined conv2: enc12.hip), with and without a frame
    index: conv1's activation and its ReLU bit words bitwise mi_conv2d_nhwc_fwd_bits; conv2's output against the float64 convolution of the stored activation and
    against the unfused kernel at the bounds of test_encoder_head_forward_fused_equals_the_two_ops (2^-8 rel + 2^-9 of max; 2^-7 rel + 2^-8 of max); eight sentinels
    behind each output survive; the four forms' conv2 outputs are printed as equal or not (enc12.hip states no identity for them)."""
    from hip_helpers import DT, alloc, assert_close, dev, host, stream
    L = milib.get()
    code, td = DT["bf16"]
    rng = np.random.RandomState(700 + B)
    n_frames = B + 2 if with_idx else B
    frames = rng.randint(0, 256, (n_frames, 80, 160, 3)).astype(np.uint8)
    fr = dev(frames, torch.uint8)
    idxd = dev(rng.permutation(n_frames)[:B].astype(np.int32), torch.int32) if with_idx else None
    idxp = idxd.data_ptr() if with_idx else None
    w1 = (rng.randn(4, 4, 3, 32) / np.sqrt(48)).astype(np.float32)
    w2 = (rng.randn(4, 4, 32, 64) / np.sqrt(512)).astype(np.float32)
    b1d, b2 = dev((0.1 * rng.randn(32)).astype(np.float32)), (0.1 * rng.randn(64)).astype(np.float32)
    b2d = dev(b2)
    w1t = dev(torch.from_numpy(w1).permute(3, 0, 1, 2).reshape(32, -1).contiguous(), td)
    w2t = dev(torch.from_numpy(w2).permute(3, 0, 1, 2).reshape(64, -1).contiguous(), td)
    n1, nb, n2 = B * 39 * 79 * 32, B * 39 * 79 * 2, B * 18 * 38 * 64
    act1 = alloc(td, n1, fill=3.0)
    bits = torch.full((nb,), 0x55, device="cuda", dtype=torch.int32)
    wrote = np.zeros(1, np.int32)
    L.mi_conv2d_nhwc_fwd_bits(stream(), code, fr.data_ptr(), idxp, 2, B, 80, 160, 3, w1t.data_ptr(), 1, b1d.data_ptr(), 4, 4, 32, 1, act1.data_ptr(), bits.data_ptr(), wrote.ctypes.data)
    act2 = alloc(td, n2, fill=3.0)
    L.mi_conv2d_nhwc_fwd(stream(), code, act1.data_ptr(), None, 0, B, 39, 79, 32, w2t.data_ptr(), 1, b2d.data_ptr(), 4, 4, 64, 1, act2.data_ptr())
    torch.cuda.synchronize()
    assert wrote[0] == 1
    r2 = host(act2).reshape(B, 18, 38, 64)
    scale = float(np.abs(r2).max())
    x = torch.from_numpy(host(act1).reshape(B, 39, 79, 32)).permute(0, 3, 1, 2)
    w2b = torch.from_numpy(host(w2t)).reshape(64, 4, 4, 32).permute(0, 3, 1, 2)
    ref = torch.nn.functional.conv2d(x, w2b, torch.from_numpy(b2.astype(np.float64)), stride=2).clamp_min(0).permute(0, 2, 3, 1).numpy()
    seen = {}
    for name, mask in kc.ENC12_FORMS.items():
        f1 = alloc(td, n1 + 8, fill=-7.0)
        fb = torch.full((nb + 8,), 0x33, device="cuda", dtype=torch.int32)
        f2 = alloc(td, n2 + 8, fill=-7.0)
        launched = ctypes.c_int(0)
        prev = L.mi_set_tuning(23, mask)
        try:
            L.mi_conv2d_enc12_fwd(stream(), code, fr.data_ptr(), 2, idxp, B, 80, 160, w1t.data_ptr(), b1d.data_ptr(), w2t.data_ptr(), b2d.data_ptr(),
                                  f1.data_ptr(), fb.data_ptr(), f2.data_ptr(), ctypes.addressof(launched))
            torch.cuda.synchronize()
        finally:
            assert L.mi_set_tuning(23, prev) == mask
        assert prev == 0 and launched.value == 1, name
        assert torch.equal(f1[:n1].view(torch.int16), act1.view(torch.int16)), "conv1 activation, form '%s': not bitwise the layer op's" % name
        assert torch.equal(fb[:nb], bits), "ReLU bit words, form '%s'" % name
        assert (f1[n1:].float() == -7.0).all().item() and (fb[nb:] == 0x33).all().item() and (f2[n2:].float() == -7.0).all().item(), "sentinels, form '%s'" % name
        a2 = host(f2[:n2]).reshape(B, 18, 38, 64)
        assert_close(a2, ref, 2.0 ** -8, 2.0 ** -9 * scale, "conv2 output, form '%s', vs the float64 convolution of the stored activation" % name)
        assert_close(a2, r2, 2.0 ** -7, 2.0 ** -8 * scale, "conv2 output, form '%s', vs the layer op" % name)
        assert (a2 >= 0).all() and (a2 == 0).mean() > 0.05
        err = np.abs(a2 - ref) / (2.0 ** -8 * np.abs(ref) + 2.0 ** -9 * scale)
        print("MEASURE enc12 form '%s' B = %d idx = %d | conv2 output: worst |err| / (2^-8 |ref| + 2^-9 max) | %.3g | 1" % (name, B, with_idx, float(err.max())))
        seen[name] = f2[:n2].view(torch.int16).clone()
    first = seen["ring + c2"]
    print("MEASURE enc12 B = %d idx = %d | forms whose conv2 output is bitwise the product form's | %s | -" % (B, with_idx, ", ".join(n for n, v in seen.items() if torch.equal(v, first))))
