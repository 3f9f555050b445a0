"""Engine runs shared by tests/test_zzzzzzzz_mlp_engine_shapes_gpu.py and its child processes, and the child itself.

As a program (a fresh `python` started by the test, because the library reads both variables from the environment it is loaded or sized in):
  python mlp_engine_worker.py streams OUT_DIR    with MI355_MLP_STREAMS=0: one training step of cases 2 and 8 in both precisions on ONE stream; writes the gradient
                                                 buffer and the updated parameters to OUT_DIR/streams_<case>_<precision>.npz
  python mlp_engine_worker.py guards             with MI355_DEBUG_GUARDS=1: a training step, encode, reconstruct and generate_from_latent of cases 3, 7 and 8 in both
                                                 precisions, the guard counts before and after, then one guard overwritten through a torch view of the workspace and
                                                 what the checker says; one JSON line"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "carla-ppo_amd"), ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import mlp_engine_cases as mc  # noqa: E402


def make_model(root, c, precision, loss_fn="bce", kl_tolerance=0.0, beta=1.0, training=True, create_batch=None, tag=""):
    """MlpVAE of the case on the device with the case's parameters.  create_batch: the engine's max_batch at creation (default: init_session's 128 / 16)."""
    from vae.models import MlpVAE
    m = MlpVAE(np.array(c.src), np.array(c.tgt), encoder_sizes=c.enc, decoder_sizes=c.dec, z_dim=c.z, precision=precision, loss_fn=loss_fn, kl_tolerance=kl_tolerance,
               beta=beta, training=training, learning_rate=mc.LR, seed=0, model_dir=str(root / ("%d_%s_%s_%d%s" % (c.id, precision, loss_fn, training, tag))))
    m.set_weights(mc.params(c))
    if create_batch is not None:
        make = m._make_device
        m._make_device = lambda max_batch: make(create_batch)
    m.init_session(init_logging=False)
    return m


def reset(m, c):
    """Back to the case's parameters, zero Adam slots, a gradient buffer full of NaN (backward STORES), first-step bias corrections."""
    from vae.models import ADAM_BETA1, ADAM_BETA2
    dev = m.dev
    dev.load_params(mc.params(c))
    if dev.with_optimizer:
        dev.adam_m.zero_()
        dev.adam_v.zero_()
        dev.grads.fill_(float("nan"))
    m.beta1_power, m.beta2_power = np.float32(ADAM_BETA1), np.float32(ADAM_BETA2)
    torch.cuda.synchronize()


def tables(m, c, frames_u8=0, rows=None):
    """(source table, target table, eps) on the device; frames_u8 bit 0 / 1: the source / target table stays raw bytes.  rows: the first `rows` frames only."""
    d = mc.inputs(c)
    n = c.B if rows is None else rows
    dv = m.dev.device

    def tab(kind, u8):
        a = d[kind + ("_u8" if u8 else "")][:n].reshape(n, -1)
        return torch.from_numpy(np.ascontiguousarray(a)).to(dv)
    return tab("src", frames_u8 & 1), tab("tgt", frames_u8 & 2), torch.from_numpy(np.ascontiguousarray(d["eps"][:n])).to(dv)


def f64(t):
    return None if t is None else t.float().cpu().numpy().astype(np.float64)


def grab_stored(m, c, B):
    """Every tensor the last forward + backward stored, float64 numpy, in mlp_engine_cases.layer_report's form."""
    dev = m.dev
    st = {"x": f64(dev.stored("x", 0, B)), "heads": f64(dev.stored("heads", 0, B)), "dz": f64(dev.stored("dz", 0, B)), "dheads": f64(dev.stored("dheads", 0, B)),
          "mean": f64(dev._view(1, B * c.z)).reshape(B, c.z), "logvar": f64(dev._view(2, B * c.z)).reshape(B, c.z), "z": f64(dev._view(5, B * c.z, dev.T)).reshape(B, c.z)}
    for i in range(len(c.enc)):
        st["h%d" % i], st["gh%d" % i] = f64(dev.stored("h", i, B)), f64(dev.stored("gh", i, B))
    for i in range(len(c.dec) + 1):
        st["d%d" % i], st["gd%d" % i] = f64(dev.stored("d", i, B)), f64(dev.stored("gd", i, B))
    return st


def run_step(m, c, frames_u8=0, idx=None, grab=False, adam=True, src_tgt_eps=None, B=None):
    """forward + backward(part 0) (+ Adam) from the case's parameters -> dict(losses, mean, flat, grads[, stored][, params_after, flat_after, m, v, weights_t])."""
    reset(m, c)
    dev = m.dev
    B = c.B if B is None else B
    src, tgt, e = tables(m, c, frames_u8, rows=None if idx is not None else B) if src_tgt_eps is None else src_tgt_eps
    dev.forward(src, tgt, idx, B, 1.0 / B, e, 1, 1)
    out = {"losses": dev.losses.cpu().numpy().copy(), "mean": dev._view(1, B * c.z).cpu().numpy().reshape(B, c.z).copy()}
    dev.backward(src, idx, e, 1.0 / B, 0)
    torch.cuda.synchronize()
    out["flat"] = dev.grads.cpu().numpy().copy()
    out["grads"] = dev._from_flat(out["flat"])
    if grab:
        out["stored"] = grab_stored(m, c, B)
    if adam:
        m._adam_step()
        torch.cuda.synchronize()
        out["flat_after"] = dev.params.cpu().numpy().copy()
        out["params_after"] = dev._from_flat(out["flat_after"])
        out["m"], out["v"] = dev.adam_m.cpu().numpy().copy(), dev.adam_v.cpu().numpy().copy()
        out["weights_t"] = dev.weights_t.view(torch.int16 if dev.bf16 else torch.int32).cpu().numpy().copy()
    return out


def infer(m, c):
    """(encode, reconstruct with the case's eps or None where P != S, generate_from_latent with eps as the latent) through the model's inference surface."""
    d = mc.inputs(c)
    mean = m.encode(d["src"])
    rec = None
    if mc.P(c) == mc.S(c):
        rec = np.stack([r.reshape(-1) for r in m.reconstruct(d["src"], eps=d["eps"])])
    return mean, rec, m.generate_from_latent(d["eps"])


def device_reconstruct(m, c):
    """mi_mlpvae_reconstruct on the case's frames with its eps, whatever the target's size ([B, P]; the model's reconstruct() reshapes with the SOURCE shape and
    raises where P != S, after the device pass has run)."""
    src, _, e = tables(m, c)
    out = torch.empty(c.B, mc.P(c), device=m.dev.device)
    m.dev.reconstruct(src, None, c.B, e, 1, out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def split_prefix_floats(c, kinds):
    """Floats at the start of the slab region that the split products of `kinds` ('fwd', 'dgrad') write at batch c.B: every split product stores its
    [slabs][B][N] from the region's start, so the written part is a prefix as long as the largest of them (0: no product of these kinds splits)."""
    r = mc.route(c, "fp32")                                 # (slab counts do not depend on the precision)
    best = 0
    for j, (_, _, K, N) in enumerate(mc.layers(c)):
        if "fwd" in kinds and r["fwd"][j] > 1:
            best = max(best, r["fwd"][j] * c.B * N)
        if "dgrad" in kinds and j and r["dgrad"][j] > 1:
            best = max(best, r["dgrad"][j] * c.B * K)
    return best


def streams_run(out_dir):
    import pathlib
    import tempfile
    assert os.environ.get("MI355_MLP_STREAMS") == "0"
    with tempfile.TemporaryDirectory() as tmp:
        for cid in mc.STREAM_CASES:
            c = mc.by_id(cid)
            for precision in mc.precisions(c):
                m = make_model(pathlib.Path(tmp), c, precision)
                r = run_step(m, c)
                np.savez(os.path.join(out_dir, "streams_%d_%s.npz" % (cid, precision)), flat=r["flat"], flat_after=r["flat_after"], losses=r["losses"])
                m.dev.close()
    return {"cases": list(mc.STREAM_CASES)}


def guards_run():
    import pathlib
    import tempfile
    assert os.environ.get("MI355_DEBUG_GUARDS") == "1"
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for cid in mc.GUARD_CASES:
            c = mc.by_id(cid)
            for precision in mc.precisions(c):
                m = make_model(pathlib.Path(tmp), c, precision, create_batch=mc.CREATE_BATCH.get(cid))
                run_step(m, c)                             # (case 3 grows its engine here: the guards of the NEW workspace are the ones checked)
                dev = m.dev
                n0, bad0, _ = dev.check_guards()
                run_step(m, c)
                infer(m, c)                                # encode, generate_from_latent (and the model's reconstruct where P == S)
                rec = device_reconstruct(m, c)             # the device's reconstruct for every case, P != S included
                assert rec.shape == (c.B, mc.P(c)) and np.isfinite(rec).all()
                n, bad, _ = dev.check_guards()
                msg = dev.L.cdll.mi_last_error().decode() if bad else ""
                # overwrite one guard (the last region's) through a torch view of the engine's own workspace: the checker names it
                k = n - 1
                _, _, off = dev.check_guards(k)
                inside = 0 <= off and off + 256 <= dev.workspace.numel()
                named = ""
                if inside:
                    dev.workspace[off + 5:off + 6].fill_(0x5A)
                    _, bad_after, _ = dev.check_guards()
                    named = dev.L.cdll.mi_last_error().decode()
                else:
                    bad_after = -1
                out["%d %s" % (cid, precision)] = {"n0": n0, "bad0": bad0, "n": n, "bad": bad, "msg": msg, "guard": k, "offset": off, "inside": inside,
                                                   "bad_after": bad_after, "named": named, "regions": len(mc.workspace_layout(c, precision, dev.max_batch)[0])}
                dev.close()
    return out


if __name__ == "__main__":
    if sys.argv[1] == "streams":
        print(json.dumps(streams_run(sys.argv[2])))
    elif sys.argv[1] == "guards":
        print(json.dumps(guards_run()))
    else:
        raise SystemExit("usage: mlp_engine_worker.py streams OUT_DIR | guards")
