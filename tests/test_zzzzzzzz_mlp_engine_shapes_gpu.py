"""The MlpVAE ENGINE (csrc/mlp_engine.hip) against float64 OFF the one family of models every other test builds: nine models (tests/mlp_engine_cases.py) that take
the parameter layout, the workspace carve, splitk_slabs, the routing of every filter gradient, the two-stream backward pass and Adam's kernel table down the
branches the 38400-wide, two-layer, 64-latent models never reach.

A  one whole step of the fp32 engine against the float64 oracle at the project's bounds for this engine (tests/test_f_mlp_vae_gpu.py): losses 1e-4 (+ 4e-6 abs on
   KL), every gradient tensor 1e-4 of its max, parameters after Adam within 2e-6 + 1e-5 max|w| of AdamTF on the device's own gradients, encode / reconstruct /
   generate_from_latent on the updated weights 1e-4 of max.
B  the bf16 engine op by op on its OWN stored tensors (mi_mlpvae_buffer 10 .. 61) against derived bounds (mlp_engine_cases.layer_report); its losses against the
   oracle's bf16 emulation.
C  identities, bitwise: stored gradients, backward in parts, the one-call step, uint8 tables, the caller's table as layer 0's operand, a short batch behind a long
   one, regrowth, the inference engine, one stream against two (child process).
D  workspace guards (child process).

Measured deviations are printed (pytest -s) as `MEASURE case precision | what | achieved | bound`: profiles/r31_mlp_engine_shapes.md."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mlp_engine_cases as mc  # noqa: E402
import mlp_engine_worker as mw  # noqa: E402

WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mlp_engine_worker.py")


def measure(c, precision, what, achieved, bound):
    print("MEASURE case %d %s | %s | %.3e | %.3e" % (c.id, precision, what, achieved, bound))


class Zoo:
    """One model per (case, precision, loss, mode, tag), built once."""

    def __init__(self, root):
        self.root, self.models = root, {}

    def release(self):
        for m in self.models.values():
            m.dev.close()
        self.models.clear()
        torch.cuda.empty_cache()

    def get(self, c, precision, loss_fn="bce", kl_tolerance=0.0, beta=1.0, training=True, create_batch=None, tag=""):
        key = (c.id, precision, loss_fn, kl_tolerance, beta, training, create_batch, tag)
        if key not in self.models:
            self.models[key] = mw.make_model(self.root, c, precision, loss_fn, kl_tolerance, beta, training, create_batch, tag="%s_%s" % (tag, create_batch))
        return self.models[key]


@pytest.fixture(scope="module")
def zoo(tmp_path_factory):
    z = Zoo(tmp_path_factory.mktemp("mlp_engine_shapes"))
    yield z
    z.release()


def combos(cases):
    return [(cid, p) for cid in cases for p in mc.precisions(mc.by_id(cid))]


# ---------------------------------------------------------------------------------------------------------------------------------------
# Part A
# ---------------------------------------------------------------------------------------------------------------------------------------
PART_A = [(c.id, "bce") for c in mc.CASES] + [(cid, k) for cid in mc.LOSS_KIND_CASES for k in ("bce_v2", "mse")]


@pytest.mark.parametrize("cid,loss_fn", PART_A)
def test_fp32_step_against_float64(zoo, cid, loss_fn):
    """Losses, every gradient tensor, one TF-Adam step and the inference surface of the fp32 engine against float64 (worst deviations of this engine alone, measured:
    profiles/r31_mlp_engine_shapes.md)."""
    c = mc.by_id(cid)
    kw = dict(loss_fn=loss_fn, kl_tolerance=mc.KL_TOLERANCE[cid], beta=mc.LOSS_KIND_BETA) if loss_fn != "bce" else dict(loss_fn="bce", kl_tolerance=0.0, beta=1.0)
    m = zoo.get(c, "fp32", create_batch=mc.CREATE_BATCH.get(cid), **kw)
    created = m.dev.max_batch
    r = mw.run_step(m, c)
    if cid in mc.CREATE_BATCH:
        assert created in (mc.CREATE_BATCH[cid], c.B) and m.dev.max_batch == c.B          # grown by ensure_batch inside the first pass
    ref = mc.reference(c, **kw)
    rows, bad = mc.step_report(ref, float(r["losses"][0]), float(r["losses"][1]), r["grads"])
    tag = "fp32" if loss_fn == "bce" else "fp32 " + loss_fn
    measure(c, tag, "reconstruction loss rel", rows[0][1], rows[0][2])
    measure(c, tag, "kl loss / (1e-4 rel + 4e-6)", rows[1][1], rows[1][2])
    worst = max(rows[2:], key=lambda x: x[1])
    measure(c, tag, "worst gradient (%s) / max" % worst[0][5:], worst[1], worst[2])
    assert np.isfinite(r["flat"]).all()
    assert not bad, bad
    ad = mc.adam_report(mc.params(c), r["grads"], r["params_after"])
    measure(c, tag, "Adam step / (2e-6 + 1e-5 max|w|)", max(ad.values()), 1.0)
    assert max(ad.values()) <= 1.0, ad
    # the inference surface on the updated weights (the device's own copy)
    want = mc.inference_reference(r["params_after"], c)
    d = mc.inputs(c)
    e_mean, e_gen = mc.rel_err(m.encode(d["src"]), want["mean"]), mc.rel_err(m.generate_from_latent(d["eps"]), want["gen"])
    measure(c, tag, "encode / max", e_mean, mc.INFER_BOUND)
    measure(c, tag, "generate_from_latent / max", e_gen, mc.INFER_BOUND)
    assert e_mean < mc.INFER_BOUND and e_gen < mc.INFER_BOUND
    if mc.P(c) != mc.S(c):                                  # the reference reshapes reconstructions with the SOURCE shape (vae/models.py:193-197): same failure here
        with pytest.raises(ValueError):
            m.reconstruct(d["src"], eps=d["eps"])
        return
    rec = m.reconstruct(d["src"], eps=d["eps"])
    assert len(rec) == c.B and rec[0].shape == c.src
    e_rec = mc.rel_err(np.stack([x.reshape(-1) for x in rec]), want["recon"])
    measure(c, tag, "reconstruct / max", e_rec, mc.INFER_BOUND)
    assert e_rec < mc.INFER_BOUND


# ---------------------------------------------------------------------------------------------------------------------------------------
# Part B
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c.id for c in mc.CASES if c.id not in mc.FP32_ONLY])
def test_bf16_engine_layer_by_layer(zoo, cid):
    """Every op of one forward + backward(part 0) of the bf16 engine against the float64 statement of that op on the engine's own stored tensors and its bf16 shadow
    weights, at the derived bounds of mlp_engine_cases.layer_report (ratio 1.0 = at the bound); the two losses against the oracle's bf16 emulation."""
    c = mc.by_id(cid)
    m = zoo.get(c, "bf16", create_batch=mc.CREATE_BATCH.get(cid))
    r = mw.run_step(m, c, grab=True, adam=False)
    assert np.isfinite(r["flat"]).all()
    m.dev.sync_shadow()
    R = mc.layer_report(c, r["stored"], r["grads"], m.dev.export_params(), mc.inputs(c))
    for name, worst in R.rows:
        measure(c, "bf16", name + " err / bound", worst, 1.0)
    assert not R.bad, R.bad
    rows, bad = mc.bf16_loss_report(c, float(r["losses"][0]), float(r["losses"][1]))
    for name, v in rows:
        measure(c, "bf16", name, v, 1.0)
    assert not bad, bad


@pytest.mark.parametrize("N", [16, 48, 80, 32])
@pytest.mark.parametrize("masked", [False, True])
def test_bf16_dense_output_of_16_mod_32_columns_stays_in_its_rows(N, masked):
    """What Part B found on case 2 (layer width 16; the run stopped there, and cases 3, 7 and 8, whose 16- and 48-wide bf16 tensors the same kernel writes, first ran
    with the fix), at the op: the bf16 epilogue of the tile kernels stored both 16-channel groups of every 32-column subtile, so with N = 16 (mod 32) row m's second group overwrote row m + 1's first 16 channels, the last row's went 32 bytes past the tensor, and the
    bias vector was read past its end.  mi_gemm_bias_act in the engine's form (K-contiguous weights; bias + ReLU forward, ReluGrad mask backward) against float64 at
    the layer_report bound, with sentinels behind the output; N = 32 keeps the paired-store path under the same assertions."""
    from hip_helpers import dev, host, stream
    from mi355 import lib as milib
    L = milib.get()
    M, K = 5, 24
    rng = np.random.RandomState(N + masked)
    a, w = mc.bf16r(rng.standard_normal((M, K))), mc.bf16r(rng.standard_normal((N, K)) / np.sqrt(K))
    bias = rng.standard_normal(N).astype(np.float32)
    mask = mc.bf16r(rng.standard_normal((M, N)))
    out = torch.full((M * N + 64,), -768.0, device="cuda", dtype=torch.bfloat16)
    a_d, w_d, b_d, m_d = dev(a, torch.bfloat16), dev(w, torch.bfloat16), dev(bias), dev(mask, torch.bfloat16)
    L.mi_gemm_bias_act(stream(), milib.MI_BF16, a_d.data_ptr(), M, K, w_d.data_ptr(), 1, N, None if masked else b_d.data_ptr(), 0 if masked else 1,
                       m_d.data_ptr() if masked else None, out.data_ptr(), 0, 1)
    got = host(out)
    assert (got[M * N:] == -768.0).all()
    R = mc.OpReport()
    R.product("N = %d" % N, got[:M * N].reshape(M, N), a, w.T, K, bias=None if masked else bias.astype(np.float64), relu=not masked, mask=(mask > 0) if masked else None)
    assert not R.bad, R.bad


def test_widths_and_precisions_the_engine_cannot_run_are_refused_by_name(tmp_path):
    c = mc.by_id(5)
    with pytest.raises(ValueError, match="multiple of 8.*got 4092"):
        mw.make_model(tmp_path, c, "bf16")
    with pytest.raises(ValueError, match="bf16x3"):
        mw.make_model(tmp_path, mc.by_id(1), "bf16x3")


# ---------------------------------------------------------------------------------------------------------------------------------------
# Part C
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,precision", combos(mc.IDENTITY_CASES))
def test_backward_stores_repeats_and_splits_into_parts(zoo, cid, precision):
    """C1 / C2: over a gradient buffer full of NaN backward(0) leaves every element finite, two runs are bitwise equal (plain stores, the slab sum's storing form and the
    one-wave kernel alike); backward(1) leaves grads[:decoder_offset] untouched and backward(2) completes the buffer to backward(0)'s bitwise."""
    c = mc.by_id(cid)
    m = zoo.get(c, precision)
    a = mw.run_step(m, c, adam=False)
    b = mw.run_step(m, c, adam=False)
    assert np.isfinite(a["flat"]).all() and np.array_equal(a["flat"], b["flat"]) and np.array_equal(a["losses"], b["losses"])
    dev, B = m.dev, c.B
    src, tgt, e = mw.tables(m, c)
    mw.reset(m, c)
    dev.forward(src, tgt, None, B, 1.0 / B, e, 1, 1)
    dev.grads.fill_(-7.0)
    dev.backward(src, None, e, 1.0 / B, 1)
    got = dev.grads.cpu().numpy()
    off = dev.decoder_offset
    assert off == sum(K * N + N for t, _, K, N in mc.layers(c) if not t.startswith("dec"))
    assert np.array_equal(got[off:], a["flat"][off:]) and (got[:off] == -7.0).all()
    dev.backward(src, None, e, 1.0 / B, 2)
    assert np.array_equal(dev.grads.cpu().numpy(), a["flat"])
    assert [tuple(x) for x in dev.grad_buckets] == [(1, off, dev.n_flat), (2, 0, off)]


@pytest.mark.parametrize("cid,precision", combos(mc.IDENTITY_CASES))
def test_three_steps_op_by_op_equal_three_one_call_steps(zoo, cid, precision):
    """C3: params, both Adam slots and weights_t after three forward + backward + apply_adam equal three mi_mlpvae_train_step calls bitwise."""
    c = mc.by_id(cid)
    m, m2 = zoo.get(c, precision), zoo.get(c, precision, tag="b")
    B = c.B
    for mm in (m, m2):
        mw.reset(mm, c)
    src, tgt, e = mw.tables(m, c)
    for _ in range(3):
        m.dev.forward(src, tgt, None, B, 1.0 / B, e, 1, 1)
        m.dev.backward(src, None, e, 1.0 / B, 0)
        m._adam_step()
        m2._train_minibatch(src, tgt, None, B, 1.0 / B, e)
    torch.cuda.synchronize()
    for name in ("params", "adam_m", "adam_v", "weights_t", "losses"):
        assert torch.equal(getattr(m.dev, name), getattr(m2.dev, name)), name
    assert not torch.equal(m.dev.params, torch.from_numpy(m.dev._to_flat(mc.params(c))).to(m.dev.device))


@pytest.mark.parametrize("cid,precision", combos(mc.IDENTITY_CASES))
def test_uint8_tables_equal_float_tables_in_every_mix(zoo, cid, precision):
    """C4: frames_u8 = 1, 2, 3 (source, target, both tables raw bytes) through an index vector equal the float tables of byte / 255 bitwise: losses and posterior means
    of two steps, parameters after them."""
    c = mc.by_id(cid)
    m = zoo.get(c, precision)
    B = c.B
    d = mc.inputs(c)
    rng = np.random.RandomState(40 + cid)
    N = B + 3                                               # a table of more rows than the minibatch, read through a permutation
    pick = rng.randint(0, B, N)
    perm = torch.from_numpy(np.stack([rng.permutation(N)[:B] for _ in range(2)]).astype(np.int32)).to(m.dev.device)
    e = torch.from_numpy(d["eps"]).to(m.dev.device)
    res = {}
    for u8 in (0, 1, 2, 3):
        mw.reset(m, c)
        src = torch.from_numpy(np.ascontiguousarray(d["src_u8" if u8 & 1 else "src"][pick].reshape(N, -1))).to(m.dev.device)
        tgt = torch.from_numpy(np.ascontiguousarray(d["tgt_u8" if u8 & 2 else "tgt"][pick].reshape(N, -1))).to(m.dev.device)
        assert m.dev._u8(src, tgt) == u8
        losses = []
        for s in range(2):
            m._train_minibatch(src, tgt, perm[s], B, 1.0 / B, e)
            losses.append(m.dev.losses.cpu().numpy().copy())
        mean = torch.empty(B, c.z, device=m.dev.device)
        m.dev.encode(src, perm[0], B, mean)
        res[u8] = (np.array(losses), mean.cpu().numpy(), m.dev.params.cpu().numpy().copy())
    for u8 in (1, 2, 3):
        for a, b, what in zip(res[u8], res[0], ("losses", "means", "parameters")):
            assert np.array_equal(a, b), (u8, what)
    assert np.isfinite(res[0][2]).all() and not np.array_equal(res[0][2], m.dev._to_flat(mc.params(c)))


@pytest.mark.parametrize("cid", mc.IDENTITY_CASES)
def test_fp32_layer0_reads_the_callers_table_or_the_staged_copy_alike(zoo, cid):
    """C5: idx = None (layer 0's forward and filter-gradient operand is the caller's table) equals idx = arange(B) (the staged copy) bitwise, over a table of more
    than B rows."""
    c = mc.by_id(cid)
    m = zoo.get(c, "fp32")
    B = c.B
    d = mc.inputs(c)
    extra = np.random.RandomState(50 + cid).randint(0, 256, (3, mc.S(c))).astype(np.float32) / np.float32(255)
    src = torch.from_numpy(np.concatenate([d["src"].reshape(B, -1), extra])).to(m.dev.device)
    tgt = torch.from_numpy(np.concatenate([d["tgt"].reshape(B, -1), np.zeros((3, mc.P(c)), np.float32)])).to(m.dev.device)
    e = torch.from_numpy(d["eps"]).to(m.dev.device)
    ar = torch.arange(B, dtype=torch.int32, device=m.dev.device)
    m.dev.stored("x", 0, B).fill_(float("nan"))             # idx = None must not read the staging region
    a = mw.run_step(m, c, src_tgt_eps=(src, tgt, e), idx=None)
    b = mw.run_step(m, c, src_tgt_eps=(src, tgt, e), idx=ar)
    for k in ("losses", "mean", "flat", "flat_after", "m", "v", "weights_t"):
        assert np.array_equal(a[k], b[k]), k
    assert np.isfinite(a["flat"]).all()


@pytest.mark.parametrize("cid,precision", combos(sorted(mc.SHORT_AFTER_LONG)))
def test_a_short_batch_behind_a_long_one_equals_a_fresh_engine(zoo, cid, precision):
    """C6: a step at B' < B on an engine that has just run batch B equals the same step on a fresh engine bitwise (stale rows of the workspace are never read)."""
    c = mc.by_id(cid)
    short = mc.SHORT_AFTER_LONG[cid]
    used, fresh = zoo.get(c, precision), zoo.get(c, precision, tag="fresh")
    mw.run_step(used, c)                                    # the long batch
    a = mw.run_step(used, c, B=short)
    fresh.dev.workspace.fill_(0xFF)                         # (NaN patterns in every region a kernel could read by mistake)
    b = mw.run_step(fresh, c, B=short)
    for k in ("losses", "mean", "flat", "flat_after", "m", "v", "weights_t"):
        assert np.array_equal(a[k], b[k]), k
    assert np.isfinite(a["flat"]).all() and np.isfinite(a["flat_after"]).all()


@pytest.mark.parametrize("precision", mc.PRECISIONS)
def test_an_engine_grown_by_ensure_batch_equals_one_created_large(zoo, precision):
    """C7: case 3 created at max_batch 4; the step at 33 rows re-creates engine and workspace and matches a model created at 128 bitwise."""
    c = mc.by_id(3)
    small = mw.make_model(zoo.root, c, precision, create_batch=4, tag="grow")
    try:
        assert small.dev.max_batch == 4
        ws_small = small.dev.workspace.numel()
        a = mw.run_step(small, c)
        assert small.dev.max_batch == c.B and small.dev.workspace.numel() > ws_small
        large = zoo.get(c, precision)
        assert large.dev.max_batch == 128
        b = mw.run_step(large, c)
        for k in ("losses", "mean", "flat", "flat_after", "m", "v", "weights_t"):
            assert np.array_equal(a[k], b[k]), k
        with pytest.raises(Exception, match="batch outside 1 .. max_batch"):      # the C entry itself refuses what the Python side did not grow for
            small.dev.L.mi_mlpvae_encode(small.dev.handle, small.dev.stream(), 1, 0, None, c.B + 1, 1)
    finally:
        small.dev.close()


@pytest.mark.parametrize("precision", mc.PRECISIONS)
def test_the_inference_engine_encodes_and_refuses_to_train(zoo, precision):
    """C8: a model built with training=False (with_optimizer = 0, engine at 16 rows, no gradient regions): encode of 33 frames against float64 (fp32: 1e-4 of max; bf16:
    against the oracle's bf16 emulation at the project's 3e-2 of max for a bf16 posterior mean); backward and apply_adam are refused with the engine's own message."""
    c = mc.by_id(3)
    m = zoo.get(c, precision, training=False)
    assert m.dev.max_batch == 16 and m.dev.grads is None and m.dev.stored("gd", 0, 4) is None and m.dev.stored("dheads", 0, 4) is None and m.dev.stored("h", 0, 4) is not None
    d = mc.inputs(c)
    got = m.encode(d["src"])
    assert m.dev.max_batch == c.B == 33
    if precision == "fp32":
        err, bound = mc.rel_err(got, mc.reference(c).mean), mc.INFER_BOUND
    else:
        err, bound = mc.rel_err(got, mc.reference(c, storage="bf16", dtype="f32").mean), 3e-2
    measure(c, precision, "inference engine encode / max", err, bound)
    assert err < bound
    gen = m.generate_from_latent(d["eps"])
    assert gen.shape == (c.B, mc.P(c)) and np.isfinite(gen).all()
    src, tgt, e = mw.tables(m, c)
    m.dev.forward(src, tgt, None, c.B, 1.0 / c.B, e, 0, 1)  # a forward pass runs (evaluation); want_grad is ignored without optimiser buffers
    with pytest.raises(Exception, match="mi_mlpvae_backward: engine created without optimiser buffers"):
        m.dev.backward(src, None, e, 1.0 / c.B, 0)
    with pytest.raises(Exception, match="mi_mlpvae_apply_adam: engine created without optimiser buffers"):
        m.dev.apply_adam(1e-5)


@pytest.mark.parametrize("cid,precision", combos((4, 7, 8)))
def test_split_products_write_the_slab_region_they_are_stated_to(zoo, cid, precision):
    """dense() falls back to the unsplit kernel without a word when the slab region is too small for ns x B x N floats, and Part B takes its slab counts from the
    restated gates.  Observed directly: over a slab region full of NaN (mi_mlpvae_buffer 12) a forward pass leaves written exactly the prefix its largest split
    product fills (case 4: 2 x 16 x 64 floats, case 7: 7 x 4 x 32, case 8: 4 x 3 x 64 of the output layer), and backward(0) alone exactly that of its largest split
    input gradient (case 8: 4 x 3 x 16 over N = 5120; none in cases 4 and 7) -- so every count route() states is the one the engine ran with, and no split layer
    fell back."""
    c = mc.by_id(cid)
    m = zoo.get(c, precision)
    dev, B = m.dev, c.B
    n_fwd, n_bwd = mw.split_prefix_floats(c, ("fwd",)), mw.split_prefix_floats(c, ("dgrad",))
    assert (n_fwd, n_bwd) == {4: (2 * 16 * 64, 0), 7: (7 * 4 * 32, 0), 8: (4 * 3 * 64, 4 * 3 * 16)}[cid]
    cap = max(n_fwd, n_bwd) + 64
    slab = dev._view(12, cap)
    assert dev.max_batch == 128 and slab.numel() == cap                # (the region is sized for 128 rows: the 64 floats behind the prefix are inside it)
    src, tgt, e = mw.tables(m, c)
    mw.reset(m, c)
    slab.fill_(float("nan"))
    dev.forward(src, tgt, None, B, 1.0 / B, e, 1, 1)
    torch.cuda.synchronize()
    written = ~torch.isnan(slab).cpu().numpy()
    assert written[:n_fwd].all() and not written[n_fwd:].any(), (int(written.sum()), n_fwd)
    slab.fill_(float("nan"))
    dev.backward(src, None, e, 1.0 / B, 0)
    torch.cuda.synchronize()
    written = ~torch.isnan(slab).cpu().numpy()
    assert written[:n_bwd].all() and not written[n_bwd:].any(), (int(written.sum()), n_bwd)
    assert np.isfinite(dev.grads.cpu().numpy()).all()


def _child(args, env, timeout=170):
    r = subprocess.run([sys.executable, WORKER] + args, env=dict(os.environ, **env), capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, "exit status %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return json.loads([line for line in r.stdout.splitlines() if line.startswith("{")][-1])


def test_one_stream_equals_two(zoo, tmp_path):
    """C9: MI355_MLP_STREAMS=0 is read when the library is loaded: a fresh child runs cases 2 and 8 on one stream; this process's default two-stream pass (the
    output layer's filter gradient under the chain, nine deferred ones behind it, two flushes, one join) gives its gradients and updated parameters bitwise."""
    assert os.environ.get("MI355_MLP_STREAMS") in (None, "1")
    out = _child(["streams", str(tmp_path)], {"MI355_MLP_STREAMS": "0"})
    assert out["cases"] == list(mc.STREAM_CASES)
    for cid, precision in combos(mc.STREAM_CASES):
        c = mc.by_id(cid)
        r = mw.run_step(zoo.get(c, precision), c)
        one = np.load(os.path.join(str(tmp_path), "streams_%d_%s.npz" % (cid, precision)))
        for k in ("losses", "flat", "flat_after"):
            assert np.array_equal(one[k], r[k]), (cid, precision, k)
        assert np.isfinite(r["flat"]).all()


# ---------------------------------------------------------------------------------------------------------------------------------------
# Part D
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_workspace_guards_stay_intact_and_name_an_overwritten_one():
    """MI355_DEBUG_GUARDS=1 in a fresh child: 256 patterned bytes behind every region of the workspace (case 3's regrown one included); after a training step, encode,
    reconstruct and generate_from_latent of cases 3, 7 and 8 in both precisions every guard holds (reconstruct through the device call itself, so that it runs where P != S too: cases 3 and 7); one guard then overwritten through a torch view of the engine's
    own workspace is the one the checker names."""
    out = _child(["guards"], {"MI355_DEBUG_GUARDS": "1"})
    assert set(out) == {"%d %s" % (cid, p) for cid, p in combos(mc.GUARD_CASES)}
    for key, r in out.items():
        assert r["n0"] == r["n"] == r["regions"] > 0 and r["bad0"] == 0 and r["bad"] == 0, (key, r)
        assert r["inside"] and r["bad_after"] == 1 and ("workspace guard %d (byte offset %d) overwritten" % (r["guard"], r["offset"])) in r["named"], (key, r)
