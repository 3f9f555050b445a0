"""The case table, references and route predicates of tests/vae_engine_cases.py checked without a GPU, the descriptor refusals of the ConvVAE engine
(latent widths and frame sizes the kernels cannot take) through the C ABI, and the stored-tensor cases of mi_vae_buffer on an engine over host memory
(mi_vae_create launches nothing)."""
import ctypes

import numpy as np
import pytest
import torch

import vae_engine_cases as vc
from oracle import vae_oracle as vo


def test_every_case_has_legal_sides_and_the_oracle_agrees_on_the_encoded_shape(tmp_path):
    from mi355.init import encoded_shape, vae_variables
    from vae.models import ConvVAE
    for c in vc.CASES + [vc.Z12]:
        assert vc.legal_side(c.H) and vc.legal_side(c.W), c
        g = vc.geom(c)
        assert g["dec"][4] == vc.tgt_shape(c), (c, g["dec"][4])                    # the decoder returns the source's height and width
        m = ConvVAE(np.array(vc.src_shape(c)), np.array(vc.tgt_shape(c)), z_dim=c.z, model_dir=str(tmp_path / str(c.id)), precision="fp32")
        assert vo.encoded_shape(vc.src_shape(c)) == m.encoded_shape == encoded_shape(vc.src_shape(c)) == g["enc"][4], c
        specs = vo.vae_variable_specs(c.z, vc.src_shape(c), vc.tgt_shape(c))
        assert dict(specs) == dict(vae_variables(c.z, vc.src_shape(c), vc.tgt_shape(c))) and list(specs) == list(m._variables), c
        assert c.B <= 33
    assert [s for s in range(40, 200) if vc.legal_side(s)] == [48, 64, 80, 96, 112, 128, 144, 160, 176, 192]
    assert vo.encoded_shape() == vo.ENCODED_SHAPE == (3, 8, 256)
    for bad in ((50, 160, 3), (80, 150, 3)):                                        # a side that is no 16 e + 32 fails the reference's assertion (vae/models.py:265)
        with pytest.raises(AssertionError):
            ConvVAE(np.array(bad), z_dim=64, model_dir=str(tmp_path / "bad"))


def test_every_case_takes_the_route_its_row_states():
    seen = {k: set() for k in ("enc_head", "head_bwd", "ares", "tail", "fuse_b4", "stream_mask", "conv1", "pair_launch")}
    for c in vc.CASES:
        for prec in vc.PRECISIONS:
            r = vc.route(c, prec, max_batch=vc.CREATE_BATCH.get(c.id, 128))
            want = (vc.STATED_BF16 if prec == "bf16" else vc.STATED_F32)[c.id]
            assert vc.route_tuple(r) == want, (c.id, prec, vc.route_tuple(r), want)
            assert r["ns_heads"] >= 1 and r["ns_dz"] >= 1
            for k in seen:
                seen[k].add(r[k])
    # every branch of every gate is taken by some (case, precision).  The mid-layer activation-resident forms depend on channel counts alone, which no ConvVAE changes:
    # "mid" is reached exactly where "on" is (case 7, bf16) and nowhere else.
    assert seen["enc_head"] == {"fused", "two launches"} and seen["head_bwd"] == {"fused", "layer ops"} and seen["ares"] == {"on+mid", "off"}
    assert seen["tail"] == {"fused", "epilogue", "plain"} and seen["fuse_b4"] == {True, False} and seen["stream_mask"] == {1, 5}
    assert seen["conv1"] == {"narrow", "general"} and seen["pair_launch"] == {True, False}
    # inference engines never fuse the tail and write no ReLU bit words
    r = vc.route(vc.by_id(7), "bf16", training=False)
    assert r["tail"] == "epilogue" and r["head_bwd"] == "layer ops" and r["enc_head"] == "fused"
    # the split counts at the model's own shape: what the engine's comments quote (16 slabs for both latent sums at batch 512)
    assert vc.pick_split(512, 128, 6144, 32) == 16 and vc.pick_split(512, 64, 6144, 32) == 16
    # the smallest model has one K block per slab at most: flat 256 in bf16 (bk 32) gives 8 slabs, never an empty one
    assert vc.route(vc.by_id(1), "bf16")["ns_heads"] == 8 and vc.route(vc.by_id(1), "fp32")["ns_heads"] == 16


def test_the_reference_at_the_models_shape_is_todays_oracle_bitwise():
    c = vc.by_id(7)
    d, p = vc.inputs(c), vc.params(c)
    ref = vc.reference(c)
    (recon, kl, _), grads, fw = vo.vae_loss_and_grads(p, d["src"], d["tgt"], d["eps"], dtype=torch.float64)       # the module constant ENCODED_SHAPE
    assert (recon, kl) == (ref.recon, ref.kl) and np.array_equal(fw["mean"].numpy(), ref.mean)
    assert all(np.array_equal(grads[k], ref.grads[k]) for k in grads)
    o = vo.OracleVAE(vc.src_shape(c), vc.tgt_shape(c), c.z, params=p, training=False, dtype=torch.float64)
    assert np.array_equal(o.encode(d["src"]), vc.inference_reference(c)["mean"].astype(np.float32))


# the fp32 oracle alone against float64 on every row, measured on the CPU: the figures the issue states.  Asserted at 10 x margin: the device bounds of Part A
# (2e-4 / 1e-4 / 1e-4 / 1e-4) then leave the implementation under test at least 90 % of each bound.
ALONE = {"grad": 2.6e-6, "kl": 7.9e-7, "recon": 1.0e-7, "mean": 7.6e-7}


@pytest.mark.parametrize("cid", [c.id for c in vc.CASES])
def test_the_fp32_oracle_alone_is_well_inside_the_bounds(cid):
    c = vc.by_id(cid)
    ref, o32 = vc.reference(c), vc.reference(c, dtype="f32")
    rows, bad = vc.step_report(ref, o32.recon, o32.kl, o32.mean, o32.grads, "fp32")
    assert not bad, bad
    worst_grad = max(v for n, v, _ in rows if n.startswith("grad "))
    print("case %d: fp32 oracle vs float64: recon %.2e kl %.2e mean %.2e worst grad %.2e" % (cid, rows[0][1], rows[1][1], rows[2][1], worst_grad))
    assert rows[0][1] <= 10 * ALONE["recon"] and rows[1][1] <= 10 * ALONE["kl"] and rows[2][1] <= 10 * ALONE["mean"] and worst_grad <= 10 * ALONE["grad"], rows
    assert len([n for n, _, _ in rows if n.startswith("grad ")]) == 22
    # the optimiser statement holds for the oracle's own update
    after = {k: v.copy() for k, v in vc.params(c).items()}
    vo.AdamTF({k: v.shape for k, v in after.items()}).step(after, o32.grads, vc.LR)
    assert max(vc.adam_report(vc.params(c), o32.grads, after).values()) == 0.0


@pytest.mark.parametrize("loss_fn", ["bce_v2", "mse"])
@pytest.mark.parametrize("cid", vc.LOSS_KIND_CASES)
def test_the_other_loss_kinds_clamp_some_rows_and_stay_inside_the_bounds(cid, loss_fn):
    c = vc.by_id(cid)
    tol = vc.KL_TOLERANCE[cid]
    ref, o32 = vc.reference(c, loss_fn=loss_fn, kl_tolerance=tol), vc.reference(c, dtype="f32", loss_fn=loss_fn, kl_tolerance=tol)
    _, bad = vc.step_report(ref, o32.recon, o32.kl, o32.mean, o32.grads, "fp32")
    assert not bad, bad
    kl_b = -0.5 * (1 + ref.logvar - ref.mean ** 2 - np.exp(ref.logvar)).sum(1)
    assert list(kl_b < tol * c.z) == [True, False, True]                           # some rows clamped, one not: both branches of the KL gradient's switch
    assert np.abs(kl_b / (tol * c.z) - 1).min() > 0.04                             # ... and none near the threshold
    assert ref.kl == pytest.approx(np.maximum(kl_b, tol * c.z).mean(), rel=1e-12)


def test_a_misstated_encoded_shape_fails_part_a():
    """Swap H and W of the encoded shape in the reference (case 2: 1 x 5 -> 5 x 1): the decoder's reshape then feeds deconv1 another map, and the assertions of Part A,
    given the correct implementation (the fp32 oracle stands in for the device), fail on the reconstruction loss and on every decoder gradient."""
    c = vc.by_id(2)
    good = vc.reference(c, dtype="f32")
    eh, ew, ec = vo.encoded_shape(vc.src_shape(c))
    assert (eh, ew) == (1, 5)
    wrong = vc.reference(c, encoded=(ew, eh, ec))
    _, bad = vc.step_report(wrong, good.recon, good.kl, good.mean, good.grads, "fp32")
    names = {b[0] for b in bad}
    assert "grad vae/decoder/deconv1/kernel" in names and "grad vae/decoder/dense1/kernel" in names and "grad vae/encoder/conv1/kernel" in names, names
    _, bad = vc.step_report(wrong, good.recon, good.kl, good.mean, good.grads, "bf16x3")       # ... at the bf16x3 bound as well
    assert "grad vae/decoder/deconv1/kernel" in {b[0] for b in bad}


def test_a_misstated_slab_layout_fails_the_posterior_mean():
    """The heads' split-K slabs are [ns][B][2 z] with the CURRENT batch as the middle dimension.  Summing them with max_batch there reads other rows' partial sums:
    the posterior-mean bound of Part A catches it (and the correctly stated sum reproduces the mean to rounding)."""
    c = vc.by_id(1)
    ref, d, p = vc.reference(c), vc.inputs(c), vc.params(c)
    with torch.no_grad():
        P = {k: torch.from_numpy(v).double() for k, v in p.items()}
        flat = vo.vae_forward(P, d["src"], sample=False, dtype=torch.float64, keep=True, encoded=vo.encoded_shape(vc.src_shape(c)))["conv4"].reshape(c.B, -1).numpy()
    wh = np.concatenate([p["vae/mean/kernel"], p["vae/logstd_sqare/kernel"]], 1).astype(np.float64)
    ns, max_batch = 8, 128
    K = flat.shape[1] // ns
    slabs = np.zeros((ns, c.B, 2 * c.z))
    for s in range(ns):
        slabs[s] = flat[:, s * K:(s + 1) * K] @ wh[s * K:(s + 1) * K]
    buf = np.zeros(ns * max_batch * 2 * c.z)
    buf[:slabs.size] = slabs.reshape(-1)
    right = vc.sum_slabs(buf, ns, c.B, c.B, 2 * c.z)[:, :c.z] + p["vae/mean/bias"]
    wrong = vc.sum_slabs(buf, ns, max_batch, c.B, 2 * c.z)[:, :c.z] + p["vae/mean/bias"]
    assert vc.rel_err(right, ref.mean) < 1e-12
    assert vc.rel_err(wrong, ref.mean) > 100 * vc.MEAN_BOUND


@pytest.mark.parametrize("cid", [1, 5])
def test_the_layer_report_passes_a_faithful_engine_and_fails_a_dropped_tap_row(cid):
    """Part B's checker on a CPU stand-in that stores what the bf16 engine stores (one fused and one unfused route): every layer inside its bound, with the
    stores' bf16 roundings the only differences; with a tap row of deconv1's kernel dropped from the REFERENCE, deconv1's forward output and input gradient fail."""
    c = vc.by_id(cid)
    rt = vc.route(c, "bf16")
    st, g = vc.cpu_engine_state(c, rt)
    assert (st["gdec4"] is None) == (rt["tail"] == "fused") and (st["gact1"] is None) == (rt["head_bwd"] == "fused") and (st["dec4"] is None) == (rt["tail"] != "plain")
    R = vc.layer_report(c, st, g, vc.params(c), vc.inputs(c), rt)
    assert not R.bad and len(R.rows) >= 41, R.bad
    assert max(r[2] for r in R.rows if not isinstance(r[2], tuple)) < 0.6            # a bf16 store is within 2^-9 = 0.49 of the 4e-3 relative bound
    R = vc.layer_report(c, st, g, vc.params(c), vc.inputs(c), rt, drop_tap_row=0)
    assert {b[0] for b in R.bad} == {"deconv1.fwd", "deconv1.dgrad"}, R.bad
    g2 = dict(g)
    g2["vae/decoder/deconv2/kernel"] = np.swapaxes(g["vae/decoder/deconv2/kernel"], 0, 1).copy()      # a filter gradient with kh and kw exchanged
    R = vc.layer_report(c, st, g2, vc.params(c), vc.inputs(c), rt)
    assert [b[0] for b in R.bad] == ["deconv2.wgrad"], R.bad


def test_the_inference_form_check_passes_a_faithful_head_and_fails_a_misstated_one():
    """Part B's third unstored intermediate, conv1's output behind the inference form of the fused encoder head (case 7): a float64 stand-in that stores conv2's output
    alone passes; the same reference without conv1's ReLU fails."""
    c = vc.by_id(7)
    st, _ = vc.cpu_engine_state(c, vc.route(c, "bf16"))
    R = vc.encoder_head_inference_report(c, st["act2"], vc.params(c), vc.inputs(c))
    assert not R.bad and R.rows[0][2] < 0.6, R.rows
    assert vc.encoder_head_inference_report(c, st["act2"], vc.params(c), vc.inputs(c), conv1_relu=False).bad


def test_the_rollout_assertions_fail_a_misstated_row():
    """Part E's assertions on a CPU stand-in (the fp32 oracle's encode + predict as the 'device', float64 latents as the reference): the right rows pass; latents taken
    from the neighbouring frame, or a value from the neighbouring row, fail."""
    from oracle import ppo_oracle as po
    c = vc.by_id(1)
    rng = np.random.RandomState(5)
    n, A = 3, 2
    frames = rng.randint(0, 256, (n,) + vc.src_shape(c)).astype(np.float32) / np.float32(255.0)
    meas = np.stack([rng.uniform(-1, 1, n), rng.uniform(0, 1, n), rng.uniform(0, 30, n)], axis=1).astype(np.float32)
    kw = dict(params=vc.params(c), training=False)
    z32 = vo.OracleVAE(vc.src_shape(c), vc.tgt_shape(c), c.z, **kw).encode(frames)
    z64 = vo.OracleVAE(vc.src_shape(c), vc.tgt_shape(c), c.z, dtype=torch.float64, **kw).encode(frames)
    o = po.OraclePPO([c.z + 3], po.ActionSpace(), seed=2, initial_std=1.0)
    a, v = o.predict(np.concatenate([z32, meas], 1), greedy=True)
    got = np.concatenate([np.asarray(a).reshape(n, A), np.asarray(v).reshape(n, 1), z32], 1)
    a_o, v_o = o.predict(np.concatenate([z64, meas], 1), greedy=True)
    a_o, v_o = np.asarray(a_o).reshape(n, A), np.asarray(v_o).reshape(n)
    assert vc.rollout_failures(got, z64, a_o, v_o, A) == []
    assert {b[1] for b in vc.rollout_failures(got, np.roll(z64, 1, 0), a_o, v_o, A)} == {"latent"}
    assert {b[1] for b in vc.rollout_failures(got, z64, a_o, np.roll(v_o, 1), A)} == {"value"}


# ---------------------------------------------------------------------------------------------------------------------------------------
# Part D: descriptors the engine refuses, through the C ABI (pure host functions of the descriptor)
# ---------------------------------------------------------------------------------------------------------------------------------------
def _desc(dtype, z, ih=48, iw=48, B=4, inference_only=0, cin=3, ct=3):
    from mi355 import lib as milib
    return milib.MiVaeDesc(dtype, B, ih, iw, cin, ct, z, 0, 1.0, 0.0, inference_only)


def _refused(d, *words):
    from mi355 import lib as milib
    L = milib.get()
    for fn in (L.mi_vae_param_floats, L.mi_vae_workspace_bytes):
        assert fn(ctypes.byref(d)) == -1
        msg = L.cdll.mi_last_error().decode()
        assert all(w in msg for w in words), (msg, words)
    assert not L.mi_vae_create(ctypes.byref(d), None, None, None, None, None, None, None, 0)
    msg = L.cdll.mi_last_error().decode()
    assert all(w in msg for w in words) and "mi_vae_create" in msg, (msg, words)


def test_latent_widths_the_kernels_cannot_take_are_refused_by_name():
    from mi355 import lib as milib
    L = milib.get()
    F32, BF16, X3 = milib.MI_F32, milib.MI_BF16, milib.MI_BF16X3
    _refused(_desc(BF16, 10), "z_dim 10", "multiple of 8")
    _refused(_desc(BF16, 12), "z_dim 12", "multiple of 8")
    _refused(_desc(F32, 10), "z_dim 10", "multiple of 4")
    _refused(_desc(X3, 10), "z_dim 10", "multiple of 4")
    _refused(_desc(F32, 0), "z_dim 0", "multiple of 4")
    for dt, zs in ((F32, (12, 8, 24, 40, 128)), (X3, (12, 8, 24, 40, 128)), (BF16, (8, 24, 40, 128))):
        for z in zs:
            d = _desc(dt, z)
            assert L.mi_vae_param_floats(ctypes.byref(d)) > 0 and L.mi_vae_workspace_bytes(ctypes.byref(d)) > 0, (dt, z)
    # the restated rule is the engine's
    for prec, dt in (("fp32", F32), ("bf16x3", X3), ("bf16", BF16)):
        for z in range(1, 41):
            ok = L.mi_vae_param_floats(ctypes.byref(_desc(dt, z))) > 0
            assert ok == (z % vc.z_dim_multiple(prec) == 0), (prec, z)


def test_frame_sizes_the_decoder_cannot_return_are_refused():
    from mi355 import lib as milib
    L = milib.get()
    _refused(_desc(milib.MI_BF16, 64, ih=45, iw=160), "geometry", "45 x 160")
    _refused(_desc(milib.MI_BF16, 64, ih=80, iw=47), "geometry", "80 x 47")        # the encoder runs 47 wide (as 46), the decoder returns 48: the loss would read the
    _refused(_desc(milib.MI_F32, 64, ih=46, iw=46), "geometry")                    # target table with the wrong stride
    for side in (48, 64, 80, 96, 192):
        assert L.mi_vae_param_floats(ctypes.byref(_desc(milib.MI_BF16, 64, ih=side, iw=48))) > 0, side


def test_convvae_refuses_the_width_before_anything_is_allocated(tmp_path):
    from vae.models import ConvVAE
    for prec, z in (("bf16", 10), ("bf16", 12), ("fp32", 10), ("bf16x3", 10)):
        with pytest.raises(ValueError, match="z_dim %d.*multiple of %d" % (z, vc.z_dim_multiple(prec))):
            ConvVAE(np.array([48, 48, 3]), z_dim=z, model_dir=str(tmp_path), precision=prec)
    m = ConvVAE(np.array([48, 48, 3]), z_dim=12, model_dir=str(tmp_path), precision="fp32")
    assert m.dev is None


# ---------------------------------------------------------------------------------------------------------------------------------------
# mi_vae_buffer's stored-tensor cases on engines over HOST memory: mi_vae_create stores pointers and launches nothing
# ---------------------------------------------------------------------------------------------------------------------------------------
def _aligned(nbytes):
    raw = np.zeros(nbytes + 256, np.uint8)
    off = (-raw.ctypes.data) % 256
    return raw, raw.ctypes.data + off


def _host_engine(d):
    from mi355 import lib as milib
    L = milib.get()
    n, ws = L.mi_vae_param_floats(ctypes.byref(d)), L.mi_vae_workspace_bytes(ctypes.byref(d))
    assert n > 0 and 0 < ws < (1 << 28)
    keep = [_aligned(4 * n) for _ in range(3)] + [_aligned(ws)]
    h = L.mi_vae_create(ctypes.byref(d), keep[0][1], None, None, None, keep[1][1], keep[2][1], keep[3][1], ws)
    assert h, L.cdll.mi_last_error()
    return L, h, keep, ws


@pytest.mark.parametrize("ih,iw,act1", [(80, 160, False), (48, 48, True)])
def test_stored_tensor_queries_return_null_where_the_workspace_has_no_region(ih, iw, act1):
    """An inference-only bf16 engine carves no gradient regions, and no conv1 output behind the fused encoder head (80 x 160 only): mi_vae_buffer returns NULL there
    (not workspace - 1), a pointer inside the workspace everywhere else, and NULL for every undeclared `which`."""
    from mi355 import lib as milib
    L, h, keep, ws = _host_engine(_desc(milib.MI_BF16, 16, ih=ih, iw=iw, B=2, inference_only=1))
    try:
        base = keep[3][1]
        seen = set()
        for which in [20 + i for i in range(1, 5)] + [30 + i for i in range(5)]:
            a = L.mi_vae_buffer(h, which)
            if which == 21 and not act1:
                assert a is None
                continue
            assert a is not None and base <= a < base + ws and a % 256 == 0 and a not in seen, which
            seen.add(a)
        for which in [40 + i for i in range(1, 5)] + [50 + i for i in range(5)] + [60]:
            assert L.mi_vae_buffer(h, which) is None, which
        for which in (-1, 17, 19, 20, 25, 29, 35, 40, 45, 49, 55, 59, 61, 100):
            assert L.mi_vae_buffer(h, which) is None, which
        assert L.mi_vae_buffer(h, 0) is not None and L.mi_vae_buffer(h, 5) is not None and L.mi_vae_buffer(h, 6) is None
    finally:
        L.mi_vae_destroy(h)
