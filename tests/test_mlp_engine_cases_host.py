"""The case table, references and route predicates of tests/mlp_engine_cases.py checked without a GPU: the conditions on the inputs (ReLU margin, the reference's
own room, KL tolerances), the restated gates against the written-down table, the comparison helpers against deliberately mis-stated references, and the host side
of the MlpVAE engine through the C ABI (parameter layout, workspace carve with and without MI355_DEBUG_GUARDS, mi_mlpvae_buffer on an engine over host memory:
mi_mlpvae_create stores pointers and launches nothing)."""
import ctypes

import numpy as np
import pytest

import mlp_engine_cases as mc
from oracle import vae_oracle as vo

IDS = [c.id for c in mc.CASES]


def test_the_case_table_is_the_issues():
    assert [(c.id, mc.S(c), mc.P(c), c.enc, c.dec, c.z, c.B, c.shift) for c in mc.CASES] == [
        (1, 8, 8, (8,), (8,), 8, 1, 0), (2, 72, 72, (40, 24, 16, 8), (8, 16, 24, 40), 16, 5, 0), (3, 192, 64, (64, 32, 16), (48,), 24, 33, 0),
        (4, 4096, 768, (64, 32), (32, 64), 32, 16, 0), (5, 4092, 20, (12,), (20,), 12, 3, 0), (6, 4104, 4104, (32,), (32,), 8, 2, 0),
        (7, 38528, 6152, (32,), (16,), 16, 4, 0), (8, 64, 64, (4224, 16), (16, 5120), 2048, 3, 500), (9, 768, 768, (128, 128), (128, 256), 64, 48, 800)]
    for c in mc.CASES:
        widths = (mc.S(c), mc.P(c), c.z) + c.enc + c.dec
        assert all(w % 4 == 0 for w in widths), c
        assert all(w % 8 == 0 for w in widths) == (c.id not in mc.FP32_ONLY), c
        specs = vo.mlp_vae_variable_specs(c.z, c.src, c.tgt, c.enc, c.dec)
        assert {k: v.shape for k, v in mc.params(c).items()} == dict(specs)
        assert sum(int(np.prod(s)) for s in specs.values()) <= 1.35e6                          # ("1.3 M parameters" at the most: case 7)
        d = mc.inputs(c)
        assert d["src_u8"].shape == (c.B,) + c.src and d["tgt_u8"].shape == (c.B,) + c.tgt and d["eps"].shape == (c.B, c.z)
        assert np.array_equal(d["src"], d["src_u8"].astype(np.float32) / np.float32(255))


def test_every_case_takes_the_route_its_row_states():
    seen = {"wgrad": set(), "split": set(), "fwd": set(), "dgrad": set()}
    for c in mc.CASES:
        st = mc.STATED[c.id]
        for prec in mc.precisions(c):
            fwd, dgrad, split, wgrad = mc.stated_view(c, prec)
            assert fwd == st["fwd"] and dgrad == st["dgrad"], (c.id, prec, fwd, dgrad)
            assert wgrad == st["wgrad_" + prec], (c.id, prec, wgrad)
            want_split = st["split_bf16"] if prec == "bf16" else {k: "gemm2" for k in st["split_bf16"]}
            assert split == want_split, (c.id, prec, split)
            seen["wgrad"].update((prec, w) for w in wgrad)
            seen["split"].update(split.values())
            seen["fwd"].update(fwd)
            seen["dgrad"].update(x for x in dgrad if x)
        assert st["wgrad_bf16"] is not None or c.id in mc.FP32_ONLY
    # every family the models of up to 1.3 M parameters can reach is reached (dwg_kernel needs K N >= 4 M elements: tests/test_zzz_dense_shapes_gpu.py has it)
    assert seen["wgrad"] == {("fp32", mc.O), ("fp32", mc.SL), ("bf16", mc.O), ("bf16", mc.WS)}
    assert seen["split"] == {"tallk", "gemm2"} and seen["fwd"] == {1, 2, 3, 4, 7} and seen["dgrad"] == {1, 2, 4}
    assert "dwg" not in {mc.wgrad_family("bf16", c.B, K, N) for c in mc.CASES for _, _, K, N in mc.layers(c)}
    assert mc.wgrad_family("bf16", 16, 38400, 512) == "dwg" and mc.wgrad_family("bf16", 16, 256, 64) == "dwgs" and mc.wgrad_family("fp32", 16, 256, 64) == mc.O
    # what the rows say about themselves
    assert mc.splitk_slabs(4096) == 2 and mc.splitk_slabs(4095) == mc.splitk_slabs(4092) == mc.splitk_slabs(4104) == 1 and mc.splitk_slabs(38400) == 30
    assert mc.splitk_walk(38528) == list(range(30, 6, -1)) and mc.splitk_slabs(38528) == 7 and 38528 == 301 * 128
    assert mc.splitk_slabs(4224) == 3 and mc.splitk_slabs(5120) == 4 and mc.splitk_slabs(6152) == 1 and mc.splitk_slabs(2048) == 1
    assert mc.split_kernel("bf16", 32, 38528, 7) == "gemm2" and mc.split_kernel("bf16", 32, 38528, 8) == "tallk" and mc.split_kernel("bf16", 64, 4096, 2) == "tallk"
    c4 = mc.by_id(4)
    assert mc.layers(c4)[0][2] * mc.layers(c4)[0][3] == 262144 and mc.wgrad_family("bf16", 16, 4096 + 64, 64) == mc.O      # at the one-wave kernel's cap; past it: gen 1
    assert mc.loss_chunks(mc.P(mc.by_id(7))) == 2 and mc.P(mc.by_id(7)) - mc.BCE_CHUNK == 8 and mc.loss_chunks(mc.P(mc.by_id(5))) == 1 and mc.P(mc.by_id(5)) < mc.BCE_CHUNK
    # row splits of the first-generation kernel: one (plain stores) wherever the batch fits a row block, several (the engine's scratch pieces) in fp32 at B = 33 / 48
    assert set(mc.route(mc.by_id(3), "fp32")["row_splits"]) == {3} and set(mc.route(mc.by_id(9), "fp32")["row_splits"]) == {3}
    assert set(mc.route(mc.by_id(3), "bf16")["row_splits"]) == {1}
    # four layers per side: ten kernels in Adam's table, nine filter gradients behind the chain (all but the output layer's)
    assert len(mc.layers(mc.by_id(2))) == 10


def test_the_scratch_pieces_cover_every_row_count():
    """wgrad_on hands every layer a piece sized for 2^20 rows; prepare_wgrad asks for splits x slab at the real row count.  The piece covers it at every batch."""
    for c in mc.CASES:
        for prec in mc.precisions(c):
            for _, _, K, N in mc.layers(c):
                piece = mc.wgrad_scratch_bytes(prec, 1 << 20, K, N)
                for M in list(range(1, 130)) + [c.B, 512, 4096]:
                    assert mc.wgrad_scratch_bytes(prec, M, K, N) <= piece, (c.id, prec, K, N, M)


# ---------------------------------------------------------------------------------------------------------------------------------------
# conditions on the inputs
# ---------------------------------------------------------------------------------------------------------------------------------------
MARGIN_STATED = {1: 4.2e-2, 2: 1.5e-4, 3: 2.2e-5, 4: 1.9e-4, 5: 2.3e-3, 6: 8.7e-3, 7: 1.4e-3, 8: 3.2e-5, 9: 3.0e-5}


@pytest.mark.parametrize("cid", IDS)
def test_walk_is_the_oracle_and_every_relu_keeps_its_margin(cid):
    c = mc.by_id(cid)
    w, ref = mc.walk(c), mc.reference(c)
    assert w.recon == pytest.approx(ref.recon, rel=1e-12) and w.kl == pytest.approx(ref.kl, rel=1e-12)
    assert mc.rel_err(w.st["mean"], ref.mean) < 1e-12 and mc.rel_err(w.st["logvar"], ref.logvar) < 1e-12
    assert set(w.grads) == set(ref.grads)
    for k in ref.grads:
        assert mc.rel_err(w.grads[k], ref.grads[k]) < 1e-11, k
    assert len(w.pre) == len(c.enc) + len(c.dec)
    m = mc.relu_margin(w)
    print("case %d: worst ReLU margin %.2e" % (cid, m))
    assert m >= mc.RELU_MARGIN, (cid, m)
    assert m == pytest.approx(MARGIN_STATED[cid], rel=0.06), (cid, m)


def test_the_unshifted_seeds_of_cases_8_and_9_miss_the_margin():
    """Why the two rows carry a shift: at shift 0 one pre-activation sits closer to zero than the margin; the shifts are the first multiples of 100 that meet it."""
    for cid, first in ((8, 500), (9, 800)):
        c = mc.by_id(cid)
        ms = {s: mc.relu_margin(mc.walk(c, d=mc.inputs(c, shift=s))) for s in range(0, first + 100, 100)}
        print("case %d margins by shift: %s" % (cid, {s: "%.1e" % v for s, v in ms.items()}))
        assert all(ms[s] < mc.RELU_MARGIN for s in range(0, first, 100)) and ms[first] >= mc.RELU_MARGIN, ms


ROOM = 1e-5                                # the fp32 oracle alone against float64: ten times inside the 1e-4 of Part A


@pytest.mark.parametrize("cid", IDS)
def test_the_fp32_oracle_alone_is_ten_times_inside_the_bounds(cid):
    c = mc.by_id(cid)
    ref, o32 = mc.reference(c), mc.reference(c, dtype="f32")
    rows, bad = mc.step_report(ref, o32.recon, o32.kl, o32.grads)
    assert not bad, bad
    worst = max(v for n, v, _ in rows if n.startswith("grad "))
    recon_rel, kl_rel = abs(o32.recon / ref.recon - 1), abs(o32.kl / ref.kl - 1)
    print("case %d: fp32 oracle vs float64 (bce): recon %.2e kl %.2e worst grad %.2e" % (cid, recon_rel, kl_rel, worst))
    assert recon_rel <= ROOM and kl_rel <= ROOM and worst <= ROOM, rows
    assert len(rows) == 2 + 2 * (len(c.enc) + len(c.dec) + 3)
    after = {k: v.copy() for k, v in mc.params(c).items()}
    vo.AdamTF({k: v.shape for k, v in after.items()}).step(after, o32.grads, mc.LR)
    assert max(mc.adam_report(mc.params(c), o32.grads, after).values()) == 0.0


@pytest.mark.parametrize("loss_fn", ["bce_v2", "mse"])
@pytest.mark.parametrize("cid", mc.LOSS_KIND_CASES)
def test_the_other_loss_kinds_clamp_some_rows_and_keep_the_room(cid, loss_fn):
    c = mc.by_id(cid)
    tol, beta = mc.KL_TOLERANCE[cid], mc.LOSS_KIND_BETA
    ref, o32 = mc.reference(c, loss_fn=loss_fn, kl_tolerance=tol, beta=beta), mc.reference(c, dtype="f32", loss_fn=loss_fn, kl_tolerance=tol, beta=beta)
    rows, bad = mc.step_report(ref, o32.recon, o32.kl, o32.grads)
    assert not bad, bad
    worst = max(v for n, v, _ in rows if n.startswith("grad "))
    print("case %d %s: fp32 oracle vs float64: worst grad %.2e" % (cid, loss_fn, worst))
    assert worst <= ROOM and abs(o32.recon / ref.recon - 1) <= ROOM and abs(o32.kl / ref.kl - 1) <= ROOM
    kl_z = mc.kl_rows(ref.mean, ref.logvar) / c.z
    print("case %d: KL / z per row %s" % (cid, np.round(kl_z, 3)))
    assert list(kl_z < tol) == mc.KL_CLAMPED[cid] and True in mc.KL_CLAMPED[cid] and False in mc.KL_CLAMPED[cid]
    assert np.abs(kl_z / tol - 1).min() >= 0.15                                    # no row near the threshold
    w = mc.walk(c, loss_fn=loss_fn, kl_tolerance=tol, beta=beta)
    assert w.recon == pytest.approx(ref.recon, rel=1e-12) and w.kl == pytest.approx(ref.kl, rel=1e-12)
    for k in ref.grads:
        assert mc.rel_err(w.grads[k], ref.grads[k]) < 1e-11, k


# ---------------------------------------------------------------------------------------------------------------------------------------
# the comparison helpers fail deliberately mis-stated references
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [2, 3, 8])
def test_part_a_fails_misstated_references(cid):
    """The fp32 oracle stands in for the device.  References with the heads' halves swapped, one bias gradient zeroed, or the decoder's last ReLU mask left out fail
    the gradient assertions of Part A; the reference stated right passes."""
    c = mc.by_id(cid)
    good = mc.reference(c, dtype="f32")
    right = mc.walk(c)
    ref = lambda w: mc.Ref(w.recon, w.kl, w.grads, w.st["mean"], w.st["logvar"])     # noqa: E731
    assert not mc.step_report(ref(right), good.recon, good.kl, good.grads)[1]
    swapped = mc.walk(c, mutate="swap_heads")
    names = {b[0] for b in mc.step_report(ref(swapped), good.recon, good.kl, good.grads)[1]}
    assert {"grad vae/mean/kernel", "grad vae/logstd_sqare/kernel", "grad vae/mean/bias", "kl loss |err| / (1e-4 |ref| + 4e-6)"} <= names, names
    zeroed = dict(right.grads)
    zeroed[mc.layer_name("decoder", 0) + "/bias"] = np.zeros_like(zeroed[mc.layer_name("decoder", 0) + "/bias"])
    names = [b[0] for b in mc.step_report(mc.Ref(right.recon, right.kl, zeroed, None, None), good.recon, good.kl, good.grads)[1]]
    assert names == ["grad vae/decoder/dense/bias"], names
    nomask = mc.walk(c, mutate="no_last_mask")
    names = {b[0] for b in mc.step_report(ref(nomask), good.recon, good.kl, good.grads)[1]}
    last_hidden = mc.layer_name("decoder", len(c.dec) - 1)
    assert "grad %s/kernel" % last_hidden in names and "grad %s/bias" % last_hidden in names and "grad vae/encoder/dense/kernel" in names, names
    assert "grad %s/kernel" % mc.layer_name("decoder", len(c.dec)) not in names      # the output layer's own gradients do not pass through that mask


@pytest.mark.parametrize("cid", [2, 4, 8])
def test_the_layer_report_passes_a_faithful_engine_and_fails_misstated_ops(cid):
    """Part B's checker on a CPU stand-in that stores what the bf16 engine stores: every op inside its bound, the bf16 stores' roundings the only differences (at
    half a bf16 step, 2^-8 of a value just above a power of two: ratio < 1); then the three mis-statements, each failing exactly the ops it touches."""
    c = mc.by_id(cid)
    w = mc.walk(c, storage="bf16")
    p, d = mc.params(c), mc.inputs(c)
    R = mc.layer_report(c, w.st, w.grads, p, d)
    n_layers = len(mc.layers(c))
    assert not R.bad and len(R.rows) == 4 * n_layers + 5, (R.bad, len(R.rows))        # 3 products per layer (no input gradient for layer 0), 6 elementwise ops
    assert max(r[1] for r in R.rows if "grad" in r[0] and "dgrad" not in r[0]) == 0.0    # fp32 outputs of the stand-in are the statement itself
    R = mc.layer_report(c, w.st, w.grads, p, d, mutate="swap_heads")
    assert {b[0] for b in R.bad} == {"heads.fwd raw", "heads.bias mean", "heads.bias logvar", "heads.wgrad", "heads.bias_grad", "heads.dgrad"}, R.bad
    g2 = dict(w.grads)
    g2["vae/encoder/dense/bias"] = np.zeros_like(g2["vae/encoder/dense/bias"])
    R = mc.layer_report(c, w.st, g2, p, d)
    assert [b[0] for b in R.bad] == ["enc0.bias_grad"], R.bad
    R = mc.layer_report(c, w.st, w.grads, p, d, mutate="no_last_mask")
    assert [b[0] for b in R.bad] == ["dec%d.dgrad" % len(c.dec)], R.bad
    # a layer that is 1 % wrong (what the end-to-end bf16 bound of test_f_mlp_vae_gpu.py lets through) fails its own op
    st2 = dict(w.st)
    st2["h0"] = mc.bf16r(w.st["h0"] * 1.01)
    assert "enc0.fwd" in {b[0] for b in mc.layer_report(c, st2, w.grads, p, d).bad}


def test_the_bf16_loss_report_takes_the_emulation_and_refuses_a_wrong_loss():
    c = mc.by_id(4)
    emul = mc.reference(c, storage="bf16", dtype="f32")
    assert not mc.bf16_loss_report(c, emul.recon, emul.kl)[1]
    assert [b[0] for b in mc.bf16_loss_report(c, emul.recon * 1.02, emul.kl)[1]] == ["reconstruction"]
    assert [b[0] for b in mc.bf16_loss_report(c, emul.recon, emul.kl * 1.2)[1]] == ["kl"]


# ---------------------------------------------------------------------------------------------------------------------------------------
# the engine's host side through the C ABI
# ---------------------------------------------------------------------------------------------------------------------------------------
def _desc(c, precision, max_batch, with_optimizer=1):
    from mi355 import lib as milib
    d = milib.MiMlpVaeDesc()
    d.dtype, d.max_batch, d.source_size, d.target_size, d.z_dim = (milib.MI_BF16 if precision == "bf16" else milib.MI_F32), max_batch, mc.S(c), mc.P(c), c.z
    d.n_enc, d.n_dec = len(c.enc), len(c.dec)
    for i, h in enumerate(c.enc):
        d.enc[i] = h
    for i, h in enumerate(c.dec):
        d.dec[i] = h
    d.loss_kind, d.with_optimizer, d.beta, d.kl_tolerance = 0, with_optimizer, 1.0, 0.0
    return d


def _aligned(nbytes):
    raw = np.zeros(nbytes + 256, np.uint8)
    return raw, raw.ctypes.data + (-raw.ctypes.data) % 256


def _host_engine(d):
    from mi355 import lib as milib
    L = milib.get()
    n, ws = L.mi_mlpvae_param_floats(ctypes.byref(d)), L.mi_mlpvae_workspace_bytes(ctypes.byref(d))
    assert n > 0 and 0 < ws < (1 << 28)
    keep = [_aligned(4 * n) for _ in range(6)] + [_aligned(ws)]
    h = L.mi_mlpvae_create(ctypes.byref(d), *[k[1] for k in keep], ws)
    assert h, L.cdll.mi_last_error()
    return L, h, keep, ws


_WHICH = {"mean": 1, "logvar": 2, "klrow": 3, "z": 5, "x": 10, "heads": 11, "slab": 12, "dheads": 60, "dz": 61, "out2": 0}


def _which(name):
    if name in _WHICH:
        return _WHICH[name]
    for prefix, base in (("gh", 40), ("gd", 50), ("h", 20), ("d", 30)):
        if name.startswith(prefix) and name[len(prefix):].isdigit():
            return base + int(name[len(prefix):])
    return None


@pytest.mark.parametrize("with_optimizer", [1, 0])
@pytest.mark.parametrize("cid", IDS)
def test_the_workspace_carve_without_guards_is_the_restated_one(cid, with_optimizer, monkeypatch):
    """With MI355_DEBUG_GUARDS unset mi_mlpvae_workspace_bytes and every offset mi_mlpvae_buffer returns are what init_engine always carved (restated in
    mlp_engine_cases.workspace_layout); with it set the size grows by 256 bytes per region and by nothing else.  The gradient queries of an inference-only engine and
    every undeclared `which` return NULL."""
    monkeypatch.delenv("MI355_DEBUG_GUARDS", raising=False)
    c = mc.by_id(cid)
    for prec in mc.precisions(c):
        mb = 16 if not with_optimizer else mc.CREATE_BATCH.get(cid, 128)
        d = _desc(c, prec, mb, with_optimizer)
        off, total = mc.workspace_layout(c, prec, mb, bool(with_optimizer))
        L, h, keep, ws = _host_engine(d)
        try:
            assert ws == total, (cid, prec, ws, total)
            base = keep[-1][1]
            for name, o in off.items():
                w = _which(name)
                if w is not None:
                    assert L.mi_mlpvae_buffer(h, w) == base + o, (cid, prec, name)
            assert L.mi_mlpvae_buffer(h, 4) == base + off["d%d" % len(c.dec)]
            n, bad, goff = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_longlong(0)
            L.mi_mlpvae_debug_check_guards(h, ctypes.addressof(n), ctypes.addressof(bad), 0, ctypes.addressof(goff))
            assert (n.value, bad.value, goff.value) == (0, 0, -1)
            for which in (-1, 6, 9, 13, 19, 20 + len(c.enc), 29, 30 + len(c.dec) + 1, 39, 40 + len(c.enc), 50 + len(c.dec) + 1, 59, 62, 70, 100):
                assert L.mi_mlpvae_buffer(h, which) is None, which
            if not with_optimizer:
                for which in [40 + i for i in range(len(c.enc))] + [50 + i for i in range(len(c.dec) + 1)] + [60, 61]:
                    assert L.mi_mlpvae_buffer(h, which) is None, which
        finally:
            L.mi_mlpvae_destroy(h)
        monkeypatch.setenv("MI355_DEBUG_GUARDS", "1")
        assert L.mi_mlpvae_workspace_bytes(ctypes.byref(d)) == total + 256 * len(off)
        monkeypatch.delenv("MI355_DEBUG_GUARDS")
        assert L.mi_mlpvae_workspace_bytes(ctypes.byref(d)) == total


def test_the_parameter_layout_has_no_padding_and_the_engine_refuses_what_it_cannot_run():
    from mi355 import lib as milib
    L = milib.get()
    for c in mc.CASES:
        for prec in mc.precisions(c):
            d = _desc(c, prec, 4)
            n = L.mi_mlpvae_tensor_count(ctypes.byref(d))
            assert n == 2 * len(mc.layers(c))
            off, size = np.zeros(n, np.int64), np.zeros(n, np.int64)
            L.mi_mlpvae_param_layout(ctypes.byref(d), off.ctypes.data, size.ctypes.data, n)
            want = [x for _, _, K, N in mc.layers(c) for x in (K * N, N)]
            assert list(size) == want and list(off) == list(np.cumsum([0] + want[:-1]))
            assert L.mi_mlpvae_param_floats(ctypes.byref(d)) == sum(want)
    assert L.mi_mlpvae_param_floats(ctypes.byref(_desc(mc.by_id(5), "bf16", 4))) == -1      # 4092, 12, 20: multiples of 4, not of 8
    d = _desc(mc.by_id(1), "fp32", 4)
    d.n_enc = 5                                                                              # five hidden layers
    assert L.mi_mlpvae_param_floats(ctypes.byref(d)) == -1
