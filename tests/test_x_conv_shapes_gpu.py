"""The conv / deconv layer-op entry points against float64 OFF the model's nine layer geometries: every case of tests/conv_shape_cases.py (kernel sizes 2 - 6, ragged
128-byte channel stages, partly filled output tiles, slot grids at and past the halo limits, position counts below / at / past a tile, the filter gradients' split /
scratch / bias plumbing, the narrow-layer kernels off 3 -> 32 and 32 -> 3, the merged first-generation path, and the shapes the launchers must refuse) through the C
ABI, with the dispatch pinned by mi_set_tuning (restored in `finally`).  The family each case reaches is asserted on the CPU (test_conv_shape_cases_host.py).

Every output, dW and dbias buffer carries eight sentinel elements behind its extent that must survive; every forward / input-gradient output starts at a fill value.
Bounds are the project's: hip_helpers.tols for forward and input gradients, 1e-5 / 2e-5 s (fp32, split) and 1e-4 / 1e-4 s (bf16) for filter gradients, 1e-4 max for
bias gradients.  Measured distances are printed (pytest -s) as `MEASURE family | what | achieved | bound`: profiles/r23_conv_shapes.md."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import conv_shape_cases as cc  # noqa: E402
from hip_helpers import DT, P, alloc, assert_close, dev, host, keep_reset, stream, tols  # noqa: E402
from mi355 import lib as milib  # noqa: E402

FILL, SENT, EXTRA = 7.0, 7.0, 8
BIG_SCRATCH = 48 << 20
MEAS = {}


def note(section, what, achieved, bound=None):
    a = float(np.max(achieved)) if np.size(achieved) else 0.0
    key = (section, what)
    if key not in MEAS or a > MEAS[key][0]:
        MEAS[key] = (a, None if bound is None else float(bound))


def note_flag(section, what, flag):
    key = (section, what)
    MEAS[key] = (bool(flag) and MEAS.get(key, (True,))[0] is True, "flag")


@pytest.fixture(scope="module", autouse=True)
def _print_measurements():
    yield
    for (section, what), (a, b) in sorted(MEAS.items()):
        if b == "flag":
            print("MEASURE %s | %s | %s | -" % (section, what, "yes" if a else "no"))
        else:
            print("MEASURE %s | %s | %.3g | %s" % (section, what, a, "-" if b is None else "%.3g" % b))


class Tuning:
    def __init__(self, settings):
        self.settings, self.prev = settings, {}

    def __enter__(self):
        L = milib.get()
        for k, v in self.settings.items():
            self.prev[k] = L.mi_set_tuning(k, v)

    def __exit__(self, *exc):
        L = milib.get()
        for k, v in self.prev.items():
            L.mi_set_tuning(k, v)
        keep_reset()


def measure(c, what, got, ref, rtol, atol):
    err = np.abs(np.asarray(got, np.float64) - ref)
    scale = float(np.abs(ref).max()) or 1.0
    note(c.family, what + " (%s): worst |err| / max|ref|" % c.dt, err.max() / scale, (atol + rtol * scale) / scale)


def frames_arg(c, d):
    """(device tensor of x, frame_idx device pointer or None, x_is_f32 flag)."""
    td = DT[c.dt][1]
    fr = c.opt.get("frames")
    idx = P(dev(d["idx"], torch.int32)) if d["idx"] is not None else None
    if fr == "u8":
        return torch.from_numpy(d["x_u8"]).cuda().contiguous(), idx, 2
    if fr == "f32":
        return dev(d["x"], torch.float32), idx, 1
    return dev(d["x"], td), idx, 0


def kcontig(w, cols):
    """[.., cols] kernel as its K-contiguous copy [cols][K]."""
    return np.ascontiguousarray(w.reshape(-1, cols).T)


def run_fwd_dgrad(c, d, wT=None, raw=False):
    """-> (result [.., float64], sentinel tail survived, return code).  raw: the unchecked binding (a refused call returns its error code instead of raising)."""
    L = milib.get().cdll if raw else milib.get()
    code, td = DT[c.dt]
    OH, OW = cc.out_hw(c)
    k, o = c.k, c.opt
    wT = o.get("wT", 1) if wT is None else wT
    bias = P(dev(d["b"])) if o.get("bias", True) else None
    relu = int(o.get("relu", True))
    if c.entry == "conv.fwd":
        shape = (c.B, OH, OW, c.N)
        n = int(np.prod(shape))
        out = alloc(td, n + EXTRA, fill=FILL)
        xd, idx, isf = frames_arg(c, d)
        wd = dev(kcontig(d["w"], c.N) if wT else d["w"], td)
        rc = L.mi_conv2d_nhwc_fwd(stream(), code, P(xd), idx, isf, c.B, c.IH, c.IW, c.C, P(wd), int(wT), bias, k, k, c.N, relu, P(out))
    elif c.entry == "deconv.fwd":
        shape = (c.B, OH, OW, c.N)
        n = int(np.prod(shape))
        out = alloc(td, n + EXTRA, fill=FILL)
        rc = L.mi_deconv2d_nhwc_fwd(stream(), code, P(dev(d["x"], td)), c.B, c.IH, c.IW, c.C, P(dev(d["w"], td)), bias, k, k, c.N, relu, P(out))
    elif c.entry == "conv.dgrad":
        shape = (c.B, c.IH, c.IW, c.C)
        n = int(np.prod(shape))
        out = alloc(td, n + EXTRA, fill=FILL)
        mask = P(dev(d["mask"], td)) if o.get("mask", True) else None
        rc = L.mi_conv2d_nhwc_dgrad(stream(), code, P(dev(d["dy"], td)), c.B, OH, OW, c.N, P(dev(d["w"], td)), k, k, c.C, c.IH, c.IW, mask, P(out))
    else:                                                  # deconv.dgrad: kernel [kh, kw, N, C], K-contiguous copy [C][k k N]
        shape = (c.B, c.IH, c.IW, c.C)
        n = int(np.prod(shape))
        out = alloc(td, n + EXTRA, fill=FILL)
        mask = P(dev(d["mask"], td)) if o.get("mask", True) else None
        wd = dev(kcontig(d["w"], c.C) if wT else d["w"], td)
        rc = L.mi_deconv2d_nhwc_dgrad(stream(), code, P(dev(d["dy"], td)), c.B, OH, OW, c.N, P(wd), int(wT), k, k, c.C, mask, P(out))
    h = host(out)
    return h[:n].reshape(shape), bool((h[n:] == SENT).all()), rc


def scratch_need(c):
    """Bytes of scratch the launch's slabs (+ bias partial sums) take, by the predicates of conv_shape_cases."""
    fam, plan = cc.family_of(c)
    if fam.startswith("tapwgrad"):
        return plan["slab_bytes"] + plan["bias_bytes"]
    if fam == "gen1":
        return plan["slab_bytes"]
    raise AssertionError(fam)


def run_wgrad(c, d, scratch=None, dbias=None, raw=False):
    """-> {dw, db, tails, touched (scratch), rc}: one call of the filter-gradient entry point into buffers that start at dw0 / db0."""
    L = milib.get().cdll if raw else milib.get()
    code, td = DT[c.dt]
    OH, OW = cc.out_hw(c)
    k, o = c.k, c.opt
    mode = o.get("scratch", "none") if scratch is None else scratch
    want_db = bool(o.get("dbias")) if dbias is None else dbias
    nw = d["w"].size
    dw = torch.full((nw + EXTRA,), SENT, device="cuda")
    dw[:nw] = torch.from_numpy(d["dw0"].reshape(-1)).cuda()
    db = torch.full((c.N + EXTRA,), SENT, device="cuda")
    db[:c.N] = torch.from_numpy(d["db0"]).cuda()
    ws, wp, wb = None, None, 0
    if mode == "big":
        ws = torch.full((BIG_SCRATCH,), 0x7f, device="cuda", dtype=torch.uint8)
        wp, wb = ws.data_ptr(), BIG_SCRATCH
    elif mode in ("exact", "short", "off8"):
        need = scratch_need(c) if want_db == bool(o.get("dbias")) else scratch_need(c._replace(opt=dict(o, dbias=want_db)))
        ws = torch.full((need + 512,), 0x7f, device="cuda", dtype=torch.uint8)
        assert ws.data_ptr() % 256 == 0
        wp, wb = ws.data_ptr() + (8 if mode == "off8" else 0), need - (256 if mode == "short" else 0)
    dyd = dev(d["dy"], td)
    dbp = db.data_ptr() if want_db else None
    if c.entry == "conv.wgrad":
        xd, idx, isf = frames_arg(c, d)
        rc = L.mi_conv2d_nhwc_wgrad_ws(stream(), code, P(xd), idx, isf, c.B, c.IH, c.IW, c.C, P(dyd), k, k, c.N, dw.data_ptr(), wp, wb, dbp)
    else:
        rc = L.mi_deconv2d_nhwc_wgrad_ws(stream(), code, P(dyd), c.B, OH, OW, c.N, P(dev(d["x"], td)), k, k, c.C, dw.data_ptr(), wp, wb, dbp)
    torch.cuda.synchronize()
    hw, hb = host(dw), host(db)
    touched = None if ws is None else bool((ws != 0x7f).any().item())
    return {"rc": rc, "dw": hw[:nw].reshape(d["w"].shape), "db": hb[:c.N], "tails": bool((hw[nw:] == SENT).all() and (hb[c.N:] == SENT).all()),
            "db_untouched": bool((hb[:c.N] == d["db0"].astype(np.float64)).all()), "touched": touched}


FWD = [c for c in cc.CASES if not c.family.startswith("refused") and not c.entry.endswith(".wgrad")]
WGRAD = [c for c in cc.CASES if not c.family.startswith("refused") and c.entry.endswith(".wgrad")]
REFUSED = [c for c in cc.CASES if c.family.startswith("refused")]


@pytest.mark.parametrize("c", FWD, ids=cc.case_id)
def test_forward_and_input_gradient(c):
    d = cc.make_inputs(c)
    ref = cc.reference(c, d)["out"]
    with Tuning(c.tune):
        got, tail_ok, _ = run_fwd_dgrad(c, d)
        got_t = run_fwd_dgrad(c, d, wT=1)[0] if c.opt.get("also_wT") else None
    rt, at = tols(c.dt, float(np.abs(ref).max()))
    measure(c, c.entry, got, ref, rt, at)
    assert_close(got, ref, rt, at, "%s [%s] %s" % (c.entry, c.family, c.why))
    assert tail_ok, "the sentinels behind the output were overwritten"
    if "larger_input" in c.tags:                           # rows / columns no window reaches: exact zeros, not small numbers and not the fill value
        un = cc.unreached(c)
        assert un.any() and (got[:, un] == 0).all()
    if c.entry.endswith(".dgrad") and c.opt.get("mask", True):
        flat = got.reshape(-1)
        assert flat[0] == 0 and flat[1] == 0               # the planted 0.0 and the planted negative value of the mask
    if got_t is not None:                                  # K-contiguous weights on the same first-generation kernel: the same sums in the same order
        assert_close(got_t, ref, rt, at, "K-contiguous weights")
        note_flag(c.family, "K-contiguous weights bitwise equal to plain weights", np.array_equal(got, got_t))
        assert np.array_equal(got, got_t)


@pytest.mark.parametrize("c", WGRAD, ids=cc.case_id)
def test_filter_gradient(c):
    d = cc.make_inputs(c)
    ref = cc.reference(c, d)
    o = c.opt
    fam, plan = cc.family_of(c)
    bf = c.dt == "bf16"
    rt, at = (1e-4, 1e-4 * ref["dw_scale"]) if bf else (1e-5, 2e-5 * ref["dw_scale"])
    with Tuning(c.tune):
        if o.get("slab_bf16"):                             # bf16 slabs against the fp32 slabs of the same kernel: the bound of test_bf16_partial_sum_slabs_error_bound_at_batch_512
            L = milib.get()
            r1 = run_wgrad(c, d)
            prev = L.mi_set_tuning(18, 0)
            try:
                r0 = run_wgrad(c._replace(tune={**c.tune, 18: 0}), d)
            finally:
                L.mi_set_tuning(18, prev)
            e = (r1["dw"] - r0["dw"])
            g0 = r0["dw"] - d["dw0"]
            rms, scale = float(np.sqrt(np.mean(e ** 2))), float(np.sqrt(np.mean(g0 ** 2)))
            note(c.family, "bf16 slabs vs fp32 slabs: rms err / rms", rms / scale, 2e-3)
            note(c.family, "bf16 slabs vs fp32 slabs: max err / max", np.abs(e).max() / np.abs(g0).max(), 1e-2)
            assert r1["touched"] and r1["tails"] and not np.array_equal(r0["dw"], r1["dw"])
            assert rms <= 2e-3 * scale and np.abs(e).max() <= 1e-2 * np.abs(g0).max()
            return
        r = run_wgrad(c, d)
        extra = {}
        if o.get("twice"):
            extra["twice"] = run_wgrad(c, d)
        if o.get("decodes"):
            L = milib.get()
            for mode in (0, 3):
                prev = L.mi_set_tuning(24, mode)
                try:
                    extra["dec%d" % mode] = run_wgrad(c, d)
                finally:
                    L.mi_set_tuning(24, prev)
        if o.get("same_as_dbias"):
            extra["with_db"] = run_wgrad(c, d, dbias=True)
        if o.get("scratch") in ("short", "off8", "none") and fam != "narrow_wgrad" and plan.get("splits", 1) > 1:
            extra["again"] = run_wgrad(c, d)
    measure(c, "dw", r["dw"] - d["dw0"], ref["dw"] - d["dw0"], rt, at)
    assert_close(r["dw"], ref["dw"], rt, at, "%s dw [%s] %s" % (c.entry, c.family, c.why))
    assert r["tails"], "the sentinels behind dw / dbias were overwritten"
    if o.get("dbias"):
        measure(c, "dbias", r["db"] - d["db0"], ref["db"] - d["db0"], 0.0, 1e-4 * ref["db_scale"])
        assert_close(r["db"], ref["db"], 0.0, 1e-4 * ref["db_scale"], "%s dbias [%s]" % (c.entry, c.family))
    else:
        assert r["db_untouched"]
    # where the slabs land: the scratch the predicates size is the scratch the launcher takes
    if fam.startswith("tapwgrad") and not plan.get("x3"):
        uses = o.get("scratch") in ("exact", "big") and plan["slabs_possible"]
        assert r["touched"] is (uses if o.get("scratch", "none") != "none" else None), (r["touched"], uses)
    if fam == "gen1" and "wgrad" in c.tags and o.get("scratch", "none") != "none" and not o.get("dbias"):
        assert r["touched"] is (o["scratch"] in ("exact", "big") and plan["splits"] > 1)
    if "twice" in extra:                                   # slabs + one ordered sum: two runs are bitwise equal
        assert np.array_equal(extra["twice"]["dw"], r["dw"]) and np.array_equal(extra["twice"]["db"], r["db"])
    if "dec0" in extra:                                    # the two DMA-row decodes (key 24): same addresses, same order
        assert np.array_equal(extra["dec0"]["dw"], extra["dec3"]["dw"]) and np.array_equal(extra["dec0"]["db"], extra["dec3"]["db"])
        assert np.array_equal(extra["dec0"]["dw"], r["dw"])
    if "with_db" in extra:                                 # asking for the bias gradient does not change dW
        assert np.array_equal(extra["with_db"]["dw"], r["dw"])
        assert_close(extra["with_db"]["db"], ref["db"], 0.0, 1e-4 * ref["db_scale"], "dbias")
    if "again" in extra:                                   # splits that meet in atomics: recorded, not asserted
        note_flag(c.family, "two runs through atomics bitwise equal (%s)" % cc.case_id(c), np.array_equal(extra["again"]["dw"], r["dw"]))
        assert_close(extra["again"]["dw"], ref["dw"], rt, at, "second run")


@pytest.mark.parametrize("c", REFUSED, ids=cc.case_id)
def test_refused_shapes_raise_and_write_nothing(c):
    d = cc.make_inputs(c)
    with Tuning(c.tune):
        if c.entry.endswith(".wgrad"):
            with pytest.raises(milib.MiError):
                run_wgrad(c, d)
            r = run_wgrad(c, d, raw=True)
            assert r["rc"] != 0 and r["tails"] and r["db_untouched"]
            assert np.array_equal(r["dw"], d["dw0"].astype(np.float64)), "a refused call wrote into dw"
            return
        with pytest.raises(milib.MiError):
            run_fwd_dgrad(c, d)
        got, tail_ok, rc = run_fwd_dgrad(c, d, raw=True)
        assert rc != 0 and tail_ok
        assert (got == FILL).all(), "a refused call wrote into its output"


# ---------------------------------------------------------------------------------------------------------------------------------------
# the fused-loss form of gather_narrow_kernel (mi_deconv2d_nhwc_fwd_bce) off 39 x 79: references and bounds as test_deconv_fwd_with_fused_reconstruction_loss states them
# ---------------------------------------------------------------------------------------------------------------------------------------
FUSED = [(dt, N, kind, dl) for dt in ("f32", "bf16", "x3") for N in (1, 3) for kind in (0, 2) for dl in (True, False)]


def run_fused_loss(dt, N, kind, with_dl, k=4, B=2, IH=3, IW=5, C=32):
    """-> None (asserts).  Even OW: logits, loss, dlogits and the per-channel dlogits sums against float64; odd OW (k = 5): n_partial = 0 and nothing written."""
    import ctypes
    import torch.nn.functional as F
    from hip_helpers import rounded
    L = milib.get()
    code, td = DT[dt]
    OH, OW = (IH - 1) * 2 + k, (IW - 1) * 2 + k
    rng = np.random.RandomState(7 + 10 * N + kind)
    x = rng.randn(B, IH, IW, C).astype(np.float32)
    w = (rng.randn(k, k, N, C) / np.sqrt(4 * C)).astype(np.float32)
    b = (0.1 * rng.randn(N)).astype(np.float32)
    frames = rng.rand(3, OH * OW * N).astype(np.float32)
    idx = np.array([2, 2], np.int32)                        # a repeated index
    inv_b = 1.0 / 8.0
    n = B * OH * OW * N
    cap = 8
    lp, bp = torch.full((cap + 1,), -3.0, device="cuda"), torch.full((cap + 1, 4), -3.0, device="cuda")
    logits, dl = alloc(td, n + EXTRA, fill=FILL), alloc(td, n + EXTRA, fill=FILL)
    npart = ctypes.c_int(-1)
    with Tuning(cc.NEW):
        L.mi_deconv2d_nhwc_fwd_bce(stream(), code, P(dev(x, td)), B, IH, IW, C, P(dev(w, td)), P(dev(b)), k, k, N, P(logits), P(dev(frames)), P(dev(idx, torch.int32)),
                                   OH * OW * N, kind, inv_b, P(dl) if with_dl else None, lp.data_ptr(), bp.data_ptr(), cap, ctypes.addressof(npart))
        torch.cuda.synchronize()
    hl, hd = host(logits), host(dl)
    if OW % 2:                                              # the fused form needs whole pixel pairs: refused without an error, nothing launched
        assert npart.value == 0
        assert (hl == FILL).all() and (hd == FILL).all() and bool((lp == -3.0).all()) and bool((bp == -3.0).all())
        return
    MP = B * ((OH + 1) // 2 + 1) * ((OW + 1) // 2 + 1)
    assert npart.value == -(-MP // cc.GN_BMT)
    xr, wr = rounded(x, td), rounded(w, td)
    y = F.conv_transpose2d(xr.permute(0, 3, 1, 2), wr.permute(3, 2, 0, 1), torch.from_numpy(b).double(), stride=2).permute(0, 2, 3, 1).contiguous()
    lref = rounded(y.float().numpy(), td).requires_grad_(True)                            # the loss reads the STORED logits
    t = torch.from_numpy(frames[idx]).double().reshape(B, OH, OW, N)
    if kind == 0:
        per = torch.clamp(lref, min=0) - lref * t + torch.log1p(torch.exp(-lref.abs()))
    else:
        per = (t - torch.sigmoid(lref)) ** 2
    (per.sum() * inv_b).backward()
    rt, at = tols(dt, float(lref.abs().max()))
    assert_close(hl[:n].reshape(y.shape), y.detach().numpy(), rt, at, "logits")
    assert (hl[n:] == SENT).all() and (hd[n:] == SENT).all()
    nb = npart.value
    loss_rel = abs(float(lp[:nb].double().sum()) / float(per.sum()) - 1)
    note("gather_narrow", "fused loss (%s): relative error of the sum" % dt, loss_rel, 1e-5 if dt != "bf16" else 3e-3)
    assert loss_rel < (1e-5 if dt != "bf16" else 3e-3)
    assert bool((lp[nb:] == -3.0).all()) and bool((bp[nb:] == -3.0).all())
    if with_dl:
        rt, at = tols(dt, float(lref.grad.abs().max()))
        assert_close(hd[:n].reshape(y.shape), lref.grad.numpy(), rt, at, "dlogits")
    else:
        assert (hd == FILL).all()
    bias_ref = lref.grad.sum((0, 1, 2)).numpy()
    got = bp[:nb, :N].double().sum(0).cpu().numpy()
    # the kernel sums the STORED dlogits (rounded to the storage type): the reference is the float64 sum of the dlogits a call with `dlogits` returns (held to float64
    # above), so the sum's cancellation and the elements' rounding are in the reference and the bound is the fp32 summation's: 1e-5 x sum |dlogits| per channel
    if with_dl:
        stored = hd[:n].reshape(y.shape)
    else:
        dl2, lp2, bp2, np2 = alloc(td, n + EXTRA, fill=FILL), torch.zeros(cap + 1, device="cuda"), torch.zeros(cap + 1, 4, device="cuda"), ctypes.c_int(-1)
        with Tuning(cc.NEW):
            L.mi_deconv2d_nhwc_fwd_bce(stream(), code, P(dev(x, td)), B, IH, IW, C, P(dev(w, td)), P(dev(b)), k, k, N, P(logits), P(dev(frames)), P(dev(idx, torch.int32)),
                                       OH * OW * N, kind, inv_b, P(dl2), lp2.data_ptr(), bp2.data_ptr(), cap, ctypes.addressof(np2))
            torch.cuda.synchronize()
        stored = host(dl2)[:n].reshape(y.shape)
        rt, at = tols(dt, float(lref.grad.abs().max()))
        assert_close(stored, lref.grad.numpy(), rt, at, "dlogits of the twin call")
    bias_ref = stored.sum((0, 1, 2))
    gabs = np.abs(stored).sum((0, 1, 2))
    got = bp[:nb, :N].double().sum(0).cpu().numpy()
    note("gather_narrow", "fused bias gradient (%s): |err| / sum|dlogits|" % dt, (np.abs(got - bias_ref) / gabs).max(), 1e-5)
    assert (np.abs(got - bias_ref) <= 1e-5 * gabs).all(), ("fused bias gradient", got, bias_ref, gabs)


@pytest.mark.parametrize("dt,N,kind,with_dl", FUSED)
def test_fused_loss_form_off_the_model_shape(dt, N, kind, with_dl):
    run_fused_loss(dt, N, kind, with_dl)                    # OW = 12


@pytest.mark.parametrize("dt", ["f32", "bf16", "x3"])
@pytest.mark.parametrize("N", [1, 3])
def test_fused_loss_form_refuses_an_odd_output_width(dt, N):
    run_fused_loss(dt, N, 0, True, k=5)                     # OW = 13: n_partial = 0, nothing launched


LEAN_IDS = [c.id for c in cc.CASES if c.family == "narrow_conv" and c.opt.get("lean")]


def first_generation_narrow_forms():
    """The narrow-layer cases whose bf16 form is the instruction-lean one, and the fused loss whose bf16 kind-0 form is the hardware-transcendental one: run by
    narrow_lean_worker.py in a process started with MI355_NARROW_LEAN=0 (environment only), where the first-generation forms take them."""
    done = []
    for c in cc.CASES:
        if c.id in LEAN_IDS:
            d = cc.make_inputs(c)
            ref = cc.reference(c, d)["out"]
            with Tuning(c.tune):
                got, tail_ok, _ = run_fwd_dgrad(c, d)
            rt, at = tols(c.dt, float(np.abs(ref).max()))
            assert_close(got, ref, rt, at, "first-generation form: " + c.why)
            assert tail_ok
            done.append(cc.case_id(c))
    for with_dl in (True, False):
        run_fused_loss("bf16", 3, 0, with_dl)
        done.append("fused loss bf16 N = 3 kind 0 dlogits %s" % with_dl)
    return done


def test_first_generation_narrow_forms_in_a_child_process():
    """MI355_NARROW_LEAN is read when the library is loaded: one fresh child process (tests/narrow_lean_worker.py) runs the lean cases with the knob off."""
    import json
    import os
    import subprocess
    import sys
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "narrow_lean_worker.py")
    r = subprocess.run([sys.executable, worker], env=dict(os.environ, MI355_NARROW_LEAN="0"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    done = json.loads(r.stdout.strip().splitlines()[-1])
    assert len(done) == len(LEAN_IDS) + 2 and len(LEAN_IDS) == 6
