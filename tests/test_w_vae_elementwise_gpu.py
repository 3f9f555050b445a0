"""The VAE elementwise kernels (csrc/elementwise.hip) against float64 off the one shape each is tested at in test_ops_gpu.py: the scalar and the vector path of the
reconstruction loss, ragged groups, a second chunk, misaligned rows, the fused bias gradient; the reparameterisation's slab groups and lane trips, its Philox draw and
its wide variant; the one-block loss finalisation's unrolled loop and bias path; Adam's second grid-stride trip, tail and planted gradients; the split-K finish, the
byte -> [0, 1] pass, sigmoid, range check, casts and the scalar column sums.  Cases, references and bounds: tests/vae_elementwise_cases.py (asserted on the CPU by
test_vae_elementwise_cases_host.py).  Every output buffer carries at least one element more than the operation's extent, holding a sentinel that must survive.
Measured distances are printed (pytest -s) as `MEASURE section | what | achieved | bound`: profiles/r22_vae_elementwise.md."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import vae_elementwise_cases as vc  # noqa: E402
from hip_helpers import DT, DTS, P, X3, alloc, assert_close, dev, host, split_decode, split_encode, stream, tols  # noqa: E402
from mi355 import lib as milib  # noqa: E402

F32 = np.float32
SENT = 7.0
ITEM = {"f32": 4, "bf16": 2, "x3": 4}
MEAS = {}


def note(section, what, achieved, bound=None):
    """Keeps, per (section, what), the largest achieved distance (and the bound it was held to at that point)."""
    a = float(np.max(achieved)) if np.size(achieved) else 0.0
    key = (section, what)
    if key not in MEAS or a > MEAS[key][0]:
        MEAS[key] = (a, None if bound is None else float(np.max(bound)))


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


def raw(t):
    return t.view(torch.int32) if t.dtype == X3 else t


def bits(t):
    """The raw words of a device tensor."""
    torch.cuda.synchronize()
    if t.dtype in (X3, torch.float32):
        return t.view(torch.int32).reshape(-1).cpu().numpy().view(np.uint32)
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).reshape(-1).cpu().numpy().view(np.uint16)
    return t.reshape(-1).cpu().numpy()


def store_bits(a32, dt):
    """The raw words the storage type holds for a float32 array."""
    a32 = np.array(a32, F32).reshape(-1)
    if dt == "f32":
        return a32.view(np.uint32)
    if dt == "x3":
        return split_encode(a32).view(np.uint32)
    return torch.from_numpy(a32.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def out_buf(dt, n, extra=8):
    """An output buffer of n elements of the storage type + `extra` sentinels."""
    return alloc(DT[dt][1], n + extra, fill=SENT)


def fbuf(n, extra=1, fill=SENT):
    return torch.full((n + extra,), float(fill), device="cuda")


def tail_untouched(t, n, dt=None, fill=SENT):
    b = bits(t)
    want = store_bits(np.full(b.size - n, fill, F32), dt or "f32")
    return b.size > n and np.array_equal(b[n:], want)


def placed(a, dt, off, extra=8):
    """A device buffer holding the float32 array `a` in the storage type from element `off` on; -> (tensor, pointer of element off)."""
    td = DT[dt][1]
    a = np.ascontiguousarray(a, F32).reshape(-1)
    buf = alloc(td, a.size + off + extra, fill=0.0)
    raw(buf)[off:off + a.size] = raw(dev(a.copy(), td))
    return buf, P(buf) + off * ITEM[dt]


def iptr(a):
    return None if a is None else P(dev(np.ascontiguousarray(a), torch.int32))


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. reconstruction loss
# ---------------------------------------------------------------------------------------------------------------------------------------
def run_recon(dt, B, Pn, kind, logits, labels, stride, idx, u8=False, want_dl=True, x_off=0, channels=None, dbias=None):
    L = milib.get()
    code = DT[dt][0]
    _, xp = placed(logits, dt, x_off)
    nch = vc.recon_chunks(Pn)
    assert L.mi_recon_loss_chunks(Pn) == nch
    partial = fbuf(B * nch)
    dl = out_buf(dt, B * Pn) if want_dl else None
    lab = torch.from_numpy(np.ascontiguousarray(labels).copy()).cuda()
    args = (stream(), code, xp, P(lab), iptr(idx), stride, B, Pn, kind, vc.INV_B, None if dl is None else dl.data_ptr(), partial.data_ptr())
    if u8:
        L.mi_bce_logits_fwd_bwd_u8(*args)
    elif channels is not None:
        L.mi_bce_logits_fwd_bwd_bias(*args, channels, None if dbias is None else dbias.data_ptr())
    else:
        L.mi_bce_logits_fwd_bwd(*args)
    torch.cuda.synchronize()
    return {"dl": dl, "partial": partial}


def check_recon(res, r, dt, B, Pn, kind, tag):
    nch = vc.recon_chunks(Pn)
    got = host(res["partial"])[:B * nch].reshape(B, nch)
    assert np.isfinite(got).all() and tail_untouched(res["partial"], B * nch), tag
    err = np.abs(got - r["chunks"])
    if kind == 1:
        bound = vc.RECON_K1_FACTOR * r["d32_chunks"] + tols("f32", float(np.abs(r["chunks"]).max()))[1]
    else:
        bound = vc.RECON_LOSS_REL * r["abs_chunks"] + vc.RECON_LOSS_ABS
    note("1 recon", "chunk partial / bound, kind %d" % kind, err / bound, 1.0)
    note("1 recon", "chunk partial rel. to sum|loss|, kind %d" % kind, err / np.maximum(r["abs_chunks"], 1e-30))
    assert (err <= bound).all(), (tag, "partials", err.max(), bound.min())
    if res["dl"] is None:
        return
    g = host(res["dl"])[:B * Pn].reshape(B, Pn)
    assert np.isfinite(g).all() and tail_untouched(res["dl"], B * Pn, dt), tag
    rt, at = tols(dt, float(np.abs(r["g"]).max()))
    if kind == 1:
        gerr, gb = np.abs(g - r["g"]), vc.RECON_K1_FACTOR * r["d32_g"] + at
        note("1 recon", "dlogits %s abs, kind 1 (bound 4 d32 + atol)" % dt, gerr, gb)
        assert (gerr <= gb).all(), (tag, "dlogits", gerr.max(), gb)
    else:
        note("1 recon", "dlogits %s abs, kind %d (bound rtol |ref| + atol)" % (dt, kind), np.abs(g - r["g"]), at)
        assert_close(g, r["g"], rt, at, tag + " dlogits")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kind,R", vc.RECON_KIND_R)
@pytest.mark.parametrize("BP", vc.RECON_SHAPES)
def test_recon_loss_shapes_and_arguments(BP, kind, R, dt):
    B, Pn = BP
    d = vc.recon_data(B, Pn, kind, R)
    y32 = vc.unit_labels(d["bytes"])
    a = run_recon(dt, B, Pn, kind, d["logits"], y32, Pn, None)                                   # frame_idx NULL
    check_recon(a, vc.recon_reference(B, Pn, kind, R, dt, "none"), dt, B, Pn, kind, "idx NULL")
    idx = vc.recon_frame_idx(B, "rep")
    r = vc.recon_reference(B, Pn, kind, R, dt, "rep")
    b = run_recon(dt, B, Pn, kind, d["logits"], y32, Pn, idx)                                    # a repeated index
    check_recon(b, r, dt, B, Pn, kind, "idx repeated")
    c = run_recon(dt, B, Pn, kind, d["logits"], d["bytes"], Pn, idx, u8=True)                    # byte labels: k / 255 formed exactly in registers -> the same bits
    check_recon(c, r, dt, B, Pn, kind, "byte labels")
    assert np.array_equal(bits(c["dl"]), bits(b["dl"])) and np.array_equal(bits(c["partial"]), bits(b["partial"]))
    for u8 in (False, True):                                                                     # dlogits NULL: the same partials, nothing else written
        e = run_recon(dt, B, Pn, kind, d["logits"], d["bytes"] if u8 else y32, Pn, idx, u8=u8, want_dl=False)
        check_recon(e, r, dt, B, Pn, kind, "dlogits NULL")
        assert np.array_equal(bits(e["partial"]), bits(b["partial"]))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kind,R", vc.RECON_KIND_R)
@pytest.mark.parametrize("BP", vc.RECON_ALIGN_SHAPES)
def test_recon_loss_vector_and_scalar_path_give_the_same_bits(BP, kind, R, dt):
    """The same values once in aligned rows (P = 6168: the 16-byte vector path) and once behind a label table whose odd rows are misaligned (stride P + 1 floats, P + 3
    bytes) or a logits pointer one element off a 16-byte boundary (the scalar path): dlogits bit for bit, the partials inside their bound."""
    B, Pn = BP
    d = vc.recon_data(B, Pn, kind, R)
    y32 = vc.unit_labels(d["bytes"])
    idx = vc.recon_frame_idx(B, "align")
    r = vc.recon_reference(B, Pn, kind, R, dt, "align")
    a = run_recon(dt, B, Pn, kind, d["logits"], y32, Pn, idx)
    check_recon(a, r, dt, B, Pn, kind, "aligned")
    runs = {"float table, stride P + 1": run_recon(dt, B, Pn, kind, d["logits"], vc.padded_table(y32, Pn + 1, F32(0.5)), Pn + 1, idx),
            "byte table, stride P + 3": run_recon(dt, B, Pn, kind, d["logits"], vc.padded_table(d["bytes"], Pn + 3, 77), Pn + 3, idx, u8=True),
            "byte table, aligned": run_recon(dt, B, Pn, kind, d["logits"], d["bytes"], Pn, idx, u8=True),
            "logits one element off": run_recon(dt, B, Pn, kind, d["logits"], y32, Pn, idx, x_off=1)}
    same_partials = True
    for tag, res in runs.items():
        check_recon(res, r, dt, B, Pn, kind, tag)
        assert np.array_equal(bits(res["dl"]), bits(a["dl"])), tag
        same_partials &= np.array_equal(bits(res["partial"]), bits(a["partial"]))
    note_flag("1 recon", "partials of the scalar path bitwise those of the vector path (asserted: bound only)", same_partials)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("channels", vc.RECON_CHANNELS)
@pytest.mark.parametrize("BP", vc.RECON_BIAS_SHAPES)
def test_recon_loss_fused_bias_gradient(BP, channels, dt):
    """mi_bce_logits_fwd_bwd_bias (the ConvVAE engine's path when the fused decoder tail is not eligible): dbias[c] += sum of the STORED dlogits of channel c = element % channels.
    The chunks meet in fp32 atomics: two runs are compared and the outcome recorded, not asserted."""
    B, Pn = BP
    kind, R = 0, 6.0
    d = vc.recon_data(B, Pn, kind, R)
    y32 = vc.unit_labels(d["bytes"])
    idx = vc.recon_frame_idx(B, "rep")
    r = vc.recon_reference(B, Pn, kind, R, dt, "rep")
    plain = run_recon(dt, B, Pn, kind, d["logits"], y32, Pn, idx)
    got = []
    for _ in range(2):
        db = fbuf(channels, fill=vc.DBIAS_START)
        res = run_recon(dt, B, Pn, kind, d["logits"], y32, Pn, idx, channels=channels, dbias=db)
        check_recon(res, r, dt, B, Pn, kind, "fused bias")
        assert np.array_equal(bits(res["dl"]), bits(plain["dl"])) and np.array_equal(bits(res["partial"]), bits(plain["partial"]))
        stored = host(res["dl"])[:B * Pn].reshape(B, Pn)
        ref = np.array([stored[:, c::channels].sum() for c in range(channels)]) + vc.DBIAS_START
        bound = vc.DBIAS_REL * np.array([np.abs(stored[:, c::channels]).sum() for c in range(channels)])
        g = host(db)
        assert g[channels] == vc.DBIAS_START                                                    # nothing past the channels
        err = np.abs(g[:channels] - ref)
        note("1 recon", "fused dbias / bound", err / bound, 1.0)
        assert (err <= bound).all(), (err, bound)
        got.append(bits(db))
    note_flag("1 recon", "fused dbias (fp32 atomics) equal in two runs (not asserted)", np.array_equal(got[0], got[1]))
    # channels == 1 with no dbias is the plain entry point; a channel count outside 1 .. 3 or a bias without dlogits is refused
    L = milib.get()
    code = DT[dt][0]
    _, xp = placed(d["logits"], dt, 0)
    lab, part, db, dl = dev(y32), fbuf(B * vc.recon_chunks(Pn)), fbuf(4, fill=vc.DBIAS_START), out_buf(dt, B * Pn)
    for ch, dlp in ((0, dl.data_ptr()), (4, dl.data_ptr()), (channels, None)):
        with pytest.raises(milib.MiError):
            L.mi_bce_logits_fwd_bwd_bias(stream(), code, xp, P(lab), None, Pn, B, Pn, kind, vc.INV_B, dlp, part.data_ptr(), ch, db.data_ptr())
    assert tail_untouched(db, 0, fill=vc.DBIAS_START) and tail_untouched(dl, 0, dt) and tail_untouched(part, 0)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. reparameterisation + KL
# ---------------------------------------------------------------------------------------------------------------------------------------
def reparam_fwd(dt, d, B, Z, ns, sample=1, eps=True, rng=None, eps_out=None):
    L = milib.get()
    o = {"mean": fbuf(B * Z, Z), "logvar": fbuf(B * Z, Z), "kl": fbuf(B), "z": out_buf(dt, B * Z, Z), "eps": dev(np.array(d["eps"]))}
    L.mi_vae_reparam_kl_fwd_rng(stream(), DT[dt][0], P(dev(np.array(d["heads"]))), ns, P(dev(np.array(d["bm"]))), P(dev(np.array(d["bl"]))), o["eps"].data_ptr() if eps else None, sample, B, Z,
                                o["mean"].data_ptr(), o["logvar"].data_ptr(), o["z"].data_ptr(), o["kl"].data_ptr(), None if rng is None else rng.data_ptr(),
                                None if eps_out is None else eps_out.data_ptr())
    torch.cuda.synchronize()
    return o


def reparam_bwd(dt, d, o, B, Z, nd, floor, dzs=None, kl=None):
    L = milib.get()
    dh = out_buf(dt, B * 2 * Z, 2 * Z)
    L.mi_vae_reparam_kl_bwd(stream(), DT[dt][0], P(dev(np.array(d["dzs"] if dzs is None else dzs))), nd, o["mean"].data_ptr(), o["logvar"].data_ptr(), o["eps"].data_ptr(),
                            (o["kl"] if kl is None else kl).data_ptr(), vc.REPARAM_BETA, floor, vc.INV_B, B, Z, dh.data_ptr())
    torch.cuda.synchronize()
    return dh


REPARAM_CASES = [s + (False,) for s in vc.REPARAM_SHAPES] + [vc.REPARAM_NEAR_PRIOR + (True,)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", REPARAM_CASES)
def test_reparam_kl_slab_groups_and_lane_trips(case, dt):
    B, Z, ns, nd, near = case
    d = vc.reparam_data(B, Z, ns, nd, near)
    r = vc.reparam_ref64(d, 0.0)
    o = reparam_fwd(dt, d, B, Z, ns)
    n = B * Z
    # mean / logvar: the float32 sum bias, slab 0, slab 1, ... -- the kernel's contract, bit for bit
    assert np.array_equal(bits(o["mean"])[:n], store_bits(d["mean32"], "f32")) and np.array_equal(bits(o["logvar"])[:n], store_bits(d["logvar32"], "f32"))
    for k, cnt, t in (("mean", n, None), ("logvar", n, None), ("kl", B, None), ("z", n, dt)):
        assert tail_untouched(o[k], cnt, t), k
    kl = host(o["kl"])[:B]
    kerr, kb = np.abs(kl - r["kl"]), vc.kl_bound(r["mean"], r["logvar"], r["kl"])
    note("2 reparam", "kl_row / bound%s" % (" (near prior)" if near else ""), kerr / kb, 1.0)
    note("2 reparam", "kl_row rel.%s" % (" (near prior)" if near else ""), kerr / np.abs(r["kl"]), None)
    assert (kerr <= kb).all() and np.isfinite(kl).all(), (kerr, kb)
    rt, at = tols(dt, float(np.abs(r["z"]).max()))
    z = host(o["z"])[:n].reshape(B, Z)
    note("2 reparam", "z %s abs / max|ref|" % dt, np.abs(z - r["z"]).max() / np.abs(r["z"]).max(), at / np.abs(r["z"]).max())
    assert_close(z, r["z"], rt, at, "z")
    # sample = 0: z is the mean rounded to the storage type, no eps needed
    o0 = reparam_fwd(dt, d, B, Z, ns, sample=0, eps=False)
    assert np.array_equal(bits(o0["z"])[:n], store_bits(d["mean32"], dt)) and tail_untouched(o0["z"], n, dt)
    assert np.array_equal(bits(o0["kl"]), bits(o["kl"])) and np.array_equal(bits(o0["mean"]), bits(o["mean"]))
    # backward: no floor; the floor between the planted rows; a zero upstream gradient (only the KL term is left)
    floors = [0.0] + ([d["floor"]] if d["floor"] is not None else [])
    for floor in floors:
        rf = vc.reparam_ref64(d, floor)
        dh = reparam_bwd(dt, d, o, B, Z, nd, floor)
        assert tail_untouched(dh, n * 2, dt)
        rt, at = tols(dt, float(np.abs(rf["dheads"]).max()))
        g = host(dh)[:2 * n].reshape(B, 2 * Z)
        note("2 reparam", "dheads %s abs / max|ref|" % dt, np.abs(g - rf["dheads"]).max() / np.abs(rf["dheads"]).max(), at / np.abs(rf["dheads"]).max())
        assert_close(g, rf["dheads"], rt, at, "dheads, floor %g" % floor)
    if d["floor"] is not None:
        below = r["kl"] < d["floor"]
        assert below[1] and not below[0] and np.array_equal(kl < d["floor"], below)
        g = host(reparam_bwd(dt, d, o, B, Z, nd, d["floor"], dzs=np.zeros_like(d["dzs"])))[:2 * n].reshape(B, 2 * Z)
        assert (g[below] == 0.0).all() and (np.abs(g[~below]).sum(1) > 0).all()
    # kl_floor == 0 clamps nothing, whatever the sign of the row's KL (a row the fp32 sum left a hair below zero keeps its gradient)
    neg = fbuf(B)
    neg[:B] = -o["kl"][:B].abs() - 1.0
    assert np.array_equal(bits(reparam_bwd(dt, d, o, B, Z, nd, 0.0, kl=neg)), bits(reparam_bwd(dt, d, o, B, Z, nd, 0.0)))
    # the combined entry point: both halves in one call == the two calls
    L = milib.get()
    m2, l2, k2, z2, dh2 = fbuf(n, Z), fbuf(n, Z), fbuf(B), out_buf(dt, n, Z), out_buf(dt, 2 * n, 2 * Z)
    floor = floors[-1]
    L.mi_vae_reparam_kl_fwd_bwd(stream(), DT[dt][0], P(dev(np.array(d["heads"]))), ns, P(dev(np.array(d["bm"]))), P(dev(np.array(d["bl"]))), o["eps"].data_ptr(), 1, B, Z, m2.data_ptr(), l2.data_ptr(),
                                z2.data_ptr(), k2.data_ptr(), P(dev(np.array(d["dzs"]))), nd, vc.REPARAM_BETA, floor, vc.INV_B, dh2.data_ptr())
    for a, b_, what in ((m2, o["mean"], "mean"), (l2, o["logvar"], "logvar"), (k2, o["kl"], "kl"), (z2, o["z"], "z"), (dh2, reparam_bwd(dt, d, o, B, Z, nd, floor), "dheads")):
        assert np.array_equal(bits(a), bits(b_)), what


def test_reparam_philox_draw_inside_the_kernel():
    """eps == NULL: the kernel draws the noise (three blocks, ragged lanes), stores it, and the last block advances the offset."""
    import philox_ref as pr
    L = milib.get()
    B, Z, ns, nd = 9, 65, 16, 17
    n = B * Z
    d = vc.reparam_data(B, Z, ns, nd)
    seed = 0x5EED1234ABC
    rng = torch.tensor([seed, 1000, 0, 0xDEAD], dtype=torch.int64, device="cuda")
    eps_out = fbuf(n, Z)
    o = reparam_fwd("f32", d, B, Z, ns, eps=False, rng=rng, eps_out=eps_out)
    assert rng.cpu().tolist() == [seed, 1000 + n, 0, 0xDEAD]
    assert tail_untouched(eps_out, n)
    e = host(eps_out)[:n]
    ref = np.asarray(pr.normal(seed, 1000, n), np.float64)
    note("2 reparam", "in-kernel eps vs philox_ref abs", np.abs(e - ref), 2e-5)
    assert np.abs(e - ref).max() <= 2e-5
    alone = fbuf(n)
    L.mi_normal_philox(stream(), seed, 1000, alone.data_ptr(), n)
    a = host(alone)[:n]
    assert (np.abs(e - a) <= np.spacing(np.abs(a).astype(F32)).astype(np.float64)).all() and tail_untouched(alone, n)
    note_flag("2 reparam", "in-kernel eps bitwise mi_normal_philox (asserted: 1 ulp)", np.array_equal(e, a))
    assert np.array_equal(bits(o["mean"])[:n], store_bits(d["mean32"], "f32"))
    zref = d["mean32"].astype(np.float64) + np.exp(0.5 * d["logvar32"].astype(np.float64)) * e.reshape(B, Z)
    rt, at = tols("f32", float(np.abs(zref).max()))
    assert_close(host(o["z"])[:n].reshape(B, Z), zref, rt, at, "z on the drawn noise")
    eps2 = fbuf(n, Z)
    reparam_fwd("f32", d, B, Z, ns, eps=False, rng=rng, eps_out=eps2)                             # the next call continues the stream
    assert rng.cpu().tolist() == [seed, 1000 + 2 * n, 0, 0xDEAD]
    L.mi_normal_philox(stream(), seed, 1000 + n, alone.data_ptr(), n)
    assert (np.abs(host(eps2)[:n] - host(alone)[:n]) <= np.spacing(np.abs(host(alone)[:n]).astype(F32)).astype(np.float64)).all()
    assert not np.array_equal(host(eps2)[:n], e)
    with pytest.raises(milib.MiError):                                                           # sampling without eps and without a state
        reparam_fwd("f32", d, B, Z, ns, eps=False)
    with pytest.raises(milib.MiError):
        reparam_fwd("f32", d, B, Z, ns, eps=False, rng=rng)


def test_reparam_wide_variant_gives_the_same_bits():
    """MI355_REPARAM_WIDE=1 (up to 32 slabs requested before the first add) claims "same order, same sums": a fresh process with the knob on and this one, with it off,
    give equal digests of every output, 33 slabs (two groups of the wide variant) included."""
    import reparam_wide_worker as w
    assert os.environ.get("MI355_REPARAM_WIDE") != "1", "this process is the run with the knob off"
    here = w.digests()
    r = subprocess.run([sys.executable, os.path.abspath(w.__file__)], env=dict(os.environ, MI355_REPARAM_WIDE="1"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    there = json.loads(r.stdout.strip().splitlines()[-1])
    assert sorted(there) == sorted(here) and len(here) == 5 * len(vc.REPARAM_WIDE_SHAPES)
    assert there == here, [k for k in here if here[k] != there[k]]


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. loss finalisation
# ---------------------------------------------------------------------------------------------------------------------------------------
def run_finalize(d, n_partial, B, kl_floor, inv_b, metrics, channels=0, flat=True, nchunks=None):
    L = milib.get()
    out2 = fbuf(2)
    met = None if not metrics else torch.zeros(4, device="cuda")
    if met is not None:
        met[3] = SENT
    db = fbuf(0, 4, fill=vc.DBIAS_START)
    bp = d["bpart"]
    for _ in range(2 if metrics else 1):
        if flat:
            L.mi_vae_finalize_losses_flat(stream(), P(dev(np.array(d["partial"]))), n_partial, P(dev(np.array(d["kl"]))), kl_floor, B, inv_b, out2.data_ptr(), None if met is None else met.data_ptr(), 2.5,
                                          None if bp is None else P(dev(np.array(bp))), 0 if bp is None else bp.shape[0], channels, db.data_ptr() if bp is not None else None)
        else:
            L.mi_vae_finalize_losses(stream(), P(dev(np.array(d["partial"]))), nchunks, P(dev(np.array(d["kl"]))), kl_floor, B, inv_b, out2.data_ptr(), None if met is None else met.data_ptr(), 2.5)
    torch.cuda.synchronize()
    return out2, met, db


def check_finalize(d, res, kl_floor, B, inv_b, channels, calls):
    out2, met, db = res
    r = vc.fin_ref64(d, kl_floor, B, inv_b)
    o = host(out2)
    assert tail_untouched(out2, 2) and np.isfinite(o).all()
    rel = np.abs(o[:2] - [r["recon"], r["kl"]]) / np.abs([r["recon"], r["kl"]])
    note("3 finalize", "out2 rel.", rel, vc.FIN_OUT_REL)
    assert (rel <= vc.FIN_OUT_REL).all(), rel
    if met is not None:                                                                          # two calls: r + r is exact in fp32
        m = host(met)
        assert m[0] == 2 * o[0] and m[1] == 2 * o[1] and m[2] == 5.0 and m[3] == SENT
    g = host(db)
    if d["bpart"] is not None:
        err, bound = np.abs(g[:channels] - (vc.DBIAS_START + calls * r["dbias"][:channels])), vc.FIN_DBIAS_REL * calls * r["dbias_abs"][:channels]
        note("3 finalize", "dbias / bound", err / bound, 1.0)
        assert (err <= bound).all() and np.isfinite(g).all(), (err, bound)
    assert (g[channels if d["bpart"] is not None else 0:] == vc.DBIAS_START).all()               # dbias[channels:] untouched (the NaN column included)


@pytest.mark.parametrize("i", range(len(vc.FIN_N_PARTIAL)))
def test_finalize_losses_flat_partials(i):
    n, B = vc.FIN_N_PARTIAL[i], vc.FIN_B[i % 4]
    kl_floor = 0.0 if i % 2 == 0 else 0.5
    d = vc.fin_data(n, B, kl_floor, 0)
    inv_b = 1.0 / (B + 3)
    for metrics in (False, True):
        a = run_finalize(d, n, B, kl_floor, inv_b, metrics)
        check_finalize(d, a, kl_floor, B, inv_b, 0, 1)
        b = run_finalize(d, n, B, kl_floor, inv_b, metrics)                                      # one block, a fixed tree: two runs are bitwise equal
        assert np.array_equal(bits(a[0]), bits(b[0])) and (not metrics or np.array_equal(bits(a[1]), bits(b[1])))


@pytest.mark.parametrize("channels", [1, 2, 3])
@pytest.mark.parametrize("nb", vc.FIN_N_BIAS)
def test_finalize_losses_bias_partials(nb, channels):
    n, B, kl_floor = 35, 5, 0.5
    d = vc.fin_data(n, B, kl_floor, nb)
    for metrics in (False, True):
        a = run_finalize(d, n, B, kl_floor, 1.0 / B, metrics, channels)
        check_finalize(d, a, kl_floor, B, 1.0 / B, channels, 2 if metrics else 1)
        b = run_finalize(d, n, B, kl_floor, 1.0 / B, metrics, channels)
        assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[2]), bits(b[2]))
    c = run_finalize(d, n, B, kl_floor, 1.0 / B, False, flat=False, nchunks=7)                   # the [B][chunks] entry point: the same list
    assert np.array_equal(bits(c[0]), bits(run_finalize(dict(d, bpart=None), n, B, kl_floor, 1.0 / B, False)[0]))


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. Adam over the flat buffer
# ---------------------------------------------------------------------------------------------------------------------------------------
def _adam_ref():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ref = ctypes.CDLL(os.path.join(root, "oracle", "libgae_ref.so"))
    ref.adam_tf_f32.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_size_t] + [ctypes.c_float] * 4
    return ref


@pytest.mark.parametrize("n", vc.ADAM_N)
def test_adam_tf_flat_trips_tail_and_planted_gradients(n):
    L = milib.get()
    p, m, v, g = vc.adam_data(n)
    alpha = vc.adam_alpha()
    pc, mc, vc_ = p.copy(), m.copy(), v.copy()
    _adam_ref().adam_tf_f32(pc.ctypes.data, mc.ctypes.data, vc_.ctypes.data, g.ctypes.data, n, alpha, F32(0.9), F32(0.999), F32(1e-8))
    assert np.isfinite(pc).all()                                                                 # g x g overflows: v is inf, the step 0, p stays finite
    npad = (n + 7) // 8 * 8 + 8
    big = n > 1 << 20
    variants = [("bf16", 1, False), (None, 0, True)] if big else [(None, 1, False), (None, 0, False), ("bf16", 0, False), ("bf16", 1, True), ("x3", 1, False), ("x3", 0, True)]
    for shadow_dt, clear, use_dev in variants:
        buf = [torch.full((npad,), vc.ADAM_PAD, device="cuda") for _ in range(4)]
        for t, a in zip(buf, (p, m, v, g)):
            t[:n] = torch.from_numpy(a.copy()).cuda()
        sh = None if shadow_dt is None else alloc(DT[shadow_dt][1], npad, fill=vc.ADAM_PAD)
        ptrs = [t.data_ptr() for t in buf]
        shp = None if sh is None else sh.data_ptr()
        if use_dev:                                                                              # the step size comes from device memory; the argument holds a wrong one
            adev = dev(np.array([alpha], F32))
            if shadow_dt == "x3":
                L.mi_adam_tf_flat_shadow(stream(), *ptrs, n, 123.0, adev.data_ptr(), 0.9, 0.999, 1e-8, shp, milib.MI_BF16X3, clear)
            else:
                L.mi_adam_tf_flat_dev(stream(), *ptrs, n, 123.0, adev.data_ptr(), 0.9, 0.999, 1e-8, shp, clear)
        elif shadow_dt == "x3":
            L.mi_adam_tf_flat_shadow(stream(), *ptrs, n, float(alpha), None, 0.9, 0.999, 1e-8, shp, milib.MI_BF16X3, clear)
        else:
            L.mi_adam_tf_flat(stream(), *ptrs, n, float(alpha), 0.9, 0.999, 1e-8, shp, clear)
        tag = (shadow_dt, clear, use_dev)
        for t, want, what in zip(buf, (pc, mc, vc_, np.zeros(n, F32) if clear else g), "pmvg"):
            b = bits(t)
            bad = np.flatnonzero(b[:n] != want.view(np.uint32))
            assert bad.size == 0, (tag, what, bad[:8], t[:n].cpu().numpy()[bad[:8]], want[bad[:8]])
            assert tail_untouched(t, n, fill=vc.ADAM_PAD), (tag, what, "pad")
        if sh is not None:
            assert np.array_equal(bits(sh)[:n], store_bits(pc, shadow_dt)) and tail_untouched(sh, n, shadow_dt, fill=vc.ADAM_PAD), tag
    if not big:
        buf = [torch.full((npad,), vc.ADAM_PAD, device="cuda") for _ in range(4)]
        with pytest.raises(milib.MiError):                                                       # a parameter pointer that is not 16-byte aligned
            L.mi_adam_tf_flat(stream(), buf[0].data_ptr() + 4, buf[1].data_ptr(), buf[2].data_ptr(), buf[3].data_ptr(), n, float(alpha), 0.9, 0.999, 1e-8, None, 1)
        assert all(tail_untouched(t, 0, fill=vc.ADAM_PAD) for t in buf)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. split-K finish, uint8 -> [0, 1]
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("MN", vc.SPLITK_SHAPES)
def test_splitk_finish(MN, dt):
    L = milib.get()
    code, td = DT[dt]
    M, N = MN
    mn = M * N
    for ns in vc.SPLITK_NSPLIT:
        slabs, bias, mask = vc.splitk_data(M, N, ns, dt)
        sd, bd, md = dev(np.array(slabs)), dev(np.array(bias)), dev(np.array(mask), td)
        assert np.array_equal(np.isnan(host(md).reshape(-1)), np.isnan(mask.reshape(-1))) and np.array_equal(np.nan_to_num(host(md).reshape(-1)), np.nan_to_num(mask.reshape(-1)).astype(np.float64))
        for use_bias in (0, 1):
            for relu in (0, 1):
                for use_mask in (0, 1):
                    ref = vc.splitk_ref32(slabs, bias if use_bias else None, relu, mask if use_mask else None)
                    for out_f32 in (0, 1):
                        out = fbuf(mn, 4) if out_f32 else out_buf(dt, mn, 4)
                        L.mi_splitk_finish(stream(), code, sd.data_ptr(), ns, M, N, bd.data_ptr() if use_bias else None, relu, md.data_ptr() if use_mask else None, out.data_ptr(), out_f32)
                        tag = (ns, use_bias, relu, use_mask, out_f32)
                        assert np.array_equal(bits(out)[:mn], store_bits(ref, "f32" if out_f32 else dt)), tag
                        assert tail_untouched(out, mn, "f32" if out_f32 else dt), tag
    out = out_buf(dt, 64)
    for badN in (6, 0):
        with pytest.raises(milib.MiError):
            L.mi_splitk_finish(stream(), code, sd.data_ptr(), 1, 1, badN, None, 0, None, out.data_ptr(), 0)
    assert tail_untouched(out, 0, dt)


@pytest.mark.parametrize("n", vc.U8_N)
def test_u8_to_unit_f32(n):
    L = milib.get()
    b = vc.u8_input(n)
    want = (b.astype(F32) / F32(255)).view(np.uint32)
    src = torch.from_numpy(b).cuda()
    dst = fbuf(n)
    L.mi_u8_to_unit_f32(stream(), src.data_ptr(), dst.data_ptr(), n)                             # aligned: the 16-byte path (and the scalar tail)
    assert np.array_equal(bits(dst)[:n], want) and tail_untouched(dst, n)
    off = torch.zeros(n + 1, dtype=torch.uint8, device="cuda")
    off[1:] = src
    dst2 = fbuf(n)
    L.mi_u8_to_unit_f32(stream(), off.data_ptr() + 1, dst2.data_ptr(), n)                        # a source one byte off: the scalar path, the same bits
    assert np.array_equal(bits(dst2)[:n], want) and tail_untouched(dst2, n)
    if n == 1:
        dst3 = fbuf(4)
        L.mi_u8_to_unit_f32(stream(), src.data_ptr(), dst3.data_ptr(), 0)                        # n = 0 is accepted and writes nothing
        with pytest.raises(milib.MiError):
            L.mi_u8_to_unit_f32(stream(), src.data_ptr(), dst3.data_ptr(), -1)
        assert tail_untouched(dst3, 0)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 6. sigmoid, range check, casts, column sums
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("n", vc.SIGMOID_N)
def test_sigmoid(n, dt):
    L = milib.get()
    code, td = DT[dt]
    x = vc.sigmoid_input(n)
    xd = dev(x.copy(), td)
    out = fbuf(n)
    L.mi_sigmoid(stream(), code, xd.data_ptr(), out.data_ptr(), n)
    got = host(out)[:n]
    ref = vc.sigmoid64(host(xd).reshape(-1))
    assert tail_untouched(out, n) and np.isfinite(got).all() and (got >= 0).all() and (got <= 1).all()
    note("6 pointwise", "sigmoid |err| / (1e-6 |ref| + 1e-7)", np.abs(got - ref) / (1e-6 * np.abs(ref) + 1e-7), 1.0)
    assert_close(got, ref, 1e-6, 1e-7, "sigmoid")


@pytest.mark.parametrize("n", vc.RANGE_N)
def test_range_check(n):
    L = milib.get()
    lo, hi = 0.0, 1.0
    x = dev(vc.range_input(n, lo, hi))

    def run(preset=0):
        flag = torch.tensor([preset, 77], dtype=torch.int32, device="cuda")
        L.mi_range_check(stream(), x.data_ptr(), n, lo, hi, flag.data_ptr())
        f = flag.cpu().tolist()
        assert f[1] == 77                                                                        # the word behind the flag
        return f[0]

    assert run(0) == 0 and run(1) == 1                                                           # clean data (the bounds themselves included); a raised flag stays raised
    places = sorted({0, n - 1} | ({2048 * 256 + 1} if n > 2048 * 256 + 1 else set()))
    for i in places:
        keep = x[i].clone()
        for name, bad in vc.range_bad_values(lo, hi):
            x[i] = float(bad)
            assert bits(x[i:i + 1])[0] == np.array([bad], F32).view(np.uint32)[0]
            assert run(0) == 1, (i, name)
        x[i] = keep
    assert run(0) == 0


@pytest.mark.parametrize("n", [1000, vc.BIG_N])
def test_casts_bf16_and_split(n):
    L = milib.get()
    x = vc.cast_input(n)
    bf = alloc(torch.bfloat16, n + 1, fill=SENT)
    L.mi_cast_f32_to_bf16(stream(), P(dev(x.copy())), bf.data_ptr(), n)
    got, want = bits(bf)[:n], store_bits(x, "bf16")
    nan = np.isnan(x)
    assert tail_untouched(bf, n, "bf16") and nan.sum() == 1
    assert np.array_equal(got[~nan], want[~nan]) and ((got[nan] & 0x7fff) > 0x7f80).all()        # NaN by isnan, not by payload
    xs = vc.cast_input(n, split=True)
    words = split_encode(xs)
    sp = out_buf("x3", n, 1)
    L.mi_cast_f32_to_split(stream(), P(dev(xs.copy())), sp.data_ptr(), n)
    assert np.array_equal(bits(sp)[:n], words.view(np.uint32)) and tail_untouched(sp, n, "x3")
    back = fbuf(n)
    L.mi_cast_split_to_f32(stream(), sp.data_ptr(), back.data_ptr(), n)
    assert np.array_equal(bits(back)[:n], split_decode(words).astype(F32).view(np.uint32)) and tail_untouched(back, n)
    rt = np.abs(host(back)[:n] - xs.astype(np.float64))
    big = np.abs(xs) >= vc.SPLIT_RT_FROM
    note("6 pointwise", "split round trip rel. (|x| >= 2^-117)", rt[big] / np.abs(xs[big]), vc.SPLIT_RT_REL)
    assert (rt <= vc.split_round_trip_bound(xs)).all()


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("MN", vc.COLSUM_SHAPES)
def test_colsum_misaligned_rows_take_the_scalar_kernel(MN, dt):
    L = milib.get()
    code, td = DT[dt]
    M, N = MN
    x = vc.colsum_input(M, N)
    xb, xp = placed(x, dt, 1)
    assert xp % 16 != 0
    xr = host(xb).reshape(-1)[1:1 + M * N].reshape(M, N)
    ref = xr.sum(0) + 1.0
    out = fbuf(N, fill=1.0)
    L.mi_colsum(stream(), code, xp, M, N, out.data_ptr())
    g = host(out)
    assert g[N] == 1.0
    atol = 1e-4 * max(1.0, float(np.abs(ref).max()))
    note("6 pointwise", "colsum %s abs (bound 1e-5 |ref| + 1e-4 max)" % dt, np.abs(g[:N] - ref), atol)
    assert_close(g[:N], ref, 1e-5, atol, "colsum")
    nbytes = L.mi_colsum_scratch_bytes(code, M, N)
    runs = []
    for _ in range(2):
        scratch = torch.full((nbytes // 4 + 4,), SENT, device="cuda")
        o = fbuf(N, fill=1.0)
        L.mi_colsum_ws(stream(), code, xp, M, N, o.data_ptr(), scratch.data_ptr(), nbytes)
        assert_close(host(o)[:N], ref, 1e-5, atol, "colsum_ws")
        assert host(o)[N] == 1.0 and tail_untouched(scratch, nbytes // 4)
        runs.append(bits(o))
    assert np.array_equal(runs[0], runs[1])
