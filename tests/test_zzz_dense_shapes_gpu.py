"""The dense entry points against float64 OFF the models' shapes: every case of tests/dense_shape_cases.py (the small-M kernel at the edge of its predicate, every tall-K
instantiation with step counts around its six-step group, gemm2's split-K with a short last slab and its fall-backs, every gemm2 / first-generation tile from below, at
and past its size, the whole-tile filter gradient with idle blocks and every fill level of its ring, the one-wave-per-tile filter gradient with 1 / 2 / 4 waves, the
first-generation filter gradient's row splits / scratch / bias row, the pair launch, and the shapes the launchers must refuse) through the C ABI, with the dispatch pinned
by mi_set_tuning (restored in `finally`).  The family each case reaches is asserted on the CPU (test_dense_shape_cases_host.py).

Every output, dW, dbias and slab buffer carries sentinel elements behind its extent that must survive; every output buffer starts at a fill value.  Bounds are the
project's (tests/test_ops_gpu.py): hip_helpers.tols for outputs in the storage type, 1e-5 / 3e-5 max|ref| for fp32 outputs and split-K slabs, 1e-5 / 3e-5 max|ref| for
filter and bias gradients, times max(1, sqrt(M / 512)) on the whole-tile and one-wave-per-tile kernels.  Measured distances are printed (pytest -s) as
`MEASURE family | what | achieved | bound`: profiles/r26_dense_shapes.md."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import dense_shape_cases as dc  # noqa: E402
from hip_helpers import DT, P, alloc, assert_close, dev, host, keep_reset, stream, tols  # noqa: E402
from mi355 import lib as milib  # noqa: E402

FILL, SENT, EXTRA, GUARD = 7.0, 7.0, 8, 256
MEAS = {}


def note(section, what, achieved, bound=None):
    a = float(np.max(achieved)) if np.size(achieved) else 0.0
    key = (section, what)
    if key not in MEAS or a > MEAS[key][0]:
        MEAS[key] = (a, None if bound is None else float(bound))


def print_measurements():
    print()
    for (section, what), (a, b) in sorted(MEAS.items()):
        print("MEASURE %s | %s | %.3g | %s" % (section, what, a, "-" if b is None else "%.3g" % b))


@pytest.fixture(scope="module", autouse=True)
def _print_measurements():
    yield
    print_measurements()


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


def measure(fam, dt, what, got, ref, rtol, atol):
    """assert_close with the achieved distance noted first (so that a failing case still leaves its figure)."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    scale = float(np.abs(ref).max()) or 1.0
    note(fam, "%s (%s): worst |err| / max|ref|" % (what, dt), err.max() / scale, (atol + rtol * scale) / scale)
    assert_close(got, ref, rtol, atol, "%s %s %s" % (fam, dt, what))


def ptr(t):
    return None if t is None else P(t)


def buf32(start, n):
    """fp32 device buffer of n + EXTRA elements: `start` (a float: fill value, or an array: previous contents) and the sentinel tail."""
    t = torch.full((n + EXTRA,), SENT, device="cuda", dtype=torch.float32)
    if isinstance(start, float):
        t[:n] = start
    else:
        t[:n] = torch.from_numpy(np.ascontiguousarray(start, np.float32).reshape(-1)).cuda()
    return t


def split32(t, n, shape):
    """-> (float32 numpy [shape], the sentinel tail survived)."""
    torch.cuda.synchronize()
    h = t.detach().cpu().numpy()
    return h[:n].reshape(shape).copy(), bool((h[n:] == SENT).all())


def scratch_buf(nbytes):
    return torch.full((nbytes + GUARD,), 0xA5, device="cuda", dtype=torch.uint8)


def guard_ok(ws, nbytes):
    torch.cuda.synchronize()
    return bool((ws[nbytes:] == 0xA5).all().item())


# ---------------------------------------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------------------------------------
def run_fwd(c, d, raw=False):
    """-> (result float64 [M, N] or [nsplit, M, N], the sentinel tail survived, return code).  raw: the unchecked binding (a refused call returns its code)."""
    L = milib.get().cdll if raw else milib.get()
    code, td = DT[c.dt]
    o = c.opt
    out_f32 = bool(o.get("out_f32"))
    shape = (c.nsplit, c.M, c.N) if c.nsplit > 1 else (c.M, c.N)
    n = int(np.prod(shape))
    out = torch.full((n + EXTRA,), FILL, device="cuda", dtype=torch.float32) if out_f32 else alloc(td, n + EXTRA, fill=FILL)
    wd = dev(d["w"] if c.layout == 0 else np.ascontiguousarray(d["w"].T), td)
    bias = dev(d["b"]) if o.get("bias") else None
    mask = dev(d["mask"], td) if o.get("mask") else None
    rc = L.mi_gemm_bias_act(stream(), code, P(dev(d["a"], td)), c.M, c.K, P(wd), c.layout, c.N, ptr(bias), int(bool(o.get("relu"))), ptr(mask), P(out), int(out_f32), c.nsplit)
    h = host(out)
    return h[:n].reshape(shape), bool((h[n:] == SENT).all()), rc


def check_fwd(c, env=None):
    fam, _ = dc.family_of(c, env)
    d, r = dc.reference(c, env)
    with Tuning(c.tune):
        got, tail_ok, _ = run_fwd(c, d)
        again = run_fwd(c, d)[0] if c.nsplit > 1 else None
    assert tail_ok, "wrote behind the output"
    if c.nsplit > 1:
        measure(fam, c.dt, "split-K slab", got, r["slabs"], 1e-5, 3e-5 * float(np.abs(r["slabs"]).max()))
        measure(fam, c.dt, "split-K slabs summed", got.sum(0), r["out"], 1e-5, 3e-5 * float(np.abs(r["out"]).max()))
        assert np.array_equal(got, again), "two runs of the slab form differ"
    elif c.opt.get("out_f32"):
        measure(fam, c.dt, "fp32 output", got, r["out"], 1e-5, 3e-5 * float(np.abs(r["out"]).max()))
    else:
        rt, at = tols(c.dt, float(np.abs(r["out"]).max()))
        measure(fam, c.dt, "output", got, r["out"], rt, at)
    return fam


FWD = [c for c in dc.CASES if c.entry == "fwd" and not c.family.startswith("refused")]


@pytest.mark.parametrize("c", FWD, ids=dc.case_id)
def test_dense_forward_case(c):
    assert check_fwd(c) == c.family


# ---------------------------------------------------------------------------------------------------------------------------------------
# filter gradients
# ---------------------------------------------------------------------------------------------------------------------------------------
def run_wgrad(c, d, overwrite=None, dbias=None, raw=False, start=None):
    """One call of the filter-gradient entry point the case's options select -> {dw, db (float32), tails (all sentinels survived), rc}.  The buffers start at the fill
    value (storing form) or at dw0 / db0 (adding form) unless `start` = (dw, db) says otherwise."""
    L = milib.get().cdll if raw else milib.get()
    code, td = DT[c.dt]
    o = c.opt
    ow = bool(o.get("overwrite")) if overwrite is None else overwrite
    want_db = bool(o.get("dbias")) if dbias is None else dbias
    M, K, N = c.M, c.K, c.N
    s_dw, s_db = start if start is not None else ((FILL, FILL) if ow else (d["dw0"], d["db0"]))
    dw, db = buf32(s_dw, K * N), buf32(s_db, N)
    nbytes = dc.scratch_given(c, dc.knobs_of(c))
    ws = scratch_buf(nbytes) if nbytes > 0 else None
    ad, dyd = dev(d["a"], td), dev(d["dy"], td)
    args = (stream(), code, P(ad), P(dyd), M, K, N, P(dw))
    if ow:
        rc = L.mi_gemm_wgrad_bias_set(*args, P(db) if want_db else None, ptr(ws), nbytes, 1)
    elif want_db:
        rc = L.mi_gemm_wgrad_bias_ws(*args, P(db), ptr(ws), nbytes)
    elif ws is not None:
        rc = L.mi_gemm_wgrad_ws(*args, P(ws), nbytes)
    else:
        rc = L.mi_gemm_wgrad(*args)
    gw, t0 = split32(dw, K * N, (K, N))
    gb, t1 = split32(db, N, (N,))
    return {"dw": gw, "db": gb, "tails": t0 and t1 and (ws is None or guard_ok(ws, nbytes)), "rc": rc, "scratch": ws, "nbytes": nbytes}


def wgrad_bounds(fam, M, ref):
    f = max(1.0, (M / 512.0) ** 0.5) if fam.startswith(("dwg.", "dwgs.")) else 1.0
    return 1e-5, 3e-5 * float(np.abs(ref).max()) * f


def check_wgrad(c, env=None):
    L = milib.get()
    fam, plan = dc.family_of(c, env)
    d, r = dc.reference(c, env)
    o = c.opt
    ow, want_db = bool(o.get("overwrite")), bool(o.get("dbias"))
    with Tuning(c.tune):
        if o.get("scratch") == "exact":
            assert int(L.mi_gemm_wgrad_scratch_bytes(DT[c.dt][0], c.M, c.K, c.N)) == dc.scratch_bytes(c.dt, c.M, c.K, c.N, dc.knobs_of(c))
        g = run_wgrad(c, d)
        assert g["tails"], "wrote behind dW, dbias or the slabs"
        want_w = r["dw"] if ow else d["dw0"].astype(np.float64) + r["dw"]
        want_b = r["db"] if ow else d["db0"].astype(np.float64) + r["db"]
        rt, at = wgrad_bounds(fam, c.M, r["dw"])
        measure(fam, c.dt, "dW", g["dw"], want_w, rt, at)
        if want_db:
            rt, at = wgrad_bounds(fam, c.M, r["db"])
            measure(fam, c.dt, "dbias", g["db"], want_b, rt, at)
        else:
            assert (g["db"] == (FILL if ow else d["db0"])).all(), "dbias = NULL, yet the bias buffer changed"
        if fam.endswith(".slabs"):                           # the slabs were used: the scratch no longer holds its fill pattern
            assert not bool((g["scratch"][:g["nbytes"]] == 0xA5).all().item())
        deterministic = not fam.endswith(".atomics")
        if deterministic and (o.get("twice") or c.K * c.N <= 1 << 20):
            g2 = run_wgrad(c, d)
            assert np.array_equal(g["dw"], g2["dw"]) and np.array_equal(g["db"], g2["db"]), "two runs differ"
        if fam.startswith("dwgs."):
            # adding form = storing form + the previous contents, bit for bit (one fp32 add per element); the bias row does not change dW
            st = g if ow else run_wgrad(c, d, overwrite=True)
            ad_ = run_wgrad(c, d, overwrite=False) if ow else g
            assert st["tails"] and ad_["tails"]
            assert np.array_equal(ad_["dw"], d["dw0"] + st["dw"]), "adding form != storing form + previous contents"
            if want_db:
                assert np.array_equal(ad_["db"], d["db0"] + st["db"])
                nb = run_wgrad(c, d, dbias=False)
                assert np.array_equal(nb["dw"], g["dw"]) and nb["tails"]
        if fam.startswith("dwg.") and want_db and o.get("twice"):
            nb = run_wgrad(c, d, dbias=False)
            assert np.array_equal(nb["dw"], g["dw"]) and nb["tails"] and (nb["db"] == FILL).all()
    return fam


WGRAD = [c for c in dc.CASES if c.entry == "wgrad" and not c.family.startswith("refused")]


@pytest.mark.parametrize("c", WGRAD, ids=dc.case_id)
def test_dense_filter_gradient_case(c):
    assert check_wgrad(c) == c.family


PAIR = [c for c in dc.CASES if c.entry == "pair"]


@pytest.mark.parametrize("c", PAIR, ids=dc.case_id)
def test_two_filter_gradients_in_one_launch_case(c):
    """mi_gemm_wgrad_bias_pair_ws off (64, 6144) / (6144, 128): against float64, and bit for bit the two single calls -- on the one-launch kernel and on the fall-back."""
    L = milib.get()
    code, td = DT[c.dt]
    d, r = dc.reference(c)
    probs = [(c.M, c.K, c.N, c.opt.get("dbias", True), ""), tuple(c.opt["second"]) + (c.opt.get("dbias1", True), "1")]
    with Tuning(c.tune):
        res = []
        for pair in (True, False):
            bufs, args = [], []
            for (m, k, n, with_db, sfx) in probs:
                nb = int(L.mi_gemm_wgrad_scratch_bytes(code, m, k, n)) if c.opt.get("scratch") == "exact" else 0
                assert nb == (dc.scratch_bytes(c.dt, m, k, n, dc.knobs_of(c)) if c.opt.get("scratch") == "exact" else 0)
                dw, db, ws = buf32(d["dw0" + sfx], k * n), buf32(d["db0" + sfx], n), (scratch_buf(nb) if nb else None)
                bufs.append((dw, db, ws, nb, k, n))
                args.append((P(dev(d["a" + sfx], td)), P(dev(d["dy" + sfx], td)), m, k, n, P(dw), P(db) if with_db else None, ptr(ws), nb))
            if pair:
                L.mi_gemm_wgrad_bias_pair_ws(stream(), code, *args[0], *args[1])
            else:
                for a in args:
                    L.mi_gemm_wgrad_bias_ws(stream(), code, *a)
            out = []
            for (dw, db, ws, nb, k, n) in bufs:
                gw, t0 = split32(dw, k * n, (k, n))
                gb, t1 = split32(db, n, (n,))
                assert t0 and t1 and (ws is None or guard_ok(ws, nb)), "wrote behind dW, dbias or the slabs"
                out += [gw, gb]
            res.append(out)
    for i, (m, k, n, with_db, sfx) in enumerate(probs):
        rt, at = wgrad_bounds(c.family, m, r["dw" + sfx])
        measure(c.family, c.dt, "dW", res[0][2 * i], d["dw0" + sfx].astype(np.float64) + r["dw" + sfx], rt, at)
        if with_db:
            rt, at = wgrad_bounds(c.family, m, r["db" + sfx])
            measure(c.family, c.dt, "dbias", res[0][2 * i + 1], d["db0" + sfx].astype(np.float64) + r["db" + sfx], rt, at)
        else:
            assert np.array_equal(res[0][2 * i + 1], d["db0" + sfx])
    if c.dt == "bf16":
        for x, y in zip(res[0], res[1]):
            assert np.array_equal(x, y), "the pair launch differs from the two single calls"


REFUSED = [c for c in dc.CASES if c.family.startswith("refused")]


@pytest.mark.parametrize("c", REFUSED, ids=dc.case_id)
def test_refused_shapes_return_an_error_and_write_nothing(c):
    d = dc.make_inputs(c)
    with Tuning(c.tune):
        if c.entry == "fwd":
            got, tail_ok, rc = run_fwd(c, d, raw=True)
            assert rc != 0 and tail_ok and (got == FILL).all()
        else:
            g = run_wgrad(c, d, raw=True)
            start_w, start_b = (FILL, FILL) if c.opt.get("overwrite") else (d["dw0"], d["db0"])
            assert g["rc"] != 0 and g["tails"] and (g["dw"] == start_w).all() and (g["db"] == start_b).all()
            if g["scratch"] is not None:
                assert bool((g["scratch"] == 0xA5).all().item())
        assert milib.get().cdll.mi_last_error()
    with pytest.raises(milib.MiError):                       # and through the checked binding: an exception
        with Tuning(c.tune):
            run_fwd(c, d) if c.entry == "fwd" else run_wgrad(c, d)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the environment-only knobs: fresh child processes (tests/dense_knob_worker.py)
# ---------------------------------------------------------------------------------------------------------------------------------------
def knob_step(step):
    """Runs in the child: the cases of dc.env_cases(step) on the kernel the step's knobs leave them, against the same float64 references and bounds."""
    env, _, allowed = dc.ENV_STEPS[step]
    for name, v in env.items():
        assert os.environ.get(name) == str(v), name
    done = []
    for c in dc.env_cases(step):
        fam = check_fwd(c, env) if c.entry == "fwd" else check_wgrad(c, env)
        assert fam in allowed and fam != c.family
        done.append([dc.case_id(c), fam])
    return done


def test_environment_only_knobs_in_child_processes():
    """MI355_TALLK, MI355_GEMM2_SPLITK, MI355_DWG and MI355_DWG_NST are read when the library is loaded: two fresh child processes run the tall-K, gemm2 split-K and
    whole-tile cases on the kernels the knobs fall back to (and on dwg_kernel<4>), each under its own time limit; nothing is started after a bad exit status."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dense_knob_worker.py")
    for step, (env, _, _) in enumerate(dc.ENV_STEPS):
        r = subprocess.run([sys.executable, worker, str(step)], env=dict(os.environ, **{k: str(v) for k, v in env.items()}), capture_output=True, text=True, timeout=150)
        for line in r.stdout.splitlines():
            if line.startswith("MEASURE"):
                print(line.replace("MEASURE ", "MEASURE [%s] " % " ".join("%s=%s" % kv for kv in sorted(env.items())), 1))
        assert r.returncode == 0, "step %d: exit status %d\n%s\n%s" % (step, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        done = json.loads([line for line in r.stdout.splitlines() if line.startswith("[")][-1])
        assert [x[0] for x in done] == [dc.case_id(c) for c in dc.env_cases(step)] and len(done) >= 15
