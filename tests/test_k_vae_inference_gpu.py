"""The forward-only inference path of the ConvVAE engine: the inference form of the fused encoder-head kernel (mi_conv2d_enc12_fwd with act1 == NULL: act2 alone,
conv1's band never leaves LDS) and the inference engine's slim workspace (no gradient tensors, bit words or split-K slabs of the backward pass; no conv1 activation
behind the fused head).  Every result is BITWISE what the training form / a training engine computes."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mi355 import lib as milib  # noqa: E402
from hip_helpers import DT, alloc, dev, stream  # noqa: E402
from vae_gpu_common import trained_like_params  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 80 * 160 * 3
FUSED = os.environ.get("MI355_ENC12", "1")[:1] != "0" and os.environ.get("MI355_NARROW", "1")[:1] != "0"


def _bits(t):
    return t.contiguous().view(torch.int32) if t.element_size() == 4 else t.contiguous().view(torch.int16)


@pytest.mark.parametrize("gather", [True, False])
@pytest.mark.parametrize("u8", [True, False])
@pytest.mark.parametrize("B", [1, 3, 37, 512])
def test_encoder_head_inference_form_writes_act2_of_the_training_form(B, u8, gather):
    """mi_conv2d_enc12_fwd(act1 = NULL, relu_bits1 = NULL) launches the inference form: conv2's output bit for bit what the training form (act1 + bit words stored)
    writes, on camera bytes and fp32 frames, gathered through a frame index or not; every element written (the two outputs start from different garbage).
    Bit words without act1 are refused."""
    if not FUSED:
        pytest.skip("MI355_ENC12=0 / MI355_NARROW=0 switch the fused op off (A/B runs): nothing to compare")
    L = milib.get()
    code, td = DT["bf16"]
    rng = np.random.RandomState(200 + B)
    n_frames = B + 3
    frames_u8 = rng.randint(0, 256, (n_frames, 80, 160, 3)).astype(np.uint8)
    fr = dev(frames_u8, torch.uint8) if u8 else dev(frames_u8.astype(np.float32) / np.float32(255.0))
    idxd = dev(rng.permutation(n_frames)[:B].astype(np.int32), torch.int32) if gather else None
    fmt = 2 if u8 else 1
    w1 = (rng.randn(4, 4, 3, 32) / np.sqrt(48)).astype(np.float32)
    w2 = (rng.randn(4, 4, 32, 64) / np.sqrt(512)).astype(np.float32)
    b1d, b2d = dev((0.1 * rng.randn(32)).astype(np.float32)), dev((0.1 * rng.randn(64)).astype(np.float32))
    w1t = dev(torch.from_numpy(w1).permute(3, 0, 1, 2).reshape(32, -1).contiguous(), td)
    w2t = dev(torch.from_numpy(w2).permute(3, 0, 1, 2).reshape(64, -1).contiguous(), td)
    ip = idxd.data_ptr() if gather else None
    act1 = alloc(td, B, 39, 79, 32, fill=-7.0)
    bits = torch.full((B * 39 * 79 * 2,), 0x33, device="cuda", dtype=torch.int32)
    a2_train, a2_inf = alloc(td, B, 18, 38, 64, fill=-7.0), alloc(td, B, 18, 38, 64, fill=3.0)
    launched = ctypes.c_int(0)
    L.mi_conv2d_enc12_fwd(stream(), code, fr.data_ptr(), fmt, ip, B, 80, 160, w1t.data_ptr(), b1d.data_ptr(), w2t.data_ptr(), b2d.data_ptr(),
                          act1.data_ptr(), bits.data_ptr(), a2_train.data_ptr(), ctypes.addressof(launched))
    torch.cuda.synchronize()
    assert launched.value == 1
    launched.value = -1
    L.mi_conv2d_enc12_fwd(stream(), code, fr.data_ptr(), fmt, ip, B, 80, 160, w1t.data_ptr(), b1d.data_ptr(), w2t.data_ptr(), b2d.data_ptr(),
                          None, None, a2_inf.data_ptr(), ctypes.addressof(launched))
    torch.cuda.synchronize()
    assert launched.value == 1
    assert torch.equal(_bits(a2_inf), _bits(a2_train)), "conv2's output: inference form vs training form, bit for bit"
    a2 = a2_inf.float()
    assert (a2 >= 0).all() and (a2 == 0).float().mean() > 0.05 and float(a2.max()) > 0.1
    with pytest.raises(milib.MiError, match="bit words without act1"):
        L.mi_conv2d_enc12_fwd(stream(), code, fr.data_ptr(), fmt, ip, B, 80, 160, w1t.data_ptr(), b1d.data_ptr(), w2t.data_ptr(), b2d.data_ptr(),
                              None, bits.data_ptr(), a2_inf.data_ptr(), ctypes.addressof(launched))


def _engine(precision, train, params, max_batch=512):
    from mi355.vae_device import VaeDevice
    d = VaeDevice((80, 160, 3), (80, 160, 3), 64, 1.0, 0.0, "bce", precision, max_batch=max_batch, with_optimizer=train)
    d.load_params(params)
    return d


def _table(precision, n, seed):
    u8 = np.random.RandomState(seed).randint(0, 256, (n, P), dtype=np.uint8)
    if precision == "bf16":                                 # the bf16 engine reads camera bytes (the production format)
        return torch.from_numpy(u8).cuda()
    return torch.from_numpy(u8.astype(np.float32) / np.float32(255.0)).cuda()


@pytest.mark.parametrize("B", [1, 37, 512])
@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "bf16"])
def test_inference_engine_matches_a_training_engine_bitwise(precision, B):
    """An inference engine (with_optimizer=False: the slim workspace) and a training engine with the same parameters and max_batch: encode, reconstruct (mean-fed and
    sampled with injected noise), decode and the evaluation pass (forward without gradient: losses, posterior means, KL rows) are bitwise equal -- and the posterior
    means equal those of the training engine's TRAINING forward (the encoder head's training form)."""
    params = trained_like_params(4)
    rng = np.random.RandomState(50 + B)
    n = B + 5
    table = _table(precision, n, 60 + B)
    idx = torch.from_numpy(rng.permutation(n)[:B].astype(np.int32)).cuda()
    eps = torch.from_numpy(rng.standard_normal((B, 64)).astype(np.float32)).cuda()
    z = torch.from_numpy(rng.standard_normal((B, 64)).astype(np.float32)).cuda()

    def run(d):
        out = {}
        mean = torch.empty(B, 64, device="cuda")
        d.encode(table, idx, B, mean)
        out["encode"] = mean
        for s in (0, 1):
            r = torch.empty(B, P, device="cuda")
            d.reconstruct(table, idx, B, eps if s else None, s, r)
            out["reconstruct%d" % s] = r
        r = torch.empty(B, P, device="cuda")
        d.decode(z, B, r)
        out["decode"] = r
        for s in (0, 1):
            d.forward(table, table, idx, B, 1.0 / B, eps if s else None, s, 0, accumulate_metrics=False)
            out["evaluate%d" % s] = torch.cat([d.losses.clone(), d._view(1, B * 64).clone(), d._view(2, B * 64).clone(), d._view(3, B).clone()])
        torch.cuda.synchronize()
        return out

    inf, tr = _engine(precision, False, params), _engine(precision, True, params)
    a, b = run(inf), run(tr)
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), "%s (%s, B = %d): inference engine vs training engine" % (k, precision, B)
    assert 0.0 < float(a["reconstruct0"].min()) and float(a["reconstruct0"].max()) < 1.0 and float(a["encode"].abs().max()) > 0
    assert float(a["evaluate0"][0]) > 0
    tr.forward(table, table, idx, B, 1.0 / B, eps, 1, 1, accumulate_metrics=False)      # the training forward: act1 (+ bit words) stored for a backward pass
    torch.cuda.synchronize()
    assert torch.equal(_bits(tr._view(1, B * 64)), _bits(a["encode"].flatten())), "posterior means: training forward vs the inference engine's encode"
    inf.close(); tr.close()


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_encode_between_training_steps_changes_nothing(precision):
    """On a training engine, encode() runs the inference form (nothing is stored for a backward pass).  train_step -> encode(other frames) -> train_step leaves parameters,
    Adam state, losses and accumulated metrics bitwise where train_step -> train_step leaves them."""
    params = trained_like_params(5)
    B = 64
    table = _table(precision, 3 * B, 70)
    rng = np.random.RandomState(71)
    perm = rng.permutation(3 * B).astype(np.int32)
    idx_train, idx_other = torch.from_numpy(perm[:B]).cuda(), torch.from_numpy(perm[B:2 * B]).cuda()
    eps = [torch.from_numpy(rng.standard_normal((B, 64)).astype(np.float32)).cuda() for _ in range(2)]
    a, b = _engine(precision, True, params, 128), _engine(precision, True, params, 128)
    mean = torch.empty(B, 64, device="cuda")
    a.train_step(table, table, idx_train, B, 1.0 / B, eps[0], 1e-3)
    a.encode(table, idx_other, B, mean)
    a.train_step(table, table, idx_train, B, 1.0 / B, eps[1], 1e-3)
    b.train_step(table, table, idx_train, B, 1.0 / B, eps[0], 1e-3)
    b.train_step(table, table, idx_train, B, 1.0 / B, eps[1], 1e-3)
    torch.cuda.synchronize()
    assert float(mean.abs().max()) > 0
    for name in ("params", "adam_m", "adam_v", "metrics", "losses"):
        assert torch.equal(_bits(getattr(a, name)), _bits(getattr(b, name))), name
    a.close(); b.close()


def test_inference_engine_refuses_backward_and_adam():
    """An inference engine has no gradient buffer and no gradient regions: backward, Adam and the one-call step raise MiError; forward(want_grad=1) is a forward
    without gradient (bitwise the evaluation pass)."""
    params = trained_like_params(6)
    B = 37
    d = _engine("bf16", False, params, 64)
    table = _table("bf16", B, 80)
    eps = torch.from_numpy(np.random.RandomState(81).standard_normal((B, 64)).astype(np.float32)).cuda()
    d.forward(table, table, None, B, 1.0 / B, eps, 1, 1, accumulate_metrics=False)
    l1 = d.losses.clone()
    d.forward(table, table, None, B, 1.0 / B, eps, 1, 0, accumulate_metrics=False)
    torch.cuda.synchronize()
    assert torch.equal(_bits(l1), _bits(d.losses)) and float(l1[0]) > 0
    with pytest.raises(milib.MiError):
        d.backward(table, None, eps, 1.0 / B)
    with pytest.raises(milib.MiError):
        d.apply_adam(1e-3)
    with pytest.raises(milib.MiError):
        d.train_step(table, table, None, B, 1.0 / B, eps, 1e-3)
    d.close()


_GUARD_CHILD = r"""
import ctypes, json, sys
sys.path[:0] = [%(pkg)r, %(root)r, %(tests)r]
import numpy as np, torch
from mi355 import lib as milib
from mi355.vae_device import VaeDevice
from vae_gpu_common import trained_like_params
L = milib.get()
res = {}
for precision in ("bf16", "fp32"):
    d = VaeDevice((80, 160, 3), (80, 160, 3), 64, 1.0, 0.0, "bce", precision, max_batch=64, with_optimizer=False)
    d.load_params(trained_like_params(7))
    B = 37
    u8 = np.random.RandomState(8).randint(0, 256, (B + 3, 80 * 160 * 3), dtype=np.uint8)
    table = torch.from_numpy(u8).cuda() if precision == "bf16" else torch.from_numpy(u8.astype(np.float32) / np.float32(255.0)).cuda()
    idx = torch.from_numpy(np.random.RandomState(9).permutation(B + 3)[:B].astype(np.int32)).cuda()
    eps = torch.from_numpy(np.random.RandomState(10).standard_normal((B, 64)).astype(np.float32)).cuda()
    mean, rec = torch.empty(B, 64, device="cuda"), torch.empty(B, 80 * 160 * 3, device="cuda")
    n0, bad0, _ = d.check_guards()
    d.encode(table, idx, B, mean)
    d.reconstruct(table, idx, B, None, 0, rec)
    d.reconstruct(table, idx, B, eps, 1, rec)
    d.decode(mean, B, rec)
    for s in (0, 1):
        for g in (0, 1):
            d.forward(table, table, idx, B, 1.0 / B, eps if s else None, s, g)
    # per-op timing of every op (mode 1): where the workspace has no conv1 activation the fused launch is what is timed
    nops = L.mi_vae_op_count()
    ms, cnt = np.zeros(nops, np.float32), np.zeros(nops, np.int32)
    L.mi_vae_timing_begin(d.handle, 1, 0, 256)
    d.encode(table, idx, B, mean)
    L.mi_vae_timing_collect(d.handle, ms.ctypes.data, cnt.ctypes.data, nops)
    n, bad, _ = d.check_guards()
    res[precision] = {"regions": n, "regions0": n0, "bad0": bad0, "bad": bad, "err": L.cdll.mi_last_error().decode() if bad else "",
                      "conv1": int(cnt[0]), "conv2": int(cnt[1]), "finite": bool(torch.isfinite(rec).all())}
    d.close()
print(json.dumps(res))
"""


def test_inference_engine_touches_no_guard_in_debug_mode():
    """MI355_DEBUG_GUARDS=1 (read when the workspace is sized and carved; a fresh child process): 256 guard bytes behind every region of the slim inference workspace.
    encode, reconstruct (mean-fed and sampled), decode, the evaluation pass (with and without want_grad) and per-op timing write none of them -- on the bf16 engine
    (no conv1 activation: the timed encode records the one fused launch) and on the fp32 engine (two launches)."""
    code = _GUARD_CHILD % {"pkg": os.path.join(ROOT, "carla-ppo_amd"), "root": ROOT, "tests": os.path.join(ROOT, "tests")}
    env = dict(os.environ, MI355_DEBUG_GUARDS="1")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    for precision, v in res.items():
        assert v["regions"] >= 20 and v["regions"] == v["regions0"] and v["bad0"] == 0, (precision, v)
        assert v["bad"] == 0, (precision, v["err"])
        assert v["finite"], precision
    assert res["fp32"]["conv1"] == 1 and res["fp32"]["conv2"] == 1
    if FUSED:
        assert res["bf16"]["conv1"] == 0 and res["bf16"]["conv2"] == 1
