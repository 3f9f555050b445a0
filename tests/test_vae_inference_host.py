"""CPU-only: the workspace of an inference ConvVAE engine (MiVaeDesc::inference_only, VAE(training=False)) holds the regions of its forward passes only.
mi_vae_workspace_bytes is a pure host function of the descriptor (no GPU)."""
import ctypes
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MB = 1 << 20
ENC_C = (3, 32, 64, 128, 256)
DEC_C = (256, 128, 64, 32)
DEC_K = (4, 4, 5, 4)


def _maps(ct):
    """(conv outputs act[1..4], decoder maps dec[0..4]) as element counts per frame, from the reference geometry (80 x 160 x 3 frames, k4 s2 convolutions)."""
    h, w, act = 80, 160, []
    for i in range(4):
        h, w = (h - 4) // 2 + 1, (w - 4) // 2 + 1
        act.append(h * w * ENC_C[i + 1])
    dec = [h * w * DEC_C[0]]
    for i in range(4):
        h, w = (h - 1) * 2 + DEC_K[i], (w - 1) * 2 + DEC_K[i]
        dec.append(h * w * (DEC_C[i + 1] if i < 3 else ct))
    return act, dec


def _desc(dtype, B, ct, inference_only):
    from mi355 import lib as milib
    return milib.MiVaeDesc(dtype, B, 80, 160, 3, ct, 64, 0, 1.0, 0.0, inference_only)


def _ws(dtype, B, ct, inference_only):
    from mi355 import lib as milib
    n = milib.get().mi_vae_workspace_bytes(ctypes.byref(_desc(dtype, B, ct, inference_only)))
    assert n > 0
    return n


@pytest.mark.parametrize("B", [1, 16, 512, 4096])
@pytest.mark.parametrize("ct", [3, 1])
@pytest.mark.parametrize("dtype", [0, 2, 1])
def test_inference_workspace_carries_forward_regions_only(dtype, ct, B):
    """Forward activations act[2..4] and dec[0..4], plus conv1's activation act[1] unless the bf16 engine runs conv1 + conv2 as the fused encoder head (it never
    leaves LDS there), plus 16 KB per frame and 32 MB for the latent, the loss partials, the split-K heads slab, the rollout buffer, the noise and the weight-fragment
    copies.  No gradient tensors, ReLU bit words or slab scratch.  The training engine of the same descriptor still carries every gradient tensor."""
    act, dec = _maps(ct)
    esz = 2 if dtype == 1 else 4
    fused = dtype == 1 and os.environ.get("MI355_ENC12", "1")[:1] != "0" and os.environ.get("MI355_NARROW", "1")[:1] != "0"
    fwd = B * esz * (sum(act[1:]) + sum(dec) + (0 if fused else act[0]))
    inf = _ws(dtype, B, ct, 1)
    assert inf >= fwd, "the forward regions must fit"
    assert inf <= fwd + B * 16 * 1024 + 32 * MB, "inference workspace %.1f MB against %.1f MB of forward activations" % (inf / MB, fwd / MB)
    grads = B * esz * (sum(act) + sum(dec))                 # gact[1..4] + gdec[0..4] of the training engine
    assert _ws(dtype, B, ct, 0) >= inf + grads


def test_inference_workspace_at_batch_512_bf16():
    """The replay encoder's engine (bench.py: VAE(training=False), bf16, chunks of 512): about 300 MB instead of about 810 MB."""
    inf, tr = _ws(1, 512, 3, 1), _ws(1, 512, 3, 0)
    assert inf < 320 * 1e6 and tr > 1200 * 1e6


def test_conv1_activation_is_carved_where_the_encoder_head_runs_as_two_launches():
    """With the fused encoder head switched off (MI355_ENC12=0, read once per process: a fresh child) the bf16 inference engine carves conv1's activation again,
    exactly that region; the fp32 engine (always two launches) is unchanged, and so is every training engine."""
    code = ("import ctypes, json, sys\n"
            "sys.path[:0] = [%r, %r]\n"
            "from mi355 import lib as milib\n"
            "L = milib.get()\n"
            "out = {}\n"
            "for dt in (0, 1):\n"
            "    for inf in (0, 1):\n"
            "        out['%%d/%%d' %% (dt, inf)] = L.mi_vae_workspace_bytes(ctypes.byref(milib.MiVaeDesc(dt, 512, 80, 160, 3, 3, 64, 0, 1.0, 0.0, inf)))\n"
            "print(json.dumps(out))\n") % (os.path.join(ROOT, "carla-ppo_amd"), ROOT)
    import json
    env = dict(os.environ, MI355_ENC12="0")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    off = json.loads(r.stdout.strip().splitlines()[-1])
    if os.environ.get("MI355_ENC12", "1")[:1] == "0" or os.environ.get("MI355_NARROW", "1")[:1] == "0":
        pytest.skip("the fused encoder head is already off in this environment: nothing to compare")
    act1 = 512 * 39 * 79 * 32 * 2
    assert off["1/1"] - _ws(1, 512, 3, 1) == (act1 + 255) // 256 * 256
    assert off["0/1"] == _ws(0, 512, 3, 1)
    assert off["1/0"] == _ws(1, 512, 3, 0) and off["0/0"] == _ws(0, 512, 3, 0)
