"""Worker of test_reparam_wide_variant_gives_the_same_bits (tests/test_w_vae_elementwise_gpu.py): the reparameterisation kernels forward and backward at the shapes of
vae_elementwise_cases.REPARAM_WIDE_SHAPES in fp32, and the SHA-256 of every output.  The test starts this file once as a fresh process with MI355_REPARAM_WIDE=1 (the
knob is read when the library is loaded: a process has it or has it not) and calls digests() itself with the knob off: "same order, same sums" means equal digests."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "carla-ppo_amd"), ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import vae_elementwise_cases as vc  # noqa: E402
from mi355 import lib as milib  # noqa: E402


def digests():
    L = milib.get()
    st = torch.cuda.current_stream().cuda_stream
    out = {}
    for B, Z, ns, nd in vc.REPARAM_WIDE_SHAPES:
        d = vc.reparam_data(B, Z, ns, nd)
        t = {k: torch.from_numpy(np.array(d[k])).cuda() for k in ("heads", "bm", "bl", "eps", "dzs")}
        mean, logvar, z = (torch.zeros(B, Z, device="cuda") for _ in range(3))
        kl, dh = torch.zeros(B, device="cuda"), torch.zeros(B, 2 * Z, device="cuda")
        L.mi_vae_reparam_kl_fwd(st, milib.MI_F32, t["heads"].data_ptr(), ns, t["bm"].data_ptr(), t["bl"].data_ptr(), t["eps"].data_ptr(), 1, B, Z,
                                mean.data_ptr(), logvar.data_ptr(), z.data_ptr(), kl.data_ptr())
        L.mi_vae_reparam_kl_bwd(st, milib.MI_F32, t["dzs"].data_ptr(), nd, mean.data_ptr(), logvar.data_ptr(), t["eps"].data_ptr(), kl.data_ptr(),
                                vc.REPARAM_BETA, 0.0, vc.INV_B, B, Z, dh.data_ptr())
        torch.cuda.synchronize()
        for name, a in (("mean", mean), ("logvar", logvar), ("z", z), ("kl", kl), ("dheads", dh)):
            out["%dx%dx%dx%d.%s" % (B, Z, ns, nd, name)] = hashlib.sha256(a.cpu().numpy().tobytes()).hexdigest()
    return out


if __name__ == "__main__":
    assert os.environ.get("MI355_REPARAM_WIDE") == "1", "the worker is the run with the knob on"
    print(json.dumps(digests()))
