"""CPU-only tests of the PPO precision switch (split-bf16 "bf16x3" mode of the training step): the constructor surface and its environment
knob, the C-ABI entry points, and the gfx950 code of the split instantiations of the fused kernels (compiled here, no GPU needed)."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Box:
    low, high, shape = np.array([-1, 0], np.float32), np.array([1, 1], np.float32), (2,)


def test_ppo_constructor_takes_a_precision(tmp_path, monkeypatch):
    import ppo
    monkeypatch.delenv("MI355_PPO_PRECISION", raising=False)
    monkeypatch.delenv("MI355_PRECISION", raising=False)
    assert list(__import__("inspect").signature(ppo.PPO.__init__).parameters)[-1] == "precision"
    assert ppo.PPO(np.array([67]), Box(), model_dir=str(tmp_path / "a"), precision="bf16x3").precision == "bf16x3"
    assert ppo.PPO(np.array([67]), Box(), model_dir=str(tmp_path / "b")).precision == "fp32"
    assert ppo.PPO(np.array([67]), Box(), model_dir=str(tmp_path / "c"), precision="f32").precision == "fp32"
    for bad in ("bf16", "fp16", "x3"):
        with pytest.raises(ValueError):
            ppo.PPO(np.array([67]), Box(), model_dir=str(tmp_path / "d"), precision=bad)


def test_vae_precision_variable_does_not_reach_ppo(tmp_path, monkeypatch):
    import ppo
    monkeypatch.delenv("MI355_PPO_PRECISION", raising=False)
    monkeypatch.setenv("MI355_PRECISION", "bf16x3")              # the VAE's knob (bench.py, test tooling)
    assert ppo.PPO(np.array([67]), Box(), model_dir=str(tmp_path / "a")).precision == "fp32"
    monkeypatch.setenv("MI355_PPO_PRECISION", "bf16x3")
    assert ppo.PPO(np.array([67]), Box(), model_dir=str(tmp_path / "b")).precision == "bf16x3"
    assert ppo.PPO(np.array([67]), Box(), model_dir=str(tmp_path / "c"), precision="fp32").precision == "fp32"     # the argument wins
    monkeypatch.setenv("MI355_PPO_PRECISION", "bogus")
    with pytest.raises(ValueError):
        ppo.PPO(np.array([67]), Box(), model_dir=str(tmp_path / "d"))


def test_precision_entry_points_are_declared_exported_and_checked():
    from mi355 import lib as milib
    protos = milib.parse_header()
    assert protos["mi_ppo_set_precision"] == ("int", [("void*", "h"), ("int", "dtype")])
    assert protos["mi_ppo_precision"] == ("int", [("void*", "h")])
    L = milib.get()
    assert hasattr(L.cdll, "mi_ppo_set_precision") and hasattr(L.cdll, "mi_ppo_precision")
    assert L.mi_abi_version() == 7
    text = open(milib.HEADER).read()
    for fn in ("int mi_ppo_set_precision", "int mi_ppo_precision"):          # every prototype cites the reference op, as its neighbours do
        i = text.index(fn)
        assert "ppo.py:42-66,112-147,218-229" in text[text.rfind("/*", 0, i):i], fn
    # a null engine is refused before anything touches a device
    assert L.cdll.mi_ppo_set_precision(None, milib.MI_BF16X3) == -4
    assert L.cdll.mi_ppo_precision(None) == -4
    # the descriptor and the workspace are those of the fp32 engine
    d = milib.MiPpoDesc(2048, 67, 2, 500, 300, 0.2, 1.0, 0.01)
    assert L.mi_ppo_workspace_bytes(__import__("ctypes").byref(d)) > 0


SPLIT = [r"_ZN2mi13ppo_l1_kernelILb1EE", r"_ZN2mi13ppo_l2_kernelILb1EE", r"_ZN2mi14ppo_dh1_kernelILb1EE",
         r"_ZN2mi16ppo_wgrad_kernelILb1ELb1EE", r"_ZN2mi16ppo_wgrad_kernelILb0ELb1EE"]
EXACT = [r"_ZN2mi13ppo_l1_kernelILb0EE", r"_ZN2mi13ppo_l2_kernelILb0EE", r"_ZN2mi14ppo_dh1_kernelILb0EE",
         r"_ZN2mi16ppo_wgrad_kernelILb1ELb0EE", r"_ZN2mi16ppo_wgrad_kernelILb0ELb0EE"]


@pytest.fixture(scope="module")
def fused_listing():
    path = os.path.join(tempfile.mkdtemp(), "ppo_fused.s")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-S",
                    "--cuda-device-only", os.path.join(ROOT, "carla-ppo_amd", "csrc", "ppo_fused.hip"), "-o", path], check=True, capture_output=True)
    return open(path).read()


def _kernel(text, prefix):
    m = re.search(r"^(" + prefix + r"[A-Za-z0-9_]*):", text, re.M)
    assert m, prefix
    name = m.group(1)
    body = text[m.start():text.index("s_endpgm", m.start())]
    scratch = re.search(r"\.name:\s+" + re.escape(name) + r"\s*\n\s+\.private_segment_fixed_size:\s+(\d+)", text)
    assert scratch, name
    return name, body, int(scratch.group(1))


def test_split_instantiations_run_on_the_bf16_matrix_pipe(fused_listing):
    """The split-bf16 forms of the four GEMM kernels issue v_mfma_f32_32x32x16_bf16, no exact-fp32 MFMA at all (the bias rows included), and spill nothing;
    the fp32 forms still use the exact-fp32 MFMA only."""
    for prefix in SPLIT:
        name, body, scratch = _kernel(fused_listing, prefix)
        assert "v_mfma_f32_32x32x16_bf16" in body, name
        assert "v_mfma_f32_32x32x2_f32" not in body, name
        assert scratch == 0, name
    for prefix in EXACT:
        name, body, scratch = _kernel(fused_listing, prefix)
        assert "v_mfma_f32_32x32x2_f32" in body and "v_mfma_f32_32x32x16_bf16" not in body, name
        assert scratch == 0, name
