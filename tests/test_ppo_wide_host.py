"""CPU-only tests of the wide-input setting of the PPO engine (mi_ppo_set_wide_inputs / PPO.set_wide_inputs): the case table of tests/ppo_wide_cases.py against its
own float64 reference, the restated range predicate and share arithmetic, the environment knob, the pinned signature of PPO.__init__, the C-ABI surface, and the
gfx950 code of the new layer-1 kernel (compiled here, no GPU needed)."""
import ctypes
import inspect
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import ppo_shape_cases as pc
import ppo_wide_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Box:
    low, high, shape = np.array([-1, 0], np.float32), np.array([1, 1], np.float32), (2,)


@pytest.mark.parametrize("name", list(wc.WIDE_CASES))
def test_reference_meets_the_conditions(name):
    """The float64 reference of every pinned case: a clipped fraction strictly between 0 and 1 (ppo_shape_cases.conditions_met asks 10 % .. 60 % with both sides
    present, no ratio at a clip edge, ratios inside [1 / 20, 20]), and no action mean within 1 % of its range of a bound."""
    c = wc.wide_case(name)
    din, A, hidden, M = wc.WIDE_CASES[name][:4]
    assert c.s.shape == (M, din) and c.a.shape == (M, A) and c.hidden == hidden
    assert pc.conditions_met(c.cond), c.cond
    assert 0 < c.cond["share"] < 1
    assert wc.saturation_margin(c) > wc.SATURATION_MARGIN, wc.saturation_margin(c)
    assert all(np.isfinite(g).all() and np.abs(g).max() > 0 for g in c.grads.values())
    assert np.isfinite(c.logp_old).all() and np.isfinite(c.logp).all()


def test_case_table_covers_what_the_issue_names():
    kin = {k: wc.kin_of(v[0]) for k, v in wc.SHAPES.items()}
    assert kin == {"W100": 104, "W131": 136, "W259": 264, "W515": 520, "W1024": 1024, "W1025": 1032}
    assert wc.SHAPES["W131"][0] % 8 == 3 and wc.SHAPES["W131"][2][0] % 32 != 0          # din % 8 = 3; H1 a partial tile
    assert wc.SHAPES["W259"][2] == (132, 320) and wc.SHAPES["W515"][2] == (500, 300) and wc.SHAPES["W1024"][1] == 8
    ms = {}
    for k in wc.WIDE_CASES:
        ms.setdefault(k.split("-")[0], []).append(wc.WIDE_CASES[k][3])
    for k in ("W100", "W259", "W1024"):
        assert ms[k] == [5, 33, 77]
    assert ms["W131"] == ms["W515"] == [5, 33, 77, 257] and wc.SLAB_CASES == ["W131-257", "W515-257"]


def test_range_predicate_agrees_with_the_table():
    """Mode 0 takes none of the wide cases, modes 1 and 2 take all but W1025; the narrow range is what tests/ppo_shape_cases.py says it is."""
    for name, (din, A, hidden) in wc.SHAPES.items():
        assert not wc.fused_in_mode(din, A, hidden, 0), name
        for mode in (1, 2):
            assert wc.fused_in_mode(din, A, hidden, mode) == (name != "W1025"), (name, mode)
    assert set(wc.FUSED_WIDE) == {k for k in wc.WIDE_CASES if k.split("-")[0] != "W1025"}
    for name, v in pc.ENGINE_CASES.items():
        assert wc.fused_in_mode(v[0], v[1], v[2], 0) == (name in pc.FUSED_CASES), name
        if name.startswith("C100"):
            assert wc.fused_in_mode(v[0], v[1], v[2], 1)                                  # kin = 104: inside the wide range
        if name.startswith("C67"):
            assert not wc.fused_in_mode(v[0], v[1], v[2], 1)                              # H2 = 324 stays outside
    assert wc.fused_in_mode(1024, 8, (64, 320), 1) and not wc.fused_in_mode(1024, 9, (64, 320), 1) and not wc.fused_in_mode(1024, 8, (64, 322), 1)


def test_share_arithmetic():
    assert wc.wave_shares(104, False) == [(0, 4), (4, 8), (8, 12), (12, 13)]              # W100: 13 k-steps deal 4 / 4 / 4 / 1
    s = wc.wave_shares(136, True)                                                         # W131, split mode: 9 k-blocks, wave 3 has none
    assert s[:3] == [(0, 3), (3, 6), (6, 9)] and s[3][0] >= s[3][1]
    assert [e - b for b, e in wc.wave_shares(264, False)] == [9, 9, 9, 6]                 # W259: 33 steps
    assert [e - b for b, e in wc.wave_shares(520, False)] == [17, 17, 17, 14]             # W515: 17 steps, one past the chunk of 16
    assert [e - b for b, e in wc.wave_shares(512, False)] == [16] * 4 and [e - b for b, e in wc.wave_shares(512, True)] == [8] * 4
    assert [e - b for b, e in wc.wave_shares(1024, False)] == [32] * 4
    for kin in range(104, 1025, 8):
        for split in (False, True):
            sh = wc.wave_shares(kin, split)
            steps = (kin + 15) // 16 if split else kin // 8
            covered = [k for b, e in sh for k in range(b, e)]
            assert covered == list(range(steps)), (kin, split)


def test_environment_knob_and_setter(tmp_path, monkeypatch):
    import ppo
    monkeypatch.delenv("MI355_PPO_WIDE_INPUTS", raising=False)
    assert ppo.PPO(np.array([131]), Box(), model_dir=str(tmp_path / "a")).wide_inputs is False
    for text, want in (("", False), ("0", False), ("1", True), (" 1 ", True)):
        monkeypatch.setenv("MI355_PPO_WIDE_INPUTS", text)
        assert ppo.PPO(np.array([131]), Box(), model_dir=str(tmp_path / "b")).wide_inputs is want, text
    for text in ("2", "true", "yes", "on", "-1", "1.0"):
        monkeypatch.setenv("MI355_PPO_WIDE_INPUTS", text)
        with pytest.raises(ValueError, match="MI355_PPO_WIDE_INPUTS"):
            ppo.PPO(np.array([131]), Box(), model_dir=str(tmp_path / "c"))
    monkeypatch.delenv("MI355_PPO_WIDE_INPUTS")
    m = ppo.PPO(np.array([131]), Box(), model_dir=str(tmp_path / "d"))
    m.set_wide_inputs()                                                                   # before init_session: remembered, no device touched
    assert m.wide_inputs is True
    m.set_wide_inputs(False)
    assert m.wide_inputs is False
    for bad in (1, 0, None, "1", 2):
        with pytest.raises(ValueError, match="set_wide_inputs"):
            m.set_wide_inputs(bad)
    assert list(inspect.signature(ppo.PPO.set_wide_inputs).parameters) == ["self", "on"]
    assert inspect.signature(ppo.PPO.set_wide_inputs).parameters["on"].default is True


def test_ppo_constructor_signature_is_unchanged():
    import ppo
    assert list(inspect.signature(ppo.PPO.__init__).parameters) == ["self", "input_shape", "action_space", "learning_rate", "lr_decay", "epsilon", "value_scale",
                                                                     "entropy_scale", "initial_std", "model_dir", "seed", "precision"]


def test_device_mode_values():
    from mi355.ppo_device import PpoDevice, wide_inputs_mode
    assert [wide_inputs_mode(x) for x in (0, 1, 2, False, True, np.int32(2))] == [0, 1, 2, 0, 1, 2]
    for bad in (3, -1, None, "1", 1.0):
        with pytest.raises(ValueError):
            wide_inputs_mode(bad)
    assert list(inspect.signature(PpoDevice.set_wide_inputs).parameters) == ["self", "mode"]
    assert inspect.signature(PpoDevice.__init__).parameters["wide_inputs"].default == 0


def test_entry_points_are_declared_exported_and_checked():
    from mi355 import lib as milib
    protos = milib.parse_header()
    assert protos["mi_ppo_set_wide_inputs"] == ("int", [("void*", "h"), ("int", "mode")])
    assert protos["mi_ppo_wide_inputs"] == ("int", [("void*", "h")])
    L = milib.get()
    assert hasattr(L.cdll, "mi_ppo_set_wide_inputs") and hasattr(L.cdll, "mi_ppo_wide_inputs")
    assert L.mi_abi_version() == 7
    assert L.cdll.mi_ppo_set_wide_inputs(None, 1) == -4 and L.cdll.mi_ppo_wide_inputs(None) == -4      # a null engine is refused before anything touches a device
    text = open(milib.HEADER).read()
    i = text.index("int mi_ppo_set_wide_inputs")
    comment = text[text.rfind("/*", 0, i):i]
    for word in ("1024", "320", "num_actions <= 8", "2^31", "checkpoint"):
        assert word in comment, word
    # the setting adds nothing to the descriptor or the workspace
    d = milib.MiPpoDesc(320, 515, 2, 500, 300, 0.2, 1.0, 0.01)
    assert L.mi_ppo_workspace_bytes(ctypes.byref(d)) > 0 and L.mi_ppo_desc_size() == ctypes.sizeof(milib.MiPpoDesc)


def test_error_texts_name_the_setting():
    """rollout.py's three refusals name the setting.  (ppo.py's two texts are pinned word for word by tests/test_ppo_step_dispatch_host.py and stay as they are.)"""
    text = open(os.path.join(ROOT, "carla-ppo_amd", "rollout.py")).read()
    assert text.count("outside their range (more than 96 inputs: PPO.set_wide_inputs())") == 3


@pytest.fixture(scope="module")
def fused_listing():
    path = os.path.join(tempfile.mkdtemp(), "ppo_fused.s")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-S",
                    "--cuda-device-only", os.path.join(ROOT, "carla-ppo_amd", "csrc", "ppo_fused.hip"), "-o", path], check=True, capture_output=True)
    return open(path).read()


@pytest.mark.parametrize("prefix,split", [(r"_ZN2mi18ppo_l1_wide_kernelILb0EE", False), (r"_ZN2mi18ppo_l1_wide_kernelILb1EE", True)])
def test_wide_layer1_kernel_code(fused_listing, prefix, split):
    """The K-split layer-1 kernel: the MFMA of its precision only, one barrier, 12 KB of LDS for the three partial tiles, no private segment, no atomics."""
    m = re.search(r"^(" + prefix + r"[A-Za-z0-9_]*):", fused_listing, re.M)
    assert m, prefix
    name = m.group(1)
    body = fused_listing[m.start():fused_listing.index("s_endpgm", m.start())]
    want, other = ("v_mfma_f32_32x32x16_bf16", "v_mfma_f32_32x32x2_f32") if split else ("v_mfma_f32_32x32x2_f32", "v_mfma_f32_32x32x16_bf16")
    assert want in body and other not in body, name
    assert body.count("s_barrier") == 1, name
    meta = re.search(r"\.name:\s+" + re.escape(name) + r"\s*\n\s+\.private_segment_fixed_size:\s+(\d+)", fused_listing)
    assert meta, name
    lds = re.findall(r"\.group_segment_fixed_size:\s+(\d+)", fused_listing[:meta.start()])[-1]      # (the metadata lists a kernel's keys in alphabetical order)
    assert int(lds) == 3 * 16 * 64 * 4 and int(meta.group(1)) == 0, (name, lds, meta.group(1))
