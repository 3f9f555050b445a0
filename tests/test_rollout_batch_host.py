"""CPU-only tests of the batched rollout step (mi_rollout_step_batch / rollout.BatchedRolloutStep): the C-ABI surface, the Python signature, and the gfx950 code
of rollout.hip (compiled here, no GPU needed): the batched kernels exist, run on the exact-fp32 MFMA, spill nothing and store nothing through the scalar unit; the
B = 1 kernels mi_rollout_step launches are still there."""
import inspect
import re

import pytest

from rollout_host_common import SCALAR_WRITES, _kernel, _listing


def test_batch_entry_points_are_declared_exported_and_checked():
    from mi355 import lib as milib
    protos = milib.parse_header()
    assert protos["mi_rollout_batch_workspace_bytes"] == ("long long", [("void*", "vae_h"), ("void*", "ppo_h"), ("int", "n_envs")])
    assert protos["mi_rollout_step_batch"] == ("int", [("void*", "vae_h"), ("void*", "ppo_h"), ("void*", "stream"), ("const unsigned char*", "frames_u8"),
                                                       ("const float*", "measurements"), ("int", "n_meas"), ("const float*", "noise"), ("int", "greedy"), ("int", "n"),
                                                       ("void*", "scratch"), ("long long", "scratch_bytes"), ("float*", "out")])
    L = milib.get()
    assert hasattr(L.cdll, "mi_rollout_step_batch") and hasattr(L.cdll, "mi_rollout_batch_workspace_bytes")
    assert L.mi_abi_version() == 7
    text = open(milib.HEADER).read()
    for fn in ("long long mi_rollout_batch_workspace_bytes", "int mi_rollout_step_batch"):      # every prototype cites the reference lines it replaces
        i = text.index(fn)
        comment = text[text.rfind("/*", 0, i):i]
        assert "vae_common.py:45-61" in comment and "ppo.py:231-251" in comment, fn
    m = re.search(r"#define\s+MI_ROLLOUT_MAX_ENVS\s+(\d+)", text)                               # the supported maximum of n is stated, at least 64
    assert m and int(m.group(1)) >= 64
    import rollout
    assert rollout.MAX_ENVS == int(m.group(1))
    # null handles are refused before anything touches a device
    assert L.cdll.mi_rollout_batch_workspace_bytes(None, None, 4) == -4
    assert L.cdll.mi_rollout_step_batch(None, None, None, None, None, 3, None, 1, 4, None, 0, None) == -4
    assert b"null handle" in L.cdll.mi_last_error()


def test_batched_rollout_step_signature():
    import rollout
    assert list(inspect.signature(rollout.BatchedRolloutStep.__init__).parameters) == ["self", "vae", "ppo", "num_envs", "seed", "io"]
    assert list(inspect.signature(rollout.BatchedRolloutStep.__call__).parameters) == ["self", "frames_u8", "measurements", "greedy", "noise"]
    assert list(inspect.signature(rollout.RolloutStep.__init__).parameters) == ["self", "vae", "ppo", "seed", "io"]


BATCHED = [r"_ZN2mi26rollout_conv1_batch_kernelILi12EE", r"_ZN2mi26rollout_conv1_batch_kernelILi0EE"] + \
          [r"_ZN2mi25rollout_conv_batch_kernelILi%dEE" % m for m in range(5)]
BATCHED_HEADS = [r"_ZN2mi25rollout_head_batch_kernelILi2EE", r"_ZN2mi25rollout_head_batch_kernelILi8EE"]
SINGLE = [r"_ZN2mi20rollout_conv1_kernelILi12EE", r"_ZN2mi20rollout_conv1_kernelILi0EE"] + [r"_ZN2mi19rollout_conv_kernelILi%dEE" % m for m in range(5)]
SINGLE_HEADS = [r"_ZN2mi19rollout_head_kernelILi2EE", r"_ZN2mi19rollout_head_kernelILi8EE"]
@pytest.fixture(scope="module")
def rollout_listing():
    return _listing("rollout")


def test_batched_kernels_are_exact_fp32_mfma_and_spill_free(rollout_listing):
    for prefix in BATCHED:
        name, body, scratch, _ = _kernel(rollout_listing, prefix)
        assert "v_mfma_f32_32x32x2_f32" in body, name
        assert "bf16" not in body, name
        assert scratch == 0, name
        assert not SCALAR_WRITES.search(body), name
    for prefix in BATCHED_HEADS:
        name, body, scratch, _ = _kernel(rollout_listing, prefix)
        assert scratch == 0 and "v_mfma" not in body, name
        assert not SCALAR_WRITES.search(body), name
    assert not SCALAR_WRITES.search(rollout_listing)


def test_single_frame_kernels_are_still_there(rollout_listing):
    for prefix in SINGLE:
        name, body, scratch, _ = _kernel(rollout_listing, prefix)
        assert "v_mfma_f32_32x32x2_f32" in body and "bf16" not in body, name
        assert scratch == 0, name
    for prefix in SINGLE_HEADS:
        name, body, scratch, _ = _kernel(rollout_listing, prefix)
        assert scratch == 0, name
