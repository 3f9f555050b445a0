"""CPU-only tests of the device-resident rollout buffer (mi_rollout_step_batch_rec / mi_rollout_finish / rollout.RolloutBuffer): the C-ABI surface, the Python
signatures, the row book-keeping (rollout.RolloutRows, numpy only) on a scripted ragged collection and every misuse, and the gfx950 code of rollout.hip and
ppo_ops.hip (compiled here, no GPU needed): the recording heads and the finish kernel exist, spill nothing and store nothing through the scalar unit; the kernels
the existing steps launch are still found by their names."""
import inspect
import os
import re

import numpy as np
import pytest

from rollout_host_common import ROOT, SCALAR_WRITES, _kernel, _listing


def test_entry_points_are_declared_exported_and_checked():
    from mi355 import lib as milib
    protos = milib.parse_header()
    batch = [("void*", "vae_h"), ("void*", "ppo_h"), ("void*", "stream"), ("const unsigned char*", "frames_u8"), ("const float*", "measurements"), ("int", "n_meas"),
             ("const float*", "noise"), ("int", "greedy"), ("int", "n"), ("void*", "scratch"), ("long long", "scratch_bytes"), ("float*", "out")]
    assert protos["mi_rollout_step_batch"] == ("int", batch)
    assert protos["mi_rollout_step_batch_rec"] == ("int", batch + [("const int*", "table_rows"), ("long long", "n_table_rows"), ("float*", "tab_states"),
                                                                  ("float*", "tab_actions"), ("float*", "tab_values")])
    assert protos["mi_rollout_finish"] == ("int", [("void*", "stream"), ("const float*", "tab_values"), ("const double*", "rewards"), ("const double*", "terminals"),
                                                   ("const int*", "len"), ("int", "num_envs"), ("int", "T"), ("double", "gamma"), ("double", "lam"),
                                                   ("float*", "tab_returns"), ("float*", "tab_advantages"), ("double*", "adv_raw"), ("double*", "returns"),
                                                   ("double*", "adv_norm")])
    L = milib.get()
    assert hasattr(L.cdll, "mi_rollout_step_batch_rec") and hasattr(L.cdll, "mi_rollout_finish")
    assert L.mi_abi_version() == 7
    text = open(milib.HEADER).read()
    for fn, cites in (("int mi_rollout_step_batch_rec", ("vae_common.py:45-61", "ppo.py:231-251", "train.py:172")),
                      ("int mi_rollout_finish", ("utils.py:45-50", "train.py:175-177"))):
        i = text.index(fn)
        comment = text[text.rfind("/*", 0, i):i]
        for c in cites:
            assert c in comment, (fn, c)
    m = re.search(r"#define\s+MI_ROLLOUT_MAX_HORIZON\s+(\d+)", text)
    assert m and int(m.group(1)) >= 1024
    import rollout
    assert rollout.MAX_HORIZON == int(m.group(1))
    limit = int(m.group(1))
    # null handles are refused before anything touches a device
    assert L.cdll.mi_rollout_step_batch_rec(None, None, None, None, None, 3, None, 1, 4, None, 0, None, None, 8, None, None, None) == -4
    assert b"null handle" in L.cdll.mi_last_error()
    # the finish call: NULL tables, empty shapes and a horizon over the limit are argument errors with a message (the pointers are never dereferenced on the host)
    import ctypes
    buf = (ctypes.c_double * 16)()
    p = ctypes.addressof(buf)
    fin = L.cdll.mi_rollout_finish
    assert fin(None, None, p, p, p, 2, 4, 0.99, 0.95, p, p, None, None, None) == -1 and b"missing buffers" in L.cdll.mi_last_error()
    assert fin(None, p, p, p, p, 2, 4, 0.99, 0.95, None, p, None, None, None) == -1 and b"missing buffers" in L.cdll.mi_last_error()
    assert fin(None, p, p, p, p, 2, 4, 0.99, 0.95, p, None, None, None, None) == -1
    assert fin(None, p, None, p, p, 2, 4, 0.99, 0.95, p, p, None, None, None) == -1
    assert fin(None, p, p, p, None, 2, 4, 0.99, 0.95, p, p, None, None, None) == -1
    assert fin(None, p, p, p, p, 2, 0, 0.99, 0.95, p, p, None, None, None) == -1 and b"empty" in L.cdll.mi_last_error()
    assert fin(None, p, p, p, p, 0, 4, 0.99, 0.95, p, p, None, None, None) == -1 and b"empty" in L.cdll.mi_last_error()
    assert fin(None, p, p, p, p, 2, limit + 1, 0.99, 0.95, p, p, None, None, None) == -1 and b"MI_ROLLOUT_MAX_HORIZON" in L.cdll.mi_last_error()


def test_rollout_buffer_signatures():
    import rollout
    sig = lambda f: list(inspect.signature(f).parameters)      # noqa: E731
    B = rollout.RolloutBuffer
    assert sig(B.__init__) == ["self", "vae", "ppo", "num_envs", "horizon", "seed", "io"]
    assert sig(B.reset) == ["self"]
    assert sig(B.step) == ["self", "frames_u8", "measurements", "env_ids", "greedy", "noise"]
    assert sig(B.outcome) == ["self", "rewards", "dones", "env_ids"]
    assert sig(B.bootstrap) == ["self", "frames_u8", "measurements", "env_ids"]
    assert sig(B.update) == ["self", "gamma", "lam", "num_epochs", "batch_size", "stage_times"]
    d = {k: v.default for k, v in inspect.signature(B.update).parameters.items() if k != "self"}
    assert d == dict(gamma=0.99, lam=0.95, num_epochs=3, batch_size=32, stage_times=None)
    d = {k: v.default for k, v in inspect.signature(B.step).parameters.items()}
    assert d["env_ids"] is None and d["greedy"] is False and d["noise"] is None


def test_row_bookkeeping_of_a_scripted_ragged_collection():
    """E = 5, T = 4: environment 1 reports done at its step 1, environment 3 at its step 3, environments 0 and 2 reach the horizon, environment 4 is never stepped."""
    from rollout import RolloutRows
    E, T = 5, 4
    rows = RolloutRows(E, T)
    done_at = {1: 1, 3: 3}
    live = np.array([0, 1, 2, 3])
    calls, t = [], 0
    while len(live):
        got = rows.step_rows(live, len(live))
        assert got.dtype == np.int32
        calls.append(got.tolist())
        dones = np.array([done_at.get(int(e)) == t + 1 for e in live])
        rows.outcome(10.0 * live + t, dones, live)
        t += 1
        live = live[~dones & (rows.lengths[live] < T)]
    assert calls == [[0, 5, 10, 15], [1, 11, 16], [2, 12, 17], [3, 13]]             # e (T + 1) + slot
    assert rows.lengths.tolist() == [4, 1, 4, 3, 0]
    assert rows.stepped().tolist() == [0, 1, 2, 3]
    with pytest.raises(ValueError, match="open rows"):
        rows.check_update()
    assert rows.bootstrap_rows(np.array([3, 1]), 2).tolist() == [18, 6]             # slot len[e], in the call's order
    assert rows.bootstrap_rows(None, 1).tolist() == [4]                             # None = 0 .. n-1
    assert rows.bootstrap_rows([2], 1).tolist() == [14]
    rows.check_update()
    assert rows.valid_rows().dtype == np.int32
    assert rows.valid_rows().tolist() == [0, 1, 2, 3, 5, 10, 11, 12, 13, 15, 16, 17]
    assert rows.rewards[3, :3].tolist() == [30.0, 31.0, 32.0] and rows.rewards[1, 0] == 10.0
    assert rows.dones.sum() == 2 and rows.dones[1, 0] == 1 and rows.dones[3, 2] == 1
    rows.reset()
    assert rows.lengths.tolist() == [0] * 5 and not rows.closed.any() and not rows.awaiting.any() and rows.valid_rows().size == 0
    assert rows.step_rows(None, 5).tolist() == [0, 5, 10, 15, 20]


def test_every_misuse_of_the_rows_raises_and_changes_nothing():
    import rollout
    from rollout import RolloutRows
    for bad in ((0, 4), (rollout.MAX_ENVS + 1, 4), (4, 0), (4, rollout.MAX_HORIZON + 1)):
        with pytest.raises(ValueError):
            RolloutRows(*bad)
    RolloutRows(rollout.MAX_ENVS, rollout.MAX_HORIZON)
    rows = RolloutRows(3, 2)
    with pytest.raises(ValueError, match="no samples"):
        rows.check_update()
    for ids, n in (([0, 0], 2), ([0, 3], 2), ([-1], 1), ([0, 1], 1), ([0.0, 1.0], 2), ([[0, 1]], 2), (None, 4), (None, 0)):
        with pytest.raises(ValueError):
            rows.step_rows(ids, n)
    assert not rows.awaiting.any()
    with pytest.raises(ValueError, match="without a recorded step"):
        rows.outcome([1.0], [False], [0])
    with pytest.raises(ValueError, match="empty row"):
        rows.bootstrap_rows([0], 1)
    rows.step_rows([0, 1], 2)
    with pytest.raises(ValueError, match="no outcome yet"):
        rows.step_rows([1, 2], 2)                                                   # one offender refuses the whole call ...
    assert rows.awaiting.tolist() == [True, True, False]                            # ... and environment 2 was not marked
    with pytest.raises(ValueError, match="no outcome yet"):
        rows.bootstrap_rows([0], 1)
    with pytest.raises(ValueError, match="open rows"):
        rows.check_update()                                                         # a recorded step without its outcome is an open row
    with pytest.raises(ValueError):
        rows.outcome([1.0, 2.0], [False], [0, 1])                                   # shapes
    with pytest.raises(ValueError, match="without a recorded step"):
        rows.outcome([1.0, 2.0, 3.0], [False] * 3, None)                            # environment 2 has no step
    assert rows.lengths.tolist() == [0, 0, 0]
    rows.outcome([1.0, 2.0], [False, True], [0, 1])
    assert rows.lengths.tolist() == [1, 1, 0]
    with pytest.raises(ValueError, match="full row"):
        rows.step_rows([1], 1)                                                      # done was reported
    rows.step_rows([0], 1)
    rows.outcome([3.0], [False], [0])
    with pytest.raises(ValueError, match="full row"):
        rows.step_rows([0], 1)                                                      # the horizon is reached
    with pytest.raises(ValueError, match="open rows"):
        rows.check_update()
    rows.bootstrap_rows([0, 1], 2)
    with pytest.raises(ValueError, match="closed row"):
        rows.step_rows([0], 1)
    with pytest.raises(ValueError, match="closed row"):
        rows.bootstrap_rows([1], 1)
    rows.check_update()                                                             # environment 2 was never stepped: an empty row is not an open one
    assert rows.valid_rows().tolist() == [0, 1, 3]


HEADS_REC = [r"_ZN2mi23rollout_head_rec_kernelILi2EE", r"_ZN2mi23rollout_head_rec_kernelILi8EE"]
FINISH = r"_ZN2mi21rollout_finish_kernelE"
EXISTING = [r"_ZN2mi19rollout_head_kernelILi2EE", r"_ZN2mi19rollout_head_kernelILi8EE", r"_ZN2mi25rollout_head_batch_kernelILi2EE", r"_ZN2mi25rollout_head_batch_kernelILi8EE",
            r"_ZN2mi20rollout_conv1_kernelILi12EE", r"_ZN2mi20rollout_conv1_kernelILi0EE", r"_ZN2mi26rollout_conv1_batch_kernelILi12EE", r"_ZN2mi26rollout_conv1_batch_kernelILi0EE"] + \
           [r"_ZN2mi19rollout_conv_kernelILi%dEE" % m for m in range(5)] + [r"_ZN2mi25rollout_conv_batch_kernelILi%dEE" % m for m in range(5)]

def test_recording_heads_and_existing_rollout_kernels_in_the_gfx950_listing():
    text = _listing("rollout")
    for prefix in HEADS_REC:
        name, body, scratch, _ = _kernel(text, prefix)
        assert scratch == 0 and "v_mfma" not in body, name
        assert not SCALAR_WRITES.search(body), name
        assert "global_store_dword" in body, name                                  # the table rows leave through the vector unit
    for prefix in EXISTING:
        _kernel(text, prefix)
    assert not SCALAR_WRITES.search(text)


def test_finish_kernel_in_the_gfx950_listing():
    text = _listing("ppo_ops")
    name, body, scratch, _ = _kernel(text, FINISH)
    assert scratch == 0, name
    assert not SCALAR_WRITES.search(body), name
    assert "v_add_f64" in body and "v_mul_f64" in body and "v_cvt_f32_f64" in body, name
    assert not SCALAR_WRITES.search(text)


def test_new_sources_do_not_spell_scalar_unit_writes():
    for rel in ("carla-ppo_amd/csrc/rollout.hip", "carla-ppo_amd/csrc/ppo_ops.hip", "carla-ppo_amd/csrc/vae_engine.hip", "carla-ppo_amd/rollout.py",
                "tests/test_rollout_buffer_host.py", "tests/test_m_rollout_buffer_gpu.py", "tests/rollout_host_common.py", "tests/rollout_gpu_common.py", "tools/rollout_latency.py", "tools/rollout_buffer_bench.py"):
        path = os.path.join(ROOT, rel)
        if os.path.exists(path):
            assert not SCALAR_WRITES.search(open(path).read().lower()), rel
