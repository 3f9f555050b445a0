"""CPU-only tests of continuous collection (mi_rollout_finish_segments / rollout.SegmentedRows / rollout.ContinuousRolloutBuffer): the C-ABI surface and every
host-checkable argument error, the segment book-keeping (numpy only) on a scripted collection and every misuse, the parent classes left as they were, and the gfx950
code of ppo_ops.hip (compiled here, no GPU needed): the segment kernels exist, spill nothing and store nothing through the scalar unit, and the dense finish kernel
is still found by its name."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from rollout_host_common import ROOT, SCALAR_WRITES, _kernel, _listing


def test_entry_point_is_declared_exported_and_checked():
    from mi355 import lib as milib
    protos = milib.parse_header()
    assert protos["mi_rollout_finish_segments"] == ("int", [("void*", "stream"), ("const float*", "tab_values"), ("const double*", "rewards"), ("const double*", "terminals"),
                                                            ("const int*", "seg_row"), ("const int*", "seg_len"), ("int", "n_seg"), ("int", "num_envs"), ("int", "T"),
                                                            ("double", "gamma"), ("double", "lam"), ("int", "normalize"), ("double*", "scratch"), ("float*", "tab_returns"),
                                                            ("float*", "tab_advantages"), ("double*", "adv_raw"), ("double*", "returns"), ("double*", "adv_norm")])
    assert protos["mi_rollout_finish_segments_scratch_doubles"] == ("long long", [("int", "n_seg")])
    # everything mi_rollout_finish takes except len, in its order
    dense = [a for a in protos["mi_rollout_finish"][1] if a[1] != "len"]
    mine = [a for a in protos["mi_rollout_finish_segments"][1] if a[1] not in ("seg_row", "seg_len", "n_seg", "normalize", "scratch")]
    assert mine == dense
    L = milib.get()
    assert hasattr(L.cdll, "mi_rollout_finish_segments") and hasattr(L.cdll, "mi_rollout_finish_segments_scratch_doubles")
    assert L.mi_abi_version() == 7
    text = open(milib.HEADER).read()
    i = text.index("int mi_rollout_finish_segments")
    comment = text[text.rfind("/*", 0, i):i]
    for c in ("utils.py:45-50", "train.py:175-177", "adv_raw", "mi_rollout_finish_segments_scratch_doubles"):
        assert c in comment, c
    limit = int(re.search(r"#define\s+MI_ROLLOUT_MAX_HORIZON\s+(\d+)", text).group(1))
    assert L.mi_rollout_finish_segments_scratch_doubles(1) == 4 and L.mi_rollout_finish_segments_scratch_doubles(1000) == 2002
    assert L.mi_rollout_finish_segments_scratch_doubles(0) < 0
    # every host-checkable argument error returns MI_ERR_ARG with a message before any launch (the pointers are never dereferenced on the host)
    buf = (ctypes.c_double * 16)()
    p = ctypes.addressof(buf)
    fin, err = L.cdll.mi_rollout_finish_segments, L.cdll.mi_last_error
    names = [a[1] for a in protos["mi_rollout_finish_segments"][1]]
    good = dict(stream=None, tab_values=p, rewards=p, terminals=p, seg_row=p, seg_len=p, n_seg=3, num_envs=2, T=4, gamma=0.99, lam=0.95, normalize=0, scratch=None,
                tab_returns=p, tab_advantages=p, adv_raw=None, returns=None, adv_norm=None)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return fin(*[a[n] for n in names])
    for missing in ("tab_values", "rewards", "terminals", "seg_row", "seg_len", "tab_returns", "tab_advantages"):
        assert call(**{missing: None}) == -1 and b"missing buffers" in err(), missing
    for kw in (dict(n_seg=0), dict(n_seg=-1), dict(num_envs=0), dict(T=0)):
        assert call(**kw) == -1 and b"empty" in err(), kw
    assert call(T=limit + 1) == -1 and b"MI_ROLLOUT_MAX_HORIZON" in err()
    for bad in (2, -1):
        assert call(normalize=bad, scratch=p, adv_raw=p) == -1 and b"normalize" in err(), bad
    assert call(normalize=1, scratch=None, adv_raw=p) == -1 and b"scratch" in err()
    assert call(normalize=1, scratch=p, adv_raw=None) == -1 and b"adv_raw" in err()


def script(rows, done_at, stop_at=None, reward=lambda e, t: 10.0 * e + t):
    """Steps every lane that is not full (and not stopped: stop_at[e] = number of steps lane e takes) until none is left; lane e reports done at its steps done_at[e]
    (1-based).  Returns the table rows of every step_rows call."""
    E, T = rows.num_envs, rows.horizon
    stop_at = stop_at or {}
    calls = []
    while True:
        live = np.array([e for e in range(E) if rows.lengths[e] < min(T, stop_at.get(e, T))], np.int64)
        if not len(live):
            return calls
        want = [int(e * (T + 1) + rows.lengths[e]) for e in live]
        got = rows.step_rows(live, len(live))
        assert got.dtype == np.int32 and got.tolist() == want                       # e (T + 1) + lengths[e]
        calls.append(got.tolist())
        t = rows.lengths[live].copy()
        rows.outcome([reward(int(e), int(s)) for e, s in zip(live, t)], np.array([int(s) + 1 in done_at.get(int(e), ()) for e, s in zip(live, t)]), live)


def test_segment_bookkeeping_of_a_scripted_collection():
    """E = 4, T = 6: lane 0 has no done, lane 1 dones at its slots 2 and 5 (slot 5 is its last step), lane 2 a done at step 6 (the lane's last slot), lane 3 is stopped
    after 3 steps without one.  (A lane whose mid-lane done is followed by an open tail is the second script below.)"""
    from rollout import SegmentedRows
    E, T = 4, 6
    rows = SegmentedRows(E, T)
    calls = script(rows, {1: (3, 6), 2: (6,)}, {3: 3})
    assert calls[:3] == [[0, 7, 14, 21], [1, 8, 15, 22], [2, 9, 16, 23]] and calls[3:] == [[3, 10, 17], [4, 11, 18], [5, 12, 19]]
    assert rows.lengths.tolist() == [6, 6, 6, 3]
    assert rows.ended.tolist() == [True, True, True, False] and not rows.awaiting.any() and not rows.closed.any()
    segs = rows.segments()
    assert segs.dtype == np.int32 and segs.tolist() == [[0, 0, 6], [1, 0, 3], [1, 3, 3], [2, 0, 6], [3, 0, 3]]
    covered = np.concatenate([e * (T + 1) + s + np.arange(n) for e, s, n in segs])
    assert covered.tolist() == rows.valid_rows().tolist()                            # every recorded step is in exactly one segment
    assert rows.valid_rows().dtype == np.int32
    assert rows.valid_rows().tolist() == list(range(0, 6)) + list(range(7, 13)) + list(range(14, 20)) + [21, 22, 23]
    assert rows.needs_bootstrap().tolist() == [0, 3]
    with pytest.raises(ValueError, match="bootstrap them first"):
        rows.check_update()
    assert rows.bootstrap_rows([3], 1).tolist() == [24]                             # slot lengths[e]
    assert rows.needs_bootstrap().tolist() == [0]
    with pytest.raises(ValueError, match=r"environments \[0\]"):
        rows.check_update()
    assert rows.bootstrap_rows([0], 1).tolist() == [6]
    rows.check_update()                                                              # lanes 1 and 2 end in a done: they need no bootstrap ...
    assert rows.closed.tolist() == [True, False, False, True]
    assert rows.bootstrap_rows([2, 1], 2).tolist() == [20, 13]                      # ... and take one all the same (the value is never read)
    rows.check_update()
    assert rows.segments().tolist() == segs.tolist()
    assert rows.rewards[1].tolist() == [10.0, 11.0, 12.0, 13.0, 14.0, 15.0] and rows.dones[1].tolist() == [0, 0, 1, 0, 0, 1] and rows.dones[2].tolist() == [0, 0, 0, 0, 0, 1]
    rows.reset()
    assert rows.lengths.tolist() == [0] * 4 and rows.segments().shape == (0, 3) and rows.needs_bootstrap().size == 0 and rows.valid_rows().size == 0
    assert rows.step_rows(None, 4).tolist() == [0, 7, 14, 21]
    # a lane whose only step is a done, and a done in the middle followed by one open step
    rows = SegmentedRows(2, 4)
    script(rows, {0: (1,), 1: (2,)}, {0: 1, 1: 3})
    assert rows.segments().tolist() == [[0, 0, 1], [1, 0, 2], [1, 2, 1]] and rows.needs_bootstrap().tolist() == [1]


def test_every_misuse_of_the_segmented_rows_raises_and_changes_nothing():
    """test_rollout_buffer_host.py's list on SegmentedRows; stepping after a done is now allowed."""
    import rollout
    from rollout import SegmentedRows
    for bad in ((0, 4), (rollout.MAX_ENVS + 1, 4), (4, 0), (4, rollout.MAX_HORIZON + 1)):
        with pytest.raises(ValueError):
            SegmentedRows(*bad)
    SegmentedRows(rollout.MAX_ENVS, rollout.MAX_HORIZON)
    rows = SegmentedRows(3, 3)
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
    assert rows.needs_bootstrap().size == 0                                         # (awaiting lanes are not named: they cannot take a bootstrap yet)
    with pytest.raises(ValueError):
        rows.outcome([1.0, 2.0], [False], [0, 1])                                   # shapes
    with pytest.raises(ValueError, match="without a recorded step"):
        rows.outcome([1.0, 2.0, 3.0], [False] * 3, None)                            # environment 2 has no step
    assert rows.lengths.tolist() == [0, 0, 0] and rows.awaiting.tolist() == [True, True, False]
    rows.outcome([1.0, 2.0], [False, True], [0, 1])
    assert rows.lengths.tolist() == [1, 1, 0] and not rows.ended.any()
    assert rows.step_rows([1], 1).tolist() == [5]                                   # done was reported: the lane goes on at slot 1
    rows.outcome([4.0], [False], [1])
    with pytest.raises(ValueError, match="open rows"):
        rows.check_update()                                                         # both lanes end without a done
    rows.step_rows([0, 1], 2)
    rows.outcome([3.0, 5.0], [False, True], [0, 1])
    rows.step_rows([0], 1)
    rows.outcome([3.5], [False], [0])
    assert rows.lengths.tolist() == [3, 3, 0] and rows.ended.tolist() == [True, True, False]
    for e in (0, 1):
        with pytest.raises(ValueError, match="full row"):
            rows.step_rows([e], 1)                                                  # the horizon is reached, with and without a done
    assert rows.needs_bootstrap().tolist() == [0]
    with pytest.raises(ValueError, match="open rows"):
        rows.check_update()
    before = (rows.lengths.copy(), rows.state.copy(), rows.rewards.copy(), rows.dones.copy())
    with pytest.raises(ValueError, match="empty row"):
        rows.bootstrap_rows([0, 2], 2)                                              # one empty lane refuses the whole call
    for x, y in zip(before, (rows.lengths, rows.state, rows.rewards, rows.dones)):
        assert np.array_equal(x, y)
    assert rows.bootstrap_rows([0], 1).tolist() == [3]
    with pytest.raises(ValueError, match="closed row"):
        rows.step_rows([0], 1)
    with pytest.raises(ValueError, match="closed row"):
        rows.bootstrap_rows([0], 1)
    rows.check_update()                                                             # lane 1 ends in a done, lane 2 was never stepped
    assert rows.valid_rows().tolist() == [0, 1, 2, 4, 5, 6]
    assert rows.segments().tolist() == [[0, 0, 3], [1, 0, 1], [1, 1, 2]]


def test_parent_classes_are_untouched_and_the_new_signatures():
    import rollout
    from rollout import ContinuousRolloutBuffer, RolloutBuffer, RolloutRows, SegmentedRows
    rows = RolloutRows(2, 4)
    rows.step_rows(None, 2)
    rows.outcome([1.0, 2.0], [True, False])
    assert rows.ended.tolist() == [True, False]                                      # a done still ends a RolloutRows row
    with pytest.raises(ValueError, match="full row"):
        rows.step_rows([0], 1)
    assert not hasattr(rows, "segments") and not hasattr(rows, "needs_bootstrap")
    assert issubclass(SegmentedRows, RolloutRows) and issubclass(ContinuousRolloutBuffer, RolloutBuffer) and ContinuousRolloutBuffer is not RolloutBuffer
    sig = lambda f: list(inspect.signature(f).parameters)      # noqa: E731
    defaults = lambda f: {k: v.default for k, v in inspect.signature(f).parameters.items() if k != "self"}      # noqa: E731
    C, B = ContinuousRolloutBuffer, RolloutBuffer
    assert sig(C.__init__) == ["self", "vae", "ppo", "num_envs", "horizon", "seed", "io"]
    assert defaults(C.__init__)["seed"] is None and defaults(C.__init__)["io"] is None
    assert sig(C.reset) == ["self"]
    assert sig(C.step) == ["self", "frames_u8", "measurements", "env_ids", "greedy", "noise"]
    assert sig(C.outcome) == ["self", "rewards", "dones", "env_ids"]
    assert sig(C.bootstrap) == ["self", "frames_u8", "measurements", "env_ids"] and defaults(C.bootstrap)["env_ids"] is None
    assert sig(C.update) == ["self", "gamma", "lam", "num_epochs", "batch_size", "normalize", "stage_times"]
    assert defaults(C.update) == dict(gamma=0.99, lam=0.95, num_epochs=3, batch_size=32, normalize="segment", stage_times=None)
    # the pinned ones
    assert sig(B.__init__) == ["self", "vae", "ppo", "num_envs", "horizon", "seed", "io"]
    assert sig(B.step) == ["self", "frames_u8", "measurements", "env_ids", "greedy", "noise"]
    assert sig(B.outcome) == ["self", "rewards", "dones", "env_ids"]
    assert sig(B.bootstrap) == ["self", "frames_u8", "measurements", "env_ids"]
    assert sig(B.update) == ["self", "gamma", "lam", "num_epochs", "batch_size", "stage_times"]
    assert defaults(B.update) == dict(gamma=0.99, lam=0.95, num_epochs=3, batch_size=32, stage_times=None)
    for text in (rollout.__doc__, open(os.path.join(ROOT, "INTEGRATION.md")).read()):
        assert "ContinuousRolloutBuffer(vae, ppo, num_envs=8, horizon=128)" in text and "needs_bootstrap()" in text


SEGMENT_KERNELS = [r"_ZN2mi25rollout_finish_seg_kernelILi0EE", r"_ZN2mi25rollout_finish_seg_kernelILi1EE", r"_ZN2mi25rollout_seg_reduce_kernelILi0EE",
                   r"_ZN2mi25rollout_seg_reduce_kernelILi1EE", r"_ZN2mi23rollout_seg_norm_kernelILi0EE", r"_ZN2mi23rollout_seg_norm_kernelILi1EE"]
FINISH = r"_ZN2mi21rollout_finish_kernelE"


def test_segment_kernels_in_the_gfx950_listing():
    text = _listing("ppo_ops")
    for prefix in SEGMENT_KERNELS:
        name, body, scratch, static_lds = _kernel(text, prefix)
        assert scratch == 0, name
        assert static_lds == 0, name                                                # the deltas live in dynamic LDS sized by the horizon, not by the limit
        assert not SCALAR_WRITES.search(body), name
        assert "v_mfma" not in body, name
    for prefix in SEGMENT_KERNELS[:2]:                                               # the GAE bodies: fp64 adds and multiplies, the fp32 cast of the returns, deltas through LDS
        name, body, _, _ = _kernel(text, prefix)
        assert "v_add_f64" in body and "v_mul_f64" in body and "v_cvt_f32_f64" in body, name
        assert "ds_write" in body, name
    name, body, _, _ = _kernel(text, SEGMENT_KERNELS[5])
    assert "v_cvt_f32_f64" in body, name                                             # the batch-normalised advantages' fp32 cast
    name, body, scratch, static_lds = _kernel(text, FINISH)
    assert scratch == 0 and static_lds == 32768, name                                # the dense finish kernel is still there, as it was
    assert not SCALAR_WRITES.search(text)


def test_new_sources_do_not_spell_scalar_unit_writes():
    for rel in ("carla-ppo_amd/csrc/ppo_ops.hip", "carla-ppo_amd/rollout.py", "include/mi355_carla.h", "tests/test_rollout_segments_host.py",
                "tests/test_n_rollout_segments_gpu.py", "tests/rollout_host_common.py", "tests/rollout_gpu_common.py", "tools/rollout_buffer_bench.py", "tools/rollout_finish_bench.py"):
        path = os.path.join(ROOT, rel)
        assert os.path.exists(path), rel
        assert not SCALAR_WRITES.search(open(path).read().lower()), rel
