"""CPU-only tests of truncation in continuous collection (mi_rollout_value_batch_rec / mi_rollout_finish_segments_boot / rollout.SegmentedRows.truncate_rows /
rollout.ContinuousRolloutBuffer.truncate): the C-ABI surface and every argument error the host can check without an engine, the book-keeping (numpy only) on a scripted
collection with the three kinds of truncation and every misuse, a collection without truncation left as it was, and the gfx950 code of ppo_ops.hip and rollout.hip
(compiled here, no GPU needed): the two new kernels exist under names of their own beside the old ones, spill nothing, and the finish kernel has no static LDS."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from rollout_host_common import ROOT, _kernel, _listing


FINISH_ARGS = [("void*", "stream"), ("const float*", "tab_values"), ("const double*", "rewards"), ("const double*", "terminals"), ("const int*", "seg_row"),
               ("const int*", "seg_len"), ("int", "n_seg"), ("int", "num_envs"), ("int", "T"), ("double", "gamma"), ("double", "lam"), ("int", "normalize"),
               ("double*", "scratch"), ("float*", "tab_returns"), ("float*", "tab_advantages"), ("double*", "adv_raw"), ("double*", "returns"), ("double*", "adv_norm")]
VALUE_ARGS = [("void*", "vae_h"), ("void*", "ppo_h"), ("void*", "stream"), ("const unsigned char*", "frames_u8"), ("const float*", "measurements"), ("int", "n_meas"),
              ("int", "n"), ("void*", "scratch"), ("long long", "scratch_bytes"), ("float*", "out"), ("const int*", "table_rows"), ("long long", "n_table_rows"),
              ("float*", "tab_final_values")]


def test_entry_points_are_declared_and_exported():
    from mi355 import lib as milib
    protos = milib.parse_header()
    assert protos["mi_rollout_finish_segments"] == ("int", FINISH_ARGS)                                  # the old entry, as it was
    assert protos["mi_rollout_finish_segments_boot"] == ("int", FINISH_ARGS + [("const float*", "tab_final_values"), ("const int*", "seg_boot")])
    assert protos["mi_rollout_value_batch_rec"] == ("int", VALUE_ARGS)
    # the value call takes what the recording step takes, without the noise, the greedy flag and the three step tables
    rec = [a for a in protos["mi_rollout_step_batch_rec"][1] if a[1] not in ("noise", "greedy", "tab_states", "tab_actions", "tab_values")]
    assert rec == VALUE_ARGS[:-1]
    L = milib.get()
    assert hasattr(L.cdll, "mi_rollout_finish_segments_boot") and hasattr(L.cdll, "mi_rollout_value_batch_rec")
    assert L.mi_abi_version() == 7
    text = open(milib.HEADER).read()
    for fn, cites in (("int mi_rollout_finish_segments_boot", ("utils.py:45-50", "train.py:175-177", "seg_boot", "tab_final_values", "NOT read")),
                      ("int mi_rollout_value_batch_rec", ("train.py:172", "ppo.py:70-71", "table_rows", "records nothing"))):
        i = text.index(fn)
        comment = text[text.rfind("/*", 0, i):i]
        for c in cites:
            assert c in comment, (fn, c)


def test_every_host_checkable_argument_error_of_the_finish_entry():
    """test_rollout_segments_host.py's table on the new entry, plus its two own buffers.  The pointers are never dereferenced on the host."""
    from mi355 import lib as milib
    L = milib.get()
    limit = int(re.search(r"#define\s+MI_ROLLOUT_MAX_HORIZON\s+(\d+)", open(milib.HEADER).read()).group(1))
    buf = (ctypes.c_double * 16)()
    p = ctypes.addressof(buf)
    fin, err = L.cdll.mi_rollout_finish_segments_boot, L.cdll.mi_last_error
    names = [a[1] for a in milib.parse_header()["mi_rollout_finish_segments_boot"][1]]
    good = dict(stream=None, tab_values=p, rewards=p, terminals=p, seg_row=p, seg_len=p, n_seg=3, num_envs=2, T=4, gamma=0.99, lam=0.95, normalize=0, scratch=None,
                tab_returns=p, tab_advantages=p, adv_raw=None, returns=None, adv_norm=None, tab_final_values=p, seg_boot=p)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return fin(*[a[n] for n in names])
    for missing in ("tab_values", "rewards", "terminals", "seg_row", "seg_len", "tab_returns", "tab_advantages", "tab_final_values", "seg_boot"):
        assert call(**{missing: None}) == -1 and b"missing buffers" in err() and err().startswith(b"mi_rollout_finish_segments_boot:"), missing
    for missing in ("tab_final_values", "seg_boot"):
        assert call(**{missing: None}) == -1 and missing.encode() in err(), missing
    for kw in (dict(n_seg=0), dict(n_seg=-1), dict(num_envs=0), dict(T=0)):
        assert call(**kw) == -1 and b"empty" in err(), kw
    assert call(T=limit + 1) == -1 and b"MI_ROLLOUT_MAX_HORIZON" in err()
    for bad in (2, -1):
        assert call(normalize=bad, scratch=p, adv_raw=p) == -1 and b"normalize" in err(), bad
    assert call(normalize=1, scratch=None, adv_raw=p) == -1 and b"scratch" in err()
    assert call(normalize=1, scratch=p, adv_raw=None) == -1 and b"adv_raw" in err()
    assert err().startswith(b"mi_rollout_finish_segments_boot:")
    # the old entry still answers under its own name
    old = L.cdll.mi_rollout_finish_segments
    assert old(*[dict(good, tab_values=None)[n] for n in names[:-2]]) == -1 and err().startswith(b"mi_rollout_finish_segments: missing buffers")


def test_every_host_checkable_argument_error_of_the_value_entry():
    """Null handles are a state error; everything checked before an engine is looked at is MI_ERR_ARG with a message.  The handles here are never dereferenced: every
    call fails before the first check that needs the engine (the scratch size; tested on the GPU, with real handles)."""
    from mi355 import lib as milib
    L = milib.get()
    limit = int(re.search(r"#define\s+MI_ROLLOUT_MAX_ENVS\s+(\d+)", open(milib.HEADER).read()).group(1))
    buf = (ctypes.c_double * 16)()
    p = ctypes.addressof(buf)
    assert p % 16 == 0 or (p + 8) % 16 == 0
    aligned = p if p % 16 == 0 else p + 8
    val, err = L.cdll.mi_rollout_value_batch_rec, L.cdll.mi_last_error
    names = [a[1] for a in VALUE_ARGS]
    good = dict(vae_h=p, ppo_h=p, stream=None, frames_u8=p, measurements=p, n_meas=3, n=2, scratch=aligned, scratch_bytes=1 << 30, out=p, table_rows=p, n_table_rows=8,
                tab_final_values=p)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return val(*[a[n] for n in names])
    for h in ("vae_h", "ppo_h"):
        assert call(**{h: None}) == -4 and err() == b"mi_rollout_value_batch_rec: null handle", h
    for missing in ("frames_u8", "measurements", "scratch", "out"):
        assert call(**{missing: None}) == -1 and err() == b"mi_rollout_value_batch_rec: missing buffers", missing
    for kw in (dict(table_rows=None), dict(tab_final_values=None), dict(n_table_rows=0), dict(n_table_rows=-3)):
        assert call(**kw) == -1 and err() == b"mi_rollout_value_batch_rec: missing tables", kw
    for n in (0, -1, limit + 1):
        assert call(n=n) == -1 and err().startswith(b"mi_rollout_value_batch_rec: 1 <= n <= MI_ROLLOUT_MAX_ENVS"), n
    assert call(scratch=aligned + 4) == -1 and err().startswith(b"mi_rollout_value_batch_rec: the scratch must be 16-byte aligned")
    # the step's own entries keep their messages
    assert L.cdll.mi_rollout_step_batch_rec(p, p, None, None, p, 3, None, 1, 4, aligned, 0, p, p, 8, p, p, p) == -1 and err() == b"mi_rollout_step_batch: missing buffers"
    assert L.cdll.mi_rollout_step_batch_rec(p, p, None, p, p, 3, None, 1, 4, aligned, 0, p, None, 8, p, p, p) == -1 and err() == b"mi_rollout_step_batch_rec: missing tables"


def test_the_new_signatures_and_the_old_ones_unchanged():
    import rollout
    from rollout import ContinuousRolloutBuffer as C, RolloutBuffer as B, RolloutRows, SegmentedRows
    sig = lambda f: list(inspect.signature(f).parameters)      # noqa: E731
    defaults = lambda f: {k: v.default for k, v in inspect.signature(f).parameters.items() if k != "self"}      # noqa: E731
    assert sig(C.truncate) == ["self", "final_frames_u8", "final_measurements", "env_ids"] and defaults(C.truncate)["env_ids"] is None
    assert sig(SegmentedRows.truncate_rows) == ["self", "env_ids", "n"] and sig(SegmentedRows.segment_truncated) == ["self"]
    assert sig(rollout.BatchedRolloutStep.record_value) == ["self", "f", "n", "meas", "table_rows", "final_values"]
    assert sig(C.__init__) == ["self", "vae", "ppo", "num_envs", "horizon", "seed", "io"] and defaults(C.__init__) == dict(
        vae=inspect.Parameter.empty, ppo=inspect.Parameter.empty, num_envs=inspect.Parameter.empty, horizon=inspect.Parameter.empty, seed=None, io=None)
    assert sig(C.reset) == ["self"]
    assert sig(C.step) == ["self", "frames_u8", "measurements", "env_ids", "greedy", "noise"]
    assert sig(C.outcome) == ["self", "rewards", "dones", "env_ids"]
    assert sig(C.bootstrap) == ["self", "frames_u8", "measurements", "env_ids"] and defaults(C.bootstrap)["env_ids"] is None
    assert sig(C.update) == ["self", "gamma", "lam", "num_epochs", "batch_size", "normalize", "stage_times"]
    assert defaults(C.update) == dict(gamma=0.99, lam=0.95, num_epochs=3, batch_size=32, normalize="segment", stage_times=None)
    # RolloutRows and RolloutBuffer stay as they are: no truncation there
    for name in ("truncate", "final_values"):
        assert not hasattr(B, name), name
    rows = RolloutRows(2, 4)
    for name in ("truncs", "truncate_rows", "segment_truncated", "segments"):
        assert not hasattr(rows, name), name
    assert sig(B.update) == ["self", "gamma", "lam", "num_epochs", "batch_size", "stage_times"]
    for text in (rollout.__doc__, open(os.path.join(ROOT, "INTEGRATION.md")).read()):
        assert "buf.truncate(final_frames[cut], final_measurements[cut], env_ids=cut)" in text and "mi_rollout_value_batch_rec" in text
        assert "mi_rollout_finish_segments_boot" in text


def collect(rows, done_at, trunc_at, steps=None):
    """Every lane steps `steps` (default: the horizon) times, all lanes in every call; lane e reports done at its steps done_at[e] and is truncated behind its steps
    trunc_at[e] (1-based).  -> the rows every truncate_rows call returned."""
    E, T = rows.num_envs, rows.horizon
    got = []
    for t in range(1, (steps or T) + 1):
        assert rows.step_rows(None, E).tolist() == [e * (T + 1) + t - 1 for e in range(E)]
        rows.outcome([10.0 * e + t for e in range(E)], np.array([t in done_at.get(e, ()) for e in range(E)]))
        cut = np.array([e for e in range(E) if t in trunc_at.get(e, ())], np.int64)
        if len(cut):
            r = rows.truncate_rows(cut, len(cut))
            assert r.dtype == np.int32 and r.tolist() == [int(e) * (T + 1) + t - 1 for e in cut]          # the row of the LAST COUNTED step, slot lengths[e] - 1
            got.append(r.tolist())
    return got


def test_bookkeeping_of_a_scripted_collection_with_truncations():
    """E = 3, T = 6: lane 0 is truncated behind its step 3 and goes on to the horizon, lane 1 is truncated at its last slot, lane 2 has a done at step 2 and a truncation
    behind step 4."""
    from rollout import SegmentedRows
    E, T = 3, 6
    rows = SegmentedRows(E, T)
    assert rows.truncs.shape == (E, T) and not rows.truncs.any()
    got = collect(rows, {2: (2,)}, {0: (3,), 1: (6,), 2: (4,)})
    assert got == [[2], [17], [12]]
    assert rows.lengths.tolist() == [6, 6, 6] and rows.ended.all() and not rows.awaiting.any() and not rows.closed.any()
    assert np.argwhere(rows.truncs).tolist() == [[0, 2], [1, 5], [2, 3]]
    assert rows.dones[2].tolist() == [0, 1, 0, 0, 0, 0] and not rows.dones[:2].any()                      # a truncated step reports done False
    segs = rows.segments()
    assert segs.dtype == np.int32 and segs.shape == (6, 3)
    assert segs.tolist() == [[0, 0, 3], [0, 3, 3], [1, 0, 6], [2, 0, 2], [2, 2, 2], [2, 4, 2]]
    st = rows.segment_truncated()
    assert st.dtype == np.int32 and st.tolist() == [1, 0, 1, 0, 1, 0]
    covered = np.concatenate([e * (T + 1) + s + np.arange(n) for e, s, n in segs])
    assert covered.tolist() == rows.valid_rows().tolist() == list(range(0, 6)) + list(range(7, 13)) + list(range(14, 20))      # every recorded step in exactly one segment
    assert rows.needs_bootstrap().tolist() == [0, 2]                                                     # lane 1: full AND truncated at its last slot: nothing more is needed
    assert rows._last_done().tolist() == [False, True, False]
    with pytest.raises(ValueError, match=r"environments \[0, 2\]\): bootstrap them first"):
        rows.check_update()
    assert rows.bootstrap_rows([0, 2], 2).tolist() == [6, 20]
    rows.check_update()
    assert rows.bootstrap_rows([1], 1).tolist() == [13]                                                  # given one anyway: recorded, never read
    rows.check_update()
    assert rows.segments().tolist() == segs.tolist() and rows.segment_truncated().tolist() == st.tolist()
    rows.reset()
    assert not rows.truncs.any() and rows.truncs.shape == (E, T) and rows.segments().shape == (0, 3) and rows.segment_truncated().shape == (0,)
    assert rows.segment_truncated().dtype == np.int32
    # lanes that stop early: one whose only step is truncated, and one truncated step behind a done
    rows = SegmentedRows(2, 4)
    collect(rows, {1: (1,)}, {0: (1,), 1: (2,)}, steps=2)
    assert rows.segments().tolist() == [[0, 0, 1], [0, 1, 1], [1, 0, 1], [1, 1, 1]] and rows.segment_truncated().tolist() == [1, 0, 0, 1]
    assert rows.needs_bootstrap().tolist() == [0]


def snapshot(rows):
    return [x.copy() for x in (rows.lengths, rows.state, rows.rewards, rows.dones, rows.truncs)]


def test_every_misuse_of_truncate_rows_raises_and_changes_nothing():
    from rollout import SegmentedRows
    rows = SegmentedRows(4, 3)

    def refused(ids, n, match):
        before = snapshot(rows)
        with pytest.raises(ValueError, match=match):
            rows.truncate_rows(ids, n)
        for x, y in zip(before, snapshot(rows)):
            assert np.array_equal(x, y), match
    refused([0], 1, "empty row")
    rows.step_rows([0, 1, 2], 3)
    refused([0], 1, "no outcome yet")                                                # awaiting
    rows.outcome([1.0, 2.0, 3.0], [False, True, False], [0, 1, 2])
    refused([1], 1, "terminal stays a terminal")                                     # the last counted step reported done
    refused([0, 1], 2, "terminal stays a terminal")                                  # one offender refuses the whole call ...
    assert not rows.truncs.any()                                                     # ... and lane 0 was not marked
    refused([0, 3], 2, "empty row")
    for ids, n in (([0, 0], 2), ([0, 4], 2), ([-1], 1), ([0, 2], 1), ([0.0, 2.0], 2), ([[0, 2]], 2), (None, 5), (None, 0)):      # the usual env_ids errors
        refused(ids, n, "RolloutBuffer")
    assert rows.truncate_rows([0], 1).tolist() == [0]
    refused([0], 1, "already truncated")
    refused([2, 0], 2, "already truncated")
    assert rows.truncs.sum() == 1 and rows.truncs[0, 0]
    rows.step_rows([0], 1)                                                           # the lane goes on behind a truncation
    refused([0], 1, "no outcome yet")
    rows.outcome([1.5], [False], [0])
    assert rows.truncate_rows([0], 1).tolist() == [1]                                # back to back, like dones
    rows.step_rows([0, 2], 2)
    rows.outcome([1.0, 1.0], [False, False], [0, 2])
    assert rows.ended.tolist() == [True, False, False, False]
    assert rows.truncate_rows([0], 1).tolist() == [2]                                # a full lane may be truncated ...
    assert rows.needs_bootstrap().tolist() == [2]                                    # ... and then needs no bootstrap
    assert rows.bootstrap_rows([2], 1).tolist() == [10]
    refused([2], 1, "closed row")
    rows.check_update()
    assert rows.segments().tolist() == [[0, 0, 1], [0, 1, 1], [0, 2, 1], [1, 0, 1], [2, 0, 2]] and rows.segment_truncated().tolist() == [1, 1, 1, 0, 0]


def parent_segments(rows):
    """SegmentedRows.segments() as it was before truncation existed: a cut behind every done, and the lane's end."""
    out = []
    for e in range(rows.num_envs):
        n = int(rows.lengths[e])
        ends = (np.nonzero(rows.dones[e, :n] != 0)[0] + 1).tolist()
        if n and (not ends or ends[-1] != n):
            ends.append(n)
        first = 0
        for end in ends:
            out.append((e, first, end - first))
            first = end
    return np.asarray(out, np.int32).reshape(-1, 3)


def test_a_collection_without_truncation_is_what_it_was():
    """test_rollout_segments_host.py's script and its pinned results, and the earlier rule restated, on seeded random scripts."""
    from rollout import SegmentedRows
    from test_rollout_segments_host import script
    rows = SegmentedRows(4, 6)
    script(rows, {1: (3, 6), 2: (6,)}, {3: 3})
    assert rows.segments().tolist() == [[0, 0, 6], [1, 0, 3], [1, 3, 3], [2, 0, 6], [3, 0, 3]] and rows.segments().dtype == np.int32
    assert rows.segment_truncated().tolist() == [0] * 5 and not rows.truncs.any()
    assert rows.needs_bootstrap().tolist() == [0, 3] and rows._last_done().tolist() == [False, True, True, False]
    rng = np.random.RandomState(5)
    for _ in range(20):
        E, T = int(rng.randint(1, 6)), int(rng.randint(1, 9))
        rows = SegmentedRows(E, T)
        done_at = {e: tuple(np.nonzero(rng.rand(T) < 0.3)[0] + 1) for e in range(E)}
        stop_at = {e: int(rng.randint(0, T + 1)) for e in range(E)}
        script(rows, done_at, stop_at)
        assert np.array_equal(rows.segments(), parent_segments(rows)) and rows.segments().dtype == np.int32
        last = np.maximum(rows.lengths, 1) - 1
        last_done = (rows.lengths > 0) & (rows.dones[np.arange(E), last] != 0)
        assert rows._last_done().tolist() == last_done.tolist()
        assert rows.needs_bootstrap().tolist() == np.nonzero((rows.lengths > 0) & ~last_done)[0].tolist()
        assert not rows.segment_truncated().any()


NEW_FINISH = [r"_ZN2mi30rollout_finish_seg_boot_kernelILi0EE", r"_ZN2mi30rollout_finish_seg_boot_kernelILi1EE"]
NEW_VALUE = r"_ZN2mi24rollout_value_rec_kernelE"
OLD_PPO_OPS = [r"_ZN2mi25rollout_finish_seg_kernelILi0EE", r"_ZN2mi25rollout_finish_seg_kernelILi1EE", r"_ZN2mi25rollout_seg_reduce_kernelILi0EE",
               r"_ZN2mi25rollout_seg_reduce_kernelILi1EE", r"_ZN2mi23rollout_seg_norm_kernelILi0EE", r"_ZN2mi23rollout_seg_norm_kernelILi1EE", r"_ZN2mi21rollout_finish_kernelE"]
OLD_ROLLOUT = [r"_ZN2mi23rollout_head_rec_kernelILi2EE", r"_ZN2mi23rollout_head_rec_kernelILi8EE", r"_ZN2mi25rollout_head_batch_kernelILi2EE",
               r"_ZN2mi25rollout_conv_batch_kernelILi2EE", r"_ZN2mi25rollout_conv_batch_kernelILi3EE", r"_ZN2mi26rollout_conv1_batch_kernelILi12EE"]


def test_the_new_kernels_in_the_gfx950_listings():
    text = _listing("ppo_ops")
    for prefix in NEW_FINISH:
        name, body, scratch, static_lds = _kernel(text, prefix)
        assert scratch == 0, name                                                    # no private segment
        assert static_lds == 0, name                                                 # the deltas live in dynamic LDS sized by the horizon
    for prefix in OLD_PPO_OPS:                                                       # the old kernels keep their names
        _kernel(text, prefix)
    text = _listing("rollout")
    name, body, scratch, static_lds = _kernel(text, NEW_VALUE)
    assert scratch == 0, name
    assert static_lds == 16, name                                                    # one partial sum per wave
    for prefix in OLD_ROLLOUT:
        _kernel(text, prefix)
