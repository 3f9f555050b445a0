"""CPU-only: what each of the eleven batched rollout entries answers to a call with exactly ONE defect, for every refusal that comes before either handle is read.
Each entry starts from one set of good arguments (normalising, recording and stacking wherever its signature can) and every case changes one thing; the return code
and the whole message are compared with the literal table WANT below, which was produced by running these cases against the library once and is the contract of any
change to the drivers behind the entries.  The handles and buffers are one zeroed host block that no case may write.  A case that another host test already pins with
the whole message is listed in ELSEWHERE and not repeated here."""
import ctypes
import re

ENTRIES = ("mi_rollout_step_batch", "mi_rollout_step_batch_rec", "mi_rollout_value_batch_rec", "mi_rollout_step_batch_norm", "mi_rollout_value_batch_norm",
           "mi_rollout_step_batch_stack", "mi_rollout_value_batch_stack", "mi_mlp_rollout_step_batch", "mi_mlp_rollout_value_batch",
           "mi_mlp_rollout_step_batch_stack", "mi_mlp_rollout_value_batch_stack")
TABLES = ("table_rows", "tab_states", "tab_raw_states", "tab_actions", "tab_values", "tab_final_values")
# table_rows NULL is a form of the call there (nothing is recorded), not a defect
ROWS_OPTIONAL = {e for e in ENTRIES if "mlp" in e or e in ("mi_rollout_step_batch_norm", "mi_rollout_step_batch_stack")}
# obs_mean NULL is a form of the call there (not normalised), and what belongs to obs_mean is then NULL too
MEAN_OPTIONAL = {e for e in ENTRIES if "mlp" in e or e.endswith("_stack")}

# (entry, case) pairs asserted with `==` on the whole message in test_observation_normalization_host.py (the _norm entries and the neighbours), test_mlp_rollout_host.py
# (the two plain MLP entries), test_rollout_truncation_host.py (mi_rollout_value_batch_rec, mi_rollout_step_batch_rec) and test_latent_stack_host.py (the four _stack
# entries: their first handle, latent_stack, hist / lanes / first / sstate / n_lanes, the alignment of sstate; tab_states / tab_raw_states of the two step entries)
ELSEWHERE = {("mi_rollout_step_batch", "frames_u8=NULL"), ("mi_rollout_step_batch_rec", "frames_u8=NULL"), ("mi_rollout_step_batch_rec", "table_rows=NULL"),
             ("mi_rollout_step_batch_rec", "tab_states=NULL"), ("mi_rollout_value_batch_norm", "table_rows=NULL")}
ELSEWHERE |= {("mi_rollout_value_batch_rec", c) for c in ("vae_h=NULL", "ppo_h=NULL", "frames_u8=NULL", "measurements=NULL", "scratch=NULL", "out=NULL", "table_rows=NULL",
                                                          "tab_final_values=NULL", "n_table_rows=0")}
ELSEWHERE |= {("mi_rollout_step_batch_norm", c) for c in ("vae_h=NULL", "ppo_h=NULL", "frames_u8=NULL", "greedy=0", "tab_states=NULL", "tab_raw_states=NULL", "tab_actions=NULL",
                                                          "tab_values=NULL", "n_table_rows=0")}
ELSEWHERE |= {("mi_rollout_value_batch_norm", c) for c in ("vae_h=NULL", "ppo_h=NULL", "tab_final_values=NULL", "n_table_rows=0")}
ELSEWHERE |= {("mi_mlp_rollout_step_batch", c) for c in ("mlp_h=NULL", "ppo_h=NULL", "frames_u8=NULL", "measurements=NULL", "scratch=NULL", "out=NULL", "greedy=0", "tab_states=NULL",
                                                         "tab_raw_states=NULL", "tab_actions=NULL", "tab_values=NULL", "n_table_rows=0")}
ELSEWHERE |= {("mi_mlp_rollout_value_batch", c) for c in ("mlp_h=NULL", "ppo_h=NULL", "frames_u8=NULL", "measurements=NULL", "scratch=NULL", "out=NULL", "tab_final_values=NULL",
                                                          "n_table_rows=0")}
for _e in ENTRIES:
    if _e.endswith("_stack"):
        ELSEWHERE |= {(_e, c) for c in ("vae_h=NULL", "mlp_h=NULL", "latent_stack=1", "latent_stack=MAX+1", "hist=NULL", "lanes=NULL", "first=NULL", "sstate=NULL", "n_lanes=0",
                                        "sstate=odd")}
        if "step" in _e:
            ELSEWHERE |= {(_e, "tab_states=NULL"), (_e, "tab_raw_states=NULL")}

WANT = {
    "mi_rollout_step_batch": {
        (-4, "mi_rollout_step_batch: null handle"): ["vae_h=NULL", "ppo_h=NULL"],
        (-1, "mi_rollout_step_batch: missing buffers"): ["measurements=NULL", "scratch=NULL", "out=NULL", "greedy=0"],
        (-1, "mi_rollout_step_batch: 1 <= n <= MI_ROLLOUT_MAX_ENVS"): ["n=0", "n=MAX+1"],
        (-1, "mi_rollout_step_batch: the scratch must be 16-byte aligned"): ["scratch=odd"],
    },
    "mi_rollout_step_batch_rec": {
        (-4, "mi_rollout_step_batch_rec: null handle"): ["vae_h=NULL", "ppo_h=NULL"],
        (-1, "mi_rollout_step_batch: missing buffers"): ["measurements=NULL", "scratch=NULL", "out=NULL", "greedy=0"],
        (-1, "mi_rollout_step_batch_rec: missing tables"): ["tab_actions=NULL", "tab_values=NULL", "n_table_rows=0"],
        (-1, "mi_rollout_step_batch: 1 <= n <= MI_ROLLOUT_MAX_ENVS"): ["n=0", "n=MAX+1"],
        (-1, "mi_rollout_step_batch: the scratch must be 16-byte aligned"): ["scratch=odd"],
    },
    "mi_rollout_value_batch_rec": {
        (-1, "mi_rollout_value_batch_rec: 1 <= n <= MI_ROLLOUT_MAX_ENVS"): ["n=0", "n=MAX+1"],
        (-1, "mi_rollout_value_batch_rec: the scratch must be 16-byte aligned"): ["scratch=odd"],
    },
    "mi_rollout_step_batch_norm": {
        (-1, "mi_rollout_step_batch_norm: missing buffers"): ["measurements=NULL", "scratch=NULL", "out=NULL"],
        (-1, "mi_rollout_step_batch_norm: missing obs_mean / obs_inv_std / nstate"): ["obs_mean=NULL", "obs_inv_std=NULL", "nstate=NULL"],
        (-1, "mi_rollout_step_batch_norm: nstate must be 16-byte aligned"): ["nstate=odd"],
        (-1, "mi_rollout_step_batch_norm: obs_clip is a positive value (+inf: never clamp)"): ["obs_clip=0.0", "obs_clip=-1.0", "obs_clip=nan"],
        (-1, "mi_rollout_step_batch_norm: 1 <= n <= MI_ROLLOUT_MAX_ENVS"): ["n=0", "n=MAX+1"],
        (-1, "mi_rollout_step_batch_norm: the scratch must be 16-byte aligned"): ["scratch=odd"],
    },
    "mi_rollout_value_batch_norm": {
        (-1, "mi_rollout_value_batch_norm: missing buffers"): ["frames_u8=NULL", "measurements=NULL", "scratch=NULL", "out=NULL"],
        (-1, "mi_rollout_value_batch_norm: missing obs_mean / obs_inv_std / nstate"): ["obs_mean=NULL", "obs_inv_std=NULL", "nstate=NULL"],
        (-1, "mi_rollout_value_batch_norm: nstate must be 16-byte aligned"): ["nstate=odd"],
        (-1, "mi_rollout_value_batch_norm: obs_clip is a positive value (+inf: never clamp)"): ["obs_clip=0.0", "obs_clip=-1.0", "obs_clip=nan"],
        (-1, "mi_rollout_value_batch_norm: 1 <= n <= MI_ROLLOUT_MAX_ENVS"): ["n=0", "n=MAX+1"],
        (-1, "mi_rollout_value_batch_norm: the scratch must be 16-byte aligned"): ["scratch=odd"],
    },
    "mi_rollout_step_batch_stack": {
        (-4, "mi_rollout_step_batch_stack: null handle"): ["ppo_h=NULL"],
        (-1, "mi_rollout_step_batch_stack: missing buffers"): ["frames_u8=NULL", "measurements=NULL", "scratch=NULL", "out=NULL", "greedy=0"],
        (-1, "mi_rollout_step_batch_stack: missing tables"): ["tab_actions=NULL", "tab_values=NULL", "n_table_rows=0"],
        (-1, "mi_rollout_step_batch_stack: obs_inv_std and tab_raw_states are NULL where obs_mean is"): ["obs_mean=NULL", "plain+obs_inv_std", "plain+tab_raw_states"],
        (-1, "mi_rollout_step_batch_stack: obs_inv_std is missing or obs_clip is not a positive value (+inf: never clamp)"):
            ["obs_inv_std=NULL", "obs_clip=0.0", "obs_clip=-1.0", "obs_clip=nan"],
        (-1, "mi_rollout_step_batch_stack: 1 <= n <= MI_ROLLOUT_MAX_ENVS"): ["n=0", "n=MAX+1"],
        (-1, "mi_rollout_step_batch_stack: the scratch must be 16-byte aligned"): ["scratch=odd"],
    },
    "mi_rollout_value_batch_stack": {
        (-4, "mi_rollout_value_batch_stack: null handle"): ["ppo_h=NULL"],
        (-1, "mi_rollout_value_batch_stack: missing buffers"): ["frames_u8=NULL", "measurements=NULL", "scratch=NULL", "out=NULL"],
        (-1, "mi_rollout_value_batch_stack: missing tables"): ["table_rows=NULL", "tab_final_values=NULL", "n_table_rows=0"],
        (-1, "mi_rollout_value_batch_stack: obs_inv_std and tab_raw_states are NULL where obs_mean is"): ["obs_mean=NULL"],
        (-1, "mi_rollout_value_batch_stack: obs_inv_std is missing or obs_clip is not a positive value (+inf: never clamp)"):
            ["obs_inv_std=NULL", "obs_clip=0.0", "obs_clip=-1.0", "obs_clip=nan"],
        (-1, "mi_rollout_value_batch_stack: 1 <= n <= MI_ROLLOUT_MAX_ENVS"): ["n=0", "n=MAX+1"],
        (-1, "mi_rollout_value_batch_stack: the scratch must be 16-byte aligned"): ["scratch=odd"],
    },
    "mi_mlp_rollout_step_batch": {
        (-1, "mi_mlp_rollout_step_batch: obs_inv_std, nstate and tab_raw_states are NULL where obs_mean is"):
            ["obs_mean=NULL", "plain+obs_inv_std", "plain+nstate", "plain+tab_raw_states"],
        (-1, "mi_mlp_rollout_step_batch: missing obs_mean / obs_inv_std / nstate"): ["obs_inv_std=NULL", "nstate=NULL"],
        (-1, "mi_mlp_rollout_step_batch: nstate must be 16-byte aligned"): ["nstate=odd"],
        (-1, "mi_mlp_rollout_step_batch: obs_clip is a positive value (+inf: never clamp)"): ["obs_clip=0.0", "obs_clip=-1.0", "obs_clip=nan"],
        (-1, "mi_mlp_rollout_step_batch: 1 <= n <= MI_ROLLOUT_MAX_ENVS"): ["n=0", "n=MAX+1"],
        (-1, "mi_mlp_rollout_step_batch: the scratch must be 16-byte aligned"): ["scratch=odd"],
        (-1, "mi_mlp_rollout_step_batch: the frames must be 4-byte aligned"): ["frames_u8=odd"],
    },
    "mi_mlp_rollout_value_batch": {
        (-1, "mi_mlp_rollout_value_batch: obs_inv_std, nstate and tab_raw_states are NULL where obs_mean is"): ["obs_mean=NULL", "plain+obs_inv_std", "plain+nstate"],
        (-1, "mi_mlp_rollout_value_batch: missing obs_mean / obs_inv_std / nstate"): ["obs_inv_std=NULL", "nstate=NULL"],
        (-1, "mi_mlp_rollout_value_batch: nstate must be 16-byte aligned"): ["nstate=odd"],
        (-1, "mi_mlp_rollout_value_batch: obs_clip is a positive value (+inf: never clamp)"): ["obs_clip=0.0", "obs_clip=-1.0", "obs_clip=nan"],
        (-1, "mi_mlp_rollout_value_batch: 1 <= n <= MI_ROLLOUT_MAX_ENVS"): ["n=0", "n=MAX+1"],
        (-1, "mi_mlp_rollout_value_batch: the scratch must be 16-byte aligned"): ["scratch=odd"],
        (-1, "mi_mlp_rollout_value_batch: the frames must be 4-byte aligned"): ["frames_u8=odd"],
    },
    "mi_mlp_rollout_step_batch_stack": {
        (-4, "mi_mlp_rollout_step_batch_stack: null handle"): ["ppo_h=NULL"],
        (-1, "mi_mlp_rollout_step_batch_stack: missing buffers"): ["frames_u8=NULL", "measurements=NULL", "scratch=NULL", "out=NULL", "greedy=0"],
        (-1, "mi_mlp_rollout_step_batch_stack: missing tables"): ["tab_actions=NULL", "tab_values=NULL", "n_table_rows=0"],
        (-1, "mi_mlp_rollout_step_batch_stack: obs_inv_std and tab_raw_states are NULL where obs_mean is"): ["obs_mean=NULL", "plain+obs_inv_std", "plain+tab_raw_states"],
        (-1, "mi_mlp_rollout_step_batch_stack: obs_inv_std is missing or obs_clip is not a positive value (+inf: never clamp)"):
            ["obs_inv_std=NULL", "obs_clip=0.0", "obs_clip=-1.0", "obs_clip=nan"],
        (-1, "mi_mlp_rollout_step_batch_stack: 1 <= n <= MI_ROLLOUT_MAX_ENVS"): ["n=0", "n=MAX+1"],
        (-1, "mi_mlp_rollout_step_batch_stack: the scratch must be 16-byte aligned"): ["scratch=odd"],
        (-1, "mi_mlp_rollout_step_batch_stack: the frames must be 4-byte aligned"): ["frames_u8=odd"],
    },
    "mi_mlp_rollout_value_batch_stack": {
        (-4, "mi_mlp_rollout_value_batch_stack: null handle"): ["ppo_h=NULL"],
        (-1, "mi_mlp_rollout_value_batch_stack: missing buffers"): ["frames_u8=NULL", "measurements=NULL", "scratch=NULL", "out=NULL"],
        (-1, "mi_mlp_rollout_value_batch_stack: missing tables"): ["tab_final_values=NULL", "n_table_rows=0"],
        (-1, "mi_mlp_rollout_value_batch_stack: obs_inv_std and tab_raw_states are NULL where obs_mean is"): ["obs_mean=NULL"],
        (-1, "mi_mlp_rollout_value_batch_stack: obs_inv_std is missing or obs_clip is not a positive value (+inf: never clamp)"):
            ["obs_inv_std=NULL", "obs_clip=0.0", "obs_clip=-1.0", "obs_clip=nan"],
        (-1, "mi_mlp_rollout_value_batch_stack: 1 <= n <= MI_ROLLOUT_MAX_ENVS"): ["n=0", "n=MAX+1"],
        (-1, "mi_mlp_rollout_value_batch_stack: the scratch must be 16-byte aligned"): ["scratch=odd"],
        (-1, "mi_mlp_rollout_value_batch_stack: the frames must be 4-byte aligned"): ["frames_u8=odd"],
    },
}


def cases(entry, names, p, max_envs, max_stack):
    """-> [(case, {argument: value})]: the single defects of `entry`, whose arguments are `names`; p: the address of the zeroed block (16-byte aligned)."""
    out = [(h + "=NULL", {h: None}) for h in (names[0], "ppo_h")]
    out += [(b + "=NULL", {b: None}) for b in ("frames_u8", "measurements", "scratch", "out")]
    if "greedy" in names:
        out.append(("greedy=0", {"greedy": 0}))                                      # sampling without noise
    if "table_rows" in names:
        out += [(t + "=NULL", {t: None}) for t in TABLES if t in names and not (t == "table_rows" and entry in ROWS_OPTIONAL)]
        out.append(("n_table_rows=0", {"n_table_rows": 0}))
    if "obs_mean" in names:
        norm = [a for a in ("obs_mean", "obs_inv_std", "nstate") if a in names]
        out += [(a + "=NULL", {a: None}) for a in norm]
        if "nstate" in names:
            out.append(("nstate=odd", {"nstate": p + 4}))
        out += [("obs_clip=%r" % c, {"obs_clip": c}) for c in (0.0, -1.0, float("nan"))]
        if entry in MEAN_OPTIONAL:                                                   # the call that does not normalise, and one of them given all the same
            plain = {a: None for a in norm + ["tab_raw_states"] if a in names}
            out += [("plain+" + a, {k: v for k, v in plain.items() if k != a}) for a in plain if a != "obs_mean" and len(plain) > 2]
    if "latent_stack" in names:
        out += [("latent_stack=1", {"latent_stack": 1}), ("latent_stack=MAX+1", {"latent_stack": max_stack + 1})]
        out += [(a + "=NULL", {a: None}) for a in ("hist", "lanes", "first", "sstate")]
        out += [("n_lanes=0", {"n_lanes": 0}), ("sstate=odd", {"sstate": p + 4})]
    out += [("n=0", {"n": 0}), ("n=MAX+1", {"n": max_envs + 1}), ("scratch=odd", {"scratch": p + 4})]
    if "mlp" in entry:
        out.append(("frames_u8=odd", {"frames_u8": p + 2}))
    return [(c, kw) for c, kw in out if (entry, c) not in ELSEWHERE]


def answers():
    """-> ({entry: {(return code, message): [case, ..]}}, the zeroed block) from the library."""
    from mi355 import lib as milib
    L = milib.get()
    text = open(milib.HEADER).read()
    max_envs, max_stack = (int(re.search(r"#define\s+%s\s+(\d+)" % d, text).group(1)) for d in ("MI_ROLLOUT_MAX_ENVS", "MI_ROLLOUT_MAX_STACK"))
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    p += -p % 16
    scalars = dict(stream=None, n_meas=3, noise=None, greedy=1, n=4, scratch_bytes=0, obs_clip=10.0, n_table_rows=8, latent_stack=4, n_lanes=4, advance=1)
    got = {}
    for entry in ENTRIES:
        names = [a[1] for a in L.protos[entry][1]]
        good = {a: scalars.get(a, p) for a in names}
        for case, kw in cases(entry, names, p, max_envs, max_stack):
            rc = getattr(L.cdll, entry)(*[dict(good, **kw)[a] for a in names])
            got.setdefault(entry, {}).setdefault((rc, L.cdll.mi_last_error().decode()), []).append(case)
    return got, buf


def test_every_single_defect_gets_the_code_and_the_message_of_the_table():
    got, buf = answers()
    assert sorted(got) == sorted(WANT)
    for entry in ENTRIES:
        assert got[entry] == WANT[entry], entry
    assert all(x == 0.0 for x in buf)                                                # nothing was written
