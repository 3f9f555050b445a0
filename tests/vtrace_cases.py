"""Cases and references of the V-trace tests (test infrastructure; used by test_vtrace_cases_host.py and test_zzzzzzzzzzzzzz_vtrace_gpu.py).  numpy only: nothing
here calls rollout.py, ppo.py or the library.

The op under test is mi_rollout_finish_vtrace (include/mi355_carla.h): per segment, from its last step to its first, with Dn = 0.0 and gl = gamma * lam,
    cw = min(c_bar, w_t), rw = min(rho_bar, w_t)     (as w > bar ? bar : w)
    A_t = gl Dn + delta_t ;  D_t = ((gl cw) Dn) + (rw delta_t) ;  Dn = D_t
returns = D + V, raw advantages = A, advantages = A normalised per segment or over the batch.

Two float64 references:
  (a) recurrence(): the recurrence above in the same operation order (python floats: every product and sum rounded once).  It takes the weights as an argument.
  (b) forward_definition(): the textbook forward definition (Espeholt et al. 2018, eq. 1 and section 4.2), written on its own and sharing no code with (a):
          vs_t - V_t = sum_k gamma^k (prod_{i<k} lam c_{t+i}) rho_{t+k} delta_{t+k} ,   A_t = delta_t + gamma lam (vs_{t+1} - V_{t+1})

Cases.  SHAPES (E, T) = (1, 1), (3, 5), (2, 64), (2, 65), (5, 70) -- 64 and 65 straddle the wave width -- times BARS (rho_bar, c_bar) = (1, 1), (2.5, 1.5), (inf, inf),
(0.5, 0).  A case's lanes are cut into several segments of ragged lengths (with unused slots between some of them) whose kinds cycle through: a terminal last step, a
truncated segment with a final value, and a segment that ends without done (the value behind it is read).  Every case with room for it also carries the four bad
descriptors (n < 1, s + n > T, lane >= num_envs, negative row), which are not executed.  The log-ratios lp_now - lp_old are uniform in +-1.25 (weights in
[0.29, 3.5]), with the first executed steps forced to +-1.2 so that every case has a weight above and a weight below each finite positive bar (asserted by the host
test; at c_bar = 0 no weight can lie below the bar, and every weight lies above it).  The one-step shape (1, 1) cannot have both in one table: it comes as two
variants, one weight above every finite bar and one below, and the condition is asserted over the pair."""
import itertools

import numpy as np

SHAPES = ((1, 1), (3, 5), (2, 64), (2, 65), (5, 70))
BARS = ((1.0, 1.0), (2.5, 1.5), (float("inf"), float("inf")), (0.5, 0.0))
GAMMA, LAM = 0.99, 0.95
TERMINAL, TRUNCATED, OPEN = 0, 1, 2


def layout(E, T, seed):
    """-> executed segments [(lane, first slot, length, kind)]: several per lane, ragged, kinds cycling."""
    rng = np.random.RandomState(900 + 31 * E + T + seed)
    segs, kind = [], seed % 3
    for e in range(E):
        s = 0
        while s < T:
            n = int(rng.randint(1, max(2, min(T - s, 1 + T // 2)) + 1))
            n = min(n, T - s)
            segs.append((e, s, n, kind))
            kind = (kind + 1) % 3
            s += n + (int(rng.randint(0, 2)) if T > 4 else 0)      # (an unused slot between some segments: it belongs to no segment)
    return segs


def build(E, T, bars, variant=0, seed=0):
    """One case -> dict.  Tables are float32 [E, T + 1] (the device's layout flattened), rewards / dones float64 [E, T]; seg_row / seg_len / seg_boot int32 with the bad
    descriptors appended behind the executed ones; executed: bool per descriptor."""
    rng = np.random.RandomState(4000 + 97 * E + 7 * T + seed)
    segs = layout(E, T, seed)
    values = rng.standard_normal((E, T + 1)).astype(np.float32)
    final_values = rng.standard_normal((E, T + 1)).astype(np.float32)
    lp_old = (-1.5 + 0.8 * rng.standard_normal((E, T + 1))).astype(np.float32)
    ratio = rng.uniform(-1.25, 1.25, (E, T + 1))
    steps = [(e, s + i) for e, s, n, _ in segs for i in range(n)]
    forced = (1.2, -1.2) if len(steps) > 1 else ((1.2,) if variant == 0 else (-1.2,))
    for (e, t), x in zip(steps, forced):
        ratio[e, t] = x
    lp_now = (lp_old.astype(np.float64) + ratio).astype(np.float32)
    rewards = rng.uniform(-1, 1, (E, T))
    dones = np.zeros((E, T))
    for e, s, n, kind in segs:
        if kind == TERMINAL:
            dones[e, s + n - 1] = 1.0
    row = [e * (T + 1) + s for e, s, n, _ in segs]
    length = [n for _, _, n, _ in segs]
    boot = [1 if kind == TRUNCATED else 0 for *_, kind in segs]
    bad = [(0, 0), (max(T - 1, 0), 3), (E * (T + 1), 1), (-1, 1)]      # n < 1 | s + n > T | lane >= num_envs | negative row
    if E * T == 1:
        bad = bad[:2]                                                     # (kept small at the one-step shape: still one of each kind that fits)
    for r, n in bad:
        row.append(r), length.append(n), boot.append(0)
    executed = np.array([True] * len(segs) + [False] * len(bad))
    return dict(E=E, T=T, rho_bar=float(bars[0]), c_bar=float(bars[1]), variant=variant, segs=segs, values=values, final_values=final_values, lp_old=lp_old,
                lp_now=lp_now, rewards=rewards, dones=dones, seg_row=np.asarray(row, np.int32), seg_len=np.asarray(length, np.int32),
                seg_boot=np.asarray(boot, np.int32), executed=executed, gamma=GAMMA, lam=LAM)


def case_ids():
    """-> [(E, T, bars, variant)] of every case."""
    out = []
    for (E, T), bars in itertools.product(SHAPES, BARS):
        for variant in ((0, 1) if E * T == 1 else (0,)):
            out.append((E, T, bars, variant))
    return out


def case_name(cid):
    E, T, bars, variant = cid
    return "%dx%d-rho%g-c%g%s" % (E, T, bars[0], bars[1], "-b" if variant else "")


_CASES = {}


def case(cid):
    """The case of this id, built once and not to be modified."""
    if cid not in _CASES:
        _CASES[cid] = build(cid[0], cid[1], cid[2], cid[3])
    return _CASES[cid]


def weights64(c):
    """numpy's weights exp(float64(lp_now) - float64(lp_old)), [E, T + 1]."""
    return np.exp(c["lp_now"].astype(np.float64) - c["lp_old"].astype(np.float64))


def successor(c, e, s, n, kind, read_behind_done, with_final=True):
    """The value behind the segment's last step: a truncated segment's final value; else the table slot behind it -- which the segment kernels' rule
    (read_behind_done = False) replaces by 0.0 behind a terminal last step."""
    last = s + n - 1
    if kind == TRUNCATED and with_final:
        return float(c["final_values"][e, last])
    if not read_behind_done and c["dones"][e, last] != 0.0:
        return 0.0
    return float(c["values"][e, last + 1])


def deltas(c, e, s, n, kind, read_behind_done, with_final=True):
    """delta_t = (r_t + ((1 - done_t) gamma) V_{t+1}) - V_t in this order (gae_delta), float64 [n]."""
    v = c["values"][e].astype(np.float64)
    out = np.empty(n)
    for i in range(n):
        t = s + i
        vnext = successor(c, e, s, n, kind, read_behind_done, with_final) if i == n - 1 else float(v[t + 1])
        nonterm = 1.0 - float(c["dones"][e, t])
        out[i] = (float(c["rewards"][e, t]) + (nonterm * c["gamma"]) * vnext) - float(v[t])
    return out


# ---- reference (a): the recurrence, in the kernel's operation order ----
def recurrence(delta, w, gl, rho_bar, c_bar):
    """-> (D, A), float64 [n]."""
    n = len(delta)
    D, A = np.empty(n), np.empty(n)
    Dn = 0.0
    for t in range(n - 1, -1, -1):
        wt, dt = float(w[t]), float(delta[t])
        cw = c_bar if wt > c_bar else wt
        rw = rho_bar if wt > rho_bar else wt
        A[t] = (gl * Dn) + dt
        D[t] = ((gl * cw) * Dn) + (rw * dt)
        Dn = D[t]
    return D, A


# ---- reference (b): the forward definition, on its own ----
def forward_definition(delta, w, gamma, lam, rho_bar, c_bar):
    """vs_t - V_t = sum_k gamma^k (prod_{i<k} lam c_{t+i}) rho_{t+k} delta_{t+k} with c = min(c_bar, w), rho = min(rho_bar, w); A_t = delta_t + gamma lam (vs_{t+1} -
    V_{t+1}) -> (vs - V, A), float64 [n]."""
    delta, w = np.asarray(delta, np.float64), np.asarray(w, np.float64)
    n = len(delta)
    rho, c = np.minimum(rho_bar, w), np.minimum(c_bar, w)
    dv = np.zeros(n + 1)
    for t in range(n):
        total = 0.0
        for k in range(n - t):
            total += gamma ** k * np.prod(lam * c[t:t + k]) * rho[t + k] * delta[t + k]
        dv[t] = total
    return dv[:n], delta + gamma * lam * dv[1:]


def wave_sum(x):
    """The sum of x in the order the finish kernels form it: 64 lanes add their elements lane, lane + 64, .. from 0.0 in ascending order, then the lanes meet in an
    xor butterfly (offsets 32, 16, .. 1; every lane ends with the same sum)."""
    x = np.asarray(x, np.float64)
    p = np.zeros(64)
    for i in range(0, len(x), 64):
        chunk = x[i:i + 64]
        p[:len(chunk)] = p[:len(chunk)] + chunk
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        p = p + p[lanes ^ o]
    return float(p[0])


def reference(c, w, read_behind_done, normalize, with_final=True):
    """Reference (a) over the whole case from weights w [E, T + 1] -> dict of float64 [E, T] arrays raw (A), returns (D + V), adv (normalised), NaN where no executed
    segment has a step.  The normalisation is train.py:176-177's -- (A - mean) / (std + 1e-8), population std -- per segment, or with normalize = 1 over all steps of
    all executed segments, with every sum in the finish kernels' documented order (wave_sum; the batch sums: per-segment partials, bad descriptors adding 0.0, then
    wave_sum over the descriptors)."""
    E, T = c["E"], c["T"]
    gl = c["gamma"] * c["lam"]
    raw, ret, adv = (np.full((E, T), np.nan) for _ in range(3))
    n_desc = len(c["seg_row"])
    part = np.zeros(n_desc)
    for i, (e, s, n, kind) in enumerate(c["segs"]):
        D, A = recurrence(deltas(c, e, s, n, kind, read_behind_done, with_final), w[e, s:s + n], gl, c["rho_bar"], c["c_bar"])
        raw[e, s:s + n] = A
        ret[e, s:s + n] = D + c["values"][e, s:s + n].astype(np.float64)
        total = wave_sum(A)
        part[i] = total
        if not normalize:
            mean = total / float(n)
            sd = np.sqrt(wave_sum((A - mean) * (A - mean)) / float(n))
            adv[e, s:s + n] = (A - mean) / (sd + 1e-8)
    if normalize:
        count = float(sum(n for _, _, n, _ in c["segs"]))
        mean = wave_sum(part) / count
        part2 = np.zeros(n_desc)
        for i, (e, s, n, _) in enumerate(c["segs"]):
            A = raw[e, s:s + n]
            part2[i] = wave_sum((A - mean) * (A - mean))
        sd = np.sqrt(wave_sum(part2) / count)
        for e, s, n, _ in c["segs"]:
            adv[e, s:s + n] = (raw[e, s:s + n] - mean) / (sd + 1e-8)
    return dict(raw=raw, returns=ret, adv=adv)


def both_sides(cases):
    """For a group of cases with the same bars: per finite positive bar, is there an executed step with a weight above it and one below -> {bar name: (above, below)}."""
    out = {}
    for name in ("rho_bar", "c_bar"):
        bar = cases[0][name]
        if not np.isfinite(bar):
            continue
        ws = np.concatenate([weights64(c)[e, s:s + n] for c in cases for e, s, n, _ in c["segs"]])
        out[name] = (bool((ws > bar).any()), bool((ws < bar).any()))
    return out
