"""The VAE elementwise kernels (csrc/elementwise.hip) off the one shape each is tested at elsewhere: the cases, their float64 references and, where a bound is tied
to the reference's own arithmetic, a numpy float32 restatement of the reference formula (test infrastructure; used by test_vae_elementwise_cases_host.py, which asserts
on the CPU what every case claims about itself, and by test_w_vae_elementwise_gpu.py, which runs the kernels).  Everything is built from fixed seeds; nothing searches.

Bounds (each derived here or taken from the test that already uses it):
  recon, kinds 0 / 2   dlogits tols(dt, max|ref|) (tests/hip_helpers.py); a chunk's partial sum 2e-6 x sum|per-element loss| + 1e-6
  recon, kind 1        tied to the reference: d32 = distance of the float32 restatement from float64 on the same elements (max over the tensor for dlogits, summed
                       over the chunk for the loss); the kernel may be 4 x d32 + the tols() atol away (v_exp / v_log / v_rcp stand in for libm).  Only |x| <= 8: the
                       reference's own log(1e-10 + 1 - s) is -inf / NaN once s rounds to 1 in fp32 (x >= ~17); the kernel restates that faithfully (documented, not tested)
  fused dbias          1e-5 x sum|stored dlogits of the channel| against the float64 sum of the STORED dlogits (+ the 1.5 the buffer starts at)
  reparam              mean / logvar bitwise the float32 sum bias, slab 0, slab 1, ...; kl_row 1e-5 |ref| + 2^-20 sum_j(|1 + lv| + mu^2 + e^lv) (at most four
                       sequential adds per lane, a six-step butterfly, a few roundings per term); z / dheads tols(dt, max|ref|)
  finalize             out2 1e-5 rel (derived rounding bound (ceil(n / 4096) + 14) 2^-24 is below it); dbias 1e-5 x sum|column|
  split round trip     2^-17 |x| (lo carries 8 more bits) where lo's 8 bits are all above the smallest bf16 step, 2^-133: |x| >= 2^-117.  Below that a pair of bf16 numbers
                       cannot hold the value (fp32 goes down to 2^-149): there the error is at most half the smallest bf16 step, 2^-134."""
import functools

import numpy as np
import torch

from hip_helpers import rounded, split_decode, split_encode

F32 = np.float32
INV_B = 1.0 / 16.0                      # inv_batch of every loss case: a global batch of 16 (data parallelism), not the local row count

# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. reconstruction loss
# ---------------------------------------------------------------------------------------------------------------------------------------
BCE_PER_THREAD, BCE_CHUNK = 24, 256 * 24
RECON_SHAPES = [(1, 23), (1, 24), (3, 30), (2, 6144), (2, 6150), (2, 6168)]
RECON_KIND_R = [(0, 100.0), (0, 6.0), (2, 100.0), (2, 6.0), (1, 8.0)]
RECON_ALIGN_SHAPES = [(2, 6168), (3, 30)]
RECON_BIAS_SHAPES = [(3, 30), (2, 6150), (2, 6168)]
RECON_CHANNELS = (1, 2, 3)
RECON_FRAMES = 4                        # rows of the label table
RECON_LOSS_REL, RECON_LOSS_ABS = 2e-6, 1e-6
RECON_K1_FACTOR, RECON_K1_D32_MAX = 4.0, 1e-3
DBIAS_START, DBIAS_REL = 1.5, 1e-5


def recon_frame_idx(B, which):
    """which: 'none' (rows 0 .. B-1), 'rep' (a repeated index), 'align' (row 0: 16-byte aligned in the padded tables; row 1: not)."""
    if which == "none":
        return None
    if which == "rep":
        return np.array([3, 1, 1][:B] if B != 2 else [3, 3], np.int32)
    return np.array([0, 1, 1][:B], np.int32)


def recon_chunks(P):
    return (P + BCE_CHUNK - 1) // BCE_CHUNK


def sigmoid64(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def recon_ref64(x, y, kind, inv_b=INV_B):
    """float64: per-element loss and d(sum loss x inv_b) / dx of vae/models.py:11-22 (bce, bce_v2, mse)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    s = sigmoid64(x)
    if kind == 0:
        per = np.maximum(x, 0.0) - x * y + np.log1p(np.exp(-np.abs(x)))
        g = s - y
    elif kind == 1:
        per = -(y * np.log(1e-10 + s) + (1.0 - y) * np.log(1e-10 + 1.0 - s))
        g = (-y / (1e-10 + s) + (1.0 - y) / (1e-10 + 1.0 - s)) * s * (1.0 - s)
    else:
        per = (y - s) ** 2
        g = 2.0 * (s - y) * s * (1.0 - s)
    return per, g * inv_b


def recon_ref32(x, y, kind, inv_b=INV_B):
    """The same formulas with every operation in numpy float32, written as the reference writes them (tf.nn.sigmoid_cross_entropy_with_logits for kind 0,
    tf.nn.sigmoid = 1 / (1 + exp(-x)) and the 1e-10 guards left to right for kind 1)."""
    x, y = np.asarray(x, F32), np.asarray(y, F32)
    one, guard = F32(1.0), F32(1e-10)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        s = one / (one + np.exp(-x))
        if kind == 0:
            per = np.maximum(x, F32(0)) - x * y + np.log1p(np.exp(-np.abs(x)))
            g = s - y
        elif kind == 1:
            per = -(y * np.log(guard + s) + (one - y) * np.log(guard + one - s))
            g = (-y / (guard + s) + (one - y) / (guard + one - s)) * s * (one - s)
        else:
            d = y - s
            per = d * d
            g = F32(2.0) * (s - y) * s * (one - s)
        return per, g * F32(inv_b)


def chunk_sums(per):
    """[B, P] float64 -> [B, chunks] sums over the kernel's chunks of 6144 elements."""
    B, P = per.shape
    nch = recon_chunks(P)
    pad = np.zeros((B, nch * BCE_CHUNK), np.float64)
    pad[:, :P] = per
    return pad.reshape(B, nch, BCE_CHUNK).sum(2)


@functools.lru_cache(maxsize=None)
def recon_data(B, P, kind, R):
    """logits uniform in [-R, R] with +R, -R, 0.0 and -0.0 planted once each; RECON_FRAMES frames of random bytes with 0 and 255 forced into every frame."""
    rng = np.random.RandomState(1000 * kind + 7 * P + B + int(R))
    logits = rng.uniform(-R, R, (B, P)).astype(F32)
    pos = rng.permutation(B * P)[:4]
    logits.reshape(-1)[pos] = np.array([R, -R, 0.0, -0.0], F32)
    frames = rng.randint(0, 256, (RECON_FRAMES, P)).astype(np.uint8)
    cols = rng.permutation(P)[:2]
    frames[:, cols[0]] = 0
    frames[:, cols[1]] = 255
    for a in (logits, frames):
        a.setflags(write=False)
    return {"logits": logits, "bytes": frames, "planted": pos}


def unit_labels(frames_u8):
    return frames_u8.astype(F32) / F32(255)            # the value the reference's host preprocessing produces (vae/train_vae.py:15-18)


def padded_table(rows, stride, fill):
    """[n, P] -> a flat table whose row r starts at r * stride (stride > P: the gap holds `fill`)."""
    n, Pn = rows.shape
    t = np.full(n * stride, fill, rows.dtype)
    for r in range(n):
        t[r * stride:r * stride + Pn] = rows[r]
    return t


@functools.lru_cache(maxsize=None)
def recon_reference(B, P, kind, R, dt_name, which_idx):
    """Everything the GPU test compares against, for the logits as the storage type holds them."""
    from hip_helpers import DT
    td = DT[dt_name][1]
    d = recon_data(B, P, kind, R)
    idx = recon_frame_idx(B, which_idx)
    y = unit_labels(d["bytes"])[np.arange(B) if idx is None else idx]
    x = rounded(d["logits"].copy(), td).numpy()
    per, g = recon_ref64(x, y, kind)
    per32, g32 = recon_ref32(x.astype(F32), y, kind)
    out = {"x": x, "y": y, "per": per, "g": g, "chunks": chunk_sums(per), "abs_chunks": chunk_sums(np.abs(per)),
           "d32_g": float(np.max(np.abs(g32.astype(np.float64) - g))), "d32_per_max": float(np.max(np.abs(per32.astype(np.float64) - per))),
           "d32_chunks": chunk_sums(np.abs(per32.astype(np.float64) - per)), "chunks32": chunk_sums(per32.astype(np.float64))}
    return out


def recon_conditions_met(B, P, kind, R, dt_name="f32", which_idx="none"):
    """What a recon case claims about itself (asserted on the CPU): finite reference, the planted logits and labels present, the float32 restatement inside the
    bound the kernel is held to (kinds 0 / 2) or its distance finite and below 1e-3 (kind 1)."""
    d, r = recon_data(B, P, kind, R), recon_reference(B, P, kind, R, dt_name, which_idx)
    flat = d["logits"].reshape(-1)
    planted = flat[d["planted"]]
    ok = bool(np.isfinite(r["per"]).all() and np.isfinite(r["g"]).all())
    ok &= planted[0] == F32(R) and planted[1] == F32(-R) and planted[2] == 0 and not np.signbit(planted[2]) and planted[3] == 0 and bool(np.signbit(planted[3]))
    ok &= bool(np.abs(flat).max() <= R)
    ok &= all((d["bytes"][f] == 0).any() and (d["bytes"][f] == 255).any() for f in range(RECON_FRAMES))
    if kind == 1:
        ok &= bool(np.isfinite(r["d32_g"]) and np.isfinite(r["d32_per_max"]) and r["d32_g"] < RECON_K1_D32_MAX and r["d32_per_max"] < RECON_K1_D32_MAX)
    else:
        ok &= bool((np.abs(r["chunks32"] - r["chunks"]) <= RECON_LOSS_REL * r["abs_chunks"] + RECON_LOSS_ABS).all())
    return bool(ok)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. reparameterisation + KL
# ---------------------------------------------------------------------------------------------------------------------------------------
REPARAM_SHAPES = [(1, 1, 1, 1), (4, 63, 8, 8), (5, 64, 9, 9), (9, 65, 16, 17), (3, 200, 17, 1)]          # (B, Z, slabs of heads, slabs of dz)
REPARAM_NEAR_PRIOR = (5, 64, 9, 9)
REPARAM_WIDE_SHAPES = [(5, 64, 9, 9), (9, 65, 16, 17), (4, 63, 33, 33)]
REPARAM_BETA = 1.5
KL_REL, KL_SUM_EPS = 1e-5, 2.0 ** -20
FLOOR_GAP = 2e-3                        # the planted rows sit this far (relative) on either side of the floor
FLOOR_GAP_MIN = 1e-3


@functools.lru_cache(maxsize=None)
def reparam_data(B, Z, ns, nd, near_prior=False):
    """heads [ns, B, 2Z] whose slab sum (+ bias) is mu in +-3, logvar in [-6, 4] (near_prior: both of size 1e-3); eps N(0, 1); dz slabs N(0, 1).
    B >= 2 and not near_prior: row 1 is row 0 with mu scaled so that its KL is 2 FLOOR_GAP below row 0's; `floor` lies between the two."""
    rng = np.random.RandomState(100 * B + Z + 1000 * ns + (7 if near_prior else 0))
    size = 1e-3 if near_prior else 1.0
    mu = rng.uniform(-3, 3, (B, Z)) * size
    lv = (rng.uniform(-6, 4, (B, Z)) if not near_prior else rng.uniform(-1, 1, (B, Z)) * size)
    floor = None
    if B >= 2 and not near_prior:
        kl0 = 0.5 * np.sum(mu[0] ** 2 + np.exp(lv[0]) - 1.0 - lv[0])
        t2 = 1.0 - 2 * FLOOR_GAP * kl0 / (0.5 * np.sum(mu[0] ** 2))
        assert t2 > 0.25, "row 0's KL is not carried by mu: cannot plant row 1 below it"
        mu[1], lv[1] = np.sqrt(t2) * mu[0], lv[0]
    bm, bl = rng.randn(Z) * 0.1 * size, rng.randn(Z) * 0.1 * size
    heads = rng.randn(ns, B, 2 * Z) * 0.3 * size
    heads[0, :, :Z] = mu - bm - heads[1:, :, :Z].sum(0)
    heads[0, :, Z:] = lv - bl - heads[1:, :, Z:].sum(0)
    out = {"heads": heads.astype(F32), "bm": bm.astype(F32), "bl": bl.astype(F32), "eps": rng.randn(B, Z).astype(F32), "dzs": rng.randn(nd, B, Z).astype(F32)}
    mean32, logvar32 = slab_sum32(out["heads"], out["bm"], out["bl"])
    kl = kl_rows64(mean32, logvar32)
    if B >= 2 and not near_prior:
        floor = float(F32(kl[0] * (1.0 - FLOOR_GAP)))
    out.update(mean32=mean32, logvar32=logvar32, floor=floor)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def slab_sum32(heads, bm, bl):
    """The kernel's contract: float32, bias first, then slab 0, 1, 2, ... (both U variants)."""
    Z = bm.size
    mu = np.broadcast_to(bm, heads.shape[1:2] + (Z,)).astype(F32).copy()
    lv = np.broadcast_to(bl, heads.shape[1:2] + (Z,)).astype(F32).copy()
    for s in range(heads.shape[0]):
        mu = (mu + heads[s, :, :Z]).astype(F32)
        lv = (lv + heads[s, :, Z:]).astype(F32)
    return mu, lv


def dz_sum32(dzs):
    dz = np.zeros(dzs.shape[1:], F32)
    for s in range(dzs.shape[0]):
        dz = (dz + dzs[s]).astype(F32)
    return dz


def kl_rows64(mu, lv):
    mu, lv = np.asarray(mu, np.float64), np.asarray(lv, np.float64)
    return -0.5 * np.sum(1.0 + lv - mu * mu - np.exp(lv), axis=1)


def kl_rows32(mu, lv):
    """float32 restatement of the row sum: terms and a sequential sum, every operation rounded to float32."""
    mu, lv = np.asarray(mu, F32), np.asarray(lv, F32)
    t = (((F32(1.0) + lv).astype(F32) - (mu * mu).astype(F32)).astype(F32) - np.exp(lv).astype(F32)).astype(F32)
    acc = np.zeros(mu.shape[0], F32)
    for j in range(mu.shape[1]):
        acc = (acc + t[:, j]).astype(F32)
    return (F32(-0.5) * acc).astype(F32)


def kl_bound(mu, lv, ref):
    mu, lv = np.asarray(mu, np.float64), np.asarray(lv, np.float64)
    return KL_REL * np.abs(ref) + KL_SUM_EPS * np.sum(np.abs(1.0 + lv) + mu * mu + np.exp(lv), axis=1)


def reparam_ref64(d, kl_floor, inv_b=INV_B, beta=REPARAM_BETA, sample=True):
    """float64 autograd over the float32 inputs: mean, logvar, z, kl rows and d loss / d [mean | logvar] for loss = sum(z x dz) + beta x inv_b x sum_b max(kl_b, floor)."""
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))                       # noqa: E731
    Z = d["bm"].size
    h = t(d["heads"]).sum(0)
    mu = (h[:, :Z] + t(d["bm"])).requires_grad_(True)
    lv = (h[:, Z:] + t(d["bl"])).requires_grad_(True)
    z = mu + torch.exp(0.5 * lv) * t(d["eps"]) if sample else mu + 0.0 * lv
    kl = -0.5 * (1 + lv - mu * mu - lv.exp()).sum(1)
    klc = torch.where(kl < kl_floor, torch.full_like(kl, kl_floor), kl) if kl_floor > 0 else kl
    ((z * t(d["dzs"]).sum(0)).sum() + beta * inv_b * klc.sum()).backward()
    return {"mean": mu.detach().numpy(), "logvar": lv.detach().numpy(), "z": z.detach().numpy(), "kl": kl.detach().numpy(),
            "dheads": torch.cat([mu.grad, lv.grad], 1).numpy()}


def reparam_conditions_met(B, Z, ns, nd, near_prior=False):
    d = reparam_data(B, Z, ns, nd, near_prior)
    r = reparam_ref64(d, 0.0)
    ok = all(bool(np.isfinite(v).all()) for v in r.values())
    if near_prior:
        ok &= bool(np.abs(r["mean"]).max() < 5e-3 and np.abs(r["logvar"]).max() < 5e-3)
    else:
        ok &= bool(np.abs(r["mean"]).max() <= 3.001 and r["logvar"].max() <= 4.001 and r["logvar"].min() >= -6.001)
    kl32 = kl_rows32(d["mean32"], d["logvar32"]).astype(np.float64)
    ok &= bool((np.abs(kl32 - r["kl"]) <= kl_bound(r["mean"], r["logvar"], r["kl"])).all())
    if d["floor"] is not None:
        gap = (r["kl"] - d["floor"]) / d["floor"]
        ok &= bool(gap[0] >= FLOOR_GAP_MIN and gap[1] <= -FLOOR_GAP_MIN and (np.abs(gap) >= FLOOR_GAP_MIN).all() and gap[0] < 4 * FLOOR_GAP and gap[1] > -4 * FLOOR_GAP)
    return bool(ok)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. loss finalisation
# ---------------------------------------------------------------------------------------------------------------------------------------
FIN_N_PARTIAL = [1, 1023, 1024, 1025, 3072, 3073, 4097, 13001]
FIN_B = [1, 1024, 1025, 2049]
FIN_N_BIAS = [1, 1024, 1025, 2049]
FIN_OUT_REL, FIN_DBIAS_REL = 1e-5, 1e-5


def fin_derived_bound(n):
    """Relative rounding bound of the one-block sum of n positive values: ceil(n / 4096) sequential adds per lane, 2 to join the four accumulators, a ten-step tree, the scale."""
    return (-(-n // 4096) + 14) * 2.0 ** -24


@functools.lru_cache(maxsize=None)
def fin_data(n_partial, B, kl_floor, n_bias):
    rng = np.random.RandomState(n_partial + 31 * B + n_bias)
    partial = rng.uniform(0.5, 200.0, n_partial).astype(F32)
    kl = rng.uniform(0.1, 2.0, B).astype(F32)
    if kl_floor == 0.0:
        kl[::3] = -kl[::3] * F32(0.25)                 # negative rows: with kl_floor == 0 nothing is clamped, they count as they are
    bp = None
    if n_bias:
        bp = rng.randn(n_bias, 4).astype(F32)
        bp[:, 3] = np.nan                              # the fourth column is padding: it must not reach dbias
    for a in (partial, kl, bp):
        if a is not None:
            a.setflags(write=False)
    return {"partial": partial, "kl": kl, "bpart": bp}


def fin_ref64(d, kl_floor, B, inv_b):
    recon = d["partial"].astype(np.float64).sum() * inv_b
    k = d["kl"].astype(np.float64)
    kl = (np.maximum(k, kl_floor) if kl_floor > 0 else k).sum() * inv_b
    out = {"recon": recon, "kl": kl}
    if d["bpart"] is not None:
        col = d["bpart"][:, :3].astype(np.float64)
        out["dbias"], out["dbias_abs"] = col.sum(0), np.abs(col).sum(0)
    return out


def fin_conditions_met(n_partial, B, kl_floor, n_bias):
    d = fin_data(n_partial, B, kl_floor, n_bias)
    r = fin_ref64(d, kl_floor, B, 1.0 / B)
    ok = np.isfinite(r["recon"]) and np.isfinite(r["kl"]) and (d["partial"] > 0).all() and fin_derived_bound(n_partial) < FIN_OUT_REL
    ok &= (d["kl"] < 0).any() if kl_floor == 0.0 else (d["kl"] > 0).all() and ((d["kl"] < kl_floor).any() or B == 1)
    ok &= abs(r["kl"]) > 0.05 * np.abs(d["kl"]).astype(np.float64).sum() / B                # no cancellation: a relative bound on the KL mean means something
    if n_bias:
        ok &= np.isfinite(r["dbias"]).all() and np.isnan(d["bpart"][:, 3]).all()
    return bool(ok)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. Adam
# ---------------------------------------------------------------------------------------------------------------------------------------
ADAM_N = [1, 3, 4, 5, 1027, 2048 * 256 * 4 + 1027]
ADAM_PLANTED_G = np.array([0.0, 1e20, 1e-42, -0.0], F32)        # g = 0 on m = v = 0; g x g overflows; a denormal; negative zero
ADAM_PAD = 3.25


@functools.lru_cache(maxsize=None)
def adam_data(n):
    """p, m, v, g of the existing bit-exactness test, with the planted gradients at the head (vector body) and, from n = 8 on, again at the tail."""
    rng = np.random.RandomState(n % 100003)
    p, g = rng.randn(n).astype(F32), (rng.randn(n) * 10 ** rng.uniform(-6, 1, n)).astype(F32)
    m, v = (rng.randn(n) * 0.1).astype(F32), (rng.rand(n) * 0.01).astype(F32)
    k = min(n, 4)
    g[:k] = ADAM_PLANTED_G[:k]
    m[0] = v[0] = 0.0
    if n >= 8:
        g[n - 4:] = ADAM_PLANTED_G
        m[n - 4] = v[n - 4] = 0.0
    for a in (p, m, v, g):
        a.setflags(write=False)
    return p, m, v, g


def adam_alpha(step=3, lr=1e-4):
    return F32(lr * np.sqrt(1 - 0.999 ** step) / (1 - 0.9 ** step))


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. split-K finish, uint8 -> [0, 1]
# ---------------------------------------------------------------------------------------------------------------------------------------
SPLITK_SHAPES = [(1, 4), (3, 20), (5, 1028), (37, 64)]
SPLITK_NSPLIT = [1, 2, 7]
U8_N = [1, 15, 16, 17, 4099, 2048 * 256 * 16 + 5]


def tiny_positive(dt_name):
    """The smallest positive value of a storage type: fp32 2^-149; bf16 and split storage (hi half 0x0001) 2^-133."""
    return F32(2.0 ** -149) if dt_name == "f32" else F32(2.0 ** -133)


@functools.lru_cache(maxsize=None)
def splitk_data(M, N, nsplit, dt_name):
    rng = np.random.RandomState(M * 131 + N + nsplit)
    slabs = rng.randn(nsplit, M, N).astype(F32)
    bias = rng.randn(N).astype(F32)
    mask = (rng.rand(M, N) < 0.6).astype(F32)
    planted = np.array([0.0, -0.0, -1.0, np.nan, tiny_positive(dt_name)], F32)
    k = min(M * N, planted.size)
    mask.reshape(-1)[:k] = planted[:k]
    if k < planted.size:                               # (1, 4): the tiny positive entry takes the place of the negative one
        mask.reshape(-1)[2] = planted[4]
    for a in (slabs, bias, mask):
        a.setflags(write=False)
    return slabs, bias, mask


def splitk_ref32(slabs, bias, relu, mask):
    """float32: slabs in order, + bias, max(., 0), then the mask (only an entry that compares > 0 lets the value through).  No product: nothing to contract."""
    s = slabs[0].copy()
    for k in range(1, slabs.shape[0]):
        s = (s + slabs[k]).astype(F32)
    if bias is not None:
        s = (s + bias[None, :]).astype(F32)
    if relu:
        s = np.maximum(s, F32(0))
    if mask is not None:
        with np.errstate(invalid="ignore"):
            s = np.where(mask > 0, s, F32(0))
    return s.astype(F32)


def u8_input(n):
    """Every byte value 0 .. 255 cycled, each cycle of 256 starting one value later: from n = 4096 on each value meets each of the 16 lane positions."""
    i = np.arange(n, dtype=np.int64)
    return ((i + i // 256) % 256).astype(np.uint8)


def u8_conditions_met(n=4099):
    b = u8_input(n)
    seen = np.zeros((256, 16), bool)
    seen[b, np.arange(n) % 16] = True
    return bool(seen.all())


# ---------------------------------------------------------------------------------------------------------------------------------------
# 6. sigmoid, range check, casts, column sums
# ---------------------------------------------------------------------------------------------------------------------------------------
BIG_N = 2048 * 256 + 3
SIGMOID_N = [1, 1000, BIG_N]
SIGMOID_PLANTED = np.array([-100.0, 100.0, 0.0, -0.0, 20.0, -20.0], F32)
RANGE_N = [1, 5000, BIG_N]
COLSUM_SHAPES = [(40, 12), (40, 250), (1000, 64)]
SPLIT_RT_REL, SPLIT_RT_ABS, SPLIT_RT_FROM = 2.0 ** -17, 2.0 ** -134, 2.0 ** -117


def sigmoid_input(n):
    x = (np.random.RandomState(n % 9973).randn(n) * 5).astype(F32)
    k = min(n, SIGMOID_PLANTED.size)
    x[:k] = SIGMOID_PLANTED[:k]
    return x


def _bits(u):
    return np.array(u, np.uint32).view(F32)


def cast_values():
    """Exact ties both ways, the largest fp32 below the bf16 overflow point and the first that rounds to infinity, denormals, +-0, +-inf, NaN, each with both signs."""
    pos = np.concatenate([
        np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -23, 1.0 + 2.0 ** -8 - 2.0 ** -23, 3.0e38, 1.0, 0.1, 1e-30, 2.0 ** -126, 2.0 ** -117], F32),
        _bits([0x7f7f7fff, 0x7f7f8000, 0x7f7fffff, 0x7f000000, 0x7effffff]),                   # around the bf16 overflow point; 2^127 and the fp32 just below it
        _bits([0x00000001, 0x00008000, 0x00010000, 0x00018000, 0x00010001, 0x007fffff, 0x000002c9]),   # denormals (bf16 step 2^-133 = 0x00010000), ties among them
        np.array([0.0, np.inf], F32)])
    v = np.concatenate([pos, -pos, np.array([np.nan], F32)]).astype(F32)
    return v


def cast_input(n, split=False):
    v = cast_values()
    if split:
        v = v[np.abs(v) < 2.0 ** 127]                 # drops the NaN too
    x = (np.random.RandomState(n % 9973).randn(n) * 10 ** np.random.RandomState(5).uniform(-30, 30, n)).astype(F32)
    k = min(n, v.size)
    x[:k] = v[:k]
    return x


def cast_conditions_met():
    v = cast_values()
    b = torch.from_numpy(v).to(torch.bfloat16).view(torch.int16).numpy().astype(np.uint16)
    one = lambda x: int(torch.tensor([x], dtype=torch.float32).to(torch.bfloat16).view(torch.int16).item()) & 0xffff        # noqa: E731
    ok = one(1.0 + 2.0 ** -8) == 0x3f80 and one(1.0 + 3 * 2.0 ** -8) == 0x3f82                 # ties: to even, down and up
    ok &= one(float(_bits([0x7f7f7fff])[0])) == 0x7f7f and one(float(_bits([0x7f7f8000])[0])) == 0x7f80
    ok &= bool(np.isnan(v).sum() == 1 and np.isinf(v).sum() == 2 and (np.signbit(v) & (v == 0)).sum() == 1 and b.size == v.size)
    s = cast_input(4096, split=True)
    ok &= bool(np.isfinite(s).all() and (np.abs(s) < 2.0 ** 127).all())
    rt = split_decode(split_encode(s))                                                         # the host restatement itself keeps the round-trip bound
    ok &= bool((np.abs(rt - s.astype(np.float64)) <= split_round_trip_bound(s)).all())
    return bool(ok)


def split_round_trip_bound(x):
    a = np.abs(np.asarray(x, np.float64))
    return np.where(a >= SPLIT_RT_FROM, SPLIT_RT_REL * a, SPLIT_RT_ABS)


def range_bad_values(lo, hi):
    lo, hi = F32(lo), F32(hi)
    return [("hi+ulp", np.nextafter(hi, F32(np.inf))), ("lo-ulp", np.nextafter(lo, F32(-np.inf))), ("nan", F32(np.nan)), ("+inf", F32(np.inf))]


def range_input(n, lo=0.0, hi=1.0):
    x = np.random.RandomState(n % 9973).uniform(lo, hi, n).astype(F32)
    x = np.clip(x, F32(lo), F32(hi))
    if n >= 4:
        x[1], x[n - 2] = lo, hi                        # the bounds themselves pass
    return x


def colsum_input(M, N):
    return np.random.RandomState(M + N).randn(M, N).astype(F32)
