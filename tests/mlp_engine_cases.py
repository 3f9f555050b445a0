"""Cases, float64 references and route predicates for test_zzzzzzzz_mlp_engine_shapes_gpu.py (test infrastructure; imports no GPU): the MlpVAE ENGINE
(csrc/mlp_engine.hip: the parameter layout, the workspace carving, splitk_slabs and the slab region, the routing of every filter gradient, the two-stream backward
pass with its deferred slab sums, Adam's kernel table) OFF the one family of models every other test builds (38400 -> (512, 256) or (64, 32) -> 64 latents).

A case = source shape, target shape, encoder sizes, decoder sizes, z_dim, batch.  Parameters are vo.init_mlp_vae_params(seed = id) with 0.05 x N(0, 1) biases from
RandomState(100 + id); inputs are drawn from RandomState(3000 + id + shift) in the order source bytes, target bytes, eps; float tables are byte / 255 in float32.

References: the oracle (oracle/vae_oracle.py) in float64, once per (case, loss) and cached; walk() is the same network stated op by op in numpy float64 -- it gives
the ReLU pre-activations (the margin condition), the deliberately mis-stated references of the host test, and, with bf16 stores, the CPU stand-in for the bf16 engine;
layer_report() is Part B: each op recomputed in float64 from the tensors the engine ITSELF stored, against derived bounds.

route() restates the HOST gates that choose the kernels of a step (mlp_engine.hip splitk_slabs; conv_ops.hip mi_gemm_bias_act's tall-K gate, mi_gemm_wgrad_bias_set,
wgrad_splits) at the default knobs; STATED is the written-down table of what each row is stated to take.  test_mlp_engine_cases_host.py asserts that they agree."""
import collections

import numpy as np
import torch

from oracle import vae_oracle as vo

Case = collections.namedtuple("Case", "id src tgt enc dec z B shift why")

CASES = [
    Case(1, (2, 2, 2), (2, 2, 2), (8,), (8,), 8, 1, 0, "smallest legal model; every width one bf16 vector; one hidden layer per side; batch 1"),
    Case(2, (4, 6, 3), (4, 6, 3), (40, 24, 16, 8), (8, 16, 24, 40), 16, 5, 0, "four layers per side; ten kernels in Adam's table; nine deferred filter gradients"),
    Case(3, (8, 8, 3), (8, 8, 1), (64, 32, 16), (48,), 24, 33, 0, "3 + 1 layers; P != S; batch across the 32-row tiles; engine created at max_batch 4 and grown by ensure_batch"),
    Case(4, (32, 32, 4), (16, 16, 3), (64, 32), (32, 64), 32, 16, 0, "K = 4096 exactly gives 2 slabs; bf16 gives tall-K at N = 64; layer 0's filter gradient 4096 x 64 at the one-wave kernel's cap"),
    Case(5, (31, 33, 4), (4, 5, 1), (12,), (20,), 12, 3, 0, "fp32 only (4092, 12, 20 are multiples of 4, not 8); K just under the split threshold; row length with a tail in "
                                                            "mi_gather_rows_cast*; P under one loss chunk"),
    Case(6, (27, 19, 8), (27, 19, 8), (32,), (32,), 8, 2, 0, "K >= 4096 but no multiple of 128: one unsplit 4104-long reduction forward; unsplit over P in the output layer's input gradient"),
    Case(7, (56, 86, 8), (769, 8, 1), (32,), (16,), 16, 4, 0, "splitk_slabs walks 30 down to 7; N = 32 with 7 slabs is refused by tall-K and goes to gemm2 split-K; two loss chunks, "
                                                             "the second 8 elements long"),
    Case(8, (4, 4, 4), (4, 4, 4), (4224, 16), (16, 5120), 2048, 3, 500, "split-K inside the net: forward of enc[1] (K = 4224, 3 slabs) and of the output layer (K = 5120, 4 slabs); "
                                                                        "input gradients over N = 5120 (4 slabs, mask) and over 2 z = 4096 (2 slabs, mask); 2048 latents"),
    Case(9, (16, 16, 3), (16, 16, 3), (128, 128), (128, 256), 64, 48, 800, "bf16: every filter gradient on the one-wave kernel (B a multiple of 16; widths multiples of 64)"),
]
CREATE_BATCH = {3: 4}                      # case id -> max_batch the engine is created with (default: what init_session asks for, 128)
PRECISIONS = ("fp32", "bf16")
FP32_ONLY = (5,)
LOSS_KIND_CASES = (5, 7)                   # bce_v2 and mse with kl_tolerance > 0 and beta = 4
# kl_tolerance of those runs: between the rows' own KL / z (float64: case 5 0.266, 0.272, 0.401; case 7 0.204, 0.350, 0.352, 0.438), every row at least 15 % away
KL_TOLERANCE = {5: 0.33, 7: 0.28}
KL_CLAMPED = {5: [True, True, False], 7: [True, False, False, False]}
LOSS_KIND_BETA = 4.0
IDENTITY_CASES = (2, 4, 7, 8)              # Part C
SHORT_AFTER_LONG = {3: 5, 9: 16}           # Part C 6: case -> the short batch run behind the case's own
STREAM_CASES = (2, 8)                      # Part C 9
GUARD_CASES = (3, 7, 8)                    # Part D
RELU_MARGIN = 2e-5                         # of the layer's largest |pre-activation|: 20 x the fp32 oracle's own worst distance from float64
BCE_CHUNK = 256 * 24                       # elementwise.hip: elements per partial sum of the reconstruction loss


def by_id(i):
    return CASES[i - 1]


def S(c):
    return int(np.prod(c.src))


def P(c):
    return int(np.prod(c.tgt))


def precisions(c):
    return ("fp32",) if c.id in FP32_ONLY else PRECISIONS


def layer_name(side, i):
    return "vae/%s/dense" % side + ("_%d" % i if i else "")


def layers(c):
    """[(tag, TF name or '@heads', K, N)] in the engine's order: encoder layers, the heads as one [K, 2 z] product, decoder layers incl. the output layer."""
    out, k = [], S(c)
    for i, n in enumerate(c.enc):
        out.append(("enc%d" % i, layer_name("encoder", i), k, n))
        k = n
    out.append(("heads", "@heads", k, 2 * c.z))
    k = c.z
    for i, n in enumerate(c.dec + (P(c),)):
        out.append(("dec%d" % i, layer_name("decoder", i), k, n))
        k = n
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# route predicates: the host gates of csrc/mlp_engine.hip and of the launchers it calls, restated
# ---------------------------------------------------------------------------------------------------------------------------------------
SPLIT_K = 4096
DENSE_WGRAD_BLOCKS = 256                   # tuning.hip K_DENSE_WGRAD_BLOCKS


def splitk_slabs(K):
    """mlp_engine.hip splitk_slabs."""
    if K < SPLIT_K or K % 128 != 0:
        return 1
    ns = max(min(K // 1280, 32), 1)
    while ns > 1 and K % (ns * 128) != 0:
        ns -= 1
    return ns


def splitk_walk(K):
    """The slab counts the --ns loop of splitk_slabs tries, first to last."""
    if K < SPLIT_K or K % 128 != 0:
        return [1]
    ns = max(min(K // 1280, 32), 1)
    seen = [ns]
    while ns > 1 and K % (ns * 128) != 0:
        ns -= 1
        seen.append(ns)
    return seen


def split_kernel(precision, N, K, ns):
    """mi_gemm_bias_act with nsplit > 1 as the engine calls it (K-contiguous weights, raw fp32 slabs): tallk_kernel or the general split-K GEMM."""
    if ns <= 1:
        return "unsplit"
    if precision == "bf16" and N in (32, 64, 128) and K % (ns * 16) == 0 and ns % (4 // (N // 32)) == 0:
        return "tallk"
    return "gemm2"


def wgrad_splits(precision, M, Kc, N, target=DENSE_WGRAD_BLOCKS):
    """conv_ops.hip wgrad_splits: row splits of a first-generation filter-gradient launch."""
    BP = 16 if precision == "fp32" else 64
    gx, gy = (-(-Kc // 128) if Kc > 64 else 1), -(-N // 64)
    splits = max(target // (gx * gy), 1)
    mps = max(-(-(-(-M // splits)) // BP) * BP, BP)
    return -(-M // mps)


def wgrad_scratch_bytes(precision, M, K, N):
    """conv_ops.hip mi_gemm_wgrad_scratch_bytes."""
    splits = wgrad_splits(precision, M, K + 1, N)
    return splits * (((K + 1) * N + 3) // 4 * 4) * 4 if splits > 1 else 0


def wgrad_family(precision, M, K, N):
    """conv_ops.hip mi_gemm_wgrad_bias_set in its storing form at the default knobs."""
    bf16 = precision == "bf16"
    if bf16 and M >= 1 and K % 128 == 0 and N % 128 == 0 and (K // 128) * (N // 128) >= 256:
        return "dwg"
    if bf16 and M >= 16 and M % 16 == 0 and K % 64 == 0 and N % 64 == 0 and K * N <= 262144:
        return "dwgs"
    return "gen1.one_split" if wgrad_splits(precision, M, K + 1, N) == 1 else "gen1.slabs"


def loss_chunks(Pn):
    """elementwise.hip mi_recon_loss_chunks."""
    return -(-Pn // BCE_CHUNK)


def route(c, precision):
    """{'fwd': slabs per layer, 'fwd_kernel', 'dgrad': slabs per input gradient (None: the first encoder layer has none), 'dgrad_kernel', 'wgrad': family per layer,
    'row_splits': row splits of a gen-1 launch (1 elsewhere)} -- every list in layers() order."""
    r = {"fwd": [], "fwd_kernel": [], "dgrad": [], "dgrad_kernel": [], "wgrad": [], "row_splits": []}
    for j, (tag, _, K, N) in enumerate(layers(c)):
        ns = splitk_slabs(K)
        r["fwd"].append(ns)
        r["fwd_kernel"].append(split_kernel(precision, N, K, ns))
        if j == 0:
            r["dgrad"].append(None)
            r["dgrad_kernel"].append(None)
        else:                                              # x * W^T reduces over the layer's N into its K columns
            nd = splitk_slabs(N)
            r["dgrad"].append(nd)
            r["dgrad_kernel"].append(split_kernel(precision, K, N, nd))
        fam = wgrad_family(precision, c.B, K, N)
        r["wgrad"].append(fam)
        r["row_splits"].append(wgrad_splits(precision, c.B, K + 1, N) if fam.startswith("gen1") else 1)
    return r


def _u(n, v):
    return (v,) * n


O, SL, WS = "gen1.one_split", "gen1.slabs", "dwgs"
# What each row is stated to take (the issue's table, written down, not derived).  Per case: forward slabs per layer, input-gradient slabs per layer (None: layer 0),
# the kernel of every split product in bf16 (fp32: always the general split-K GEMM), the filter-gradient family per layer in fp32 and in bf16.
STATED = {
    1: dict(fwd=_u(4, 1), dgrad=(None, 1, 1, 1), split_bf16={}, wgrad_fp32=_u(4, O), wgrad_bf16=_u(4, O)),
    2: dict(fwd=_u(10, 1), dgrad=(None,) + _u(9, 1), split_bf16={}, wgrad_fp32=_u(10, O), wgrad_bf16=_u(10, O)),
    3: dict(fwd=_u(6, 1), dgrad=(None,) + _u(5, 1), split_bf16={}, wgrad_fp32=_u(6, SL), wgrad_bf16=_u(6, O)),
    4: dict(fwd=(2, 1, 1, 1, 1, 1), dgrad=(None,) + _u(5, 1), split_bf16={"fwd enc0": "tallk"}, wgrad_fp32=_u(6, O), wgrad_bf16=(WS, O, O, O, O, WS)),
    5: dict(fwd=_u(4, 1), dgrad=(None, 1, 1, 1), split_bf16={}, wgrad_fp32=_u(4, O), wgrad_bf16=None),
    6: dict(fwd=_u(4, 1), dgrad=(None, 1, 1, 1), split_bf16={}, wgrad_fp32=_u(4, O), wgrad_bf16=_u(4, O)),
    7: dict(fwd=(7, 1, 1, 1), dgrad=(None, 1, 1, 1), split_bf16={"fwd enc0": "gemm2"}, wgrad_fp32=_u(4, O), wgrad_bf16=_u(4, O)),
    8: dict(fwd=(1, 3, 1, 1, 1, 4), dgrad=(None, 1, 2, 1, 4, 1), split_bf16={"fwd enc1": "gemm2", "fwd dec2": "tallk", "dgrad heads": "gemm2", "dgrad dec1": "gemm2"},
            wgrad_fp32=_u(6, O), wgrad_bf16=_u(6, O)),
    9: dict(fwd=_u(6, 1), dgrad=(None,) + _u(5, 1), split_bf16={}, wgrad_fp32=_u(6, SL), wgrad_bf16=_u(6, WS)),
}


def stated_view(c, precision):
    """route() in STATED's form."""
    r = route(c, precision)
    tags = [t for t, _, _, _ in layers(c)]
    split = {}
    for kind in ("fwd", "dgrad"):
        for t, k in zip(tags, r[kind + "_kernel"]):
            if k not in (None, "unsplit"):
                split["%s %s" % (kind, t)] = k
    return tuple(r["fwd"]), tuple(r["dgrad"]), split, tuple(r["wgrad"])


def workspace_layout(c, precision, max_batch, with_optimizer=True):
    """mlp_engine.hip init_engine's carve with the guards off: ({region: byte offset}, total bytes)."""
    esz = 2 if precision == "bf16" else 4
    B, z, L = max_batch, c.z, layers(c)
    enc = [l for l in L if l[0].startswith("enc")]
    dec = [l for l in L if l[0].startswith("dec")]
    heads = [l for l in L if l[0] == "heads"][0]
    off, w = collections.OrderedDict(), [0]

    def reg(name, nbytes):
        off[name] = w[0]
        w[0] += (nbytes + 255) // 256 * 256

    reg("x", B * S(c) * esz)
    for i, l in enumerate(enc):
        reg("h%d" % i, B * l[3] * esz)
    reg("heads", B * 2 * z * 4)
    reg("mean", B * z * 4)
    reg("logvar", B * z * 4)
    reg("klrow", B * 4)
    reg("z", B * z * esz)
    for i, l in enumerate(dec):
        reg("d%d" % i, B * l[3] * esz)
    reg("partial", B * loss_chunks(P(c)) * 4)
    reg("out2", 16)
    slab = [0]

    def use(K, N):
        ns = splitk_slabs(K)
        if ns > 1:
            slab[0] = max(slab[0], ns * B * N * 4)

    for _, _, K, N in L:
        use(K, N)
    scr = 0
    if with_optimizer:
        for i, l in enumerate(dec):
            reg("gd%d" % i, B * l[3] * esz)
        reg("dz", B * z * 4)
        reg("dheads", B * 2 * z * esz)
        for i, l in enumerate(enc):
            reg("gh%d" % i, B * l[3] * esz)
        for j, (_, _, K, N) in enumerate(L):
            scr += (wgrad_scratch_bytes(precision, 1 << 20, K, N) + 255) // 256 * 256
            if j:
                use(N, K)
    reg("slab", slab[0] or 16)
    reg("scratch", scr or 16)
    return off, w[0]


# ---------------------------------------------------------------------------------------------------------------------------------------
# parameters, inputs, references (each computed once and left unchanged)
# ---------------------------------------------------------------------------------------------------------------------------------------
_CACHE = {}


def params(c):
    key = ("params", c.id)
    if key not in _CACHE:
        p = vo.init_mlp_vae_params(seed=c.id, z_dim=c.z, source_shape=c.src, target_shape=c.tgt, encoder_sizes=c.enc, decoder_sizes=c.dec)
        rng = np.random.RandomState(100 + c.id)
        for k in p:
            if k.endswith("bias"):
                p[k] = (0.05 * rng.standard_normal(p[k].shape)).astype(np.float32)
        _CACHE[key] = p
    return _CACHE[key]


def inputs(c, shift=None):
    """{'src_u8', 'tgt_u8', 'src', 'tgt', 'eps'}: independent random bytes (float tables = byte / 255 in float32), seeded noise.  shift: another seed shift than the
    row's (the host test shows what the unshifted seeds of cases 8 and 9 do; never cached)."""
    key = ("inputs", c.id)
    if shift is None and key in _CACHE:
        return _CACHE[key]
    rng = np.random.RandomState(3000 + c.id + (c.shift if shift is None else shift))
    s8 = rng.randint(0, 256, (c.B,) + c.src).astype(np.uint8)
    t8 = rng.randint(0, 256, (c.B,) + c.tgt).astype(np.uint8)
    eps = rng.standard_normal((c.B, c.z)).astype(np.float32)
    d = {"src_u8": s8, "tgt_u8": t8, "src": s8.astype(np.float32) / np.float32(255.0), "tgt": t8.astype(np.float32) / np.float32(255.0), "eps": eps}
    if shift is None:
        _CACHE[key] = d
    return d


Ref = collections.namedtuple("Ref", "recon kl grads mean logvar")
_DT = {"f64": torch.float64, "f32": torch.float32}


def reference(c, dtype="f64", storage="fp32", loss_fn="bce", kl_tolerance=0.0, beta=1.0):
    """One forward + backward of the oracle."""
    key = ("ref", c.id, dtype, storage, loss_fn, kl_tolerance, beta)
    if key not in _CACHE:
        d = inputs(c)
        (recon, kl, _), grads, fw = vo.mlp_vae_loss_and_grads(params(c), d["src"], d["tgt"], d["eps"], beta, kl_tolerance, loss_fn, _DT[dtype], storage)
        _CACHE[key] = Ref(recon, kl, grads, fw["mean"].numpy(), fw["logvar"].numpy())
    return _CACHE[key]


def inference_reference(p, c, dtype=torch.float64):
    """float64 encode / reconstruct(eps) / generate_from_latent(eps as the latent) on the parameters p (the device's own after its Adam step)."""
    d = inputs(c)
    with torch.no_grad():
        pt = {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in p.items()}
        mean = vo.mlp_vae_forward(pt, d["src"], sample=False, dtype=dtype)["mean"].numpy()
        rec = torch.sigmoid(vo.mlp_vae_forward(pt, d["src"], d["eps"], sample=True, dtype=dtype)["logits"]).numpy()
        gen = torch.sigmoid(vo.mlp_vae_forward(pt, None, z_override=d["eps"], dtype=dtype)["logits"]).numpy()
    return {"mean": mean, "recon": rec, "gen": gen}


def rel_err(a, b):
    """vae_gpu_common.rel_err."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


# ---------------------------------------------------------------------------------------------------------------------------------------
# Part A: one whole step against float64.  `got` is what an implementation under test produced (the device; on the CPU the fp32 oracle stands in).
# The bounds are the project's for this engine (tests/test_f_mlp_vae_gpu.py).
# ---------------------------------------------------------------------------------------------------------------------------------------
LOSS_REL, KL_ABS, GRAD_BOUND, INFER_BOUND = 1e-4, 4e-6, 1e-4, 1e-4
LR = 1e-5
ADAM_ABS, ADAM_REL = 2e-6, 1e-5


def step_report(ref, recon, kl, grads):
    """(rows, failures): every measured deviation next to its bound."""
    rows, bad = [], []

    def row(name, val, bound):
        rows.append((name, float(val), float(bound)))
        if not val <= bound:
            bad.append((name, float(val), float(bound)))

    row("reconstruction loss |err| / |ref|", abs(recon - ref.recon) / abs(ref.recon), LOSS_REL)
    row("kl loss |err| / (1e-4 |ref| + 4e-6)", abs(kl - ref.kl) / (LOSS_REL * abs(ref.kl) + KL_ABS), 1.0)
    assert set(grads) == set(ref.grads), sorted(set(grads) ^ set(ref.grads))
    for k in ref.grads:
        # (a reference tensor that is identically zero fails: rel_err is of a real maximum, and no gradient of these models is zero)
        e = rel_err(grads[k], ref.grads[k]) if np.abs(ref.grads[k]).max() > 0 else float("inf")
        rows.append(("grad " + k, e, GRAD_BOUND))
        if not e < GRAD_BOUND:
            bad.append(("grad " + k, e, GRAD_BOUND))
    return rows, bad


def adam_report(params_before, grads, params_after):
    """Worst |p_after - AdamTF(p_before, grads)| / (2e-6 + 1e-5 max|w|) per tensor at LR: 1.0 = at the bound."""
    adam = vo.AdamTF({k: v.shape for k, v in params_before.items()})
    want = {k: np.array(v, np.float32) for k, v in params_before.items()}
    adam.step(want, grads, LR)
    return {k: float(np.abs(params_after[k].astype(np.float64) - want[k]).max() / (ADAM_ABS + ADAM_REL * np.abs(want[k]).max())) for k in want}


# ---------------------------------------------------------------------------------------------------------------------------------------
# walk(): the network op by op in numpy float64
# ---------------------------------------------------------------------------------------------------------------------------------------
def bf16r(a):
    """float64 values of an array rounded to bf16 (round to nearest even, as the kernels store)."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(torch.float32).to(torch.bfloat16).to(torch.float64).numpy()


def heads_of(p, swap=False):
    """([K, 2 z] kernel, [2 z] bias) = [mean | logstd_sqare]; swap: the two halves exchanged (a deliberately WRONG statement)."""
    a, b = ("vae/logstd_sqare", "vae/mean") if swap else ("vae/mean", "vae/logstd_sqare")
    return (np.concatenate([p[a + "/kernel"], p[b + "/kernel"]], 1).astype(np.float64), np.concatenate([p[a + "/bias"], p[b + "/bias"]]).astype(np.float64))


def loss_rows(logits, y, loss_fn):
    """(per-row loss sums, d(row sum) / dlogits) in float64."""
    x = np.asarray(logits, np.float64)
    s = 1.0 / (1.0 + np.exp(-x))
    if loss_fn == "bce":
        per, g = np.maximum(x, 0) - x * y + np.log1p(np.exp(-np.abs(x))), s - y
    elif loss_fn == "bce_v2":
        per = -(y * np.log(1e-10 + s) + (1 - y) * np.log(1e-10 + 1 - s))
        g = -(y / (1e-10 + s) - (1 - y) / (1e-10 + 1 - s)) * s * (1 - s)
    elif loss_fn == "mse":
        per, g = (y - s) ** 2, -2.0 * (y - s) * s * (1 - s)
    else:
        raise ValueError(loss_fn)
    return per.sum(1), g


def kl_rows(mean, logvar):
    return -0.5 * (1.0 + logvar - mean * mean - np.exp(logvar)).sum(1)


def reparam_bwd(dz, mean, logvar, eps, inv_b, beta, kl_tolerance, z):
    """dheads [B, 2 z] = [dmean | dlogvar] (elementwise.hip reparam_kl_bwd)."""
    act = (kl_rows(mean, logvar) >= kl_tolerance * z).astype(np.float64).reshape(-1, 1) if kl_tolerance > 0 else 1.0
    dmu = dz + beta * mean * inv_b * act
    dlv = dz * eps * 0.5 * np.exp(0.5 * logvar) + beta * 0.5 * (np.exp(logvar) - 1.0) * inv_b * act
    return np.concatenate([dmu, dlv], 1)


Walk = collections.namedtuple("Walk", "recon kl grads st pre")


def walk(c, loss_fn="bce", kl_tolerance=0.0, beta=1.0, storage="f64", mutate=None, d=None):
    """One forward + backward, every tensor the engine stores kept in st (names as MlpVaeDevice.stored: x, h<i>, heads, mean, logvar, z, d<i>, gd<i>, dz, dheads,
    gh<i>) and every ReLU pre-activation in pre.  storage 'bf16': weights, the staged input and every stored activation / gradient rounded to bf16 -- the CPU stand-in
    for the bf16 engine.  mutate (deliberately WRONG statements for the host test): 'swap_heads' = the mean and logstd_sqare halves of the heads exchanged,
    'no_last_mask' = the ReLU mask of the decoder's last hidden layer left out of the output layer's input gradient."""
    p, d = params(c), inputs(c) if d is None else d
    q = bf16r if storage == "bf16" else (lambda a: a)
    B, z, inv_b = c.B, c.z, 1.0 / c.B
    L = layers(c)
    enc = [l for l in L if l[0].startswith("enc")]
    dec = [l for l in L if l[0].startswith("dec")]
    W = {l[1]: q(p[l[1] + "/kernel"].astype(np.float64)) for l in enc + dec}
    bias = {l[1]: p[l[1] + "/bias"].astype(np.float64) for l in enc + dec}
    wh, bh = heads_of(p, swap=mutate == "swap_heads")
    wh = q(wh)
    eps = d["eps"].astype(np.float64)
    st, pre, grads = {}, {}, {}
    a = st["x"] = q(d["src"].reshape(B, -1).astype(np.float64))
    for i, l in enumerate(enc):
        pre["h%d" % i] = a @ W[l[1]] + bias[l[1]]
        a = st["h%d" % i] = q(np.maximum(pre["h%d" % i], 0))
    st["heads"] = a @ wh
    mean, logvar = st["heads"][:, :z] + bh[:z], st["heads"][:, z:] + bh[z:]
    st["mean"], st["logvar"] = mean, logvar
    a = st["z"] = q(mean + np.exp(0.5 * logvar) * eps)
    nd = len(dec)
    for i, l in enumerate(dec):
        t = a @ W[l[1]] + bias[l[1]]
        if i + 1 < nd:
            pre["d%d" % i] = t
            t = np.maximum(t, 0)
        a = st["d%d" % i] = q(t)
    rows, g = loss_rows(a, d["tgt"].reshape(B, -1).astype(np.float64), loss_fn)
    klr = kl_rows(mean, logvar)
    recon, kl = float(rows.mean()), float((np.maximum(klr, kl_tolerance * z) if kl_tolerance > 0 else klr).mean())
    gy = st["gd%d" % (nd - 1)] = q(g * inv_b)
    for i in range(nd - 1, -1, -1):
        l = dec[i]
        ain = st["d%d" % (i - 1)] if i else st["z"]
        grads[l[1] + "/kernel"], grads[l[1] + "/bias"] = ain.T @ gy, gy.sum(0)
        dx = gy @ W[l[1]].T
        if i:
            if not (mutate == "no_last_mask" and i == nd - 1):
                dx = dx * (ain > 0)
            gy = st["gd%d" % (i - 1)] = q(dx)
        else:
            st["dz"] = dx
    dh = st["dheads"] = q(reparam_bwd(st["dz"], mean, logvar, eps, inv_b, beta, kl_tolerance, z))
    hl = st["h%d" % (len(enc) - 1)]
    gwh, gbh = hl.T @ dh, dh.sum(0)
    ha, hb = ("vae/logstd_sqare", "vae/mean") if mutate == "swap_heads" else ("vae/mean", "vae/logstd_sqare")
    grads[ha + "/kernel"], grads[hb + "/kernel"], grads[ha + "/bias"], grads[hb + "/bias"] = gwh[:, :z], gwh[:, z:], gbh[:z], gbh[z:]
    gy = st["gh%d" % (len(enc) - 1)] = q((dh @ wh.T) * (hl > 0))
    for i in range(len(enc) - 1, -1, -1):
        l = enc[i]
        ain = st["h%d" % (i - 1)] if i else st["x"]
        grads[l[1] + "/kernel"], grads[l[1] + "/bias"] = ain.T @ gy, gy.sum(0)
        if i:
            gy = st["gh%d" % (i - 1)] = q((gy @ W[l[1]].T) * (ain > 0))
    return Walk(recon, kl, grads, st, pre)


def relu_margin(w):
    """Smallest |pre-activation| / (largest |pre-activation| of its layer) over every ReLU of the network."""
    return min(float(np.abs(v).min() / np.abs(v).max()) for v in w.pre.values())


# ---------------------------------------------------------------------------------------------------------------------------------------
# Part B: the bf16 engine layer by layer, each op in float64 on the tensors the engine ITSELF stored.  The bounds are derived, not measured:
#   a product of reduction length K accumulated in fp32 (any order, any tree) is within (K + 2) 2^-24 sum_k |a_k| |w_k| of the exact sum of the same operands (K - 1
#   additions and one product rounding each, the bias addition, one spare); every slab of a split sum adds one more 2^-24 of that; a store in bf16 (8 significant bits)
#   adds 2^-8 |ref|.  Masked elements are exact zeros on both sides (bound 0).
#   Elementwise ops (reparameterisation, loss gradient, reparameterisation backward) have no reduction: the project's fp32 bound for these kernels (hip_helpers.tols:
#   1e-5 relative + 2e-5 of the tensor's max, their exp / sigmoid included) plus the bf16 store's 2^-8 |ref|.
# ---------------------------------------------------------------------------------------------------------------------------------------
U32, UBF = 2.0 ** -24, 2.0 ** -8
ELT_REL, ELT_MAX = 1e-5, 2e-5


class OpReport:
    def __init__(self):
        self.rows, self.bad = [], []

    def _close(self, name, got, ref, lim):
        got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        err = np.abs(got - ref)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err == 0, 0.0, err / lim)
        worst = float(ratio.max()) if np.isfinite(got).all() else float("inf")        # 1.0 = at the bound
        self.rows.append((name, worst))
        if not worst <= 1.0:
            self.bad.append((name, worst))

    def product(self, name, got, a, w, K, bias=None, relu=False, mask=None, bf16_out=True, slabs=1):
        """got against a @ w (+ bias, ReLU, mask): a [M, K], w [K, N]."""
        a, w = np.asarray(a, np.float64), np.asarray(w, np.float64)
        assert a.shape[1] == w.shape[0] == K, (name, a.shape, w.shape, K)
        ref, mag = a @ w, np.abs(a) @ np.abs(w)
        if bias is not None:
            ref, mag = ref + bias, mag + np.abs(bias)
        if relu:
            ref = np.maximum(ref, 0)
        if mask is not None:
            ref, mag = ref * mask, mag * mask
        extra = slabs if slabs > 1 else 0
        self._close(name, got, ref, (UBF * np.abs(ref) if bf16_out else 0.0) + (K + 2 + extra) * U32 * mag)

    def elementwise(self, name, got, ref, bf16_out=True):
        ref = np.asarray(ref, np.float64)
        self._close(name, got, ref, (UBF if bf16_out else 0.0) * np.abs(ref) + ELT_REL * np.abs(ref) + ELT_MAX * np.abs(ref).max())


def layer_report(c, st, grads, p, d, loss_fn="bce", kl_tolerance=0.0, beta=1.0, mutate=None):
    """Every op of one forward + backward of the bf16 engine against the float64 statement of that ONE op on the engine's own stored inputs.
    st: {'x', 'h<i>', 'heads', 'mean', 'logvar', 'z', 'd<i>', 'gd<i>', 'dz', 'dheads', 'gh<i>'} float64 numpy; grads: the gradient tensors (TF names); p: the fp32
    parameters (rounded to bf16 here: the shadow copy the kernels multiply); d: inputs().  The ReLU masks are the engine's own stored activations.
    mutate: as walk() (a deliberately WRONG statement)."""
    R = OpReport()
    B, z, inv_b = c.B, c.z, 1.0 / c.B
    L = layers(c)
    rt = route(c, "bf16")
    idx = {l[0]: j for j, l in enumerate(L)}
    enc = [l for l in L if l[0].startswith("enc")]
    dec = [l for l in L if l[0].startswith("dec")]
    W = {l[1]: bf16r(p[l[1] + "/kernel"]) for l in enc + dec}
    bias = {l[1]: np.asarray(p[l[1] + "/bias"], np.float64) for l in enc + dec}
    wh, bh = heads_of(p, swap=mutate == "swap_heads")
    wh = bf16r(wh)
    eps = d["eps"].astype(np.float64)
    ne, nd = len(enc), len(dec)
    # ---- forward ----
    R.elementwise("stage x", st["x"], d["src"].reshape(B, -1).astype(np.float64))
    a = st["x"]
    for i, l in enumerate(enc):
        R.product("%s.fwd" % l[0], st["h%d" % i], a, W[l[1]], l[2], bias=bias[l[1]], relu=True, slabs=rt["fwd"][idx[l[0]]])
        a = st["h%d" % i]
    R.product("heads.fwd raw", st["heads"], a, wh, L[idx["heads"]][2], bf16_out=False, slabs=rt["fwd"][idx["heads"]])
    R.elementwise("heads.bias mean", st["mean"], st["heads"][:, :z] + bh[:z], bf16_out=False)
    R.elementwise("heads.bias logvar", st["logvar"], st["heads"][:, z:] + bh[z:], bf16_out=False)
    mean, logvar = st["mean"], st["logvar"]
    R.elementwise("reparam.fwd z", st["z"], mean + np.exp(0.5 * logvar) * eps)
    a = st["z"]
    for i, l in enumerate(dec):
        R.product("%s.fwd" % l[0], st["d%d" % i], a, W[l[1]], l[2], bias=bias[l[1]], relu=i + 1 < nd, slabs=rt["fwd"][idx[l[0]]])
        a = st["d%d" % i]
    # ---- loss gradient ----
    _, g = loss_rows(a, d["tgt"].reshape(B, -1).astype(np.float64), loss_fn)
    R.elementwise("loss.dlogits", st["gd%d" % (nd - 1)], g * inv_b)
    # ---- backward: decoder ----
    for i in range(nd - 1, -1, -1):
        l, j = dec[i], idx[dec[i][0]]
        gy = st["gd%d" % i]
        ain = st["d%d" % (i - 1)] if i else st["z"]
        rs = rt["row_splits"][j]
        R.product("%s.wgrad" % l[0], grads[l[1] + "/kernel"], ain.T, gy, B, bf16_out=False, slabs=rs)
        R.product("%s.bias_grad" % l[0], grads[l[1] + "/bias"].reshape(1, -1), np.ones((1, B)), gy, B, bf16_out=False, slabs=rs)
        if i:
            mask = None if (mutate == "no_last_mask" and i == nd - 1) else (ain > 0)
            R.product("%s.dgrad" % l[0], st["gd%d" % (i - 1)], gy, W[l[1]].T, l[3], mask=mask, slabs=rt["dgrad"][j])
        else:
            R.product("%s.dgrad dz" % l[0], st["dz"], gy, W[l[1]].T, l[3], bf16_out=False, slabs=rt["dgrad"][j])
    R.elementwise("reparam.bwd dheads", st["dheads"], reparam_bwd(st["dz"], mean, logvar, eps, inv_b, beta, kl_tolerance, z))
    # ---- backward: heads and encoder ----
    dh, hl, jh = st["dheads"], st["h%d" % (ne - 1)], idx["heads"]
    ha, hb = ("vae/logstd_sqare", "vae/mean") if mutate == "swap_heads" else ("vae/mean", "vae/logstd_sqare")
    gw = np.concatenate([grads[ha + "/kernel"], grads[hb + "/kernel"]], 1)
    gb = np.concatenate([grads[ha + "/bias"], grads[hb + "/bias"]])
    R.product("heads.wgrad", gw, hl.T, dh, B, bf16_out=False, slabs=rt["row_splits"][jh])
    R.product("heads.bias_grad", gb.reshape(1, -1), np.ones((1, B)), dh, B, bf16_out=False, slabs=rt["row_splits"][jh])
    R.product("heads.dgrad", st["gh%d" % (ne - 1)], dh, wh.T, 2 * z, mask=hl > 0, slabs=rt["dgrad"][jh])
    for i in range(ne - 1, -1, -1):
        l, j = enc[i], idx[enc[i][0]]
        gy = st["gh%d" % i]
        ain = st["h%d" % (i - 1)] if i else st["x"]
        R.product("%s.wgrad" % l[0], grads[l[1] + "/kernel"], ain.T, gy, B, bf16_out=False, slabs=rt["row_splits"][j])
        R.product("%s.bias_grad" % l[0], grads[l[1] + "/bias"].reshape(1, -1), np.ones((1, B)), gy, B, bf16_out=False, slabs=rt["row_splits"][j])
        if i:
            R.product("%s.dgrad" % l[0], st["gh%d" % (i - 1)], gy, W[l[1]].T, l[3], mask=ain > 0, slabs=rt["dgrad"][j])
    return R


# bf16 losses against the oracle's bf16 emulation (tests/test_f_mlp_vae_gpu.py); a case that cannot meet them: the ConvVAE engine test's form against float64
BF16_RECON_REL, BF16_KL_REL, BF16_KL_ABS = 2e-3, 2e-2, 1e-4


def bf16_loss_report(c, recon, kl):
    """(rows, failures) of the bf16 engine's two losses."""
    emul, exact = reference(c, storage="bf16", dtype="f32"), reference(c)
    rows, bad = [], []
    for name, got, e, x, rel, ab in (("reconstruction", recon, emul.recon, exact.recon, BF16_RECON_REL, 0.0), ("kl", kl, emul.kl, exact.kl, BF16_KL_REL, BF16_KL_ABS)):
        first = abs(got - e) / (rel * abs(e) + ab)
        fallback = abs(got - x) / (1.25 * abs(e - x) + 5e-3 * abs(x))
        rows.append((name + " loss vs emulation / bound", float(first)))
        rows.append((name + " loss vs float64 / (1.25 |emul - exact| + 5e-3 |exact|)", float(fallback)))
        if not (first <= 1.0 or fallback <= 1.0):
            bad.append((name, float(first), float(fallback)))
    return rows, bad
