"""What the cases of tests/vae_elementwise_cases.py claim about themselves, asserted on the CPU: a failure of test_w_vae_elementwise_gpu.py is then never the reference's
fault.  For every case: the float64 reference is finite; the float32 restatement of the reference formula is inside the bound the kernel is held to, where one is
stated; the kl_floor and planted-value gaps hold; every P listed for a channel count is divisible by it."""
import numpy as np
import pytest

import vae_elementwise_cases as vc
from hip_helpers import DTS


@pytest.mark.parametrize("kind,R", vc.RECON_KIND_R)
@pytest.mark.parametrize("BP", vc.RECON_SHAPES)
def test_recon_cases(BP, kind, R):
    for dt in DTS:
        for which in ("none", "rep"):
            assert vc.recon_conditions_met(BP[0], BP[1], kind, R, dt, which), (dt, which)
    if BP in vc.RECON_ALIGN_SHAPES:
        assert vc.recon_conditions_met(BP[0], BP[1], kind, R, "f32", "align")
        idx = vc.recon_frame_idx(BP[0], "align")
        assert idx[0] % 2 == 0 and idx[1] % 2 == 1
        # row 0 of the padded tables is aligned, row 1 is not: float labels (stride P + 1, 4 bytes each, 16-byte vectors), byte labels (stride P + 3, 8-byte loads)
        assert ((BP[1] + 1) * 4 * int(idx[1])) % 16 != 0 and ((BP[1] + 3) * int(idx[1])) % 8 != 0


def test_recon_shapes_take_the_paths_they_are_listed_for():
    assert vc.BCE_CHUNK == 6144
    paths = {(B, P): (P % vc.BCE_PER_THREAD == 0, vc.recon_chunks(P)) for B, P in vc.RECON_SHAPES}
    assert paths == {(1, 23): (False, 1), (1, 24): (True, 1), (3, 30): (False, 1), (2, 6144): (True, 1), (2, 6150): (False, 2), (2, 6168): (True, 2)}
    assert 6168 == 24 * 257                              # the second chunk has one active thread
    for B, P in vc.RECON_BIAS_SHAPES:
        for c in vc.RECON_CHANNELS:
            assert P % c == 0 and vc.BCE_PER_THREAD % c == 0
    for B in (1, 2, 3):
        idx = vc.recon_frame_idx(B, "rep")
        assert idx.max() < vc.RECON_FRAMES and (B == 1 or len(set(idx.tolist())) < B)


def test_recon_kind1_is_only_tested_where_the_reference_itself_is_finite():
    """The reference's own fp32 formula log(1e-10 + 1 - s) leaves the finite numbers once s rounds to 1 (x >= ~17): the float32 restatement shows it; R = 8 stays clear of it."""
    y = np.array([0.5], np.float32)
    with np.errstate(all="ignore"):
        per17, _ = vc.recon_ref32(np.array([17.5], np.float32), y, 1)
        per8, g8 = vc.recon_ref32(np.array([8.0], np.float32), y, 1)
    assert not np.isfinite(per17).all() or per17[0] > 10.0
    assert np.isfinite(per8).all() and np.isfinite(g8).all()
    assert all(R <= 8.0 for k, R in vc.RECON_KIND_R if k == 1)


@pytest.mark.parametrize("shape", vc.REPARAM_SHAPES + [vc.REPARAM_WIDE_SHAPES[-1]])
def test_reparam_cases(shape):
    assert vc.reparam_conditions_met(*shape)
    if shape == vc.REPARAM_NEAR_PRIOR:
        assert vc.reparam_conditions_met(*shape, near_prior=True)
        d = vc.reparam_data(*shape, near_prior=True)
        r = vc.reparam_ref64(d, 0.0)
        b = vc.kl_bound(r["mean"], r["logvar"], r["kl"])
        assert (vc.KL_REL * np.abs(r["kl"]) < 0.01 * b).all()          # near the prior the sum's own rounding, not the relative term, decides
    d = vc.reparam_data(*shape)
    assert np.array_equal(vc.slab_sum32(d["heads"], d["bm"], d["bl"])[0], d["mean32"])


def test_reparam_floor_reference_stops_the_gradient_of_the_rows_below():
    shape = (5, 64, 9, 9)
    d = vc.reparam_data(*shape)
    zero = dict(d, dzs=np.zeros_like(d["dzs"]))
    g = vc.reparam_ref64(zero, d["floor"])["dheads"]
    kl = vc.reparam_ref64(zero, 0.0)["kl"]
    below = kl < d["floor"]
    assert below[1] and not below[0]
    assert (g[below] == 0).all() and (np.abs(g[~below]).sum(1) > 0).all()


@pytest.mark.parametrize("i", range(len(vc.FIN_N_PARTIAL)))
def test_finalize_cases(i):
    n, B = vc.FIN_N_PARTIAL[i], vc.FIN_B[i % 4]
    assert vc.fin_conditions_met(n, B, 0.0 if i % 2 == 0 else 0.5, 0)
    for nb in vc.FIN_N_BIAS:
        assert vc.fin_conditions_met(35, 5, 0.5, nb)
    assert vc.fin_derived_bound(13001) < vc.FIN_OUT_REL


def test_adam_cases():
    for n in vc.ADAM_N:
        p, m, v, g = vc.adam_data(n)
        assert np.isfinite(p).all() and g[0] == 0 and m[0] == 0 and v[0] == 0
        if n >= 4:
            assert g[1] == np.float32(1e20) and np.float64(g[1]) ** 2 > np.finfo(np.float32).max and 0 < g[2] < np.finfo(np.float32).tiny and g[3] == 0 and np.signbit(g[3])
        if n >= 8:
            assert np.array_equal(g[n - 4:].view(np.uint32), vc.ADAM_PLANTED_G.view(np.uint32))
    big = vc.ADAM_N[-1]
    assert big // 4 > 2048 * 256 and big % 4 == 3 and 4 * 4 * (big + 16) + 2 * (big + 16) < 40e6          # a second grid-stride trip, a tail, under 40 MB with a bf16 shadow


def test_splitk_u8_cases():
    for dt in DTS:
        for M, N in vc.SPLITK_SHAPES:
            slabs, bias, mask = vc.splitk_data(M, N, 7, dt)
            flat = mask.reshape(-1)
            assert np.isnan(flat).sum() == 1 and (flat == vc.tiny_positive(dt)).sum() == 1 and (np.signbit(flat) & (flat == 0)).sum() == 1
            ref = vc.splitk_ref32(slabs, bias, 1, mask)
            assert np.isfinite(ref).all() and ref.reshape(-1)[0] == 0 and ref.reshape(-1)[3] == 0
            open_ = vc.splitk_ref32(slabs, bias, 0, None).reshape(-1)
            tiny_at = int(np.flatnonzero(flat == vc.tiny_positive(dt))[0])
            assert vc.splitk_ref32(slabs, bias, 0, mask).reshape(-1)[tiny_at] == open_[tiny_at] != 0
    assert vc.u8_conditions_met()
    assert vc.U8_N[-1] > 2048 * 256 * 16


def test_pointwise_cases():
    assert vc.cast_conditions_met()
    x = vc.sigmoid_input(1000)
    assert set(vc.SIGMOID_PLANTED.tolist()) <= set(x.tolist()) and np.signbit(x[3])
    for n in vc.RANGE_N:
        x = vc.range_input(n)
        assert ((x >= 0) & (x <= 1)).all()
        if n >= 4:
            assert x[1] == 0 and x[n - 2] == 1
    for name, b in vc.range_bad_values(0.0, 1.0):
        assert not (b >= 0 and b <= 1), name
    assert vc.BIG_N > 2048 * 256
    for M, N in vc.COLSUM_SHAPES:
        assert N <= 256 and np.isfinite(vc.colsum_input(M, N)).all()
