"""The bf16 interval checker of tests/ulp_ref.py has teeth (CPU): faithful float32 restatements of the kernels pass it
at margin 8 on the GPU tests' own inputs, every subtly wrong one fails it, and the references alone meet the sharpness
condition. So tests/test_gpu_ulp.py would fail on a kernel that is wrong in any of these ways."""
import numpy as np
import pytest
import torch

import ulp_ref as U

LN_D = (256, 260, 384, 388, 512, 768, 1024, 1280, 1536, 1796, 2048, 2052, 4096)  # tests/test_gpu_ulp.py's widths
LN_M = (1, 5, 33)
TEETH_D = (256, 388, 1280, 4096)
GEMM_SHAPES = ((129, 200, 64), (300, 384, 256), (257, 768, 384), (24, 1280, 1280), (7, 384, 384), (192, 512, 128))
GEMV_SHAPES = ((24, 1280, 1280), (13, 1536, 384), (33, 1536, 384), (64, 1296, 1280))


def fails(got_bits, ref, slack):
    try:
        U.assert_bf16_correctly_rounded(got_bits, ref, slack, "mutant")
    except AssertionError:
        return True
    return False


# ---- the rounding and the checker themselves ---------------------------------------------------------------------
def test_bf16_rne_equals_torch_on_float32_bit_patterns():
    u = np.random.default_rng(0).integers(0, 2 ** 32, 1_000_000, dtype=np.uint64).astype(np.uint32)
    edge = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF,
                     0x00000001, 0x00008000, 0x00008001, 0x00018000, 0x007FFFFF, 0x00800000, 0x3F808000, 0x3F818000,
                     0x3F807FFF, 0x3F808001], np.uint32)
    f = np.concatenate([u, edge]).view(np.float32)
    want = torch.from_numpy(f.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    got = U.bf16_rne(f)
    nan = np.isnan(f)
    assert np.array_equal(got[~nan], want[~nan])
    assert U.bf16_is_nan(got[nan]).all() and np.array_equal(got[nan] >> 15, f.view(np.uint32)[nan] >> 31)


def test_bf16_rne_rounds_float64_once():
    one_step = 2.0 ** -7  # the bf16 step at 1.0
    # just above the tie between 1 and 1 + 2^-7: float32 first would land on the tie and go to even (1.0)
    assert U.bf16_rne(1.0 + 2.0 ** -8 + 2.0 ** -40) == U.bf16_rne(1.0 + one_step) == 0x3F81
    assert U.bf16_rne(1.0 + 2.0 ** -8) == 0x3F80 and U.bf16_rne(1.0 + 3 * 2.0 ** -8) == 0x3F82  # ties to even
    assert U.bf16_rne(1.0 + 2.0 ** -8 - 2.0 ** -40) == 0x3F80
    assert U.bf16_rne(np.float32(3.4028234663852886e38)) == 0x7F80  # the largest finite f32 -> inf
    assert U.bf16_rne(-1e300) == 0xFF80 and U.bf16_rne(np.inf) == 0x7F80
    assert U.bf16_rne((2.0 - 2.0 ** -7) * 2.0 ** 127) == 0x7F7F  # the largest bf16 stays finite
    assert U.bf16_rne((2.0 - 2.0 ** -8) * 2.0 ** 127) == 0x7F80  # its tie with 2^128 goes to even: inf
    assert U.bf16_is_nan(U.bf16_rne(np.nan)) and U.bf16_is_nan(U.bf16_rne(np.float32(np.nan)))
    assert U.bf16_rne(2.0 ** -133) == 0x0001 and U.bf16_rne(2.0 ** -134) == 0x0000  # subnormals; a tie to even
    assert U.bf16_rne(3 * 2.0 ** -134) == 0x0002 and U.bf16_rne(-2.0 ** -126) == 0x8080
    assert U.bf16_rne(-0.0) == 0x8000


def test_bf16_key_is_monotone_and_dense():
    bits = np.arange(0x10000, dtype=np.uint32).astype(np.uint16)
    fin = bits[~U.bf16_is_nan(bits)]
    order = np.argsort(U.bf16_key(fin), kind="stable")
    vals = U.bf16_to_f64(fin[order])
    assert (np.diff(vals) >= 0).all()
    keys = np.unique(U.bf16_key(fin))
    assert (np.diff(keys) == 1).all() and U.bf16_key(0x8000) == U.bf16_key(0x0000)


def test_checker_accepts_the_interval_and_nothing_else():
    ref = np.array([[1.0, 1.0 + 2.0 ** -8, -3.0, 0.0]])
    ok = U.bf16_rne(ref)
    U.assert_bf16_correctly_rounded(ok, ref, 0.0)
    up = ok.copy()
    up[0, 0] += 1
    assert fails(up, ref, 0.0) and fails(up, ref, 2.0 ** -9)
    assert fails(up, ref, 2.0 ** -8)  # ref + slack is the tie, which rounds to even: back to 1.0
    U.assert_bf16_correctly_rounded(up, ref, 2.0 ** -8 + 2.0 ** -30)
    U.assert_bf16_correctly_rounded(up, ref, np.array([[2.0 ** -7, 0, 0, 0]]))  # per element
    U.assert_bf16_correctly_rounded(up, ref, np.array([[2.0 ** -7]]))  # per row
    tie_up = ok.copy()
    tie_up[0, 1] = 0x3F81
    assert fails(tie_up, ref, 0.0)  # the tie goes to even without slack
    U.assert_bf16_correctly_rounded(tie_up, ref, 1e-12)
    neg0 = ok.copy()
    neg0[0, 3] = 0x8000
    U.assert_bf16_correctly_rounded(neg0, ref, 0.0)  # -0 is 0
    nan = ok.copy()
    nan[0, 2] = 0x7FC0
    assert fails(nan, ref, 1e30)
    U.assert_bf16_correctly_rounded(np.array([0xFFC1]), np.array([np.nan]), 0.0)
    assert fails(np.array([0x3F80]), np.array([np.nan]), 0.0)


def test_checker_failure_report():
    ref = np.tile(np.array([1.0, 2.0, 3.0]), (4, 1))
    got = U.bf16_rne(ref)
    got[2, 1] += 3
    got[3, 0] += 1
    with pytest.raises(AssertionError) as e:
        U.assert_bf16_correctly_rounded(got, ref, 1e-9, "k_test")
    msg = str(e.value)
    assert "k_test" in msg and "2 of 12" in msg and "row 2 col 1" in msg and "0x4003" in msg and "ref 2.0" in msg
    assert "[2.0 (0x4000), 2.0 (0x4000)]" in msg and "3 bf16 steps" in msg
    assert U.margin_needed(got, ref, 1e-3) == pytest.approx((2.0 + 2.5 * 2.0 ** -6 - 2.0) / 1e-3)
    assert U.margin_needed(U.bf16_rne(ref), ref, 0.0) == 0.0


def test_pack_act_index_is_the_existing_layout():
    for M, K in ((1, 32), (17, 64), (33, 384), (64, 1280)):
        idx = U.pack_act_index(M, K)
        m = torch.arange(M).view(M, 1)
        k = torch.arange(K).view(1, K)
        old = (m // 32) * 32 * K + (((k // 32) * 2 + (m // 16) % 2) * 64 + m % 16 + 16 * ((k // 8) % 4)) * 8 + k % 8
        assert np.array_equal(idx, old.numpy())
        assert len(np.unique(idx)) == M * K and idx.max() < 64 * K


# ---- LayerNorm ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", LN_D)
def test_reference_alone_is_sharp(D):
    """At every width, row count and well-conditioned family of the GPU test, slack = 8 E stays below 2^-12 |ref| on
    95 % of the elements (the outlier family only since its outlier was shrunk to 16)."""
    for M in LN_M:
        for fam in U.WELL_CONDITIONED:
            c = U.ln_case(fam, M, D)
            share = U.sharp_share(c["ref"], U.MARGIN * c["E"])
            assert share >= U.SHARP_SHARE, (fam, M, D, share)


@pytest.mark.parametrize("fam", U.FAMILIES)
@pytest.mark.parametrize("D", TEETH_D)
def test_faithful_layernorms_pass(D, fam):
    """Two float32 LayerNorms that ln_E does not contain (the restatements behind E pass by construction): the
    256-thread block order of tw_row_ln_store, and torch's."""
    c = U.ln_case(fam, 33, D)
    t = torch.nn.functional.layer_norm(torch.from_numpy(c["x"]), (D,), torch.from_numpy(c["g"]),
                                       torch.from_numpy(c["b"]), U.LN_EPS).numpy()
    for name, y in (("block order", U.layer_norm32_block_order(c["x"], c["g"], c["b"], U.LN_EPS)), ("torch", t)):
        U.assert_bf16_correctly_rounded(U.bf16_rne(y), c["ref"], U.MARGIN * c["E"], f"{name} {fam} D={D}")


@pytest.mark.parametrize("D", TEETH_D)
def test_kernel_order_passes_against_the_numpy_restatement_alone(D):
    """In the well-conditioned families the kernel-order restatement needs none of ln_E's other members: it passes
    against E taken from numpy's sums alone."""
    for fam in U.WELL_CONDITIONED:
        c = U.ln_case(fam, 33, D)
        E = U.row_E(U.layer_norm32(c["x"], c["g"], c["b"], U.LN_EPS), c["ref"])
        for y in (U.layer_norm32_kernel_order(c["x"], c["g"], c["b"], U.LN_EPS),
                  U.layer_norm32_block_order(c["x"], c["g"], c["b"], U.LN_EPS)):
            U.assert_bf16_correctly_rounded(U.bf16_rne(y), c["ref"], U.MARGIN * E, f"{fam} D={D}")


def test_kernel_order_restatement_is_a_layernorm():
    """(so that the mutants built on it differ from a faithful one only where they say)"""
    for D in (260, 388, 1280):
        c = U.ln_case("plain", 5, D)
        for f in (U.layer_norm32_kernel_order, U.layer_norm32_block_order):
            np.testing.assert_allclose(f(c["x"], c["g"], c["b"], U.LN_EPS), c["ref"], rtol=0, atol=2e-5)


def _ln_mutants():
    eps = U.LN_EPS
    return {
        "bf16 truncation": lambda x, g, b: U.f32_bits_to_bf16_trunc(U.layer_norm32(x, g, b, eps)),
        "variance over D - 1": lambda x, g, b: U.bf16_rne(U.layer_norm32(x, g, b, eps, ddof=1)),
        "eps 1e-6": lambda x, g, b: U.bf16_rne(U.layer_norm32(x, g, b, 1e-6)),
        "one-pass variance": lambda x, g, b: U.bf16_rne(U.layer_norm32(x, g, b, eps, one_pass=True)),
        "statistics skip the partial group": lambda x, g, b: U.bf16_rne(
            U.layer_norm32_kernel_order(x, g, b, eps, skip_partial_group=True)),
        "gamma / beta one chunk off": lambda x, g, b: U.bf16_rne(
            U.layer_norm32_kernel_order(x, g, b, eps, affine_shift=1)),
    }


@pytest.mark.parametrize("name", list(_ln_mutants()))
def test_layernorm_mutants_fail(name):
    mutant = _ln_mutants()[name]
    caught = {}
    for D in TEETH_D:
        for fam in U.FAMILIES:
            c = U.ln_case(fam, 33, D)
            caught[D, fam] = fails(mutant(c["x"], c["g"], c["b"]), c["ref"], U.MARGIN * c["E"])
    assert any(caught.values()), name
    # where each one must show: every width for the arithmetic mutants, the family built for it
    if name == "eps 1e-6":
        assert all(caught[D, "tinyvar"] for D in TEETH_D)
    elif name == "one-pass variance":
        assert all(caught[D, "offset"] for D in TEETH_D)
    elif name == "statistics skip the partial group":
        assert all(caught[388, fam] for fam in U.FAMILIES)  # D / 4 = 97 = 64 + 33
        assert not any(caught[D, fam] for D in (256, 1280, 4096) for fam in U.FAMILIES)  # (no partial group there)
    else:
        assert all(caught[D, "plain"] for D in TEETH_D)


def test_half_away_rounding_fails_on_exact_ties():
    """A conversion has E = 0: the interval is the one correctly rounded value."""
    x = U.tie_block(512)
    assert np.array_equal(x.view(np.uint32) & 0xFFFF, np.full(512, 0x8000))
    ref = x.astype(np.float64)
    U.assert_bf16_correctly_rounded(U.bf16_rne(x), ref, 0.0)
    got = U.bf16_half_away(x)
    even = (x.view(np.uint32) >> 16) & 1 == 0
    assert np.array_equal(got[~even], U.bf16_rne(x)[~even]) and fails(got, ref, 0.0)
    assert fails(U.f32_bits_to_bf16_trunc(x), ref, 0.0)
    # on randn the half-away mutant is invisible: only the tie block catches it
    r = np.random.default_rng(1).standard_normal(4096).astype(np.float32)
    U.assert_bf16_correctly_rounded(U.bf16_half_away(r), r.astype(np.float64), 0.0)


def test_residual_sum_order_is_checked_exactly():
    g = np.random.default_rng(3)
    M, D = 24, 1280
    x = U.ln_rows("plain", M, D)
    bias = g.standard_normal(D).astype(np.float32)
    parts = g.standard_normal((16, M, D)).astype(np.float32)
    for nparts in (1, 3, 4, 5, 16):
        want = U.resid_sum32(x, bias, parts, nparts)
        # the definition, element by element, on one row
        row = x[7].copy()
        row = row + bias
        for p in range(nparts):
            row = row + parts[p, 7]
        assert np.array_equal(want[7].view(np.uint32), row.view(np.uint32))
        other = U.resid_sum32(x, bias, parts, nparts, order="grouped")
        np.testing.assert_allclose(other, want, rtol=1e-5, atol=1e-5)  # (what the older tests ask: it passes them)
        assert not np.array_equal(other.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(U.resid_sum32(x, None, parts, 0), x)


# ---- GEMM --------------------------------------------------------------------------------------------------------
def _tiled32(a, w, bias, gelu=False, drop_last_tile=False):
    """float32 product accumulated over 64-deep K tiles in order, as the kernels walk K."""
    K = a.shape[1] - (64 if drop_last_tile else 0)
    acc = np.zeros((a.shape[0], w.shape[0]), np.float32)
    for k0 in range(0, K, 64):
        acc = acc + a[:, k0: k0 + 64] @ w[:, k0: k0 + 64].T
    y = acc + bias
    return U.gelu_as32(y) if gelu else y


@pytest.mark.parametrize("M,N,K", sorted(set(GEMM_SHAPES + GEMV_SHAPES)))
def test_faithful_gemm_passes_and_mutants_fail(M, N, K):
    c = U.gemm_case(M, N, K)
    for gelu in (False, True):
        ref, E = (c["ref_gelu"], c["E_gelu"]) if gelu else (c["ref"], c["E"])
        slack = U.MARGIN * E
        assert U.sharp_share(ref, slack) >= U.SHARP_SHARE  # (GELU: with its per-element E, U.gemm_case)
        for y in (U.gemm_bias32(c["A"], c["W"], c["bias"], gelu), _tiled32(c["A"], c["W"], c["bias"], gelu)):
            U.assert_bf16_correctly_rounded(U.bf16_rne(y), ref, slack, f"gemm {M}x{N}x{K} gelu={gelu}")
        y = U.gemm_bias32(c["A"], c["W"], c["bias"], gelu)
        assert fails(U.f32_bits_to_bf16_trunc(y), ref, slack)
        assert fails(U.bf16_rne(_tiled32(c["A"], c["W"], c["bias"], gelu, drop_last_tile=True)), ref, slack)
    # the tanh form of GELU instead of the erf form
    x = U.gemm_bias32(c["A"], c["W"], c["bias"])
    inner = np.float32(0.7978845608) * (x + np.float32(0.044715) * x * x * x)
    tanh = np.float32(0.5) * x * (np.float32(1) + np.tanh(inner))
    assert fails(U.bf16_rne(tanh), c["ref_gelu"], U.MARGIN * c["E_gelu"])
    # bias added after the rounding (and the sum rounded again)
    acc = U.gemm_bias32(c["A"], c["W"])
    late = U.bf16_rne(U.bf16_to_f64(U.bf16_rne(acc)).astype(np.float32) + c["bias"])
    assert fails(late, c["ref"], U.MARGIN * c["E"])


def test_gelu_restatement_against_float64():
    x = np.linspace(-8, 8, 20001).astype(np.float32)
    err = np.abs(U.gelu_as32(x).astype(np.float64) - U.gelu64(x))
    assert err.max() < 5e-7  # 0.5 |x| (1.5e-7 of the erf formula + float32 rounding)
    assert U.gelu64(np.array([0.0, 1.0]))[1] == pytest.approx(0.8413447460685429, abs=1e-15)


# ---- im2col ------------------------------------------------------------------------------------------------------
def test_im2col_conv1_ref_is_the_conv_input():
    """The restated im2col times a k3 p1 convolution's reordered weights is the convolution of the seek window."""
    g = np.random.default_rng(5)
    n_mels, kpad, ld = 8, 64, 3100
    feats = U.bf16_exact(g.standard_normal((4, n_mels, ld)))[0]
    row_map, seek, maxf = [2, 0, 2], [0, 2999, 17], [3000, 3100, 1000, 3100]
    bits = U.im2col_conv1_ref(feats, n_mels, row_map, seek, 3, kpad, maxf)
    a = U.bf16_to_f64(bits).reshape(3, 3000, kpad)
    assert not a[:, :, 3 * n_mels:].any()
    for r in range(3):
        valid = min(3000, maxf[row_map[r]] - seek[r])
        seg = np.zeros((n_mels, 3000))
        seg[:, :valid] = feats[row_map[r], :, seek[r]: seek[r] + valid]
        padded = np.pad(seg, ((0, 0), (1, 1)))
        for j in range(3):
            assert np.array_equal(a[r, :, j * n_mels: (j + 1) * n_mels], padded[:, j: j + 3000].T)
    assert not a[1, 2:].any() and a[1, 0, n_mels: 2 * n_mels].any()  # one valid frame: rows 0 and 1 only
