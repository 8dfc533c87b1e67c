"""The "correctly rounded bf16" criterion for kernels that compute in f32 and store bf16, and the float64
references, float32 restatements and input generators it needs (tests/test_ulp_ref.py on the CPU,
tests/test_gpu_ulp.py on the MI355X).

The criterion. A kernel's bf16 output `got` is compared with a float64 reference `ref` of the same operation on the
same inputs. Element i passes when `got` lies in the closed bf16 interval

    [bf16_rne(ref - slack), bf16_rne(ref + slack)]

so where ref is further than `slack` from a bf16 rounding boundary exactly one bf16 value passes. There is no atol /
rtol and no share of elements that may be left out.

The slack is never a fixed number and never comes from the kernel under test: slack = MARGIN * E, where E is the
largest |float32 restatement - float64 reference| on the same inputs, computed on the CPU (per row for row-wise
kernels: `ln_E`; over the whole output for a GEMM, and carried through GELU per element for the GELU epilogues:
`gemm_case`). MARGIN = 8 because the kernels sum in another order (64-lane xor butterflies, MFMA accumulators), use
the hardware rsq / rcp (1 ulp each) and are compiled with a * b + c contracted, each of which contributes an error of
the order of the restatement's own. `sharp_share` measures how tight that is: the share of elements with
slack <= 2^-12 |ref|, an eighth of the bf16 half-ulp; the tests require 95 % on well-conditioned inputs.
"""
import numpy as np

MARGIN = 8.0
SHARP = 2.0 ** -12
SHARP_SHARE = 0.95

_BF16_MAX = (2.0 - 2.0 ** -7) * 2.0 ** 127


# ---- bf16 -------------------------------------------------------------------------------------------------------
def bf16_rne(x):
    """bf16 bits (uint16) of float64 / float32 `x`, rounded to nearest, ties to even, in ONE rounding from the float64
    value (a float32 input converts to float64 exactly). NaN -> a quiet NaN of the same sign, overflow -> inf,
    results below 2^-126 are bf16 subnormals (multiples of 2^-133)."""
    with np.errstate(invalid="ignore"):  # (a signalling NaN converts with a warning)
        x = np.asarray(x, dtype=np.float64)
    a = np.abs(x)
    nan = np.isnan(x)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        fin = np.where(nan | np.isinf(x), 0.0, a)
        big = fin >= 2.0 ** 128  # far past the bf16 range: inf (and keeps ldexp below in range)
        fin = np.where(big, 0.0, fin)
        _, e = np.frexp(fin)  # fin = m * 2^e, 0.5 <= m < 1: the leading bit has weight 2^(e-1)
        q = np.maximum(e - 1, -126) - 7  # weight of the last kept bit (8 significant bits; fixed below 2^-126)
        n = np.rint(np.ldexp(fin, -q))  # exact scaling; rint rounds half to even
        r = np.ldexp(n, q)  # <= 2^128, exact
        r = np.where(big | np.isinf(x) | (r > _BF16_MAX), np.inf, r)
        f = np.where(nan, np.nan, np.copysign(r, x)).astype(np.float32)  # exact: r is a bf16 value or inf
    bits = (f.view(np.uint32) >> 16).astype(np.uint16)
    sign = (np.signbit(x).astype(np.uint16) << 15)
    return np.where(nan, sign | np.uint16(0x7FC0), bits).astype(np.uint16)


def bf16_to_f64(bits):
    b = np.asarray(bits).astype(np.uint16)
    return (b.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def bf16_key(bits):
    """Monotone integer key of bf16 bits: key(a) < key(b) iff a < b as numbers, consecutive bf16 values have
    consecutive keys, and -0 and +0 share one key. (NaNs lie beyond the infinities; callers treat them apart.)"""
    b = np.asarray(bits).astype(np.int32) & 0xFFFF
    mag = b & 0x7FFF
    return np.where(b & 0x8000, -mag, mag).astype(np.int32)


def bf16_is_nan(bits):
    b = np.asarray(bits).astype(np.int32) & 0x7FFF
    return b > 0x7F80


def sharp_share(ref64, slack):
    """Share of elements whose slack is at most 2^-12 |ref| (an eighth of the bf16 half-ulp)."""
    ref64 = np.asarray(ref64, dtype=np.float64)
    s = np.broadcast_to(np.asarray(slack, dtype=np.float64), ref64.shape)
    return float(np.mean(s <= SHARP * np.abs(ref64)))


def margin_needed(got_bits, ref64, E):
    """The margin this output needed: the largest distance from ref to the set of reals that round to `got` (0 where
    got is the correctly rounded ref), over E. E broadcasts like a slack; where E is 0 and the distance is not, inf."""
    ref64 = np.asarray(ref64, dtype=np.float64)
    g = np.asarray(got_bits).astype(np.uint16).reshape(ref64.shape)
    k = bf16_key(g)
    v = bf16_to_f64(g)
    with np.errstate(invalid="ignore", over="ignore"):
        lo = 0.5 * (v + bf16_to_f64(_key_to_bits(k - 1)))
        hi = 0.5 * (v + bf16_to_f64(_key_to_bits(k + 1)))
        d = np.maximum(np.maximum(lo - ref64, ref64 - hi), 0.0)
        d = np.where(np.isfinite(d), d, 0.0)
        e = np.broadcast_to(np.asarray(E, dtype=np.float64), ref64.shape)
        m = np.where(d > 0, d / np.where(e > 0, e, np.nan), 0.0)
    m = np.where(np.isnan(m), np.inf, m)
    return float(m.max()) if m.size else 0.0


def _key_to_bits(k):
    k = np.clip(np.asarray(k, dtype=np.int32), -0x7F80, 0x7F80)
    return np.where(k < 0, 0x8000 | (-k), k).astype(np.uint16)


def assert_bf16_correctly_rounded(got_bits, ref64, slack, what=""):
    """Every element of `got_bits` (bf16 bits, any integer dtype) lies in [bf16_rne(ref64 - slack),
    bf16_rne(ref64 + slack)], compared on the monotone key. `slack` (>= 0) broadcasts against ref64: a scalar, one
    value per row ([M, 1]) or per element. A NaN passes only where the reference is NaN. On failure: the count, the
    worst element (by distance from the interval in bf16 steps) with its row and column, got, ref and the interval."""
    ref64 = np.asarray(ref64, dtype=np.float64)
    got = np.asarray(got_bits).astype(np.int32).reshape(ref64.shape) & 0xFFFF
    s = np.broadcast_to(np.asarray(slack, dtype=np.float64), ref64.shape)
    assert not np.isnan(s).any() and (s >= 0).all(), f"{what}: slack must be a number >= 0"
    lo_bits, hi_bits = bf16_rne(ref64 - s), bf16_rne(ref64 + s)
    k, lo, hi = bf16_key(got), bf16_key(lo_bits), bf16_key(hi_bits)
    ref_nan, got_nan = np.isnan(ref64), bf16_is_nan(got)
    dist = np.maximum(np.maximum(lo - k, k - hi), 0)
    dist = np.where(ref_nan, np.where(got_nan, 0, 1 << 16), np.where(got_nan, 1 << 16, dist))
    bad = dist > 0
    if not bad.any():
        return
    idx = np.unravel_index(int(np.argmax(dist)), dist.shape)
    pos = f"row {idx[0]} col {idx[1]}" if dist.ndim == 2 else f"index {tuple(int(i) for i in idx)}"
    raise AssertionError(
        f"{what}: {int(bad.sum())} of {bad.size} bf16 outputs outside the correctly rounded interval; worst at {pos}: "
        f"got {float(bf16_to_f64(got[idx]))!r} (0x{int(got[idx]):04x}), ref {float(ref64[idx])!r}, slack "
        f"{float(s[idx]):.3e}, interval [{float(bf16_to_f64(lo_bits[idx]))!r} (0x{int(lo_bits[idx]):04x}), "
        f"{float(bf16_to_f64(hi_bits[idx]))!r} "
        f"(0x{int(hi_bits[idx]):04x})], {int(dist[idx])} bf16 steps off")


def f32_bits_to_bf16_trunc(y32):
    """(mutant) bf16 by dropping the low 16 bits of the float32."""
    return (np.asarray(y32, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)


def bf16_half_away(y32):
    """(mutant) float32 -> bf16 rounding halves away from zero: right except on exact ties above an even value."""
    u = np.asarray(y32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x8000) >> 16).astype(np.uint16)


# ---- inputs -----------------------------------------------------------------------------------------------------
FAMILIES = ("plain", "offset", "tinyvar", "outlier")
WELL_CONDITIONED = ("plain", "tinyvar", "outlier")
# The outlier column (Whisper's massive activations). The outlier's own f32 error sets its row's E, in proportion to
# its normalised value times its gamma; at 300 the reference alone misses the 95 % sharpness share from D = 1280 up
# (0.84 at D = 1280, where gamma is 2.4 there), at 40 still (0.88), at 16 every tested (M, D) holds 0.96 or more
# (tests/test_ulp_ref.py::test_reference_alone_is_sharp checks it).
OUTLIER = 16.0


def ln_rows(family, M, D, seed=0):
    """Seeded f32 [M][D] rows of one input family."""
    z = np.random.default_rng([seed, FAMILIES.index(family), M, D]).standard_normal((M, D))
    if family == "plain":
        z = z * 3 + 1
    elif family == "offset":  # ill-conditioned: catches a one-pass variance
        z = z * 0.1 + 100
    elif family == "tinyvar":  # variance 1e-6: the epsilon matters
        z = z * 1e-3
    else:
        z[:, D // 3] = OUTLIER
    return z.astype(np.float32)


def ln_affine(D, seed=0):
    g = np.random.default_rng([seed, 77, D])
    return g.standard_normal(D).astype(np.float32), g.standard_normal(D).astype(np.float32)


def bf16_exact(x):
    """`x` rounded to bf16 and returned as (float32 values, uint16 bits)."""
    bits = bf16_rne(x)
    return bf16_to_f64(bits).astype(np.float32), bits


def gemm_inputs(M, N, K, seed=0):
    """bf16-exact A [M][K], W [N][K] scaled by K^-0.5, f32 bias 0.1 randn: (A32, Abits, W32, Wbits, bias)."""
    g = np.random.default_rng([seed, M, N, K])
    a32, abits = bf16_exact(g.standard_normal((M, K)))
    w32, wbits = bf16_exact(g.standard_normal((N, K)) * K ** -0.5)
    return a32, abits, w32, wbits, (g.standard_normal(N) * 0.1).astype(np.float32)


def tie_block(n, seed=0):
    """n float32 values that are exact bf16 ties (low half 0x8000), upper halves alternately even and odd, random
    sign and exponent (normal range)."""
    g = np.random.default_rng([seed, 99, n])
    hi = g.integers(0x3000, 0x4F00, n).astype(np.uint32)  # exponents 2^-31 .. 2^31
    hi = (hi & ~np.uint32(1)) | (np.arange(n, dtype=np.uint32) & 1)
    hi |= g.integers(0, 2, n).astype(np.uint32) << 15
    return ((hi << 16) | np.uint32(0x8000)).view(np.float32)


# ---- float64 references -----------------------------------------------------------------------------------------
def layer_norm64(x, gamma, beta, eps):
    """nn.LayerNorm in float64 (biased variance over the row, eps inside the square root). eps as the kernel gets it:
    the float32 value."""
    x = np.asarray(x, dtype=np.float64)
    mean = x.mean(-1, keepdims=True)
    d = x - mean
    var = (d * d).mean(-1, keepdims=True)
    return d / np.sqrt(var + np.float64(np.float32(eps))) * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64)


def gelu64(x):
    """0.5 x (1 + erf(x / sqrt 2)) in float64."""
    import torch

    x = np.asarray(x, dtype=np.float64)
    return 0.5 * x * (1.0 + torch.erf(torch.from_numpy(np.ascontiguousarray(x)) / np.sqrt(2.0)).numpy())


def gelu_prime64(x):
    """d/dx of gelu64: Phi(x) + x phi(x)."""
    import torch

    x = np.asarray(x, dtype=np.float64)
    cdf = 0.5 * (1.0 + torch.erf(torch.from_numpy(np.ascontiguousarray(x)) / np.sqrt(2.0)).numpy())
    return cdf + x * np.exp(-0.5 * x * x) / np.sqrt(2.0 * np.pi)


def gemm_bias64(a, w, bias=None):
    y = np.asarray(a, np.float64) @ np.asarray(w, np.float64).T
    return y if bias is None else y + np.asarray(bias, np.float64)


def pack_act_index(M, K):
    """tw_pack_act_idx restated: int64 [M][K] positions of element (m, k) of a packed activation (M <= 64 rows;
    rows 32..63 are a second 32-row block 32 K elements on)."""
    m = np.arange(M, dtype=np.int64).reshape(M, 1)
    k = np.arange(K, dtype=np.int64).reshape(1, K)
    return (m // 32) * 32 * K + (((k // 32) * 2 + (m // 16) % 2) * 64 + m % 16 + 16 * ((k // 8) % 4)) * 8 + k % 8


def pack_w_index(N, K):
    """tw_pack_w_idx restated: int64 [N][K] positions of W[n][k] in the packed weight (ceil(N / 16) 16 K elements)."""
    n = np.arange(N, dtype=np.int64).reshape(N, 1)
    k = np.arange(K, dtype=np.int64).reshape(1, K)
    return ((n // 16 * (K // 32) + k // 32) * 64 + n % 16 + 16 * ((k // 8) % 4)) * 8 + k % 8


def crosskv_index(S, B, D, H, L):
    """TW_EPI_CROSSKV restated: int64 [B S][L 2 D] positions in the [L][2][B][H][S][64] output."""
    m = np.arange(B * S, dtype=np.int64).reshape(-1, 1)
    n = np.arange(L * 2 * D, dtype=np.int64).reshape(1, -1)
    layer, rem = n // (2 * D), n % (2 * D)
    kv, hd = rem // D, rem % D
    h, d = hd // 64, hd % 64
    b, s = m // S, m % S
    return ((((layer * 2 + kv) * B + b) * H + h) * S + s) * 64 + d


def im2col_conv1_ref(feats, n_mels, row_map, seek, R, kpad, max_frames=None, feat_bits=None):
    """tw_im2col_conv1[_long] restated: bf16 bits [R 3000][kpad]. feats f32 [rows][n_mels][ld]; output row r reads
    feature row row_map[r] (None: r) from frame seek[r] (None: 0); column k = j n_mels + c holds bf16_rne of frame
    t + j - 1 of mel c where that frame lies in [0, min(3000, max_frames[row] - seek)) (max_frames None: 3000), else
    zero; columns >= 3 n_mels are zero. feat_bits: bf16_rne(feats) where the caller has it already (the rounding is
    element-wise, so it commutes with the gather)."""
    fb = bf16_rne(np.asarray(feats, dtype=np.float32)) if feat_bits is None else feat_bits
    out = np.zeros((R, 3000, kpad), np.uint16)
    for r in range(R):
        row = r if row_map is None else int(row_map[r])
        sk = 0 if seek is None else int(seek[r])
        valid = min(3000, (3000 if max_frames is None else int(max_frames[row])) - sk)
        if valid <= 0:
            continue
        seg = np.zeros((n_mels, 3002), np.uint16)  # seg[:, 1 + u] = frame u of the window
        seg[:, 1: 1 + valid] = fb[row, :, sk: sk + valid]
        for j in range(3):
            out[r, :, j * n_mels: (j + 1) * n_mels] = seg[:, j: j + 3000].T
    return out.reshape(R * 3000, kpad)


# ---- float32 restatements ---------------------------------------------------------------------------------------
_F = np.float32


def layer_norm32(x, gamma, beta, eps, ddof=0, one_pass=False, mean_ulps=0):
    """The straightforward float32 LayerNorm (numpy sums). mean_ulps moves the float32 mean that many ulps (ln_E).
    ddof = 1 and one_pass are the variance mutants (variance over D - 1; E[x^2] - mean^2)."""
    x = np.asarray(x, dtype=np.float32)
    D = x.shape[-1]
    mean = x.sum(-1, keepdims=True, dtype=np.float32) / _F(D)
    for _ in range(abs(mean_ulps)):
        mean = np.nextafter(mean, _F(np.inf if mean_ulps > 0 else -np.inf)).astype(np.float32)
    d = x - mean
    if one_pass:
        var = (x * x).sum(-1, keepdims=True, dtype=np.float32) / _F(D) - mean * mean
    else:
        var = (d * d).sum(-1, keepdims=True, dtype=np.float32) / _F(D - ddof)
    rstd = _F(1) / np.sqrt(var + _F(eps))
    return d * rstd * np.asarray(gamma, np.float32) + np.asarray(beta, np.float32)


def _butterfly64(v):
    """wave_sum: v += shfl_xor(v, o) for o = 32 .. 1 over the last axis (64 lanes); every lane ends with the sum."""
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ o]
    return v


def layer_norm32_kernel_order(x, gamma, beta, eps, skip_partial_group=False, affine_shift=0):
    """k_layernorm's float32 order: lane l holds float4 chunks c = l + 64 i; its partial sum adds (x + y) + (z + w) per
    chunk; the 64 lanes are summed by the xor butterfly; the variance is the second pass over the centred values.
    Mutants: skip_partial_group leaves the last, partly filled group of 64 chunks out of both statistics;
    affine_shift reads gamma / beta that many chunks on (wrapping)."""
    x = np.asarray(x, dtype=np.float32)
    M, D = x.shape
    nc = D // 4
    ngrp = -(-nc // 64)
    pad = np.zeros((M, ngrp * 64 * 4), np.float32)
    pad[:, :D] = x
    v = pad.reshape(M, ngrp, 64, 4)
    live = (np.arange(ngrp * 64).reshape(ngrp, 64) < nc)[None, :, :, None]
    stat = live
    if skip_partial_group and nc % 64:
        stat = live & (np.arange(ngrp) < ngrp - 1)[None, :, None, None]

    def lane_sums(t):  # [M][ngrp][64][4] -> [M][64]; chunks outside `stat` add an exact zero
        t = np.where(stat, t, _F(0))
        c = (t[..., 0] + t[..., 1]) + (t[..., 2] + t[..., 3])
        s = np.zeros((M, 64), np.float32)
        for i in range(ngrp):
            s = s + c[:, i]
        return s

    mean = (_butterfly64(lane_sums(v))[:, :1] / _F(D)).reshape(M, 1, 1, 1)
    d = v - mean
    var = _butterfly64(lane_sums(d * d))[:, :1] / _F(D)
    rstd = (_F(1) / np.sqrt(var + _F(eps))).reshape(M, 1, 1, 1)
    g = np.roll(np.asarray(gamma, np.float32).reshape(nc, 4), -affine_shift, axis=0).reshape(-1)
    b = np.roll(np.asarray(beta, np.float32).reshape(nc, 4), -affine_shift, axis=0).reshape(-1)
    y = (d * rstd).reshape(M, -1)[:, :D]
    return y * g + b


def erf_as32(x):
    """tw_common.h erf_fast in float32: Abramowitz & Stegun 7.1.26."""
    x = np.asarray(x, dtype=np.float32)
    z = np.abs(x)
    t = _F(1) / (_F(0.3275911) * z + _F(1))
    p = _F(1.061405429) * t + _F(-1.453152027)
    p = p * t + _F(1.421413741)
    p = p * t + _F(-0.284496736)
    p = p * t + _F(0.254829592)
    p = p * t
    e = np.exp2(-z * z * _F(1.4426950408889634)).astype(np.float32)
    return np.copysign(_F(1) - p * e, x).astype(np.float32)


def gelu_as32(x):
    x = np.asarray(x, dtype=np.float32)
    return _F(0.5) * x * (_F(1) + erf_as32(x * _F(0.70710678118654752)))


def gemm_bias32(a, w, bias=None, gelu=False):
    """float32 A . W^T + bias (+ the kernel's GELU) the way an MFMA chain accumulates it: the dot product of each
    32-deep K block (v_mfma_f32_16x16x32_bf16's depth; taken in float64 and rounded once, so the result does not
    depend on the host's BLAS) added to a float32 accumulator, block after block; then the bias in float32."""
    a64, w64 = np.asarray(a, np.float64), np.asarray(w, np.float64)
    K = a64.shape[1]
    y = np.zeros((a64.shape[0], w64.shape[0]), np.float32)
    for k0 in range(0, K, 32):
        y = y + (a64[:, k0: min(k0 + 32, K)] @ w64[:, k0: min(k0 + 32, K)].T).astype(np.float32)
    if bias is not None:
        y = y + np.asarray(bias, np.float32)
    return gelu_as32(y) if gelu else y


def resid_sum32(x, bias, parts, nparts, order="kernel"):
    """The residual update in float32 in the kernel's documented order, ((x + bias) + p0) + p1 + ... (bias None: no
    bias; parts f32 [>= nparts][M][D]). order="grouped" is the mutant x + (bias + sum of parts)."""
    x = np.asarray(x, dtype=np.float32)
    if order == "kernel":
        a = x.copy()
        if bias is not None:
            a = a + np.asarray(bias, np.float32)
        for p in range(nparts):
            a = a + np.asarray(parts[p], np.float32)
        return a
    t = np.zeros(x.shape[-1], np.float32) if bias is None else np.asarray(bias, np.float32)
    t = np.broadcast_to(t, x.shape)
    for p in range(nparts):
        t = t + np.asarray(parts[p], np.float32)
    return x + t


def layer_norm32_block_order(x, gamma, beta, eps):
    """tw_row_ln_store's float32 order (k_resid_ln, D <= 4096): 256 threads, thread t holds float4 chunks c = t + 256 i;
    each of the 4 waves sums its 64 threads by the xor butterfly, then the four wave sums are added in order,
    ((r0 + r1) + r2) + r3. Not one of the restatements behind ln_E: a third float32 LayerNorm to check against it."""
    x = np.asarray(x, dtype=np.float32)
    M, D = x.shape
    nc = D // 4
    ngrp = -(-nc // 256)
    pad = np.zeros((M, ngrp * 256 * 4), np.float32)
    pad[:, :D] = x
    v = pad.reshape(M, ngrp, 256, 4)
    live = (np.arange(ngrp * 256).reshape(ngrp, 256) < nc)[None, :, :, None]

    def block_sum(t):
        t = np.where(live, t, _F(0))
        c = (t[..., 0] + t[..., 1]) + (t[..., 2] + t[..., 3])
        s = np.zeros((M, 256), np.float32)
        for i in range(ngrp):
            s = s + c[:, i]
        w = _butterfly64(s.reshape(M, 4, 64))[:, :, 0]
        return (((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]).reshape(M, 1, 1, 1)

    mean = block_sum(v) / _F(D)
    d = v - mean
    rstd = _F(1) / np.sqrt(block_sum(d * d) / _F(D) + _F(eps))
    y = (d * rstd).reshape(M, -1)[:, :D]
    return y * np.asarray(gamma, np.float32) + np.asarray(beta, np.float32)


def ln_E(x, gamma, beta, eps, ref64):
    """E of a LayerNorm, per row ([M, 1]): the largest |float32 restatement - float64 reference| over the row and over
    four float32 restatements: numpy's sums, the kernel's order (float4 chunks per lane, xor butterfly), and numpy's
    with its float32 mean one ulp up and one ulp down. The last two are there because the error of a row with a large
    mean ("offset") is almost all the mean's: common to the whole row and, by luck, next to nothing in a row whose
    exact mean happens to lie beside a float32. No float32 sum of D terms is good to better than an ulp of its result,
    so a restatement that is one ulp off in the mean is as faithful as the lucky one; without it the kernel-order
    restatement itself needed margins of 45-160 in such rows. In the other families the two change E by little."""
    ys = (layer_norm32(x, gamma, beta, eps), layer_norm32_kernel_order(x, gamma, beta, eps),
          layer_norm32(x, gamma, beta, eps, mean_ulps=1), layer_norm32(x, gamma, beta, eps, mean_ulps=-1))
    return np.max([row_E(y, ref64) for y in ys], axis=0)


def row_E(y32, ref64):
    """E per row: [M, 1] largest |float32 restatement - float64 reference|."""
    return np.abs(np.asarray(y32, np.float64) - ref64).max(-1, keepdims=True)


# ---- cases shared by the CPU and the GPU tests -------------------------------------------------------------------
LN_EPS = 1e-5


def ln_case(family, M, D, seed=0):
    """Inputs, float64 reference and E of one LayerNorm case: dict x, g, b, ref, E."""
    x = ln_rows(family, M, D, seed)
    g, b = ln_affine(D, seed)
    return ln_case_of(x, g, b)


def ln_case_of(x, g, b):
    ref = layer_norm64(x, g, b, LN_EPS)
    return {"x": x, "g": g, "b": b, "ref": ref, "E": ln_E(x, g, b, LN_EPS, ref)}


_GEMM_CACHE = {}


def gemm_case(M, N, K, seed=0):
    """Inputs, float64 references and E of A . W^T + bias and of its GELU, computed once per shape: dict A, Abits, W,
    Wbits, bias, ref, E, ref_gelu, E_gelu.

    E is one number over the output: the largest |gemm_bias32 - ref|. A float32 accumulation error is absolute, so
    one number fits the linear epilogues. It does not fit GELU, which maps a tenth of these pre-activations to
    |y| < 0.04: the largest error over the output (about 1e-6) is more than 2^-12 |y| on 3-9 % of them, and the
    reference alone then misses the sharpness share (0.91-0.97). E_gelu is therefore per element, the same E carried
    through GELU plus the float32 GELU restatement's own error:

        E_gelu = E |gelu'(x)| + c |x| + 4 E^2

    x the float64 pre-activation; c the largest |gelu_as32(x32) - gelu64(x32)| / |x32| over the output's own
    pre-activations x32 = float32(x) (the formula's error grows with |x|: 0.5 |x| times the erf error, on either
    side; measured 2.6e-7 to 3.1e-7); 4 E^2 bounds the second-order term at margin 8 (|gelu''| <= 0.8, so a
    pre-activation error d <= 8 E moves GELU by at most |gelu'| d + 0.4 d^2 <= 8 (E |gelu'| + 4 E^2))."""
    key = (M, N, K, seed)
    if key not in _GEMM_CACHE:
        a32, abits, w32, wbits, bias = gemm_inputs(M, N, K, seed)
        ref = gemm_bias64(a32, w32, bias)
        refg = gelu64(ref)
        c = {"A": a32, "Abits": abits, "W": w32, "Wbits": wbits, "bias": bias, "ref": ref, "ref_gelu": refg,
             "E": float(np.abs(gemm_bias32(a32, w32, bias) - ref).max()),
             "E_gelu": None}
        x32 = ref.astype(np.float32)
        own = np.abs(gelu_as32(x32).astype(np.float64) - gelu64(x32))
        c["gelu_c"] = float((own / np.maximum(np.abs(x32), np.float32(1e-30))).max())
        c["E_gelu"] = c["E"] * np.abs(gelu_prime64(ref)) + c["gelu_c"] * np.abs(ref) + 4.0 * c["E"] ** 2
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _GEMM_CACHE[key] = c
    return _GEMM_CACHE[key]
