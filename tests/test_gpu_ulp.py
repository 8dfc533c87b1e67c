"""The kernels that compute in f32 and store bf16, pinned on the MI355X to float64 within the correct bf16 rounding
(tests/ulp_ref.py: the interval criterion, slack = 8 E from CPU float32 restatements; tests/test_ulp_ref.py shows on
the CPU that a truncating store, a variance over D - 1, eps 1e-6, a one-pass variance, skipped or shifted chunks, a
regrouped residual sum, a dropped K tile and a late bias all fail it). Data-movement kernels (im2col, embedding,
checkpoint conversion) and the residual update are exact: compared bit for bit.

Every output buffer lies between two canary regions (one row, or 64 elements) that must come back unchanged, and what
an entry point documents as not written is compared bit for bit. Each test prints one `ulp-pin` line per kernel,
shape and input family: the margin the device needed (the largest distance from the float64 reference to the reals
that round to the device's bf16, over E; 0 = every output is the correctly rounded reference) and the sharpness
share (elements with slack <= 2^-12 |ref|). One run's lines are kept in profiles/ulp_pins.txt."""
import ctypes

import numpy as np
import pytest
import torch

import ulp_ref as U
from twamd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = U.LN_EPS
CANARY = 0xA5  # every byte of a guarded buffer before the kernel runs


def S():
    return torch.cuda.current_stream().cuda_stream


def dev(a):
    """numpy -> device tensor of the same bits (uint16 travels as int16)."""
    a = np.array(a, order="C")  # (a copy: the cached cases are read-only)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a).to(DEV)


def bits16(t):
    return t.cpu().numpy().view(np.uint16)


def bits32(t):
    return t.cpu().numpy().view(np.uint32)


class Guarded:
    """n elements of `dtype` on the device between two canary regions of `pad` elements; everything starts as the
    canary byte. `.t` is the interior (what the kernel gets: pad * itemsize keeps 16-byte alignment for f32 rows of
    D % 4 == 0 elements and 8-byte alignment for bf16 rows)."""

    def __init__(self, n, pad, dtype):
        size = torch.empty(0, dtype=dtype).element_size()
        self.raw = torch.full(((n + 2 * pad) * size,), CANARY, dtype=torch.uint8, device=DEV)
        self.lo, self.hi = pad * size, (pad + n) * size
        self.t = self.raw[self.lo: self.hi].view(dtype)
        assert self.t.data_ptr() % (16 if (pad * size) % 16 == 0 else 8) == 0

    def ptr(self):
        return self.t.data_ptr()

    def check(self, what):
        torch.cuda.synchronize()
        assert bool((self.raw[: self.lo] == CANARY).all()), f"{what}: wrote in front of its output"
        assert bool((self.raw[self.hi:] == CANARY).all()), f"{what}: wrote behind its output"

    def untouched(self):
        return bool((self.raw == CANARY).all())


def canary_like(n, np_dtype):
    return np.full(n * np.dtype(np_dtype).itemsize, CANARY, np.uint8).view(np_dtype)


def pin(kernel, shape, family, margin, share):
    print(f"ulp-pin {kernel} shape={shape} family={family} margin_needed={margin:.3f} sharp_share={share:.3f}")


def check_rounded(got_bits, ref, E, what, sharp):
    """The interval criterion at margin 8; returns (margin needed, sharpness share). sharp: assert the 95 % share."""
    slack = U.MARGIN * E
    share = U.sharp_share(ref, slack)
    need = U.margin_needed(got_bits, ref, E)
    try:
        U.assert_bf16_correctly_rounded(got_bits, ref, slack, what)
    except AssertionError as e:
        raise AssertionError(f"{e} [margin needed {need:.2f}, sharp share {share:.3f}]") from None
    if sharp:
        assert share >= U.SHARP_SHARE, f"{what}: slack <= 2^-12 |ref| on {share:.3f} of the elements only"
    return need, share


class FamilyPins:
    """The residual-LayerNorm tests' records by input family of x: the worst margin needed, and the sharpness share
    over all the elements of the family's cases in the test. The share is asserted over that pool and not case by
    case: the cases include single rows of a few hundred elements, where one row's E (a maximum over the row) and a
    count of a dozen elements decide between 0.94 and 0.98 whatever the inputs are (measured on the CPU: plain and
    outlier rows alike); the issue's remedy for such noise is more rows, and the pool is those rows."""

    def __init__(self):
        self.by = {}

    def add(self, fam, need, ref, E):
        w, ok, n = self.by.get(fam, (0.0, 0, 0))
        self.by[fam] = (max(w, need), ok + int((U.MARGIN * E <= U.SHARP * np.abs(ref)).sum()), n + ref.size)

    def finish(self, kernel, shape):
        for fam, (w, ok, n) in self.by.items():
            pin(kernel, shape, fam, w, ok / n)
            if fam != "offset":
                assert ok / n >= U.SHARP_SHARE, f"{kernel} {shape} {fam}: slack <= 2^-12 |ref| on {ok / n:.3f} only"


# ---- tw_layernorm ------------------------------------------------------------------------------------------------
LN_D = (256, 260, 384, 388, 512, 768, 1024, 1280, 1536, 1796, 2048, 2052, 4096)


@pytest.mark.parametrize("D", LN_D)
def test_layernorm(D):
    """k_layernorm<1, 2, 3, 4, 5, 6, 8, 16> (every case of the launcher's switch), widths whose last group of 64 float4
    chunks is partly filled (260, 388, 1796, 2052), 1 / 5 / 33 rows (a block holds 4), the four input families."""
    for fam in U.FAMILIES:
        worst, low = 0.0, 1.0
        for M in (1, 5, 33):
            c = U.ln_case(fam, M, D)
            x, g, b = dev(c["x"]), dev(c["g"]), dev(c["b"])
            out = Guarded(M * D, D, torch.int16)
            _lib.call("tw_layernorm", x.data_ptr(), g.data_ptr(), b.data_ptr(), M, D, EPS, out.ptr(), S())
            out.check(f"tw_layernorm M={M} D={D}")
            need, share = check_rounded(bits16(out.t).reshape(M, D), c["ref"], c["E"],
                                        f"tw_layernorm {fam} M={M} D={D}", fam in U.WELL_CONDITIONED)
            worst, low = max(worst, need), min(low, share)
        pin("tw_layernorm", f"M=1,5,33 D={D}", fam, worst, low)


def test_layernorm_lds_pad_is_bit_identical():
    """tw_layernorm_set_lds_pad only reserves LDS: the same bits at 16 and 64 KiB as at 0; out of range is refused."""
    M, D = 33, 1280
    c = U.ln_case("plain", M, D)
    x, g, b = dev(c["x"]), dev(c["g"]), dev(c["b"])
    got = {}
    try:
        for kib in (0, 16, 64):
            _lib.call("tw_layernorm_set_lds_pad", kib)
            out = Guarded(M * D, D, torch.int16)
            _lib.call("tw_layernorm", x.data_ptr(), g.data_ptr(), b.data_ptr(), M, D, EPS, out.ptr(), S())
            out.check(f"tw_layernorm lds pad {kib}")
            got[kib] = bits16(out.t)
        for bad in (-1, 65):
            with pytest.raises(_lib.TwError):
                _lib.call("tw_layernorm_set_lds_pad", bad)
    finally:
        _lib.call("tw_layernorm_set_lds_pad", 0)
    assert np.array_equal(got[16], got[0]) and np.array_equal(got[64], got[0])


# ---- tw_resid_layernorm, _packed, _packed_to ---------------------------------------------------------------------
NPARTS = (0, 1, 3, 4, 5, 16)
RESID_D = (1280, 384, 512, 768, 1024, 4096)  # 1280: the one-wave kernel; the others: the 256-thread block kernel


def _resid_inputs(D):
    """parts f32 [16][64][D], bias, gamma, beta of one width (a case takes the first nparts partials and M rows)."""
    g = np.random.default_rng([11, D])
    parts, bias = g.standard_normal((16, 64, D)).astype(np.float32), g.standard_normal(D).astype(np.float32)
    return (parts, bias) + U.ln_affine(D, 1)


def _resid_combos(im):
    """(nparts, with_bias, family) for the im-th row count: every (nparts, bias) pair, the family of x rotating out of
    step with both (each family meets a bias, a NULL bias and most partial counts); and with no partials and no bias,
    where the LayerNorm sees the family's own rows (the tiny-variance rows keep their variance only there), all four
    families."""
    out = []
    for ip, nparts in enumerate(NPARTS):
        for ib, with_bias in enumerate((True, False)):
            if nparts == 0 and not with_bias:
                out += [(0, False, fam) for fam in U.FAMILIES]
            else:
                out.append((nparts, with_bias, U.FAMILIES[(2 * ip + ib + ip // 2 + im) % 4]))
    return out


@pytest.mark.parametrize("D", RESID_D + (260,))
def test_resid_layernorm(D):
    """tw_resid_layernorm (row-major): x becomes the float32 sum ((x + bias) + p0) + p1 + ... bit for bit, for 0 to 16
    partials with and without a bias; the bf16 output is the correctly rounded LayerNorm of that float32 row; with
    gamma NULL only the residual update runs and out is not written. D = 260: D % 4 alone, a partly filled chunk
    group in the block kernel."""
    parts_all, bias_np, g_np, b_np = _resid_inputs(D)
    bias_d, g_d, b_d = dev(bias_np), dev(g_np), dev(b_np)
    pins = FamilyPins()
    case = 0
    for im, M in enumerate((1, 24, 33)):
        parts_d = dev(parts_all[:, :M])
        for nparts, with_bias, fam in _resid_combos(im):
            for with_gamma in (True, False):
                if not with_gamma and M != 24:
                    continue
                case += 1
                what = f"tw_resid_layernorm {fam} M={M} D={D} nparts={nparts} bias={with_bias} gamma={with_gamma}"
                x_np = U.ln_rows(fam, M, D, seed=case)
                want = U.resid_sum32(x_np, bias_np if with_bias else None, parts_all[:, :M], nparts)
                x = Guarded(M * D, D, torch.float32)
                x.t.copy_(dev(x_np).reshape(-1))
                out = Guarded(M * D, D, torch.int16)
                _lib.call("tw_resid_layernorm", x.ptr(), parts_d.data_ptr() if nparts else None, nparts,
                          bias_d.data_ptr() if with_bias else None, g_d.data_ptr() if with_gamma else None,
                          b_d.data_ptr() if with_gamma else None, M, D, EPS, out.ptr(), S())
                x.check(what)
                out.check(what)
                assert np.array_equal(bits32(x.t).reshape(M, D), want.view(np.uint32)), f"{what}: residual sum"
                if not with_gamma:
                    assert out.untouched(), f"{what}: out written with gamma NULL"
                    continue
                c = U.ln_case_of(want, g_np, b_np)
                need, _ = check_rounded(bits16(out.t).reshape(M, D), c["ref"], c["E"], what, False)
                pins.add(fam, need, c["ref"], c["E"])
    pins.finish("tw_resid_layernorm", f"M=1,24,33 D={D} nparts=0..16")


@pytest.mark.parametrize("form", ["packed", "packed_to"])
@pytest.mark.parametrize("D", RESID_D)
def test_resid_layernorm_packed(D, form):
    """tw_resid_layernorm_packed / _packed_to: the same sum and LayerNorm with the output in the packed activation
    layout (row 32 starts the second 32-row block), equal bit for bit to the row-major kernel's through the restated
    index; packed rows M..63 are not written; _packed_to leaves x as it was and writes the sum to x_out."""
    parts_all, bias_np, g_np, b_np = _resid_inputs(D)
    bias_d, g_d, b_d = dev(bias_np), dev(g_np), dev(b_np)
    idx64 = U.pack_act_index(64, D)
    pins = FamilyPins()
    case = 0
    for im, M in enumerate((1, 16, 17, 32, 33, 64)):
        parts_d = dev(parts_all[:, :M])
        idx = idx64[:M]
        rest = np.ones(64 * D, bool)
        rest[idx.reshape(-1)] = False
        for nparts, with_bias, fam in _resid_combos(im):
            case += 1
            what = f"tw_resid_layernorm_{form} {fam} M={M} D={D} nparts={nparts} bias={with_bias}"
            x_np = U.ln_rows(fam, M, D, seed=case)
            want = U.resid_sum32(x_np, bias_np if with_bias else None, parts_all[:, :M], nparts)
            pp = parts_d.data_ptr() if nparts else None
            bp = bias_d.data_ptr() if with_bias else None
            out = Guarded(64 * D, 64, torch.int16)
            if form == "packed":
                x = Guarded(M * D, D, torch.float32)
                x.t.copy_(dev(x_np).reshape(-1))
                _lib.call("tw_resid_layernorm_packed", x.ptr(), pp, nparts, bp, g_d.data_ptr(), b_d.data_ptr(), M,
                          D, EPS, out.ptr(), S())
                x.check(what)
                new_x = x.t
            else:
                x_in = dev(x_np)
                xo = Guarded(M * D, D, torch.float32)
                _lib.call("tw_resid_layernorm_packed_to", x_in.data_ptr(), xo.ptr(), pp, nparts, bp, g_d.data_ptr(),
                          b_d.data_ptr(), M, D, EPS, out.ptr(), S())
                xo.check(what)
                assert np.array_equal(bits32(x_in), x_np.view(np.uint32)), f"{what}: x was written"
                new_x = xo.t
            out.check(what)
            assert np.array_equal(bits32(new_x).reshape(M, D), want.view(np.uint32)), f"{what}: residual sum"
            packed = bits16(out.t)
            assert np.array_equal(packed[rest], canary_like(int(rest.sum()), np.uint16)), f"{what}: rows M..63"
            got = packed[idx]
            c = U.ln_case_of(want, g_np, b_np)
            need, _ = check_rounded(got, c["ref"], c["E"], what, False)
            pins.add(fam, need, c["ref"], c["E"])
            # the row-major kernel on the same inputs: the same bits
            x2 = dev(x_np)
            rm = Guarded(M * D, D, torch.int16)
            _lib.call("tw_resid_layernorm", x2.data_ptr(), pp, nparts, bp, g_d.data_ptr(), b_d.data_ptr(), M, D,
                      EPS, rm.ptr(), S())
            rm.check(what + " (row-major)")
            assert np.array_equal(bits16(rm.t).reshape(M, D), got), f"{what}: differs from the row-major kernel"
    pins.finish(f"tw_resid_layernorm_{form}", f"M=1..64 D={D} nparts=0..16")


# ---- bf16 epilogues of tw_gemm_bf16 ------------------------------------------------------------------------------
GEMM_SHAPES = [(129, 200, 64), (300, 384, 256), (257, 768, 384), (24, 1280, 1280), (7, 384, 384)]


@pytest.fixture(params=[0, 1], ids=["f32img", "tr"])
def gemm_epilogue(request):
    _lib.call("tw_gemm_set_epilogue", request.param)
    try:
        yield request.param
    finally:
        _lib.call("tw_gemm_set_epilogue", 0)


@pytest.fixture(params=[1, 5, 6], ids=["big", "8p", "8pp"])
def gemm_variant(request):
    _lib.call("tw_gemm_set_variant", request.param)
    try:
        yield request.param
    finally:
        _lib.call("tw_gemm_set_variant", 1)


@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_gemm_bf16_epilogues(M, N, K, gemm_variant, gemm_epilogue):
    """TW_EPI_BF16 and TW_EPI_GELU_BF16 of k_gemm_big / k_gemm_8p / k_gemm_8pp in both epilogue forms (and of the
    skinny kernel at M <= 32) against the float64 product of the bf16-exact operands: ragged right edge (N = 200),
    partial tiles, one and several K tiles. E of the linear epilogue is one number over the output (the float32
    MFMA-order restatement); GELU's is that E carried through GELU per element plus the float32 GELU's own error
    (ulp_ref.gemm_case: with one number over the output GELU's many near-zero outputs keep the reference alone at a
    sharpness share of 0.91-0.97). The 95 % share is required of both."""
    c = U.gemm_case(M, N, K)
    A, W, bias = dev(c["Abits"]), dev(c["Wbits"]), dev(c["bias"])
    for epi, name, ref, E in ((_lib.TW_EPI_BF16, "bf16", c["ref"], c["E"]),
                              (_lib.TW_EPI_GELU_BF16, "gelu_bf16", c["ref_gelu"], c["E_gelu"])):
        what = f"tw_gemm_bf16 {name} {M}x{N}x{K} variant {gemm_variant} epilogue {gemm_epilogue}"
        out = Guarded(M * N, 64, torch.int16)
        _lib.call("tw_gemm_bf16", A.data_ptr(), W.data_ptr(), M, N, K, K, K, epi, out.ptr(), N, bias.data_ptr(), None,
                  0, None, S())
        out.check(what)
        need, share = check_rounded(bits16(out.t).reshape(M, N), ref, E, what, True)
        pin(f"tw_gemm_bf16[{name},v{gemm_variant},e{gemm_epilogue}]", f"{M}x{N}x{K}", "gemm", need, share)


def test_gemm_crosskv_epilogue(gemm_variant, gemm_epilogue):
    """TW_EPI_CROSSKV: the same rounding, scattered to [L][2][B][H][S][64] (S = 96, B = 2, D = 128, H = 2, L = 2)."""
    Sx, B, D, H, L = 96, 2, 128, 2, 2
    M, N, K = B * Sx, L * 2 * D, D
    c = U.gemm_case(M, N, K)
    A, W, bias = dev(c["Abits"]), dev(c["Wbits"]), dev(c["bias"])
    what = f"tw_gemm_bf16 crosskv {M}x{N}x{K} variant {gemm_variant} epilogue {gemm_epilogue}"
    out = Guarded(M * N, 64, torch.int16)
    geom = (ctypes.c_int * 4)(Sx, B, D, H)
    _lib.call("tw_gemm_bf16", A.data_ptr(), W.data_ptr(), M, N, K, K, K, _lib.TW_EPI_CROSSKV, out.ptr(), N,
              bias.data_ptr(), None, 0, geom, S())
    out.check(what)
    idx = U.crosskv_index(Sx, B, D, H, L)
    assert len(np.unique(idx)) == M * N
    need, share = check_rounded(bits16(out.t)[idx], c["ref"], c["E"], what, True)
    pin(f"tw_gemm_bf16[crosskv,v{gemm_variant},e{gemm_epilogue}]", f"{M}x{N}x{K}", "gemm", need, share)


# ---- bf16 epilogues of tw_gemv_packed ----------------------------------------------------------------------------
@pytest.fixture(params=[0, 1], ids=["gemv_pc", "gemv_q"])
def gemv_variant(request):
    _lib.call("tw_gemv_set_variant", request.param)
    try:
        yield request.param
    finally:
        _lib.call("tw_gemv_set_variant", 0)


@pytest.mark.parametrize("a_packed", [0, 1])
@pytest.mark.parametrize("M,N,K", [(24, 1280, 1280), (13, 1536, 384), (33, 1536, 384), (64, 1296, 1280)])
def test_gemv_packed_bf16_epilogues(M, N, K, a_packed, gemv_variant):
    """TW_EPI_BF16 (row-major) and TW_EPI_GELU_PACKED (packed activation out, rows M..63 not written) of the packed
    GEMV, from a packed and a row-major A. N = 1296 is no multiple of 32, which GELU_PACKED refuses (its output is the
    next GEMV's K). E and the sharpness share as in test_gemm_bf16_epilogues."""
    c = U.gemm_case(M, N, K)
    wp = np.zeros(-(-N // 16) * 16 * K, np.uint16)
    wp[U.pack_w_index(N, K).reshape(-1)] = c["Wbits"].reshape(-1)
    if a_packed:
        a = np.zeros(64 * K, np.uint16)
        a[U.pack_act_index(M, K).reshape(-1)] = c["Abits"].reshape(-1)
    else:
        a = c["Abits"]
    A, Wp, bias = dev(a), dev(wp), dev(c["bias"])
    tag = f"{M}x{N}x{K} a_packed {a_packed} variant {gemv_variant}"
    out = Guarded(M * N, 64, torch.int16)
    _lib.call("tw_gemv_packed", A.data_ptr(), a_packed, K, Wp.data_ptr(), M, N, K, _lib.TW_EPI_BF16, out.ptr(), N,
              bias.data_ptr(), 1, S())
    out.check("tw_gemv_packed bf16 " + tag)
    need, share = check_rounded(bits16(out.t).reshape(M, N), c["ref"], c["E"], "tw_gemv_packed bf16 " + tag, True)
    pin(f"tw_gemv_packed[bf16,a{a_packed},v{gemv_variant}]", f"{M}x{N}x{K}", "gemm", need, share)
    out = Guarded(64 * N, 64, torch.int16)
    args = (A.data_ptr(), a_packed, K, Wp.data_ptr(), M, N, K, _lib.TW_EPI_GELU_PACKED, out.ptr(), 0,
            bias.data_ptr(), 1, S())
    if N % 32:
        with pytest.raises(_lib.TwError):
            _lib.call("tw_gemv_packed", *args)
        torch.cuda.synchronize()
        assert out.untouched()
        return
    _lib.call("tw_gemv_packed", *args)
    out.check("tw_gemv_packed gelu_packed " + tag)
    packed = bits16(out.t)
    idx = U.pack_act_index(M, N)
    rest = np.ones(64 * N, bool)
    rest[idx.reshape(-1)] = False
    assert np.array_equal(packed[rest], canary_like(int(rest.sum()), np.uint16)), "rows M..63 written"
    need, share = check_rounded(packed[idx], c["ref_gelu"], c["E_gelu"], "tw_gemv_packed gelu_packed " + tag, True)
    pin(f"tw_gemv_packed[gelu_packed,a{a_packed},v{gemv_variant}]", f"{M}x{N}x{K}", "gemm", need, share)


# ---- conv-stem im2col: exact bits --------------------------------------------------------------------------------
def _feats(rows, n_mels, ld, seed):
    """randn features with exact bf16 ties at the first, the last and 64 inner frames of every row."""
    f = np.random.default_rng([seed, n_mels, ld]).standard_normal((rows, n_mels, ld)).astype(np.float32)
    for lo in (0, 1490, ld - 64):
        f[:, :, lo: lo + 64] = U.tie_block(rows * n_mels * 64, seed=lo).reshape(rows, n_mels, 64)
    return f


@pytest.mark.parametrize("n_mels,kpad", [(80, 256), (128, 384), (128, 448)])
def test_im2col_conv1(n_mels, kpad):
    """tw_im2col_conv1 against im2col_conv1_ref: the bf16 RNE of the f32 feature (ties included), the three taps with
    the zero frame on either side, the seek window cut at 3000 frames (seek 3000: all zero), a row map that permutes
    and repeats, NULL row_map / seek, zero pad columns (kpad = 3 n_mels and beyond)."""
    R = 3
    f = _feats(4, n_mels, 3000, 3)
    fb = U.bf16_rne(f)
    F = dev(f)
    perm = [3, 1, 3]
    for row_map, seek in ((perm, [0, 1, 1499]), (perm, [2999, 3000, 1]), (None, [3000, 3000, 3000]),
                          (None, [1499, 0, 2999]), (perm, None), (None, None)):
        what = f"tw_im2col_conv1 n_mels={n_mels} kpad={kpad} row_map={row_map} seek={seek}"
        rm = None if row_map is None else dev(np.array(row_map, np.int32))
        sk = None if seek is None else dev(np.array(seek, np.int32))
        out = Guarded(R * 3000 * kpad, 64, torch.int16)
        _lib.call("tw_im2col_conv1", F.data_ptr(), n_mels, _lib.ptr(rm) or None, _lib.ptr(sk) or None, R, kpad,
                  out.ptr(), S())
        out.check(what)
        want = U.im2col_conv1_ref(f, n_mels, row_map, seek, R, kpad, feat_bits=fb)
        got = bits16(out.t).reshape(R * 3000, kpad)
        assert np.array_equal(got, want), f"{what}: {int((got != want).sum())} elements differ"
        assert not got[:, 3 * n_mels:].any()
        if seek == [3000, 3000, 3000]:
            assert not got.any()
    print(f"ulp-pin tw_im2col_conv1 shape=R=3 n_mels={n_mels} kpad={kpad} family=randn+ties exact")


@pytest.mark.parametrize("ld", [3000, 7013])
def test_im2col_conv1_long(ld):
    """tw_im2col_conv1_long: feature rows of ld frames, a row's valid frames end at max_frames[row] - seek: below, at
    and (ld = 7013) above seek + 3000, one valid frame, and a seek past the row's end (all zero)."""
    n_mels, kpad = 80, 256
    f = _feats(4, n_mels, ld, 4)
    fb = U.bf16_rne(f)
    F = dev(f)
    if ld == 3000:
        # (max_frames is per feature row) rows: at; below; seek past the row's end (all zero); 500 frames left
        cases = [([2, 0, 3, 1], [2000, 3000, 3000, 2000], [0, 0, 2500, 2500]),
                 (None, [3000, 2000, 1, 3000], [2999, 1999, 0, 0])]  # one valid frame (three ways); at
    else:
        cases = [([1, 0, 3, 2], [3500, 5000, 7013, 7000], [2000, 1000, 6999, 3000]),  # at; below; one frame; above
                 (None, [7013, 7013, 3000, 2999], [4013, 4012, 0, 0])]  # at the row's end; above by 1; at; below by 1
    for row_map, maxf, seek in cases:
        what = f"tw_im2col_conv1_long ld={ld} row_map={row_map} max_frames={maxf} seek={seek}"
        rm = None if row_map is None else dev(np.array(row_map, np.int32))
        mf, sk = dev(np.array(maxf, np.int32)), dev(np.array(seek, np.int32))
        out = Guarded(4 * 3000 * kpad, 64, torch.int16)
        _lib.call("tw_im2col_conv1_long", F.data_ptr(), n_mels, ld, mf.data_ptr(), _lib.ptr(rm) or None, sk.data_ptr(),
                  4, kpad, out.ptr(), S())
        out.check(what)
        want = U.im2col_conv1_ref(f, n_mels, row_map, seek, 4, kpad, max_frames=maxf, feat_bits=fb)
        got = bits16(out.t).reshape(4 * 3000, kpad)
        assert np.array_equal(got, want), f"{what}: {int((got != want).sum())} elements differ"
    print(f"ulp-pin tw_im2col_conv1_long shape=R=4 n_mels={n_mels} kpad={kpad} ld={ld} family=randn+ties exact")


# ---- tw_embed_decoder: exact f32 bits ----------------------------------------------------------------------------
@pytest.mark.parametrize("D", [100, 384, 1280])
def test_embed_decoder(D):
    """x[b] = embed_tokens[ids[b]] + embed_positions[pos[b]]: the sum of two bf16 values rounded once to f32, with the
    first and the last row of both tables and repeated ids, for 1, 24 and 64 rows."""
    V, P = 51866, 448
    gen = torch.Generator(device=DEV).manual_seed(D)
    tok = (torch.randn(V, D, device=DEV, generator=gen) * 3).to(torch.bfloat16)
    # positions 1 to 1e-7 times as large by column: two bf16 values more than 2^16 apart do not add exactly in f32
    col = 10.0 ** -(torch.arange(D, device=DEV) % 8).float()
    pos = (torch.randn(P, D, device=DEV, generator=gen) * col).to(torch.bfloat16)
    g = np.random.default_rng(D)
    for B in (1, 24, 64):
        ids = g.integers(0, V, B).astype(np.int32)
        pp = g.integers(0, P, B).astype(np.int32)
        ids[0], pp[0] = V - 1, P - 1
        if B > 1:
            ids[1], pp[1] = 0, 0
            ids[B // 2:] = ids[B // 2 - 1]  # repeated ids at different positions
            pp[-1] = pp[-2]  # and one fully repeated row
        ids_d, pp_d = dev(ids), dev(pp)
        x = Guarded(B * D, D, torch.float32)
        _lib.call("tw_embed_decoder", tok.data_ptr(), pos.data_ptr(), ids_d.data_ptr(), pp_d.data_ptr(), B, D, x.ptr(),
                  S())
        x.check(f"tw_embed_decoder B={B} D={D}")
        te = tok[ids_d.long()].float().cpu().numpy().astype(np.float64)
        pe = pos[pp_d.long()].float().cpu().numpy().astype(np.float64)
        want = (te + pe).astype(np.float32)  # the float64 sum of two bf16 values is exact: one rounding
        assert (te + pe != want).any()  # (the inputs do make it round)
        assert np.array_equal(bits32(x.t).reshape(B, D), want.view(np.uint32)), f"tw_embed_decoder B={B} D={D}"
    print(f"ulp-pin tw_embed_decoder shape=B=1,24,64 D={D} family=randn exact")


# ---- tw_f32_to_bf16: exact bits ----------------------------------------------------------------------------------
_FMAX = np.float32(3.4028234663852886e38)
_SPECIAL = np.concatenate([
    np.array([0x3F818000, 0x3F808000], np.uint32).view(np.float32),  # ties: odd upper half (up), even (down)
    np.array([-0.0, np.inf, np.nan, _FMAX, 1e-40, 0.0, -np.inf, -_FMAX, -1e-40, 1.401298464324817e-45,
              2.0 ** -126, 1.5 * 2.0 ** -124, -1.7 * 2.0 ** -125, 2.0 ** -133, 3 * 2.0 ** -134], np.float32),
    np.array([0xFFC00001, 0x7F800001, 0x00008000, 0x00018000, 0x80008000], np.uint32).view(np.float32)])


@pytest.mark.parametrize("scale", [1.0, 0.125])
@pytest.mark.parametrize("n", [1, 7, 4097, 16384 * 256 + 3])
def test_f32_to_bf16(n, scale):
    """out = bf16_rne(float32(in) * float32(scale)) bit for bit: randn, exact ties above even and odd upper halves,
    +-0, +-inf, NaN (stays NaN), the largest finite f32 (rounds to inf at scale 1), subnormal inputs and products,
    and n past the grid's 16384 * 256 threads (the grid-stride loop's second trip: the last 3 elements).
    Subnormals: where the float32 product is subnormal the device may either keep it (then the bits are exact) or
    flush it (then only |out| <= the smallest normal bf16 is required). Observed on the MI355X: kept, bits exact."""
    x = np.random.default_rng([n, 5]).standard_normal(n).astype(np.float32)
    x[: min(n, 64)] = np.concatenate([_SPECIAL, U.tie_block(64)])[: min(n, 64)]
    if n > 4096:
        x[-7:] = _SPECIAL[:7]  # (the tail: the grid-stride trip, or the last block)
        x[1000:1512] = U.tie_block(512, seed=1)
    xin = dev(x)
    out = Guarded(n, 64, torch.int16)
    _lib.call("tw_f32_to_bf16", xin.data_ptr(), out.ptr(), n, scale, S())
    out.check(f"tw_f32_to_bf16 n={n}")
    got = bits16(out.t)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        prod = x * np.float32(scale)
    want = U.bf16_rne(prod)
    nan = np.isnan(prod)
    assert U.bf16_is_nan(got[nan]).all() and not U.bf16_is_nan(got[~nan]).any()
    sub = ~nan & (np.abs(prod) < np.float32(2.0 ** -126)) & (x != 0)
    exact = ~nan & ~sub
    assert np.array_equal(got[exact], want[exact]), f"{int((got[exact] != want[exact]).sum())} elements differ"
    kept = np.array_equal(got[sub], want[sub])
    if not kept:
        assert ((got[sub] & 0x7FFF) <= 0x0080).all() and np.array_equal(got[sub] >> 15, want[sub] >> 15)
    print(f"ulp-pin tw_f32_to_bf16 shape=n={n} scale={scale} family=randn+ties+specials exact "
          f"subnormals={'kept' if kept else 'flushed'} ({int(sub.sum())})")
