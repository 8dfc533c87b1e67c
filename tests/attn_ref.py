"""Float64 references, float32 restatements, bounds and input families for the attention kernels of
csrc/attention.hip (tests/test_attn_ref.py on the CPU, tests/test_gpu_attn_ulp.py on the MI355X). The interval
criterion, MARGIN and SHARP_SHARE are tests/ulp_ref.py's, used as they are.

Two bounds, both derived and never measured on the kernel under test:

* Decode kernels (k_attn_decode_self2, dec_attend_off, k_attn_decode_cross_lean, k_attn_decode_cross_grp,
  k_attn_cross_merge, k_attn_decode_cross_probs) do all their arithmetic in f32 and round once on the store:
  slack = MARGIN * E, E per (row, head) the largest |float32 restatement - float64| over the head's 64 outputs and over
  the restatements of `dec_restatements` (numpy two-pass; the lean kernel's online-softmax order with NG = 32 and 64;
  dec_attend_off's two-pass order; the three-slice split and merge).

* Encoder kernels (k_attn_enc2 / enc4 / enc5). Read in the code: each kernel converts the f32 p of a tile to bf16
  (`pb[j] = (__bf16)...`) as the B operand of the PV MFMA, while the denominator l adds the UNROUNDED f32 p
  (`ps += sc[0][t][r] + sc[1][t][r]` before the conversion). So O = sum_j bf16(p_j) v_j / sum_j p_j with
  bf16(p_j) = p_j (1 + d_j), |d_j| <= u = 2^-8, and

      |O - ref| <= u * sum_j p_j |v_j| / sum_j p_j + (f32 error) = u * A + MARGIN * E

  A per output element from the float64 reference, E per (query, head) from float32 restatements of the same operation
  with unrounded P (`enc_case`). All three variants do this; enc5 differs only in its input: it multiplies q by log2(e)
  and rounds that to bf16 before the score MFMA, which is its documented input rounding. Its reference therefore takes
  q' = bf16_rne(float32(q) * float32(log2 e)) and p = 2^(q' . k), exactly; `enc5_distance` reports how far that
  reference is from the true attention (recorded, not asserted)."""
import numpy as np

import ulp_ref as U

_F = np.float32
U_BF16 = 2.0 ** -8  # bf16 unit roundoff
LOG2E32 = _F(1.4426950408889634)
TIGHT = 2.0 ** -7  # one bf16 ulp of |ref|
TIGHT_SHARE = 0.9
GUARD = _F(64.0)  # EA_GUARD
NEG_INF = _F(-np.inf)

FAMILIES = ("peaked", "diffuse", "late_max", "extreme_late", "extreme_neg", "extreme_pos", "ties")
# q = PEAK_G * (one key row): that key scores PEAK_G |k|^2 ~ 32, the best of the others ~ 8 PEAK_G z_max ~ 14: the
# one key carries all but e^-18 of the weight, A = |ref| to that order (test_attn_ref.py checks the tight share).
PEAK_G = 0.5
TIE_G = 0.625  # the two hot keys score ~ +40, every other key ~ -40: weights 1/2, 1/2, e^-80


# ---- float64 reference ----------------------------------------------------------------------------------------------
def attn64(q, K, V, lo=0, hi=None, base2=False):
    """softmax(q . K^T) . V over keys lo .. hi-1 in float64 (q [.., Nq, 64], K / V [.., S, 64]; base2: p = 2^score).
    Returns (out, A, p): A = sum_j p_j |v_j| / sum_j p_j per output element, p the probabilities [.., Nq, hi - lo]."""
    q = np.asarray(q, np.float64)
    K = np.asarray(K, np.float64)[..., lo:hi, :]
    V = np.asarray(V, np.float64)[..., lo:hi, :]
    s = q @ np.swapaxes(K, -1, -2)
    s = s - s.max(-1, keepdims=True)
    p = np.exp2(s) if base2 else np.exp(s)
    p = p / p.sum(-1, keepdims=True)
    return p @ V, p @ np.abs(V), p


def enc5_q(q):
    """k_attn_enc5's input rounding: bf16_rne(float32(q) * float32(log2 e)), as float32 values."""
    return U.bf16_exact(np.asarray(q, _F) * LOG2E32)[0]


def tight_share(ref64, slack):
    """Share of elements whose slack is at most one bf16 ulp of |ref| (2^-7 |ref|)."""
    ref64 = np.asarray(ref64, np.float64)
    return float(np.mean(np.broadcast_to(slack, ref64.shape) <= TIGHT * np.abs(ref64)))


# ---- float32 pieces -------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """a * b + c rounded once (the float64 product of two float32 is exact)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(_F)


def expf32(x, log2e=LOG2E32, ftz=False):
    """__expf: v_exp_f32(float32(x * log2 e)). ftz: results below 2^-126 are 0, as the bare v_exp_f32 gives them (it
    has no denormal range; the kernels use it without ocml's fix-up, which the encoder's comment says in so many
    words: "a flushed underflow is exact enough for softmax")."""
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        r = np.exp2((np.asarray(x, _F) * log2e).astype(_F)).astype(_F)
    return np.where(r < _F(2.0 ** -126), _F(0), r) if ftz else r


def exp2f32(x):
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        return np.exp2(np.asarray(x, _F)).astype(_F)


def score_lanes32(q, K):
    """The decode kernels' score: lane gl adds its 8 products in order (bf16 products are exact in f32), then
    lane8_sum: xor 1, xor 2, mirror. q [64], K [n, 64] -> [n]."""
    K = np.asarray(K, _F)
    prod = K.reshape(-1, 8, 8) * np.asarray(q, _F).reshape(8, 8)
    d = np.zeros(prod.shape[:2], _F)
    for e in range(8):
        d = d + prod[:, :, e]
    d = d + d[:, [1, 0, 3, 2, 5, 4, 7, 6]]
    d = d + d[:, [2, 3, 0, 1, 6, 7, 4, 5]]
    d = d + d[:, ::-1]
    return d[:, 0]


# ---- decode restatements (one query, one head) ----------------------------------------------------------------------
def dec32_plain(q, K, V, log2e=None):
    """Two passes in numpy float32: (out [64], probabilities [n])."""
    q, K, V = np.asarray(q, _F), np.asarray(K, _F), np.asarray(V, _F)
    s = (K * q).sum(-1, dtype=_F)
    x = s - s.max()
    with np.errstate(under="ignore"):
        p = np.exp(x).astype(_F) if log2e is None else expf32(x, log2e)
    l = p.sum(dtype=_F)
    return (p[:, None] * V).sum(0, dtype=_F) / l, p / l


def dec32_lean_state(q, K, V, NG=32, UNR=8, log2e=LOG2E32):
    """k_attn_decode_cross_lean / _grp over one key range, unnormalised: (M, tot, v [64]). Key group g takes keys
    it * NG + g; blocks of UNR keys per group with one rescale per block; the 8 groups of a wave merge by xor 1, 2, 4;
    the per-wave records are combined in order."""
    V = np.asarray(V, _F)
    n = len(V)
    s = score_lanes32(q, K)
    nit = -(-n // NG)
    nitp = -(-nit // UNR) * UNR
    sv = np.full(nitp * NG, NEG_INF, _F)
    sv[:n] = s
    sv = sv.reshape(nitp, NG)
    Vp = np.zeros((nitp * NG, 64), _F)
    Vp[:n] = V
    Vp = Vp.reshape(nitp, NG, 64)
    m = np.full(NG, NEG_INF, _F)
    l = np.zeros(NG, _F)
    acc = np.zeros((NG, 64), _F)
    with np.errstate(invalid="ignore"):
        for it0 in range(0, nit, UNR):
            blk = sv[it0: it0 + UNR]
            bm = np.maximum(m, blk.max(0))
            live = bm > NEG_INF
            sc = np.where(live, expf32(m - bm, log2e), _F(1))
            l = l * sc
            acc = acc * sc[:, None]
            for u in range(UNR):
                p = np.where(live, expf32(blk[u] - bm, log2e), _F(0))
                l = l + p
                acc = fma32(p[:, None], Vp[it0 + u], acc)
            m = np.where(live, bm, m)
        W = NG // 8
        m, l, acc = m.reshape(W, 8), l.reshape(W, 8), acc.reshape(W, 8, 64)
        for o in (1, 2, 4):
            idx = np.arange(8) ^ o
            m2, l2, a2 = m[:, idx], l[:, idx], acc[:, idx]
            M = np.maximum(m, m2)
            s1 = np.where(m == NEG_INF, _F(0), expf32(m - M, log2e))
            s2 = np.where(m2 == NEG_INF, _F(0), expf32(m2 - M, log2e))
            l = l * s1 + l2 * s2
            acc = acc * s1[..., None] + a2 * s2[..., None]
            m = M
        return merge32([(m[w, 0], l[w, 0], acc[w, 0]) for w in range(W)], log2e=log2e)


def merge32(states, log2e=LOG2E32, drop=None, own_max=False):
    """The record merge of the lean kernels and of k_attn_cross_merge: M = max, tot = sum wt l, v = sum wt part, in
    order. Mutants: drop = index of a record left out; own_max = every record weighted as if its max were M."""
    if drop is not None:
        states = [s for i, s in enumerate(states) if i != drop]
    M = NEG_INF
    for mz, _, _ in states:
        M = np.maximum(M, mz)
    tot, v = _F(0), np.zeros(64, _F)
    with np.errstate(invalid="ignore"):
        for mz, lz, vz in states:
            wt = _F(0) if mz == NEG_INF else (_F(1) if own_max else expf32(mz - M, log2e))
            tot = _F(tot + wt * lz)
            v = (v + wt * vz).astype(_F)
    return M, tot, v


def dec32_lean(q, K, V, NG=32, log2e=LOG2E32):
    _, tot, v = dec32_lean_state(q, K, V, NG, log2e=log2e)
    return (v / tot).astype(_F)


def split_bounds(S, NS=3):
    return [(z * S // NS, (z + 1) * S // NS) for z in range(NS)]


def dec32_split(q, K, V, NS=3, drop=None, own_max=False):
    """k_attn_decode_cross_grp<G, 32> over NS key slices + k_attn_cross_merge."""
    st = [dec32_lean_state(q, K[a:b], V[a:b], 32) for a, b in split_bounds(len(K), NS)]
    _, tot, v = merge32(st, drop=drop, own_max=own_max)
    return (v / tot).astype(_F)


def dec32_two_pass_kernel(q, K, V, ftz=False, inv_ulps=0):
    """dec_attend_off: scores, block max, p = __expf(s - max); thread t adds keys t, t + 256, ..; each wave's 64 sums by
    the xor butterfly, the four waves in order; P.V per 8-lane group over keys it * 32 + g in order, the 32 groups in
    order, times 1 / sum. ftz: expf32's flushed underflow; inv_ulps: the
    float32 normaliser 1 / sum moved that many ulps (dec_case). Returns (out [64], probabilities [n])."""
    V = np.asarray(V, _F)
    n = len(V)
    s = score_lanes32(q, K)
    p = expf32(s - s.max(), ftz=ftz)
    pp = np.zeros(-(-n // 256) * 256, _F)
    pp[:n] = p
    t = np.zeros(256, _F)
    for row in pp.reshape(-1, 256):
        t = t + row
    w = U._butterfly64(t.reshape(4, 64))[:, 0]
    inv = _F(1) / _F(_F(_F(w[0] + w[1]) + w[2]) + w[3])
    for _ in range(abs(inv_ulps)):
        inv = np.nextafter(inv, _F(np.inf if inv_ulps > 0 else 0))
    nit = -(-n // 32)
    pg = np.zeros(nit * 32, _F)
    pg[:n] = p
    Vg = np.zeros((nit * 32, 64), _F)
    Vg[:n] = V
    pg, Vg = pg.reshape(nit, 32), Vg.reshape(nit, 32, 64)
    acc = np.zeros((32, 64), _F)
    for it in range(nit):
        acc = fma32(pg[it][:, None], Vg[it], acc)
    v = np.zeros(64, _F)
    for g in range(32):
        v = v + acc[g]
    return v * inv, p * inv


def dec_restatements(q, K, V):
    """name -> float32 output of every decode restatement that applies to this key count."""
    r = {"plain": dec32_plain(q, K, V)[0], "lean32": dec32_lean(q, K, V, 32), "lean64": dec32_lean(q, K, V, 64),
         "two_pass": dec32_two_pass_kernel(q, K, V)[0]}
    if len(K) >= 3:
        r["split3"] = dec32_split(q, K, V)
    return r


def dec_case(q, K, V):
    """One (row, head) of a decode kernel: dict ref [64], A, p (float64), E (one number), and for the probs output
    E_p (the largest |float32 probability - float64| over the keys) and E_sum (the largest |sum of the float32
    probabilities - 1|, the sum taken exactly), both over the same six restatements of the probabilities: numpy
    two-pass with numpy's exp and with the kernel's exp2 form; dec_attend_off's order; that order with the flushed
    underflow of the bare v_exp_f32 (on `ties` the cold keys' p of about 1e-38 come back as 0); and that order with
    the normaliser 1 / l one float32 ulp up and one down. The last two are there for the reason ulp_ref.ln_E moves
    its mean: every probability of a row carries the one normaliser, l is a float32 sum of up to 1536 terms and
    1 / l one more rounding, so no float32 normaliser is good to better than an ulp, and a row whose l and 1 / l
    happen to round exactly (sums of 0 to 4e-9 off 1 on most of these rows) is lucky, not more faithful. No number
    is set by hand: E_sum is the computed |sum - 1| of those restatements."""
    ref, A, p = attn64(q[None], K, V)
    ref, A, p = ref[0], A[0], p[0]
    E = max(float(np.abs(r.astype(np.float64) - ref).max()) for r in dec_restatements(q, K, V).values())
    ps = (dec32_plain(q, K, V)[1], dec32_two_pass_kernel(q, K, V)[1], dec32_plain(q, K, V, LOG2E32)[1],
          dec32_two_pass_kernel(q, K, V, ftz=True)[1], dec32_two_pass_kernel(q, K, V, inv_ulps=1)[1],
          dec32_two_pass_kernel(q, K, V, inv_ulps=-1)[1])
    E_p = max(float(np.abs(x.astype(np.float64) - p).max()) for x in ps)
    E_sum = max(abs(float(x.astype(np.float64).sum()) - 1.0) for x in ps)
    return {"ref": ref, "A": A, "p": p, "E": E, "E_p": E_p, "E_sum": E_sum}


# ---- encoder restatements (batched over leading axes) ---------------------------------------------------------------
def mfma_scores32(q, K):
    """S = q . K^T as four v_mfma_f32_32x32x16_bf16 steps: each 16-deep block's dot product (float64, rounded once)
    added to a float32 accumulator."""
    q64, K64 = np.asarray(q, np.float64), np.asarray(K, np.float64)
    s = None
    for d0 in range(0, 64, 16):
        blk = (q64[..., d0: d0 + 16] @ np.swapaxes(K64[..., d0: d0 + 16], -1, -2)).astype(_F)
        s = blk if s is None else s + blk
    return s


def enc32_plain(q, K, V, base2=False):
    """Two passes in float32 with unrounded P."""
    s = mfma_scores32(q, K)
    x = s - s.max(-1, keepdims=True)
    with np.errstate(under="ignore"):
        p = exp2f32(x) if base2 else np.exp(x).astype(_F)
    l = p.sum(-1, keepdims=True, dtype=_F)
    return (p.astype(np.float64) @ np.asarray(V, np.float64)).astype(_F) / l


def _pv32(O, p, V64, k0):
    """O += P . V over one tile, one float32 accumulation per 16-key MFMA step."""
    for j0 in range(0, p.shape[-1], 16):
        O = O + (p[..., j0: j0 + 16].astype(np.float64) @ V64[..., k0 + j0: k0 + j0 + 16, :]).astype(_F)
    return O


def _round_p(p):
    return U.bf16_exact(p)[0]


def _tile_keys(K, V, S, mut):
    """The keys a tiled kernel attends, with the key-range mutants: drop_last; pad_zero (key S with zero K and V
    rows); pad_clamp (key S re-reads row S - 1, as the staging clamps it); mask_off_by_one (pad_clamp in a ragged
    last tile only)."""
    K, V = np.asarray(K, _F), np.asarray(V, _F)
    if mut == "drop_last" and S > 1:
        return K[..., : S - 1, :], V[..., : S - 1, :]
    if mut == "pad_zero":
        z = np.zeros_like(K[..., :1, :])
        return np.concatenate([K, z], -2), np.concatenate([V, z], -2)
    if mut == "pad_clamp" or (mut == "mask_off_by_one" and S % 64):
        return np.concatenate([K, K[..., -1:, :]], -2), np.concatenate([V, V[..., -1:, :]], -2)
    return K, V


def enc32_tiles(q, K, V, round_p=False, mut=None, log2e=LOG2E32):
    """k_attn_enc2 / k_attn_enc4: 64-key tiles, running max m, O and l rescaled by exp2((m - m') log2e) when it
    grows, p = exp2(fma(s, log2e, -m' log2e)), l += the tile's f32 p, O += (bf16(p) if round_p else p) . V.
    Mutants: the key-range ones of _tile_keys; skip_O / skip_l (no rescale of O / of l after the first tile);
    l_rounded (l adds the bf16-rounded p)."""
    K, V = _tile_keys(K, V, K.shape[-2], mut)
    V64 = np.asarray(V, np.float64)
    n = K.shape[-2]
    m = l = O = None
    with np.errstate(invalid="ignore", under="ignore"):
        for k0 in range(0, n, 64):
            s = mfma_scores32(q, K[..., k0: k0 + 64, :])
            tmax = s.max(-1)
            if m is None:
                m = tmax
                l = np.zeros_like(tmax)
                O = np.zeros(tmax.shape + (64,), _F)
            else:
                m_new = np.maximum(m, tmax)
                alpha = exp2f32((m - m_new) * log2e)
                if mut != "skip_l":
                    l = l * alpha
                if mut != "skip_O":
                    O = O * alpha[..., None]
                m = m_new
            mb = (m * log2e).astype(_F)
            p = exp2f32(fma32(s, log2e, -mb[..., None]))
            pr = _round_p(p)
            l = l + (pr if mut == "l_rounded" else p).sum(-1, dtype=_F)
            O = _pv32(O, pr if round_p else p, V64, k0)
    return O * (_F(1) / l)[..., None]


def enc5_32_tiles(qp, K, V, round_p=False, mut=None):
    """k_attn_enc5 on q' = enc5_q(q): scores in log2 units, p = exp2(s - c) with the guarded stabiliser c (0 unless
    the first tile's |max| > 64; raised by g = tmax - c, with O and l scaled by exp2(-g), only where tmax - c > 64).
    Mutants as enc32_tiles, and guard0: the guard tests tmax > 64 instead of tmax - c > 64."""
    K, V = _tile_keys(K, V, K.shape[-2], mut)
    V64 = np.asarray(V, np.float64)
    n = K.shape[-2]
    c = l = O = None
    with np.errstate(invalid="ignore", under="ignore", over="ignore"):
        for k0 in range(0, n, 64):
            s = mfma_scores32(qp, K[..., k0: k0 + 64, :])
            tmax = s.max(-1)
            if c is None:
                c = np.where(np.abs(tmax) > GUARD, tmax, _F(0)).astype(_F)
                l = np.zeros_like(tmax)
                O = np.zeros(tmax.shape + (64,), _F)
            else:
                over = (tmax > GUARD) if mut == "guard0" else (tmax - c > GUARD)
                g = np.where(over, tmax - c, _F(0)).astype(_F)
                alpha = exp2f32(-g)
                c = c + g
                if mut != "skip_l":
                    l = l * alpha
                if mut != "skip_O":
                    O = O * alpha[..., None]
            p = exp2f32(s - c[..., None])
            pr = _round_p(p)
            l = l + (pr if mut == "l_rounded" else p).sum(-1, dtype=_F)
            O = _pv32(O, pr if round_p else p, V64, k0)
        return O * (_F(1) / l)[..., None]


# ---- input families -------------------------------------------------------------------------------------------------
def _bf(x):
    return U.bf16_exact(x)[0]


def family_qkv(family, Nq, S, seed=0):
    """bf16-exact float32 (q [Nq, 64], K [S, 64], V [S, 64]) of one head. |V| lies in [0.5, 2): no output is small
    against its row for want of a value (the share conditions are about the kernels, not about v near 0).
    peaked: query i is PEAK_G times key row (7 i + S - 1) % S, so that key carries the weight (query 0: the
        last key); diffuse: q = 0.02 randn, near-uniform weights; late_max: every score is about N(0, 1.2) but the last
        key's, about 8, after all the small ones; extreme_late / _neg / _pos: q = +-1 in every dim (-1 where
        (i + seed) % 3 == 0), one late key / the first 64 keys with K = +2 / -2 / +2 in every dim: scores of +-128,
        +-185 in enc5's log2 units, with queries of either sign (per-lane growth 0 and > 0) in one wave; ties: two hot
        keys (the last two) with weight 1/2 each to 2^-100 and adjacent bf16 values in V, so the reference is the tie
        between them in every dim, even and odd lower neighbours alternating."""
    g = np.random.default_rng([seed, FAMILIES.index(family), Nq, S])
    K = _bf(g.standard_normal((S, 64)))
    V = _bf(g.uniform(0.5, 2.0, (S, 64)) * g.choice([-1.0, 1.0], (S, 64)))
    i = np.arange(Nq)
    if family == "peaked":
        q = _bf(PEAK_G * K[(7 * i + S - 1) % S])
    elif family == "diffuse":
        q = _bf(0.02 * g.standard_normal((Nq, 64)))
    elif family == "late_max":
        d = g.choice([-1.0, 1.0], 64)
        q = _bf(0.05 * g.standard_normal((Nq, 64)) + 0.5 * d)
        K = _bf(0.3 * g.standard_normal((S, 64)))
        K[S - 1] = 0.25 * d
    elif family.startswith("extreme"):
        q = np.where((i + seed) % 3 == 0, -1.0, 1.0)[:, None] * np.ones((1, 64))
        q = q.astype(_F)
        K = _bf(0.3 * g.standard_normal((S, 64)))
        if family == "extreme_late":
            K[S - 1 - S // 15] = 2.0
        else:
            K[:64] = -2.0 if family == "extreme_neg" else 2.0
    else:
        r = _bf(g.standard_normal(64))
        K = np.tile(-r, (S, 1))
        hot = [S - 2, S - 1] if S > 1 else [0]
        K[hot] = r
        q = np.tile(_bf(TIE_G * r), (Nq, 1))
        hi = g.integers(0x3F00, 0x4000, 64).astype(np.uint16)  # 0.5 .. 2
        hi = (hi & ~np.uint16(1)) | (np.arange(64, dtype=np.uint16) & 1)
        hi |= g.integers(0, 2, 64).astype(np.uint16) << 15
        V[hot[0]] = U.bf16_to_f64(hi)
        V[hot[-1]] = U.bf16_to_f64(hi + np.uint16(len(hot) - 1))
    return q.astype(_F), K.astype(_F), V.astype(_F)


# ---- encoder cases shared by the CPU and the GPU tests --------------------------------------------------------------
_ENC_CACHE = {}


def enc_case(family, B, H, S, seed=0):
    """Inputs, references and slacks of one tw_attn_encoder call, computed once: dict q, K, V [B H, S, 64] (float32,
    bf16-exact), qkv (bf16 bits [B S, 3 H 64]), and per kernel class ("nat": variants 8 and 16; "enc5": variant 32)
    ref, A, E ([B H, S, 1]) and slack = u A + MARGIN E, each [B H, S, 64] in (b, h) order."""
    key = (family, B, H, S, seed)
    if key not in _ENC_CACHE:
        qs, Ks, Vs = zip(*(family_qkv(family, S, S, seed + 101 * bh) for bh in range(B * H)))
        q, K, V = np.stack(qs), np.stack(Ks), np.stack(Vs)
        c = {"q": q, "K": K, "V": V}
        t = np.stack([q, K, V]).reshape(3, B, H, S, 64).transpose(1, 3, 0, 2, 4)  # [B][S][3][H][64]
        c["qkv"] = U.bf16_rne(t.reshape(B * S, 3 * H * 64))
        qp = enc5_q(q)
        for name, qq, base2, rs in (("nat", q, False, (enc32_plain(q, K, V), enc32_tiles(q, K, V))),
                                    ("enc5", qp, True, (enc32_plain(qp, K, V, True), enc5_32_tiles(qp, K, V)))):
            ref, A, _ = attn64(qq, K, V, base2=base2)
            E = np.max([np.abs(r.astype(np.float64) - ref).max(-1, keepdims=True) for r in rs], axis=0)
            c[name] = {"ref": ref, "A": A, "E": E, "slack": U_BF16 * A + U.MARGIN * E}
        for v in list(c.values()) + list(c["nat"].values()) + list(c["enc5"].values()):
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _ENC_CACHE[key] = c
        while len(_ENC_CACHE) > 8:  # (S = 513 cases hold tens of MB each)
            _ENC_CACHE.pop(next(iter(_ENC_CACHE)))
    return _ENC_CACHE[key]


def enc_out_rows(x, B, H, S):
    """[B H, S, 64] in (b, h) order -> the kernel's output layout [B S, H 64]."""
    return np.asarray(x).reshape(B, H, S, 64).transpose(0, 2, 1, 3).reshape(B * S, H * 64)


def enc5_distance(c):
    """How far enc5's reference (q' rounded) lies from the true attention: (largest |difference|, the same over the
    true reference's slack). Recorded, never asserted."""
    d = np.abs(c["enc5"]["ref"] - c["nat"]["ref"])
    return float(d.max()), float((d / c["nat"]["slack"]).max())


def enc_margin_needed(got_bits, ref, A, E):
    """The margin an encoder output needed: what MARGIN would have to be for every element to pass with slack
    u A + margin E (0: all pass on u A alone)."""
    ref = np.asarray(ref, np.float64)
    g = np.asarray(got_bits).astype(np.uint16).reshape(ref.shape)
    k = U.bf16_key(g)
    v = U.bf16_to_f64(g)
    lo = 0.5 * (v + U.bf16_to_f64(U._key_to_bits(k - 1)))
    hi = 0.5 * (v + U.bf16_to_f64(U._key_to_bits(k + 1)))
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.maximum(np.maximum(lo - ref, ref - hi), 0.0) - U_BF16 * A
        m = np.where(d > 0, d / np.broadcast_to(E, ref.shape), 0.0)
    m = np.where(np.isnan(m), np.inf, m)
    return float(m.max())


# ---- decode cases shared by the CPU and the GPU tests ---------------------------------------------------------------
DS2_KEYS = 256  # k_attn_decode_self2: pos < DS2_KEYS takes the one-round-trip path, pos >= DS2_KEYS dec_attend_off
SELF_POS = (0, 1, 7, 8, 31, 32, 33, 254, 255, 256, 257, 447)
KV_CHOICES = ("0", "1", "pos", "pos+1", "255", "256")
NAN_BITS = 0x7FC1  # what cache cells no row may read hold on input


def self_positions(max_pos):
    return [p for p in SELF_POS if p < max_pos - 1] + [max_pos - 1]


def kv_start_of(choice, pos):
    return {"pos": pos, "pos+1": pos + 1}.get(choice, None) if choice in ("pos", "pos+1") else int(choice)


def tab_source(b, qpos, pos, row0):
    """The cache row (global) that holds position qpos < pos[b] of row b in the tests' position table: another row of
    the launch, a different one for every b at a given position (so no two rows share a cell), and the spare row 0 in
    front of the launch where that row writes position qpos itself in this launch (tw_kv_tab_check's precondition)."""
    B = len(pos)
    b2 = (b + 1 + qpos) % B
    return 0 if pos[b2] == qpos else row0 + b2


def self_case(family, max_pos, tab, kv_choice=None, H=2, seed=0):
    """One launch of tw_attn_decode_self[_tab][_masked]: one row per position of self_positions(max_pos).
    dict pos, kv_start (None: unmasked), row0, rows (cache rows in all), qkv (bf16 bits [B, 3 H 64]), kc / vc (bf16 bits
    [rows, H, max_pos, 64]: NAN_BITS wherever no row's query may read: past pos, masked positions, unused rows), tab
    (int32 [rows, max_pos] or None), prob[b][h] = (q, K, V) of the keys the row attends (the last one its own k / v),
    ks[b] the first attended position, ref [B, H 64], E [B, H]."""
    pos = self_positions(max_pos)
    B = len(pos)
    row0 = 2 if tab else 0
    rows = row0 + B + (1 if tab else 0)
    kc = np.full((rows, H, max_pos, 64), NAN_BITS, np.uint16)
    vc = np.full((rows, H, max_pos, 64), NAN_BITS, np.uint16)
    table = None
    if tab:
        table = np.tile(np.arange(rows, dtype=np.int32)[:, None], (1, max_pos))
    kv = None if kv_choice is None else [kv_start_of(kv_choice, p) for p in pos]
    qkv = np.zeros((B, 3, H, 64), np.uint16)
    ref, E, prob, kss = np.zeros((B, H, 64)), np.zeros((B, H)), [], []
    for b, p in enumerate(pos):
        ks = 0 if kv is None or p < kv[b] else kv[b]
        kss.append(ks)
        prob.append([])
        for h in range(H):
            q, K, V = family_qkv(family, 1, p + 1 - ks, seed + 1000 * b + h)
            prob[b].append((q[0], K, V))
            qkv[b, :, h] = U.bf16_rne(np.stack([q[0], K[-1], V[-1]]))
            for j in range(p - ks):
                r = tab_source(b, ks + j, pos, row0) if tab else b
                kc[r, h, ks + j], vc[r, h, ks + j] = U.bf16_rne(K[j]), U.bf16_rne(V[j])
                if tab:
                    table[row0 + b, ks + j] = r
            c = dec_case(q[0], K, V)
            ref[b, h], E[b, h] = c["ref"], c["E"]
    return {"pos": pos, "kv_start": kv, "ks": kss, "row0": row0, "rows": rows, "qkv": qkv.reshape(B, 3 * H * 64),
            "kc": kc, "vc": vc, "tab": table, "prob": prob, "ref": ref.reshape(B, H * 64), "E": E, "H": H}


def self_keys(c, b, h, ks=None, table_row=None, own_from_cache=False, head=None):
    """(q, K, V) float32 as row b, head h of self_case c reads them through the cache and the table: the restatement
    of the kernel's addressing. Mutants: ks (another first key), table_row (the table row consulted), own_from_cache
    (key pos from the cache cell instead of the step's k / v), head (another head's cache and q / k / v)."""
    H, p = c["H"], c["pos"][b]
    hh = h if head is None else head
    ks = c["ks"][b] if ks is None else ks
    row = c["row0"] + b
    t = c["tab"]
    tr = None if t is None else t[row if table_row is None else table_row]
    qkv = c["qkv"].reshape(-1, 3, H, 64)
    Kb, Vb = [], []
    for key in range(ks, p + 1):
        if key == p and not own_from_cache:
            Kb.append(qkv[b, 1, hh])
            Vb.append(qkv[b, 2, hh])
        else:
            r = row if tr is None or key == p else tr[key]
            Kb.append(c["kc"][r, hh, key])
            Vb.append(c["vc"][r, hh, key])
    f = lambda bits: U.bf16_to_f64(np.array(bits)).astype(_F)  # noqa: E731
    if not Kb:
        return f(qkv[b, 0, hh]), np.zeros((0, 64), _F), np.zeros((0, 64), _F)
    return f(qkv[b, 0, hh]), f(Kb), f(Vb)


def cross_case(family, S, row_slots, Bt, H=2, seed=0, want_p=False):
    """One launch of tw_attn_decode_cross / _grouped / _probs: row b reads encoder slot row_slots[b]; rows of one slot
    share its K / V and differ in q. dict q (bf16 bits [B, H 64]), ckv (bf16 bits [2, Bt, H, S, 64]), prob[b][h] =
    (q, K, V), ref [B, H 64], E [B, H]; want_p: also p [B, H, S], E_p, E_sum [B, H]."""
    B = len(row_slots)
    ckv = np.zeros((2, Bt, H, S, 64), np.uint16)
    qb = np.zeros((B, H, 64), np.uint16)
    ref, E = np.zeros((B, H, 64)), np.zeros((B, H))
    p, E_p, E_sum = np.zeros((B, H, S)), np.zeros((B, H)), np.zeros((B, H))
    prob = [[None] * H for _ in range(B)]
    for s in range(Bt):
        mine = [b for b in range(B) if row_slots[b] == s]
        for h in range(H):
            q, K, V = family_qkv(family, max(len(mine), 1), S, seed + 100 * s + h)
            ckv[0, s, h], ckv[1, s, h] = U.bf16_rne(K), U.bf16_rne(V)
            for i, b in enumerate(mine):
                qb[b, h] = U.bf16_rne(q[i])
                prob[b][h] = (q[i], K, V)
                c = dec_case(q[i], K, V)
                ref[b, h], E[b, h] = c["ref"], c["E"]
                p[b, h], E_p[b, h], E_sum[b, h] = c["p"], c["E_p"], c["E_sum"]
    out = {"q": qb.reshape(B, H * 64), "ckv": ckv, "prob": prob, "ref": ref.reshape(B, H * 64), "E": E, "H": H,
           "slots": list(row_slots)}
    if want_p:
        out.update(p=p, E_p=E_p, E_sum=E_sum)
    return out


def grouped_slots(B, group, first):
    """Slots of a grouped view: the first `first` rows continue slot 0, then every `group` rows the next slot."""
    return [0 if b < first else (1 if first else 0) + (b - first) // group for b in range(B)]


def per_head(x, H):
    """[B, H] -> [B, H 64] (a per-(row, head) E or slack spread over the head's outputs)."""
    return np.repeat(np.asarray(x), 64, axis=1)


# ---- the shapes of tests/test_gpu_attn_ulp.py (tests/test_attn_ref.py names its mutants' failures at these) ---------
ENC_S = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 513)
ENC_BH = ((1, 1), (2, 3), (3, 3))
ENC_S_LONG = 1500  # once per variant, peaked only, (B, H) = (1, 1)
SELF_MAX_POS = (448, 64)
CROSS_S = (1, 7, 31, 32, 33, 255, 256, 257, 1500, 1536)
CROSS_SLOTS = (2, 0, 3)  # a non-identity row_map into Bt = 4 slots
GROUP_DIRECT = ((2, 3, 4, 5), (3, 63, 64, 65, 511, 512, 513, 1500))
GROUP_SPLIT = ((6, 7, 8), (3, 4, 5, 97, 1500))
PROBS_S = (7, 257, 1500)
