"""The attention criteria of tests/attn_ref.py have teeth (CPU): on the shapes and input families of
tests/test_gpu_attn_ulp.py every faithful float32 restatement of the kernels passes its criterion, `peaked` reaches its
share from the reference alone, and each subtly wrong kernel, written as a restatement, fails at a named family and
shape. What the ENCODER bound u A + MARGIN E cannot see is shown, not hidden (test_what_the_encoder_bound_cannot_see and
DESIGN.md, "Attention pins"): l summed from the bf16-rounded p fails no criterion here; a truncating store and a
bf16 log2 e fail for enc5 or for the decode kernels only."""
import numpy as np
import pytest

import attn_ref as R
import ulp_ref as U


def fails(got_bits, ref, slack):
    try:
        U.assert_bf16_correctly_rounded(got_bits, ref, slack, "mutant")
    except AssertionError:
        return True
    return False


def enc_model(c, kind, **kw):
    """The kernels' model with bf16-rounded P on case c: bf16 bits. kind "nat": k_attn_enc2 / enc4; "enc5"."""
    q = kw.pop("q", c["q"])
    if kind == "nat":
        return U.bf16_rne(R.enc32_tiles(q, c["K"], c["V"], round_p=True, **kw))
    return U.bf16_rne(R.enc5_32_tiles(R.enc5_q(q), c["K"], c["V"], round_p=True, **kw))


# ---- the reference alone ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", R.ENC_S + (R.ENC_S_LONG,))
def test_peaked_reaches_the_tight_share_from_the_reference_alone(S):
    """slack = u A + MARGIN E <= one bf16 ulp of |ref| on at least 0.9 of the elements of every head used on the GPU
    ((3, 3) holds the heads of (1, 1) and (2, 3): head bh has seed 101 bh), for both references."""
    B, H = (1, 1) if S == R.ENC_S_LONG else (3, 3)
    c = R.enc_case("peaked", B, H, S)
    for kind in ("nat", "enc5"):
        for bh in range(B * H):
            share = R.tight_share(c[kind]["ref"][bh], c[kind]["slack"][bh])
            assert share >= R.TIGHT_SHARE, f"peaked S={S} head {bh} {kind}: tight share {share:.3f}"


@pytest.mark.parametrize("max_pos", R.SELF_MAX_POS)
def test_peaked_decode_self_is_sharp(max_pos):
    c = R.self_case("peaked", max_pos, True, "1")
    assert U.sharp_share(c["ref"], U.MARGIN * R.per_head(c["E"], c["H"])) >= U.SHARP_SHARE


@pytest.mark.parametrize("S", R.CROSS_S)
def test_peaked_decode_cross_is_sharp(S):
    c = R.cross_case("peaked", S, R.CROSS_SLOTS, 4)
    assert U.sharp_share(c["ref"], U.MARGIN * R.per_head(c["E"], c["H"])) >= U.SHARP_SHARE


# ---- every restatement is inside its criterion ---------------------------------------------------------------------------
@pytest.mark.parametrize("family", R.FAMILIES)
def test_encoder_models_pass_on_every_family(family):
    """The kernels' models with bf16-rounded P (the running-max tiles of enc2 / enc4; enc5's guarded unshifted exp2
    on q') pass u A + MARGIN E at every S, and so does each unrounded float32 restatement at MARGIN E alone."""
    for S in R.ENC_S:
        c = R.enc_case(family, 1, 1, S)
        for kind in ("nat", "enc5"):
            k = c[kind]
            U.assert_bf16_correctly_rounded(enc_model(c, kind), k["ref"], k["slack"], f"{kind} model {family} S={S}")
        q5 = R.enc5_q(c["q"])
        for kind, r in (("nat", R.enc32_plain(c["q"], c["K"], c["V"])), ("nat", R.enc32_tiles(c["q"], c["K"], c["V"])),
                        ("enc5", R.enc32_plain(q5, c["K"], c["V"], True)), ("enc5", R.enc5_32_tiles(q5, c["K"], c["V"]))):
            U.assert_bf16_correctly_rounded(U.bf16_rne(r), c[kind]["ref"], U.MARGIN * c[kind]["E"], f"{family} S={S}")


@pytest.mark.parametrize("family", R.FAMILIES)
def test_decode_restatements_pass_on_every_family(family):
    """Every restatement behind E, and two that are not (numpy two-pass with the kernel's exp2 form; the lean order
    with blocks of 4), pass MARGIN E on the cross shapes and on a table-and-mask self launch."""
    probs = []
    for S in R.CROSS_S:
        c = R.cross_case(family, S, R.CROSS_SLOTS, 4)
        probs += [(c["prob"][b][h], c["ref"][b, 64 * h: 64 * h + 64], c["E"][b, h], f"cross S={S}")
                  for b in range(3) for h in range(2)]
    c = R.self_case(family, 448, True, "1")
    probs += [(c["prob"][b][h], c["ref"][b, 64 * h: 64 * h + 64], c["E"][b, h], f"self pos={c['pos'][b]}")
              for b in range(len(c["pos"])) for h in range(2)]
    for (q, K, V), ref, E, what in probs:
        rs = dict(R.dec_restatements(q, K, V))
        rs["plain_exp2"] = R.dec32_plain(q, K, V, R.LOG2E32)[0]
        _, tot, v = R.dec32_lean_state(q, K, V, 32, UNR=4)
        rs["lean32_unr4"] = v / tot
        for name, r in rs.items():
            U.assert_bf16_correctly_rounded(U.bf16_rne(r), ref, U.MARGIN * E, f"{name} {family} {what}")


# ---- encoder mutants -----------------------------------------------------------------------------------------------------
# (mutant, kernel class, family, S): where it fails. B, H = 1, 1.
ENC_MUTANTS = [
    ("pad_zero", "nat", "diffuse", 1), ("pad_zero", "enc5", "diffuse", 1),  # one zero key beside the only key
    ("pad_zero", "nat", "diffuse", 33), ("pad_zero", "enc5", "diffuse", 33),
    ("pad_clamp", "nat", "late_max", 300), ("pad_clamp", "enc5", "late_max", 300),  # the last key counted twice
    ("drop_last", "nat", "peaked", 300), ("drop_last", "enc5", "peaked", 300),  # query 0's key is the last one
    ("mask_off_by_one", "nat", "late_max", 300), ("mask_off_by_one", "enc5", "late_max", 300),
    ("skip_O", "nat", "late_max", 300), ("skip_l", "nat", "late_max", 300),  # the max grows in the last tile
    ("skip_O", "enc5", "extreme_late", 300), ("skip_l", "enc5", "extreme_late", 300),  # (enc5 rescales past the guard)
    ("guard0", "enc5", "extreme_neg", 300),  # c = -185 from the first tile must move up at the second
]


@pytest.mark.parametrize("mut,kind,family,S", ENC_MUTANTS)
def test_encoder_mutant_fails(mut, kind, family, S):
    c = R.enc_case(family, 1, 1, S)
    k = c[kind]
    U.assert_bf16_correctly_rounded(enc_model(c, kind), k["ref"], k["slack"], "the unmutated model")
    assert fails(enc_model(c, kind, mut=mut), k["ref"], k["slack"]), f"{mut} passes on {family} S={S} ({kind})"


def test_encoder_mask_off_by_one_needs_a_ragged_tile():
    """With S a multiple of the 64-key tile there is no masked tile: the mutant is the kernel."""
    c = R.enc_case("late_max", 1, 1, 256)
    assert np.array_equal(enc_model(c, "nat", mut="mask_off_by_one"), enc_model(c, "nat"))


@pytest.mark.parametrize("kind", ["nat", "enc5"])
def test_encoder_scale_applied_twice_fails(kind):
    """q already carries 0.125; once more and `peaked` (S = 300) is no longer peaked."""
    c = R.enc_case("peaked", 1, 1, 300)
    assert fails(enc_model(c, kind, q=c["q"] * np.float32(0.125)), c[kind]["ref"], c[kind]["slack"])


def test_encoder_store_truncates_fails_for_enc5():
    """late_max, S = 300: enc5's unshifted p of the one heavy key is no power of two, so its bf16 rounding uses the
    u A term and a store that truncates as well leaves the interval. (pack_bf16x2 is one helper for the three
    kernels; enc2 / enc4 on these families round a p of exactly 1, see the next test.)"""
    c = R.enc_case("late_max", 1, 1, 300)
    k = c["enc5"]
    o = R.enc5_32_tiles(R.enc5_q(c["q"]), c["K"], c["V"], round_p=True)
    assert not fails(U.bf16_rne(o), k["ref"], k["slack"])
    assert fails(U.f32_bits_to_bf16_trunc(o), k["ref"], k["slack"])


def test_enc5_log2e_rounded_to_bf16_fails():
    """late_max, S = 300: in enc5 the constant enters q' = bf16(q log2 e) itself; with bf16(log2 e) the scores are
    0.18 % large, the last key (score about 8 above the rest, 26 % of the weight with the others) gains weight, and
    enc5's own P rounding has already used most of u A: outside the bound. (Also at S = 256 and 513; at smaller S
    the last key has nearly all the weight either way.)"""
    c = R.enc_case("late_max", 1, 1, 300)
    k = c["enc5"]
    qp = U.bf16_exact(c["q"] * U.bf16_exact(R.LOG2E32)[0])[0]
    assert fails(U.bf16_rne(R.enc5_32_tiles(qp, c["K"], c["V"], round_p=True)), k["ref"], k["slack"])
    assert not fails(enc_model(c, "enc5"), k["ref"], k["slack"])


def test_what_the_encoder_bound_cannot_see():
    """Stated, not hidden ("Attention pins"). u A >= u |ref| is at least half a bf16 ulp of |ref|, so the
    encoder bound is blind to anything that moves an output by less than that from a value that used none of it:
    * a truncating store in enc2 / enc4, whose heavy keys have p = 1 exactly on these families (enc5 above and the
      decode criterion, test_decode_store_truncates_fails, catch the same f32_to_bf16 helper);
    * l summed from bf16(p) (the kernels sum the unrounded f32 p): it moves the output by at most
      u sum p |v - ref| / sum p, within u A on every family;
    * log2 e rounded to bf16 in enc2 / enc4 (a softmax at temperature 1.0018: at most 0.0018 Cov_p(s, v), below
      u A at every S up to 513); enc5 (test_enc5_log2e_rounded_to_bf16_fails) and the decode criterion, in __expf
      (test_decode_log2e_rounded_to_bf16_and_scale_twice_fail), catch it."""
    log2e_bf16 = U.bf16_exact(R.LOG2E32)[0]
    for family in R.FAMILIES:
        for S in (33, 300, 513):
            c = R.enc_case(family, 1, 1, S)
            k = c["nat"]
            o = R.enc32_tiles(c["q"], c["K"], c["V"], round_p=True)
            assert not fails(U.f32_bits_to_bf16_trunc(o), k["ref"], k["slack"])
            o = R.enc32_tiles(c["q"], c["K"], c["V"], round_p=True, log2e=log2e_bf16)
            assert not fails(U.bf16_rne(o), k["ref"], k["slack"])
            for kind, fn, q in (("nat", R.enc32_tiles, c["q"]), ("enc5", R.enc5_32_tiles, R.enc5_q(c["q"]))):
                o = fn(q, c["K"], c["V"], round_p=True, mut="l_rounded")
                assert not fails(U.bf16_rne(o), c[kind]["ref"], c[kind]["slack"])


# ---- decode mutants ------------------------------------------------------------------------------------------------------
def dec_fails(out32, ref, E):
    return fails(U.bf16_rne(out32), ref, U.MARGIN * E)


def _cross(family, S):
    c = R.cross_case(family, S, R.CROSS_SLOTS, 4)
    return c, lambda b, h: (c["ref"][b, 64 * h: 64 * h + 64], c["E"][b, h])


def test_decode_padded_key_fails():
    """Key S included with a zero row (diffuse, S = 33) or with the clamped row S - 1 (late_max, S = 33)."""
    c, at = _cross("diffuse", 33)
    q, K, V = c["prob"][0][0]
    z = np.zeros((1, 64), np.float32)
    assert dec_fails(R.dec32_lean(q, np.concatenate([K, z]), np.concatenate([V, z])), *at(0, 0))
    c, at = _cross("late_max", 33)
    q, K, V = c["prob"][0][0]
    assert dec_fails(R.dec32_lean(q, np.concatenate([K, K[-1:]]), np.concatenate([V, V[-1:]])), *at(0, 0))
    assert not dec_fails(R.dec32_lean(q, K, V), *at(0, 0))


def test_decode_last_key_dropped_fails():
    """peaked, S = 33: row 0 of a slot attends the last key."""
    c, at = _cross("peaked", 33)
    q, K, V = c["prob"][0][0]
    assert dec_fails(R.dec32_lean(q, K[:-1], V[:-1]), *at(0, 0))


def _self_out(c, b, h, **kw):
    q, K, V = R.self_keys(c, b, h, **kw)
    if len(K) == 0 or np.isnan(K).any() or np.isnan(V).any():
        return np.full(64, np.nan, np.float32)
    return R.dec32_two_pass_kernel(q, K, V)[0]


def _self_at(c, b, h):
    return c["ref"][b, 64 * h: 64 * h + 64], c["E"][b, h]


def _stale(c, seed=5):
    """c with finite stale data (random bf16 in +-[0.5, 2)) in every cache cell that held NaN bits: what a cache that
    has been through earlier passes holds there."""
    g = np.random.default_rng(seed)
    d = dict(c)
    for name in ("kc", "vc"):
        a = c[name].copy()
        fill = U.bf16_rne(g.uniform(0.5, 2.0, a.shape) * g.choice([-1.0, 1.0], a.shape))
        d[name] = np.where(a == R.NAN_BITS, fill, a)
    return d


def test_self_addressing_restated_is_the_case():
    """self_keys (the cache, the table and the mask as the kernel addresses them) gives back each row's own problem."""
    for tab in (False, True):
        c = R.self_case("diffuse", 448, tab, "1")
        for b in range(len(c["pos"])):
            for h in range(2):
                for got, want in zip(R.self_keys(c, b, h), c["prob"][b][h]):
                    assert np.array_equal(got, want)
                assert not dec_fails(_self_out(c, b, h), *_self_at(c, b, h))


def test_kv_start_off_by_one_fails():
    """diffuse, max_pos 448, kv_start 1: one key more (position 0: a masked cell, NaN on input) or one key less, at
    pos 33 (one round trip) and 257 (two-pass)."""
    c = R.self_case("diffuse", 448, False, "1")
    for p in (33, 257):
        b = c["pos"].index(p)
        assert c["ks"][b] == 1
        assert dec_fails(_self_out(c, b, 0, ks=0), *_self_at(c, b, 0))
        assert dec_fails(_self_out(c, b, 0, ks=2), *_self_at(c, b, 0))
        # not by NaN alone: with finite stale data in the masked cell the output is finite and still outside
        stale = _self_out(_stale(c), b, 0, ks=0)
        assert np.isfinite(stale).all() and dec_fails(stale, *_self_at(c, b, 0))
        assert not dec_fails(_self_out(_stale(c), b, 0), *_self_at(c, b, 0))


def test_kv_start_applied_to_a_pad_query_fails():
    """kv_start = pos + 1 (a pad query attends from 0): with the mask applied nothing is attended. This one is a
    0 / 0 whatever the cache holds: every pad query has kv_start > pos, so the mutant's key set is always empty."""
    c = R.self_case("diffuse", 448, False, "pos+1")
    b = c["pos"].index(33)
    assert c["ks"][b] == 0 and c["kv_start"][b] == 34
    assert dec_fails(_self_out(c, b, 0, ks=34), *_self_at(c, b, 0))


def test_cached_row_in_place_of_the_steps_own_kv_fails():
    """Cache cell pos[b] is not yet written when the step reads its keys (NaN on input)."""
    c = R.self_case("peaked", 448, False)
    b = c["pos"].index(33)
    assert dec_fails(_self_out(c, b, 0, own_from_cache=True), *_self_at(c, b, 0))
    for family in ("peaked", "diffuse"):  # and with a finite stale k / v in the cell: finite, and outside
        c = R.self_case(family, 448, False)
        for p in (33, 257):
            b = c["pos"].index(p)
            stale = _self_out(_stale(c), b, 0, own_from_cache=True)
            assert np.isfinite(stale).all() and dec_fails(stale, *_self_at(c, b, 0))


def test_position_table_row_without_row0_fails():
    """peaked, max_pos 448: table row b instead of row0 + b names other cells."""
    c = R.self_case("peaked", 448, True)
    b = c["pos"].index(33)
    assert dec_fails(_self_out(c, b, 0, table_row=b), *_self_at(c, b, 0))


def test_two_heads_swapped_fails():
    c = R.self_case("peaked", 448, True)
    b = c["pos"].index(33)
    assert dec_fails(_self_out(c, b, 0, head=1), *_self_at(c, b, 0))
    c, at = _cross("peaked", 33)
    assert dec_fails(R.dec32_lean(*c["prob"][0][1]), *at(0, 0))


def test_row_map_ignored_fails():
    """peaked, S = 33, row_map (2, 0, 3): row 0 reading slot 0 reads row 1's keys."""
    c, at = _cross("peaked", 33)
    q = c["prob"][0][0][0]
    _, K, V = c["prob"][1][0]  # slot 0
    assert dec_fails(R.dec32_lean(q, K, V), *at(0, 0))


def test_grouped_row_reading_its_neighbours_q_fails():
    """peaked, group 3, S = 63: rows 0 and 1 share a slot and differ in q."""
    c = R.cross_case("peaked", 63, R.grouped_slots(7, 3, 0), 3)
    _, K, V = c["prob"][0][0]
    assert np.array_equal(K, c["prob"][1][0][1])
    assert dec_fails(R.dec32_lean(c["prob"][1][0][0], K, V, 64), c["ref"][0, :64], c["E"][0, 0])
    assert not dec_fails(R.dec32_lean(c["prob"][0][0][0], K, V, 64), c["ref"][0, :64], c["E"][0, 0])


@pytest.mark.parametrize("S", R.GROUP_SPLIT[1])
def test_split_merge_mutants_fail(S):
    """The three-slice split: a dropped slice and a slice weighted as if its maximum were the global one both fail on
    `diffuse` (every slice carries weight) at every S of the split form; the faithful merge passes."""
    c = R.cross_case("diffuse", S, R.grouped_slots(7, 6, 0), 2)
    q, K, V = c["prob"][0][0]
    at = (c["ref"][0, :64], c["E"][0, 0])
    assert not dec_fails(R.dec32_split(q, K, V), *at)
    for z in range(3):
        assert dec_fails(R.dec32_split(q, K, V, drop=z), *at)
    if S > 3:  # (one key per slice: each slice's p is 1 at its own maximum, and the scores differ)
        assert dec_fails(R.dec32_split(q, K, V, own_max=True), *at)


def test_split_merge_wrong_maximum_fails_at_three_keys():
    c = R.cross_case("late_max", 3, R.grouped_slots(7, 6, 0), 2)
    q, K, V = c["prob"][0][0]
    assert dec_fails(R.dec32_split(q, K, V, own_max=True), c["ref"][0, :64], c["E"][0, 0])


def test_decode_store_truncates_fails():
    """diffuse and ties, S = 33: the truncated f32 is outside the interval wherever the f32 lies above the middle, and
    on every tie above an odd value."""
    for family in ("diffuse", "ties"):
        c, at = _cross(family, 33)
        r = R.dec32_lean(*c["prob"][0][0])
        assert fails(U.f32_bits_to_bf16_trunc(r), at(0, 0)[0], U.MARGIN * at(0, 0)[1])
        assert not fails(U.bf16_rne(r), at(0, 0)[0], U.MARGIN * at(0, 0)[1])


def test_decode_log2e_rounded_to_bf16_and_scale_twice_fail():
    """late_max, S = 1500 (the last key holds about half the weight): __expf with bf16(log2 e); peaked, S = 33:
    q scaled by 0.125 once more."""
    c, at = _cross("late_max", 1500)
    q, K, V = c["prob"][0][0]
    assert dec_fails(R.dec32_lean(q, K, V, log2e=U.bf16_exact(R.LOG2E32)[0]), *at(0, 0))
    c, at = _cross("peaked", 33)
    q, K, V = c["prob"][0][0]
    assert dec_fails(R.dec32_lean(q * np.float32(0.125), K, V), *at(0, 0))


def test_probs_bounds_hold_for_the_restatements():
    """The probabilities of the two-pass kernel order lie within MARGIN E_p of the float64 ones and sum to 1 within
    MARGIN E_sum, on every family and probs shape; one dropped key does not."""
    for family in R.FAMILIES:
        for S in R.PROBS_S:
            c = R.cross_case(family, S, (1, 0), 2, want_p=True)
            q, K, V = c["prob"][0][0]
            p = R.dec32_two_pass_kernel(q, K, V)[1].astype(np.float64)
            assert np.abs(p - c["p"][0, 0]).max() <= U.MARGIN * c["E_p"][0, 0]
            assert abs(p.sum() - 1.0) <= U.MARGIN * c["E_sum"][0, 0]
    c = R.cross_case("diffuse", 257, (1, 0), 2, want_p=True)
    q, K, V = c["prob"][0][0]
    p = np.append(R.dec32_two_pass_kernel(q, K[:-1], V[:-1])[1], 0).astype(np.float64)
    assert np.abs(p - c["p"][0, 0]).max() > U.MARGIN * c["E_p"][0, 0]
