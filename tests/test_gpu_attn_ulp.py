"""The attention kernels of csrc/attention.hip pinned on the MI355X to float64 within derived rounding bounds
(tests/attn_ref.py: decode kernels slack = MARGIN E; encoder kernels slack = u A + MARGIN E, enc5 against the reference
on its documented q' = bf16(q log2 e); tests/test_attn_ref.py shows on the CPU which wrong kernels these bounds refuse).

Every output buffer (outputs, both K/V caches, the grouped workspace, probs) lies between canary regions that must come
back unchanged, and everything an entry point documents as not written is compared bit for bit: cache cells other than
(row, pos[row]), probs rows and slots that were not selected. Cache cells no query may read hold NaN bits on input.
Each test records `attn-pin` lines (printed when the module finishes): per kernel, shape set and input family the margin
needed (what MARGIN would have had to be; 0 = inside u A, or correctly rounded), the tight share (encoder: slack <= one
bf16 ulp of |ref|) or the sharp share (decode: slack <= 2^-12 |ref|), for the encoder the largest share of its slack
an element used, for enc5 the distance of its reference from the true attention, and for the f32 probs rows (which
have no share) the margin their sums needed. One run's lines are kept in profiles/attn_pins.txt."""
import numpy as np
import pytest
import torch

import attn_ref as R
import ulp_ref as U
from test_gpu_ulp import Guarded, S, bits16, canary_like, dev
from twamd import _lib

pytestmark = pytest.mark.gpu
DEFAULT_VARIANT = 32  # the library's default encoder kernel
PINS = {}


def record(kernel, shapes, family, need, ok, n, **extra):
    """Worst margin and pooled share per (kernel, shape set, family); extra: named figures, the largest kept."""
    w, a, b, x = PINS.get((kernel, shapes, family), (0.0, 0, 0, {}))
    x = {k: max(v, x.get(k, v)) for k, v in extra.items()}
    PINS[(kernel, shapes, family)] = (max(w, need), a + ok, b + n, x)


@pytest.fixture(scope="module", autouse=True)
def print_pins():
    yield
    print()  # (the first line must not follow pytest's progress dots)
    for (kernel, shapes, family), (w, a, b, x) in PINS.items():
        tail = "".join(f" {k}={v:.3e}" for k, v in x.items())
        share = f" share={a / b:.3f}" if b else ""  # (the f32 probs rows have no share)
        print(f"attn-pin {kernel} shapes={shapes} family={family} margin_needed={w:.3f}{share}{tail}")


def check_decode(got_bits, c, what, kernel, shapes, family):
    """The decode criterion on a whole launch: got [B, H 64] against c["ref"] with slack MARGIN E per (row, head)."""
    E = R.per_head(c["E"], c["H"])
    need = U.margin_needed(got_bits, c["ref"], E)
    slack = U.MARGIN * E
    try:
        U.assert_bf16_correctly_rounded(got_bits, c["ref"], slack, what)
    except AssertionError as e:
        raise AssertionError(f"{e} [margin needed {need:.2f}]") from None
    record(kernel, shapes, family, need, int((slack <= U.SHARP * np.abs(c["ref"])).sum()), c["ref"].size)
    if family == "peaked":
        share = U.sharp_share(c["ref"], slack)
        assert share >= U.SHARP_SHARE, f"{what}: slack <= 2^-12 |ref| on {share:.3f} of the elements only"


# ---- tw_attn_encoder ------------------------------------------------------------------------------------------------
def _encoder(c, B, H, Sx, variant, what):
    qkv = dev(c["qkv"])
    out = Guarded(B * Sx * H * 64, H * 64, torch.int16)
    _lib.call("tw_attn_set_variant", variant)
    _lib.call("tw_attn_encoder", qkv.data_ptr(), B, Sx, H, out.ptr(), S())
    out.check(what)
    return bits16(out.t).reshape(B * Sx, H * 64)


def _slack_used(got, ref, slack):
    """The largest share of its slack an element used: distance from ref to the reals that round to got, over slack."""
    k = U.bf16_key(got)
    v = U.bf16_to_f64(got)
    lo = 0.5 * (v + U.bf16_to_f64(U._key_to_bits(k - 1)))
    hi = 0.5 * (v + U.bf16_to_f64(U._key_to_bits(k + 1)))
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.maximum(np.maximum(lo - ref, ref - hi), 0.0)
        r = np.where(d > 0, d / slack, 0.0)
    return float(np.nanmax(r))


def _check_encoder(got, c, B, H, Sx, variant, family, shapes, what):
    k = c["enc5" if variant == 32 else "nat"]
    ref, A, slack = (R.enc_out_rows(k[n], B, H, Sx) for n in ("ref", "A", "slack"))
    E = R.enc_out_rows(np.broadcast_to(k["E"], k["ref"].shape), B, H, Sx)
    need = R.enc_margin_needed(got, ref, A, E)
    try:
        U.assert_bf16_correctly_rounded(got, ref, slack, what)
    except AssertionError as e:
        raise AssertionError(f"{e} [margin needed {need:.2f}]") from None
    share = R.tight_share(ref, slack)
    if family == "peaked":
        assert share >= R.TIGHT_SHARE, f"{what}: slack <= one bf16 ulp of |ref| on {share:.3f} of the elements only"
    extra = {"slack_used": _slack_used(got, ref, slack)}
    if variant == 32:
        extra["enc5_ref_to_true"] = R.enc5_distance(c)[0]
    record(f"tw_attn_encoder[v{variant}]", shapes, family, need, int((slack <= R.TIGHT * np.abs(ref)).sum()), ref.size,
           **extra)


@pytest.mark.parametrize("Sx", R.ENC_S)
@pytest.mark.parametrize("B,H", R.ENC_BH)
def test_encoder(B, H, Sx):
    """k_attn_enc2 (8), k_attn_enc4 (16) and k_attn_enc5 (32) on every family: one masked first tile (S < 64), ragged
    and full last tiles, the 256-query workgroup boundary, several work items ((3, 3) at S = 300: 18, a remainder in
    the XCD remap). Variant 16 is variant 8 bit for bit. At (3, 3), S = 300 the LDS pad leaves the bits alone."""
    try:
        _lib.call("tw_attn_set_lds_pad", 0)
        for family in R.FAMILIES:
            c = R.enc_case(family, B, H, Sx)
            got = {}
            for v in (8, 16, 32):
                what = f"tw_attn_encoder variant {v} {family} B={B} H={H} S={Sx}"
                got[v] = _encoder(c, B, H, Sx, v, what)
                _check_encoder(got[v], c, B, H, Sx, v, family, f"B={B},H={H},S=1..513", what)
            assert np.array_equal(got[16], got[8]), f"{family} B={B} H={H} S={Sx}: variant 16 differs from variant 8"
            if (B, H, Sx) == (3, 3, 300):
                _lib.call("tw_attn_set_lds_pad", 4)
                for v in (8, 16, 32):
                    assert np.array_equal(_encoder(c, B, H, Sx, v, f"{family} lds pad 4 variant {v}"), got[v])
                _lib.call("tw_attn_set_lds_pad", 0)
    finally:
        _lib.call("tw_attn_set_variant", DEFAULT_VARIANT)
        _lib.call("tw_attn_set_lds_pad", 0)


@pytest.mark.parametrize("variant", [8, 16, 32])
def test_encoder_1500(variant):
    """The model's own length once per kernel, on `peaked` (24 key tiles, the last one ragged; 6 workgroups)."""
    Sx = R.ENC_S_LONG
    c = R.enc_case("peaked", 1, 1, Sx)
    what = f"tw_attn_encoder variant {variant} peaked S={Sx}"
    try:
        _lib.call("tw_attn_set_lds_pad", 0)
        got = _encoder(c, 1, 1, Sx, variant, what)
    finally:
        _lib.call("tw_attn_set_variant", DEFAULT_VARIANT)
        _lib.call("tw_attn_set_lds_pad", 0)
    _check_encoder(got, c, 1, 1, Sx, variant, "peaked", f"B=1,H=1,S={Sx}", what)


# ---- tw_attn_decode_self, _masked, _tab, _tab_masked ----------------------------------------------------------------
def _run_self(c, max_pos, tab, masked, what):
    """One launch on self_case c; returns the output bits [B, H 64] after checking the canaries, the cache append and
    that every other cache cell kept its bits."""
    H, pos, row0, rows = c["H"], c["pos"], c["row0"], c["rows"]
    B, D = len(pos), c["H"] * 64
    cell = H * max_pos * 64
    qkv, pos_d = dev(c["qkv"]), dev(np.array(pos, np.int32))
    kc, vc = Guarded(rows * cell, cell, torch.int16), Guarded(rows * cell, cell, torch.int16)
    kc.t.copy_(dev(c["kc"]).reshape(-1))
    vc.t.copy_(dev(c["vc"]).reshape(-1))
    out = Guarded(B * D, D, torch.int16)
    kp, vp = kc.ptr() + 2 * row0 * cell, vc.ptr() + 2 * row0 * cell
    kv_d = dev(np.array(c["kv_start"], np.int32)) if masked else None
    if tab:
        tab_d = dev(c["tab"])
        bad = torch.full((B,), -1, dtype=torch.int32, device="cuda")
        _lib.call("tw_kv_tab_check", tab_d.data_ptr(), pos_d.data_ptr(), row0, B, max_pos, bad.data_ptr(), S())
        assert not bad.cpu().numpy().any(), f"{what}: the test's table breaks the precondition"
        args = (qkv.data_ptr(), B, H, max_pos, pos_d.data_ptr(), kp, vp, tab_d.data_ptr(), row0)
        if masked:
            _lib.call("tw_attn_decode_self_tab_masked", *args, kv_d.data_ptr(), out.ptr(), S())
        else:
            _lib.call("tw_attn_decode_self_tab", *args, out.ptr(), S())
    else:
        args = (qkv.data_ptr(), B, H, max_pos, pos_d.data_ptr(), kp, vp)
        if masked:
            _lib.call("tw_attn_decode_self_masked", *args, kv_d.data_ptr(), out.ptr(), S())
        else:
            _lib.call("tw_attn_decode_self", *args, out.ptr(), S())
    for g in (out, kc, vc):
        g.check(what)
    step = c["qkv"].reshape(B, 3, H, 64)
    for name, g, before, part in (("K", kc, c["kc"], 1), ("V", vc, c["vc"], 2)):
        want = before.copy()
        for b, p in enumerate(pos):
            want[row0 + b, :, p] = step[b, part]
        after = bits16(g.t).reshape(want.shape)
        for b, p in enumerate(pos):
            assert np.array_equal(after[row0 + b, :, p], step[b, part]), f"{what}: {name} cache row pos[{b}] = {p}"
        assert np.array_equal(after, want), f"{what}: {int((after != want).sum())} other {name} cache elements changed"
    return bits16(out.t).reshape(B, D)


@pytest.mark.parametrize("max_pos", R.SELF_MAX_POS)
@pytest.mark.parametrize("tab", [False, True], ids=["rows", "tab"])
def test_decode_self(tab, max_pos):
    """tw_attn_decode_self / _tab: every position of self_positions in one launch (both sides of DS2_KEYS = 256 at
    max_pos 448; the last position of a 64-position cache), every family; the table names other rows of the launch and
    the spare row in front of it, row0 = 2."""
    name = "tw_attn_decode_self_tab" if tab else "tw_attn_decode_self"
    for family in R.FAMILIES:
        c = R.self_case(family, max_pos, tab)
        what = f"{name} {family} max_pos={max_pos}"
        check_decode(_run_self(c, max_pos, tab, False, what), c, what, name, f"max_pos={max_pos},pos=0..{max_pos - 1}",
                     family)


@pytest.mark.parametrize("max_pos", R.SELF_MAX_POS)
@pytest.mark.parametrize("tab", [False, True], ids=["rows", "tab"])
def test_decode_self_masked(tab, max_pos):
    """tw_attn_decode_self_masked / _tab_masked with kv_start 0, 1, pos, pos + 1 (a pad query: attends from 0), 255 and
    256 for every position; the masked cells hold NaN bits. Every family at every kv_start."""
    name = "tw_attn_decode_self_tab_masked" if tab else "tw_attn_decode_self_masked"
    for choice in R.KV_CHOICES:
        for family in R.FAMILIES:
            c = R.self_case(family, max_pos, tab, choice)
            what = f"{name} {family} max_pos={max_pos} kv_start={choice}"
            check_decode(_run_self(c, max_pos, tab, True, what), c, what, name,
                         f"max_pos={max_pos},pos=0..{max_pos - 1},kv_start=0..256", family)


# ---- tw_attn_decode_cross -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Sx", R.CROSS_S)
def test_decode_cross(Sx):
    """k_attn_decode_cross_lean<32>: key counts that leave key groups empty (1, 7, 31), one partial pass (33), the
    unrolled block's boundary (255, 256, 257), the model's 1500 and DA_MAXK = 1536; a row_map that is no identity into
    4 slots, and a NULL row_map."""
    for slots, Bt in ((R.CROSS_SLOTS, 4), (None, 3)):
        for family in R.FAMILIES:
            c = R.cross_case(family, Sx, slots or (0, 1, 2), Bt)
            what = f"tw_attn_decode_cross {family} S={Sx} row_map={slots}"
            q, ckv = dev(c["q"]), dev(c["ckv"])
            rm = None if slots is None else dev(np.array(slots, np.int32))
            out = Guarded(3 * 128, 128, torch.int16)
            _lib.call("tw_attn_decode_cross", q.data_ptr(), 3, 2, Sx, Bt, _lib.ptr(rm) or None, ckv.data_ptr(), out.ptr(),
                      S())
            out.check(what)
            check_decode(bits16(out.t).reshape(3, 128), c, what, "tw_attn_decode_cross", "S=1..1536", family)


# ---- tw_attn_decode_cross_grouped -----------------------------------------------------------------------------------
def _grouped(group, Sx, shapes):
    """Every family with both `first` values (0 and group - 1); B = first + group + 1: a leading tail, one full group
    and a last group of one row."""
    H = 2
    lib = _lib.load()
    for family in R.FAMILIES:
        for first in (0, group - 1):
            B = first + group + 1
            slots = R.grouped_slots(B, group, first)
            Bt = max(slots) + 1
            c = R.cross_case(family, Sx, slots, Bt, H)
            what = f"tw_attn_decode_cross_grouped {family} group={group} first={first} B={B} S={Sx}"
            q, ckv, rm = dev(c["q"]), dev(c["ckv"]), dev(np.array(slots, np.int32))
            nws = int(lib.tw_attn_decode_cross_grouped_ws_bytes(B, H)) // 4
            ws = Guarded(nws, 64, torch.float32)
            out = Guarded(B * H * 64, H * 64, torch.int16)
            _lib.call("tw_attn_decode_cross_grouped", q.data_ptr(), B, H, Sx, Bt, rm.data_ptr(), group, first,
                      ckv.data_ptr(), ws.ptr(), out.ptr(), S())
            out.check(what)
            ws.check(what + " (workspace)")
            check_decode(bits16(out.t).reshape(B, H * 64), c, what, f"tw_attn_decode_cross_grouped[{shapes}]",
                         "group=2..5,S=3..1500" if group <= 5 else "group=6..8,S=3..1500", family)


@pytest.mark.parametrize("Sx", R.GROUP_DIRECT[1])
@pytest.mark.parametrize("group", R.GROUP_DIRECT[0])
def test_decode_cross_grouped_direct(group, Sx):
    """k_attn_decode_cross_grp<G, 64>: the 512-thread form that writes the output itself (no key split)."""
    _grouped(group, Sx, "direct")


@pytest.mark.parametrize("Sx", R.GROUP_SPLIT[1])
@pytest.mark.parametrize("group", R.GROUP_SPLIT[0])
def test_decode_cross_grouped_split(group, Sx):
    """k_attn_decode_cross_grp<G, 32> over three key slices (one key each at S = 3) and k_attn_cross_merge."""
    _grouped(group, Sx, "split3")


def test_decode_cross_grouped_refuses_two_keys():
    """S = 2 is fewer keys than slices: refused, nothing written."""
    c = R.cross_case("diffuse", 3, (0, 0, 0), 1)
    q, ckv, rm = dev(c["q"]), dev(c["ckv"]), dev(np.zeros(3, np.int32))
    ws, out = Guarded(4096, 64, torch.float32), Guarded(3 * 128, 128, torch.int16)
    for group in (3, 6):
        with pytest.raises(_lib.TwError):
            _lib.call("tw_attn_decode_cross_grouped", q.data_ptr(), 3, 2, 2, 1, rm.data_ptr(), group, 0, ckv.data_ptr(),
                      ws.ptr(), out.ptr(), S())
    torch.cuda.synchronize()
    assert ws.untouched() and out.untouched()


# ---- tw_attn_decode_cross_probs -------------------------------------------------------------------------------------
@pytest.mark.parametrize("Sx", R.PROBS_S)
def test_decode_cross_probs(Sx):
    """k_attn_decode_cross_probs: the bf16 output under the decode criterion; the f32 probabilities of heads 1 and 3
    (head_mask 0b1010: gaps) in slots 1 and 2 of 4 (slot0 = 1) at step pos - 5 for pos 5, 6, 7 (pos 4 lies below,
    pos 8 past [pos0, pos0 + 3)): |got - p64| <= MARGIN E_p per row and |sum - 1| <= MARGIN E_sum (attn_ref.dec_case: both from
    the same restatements, none set by hand); every other row
    and slot of probs comes back as canary."""
    B, H, Bt, mask, slot0, n_slots, pos0, n_steps = 5, 4, 5, 0b1010, 1, 4, 5, 3
    pos = [4, 5, 6, 7, 8]
    slots = (1, 0, 2, 4, 3)
    for family in R.FAMILIES:
        c = R.cross_case(family, Sx, slots, Bt, H, want_p=True)
        what = f"tw_attn_decode_cross_probs {family} S={Sx}"
        q, ckv, rm, pos_d = dev(c["q"]), dev(c["ckv"]), dev(np.array(slots, np.int32)), dev(np.array(pos, np.int32))
        out = Guarded(B * H * 64, H * 64, torch.int16)
        probs = Guarded(B * n_steps * n_slots * Sx, 64, torch.float32)
        _lib.call("tw_attn_decode_cross_probs", q.data_ptr(), B, H, Sx, Bt, rm.data_ptr(), ckv.data_ptr(), out.ptr(),
                  probs.ptr(), mask, slot0, n_slots, pos_d.data_ptr(), pos0, n_steps, S())
        out.check(what)
        probs.check(what + " (probs)")
        check_decode(bits16(out.t).reshape(B, H * 64), c, what, "tw_attn_decode_cross_probs", "S=7,257,1500", family)
        got = probs.t.cpu().numpy().reshape(B, n_steps, n_slots, Sx)
        rest = np.ones(got.shape, bool)
        need = need_sum = 0.0
        for b in range(B):
            k = pos[b] - pos0
            if not 0 <= k < n_steps:
                continue
            for sl, h in ((1, 1), (2, 3)):
                rest[b, k, sl] = False
                row = got[b, k, sl].astype(np.float64)
                d, ds = np.abs(row - c["p"][b, h]).max(), abs(row.sum() - 1.0)
                assert d <= U.MARGIN * c["E_p"][b, h], f"{what}: row {b} head {h}: |p - p64| {d:.3e}, E_p {c['E_p'][b, h]:.3e}"
                assert ds <= U.MARGIN * c["E_sum"][b, h], f"{what}: row {b} head {h}: |sum - 1| {ds:.3e}"
                need = max(need, d / c["E_p"][b, h] if d else 0.0)
                need_sum = max(need_sum, ds / c["E_sum"][b, h] if ds else 0.0)
        assert np.array_equal(got.view(np.uint32)[rest], canary_like(int(rest.sum()), np.uint32)), \
            f"{what}: probs rows or slots that were not selected were written"
        record("tw_attn_decode_cross_probs[probs]", "S=7,257,1500", family, need, 0, 0, sum_margin_needed=need_sum)
