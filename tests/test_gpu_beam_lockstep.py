"""tw_beam_step (k_beam_partial<K> / k_beam_step<K>, K = 2 * num_beams) in lockstep with the oracle: one call per
token, and after EVERY call every output — histories, scores, src_rows, ids, pos, the processor state rows, win, all
finished slots, the K/V position table, the finished tables and the log-probability sums and terms — against that
step's record of oracle.whisper_oracle.beam_search_core (on_step) and the host reference built from it
(tests/beam_ref.py). Every beam width 2..8 runs, with ties, a padded row stride, a NULL suppress mask, NULL optional
outputs, other token layouts, log-probability input, length penalties, the smallest history stride, the tail loop of
k_beam_partial and a max_new stop. The inputs (tests/beam_ref.py: CASES) were chosen on the CPU so that no selection
of the oracle hangs on less than ten times the comparison tolerance (beam_ref.check_gaps, asserted again here)."""
import ctypes
import time

import numpy as np
import pytest
import torch

import beam_ref as br
from twamd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = br.TOK_SENTINEL
FIN_KEYS = ("fin_score", "fin_flag", "fin_len", "fin_tokens", "fin_lp", "fin_tlp", "fin_tab")
OPT_KEYS = ("kv_tab", "fin_tab", "run_lp", "fin_lp", "run_tlp", "fin_tlp")


def S():
    return torch.cuda.current_stream().cuda_stream


def _bits(a):
    """Bit pattern of an array (NaN sentinels compare equal to themselves)."""
    return np.ascontiguousarray(a).view(np.int32) if a.dtype == np.float32 else a


def _device_arrays(c, L):
    nb, W, T = c.nb, c.W, c.T
    R = W * nb
    i32 = dict(dtype=torch.int32, device=DEV)
    a = {
        "state": torch.full((R, br.STATE_STRIDE), SENT, **i32),
        "tokens": torch.full((R, T), SENT, **i32), "ids": torch.full((R,), SENT, **i32),
        "pos": torch.full((R,), br.P, **i32),
        "run_score": torch.full((W, nb), -1e9, device=DEV), "fin_score": torch.full((R,), -1e9, device=DEV),
        "fin_flag": torch.zeros(R, **i32), "fin_len": torch.zeros(R, **i32),
        "fin_tokens": torch.full((R, T), SENT, **i32),
        "win": torch.tensor([[1, 0, 0, SENT]] * W, **i32), "src_rows": torch.full((R,), SENT, **i32),
        "kv_tab": torch.arange(R, **i32)[:, None].repeat(1, T).contiguous(), "fin_tab": torch.full((R, T), SENT, **i32),
        "run_lp": torch.zeros(R, device=DEV), "fin_lp": torch.zeros(R, device=DEV),
        "run_tlp": torch.full((R, T), float("nan"), device=DEV), "fin_tlp": torch.full((R, T), float("nan"), device=DEV),
    }
    a["state"][:, br.ST_NGEN] = 0
    a["state"][:, br.ST_LAST:br.ST_LASTTS + 1] = -1
    a["state"][:, br.ST_FINISHED] = 0
    a["run_score"][:, 0] = 0
    return a


def _select_params(c, L):
    p = _lib.TwSelectParams()
    p.V, p.eos, p.pad = L.V, L.eot, L.eot
    p.ts_begin, p.no_timestamps = L.ts_begin, L.notimestamps
    p.max_initial_ts = L.mit
    p.use_timestamps, p.max_new, p.mode = int(c.use_ts), c.max_new, 0
    p.lo, p.hi = L.lang_begin, L.lang_begin + L.n_lang
    p.n_begin_suppress = len(L.begin_suppress)
    for i, t in enumerate(L.begin_suppress):
        p.begin_suppress[i] = t
    return p


def _compare_live(c, w, t, got, ref, worst):
    nb, T = c.nb, c.T
    sl = slice(w * nb, (w + 1) * nb)
    tag = (c.name, "window", w, "step", t)
    for k in ("tokens", "ids", "pos", "src_rows", "state", "fin_flag", "fin_len"):  # (tokens: sentinel past t too)
        assert np.array_equal(got[k][sl], getattr(ref, k)), tag + (k, got[k][sl].tolist(), getattr(ref, k).tolist())
    assert np.array_equal(got["win"][w], ref.win), tag + ("win", got["win"][w], ref.win)
    for s in range(nb):  # every finished slot, not slot 0 alone
        n = int(ref.fin_len[s])
        assert got["fin_tokens"][w * nb + s, :n].tolist() == ref.fin_seq[s], tag + ("fin_tokens", s)
    for k in ("run_score", "fin_score"):
        np.testing.assert_allclose(got[k][sl], getattr(ref, k), rtol=1e-5, atol=1e-4, err_msg=str(tag + (k,)))
    if not c.opt:
        return
    for k in ("kv_tab", "fin_tab"):  # (fin_tab: a just-finished slot's entries past the fed position are 0)
        assert np.array_equal(got[k][sl], getattr(ref, k)), tag + (k,)
    for k in ("run_lp", "fin_lp"):
        np.testing.assert_allclose(got[k][sl], getattr(ref, k), rtol=1e-5, atol=1e-4, err_msg=str(tag + (k,)))
    # the terms over the live positions, to test_beam_step_token_logprobs' tolerance; NaN (untouched) past them
    d = np.abs(got["run_tlp"][sl, :t + 1] - ref.run_tlp[:, :t + 1])
    assert np.all(d <= 1e-3), tag + ("run_tlp", float(np.nanmax(d)))
    assert np.all(np.isnan(got["run_tlp"][sl, t + 1:])), tag + ("run_tlp past t",)
    worst[0] = max(worst[0], float(d.max()))
    for s in range(nb):
        n = int(ref.fin_len[s])
        d = np.abs(got["fin_tlp"][w * nb + s, :n] - ref.fin_tlp[s, :n])
        assert np.all(d <= 1e-3), tag + ("fin_tlp", s)


def _lockstep(c):
    L = br.layout(c.lay)
    nb, W, T, V = c.nb, c.W, c.T, L.V
    R, ld = W * nb, V + c.ld_pad
    t0 = time.time()
    facts = [br.window_facts(c, w) for w in range(W)]  # (asserts the precondition: a violated one fails the test)
    refs = [br.WindowRef(c, w, L) for w in range(W)]
    a = _device_arrays(c, L)
    init = {k: v.cpu().numpy().copy() for k, v in a.items()}
    logits = torch.empty(R, ld, device=DEV)
    ws = torch.empty(int(_lib.load().tw_beam_workspace_bytes(R)), dtype=torch.uint8, device=DEV)
    sup = None
    if not c.null_mask:
        bits = np.zeros((V + 31) // 32, np.uint32)
        for tok in L.suppress:
            bits[tok >> 5] |= np.uint32(1) << np.uint32(tok & 31)
        sup = torch.from_numpy(bits.view(np.int32)).to(DEV)
    sel = _select_params(c, L)
    bp = _lib.TwBeamParams(nb, c.max_new, c.lp, T, int(bool(c.hist)))
    ptr = lambda k: a[k].data_ptr() if c.opt else None  # noqa: E731
    bst = _lib.TwBeamState(a["run_score"].data_ptr(), a["fin_score"].data_ptr(), a["fin_flag"].data_ptr(),
                           a["fin_len"].data_ptr(), a["fin_tokens"].data_ptr(), a["win"].data_ptr(),
                           a["src_rows"].data_ptr(), *[ptr(k) for k in OPT_KEYS])
    if c.hist:
        LP = 8
        pre = np.full((R, LP), SENT, np.int32)
        plen = np.zeros(R, np.int32)
        for r in range(R):
            ids = c.prefix(r // nb, L)
            pre[r, :len(ids)], plen[r] = ids, len(ids)
        pre_d, plen_d = torch.from_numpy(pre).to(DEV), torch.from_numpy(plen).to(DEV)
    n_steps = max(f["steps"] for f in facts)
    assert n_steps <= c.max_new and (W == 1 or c.max_new <= 5 or len({f["steps"] for f in facts}) > 1)
    frozen, worst = {}, [0.0]
    t_host = time.time() - t0
    for t in range(n_steps):
        tk = a["tokens"].cpu().numpy()
        host = np.full((R, ld), np.nan, np.float32)  # (a read past V poisons the row's log-sum-exp)
        for r in range(R):
            host[r, :V] = br.synthetic_logits(tk[r, :t], V, L.ts_begin, L.eot, c.salts[r // nb], c.quant, c.hot)
        logits.copy_(torch.from_numpy(host))
        if c.hist:
            _lib.call("tw_logits_history", logits.data_ptr(), R, ld, V, pre_d.data_ptr(), LP, plen_d.data_ptr(),
                      a["tokens"].data_ptr(), T, a["state"].data_ptr(), float(c.hist[0]), int(c.hist[1]), 1, S())
        _lib.call("tw_beam_step", logits.data_ptr(), W, ld, _lib.ptr(sup), ctypes.byref(sel), ctypes.byref(bp),
                  ctypes.byref(bst), a["state"].data_ptr(), a["tokens"].data_ptr(), a["ids"].data_ptr(),
                  a["pos"].data_ptr(), ws.data_ptr(), S())
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in a.items()}
        got["run_score"] = got["run_score"].reshape(R)
        for w in range(W):
            sl = slice(w * nb, (w + 1) * nb)
            if t < facts[w]["steps"]:
                th = time.time()
                ref = refs[w].apply(facts[w]["recs"][t], facts[w]["fed"][t])
                t_host += time.time() - th
                _compare_live(c, w, t, got, ref, worst)
                if t == facts[w]["steps"] - 1:  # the window is done from here on (win[1] compared above)
                    assert ref.win[1] == 1
                    frozen[w] = {k: got[k][sl].copy() for k in FIN_KEYS}
            else:  # a done window that is still stepped: its finished slots stay bit for bit, its done flag set
                assert got["win"][w, 1] == 1, (c.name, w, t)
                for k in FIN_KEYS:
                    assert np.array_equal(_bits(got[k][sl]), _bits(frozen[w][k])), (c.name, "done window", w, t, k)
    # untouched positions
    assert np.all(got["tokens"][:, n_steps:] == SENT) and np.all(got["fin_tokens"][:, n_steps:] == SENT)
    assert np.all(got["state"][:, 5:] == SENT) and np.all(got["win"][:, 3] == SENT)
    if c.opt:
        assert np.all(np.isnan(got["run_tlp"][:, n_steps:])) and np.all(np.isnan(got["fin_tlp"][:, n_steps:]))
        own = np.arange(R, dtype=np.int32)[:, None]
        assert np.all(got["kv_tab"][:, br.P + n_steps:] == own)
    else:
        for k in OPT_KEYS:
            assert np.array_equal(_bits(got[k]), _bits(init[k])), (c.name, k, "written though its pointer was NULL")
    print(f"{c.name}: {n_steps} calls, {W} x {nb} rows, worst |term - host| {worst[0]:.2e} (bound 1e-3), "
          f"{time.time() - t0:.1f} s ({t_host:.1f} s of it the host reference)")
    return facts


@pytest.mark.parametrize("c", br.CASES, ids=repr)
def test_beam_step_lockstep(c):
    _lockstep(c)


def test_the_timestamp_cases_reach_every_processor_state():
    """The passes are only worth something if the processors' states occur: over the timestamp cases' oracle traces,
    every mask of row_mask (csrc/decode.hip), the rule firing and not, an EOS finish before max_new and a beam that
    continues another row."""
    seen = set()
    for name in br.TS_COVERAGE_CASES:
        c = br.case(name)
        for w in range(c.W):
            seen |= br.window_facts(c, w)["coverage"]
    assert seen == set(br.STATES), sorted(set(br.STATES) - seen)
