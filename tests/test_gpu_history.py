"""tw_logits_history on the GPU: the repetition penalty and the no-repeat n-gram ban against the numpy restatement
(tests/history_ref.py, pinned to transformers' processors by tests/test_history_processors.py) — alone (bit for bit
on raw logits, 1e-4 on log-probabilities), chained with tw_logits_select / tw_logits_sample over 30 steps, and in
front of tw_beam_step against the numpy beam core fed penalised log-probabilities."""
import ctypes

import numpy as np
import pytest
import torch

import history_ref as hr
from oracle import whisper_oracle as wo
from test_history_processors import NGRAMS, PENALTIES, kernel_cases, kernel_logits
from twamd import _lib
from twamd.config import PRESETS, GenerationSettings

pytestmark = pytest.mark.gpu
DEV = "cuda"
D = PRESETS["test-mini"]
V, T = D.vocab, 448


def S():
    return torch.cuda.current_stream().cuda_stream


def _gcfg():
    gen = GenerationSettings.default(D)
    st = gen.special
    return gen, wo.GenCfg(D.vocab, st.eot, st.sot, st.lang_begin, st.n_languages, st.transcribe, st.translate,
                          st.notimestamps, gen.suppress_tokens, gen.begin_suppress_tokens)


def _params(gen, max_new, use_ts=True):
    st = gen.special
    p = _lib.TwSelectParams()
    p.V, p.eos, p.pad = V, st.eot, st.eot
    p.ts_begin, p.no_timestamps = st.timestamp_begin, st.notimestamps
    p.max_initial_ts = gen.max_initial_timestamp_index
    p.use_timestamps, p.max_new, p.mode = int(use_ts), max_new, 0
    p.lo, p.hi = st.lang_begin, st.lang_end
    p.n_begin_suppress = len(gen.begin_suppress_tokens)
    for i, t in enumerate(gen.begin_suppress_tokens):
        p.begin_suppress[i] = t
    return p


def _suppress_bits(tokens):
    bits = np.zeros((V + 31) // 32, np.uint32)
    for t in tokens:
        bits[t >> 5] |= np.uint32(1) << np.uint32(t & 31)
    return torch.from_numpy(bits.view(np.int32)).to(DEV)


def _fresh_state(R):
    st = torch.zeros(R, _lib.TW_STATE_STRIDE, dtype=torch.int32, device=DEV)
    st[:, _lib.TW_ST_LAST:_lib.TW_ST_LASTTS + 1] = -1
    return st


def _device_rows(rows, lang_slot=False):
    """prefix [R][T], prefix_len, tokens [R][T], state for (prefix, generated, finished) rows. lang_slot: the first
    prefix entry of every row is written as TW_HIST_LANG and its id goes to state[TW_ST_LANG] instead."""
    R = len(rows)
    prefix = np.full((R, T), -7, np.int32)  # (entries past a row's length are never read: any value)
    tokens = np.full((R, T), -7, np.int32)
    plen = np.zeros(R, np.int32)
    state = _fresh_state(R)
    for r, (pre, gen, fin) in enumerate(rows):
        prefix[r, : len(pre)] = pre
        tokens[r, : len(gen)] = gen
        plen[r] = len(pre)
        state[r, _lib.TW_ST_NGEN] = len(gen)
        state[r, _lib.TW_ST_FINISHED] = int(fin)
        state[r, _lib.TW_ST_LANG] = 12345  # (read only through a TW_HIST_LANG entry)
        if lang_slot and pre:
            prefix[r, 0] = _lib.TW_HIST_LANG
            state[r, _lib.TW_ST_LANG] = pre[0]
    return (torch.from_numpy(prefix).to(DEV), torch.from_numpy(plen).to(DEV), torch.from_numpy(tokens).to(DEV), state)


def _history(lg, R, ld, prefix, plen, tokens, state, p, n, to_lp):
    _lib.call("tw_logits_history", lg.data_ptr(), R, ld, V, _lib.ptr(prefix), T if prefix is not None else 0,
              _lib.ptr(plen), tokens.data_ptr(), T, state.data_ptr(), float(p), int(n), int(to_lp), S())


@pytest.mark.parametrize("n", NGRAMS)
def test_raw_mode_is_bit_equal_to_the_restatement(n):
    """R = 6 rows of test-mini's vocabulary with ld = V + 3: history lengths 0, 1, n - 1, n, 40 (a run of one id) and
    447 (n-grams across the prefix / generated boundary), ids from an 8-id alphabet with 0 and V - 1, some logits
    already -inf, every penalty; once with all rows live and once with one finished. The output equals the
    restatement bit for bit (its -inf set included), finished rows and the padding columns are untouched, and state
    and tokens are not written."""
    ld = V + 3
    for finished in (None, 3):
        rows = [(pre, gen, r == finished) for r, (pre, gen, _) in enumerate(kernel_cases(n))]
        R = len(rows)
        x = kernel_logits(R, ld)
        for lang_slot in (False, True):
            prefix, plen, tokens, state = _device_rows(rows, lang_slot)
            s0, t0 = state.clone(), tokens.clone()
            for p in PENALTIES:
                lg = torch.from_numpy(x).to(DEV)
                _history(lg, R, ld, prefix, plen, tokens, state, p, n, False)
                torch.cuda.synchronize()
                got = lg.cpu().numpy()
                for r, (pre, gen, fin) in enumerate(rows):
                    ref = x[r, :V] if fin else hr.history_processors(x[r, :V], pre + gen, p, n)
                    assert np.array_equal(got[r, :V].view(np.int32), ref.view(np.int32)), (n, p, r, finished)
                assert np.array_equal(got[:, V:].view(np.int32), x[:, V:].view(np.int32))
            assert torch.equal(state, s0) and torch.equal(tokens, t0)


def test_history_without_a_prefix_buffer():
    rows = [([], pre + gen, False) for pre, gen, _ in kernel_cases(3)]
    x = kernel_logits(len(rows), V)
    _, _, tokens, state = _device_rows(rows)
    lg = torch.from_numpy(x).to(DEV)
    _history(lg, len(rows), V, None, None, tokens, state, 1.3, 3, False)
    got = lg.cpu().numpy()
    for r, (_, gen, _) in enumerate(rows):
        ref = hr.history_processors(x[r], gen, 1.3, 3)
        assert np.array_equal(got[r].view(np.int32), ref.view(np.int32)), r


def test_torch_op_addresses_views_by_their_row_stride():
    """torch.ops.tw.logits_history_ on column-sliced views of wider buffers (tokens[:, :64] of [R][448], a prefix
    view, logits[:, :V] of ld = V + 3) equals the C-ABI call on the whole buffers."""
    from twamd import _ops

    tw = _ops.load()
    rows = [(pre, gen[:50], False) for pre, gen, _ in kernel_cases(3)]
    R, ld = len(rows), V + 3
    x = kernel_logits(R, ld)
    prefix, plen, tokens, state = _device_rows(rows)
    a, b = torch.from_numpy(x).to(DEV), torch.from_numpy(x).to(DEV)
    _history(a, R, ld, prefix, plen, tokens, state, 1.3, 3, False)
    tw.logits_history_(b[:, :V], V, prefix[:, :8], plen, tokens[:, :64], state, 1.3, 3, False)
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert not torch.equal(a, torch.from_numpy(x).to(DEV))


@pytest.mark.parametrize("n,p", [(0, 1.3), (2, 1.0), (3, 1.3), (1, 0.7), (5, 1.3)])
def test_logprob_mode_against_float64(n, p):
    """to_logprobs: the -inf set is exact and finite values are within 1e-4 of the float64 restatement (scores under
    64 in magnitude: an f32 ulp is ~4e-6 and the tree-summed logsumexp over 5e4 terms adds a few)."""
    ld = V + 3
    rows = kernel_cases(n)
    R = len(rows)
    x = kernel_logits(R, ld)
    prefix, plen, tokens, state = _device_rows(rows)
    lg = torch.from_numpy(x).to(DEV)
    _history(lg, R, ld, prefix, plen, tokens, state, p, n, True)
    got = lg.cpu().numpy()
    for r, (pre, gen, _) in enumerate(rows):
        ref = hr.history_processors(x[r, :V].astype(np.float64), pre + gen, p, n, to_logprobs=True)
        assert np.array_equal(np.isneginf(got[r, :V]), np.isneginf(ref)), r
        fin = np.isfinite(ref)
        err = np.abs(got[r, :V][fin] - ref[fin]).max()
        print(f"n={n} p={p} row {r}: max |err| {err:.2e}")
        assert err <= 1e-4, (r, err)
    assert np.array_equal(got[:, V:].view(np.int32), x[:, V:].view(np.int32))


def test_chain_with_select_and_sample():
    """30 steps of pre-pass + tw_logits_select on random logits with a few dominant text tokens (so ids and 2-grams
    repeat) and an often dominant timestamp block: tokens and state equal restatement + the oracle's processor chain
    + argmax at every step; the same run through tw_logits_sample at temperature 0 picks the same tokens, and its
    SUMLP is the penalised scores' log-probability (1e-3 per step)."""
    gen, g = _gcfg()
    st = gen.special
    R, steps, pen, n = 6, 30, 1.3, 2
    p = _params(gen, max_new=steps)
    sb = _suppress_bits(gen.suppress_tokens)
    pres = [[], [st.sot], [st.sot, st.lang_begin + 3, st.transcribe], [1000, 2000, st.sot, st.lang_begin, st.transcribe],
            [st.eot, st.eot, 1000, st.sot, st.lang_begin + 1, st.transcribe], [2000] * 7]
    rows = [(pre, [], False) for pre in pres]
    prefix, plen, _, _ = _device_rows(rows, lang_slot=True)
    sa, sb2 = _fresh_state(R), _fresh_state(R)
    for r, pre in enumerate(pres):
        if pre:
            sa[r, _lib.TW_ST_LANG] = sb2[r, _lib.TW_ST_LANG] = pre[0]
    toka = torch.zeros(R, T, dtype=torch.int32, device=DEV)
    tokb = torch.zeros_like(toka)
    ida, idb = torch.zeros(R, dtype=torch.int32, device=DEV), torch.zeros(R, dtype=torch.int32, device=DEV)
    ws = torch.empty(R, _lib.TW_SELECT_WS_PER_ROW, device=DEV)
    rng = np.random.default_rng(5)
    hot = rng.choice(st.eot, 5, replace=False)
    ref_lp = np.zeros(R)
    hist = [[] for _ in range(R)]
    done = [False] * R
    changed = 0
    for step in range(steps):
        x = rng.standard_normal((R, V)).astype(np.float32) * 2
        x[:, hot] += rng.choice([5.0, 7.0, 9.0], size=(R, 5)).astype(np.float32)
        x[:, g.ts_begin:] += rng.choice([-4.0, 0.5, 3.0], size=(R, 1)).astype(np.float32)
        la, lb = torch.from_numpy(x).to(DEV), torch.from_numpy(x).to(DEV)
        _history(la, R, V, prefix, plen, toka, sa, pen, n, False)
        _lib.call("tw_logits_select", la.data_ptr(), R, V, sb.data_ptr(), ctypes.byref(p), sa.data_ptr(),
                  toka.data_ptr(), T, ida.data_ptr(), None, ws.data_ptr(), S())
        _history(lb, R, V, prefix, plen, tokb, sb2, pen, n, False)
        _lib.call("tw_logits_sample", lb.data_ptr(), R, V, sb.data_ptr(), ctypes.byref(p), 0.0, 50, 7, None,
                  sb2.data_ptr(), tokb.data_ptr(), T, idb.data_ptr(), None, S())
        torch.cuda.synchronize()
        ref_state = sa[:, :6].cpu().numpy()
        for r in range(R):
            if done[r]:
                ref = g.eot
            else:
                y = hr.history_processors(x[r], pres[r] + hist[r], pen, n)
                s = wo.process_logits(y, hist[r], g, True)
                ref = int(np.argmax(s))
                changed += ref != int(np.argmax(wo.process_logits(x[r], hist[r], g, True)))
                fin = s[np.isfinite(s)].astype(np.float64)
                m = fin.max()
                ref_lp[r] += s[ref] - (m + np.log(np.exp(fin - m).sum()))
            assert int(toka[r, step]) == ref and int(tokb[r, step]) == ref, (step, r)
            hist[r].append(ref)
            done[r] = done[r] or ref == g.eot or len(hist[r]) >= steps
            assert ref_state[r, _lib.TW_ST_NGEN] == step + 1 and ref_state[r, _lib.TW_ST_LAST] == ref
            assert ref_state[r, _lib.TW_ST_FINISHED] == int(done[r]), (step, r)
        assert torch.equal(sa[:, :6], sb2[:, :6]), step
    assert changed > 0, "the processors never changed a decision: the test inputs do not exercise them"
    got = sb2[:, _lib.TW_ST_SUMLP].cpu().view(torch.float32).numpy()
    np.testing.assert_allclose(got, ref_lp, atol=1e-3 * steps, rtol=0)


def _synthetic_logits(history, salt, tsb, eot):
    """Deterministic logits of a beam's history (as tests/test_gpu_beam.py: Gaussian + boosted tokens), with a few
    fixed hot text tokens so that beams repeat ids and 2-grams."""
    h = hash((salt,) + tuple(int(t) for t in history)) & 0xFFFFFFFF
    rng = np.random.default_rng(h)
    x = rng.standard_normal(V).astype(np.float32) * 2.0
    x[[1000 + salt, 2000, 3000]] += 8.0
    x[rng.integers(0, tsb, 4)] += 7.0
    x[tsb + rng.integers(0, 60, 3)] += 6.5
    x[eot] += 3.0 + 0.3 * len(history)
    return x


def _beam_run(W, nb, max_new, pen, n, prefixes, flag, salt0=0, lp=1.0):
    gen, g = _gcfg()
    st = gen.special
    R, P = W * nb, 3
    logits = torch.empty(R, V, device=DEV)
    state = _fresh_state(R)
    tokens = torch.zeros(R, T, dtype=torch.int32, device=DEV)
    ids = torch.zeros(R, dtype=torch.int32, device=DEV)
    pos = torch.full((R,), P, dtype=torch.int32, device=DEV)
    run_score = torch.full((W, nb), -1e9, device=DEV)
    run_score[:, 0] = 0
    fin_score = torch.full((R,), -1e9, device=DEV)
    fin_flag = torch.zeros(R, dtype=torch.int32, device=DEV)
    fin_len = torch.zeros(R, dtype=torch.int32, device=DEV)
    fin_tokens = torch.zeros(R, T, dtype=torch.int32, device=DEV)
    win = torch.tensor([[1, 0, 0, 0]] * W, dtype=torch.int32, device=DEV)
    src_rows = torch.zeros(R, dtype=torch.int32, device=DEV)
    ws = torch.empty(int(_lib.load().tw_beam_workspace_bytes(R)), dtype=torch.uint8, device=DEV)
    sup = _suppress_bits(gen.suppress_tokens)
    sel = _params(gen, max_new)
    bp = _lib.TwBeamParams(nb, max_new, lp, T) if flag is None else _lib.TwBeamParams(nb, max_new, lp, T, flag)
    bst = _lib.TwBeamState(run_score.data_ptr(), fin_score.data_ptr(), fin_flag.data_ptr(), fin_len.data_ptr(),
                           fin_tokens.data_ptr(), win.data_ptr(), src_rows.data_ptr())
    prefix = plen = None
    if prefixes is not None:
        prefix, plen, _, _ = _device_rows([(prefixes[r // nb], [], False) for r in range(R)])
    tsb = st.timestamp_begin
    hist = [[] for _ in range(R)]
    steps = 0
    while steps < max_new:
        host = np.stack([_synthetic_logits(hist[r], salt0 + r // nb, tsb, st.eot) for r in range(R)])
        logits.copy_(torch.from_numpy(host))
        if prefixes is not None:
            _history(logits, R, V, prefix, plen, tokens, state, pen, n, True)
        _lib.call("tw_beam_step", logits.data_ptr(), W, V, sup.data_ptr(), ctypes.byref(sel), ctypes.byref(bp),
                  ctypes.byref(bst), state.data_ptr(), tokens.data_ptr(), ids.data_ptr(), pos.data_ptr(),
                  ws.data_ptr(), S())
        steps += 1
        tk = tokens.cpu().numpy()
        hist = [list(tk[r, :steps]) for r in range(R)]
        if bool(win[:, 1].all().item()):
            break
    return {"fin_tokens": fin_tokens.cpu(), "fin_len": fin_len.cpu(), "fin_score": fin_score.cpu(),
            "fin_flag": fin_flag.cpu(), "tokens": tokens.cpu(), "run_score": run_score.cpu(), "state": state.cpu(),
            "steps": steps}


def test_beam_step_after_the_history_pass(monkeypatch):
    """2 windows x 3 beams: pre-pass (to_logprobs) + tw_beam_step with TwBeamParams.scores_are_logprobs against the
    numpy beam core whose processor chain is fed penalised log-probabilities; the pass rule of tests/test_gpu_beam.py
    (best hypothesis equal, finished scores rtol 1e-5 / atol 1e-4, finished flags equal)."""
    gen, g = _gcfg()
    st = gen.special
    W, nb, max_new, pen, n, P = 2, 3, 10, 1.3, 2, 3
    prefixes = [[st.sot, st.lang_begin, st.transcribe], [2000, 3000, st.sot, st.lang_begin + 1, st.transcribe]]
    out = _beam_run(W, nb, max_new, pen, n, prefixes, flag=1)
    plain = _beam_run(W, nb, max_new, pen, n, None, flag=0)
    orig = wo.process_logits
    differs = 0
    for w in range(W):
        monkeypatch.setattr(wo, "process_logits", lambda s, sampled, g_, use_ts, _w=w: orig(
            hr.history_processors(s, prefixes[_w] + [int(t) for t in sampled], pen, n), sampled, g_, use_ts))

        def step(srcs, toks, _st={"h": [[] for _ in range(nb)]}, _w=w):
            _st["h"] = [_st["h"][s] + [t] for s, t in zip(srcs, toks)]
            return [_synthetic_logits(h, _w, st.timestamp_begin, st.eot) for h in _st["h"]]

        ref, tr = wo.beam_search_core(_synthetic_logits([], w, st.timestamp_begin, st.eot), step, P, max_new, g, True, nb)
        monkeypatch.setattr(wo, "process_logits", orig)
        got = out["fin_tokens"][w * nb, : int(out["fin_len"][w * nb])].tolist()
        assert got == ref, (w, got, ref)
        np.testing.assert_allclose(out["fin_score"].view(W, nb)[w].numpy(), tr["fin_score"], rtol=1e-5, atol=1e-4)
        assert [bool(x) for x in out["fin_flag"].view(W, nb)[w].numpy()] == [bool(x) for x in tr["fin_flag"]]
        differs += got != plain["fin_tokens"][w * nb, : int(plain["fin_len"][w * nb])].tolist()
    assert differs > 0, "the processors changed no window's best hypothesis: the inputs do not exercise them"


@pytest.mark.parametrize("lp", [0.5, -2.0])
def test_beam_step_length_penalty_changes_the_best_hypothesis(lp):
    """TwBeamParams.length_penalty (what generate_kwargs' length_penalty sets): 4 windows x 3 beams of the synthetic
    logits, whose EOS grows likelier with length so hypotheses finish at different lengths. The kernel equals the numpy
    beam core at that exponent (the pass rule of tests/test_gpu_beam.py), and some window's best hypothesis differs
    from the one at 1.0 — on the device and in the reference alike."""
    gen, g = _gcfg()
    st = gen.special
    W, nb, max_new, P = 4, 3, 16, 3
    out, plain = _beam_run(W, nb, max_new, 1.0, 0, None, 0, lp=lp), _beam_run(W, nb, max_new, 1.0, 0, None, 0)
    differs = 0
    for w in range(W):
        refs = []
        for e in (lp, 1.0):
            def step(srcs, toks, _st={"h": [[] for _ in range(nb)]}, _w=w):
                _st["h"] = [_st["h"][s] + [t] for s, t in zip(srcs, toks)]
                return [_synthetic_logits(h, _w, st.timestamp_begin, st.eot) for h in _st["h"]]

            refs.append(wo.beam_search_core(_synthetic_logits([], w, st.timestamp_begin, st.eot), step, P, max_new, g,
                                            True, nb, e))
        (ref, tr), (ref1, _) = refs
        got = out["fin_tokens"][w * nb, : int(out["fin_len"][w * nb])].tolist()
        got1 = plain["fin_tokens"][w * nb, : int(plain["fin_len"][w * nb])].tolist()
        assert got == ref and got1 == ref1, (w, got, ref)
        np.testing.assert_allclose(out["fin_score"].view(W, nb)[w].numpy(), tr["fin_score"], rtol=1e-5, atol=1e-4)
        assert [bool(x) for x in out["fin_flag"].view(W, nb)[w].numpy()] == [bool(x) for x in tr["fin_flag"]]
        differs += got != got1
    assert differs > 0, "the exponent changed no window's best hypothesis: the inputs do not exercise it"


def test_beam_step_flag_zero_is_the_parent_struct():
    """tw_beam_step with the options off: TwBeamParams with the new flag set to zero and the struct as the parent
    fills it (four fields) give identical outputs. ctypes zero-fills the field the parent leaves out, so the two
    structs are the same bytes: this pins the ABI default (an appended field, zero = off), not the kernel. What
    protects the default beam arithmetic are the bit-for-bit beam pins of tests/test_gpu_beam.py
    (test_beam_step_matches_oracle_core, test_engine_beam_search_matches_transformers), which run with the flag zero."""
    a = _beam_run(2, 3, 8, 1.0, 0, None, flag=0)
    b = _beam_run(2, 3, 8, 1.0, 0, None, flag=None)
    assert a["steps"] == b["steps"]
    for k in ("fin_tokens", "fin_len", "fin_score", "fin_flag", "tokens", "run_score", "state"):
        assert torch.equal(a[k].view(torch.int32) if a[k].dtype == torch.float32 else a[k],
                           b[k].view(torch.int32) if b[k].dtype == torch.float32 else b[k]), k
