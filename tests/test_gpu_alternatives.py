"""Token alternatives on the MI355X: tw_token_topk against the float64 restatement (tests/alternatives_ref.py) and on
edge rows, the captured against the eager decode, the engine's invariants per pass type, the fp32 engine's forced
lists against the oracle, and the callable's return_alternatives / align(alternatives=).

Tolerances. Ids are compared exactly: the ranking compares f32 values. Log-probabilities 1e-3 against float64 (the
per-step f32-vs-f64 bound of tests/test_gpu_confidence.py). A step whose timestamp-rule margin is within 1e-3 of zero
is left out of the id comparison (the f32 and the f64 rule may decide differently), at most 1 % of the steps: on the
seeded logits used here the smallest |margin| is 0.25 where the rule fires and 0.059 where it does not (R = 1; 0.31
at R = 5), checked on the CPU, so none is left out. Two values of the same quantity from two f32 kernels (slot 0
against token_lp, a beam token against its fin_tlp term) 1e-4. The fp32 engine against the oracle: an entry is
compared when the oracle's gaps to the neighbouring ranks exceed 2e-3, twice the 1e-3 logit bound that engine is
asserted at; at most 5 % may be left out (2.1 % on the CPU with the oracle alone)."""
import ctypes

import numpy as np
import pytest
import torch

import align_ref
import alternatives_ref as ar
import confidence_ref as cr
from oracle import whisper_oracle as wo
from test_gpu_confidence import STEPS, _fresh_state, _gcfg, _params, _step_logits, _suppress_bits
from twamd import _lib
from twamd.config import PRESETS
from twamd.frontend import chunk_windows, time_precision
from twamd.pipeline import TurboTranscriber
from twamd.segments import retrieve_segment, strip_generated
from twamd.synth_audio import speech_like, white_noise
from twamd.tokenizer import decode_asr

pytestmark = pytest.mark.gpu
DEV = "cuda"
D = PRESETS["test-mini"]
V = D.vocab
CANARY_ID, CANARY_LP = -777, 12345.0


def S():
    return torch.cuda.current_stream().cuda_stream


def _ws(R):
    return torch.empty(int(_lib.load().tw_token_topk_workspace_bytes(R)), dtype=torch.uint8, device=DEV)


def _out(R, T, k):
    return (torch.full((R, T, k), CANARY_ID, dtype=torch.int32, device=DEV),
            torch.full((R, T, k), CANARY_LP, dtype=torch.float32, device=DEV))


def _topk(lg, R, ld, sb, p, st, k, ids, lps, T, ws):
    _lib.call("tw_token_topk", lg.data_ptr(), R, ld, None if sb is None else sb.data_ptr(), ctypes.byref(p),
              st.data_ptr(), k, ids.data_ptr(), lps.data_ptr(), T, ws.data_ptr(), S())


# ---- 1. the kernel against the restatement --------------------------------------------------------------------------
PAD = 6
T_OUT = 40


def _run_steps(R, xs, gen, k):
    """tw_token_topk (k > 0) then tw_logits_select on every step's logits, rows of V + PAD columns whose pad is
    +inf. Returns tokens, state and the two output buffers."""
    p = _params(gen, max_new=STEPS)
    sb = _suppress_bits(gen.suppress_tokens, V)
    st = _fresh_state(R)
    tok = torch.zeros(R, 64, dtype=torch.int32, device=DEV)
    ids = torch.zeros(R, dtype=torch.int32, device=DEV)
    pos = torch.zeros(R, dtype=torch.int32, device=DEV)
    sel_ws = torch.empty(R, _lib.TW_SELECT_WS_PER_ROW, device=DEV)
    a_ids, a_lps = _out(R, T_OUT, max(k, 1))
    ws = _ws(R)
    lg = torch.full((R, V + PAD), float("inf"), device=DEV)
    for x in xs:
        lg[:, :V] = torch.from_numpy(x).to(DEV)
        if k:
            _topk(lg, R, V + PAD, sb, p, st, k, a_ids, a_lps, T_OUT, ws)
        _lib.call("tw_logits_select", lg.data_ptr(), R, V + PAD, sb.data_ptr(), ctypes.byref(p), st.data_ptr(),
                  tok.data_ptr(), 64, ids.data_ptr(), pos.data_ptr(), sel_ws.data_ptr(), S())
    torch.cuda.synchronize()
    return tok.cpu(), st.cpu(), a_ids.cpu().numpy(), a_lps.cpu().numpy()


@pytest.fixture(scope="module")
def step_ref():
    """Per R: the step logits, the plain selection's tokens / state, and per live (row, step) the restatement's top 8
    (computed once, shared by every k)."""
    gen, g = _gcfg()
    out = {}
    for R in (1, 5):
        xs = _step_logits(R, V, g.ts_begin, g.eot)
        tok, st, _, _ = _run_steps(R, xs, gen, 0)
        ref, n_live = {}, []
        for r in range(R):
            hist = []
            for step in range(STEPS):
                ref[r, step] = ar.step_alternatives(xs[step][r], hist, g, True, 8)
                t = int(tok[r, step])
                hist.append(t)
                if t == g.eot:
                    break
            n_live.append(len(hist))
        out[R] = {"xs": xs, "tok": tok, "st": st, "ref": ref, "n_live": n_live}
    return out


@pytest.mark.parametrize("R", [1, 5])
@pytest.mark.parametrize("k", [1, 3, 8])
def test_topk_in_front_of_select(step_ref, R, k):
    gen, g = _gcfg()
    z = step_ref[R]
    tok, st, ids, lps = _run_steps(R, z["xs"], gen, k)
    assert torch.equal(tok, z["tok"]), "the call changed a token"
    assert torch.equal(st, z["st"]), "the call changed the row state"
    if R == 5:
        assert z["n_live"][1] == 11 and z["n_live"][4] == 18 and max(z["n_live"]) == STEPS  # rows that finish early
    skipped, steps, worst = 0, 0, 0.0
    for r in range(R):
        n = z["n_live"][r]
        for q in range(n):
            want_ids, want_lps, margin = z["ref"][r, q]
            steps += 1
            assert len(want_ids) >= 8  # (every step here has at least 9 eligible ids: no sentinel among the k)
            if abs(margin) <= 1e-3:
                skipped += 1
                continue
            assert ids[r, q].tolist() == want_ids[:k], (r, q)
            d = np.abs(lps[r, q].astype(np.float64) - np.asarray(want_lps[:k]))
            worst = max(worst, float(d.max()))
            assert int(ids[r, q, 0]) == int(tok[r, q]), (r, q, "slot 0 is the token the selection commits")
        # a finished row writes sentinels, at every later position the steps reach
        assert np.all(ids[r, n:STEPS] == -1) and np.all(np.isneginf(lps[r, n:STEPS])), r
        # nothing outside [b][q][0..k) of the positions the steps reached
        assert np.all(ids[r, STEPS:] == CANARY_ID) and np.all(lps[r, STEPS:] == CANARY_LP), r
    print(f"R={R} k={k}: {steps} steps, {skipped} borderline left out, worst |lp - f64| {worst:.2e} (bound 1e-3)")
    assert skipped <= 0.01 * steps
    assert worst <= 1e-3


# ---- 2. edge rows, one launch each ----------------------------------------------------------------------------------
def _neutral(gen):
    p = _params(gen, use_ts=False)
    p.n_begin_suppress = 0
    return p


def _one(x, p, sb, k, q=1, T=4, finished=False):
    """One launch on one row at generated position q; returns (ids [T][k], lps [T][k])."""
    lg = torch.from_numpy(np.asarray(x, np.float32)[None, :]).to(DEV).contiguous()
    st = _fresh_state(1)
    st[0, _lib.TW_ST_NGEN] = q
    st[0, _lib.TW_ST_FINISHED] = int(finished)
    st0 = st.clone()
    ids, lps = _out(1, T, k)
    _topk(lg, 1, lg.shape[1], sb, p, st, k, ids, lps, T, _ws(1))
    torch.cuda.synchronize()
    assert torch.equal(st, st0), "the state is only read"
    return ids[0].cpu().numpy(), lps[0].cpu().numpy()


def _only(ids, lps, q):
    """Every position but q still holds the canary."""
    m = np.ones(ids.shape[0], bool)
    m[q] = False
    return np.all(ids[m] == CANARY_ID) and np.all(lps[m] == CANARY_LP)


def test_edge_three_eligible_ids():
    gen, _ = _gcfg()
    rng = np.random.default_rng(1)
    x = rng.standard_normal(V).astype(np.float32)
    keep = [17, 30000, V - 1]
    sb = _suppress_bits([t for t in range(V) if t not in keep], V)
    ids, lps = _one(x, _neutral(gen), sb, 8)
    s = np.full(V, -np.inf, np.float32)
    s[keep] = x[keep]
    want_ids, want_lps = ar.rank(s, 8)
    assert len(want_ids) == 3
    assert ids[1].tolist() == want_ids + [-1] * 5
    np.testing.assert_allclose(lps[1, :3], want_lps, atol=1e-3, rtol=0)
    assert np.all(np.isneginf(lps[1, 3:])) and _only(ids, lps, 1)
    # a finished row: sentinels in every slot
    ids, lps = _one(x, _neutral(gen), sb, 8, finished=True)
    assert np.all(ids[1] == -1) and np.all(np.isneginf(lps[1])) and _only(ids, lps, 1)


@pytest.mark.parametrize("use_ts", [False, True])
def test_edge_exact_ties_lower_id_first(use_ts):
    """The same value at ids that fall in different threads (v, v + 64: also different waves of a 256-thread block's
    stride), v + 256 (the same thread's next element) and on the two sides of a chunk boundary; one larger value
    above them, so the ties sit inside the top k."""
    gen, g = _gcfg()
    rng = np.random.default_rng(2)
    x = rng.standard_normal(V).astype(np.float32)
    span = g.ts_begin if use_ts else V  # (with timestamps the text ids are split over 15 chunks, else all over 16)
    nc = _lib.TW_SELECT_CHUNKS - 1 if use_ts else _lib.TW_SELECT_CHUNKS
    b = 5 * span // nc  # the first id of chunk 5
    v = 1000
    tied = [v, v + 64, v + 256, b - 1, b]
    x[tied] = 9.0
    x[40000] = 10.0
    p = _params(gen, use_ts=use_ts)
    sb = _suppress_bits(gen.suppress_tokens, V)
    assert not set(tied + [40000]) & set(gen.suppress_tokens)
    hist = [g.ts_begin + 3, 300]  # (text after a timestamp: text ids are allowed; the rule does not fire here)
    lg = torch.from_numpy(x[None, :]).to(DEV)
    st = _fresh_state(1)
    st[0, _lib.TW_ST_NGEN], st[0, _lib.TW_ST_LAST], st[0, _lib.TW_ST_PENULT] = 2, hist[1], hist[0]
    st[0, _lib.TW_ST_LASTTS] = hist[0]
    ids, lps = _out(1, 4, 8)
    _topk(lg, 1, V, sb, p, st, 8, ids, lps, 4, _ws(1))
    torch.cuda.synchronize()
    want_ids, want_lps, margin = ar.step_alternatives(x, hist, g, use_ts, 8)
    assert want_ids[:6] == [40000] + sorted(tied) and not margin > 0
    assert ids[0, 2].tolist() == want_ids
    np.testing.assert_allclose(lps[0, 2].cpu().numpy(), want_lps, atol=1e-3, rtol=0)
    assert lps[0, 2, 1] == lps[0, 2, 5]


def test_edge_raw_row_is_log_softmax():
    gen, _ = _gcfg()
    rng = np.random.default_rng(3)
    x = (rng.standard_normal(V) * 3).astype(np.float32)
    x[gen.suppress_tokens[0]] = 50.0  # (a suppressed id wins: no mask in raw mode)
    ids, lps = _one(x, _neutral(gen), None, 8, q=0)  # (q = 0: no begin-suppression either)
    want_ids, want_lps = ar.raw_alternatives(x, 8)
    assert ids[0].tolist() == want_ids and want_ids[0] == gen.suppress_tokens[0]
    np.testing.assert_allclose(lps[0], want_lps, atol=1e-3, rtol=0)
    ls = torch.log_softmax(torch.from_numpy(x).double(), 0).numpy()
    np.testing.assert_allclose(lps[0], ls[want_ids], atol=1e-3, rtol=0)
    assert _only(ids, lps, 0)


def test_edge_position_outside_the_buffer_and_bad_k():
    gen, _ = _gcfg()
    x = np.random.default_rng(4).standard_normal(V).astype(np.float32)
    for q in (4, 5, -1):
        ids, lps = _one(x, _neutral(gen), None, 3, q=q, T=4)
        assert np.all(ids == CANARY_ID) and np.all(lps == CANARY_LP), q
    lib = _lib.load()
    lg = torch.from_numpy(x[None, :]).to(DEV)
    st = _fresh_state(1)
    ids, lps = _out(1, 4, 8)
    ws = _ws(1)
    p = _neutral(gen)
    ok = [lg.data_ptr(), 1, V, None, ctypes.byref(p), st.data_ptr(), 3, ids.data_ptr(), lps.data_ptr(), 4,
          ws.data_ptr(), S()]
    for k in (0, 9):
        bad = list(ok)
        bad[6] = k
        assert lib.tw_token_topk(*bad) == 1 and b"tw_token_topk" in lib.tw_last_error(), k  # TW_ERR_ARG
    for i in (0, 4, 5, 7, 8, 10):  # every required pointer
        bad = list(ok)
        bad[i] = None
        assert lib.tw_token_topk(*bad) == 1, i
    torch.cuda.synchronize()
    assert torch.all(ids == CANARY_ID) and torch.all(lps == CANARY_LP)  # nothing ran
    assert lib.tw_token_topk(*ok) == 0
    torch.cuda.synchronize()
    assert torch.all(ids[0, 0, :3] >= 0)


# ---- the engine -----------------------------------------------------------------------------------------------------
CLIPS = [speech_like(30.0, 1234), white_noise(12.3, 7), speech_like(40.0, 5)[: 20 * 16000]]  # test_gpu_align.py's
NF = [-(-len(c) // 160) for c in CLIPS]


def _load(eng):
    host = np.zeros((3, 480000), np.float32)
    for i, c in enumerate(CLIPS):
        host[i, : len(c)] = c
    eng.wave[:3].copy_(torch.from_numpy(host))
    eng.logmel(3)
    eng.encode(3, row_map=False, seek=False)


@pytest.fixture(scope="module")
def mini():
    t = TurboTranscriber.from_pretrained("test-mini", seed=1234, max_batch=3)
    yield t
    t.close()


def _well_formed(alts, gen, k):
    """One token's list: at most k entries, descending, ids distinct, inside [0, V), never a suppressed id, and
    probabilities that sum to at most 1 (lse <= 0 up to the f32 rounding of the kernel's own logsumexp: one ulp of a
    value below 16 is 9.5e-7, so 2e-6)."""
    ids, lps = [a[0] for a in alts], [a[1] for a in alts]
    assert 1 <= len(alts) <= k
    assert lps == sorted(lps, reverse=True) and all(np.isfinite(lps))
    assert len(set(ids)) == len(ids) and all(0 <= i < V for i in ids)
    assert not set(ids) & set(gen.suppress_tokens)
    assert cr.logsumexp(np.asarray(lps)) <= 2e-6


def test_captured_equals_eager(mini):
    """decode_pass(top_alternatives=8) with the captured prompt / step graphs and issued eagerly: identical lists,
    and the tokens of the pass without the option."""
    eng = mini.engine
    tail = eng.prompt_tail("transcribe", True)
    res = {}
    try:
        for graphs in (True, False):
            eng.use_graphs = graphs
            _load(eng)
            plain = eng.decode_pass(3, tail, None, 40)
            assert plain.token_alt is None
            _load(eng)
            res[graphs] = eng.decode_pass(3, tail, None, 40, top_alternatives=8)
            assert res[graphs].tokens == plain.tokens, "the option changed a token"
    finally:
        eng.use_graphs = True
    assert res[True].tokens == res[False].tokens
    assert res[True].token_alt == res[False].token_alt
    assert sum(len(a) for row in res[True].token_alt for a in row) > 100


def test_greedy_invariants(mini):
    eng, gen = mini.engine, mini.gen
    tail = eng.prompt_tail("transcribe", True)
    _load(eng)
    res = eng.decode_pass(3, tail, None, 40, top_alternatives=8, token_logprobs=True)
    eot = gen.special.eot
    n = 0
    for toks, lps, alts in zip(res.tokens, res.token_lp, res.token_alt):
        assert len(toks) == len(lps) == len(alts)
        live = (toks.index(eot) + 1) if eot in toks else len(toks)
        for q in range(len(toks)):
            if q >= live:  # a pad after the row finished: sentinels only
                assert alts[q] == [] and lps[q] == 0.0
                continue
            _well_formed(alts[q], gen, 8)
            assert alts[q][0][0] == toks[q], (q, "slot 0 is the committed token")
            assert abs(alts[q][0][1] - lps[q]) <= 1e-4, (q, alts[q][0][1], lps[q])
            n += 1
    assert n > 30


@pytest.mark.parametrize("k", [4, 8])
def test_beam_tokens_are_in_their_lists(mini, k):
    """num_beams = 2: the chosen token is one of its row's top 2 * num_beams = 4 <= k candidates, so every token of the
    best hypothesis is in the list gathered for it, with the log-probability tw_beam_step recorded (fin_tlp). A wrong
    row or step in the gather would miss tokens or values."""
    eng, gen = mini.engine, mini.gen
    tail = eng.prompt_tail("transcribe", True)
    _load(eng)
    plain = eng.beam_pass(3, 2, tail, None, 40)
    _load(eng)
    res = eng.beam_pass(3, 2, tail, None, 40, top_alternatives=k, token_logprobs=True)
    assert res.tokens == plain.tokens
    n = 0
    for toks, lps, alts in zip(res.tokens, res.token_lp, res.token_alt):
        assert len(toks) == len(lps) == len(alts) and len(toks) > 0
        for q, t in enumerate(toks):
            _well_formed(alts[q], gen, k)
            d = dict(alts[q])
            assert t in d, (q, t, alts[q])
            assert abs(d[t] - lps[q]) <= 1e-4, (q, d[t], lps[q])
            n += 1
    assert n > 20


def test_sampled_lists_equal_the_restatement(mini, monkeypatch):
    """temperature 0.4: the lists are the greedy ones of each step's scores (temperature 1, no top-k warper),
    restated on the host from the logits the launch read and the pass's own tokens."""
    eng, gen = mini.engine, mini.gen
    _, g = _gcfg()
    tail = eng.prompt_tail("transcribe", True)
    seen = []
    real = _lib.call

    def spy(name, *args):
        if name == "tw_token_topk":
            seen.append(eng.logits[:3].clone())  # (on the engine's stream, in front of the launch)
        return real(name, *args)

    _load(eng)
    monkeypatch.setattr(_lib, "call", spy)
    res = eng.sample_pass(3, tail, None, 24, temperature=0.4, seed=11, top_alternatives=8)
    monkeypatch.setattr(_lib, "call", real)
    xs = [x.cpu().numpy() for x in seen]
    eot = gen.special.eot
    skipped = steps = 0
    worst = 0.0
    drawn_elsewhere = 0
    for r, (toks, alts) in enumerate(zip(res.tokens, res.token_alt)):
        assert len(toks) == len(alts) <= len(xs)
        live = (toks.index(eot) + 1) if eot in toks else len(toks)
        for q in range(live):
            _well_formed(alts[q], gen, 8)
            ids, lps, margin = ar.step_alternatives(xs[q][r], toks[:q], g, True, 8)
            steps += 1
            if abs(margin) <= 1e-3:
                skipped += 1
                continue
            assert [a[0] for a in alts[q]] == ids, (r, q)
            worst = max(worst, float(np.abs(np.asarray([a[1] for a in alts[q]]) - np.asarray(lps)).max()))
            drawn_elsewhere += toks[q] != ids[0]
        assert all(a == [] for a in alts[live:])
    print(f"sampled: {steps} steps, {skipped} borderline, worst |lp - f64| {worst:.2e}, "
          f"{drawn_elsewhere} draws that are not slot 0")
    assert steps > 20 and skipped <= 0.01 * steps + 1 and worst <= 1e-3


# ---- 5. the fp32 engine against the oracle --------------------------------------------------------------------------
def _oracle_steps(oracle, enc, prompt, text_ids, eot, nf):
    """align_ref.forced_reference's own per-step logits (the scoring steps: one per given token, EOT included)."""
    got = []
    real = oracle.decoder_step

    def step(t, cache):
        x = real(t, cache)
        got.append(np.asarray(x, np.float32).copy())
        return x

    oracle.decoder_step = step
    try:
        toks, lps, _ = align_ref.forced_reference(oracle, enc, prompt, text_ids, eot, [(1, 0)], nf)
    finally:
        del oracle.decoder_step
    return toks, lps, got[len(prompt) - 1:]


def test_fp32_forced_lists_vs_oracle():
    K, GAP = 8, 2e-3
    sd = wo.synth_state_dict(D.d_model, D.encoder_layers, D.decoder_layers, D.ffn, D.n_mels, D.vocab, 1234)
    oracle = wo.WhisperOracle(sd, D.heads)
    with TurboTranscriber.from_pretrained("test-mini", seed=1234, max_batch=3, precision="fp32") as t:
        eng, st = t.engine, t.gen.special
        eng.gen.alignment_heads = [(1, 0), (1, 1), (1, 2), (1, 3)]
        host = np.zeros((3, 480000), np.float32)
        for i, c in enumerate(CLIPS):
            host[i, : len(c)] = c
        eng.wave[:3].copy_(torch.from_numpy(host))
        eng.logmel(3)
        segs = eng.generate(3, task="transcribe", max_new_tokens=40)
        forced = [[x for x in s if x < st.eot][:23] for s in segs]
        assert all(len(f) >= 3 for f in forced)
        _load(eng)
        tail = eng.prompt_tail("transcribe", False)
        res = eng.force_pass(3, tail, None, forced, num_frames=NF, top_alternatives=K)
        _load(eng)
        plain = eng.force_pass(3, tail, None, forced, num_frames=NF)
    assert plain.token_alt is None and plain.tokens == res.tokens and plain.token_lp == res.token_lp
    total = left_out = 0
    worst = 0.0
    member_checked = 0
    for i in range(3):
        prompt = [st.sot, res.lang_ids[i], st.transcribe, st.notimestamps]
        enc = oracle.encode(wo.log_mel(CLIPS[i], D.n_mels))
        toks, _, steps = _oracle_steps(oracle, enc, prompt, forced[i], st.eot, NF[i])
        assert res.tokens[i] == toks and len(steps) == len(toks) == len(res.token_alt[i])
        for n, x in enumerate(steps):
            ids9, _ = ar.raw_alternatives(x, K + 1)
            xs = x[ids9].astype(np.float64)
            ls = align_ref.log_softmax64(x)
            got = res.token_alt[i][n]
            assert len(got) == K
            for j in range(K):
                total += 1
                if (j > 0 and xs[j - 1] - xs[j] <= GAP) or xs[j] - xs[j + 1] <= GAP:
                    left_out += 1
                    continue
                assert got[j][0] == ids9[j], (i, n, j, got, ids9)
                worst = max(worst, abs(got[j][1] - float(ls[ids9[j]])))
            # the given token: in its list exactly when its oracle rank is at most K, outside the margin
            tok = toks[n]
            in_list = dict(got)
            if tok in ids9[:K]:
                j = ids9.index(tok)
                if not ((j > 0 and xs[j - 1] - xs[j] <= GAP) or xs[j] - xs[j + 1] <= GAP):
                    assert tok in in_list and abs(in_list[tok] - res.token_lp[i][n]) <= 1e-4, (i, n, tok)
                    member_checked += 1
            elif xs[K - 1] - float(x[tok]) > GAP:
                assert tok not in in_list, (i, n, tok)
                member_checked += 1
    print(f"fp32 forced lists: {total} entries, {left_out} left out ({left_out / total:.1%}, cap 5 %), "
          f"worst |lp - oracle| {worst:.2e} (bound 1e-3), {member_checked} membership checks")
    assert left_out <= 0.05 * total
    assert worst <= 1e-3
    assert member_checked > 30


# ---- 6. the callable ------------------------------------------------------------------------------------------------
def _audio():
    return np.concatenate([speech_like(40.0, 5), white_noise(35.0, 11)]).astype(np.float32)


def _strip(out):
    return {"text": out["text"], "chunks": [{k: v for k, v in c.items() if k != "alternatives"} for c in out["chunks"]]}


def _check_words(tr, on, k):
    st = tr.gen.special
    for w in on["chunks"]:
        assert w["alternatives"], w
        for lst in w["alternatives"]:
            assert 1 <= len(lst) <= k
            assert [set(a) for a in lst] == [{"id", "text", "logprob"}] * len(lst)
            lps = [a["logprob"] for a in lst]
            assert lps == sorted(lps, reverse=True)
            for a in lst:
                special = a["id"] >= st.timestamp_begin or a["id"] in tr.vocab.all_special_ids
                assert a["text"] == (tr.vocab.id_to_token[a["id"]] if special else tr.vocab.decode([a["id"]]))


@pytest.mark.parametrize("num_beams", [1, None])
def test_callable_return_alternatives(mini, num_beams):
    """Greedy, and as shipped (no num_beams: beam 5)."""
    audio = _audio()
    gk = {"task": "transcribe", "max_new_tokens": 24, **({"num_beams": num_beams} if num_beams else {})}
    kw = dict(chunk_length_s=30, batch_size=2, return_timestamps="word", generate_kwargs=gk)
    off = mini(audio.copy(), **kw)
    on = mini(audio.copy(), **kw, return_alternatives=3)
    assert all("alternatives" not in c for c in off["chunks"])
    assert _strip(on) == off and on["chunks"]
    _check_words(mini, on, 3)
    # one list per token of the word: the windows' kept tokens (rebuilt from the raw passes, as the pipeline keeps
    # them) stitched on the host with each token riding as its own single alternative show every word's tokens
    st, sr = mini.gen.special, mini.sampling_rate
    outputs = []
    for i, w in enumerate(chunk_windows(len(audio), 30, None, sr)):
        seek, toks = 0, []
        for raw in mini.last_window_passes[i]:
            seg, adv = retrieve_segment(strip_generated(raw, st.eot), seek, min(3000 - seek, 3000), st.timestamp_begin)
            toks += seg
            seek += adv
        assert len(mini.last_window_token_alternatives[i]) == len(toks) == len(mini.last_window_token_timestamps[i])
        outputs.append({"tokens": toks, "token_timestamps": mini.last_window_token_timestamps[i],
                        "token_alternatives": [[[t, 0.0]] for t in toks],
                        "stride": (w.length / sr, w.stride_left / sr, w.stride_right / sr)})
    _, own = decode_asr(mini.vocab, outputs, return_timestamps="word", alternatives=True,
                        time_precision=time_precision(mini.engine.d.max_source_positions))
    assert [c["text"] for c in own["chunks"]] == [c["text"] for c in on["chunks"]]
    for w, o in zip(on["chunks"], own["chunks"]):
        word_tokens = [lst[0]["id"] for lst in o["alternatives"]]
        assert len(w["alternatives"]) == len(word_tokens), w
        if num_beams == 1:  # slot 0 is the chosen token: the word's own tokens (joined, its text)
            assert [lst[0]["id"] for lst in w["alternatives"]] == word_tokens, w
            assert mini.vocab.decode(word_tokens) == w["text"], w
    both = mini(audio.copy(), **kw, return_alternatives=3, return_confidence=True)
    assert [c["alternatives"] for c in both["chunks"]] == [c["alternatives"] for c in on["chunks"]]
    assert all(0.0 < c["probability"] <= 1.0 for c in both["chunks"])
    if num_beams == 1:  # greedy: the word's probability is the mean of its slot-0 probabilities
        for c in both["chunks"]:
            p = float(np.mean([np.exp(lst[0]["logprob"]) for lst in c["alternatives"]]))
            assert abs(p - c["probability"]) <= 1e-4, c


def test_callable_long_form(mini):
    audio = _audio()
    kw = dict(return_timestamps="word", generate_kwargs={"task": "transcribe", "num_beams": 1, "max_new_tokens": 40})
    off = mini(audio.copy(), **kw)
    on = mini(audio.copy(), **kw, return_alternatives=3)
    assert _strip(on) == off and on["chunks"]
    _check_words(mini, on, 3)
    for w in on["chunks"]:
        assert mini.vocab.decode([lst[0]["id"] for lst in w["alternatives"]]) == w["text"], w


def test_align_alternatives(mini):
    from test_gpu_align import _token_chunks
    mini.engine.gen.alignment_heads = [(1, 0), (1, 1), (1, 2), (1, 3)]
    x = np.concatenate([speech_like(40.0, 5), white_noise(35.0, 11)])
    r = mini(x, chunk_length_s=30, return_timestamps=True,
             generate_kwargs={"task": "transcribe", "num_beams": 1, "max_new_tokens": 40, "max_passes": 1})
    assert r["chunks"]
    chunks = _token_chunks(mini, x)
    assert len(chunks) >= 2
    off = mini.align(x, chunks, language="english", task="transcribe", batch_size=2)
    on = mini.align(x, chunks, language="english", task="transcribe", batch_size=2, alternatives=3)
    assert _strip(on) == {"text": off["text"], "chunks": off["chunks"]}
    assert on["chunk_avg_logprob"] == off["chunk_avg_logprob"]
    _check_words(mini, on, 3)
    n_lists = sum(len(w["alternatives"]) for w in on["chunks"])
    assert n_lists == sum(len(c["tokens"]) for c in chunks), "one list per given token"
    assert all(len(lst) == 3 for w in on["chunks"] for lst in w["alternatives"])  # (raw logits: every id is eligible)


def test_callable_refuses_bad_alternatives(mini):
    x = np.zeros(16000, np.float32)
    for kw in (dict(return_alternatives=3), dict(return_alternatives=3, return_timestamps=True),
               dict(return_alternatives=9, return_timestamps="word"),
               dict(return_alternatives=-1, return_timestamps="word")):
        with pytest.raises(ValueError, match="return_alternatives"):
            mini(x, chunk_length_s=30, **kw)
    with pytest.raises(ValueError, match="alternatives"):
        mini.align(x, [{"timestamp": (0.0, 1.0), "tokens": [300]}], alternatives=9)
