"""Per-token log-probabilities on the MI355X: tw_token_logprob (the pre-kernel of the greedy path), tw_logits_sample_lp,
tw_beam_step's run_tlp / fin_tlp, the engine's generate(token_logprobs=True) against transformers' own terms
(tests/golden/confidence.json, made by make_golden_confidence.py) and the callable's return_confidence.

Tolerances: tokens, draws and state bit-equal with the option off; per-step log-probabilities 1e-3 against the numpy
restatement (tests/confidence_ref.py; test_gpu_fallback.py's per-step bound: fp32 logits, fp32 vs float64); a sampled
step 1e-4; a beam hypothesis' terms sum to fin_lp within 1e-4 per token; the bf16 engine's per-token |d| <= 0.30
against transformers fp32 (|dx_tok| + |dlse|, each within the 0.15 logit bound test_gpu_fallback.py states for bf16
test-mini), its pass mean within that file's 0.03; the fp32 engine's per-token 1e-3. Observed on the MI355X: kernels
within 1.2e-6 of the restatement, the bf16 engine's worst per-token |d| 0.020 (pass means within 0.004), the fp32
engine's 1e-5."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import confidence_ref as cr
from oracle import whisper_oracle as wo
from twamd import _lib
from twamd.config import PRESETS, GenerationSettings
from twamd.pipeline import TurboTranscriber
from twamd.frontend import chunk_windows, time_precision
from twamd.segments import FallbackConfig, retrieve_segment, strip_generated
from twamd.synth_audio import silence, speech_like, white_noise
from twamd.tokenizer import decode_asr

pytestmark = pytest.mark.gpu
DEV = "cuda"
G = os.path.join(os.path.dirname(__file__), "golden")
D = PRESETS["test-mini"]


def S():
    return torch.cuda.current_stream().cuda_stream


def _gcfg():
    gen = GenerationSettings.default(D)
    st = gen.special
    return gen, wo.GenCfg(D.vocab, st.eot, st.sot, st.lang_begin, st.n_languages, st.transcribe, st.translate,
                          st.notimestamps, gen.suppress_tokens, gen.begin_suppress_tokens)


def _params(gen, max_new=40, use_ts=True, V=None):
    st = gen.special
    p = _lib.TwSelectParams()
    p.V, p.eos, p.pad = V or D.vocab, st.eot, st.eot
    p.ts_begin, p.no_timestamps = st.timestamp_begin, st.notimestamps
    p.max_initial_ts = gen.max_initial_timestamp_index
    p.use_timestamps, p.max_new, p.mode = int(use_ts), max_new, 0
    p.lo, p.hi = st.lang_begin, st.lang_end
    p.n_begin_suppress = len(gen.begin_suppress_tokens)
    for i, t in enumerate(gen.begin_suppress_tokens):
        p.begin_suppress[i] = t
    return p


def _suppress_bits(tokens, V):
    bits = np.zeros((V + 31) // 32, np.uint32)
    for t in tokens:
        bits[t >> 5] |= np.uint32(1) << np.uint32(t & 31)
    return torch.from_numpy(bits.view(np.int32)).to(DEV)


def _fresh_state(R):
    st = torch.zeros(R, _lib.TW_STATE_STRIDE, dtype=torch.int32, device=DEV)
    st[:, _lib.TW_ST_LAST:_lib.TW_ST_LASTTS + 1] = -1
    return st


# ---- the greedy pre-kernel ------------------------------------------------------------------------------------------
STEPS = 30


def _step_logits(R, V, tsb, eot):
    """The 30 steps of random logits of test_gpu_fallback.test_sample_greedy_equals_select_and_logprob (timestamp
    block often dominant); rows 1 and 4 (when present) are pushed to EOS at steps 10 and 17 so that they finish
    before the others."""
    rng = np.random.default_rng(5)
    out = []
    for step in range(STEPS):
        x = rng.standard_normal((R, V)).astype(np.float32) * 2
        x[:, tsb:] += rng.choice([-4.0, 0.5, 3.0], size=(R, 1)).astype(np.float32)
        for r, s0 in ((1, 10), (4, 17)):
            if r < R and step == s0:
                x[r, eot] += 30.0
        out.append(x)
    return out


def _run_greedy(R, xs, gen, mode):
    """mode "select": tw_logits_select alone; "lp": tw_token_logprob in front of it; "embed" / "lp_embed": the same
    with tw_logits_select_embed; "sample" / "sample_lp": tw_logits_sample(_lp) at temperature 0. Returns tokens,
    state, the lp buffer (NaN where never written) and, for the embed modes, the embedding outputs."""
    V, T, Dm = D.vocab, 64, 64
    p = _params(gen, max_new=STEPS)
    sb = _suppress_bits(gen.suppress_tokens, V)
    st = _fresh_state(R)
    tok = torch.zeros(R, T, dtype=torch.int32, device=DEV)
    ids = torch.zeros(R, dtype=torch.int32, device=DEV)
    pos = torch.zeros(R, dtype=torch.int32, device=DEV)
    ws = torch.empty(R, _lib.TW_SELECT_WS_PER_ROW, device=DEV)
    lp = torch.full((R, T), float("nan"), device=DEV)
    g = torch.Generator(device="cpu").manual_seed(3)
    emb = (torch.randn(V, Dm, generator=g) * 0.1).to(torch.bfloat16).to(DEV)
    pe = (torch.randn(T, Dm, generator=g) * 0.1).to(torch.bfloat16).to(DEV)
    gam, bet = torch.ones(Dm, device=DEV), torch.zeros(Dm, device=DEV)
    x_out = torch.zeros(R, Dm, device=DEV)
    ln_out = torch.zeros(R, Dm, dtype=torch.bfloat16, device=DEV)
    embeds = []
    for x in xs:
        lg = torch.from_numpy(x).to(DEV)
        if mode in ("lp", "lp_embed"):
            _lib.call("tw_token_logprob", lg.data_ptr(), R, V, sb.data_ptr(), ctypes.byref(p), st.data_ptr(),
                      lp.data_ptr(), T, S())
        if mode in ("select", "lp"):
            _lib.call("tw_logits_select", lg.data_ptr(), R, V, sb.data_ptr(), ctypes.byref(p), st.data_ptr(),
                      tok.data_ptr(), T, ids.data_ptr(), pos.data_ptr(), ws.data_ptr(), S())
        elif mode in ("embed", "lp_embed"):
            _lib.call("tw_logits_select_embed", lg.data_ptr(), R, V, sb.data_ptr(), ctypes.byref(p), st.data_ptr(),
                      tok.data_ptr(), T, ids.data_ptr(), pos.data_ptr(), ws.data_ptr(), emb.data_ptr(), pe.data_ptr(),
                      Dm, T, x_out.data_ptr(), gam.data_ptr(), bet.data_ptr(), 1e-5, ln_out.data_ptr(), 0, S())
            embeds.append((x_out.clone(), ln_out.clone()))
        elif mode == "sample":
            _lib.call("tw_logits_sample", lg.data_ptr(), R, V, sb.data_ptr(), ctypes.byref(p), 0.0, 50, 7, None,
                      st.data_ptr(), tok.data_ptr(), T, ids.data_ptr(), pos.data_ptr(), S())
        else:
            assert mode == "sample_lp", mode
            _lib.call("tw_logits_sample_lp", lg.data_ptr(), R, V, sb.data_ptr(), ctypes.byref(p), 0.0, 50, 7, None,
                      st.data_ptr(), tok.data_ptr(), T, ids.data_ptr(), pos.data_ptr(), lp.data_ptr(), T, S())
    torch.cuda.synchronize()
    return tok.cpu(), st.cpu(), lp.cpu().numpy(), embeds


@pytest.fixture(scope="module")
def greedy_ref():
    """Per R: the step logits, the tokens / state of the plain selection and the numpy log-probabilities of its
    tokens (computed once, shared by the tests below)."""
    gen, g = _gcfg()
    out = {}
    for R in (6, 1):
        xs = _step_logits(R, D.vocab, g.ts_begin, g.eot)
        tok, st, _, _ = _run_greedy(R, xs, gen, "select")
        ref = np.zeros((R, STEPS))
        n_live = []
        for r in range(R):
            hist = []
            for step in range(STEPS):
                t = int(tok[r, step])
                ref[r, step] = cr.token_logprob(xs[step][r], hist, t, g, True)
                hist.append(t)
                if t == g.eot:
                    break
            n_live.append(len(hist))
        out[R] = {"xs": xs, "tok": tok, "st": st, "ref": ref, "n_live": n_live}
    return out


@pytest.mark.parametrize("R,embed", [(6, False), (1, False), (6, True)])
def test_token_logprob_in_front_of_select(greedy_ref, R, embed):
    gen, g = _gcfg()
    z = greedy_ref[R]
    tok, st, lp, emb = _run_greedy(R, z["xs"], gen, "lp_embed" if embed else "lp")
    if embed:  # the plain reference of the fused variant: tokens, state and what it embedded
        tok0, st0, _, emb0 = _run_greedy(R, z["xs"], gen, "embed")
        assert torch.equal(tok0, z["tok"]) and torch.equal(st0, z["st"])
        for (a, b), (a0, b0) in zip(emb, emb0):
            assert torch.equal(a, a0) and torch.equal(b, b0)
    assert torch.equal(tok, z["tok"]), "the pre-kernel changed a token"
    assert torch.equal(st, z["st"]), "the pre-kernel changed the row state"
    if R == 6:
        assert z["n_live"][1] == 11 and z["n_live"][4] == 18 and max(z["n_live"]) == STEPS  # rows that finish early
    worst = 0.0
    for r in range(R):
        n = z["n_live"][r]
        d = np.abs(lp[r, :n] - z["ref"][r, :n])
        worst = max(worst, float(d.max()))
        assert np.all(lp[r, n:STEPS] == 0.0), (r, lp[r, n:STEPS])  # pads after the row finished: exactly 0.0
        assert np.all(np.isnan(lp[r, STEPS:]))  # nothing written past the generated positions
    print(f"R={R} embed={embed}: worst |lp - numpy| {worst:.2e} (bound 1e-3)")
    assert worst <= 1e-3
    # the row sums are what tw_logits_sample accumulates in TW_ST_SUMLP
    _, st_s, _, _ = _run_greedy(R, z["xs"], gen, "sample")
    sumlp = st_s[:, _lib.TW_ST_SUMLP].contiguous().view(torch.float32).numpy()
    for r in range(R):
        n = z["n_live"][r]
        assert abs(float(lp[r, :n].astype(np.float64).sum()) - float(sumlp[r])) <= 1e-3 * n, r


def test_sample_lp_greedy(greedy_ref):
    """temperature 0: tw_logits_sample_lp's tokens and state are tw_logits_sample's bit for bit (SUMLP included), its
    per-token values those of the pre-kernel's reference."""
    gen, g = _gcfg()
    z = greedy_ref[6]
    tok_s, st_s, _, _ = _run_greedy(6, z["xs"], gen, "sample")
    tok, st, lp, _ = _run_greedy(6, z["xs"], gen, "sample_lp")
    assert torch.equal(tok, tok_s) and torch.equal(st, st_s)
    assert torch.equal(tok, z["tok"])
    for r in range(6):
        n = z["n_live"][r]
        assert np.abs(lp[r, :n] - z["ref"][r, :n]).max() <= 1e-3, r
        assert np.all(lp[r, n:STEPS] == 0.0), r


def test_sample_lp_sampling_topk():
    """T = 0.7, top_k = 50, V = 2048, 256 rows of the same logits (the row key varies): lp = x[tok] - logsumexp(kept
    set) and the draws are tw_logits_sample's with the same seed and keys."""
    gen, _ = _gcfg()
    V, R, T, K = 2048, 256, 0.7, 50
    rng = np.random.default_rng(11)
    x = rng.standard_normal(V).astype(np.float32) * 1.5
    x[rng.choice(V, 80, replace=False)] += 4.0
    x[7] = x[9]
    p = _params(gen, max_new=4, use_ts=False, V=V)
    p.n_begin_suppress = 0
    lg = torch.from_numpy(np.tile(x, (R, 1))).to(DEV)
    keys = torch.arange(R, dtype=torch.int32, device=DEV)
    outs = []
    for with_lp in (False, True):
        st = _fresh_state(R)
        st[:, _lib.TW_ST_NGEN] = 1  # (not the first step: no begin-suppression)
        tok = torch.zeros(R, 8, dtype=torch.int32, device=DEV)
        ids = torch.zeros(R, dtype=torch.int32, device=DEV)
        lp = torch.full((R, 8), float("nan"), device=DEV)
        if with_lp:
            _lib.call("tw_logits_sample_lp", lg.data_ptr(), R, V, None, ctypes.byref(p), T, K, 12345, keys.data_ptr(),
                      st.data_ptr(), tok.data_ptr(), 8, ids.data_ptr(), None, lp.data_ptr(), 8, S())
        else:
            _lib.call("tw_logits_sample", lg.data_ptr(), R, V, None, ctypes.byref(p), T, K, 12345, keys.data_ptr(),
                      st.data_ptr(), tok.data_ptr(), 8, ids.data_ptr(), None, S())
        torch.cuda.synchronize()
        outs.append((ids.cpu(), st.cpu(), tok.cpu(), lp.cpu().numpy()))
    (ids0, st0, tok0, _), (ids1, st1, tok1, lp) = outs
    assert torch.equal(ids0, ids1) and torch.equal(st0, st1) and torch.equal(tok0, tok1)
    assert len(set(ids1.tolist())) > 1
    ref = np.array([cr.topk_logprob(x, int(t), K) for t in ids1.tolist()])
    np.testing.assert_allclose(lp[:, 1], ref, atol=1e-4, rtol=0)
    assert np.all(np.isnan(lp[:, 0])) and np.all(np.isnan(lp[:, 2:]))  # only position n_gen = 1 is written


# ---- beams ----------------------------------------------------------------------------------------------------------
def _synthetic_logits(history, V, tsb, eot, salt, _cache={}):
    """test_gpu_beam._synthetic_logits (deterministic in the beam's history and the window salt), memoised."""
    key = (salt,) + tuple(int(t) for t in history)
    if key not in _cache:
        rng = np.random.default_rng(hash(key) & 0xFFFFFFFF)
        x = rng.standard_normal(V).astype(np.float32) * 2.0
        x[rng.integers(0, tsb, 6)] += 7.0
        x[tsb + rng.integers(0, 60, 3)] += 6.5
        x[eot] += 5.0 + 0.4 * len(history)
        _cache[key] = x
    return _cache[key]


def _run_beam(nb, W, max_new, mode):
    """test_gpu_beam.test_beam_step_matches_oracle_core's loop. mode "off": no log-probability pointers; "sum":
    run_lp / fin_lp; "terms": also run_tlp / fin_tlp. Returns the final device arrays and the logits fed per step."""
    gen, g = _gcfg()
    st = gen.special
    V, T, R, P = D.vocab, 448, W * nb, 3
    logits = torch.empty(R, V, device=DEV)
    state = _fresh_state(R)
    tokens = torch.zeros(R, T, dtype=torch.int32, device=DEV)
    ids = torch.zeros(R, dtype=torch.int32, device=DEV)
    pos = torch.full((R,), P, dtype=torch.int32, device=DEV)
    a = {
        "run_score": torch.full((W, nb), -1e9, device=DEV), "fin_score": torch.full((R,), -1e9, device=DEV),
        "fin_flag": torch.zeros(R, dtype=torch.int32, device=DEV), "fin_len": torch.zeros(R, dtype=torch.int32, device=DEV),
        "fin_tokens": torch.zeros(R, T, dtype=torch.int32, device=DEV),
        "win": torch.tensor([[1, 0, 0, 0]] * W, dtype=torch.int32, device=DEV),
        "src_rows": torch.zeros(R, dtype=torch.int32, device=DEV),
        "kv_tab": torch.arange(R, dtype=torch.int32, device=DEV)[:, None].repeat(1, T).contiguous(),
        "fin_tab": torch.zeros(R, T, dtype=torch.int32, device=DEV),
        "run_lp": torch.zeros(R, device=DEV), "fin_lp": torch.zeros(R, device=DEV),
        "run_tlp": torch.full((R, T), float("nan"), device=DEV), "fin_tlp": torch.full((R, T), float("nan"), device=DEV),
    }
    a["run_score"][:, 0] = 0
    ws = torch.empty(int(_lib.load().tw_beam_workspace_bytes(R)), dtype=torch.uint8, device=DEV)
    sup = _suppress_bits(gen.suppress_tokens, V)
    sel = _params(gen, max_new=max_new)
    bp = _lib.TwBeamParams(nb, max_new, 1.0, T)
    ptr = lambda k, on: a[k].data_ptr() if on else None  # noqa: E731
    bst = _lib.TwBeamState(a["run_score"].data_ptr(), a["fin_score"].data_ptr(), a["fin_flag"].data_ptr(),
                           a["fin_len"].data_ptr(), a["fin_tokens"].data_ptr(), a["win"].data_ptr(),
                           a["src_rows"].data_ptr(), a["kv_tab"].data_ptr(), a["fin_tab"].data_ptr(),
                           ptr("run_lp", mode != "off"), ptr("fin_lp", mode != "off"),
                           ptr("run_tlp", mode == "terms"), ptr("fin_tlp", mode == "terms"))
    hist = [[] for _ in range(R)]
    fed = []
    steps = 0
    while steps < max_new:
        host = np.stack([_synthetic_logits(hist[r], V, st.timestamp_begin, st.eot, r // nb) for r in range(R)])
        fed.append(host)
        logits.copy_(torch.from_numpy(host))
        _lib.call("tw_beam_step", logits.data_ptr(), W, V, sup.data_ptr(), ctypes.byref(sel), ctypes.byref(bp),
                  ctypes.byref(bst), state.data_ptr(), tokens.data_ptr(), ids.data_ptr(), pos.data_ptr(),
                  ws.data_ptr(), S())
        steps += 1
        tk = tokens.cpu().numpy()
        hist = [list(tk[r, :steps]) for r in range(R)]
        if bool(a["win"][:, 1].all().item()):
            break
    torch.cuda.synchronize()
    out = {k: v.cpu() for k, v in a.items()}
    out.update(tokens=tokens.cpu(), state=state.cpu(), ids=ids.cpu(), pos=pos.cpu(), steps=steps)
    return out, fed, P


@pytest.mark.parametrize("nb,W", [(2, 1), (2, 3), (5, 1), (5, 3)])
def test_beam_step_token_logprobs(nb, W):
    gen, g = _gcfg()
    max_new = 24
    off, _, _ = _run_beam(nb, W, max_new, "off")
    summ, _, _ = _run_beam(nb, W, max_new, "sum")
    on, fed, P = _run_beam(nb, W, max_new, "terms")
    same = ["run_score", "fin_score", "fin_flag", "fin_len", "fin_tokens", "win", "src_rows", "kv_tab", "fin_tab",
            "tokens", "state", "ids", "pos"]
    for k in same:  # decisions, tokens and scores: those of the runs with the pointers null
        assert torch.equal(on[k], off[k]), k
        assert torch.equal(on[k], summ[k]), k
    assert on["steps"] == off["steps"]
    for k in ("run_lp", "fin_lp"):
        assert torch.equal(on[k], summ[k]), k
    checked = 0
    worst = 0.0
    for row in range(W * nb):
        if not int(on["fin_flag"][row]):
            continue
        n = int(on["fin_len"][row])
        h = on["fin_tokens"][row, :n].tolist()
        terms = on["fin_tlp"][row, :n].numpy().astype(np.float64)
        assert np.all(np.isfinite(terms)), (row, terms)
        assert abs(terms.sum() - float(on["fin_lp"][row])) <= 1e-4 * n, (row, terms.sum(), float(on["fin_lp"][row]))
        for q in range(n):  # the step-q logits of the row that fed it (the hypothesis' lineage), processed on the host
            src = int(on["fin_tab"][row, P + q])
            assert src // nb == row // nb
            x = fed[q][src]
            lsm = (x.astype(np.float64) - cr.logsumexp(x)).astype(np.float32)  # (beam search scores log-probabilities)
            ref = cr.token_logprob(lsm, h[:q], h[q], g, True)
            worst = max(worst, abs(ref - terms[q]))
        checked += 1
    # a running beam's history sums to its run_lp too (the histories moved with the beams)
    t = on["steps"]
    for row in range(W * nb):
        if float(on["run_score"].view(-1)[row]) > -1e8:
            terms = on["run_tlp"][row, :t].numpy().astype(np.float64)
            assert abs(terms.sum() - float(on["run_lp"][row])) <= 1e-4 * t, row
    print(f"nb={nb} W={W}: {checked} finished hypotheses, worst |term - host| {worst:.2e} (bound 1e-3)")
    assert checked >= W
    assert worst <= 1e-3


# ---- the engine vs transformers -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return json.load(open(os.path.join(G, "confidence.json")))


@pytest.fixture(scope="module")
def mini():
    return TurboTranscriber.from_pretrained("test-mini", seed=1234, max_batch=4)


CLIPS = {"speech30": lambda: speech_like(30.0, 1234), "noise12": lambda: white_noise(12.3, 7),
         "zeros30": lambda: silence(30.0), "speech45": lambda: speech_like(45.0, 99),
         "noise20": lambda: white_noise(20.0, 3)}


def _load3(tr, names=("speech30", "noise12", "zeros30")):
    """The named clips' first 30 s into the engine's first three windows (make_golden_confidence.py's features)."""
    eng = tr.engine
    clips = [CLIPS[k]() for k in names]
    assert len(clips) == 3
    host = np.zeros((3, 480000), np.float32)
    for i, c in enumerate(clips):
        host[i, : len(c)] = c[:480000]
    eng.wave[:3].copy_(torch.from_numpy(host))
    eng.logmel(3)


def _compare_engine(tr, case, tol_token, tol_mean, fallback=None):
    """generate(token_logprobs=True) on the golden's clips: every seek pass of every window has transformers' tokens,
    position for position, and its per-token log-probabilities within tol_token (pass mean within tol_mean).
    Returns the worst per-token difference."""
    eng = tr.engine
    st = tr.gen.special
    _load3(tr, case["clips"])
    kw = dict(case["kwargs"])
    kw = dict(task="transcribe", max_new_tokens=40, return_timestamps=kw.pop("return_timestamps"), **kw)
    plain = eng.generate(3, **kw, **({"fallback": fallback} if fallback else {}))
    assert eng.last_pass_logprobs is None and eng.last_token_logprobs is None
    plain_passes = [[list(p) for p in w] for w in eng.last_passes]
    _load3(tr, case["clips"])
    seqs = eng.generate(3, **kw, token_logprobs=True, **({"fallback": fallback} if fallback else {}))
    assert seqs == plain and eng.last_passes == plain_passes  # the option changes no token
    passes, lps = eng.last_passes, eng.last_pass_logprobs
    for i in range(3):
        assert len(eng.last_token_logprobs[i]) == len(seqs[i])
        assert [len(p) for p in passes[i]] == [len(p) for p in lps[i]]
    n_pass = [0, 0, 0]
    worst = 0.0
    for p in case["passes"]:
        for row, call in zip(p["rows"], p["calls"]):
            k = n_pass[row]
            n_pass[row] += 1
            assert k < len(passes[row]), (case["name"], row, k, "missing pass")
            raw, lp = list(passes[row][k]), list(lps[row][k])
            ref_t, ref_lp = list(call["tokens"]), np.asarray(call["logprobs"])
            if fallback and ref_t[-1] == st.eot:  # (the fallback loop keeps a pass without its EOS)
                ref_t, ref_lp = ref_t[:-1], ref_lp[:-1]
            n = len(ref_t)
            got_t = raw[:n]
            assert got_t == ref_t, (case["name"], row, k, got_t, ref_t)
            assert all(t == st.eot for t in raw[n:]) and (fallback or all(x == 0.0 for x in lp[n:])), (row, k)
            d = np.abs(np.asarray(lp[:n]) - ref_lp)
            worst = max(worst, float(d.max()))
            assert d.max() <= tol_token, (case["name"], row, k, int(d.argmax()), float(d.max()))
            assert abs(np.mean(lp[:n]) - ref_lp.mean()) <= tol_mean, (case["name"], row, k)
    assert n_pass == [len(p) for p in passes], (n_pass, [len(p) for p in passes])
    print(f"{case['name']}{' (fallback loop)' if fallback else ''}: worst per-token |d| vs transformers {worst:.4f} "
          f"(bound {tol_token})")
    return worst


@pytest.mark.parametrize("name", ["greedy_ts", "greedy_no_ts", "greedy_ts_rp1.3"])
def test_engine_token_logprobs_vs_transformers(mini, gold, name):
    """The captured greedy path (tw_token_logprob inside the step graph)."""
    case = next(c for c in gold["cases"] if c["name"] == name)
    _compare_engine(mini, case, 0.30, 0.03)


def test_engine_fallback_loop_token_logprobs_vs_transformers(mini, gold):
    """The eager fallback loop at its only temperature 0 (tw_logits_sample_lp), thresholds inert as the golden's."""
    case = next(c for c in gold["cases"] if c["name"] == "greedy_ts")
    fb = FallbackConfig(temperatures=(0.0,), compression_ratio_threshold=1e9, logprob_threshold=-1e9)
    _compare_engine(mini, case, 0.30, 0.03, fallback=fb)


def test_engine_fp32_token_logprobs_vs_transformers(gold):
    tr = TurboTranscriber.from_pretrained("test-mini", seed=1234, max_batch=4, precision="fp32")
    try:
        for name in ("greedy_ts", "greedy_ts_rp1.3"):
            case = next(c for c in gold["cases"] if c["name"] == name)
            _compare_engine(tr, case, 1e-3, 1e-3)
    finally:
        tr.close()


def test_engine_fused_decode_and_prompt(mini):
    """The persistent fused decode (rows <= 4) and a prompted, conditioned call keep their tokens with the option on
    and return one finite log-probability per kept token."""
    eng = mini.engine
    base = dict(task="transcribe", max_new_tokens=24, return_timestamps=True)
    cond = dict(base, condition_on_prev_tokens=True, prompt_ids=[mini.gen.special.startofprev, 1000, 1001])
    for fused, kw in ((True, base), (False, cond)):
        eng.dec_fused_alone = fused
        try:
            _load3(mini)
            a = eng.generate(3, **kw)
            _load3(mini)
            b = eng.generate(3, **kw, token_logprobs=True)
        finally:
            eng.dec_fused_alone = False
        assert a == b
        for i in range(3):
            lp = np.asarray(eng.last_token_logprobs[i])
            assert len(lp) == len(b[i]) and np.all(np.isfinite(lp)) and np.all(lp <= 0.0)


# ---- the callable ---------------------------------------------------------------------------------------------------
def _options_audio():
    return np.concatenate([speech_like(40.0, 5), white_noise(35.0, 11)]).astype(np.float32)


def _strip(out, key):
    return {"text": out["text"], "chunks": [{k: v for k, v in c.items() if k != key} for c in out["chunks"]]}


@pytest.mark.parametrize("num_beams", [1, 3])
def test_callable_word_probabilities(mini, num_beams):
    audio = _options_audio()
    kw = dict(chunk_length_s=30, batch_size=2, return_timestamps="word",
              generate_kwargs={"task": "transcribe", "num_beams": num_beams, "max_new_tokens": 24})
    off = mini(audio.copy(), **kw)
    on = mini(audio.copy(), **kw, return_confidence=True)
    assert all("probability" not in c for c in off["chunks"])
    assert _strip(on, "probability") == off
    probs = [c["probability"] for c in on["chunks"]]
    assert probs and all(0.0 < p <= 1.0 for p in probs)
    # the CPU functions over the passes' recorded values: each window's kept tokens and their log-probabilities from
    # last_window_passes / last_window_pass_logprobs, stitched on the host
    st = mini.gen.special
    passes, plps = mini.last_window_passes, mini.last_window_pass_logprobs
    assert len(passes) == len(plps) == len(mini.last_window_token_logprobs)
    sr = mini.sampling_rate
    outputs = []
    for i, w in enumerate(chunk_windows(len(audio), 30, None, sr)):
        seek, toks, lps = 0, [], []
        for raw, lp in zip(passes[i], plps[i]):
            assert len(raw) == len(lp)
            seg, adv = retrieve_segment(strip_generated(raw, st.eot), seek, min(3000 - seek, 3000), st.timestamp_begin)
            toks += seg
            lps += list(lp[: len(seg)])
            seek += adv
        assert lps == list(mini.last_window_token_logprobs[i])
        outputs.append({"tokens": toks, "token_timestamps": mini.last_window_token_timestamps[i], "token_logprobs": lps,
                        "stride": (w.length / sr, w.stride_left / sr, w.stride_right / sr)})
    text, opt = decode_asr(mini.vocab, outputs, return_timestamps="word", confidence=True,
                           time_precision=time_precision(mini.engine.d.max_source_positions))
    assert text == on["text"] and opt["chunks"] == on["chunks"]


def test_callable_segment_and_plain_avg_logprob(mini):
    audio = _options_audio()
    gk = {"task": "transcribe", "num_beams": 1, "max_new_tokens": 24}
    off = mini(audio.copy(), chunk_length_s=30, batch_size=2, return_timestamps=True, generate_kwargs=gk)
    on = mini(audio.copy(), chunk_length_s=30, batch_size=2, return_timestamps=True, generate_kwargs=gk,
              return_confidence=True)
    assert _strip(on, "avg_logprob") == off
    assert all(c["avg_logprob"] is None or c["avg_logprob"] <= 0.0 for c in on["chunks"])
    assert any(c["avg_logprob"] is not None for c in on["chunks"])
    off = mini(audio.copy(), chunk_length_s=30, batch_size=2, generate_kwargs=gk)
    on = mini(audio.copy(), chunk_length_s=30, batch_size=2, generate_kwargs=gk, return_confidence=True)
    assert on["text"] == off["text"] and set(on) - set(off) == {"avg_logprob"}
    assert on["avg_logprob"] is not None and on["avg_logprob"] <= 0.0


def test_callable_long_form_conditioned(mini):
    audio = _options_audio()
    kw = dict(return_timestamps="word", generate_kwargs={"task": "transcribe", "num_beams": 1, "max_new_tokens": 40,
                                                         "condition_on_prev_tokens": True})
    off = mini(audio.copy(), **kw)
    on = mini(audio.copy(), **kw, return_confidence=True)
    assert _strip(on, "probability") == off
    assert on["chunks"] and all(0.0 < c["probability"] <= 1.0 for c in on["chunks"])
    assert len(mini.last_window_pass_logprobs[0]) == len(mini.last_window_passes[0])
