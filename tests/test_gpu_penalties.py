"""repetition_penalty / no_repeat_ngram_size / length_penalty end to end on the GPU against transformers
(tests/golden/penalties.json, written by tests/golden/make_golden_penalties.py).

Every case is token-exact, or — the bf16 engine ranks a near-tie of this random-weight model the other way — its
decisions are within the project's tolerance on the fp32 oracle's scores after the restated processors
(tests/history_ref.py): TAU = 0.3 logits for greedy passes (wo.decision_ok along the device's own passes), the rule of
test_gpu_e2e._beam_passes_within_tau for beam passes. So that the tolerance branch cannot hide a no-op, every case also
checks that the device output differs from the device's own output without the option (where transformers' does), and
that with no_repeat_ngram_size = n no pass generates an n-gram its history already holds."""
import contextlib
import functools
import json
import os
import types

import numpy as np
import pytest
import torch

import history_ref as hr
from oracle import whisper_oracle as wo
from twamd import _lib
from twamd.config import PRESETS, GenerationSettings
from twamd.pipeline import TurboTranscriber
from twamd.synth_audio import silence, speech_like, white_noise

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
D = PRESETS["test-mini"]
TAU = 0.3
BRANCH = {"exact": 0, "tolerance": 0}


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(G, "penalties.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def tr(gold):
    t = TurboTranscriber.from_pretrained("test-mini", seed=1234, max_batch=4, max_beams=5)
    t.engine.gen.prev_sot_token_id = gold["generate"]["prompt_ids"][0]  # (the golden's prev_sot_token_id)
    return t


@pytest.fixture(scope="module")
def oracle():
    sd = wo.synth_state_dict(D.d_model, D.encoder_layers, D.decoder_layers, D.ffn, D.n_mels, D.vocab, 1234)
    return wo.WhisperOracle(sd, D.heads)


def _gcfg():
    gen = GenerationSettings.default(D)
    st = gen.special
    return wo.GenCfg(D.vocab, st.eot, st.sot, st.lang_begin, st.n_languages, st.transcribe, st.translate,
                     st.notimestamps, gen.suppress_tokens, gen.begin_suppress_tokens)


def _clips():
    host = np.zeros((3, 480000), np.float32)
    for i, c in enumerate([speech_like(30.0, 1234), white_noise(12.3, 7), silence(30.0)]):
        host[i, : len(c)] = c[:480000]
    return host


def _load3(t):
    host = _clips()
    t.engine.wave[:3].copy_(torch.from_numpy(host))
    t.engine.logmel(3)
    return host


def _audio():
    return np.concatenate([speech_like(40.0, 5), white_noise(35.0, 11)]).astype(np.float32)


def _strip(seq, eot):
    seq = [int(t) for t in seq]
    while seq and seq[-1] == eot:
        seq.pop()
    return seq


def _cut(raw, eot):
    raw = [int(t) for t in raw]
    return raw[: raw.index(eot) + 1] if eot in raw else raw


def _pass_history(prefix, prompt):
    """What transformers hands the processors before a pass's first token: the fed prefix row (pads included) + the
    init tokens."""
    return ([int(t) for t in prefix[0]] if prefix is not None else []) + list(prompt)


def _no_repeated_ngram(history, generated, n):
    """No n-gram that ends on a generated token (up to the first EOT) occurs earlier in history + generated."""
    h = list(history) + list(generated)
    seen = {tuple(h[i: i + n]) for i in range(max(0, len(history) - n + 1))}
    for j in range(len(history), len(h)):
        if j + 1 < n:
            continue
        ng = tuple(h[j + 1 - n: j + 1])
        if ng in seen:
            return False
        seen.add(ng)
    return True


@contextlib.contextmanager
def _oracle_with_history(history, p, n, length_penalty=1.0):
    """The frozen oracle's processor chain with the restated history processors in front, for one pass whose
    decoder_input_ids were `history` (the chain's `sampled` argument is what the pass generated), and its beam pass at
    `length_penalty`."""
    no_rule, proc, beam = wo.process_logits_no_rule, wo.process_logits, wo.beam_pass

    def hist(scores, sampled):
        return hr.history_processors(np.asarray(scores, np.float32), list(history) + [int(t) for t in sampled], p, n)

    def proc2(scores, sampled, g, use_ts):  # (with timestamps the original goes through process_logits_no_rule)
        return proc(scores, sampled, g, use_ts) if use_ts else proc(hist(scores, sampled), sampled, g, use_ts)

    wo.process_logits_no_rule = lambda scores, sampled, g: no_rule(hist(scores, sampled), sampled, g)
    wo.process_logits = proc2
    wo.beam_pass = functools.partial(beam, length_penalty=length_penalty)
    try:
        yield
    finally:
        wo.process_logits_no_rule, wo.process_logits, wo.beam_pass = no_rule, proc, beam


def _replay_greedy(oracle, feats, max_frames, passes, lang, prefixes, use_ts, max_new, p, n):
    """wo.replay_generate's walk over one window's device passes, with the history processors in the oracle's chain:
    every device decision must be the fp32 argmax or within TAU of it (wo.decision_ok)."""
    g = _gcfg()
    prompt = [g.sot, int(lang), g.transcribe] + ([] if use_ts else [g.notimestamps])
    stats = {"ok": True, "decisions": 0, "exact": 0, "first_bad": None}
    seek = 0
    for k, raw in enumerate(passes):
        assert seek < max_frames, ("extra pass", k)
        pf = prefixes[k] if prefixes is not None and k < len(prefixes) else None
        toks_p, pads = (list(pf[0][pf[1]:]), int(pf[1])) if pf is not None else ([], 0)
        cache = oracle.new_cache(oracle.encode(wo.segment_input(feats, seek, max_frames)), pos0=pads)
        for t in toks_p + prompt[:-1]:
            oracle.decoder_step(int(t), cache)
        logits = oracle.decoder_step(prompt[-1], cache)
        out = []
        with _oracle_with_history(_pass_history(pf, prompt), p, n):
            for tok in raw:
                tok = int(tok)
                stats["decisions"] += 1
                if int(np.argmax(wo.process_logits(logits, out, g, use_ts))) == tok:
                    stats["exact"] += 1
                elif not wo.decision_ok(logits, out, g, use_ts, tok, TAU) and stats["first_bad"] is None:
                    stats["ok"], stats["first_bad"] = False, (k, len(out), tok, out[-5:])
                out.append(tok)
                if tok == g.eot or len(out) >= max_new:
                    break
                logits = oracle.decoder_step(tok, cache)
        seq = out[:-1] if out and out[-1] == g.eot else out
        _, off = wo.retrieve_segment(seq, min(max_frames - seek, 3000), g.ts_begin)
        seek += off
    assert seek >= max_frames, ("missing pass", seek)
    return stats


def _beam_window_within_tau(oracle, audio, lang, passes, use_ts, max_new, nb, p, n, lp):
    """test_gpu_e2e._beam_passes_within_tau for one window (no conditioning: every pass starts from the init tokens)."""
    from test_gpu_e2e import _beam_passes_within_tau

    g = _gcfg()
    prompt = [g.sot, int(lang), g.transcribe] + ([] if use_ts else [g.notimestamps])
    shim = types.SimpleNamespace(last_window_langs=[lang], last_window_passes=[passes])
    with _oracle_with_history(prompt, p, n, lp):
        return _beam_passes_within_tau(shim, oracle, audio, {}, "transcribe", max_new, num_beams=nb, use_ts=use_ts)


def _took(branch, what):
    BRANCH[branch] += 1
    print(f"{what}: {branch}; cases so far: {BRANCH['exact']} exact, {BRANCH['tolerance']} on the tolerance branch")


GEN_CASES = ["greedy_rp", "greedy_ngram2", "greedy_rp_ngram3", "greedy_rp_ngram3_no_ts", "greedy_prompt_rp_ngram2",
             "beam3_rp_ngram2", "beam3_lp0.5", "beam3_lp2.0"]


def _generate_case(t, oracle, gold, name):
    case = next(c for c in gold["generate"]["cases"] if c["name"] == name)
    eng, st = t.engine, t.gen.special
    host = _load3(t)
    shared, opts = case["shared"], case["options"]
    use_ts, max_new, nb = shared["return_timestamps"], shared["max_new_tokens"], shared.get("num_beams", 1)
    kw = dict(task="transcribe", max_new_tokens=max_new, return_timestamps=use_ts, num_beams=nb)
    if shared.get("prompt"):
        kw["prompt_ids"] = gold["generate"]["prompt_ids"]
    plain = eng.generate(3, **kw)
    seqs = eng.generate(3, **kw, **opts)
    passes, langs, prefixes = list(eng.last_passes), list(eng.last_langs), list(eng.last_pass_prefixes)
    if case["differs_from_plain"]:
        assert seqs != plain, f"{name}: the option changed nothing on the device"
    p, n, lp = opts.get("repetition_penalty", 1.0), opts.get("no_repeat_ngram_size", 0), opts.get("length_penalty", 1.0)
    for i in range(3):
        prompt = [st.sot, int(langs[i]), st.transcribe] + ([] if use_ts else [st.notimestamps])
        for k, raw in enumerate(passes[i]):
            if n:
                assert _no_repeated_ngram(_pass_history(prefixes[i][k], prompt), _cut(raw, st.eot), n), (name, i, k)
    exact = all(list(got) == _strip(ref, st.eot) for got, ref in zip(seqs, case["sequences"]))
    if exact:
        _took("exact", name)
        return
    for i in range(3):
        if nb > 1:
            _beam_window_within_tau(oracle, host[i], langs[i], passes[i], use_ts, max_new, nb, p, n, lp)
        else:
            stt = _replay_greedy(oracle, wo.log_mel(host[i], D.n_mels), 3000, passes[i], langs[i], prefixes[i], use_ts,
                                 max_new, p, n)
            print(f"{name} clip {i}: {stt}")
            assert stt["ok"], (name, i, stt)
    _took("tolerance", name)


@pytest.mark.parametrize("name", GEN_CASES)
def test_generate_matches_transformers(tr, oracle, gold, name):
    _generate_case(tr, oracle, gold, name)


def test_fp32_engine_greedy_penalties(oracle, gold):
    """precision="fp32", greedy, repetition_penalty=1.3 with no_repeat_ngram_size=3: the engine runs fp32 like the
    golden, so the tolerance branch is reported if taken."""
    t = TurboTranscriber.from_pretrained("test-mini", seed=1234, max_batch=3, precision="fp32")
    t.engine.gen.prev_sot_token_id = gold["generate"]["prompt_ids"][0]
    before = BRANCH["tolerance"]
    _generate_case(t, oracle, gold, "greedy_rp_ngram3")
    print("fp32 engine took the tolerance branch:", BRANCH["tolerance"] > before)
    t.close()


def _oracle_avg_logprob(oracle, wav, lang, toks, p, n):
    """The fp32 oracle's average log-probability of `toks` (a first seek pass, timestamps on) under the processed
    scores after the restated history processors — what _retrieve_avg_logprobs takes from generate()'s scores — and
    the same without them, from one teacher-forced walk."""
    g = _gcfg()
    prompt = [g.sot, int(lang), g.transcribe]
    cache = oracle.new_cache(oracle.encode(wo.segment_input(wo.log_mel(wav, D.n_mels), 0, 3000)))
    for t in prompt[:-1]:
        oracle.decoder_step(t, cache)
    logits = oracle.decoder_step(prompt[-1], cache)

    def logprob(s, tok):
        fin = s[np.isfinite(s)].astype(np.float64)
        return float(s[tok]) - (fin.max() + np.log(np.exp(fin - fin.max()).sum()))

    with_p, without, out = 0.0, 0.0, []
    for tok in toks:
        without += logprob(wo.process_logits(logits, out, g, True), tok)
        with _oracle_with_history(prompt, p, n):
            with_p += logprob(wo.process_logits(logits, out, g, True), tok)
        out.append(int(tok))
        if len(out) < len(toks):
            logits = oracle.decoder_step(int(tok), cache)
    return with_p / len(toks), without / len(toks)


def test_fallback_criteria_under_repetition_penalty(tr, oracle, gold):
    """sample_pass at temperature 0 with repetition_penalty=1.3. Every window's average log-probability is within
    test_gpu_fallback.py's bound (0.03) of the fp32 oracle's for the device's own tokens after the restated processors,
    and further than that from the oracle's for the same tokens without the penalty, so a sum taken from the
    unpenalised row fails. Windows whose tokens equal transformers' are also held to the average _need_fallback saw
    (at least one is), which itself is further than the bound from the unpenalised golden."""
    eng, st = tr.engine, tr.gen.special
    host = _load3(tr)
    eng.row_map[:3] = torch.arange(3, dtype=torch.int32)
    eng.seek[:3] = 0
    eng.encode(3)
    tail = eng.prompt_tail("transcribe", True)
    fb = gold["fallback"]
    pen = fb["repetition_penalty"]
    res = eng.sample_pass(3, tail, None, 40, temperature=0.0, no_speech_token=st.notimestamps - 1,
                          repetition_penalty=pen)
    plain = eng.sample_pass(3, tail, None, 40, temperature=0.0, no_speech_token=st.notimestamps - 1)
    assert res.tokens != plain.tokens
    compared = 0
    for i, c in enumerate(fb["calls"][:3]):
        toks = [int(t) for t in res.tokens[i]]
        k = toks.index(st.eot) + 1 if st.eot in toks else len(toks)
        avg = res.sum_logprob[i] / k
        ora, ora_plain = _oracle_avg_logprob(oracle, host[i], res.lang_ids[i], toks[:k], pen, 0)
        print(f"window {i}: tokens equal {toks[:k] == c['tokens']}, avg logprob {avg:.4f}, fp32 oracle {ora:.4f} "
              f"(unpenalised {ora_plain:.4f}), transformers {c['avg_logprob']:.4f} "
              f"(unpenalised golden {fb['plain_calls'][i]['avg_logprob']:.4f}), no-speech {res.no_speech_prob[i]:.3e}")
        assert abs(avg - ora) < 0.03, (i, avg, ora)
        assert abs(avg - ora_plain) > 0.03, (i, avg, ora_plain)
        assert abs(c["avg_logprob"] - fb["plain_calls"][i]["avg_logprob"]) > 0.03
        if toks[:k] == c["tokens"]:
            assert abs(avg - c["avg_logprob"]) < 0.03
            compared += 1
        assert abs(res.no_speech_prob[i] - c["no_speech_prob"]) <= 0.1 * c["no_speech_prob"]  # (raw logits: untouched)
    assert compared >= 1, "no window's tokens equal transformers': the recorded averages were not compared"


def test_length_penalty_reaches_the_beam_kernel(monkeypatch):
    """generate_kwargs' length_penalty arrives in every tw_beam_step's TwBeamParams, whichever way the call goes:
    chunked windows (run_batches), an unchunked long-form input, the temperature fallback's beam round, and
    engine.generate; unset, the kernel gets 1.0. (No exponent from -4 to 8 changes transformers' output on the fixture
    clips, so the goldens cannot show the option; tests/test_gpu_history.py shows the kernel honours the exponent.)"""
    t = TurboTranscriber.from_pretrained("test-mini", seed=1234, max_batch=3, max_beams=3, use_graphs=False)
    seen = []
    call = _lib.call

    def spy(name, *args):
        if name == "tw_beam_step":
            seen.append(float(args[5]._obj.length_penalty))
        return call(name, *args)

    monkeypatch.setattr(_lib, "call", spy)
    x = _audio()[: 16000 * 45]
    gk = {"task": "transcribe", "num_beams": 3, "max_new_tokens": 6}
    routes = {"chunked": dict(chunk_length_s=30, stride_length_s=0, batch_size=3), "long-form": {}}
    for lp, want in ((0.5, 0.5), (None, 1.0)):
        opt = {} if lp is None else {"length_penalty": lp}
        for name, kw in routes.items():
            seen.clear()
            t(x.copy(), generate_kwargs=dict(gk, **opt), return_timestamps=True, **kw)
            assert seen and all(v == want for v in seen), (name, lp, seen[:4])
        seen.clear()
        t(x.copy(), generate_kwargs=dict(gk, temperature=(0.0,), logprob_threshold=-1e9, **opt), return_timestamps=True,
          chunk_length_s=30, stride_length_s=0, batch_size=3)
        assert seen and all(v == want for v in seen), ("fallback", lp, seen[:4])
        seen.clear()
        _load3(t)
        t.engine.generate(3, task="transcribe", max_new_tokens=6, num_beams=3, **opt)
        assert seen and all(v == want for v in seen), ("generate", lp, seen[:4])
    t.close()


PIPE_CASES = ["ref_call_greedy", "ref_call_as_shipped", "long_cond_ngram3"]


@pytest.mark.parametrize("name", PIPE_CASES)
def test_pipeline_matches_transformers(tr, oracle, gold, name):
    from twamd.frontend import chunk_windows

    case = next(c for c in gold["pipeline"]["cases"] if c["name"] == name)
    st = tr.gen.special
    x = _audio()
    gk, opts, kw = case["generate_kwargs"], case["options"], case["kwargs"]
    r = tr(x.copy(), generate_kwargs=dict(gk, **opts), return_timestamps=True, **kw)
    got = json.loads(json.dumps(r))
    passes, langs = list(tr.last_window_passes), list(tr.last_window_langs)
    prefixes = [list(pf) for pf in tr.last_window_prefixes]
    plain = json.loads(json.dumps(tr(x.copy(), generate_kwargs=dict(gk), return_timestamps=True, **kw)))
    assert got != plain, f"{name}: the options changed nothing on the device"
    p, n = opts.get("repetition_penalty", 1.0), opts.get("no_repeat_ngram_size", 0)
    for i in range(len(passes)):
        prompt = [st.sot, int(langs[i]), st.transcribe]
        for k, raw in enumerate(passes[i]):
            assert _no_repeated_ngram(_pass_history(prefixes[i][k], prompt), _cut(raw, st.eot), n), (name, i, k)
    if got == case["output"]:
        _took("exact", name)
        return
    print(f"{name}: differs from transformers' (near-tie): {r['text'][:70]!r}")
    nb = gk.get("num_beams", 5)
    if kw.get("chunk_length_s"):
        wins = [x[w.start: w.start + min(w.length, 480000)]
                for w in chunk_windows(len(x), kw["chunk_length_s"], kw.get("stride_length_s"), 16000)]
    else:
        wins = [x]
    for i, wav in enumerate(wins):
        if nb > 1:
            _beam_window_within_tau(oracle, wav, langs[i], passes[i], True, gk["max_new_tokens"], nb, p, n, 1.0)
            continue
        f = wo.log_mel(wav, D.n_mels, long=not kw.get("chunk_length_s"))
        stt = _replay_greedy(oracle, f, 3000 if kw.get("chunk_length_s") else f.shape[1], passes[i], langs[i],
                             prefixes[i], True, gk["max_new_tokens"], p, n)
        print(f"{name} window {i}: {stt}")
        assert stt["ok"], (name, i, stt)
    _took("tolerance", name)


def test_unsupported_kwargs_still_raise(tr):
    for key, val in (("top_p", 0.9), ("num_return_sequences", 2), ("encoder_repetition_penalty", 1.2),
                     ("bad_words_ids", [[5]])):
        with pytest.raises(ValueError, match="generate_kwargs not supported"):
            tr(np.zeros(16000, np.float32), generate_kwargs={key: val})


def test_graphs_are_keyed_by_the_options():
    """One engine, first with then without the options: the second call equals a fresh engine's plain output bit for
    bit (a captured prompt / step / beam graph that baked the pre-pass in, reused for the plain call, would not)."""
    outs = {}
    for who in ("used", "fresh"):
        t = TurboTranscriber.from_pretrained("test-mini", seed=1234, max_batch=3, max_beams=3)
        _load3(t)
        eng = t.engine
        res = []
        for nb in (1, 3):
            kw = dict(task="transcribe", max_new_tokens=24, return_timestamps=True, num_beams=nb)
            if who == "used":
                with_opts = eng.generate(3, **kw, repetition_penalty=1.3, no_repeat_ngram_size=2)
            res.append(eng.generate(3, **kw))
            if who == "used":
                assert with_opts != res[-1]
                assert eng.generate(3, **kw, repetition_penalty=1.3, no_repeat_ngram_size=2) == with_opts
        outs[who] = res
        t.close()
    assert outs["used"] == outs["fresh"]
