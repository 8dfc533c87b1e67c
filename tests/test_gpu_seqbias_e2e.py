"""sequence_bias / bad_words_ids end to end on the GPU against transformers (tests/golden/seqbias.json, written by
tests/golden/make_golden_seqbias.py).

The golden is transformers in float32, so the cases are pinned with the fp32 engine (precision="fp32"): every generate
case token for token, every seek pass included, and the pipeline cases' output and passes (the callable refuses
bad_words_ids, as tests/test_gpu_penalties.py pins: there the forbidden sequences are -inf sequence_bias entries, and
the golden's own kwargs go through transcribe_windows and the engine's generate()). The bf16 engine is not
pinned to the golden here (whether it ranks a near-tie of this random-weight model as float32 does is a property of
the clip, not of the feature: tests/test_gpu_penalties.py carries the tolerance machinery for that); it is held to
itself instead: two tables in succession through captured graphs against fresh engines, and the plain call after a
biased one against a fresh engine's."""
import json
import os

import numpy as np
import pytest
import torch

from twamd.config import PRESETS
from twamd.pipeline import TurboTranscriber
from twamd.synth_audio import silence, speech_like, white_noise

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
D = PRESETS["test-mini"]


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(G, "seqbias.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def tr32(gold):
    t = TurboTranscriber.from_pretrained("test-mini", seed=1234, max_batch=3, max_beams=3, precision="fp32")
    t.engine.gen.prev_sot_token_id = gold["generate"]["prompt_ids"][0]  # (the golden's prev_sot_token_id)
    yield t
    t.close()


def _load3(t):
    host = np.zeros((3, 480000), np.float32)
    for i, c in enumerate([speech_like(30.0, 1234), white_noise(12.3, 7), silence(30.0)]):
        host[i, : len(c)] = c[:480000]
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
    return raw[: raw.index(eot)] if eot in raw else raw


def _passes_equal(name, device_passes, gold_passes, eot):
    """Every golden seek pass (rows: the windows in the pass's batch) equals the device's pass of that window, up to
    the first EOS; no device pass is left over."""
    n_pass = [0] * len(device_passes)
    for p in gold_passes:
        for row, ref in zip(p["rows"], p["sequences"]):
            k = n_pass[row]
            n_pass[row] += 1
            assert k < len(device_passes[row]), (name, row, k, "missing pass")
            assert _cut(device_passes[row][k], eot) == _cut(ref, eot), (name, row, k)
    assert n_pass == [len(p) for p in device_passes], (name, "extra pass")


GEN_CASES = ["greedy_sb", "greedy_bw", "greedy_sb_bw_rp_ngram2", "greedy_prompt_sb_bw_rp_ngram2", "beam3_sb_bw"]


@pytest.mark.parametrize("name", GEN_CASES)
def test_fp32_engine_matches_transformers(tr32, gold, name):
    case = next(c for c in gold["generate"]["cases"] if c["name"] == name)
    eng, st = tr32.engine, tr32.gen.special
    _load3(tr32)
    shared, opts = case["shared"], dict(case["options"])
    kw = dict(task="transcribe", max_new_tokens=shared["max_new_tokens"], return_timestamps=shared["return_timestamps"],
              num_beams=shared.get("num_beams", 1))
    if shared.get("prompt"):
        kw["prompt_ids"] = gold["generate"]["prompt_ids"]
    seqs = eng.generate(3, **kw, **opts)
    passes = [list(p) for p in eng.last_passes]
    assert [list(s) for s in seqs] == [_strip(ref, st.eot) for ref in case["sequences"]], name
    _passes_equal(name, passes, case["passes"], st.eot)
    plain = eng.generate(3, **kw)
    assert [list(s) for s in plain] == [_strip(ref, st.eot) for ref in case["plain"]["sequences"]], name
    assert plain != seqs


def test_fallback_average_logprob_under_sequence_bias(tr32, gold):
    """sample_pass at temperature 0 with the golden's sequence_bias: the tokens are transformers' and every window's
    average log-probability is within tests/test_gpu_penalties.py's bound (0.03) of the one _need_fallback saw, which
    itself is further than that from the unbiased golden on some window (the sum comes from the biased scores)."""
    eng, st = tr32.engine, tr32.gen.special
    _load3(tr32)
    eng.row_map[:3] = torch.arange(3, dtype=torch.int32)
    eng.seek[:3] = 0
    eng.encode(3)
    tail = eng.prompt_tail("transcribe", True)
    fb = gold["fallback"]
    res = eng.sample_pass(3, tail, None, fb["max_new_tokens"], temperature=0.0, no_speech_token=st.notimestamps - 1,
                          sequence_bias=fb["sequence_bias"])
    moved = 0
    for i, c in enumerate(fb["calls"][:3]):
        assert c["index"] == i
        toks = [int(t) for t in res.tokens[i]]
        k = toks.index(st.eot) + 1 if st.eot in toks else len(toks)
        assert _cut(toks, st.eot) == _strip(c["tokens"], st.eot), i  # (the fallback loop keeps a pass without its EOS)
        avg = res.sum_logprob[i] / k
        print(f"window {i}: avg logprob {avg:.4f}, transformers {c['avg_logprob']:.4f} "
              f"(unbiased golden {fb['plain_calls'][i]['avg_logprob']:.4f})")
        assert abs(avg - c["avg_logprob"]) < 0.03, (i, avg, c["avg_logprob"])
        moved += abs(c["avg_logprob"] - fb["plain_calls"][i]["avg_logprob"]) > 0.03
    assert moved >= 1


def _through_the_callable(options):
    """The case's options as the callable takes them: it refuses bad_words_ids (tests/test_gpu_penalties.py pins
    that), so the forbidden sequences go in as sequence_bias entries of -inf, which give the same scores bit for bit
    (tests/test_seqbias_processors.py::test_minus_inf_bias_forbids_like_a_bad_word)."""
    d = {tuple(ids): float(b) for ids, b in options.get("sequence_bias", [])}
    d.update({tuple(w): float("-inf") for w in options.get("bad_words_ids", [])})
    return {"sequence_bias": d}


def test_window_path_with_both_options_matches_transformers(tr32, gold):
    """The reference call's windows (chunk 60 s, stride 5 s) through transcribe_windows with the golden's
    sequence_bias and bad_words_ids as transformers took them: every seek pass of every window is transformers'."""
    from twamd.frontend import chunk_windows

    case = next(c for c in gold["pipeline"]["cases"] if c["name"] == "ref_call_greedy_sb_bw")
    x, gk, kw = _audio(), case["generate_kwargs"], case["kwargs"]
    wins = list(chunk_windows(len(x), kw["chunk_length_s"], kw["stride_length_s"], 16000))
    tr32.transcribe_windows(x, wins, task=gk["task"], lang_id=None, return_timestamps=True,
                            max_new_tokens=gk["max_new_tokens"], num_beams=gk["num_beams"],
                            history=json.loads(json.dumps(case["options"])))
    _passes_equal(case["name"], [[list(q) for q in p] for p in tr32.last_window_passes], case["passes"],
                  tr32.gen.special.eot)


def test_long_form_conditioned_with_bad_words_matches_transformers(tr32, gold):
    """The unchunked 75-s input, condition_on_prev_tokens and bad_words_ids through the engine's generate(): every
    seek pass is transformers'."""
    case = next(c for c in gold["pipeline"]["cases"] if c["name"] == "long_cond_bw")
    eng, gk = tr32.engine, case["generate_kwargs"]
    eng.set_long_input(torch.from_numpy(_audio()))
    try:
        eng.generate(1, task=gk["task"], max_new_tokens=gk["max_new_tokens"], return_timestamps=True,
                     num_beams=gk["num_beams"], condition_on_prev_tokens=True,
                     bad_words_ids=case["options"]["bad_words_ids"])
    finally:
        eng.set_long_input(None)
    _passes_equal(case["name"], [[list(q) for q in p] for p in eng.last_passes], case["passes"], tr32.gen.special.eot)


@pytest.mark.parametrize("name", ["ref_call_greedy_sb_bw", "long_cond_bw"])
def test_pipeline_matches_transformers(tr32, gold, name):
    case = next(c for c in gold["pipeline"]["cases"] if c["name"] == name)
    st = tr32.gen.special
    x = _audio()
    gk, kw = case["generate_kwargs"], case["kwargs"]
    opts = _through_the_callable(case["options"])
    r = tr32(x.copy(), generate_kwargs=dict(gk, **opts), return_timestamps=True, **kw)
    assert json.loads(json.dumps(r)) == case["output"], name
    biased = [[list(q) for q in p] for p in tr32.last_window_passes]
    _passes_equal(name, biased, case["passes"], st.eot)
    plain = tr32(x.copy(), generate_kwargs=dict(gk), return_timestamps=True, **kw)
    assert json.loads(json.dumps(plain)) == case["plain"]["output"] and plain != r, name
    assert [[list(q) for q in p] for p in tr32.last_window_passes] != biased


def test_token_logprobs_come_from_the_biased_scores(tr32, gold):
    """token_logprobs with sequence_bias: the tokens are those of the call without token_logprobs, and their terms
    differ from the plain call's where the tokens agree but a bias acts (the 1-token entries act on every step)."""
    case = next(c for c in gold["generate"]["cases"] if c["name"] == "greedy_sb")
    eng = tr32.engine
    _load3(tr32)
    kw = dict(task="transcribe", max_new_tokens=40, return_timestamps=True)
    seqs = eng.generate(3, **kw, **case["options"])
    with_lp = eng.generate(3, **kw, **case["options"], token_logprobs=True)
    lp = [list(v) for v in eng.last_token_logprobs]
    assert with_lp == seqs and [len(v) for v in lp] == [len(s) for s in seqs]
    eng.generate(3, **kw, token_logprobs=True)
    assert lp != [list(v) for v in eng.last_token_logprobs]
    assert all(v <= 1e-6 for row in lp for v in row)


def test_graphs_are_keyed_by_the_table_and_plain_calls_stay_plain(gold):
    """One bf16 engine with use_graphs: table A, table B (other entry counts), table A' (A's counts, other contents),
    then no option, greedy and with beams. Every call equals a fresh engine's, so a captured graph replayed with
    another call's counts, or table buffers still holding another call's entries, would show; and the plain call after
    the biased ones equals a fresh engine's plain output."""
    a = dict(next(c for c in gold["generate"]["cases"] if c["name"] == "greedy_sb_bw_rp_ngram2")["options"])
    a.pop("repetition_penalty"), a.pop("no_repeat_ngram_size")
    b = {"bad_words_ids": a["bad_words_ids"][:1]}
    a2 = {"sequence_bias": [[ids, -bias] for ids, bias in a["sequence_bias"]], "bad_words_ids": a["bad_words_ids"]}
    calls = [a, b, a2, {}]

    def run(t, opts, nb):
        return t.engine.generate(3, task="transcribe", max_new_tokens=24, return_timestamps=True, num_beams=nb,
                                 **json.loads(json.dumps(opts)))

    used = TurboTranscriber.from_pretrained("test-mini", seed=1234, max_batch=3, max_beams=3, use_graphs=True)
    _load3(used)
    got = {(i, nb): run(used, opts, nb) for nb in (1, 3) for i, opts in enumerate(calls)}
    again = run(used, a, 1)  # (replays A's graphs after the buffers held B and A')
    used.close()
    assert again == got[(0, 1)]
    for nb in (1, 3):  # (the tables act, and differently)
        assert got[(0, nb)] != got[(3, nb)] and got[(1, nb)] != got[(3, nb)] and got[(0, nb)] != got[(2, nb)]
    for i, opts in enumerate(calls):
        if i == 0:  # (table A ran first: the used engine was fresh then)
            continue
        fresh = TurboTranscriber.from_pretrained("test-mini", seed=1234, max_batch=3, max_beams=3, use_graphs=True)
        _load3(fresh)
        for nb in (1, 3):
            assert run(fresh, opts, nb) == got[(i, nb)], (i, nb)
        fresh.close()


def test_kwargs_are_checked_before_any_work(tr32):
    x = np.zeros(16000, np.float32)
    with pytest.raises(ValueError, match="`bad_words_ids` has to be a non-empty list"):
        tr32.engine.generate(1, bad_words_ids=[])
    with pytest.raises(ValueError, match="The model vocabulary size is"):
        tr32(x, generate_kwargs={"sequence_bias": {(D.vocab,): 1.0}})
    with pytest.raises(ValueError, match="at most 16 per entry"):
        tr32.engine.generate(1, bad_words_ids=[list(range(1, 18))])
    with pytest.raises(ValueError, match="generate_kwargs not supported"):
        tr32(x, generate_kwargs={"top_p": 0.9, "bad_words_ids": [[5]]})
