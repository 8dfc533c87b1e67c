"""Token alternatives on the host (CPU): the float64 restatement (tests/alternatives_ref.py) on hand-built rows, the
option's bounds, the alternatives riding through the stitching of every decode_asr.json case, a stitcher state with
pending alternatives through JSON, and the two new C-ABI symbols."""
import json
import os

import numpy as np
import pytest

import alternatives_ref as ar
import confidence_ref as cr
from oracle import whisper_oracle as wo
from twamd import _lib
from twamd.config import PRESETS, GenerationSettings, SpecialTokens
from twamd.engine import DecodeOptions
from twamd.tokenizer import AsrStitcher, WhisperVocab, decode_asr, render_alternatives

G = os.path.join(os.path.dirname(__file__), "golden")
ST = SpecialTokens.for_vocab(51866)
VOCAB = WhisperVocab.synthetic(ST)
D = PRESETS["test-mini"]


def _gcfg():
    gen = GenerationSettings.default(D)
    st = gen.special
    return wo.GenCfg(D.vocab, st.eot, st.sot, st.lang_begin, st.n_languages, st.transcribe, st.translate,
                     st.notimestamps, gen.suppress_tokens, gen.begin_suppress_tokens)


# ---- the restatement ------------------------------------------------------------------------------------------------
def test_ref_fewer_than_k_eligible():
    s = np.full(100, -np.inf, np.float32)
    s[[7, 50, 3]] = [1.0, 2.0, 0.5]
    ids, lps = ar.rank(s, 8)
    assert ids == [50, 7, 3]
    assert lps == pytest.approx([x - cr.logsumexp(s) for x in (2.0, 1.0, 0.5)])
    assert np.exp(lps).sum() == pytest.approx(1.0)
    assert ar.rank(np.full(10, -np.inf, np.float32), 3) == ([], [])


def test_ref_exact_ties_go_to_the_lower_id():
    s = np.zeros(1000, np.float32)
    s[[900, 17, 400]] = 5.0
    s[5] = 6.0
    ids, lps = ar.rank(s, 5)
    assert ids == [5, 17, 400, 900, 0]
    assert lps[1] == lps[2] == lps[3] > lps[4]


def test_ref_rule_fires_and_does_not():
    g = _gcfg()
    V, tb = D.vocab, g.ts_begin
    rng = np.random.default_rng(0)
    x = rng.standard_normal(V).astype(np.float32)
    hist = [tb + 3, 300]  # (a text token after a timestamp: text and later timestamps are allowed)
    lo = x.copy()
    lo[tb:] -= 20.0
    ids, lps, margin = ar.step_alternatives(lo, hist, g, True, 8)
    assert margin < 0 and all(i < tb for i in ids), "the rule must not fire: text candidates"
    hi = x.copy()
    hi[tb:] += 20.0
    ids, lps, margin = ar.step_alternatives(hi, hist, g, True, 8)
    assert margin > 0 and all(i > tb + 3 for i in ids), "the rule fires: timestamps past the last one only"
    s = wo.process_logits(hi, hist, g, True)
    assert lps[0] == pytest.approx(float(s[ids[0]]) - cr.logsumexp(s[tb:]))
    assert lps == sorted(lps, reverse=True) and len(set(ids)) == 8
    # slot 0 is the greedy choice, its lp the per-token log-probability
    assert ids[0] == int(np.argmax(s)) and lps[0] == pytest.approx(cr.token_logprob(hi, hist, ids[0], g, True))
    # raw: log_softmax of the row
    ids, lps = ar.raw_alternatives(x, 3)
    assert ids[0] == int(np.argmax(x)) and lps[0] == pytest.approx(float(x[ids[0]]) - cr.logsumexp(x))


# ---- the option -----------------------------------------------------------------------------------------------------
def test_decode_options_bounds():
    off = DecodeOptions.make()
    assert off.top_alternatives == 0 and DecodeOptions.make(top_alternatives=0) == off
    assert DecodeOptions.make(top_alternatives=None) == off
    for k in (1, 8):
        o = DecodeOptions.make(top_alternatives=k)
        assert o.top_alternatives == k and o.graph_key != off.graph_key and o.hist_key == off.hist_key
        assert not o.history
    assert DecodeOptions.make(top_alternatives=3).graph_key != DecodeOptions.make(top_alternatives=4).graph_key
    assert (DecodeOptions.make(top_alternatives=1).graph_key != DecodeOptions.make(token_logprobs=True).graph_key)
    for bad in (-1, 9, 100):
        with pytest.raises(ValueError):
            DecodeOptions.make(top_alternatives=bad)
    assert _lib.TW_TOPK_MAX == 8


# ---- stitching ------------------------------------------------------------------------------------------------------
K = 3


def _fab(tokens):
    return [[[int(t) + j, float(-j)] for j in range(K)] for t in tokens]


def _word_outputs(case, alt, conf=False):
    outs = []
    for o in case["outputs"]:
        toks = list(o["tokens"])
        d = {"tokens": toks, "stride": tuple(o["stride"]),
             "token_timestamps": [round(0.3 * (k + 1), 2) for k in range(len(toks))]}
        if alt:
            d["token_alternatives"] = _fab(toks)
        if conf:
            d["token_logprobs"] = [-0.01 * (1 + k % 50) for k in range(len(toks))]
        outs.append(d)
    return outs


def _split_words(chunks):
    """(chunks without "alternatives", per word the first id of each of its lists)."""
    plain, firsts = [], []
    for c in chunks:
        alts = c["alternatives"]
        for lst in alts:
            assert [a["id"] for a in lst] == [lst[0]["id"] + j for j in range(K)]
            assert [a["logprob"] for a in lst] == [float(-j) for j in range(K)]
        firsts.append([lst[0]["id"] for lst in alts])
        plain.append({k: v for k, v in c.items() if k != "alternatives"})
    return plain, firsts


def _resolved_words(case):
    """Per word its token ids, from the stitching without alternatives (collate's own split of the resolved tokens)."""
    from twamd import tokenizer as tk
    words = []
    real = tk.collate_word_timestamps

    def spy(vocab, tokens, ts, language, return_language, lps=None, alts=None):
        out = real(vocab, tokens, ts, language, return_language, lps, alts)
        lang = language or "english"
        split = (tk._split_tokens_on_unicode if lang in {"chinese", "japanese", "thai", "lao", "myanmar", "cantonese"}
                 else tk._split_tokens_on_spaces)
        w, wt, ix = split(vocab, tokens)
        tk._merge_punctuations(w, wt, ix)
        words.extend([[tokens[k] for k in i] for i in ix])
        return out

    tk.collate_word_timestamps = spy
    try:
        res = decode_asr(VOCAB, _word_outputs(case, False), return_timestamps="word",
                         return_language=case["return_language"])
    finally:
        tk.collate_word_timestamps = real
    return res, words


@pytest.mark.parametrize("conf", [False, True])
def test_decode_asr_cases_word_mode_with_alternatives(conf):
    """Every decode_asr.json case in word mode: text and timestamps are those of the same outputs without
    alternatives, and every word's lists begin with exactly that word's token ids, in order — the payload stays
    aligned through stride cuts and LCS merges (alone, and beside the log-probabilities)."""
    cases = json.load(open(os.path.join(G, "decode_asr.json")))
    n_words = 0
    for c in cases:
        (text0, opt0), words = _resolved_words(c)
        text, opt = decode_asr(VOCAB, _word_outputs(c, True, conf), return_timestamps="word",
                               return_language=c["return_language"], alternatives=True, confidence=conf)
        assert text == text0
        plain, firsts = _split_words(opt["chunks"])
        if conf:
            want = decode_asr(VOCAB, _word_outputs(c, False, True), return_timestamps="word",
                              return_language=c["return_language"], confidence=True)[1]["chunks"]
            assert plain == want
            plain = [{k: v for k, v in w.items() if k != "probability"} for w in plain]
        assert plain == opt0.get("chunks", [])
        assert firsts == words
        assert all("alternatives" not in w for w in opt0.get("chunks", []))
        n_words += len(words)
    assert n_words > 100


def test_stitcher_state_with_pending_alternatives_round_trips_json():
    from test_confidence import _windows
    outs = _windows(5, word=True, seed=3)
    for o in outs:
        o["token_alternatives"] = [[(t + j, float(-j)) for j in range(K)] for t in o["tokens"]]  # (tuples, as the engine's)
    for conf in (False, True):
        want = decode_asr(VOCAB, outs, return_timestamps="word", alternatives=True, confidence=conf)
        for cut in range(1, len(outs)):
            a = AsrStitcher(VOCAB, "word", alternatives=True, confidence=conf)
            for o in outs[:cut]:
                a.feed(o)
            state = a.state()
            st = json.loads(json.dumps(state))
            assert {k: v for k, v in st.items() if k != "previous_token_timestamps"} == \
                {k: v for k, v in state.items() if k != "previous_token_timestamps"}, "lists only: JSON changes nothing"
            if cut == 1:
                assert st["previous_tokens"] and st["previous_token_aux"], "nothing pending: the case shows nothing"
                assert [len(x) for x in st["previous_token_aux"]] == [len(x) for x in st["previous_tokens"]]
            st["previous_token_timestamps"] = [[tuple(x) for x in t] for t in st["previous_token_timestamps"]]
            b = AsrStitcher(VOCAB, "word", state=st, alternatives=True, confidence=conf)
            b.chunks = list(a.chunks)
            for o in outs[cut:]:
                b.feed(o)
            assert b.finish() == want
    assert "previous_token_aux" not in AsrStitcher(VOCAB, "word").state()


def test_render_alternatives():
    tb = ST.timestamp_begin
    out = render_alternatives(VOCAB, [[300, -0.5], [ST.eot, -1.0], [tb + 5, -2.0]])
    assert [d["id"] for d in out] == [300, ST.eot, tb + 5] and [d["logprob"] for d in out] == [-0.5, -1.0, -2.0]
    assert out[0]["text"] == VOCAB.decode([300])
    assert out[1]["text"] == VOCAB.id_to_token[ST.eot] and out[2]["text"] == VOCAB.id_to_token[tb + 5]


# ---- the C-ABI ------------------------------------------------------------------------------------------------------
def test_header_lib_and_library_declare_the_symbols():
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "tw_whisper.h")).read()
    assert "#define TW_TOPK_MAX 8" in header
    lib = _lib.load()
    for name in ("tw_token_topk", "tw_token_topk_workspace_bytes"):
        assert name in header and name in _lib.EXPORTED and name in _lib._SIGS
        assert getattr(lib, name)
    # tw_token_logprob's leading arguments, then (k, ids, lps, ld, workspace, stream)
    a, b = _lib._SIGS["tw_token_logprob"][0], _lib._SIGS["tw_token_topk"][0]
    assert b[:6] == a[:6] and len(b) == 12
    per_row = int(lib.tw_token_topk_workspace_bytes(1))
    assert per_row > 0 and int(lib.tw_token_topk_workspace_bytes(7)) == 7 * per_row


def test_sharded_pieces_equal_serial_with_alternatives():
    """twamd.dist's shard-wise stitching with alternatives riding along: the merge of the ranks' pieces (each piece
    through JSON, as it travels) is the serial decode_asr, and a shard that starts clean is not stitched twice."""
    from test_confidence import _windows
    from twamd import dist as twd
    outs = _windows(7, word=True, seed=5)
    for o in outs:
        o["token_alternatives"] = _fab(o["tokens"])
    kw = dict(return_timestamps="word", alternatives=True)
    want = decode_asr(VOCAB, outs, **kw)
    assert any("alternatives" in w for w in want[1]["chunks"])
    for ws in (2, 3):
        bounds = [twd.shard_range(len(outs), ws, r) for r in range(ws)]
        pieces = [json.loads(json.dumps(twd.shard_piece(VOCAB, outs, lo, hi, **kw))) for lo, hi in bounds]
        for p in pieces:  # (JSON turns the pending (start, end) tuples into lists; the stitcher compares tuples)
            for st in (p[0], p[2]):
                st["previous_token_timestamps"] = [[tuple(x) for x in t] for t in st["previous_token_timestamps"]]
            for c in p[1]:
                c["timestamp"] = list(c["timestamp"])
                for w in c.get("words", []):
                    w["timestamp"] = tuple(w["timestamp"])
        assert twd.merge_pieces(VOCAB, outs, pieces, bounds, **kw) == want
        assert twd.merge_pieces.last_restitched < ws
