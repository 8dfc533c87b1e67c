"""Confidence on the host (CPU): the auxiliary per-token sequence through find_longest_common_sequence and AsrStitcher
(state and sharded stitching included), word probability / avg_logprob on hand-built token lists, the ctypes tables of
the new exports, and the golden's own consistency."""
import json
import math
import os
import socket

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

import confidence_ref as cr
from twamd import _lib
from twamd import dist as twd
from twamd.config import SpecialTokens
from twamd.tokenizer import (AsrStitcher, WhisperVocab, bytes_to_unicode, collate_word_timestamps, decode_asr,
                             find_longest_common_sequence, mean_logprob, word_probabilities)

G = os.path.join(os.path.dirname(__file__), "golden")
ST = SpecialTokens.for_vocab(51866)
VOCAB = WhisperVocab.synthetic(ST)
BYTE_ID = {b: i for i, b in enumerate(bytes_to_unicode())}  # synthetic vocab: ids < 256 are the byte symbols


def _lp_of(tokens, salt=0):
    """A distinct, reproducible negative float per (window, position)."""
    return [-0.01 * (1 + (7 * k + 13 * salt + t) % 97) - 1e-4 * k for k, t in enumerate(tokens)]


# ---- LCS with an auxiliary sequence ---------------------------------------------------------------------------------
def _random_runs(rng):
    V = int(rng.choice([2, 4, 16, 50000]))
    seqs = [[int(x) for x in rng.integers(0, V, rng.integers(0, 40))] for _ in range(int(rng.integers(2, 5)))]
    if len(seqs[0]) > 4 and rng.random() < 0.5:
        seqs[1] = seqs[0][-int(rng.integers(1, len(seqs[0]))):] + seqs[1]
    return seqs


def test_lcs_aux_is_cut_where_the_tokens_are():
    rng = np.random.default_rng(11)
    for _ in range(600):
        seqs = _random_runs(rng)
        aux = [[(i, k) for k in range(len(s))] for i, s in enumerate(seqs)]  # every entry names its origin
        want = find_longest_common_sequence(seqs)
        got, ts, got_aux = find_longest_common_sequence(seqs, None, aux)
        assert got == want and ts == []
        assert [seqs[i][k] for i, k in got_aux] == want
        # the same (lmid, rmid) as the independent restatement of the scan
        exp, start = [], 0
        cuts = cr.lcs_cut_points(seqs)
        for i, s in enumerate(seqs):
            end = cuts[i][0] + start if i < len(cuts) else len(s)
            exp += [(i, k) for k in range(start, end)]
            start = cuts[i][1] if i < len(cuts) else 0
        assert got_aux == exp, seqs


def test_lcs_aux_with_token_timestamps():
    rng = np.random.default_rng(5)
    for _ in range(300):
        seqs = _random_runs(rng)
        tss = [[(round(0.1 * k, 2), round(0.1 * k + 0.1, 2)) for k in range(len(s))] for s in seqs]
        aux = [[(i, k) for k in range(len(s))] for i, s in enumerate(seqs)]
        if not tss[0]:  # (an empty first run switches the timestamp scan off: no timestamps come back)
            continue
        want_t, want_ts = find_longest_common_sequence(seqs, tss)
        got_t, got_ts, got_aux = find_longest_common_sequence(seqs, tss, aux)
        assert (got_t, got_ts) == (want_t, want_ts)
        assert [seqs[i][k] for i, k in got_aux] == want_t
        assert [tss[i][k] for i, k in got_aux] == want_ts


def test_lcs_tie_where_a_widened_tuple_would_change_the_merge():
    """Overlapping tokens with equal (start, end) times: the match rule left <= right holds. Had the log-probability
    been appended to the tuples, left (s, e, -0.1) <= right (s, e, -0.9) would fail, the overlap would go unmatched
    and both copies would be kept."""
    left, right = [10, 11, 12, 13], [12, 13, 14, 15]
    lts = [(0.0, 0.5), (0.5, 1.0), (1.0, 1.5), (1.5, 2.0)]
    rts = [(1.0, 1.5), (1.5, 2.0), (2.0, 2.5), (2.5, 3.0)]
    llp, rlp = [-0.1, -0.1, -0.1, -0.1], [-0.9, -0.9, -0.9, -0.9]
    plain = find_longest_common_sequence([left, right], [lts, rts])
    toks, ts, lps = find_longest_common_sequence([left, right], [lts, rts], [llp, rlp])
    assert (toks, ts) == plain and toks == [10, 11, 12, 13, 14, 15]
    assert lps == [-0.1, -0.1, -0.1, -0.9, -0.9, -0.9]  # cut at lmid = 3 / rmid = 1
    widened = find_longest_common_sequence([left, right], [[t + (p,) for t, p in zip(lts, llp)],
                                                           [t + (p,) for t, p in zip(rts, rlp)]])
    assert widened[0] == left + right  # what carrying the value inside the tuples would have produced


# ---- word probability and avg_logprob -------------------------------------------------------------------------------
def test_word_probability_on_hand_built_tokens():
    """" ka" + "la" (one word of two tokens), "," (merged onto it), " ma" + the two bytes of "é" (a unicode character
    split over two tokens joins its word), " oa" + "." + "!" (two appended marks)."""
    b = BYTE_ID
    toks = [256, 257, b[ord(",")], 258, b[0xC3], b[0xA9], 260, b[ord(".")], b[ord("!")]]
    lps = [-0.1, -0.3, -2.0, -0.5, -0.7, -0.2, -1.1, -0.05, -3.0]
    tts = [(0.1 * k, 0.1 * k + 0.1) for k in range(len(toks))]
    words = collate_word_timestamps(VOCAB, toks, tts, "english", False, lps)
    plain = collate_word_timestamps(VOCAB, toks, tts, "english", False)
    assert [{k: v for k, v in w.items() if k != "probability"} for w in words] == plain
    text = [w["text"] for w in words]
    assert text == [VOCAB.decode(toks[0:3]), VOCAB.decode(toks[3:6]), VOCAB.decode(toks[6:9])], text
    assert text[0].endswith(",") and text[1].endswith("é") and text[2].endswith(".!")
    groups = [[0, 1, 2], [3, 4, 5], [6, 7, 8]]
    want = [sum(math.exp(lps[k]) for k in ix) / len(ix) for ix in groups]
    assert [w["probability"] for w in words] == pytest.approx(want, rel=1e-12)
    assert word_probabilities(groups, lps) == pytest.approx(cr.word_probabilities(groups, lps), rel=1e-12)
    assert all(0.0 < w["probability"] <= 1.0 for w in words)
    # the arithmetic mean of the probabilities, not exp of the mean log-probability
    assert words[0]["probability"] != pytest.approx(math.exp(sum(lps[:3]) / 3), rel=1e-3)


def _ts(t):
    return ST.timestamp_begin + int(round(t / 0.02))


def test_chunk_and_plain_avg_logprob():
    toks = [_ts(0.0), 256, 257, _ts(1.0), _ts(1.0), 258, _ts(2.0), _ts(2.0), _ts(3.0)]
    lps = [-0.4, -0.1, -0.3, -0.2, -0.6, -0.5, -0.9, -0.8, -0.7]
    out = {"tokens": toks, "token_logprobs": lps}
    off_text, off = decode_asr(VOCAB, [{"tokens": toks}], return_timestamps=True)
    text, opt = decode_asr(VOCAB, [out], return_timestamps=True, confidence=True)
    assert text == off_text
    assert [{k: v for k, v in c.items() if k != "avg_logprob"} for c in opt["chunks"]] == off["chunks"]
    # timestamps carry no text: only the text tokens' values are averaged; an empty chunk has none
    assert [c["avg_logprob"] for c in opt["chunks"]] == [pytest.approx((-0.1 - 0.3) / 2), pytest.approx(-0.5), None]
    assert mean_logprob([]) is None and cr.mean_logprob([]) is None
    text2, opt2 = decode_asr(VOCAB, [out], return_timestamps=False, confidence=True)
    assert text2 == decode_asr(VOCAB, [{"tokens": toks}], return_timestamps=False)[0]
    assert opt2 == {"avg_logprob": pytest.approx((-0.1 - 0.3 - 0.5) / 3)}


def test_decode_asr_cases_unchanged_with_confidence():
    """Every decode_asr.json case (transformers' own stitching of strided windows): with log-probabilities riding
    along, text, timestamps and chunk boundaries are those of the case; the values that come out are the kept
    tokens' own."""
    cases = json.load(open(os.path.join(G, "decode_asr.json")))
    for c in cases:
        outs = [{"tokens": o["tokens"], "stride": tuple(o["stride"]), "token_logprobs": _lp_of(o["tokens"], j)}
                for j, o in enumerate(c["outputs"])]
        text, opt = decode_asr(VOCAB, outs, return_timestamps=c["return_timestamps"],
                               return_language=c["return_language"], confidence=True)
        assert text == c["text"]
        got = json.loads(json.dumps(opt))
        key = "avg_logprob"
        if c["return_timestamps"]:
            assert all(key in ch for ch in got["chunks"])
            got["chunks"] = [{k: v for k, v in ch.items() if k != key} for ch in got["chunks"]]
        else:
            v = got.pop(key)
            assert v is None or v <= 0.0
        assert got == c["optional"]


# ---- stitcher state and sharded stitching ---------------------------------------------------------------------------
def _windows(n, word=False, seed=0):
    """n strided windows whose segments stay open across the window boundary (pending runs for the LCS)."""
    rng = np.random.default_rng(seed)
    outs = []
    prev_tail = []
    for w in range(n):
        body = [int(x) for x in 256 + 2 * rng.integers(0, 200, 6)]
        toks = [_ts(0.0)] + prev_tail + body + ([_ts(20.0), _ts(20.0)] if w % 3 == 2 else [])
        toks += [int(x) for x in 256 + 2 * rng.integers(0, 200, 3)] if w % 3 == 2 else []
        prev_tail = toks[-3:] if toks[-1] < ST.timestamp_begin else []
        o = {"tokens": toks, "stride": (30.0, 0.0 if w == 0 else 5.0, 0.0 if w == n - 1 else 5.0),
             "token_logprobs": _lp_of(toks, w)}
        if word:
            o["token_timestamps"] = [round(0.3 * (k + 1), 2) for k in range(len(toks))]
        outs.append(o)
    return outs


@pytest.mark.parametrize("rt", [True, "word"])
def test_stitcher_state_round_trip_with_pending_aux(rt):
    outs = _windows(5, word=rt == "word", seed=3)
    want = decode_asr(VOCAB, outs, return_timestamps=rt, confidence=True)
    for cut in range(1, len(outs)):
        a = AsrStitcher(VOCAB, rt, confidence=True)
        for o in outs[:cut]:
            a.feed(o)
        st = json.loads(json.dumps(a.state()))  # (a state travels between ranks: plain data)
        if cut == 1:
            assert st["previous_tokens"] and st["previous_token_aux"], "nothing pending: the case shows nothing"
            assert [len(x) for x in st["previous_token_aux"]] == [len(x) for x in st["previous_tokens"]]
        st["previous_token_timestamps"] = [[tuple(x) for x in t] for t in st["previous_token_timestamps"]]
        b = AsrStitcher(VOCAB, rt, state=st, confidence=True)
        b.chunks = list(a.chunks)
        for o in outs[cut:]:
            b.feed(o)
        assert b.finish() == want
    # a stitcher without the option keeps the old state format
    assert "previous_token_aux" not in AsrStitcher(VOCAB, rt).state()
    assert "previous_token_aux" not in AsrStitcher.initial_state()


@pytest.mark.parametrize("rt", [True, "word", False])
def test_sharded_pieces_equal_serial(rt):
    from test_host_logic import _sharded_stitch

    outs = _windows(7, word=rt == "word", seed=9)
    want = decode_asr(VOCAB, outs, return_timestamps=rt, confidence=True)
    plain = decode_asr(VOCAB, [{k: v for k, v in o.items() if k != "token_logprobs"} for o in outs],
                       return_timestamps=rt)
    assert want[0] == plain[0]
    for n in range(1, 8):
        assert _sharded_stitch(VOCAB, outs, n, return_timestamps=rt, confidence=True) == want


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _lane_windows(wav, windows):
    """(tokens, times, log-probabilities) per window: the word + confidence lanes of the callable."""
    from test_dist import fake_timed_windows
    return [(t, ts, _lp_of(t, len(t))) for t, ts in fake_timed_windows(wav, windows)]


def _worker(rank, ws, port, q):
    from twamd.frontend import chunk_windows
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=ws)
    try:
        wav = np.random.default_rng(3).standard_normal(200 * 16000).astype(np.float32)
        windows = list(chunk_windows(len(wav), 30, 5, 16000))
        lanes = twd.transcribe_sharded(_lane_windows, wav, windows, timed=2)
        outs = _windows(7, word=True, seed=9)
        stitched = twd.stitch_sharded(VOCAB, outs, return_timestamps="word", confidence=True)
        q.put((rank, lanes, stitched, twd.merge_pieces.last_restitched))
    finally:
        dist.destroy_process_group()


def test_two_rank_lanes_and_sharded_stitch_equal_serial():
    """A gloo world of two: the float lanes (times and log-probabilities) arrive bit-exact in window order, and
    stitch_sharded with confidence equals the serial decode_asr."""
    from twamd.frontend import chunk_windows
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    wav = np.random.default_rng(3).standard_normal(200 * 16000).astype(np.float32)
    windows = list(chunk_windows(len(wav), 30, 5, 16000))
    ref = []
    for r in range(2):  # (each rank's stand-in numbers its windows from 0)
        lo, hi = twd.shard_range(len(windows), 2, r)
        ref += [(t, ts, [float(np.float32(x)) for x in lp]) for t, ts, lp in _lane_windows(wav, windows[lo:hi])]
    want = decode_asr(VOCAB, _windows(7, word=True, seed=9), return_timestamps="word", confidence=True)
    for rank, lanes, stitched, restitched in res:
        assert lanes == ref
        assert stitched == want


# ---- the C-ABI tables -----------------------------------------------------------------------------------------------
def test_new_exports_and_struct_members_are_declared():
    for name in ("tw_token_logprob", "tw_logits_sample_lp"):
        assert name in _lib.EXPORTED and name in _lib._SIGS
    # tw_logits_sample_lp = tw_logits_sample + (float* token_lp, int ld_lp) in front of the stream
    a, b = _lib._SIGS["tw_logits_sample"][0], _lib._SIGS["tw_logits_sample_lp"][0]
    assert b[:len(a) - 1] == a[:-1] and len(b) == len(a) + 2 and b[-1] == a[-1]
    fields = [f for f, _ in _lib.TwBeamState._fields_]
    assert fields[-4:] == ["run_lp", "fin_lp", "run_tlp", "fin_tlp"]
    import ctypes
    assert ctypes.sizeof(_lib.TwBeamParams) == 20
    old = _lib.TwBeamState(1, 2, 3, 4, 5, 6, 7)  # an existing positional construction: the new members are off
    assert old.run_tlp is None and old.fin_tlp is None
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "tw_whisper.h")).read()
    for name in ("tw_token_logprob", "tw_logits_sample_lp", "run_tlp", "fin_tlp"):
        assert name in header


def test_built_library_exports_the_new_entry_points():
    lib = _lib.load()
    assert lib.tw_token_logprob and lib.tw_logits_sample_lp


# ---- the golden -----------------------------------------------------------------------------------------------------
def test_golden_terms_are_consistent():
    z = json.load(open(os.path.join(G, "confidence.json")))
    assert [c["name"] for c in z["cases"]] == ["greedy_ts", "greedy_no_ts", "greedy_ts_rp1.3"]
    for c in z["cases"]:
        assert len(c["clips"]) == len(c["sequences"])
        for p in c["passes"]:
            assert len(p["calls"]) == len(p["rows"])
            for call in p["calls"]:
                assert len(call["tokens"]) == len(call["logprobs"]) <= z["max_new_tokens"]
                assert all(x <= 0.0 and math.isfinite(x) for x in call["logprobs"])
