"""Forced alignment, host side (no GPU): the cost-matrix reference of tests/align_ref.py against the matrix
oracle/whisper_oracle.py's token_timestamps hands its DTW, TurboTranscriber.align's argument checks and result
assembly over a stub engine, and the two new C-ABI entries in the header and the built library."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import align_ref as ar
from oracle import whisper_oracle as wo
from twamd import _lib, alignment
from twamd.config import PRESETS, GenerationSettings
from twamd.engine import PassResult, WhisperEngine
from twamd.pipeline import TurboTranscriber
from twamd.tokenizer import WhisperVocab

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = PRESETS["test-mini"]
SR = 16000


def _peaked(rng, heads, rows, frames):
    """Attention-like weights: every token a bump that moves along the frames, plus noise; rows sum to one."""
    f = np.arange(frames)[None, None, :]
    centre = (np.arange(rows)[None, :, None] + 0.5) * frames / rows + rng.normal(0, 2, (heads, rows, 1))
    w = np.exp(-0.5 * ((f - centre) / max(2.0, frames / rows / 2)) ** 2) + 0.05 * rng.random((heads, rows, frames))
    return (w / w.sum(-1, keepdims=True)).astype(np.float32)


def _oracle_matrix(monkeypatch, w, P, num_frames, width=7):
    """The matrix wo.token_timestamps builds and hands to its DTW."""
    seen = []
    real = wo.dynamic_time_warping

    def spy(m):
        seen.append(np.array(m))
        return real(m)

    monkeypatch.setattr(wo, "dynamic_time_warping", spy)
    ts = wo.token_timestamps(w, P, num_frames, width)
    monkeypatch.setattr(wo, "dynamic_time_warping", real)
    return seen[0], ts


@pytest.mark.parametrize("heads,rows,num_frames,P", [(4, 9, 3000, 3), (1, 2, 1227, 0), (6, 5, 14, 2), (3, 4, 6, 1),
                                                     (2, 3, 2, 0)])
def test_cost_reference_is_the_oracles_matrix(monkeypatch, heads, rows, num_frames, P):
    """cost_matrix(float32) is, bit for bit, -median_filter(standardised).mean(0) as wo.token_timestamps builds it:
    at a full crop, at odd crops, and at crops of <= 3 frames (num_frames 6 and 2), which are not filtered."""
    rng = np.random.default_rng(rows * 100 + num_frames)
    w = _peaked(rng, heads, P + rows, 1500)
    seen, ts = _oracle_matrix(monkeypatch, w, P, num_frames)
    nf = min(1500, num_frames // 2)
    mine = ar.cost_matrix(w[:, P:, :nf], 7, np.float32)
    assert mine.dtype == np.float32 and mine.shape == (rows, nf)
    np.testing.assert_array_equal(seen, mine.astype(np.float64))
    np.testing.assert_array_equal(ar.times_from_cost(mine), ts[P:])
    if nf <= 3:  # not filtered: the plain head mean of the standardised weights
        with np.errstate(invalid="ignore", divide="ignore"):
            c = w[:, P:, :nf]
            z = ((c - c.mean(-2, keepdims=True)) / c.std(-2, keepdims=True)).astype(np.float32)
        np.testing.assert_array_equal(mine, -z.mean(0))


def test_cost_reference_constant_column_is_nan_sorted_last(monkeypatch):
    """A (head, frame) column whose values are identical over the tokens has zero deviation: its standardised values
    are NaN, the median's sort puts them last (a window holds at most 4 of 7 before its middle turns NaN), and the
    head mean carries the NaN. The reference reproduces the oracle's matrix there, in both precisions' pattern."""
    rng = np.random.default_rng(3)
    w = _peaked(rng, 3, 6, 1500)
    w[1, :, 40] = 0.25       # (sums of six 0.25s are exact in f32: mean == value, std == 0)
    w[0, :, 100:104] = 0.125  # four constant columns in a row: a window of seven holds four NaNs around 101.5
    seen, _ = _oracle_matrix(monkeypatch, w, 0, 1000)
    c32 = ar.cost_matrix(w[:, :, :500], 7, np.float32)
    c64 = ar.cost_matrix(w[:, :, :500], 7, np.float64)
    np.testing.assert_array_equal(seen, c32.astype(np.float64))
    nan = np.isnan(c32)
    assert nan.any() and (nan == np.isnan(c64)).all()
    assert not nan[:, 40].any()                      # one NaN in a window of seven: sorted last, the middle is finite
    assert nan[:, 100:104].all() and not nan[:, 99].any() and not nan[:, 104].any()
    assert np.abs(c32[~nan] - c64[~nan]).max() < 1e-4


def test_f32_and_f64_costs_give_the_same_times():
    """The jump times do not depend on the cost's precision on peaked inputs (the GPU test's 90 % rule caps how much
    a test may hide, it is not a measured spread), and twamd.alignment.times_from_cost (tw_dtw) equals the oracle."""
    rng = np.random.default_rng(11)
    for rows, nf in [(2, 613), (7, 1500), (40, 1000), (1, 300)]:
        w = _peaked(rng, 4, rows, nf)
        c32, c64 = ar.cost_matrix(w, 7, np.float32), ar.cost_matrix(w, 7, np.float64)
        if rows > 1:
            np.testing.assert_array_equal(ar.times_from_cost(c32), ar.times_from_cost(c64))
        np.testing.assert_array_equal(alignment.times_from_cost(c32), ar.times_from_cost(c32))
        np.testing.assert_array_equal(alignment.token_timestamps(w, 0, None), wo.token_timestamps(w, 0, None))


# ---------------------------------------------------------------- TurboTranscriber.align over a stub engine
class StubEngine:
    """What align touches of WhisperEngine. The prompt helpers are the engine's own; logmel / encode / force_pass
    record their calls, and force_pass answers with times and log-probabilities that are functions of the row."""
    prompt_tail = WhisperEngine.prompt_tail
    _prompt_len = WhisperEngine._prompt_len
    max_new_for = WhisperEngine.max_new_for

    def __init__(self, max_batch=2):
        self.gen = GenerationSettings.default(D)
        self.d = D
        self.max_batch = max_batch
        self.device = torch.device("cpu")
        self.wave = torch.zeros(max_batch, 480000)
        self.calls = []

    def logmel(self, n):
        self.calls.append(("logmel", n))

    def encode(self, n, row_map=True, seek=True):
        self.calls.append(("encode", n, row_map, seek))

    def force_pass(self, R, tail, lang_ids, forced, num_frames=None):
        st = self.gen.special
        P = self._prompt_len(tail)
        self.calls.append(("force_pass", R, list(tail), lang_ids, [list(f) for f in forced], list(num_frames),
                           [int((self.wave[r] != 0).sum()) for r in range(R)]))
        ts = [np.concatenate([np.zeros(P, np.float32), 0.5 * (1 + np.arange(len(f) + 1, dtype=np.float32))])
              for f in forced]
        lp = [[-0.1 * (k + 1) for k in range(len(f))] + [-5.0] for f in forced]
        return PassResult([list(f) + [st.eot] for f in forced], [st.lang_begin] * R, token_ts=ts, token_lp=lp)


@pytest.fixture()
def tr():
    eng = StubEngine()
    return TurboTranscriber(eng, WhisperVocab.synthetic(eng.gen.special))


WAV = (0.1 * np.sin(np.arange(70 * SR) * 0.01) + 0.01).astype(np.float32)  # 70 s, no zero sample


def test_align_exists():
    assert callable(getattr(TurboTranscriber, "align", None))
    assert callable(getattr(WhisperEngine, "force_pass", None))


@pytest.mark.parametrize("chunk,what", [
    ({"timestamp": (1.0, 31.5), "tokens": [400, 401]}, "longer than one 30 s window"),
    ({"timestamp": (5.0, 5.0), "tokens": [400]}, "timestamp"),
    ({"timestamp": (6.0, 5.0), "tokens": [400]}, "timestamp"),
    ({"timestamp": (-1.0, 5.0), "tokens": [400]}, "timestamp"),
    ({"timestamp": (60.0, 71.0), "tokens": [400]}, "timestamp"),
    ({"timestamp": (0.0, 5.0), "tokens": [400, GenerationSettings.default(D).special.eot]}, "text tokens"),
    ({"timestamp": (0.0, 5.0), "tokens": [400, GenerationSettings.default(D).special.timestamp_begin + 3]},
     "text tokens"),
    ({"timestamp": (0.0, 5.0), "tokens": [400, -1]}, "text tokens"),
    ({"timestamp": (0.0, 5.0), "tokens": [400] * 445}, "exceed"),
])
def test_align_checks_its_arguments_before_the_engine(tr, chunk, what):
    """Every check raises a ValueError that names the chunk before the engine is touched — also when an earlier chunk
    of the call is fine."""
    good = {"timestamp": (0.0, 2.0), "tokens": [400, 401]}
    with pytest.raises(ValueError, match="chunk 1") as e:
        tr.align(WAV, [good, chunk])
    assert what in str(e.value)
    assert tr.engine.calls == []


def test_align_longest_token_list_that_fits(tr):
    """prompt [SOT, lang, <|notimestamps|>] leaves 445 of 448 positions: 444 text tokens + EOT fit, 445 do not."""
    eng = tr.engine
    assert eng.max_new_for(eng._prompt_len(eng.prompt_tail(None, False))) == 445
    out = tr.align(WAV, [{"timestamp": (0.0, 5.0), "tokens": [400] * 444}])
    assert len(eng.calls[-1][4][0]) == 444 and out["chunk_avg_logprob"][0] is not None


def test_align_refuses_language_on_english_only_and_sharded_runs(tr, monkeypatch):
    from twamd import dist

    monkeypatch.setattr(dist, "collective_path", lambda: True)
    with pytest.raises(RuntimeError, match="not sharded"):
        tr.align(WAV, [{"timestamp": (0.0, 2.0), "tokens": [400]}])
    monkeypatch.setattr(dist, "collective_path", lambda: False)
    en = GenerationSettings.default(PRESETS["tiny.en"])
    assert not en.special.is_multilingual
    tr.engine.gen = tr.gen = en
    for kw in ({"language": "english"}, {"task": "transcribe"}):
        with pytest.raises(ValueError, match="English-only"):
            tr.align(WAV, [{"timestamp": (0.0, 2.0), "tokens": [400]}], **kw)
    assert tr.engine.calls == []


def test_align_assembles_words_from_the_pass_result(tr):
    """Windows, batches and the result: a chunk without tokens is not run (and yields None), the others become one
    window each (their samples, zero padded; num_frames = ceil(samples / 160)) in batches of max_batch; token k of a
    chunk spans (time of token k - 1, time of token k) shifted by the chunk's t0, as AsrStitcher's word path pairs
    them; chunk_avg_logprob is the mean over the text tokens (the EOT's -5.0 stays out)."""
    eng, st = tr.engine, tr.engine.gen.special
    vocab = tr.vocab
    # three words' worth of text ids from the synthetic vocabulary: tokens that begin with a space start a word
    ids = [i for i in range(300, 2000) if vocab.decode([i]).startswith(" ") and vocab.decode([i]).strip().isalnum()]
    a, b, c = ids[:3], ids[3:5], ids[5:9]
    chunks = [{"timestamp": (10.0, 12.5), "tokens": a}, {"timestamp": (20.0, 21.0), "tokens": []},
              {"timestamp": (30.0, 60.0), "tokens": b}, {"timestamp": (65.0, None), "tokens": c}]
    out = tr.align(WAV, chunks, return_language=True)
    runs = [x for x in eng.calls if x[0] == "force_pass"]
    assert [x[0] for x in eng.calls] == ["logmel", "encode", "force_pass"] * 2
    assert [x[1] for x in runs] == [2, 1]                                  # max_batch 2: chunks (0, 2), then (3)
    assert all(x[1:] == (n, False, False) for x, n in zip([y for y in eng.calls if y[0] == "encode"], (2, 1)))
    assert runs[0][2] == [st.notimestamps] and runs[0][3] is None           # the <|notimestamps|> tail, language detected
    assert runs[0][4] == [a, b] and runs[1][4] == [c]
    assert runs[0][5] == [250, 3000] and runs[1][5] == [500]                # ceil(samples / 160)
    assert runs[0][6] == [40000, 480000] and runs[1][6] == [80000]          # the chunk's samples, then zeros
    assert out["text"] == "".join(vocab.decode(x) for x in (a, b, c))
    assert "".join(w["text"] for w in out["chunks"]) == out["text"]
    assert len(out["chunks"]) == 9 and all(w["language"] == "english" for w in out["chunks"])
    t0s = [10.0] * 3 + [30.0] * 2 + [65.0] * 4
    ks = [0, 1, 2, 0, 1, 0, 1, 2, 3]
    for w, t0, k in zip(out["chunks"], t0s, ks):
        assert w["timestamp"] == (round(t0 + 0.5 * k, 2), round(t0 + 0.5 * (k + 1), 2))   # the stub's times
        assert math.isclose(w["probability"], math.exp(-0.1 * (k + 1)), rel_tol=1e-12)
    want = [np.mean([-0.1 * (k + 1) for k in range(n)]) for n in (3, 2, 4)]
    got = out["chunk_avg_logprob"]
    assert got[1] is None and np.allclose([got[0], got[2], got[3]], want, rtol=0, atol=1e-12)
    eng.calls.clear()
    tr.align(WAV, chunks, batch_size=1, language="english", task="transcribe")
    runs = [x for x in eng.calls if x[0] == "force_pass"]
    assert [x[1] for x in runs] == [1, 1, 1]
    assert runs[0][2] == [st.transcribe, st.notimestamps] and runs[0][3] == [st.lang_to_id()["<|en|>"]]


# ---------------------------------------------------------------- the C-ABI
def test_header_declares_and_library_exports_the_new_entries():
    hdr = open(os.path.join(ROOT, "include", "tw_whisper.h")).read()
    for name in ("tw_logits_force", "tw_align_cost"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTED and name in _lib._SIGS
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert "align.hip" in open(os.path.join(ROOT, "turbo-whisper-workspace_amd", "csrc", "Makefile")).read()
