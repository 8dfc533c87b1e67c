"""repetition_penalty / no_repeat_ngram_size without a GPU: the numpy restatement (tests/history_ref.py) equals
transformers' own processors bit for bit, the callable validates the kwargs as transformers does, and the new kernel's
symbol, ctypes signature and torch op are there."""
import ctypes

import numpy as np
import pytest
import torch

import history_ref as hr
from twamd import _lib, _ops
from twamd.config import PRESETS
from twamd.pipeline import TurboTranscriber

V = PRESETS["test-mini"].vocab
NGRAMS = (0, 1, 2, 3, 5)
PENALTIES = (1.0, 1.3, 0.7)


def kernel_cases(n: int, seed: int = 3):
    """The rows of the kernel tests for n-gram size n: (prefix, generated, finished) per row. Ids come from an
    8-id alphabet with 0 and V - 1 in it (dense repeats and n-gram matches); history lengths 0, 1, n - 1, n, 40 and
    447; the length-40 row is a run of one id and the 447 row repeats a period-7 pattern whose n-grams span the
    prefix / generated boundary. No row is finished (the GPU test sets that itself)."""
    rng = np.random.default_rng(seed + n)
    alpha = np.array([0, V - 1, 7, 1234, 50257, 50364, 50365, 31], np.int64)
    lens = [0, 1, max(n - 1, 0), n, 40, 447]
    rows = []
    for r, L in enumerate(lens):
        if L == 40:
            h = [int(alpha[3])] * L
        elif L == 447:
            h = [int(alpha[i % 7]) for i in range(L)]
        else:
            h = [int(t) for t in rng.choice(alpha, L)]
        cut = min(L, 3) if r != 5 else 5  # (row 5: prefix 5 ids, so a 5-gram covers the boundary)
        rows.append((h[:cut], h[cut:], False))
    return rows


def kernel_logits(R: int, ld: int, seed: int = 11) -> np.ndarray:
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((R, ld)) * 8).astype(np.float32)
    x[::2, 0] = -np.inf  # some logits are already -inf, ids of the histories' alphabet among them
    x[1:, 50364] = -np.inf
    x[:, 100:110] = -np.inf
    x[:, 7] = np.float32(2.5)
    x[:, 31] = np.float32(-0.0)
    return x


def test_restatement_equals_transformers_processors():
    pytest.importorskip("transformers")
    from transformers.generation.logits_process import NoRepeatNGramLogitsProcessor, RepetitionPenaltyLogitsProcessor

    for n in NGRAMS:
        rows = kernel_cases(n)
        x = kernel_logits(len(rows), V)
        for p in PENALTIES:
            for r, (pre, gen, _) in enumerate(rows):
                h = pre + gen
                s = torch.from_numpy(x[r: r + 1].copy())
                ids = torch.tensor([h], dtype=torch.long)
                if p != 1.0 and h:
                    s = RepetitionPenaltyLogitsProcessor(penalty=p)(ids, s)
                if n > 0:
                    s = NoRepeatNGramLogitsProcessor(n)(ids, s)
                ref = hr.history_processors(x[r], h, p, n)
                assert ref.dtype == np.float32
                assert np.array_equal(s[0].numpy().view(np.int32), ref.view(np.int32)), (n, p, r)


def test_restatement_properties():
    x = np.array([2.0, -2.0, 0.5, -np.inf, 1.0], np.float32)
    s = hr.repetition_penalty(x, [0, 0, 1, 3], 1.3)
    assert s[0] == np.float32(2.0) / np.float32(1.3) and s[1] == np.float32(-2.0) * np.float32(1.3)  # once, by sign
    assert s[3] == -np.inf and s[2] == x[2] and s[4] == x[4]
    assert hr.banned_ngram_tokens([1, 2, 3, 1, 2], 3) == [3]
    assert hr.banned_ngram_tokens([1, 2], 3) == [] and hr.banned_ngram_tokens([4, 2, 4], 1) == [2, 4]
    both = hr.history_processors(x, [0, 4, 0], 1.3, 2)  # the ban wins over the penalised value
    assert both[4] == -np.inf and both[0] == s[0]


def test_callable_validates_like_transformers():
    pop = TurboTranscriber._history_options
    assert pop({"repetition_penalty": None, "no_repeat_ngram_size": 0, "length_penalty": 1.0}) == {}
    assert pop({"repetition_penalty": 1.0, "no_repeat_ngram_size": None}) == {}
    gk = {"repetition_penalty": 1.3, "no_repeat_ngram_size": 3, "length_penalty": 0.5, "top_p": 0.9}
    assert pop(gk) == {"repetition_penalty": 1.3, "no_repeat_ngram_size": 3, "length_penalty": 0.5}
    assert gk == {"top_p": 0.9}  # (what is left still raises in the call)
    for bad in (0.0, -1.3, 2, "1.3"):
        with pytest.raises(ValueError, match="`penalty` has to be a strictly positive float"):
            pop({"repetition_penalty": bad})
    assert pop({"no_repeat_ngram_size": 0.0}) == {}  # (falsy: off, as generate() reads it)
    assert pop({"no_repeat_ngram_size": True}) == {"no_repeat_ngram_size": 1}  # (an int to transformers too)
    for bad in (-1, 2.0, "2"):
        with pytest.raises(ValueError, match="`ngram_size` has to be a strictly positive integer"):
            pop({"no_repeat_ngram_size": bad})


def test_validation_text_is_transformers_own():
    pytest.importorskip("transformers")
    from transformers.generation.logits_process import NoRepeatNGramLogitsProcessor, RepetitionPenaltyLogitsProcessor

    for cls, key, bad in ((RepetitionPenaltyLogitsProcessor, "repetition_penalty", -2.0),
                          (NoRepeatNGramLogitsProcessor, "no_repeat_ngram_size", -2)):
        with pytest.raises(ValueError) as theirs:
            cls(bad)
        with pytest.raises(ValueError) as ours:
            TurboTranscriber._history_options({key: bad})
        assert str(ours.value) == str(theirs.value)


def test_symbol_signatures_and_struct_layout():
    lib = _lib.load()
    assert "tw_logits_history" in _lib.EXPORTED
    fn = lib.tw_logits_history
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 14
    assert fn.argtypes[10] is ctypes.c_float  # repetition_penalty
    # the beam flag is appended: the four fields the parent fills keep their offsets and the new one defaults to 0
    bp = _lib.TwBeamParams(5, 24, 1.0, 448)
    assert bp.scores_are_logprobs == 0 and ctypes.sizeof(bp) == 20
    assert _lib.TwBeamParams.scores_are_logprobs.offset == 16 and _lib.TwBeamParams.ld_tokens.offset == 12
    # bad arguments are refused on the host, before any launch
    assert fn(None, 1, 8, 8, None, 0, None, None, 0, None, 1.3, 2, 0, None) != 0
    tw = _ops.load()
    assert "logits_history_" in _ops.OPS
    schema = str(tw.logits_history_.default._schema)
    assert "Tensor(a!) logits" in schema and "float repetition_penalty" in schema and "bool to_logprobs" in schema
    meta = torch.device("meta")
    x = torch.empty(2, 16, device=meta)
    i = torch.empty(2, 8, dtype=torch.int32, device=meta)
    assert tw.logits_history_(x, 16, None, None, i, i, 1.3, 2, False) is None
